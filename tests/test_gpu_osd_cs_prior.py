"""OSD-CS with the prior-weighted cost on the device (osd_block_cs_prior_kernel)
against the host C++ and the dense NumPy model on the same inputs, through
every block-kernel instance the bundled codes select, and through
simulate_dem and simulate_p."""
import ctypes

import numpy as np
import pytest

import dem_model as dm
import osd_cs_cases as cases
import osd_cs_prior_cases as pc

pytestmark = pytest.mark.gpu

ROWS = ("two_level", "negative", "wide", "uniform")


def _kernel_name(H, cs):
    from qldpcsim_amd import _lib
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.lib.qldpc_osd_kernel_name(_lib.code_for(H, 0).handle, int(cs), buf, 128))
    return buf.value.decode()


def _gpu_cs_prior(H, syn, perms, e0, lam, q, eps, handle=None):
    import torch
    from qldpcsim_amd import _lib
    code = _lib.code_for(H, 0)
    pd = torch.as_tensor(np.array(perms, np.int32), device="cuda")
    sd = torch.as_tensor(np.array(syn, np.uint8), device="cuda")
    ed = torch.as_tensor(np.array(e0, np.uint8), device="cuda")
    st = torch.full((len(e0),), -7, dtype=torch.int32, device="cuda")
    h = code.prior(q, eps).handle if handle is None else handle[0]
    _lib.check(_lib.lib.qldpc_osd_device_cs_prior(code.handle, len(e0), sd.data_ptr(), pd.data_ptr(), int(lam), h,
                                                  ed.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    return ed.cpu().numpy(), st.cpu().numpy()


# one code per NW instance, and the word edge at n = 127 / 128
INSTANCES = [("steane:x", 24, (0, 10, 64), "osd_block_cs_prior_kernel<4, 4, 1>"),
             ("LP04_0:x", 64, (10,), "osd_block_cs_prior_kernel<4, 4, 1>"),
             ("gen127", 16, (10,), "osd_block_cs_prior_kernel<4, 4, 1>"),
             ("gen128", 16, (10,), "osd_block_cs_prior_kernel<4, 4, 1>"),
             ("LP118_0:x", 16, (0, 10, 64), "osd_block_cs_prior_kernel<9, 4, 1>"),
             ("LP118_2:x", 16, (0, 10, 64), "osd_block_cs_prior_kernel<17, 8, 2>"),
             # |T| = 3 and |T| = 0: lambda clipped, no pair
             ("t3", 24, (10,), "osd_block_cs_prior_kernel<4, 4, 1>"),
             ("fullrank", 12, (10,), "osd_block_cs_prior_kernel<4, 4, 1>")]


@pytest.mark.parametrize("name,k,lams,kernel", INSTANCES, ids=[c[0] for c in INSTANCES])
def test_device_equals_host_and_model(name, k, lams, kernel):
    H, syn, _, e0, perms = cases.shots(name, k)
    assert _kernel_name(H, 2) == kernel
    assert _kernel_name(H, 1) == kernel.replace("_prior", "")       # the other two kinds are what they were
    assert _kernel_name(H, 0) == kernel.replace("_cs_prior", "")
    for row in ROWS:
        q, eps = pc.prior_row(name, row)
        for lam in lams:
            got, st = _gpu_cs_prior(H, syn, perms, e0, lam, q, eps)
            assert np.all(st == 0)
            msg = f"{row}, lambda {lam}"
            np.testing.assert_array_equal(got, pc.host_cs_prior(H, syn, perms, e0, lam, q, eps), err_msg=msg)
            np.testing.assert_array_equal(got, pc.model(name, k, lam, row)[0], err_msg=msg)
            if row == "uniform":
                np.testing.assert_array_equal(got, cases.model(name, k, lam)[0], err_msg=msg)


def test_index_error_case_is_status_1():
    H = np.array([[1, 1, 1, 1], [1, 1, 1, 1]], np.uint8)
    e0 = np.zeros((1, 4), np.uint8)
    got, st = _gpu_cs_prior(H, np.array([[1, 1]], np.uint8), np.array([[0, 1, 2, 3]], np.int32), e0, 10,
                            np.array([0.1, 0.2, 0.3, 0.01]), 1e-9)
    assert st[0] == 1
    np.testing.assert_array_equal(got, e0)


def test_refusals_before_any_launch():
    from qldpcsim_amd import _lib
    H, syn, _, e0, perms = cases.shots("gen127", 16)
    q, eps = pc.prior_row("gen127", "negative")
    Hz = H.copy()
    Hz[:, 9] = 0                                        # an all-zero column: the column kernel's case
    with pytest.raises(NotImplementedError, match="all-zero"):
        _gpu_cs_prior(Hz, syn, perms, e0, 10, q, eps)
    with _lib.options(osd_hbm=1):
        with pytest.raises(NotImplementedError, match="osd_hbm"):
            _gpu_cs_prior(H, syn, perms, e0, 10, q, eps)
    for lam in (-1, 65):
        with pytest.raises(ValueError):
            _gpu_cs_prior(H, syn, perms, e0, lam, q, eps)
    with pytest.raises(ValueError, match="null"):
        _gpu_cs_prior(H, syn, perms, e0, 10, q, eps, handle=(None,))
    other = _lib.code_for(cases.matrix("gen128"), 0).prior(pc.prior_row("gen128", "negative")[0], eps)
    with pytest.raises(ValueError, match="another code"):
        _gpu_cs_prior(H, syn, perms, e0, 10, q, eps, handle=(other.handle,))
    big = np.zeros((2, 1100), np.uint8)                 # past the block kernel's 1087 columns
    big[0, :] = 1
    big[1, ::2] = 1
    with pytest.raises(NotImplementedError, match="1087"):
        _gpu_cs_prior(big, np.zeros((1, 2), np.uint8), np.arange(1100, dtype=np.int32)[None],
                      np.zeros((1, 1100), np.uint8), 2, np.full(1100, 0.01), eps)


def _decode_result(post, e0):
    """A device decode's result with every shot unconverged."""
    import torch
    from qldpcsim_amd import decoders
    k = len(e0)
    return decoders.DecodeResult(torch.as_tensor(np.array(e0), device="cuda"),
                                 torch.zeros(k, dtype=torch.int32, device="cuda"),
                                 torch.as_tensor(np.array(post), device="cuda"),
                                 torch.zeros(k, dtype=torch.int32, device="cuda"))


def test_nan_row_is_spilled_and_finished_with_the_host_order_and_the_weighted_cost():
    import torch
    from qldpcsim_amd import _lib, decoders
    name, k, lam, bad = "LP04_0:x", 64, 10, 5
    H, syn, post, e0, _ = cases.shots(name, k)
    q, eps = pc.prior_row(name, "negative")
    n = H.shape[1]
    post = np.array(post)
    post[bad, 17] = np.nan
    perms = np.ascontiguousarray(decoders.osd_perms(post), np.int32)   # NumPy's own order of the NaN row
    want = pc.host_cs_prior(H, syn, perms, e0, lam, q, eps)
    assert np.any(want != cases.host_cs(H, syn, perms, e0, lam))       # the cost matters on these shots
    code = _lib.code_for(H, 0)
    res = _decode_result(post, e0)
    sd = torch.as_tensor(np.array(syn), device="cuda")
    st = torch.empty(k, dtype=torch.int32, device="cuda")
    perm_d = torch.empty((k, n), dtype=torch.int32, device="cuda")
    tie = torch.empty(k, dtype=torch.int32, device="cuda")
    sp_post = torch.zeros((4, n), dtype=torch.float64, device="cuda")
    sp_idx = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    sp_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.qldpc_osd_device_ordered_ex_cs_prior(
        code.handle, k, sd.data_ptr(), res.post.data_ptr(), lam, code.prior(q, eps).handle, res.ehat.data_ptr(),
        st.data_ptr(), perm_d.data_ptr(), tie.data_ptr(), sp_post.data_ptr(), sp_idx.data_ptr(), sp_cnt.data_ptr(), 4,
        None))
    torch.cuda.synchronize()
    status = st.cpu().numpy()
    assert status[bad] == 2 and np.all(np.delete(status, bad) == 0)
    assert int(sp_cnt[0]) == 1 and int(sp_idx[0]) == bad
    got = res.ehat.cpu().numpy()
    np.testing.assert_array_equal(got[bad], e0[bad])
    np.testing.assert_array_equal(np.delete(got, bad, 0), np.delete(want, bad, 0))
    # the form without spill buffers gives the same
    res = _decode_result(post, e0)
    _lib.check(_lib.lib.qldpc_osd_device_ordered_cs_prior(
        code.handle, k, sd.data_ptr(), res.post.data_ptr(), lam, code.prior(q, eps).handle, res.ehat.data_ptr(),
        st.data_ptr(), perm_d.data_ptr(), tie.data_ptr(), None))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(res.ehat.cpu().numpy(), got)
    # the staged form finishes the NaN shot through the host order, with the weighted cost
    res = _decode_result(post, e0)
    decoders.apply_osd_device(H, sd, res, lam, method="cs", cost="prior", prior=q, eps=eps)
    assert res.osd_host_order == (1 if decoders.numpy_order_pinned() else k)
    np.testing.assert_array_equal(res.ehat.cpu().numpy(), want)


def test_apply_osd_device_on_an_explicit_stream():
    import torch
    from qldpcsim_amd import decoders
    name, k, lam = "LP118_0:x", 16, 10
    H, syn, post, e0, _ = cases.shots(name, k)
    q, eps = pc.prior_row(name, "wide")
    stream = torch.cuda.Stream()
    res = _decode_result(post, e0)
    sd = torch.as_tensor(np.array(syn), device="cuda")
    torch.cuda.synchronize()
    decoders.apply_osd_device(H, sd, res, lam, stream=stream.cuda_stream, method="cs", cost="prior", prior=q, eps=eps)
    stream.synchronize()
    np.testing.assert_array_equal(res.ehat.cpu().numpy(), pc.model(name, k, lam, "wide")[0])
    # without the keyword the call is the Hamming one
    ref = _decode_result(post, e0)
    decoders.apply_osd_device(H, sd, ref, lam, stream=stream.cuda_stream, method="cs")
    stream.synchronize()
    np.testing.assert_array_equal(ref.ehat.cpu().numpy(), cases.model(name, k, lam)[0])
    with pytest.raises(ValueError):
        decoders.apply_osd_device(H, sd, _decode_result(post, e0), lam, method="cs", cost="prior")
    with pytest.raises(ValueError):
        decoders.apply_osd_device(H, sd, _decode_result(post, e0), 0, cost="prior", prior=q)


def test_host_decode_batch_prices_osd_with_its_own_row():
    """Host decode_batch (staged through the device) with prior= and
    osd_cost="prior": the OSD step equals apply_osd on its posteriors; the
    single-shot wrapper with an array for p does the same."""
    from qldpcsim_amd import decoders
    name, k, lam = "LP04_0:x", 64, 10
    H, syn, _, _, _ = cases.shots(name, k)
    q, _ = pc.prior_row(name, "random")
    plain = decoders.decode_batch(H, np.array(syn), None, 3, prior=q, want_post=True)
    assert not plain.converged.all()
    want = decoders.apply_osd(H, np.array(syn), plain.ehat.copy(), plain.post, plain.flags, lam, method="cs",
                              cost="prior", prior=q)
    got = decoders.decode_batch(H, np.array(syn), None, 3, prior=q, osd_order=lam, osd_method="cs", osd_cost="prior")
    np.testing.assert_array_equal(got.ehat, want)
    i = int(np.flatnonzero(~plain.converged)[0])
    one, _ = decoders.MS_decoder(H, syn[i], q, 3, OSDorder=lam, osd_method="cs", osd_cost="prior")
    np.testing.assert_array_equal(one, want[i])


def _dem():
    """dem_model's 65 x 129 word-edge model; its two columns without a detector
    get one each (the device OSD-CS takes no all-zero column). It keeps the
    p = 0 column, the p = 1 - 2^-20 one (a negative weight), the twin columns
    and the heavy detector row."""
    from qldpcsim_amd import dem as D
    H, L, pr, where = dm.edge_dem(65, 65, 129)
    H = H.copy()
    for j in np.flatnonzero(~H.any(axis=0)):
        H[1 + j % 60, j] = 1
    return D.Dem(H, L, pr)


def test_simulate_dem_device_and_host_osd_give_equal_counters():
    """330 shots of the model, BP with 3 iterations, OSD-CS with lambda = 10
    and the prior cost: simulate_dem's device OSD in batches of 100 and of 77
    against the same device-drawn shots decoded here and finished with the
    host OSD (decoders.apply_osd)."""
    import torch
    from qldpcsim_amd import decoders, simulator
    model = _dem()
    shots, seed, iters, lam = 330, 13, 3, 10
    src = simulator.DeviceDem(model, torch.device("cuda", 0), simulator._device_key([seed, 0]))
    det, obs = src.sample(shots)
    r = decoders.decode_batch(model.H, det, None, iters, algo="BP", want_post=True, prior=model.priors)
    torch.cuda.synchronize()
    flags = r.flags.cpu().numpy()
    assert 0 < int(((flags & 1) == 0).sum())            # OSD has shots to work on
    det_h = det.cpu().numpy()
    ehat = decoders.apply_osd(model.H, det_h, r.ehat.cpu().numpy(), r.post.cpu().numpy(), flags, lam, method="cs",
                              cost="prior", prior=model.priors)
    obs_h = decoders.unpack_bits(obs, model.num_observables).cpu().numpy()
    c = dm.counters(dm.classify(model.H, model.L, det_h, obs_h, ehat)[0], r.iters.cpu().numpy())
    want = [c["failures"], c["logical_errors"], c["successes"], c["iterations"]]
    kw = dict(shots=shots, decType="BP", decIterations=iters, OSDorder=lam, osd_method="cs", osd_cost="prior",
              rngSeed=seed, sampler="device", verbose=False)
    for batch in (100, 77):
        got = simulator.simulate_dem(model, batch_size=batch, **kw)
        assert [got[k] for k in simulator.DEM_KEYS] == want, batch


def test_simulate_p_pipelined_inline_and_host_give_equal_counters():
    """LP04_0 with a channel_weights array (every fourth qubit four times as
    noisy), MS with 3 iterations at p = 0.05, 330 shots, OSD-CS with lambda =
    10 and the prior cost, each half priced with its own marginals: the
    pipelined device path in batches of 100 and of 77, the same shots decoded
    here with the inline device OSD (apply_osd_device), and the host path."""
    import torch
    from qldpcsim_amd import codes, decoders, simulator
    from qldpcsim_amd.schedule import pack_layers
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    p, shots, seed, iters, lam = 0.05, 330, 13, 3, 10
    w = np.ones((3, n))
    w[:, ::4] = 4.0
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), simulator._device_key([seed, 0]))
    ch.set_probs(simulator.channel_probs(p, w, n))
    sy_z, sy_x, ewX, ewZ = ch.sample(p, shots)
    errX, errZ = ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy()
    layersX, layersZ = simulator.select_layers(Hx, Hz, "F")
    est, its, osd_shots = [], [], 0
    for H, syn, layers, row in ((Hz, sy_z, layersX, p * (w[0] + w[1])), (Hx, sy_x, layersZ, p * (w[2] + w[1]))):
        lp, lr = pack_layers(layers, H.shape[0])
        r = decoders.decode_batch(H, syn, None, iters, algo="MS", want_post=True, layer_ptr=lp, layer_rows=lr,
                                  prior=row)
        osd_shots += int((~r.converged).sum())
        decoders.apply_osd_device(H, syn, r, lam, method="cs", cost="prior", prior=row)
        est.append(r.ehat.cpu().numpy())
        its.append(r.iters.cpu().numpy())
    assert osd_shots > 20
    c = simulator.count_outcomes(Hx, Hz, sy_z.cpu().numpy(), sy_x.cpu().numpy(), errX, errZ, est[0], est[1], its[0],
                                 its[1])
    want = {"DecFailures_X": c["DecFailures_X"], "DecFailures_Z": c["DecFailures_Z"],
            "decSuccessExact": c["decSuccessExact"], "decSuccessDegen": c["decSuccessDegen"],
            "Avg_number_of_iterations_X": c["nIterAccX"] / float(shots),
            "Avg_number_of_iterations_Z": c["nIterAccZ"] / float(shots)}
    kw = dict(shots=shots, decType="MS", decIterations=iters, decSchedule="F", rngSeed=seed, verbose=False,
              OSDorder=lam, osd_method="cs", osd_cost="prior", channel_weights=w)
    for batch in (100, 77):
        got = simulator.simulate_p(Hx, Hz, p, batch_size=batch, sampler="device", **kw)
        assert got == want, batch
    host = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="host",
                                samples=(sy_z.cpu().numpy(), sy_x.cpu().numpy(), errX, errZ), **kw)
    assert host == want


def test_phenomenological_x_half_equals_simulate_dem_and_windows_do_not_depend_on_batching():
    """LP04_0, 3 rounds, p_data = 0.02 != q = 0.01 (every matrix decodes with a
    prior row), MS with 4 iterations, OSD-CS lambda = 10 with the prior cost:
    the X-half detector error model has simulate_phenomenological's matrix, row
    and Philox key, so its counters equal the _X ones; the sliding-window run
    prices every window's OSD with that window's row and gives the same
    counters whatever the batch size."""
    from qldpcsim_amd import codes, dem as D, logicals, simulator
    Hx, Hz = codes.load_code("LP04_0")
    p, q, T, shots = 0.03, 0.01, 3, 1024
    model = D.phenomenological_dem(Hz, logicals.css_logicals(Hx, Hz)[1], T, 2 * p / 3, q)
    common = dict(shots=shots, rngSeed=11, sampler="device", verbose=False, decType="MS", decIterations=4,
                  OSDorder=10, osd_method="cs", osd_cost="prior")
    want = simulator.simulate_phenomenological(Hx, Hz, p, q, T, **common)
    got = simulator.simulate_dem(model, **common)
    assert (got["DecFailures"], got["logicalErrors"], got["nIterAcc"]) == \
        (want["DecFailures_X"], want["logicalErrors_X"], want["nIterAccX"])
    assert got["DecFailures"] == 0                           # OSD reproduces every detector
    a = simulator.simulate_phenomenological(Hx, Hz, p, q, T, window=2, **common)
    b = simulator.simulate_phenomenological(Hx, Hz, p, q, T, window=2, batch_size=300, **common)
    assert a == b and a["windows"] == 2


def test_results_file_records_the_cost_only_when_it_is_prior(tmp_path):
    import json
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    np.save(tmp_path / "hx.npy", Hx)
    np.save(tmp_path / "hz.npy", Hz)
    w = np.ones((3, n))
    w[:, ::4] = 4.0
    kw = dict(HxFile=str(tmp_path / "hx.npy"), HzFile=str(tmp_path / "hz.npy"), p=[0.05], shots=200, decType="MS",
              decIterations=3, OSDorder=10, osd_method="cs", rngSeed=3, verbose=False, channel_weights=w,
              return_results=True)
    r1 = simulator.simulate(resultsFile=str(tmp_path / "prior.json"), osd_cost="prior", **kw)
    r0 = simulator.simulate(resultsFile=str(tmp_path / "hamming.json"), **kw)
    assert json.load(open(tmp_path / "prior.json"))["meta"]["osd_cost"] == "prior"
    assert "osd_cost" not in json.load(open(tmp_path / "hamming.json"))["meta"]
    assert r0 == simulator.simulate(osd_cost="hamming", **kw)
    assert r1[0].keys() == r0[0].keys()
    with pytest.raises(ValueError):                          # a bias gives each half one scalar prior
        simulator.simulate(**dict(kw, channel_weights=None, bias=10.0), osd_cost="prior")

"""OSD-CS on the device (osd_block_kernel's combination-sweep epilogue) against
the host C++ and the dense NumPy model on the same inputs, through every
block-kernel instance the bundled codes select, and through simulate_p."""
import ctypes

import numpy as np
import pytest

import osd_cs_cases as cases
import osd_cs_model

pytestmark = pytest.mark.gpu


def _kernel_name(H, cs):
    from qldpcsim_amd import _lib
    buf = ctypes.create_string_buffer(128)
    _lib.check(_lib.lib.qldpc_osd_kernel_name(_lib.code_for(H, 0).handle, int(cs), buf, 128))
    return buf.value.decode()


def _gpu_cs(H, syn, perms, e0, lam):
    import torch
    from qldpcsim_amd import _lib
    code = _lib.code_for(H, 0)
    pd = torch.as_tensor(np.array(perms, np.int32), device="cuda")
    sd = torch.as_tensor(np.array(syn, np.uint8), device="cuda")
    ed = torch.as_tensor(np.array(e0, np.uint8), device="cuda")
    st = torch.full((len(e0),), -7, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.qldpc_osd_device_cs(code.handle, len(e0), sd.data_ptr(), pd.data_ptr(), int(lam),
                                            ed.data_ptr(), st.data_ptr(), None))
    torch.cuda.synchronize()
    return ed.cpu().numpy(), st.cpu().numpy()


# one case per block-kernel instance the bundled codes and the 127 / 128-column matrices select
INSTANCES = [("steane:x", 24, "osd_block_cs_kernel<4, 4, 1>"),
             ("LP04_0:x", 64, "osd_block_cs_kernel<4, 4, 1>"),
             ("bicycle:x", 16, "osd_block_cs_kernel<4, 4, 1>"),
             ("gen127", 16, "osd_block_cs_kernel<4, 4, 1>"),
             ("gen128", 16, "osd_block_cs_kernel<4, 4, 1>"),
             ("LP118_0:x", 16, "osd_block_cs_kernel<9, 4, 1>"),
             ("LP118_2:x", 16, "osd_block_cs_kernel<17, 8, 2>"),
             ("t3", 24, "osd_block_cs_kernel<4, 4, 1>"),
             ("fullrank", 12, "osd_block_cs_kernel<4, 4, 1>")]


@pytest.mark.parametrize("name,k,kernel", INSTANCES, ids=[c for c, _, _ in INSTANCES])
def test_device_cs_equals_host_and_model(name, k, kernel):
    H, syn, _, e0, perms = cases.shots(name, k)
    assert _kernel_name(H, True) == kernel
    assert _kernel_name(H, False) == kernel.replace("_cs", "")
    for lam in cases.LAMBDAS:
        got, st = _gpu_cs(H, syn, perms, e0, lam)
        assert np.all(st == 0)
        np.testing.assert_array_equal(got, cases.host_cs(H, syn, perms, e0, lam), err_msg=f"lambda {lam}")
        np.testing.assert_array_equal(got, cases.model(name, k, lam)[0], err_msg=f"lambda {lam}")


def test_index_error_case_is_status_1():
    # rank 1 and a nonzero first column: the greedy loop runs past column n-1
    H = np.array([[1, 1, 1, 1], [1, 1, 1, 1]], np.uint8)
    perms = np.array([[0, 1, 2, 3]], np.int32)
    e0 = np.zeros((1, 4), np.uint8)
    got, st = _gpu_cs(H, np.array([[1, 1]], np.uint8), perms, e0, 10)
    assert st[0] == 1
    np.testing.assert_array_equal(got, e0)


def test_refusals_before_any_launch():
    from qldpcsim_amd import _lib
    H, syn, _, e0, perms = cases.shots("gen127", 16)
    Hz = H.copy()
    Hz[:, 9] = 0                                        # an all-zero column: the column kernel's case
    with pytest.raises(NotImplementedError, match="all-zero"):
        _gpu_cs(Hz, syn, perms, e0, 10)
    with _lib.options(osd_hbm=1):
        with pytest.raises(NotImplementedError, match="osd_hbm"):
            _gpu_cs(H, syn, perms, e0, 10)
    for lam in (-1, 65):
        with pytest.raises(ValueError):
            _gpu_cs(H, syn, perms, e0, lam)
    big = np.zeros((2, 1100), np.uint8)                 # past the block kernel's 1087 columns
    big[0, :] = 1
    big[1, ::2] = 1
    with pytest.raises(NotImplementedError, match="1087"):
        _gpu_cs(big, np.zeros((1, 2), np.uint8), np.arange(1100, dtype=np.int32)[None],
                np.zeros((1, 1100), np.uint8), 2)


def _decode_result(post, e0):
    """A device decode's result with every shot unconverged."""
    import torch
    from qldpcsim_amd import decoders
    k = len(e0)
    return decoders.DecodeResult(torch.as_tensor(np.array(e0), device="cuda"),
                                 torch.zeros(k, dtype=torch.int32, device="cuda"),
                                 torch.as_tensor(np.array(post), device="cuda"),
                                 torch.zeros(k, dtype=torch.int32, device="cuda"))


def test_nan_row_is_spilled_and_finished_with_the_host_order():
    import torch
    from qldpcsim_amd import _lib, decoders
    name, k, lam, bad = "LP04_0:x", 64, 10, 5
    H, syn, post, e0, _ = cases.shots(name, k)
    n = H.shape[1]
    post = np.array(post)
    post[bad, 17] = np.nan
    perms = np.ascontiguousarray(decoders.osd_perms(post), np.int32)   # NumPy's own order of the NaN row
    want = cases.host_cs(H, syn, perms, e0, lam)
    # the entry point: status 2 for that shot, its posteriors and index spilled, e_hat untouched
    code = _lib.code_for(H, 0)
    res = _decode_result(post, e0)
    sd = torch.as_tensor(np.array(syn), device="cuda")
    st = torch.empty(k, dtype=torch.int32, device="cuda")
    perm_d = torch.empty((k, n), dtype=torch.int32, device="cuda")
    tie = torch.empty(k, dtype=torch.int32, device="cuda")
    sp_post = torch.zeros((4, n), dtype=torch.float64, device="cuda")
    sp_idx = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    sp_cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.qldpc_osd_device_ordered_ex_cs(
        code.handle, k, sd.data_ptr(), res.post.data_ptr(), lam, res.ehat.data_ptr(), st.data_ptr(),
        perm_d.data_ptr(), tie.data_ptr(), sp_post.data_ptr(), sp_idx.data_ptr(), sp_cnt.data_ptr(), 4, None))
    torch.cuda.synchronize()
    status = st.cpu().numpy()
    assert status[bad] == 2 and np.all(np.delete(status, bad) == 0)
    assert int(sp_cnt[0]) == 1 and int(sp_idx[0]) == bad
    np.testing.assert_array_equal(sp_post[0].cpu().numpy(), post[bad])
    got = res.ehat.cpu().numpy()
    np.testing.assert_array_equal(got[bad], e0[bad])
    np.testing.assert_array_equal(np.delete(got, bad, 0), np.delete(want, bad, 0))
    # the staged form finishes it through the host order
    res = _decode_result(post, e0)
    decoders.apply_osd_device(H, sd, res, lam, method="cs")
    assert res.osd_host_order == (1 if decoders.numpy_order_pinned() else k)
    np.testing.assert_array_equal(res.ehat.cpu().numpy(), want)


def test_apply_osd_device_on_an_explicit_stream():
    import torch
    from qldpcsim_amd import decoders
    name, k, lam = "LP118_0:x", 16, 10
    H, syn, post, e0, _ = cases.shots(name, k)
    stream = torch.cuda.Stream()
    res = _decode_result(post, e0)
    sd = torch.as_tensor(np.array(syn), device="cuda")
    torch.cuda.synchronize()
    decoders.apply_osd_device(H, sd, res, lam, stream=stream.cuda_stream, method="cs")
    stream.synchronize()
    np.testing.assert_array_equal(res.ehat.cpu().numpy(), cases.model(name, k, lam)[0])
    ref = _decode_result(post, e0)
    decoders.apply_osd_device(H, sd, ref, 0, stream=stream.cuda_stream)
    stream.synchronize()
    np.testing.assert_array_equal(ref.ehat.cpu().numpy(), cases.host_order0(H, syn, cases.shots(name, k)[4], e0))


def _reference_loop(Hx, Hz, p, iters, sy_z, sy_x, errX, errZ, osd):
    """The reference's per-shot loop (simulator.py:270-303) with the oracle's
    min-sum and `osd(H, syn, post, e)` on each half's unconverged shots."""
    from oracle import oracle
    from qldpcsim_amd import simulator
    from qldpcsim_amd.schedule import pack_layers
    layersX, layersZ = simulator.select_layers(Hx, Hz, "F")
    out = []
    for H, syn, layers in ((Hz, sy_z, layersX), (Hx, sy_x, layersZ)):
        lp, lr = pack_layers(layers, H.shape[0])
        e, it, post, _ = oracle.decode_batch("MS", H, syn, p / 3, iters, lp, lr)
        e = np.array(e, dtype=np.uint8)
        bad = np.flatnonzero(np.any((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 != syn, axis=1))
        if bad.size:
            e[bad] = osd(H, syn[bad], post[bad], e[bad])
        out.append((e, it, bad.size))
    (eX, itX, nX), (eZ, itZ, nZ) = out
    shots = sy_z.shape[0]
    want = dict(DecFailures_X=0, DecFailures_Z=0, decSuccessExact=0, decSuccessDegen=0)
    for k in range(shots):
        if np.array_equal(errX[k], eX[k]) and np.array_equal(errZ[k], eZ[k]):
            want["decSuccessExact"] += 1
        elif ((Hz.astype(int) @ (errX[k].astype(int) ^ eX[k])) == 0).all() and \
                ((Hx.astype(int) @ (errZ[k].astype(int) ^ eZ[k])) == 0).all():    # (integer product: simulator.py:291)
            want["decSuccessDegen"] += 1
        want["DecFailures_X"] += int(not np.array_equal(sy_z[k], (Hz.astype(int) @ eX[k]) % 2))
        want["DecFailures_Z"] += int(not np.array_equal(sy_x[k], (Hx.astype(int) @ eZ[k]) % 2))
    want["Avg_number_of_iterations_X"] = itX.sum() / float(shots)
    want["Avg_number_of_iterations_Z"] = itZ.sum() / float(shots)
    return want, nX + nZ


def test_simulate_p_counters_equal_the_reference_loop_with_the_model():
    """LP04_0, 330 shots at p = 0.1, 3 min-sum iterations: the pipelined device
    path in batches of 100 and of 77 and the host path fed the same shots give
    the counters of the reference's loop run with the model's OSD-CS; a "ref"
    run gives those of the loop with today's order-0 OSD."""
    import torch
    from qldpcsim_amd import codes, decoders, simulator
    Hx, Hz = codes.load_code("LP04_0")
    p, shots, seed, iters, lam = 0.1, 330, 13, 3, 10
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), key)
    sy_z, sy_x, ewX, ewZ = ch.sample(p, shots)
    sy_z, sy_x = sy_z.cpu().numpy(), sy_x.cpu().numpy()
    errX, errZ = ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy()

    def model_osd(H, syn, post, e):
        return osd_cs_model.osd_cs_batch(H, syn, decoders.osd_perms(post), e, lam)[0]

    def order0(H, syn, post, e):
        return cases.host_order0(H, syn, np.ascontiguousarray(decoders.osd_perms(post), np.int32), e)

    want, osd_shots = _reference_loop(Hx, Hz, p, iters, sy_z, sy_x, errX, errZ, model_osd)
    want_ref, _ = _reference_loop(Hx, Hz, p, iters, sy_z, sy_x, errX, errZ, order0)
    assert osd_shots > 100 and want != want_ref          # OSD runs, and the search changes the counters
    kw = dict(shots=shots, decType="MS", decIterations=iters, decSchedule="F", rngSeed=seed, verbose=False)
    for batch in (100, 77):
        got = simulator.simulate_p(Hx, Hz, p, OSDorder=lam, osd_method="cs", batch_size=batch, sampler="device", **kw)
        assert got == want, batch
    host = simulator.simulate_p(Hx, Hz, p, OSDorder=lam, osd_method="cs", batch_size=100, sampler="host",
                                samples=(sy_z, sy_x, errX, errZ), **kw)
    assert host == want
    ref = simulator.simulate_p(Hx, Hz, p, OSDorder=0, osd_method="ref", batch_size=100, sampler="device", **kw)
    assert ref == want_ref
    assert simulator.simulate_p(Hx, Hz, p, OSDorder=0, batch_size=100, sampler="device", **kw) == want_ref
    with pytest.raises(ValueError):
        simulator.simulate_p(Hx, Hz, p, OSDorder=-1, osd_method="cs", **kw)
    with pytest.raises(ValueError):
        simulator.simulate_p(Hx, Hz, p, OSDorder=3, osd_method="cs", **dict(kw, decType="BF"))

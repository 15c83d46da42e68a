"""relay_vprior_kernel on the device: against relay_ms_kernel
where the prior row is uniform (GPU against GPU), against
tests/relay_vprior_model.py on general rows under both solution costs, bit for
bit (e_hat, iterations, posteriors as 64-bit patterns, flags, found and
best_leg), and through simulate_p and simulate_dem."""
import functools

import numpy as np
import pytest

import dem_model as dm
import logical_model
import relay_vprior_model as vm
from test_gpu_relay import _H, _channel, _same
from test_relay_vprior_model import vector_batch, vector_model

pytestmark = pytest.mark.gpu

COSTS = ("hamming", "prior")


def _noisy_quarter(n, base, seed, above_half=0):
    """A prior row: `base` everywhere, five times that on a quarter of the
    columns, 0.6 on `above_half` more (negative L_j and W_j)."""
    pick = np.random.default_rng(seed).permutation(n)
    q = np.full(n, base)
    q[pick[: n // 4]] = 5 * base
    q[pick[n // 4: n // 4 + above_half]] = 0.6
    return q


def _gpu(H, syn, q, T, G, S, cost, bits_in=False, bits_out=False, want_post=True, out=None):
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(syn, device="cuda:0")
    if bits_in:
        s = decoders.pack_bits(s)
    r = decoders.decode_batch(H, s, None, 0, algo="RELAY", relay=decoders.RelayConfig(T, G, S, prior=q, cost=cost),
                              want_post=want_post, ehat_bits=bits_out, out=out)
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("name,dc", [("steane", 0), ("LP04_0", 7), ("LP118_0", 8)])
def test_kernel_names_and_launch_info(name, dc):
    from qldpcsim_amd import _lib
    H = _H(name)
    n = H.shape[1]
    code = _lib.code_for(H, 0)
    rl = code.relay([5], np.zeros((1, n)), 1, prior=np.linspace(0.01, 0.2, n))
    assert rl.kernel_name() == f"relay_vprior_kernel<{dc}>"
    waves, wgs, lds = rl.launch_info()
    lay = rl.layout()
    assert waves >= 1 and wgs >= 1 and lds == lay["image"] + waves * lay["wave_bytes"]
    assert lay["image"] == code.relay([5], np.zeros((1, n)), 1).layout()["image"] + ((8 * n + 15) & ~15)


@pytest.mark.parametrize("name", ["steane", "LP04_0", "LP118_0"])
def test_uniform_row_equals_the_scalar_kernel(name):
    """A uniform row with cost "hamming" against decode_batch(algo="RELAY", p),
    GPU against GPU: every output tensor, B = 1, 65 and 1,001."""
    import torch
    from qldpcsim_amd import decoders
    H = _H(name)
    n = H.shape[1]
    p = 0.07 / 3
    T, G = [6, 5, 5], decoders.relay_gammas(n, 3, seed=7)
    for B in (1, 65, 1001):
        syn = _channel(H, B, 0.12 if name == "steane" else 0.07, 300 + B)
        s = torch.as_tensor(syn, device="cuda:0")
        w = decoders.decode_batch(H, s, p, 0, algo="RELAY", relay=decoders.RelayConfig(T, G, 2), want_post=True)
        r = _gpu(H, syn, np.full(n, p), T, G, 2, "hamming")
        assert torch.equal(r.ehat, w.ehat) and torch.equal(r.iters, w.iters) and torch.equal(r.flags, w.flags)
        assert torch.equal(r.post.view(torch.int64), w.post.view(torch.int64))
        assert torch.equal(r.found, w.found) and torch.equal(r.best_leg, w.best_leg)
        if B == 1001 and name != "steane":                       # (steane: every syndrome is solved twice)
            assert len(torch.unique(w.found)) == 3               # every count of solutions occurs


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("S", [3, 1])
def test_vector_batch_equals_the_model(S, cost):
    """LP04_0 Hz, selection_batch()'s syndromes, T = [10, 6, 6, 6, 6], a
    quarter of the columns at 0.12, five at 0.6, the rest at 0.02: found
    0 / 1 / 2 / 3 for 382 / 38 / 51 / 530 half-shots at S = 3, and the two costs
    keep different legs in 4 (test_relay_vprior_model.test_the_two_costs_part_ways)."""
    H, syn, q, T, G = vector_batch()
    want = vector_model(S, cost)
    if S == 3:
        np.testing.assert_array_equal(np.bincount(want[4], minlength=4), [382, 38, 51, 530])
    _same(_gpu(H, syn, q, T, G, S, cost), want, H.shape[1])


@pytest.mark.parametrize("cost", COSTS)
def test_lp118_0_equals_the_model(cost):
    """LP118_0 Hz (relay_vprior_kernel<8>), 130 half-shots at p = 0.07, a
    quarter of the columns five times as likely and three at 0.6,
    T = [12, 8, 8, 8], S = 2: found 0 / 1 / 2 for 53 / 17 / 60 half-shots."""
    from qldpcsim_amd import decoders
    H = _H("LP118_0")
    n = H.shape[1]
    syn = _channel(H, 130, 0.07, 5)
    q = _noisy_quarter(n, 0.07 / 3, 3, above_half=3)
    T, G = [12, 8, 8, 8], decoders.relay_gammas(n, 4, seed=7)
    want = vm.decode(H, syn, q, T, G, 2, cost)
    np.testing.assert_array_equal(np.bincount(want[4], minlength=3), [53, 17, 60])
    _same(_gpu(H, syn, q, T, G, 2, cost), want, n)


@functools.lru_cache(maxsize=None)
def _small_dem():
    """dem_model.edge_dem(20, 2, 41): 41 columns (one partial chunk), detector
    rows of degree 2 to 8. Below 64 columns edge_dem's priors are all 0.4, so
    the row is drawn here, log-uniform in [1e-3, 0.3]."""
    H, L, _, _ = dm.edge_dem(20, 2, 41)
    deg = H.sum(1)
    assert deg.min() != deg.max() and deg.max() <= 32
    pr = np.exp(np.random.default_rng(8).uniform(np.log(1e-3), np.log(0.3), H.shape[1]))
    return H, L, pr


@pytest.mark.parametrize("cost", COSTS)
@pytest.mark.parametrize("name", ["steane", "LP04_0_zero_col", "dem"])
def test_generic_instance_equals_the_model(name, cost):
    """relay_vprior_kernel<0>. steane: n = 7, one partial chunk, pad lanes;
    LP04_0 with column 70 zeroed: non-uniform rows and an isolated variable
    (whose M stays at its own L_j); a detector error model's matrix: rows of
    unequal degree, 41 columns."""
    from qldpcsim_amd import _lib, decoders
    if name == "dem":
        H, _, q = _small_dem()
        syn = ((np.random.default_rng(4).random((257, H.shape[1])) < q).astype(np.int64) @ H.T % 2).astype(np.uint8)
        hist = [5, 4, 248]
    else:
        H = _H(name)
        q = _noisy_quarter(H.shape[1], 0.08 / 3, 2, above_half=1 if name == "steane" else 3)
        syn = _channel(H, 257, 0.12 if name == "steane" else 0.08, 21)
        hist = [70, 22, 165] if name == "steane" else [111, 20, 126]
    n = H.shape[1]
    assert _lib.code_for(H, 0).relay([5], np.zeros((1, n)), 1, prior=q).kernel_name() == "relay_vprior_kernel<0>"
    T, G = [5, 5, 5], decoders.relay_gammas(n, 3, seed=7)
    want = vm.decode(H, syn, q, T, G, 2, cost)
    np.testing.assert_array_equal(np.bincount(want[4], minlength=3), hist)
    _same(_gpu(H, syn, q, T, G, 2, cost), want, n)


@pytest.mark.parametrize("bits_in,bits_out,want_post", [(True, True, False), (True, False, True), (False, True, True),
                                                        (False, False, False)])
def test_formats_and_out_reuse(bits_in, bits_out, want_post):
    """Both syndrome formats, bit-packed and byte estimates, posterior rows on
    and off; a second decode into the first one's buffers (out=)."""
    H, syn, q, T, G = vector_batch()
    n = H.shape[1]
    want = vector_model(3, "prior")
    r = _gpu(H, syn, q, T, G, 3, "prior", bits_in, bits_out, want_post)
    _same(r, want, n, bits_out, want_post)
    keep = r.ehat.data_ptr(), r.info.data_ptr()
    r.ehat.fill_(1), r.iters.fill_(-1), r.flags.fill_(-1), r.info.fill_(-7)
    r2 = _gpu(H, syn, q, T, G, 3, "prior", bits_in, bits_out, want_post, out=r)
    assert (r2.ehat.data_ptr(), r2.info.data_ptr()) == keep
    _same(r2, want, n, bits_out, want_post)
    with pytest.raises(ValueError, match="out buffers"):
        _gpu(H, syn[:10], q, T, G, 3, "prior", bits_in, bits_out, want_post, out=r)


@pytest.mark.parametrize("cost", COSTS)
def test_host_path_and_the_shim_equal_the_model(cost):
    from qldpcsim_amd import decoders
    H, syn, q, T, G = vector_batch()
    want = vector_model(3, cost)
    for want_post in (True, False):
        r = decoders.decode_batch(H, syn, None, 0, algo="RELAY", want_post=want_post,
                                  relay=decoders.RelayConfig(T, G, 3, prior=q, cost=cost))
        np.testing.assert_array_equal(r.ehat, want[0])
        np.testing.assert_array_equal(r.iters, want[1])
        if want_post:
            np.testing.assert_array_equal(r.post.view(np.uint64), want[2].view(np.uint64))
        np.testing.assert_array_equal(r.flags & (vm.FLAG_CONVERGED | vm.FLAG_MIN_ZERO), want[3])
        np.testing.assert_array_equal(r.found, want[4])
        np.testing.assert_array_equal(r.best_leg, want[5])
    differ = np.flatnonzero(vector_model(3, "hamming")[5] != vector_model(3, "prior")[5])
    for b in (5, int(differ[0])):                            # a shot on which the cost decides
        e, it = decoders.Relay_decoder(H, syn[b], q, T, G, sols=3, cost=cost)
        assert e.dtype == np.int8 and isinstance(it, int)
        np.testing.assert_array_equal(e, want[0][b])
        assert it == want[1][b]


@pytest.mark.parametrize("static", [0, 1])
def test_every_wave_restarts(static, qopt):
    """More than twice the half-shots the grid holds (one workgroup of one
    wave per CU): every wave decodes several, so a prior weight, a best
    solution or a `found` left over from the previous half-shot would show;
    cost "prior", queued and under static_sched."""
    import torch
    from qldpcsim_amd import _lib
    H, syn, q, T, G = vector_batch()
    qopt(wg_per_cu=1, waves_per_wg=1, static_sched=static)
    waves, wgs, _ = _lib.code_for(H, 0).relay(T, G, 3, prior=q).launch_info()
    assert (waves, wgs) == (1, 1)
    held = torch.cuda.get_device_properties(0).multi_processor_count
    assert len(syn) > 2 * held
    _same(_gpu(H, syn, q, T, G, 3, "prior"), vector_model(3, "prior"), H.shape[1])


def test_simulate_p_relay_priors():
    """simulate_p(decType="RELAY", relay_priors=True) on LP04_0, a quarter of
    the qubits five times as noisy, 3,000 shots, fixed seed: with logical=True
    the counters are logical_model's on the model's estimates (cost "prior":
    the default for a half decoded with a row); the device pipeline, the host
    path fed the same shots and another batch size agree."""
    import torch
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    p, shots, seed = 0.05, 3000, 11
    w = np.full((3, n), 1 / 3.0)
    w[:, np.random.default_rng(6).permutation(n)[: n // 4]] *= 5
    kw = dict(shots=shots, decType="RELAY", decIterations=10, relay_legs=4, relay_leg_iters=6, relay_sols=2,
              relay_seed=5, rngSeed=seed, verbose=False, channel_weights=w, relay_priors=True)
    got = simulator.simulate_p(Hx, Hz, p, batch_size=1000, sampler="device", logical=True, **kw)
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), key)
    ch.set_probs(simulator.channel_probs(p, w, n))
    sy_z, sy_x, ewX, ewZ = ch.sample(p, shots)
    sy_z, sy_x = sy_z.cpu().numpy(), sy_x.cpu().numpy()
    errX, errZ = ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy()
    grng = np.random.default_rng(5)                          # the Hz-decoded half draws first
    T = [10, 6, 6, 6]
    GX = np.vstack([np.full((1, n), 0.125), grng.uniform(-0.24, 0.66, (3, n))])
    GZ = np.vstack([np.full((1, n), 0.125), grng.uniform(-0.24, 0.66, (3, n))])
    mX = vm.decode(Hz, sy_z, p * (w[0] + w[1]), T, GX, 2, "prior")
    mZ = vm.decode(Hx, sy_x, p * (w[2] + w[1]), T, GZ, 2, "prior")
    c = logical_model.Model(Hx, Hz).counters(sy_z, sy_x, errX, errZ, mX[0], mZ[0], mX[1], mZ[1])
    assert c["DecFailures_X"] + c["DecFailures_Z"] > 0 and c["decSuccessLogical"] > 0
    for k in ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen", "logicalErrors_X",
              "logicalErrors_Z", "decSuccessLogical"):
        assert got[k] == c[k], k
    assert got["Avg_number_of_iterations_X"] == c["nIterAccX"] / float(shots)
    assert got["Avg_number_of_iterations_Z"] == c["nIterAccZ"] / float(shots)
    plain = simulator.simulate_p(Hx, Hz, p, batch_size=1000, sampler="device", **kw)
    host = simulator.simulate_p(Hx, Hz, p, batch_size=1000, sampler="host", samples=(sy_z, sy_x, errX, errZ), **kw)
    other = simulator.simulate_p(Hx, Hz, p, batch_size=777, sampler="device", **kw)
    assert plain == host == other
    assert plain == {k: got[k] for k in plain}
    with pytest.raises(ValueError, match="RELAY"):           # the refusal the flag lifts
        simulator.simulate_p(Hx, Hz, p, sampler="device", **{**kw, "relay_priors": False})


def test_simulate_dem_relay_priors(monkeypatch):
    """simulate_dem(decType="RELAY", relay_priors=True) on the small model,
    600 shots: the counters are dem_model's classes of the model's estimates,
    for the device sampler and for the host sampler fed the same shots."""
    from qldpcsim_amd import dem as D, simulator
    H, L, pr = _small_dem()
    model = D.Dem(H, L, pr)
    shots, seed = 600, 9
    kw = dict(shots=shots, decType="RELAY", decIterations=8, relay_legs=3, relay_leg_iters=5, relay_sols=2,
              relay_seed=4, rngSeed=seed, verbose=False, relay_priors=True)
    key = int(np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0])
    det, obs, _ = dm.sample(H, L, pr, key, 0, shots)
    n = H.shape[1]
    G = np.vstack([np.full((1, n), 0.125), np.random.default_rng(4).uniform(-0.24, 0.66, (2, n))])
    for cost in (None, "hamming"):
        e, it = vm.decode(H, det, pr, [8, 5, 5], G, 2, cost or "prior")[:2]
        c = dm.counters(dm.classify(H, L, det, obs, e)[0], it)
        want = [c["failures"], c["logical_errors"], c["successes"], c["iterations"]]
        assert min(want[:3]) > 0
        got = simulator.simulate_dem(model, sampler="device", batch_size=256, relay_cost=cost, **kw)
        assert [got[k] for k in simulator.DEM_KEYS] == want
        assert got == simulator.simulate_dem(model, sampler="device", relay_cost=cost, **kw)

        def same_shots(self, B, bits=False):
            at = self.shot
            self.shot += int(B)
            return det[at:at + B], obs[at:at + B]

        with monkeypatch.context() as mp:
            mp.setattr(simulator._HostDem, "sample", same_shots)
            host = simulator.simulate_dem(model, sampler="host", batch_size=256, relay_cost=cost, **kw)
        assert host == got
    with pytest.raises(ValueError, match="RELAY"):           # the refusal the flag lifts
        simulator.simulate_dem(model, sampler="device", **{**kw, "relay_priors": False})


def test_refusal_draws_no_shot(monkeypatch):
    """A detector row of 33 entries is past the relay's limits: it raises
    NotImplementedError when the handle is made, and the source's shot counter
    is still where it began, with unequal and with equal priors."""
    from qldpcsim_amd import dem as D, simulator
    rng = np.random.default_rng(5)
    H = np.zeros((12, 40), np.uint8)
    H[0, :33] = 1
    for j in range(40):
        H[1 + rng.choice(11, 2, replace=False), j] = 1
    L = np.zeros((1, 40), np.uint8)
    L[0, ::3] = 1
    made = []

    class Recording(simulator.DeviceDem):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(simulator, "DeviceDem", Recording)
    for priors in (np.linspace(0.001, 0.02, 40), np.full(40, 0.01)):
        with pytest.raises(NotImplementedError, match="row degree"):
            simulator.simulate_dem(D.Dem(H, L, priors), shots=64, decType="RELAY", decIterations=10, rngSeed=3,
                                   sampler="device", verbose=False, relay_priors=True)
        assert made[-1].shot == 0
    assert len(made) == 2

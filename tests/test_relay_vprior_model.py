"""Relay min-sum with per-variable priors without a device:
the test-side model (tests/relay_vprior_model.py) against relay_model (a
uniform row) and prior_model's min-sum (gamma = 0, one leg), its fixed-point
weights, the batch on which the two solution costs part ways, the static
launch arguments of relay_vprior_kernel, and the argument checks of the C
entry points, decode_batch, simulate_p and simulate_dem, all decided before
any HIP call."""
import ctypes
import functools

import numpy as np
import pytest

import dem_model as dm
import prior_model as pm
import relay_model as rm
import relay_vprior_model as vm
from qldpcsim_amd import _lib, codes, decoders, simulator
from test_relay_model import selection_batch


def vector_batch():
    """selection_batch()'s matrix, syndromes, legs and strengths (LP04_0 Hz,
    1,001 half-shots, T = [10, 6, 6, 6, 6]) with a prior row: a quarter of the
    columns at 0.12, five at 0.6 (L_j < 0, W_j < 0), the rest at 0.02. The
    seed was chosen with the model so that the two costs keep different legs
    (test_the_two_costs_part_ways); also the GPU test's batch."""
    H, syn, _, T, G = selection_batch()
    n = H.shape[1]
    pick = np.random.default_rng(19).permutation(n)
    q = np.full(n, 0.02)
    q[pick[: n // 4]] = 0.12
    q[pick[n // 4: n // 4 + 5]] = 0.6
    return H, syn, q, T, G


@functools.lru_cache(maxsize=None)
def vector_model(S, cost):
    """The model's six outputs on vector_batch(), computed once per (S, cost)
    and shared (read-only) with tests/test_gpu_relay_vprior.py."""
    H, syn, q, T, G = vector_batch()
    out = vm.decode(H, syn, q, T, G, S, cost)
    for a in out:
        a.setflags(write=False)
    return out


def _same(a, b):
    for x, y in zip(a, b):
        if x.dtype == np.float64:
            x, y = x.view(np.uint64), y.view(np.uint64)
        np.testing.assert_array_equal(x, y)


def test_uniform_row_is_the_scalar_model_on_steane():
    H = codes.load_code("steane")[0]
    n = H.shape[1]
    syn = np.random.default_rng(2).integers(0, 2, (64, H.shape[0]), dtype=np.uint8)
    T, G = [5, 5, 5], decoders.relay_gammas(n, 3, seed=7)
    for p in (0.08 / 3, 0.7):                                # L > 0 and L < 0
        _same(vm.decode(H, syn, np.full(n, p), T, G, 2, "hamming"), rm.decode(H, syn, p, T, G, 2))


@pytest.mark.parametrize("S", [1, 2, 3])
def test_uniform_row_is_the_scalar_model_on_the_selection_batch(S):
    """e_hat, iterations, posteriors as uint64, flags, found and best_leg."""
    H, syn, p, T, G = selection_batch()
    g = pm.Graph(H)
    _same(vm.decode(g, syn, np.full(g.n, p), T, G, S, "hamming"), rm.decode(g, syn, p, T, G, S))


def test_one_leg_without_memory_is_vector_prior_min_sum():
    """gamma = 0, one leg, S = 1 on vector_batch()'s row against prior_model's
    flooding MS with L[b, j] = L_j: e_hat, iterations, posterior bits, CONVERGED."""
    H, syn, q, _, _ = vector_batch()
    syn = syn[:96]
    n = H.shape[1]
    it_max = 20
    L = np.tile(vm.llr_row(q), (len(syn), 1))
    for cost in vm.COSTS:                                    # one solution: the cost cannot matter
        e, it, post, fl, found, leg = vm.decode(H, syn, q, [it_max], np.zeros((1, n)), 1, cost)
        e2, it2, post2, fl2 = pm.decode("MS", H, syn, L, it_max)
        conv = (fl2 & pm.FLAG_CONVERGED) != 0
        assert 0 < conv.sum() < len(syn)
        np.testing.assert_array_equal(e, e2)
        np.testing.assert_array_equal(it, it2)
        np.testing.assert_array_equal(post.view(np.uint64), post2.view(np.uint64))
        np.testing.assert_array_equal((fl & pm.FLAG_CONVERGED) != 0, conv)
        np.testing.assert_array_equal(found, conv)
        np.testing.assert_array_equal(leg, np.where(conv, 0, -1))


def test_weights_round_half_even():
    """W_j = round-half-even of L_j 2^20: the half-way cases by hand, and the
    row of vector_batch() against np.rint."""
    u = 2.0 ** -20
    L = np.array([0.5 * u, 1.5 * u, 2.5 * u, 3.5 * u, -0.5 * u, -1.5 * u, -2.5 * u, 1.25 * u, 1.75 * u, 3.0, -740.0])
    want = [0, 2, 2, 4, 0, -2, -2, 1, 2, 3 << 20, -740 << 20]
    got = vm.weights(L)
    assert got.dtype == np.int64 and got.tolist() == want
    Lq = vm.llr_row(vector_batch()[2])
    np.testing.assert_array_equal(vm.weights(Lq), np.rint(Lq * 2 ** 20).astype(np.int64))
    assert (vm.weights(Lq) < 0).sum() == 5                   # the five columns at q = 0.6


def test_the_two_costs_part_ways():
    """vector_batch(), S = 3: found 0 / 1 / 2 / 3 for 382 / 38 / 51 / 530
    half-shots under both costs (the legs run alike; only the choice differs),
    and in 4 of them the lightest solution by prior weight is another leg's
    than the lightest by Hamming weight."""
    H, syn, q, T, G = vector_batch()
    ham, pri = vector_model(3, "hamming"), vector_model(3, "prior")
    for k in (1, 2, 3, 4):
        np.testing.assert_array_equal(ham[k].view(np.uint64) if k == 2 else ham[k], pri[k].view(np.uint64) if k == 2
                                      else pri[k])
    np.testing.assert_array_equal(np.bincount(ham[4], minlength=4), [382, 38, 51, 530])
    differ = ham[5] != pri[5]
    assert int(differ.sum()) == 4
    assert np.all((ham[0] != pri[0]).any(1) == differ)
    W = vm.weights(vm.llr_row(q))
    wh, wp = ham[0][differ].astype(np.int64) @ W, pri[0][differ].astype(np.int64) @ W
    assert np.all(wp < wh) and np.all(pri[0][differ].sum(1) >= ham[0][differ].sum(1))
    for out in (ham, pri):
        ok = out[4] > 0
        assert np.all(((out[0][ok].astype(np.int64) @ H.T) % 2 == syn[ok]).all(1))


# ---------------------------------------------------------------------------
# C ABI: the static launch arguments and validation, no device needed
# ---------------------------------------------------------------------------
def _a16(x):
    return (x + 15) & ~15


@pytest.mark.parametrize("name,half,dc", [("steane", 0, 0), ("LP04_0", 1, 7), ("LP118_0", 1, 8), ("LP118_2", 1, 8)])
def test_static_launch_arguments(name, half, dc):
    """The scalar relay's image with the prior row f64[n] (16-byte aligned)
    behind it, the same wave slice, and the same instance of the other kernel."""
    H = codes.load_code(name)[half]
    n = H.shape[1]
    code = _lib.code_for(H)
    q = np.linspace(0.01, 0.2, n)
    G = np.zeros((2, n))
    scalar = code.relay([5, 5], G, 2)
    vec = code.relay([5, 5], G, 2, prior=q)
    assert vec is code.relay([5, 5], G, 2, prior=q.copy(), eps=1e-9) and vec is not scalar   # cached per row too
    assert vec is not code.relay([5, 5], G, 2, prior=q, eps=1e-6)
    assert scalar is code.relay([5, 5], G, 2) and scalar.prior is None and vec.prior is code.prior(q, 1e-9)
    assert scalar.kernel_name() == f"relay_ms_kernel<{dc}>"
    assert vec.kernel_name() == f"relay_vprior_kernel<{dc}>"
    a, b = scalar.layout(), vec.layout()
    assert b.pop("image") == a.pop("image") + _a16(8 * n)
    assert a == b


def test_c_entry_points_validate_before_any_hip_call():
    L = _lib.lib
    Hx, _ = codes.load_code("steane")
    code = _lib.Code(Hx)
    other = _lib.Code(Hx)
    m, n = code.m, code.n
    rl = code.relay([3, 4], np.zeros((2, n)), 1)
    q = np.linspace(0.01, 0.2, n)
    pr = code.prior(q, 1e-9)
    syn = np.zeros((2, m), np.uint8)
    e = np.zeros((2, n), np.uint8)
    it = np.zeros(2, np.int32)
    P = _lib.ptr

    def dev(c=code.handle, r=rl.handle, pv=pr.handle, cost=0, s=syn, sf=0, batch=2, eps=1e-9, eh=e, ef=0, i=it):
        return L.qldpc_decode_device_relay_vprior(c, r, pv, cost, P(s), sf, batch, 0.75, eps, P(eh), ef, P(i), None,
                                                  None, None, None)

    def host(c=code.handle, r=rl.handle, pv=pr.handle, cost=1, s=syn, batch=2, eps=1e-9):
        return L.qldpc_decode_host_relay_vprior(c, r, pv, cost, P(s), batch, 0.75, eps, P(e), P(it), None, None, None)

    EINVAL = _lib.QLDPC_EINVAL
    assert dev(sf=2) == EINVAL and dev(ef=7) == EINVAL
    assert dev(c=None) == EINVAL and dev(r=None) == EINVAL
    assert dev(pv=None) == EINVAL and b"prior handle is null" in L.qldpc_last_error()
    assert dev(pv=other.prior(q, 1e-9).handle) == EINVAL and b"different code" in L.qldpc_last_error()
    assert dev(eps=1e-6) == EINVAL and b"eps" in L.qldpc_last_error()
    assert dev(cost=2) == EINVAL and dev(cost=-1) == EINVAL and b"cost" in L.qldpc_last_error()
    assert dev(batch=-1) == EINVAL
    assert dev(s=None) == EINVAL and dev(eh=None) == EINVAL and dev(i=None) == EINVAL
    for cost in (0, 1):
        assert dev(cost=cost, batch=0, s=None, eh=None, i=None) == _lib.QLDPC_OK
    assert host(pv=None) == EINVAL and host(s=None) == EINVAL and host(batch=-1) == EINVAL and host(cost=3) == EINVAL
    assert host(eps=1e-7) == EINVAL
    assert host(batch=0) == _lib.QLDPC_OK
    buf = ctypes.create_string_buffer(64)
    out7 = np.zeros(7, np.int32)
    with _lib.options(force_hbm=1):
        assert dev() == _lib.QLDPC_EUNSUP and b"force_hbm" in L.qldpc_last_error()
        assert host() == _lib.QLDPC_EUNSUP
        assert L.qldpc_decode_relay_vprior_kernel_name(code.handle, rl.handle, buf, 64) == _lib.QLDPC_EUNSUP
        assert L.qldpc_relay_vprior_layout(rl.handle, P(out7)) == _lib.QLDPC_EUNSUP
    assert L.qldpc_decode_relay_vprior_kernel_name(code.handle, rl.handle, buf, 64) == _lib.QLDPC_OK
    assert buf.value == b"relay_vprior_kernel<0>"
    assert L.qldpc_decode_relay_vprior_kernel_name(other.handle, rl.handle, buf, 64) == EINVAL
    assert L.qldpc_relay_vprior_layout(None, P(out7)) == EINVAL and L.qldpc_relay_vprior_layout(rl.handle, None) == EINVAL
    w = ctypes.c_int()
    assert L.qldpc_decode_relay_vprior_launch_info(code.handle, None, w, w, w) == EINVAL


def test_decode_batch_validates_the_prior_row_and_the_cost():
    Hx, _ = codes.load_code("steane")
    m, n = Hx.shape
    syn = np.zeros((2, m), np.uint8)
    q = np.linspace(0.01, 0.2, n)

    def run(p, **cfg):
        return decoders.decode_batch(Hx, syn, p, 0, algo="RELAY",
                                     relay=decoders.RelayConfig([3, 3], decoders.relay_gammas(n, 2), 1, **cfg))

    with pytest.raises(ValueError, match="give the prior row"):
        run(0.01, cost="prior")
    with pytest.raises(ValueError, match="relay.cost must be one of"):
        run(0.01, cost="weight")
    with pytest.raises(ValueError, match="relay.cost must be one of"):
        run(None, prior=q, cost="Prior")
    with pytest.raises(ValueError, match="not both"):
        run(0.01, prior=q)
    with pytest.raises(ValueError, match=r"relay.prior must hold 7 probabilities .* got shape \(6,\)"):
        run(None, prior=q[:6])
    with pytest.raises(ValueError, match="relay.prior must hold 7"):
        run(None, prior=q.reshape(1, n))
    for bad in (1.0, 1.5, -0.1, np.nan):
        qb = q.copy()
        qb[3] = bad
        with pytest.raises(ValueError, match=r"p\[3\]"):
            run(None, prior=qb)
    cfg = decoders.RelayConfig([3], np.zeros((1, n)))
    assert (cfg.sols, cfg.prior, cfg.cost) == (1, None, "hamming")             # the new fields trail, with defaults
    with pytest.raises(ValueError, match="give the prior row"):
        decoders.Relay_decoder(Hx, syn[0] | 1, 0.01, [3], np.zeros((1, n)), cost="prior")
    with pytest.raises(NotImplementedError, match="row degree"):
        H = np.ones((1, 40), np.uint8)
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), None, 0, algo="RELAY",
                              relay=decoders.RelayConfig([3], np.zeros((1, 40)), 1, prior=np.full(40, 0.1)))


def _weights(n):
    """[3, n] Pauli weights: unequal marginals in both halves."""
    return np.random.default_rng(5).random((3, n)) * np.array([[1.0], [0.5], [2.0]])


def test_simulate_p_refuses_what_the_flag_does_not_lift():
    Hx, Hz = codes.load_code("steane")
    n = Hx.shape[1]
    kw = dict(shots=4, sampler="host", verbose=False, decType="RELAY", channel_weights=_weights(n), relay_priors=True)
    with pytest.raises(ValueError, match="OSD"):
        simulator.simulate_p(Hx, Hz, 0.05, OSDorder=0, **kw)
    with pytest.raises(ValueError, match="flooding"):
        simulator.simulate_p(Hx, Hz, 0.05, decSchedule="L", **kw)
    with pytest.raises(ValueError, match="relay_cost must be one of"):
        simulator.simulate_p(Hx, Hz, 0.05, relay_cost="weight", **kw)
    half_uniform = np.array([[0.2] * n, [0.1] * n, np.linspace(0.1, 0.7, n)])      # the Hz-decoded half is scalar
    for w in (half_uniform, [0.2, 0.1, 0.7], None):
        with pytest.raises(ValueError, match="scalar prior"):
            simulator.simulate_p(Hx, Hz, 0.05, relay_cost="prior", **{**kw, "channel_weights": w})
    with pytest.raises(ValueError, match="scalar prior"):
        simulator.simulate_p(Hx, Hz, 0.05, shots=4, sampler="host", verbose=False, decType="RELAY", relay_cost="prior")
    with pytest.raises(ValueError, match="decType RELAY"):
        simulator.simulate_p(Hx, Hz, 0.05, shots=4, sampler="host", verbose=False, relay_priors=True)


def _small_dem():
    from qldpcsim_amd import dem as D
    H, L, pr, _ = dm.edge_dem(20, 2, 41)
    return D.Dem(H, L, pr)


def test_simulate_dem_refuses_what_the_flag_does_not_lift():
    model = _small_dem()
    kw = dict(shots=4, sampler="host", verbose=False, decType="RELAY", relay_priors=True)
    with pytest.raises(ValueError, match="OSD"):
        simulator.simulate_dem(model, OSDorder=0, **kw)
    for sched in ("L", "S"):
        with pytest.raises(ValueError, match="flooding"):
            simulator.simulate_dem(model, decSchedule=sched, **kw)
    with pytest.raises(ValueError, match="hbm_priors"):
        simulator.simulate_dem(model, hbm_priors=True, **kw)
    with pytest.raises(ValueError, match="relay_legs"):
        simulator.simulate_dem(model, relay_legs=0, **kw)
    with pytest.raises(ValueError, match="relay_cost must be one of"):
        simulator.simulate_dem(model, relay_cost="weight", **kw)
    from qldpcsim_amd import dem as D
    flat = D.Dem(model.H, model.L, np.full(model.num_errors, 0.01))
    with pytest.raises(ValueError, match="scalar prior"):
        simulator.simulate_dem(flat, relay_cost="prior", **kw)
    with pytest.raises(ValueError, match="decType RELAY"):
        simulator.simulate_dem(model, shots=4, sampler="host", verbose=False, decType="MS", relay_priors=True)
    with pytest.raises(ValueError, match="decType RELAY"):
        simulator.simulate_dem(model, shots=4, sampler="host", verbose=False, decType="MS", relay_cost="hamming")


def test_cli_flags(tmp_path, monkeypatch, capsys):
    """--relay-priors lifts the --dem refusal and reaches simulate_dem and the
    record with --relay-cost and the relay_* settings; --relay-cost alone, the
    flag without RELAY and with --hbm-priors are usage errors."""
    import json
    model = _small_dem()
    f = tmp_path / "model.npz"
    np.savez(f, H=model.H, L=model.L, priors=model.priors)
    calls = []

    def fake(dem, **kw):
        calls.append(kw)
        return {"DecFailures": 0, "logicalErrors": 0, "decSuccess": kw["shots"], "nIterAcc": 7,
                "logical_error_rate": 0.0, "logical_error_rate_ci95": [0.0, 0.1], "detectors": 20, "errors": 41,
                "observables": 2}

    monkeypatch.setattr(simulator, "simulate_dem", fake)
    res = tmp_path / "res.json"
    base = ["--dem", str(f), "--shots", "5", "--decType", "RELAY", "--sampler", "host"]
    simulator.main(base + ["--relay-priors", "--relay-cost", "hamming", "--relay-legs", "4", "--results", str(res)])
    kw = calls[-1]
    assert (kw["decType"], kw["relay_priors"], kw["relay_cost"], kw["relay_legs"], kw["relay_seed"]) == \
        ("RELAY", True, "hamming", 4, 0)
    meta = json.loads(res.read_text())["meta"]
    assert (meta["relay_priors"], meta["relay_cost"], meta["relay_legs"], meta["relay_gamma_range"]) == \
        (True, "hamming", 4, [-0.24, 0.66])
    simulator.main(base + ["--relay-priors"])
    assert calls[-1]["relay_cost"] is None
    capsys.readouterr()
    for bad in (["--relay-cost", "prior"], ["--relay-priors", "--hbm-priors"]):
        with pytest.raises(SystemExit) as ex:
            simulator.main(base + bad)
        assert ex.value.code == 2
    with pytest.raises(SystemExit) as ex:
        simulator.main(["--dem", str(f), "--decType", "MS", "--relay-priors"])
    assert ex.value.code == 2 and "--relay-priors needs --decType RELAY" in capsys.readouterr().err


def test_sweep_records_the_flag(tmp_path, monkeypatch):
    """simulate(): relay_priors and relay_cost reach simulate_p and the meta
    next to the other relay_* keys only when the flag is given."""
    import json
    Hx, Hz = codes.load_code("steane")
    fx, fz = str(tmp_path / "hx.npy"), str(tmp_path / "hz.npy")
    np.save(fx, Hx)
    np.save(fz, Hz)
    calls = []

    def fake(Hx, Hz, p, shots, **kw):
        calls.append(kw)
        return {"DecFailures_X": 0, "DecFailures_Z": 0, "decSuccessExact": shots, "decSuccessDegen": 0,
                "Avg_number_of_iterations_X": 1.0, "Avg_number_of_iterations_Z": 1.0}

    monkeypatch.setattr(simulator, "simulate_p", fake)
    common = dict(shots=4, verbose=False, sampler="host", decType="RELAY", channel_weights=_weights(7))
    rf = str(tmp_path / "a.json")
    simulator.simulate(fx, fz, [0.01], resultsFile=rf, **common)
    assert "relay_priors" not in calls[-1] and "relay_cost" not in calls[-1]
    assert not {"relay_priors", "relay_cost"} & set(json.load(open(rf))["meta"])
    rf = str(tmp_path / "b.json")
    simulator.simulate(fx, fz, [0.01], resultsFile=rf, relay_priors=True, **common)
    meta = json.load(open(rf))["meta"]
    assert (calls[-1]["relay_priors"], calls[-1]["relay_cost"]) == (True, None)
    assert (meta["relay_priors"], meta["relay_cost"], meta["relay_legs"]) == (True, None, 11)
    with pytest.raises(ValueError, match="relay_cost needs relay_priors"):
        simulator.simulate(fx, fz, [0.01], relay_cost="prior", **common)
    with pytest.raises(ValueError, match="relay_priors goes with decType RELAY"):
        simulator.simulate(fx, fz, [0.01], relay_priors=True, **{**common, "decType": "MS"})

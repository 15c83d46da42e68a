"""Relay min-sum without a device: the test-side model (tests/relay_model.py)
against plain min-sum and the reference's goldens (gamma = 0, one leg), its
effect and the branches of its solution selection on fixed inputs, and the
argument checks of the C entry points, decode_batch and simulate_p, all
decided before any HIP call."""
import ctypes
import json

import numpy as np
import pytest

import prior_model as pm
import relay_model as rm
from conftest import golden_cases, half_matrix
from qldpcsim_amd import _lib, codes, decoders, simulator


def _flood(c, a, m):
    lp, lr = a["layer_ptr"], a["layer_rows"]
    return "raises" not in c and c["osd"] < 0 and len(lp) == 2 and np.array_equal(lr, np.arange(m))


GOLD = []
for _code in ("LP04_0", "LP118_0", "steane"):
    _cs = [(c, a) for c, a in golden_cases(f"ms_{_code}.npz") if _flood(c, a, half_matrix(c).shape[0])]
    assert _cs, _code
    GOLD += _cs[:4]


@pytest.mark.parametrize("ca", GOLD, ids=[f"{c['code']}-{c['half']}-{c['kind']}-p{c['p_phys']}-it{c['max_iter']}"
                                          for c, _ in GOLD])
def test_one_leg_without_memory_is_plain_min_sum(ca):
    """gamma = 0, one leg, S = 1: e_hat, iterations and posterior bits of the
    reference's goldens and of prior_model's MS."""
    c, a = ca
    H = half_matrix(c)
    n = H.shape[1]
    syn = a["syn"][:32]
    p = c["p_phys"] / 3
    e, it, post, fl, found, leg = rm.decode(H, syn, p, [c["max_iter"]], np.zeros((1, n)), 1)
    assert np.isfinite(post).all()
    np.testing.assert_array_equal(it, a["iters"][:32])
    np.testing.assert_array_equal(e, a["ehat"][:32])
    np.testing.assert_array_equal(post.view(np.uint64), a["post"][:32].view(np.uint64))
    e2, it2, post2, fl2 = pm.decode("MS", H, syn, np.full((len(syn), n), pm.llr(p)), c["max_iter"])
    np.testing.assert_array_equal(it, it2)
    np.testing.assert_array_equal(e, e2)
    np.testing.assert_array_equal(post.view(np.uint64), post2.view(np.uint64))
    np.testing.assert_array_equal(fl & pm.FLAG_CONVERGED, fl2 & pm.FLAG_CONVERGED)
    np.testing.assert_array_equal(found, (fl2 & pm.FLAG_CONVERGED) != 0)
    np.testing.assert_array_equal(leg, np.where(found > 0, 0, -1))


def test_gamma_table_helper():
    g = decoders.relay_gammas(5, 3, seed=7)
    assert g.shape == (3, 5) and g.dtype == np.float64 and np.all(g[0] == 0.125)
    np.testing.assert_array_equal(g[1:], np.random.default_rng(7).uniform(-0.24, 0.66, (2, 5)))
    assert np.all(decoders.relay_gammas(4, 1, gamma0=0.3) == 0.3)


def selection_batch():
    """The batch that reaches every branch of the solution selection (LP04_0
    Hz, p = 0.08, 1,001 half-shots, T = [10, 6, 6, 6, 6], S = 3); also the
    GPU test's batch."""
    Hz = codes.load_code("LP04_0")[1]
    m, n = Hz.shape
    err = (np.random.default_rng(5).random((1001, n)) < 2 * 0.08 / 3).astype(np.int64)
    syn = ((err @ Hz.T) % 2).astype(np.uint8)
    return Hz, syn, 0.08 / 3, [10, 6, 6, 6, 6], decoders.relay_gammas(n, 5, seed=7)


def test_effect_on_lp04_0():
    """LP04_0 Hz, p = 0.06, 2,000 half-shots: min-sum with 30 iterations solves
    1,916, the relay (T = [30] * 9, S = 1) 1,972 at 10.77 passes per half-shot,
    and 1 half-shot that min-sum solves the relay does not (the counts of the
    CPU prototype, reproduced by this model)."""
    Hz = codes.load_code("LP04_0")[1]
    g = pm.Graph(Hz)
    B, p = 2000, 0.06
    err = (np.random.default_rng(3).random((B, g.n)) < 2 * p / 3).astype(np.int64)
    syn = (err @ Hz.T) % 2
    _, _, _, fl = pm.decode("MS", g, syn, np.full((B, g.n), pm.llr(p / 3)), 30)
    ms = (fl & pm.FLAG_CONVERGED) != 0
    e, it, post, flr, found, leg = rm.decode(g, syn, p / 3, [30] * 9, decoders.relay_gammas(g.n, 9, seed=7), 1)
    rl = found > 0
    assert np.isfinite(post).all()
    assert np.all(((e.astype(np.int64) @ Hz.T) % 2 == syn).all(1) == rl)
    print("MS solved", ms.sum(), "relay solved", rl.sum(), "MS only", (ms & ~rl).sum(), "passes", it.mean())
    assert rl.sum() > ms.sum()
    assert (int(ms.sum()), int(rl.sum()), int((ms & ~rl).sum())) == (1916, 1972, 1)


def test_selection_reaches_every_branch():
    """found 0 / 1 / 2 / 3 for 206 / 36 / 44 / 715 half-shots; among those with
    two or more solutions a later, strictly lighter one replaced the first in
    6 and the first was kept in 753."""
    H, syn, p, T, G = selection_batch()
    e3, it3, post3, fl3, found3, leg3 = rm.decode(H, syn, p, T, G, 3)
    e1, it1, post1, fl1, found1, leg1 = rm.decode(H, syn, p, T, G, 1)
    assert np.isfinite(post3).all()
    np.testing.assert_array_equal(np.bincount(found3, minlength=4), [206, 36, 44, 715])
    multi = found3 >= 2
    replaced = multi & (leg3 != leg1)
    kept = multi & (leg3 == leg1)
    assert (int(replaced.sum()), int(kept.sum())) == (6, 753)
    assert np.all(e3[replaced].sum(1) < e1[replaced].sum(1))
    np.testing.assert_array_equal(e3[kept], e1[kept])
    ok = found3 > 0
    assert np.all(((e3[ok].astype(np.int64) @ H.T) % 2 == syn[ok]).all(1))
    np.testing.assert_array_equal((fl3 & pm.FLAG_CONVERGED) != 0, ok)
    np.testing.assert_array_equal(leg3 >= 0, ok)


# ---------------------------------------------------------------------------
# C ABI: validation and the static launch arguments, no device needed
# ---------------------------------------------------------------------------
def _create(code, T, G, sols, n=None):
    T = np.ascontiguousarray(T, np.int32)
    G = np.ascontiguousarray(G, np.float64)
    h = ctypes.c_void_p()
    rc = _lib.lib.qldpc_relay_create(code.handle, len(T), _lib.ptr(T), _lib.ptr(G), G.shape[1] if n is None else n,
                                     sols, ctypes.byref(h))
    if rc == _lib.QLDPC_OK:
        _lib.lib.qldpc_relay_destroy(h)
    return rc, _lib.lib.qldpc_last_error()


def test_relay_create_validates():
    Hx, _ = codes.load_code("steane")
    code = _lib.Code(Hx)
    n = code.n
    G = np.zeros((2, n))
    EINVAL = _lib.QLDPC_EINVAL
    assert _create(code, [3, 4], G, 1)[0] == _lib.QLDPC_OK
    assert _create(code, [], np.zeros((0, n)), 1)[0] == EINVAL                   # R = 0
    assert _create(code, [3, 0], G, 1)[0] == EINVAL                              # a zero T
    assert _create(code, [1 << 19, (1 << 19) + 1], G, 1)[0] == EINVAL            # sum T past 2^20
    assert _create(code, [1 << 19, 1 << 19], G, 1)[0] == _lib.QLDPC_OK
    assert _create(code, [3, 4], G, 0)[0] == EINVAL                              # S = 0
    for bad in (np.nan, np.inf):
        Gb = G.copy()
        Gb[1, 3] = bad
        rc, msg = _create(code, [3, 4], Gb, 1)
        assert rc == EINVAL and b"gamma[1][3]" in msg
    rc, msg = _create(code, [3, 4], np.zeros((2, n + 1)), 1)                     # a table for another n
    assert rc == EINVAL and b"variables" in msg
    h = ctypes.c_void_p()
    T = np.array([3], np.int32)
    assert _lib.lib.qldpc_relay_create(None, 1, _lib.ptr(T), _lib.ptr(G), n, 1, ctypes.byref(h)) == EINVAL
    assert _lib.lib.qldpc_relay_create(code.handle, 1, None, _lib.ptr(G), n, 1, ctypes.byref(h)) == EINVAL
    assert _lib.lib.qldpc_relay_create(code.handle, 1, _lib.ptr(T), None, n, 1, ctypes.byref(h)) == EINVAL
    assert _lib.lib.qldpc_relay_create(code.handle, 1, _lib.ptr(T), _lib.ptr(G), n, 1, None) == EINVAL
    with pytest.raises(ValueError, match="one row per leg"):
        code.relay([3, 4], np.zeros((3, n)), 1)


def _a16(x):
    return (x + 15) & ~15


@pytest.mark.parametrize("name,half,kernel", [("steane", 0, "relay_ms_kernel<0>"), ("LP04_0", 1, "relay_ms_kernel<7>"),
                                              ("LP118_0", 1, "relay_ms_kernel<8>"),
                                              ("LP118_2", 1, "relay_ms_kernel<8>")])
def test_static_launch_arguments(name, half, kernel):
    """The wave slice: X f64[n] | c2v f32[E + 8] | syndrome words | M f64[n] |
    hard-decision words | best-solution words, every part 16-byte aligned."""
    H = codes.load_code(name)[half]
    m, n = H.shape
    E = int((H % 2).sum())
    code = _lib.code_for(H)
    rl = code.relay([5, 5], np.zeros((2, n)), 2)
    assert rl is code.relay([5, 5], np.zeros((2, n)), 2)                         # cached per (T, table, S)
    assert rl is not code.relay([5, 5], np.zeros((2, n)), 1)
    assert rl.kernel_name() == kernel
    lay = rl.layout()
    wm, wn = (m + 63) // 64, (n + 63) // 64
    off_c2v = _a16(8 * n)
    off_synw = _a16(off_c2v + 4 * (E + 8))
    off_m = _a16(off_synw + 8 * wm)
    off_ew = _a16(off_m + 8 * n)
    off_best = _a16(off_ew + 8 * wn)
    assert (lay["off_c2v"], lay["off_synw"], lay["off_m"], lay["off_ew"], lay["off_best"]) == \
        (off_c2v, off_synw, off_m, off_ew, off_best)
    assert lay["wave_bytes"] == _a16(off_best + 8 * wn)
    assert lay["image"] > 0 and lay["image"] % 16 == 0


def test_c_entry_points_validate_before_any_hip_call():
    L = _lib.lib
    Hx, _ = codes.load_code("steane")
    code = _lib.Code(Hx)
    other = _lib.Code(Hx)
    m, n = code.m, code.n
    rl = code.relay([3, 4], np.zeros((2, n)), 1)
    syn = np.zeros((2, m), np.uint8)
    e = np.zeros((2, n), np.uint8)
    it = np.zeros(2, np.int32)
    P = _lib.ptr

    def dev(c=code.handle, r=rl.handle, s=syn, sf=0, batch=2, eh=e, ef=0, i=it):
        return L.qldpc_decode_device_relay(c, r, P(s), sf, batch, 0.01, 0.75, 1e-9, P(eh), ef, P(i), None, None, None,
                                           None)

    def host(c=code.handle, r=rl.handle, s=syn, batch=2):
        return L.qldpc_decode_host_relay(c, r, P(s), batch, 0.01, 0.75, 1e-9, P(e), P(it), None, None, None)

    EINVAL = _lib.QLDPC_EINVAL
    assert dev(sf=2) == EINVAL and dev(ef=7) == EINVAL
    assert dev(c=None) == EINVAL and dev(r=None) == EINVAL
    assert dev(c=other.handle) == EINVAL and b"different code" in L.qldpc_last_error()
    assert dev(batch=-1) == EINVAL
    assert dev(s=None) == EINVAL and dev(eh=None) == EINVAL and dev(i=None) == EINVAL
    assert dev(batch=0, s=None, eh=None, i=None) == _lib.QLDPC_OK
    assert host(r=None) == EINVAL and host(s=None) == EINVAL and host(batch=-1) == EINVAL
    assert host(batch=0) == _lib.QLDPC_OK
    buf = ctypes.create_string_buffer(64)
    with _lib.options(force_hbm=1):
        assert dev() == _lib.QLDPC_EUNSUP and b"force_hbm" in L.qldpc_last_error()
        assert host() == _lib.QLDPC_EUNSUP
        assert L.qldpc_decode_relay_kernel_name(code.handle, rl.handle, buf, 64) == _lib.QLDPC_EUNSUP
    assert _lib.get_option("force_hbm") == 0
    assert L.qldpc_decode_relay_kernel_name(code.handle, rl.handle, buf, 64) == _lib.QLDPC_OK
    assert buf.value == b"relay_ms_kernel<0>"
    assert L.qldpc_decode_relay_kernel_name(other.handle, rl.handle, buf, 64) == EINVAL


def test_codes_past_the_lds_kernel_are_refused_before_any_launch():
    H = np.zeros((1, 65536), np.uint8)
    H[0, :3] = 1
    cfg = decoders.RelayConfig([3], np.zeros((1, 65536)), 1)
    with pytest.raises(NotImplementedError, match="65535"):
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), 0.01, 0, algo="RELAY", relay=cfg)
    H = np.ones((1, 40), np.uint8)
    with pytest.raises(NotImplementedError, match="row degree"):
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), 0.01, 0, algo="RELAY",
                              relay=decoders.RelayConfig([3], np.zeros((1, 40)), 1))


def test_decode_batch_validates_relay_arguments():
    Hx, _ = codes.load_code("steane")
    m, n = Hx.shape
    syn = np.zeros((2, m), np.uint8)
    cfg = decoders.RelayConfig([3, 3], decoders.relay_gammas(n, 2), 1)
    kw = dict(algo="RELAY", relay=cfg)
    with pytest.raises(ValueError, match="RelayConfig"):
        decoders.decode_batch(Hx, syn, 0.01, 5, algo="RELAY")
    with pytest.raises(ValueError, match='algo="RELAY"'):
        decoders.decode_batch(Hx, syn, 0.01, 5, algo="MS", relay=cfg)
    with pytest.raises(ValueError, match="flooding"):
        decoders.decode_batch(Hx, syn, 0.01, 5, layers=[[0], [1, 2]], **kw)
    with pytest.raises(ValueError, match="prior"):
        decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=np.zeros((2, n), np.uint8), p_masked=0.4, **kw)
    with pytest.raises(ValueError, match="OSD"):
        decoders.decode_batch(Hx, syn, 0.01, 5, osd_order=0, **kw)
    with pytest.raises(ValueError, match="one row per leg"):
        decoders.decode_batch(Hx, syn, 0.01, 5, algo="RELAY",
                              relay=decoders.RelayConfig([3, 3], np.zeros((2, n + 1)), 1))
    with pytest.raises(ValueError, match="sols"):
        decoders.decode_batch(Hx, syn, 0.01, 5, algo="RELAY", relay=decoders.RelayConfig([3, 3], np.zeros((2, n)), 0))
    with pytest.raises(ValueError, match="Unrecognized decoder type"):
        decoders.decode_batch(Hx, syn, 0.01, 5, algo="RELAYS")


def test_simulate_p_refuses_what_relay_does_not_do():
    Hx, Hz = codes.load_code("steane")
    kw = dict(shots=4, sampler="host", verbose=False, decType="RELAY")
    with pytest.raises(ValueError, match="OSD"):
        simulator.simulate_p(Hx, Hz, 0.05, OSDorder=0, **kw)
    with pytest.raises(ValueError, match="correlated"):
        simulator.simulate_p(Hx, Hz, 0.05, correlated="XZ", **kw)
    with pytest.raises(ValueError, match="flooding"):
        simulator.simulate_p(Hx, Hz, 0.05, decSchedule="L", **kw)
    with pytest.raises(ValueError, match="relay_legs"):
        simulator.simulate_p(Hx, Hz, 0.05, relay_legs=0, **kw)


def test_cli_knows_the_relay_options(tmp_path, monkeypatch):
    """--decType RELAY and the relay keywords reach simulate_p and the results
    file's meta, so a resumed sweep cannot mix settings (simulate_p itself is
    stubbed out)."""
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
    rf = str(tmp_path / "res.json")
    run = lambda **kw: simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, sampler="host",  # noqa: E731
                                          resultsFile=rf, decType="RELAY", **kw)
    run(relay_legs=5, relay_seed=3)
    meta = json.load(open(rf))["meta"]
    assert meta["decType"] == "RELAY"
    assert (meta["relay_legs"], meta["relay_leg_iters"], meta["relay_sols"], meta["relay_gamma0"],
            meta["relay_gamma_range"], meta["relay_seed"]) == (5, 60, 1, 0.125, [-0.24, 0.66], 3)
    assert calls[-1]["relay_legs"] == 5 and calls[-1]["relay_seed"] == 3
    run(relay_legs=5, relay_seed=3)                              # same settings: resumed
    assert len(calls) == 1
    with pytest.raises(ValueError, match="different run"):
        run(relay_legs=6, relay_seed=3)
    with pytest.raises(SystemExit):
        simulator.main(["--Hx", fx, "--Hz", fz, "--p", "0.1", "--decType", "RELAY", "--relay-gamma-range", "0.1"])

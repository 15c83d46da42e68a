"""Logical operators of a CSS pair and the logical outcome counters on the
host: css_logicals' identities on every bundled code, count_logical_outcomes
against the independent model (tests/logical_model.py), simulate_p / the CLI
with the option on and off, the Wilson interval, and the C ABI's argument
checks (no device needed)."""
import ctypes
import json

import numpy as np
import pytest

import logical_model as lm
from qldpcsim_amd import _lib, codes, logicals, simulator

K = {"steane": 1, "shor": 1, "LP04_0": 19, "LP04_1": 21, "LP04_2": 29, "LP04_3": 31, "LP118_0": 80,
     "LP118_1": 100, "LP118_2": 136, "T": 140}
SIX = {"DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen", "Avg_number_of_iterations_X",
       "Avg_number_of_iterations_Z"}


def _rank(M):
    """GF(2) rank by the model's own elimination (n - dim ker)."""
    M = np.asarray(M)
    return M.shape[1] - lm.nullspace(M).shape[0]


def _m2(A, B):
    return (np.asarray(A).astype(np.int64) @ np.asarray(B).astype(np.int64).T) % 2


@pytest.mark.parametrize("name", sorted(K))
def test_css_logicals_identities_on_bundled_codes(name):
    Hx, Hz = codes.load_code(name)
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    n, k = Hx.shape[1], K[name]
    assert Lx.shape == (k, n) and Lz.shape == (k, n) and Lx.dtype == np.int8 and Lz.dtype == np.int8
    assert set(np.unique(Lx)) <= {0, 1} and set(np.unique(Lz)) <= {0, 1}
    rx, rz = _rank(Hx), _rank(Hz)
    assert k == n - rx - rz
    assert not _m2(Hz, Lx).any() and not _m2(Hx, Lz).any()
    # no nonzero combination of the logical rows is a stabiliser: stacking adds k to the rank
    assert _rank(np.vstack([Hx, Lx])) == rx + k
    assert _rank(np.vstack([Hz, Lz])) == rz + k
    assert np.array_equal(_m2(Lx, Lz), np.eye(k, dtype=np.int64))


def test_css_logicals_is_deterministic(monkeypatch):
    Hx, Hz = codes.load_code("LP04_0")
    a = logicals.css_logicals(Hx, Hz)
    monkeypatch.setattr(logicals, "_cache", {})           # a fresh computation, not the cached arrays
    b = logicals.css_logicals(Hx.copy(), Hz.copy())
    assert a[0] is not b[0]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert logicals.css_logicals(Hx, Hz)[0] is b[0]       # computed once per pair


def test_css_logicals_refusals_and_k0():
    Hx, Hz = codes.load_code("5qb")
    assert int(_m2(Hx, Hz).sum()) == 16
    with pytest.raises(ValueError, match="16"):
        logicals.css_logicals(Hx, Hz)
    with pytest.raises(ValueError, match="columns"):
        logicals.css_logicals(np.ones((1, 4), np.int8), np.ones((1, 6), np.int8))
    Lx, Lz = logicals.css_logicals(np.array([[1, 1]]), np.array([[1, 1]]))
    assert Lx.shape == (0, 2) and Lz.shape == (0, 2) and Lx.dtype == np.int8


def test_css_logicals_synthetic_n1500():
    Hx, Hz = lm_synthetic()
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    assert Lx.shape == (1498, 1500)
    assert not _m2(Hz, Lx).any() and not _m2(Hx, Lz).any()
    assert np.array_equal(_m2(Lx, Lz), np.eye(1498, dtype=np.int64))


def lm_synthetic():
    Hx = np.zeros((1, 1500), np.int8)
    Hz = np.zeros((1, 1500), np.int8)
    Hx[0, 0:4] = 1
    Hz[0, 2:6] = 1
    return Hx, Hz


@pytest.mark.parametrize("name", ["steane", "shor", "LP04_0"])
def test_count_logical_outcomes_equals_the_model(name):
    Hx, Hz = codes.load_code(name)
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    rng = np.random.default_rng(5)
    B = 800
    sy_z, sy_x, errX, errZ = simulator.sample_channel(Hx, Hz, 0.08, B, rng)
    eX, eZ, recX, recZ = lm.craft(rng, Hx, Hz, Lx, Lz, errX, errZ)
    itX = rng.integers(1, 50, B).astype(np.int32)
    itZ = rng.integers(1, 50, B).astype(np.int32)
    got, (cX, cZ, fX, fZ) = simulator.count_logical_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ,
                                                             want_shots=True)
    M = lm.Model(Hx, Hz)
    mX, mZ = M.classes(sy_z, sy_x, errX, errZ, eX, eZ)
    assert np.array_equal(cX, mX) and np.array_equal(cZ, mZ)
    assert got == M.counters(sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
    assert tuple(got) == simulator.COUNTER_KEYS + simulator.LOGICAL_KEYS
    assert {k: got[k] for k in simulator.COUNTER_KEYS} == \
        simulator.count_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
    assert fX.dtype == np.uint64 and fX.shape == (B, (Lz.shape[0] + 63) // 64)
    assert np.array_equal(fX, lm.flip_words(Lz, errX ^ eX)) and np.array_equal(fZ, lm.flip_words(Lx, errZ ^ eZ))
    # the recipes reach the classes they were built for
    for c, rec in ((mX, recX), (mZ, recZ)):
        assert (c[rec == 0] == 0).all() and (c[rec == 1] == 0).all() and (c[rec == 2] == 1).all()
        assert (c[rec == 3] == 2).mean() > 0.5
    lm.check_invariants(got, B)


class _R:
    def __init__(self, ehat, iters):
        self.ehat, self.iters = ehat, iters


@pytest.fixture
def oracle_decoder(monkeypatch):
    """simulate_p's host path decodes on the GPU; here the CPU oracle stands in."""
    from oracle import oracle

    def decode_batch(H, syn, p, max_iter, algo="MS", osd_order=-1, layer_ptr=None, layer_rows=None, **kw):
        e, it, _, _ = oracle.decode_batch(algo, H, np.asarray(syn), p, max_iter, layer_ptr, layer_rows)
        return _R(e, it)
    monkeypatch.setattr(simulator.decoders, "decode_batch", decode_batch)


def test_simulate_p_logical_on_and_off(oracle_decoder):
    Hx, Hz = codes.load_code("steane")
    shots = 3000
    smp = simulator.sample_channel(Hx, Hz, 0.06, shots, np.random.default_rng(2))
    kw = dict(shots=shots, decIterations=20, samples=smp, batch_size=1024, verbose=False)
    off = simulator.simulate_p(Hx, Hz, 0.06, **kw)
    assert set(off) == SIX
    assert set(simulator.simulate_p(Hx, Hz, 0.06, logical=False, **kw)) == SIX
    on = simulator.simulate_p(Hx, Hz, 0.06, logical=True, **kw)
    assert set(on) == SIX | set(simulator.LOGICAL_KEYS) | {"logical_error_rate", "logical_error_rate_ci95"}
    assert {k: on[k] for k in SIX} == off
    lm.check_invariants(on, shots)
    assert on["logicalErrors_X"] > 0 and on["decSuccessLogical"] > on["decSuccessExact"]
    assert on["logical_error_rate"] == 1. - on["decSuccessLogical"] / shots
    assert on["logical_error_rate_ci95"] == simulator.wilson_interval(shots - on["decSuccessLogical"], shots)
    # the model on the same decodes
    from oracle import oracle
    from qldpcsim_amd import schedule
    lx, lz = schedule.select_layers(Hx, Hz, "F")
    eX, itX, _, _ = oracle.decode_batch("MS", Hz, smp[0], 0.06 / 3, 20, *schedule.pack_layers(lx, Hz.shape[0]))
    eZ, itZ, _, _ = oracle.decode_batch("MS", Hx, smp[1], 0.06 / 3, 20, *schedule.pack_layers(lz, Hx.shape[0]))
    want = lm.Model(Hx, Hz).counters(smp[0], smp[1], smp[2], smp[3], eX, eZ, itX, itZ)
    assert {k: on[k] for k in simulator.LOGICAL_KEYS} == {k: want[k] for k in simulator.LOGICAL_KEYS}
    assert on["DecFailures_X"] == want["DecFailures_X"] and on["decSuccessExact"] == want["decSuccessExact"]


def test_simulate_p_logical_refuses_a_non_css_pair():
    Hx, Hz = codes.load_code("5qb")
    with pytest.raises(ValueError, match="CSS"):
        simulator.simulate_p(Hx, Hz, 0.05, shots=4, logical=True, sampler="host", verbose=False)


@pytest.mark.parametrize("x,n", [(0, 10), (10, 10), (3, 100), (1234, 98765), (1, 10 ** 9)])
def test_wilson_interval_closed_form(x, n):
    z = 1.959963984540054
    p = x / n
    centre = (p + z * z / (2 * n)) / (1 + z * z / n)
    half = z / (1 + z * z / n) * ((p * (1 - p) / n + z * z / (4 * n * n)) ** 0.5)
    lo, hi = simulator.wilson_interval(x, n)
    assert abs(lo - max(0.0, centre - half)) <= 1e-12 and abs(hi - min(1.0, centre + half)) <= 1e-12
    # the interval holds the point estimate (at x = 0 or n an end equals it up to rounding)
    assert 0.0 <= lo <= p + 1e-12 and p - 1e-12 <= hi <= 1.0


def test_cli_logical_prints_both_tables(tmp_path, capsys, oracle_decoder):
    Hx, Hz = codes.load_code("steane")
    np.save(tmp_path / "Hx.npy", Hx)
    np.save(tmp_path / "Hz.npy", Hz)
    res = tmp_path / "res.json"
    argv = ["--Hx", str(tmp_path / "Hx.npy"), "--Hz", str(tmp_path / "Hz.npy"), "--p", "0.05", "0.1", "--shots", "500",
            "--decIterations", "10", "--rngSeed", "3", "--sampler", "host", "--results", str(res)]
    simulator.main(argv + ["--logical"])
    out = capsys.readouterr().out
    assert out.count("SIMULATION RESULTS") == 1 and out.count("LOGICAL ERROR RATES") == 1
    assert out.index("SIMULATION RESULTS") < out.index("LOGICAL ERROR RATES")
    doc = json.loads(res.read_text())
    assert doc["meta"]["logical"] is True
    r = doc["results"]["0.05"]
    assert f"{r['logical_error_rate']:7.2e}" in out and f"{r['logicalErrors_X']:6},{r['logicalErrors_Z']:6}" in out
    # a results file written with the option is refused without it, and the other way round
    with pytest.raises(ValueError, match="different run"):
        simulator.main(argv)
    res.unlink()
    simulator.main(argv)
    out = capsys.readouterr().out
    assert out.count("SIMULATION RESULTS") == 1 and "LOGICAL" not in out
    doc = json.loads(res.read_text())
    assert "logical" not in doc["meta"] and set(doc["results"]["0.05"]) == SIX
    with pytest.raises(ValueError, match="different run"):
        simulator.main(argv + ["--logical"])


def test_capi_logical_argument_checks_need_no_device():
    """Every refusal of qldpc_logicals_create / qldpc_count_logical_ex comes
    before the first HIP call: the same codes with or without a device."""
    L, P, E = _lib.lib, _lib.ptr, _lib.QLDPC_EINVAL
    Hx, Hz = codes.load_code("steane")
    Sx, Sz = codes.load_code("shor")
    cx, cz, sx, sz = _lib.Code(Hx), _lib.Code(Hz), _lib.Code(Sx), _lib.Code(Sz)
    Lx, Lz = (np.ascontiguousarray(a, dtype=np.uint8) for a in logicals.css_logicals(Hx, Hz))

    def create(hx=cx.handle, hz=cz.handle, lx=Lx, lz=Lz, k=1, out=True):
        h = ctypes.c_void_p()
        rc = L.qldpc_logicals_create(hx, hz, P(lx), P(lz), k, ctypes.byref(h) if out else None)
        if rc == _lib.QLDPC_OK:
            L.qldpc_logicals_destroy(h)
        else:
            assert not h.value
        return rc

    assert create(hx=None) == E and create(hz=None) == E and create(out=False) == E
    assert create(hz=sz.handle) == E                          # 7 and 9 columns
    assert create(k=-1) == E and create(k=8) == E             # k <= n
    assert create(lx=None) == E and create(lz=None) == E
    big = _lib.Code(np.ones((1, 4097), np.uint8))
    assert create(hx=big.handle, hz=big.handle, k=0) == _lib.QLDPC_EUNSUP
    assert b"4096" in L.qldpc_last_error()
    assert L.qldpc_logicals_destroy(None) == _lib.QLDPC_OK
    if _lib.device_count() == 0:
        assert create() == _lib.QLDPC_OK and create(k=0, lx=None, lz=None) == _lib.QLDPC_OK

    lg = _lib.Logicals(cx, cz, Lx, Lz)
    other = _lib.Logicals(sx, sz, *logicals.css_logicals(Sx, Sz))
    B = 2
    W = np.zeros((B, 1), np.uint64)
    syn = np.zeros((B, 3), np.uint8)
    eh = np.zeros((B, 7), np.uint8)
    it = np.zeros(B, np.int32)
    acc = np.zeros(9, np.int64)

    def count(hx=cx.handle, hz=cz.handle, g=lg.handle, batch=B, ex=W, ez=W, s1=syn, s2=syn, sf=0, e1=eh, e2=eh,
              ef=0, i1=it, i2=it, a=acc):
        return L.qldpc_count_logical_ex(hx, hz, g, batch, P(ex), P(ez), P(s1), P(s2), sf, P(e1), P(e2), ef,
                                        P(i1), P(i2), P(a), None, None, None, None, None)

    assert count(hx=None) == E and count(hz=None) == E and count(g=None) == E
    assert count(g=other.handle) == E and b"another" in L.qldpc_last_error()
    assert count(hx=cz.handle, hz=cx.handle) == E            # the pair the other way round
    assert count(sf=2) == E and count(ef=-1) == E
    assert count(batch=-1) == E
    for name in ("ex", "ez", "s1", "s2", "e1", "e2", "i1", "i2", "a"):
        assert count(**{name: None}) == E, name
    assert b"null" in L.qldpc_last_error()
    assert count(batch=0, ex=None, a=None) == _lib.QLDPC_OK
    with _lib.options(logical_tabs=3):
        assert count() == E
    if _lib.device_count() == 0:                             # valid arguments reach the device check
        assert count() == _lib.QLDPC_EHIP
    assert acc.sum() == 0
    assert {"qldpc_logicals_create", "qldpc_logicals_destroy", "qldpc_count_logical_ex"} <= set(_lib.EXPORTS)

"""Phenomenological noise without a GPU: the space-time layout, the NumPy
twins in qldpcsim_amd.spacetime against the independent model
(tests/phenom_model.py), the model's Philox against the oracle's, and the
argument validation of the Python and C entry points."""
import ctypes
import functools

import numpy as np
import pytest

import phenom_model as pm

# the bundled halves, then four of tests/channel_shape_codes.py ("<case>_hz": Hz detects): the sampler's
# and the counter's <8>, <6>, <8> and <0> instances; q8a: m % 64 == 0 and (n + m) % 64 == 0, no padding bits
SHAPES = ("steane", "shor_x", "shor_z", "LP04_0", "q8a_hz", "q6v_hz", "q8b_hz", "g0v_hx")
# the row degree phenom_sample_kernel / phenom_count_kernel are instantiated on for each (0: the generic loop)
KERNEL_DEGREE = {"steane": 0, "shor_x": 0, "shor_z": 6, "LP04_0": 7, "q8a_hz": 8, "q6v_hz": 6, "q8b_hz": 8,
                 "g0v_hx": 0}


@functools.lru_cache(maxsize=None)
def half(name):
    """(H, L, Hstab, Lop) of one half: H detects the errors, L is the table the
    counter tests with, Hstab / Lop the stabilisers / logical operators of the
    errors' own type."""
    from qldpcsim_amd import codes, logicals
    import channel_shape_codes as csc
    if name.partition("_")[0] in csc.CASES:
        return csc.half(name)
    code, _, which = name.partition("_") if name.startswith("shor") else (name, "", "x")
    Hx, Hz = codes.load_code(code)
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    return (Hz, Lz, Hx, Lx) if which == "x" else (Hx, Lx, Hz, Lz)     # X half: Hz detects, Lz tests


@pytest.mark.parametrize("name", SHAPES)
def test_layout_of_the_spacetime_matrix(name):
    from qldpcsim_amd import spacetime
    H = half(name)[0]
    m, n = H.shape
    deg = (H % 2).sum(axis=1)
    assert np.array_equal(spacetime.spacetime_matrix(H, 1), H % 2)
    for T in (2, 3, 4):
        S = spacetime.spacetime_matrix(H, T)
        assert S.dtype == np.int8 and S.shape == (T * m, T * n + (T - 1) * m) == spacetime.spacetime_shape(n, m, T)
        assert np.array_equal(S, pm.dense_matrix(H, T))
        data = pm.is_data(n, m, T)
        for t in range(T - 1):
            for c in range(m):
                rows = np.flatnonzero(S[:, t * (n + m) + n + c])
                assert list(rows) == [t * m + c, (t + 1) * m + c]     # weight 2, adjacent rounds
        want = np.concatenate([deg + (1 if t in (0, T - 1) else 2) for t in range(T)])
        assert np.array_equal(S.sum(axis=1), want)
        pr = spacetime.spacetime_prior(n, m, T, 0.02, 0.005)
        assert pr.dtype == np.float64 and np.array_equal(pr, np.where(data, 0.02, 0.005))
        assert np.array_equal(spacetime.column_thresholds(n, m, T, 0.02, 0.005),
                              np.where(data, pm.threshold(0.02), pm.threshold(0.005)).astype(np.uint64))
        bits = np.random.default_rng(T).integers(0, 2, (9, S.shape[1]), dtype=np.uint8)
        assert np.array_equal(spacetime.fold_data(bits, n, m, T), pm.fold(bits, n, m, T))


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("T", (1, 2, 3))
def test_host_sampler_is_the_matrix_product(name, T):
    """H_st·fired mod 2 equals the host sampler's detectors on 200 random
    rows, E is the fold of the fired row and H·E equals XOR_t d_t."""
    from qldpcsim_amd import spacetime
    H = half(name)[0]
    m, n = H.shape
    det, E, fired = spacetime.sample_phenomenological(H, T, 0.2, 0.3, 200, np.random.default_rng(5), want_fired=True)
    assert det.shape == (200, T * m) and E.shape == (200, n) and fired.any() and not fired.all()
    assert np.array_equal(det, pm.mod2(fired, pm.dense_matrix(H, T)))
    assert np.array_equal(E, pm.fold(fired, n, m, T))
    x = np.zeros((200, m), np.uint8)
    for t in range(T):
        x ^= det[:, t * m:(t + 1) * m]
    assert np.array_equal(pm.mod2(E, H % 2), x)
    # the same rng gives the same shots without the fired rows; p = 0 fires nothing
    d2, E2 = spacetime.sample_phenomenological(H, T, 0.2, 0.3, 200, np.random.default_rng(5))
    assert np.array_equal(d2, det) and np.array_equal(E2, E)
    d0, E0, f0 = spacetime.sample_phenomenological(H, T, 0.0, 0.0, 20, np.random.default_rng(1), want_fired=True)
    assert not d0.any() and not E0.any() and not f0.any()


def test_model_philox_reproduces_the_oracle():
    """The model's NumPy Philox4x32-10 equals oracle_philox4x32_10 on 1000
    random (counter, key) pairs."""
    from oracle import oracle
    L = oracle.lib()
    rng = np.random.default_rng(99)
    ctr = rng.integers(0, 1 << 32, (1000, 4), dtype=np.uint64)
    key = rng.integers(0, 1 << 32, (1000, 2), dtype=np.uint64)
    got = pm.philox4x32_10(ctr, key)
    for i in range(1000):
        c = ctr[i].astype(np.uint32)
        L.oracle_philox4x32_10(c.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint32(int(key[i, 0])),
                               ctypes.c_uint32(int(key[i, 1])))
        assert [int(x) for x in c] == [int(x) for x in got[i]], i


def test_model_stream_at_one_round_is_the_channel_stream():
    """T = 1: the model's fired row equals oracle.channel_sample's errX (X | Y:
    u < T2) when p_data's threshold is T2, for shots across 2^32."""
    from oracle import oracle
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP04_0")
    p, seed, shot0 = 0.09, 0xDEADBEEF12345678, 2 ** 32 - 40
    assert pm.threshold(2 * p / 3) == oracle.channel_thresholds(p)[1]
    sy_z, _, errX, _ = oracle.channel_sample(Hx, Hz, p, seed, shot0, 90)
    det, E, fired = pm.sample(Hz, 1, 2 * p / 3, 0.5, seed, shot0, 90)
    assert errX.any()
    assert np.array_equal(fired, errX) and np.array_equal(E, errX) and np.array_equal(det, sy_z)


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("T", (1, 2, 3))
def test_host_counter_against_the_definition(name, T):
    """count_phenomenological on crafted estimates equals the dense
    brute-force classes, flips, residuals and counters; every crafted case
    occurs with its class."""
    from qldpcsim_amd import spacetime
    H, L, Hstab, Lop = half(name)
    B = 120
    det, E, fired = pm.sample(H, T, 0.08, 0.05, 3, 0, B)
    rng = np.random.default_rng(11)
    ehat, rec = pm.craft(rng, H, Hstab, Lop, T, fired)
    iters = rng.integers(1, 60, B).astype(np.int32)
    cls, F, r = pm.classify(H, L, T, det, E, ehat)
    for i, want in enumerate((0, 0, 0, 1, 2, 2)):
        hit = cls[rec == i]
        assert (T == 1 and i in (2, 5)) or hit.size >= 10, (i, hit.size)
        assert (hit == want).all(), (pm.RECIPES[i], hit)
    got, (gc, gf, gr) = spacetime.count_phenomenological(H, L, T, det, E, ehat, iters, want_shots=True)
    assert got == pm.counters(cls, iters)
    assert spacetime.count_phenomenological(H, L, T, det, E, ehat, iters) == got
    assert np.array_equal(gc, cls) and np.array_equal(gr, r) and np.array_equal(gf, pm.pack_words(F))
    assert gc.dtype == np.uint8 and gf.dtype == np.uint64 and gf.shape == (B, (L.shape[0] + 63) // 64)


def test_python_entry_points_refuse_bad_arguments():
    from qldpcsim_amd import codes, simulator, spacetime
    Hx, Hz = codes.load_code("steane")
    sim = simulator.simulate_phenomenological
    for kw in (dict(decType="RELAY"), dict(decType="NG"), dict(decType="BF"), dict(correlated="XZ"),
               dict(channel_weights=[1, 1, 1]), dict(decType="XX"), dict(decSchedule="Q"), dict(sampler="gpu")):
        with pytest.raises(ValueError):
            sim(Hx, Hz, 0.01, 0.01, 2, shots=4, verbose=False, **kw)
    for p, q, T in ((0.01, 0.01, 0), (0.01, 0.01, 1.5), (1.0, 0.01, 2), (0.01, -0.1, 2), (0.01, 1.0, 2)):
        with pytest.raises(ValueError):
            sim(Hx, Hz, p, q, T, shots=4, verbose=False)
    with pytest.raises(ValueError):                         # not a CSS pair
        sim(np.array([[1, 1, 0]], np.int8), np.array([[0, 1, 0]], np.int8), 0.01, 0.01, 2, shots=4, verbose=False)
    with pytest.raises(ValueError):
        spacetime.spacetime_matrix(Hz, 0)
    with pytest.raises(ValueError):
        spacetime.spacetime_prior(7, 3, 2, 1.0, 0.1)
    with pytest.raises(ValueError):
        spacetime.fold_data(np.zeros((2, 5), np.uint8), 7, 3, 2)


def test_c_entry_points_validate_before_any_hip_call():
    """rounds < 1, a probability outside [0, 1), an unknown format and a null
    argument give QLDPC_EINVAL (ValueError) with or without a device: every
    pointer here is a dummy the library must never touch."""
    from qldpcsim_amd import _lib, codes
    Hz = codes.load_code("steane")[1]
    code = _lib.Code(Hz)
    tab = _lib.PhenomTable(code, np.ones((1, 7), np.uint8))
    assert tab.k == 1 and tab.kw == 1
    X = 4096                                                # a non-null address that is never read
    ok = dict(rounds=2, p_data=0.1, q=0.1, seed=1, shot0=0, batch=4, det=X, det_fmt=_lib.FMT_BYTES, E=X)
    for bad in (dict(rounds=0), dict(rounds=-3), dict(p_data=1.0), dict(p_data=-0.1), dict(q=1.0),
                dict(q=float("nan")), dict(det=None), dict(E=None), dict(det_fmt=7), dict(batch=-1)):
        with pytest.raises(ValueError):
            _lib.phenom_sample(code, **{**ok, **bad})
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_phenom_sample(None, 2, 0.1, 0.1, 1, 0, 4, X, 0, X, None, None))
    okc = dict(rounds=2, batch=4, det=X, det_fmt=_lib.FMT_BITS, E=X, ehat=X, e_fmt=_lib.FMT_BITS, iters=X, acc=X)
    for bad in (dict(rounds=0), dict(det=None), dict(E=None), dict(ehat=None), dict(iters=None), dict(acc=None),
                dict(det_fmt=2), dict(e_fmt=-1), dict(batch=-1)):
        with pytest.raises(ValueError):
            _lib.phenom_count(code, tab, **{**okc, **bad})
    other = _lib.Code(np.eye(3, 7, dtype=np.uint8))
    with pytest.raises(ValueError, match="another code"):
        _lib.phenom_count(other, tab, **okc)
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_phenom_count(code.handle, None, 2, 4, X, 0, X, X, 0, X, X, None, None, None, None))
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_phenom_create(None, None, 0, ctypes.byref(ctypes.c_void_p())))
    with pytest.raises(ValueError):
        _lib.PhenomTable(code, np.ones((8, 7), np.uint8))    # k > n
    with pytest.raises(ValueError):
        _lib.PhenomTable(code, np.ones((1, 6), np.uint8))
    # past the kernels' tables: refused as unsupported, before any launch
    big = _lib.Code(np.ones((1, 4097), np.uint8))
    with pytest.raises(NotImplementedError):
        _lib.phenom_sample(big, **ok)
    assert _lib.lib.qldpc_phenom_destroy(None) == 0


def test_cli_rejects_meas_error_without_rounds(capsys):
    from qldpcsim_amd import simulator
    for argv in (["--meas-error", "0.01"], ["--rounds", "0"], ["--rounds", "2", "--logical"],
                 ["--rounds", "2", "--decType", "BF"], ["--rounds", "2", "--bias", "3"]):
        with pytest.raises(SystemExit) as e:
            simulator.main(["--Hx", "a.npy", "--Hz", "b.npy", "--p", "0.01"] + argv)
        assert e.value.code == 2
    assert "--meas-error needs --rounds" in capsys.readouterr().err


def test_results_metadata_separates_models(tmp_path, monkeypatch):
    """simulate(rounds=...) runs simulate_phenomenological with q defaulting
    to 2p/3 and records rounds and q: a results file of another model, round
    count or q is refused, and a code-capacity file refuses a rounds run."""
    import json
    from qldpcsim_amd import codes, simulator
    calls = []

    def fake(Hx, Hz, p, q, rounds, **kw):
        calls.append((p, q, rounds))
        return {"DecFailures_X": 0, "DecFailures_Z": 1, "logicalErrors_X": 2, "logicalErrors_Z": 3, "nIterAccX": 4,
                "nIterAccZ": 5, "decSuccessLogical": 90, "logical_error_rate": 0.1,
                "logical_error_rate_ci95": [0.05, 0.2], "logical_error_rate_per_round": 0.03, "rounds": rounds,
                "q": q, "p_data": 2 * p / 3}

    def fake_p(Hx, Hz, p, **kw):
        return {"DecFailures_X": 1, "DecFailures_Z": 2, "decSuccessExact": 90, "decSuccessDegen": 0,
                "Avg_number_of_iterations_X": 1.5, "Avg_number_of_iterations_Z": 1.5}

    monkeypatch.setattr(simulator, "simulate_phenomenological", fake)
    monkeypatch.setattr(simulator, "simulate_p", fake_p)
    Hx, Hz = codes.load_code("steane")
    np.save(tmp_path / "Hx.npy", Hx)
    np.save(tmp_path / "Hz.npy", Hz)
    fx, fz, f = str(tmp_path / "Hx.npy"), str(tmp_path / "Hz.npy"), str(tmp_path / "res.json")
    kw = dict(shots=100, rngSeed=1, verbose=False, return_results=True, resultsFile=f, sampler="host")
    a = simulator.simulate(fx, fz, [0.03], rounds=3, **kw)
    assert calls == [(0.03, 2 * 0.03 / 3, 3)] and a[0]["rounds"] == 3
    meta = json.load(open(f))["meta"]
    assert meta["rounds"] == 3 and meta["q"] is None
    assert simulator.simulate(fx, fz, [0.03], rounds=3, **kw) == a and len(calls) == 1     # resumed
    for other in (dict(rounds=4), dict(rounds=3, meas_error=0.01), dict()):
        with pytest.raises(ValueError, match="different run"):
            simulator.simulate(fx, fz, [0.03], **other, **kw)
    g = str(tmp_path / "cc.json")
    simulator.simulate(fx, fz, [0.03], **{**kw, "resultsFile": g})
    with pytest.raises(ValueError, match="different run"):
        simulator.simulate(fx, fz, [0.03], rounds=3, **{**kw, "resultsFile": g})
    b = simulator.simulate(fx, fz, [0.03], rounds=2, meas_error=0.01, **{**kw, "resultsFile": None})
    assert calls[-1] == (0.03, 0.01, 2) and b[0]["q"] == 0.01
    with pytest.raises(ValueError):
        simulator.simulate(fx, fz, [0.03], meas_error=0.01, **kw)
    with pytest.raises(ValueError):
        simulator.simulate(fx, fz, [0.03], rounds=2, logical=True, **kw)


def test_results_table_of_the_mode():
    from qldpcsim_amd import simulator
    r = {"DecFailures_X": 3, "DecFailures_Z": 4, "logicalErrors_X": 5, "logicalErrors_Z": 6, "decSuccessLogical": 900,
         "logical_error_rate": 0.1, "logical_error_rate_ci95": [0.08, 0.12], "logical_error_rate_per_round": 0.0345,
         "rounds": 3, "q": 0.02}
    txt = simulator.format_phenomenological_results([0.03], [r], 1000)
    assert "PHENOMENOLOGICAL" in txt and "3.00e-02" in txt and "2.00e-02" in txt and "1.00e-01" in txt
    assert "3.45e-02" in txt and "     3,     4" in txt and "     5,     6" in txt

"""Sliding-window decoding without a GPU: the window matrices and the schedule,
the properties of spacetime.window_advance (the NumPy twin of
phenom_window_kernel) that make the assembled estimate a space-time estimate,
and the argument validation of the Python, C and command-line entry points.
Every comparison is integer equality."""
import numpy as np
import pytest

import phenom_model as pm
from test_phenom_model import SHAPES, half

# (T, W, F): open windows with F < W, F = W, a closed window shorter than W, one window only
SCHEDULES = ((5, 3, 1), (6, 2, 2), (7, 4, 2), (4, 3, 3), (3, 3, 1))
B = 40
P_DATA, Q = 0.08, 0.06


def gf2_solve(A, S):
    """Rows x with A x = s for every row s of S (A [r, c], S [B, r], 0/1), by
    Gaussian elimination of [A | S^T]; asserts that every system is consistent."""
    A = (np.asarray(A) % 2).astype(np.uint8)
    r, c = A.shape
    M = np.concatenate([A, np.asarray(S, np.uint8).T], axis=1)
    piv, row = [], 0
    for col in range(c):
        hit = np.flatnonzero(M[row:, col])
        if hit.size == 0:
            continue
        M[[row, row + hit[0]]] = M[[row + hit[0], row]]
        others = np.flatnonzero(M[:, col])
        others = others[others != row]
        M[others] ^= M[row]
        piv.append(col)
        row += 1
        if row == r:
            break
    assert not M[row:, c:].any(), "inconsistent system"
    X = np.zeros((S.shape[0], c), np.uint8)
    X[:, piv] = M[:len(piv), c:].T
    return X


def _window_H(H, R, closed):
    from qldpcsim_amd import spacetime
    return spacetime.spacetime_matrix(H, R) if closed else spacetime.window_matrix(H, R)


def _run(H, T, W, F, det, estimate):
    """The schedule's loop with estimate(window, Hw, syn) -> west as the
    decoder. Returns (ehat, iters_total, the iteration counts fed)."""
    from qldpcsim_amd import spacetime
    m, n = H.shape
    nb = det.shape[0]
    ehat = np.full((nb, spacetime.spacetime_shape(n, m, T)[1]), 7, np.uint8)   # every column must be written
    total = np.zeros(nb, np.int32)
    fed = np.zeros(nb, np.int64)
    last = west = wit = None
    for k, w in enumerate(spacetime.window_schedule(T, W, F)):
        syn = spacetime.window_advance(n, m, T, det, ehat, total, last, west, wit, w)
        assert syn.shape == (nb, w[1] * m) and syn.dtype == np.uint8
        if last is None:
            assert np.array_equal(syn, det[:, :w[1] * m])
        west = estimate(w, _window_H(H, w[1], w[2]), syn)
        assert np.array_equal(pm.mod2(west, _window_H(H, w[1], w[2])), syn), "the estimate reproduces its syndrome"
        wit = np.arange(nb, dtype=np.int32) + 3 * k + 1
        fed += wit
        last = w
    assert spacetime.window_advance(n, m, T, det, ehat, total, last, west, wit, None) is None
    return ehat, total, fed


@pytest.mark.parametrize("name", SHAPES)
def test_window_matrix_is_the_slice_of_the_spacetime_matrix(name):
    from qldpcsim_amd import spacetime
    H = half(name)[0]
    m, n = H.shape
    for W in (1, 2, 3):
        A = spacetime.window_matrix(H, W)
        assert A.dtype == np.int8 and A.shape == (W * m, W * (n + m)) == spacetime.window_shape(n, m, W, False)
        assert np.array_equal(A, spacetime.spacetime_matrix(H, W + 1)[:W * m, :W * (n + m)])
        assert np.array_equal(A, pm.dense_matrix(H, W + 1)[:W * m, :W * (n + m)])
        last = A[:, (W - 1) * (n + m) + n:]
        assert (last.sum(axis=0) == 1).all() and np.array_equal(last[(W - 1) * m:], np.eye(m, dtype=np.int8))
        pr = spacetime.window_prior(n, m, W, 0.25, 0.125)
        assert np.array_equal(pr, spacetime.spacetime_prior(n, m, W + 1, 0.25, 0.125)[:W * (n + m)])
        assert spacetime.window_shape(n, m, W, True) == spacetime.spacetime_shape(n, m, W)


def test_window_schedule_tiles_the_columns():
    """All T <= 9 and 1 <= F <= W <= 4: window k starts at k F, the committed
    column ranges tile [0, N) exactly once, T <= W is one closed window of T
    rounds, only the last window is closed and it ends at T."""
    from qldpcsim_amd import spacetime
    n, m = 7, 3
    for T in range(1, 10):
        N = spacetime.spacetime_shape(n, m, T)[1]
        for W in range(1, 5):
            for F in range(1, W + 1):
                ws = spacetime.window_schedule(T, W, F)
                if T <= W:
                    assert ws == [(0, T, True, T)]
                seen = np.zeros(N, np.int64)
                for k, (a, R, closed, C) in enumerate(ws):
                    assert a == k * F and closed == (k == len(ws) - 1) == (a + W >= T)
                    assert (R, C) == ((T - a, T - a) if closed else (W, F)) and a + R <= T
                    k_cols = spacetime.window_shape(n, m, R, True)[1] if closed else C * (n + m)
                    seen[a * (n + m):a * (n + m) + k_cols] += 1
                assert (seen == 1).all(), (T, W, F)
                assert len({(R, closed) for _, R, closed, _ in ws}) <= 2


@pytest.mark.parametrize("T,W,F", SCHEDULES)
@pytest.mark.parametrize("name", SHAPES)
def test_true_window_errors_reassemble_the_fired_row(name, T, W, F):
    """Each window is fed the fired columns of its rounds (an open window's
    last measurement columns included): every corrected window syndrome is
    the window matrix times them, the assembled estimate is the fired row and
    every shot is class 0."""
    from qldpcsim_amd import spacetime
    H, L = half(name)[:2]
    m, n = H.shape
    det, E, fired = spacetime.sample_phenomenological(H, T, P_DATA, Q, B, np.random.default_rng(11), want_fired=True)
    assert fired.any() and det.any()

    def truth(w, Hw, syn):
        a = w[0] * (n + m)
        return fired[:, a:a + Hw.shape[1]]

    ehat, total, fed = _run(H, T, W, F, det, truth)
    assert np.array_equal(ehat, fired)
    assert np.array_equal(total, fed)
    assert (pm.classify(H, L, T, det, E, ehat)[0] == 0).all()
    c = spacetime.count_phenomenological(H, L, T, det, E, ehat, total)
    assert c["successes"] == B and c["iterations"] == int(fed.sum())


@pytest.mark.parametrize("T,W,F", SCHEDULES)
@pytest.mark.parametrize("name", SHAPES)
def test_any_window_estimates_telescope_to_the_detectors(name, T, W, F):
    """Each window is fed some estimate that reproduces its corrected
    syndrome, unrelated to the true errors: random data columns completed by
    the measurement columns (an open window has an identity block in every
    round) or, in the closed window, a GF(2) solution. The assembled estimate
    then reproduces the original detectors, H_st ehat = d, for every shot."""
    from qldpcsim_amd import spacetime
    H = half(name)[0]
    m, n = H.shape
    det = spacetime.sample_phenomenological(H, T, P_DATA, Q, B, np.random.default_rng(12))[0]
    rng = np.random.default_rng(13)

    def some(w, Hw, syn):
        R, closed = w[1], w[2]
        if closed:
            return gf2_solve(Hw, syn)                          # consistent by construction: skips no shot
        x = np.zeros((B, Hw.shape[1]), np.uint8)
        u = np.zeros((B, m), np.uint8)
        for t in range(R):
            o = t * (n + m)
            x[:, o:o + n] = rng.integers(0, 2, (B, n), dtype=np.uint8)
            u = syn[:, t * m:(t + 1) * m] ^ pm.mod2(x[:, o:o + n], H) ^ u
            x[:, o + n:o + n + m] = u
        return x

    ehat, total, fed = _run(H, T, W, F, det, some)
    assert ehat.max() <= 1
    assert np.array_equal(pm.mod2(ehat, pm.dense_matrix(H, T)), det)
    assert np.array_equal(spacetime.detectors(H, T, ehat), det)
    assert np.array_equal(total, fed)


def test_window_advance_leaves_other_columns_and_refuses_bad_windows():
    from qldpcsim_amd import spacetime
    n, m, T = 7, 3, 5
    rng = np.random.default_rng(3)
    det = rng.integers(0, 2, (4, T * m), dtype=np.uint8)
    ehat = rng.integers(0, 2, (4, spacetime.spacetime_shape(n, m, T)[1]), dtype=np.uint8)
    west = rng.integers(0, 2, (4, 2 * (n + m)), dtype=np.uint8)
    before = ehat.copy()
    total = np.full(4, 5, np.int32)
    syn = spacetime.window_advance(n, m, T, det, ehat, total, (1, 2, False, 1), west, np.array([1, 2, 3, 4]), (2, 2))
    assert np.array_equal(ehat[:, 10:20], west[:, :10])
    assert np.array_equal(ehat[:, :10], before[:, :10]) and np.array_equal(ehat[:, 20:], before[:, 20:])
    assert total.tolist() == [6, 7, 8, 9] and total.dtype == np.int32
    want = det[:, 6:12].copy()
    want[:, :3] ^= west[:, 7:10]
    assert np.array_equal(syn, want)
    for done, nxt in (((4, 2, False, 1), None), ((3, 2, False, 1), None), ((1, 2, False, 3), None),
                      ((1, 2, True, 2), None),
                      ((1, 2, False, 1), (3, 2)), (None, (4, 2)), ((3, 2, True, 2), (4, 1))):
        with pytest.raises(ValueError):
            spacetime.window_advance(n, m, T, det, ehat, total, done, west[:, :17] if done and done[2] else west,
                                     np.zeros(4, np.int32), nxt)


BAD_WINDOWS = (dict(window=0), dict(window=-2), dict(window=2.0), dict(window=2.5), dict(window="3"),
               dict(window=3, commit=0), dict(window=3, commit=4), dict(window=3, commit=1.0), dict(commit=1))


def test_python_entry_points_refuse_bad_windows(tmp_path):
    from qldpcsim_amd import codes, simulator, spacetime
    Hx, Hz = codes.load_code("steane")
    for kw in BAD_WINDOWS:
        with pytest.raises(ValueError):
            simulator.simulate_phenomenological(Hx, Hz, 0.01, 0.01, 4, shots=4, verbose=False, **kw)
    np.save(tmp_path / "Hx.npy", Hx)
    np.save(tmp_path / "Hz.npy", Hz)
    fx, fz = str(tmp_path / "Hx.npy"), str(tmp_path / "Hz.npy")
    for kw in BAD_WINDOWS:
        with pytest.raises(ValueError):
            simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, rounds=4, **kw)
    for kw in (dict(window=2), dict(window=2, commit=1), dict(commit=1)):       # window without rounds
        with pytest.raises(ValueError, match="need rounds"):
            simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, **kw)
    for args in ((5, 0), (5, 2, 3), (5, 2, 0), (5, 2.0), (0, 2)):
        with pytest.raises(ValueError):
            spacetime.window_schedule(*args)
    with pytest.raises(ValueError):
        spacetime.window_matrix(Hz, 0)


def test_cli_rejects_bad_windows(capsys):
    from qldpcsim_amd import simulator
    for argv, msg in ((["--window", "3"], "--window needs --rounds"),
                      (["--rounds", "5", "--commit", "1"], "--commit needs --window"),
                      (["--rounds", "5", "--window", "0"], "--window must be >= 1"),
                      (["--rounds", "5", "--window", "3", "--commit", "4"], "--commit must lie in"),
                      (["--rounds", "5", "--window", "3", "--commit", "0"], "--commit must lie in"),
                      (["--rounds", "5", "--window", "2.5"], "invalid int value")):
        with pytest.raises(SystemExit) as e:
            simulator.main(["--Hx", "a.npy", "--Hz", "b.npy", "--p", "0.01"] + argv)
        assert e.value.code == 2
        assert msg in capsys.readouterr().err


def test_c_entry_point_validates_before_any_hip_call():
    """A window outside [0, T), C > R, a closed window that is not the last, a
    next window that does not follow, an unknown format, a null buffer and a
    negative batch give QLDPC_EINVAL (ValueError) with or without a device:
    every pointer here is a dummy the library must never touch."""
    from qldpcsim_amd import _lib, codes
    code = _lib.Code(codes.load_code("steane")[1])
    X = 4096
    ok = dict(rounds=5, batch=4, done=(1, 2, False, 1), west=X, w_fmt=_lib.FMT_BITS, witers=X, ehat=X,
              e_fmt=_lib.FMT_BYTES, iters=X, nxt=(2, 3), det=X, det_fmt=_lib.FMT_BITS, syn=X, syn_fmt=_lib.FMT_BYTES)
    for bad in (dict(rounds=0), dict(batch=-1), dict(done=(4, 2, False, 1), nxt=None),
                dict(done=(3, 2, False, 1), nxt=None),
                dict(done=(-1, 2, False, 1)),
                dict(done=(1, 2, False, 3)), dict(done=(1, 2, False, 0)), dict(done=(1, 2, True, 2), nxt=None),
                dict(done=(3, 2, True, 1), nxt=None), dict(done=(3, 2, True, 2), nxt=(4, 1)), dict(nxt=(3, 2)),
                dict(nxt=(2, 4)), dict(done=None, nxt=None), dict(w_fmt=2), dict(e_fmt=-1), dict(det_fmt=7),
                dict(syn_fmt=3), dict(west=None), dict(witers=None), dict(ehat=None), dict(iters=None),
                dict(det=None), dict(syn=None)):
        with pytest.raises(ValueError):
            _lib.phenom_window(code, **{**ok, **bad})
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_phenom_window(None, 5, 4, 1, 2, 0, 1, X, 0, X, X, 0, X, 2, 3, X, 0, X, 0, None))
    big = _lib.Code(np.ones((1, 4097), np.uint8))
    with pytest.raises(NotImplementedError):
        _lib.phenom_window(big, **ok)


def test_results_table_and_metadata_carry_the_window(tmp_path, monkeypatch):
    """simulate(rounds=, window=, commit=) passes both on, records them in the
    results file's meta (another window or commit is a different run, and so is
    none) and the table shows W/F; without window= meta and table are as
    before."""
    import json
    from qldpcsim_amd import codes, simulator
    calls = []

    def fake(Hx, Hz, p, q, rounds, **kw):
        calls.append((kw.get("window"), kw.get("commit")))
        r = {"DecFailures_X": 0, "DecFailures_Z": 1, "logicalErrors_X": 2, "logicalErrors_Z": 3, "nIterAccX": 4,
             "nIterAccZ": 5, "decSuccessLogical": 90, "logical_error_rate": 0.1, "logical_error_rate_ci95": [0.05, 0.2],
             "logical_error_rate_per_round": 0.03, "rounds": rounds, "q": q, "p_data": 2 * p / 3}
        if kw.get("window") is not None:
            r.update(window=kw["window"], commit=kw.get("commit") or 1, windows=3)
        return r

    monkeypatch.setattr(simulator, "simulate_phenomenological", fake)
    Hx, Hz = codes.load_code("steane")
    np.save(tmp_path / "Hx.npy", Hx)
    np.save(tmp_path / "Hz.npy", Hz)
    fx, fz, f = str(tmp_path / "Hx.npy"), str(tmp_path / "Hz.npy"), str(tmp_path / "res.json")
    kw = dict(shots=100, rngSeed=1, verbose=False, return_results=True, resultsFile=f, sampler="host", rounds=6)
    a = simulator.simulate(fx, fz, [0.03], window=3, **kw)
    assert calls == [(3, 1)] and (a[0]["window"], a[0]["commit"]) == (3, 1)
    meta = json.load(open(f))["meta"]
    assert (meta["window"], meta["commit"], meta["rounds"]) == (3, 1, 6)
    assert simulator.simulate(fx, fz, [0.03], window=3, commit=1, **kw) == a and len(calls) == 1     # resumed
    for other in (dict(window=4), dict(window=3, commit=2), dict()):
        with pytest.raises(ValueError, match="different run"):
            simulator.simulate(fx, fz, [0.03], **other, **kw)
    g = str(tmp_path / "whole.json")
    simulator.simulate(fx, fz, [0.03], **{**kw, "resultsFile": g})
    assert "window" not in json.load(open(g))["meta"] and calls[-1] == (None, None)
    table = simulator.format_phenomenological_results([0.03], a, 100)
    assert "Window W/F" in table and "  3/1" in table
    plain = simulator.format_phenomenological_results([0.03], [{k: v for k, v in a[0].items()
                                                               if k not in ("window", "commit", "windows")}], 100)
    assert "Window" not in plain and plain.count("\n") == table.count("\n")

"""Detector error models without a GPU: the .dem reader and writer, the merge
rule, the phenomenological model, the NumPy twins in qldpcsim_amd.dem against
the independent model (tests/dem_model.py), and the argument validation of
simulate_dem, the command line and the C entry points."""
import ctypes
import json

import numpy as np
import pytest

import dem_model as dm
import phenom_model as pm
from test_phenom_model import half


def _cols(d):
    """[(p, detectors, observables)] of a Dem, column by column."""
    return [(float(d.priors[j]), tuple(np.flatnonzero(d.H[:, j])), tuple(np.flatnonzero(d.L[:, j])))
            for j in range(d.num_errors)]


# ---------------------------------------------------------------------------
# the reader
# ---------------------------------------------------------------------------
def test_every_instruction():
    from qldpcsim_amd import dem as D
    d = D.parse_dem("""
        # a comment line
        error(0.125) D0 D2 L1      # and a trailing one
        error(0.25) D1 ^ D3 L0     # the separator means nothing here

        detector(1.5, 2, 0) D4
        detector D1
        logical_observable L2
        shift_detectors(0, 0, 1) 3
        error(0.5) D0 D1           # absolute D3 D4
        shift_detectors 1
        error(0.0625) D0           # absolute D4
    """)
    assert d.H.shape == (5, 4) and d.L.shape == (3, 4) and d.H.dtype == np.uint8 and d.priors.dtype == np.float64
    assert _cols(d) == [(0.125, (0, 2), (1,)), (0.25, (1, 3), (0,)), (0.5, (3, 4), ()), (0.0625, (4,), ())]
    assert (d.num_detectors, d.num_observables, d.num_errors) == (5, 3, 4)


def test_nested_repeat_carries_the_detector_shift():
    """repeat 2 { repeat 3 { error D0 D1; shift 1 }; error D0 L0; shift 10 }:
    the inner body runs at shifts 0, 1, 2 and 13, 14, 15, the outer error at 3
    and 16; merging leaves them apart (all the sets differ)."""
    from qldpcsim_amd import dem as D
    text = """repeat 2 {
        repeat 3 {
            error(0.01) D0 D1
            shift_detectors 1
        }
        error(0.02) D0 L0
        shift_detectors(0, 1) 10
    }
    error(0.03) D0
    """
    d = D.parse_dem(text)
    want = [(0.01, (s, s + 1), ()) for s in (0, 1, 2)] + [(0.02, (3,), (0,))] + \
           [(0.01, (s, s + 1), ()) for s in (13, 14, 15)] + [(0.02, (16,), (0,))] + [(0.03, (26,), ())]
    assert _cols(d) == want and d.H.shape == (27, 9) and d.L.shape == (1, 9)
    assert D.parse_dem("repeat 0 {\n error(0.1) D5\n}\nerror(0.1) D1").H.shape == (2, 1)


def test_a_doubled_target_cancels():
    from qldpcsim_amd import dem as D
    d = D.parse_dem("error(0.1) D0 D1 ^ D1 D2 L0 L0\nerror(0.2) D3 D3 D3 L1 ^ L1 L1")
    assert _cols(d) == [(0.1, (0, 2), ()), (0.2, (3,), (1,))]
    assert d.L.shape == (2, 2)                      # a cancelled observable still counts for K


def test_declarations_raise_the_counts_and_k_may_be_zero():
    from qldpcsim_amd import dem as D
    d = D.parse_dem("error(0.1) D0\ndetector(0, 0) D7\nshift_detectors 2\ndetector D9")
    assert d.H.shape == (12, 1) and d.L.shape == (0, 1) and d.num_observables == 0
    assert not d.H[1:].any()
    d = D.parse_dem("error(0.1) D0 L0\nlogical_observable L4")
    assert d.L.shape == (5, 1)
    empty = D.parse_dem("# nothing\n\n")
    assert empty.H.shape == (0, 0) and empty.L.shape == (0, 0) and empty.priors.shape == (0,)


def test_tags_and_comments_are_ignored():
    from qldpcsim_amd import dem as D
    a = D.parse_dem("error[gate:CX q0 q1](0.1) D0 D1 L0\ndetector[x](1, 2) D2\nlogical_observable[obs] L1\n"
                    "shift_detectors[t](1) 1\nerror[] (0.2) D0 # D5 L3\n")
    b = D.parse_dem("error(0.1) D0 D1 L0\ndetector(1, 2) D2\nlogical_observable L1\nshift_detectors(1) 1\n"
                    "error(0.2) D0\n")
    assert a == b and _cols(a) == [(0.1, (0, 1), (0,)), (0.2, (1,), ())] and a.L.shape == (2, 2)


@pytest.mark.parametrize("text,line", [
    ("error(0.1) D0\nfoo(0.1) D0", 2),                          # unknown instruction
    ("\n\nerror(0.1) D0 X3", 3),                                # malformed targets
    ("error(0.1) D", 1), ("error(0.1) D-1", 1), ("error(0.1) 5", 1), ("error(0.1) D1.5", 1),
    ("# c\ndetector L0", 2), ("logical_observable D0", 1), ("detector D0 ^ D1", 1),
    ("error(1.0) D0", 1), ("error(-0.1) D0", 1), ("error(nan) D0", 1), ("error(1.5) D0", 1),   # p outside [0, 1)
    ("error D0", 1), ("error(0.1, 0.2) D0", 1), ("error(x) D0", 1),
    ("error(0.1) D0\nrepeat x {\n}", 2), ("repeat 2\nerror(0.1) D0\n}", 1), ("error(0.1) D0\n}", 2),
    ("repeat 2 {\nerror(0.1) D0", 1), ("repeat 2 {\nrepeat 3 {\nerror(0.1) D0\n}", 1),
    ("shift_detectors D1", 1), ("shift_detectors 1 2", 1), ("error(0.1) D0 {", 1),
])
def test_error_paths_name_the_line(text, line):
    from qldpcsim_amd import dem as D
    with pytest.raises(ValueError, match=rf"^line {line}:"):
        D.parse_dem(text)


# ---------------------------------------------------------------------------
# merge, the writer, files
# ---------------------------------------------------------------------------
def test_merge_rule():
    """Identical (detector set, observable set): one column at the first
    one's place, p <- p1 (1 - p2) + p2 (1 - p1), applied in order. Columns
    that differ only in observables stay apart; columns without a detector
    stay (and merge among themselves like any other)."""
    from qldpcsim_amd import dem as D
    text = """error(0.1) D0 D1
              error(0.2) D2 L0
              error(0.3) D1 D0 D2 D2
              error(0.05) D2
              error(0.4) L0
              error(0.25) D0 D1
              error(0.125) L0 ^ L1 L1
              error(0.5) L1
              error(0.01)
    """
    d = D.parse_dem(text)
    p01 = 0.1 * (1 - 0.3) + 0.3 * (1 - 0.1)
    p01 = p01 * (1 - 0.25) + 0.25 * (1 - p01)
    pl0 = 0.4 * (1 - 0.125) + 0.125 * (1 - 0.4)
    assert _cols(d) == [(p01, (0, 1), ()), (0.2, (2,), (0,)), (0.05, (2,), ()), (pl0, (), (0,)), (0.5, (), (1,)),
                        (0.01, (), ())]
    raw = D.parse_dem(text, merge=False)
    assert raw.num_errors == 9 and [c[0] for c in _cols(raw)] == [0.1, 0.2, 0.3, 0.05, 0.4, 0.25, 0.125, 0.5, 0.01]
    assert _cols(raw)[2][1:] == ((0, 1), ()) and _cols(raw)[6][1:] == ((), (0,))
    assert raw.H.shape[0] == d.H.shape[0] == 3 and raw.L.shape[0] == d.L.shape[0] == 2


@pytest.mark.parametrize("shape", dm.EDGE_SHAPES)
def test_text_round_trip(shape):
    """parse_dem(dem_text(d), merge=False) == d, exactly: the %.17g
    probabilities, the empty last row (a declaration), the all-zero and
    observable-only columns, the identical columns kept apart."""
    from qldpcsim_amd import dem as D
    H, L, pr, where = dm.edge_dem(*shape)
    d = D.Dem(H, L, pr)
    text = D.dem_text(d)
    assert text.count("error(") == shape[2]
    back = D.parse_dem(text, merge=False)
    assert back == d and back.H.shape == H.shape and back.L.shape == L.shape
    assert np.array_equal(back.priors.view(np.uint64), pr.view(np.uint64))
    if "twin" in where:
        assert D.parse_dem(text).num_errors < shape[2]          # merging joins the identical pair


def test_files(tmp_path):
    from qldpcsim_amd import dem as D
    H, L, pr, _ = dm.edge_dem(65, 65, 129)
    d = D.Dem(H, L, pr)
    np.savez(tmp_path / "m.npz", H=H, L=L, priors=pr)
    assert D.load_dem(str(tmp_path / "m.npz")) == d and D.load_dem(tmp_path / "m.npz") == d
    (tmp_path / "m.dem").write_text(D.dem_text(d))
    assert D.load_dem(str(tmp_path / "m.dem"), merge=False) == d
    assert D.load_dem(str(tmp_path / "m.dem")) == D.parse_dem(D.dem_text(d))
    np.savez(tmp_path / "bad.npz", H=H, L=L)
    with pytest.raises(ValueError, match="priors"):
        D.load_dem(str(tmp_path / "bad.npz"))
    np.savez(tmp_path / "bad2.npz", H=H, L=L, priors=pr[:-1])
    with pytest.raises(ValueError):
        D.load_dem(str(tmp_path / "bad2.npz"))


def test_dem_refuses_bad_arrays():
    from qldpcsim_amd import dem as D
    H, L, pr = np.eye(3, 4, dtype=np.uint8), np.ones((2, 4), np.uint8), np.full(4, 0.1)
    assert D.Dem(H, L, pr).uniform_prior() == 0.1 and D.Dem(H, [], pr).L.shape == (0, 4)
    assert D.Dem(H, L, [0.1, 0.2, 0.1, 0.1]).uniform_prior() is None
    for bad in ((H[0], L, pr), (H, L[:, :3], pr), (H, L, pr[:3]), (H, L[0], pr), (H * 2, L, pr), (H, L * 3, pr),
                (H.astype(float) + 0.5, L, pr), (H, L, [0.1, 0.2, 1.0, 0.1]), (H, L, [0.1, -0.2, 0.1, 0.1]),
                (H, L, [0.1, np.nan, 0.1, 0.1]), (H, L, pr.reshape(2, 2)), (H, np.zeros((0, 3)), pr)):
        with pytest.raises(ValueError):
            D.Dem(*bad)
    assert np.array_equal(D.Dem(H, L, [0.0, 0.5, 1 - 2.0 ** -20, 1e-12]).thresholds(),
                          np.array([0, 2 ** 31, 2 ** 32 - 4096, 0], np.uint64))


# ---------------------------------------------------------------------------
# the phenomenological model is a DEM
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("T", (1, 2, 3))
@pytest.mark.parametrize("name", ("steane", "shor_x", "shor_z", "LP04_0"))
def test_phenomenological_dem(name, T):
    from qldpcsim_amd import dem as D, spacetime
    H, L = half(name)[:2]
    m, n = H.shape
    d = D.phenomenological_dem(H, L, T, 0.02, 0.005)
    assert np.array_equal(d.H, spacetime.spacetime_matrix(H, T)) and np.array_equal(d.H, pm.dense_matrix(H, T))
    assert np.array_equal(d.priors, spacetime.spacetime_prior(n, m, T, 0.02, 0.005))
    assert np.array_equal(d.thresholds(), spacetime.column_thresholds(n, m, T, 0.02, 0.005))
    data = pm.is_data(n, m, T)
    assert d.L.shape == (L.shape[0], d.H.shape[1]) and not d.L[:, ~data].any()
    for t in range(T):
        assert np.array_equal(d.L[:, t * (n + m):t * (n + m) + n], L % 2)
    e = np.random.default_rng(T).integers(0, 2, (40, d.num_errors), dtype=np.uint8)
    assert np.array_equal(pm.mod2(e, d.L), pm.mod2(spacetime.fold_data(e, n, m, T), L % 2))
    assert (d.uniform_prior() is None) == (T > 1)
    assert D.phenomenological_dem(H, L, T, 0.02, 0.02).uniform_prior() == 0.02


# ---------------------------------------------------------------------------
# the NumPy twins against the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dm.EDGE_SHAPES)
def test_host_twins_against_the_model(shape):
    """sample_dem on a generator equals the model's product of the same draws;
    count_dem on crafted estimates equals the brute-force classes, flips and
    counters, and every class that the shape allows occurs."""
    from qldpcsim_amd import dem as D
    H, L, pr, where = dm.edge_dem(*shape)
    d = D.Dem(H, L, pr)
    B = 120
    det, obs, fired = D.sample_dem(d, B, np.random.default_rng(5), want_fired=True)
    u = np.random.default_rng(5).integers(0, 1 << 32, (B, shape[2]), dtype=np.uint64)
    assert np.array_equal(fired, (u < dm.thresholds(pr)).astype(np.uint8)) and fired.any()
    assert np.array_equal(det, dm._prod(fired, H)) and np.array_equal(obs, dm._prod(fired, L))
    assert det.shape == (B, shape[0]) and obs.shape == (B, shape[1]) and det.dtype == np.uint8
    d2, o2 = D.sample_dem(d, B, np.random.default_rng(5))
    assert np.array_equal(d2, det) and np.array_equal(o2, obs)
    rng = np.random.default_rng(11)
    ehat, want = dm.craft(rng, H, L, fired, where)
    iters = rng.integers(1, 60, B).astype(np.int32)
    cls, F = dm.classify(H, L, det, obs, ehat)
    assert np.array_equal(cls, want)
    assert set(cls) == ({0, 1, 2} if (shape[1] and shape[2] >= 64) else {0, 2})
    got, (gc, gf) = D.count_dem(d, det, obs, ehat, iters, want_shots=True)
    assert got == dm.counters(cls, iters) and D.count_dem(d, det, obs, ehat, iters) == got
    assert np.array_equal(gc, cls) and np.array_equal(gf, pm.pack_words(F))
    assert gc.dtype == np.uint8 and gf.dtype == np.uint64 and gf.shape == (B, (shape[1] + 63) // 64)


def test_model_stream_on_a_phenomenological_dem_is_the_phenomenological_stream():
    """The model's DEM sampler on the phenomenological model of LP04_0 (T = 3)
    gives phenom_model's detectors and fired row, and obs = L E."""
    from qldpcsim_amd import dem as D
    H, L = half("LP04_0")[:2]
    d = D.phenomenological_dem(H, L, 3, 0.05, 0.03)
    seed, shot0 = 0xDEADBEEF12345678, 2 ** 32 - 20
    det, E, fired = pm.sample(H, 3, 0.05, 0.03, seed, shot0, 50)
    gd, go, gf = dm.sample(d.H, d.L, d.priors, seed, shot0, 50)
    assert np.array_equal(gf, fired) and np.array_equal(gd, det) and np.array_equal(go, pm.mod2(E, L % 2))


# ---------------------------------------------------------------------------
# argument validation
# ---------------------------------------------------------------------------
def _small():
    from qldpcsim_amd import dem as D
    H, L = half("steane")[:2]
    return D.phenomenological_dem(H, L, 2, 0.02, 0.01)


def test_simulate_dem_refuses_bad_arguments():
    from qldpcsim_amd import simulator
    d = _small()
    for kw in (dict(decType="RELAY"), dict(decType="NG"), dict(decType="BF"), dict(decType="XX"),
               dict(decSchedule="Q"), dict(sampler="gpu"), dict(shots=-1), dict(osd_method="zz"),
               dict(osd_method="cs"), dict(osd_method="cs", OSDorder=65)):
        with pytest.raises(ValueError):
            simulator.simulate_dem(d, **{"shots": 4, "verbose": False, **kw})
    with pytest.raises(ValueError, match="Dem"):
        simulator.simulate_dem((d.H, d.L, d.priors), shots=4, verbose=False)
    with pytest.raises(TypeError):
        simulator.simulate_dem(d, shots=4, verbose=False, correlated="XZ")


def test_cli_usage_errors(capsys):
    """With --dem, every option of the CSS-pair modes is a usage error; without
    it --Hx, --Hz and --p are required as before."""
    from qldpcsim_amd import simulator
    for extra in (["--Hx", "a.npy"], ["--Hz", "b.npy"], ["--p", "0.01"], ["--rounds", "2"], ["--window", "2"],
                  ["--logical"], ["--correlated", "XZ"], ["--bias", "3"], ["--channel-weights", "w.npy"]):
        with pytest.raises(SystemExit) as e:
            simulator.main(["--dem", "m.dem"] + extra)
        assert e.value.code == 2
        assert f"--dem cannot be combined with {extra[0]}" in capsys.readouterr().err
    for dec in ("NG", "BF", "RELAY"):
        with pytest.raises(SystemExit) as e:
            simulator.main(["--dem", "m.dem", "--decType", dec])
        assert e.value.code == 2 and "--dem decodes with MS or BP" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        simulator.main(["--dem=m.dem", "--osd-method", "cs"])
    assert e.value.code == 2 and "--OSDorder" in capsys.readouterr().err
    for argv, missing in ((["--Hz", "b.npy", "--p", "0.01"], "--Hx"), (["--Hx", "a.npy", "--p", "0.01"], "--Hz"),
                          (["--Hx", "a.npy", "--Hz", "b.npy"], "--p")):
        with pytest.raises(SystemExit) as e:
            simulator.main(argv)
        assert e.value.code == 2
        assert f"the following arguments are required: {missing}" in capsys.readouterr().err


def test_cli_runs_the_model_and_writes_the_record(tmp_path, monkeypatch, capsys):
    """--dem FILE loads the file, runs simulate_dem with the command line's
    settings, prints the mode's table and writes the one record with the run's
    parameters."""
    from qldpcsim_amd import dem as D, simulator
    d = _small()
    (tmp_path / "m.dem").write_text(D.dem_text(d))
    calls = []

    def fake(dem, **kw):
        calls.append((dem, kw))
        return {"DecFailures": 3, "logicalErrors": 5, "decSuccess": 92, "nIterAcc": 250, "logical_error_rate": 0.08,
                "logical_error_rate_ci95": (0.04, 0.15), "detectors": dem.num_detectors, "errors": dem.num_errors,
                "observables": dem.num_observables}

    monkeypatch.setattr(simulator, "simulate_dem", fake)
    res = tmp_path / "res.json"
    simulator.main(["--dem", str(tmp_path / "m.dem"), "--shots", "100", "--decType", "BP", "--decIterations", "17",
                    "--decSchedule", "L", "--OSDorder", "0", "--rngSeed", "4", "--batch", "50", "--sampler", "host",
                    "--results", str(res)])
    (got, kw), = calls
    assert got == D.parse_dem(D.dem_text(d))
    assert kw == dict(shots=100, decType="BP", decIterations=17, decSchedule="L", OSDorder=0, rngSeed=4, batch_size=50,
                      sampler="host", verbose=True, osd_method="ref")
    out = capsys.readouterr().out
    assert "DETECTOR ERROR MODEL" in out and "8.00e-02" in out and "SIMULATION RESULTS" not in out
    assert f"{d.num_detectors} x {got.num_errors}, {d.num_observables}" in out
    doc = json.loads(res.read_text())
    assert doc["result"]["logicalErrors"] == 5 and doc["result"]["logical_error_rate_ci95"] == [0.04, 0.15]
    assert doc["meta"] == {"dem": str(tmp_path / "m.dem"), "shots": 100, "decType": "BP", "decIterations": 17,
                           "decSchedule": "L", "OSDorder": 0, "rngSeed": 4, "world": 1, "sampler": "host"}


def test_results_table_of_the_mode():
    from qldpcsim_amd import simulator
    r = {"DecFailures": 3, "logicalErrors": 4, "decSuccess": 993, "nIterAcc": 2500, "logical_error_rate": 0.007,
         "logical_error_rate_ci95": [0.003, 0.012], "detectors": 24, "errors": 86, "observables": 1}
    txt = simulator.format_dem_results("surface.dem", r, 1000)
    assert "DETECTOR ERROR MODEL" in txt and "surface.dem (24 x 86, 1)" in txt and "7.00e-03" in txt
    assert "3.00e-03" in txt and "1.20e-02" in txt and "2.500" in txt


def test_c_entry_points_validate_before_any_hip_call():
    """A null handle or required buffer, an unknown format, a negative batch, a
    bad prior and a bad observable count give QLDPC_EINVAL (ValueError) with
    or without a device: every pointer here is a dummy the library must never
    touch. batch == 0 is QLDPC_OK; a row past the kernels' LDS is refused as
    unsupported when the handle is made."""
    from qldpcsim_amd import _lib
    d = _small()
    code = _lib.Code(d.H)
    tab = _lib.DemTable(code, d.L, d.priors)
    assert tab.k == d.num_observables and tab.kw == 1
    assert _lib.dem_kernel_name(tab, "sample") == "dem_sample_kernel<16>"
    assert _lib.dem_kernel_name(tab, "count") == "dem_count_kernel<16>"
    X = 4096                                                # a non-null address that is never read
    ok = dict(seed=1, shot0=0, batch=4, det=X, det_fmt=_lib.FMT_BYTES, obs=X)
    for bad in (dict(det=None), dict(obs=None), dict(det_fmt=7), dict(batch=-1)):
        with pytest.raises(ValueError):
            _lib.dem_sample(tab, **{**ok, **bad})
    _lib.dem_sample(tab, **{**ok, "batch": 0})
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_dem_sample(None, 1, 0, 4, X, 0, X, None, None))
    okc = dict(batch=4, det=X, det_fmt=_lib.FMT_BITS, obs=X, ehat=X, e_fmt=_lib.FMT_BITS, iters=X, acc=X)
    for bad in (dict(det=None), dict(obs=None), dict(ehat=None), dict(iters=None), dict(acc=None), dict(det_fmt=2),
                dict(e_fmt=-1), dict(batch=-1)):
        with pytest.raises(ValueError):
            _lib.dem_count(tab, **{**okc, **bad})
    _lib.dem_count(tab, **{**okc, "batch": 0})
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_dem_count(None, 4, X, 0, X, X, 0, X, X, None, None, None))
    # no observable: the observable buffers may be null
    tab0 = _lib.DemTable(code, np.zeros((0, d.num_errors), np.uint8), d.priors)
    assert tab0.k == 0 and tab0.kw == 0
    _lib.dem_sample(tab0, **{**ok, "obs": None, "batch": 0})
    _lib.dem_count(tab0, **{**okc, "obs": None, "batch": 0})
    # the handle
    out = ctypes.c_void_p()
    pr = np.ascontiguousarray(d.priors)
    Lc = np.ascontiguousarray(d.L)
    create = _lib.lib.qldpc_dem_create
    for args in ((None, _lib.ptr(Lc), tab.k, _lib.ptr(pr), ctypes.byref(out)),
                 (code.handle, _lib.ptr(Lc), tab.k, _lib.ptr(pr), None),
                 (code.handle, None, tab.k, _lib.ptr(pr), ctypes.byref(out)),
                 (code.handle, _lib.ptr(Lc), -1, _lib.ptr(pr), ctypes.byref(out)),
                 (code.handle, _lib.ptr(Lc), tab.k, None, ctypes.byref(out))):
        with pytest.raises(ValueError):
            _lib.check(create(*args))
    for badp in (1.0, -1e-9, float("nan")):
        q = d.priors.copy()
        q[3] = badp
        with pytest.raises(ValueError, match="prior 3"):
            _lib.DemTable(code, d.L, q)
    with pytest.raises(ValueError):
        _lib.DemTable(code, d.L[:, :-1], d.priors)
    with pytest.raises(ValueError):
        _lib.DemTable(code, d.L, d.priors[:-1])
    with pytest.raises(ValueError):
        _lib.check(_lib.lib.qldpc_dem_kernel_name(tab.handle, 5, ctypes.create_string_buffer(64), 64))
    # 64 (ceil(M/64) + ceil(K/64)) bits of LDS per wave: 2^18 is the last row that fits
    thin = _lib.Code(np.zeros((2 ** 18 - 64, 1), np.uint8))
    one = np.array([0.1])
    assert _lib.dem_kernel_name(_lib.DemTable(thin, np.zeros((64, 1), np.uint8), one), "count") == \
        "dem_count_kernel<32>"
    with pytest.raises(NotImplementedError):
        _lib.DemTable(thin, np.zeros((65, 1), np.uint8), one)
    # 65536 bits is the last row with 16-bit lists
    edge = _lib.Code(np.zeros((65536 - 64, 1), np.uint8))
    assert _lib.dem_kernel_name(_lib.DemTable(edge, np.zeros((64, 1), np.uint8), one), "sample") == \
        "dem_sample_kernel<16>"
    assert _lib.dem_kernel_name(_lib.DemTable(edge, np.zeros((65, 1), np.uint8), one), "sample") == \
        "dem_sample_kernel<32>"
    assert _lib.lib.qldpc_dem_destroy(None) == 0

"""Library option vprior_hbm without a GPU: the option itself, the refusals
it leaves in place when off, the kernel hbm_tile_vprior_kernel chosen for each
case the LDS twin refuses, the C entry points' validation with the option on,
and the simulator's hbm_priors keyword, command-line flag and results meta."""
import ctypes
import json

import numpy as np
import pytest

from qldpcsim_amd import _lib, codes, decoders, dem as D, simulator

FLOOD = lambda m: (np.array([0, m], np.int32), np.arange(m, dtype=np.int32))  # noqa: E731


def _steane():
    Hx, _ = codes.load_code("steane")
    code = _lib.Code(Hx)
    sched = code.schedule(*FLOOD(code.m))
    return Hx, code, sched


def _past_the_limits():
    """(H, algo, match of today's refusal, the HBM instance's name) of the
    three refusals that need no device."""
    wide = np.zeros((1, 65536), np.uint8)
    wide[0, :3] = 1
    return [(np.ones((1, 40), np.uint8), "MS", "row degree", "hbm_tile_vprior_kernel<0, 64, 4>"),
            (wide, "MS", "65535", "hbm_tile_vprior_kernel<0, 8, 4>"),
            (np.ones((130, 2), np.uint8), "BP", "column degree", "hbm_tile_vprior_kernel<1, 8, 4>")]


def test_option_exists_defaults_to_zero_and_is_restored():
    assert _lib.get_option("vprior_hbm") == 0
    with _lib.options(vprior_hbm=1):
        assert _lib.get_option("vprior_hbm") == 1
        with _lib.options(vprior_hbm=0, force_hbm=1):
            assert _lib.get_option("vprior_hbm") == 0 and _lib.get_option("force_hbm") == 1
        assert _lib.get_option("vprior_hbm") == 1 and _lib.get_option("force_hbm") == 0
    assert _lib.get_option("vprior_hbm") == 0
    _lib.set_option("vprior_hbm", 1)
    _lib.set_option("vprior_hbm", 0)
    assert _lib.get_option("vprior_hbm") == 0


def test_option_off_keeps_every_refusal_and_name():
    """With vprior_hbm = 0 nothing changes: the refusals of
    test_vprior_model.py with their words, force_hbm's, and the LDS twin's
    names."""
    assert _lib.get_option("vprior_hbm") == 0
    for H, algo, match, _ in _past_the_limits():
        m, n = H.shape
        with pytest.raises(NotImplementedError, match=match):
            decoders.decode_batch(H, np.zeros((1, m), np.uint8), None, 5, algo=algo, prior=np.full(n, 0.01))
        with pytest.raises(NotImplementedError, match=match):
            _lib.vprior_kernel_name(H, *FLOOD(m), algo)
    Hx, code, sched = _steane()
    with _lib.options(force_hbm=1):
        with pytest.raises(NotImplementedError, match="per-variable priors: option force_hbm is set and there is no "
                                                      "HBM-resident variant"):
            _lib.vprior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "MS")
    for algo in ("MS", "BP"):
        assert _lib.vprior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, algo) == \
            f"decode_vprior_kernel<{_lib.ALGO[algo]}, false, 0>"
    Hl = codes.load_code("LP04_0")[0]
    lp, lr = simulator.pack_layers(simulator.layerize(Hl), Hl.shape[0])
    assert _lib.vprior_kernel_name(Hl, lp, lr, "MS") == "decode_vprior_kernel<0, true, 7>"


def test_option_on_names_the_hbm_instance():
    """Past each device-free limit, and everywhere with force_hbm as well:
    hbm_tile_vprior_kernel<algo, D, 4> with D from the row degree as
    select_hbm_kernel picks it. Within the limits the LDS twin keeps its name
    (without a device the LDS size is not asked)."""
    Hx, _, sched = _steane()
    with _lib.options(vprior_hbm=1):
        for H, algo, _, name in _past_the_limits():
            assert _lib.vprior_kernel_name(H, *FLOOD(H.shape[0]), algo) == name
        if _lib.device_count() == 0:
            assert _lib.vprior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "MS") == \
                "decode_vprior_kernel<0, false, 0>"
        with _lib.options(force_hbm=1):
            assert _lib.vprior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "MS") == \
                "hbm_tile_vprior_kernel<0, 8, 4>"
            assert _lib.vprior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "BP") == \
                "hbm_tile_vprior_kernel<1, 8, 4>"
            # row degrees 9, 17, 33: the next instance each
            for d, inst in ((8, 8), (9, 16), (16, 16), (17, 32), (32, 32), (33, 64), (64, 64), (65, 64)):
                H = np.ones((2, d), np.uint8)
                for algo in ("MS", "BP"):
                    assert _lib.vprior_kernel_name(H, *FLOOD(2), algo) == \
                        f"hbm_tile_vprior_kernel<{_lib.ALGO[algo]}, {inst}, 4>", d
            # the two-level twin has no HBM-resident variant
            with pytest.raises(NotImplementedError, match="two-level priors: option force_hbm"):
                _lib.prior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "MS")
        with pytest.raises(NotImplementedError, match="two-level priors: MS row degree 40 > 32"):
            _lib.prior_kernel_name(np.ones((1, 40), np.uint8), *FLOOD(1), "MS")
    assert _lib.get_option("vprior_hbm") == 0 and _lib.get_option("force_hbm") == 0


def test_c_entry_points_validate_with_both_options_on():
    """Every bad argument test_c_decode_entry_points_validate_before_any_hip_call
    lists is still QLDPC_EINVAL with vprior_hbm = force_hbm = 1, and force_hbm
    is no longer answered with QLDPC_EUNSUP (with no device the call then ends
    at the device check, QLDPC_EHIP; with one it decodes)."""
    L = _lib.lib
    Hx, code, sched = _steane()
    m, n = code.m, code.n
    pr = code.prior(np.linspace(0.01, 0.2, n), 1e-9)
    syn = np.zeros((2, m), np.uint8)
    e = np.zeros((2, n), np.uint8)
    it = np.zeros(2, np.int32)
    P = _lib.ptr

    def dev(algo=0, sf=0, batch=2, prior=pr.handle, mi=5, ef=0, s=syn, eh=e, i=it, sc=sched.handle, c=code.handle):
        return L.qldpc_decode_device_vprior(c, sc, algo, P(s), sf, batch, prior, mi, 0.75, P(eh), ef, P(i), None,
                                            None, None)

    def host(algo=0, batch=2, prior=pr.handle, mi=5, s=syn, sc=sched.handle):
        return L.qldpc_decode_host_vprior(code.handle, sc, algo, P(s), batch, prior, mi, 0.75, P(e), P(it), None, None)

    EINVAL = _lib.QLDPC_EINVAL
    buf = ctypes.create_string_buffer(64)
    with _lib.options(vprior_hbm=1, force_hbm=1):
        assert dev(prior=None) == EINVAL and b"prior" in L.qldpc_last_error()
        assert host(prior=None) == EINVAL
        assert dev(sf=2) == EINVAL and dev(ef=7) == EINVAL
        assert dev(algo=2) == EINVAL and dev(algo=3) == EINVAL
        assert host(algo=2) == EINVAL and host(algo=3) == EINVAL
        assert dev(batch=-1) == EINVAL and dev(mi=0) == EINVAL and host(batch=-1) == EINVAL and host(mi=0) == EINVAL
        assert dev(sc=None) == EINVAL and dev(c=None) == EINVAL and host(sc=None) == EINVAL
        assert dev(batch=0, s=None, eh=None, i=None) == _lib.QLDPC_OK
        assert host(batch=0, s=None) == _lib.QLDPC_OK
        other = _lib.Code(np.roll(Hx, 1, axis=1))
        foreign = other.prior(np.full(n, 0.01), 1e-9)
        assert dev(prior=foreign.handle) == EINVAL and b"different code" in L.qldpc_last_error()
        assert host(prior=foreign.handle) == EINVAL
        assert dev(prior=foreign.handle, batch=0) == EINVAL
        assert L.qldpc_decode_vprior_kernel_name(code.handle, sched.handle, 2, buf, 64) == EINVAL
        assert L.qldpc_decode_vprior_kernel_name(code.handle, None, 0, buf, 64) == EINVAL
        # null buffers: invalid on the host entry before any copy; on the device
        # entry (these are host arrays: only the validation may be reached)
        assert host(s=None) == EINVAL
        assert dev(s=None) == EINVAL and dev(eh=None) == EINVAL and dev(i=None) == EINVAL
        # force_hbm is routed, not refused
        assert L.qldpc_decode_vprior_kernel_name(code.handle, sched.handle, 0, buf, 64) == _lib.QLDPC_OK
        assert buf.value == b"hbm_tile_vprior_kernel<0, 8, 4>"
        if _lib.device_count() == 0:
            assert dev() == _lib.QLDPC_EHIP and host() == _lib.QLDPC_EHIP
        else:
            assert host() == _lib.QLDPC_OK
    with _lib.options(force_hbm=1):
        assert dev() == _lib.QLDPC_EUNSUP and host() == _lib.QLDPC_EUNSUP


def test_prior_mask_under_force_hbm_is_still_refused():
    Hx, _ = codes.load_code("steane")
    m, n = Hx.shape
    syn = np.zeros((2, m), np.uint8)
    with _lib.options(vprior_hbm=1, force_hbm=1):
        with pytest.raises(NotImplementedError, match="two-level priors: option force_hbm"):
            decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=np.zeros((2, n), np.uint8), p_masked=0.4)
        with pytest.raises(ValueError, match="prior_mask"):
            decoders.decode_batch(Hx, syn, None, 5, prior=np.full(n, 0.01), prior_mask=np.zeros((2, n), np.uint8),
                                  p_masked=0.4)


def test_cli_parses_hbm_priors(tmp_path, monkeypatch):
    Hx, Hz = codes.load_code("steane")
    fx, fz = str(tmp_path / "hx.npy"), str(tmp_path / "hz.npy")
    np.save(fx, Hx)
    np.save(fz, Hz)
    seen = []
    monkeypatch.setattr(simulator, "simulate", lambda **kw: seen.append(kw))
    base = ["--Hx", fx, "--Hz", fz, "--p", "0.01", "--rounds", "3", "--meas-error", "0.02"]
    simulator.main(base)
    assert "hbm_priors" not in seen[-1]
    simulator.main(base + ["--hbm-priors"])
    assert seen[-1]["hbm_priors"] is True and seen[-1]["rounds"] == 3
    simulator.main(base + ["--window", "2", "--hbm-priors"])
    assert seen[-1]["hbm_priors"] is True and seen[-1]["window"] == 2
    with pytest.raises(SystemExit):
        simulator.main(["--Hx", fx, "--Hz", fz, "--p", "0.01", "--hbm-priors"])   # neither --rounds nor --dem
    f = tmp_path / "m.dem"
    f.write_text("error(0.1) D0 D1 L0\nerror(0.05) D1\n")
    runs = []
    monkeypatch.setattr(simulator, "_run_dem", lambda *a, **kw: runs.append((a, kw)))
    simulator.main(["--dem", str(f)])
    assert runs[-1][1].get("hbm_priors", False) is False
    simulator.main(["--dem", str(f), "--hbm-priors"])
    assert runs[-1][1]["hbm_priors"] is True


def test_keywords_validate_and_reach_the_results_meta(tmp_path, monkeypatch):
    Hx, Hz = codes.load_code("steane")
    fx, fz = str(tmp_path / "hx.npy"), str(tmp_path / "hz.npy")
    np.save(fx, Hx)
    np.save(fz, Hz)
    model = D.parse_dem("error(0.1) D0 D1 L0\nerror(0.05) D1\n")
    for bad in (1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="hbm_priors"):
            simulator.simulate_dem(model, shots=4, sampler="host", verbose=False, hbm_priors=bad)
        with pytest.raises(ValueError, match="hbm_priors"):
            simulator.simulate_phenomenological(Hx, Hz, 0.01, 0.02, 2, shots=4, sampler="host", verbose=False,
                                                hbm_priors=bad)
        with pytest.raises(ValueError, match="hbm_priors"):
            simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, sampler="host", rounds=2, hbm_priors=bad)
    with pytest.raises(ValueError, match="hbm_priors needs rounds"):
        simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, sampler="host", hbm_priors=True)
    # the phenomenological sweep: passed on to every point and recorded only when set
    calls = []

    def fake(Hx, Hz, p, q, rounds, **kw):
        calls.append(kw)
        return {"q": q, "rounds": rounds, "logical_error_rate": 0.0, "logical_error_rate_ci95": (0.0, 1.0),
                "logical_error_rate_per_round": 0.0, "DecFailures_X": 0, "DecFailures_Z": 0, "logicalErrors_X": 0,
                "logicalErrors_Z": 0}

    monkeypatch.setattr(simulator, "simulate_phenomenological", fake)
    rf = str(tmp_path / "res.json")
    run = lambda f=rf, **kw: simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, sampler="host",  # noqa: E731
                                                resultsFile=f, rounds=3, meas_error=0.02, **kw)
    run(hbm_priors=True)
    assert json.load(open(rf))["meta"]["hbm_priors"] is True and calls[-1]["hbm_priors"] is True
    run(hbm_priors=True)                                         # same run: resumed
    assert len(calls) == 1
    with pytest.raises(ValueError, match="different run"):
        run()
    rf2 = str(tmp_path / "plain.json")
    run(rf2)
    assert "hbm_priors" not in json.load(open(rf2))["meta"] and "hbm_priors" not in calls[-1]
    # the detector error model's record
    seen = []
    monkeypatch.setattr(simulator, "simulate_dem", lambda dem, **kw: seen.append(kw) or {
        "logical_error_rate": 0.0, "logical_error_rate_ci95": (0.0, 1.0), "detectors": 2, "errors": 2,
        "observables": 1, "DecFailures": 0, "logicalErrors": 0, "nIterAcc": 4})
    f = tmp_path / "m.dem"
    f.write_text("error(0.1) D0 D1 L0\nerror(0.05) D1\n")
    rf3, rf4 = str(tmp_path / "dem.json"), str(tmp_path / "dem_plain.json")
    simulator._run_dem(str(f), 4, "MS", 5, "F", -1, 1, None, "host", rf3, "ref", hbm_priors=True)
    assert seen[-1]["hbm_priors"] is True and json.load(open(rf3))["meta"]["hbm_priors"] is True
    simulator._run_dem(str(f), 4, "MS", 5, "F", -1, 1, None, "host", rf4, "ref")
    assert "hbm_priors" not in seen[-1] and "hbm_priors" not in json.load(open(rf4))["meta"]


def test_the_option_is_set_once_around_a_run(monkeypatch):
    """hbm_priors=True sets vprior_hbm for the whole run (one option change on
    the way in, one on the way out: every change drops the cached launch
    plans) and restores it even when the run raises."""
    model = D.parse_dem("error(0.1) D0 D1 L0\nerror(0.05) D1\n")
    sets = []
    real = _lib.set_option
    monkeypatch.setattr(_lib, "set_option", lambda k, v: (sets.append((k, v)), real(k, v))[1])
    seen = []

    def probe(*a, **kw):
        seen.append(_lib.get_option("vprior_hbm"))
        raise NotImplementedError("stop here")

    monkeypatch.setattr(simulator, "_decode_half", probe)
    with pytest.raises(NotImplementedError, match="stop here"):
        simulator.simulate_dem(model, shots=4, sampler="host", verbose=False, hbm_priors=True)
    assert seen == [1] and sets == [("vprior_hbm", 1), ("vprior_hbm", 0)]
    assert _lib.get_option("vprior_hbm") == 0
    with pytest.raises(NotImplementedError, match="stop here"):
        simulator.simulate_dem(model, shots=4, sampler="host", verbose=False)
    assert seen == [1, 0] and len(sets) == 2

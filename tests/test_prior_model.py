"""Two-level priors without a device: the test-side model (tests/prior_model.py)
against the reference's goldens when every prior is equal, the argument
checks of decode_batch(prior_mask=, p_masked=) and of the C entry points
(decided before any HIP call), simulate_p's correlated= validation, and the
results file's meta."""
import ctypes
import json

import numpy as np
import pytest

import prior_model as pm
from conftest import golden_cases, half_matrix
from qldpcsim_amd import _lib, codes, decoders, simulator


def _layers(a, m):
    lp, lr = a["layer_ptr"], a["layer_rows"]
    if len(lp) == 2 and np.array_equal(lr, np.arange(m)):
        return None
    return [lr[lp[i]:lp[i + 1]] for i in range(len(lp) - 1)]


def _pick(algo, code, scheds, per=3):
    """A handful of plain golden cases per schedule (no OSD, below 100 iterations)."""
    out = []
    for sched in scheds:
        cs = [(c, a) for c, a in golden_cases(f"{algo.lower()}_{code}.npz")
              if "raises" not in c and c["sched"] == sched and c["osd"] < 0 and c["max_iter"] < 100]
        assert cs, (algo, code, sched)
        out += cs[:per]
    return out


GOLD = _pick("MS", "steane", "FL") + _pick("MS", "LP04_0", "FL") + _pick("BP", "steane", "F", 2) + \
    _pick("BP", "LP04_0", "F", 2)


@pytest.mark.parametrize("ca", GOLD, ids=[f"{c['algo']}-{c['code']}-{c['half']}-{c['sched']}-{c['kind']}-"
                                          f"p{c['p_phys']}-it{c['max_iter']}" for c, _ in GOLD])
def test_model_with_equal_priors_is_the_reference(ca):
    c, a = ca
    H = half_matrix(c)
    syn = a["syn"][:24]                                      # (the BP model is slow: a handful of shots)
    L = np.full((len(syn), H.shape[1]), pm.llr(c["p_phys"] / 3))
    e, it, post, _ = pm.decode(c["algo"], H, syn, L, c["max_iter"], _layers(a, H.shape[0]))
    np.testing.assert_array_equal(it, a["iters"][:24])
    np.testing.assert_array_equal(e, a["ehat"][:24])
    np.testing.assert_array_equal(post.view(np.uint64), a["post"][:24].view(np.uint64))


def test_model_two_level_helper():
    L = pm.two_level(np.array([[0, 1, 1]]), 0.01, 0.5)
    assert L[0, 0] == np.log(0.99 / 0.01) and L[0, 1] == 0.0 and not np.signbit(L[0, 1])


def test_decode_batch_validates_the_mask():
    Hx, _ = codes.load_code("steane")
    m, n = Hx.shape
    syn = np.zeros((2, m), np.uint8)
    mask = np.zeros((2, n), np.uint8)
    with pytest.raises(ValueError, match="both or neither"):
        decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=mask)
    with pytest.raises(ValueError, match="both or neither"):
        decoders.decode_batch(Hx, syn, 0.01, 5, p_masked=0.4)
    for algo in ("NG", "BF"):
        with pytest.raises(ValueError, match="hard-decision"):
            decoders.decode_batch(Hx, syn, 0.01, 5, algo=algo, prior_mask=mask, p_masked=0.4)
    with pytest.raises(ValueError, match="prior_mask must be"):
        decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=mask[:, :-1], p_masked=0.4)
    with pytest.raises(ValueError, match="prior_mask must be"):
        decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=mask[:1], p_masked=0.4)
    with pytest.raises(ValueError, match="0 or 1"):
        decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=mask + 2, p_masked=0.4)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="probabilities"):
            decoders.decode_batch(Hx, syn, 0.01, 5, prior_mask=mask, p_masked=bad)
        with pytest.raises(ValueError, match="probabilities"):
            decoders.decode_batch(Hx, syn, bad, 5, prior_mask=mask, p_masked=0.4)


def test_c_entry_points_validate_before_any_hip_call():
    L = _lib.lib
    Hx, _ = codes.load_code("steane")
    code = _lib.Code(Hx)
    m, n = code.m, code.n
    sched = code.schedule(np.array([0, m], np.int32), np.arange(m, dtype=np.int32))
    syn = np.zeros((2, m), np.uint8)
    mask = np.zeros((2, n), np.uint8)
    e = np.zeros((2, n), np.uint8)
    it = np.zeros(2, np.int32)
    P = _lib.ptr

    def dev(algo=0, sf=0, batch=2, p0=0.01, p1=0.4, mk=mask, mf=0, mi=5, ef=0, s=syn, eh=e, i=it, sc=sched.handle):
        return L.qldpc_decode_device_prior(code.handle, sc, algo, P(s), sf, batch, p0, p1, P(mk), mf, mi, 0.75,
                                           1e-9, P(eh), ef, P(i), None, None, None)

    def host(algo=0, batch=2, p0=0.01, p1=0.4, mk=mask, mi=5, s=syn):
        return L.qldpc_decode_host_prior(code.handle, sched.handle, algo, P(s), batch, p0, p1, P(mk), mi, 0.75,
                                         1e-9, P(e), P(it), None, None)

    EINVAL = _lib.QLDPC_EINVAL
    assert dev(mk=None) == EINVAL and b"mask" in L.qldpc_last_error()
    assert dev(mf=2) == EINVAL and dev(mf=-1) == EINVAL
    assert dev(sf=2) == EINVAL and dev(ef=7) == EINVAL
    for bad in (-1e-3, 1.0001, float("nan")):
        assert dev(p0=bad) == EINVAL and dev(p1=bad) == EINVAL
        assert host(p0=bad) == EINVAL and host(p1=bad) == EINVAL
    assert dev(algo=2) == EINVAL and dev(algo=3) == EINVAL   # NG / BF take no prior
    assert dev(batch=-1) == EINVAL and dev(mi=0) == EINVAL
    assert dev(s=None) == EINVAL and dev(eh=None) == EINVAL and dev(i=None) == EINVAL
    assert dev(sc=None) == EINVAL
    assert dev(batch=0, mk=None, s=None, eh=None, i=None) == _lib.QLDPC_OK
    assert host(mk=None) == EINVAL and host(s=None) == EINVAL and host(algo=3) != _lib.QLDPC_OK
    assert host(batch=0, mk=None) == _lib.QLDPC_OK
    # force_hbm: refused as unsupported, before the device is looked at
    with _lib.options(force_hbm=1):
        assert dev() == _lib.QLDPC_EUNSUP and b"force_hbm" in L.qldpc_last_error()
        assert host() == _lib.QLDPC_EUNSUP
        buf = ctypes.create_string_buffer(64)
        assert L.qldpc_decode_prior_kernel_name(code.handle, sched.handle, 0, buf, 64) == _lib.QLDPC_EUNSUP
    assert _lib.get_option("force_hbm") == 0
    # the kernel's name needs no device
    assert _lib.prior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "MS") == "decode_prior_kernel<0, false, 0>"
    assert _lib.prior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, "BP") == "decode_prior_kernel<1, false, 0>"
    Hl = codes.load_code("LP04_0")[0]
    lp, lr = simulator.pack_layers(simulator.layerize(Hl), Hl.shape[0])
    assert _lib.prior_kernel_name(Hl, lp, lr, "MS") == "decode_prior_kernel<0, true, 7>"
    buf = ctypes.create_string_buffer(64)
    assert L.qldpc_decode_prior_kernel_name(code.handle, sched.handle, 2, buf, 64) == EINVAL
    assert L.qldpc_decode_prior_kernel_name(code.handle, None, 0, buf, 64) == EINVAL


def test_codes_past_the_lds_kernel_are_refused_before_any_launch():
    """m, n or E > 65535 and MS row degree > 32: NotImplementedError, no device needed."""
    H = np.zeros((1, 65536), np.uint8)
    H[0, :3] = 1
    with pytest.raises(NotImplementedError, match="65535"):
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), 0.01, 5, prior_mask=np.zeros((1, 65536), np.uint8),
                              p_masked=0.4)
    H = np.ones((1, 40), np.uint8)
    with pytest.raises(NotImplementedError, match="row degree"):
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), 0.01, 5, prior_mask=np.zeros((1, 40), np.uint8),
                              p_masked=0.4)
    H = np.ones((130, 2), np.uint8)
    with pytest.raises(NotImplementedError, match="column degree"):
        decoders.decode_batch(H, np.zeros((1, 130), np.uint8), 0.01, 5, algo="BP",
                              prior_mask=np.zeros((1, 2), np.uint8), p_masked=0.4)


def test_simulate_p_validates_correlated():
    Hx, Hz = codes.load_code("steane")
    kw = dict(shots=4, sampler="host", verbose=False)
    with pytest.raises(ValueError, match="correlated must be"):
        simulator.simulate_p(Hx, Hz, 0.05, correlated="YX", **kw)
    for q1 in (0.0, -0.1, 0.51, float("nan")):
        with pytest.raises(ValueError, match="correlated_q1"):
            simulator.simulate_p(Hx, Hz, 0.05, correlated="XZ", correlated_q1=q1, **kw)
    for decType in ("NG", "BF"):
        with pytest.raises(ValueError, match="hard-decision"):
            simulator.simulate_p(Hx, Hz, 0.05, decType=decType, correlated="ZX", **kw)


def test_cli_knows_the_options():
    with pytest.raises(SystemExit):
        simulator.main(["--Hx", "x", "--Hz", "z", "--p", "0.1", "--correlated", "XY"])


def test_results_file_meta_separates_modes(tmp_path, monkeypatch):
    """A sweep is never resumed across modes: correlated and correlated_q1 are
    part of the results file's meta (simulate_p itself is stubbed out)."""
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
                                          resultsFile=rf, **kw)
    run(correlated="XZ")
    meta = json.load(open(rf))["meta"]
    assert meta["correlated"] == "XZ" and meta["correlated_q1"] == 0.49
    assert calls[-1]["correlated"] == "XZ" and calls[-1]["correlated_q1"] == 0.49
    run(correlated="XZ")                                     # same mode: resumed, nothing recomputed
    assert len(calls) == 1
    for other in (dict(), dict(correlated="ZX"), dict(correlated="XZ", correlated_q1=0.4)):
        with pytest.raises(ValueError, match="different run"):
            run(**other)
    rf2 = str(tmp_path / "plain.json")
    simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, sampler="host", resultsFile=rf2)
    meta = json.load(open(rf2))["meta"]
    assert "correlated" not in meta and "correlated_q1" not in meta
    assert "correlated" not in calls[-1]

"""The hard-decision decoders (NG, BF) without a GPU: the test-side NumPy model
(tests/hard_model.py) reproduces every recorded output of the unmodified
reference (tests/golden/hard/), the fixtures really hold the hard cases, and
the Python / C entry points validate their arguments before touching a device."""
import ctypes

import numpy as np
import pytest

import hard_model as hm
from qldpcsim_amd import _lib, decoders, simulator

CASES = hm.golden_cases()


def _by(algo, **kw):
    return [(c, a, H) for c, a, H in CASES if c["algo"] == algo and all(c[k] == v for k, v in kw.items())]


@pytest.mark.parametrize("c,a,H", CASES, ids=[hm.case_id(c) for c, _, _ in CASES])
def test_model_equals_the_reference_on_every_fixture_case(c, a, H):
    if c["algo"] == "BF":
        e, it, conv = hm.bf_batch(H, a["syn"], c["max_iter"])
    else:
        e, it, info = hm.ng_batch(H, a["syn"])
        conv = info["conv"]
    assert np.array_equal(e, a["ehat"])
    assert np.array_equal(it, a["iters"])
    assert np.array_equal(conv, a["conv"].astype(bool))


def test_fixture_cases_are_the_ones_the_issue_lists():
    got = {(c["code"], c["half"], c["kind"], c["algo"], c["max_iter"]): a["syn"].shape[0] for c, a, _ in CASES}
    want = {}
    for code, shots in (("steane", 200), ("shor", 200), ("LP04_0", 60), ("LP118_0", 24), ("LP118_2", 12)):
        for half in "XZ":
            want[(code, half, "channel", "NG", 0)] = shots
            for mi in (50,) + ((1, 2, 3, 7) if code == "LP04_0" else ()):
                want[(code, half, "channel", "BF", mi)] = shots
    for kind in ("random", "channel"):
        want[("synthetic", "X", kind, "NG", 0)] = 60
        want[("synthetic", "X", kind, "BF", 50)] = 60
    assert got == want
    H = hm.synthetic_matrix()
    assert H.shape == (37, 150)
    assert (H.sum(axis=1) == 0).sum() == 1 and (H.sum(axis=0) == 0).sum() >= 1 and H.sum(axis=1).max() == 100


def test_fixtures_hold_the_hard_cases():
    """Each condition on the reference's own recorded outputs (the model only
    supplies what a return value cannot show: ties and the zero-score stop)."""
    bf50 = _by("BF", max_iter=50)
    # BF stopped (its non-zero-count residual vanished) with the wrong true parity
    for code in ("steane", "shor", "synthetic"):
        wrong = sum(int((a["conv"].astype(bool) & (hm.true_syndrome(H, a["ehat"]) != a["syn"]).any(axis=1)).sum())
                    for c, a, H in bf50 if c["code"] == code)
        assert wrong >= 1, code
    assert any((a["conv"] == 0).any() and (a["iters"][a["conv"] == 0] == 50).all() for _, a, _ in bf50)
    # BF stops at iteration 1 or not at all: the per-iteration state is pinned
    # by the same non-converging shots at max_iter 1, 2, 3, 7, 50
    for c, a, _ in _by("BF"):
        assert set(np.unique(a["iters"])) <= {1, c["max_iter"]}
    for half in "XZ":
        est = {c["max_iter"]: a["ehat"] for c, a, _ in _by("BF", code="LP04_0", half=half)}
        assert set(est) == {1, 2, 3, 7, 50}
        assert len({est[k].tobytes() for k in est}) >= 3          # the state keeps changing
    ng = _by("NG")
    for code in ("LP04_0", "LP118_2", "synthetic"):
        assert any((a["iters"] == 2 * H.shape[1]).any() for c, a, H in ng if c["code"] == code), code
    assert any((a["iters"] == 0).any() for _, a, _ in ng)
    zero_stops = 0
    for c, a, H in ng:
        _, steps, info = hm.ng_batch(H, a["syn"])
        assert info["tied"].sum() >= 12, hm.case_id(c)
        zero_stops += int((info["zero_stop"] & (steps > 0) & (steps < 2 * H.shape[1])).sum())
    assert zero_stops >= 1


def test_algo_table_and_validation_without_a_device():
    assert _lib.ALGO == {"MS": 0, "BP": 1, "NG": 2, "BF": 3}
    assert {"NG_decoder", "BF_decoder"} <= set(decoders.__all__)
    H = hm.synthetic_matrix()
    syn = np.zeros((3, H.shape[0]), np.uint8)
    with pytest.raises(ValueError, match="Unrecognized decoder type"):
        decoders.decode_batch(H, syn, 0.01, 5, algo="XX")
    for algo in ("NG", "BF"):
        with pytest.raises(ValueError, match="posteriors"):
            decoders.decode_batch(H, syn, 0.01, 5, algo=algo, want_post=True)
        with pytest.raises(ValueError, match="posteriors"):
            decoders.decode_batch(H, syn, 0.01, 5, algo=algo, osd_order=0)
        with pytest.raises(ValueError, match=r"\[B, 37\]"):
            decoders.decode_batch(H, syn[:, :-1], 0.01, 5, algo=algo)
        with pytest.raises(ValueError, match="0 or 1"):
            decoders.decode_batch(H, syn + 2, 0.01, 5, algo=algo)
    with pytest.raises(ValueError, match="max_iter"):
        decoders.decode_batch(H, syn, 0.01, 0, algo="BF")
    with pytest.raises(ValueError, match="shape"):
        decoders.NG_decoder(H, np.zeros(5, np.int8))


def test_reference_quirks_need_no_launch():
    H = hm.synthetic_matrix()
    for fn in (decoders.NG_decoder, decoders.BF_decoder):
        r = fn(np.zeros((0, 5)), np.zeros(0))                # empty H: a bare array, no tuple
        assert isinstance(r, np.ndarray) and r.dtype == np.int8 and r.shape == (0,)
        r = fn(H, np.zeros(0))                               # empty syndrome
        assert isinstance(r, np.ndarray) and r.dtype == np.int8 and r.shape == (150,)
    for mi in (0, -3):
        e, it = decoders.BF_decoder(H, np.ones(37, np.int64), max_iter=mi)
        assert e.dtype == np.float64 and e.shape == (150,) and not e.any() and it == mi


def test_c_entry_points_validate_before_any_hip_call():
    L = _lib.lib
    code = _lib.Code(hm.synthetic_matrix())
    m, n = code.m, code.n
    syn = np.zeros((2, m), np.uint8)
    e = np.zeros((2, n), np.uint8)
    it = np.zeros(2, np.int32)
    P = _lib.ptr

    def dev(algo=3, sf=0, batch=2, mi=50, ef=0, s=syn, eh=e, i=it):
        return L.qldpc_hard_decode_device(code.handle, algo, P(s), sf, batch, mi, P(eh), ef, P(i), None, None)

    for algo in (0, 1, 4, -1):                               # MS / BP belong to qldpc_decode_*
        assert dev(algo=algo) == _lib.QLDPC_EINVAL
    assert dev(sf=2) == _lib.QLDPC_EINVAL and dev(ef=7) == _lib.QLDPC_EINVAL
    assert dev(batch=-1) == _lib.QLDPC_EINVAL
    assert dev(mi=0) == _lib.QLDPC_EINVAL                    # BF
    assert b"max_iter" in L.qldpc_last_error()
    assert dev(s=None) == _lib.QLDPC_EINVAL and dev(eh=None) == _lib.QLDPC_EINVAL and dev(i=None) == _lib.QLDPC_EINVAL
    assert dev(batch=0, s=None, eh=None, i=None) == _lib.QLDPC_OK
    assert dev(algo=2, batch=0, mi=0) == _lib.QLDPC_OK       # NG ignores max_iter
    assert L.qldpc_hard_decode_device(None, 3, P(syn), 0, 2, 50, P(e), 0, P(it), None, None) == _lib.QLDPC_EINVAL
    assert L.qldpc_hard_decode_host(code.handle, 5, P(syn), 2, 50, P(e), P(it), None) == _lib.QLDPC_EINVAL
    assert L.qldpc_hard_decode_host(code.handle, 3, None, 2, 50, P(e), P(it), None) == _lib.QLDPC_EINVAL
    # the schedule entry points keep refusing the two new algos
    sched = code.schedule(np.array([0, m], np.int32), np.arange(m, dtype=np.int32))
    for algo in (2, 3):
        assert L.qldpc_decode_host(code.handle, sched.handle, algo, P(syn), 2, 0.01, 5, 0.75, 1e-9, P(e), P(it),
                                   None, None) != _lib.QLDPC_OK
        buf = ctypes.create_string_buffer(64)
        assert L.qldpc_decode_kernel_name(code.handle, sched.handle, algo, buf, 64) == _lib.QLDPC_EINVAL
    assert _lib.kernel_name(code.H, None, None, "NG") == "ng_kernel"
    assert _lib.kernel_name(code.H, None, None, "BF") == "bf_kernel"


def test_codes_past_the_16_bit_tables_are_refused_with_the_limit():
    """Before any launch (and any HIP call): no device needed, nothing provoked."""
    H = np.zeros((1, 65536), np.uint8)
    H[0, :3] = 1
    for algo in ("NG", "BF"):
        with pytest.raises(NotImplementedError, match="65535"):
            decoders.decode_batch(H, np.zeros((1, 1), np.uint8), 0.0, 50, algo=algo)


@pytest.mark.skipif(_lib.device_count() > 0, reason="checks the no-device failure mode")
@pytest.mark.parametrize("decType", ["NG", "BF"])
def test_simulate_p_reaches_the_decoder_without_a_device(decType):
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("steane")
    with pytest.raises(ValueError):                          # decSchedule is still validated first
        simulator.simulate_p(Hx, Hz, 0.05, shots=4, decType=decType, decSchedule="Q", sampler="host", verbose=False)
    with pytest.raises(RuntimeError, match="no HIP device"):
        simulator.simulate_p(Hx, Hz, 0.05, shots=4, decType=decType, rngSeed=1, sampler="host", verbose=False)

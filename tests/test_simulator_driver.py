"""The Monte-Carlo driver's host path, pinned without a GPU: what simulate_p
and simulate_phenomenological hand to decoders.decode_batch (which matrix, which
prior, which keywords, in which order) and the counters they form from a
deterministic fake decoder's answers, in every mode; and simulate's resumable
sweep in its two modes. The literals were recorded before the driver was
restructured: they hold for any driver that keeps the random streams, the
batch slicing, the decode order and the counter definitions."""
import hashlib
import json

import numpy as np
import pytest

from qldpcsim_amd import codes, simulator

P = 0.15
SHOTS, BATCH, SEED = 500, 128, 7


class _R:
    def __init__(self, ehat, iters):
        self.ehat, self.iters = ehat, iters


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:12]


class _Recorder:
    """Stands in for decoders.decode_batch. The estimate is a function of the
    call's inputs alone: the first column of H equal to the syndrome if there is
    one (a single fault), else one fixed column per unsatisfied check (which
    often fails to reproduce the syndrome); on shots picked by a hash of the
    syndrome (and of the prior mask's weight, so the order of a correlated
    decode shows) one more bit is flipped. iters = 1 + syndrome weight, capped
    at max_iter."""

    def __init__(self, names):
        self.names = names                  # [(array, name)]: matrices recognised by identity
        self.calls = []
        self.batches = []
        self.prev = None

    def __call__(self, H, syn, p, max_iter, algo="MS", **kw):
        name = next((nm for a, nm in self.names if a is H), "ST")
        H = np.asarray(H)
        syn = np.asarray(syn)
        assert syn.dtype == np.uint8 and syn.shape[1:] == (H.shape[0],)
        relay = kw.get("relay")
        self.batches.append(syn.shape[0])
        self.calls.append((
            name, tuple(H.shape), p, max_iter, algo, tuple(sorted(kw)), kw.get("osd_order"), kw.get("p_masked"),
            [int(x) for x in kw["layer_ptr"]], [int(x) for x in kw["layer_rows"]],
            None if kw.get("prior") is None else _digest(kw["prior"]),
            None if relay is None else _digest(relay.leg_iters, relay.gammas, [relay.sols]),
            None if "prior_mask" not in kw else kw["prior_mask"] is self.prev.ehat))
        m, n = H.shape
        first = {}
        for j in range(n - 1, -1, -1):
            first[H[:, j].astype(np.uint8).tobytes()] = j
        percheck = H.argmax(axis=1)
        mask = kw.get("prior_mask")
        ehat = np.zeros((syn.shape[0], n), np.uint8)
        for b, s in enumerate(syn):
            j = first.get(s.tobytes())
            if not s.any():
                pass
            elif j is not None:
                ehat[b, j] = 1
            else:
                for i in np.flatnonzero(s):
                    ehat[b, percheck[i]] ^= 1
            h = int((s * np.arange(1, m + 1)).sum()) + (0 if mask is None else 3 * int(np.asarray(mask[b]).sum()))
            if h % 5 == 2:
                ehat[b, h % n] ^= 1
        iters = np.minimum(1 + syn.sum(axis=1), max_iter).astype(np.int32)
        self.prev = _R(ehat, iters)
        return self.prev


def _steane():
    Hx, Hz = codes.load_code("steane")
    return np.array(Hx), np.array(Hz)          # two objects even where the matrices are equal


def _weights_3n():
    return np.random.default_rng(5).random((3, 7)) * np.array([[1.0], [0.5], [2.0]])


def _samples(Hx, Hz):
    return simulator.sample_channel(Hx, Hz, P, 700, np.random.default_rng(9))


# name -> (function, keyword arguments; callables are evaluated on (Hx, Hz))
CASES = {
    "ms_F": ("p", dict()),
    "ms_L_osd0": ("p", dict(decSchedule="L", OSDorder=0, decIterations=30)),
    "logical": ("p", dict(logical=True)),
    "corr_XZ": ("p", dict(logical=True, correlated="XZ", decSchedule="L", OSDorder=0)),
    "corr_ZX": ("p", dict(logical=True, correlated="ZX", correlated_q1=0.4)),
    "weights_3": ("p", dict(channel_weights=[0.2, 0.1, 0.7], logical=True)),
    "weights_3n": ("p", dict(channel_weights=lambda Hx, Hz: _weights_3n(), OSDorder=0, logical=True)),
    "relay": ("p", dict(decType="RELAY", relay_legs=3, decIterations=20, relay_seed=4)),
    "bf_osd2": ("p", dict(decType="BF", OSDorder=2)),
    "bp_osd2": ("p", dict(decType="BP", OSDorder=2, decSchedule="S")),
    "samples": ("p", dict(samples=_samples, logical=True)),
    # the reference's degenerate test is over the integers: it can fire only on a qubit that no check touches,
    # so this case appends one to the pair (an error there is not exact, and every product with it is 0)
    "idle_qubit": ("p", dict(idle=True, logical=True)),
    "phenom_scalar": ("ph", dict(q=2 * P / 3, rounds=3, decSchedule="L", OSDorder=0)),
    "phenom_prior": ("ph", dict(q=0.03, rounds=3, decSchedule="L", OSDorder=0)),
}

FLOOD, ROWS = ([0, 3], [0, 1, 2]), ([0, 1, 2, 3], [0, 1, 2])     # the Steane halves' packed layers: F; L and S
ST_L = ([0, 1, 2, 4, 5, 7, 8, 9], [0, 1, 2, 3, 4, 5, 6, 7, 8])     # schedule L of the 3-round space-time matrix
P3, P0C = 0.049999999999999996, 0.05555555555555555                # p / 3; (p / 3) / (1 - 2 p / 3)
FOUR_BATCHES = [128, 128, 128, 128, 128, 128, 116, 116]


def _call(name, p, it, algo, osd, layers, shape=(3, 7), extra=(), p_masked=None, prior=None, relay=None, chained=None):
    """One recorded decode_batch call (the tuple _Recorder appends)."""
    return (name, shape, p, it, algo, tuple(sorted(("layer_ptr", "layer_rows", "osd_order") + extra)), osd, p_masked,
            layers[0], layers[1], prior, relay, chained)


def _counters(fX, fZ, exact, degen, itX, itZ, lX=None, lZ=None, ok=None, ler=None, ci=None):
    r = {"DecFailures_X": fX, "DecFailures_Z": fZ, "decSuccessExact": exact, "decSuccessDegen": degen,
         "Avg_number_of_iterations_X": itX, "Avg_number_of_iterations_Z": itZ}
    if lX is not None:
        r.update({"logicalErrors_X": lX, "logicalErrors_Z": lZ, "decSuccessLogical": ok, "logical_error_rate": ler,
                  "logical_error_rate_ci95": ci})
    return r


def _both(p, it, algo, osd, layers, **kw):
    return [_call("Hz", p, it, algo, osd, layers, **kw), _call("Hx", p, it, algo, osd, layers, **kw)]


# recorded on the driver as it stood before it was restructured (the commit that added phenomenological noise)
PLAIN = _counters(43, 35, 365, 0, 1.786, 1.944)
EXPECTED = {
    "ms_F": {"result": PLAIN, "calls": _both(P3, 99, "MS", -1, FLOOD)},
    "ms_L_osd0": {"result": PLAIN, "calls": _both(P3, 30, "MS", 0, ROWS)},
    "logical": {"result": _counters(43, 35, 365, 0, 1.786, 1.944, 39, 51, 371, 0.258,
                                    [0.2215962002228131, 0.29809398056057823]),
                "calls": _both(P3, 99, "MS", -1, FLOOD)},
    "corr_XZ": {"result": _counters(43, 44, 357, 0, 1.786, 1.944, 39, 45, 364, 0.272,
                                    [0.2348440922052204, 0.31263260704524753]),
                "calls": [_call("Hz", P3, 99, "MS", 0, ROWS),
                          _call("Hx", P0C, 99, "MS", 0, ROWS, extra=("p_masked", "prior_mask"), p_masked=0.49,
                                chained=True)]},
    "corr_ZX": {"result": _counters(37, 35, 355, 0, 1.786, 1.944, 40, 51, 362, 0.276,
                                    [0.23863813294339814, 0.31677757158337744]),
                "calls": [_call("Hx", P3, 99, "MS", -1, FLOOD),
                          _call("Hz", P0C, 99, "MS", -1, FLOOD, extra=("p_masked", "prior_mask"), p_masked=0.4,
                                chained=True)]},
    "weights_3": {"result": _counters(25, 44, 370, 0, 1.37, 2.032, 4, 62, 378, 0.244,
                                      [0.208398855460222, 0.2835048068560928]),
                  "calls": [_call("Hz", 0.045000000000000005, 99, "MS", -1, FLOOD),
                            _call("Hx", 0.11999999999999998, 99, "MS", -1, FLOOD)]},
    "weights_3n": {"result": _counters(43, 52, 199, 0, 1.858, 2.374, 52, 142, 245, 0.51,
                                       [0.4662736879310782, 0.5535738252596908]),
                   "calls": [_call("Hz", None, 99, "MS", 0, FLOOD, extra=("prior",), prior="90030d5fda55"),
                             _call("Hx", None, 99, "MS", 0, FLOOD, extra=("prior",), prior="fa9ea343b146")]},
    "relay": {"result": PLAIN,
              "calls": [_call("Hz", P3, 20, "RELAY", -1, FLOOD, extra=("relay",), relay="9a5b0eba30fe"),
                        _call("Hx", P3, 20, "RELAY", -1, FLOOD, extra=("relay",), relay="3acce6bae30b")]},
    "bf_osd2": {"result": PLAIN, "calls": _both(P3, 50, "BF", -1, FLOOD)},
    "bp_osd2": {"result": PLAIN, "calls": _both(P3, 99, "BP", -1, ROWS)},
    "samples": {"result": _counters(43, 31, 360, 0, 1.778, 1.81, 39, 62, 362, 0.276,
                                    [0.23863813294339814, 0.31677757158337744]),
                "calls": _both(P3, 99, "MS", -1, FLOOD)},
    "idle_qubit": {"result": _counters(50, 37, 296, 59, 1.742, 1.904, 92, 103, 299, 0.402,
                                       [0.359928740326145, 0.44556563040431935]),
                   "calls": _both(P3, 99, "MS", -1, FLOOD, shape=(3, 8))},
    "phenom_scalar": {"result": {"DecFailures_X": 341, "DecFailures_Z": 351, "logicalErrors_X": 32,
                                 "logicalErrors_Z": 31, "nIterAccX": 2088, "nIterAccZ": 2049, "decSuccessLogical": 32,
                                 "logical_error_rate": 0.9359999999999999,
                                 "logical_error_rate_ci95": [0.911047591162316, 0.9543039839552107],
                                 "logical_error_rate_per_round": 0.5999999999999999, "rounds": 3,
                                 "q": 0.09999999999999999, "p_data": 0.09999999999999999},
                      "calls": [_call("ST", 0.09999999999999999, 99, "MS", 0, ST_L, shape=(9, 27))] * 2},
    "phenom_prior": {"result": {"DecFailures_X": 301, "DecFailures_Z": 306, "logicalErrors_X": 36,
                                "logicalErrors_Z": 38, "nIterAccX": 1910, "nIterAccZ": 1891, "decSuccessLogical": 57,
                                "logical_error_rate": 0.886,
                                "logical_error_rate_ci95": [0.8551509101576845, 0.9109630990059973],
                                "logical_error_rate_per_round": 0.5151192414160121, "rounds": 3, "q": 0.03,
                                "p_data": 0.09999999999999999},
                     "calls": [_call("ST", None, 99, "MS", 0, ST_L, shape=(9, 27), extra=("prior",),
                                     prior="1ec71e34aa14")] * 2},
}


def _run(name, monkeypatch):
    Hx, Hz = _steane()
    fn, kw = CASES[name]
    kw = {k: (v(Hx, Hz) if callable(v) else v) for k, v in kw.items()}
    if kw.pop("idle", False):
        Hx, Hz = (np.hstack([H, np.zeros((H.shape[0], 1), H.dtype)]) for H in (Hx, Hz))
    rec = _Recorder([(Hx, "Hx"), (Hz, "Hz")])
    monkeypatch.setattr(simulator.decoders, "decode_batch", rec)
    common = dict(shots=SHOTS, rngSeed=SEED, batch_size=BATCH, sampler="host", verbose=False)
    if fn == "p":
        res = simulator.simulate_p(Hx, Hz, P, **common, **kw)
    else:
        res = simulator.simulate_phenomenological(Hx, Hz, P, **common, **kw)
    # every batch makes the same two calls; only the batch size differs
    assert rec.calls == rec.calls[:2] * (len(rec.calls) // 2)
    return {"result": res, "batches": rec.batches, "calls": rec.calls[:2]}


@pytest.mark.parametrize("name", list(CASES))
def test_host_driver_is_pinned(name, monkeypatch):
    got = _run(name, monkeypatch)
    want = EXPECTED[name]
    assert got["batches"] == FOUR_BATCHES                       # three full batches and a tail, two halves each
    assert got["calls"] == want["calls"]
    assert got["result"] == want["result"]
    assert list(got["result"]) == list(want["result"])          # key order too


def test_every_counter_moves_in_some_case():
    """The fake decoder is no identity: across the cases each counter is
    non-zero somewhere, so a swapped half or a lost batch shows."""
    keys = simulator.COUNTER_KEYS[:4] + simulator.LOGICAL_KEYS + ("Avg_number_of_iterations_X",
                                                                  "Avg_number_of_iterations_Z")
    for k in keys:
        assert any(e["result"].get(k, 0) for e in EXPECTED.values()), k
    for k in simulator.PHENOM_KEYS:
        assert any(EXPECTED[c]["result"][k] for c in ("phenom_scalar", "phenom_prior")), k


# ---------------------------------------------------------------- simulate's resumable sweep

BASE_META = {"shots": 100, "decType": "MS", "decIterations": 99, "decSchedule": "F", "OSDorder": -1, "rngSeed": 1,
             "world": 1, "sampler": "host"}
# the results file's run parameters (without the two paths) and what every point is called with, as recorded
SWEEP_META = {
    "plain": {**BASE_META, "logical": True, "correlated": "ZX", "correlated_q1": 0.45},
    "relay_bias": {**BASE_META, "decType": "RELAY", "relay_legs": 4, "relay_leg_iters": 60, "relay_sols": 1,
                   "relay_gamma0": 0.125, "relay_gamma_range": [-0.24, 0.66], "relay_seed": 3, "bias": 2.0},
    "weights": {**BASE_META, "channel_weights": {
        "shape": [3], "sha256": "3770e6cd83221d60f3816a323de380c1fdd4b0e696bd8dd593950740135f95c4"}},
    "rounds": {**BASE_META, "rounds": 3, "q": None},
    "rounds_q": {**BASE_META, "decType": "BP", "OSDorder": 1, "rounds": 2, "q": 0.01},
}
POINT_KW = ("OSDorder", "batch_size", "decIterations", "decSchedule", "decType", "rngSeed", "sampler", "shots",
            "verbose")
RELAY_KW = ("relay_gamma0", "relay_gamma_range", "relay_leg_iters", "relay_legs", "relay_seed", "relay_sols")
SWEEP_CALLS = {
    "plain": (tuple(sorted(POINT_KW + ("correlated", "correlated_q1", "logical"))),),
    "relay_bias": (tuple(sorted(POINT_KW + RELAY_KW + ("channel_weights",))),),
    "weights": (tuple(sorted(POINT_KW + ("channel_weights",))),),
    "rounds": (0.006666666666666667, 3, POINT_KW),
    "rounds_q": (0.01, 2, POINT_KW),
}


def _fake_point(log):
    def simulate_p(Hx, Hz, p, **kw):
        log.append(("p", p, tuple(sorted(kw))))
        return {"DecFailures_X": 1, "DecFailures_Z": 2, "decSuccessExact": 90, "decSuccessDegen": 0,
                "Avg_number_of_iterations_X": 1.5, "Avg_number_of_iterations_Z": p, "logicalErrors_X": 3,
                "logicalErrors_Z": 4, "decSuccessLogical": 93, "logical_error_rate": 0.07,
                "logical_error_rate_ci95": [0.03, 0.14]}

    def simulate_phenomenological(Hx, Hz, p, q, rounds, **kw):
        log.append(("ph", p, q, rounds, tuple(sorted(kw))))
        return {"DecFailures_X": 1, "DecFailures_Z": 2, "logicalErrors_X": 3, "logicalErrors_Z": 4, "nIterAccX": 5,
                "nIterAccZ": 6, "decSuccessLogical": 93, "logical_error_rate": 0.07,
                "logical_error_rate_ci95": [0.03, 0.14], "logical_error_rate_per_round": 0.02, "rounds": rounds,
                "q": q, "p_data": 2 * p / 3}
    return simulate_p, simulate_phenomenological


SWEEPS = {
    "plain": dict(logical=True, correlated="ZX", correlated_q1=0.45),
    "relay_bias": dict(decType="RELAY", relay_legs=4, relay_seed=3, bias=2.0),
    "weights": dict(channel_weights=[0.25, 0.25, 0.5]),
    "rounds": dict(rounds=3),
    "rounds_q": dict(rounds=2, meas_error=0.01, decType="BP", OSDorder=1),
}


@pytest.mark.parametrize("mode", list(SWEEPS))
def test_sweep_resumes_in_every_mode(mode, tmp_path, monkeypatch, capsys):
    log, seen = [], []
    for f, name in zip(_fake_point(log), ("simulate_p", "simulate_phenomenological")):
        monkeypatch.setattr(simulator, name, f)
    Hx, Hz = codes.load_code("steane")
    fx, fz, f = str(tmp_path / "Hx.npy"), str(tmp_path / "Hz.npy"), str(tmp_path / "res.json")
    np.save(fx, Hx)
    np.save(fz, Hz)
    kw = dict(shots=100, rngSeed=1, verbose=False, return_results=True, resultsFile=f, sampler="host",
              on_point=lambda pT, r, sec: seen.append((pT, r, sec >= 0)), **SWEEPS[mode])
    a = simulator.simulate(fx, fz, [0.01, 0.02], **kw)
    which = "ph" if "rounds" in SWEEPS[mode] else "p"
    assert [(c[0], c[1]) for c in log] == [(which, 0.01), (which, 0.02)]
    assert [s[0] for s in seen] == [0.01, 0.02] and [s[1] for s in seen] == a and all(s[2] for s in seen)
    b = simulator.simulate(fx, fz, [0.02, 0.05, 0.01], **kw)                 # two points are in the file
    assert [c[1] for c in log] == [0.01, 0.02, 0.05] and [s[0] for s in seen] == [0.01, 0.02, 0.05]
    assert b[0] == a[1] and b[2] == a[0] and len(b) == 3
    assert simulator.simulate(fx, fz, [0.05], **{**kw, "return_results": False}) is None
    assert len(log) == 3
    with pytest.raises(ValueError, match="different run"):
        simulator.simulate(fx, fz, [0.01], **{**kw, "shots": 200})
    assert len(log) == 3 and len(seen) == 3
    doc = json.load(open(f))
    assert sorted(doc["results"]) == ["0.01", "0.02", "0.05"]
    meta = doc["meta"]
    assert (meta.pop("Hx"), meta.pop("Hz")) == (fx, fz)
    assert meta == SWEEP_META[mode] and list(meta) == list(SWEEP_META[mode])
    assert log[0][2:] == SWEEP_CALLS[mode]                                   # what every point is called with
    out = capsys.readouterr().out
    assert ("PHENOMENOLOGICAL NOISE" in out) == (which == "ph")
    assert ("SIMULATION RESULTS" in out) == (which == "p")
    assert ("LOGICAL ERROR RATES" in out) == (mode == "plain")

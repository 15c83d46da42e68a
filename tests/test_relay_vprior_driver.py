"""What simulate_p and simulate_dem hand to decoders.decode_batch under
relay_priors=True, pinned without a GPU in the style of
tests/test_simulator_driver.py: decode_batch is replaced by a recorder with a
deterministic answer; a half with unequal priors arrives as algo "RELAY" with
the row and its cost in the RelayConfig (never as prior=), a half with equal
priors as the scalar relay call it has always been."""
import hashlib

import numpy as np
import pytest

import dem_model as dm
from qldpcsim_amd import codes, simulator

P, SHOTS, BATCH, SEED = 0.15, 300, 128, 7


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    return h.hexdigest()[:12]


class _R:
    def __init__(self, ehat, iters):
        self.ehat, self.iters = ehat, iters


class _Recorder:
    """Stands in for decoders.decode_batch: records the call and answers with
    one fixed column per unsatisfied check, iters = 1 + syndrome weight."""

    def __init__(self):
        self.calls = []

    def __call__(self, H, syn, p, max_iter, algo="MS", **kw):
        H, syn = np.asarray(H), np.asarray(syn)
        assert syn.dtype == np.uint8 and syn.shape[1:] == (H.shape[0],)
        relay = kw.get("relay")
        self.calls.append((tuple(H.shape), p, algo, tuple(sorted(kw)), [int(x) for x in kw["layer_ptr"]],
                           list(relay.leg_iters), _digest(relay.gammas), relay.sols,
                           None if relay.prior is None else _digest(relay.prior), relay.cost, len(syn)))
        ehat = np.zeros((len(syn), H.shape[1]), np.uint8)
        percheck = H.argmax(axis=1)
        for b, s in enumerate(syn):
            for i in np.flatnonzero(s):
                ehat[b, percheck[i]] ^= 1
        return _R(ehat, (1 + syn.sum(axis=1)).astype(np.int32))


def _gammas(seed, n, legs, tables):
    """The driver's tables: one generator, the Hz-decoded half first."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(tables):
        g = np.empty((legs, n))
        g[0] = 0.125
        g[1:] = rng.uniform(-0.24, 0.66, (legs - 1, n))
        out.append(g)
    return out


KEYS = ("layer_ptr", "layer_rows", "osd_order", "relay")       # the host path's keywords: no prior=


@pytest.mark.parametrize("cost", [None, "hamming"])
def test_simulate_p_hands_the_rows_to_the_relay(cost, monkeypatch):
    """Unequal marginals in the Z half only: the X half (Hz) is the scalar
    call, the Z half (Hx) carries p (w_Z + w_Y); relay_cost=None is "prior"
    there and "hamming" in the scalar half."""
    Hx, Hz = (np.array(h) for h in codes.load_code("steane"))
    n = Hx.shape[1]
    w = np.array([[0.2] * n, [0.1] * n, np.linspace(0.1, 0.7, n)])
    rec = _Recorder()
    monkeypatch.setattr(simulator.decoders, "decode_batch", rec)
    res = simulator.simulate_p(Hx, Hz, P, shots=SHOTS, rngSeed=SEED, batch_size=BATCH, sampler="host", verbose=False,
                               decType="RELAY", decIterations=20, relay_legs=3, relay_leg_iters=9, relay_sols=2,
                               relay_seed=4, channel_weights=w, relay_priors=True, relay_cost=cost)
    GX, GZ = _gammas(4, n, 3, 2)
    qZ = P * (w[2] + w[1])
    want = []
    for B in (128, 128, 44):
        want.append(((3, 7), P * 0.30000000000000004, "RELAY", KEYS, [0, 3], [20, 9, 9], _digest(GX), 2, None,
                     "hamming", B))
        want.append(((3, 7), None, "RELAY", KEYS, [0, 3], [20, 9, 9], _digest(GZ), 2, _digest(qZ), cost or "prior", B))
    assert rec.calls == want
    assert res["Avg_number_of_iterations_X"] > 1 and res["Avg_number_of_iterations_Z"] > 1


def test_simulate_p_without_the_flag_is_the_scalar_call(monkeypatch):
    """Equal marginals with and without relay_priors: the same two scalar
    calls, a RelayConfig without a row."""
    Hx, Hz = (np.array(h) for h in codes.load_code("steane"))
    seen = []
    for flag in ({}, {"relay_priors": True}, {"relay_priors": True, "relay_cost": "hamming"}):
        rec = _Recorder()
        monkeypatch.setattr(simulator.decoders, "decode_batch", rec)
        simulator.simulate_p(Hx, Hz, P, shots=100, rngSeed=SEED, batch_size=BATCH, sampler="host", verbose=False,
                             decType="RELAY", decIterations=20, relay_legs=3, relay_seed=4,
                             channel_weights=[0.2, 0.1, 0.7], **flag)
        assert [c[8:10] for c in rec.calls] == [(None, "hamming")] * 2 and rec.calls[0][1] is not None
        seen.append(rec.calls)
    assert seen[0] == seen[1] == seen[2]


@pytest.mark.parametrize("cost", [None, "hamming", "prior"])
def test_simulate_dem_hands_the_mechanisms_to_the_relay(cost, monkeypatch):
    H, L, _, _ = dm.edge_dem(20, 2, 41)
    pr = np.exp(np.random.default_rng(8).uniform(np.log(1e-3), np.log(0.3), H.shape[1]))
    from qldpcsim_amd import dem as D
    rec = _Recorder()
    monkeypatch.setattr(simulator.decoders, "decode_batch", rec)
    res = simulator.simulate_dem(D.Dem(H, L, pr), shots=SHOTS, decType="RELAY", decIterations=12, rngSeed=SEED,
                                 batch_size=BATCH, sampler="host", verbose=False, relay_priors=True, relay_cost=cost,
                                 relay_legs=4, relay_leg_iters=5, relay_sols=3, relay_seed=6)
    G, = _gammas(6, 41, 4, 1)
    call = lambda B, keys: ((20, 41), None, "RELAY", keys, [0, 20], [12, 5, 5, 5], _digest(G), 3, _digest(pr),  # noqa: E731
                            cost or "prior", B)
    # the all-zero row that meets the relay's limits before a shot is drawn, then the batches
    assert rec.calls == [call(1, ("layer_ptr", "layer_rows", "relay"))] + [call(B, KEYS) for B in (128, 128, 44)]
    assert res["DecFailures"] + res["logicalErrors"] + res["decSuccess"] == SHOTS


def test_simulate_dem_with_equal_priors_is_the_scalar_call(monkeypatch):
    H, L, _, _ = dm.edge_dem(20, 2, 41)
    from qldpcsim_amd import dem as D
    rec = _Recorder()
    monkeypatch.setattr(simulator.decoders, "decode_batch", rec)
    simulator.simulate_dem(D.Dem(H, L, np.full(41, 0.03)), shots=50, decType="RELAY", decIterations=12, rngSeed=SEED,
                           sampler="host", verbose=False, relay_priors=True)
    assert [(c[1], c[8], c[9]) for c in rec.calls] == [(0.03, None, "hamming")] * 2
    assert rec.calls[-1][5] == [12] + [60] * 10

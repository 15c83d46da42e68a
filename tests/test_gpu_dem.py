"""Detector error models on the GPU: dem_sample_kernel and dem_count_kernel
(qldpc_dem_sample / qldpc_dem_count) bit for bit against the independent NumPy
model (tests/dem_model.py) on word-edge models and against the
phenomenological kernels on phenomenological models, then simulate_dem
against simulate_phenomenological's X half. Every comparison is integer
equality."""
import functools

import numpy as np
import pytest

import dem_model as dm
import phenom_model as pm
from test_phenom_model import half

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
SHOT0 = 2 ** 32 - 100          # 257 shots from here cross shot_lo's wrap
B = 257
# one more than the issue's five: 64 (ceil(M/64) + ceil(K/64)) > 65536 selects the kernels' 32-bit lists
WIDE = (65600, 1, 70)
HALVES = ("steane", "shor_x", "shor_z", "LP04_0")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _u64(t):
    return _np(t).view(np.uint64)


def _key(seed, rank=0):
    return int(np.random.SeedSequence([seed, rank]).generate_state(1, np.uint64)[0])


@functools.lru_cache(maxsize=None)
def _edge(shape):
    """(Dem, where, model det / obs / fired of B shots from SHOT0, crafted
    estimates, the class each must have, iteration counts, model classes and
    flips) of one word-edge model; computed once."""
    from qldpcsim_amd import dem as D
    H, L, pr, where = dm.edge_dem(*shape)
    det, obs, fired = dm.sample(H, L, pr, SEED, SHOT0, B)
    rng = np.random.default_rng(23)
    ehat, want = dm.craft(rng, H, L, fired, where)
    iters = rng.integers(1, 60, B).astype(np.int32)
    cls, F = dm.classify(H, L, det, obs, ehat)
    return D.Dem(H, L, pr), where, det, obs, fired, ehat, want, iters, cls, F


def _source(dem, seed=SEED, shot0=SHOT0):
    from qldpcsim_amd import simulator
    return simulator.DeviceDem(dem, _dev(), seed, shot0)


@pytest.mark.parametrize("shape", dm.EDGE_SHAPES + (WIDE,), ids=lambda s: "x".join(map(str, s)))
def test_sampler_equals_the_model_on_word_edge_models(shape):
    """Detectors in both formats, observable words and the fired row of
    batches of 1, 3 and 257 shots from shot 2^32 - 100, bit for bit (padding
    bits zero). Every model from 64 columns up holds an all-zero column, an
    observable-only column (K > 0), a p = 0 column that never fires, a
    p = 1 - 2^-20 column that fires in every shot, an empty last row and a
    detector and an observable row of degree min(300, N - 8): 300 on the
    4097-column model, as many as there are free columns on the smaller ones.
    The instance's name is the one for the row's width."""
    import torch
    from qldpcsim_amd import _lib
    dem, where, det, obs, fired = _edge(shape)[:5]
    M, K, N = shape
    wide = shape == WIDE
    if N >= 64:
        assert not fired[:, where["p0"]].any() and fired[:, where["p1"]].all()
        assert not dem.H[:, where["zero"]].any() and not dem.L[:, where["zero"]].any() and fired[:, where["zero"]].any()
        assert not dem.H[where["empty_row"]].any() and not det[:, where["empty_row"]].any()
        assert dem.H[where["heavy_row"][0]].sum() == where["heavy_row"][1] == min(300, N - 8)
        assert dem.priors.min() == 0.0 and 1e-6 <= np.sort(dem.priors)[1] and dem.priors.max() == 1 - 2.0 ** -20
    if N >= 64 and K:
        only = where["obs_only"]
        assert not dem.H[:, only].any() and dem.L[:, only].sum() == 1 and fired[:, only].any()
        # (the special columns may add to that row)
        assert dem.L[where["heavy_obs"][0]].sum() >= where["heavy_obs"][1] == min(300, N - 8)
    if shape == (130, 3, 4097):
        assert dem.H[0].sum() == 300 and dem.L[2].sum() >= 300
    assert fired.any() and det.any() and (K == 0 or obs.any())
    for kind in ("sample", "count"):
        assert _lib.dem_kernel_name(_source(dem).table, kind) == f"dem_{kind}_kernel<{32 if wide else 16}>"
    for nb in (1, 3, B):
        for bits in (False, True):
            d, o, f = _source(dem).sample(nb, bits=bits, want_fired=True)
            assert d.dtype == (torch.int64 if bits else torch.uint8) and tuple(o.shape) == (nb, (K + 63) // 64)
            if bits:
                assert np.array_equal(_u64(d), pm.pack_words(det[:nb])), ("detector words", nb)
            else:
                assert np.array_equal(_np(d), det[:nb]), ("detector bytes", nb)
            assert np.array_equal(_u64(o), pm.pack_words(obs[:nb])), ("observable words", nb, bits)
            assert np.array_equal(_u64(f), pm.pack_words(fired[:nb])), ("fired row", nb, bits)
    # the same shots in two calls, without the fired row
    s = _source(dem)
    d1, o1 = s.sample(100)
    d2, o2 = s.sample(157)
    assert s.shot == SHOT0 + B
    assert np.array_equal(np.concatenate([_np(d1), _np(d2)]), det)
    assert np.array_equal(np.concatenate([_u64(o1), _u64(o2)]), pm.pack_words(obs))


@pytest.mark.parametrize("shape", dm.EDGE_SHAPES + (WIDE,), ids=lambda s: "x".join(map(str, s)))
def test_counter_equals_the_model_on_word_edge_models(shape):
    """The four counters, the classes and the flip words of batches of 1, 3
    and 257 crafted estimates, in both detector and both estimate formats.
    The estimates are built so that every class occurs (dem_model.craft: with
    K = 0, or on the one-column model, no estimate can be class 1, and there
    classes 0 and 2 occur): asserted on the model's own classes first."""
    import torch
    from qldpcsim_amd import decoders
    dem, where, det, obs, fired, ehat, want, iters, cls, F = _edge(shape)
    M, K, N = shape
    assert np.array_equal(cls, want)
    for nb in (3, B):
        assert set(cls[:nb]) == ({0, 1, 2} if (K and N >= 64) else {0, 2}), (nb, set(cls[:nb]))
    dev = _dev()
    tn = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    src = _source(dem)
    for nb in (1, 3, B):
        t_det, t_eh, t_it = tn(det[:nb]), tn(ehat[:nb]), tn(iters[:nb])
        t_obs = tn(pm.pack_words(obs[:nb]).view(np.int64))
        c = dm.counters(cls[:nb], iters[:nb])
        wv = [c["failures"], c["logical_errors"], c["successes"], c["iterations"]]
        for d_ in (t_det, decoders.pack_bits(t_det)):
            for e_ in (t_eh, decoders.pack_bits(t_eh)):
                acc, gc, gf = src.count_device(d_, t_obs, e_, t_it, want_shots=True)
                assert np.array_equal(_np(gc), cls[:nb]), nb
                assert np.array_equal(_u64(gf), pm.pack_words(F[:nb])), nb
                assert acc.cpu().tolist() == wv
                src.count_device(d_, t_obs, e_, t_it, acc)               # accumulates, no per-shot outputs
                assert acc.cpu().tolist() == [2 * v for v in wv]
    with pytest.raises(ValueError):
        src.count_device(tn(det), tn(pm.pack_words(obs).view(np.int64)), tn(ehat), tn(iters[:5]))


def test_dense_words_take_the_lane_walk():
    """More than 16 set columns in a word of 64 select the kernels' other walk
    (every lane its own column): a model whose every prior is 0.6, and random
    dense estimates, against the model in both formats."""
    import torch
    from qldpcsim_amd import decoders, dem as D
    H, L, _, _ = dm.edge_dem(65, 65, 129)
    pr = np.full(129, 0.6)
    det, obs, fired = dm.sample(H, L, pr, SEED, SHOT0, 40)
    words = pm.pack_words(fired)
    assert min(bin(int(x)).count("1") for x in words[:, :2].ravel()) > 16
    src = _source(D.Dem(H, L, pr))
    d, o, f = src.sample(40, want_fired=True)
    assert np.array_equal(_np(d), det) and np.array_equal(_u64(o), pm.pack_words(obs))
    assert np.array_equal(_u64(f), words)
    rng = np.random.default_rng(3)
    ehat = rng.integers(0, 2, (40, 129), dtype=np.uint8)
    ehat[::2] = fired[::2]                                   # every other shot class 0
    iters = rng.integers(1, 60, 40).astype(np.int32)
    cls, F = dm.classify(H, L, det, obs, ehat)
    assert set(cls) == {0, 2}
    tn = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=_dev())  # noqa: E731
    for e_ in (tn(ehat), decoders.pack_bits(tn(ehat))):
        acc, gc, gf = src.count_device(d, o, e_, tn(iters), want_shots=True)
        assert np.array_equal(_np(gc), cls) and np.array_equal(_u64(gf), pm.pack_words(F))
        c = dm.counters(cls, iters)
        assert acc.cpu().tolist() == [c["failures"], c["logical_errors"], c["successes"], c["iterations"]]


# ---------------------------------------------------------------------------
# phenomenological models: the existing kernels are the yardstick
# ---------------------------------------------------------------------------
P_DATA, Q = 0.11, 0.07


@pytest.mark.parametrize("T", (1, 2, 3))
@pytest.mark.parametrize("name", HALVES)
def test_sampler_and_counter_equal_the_phenomenological_kernels(name, T):
    """Same seed and shot0: dem_sample's detectors and fired row equal
    phenom_sample's, its observable words equal L E of that sampler's E;
    dem_count's classes, flip words and counters equal phenom_count's on the
    same crafted estimates; and the fired row equals qldpc_channel_sample_vec's
    errX on the materialised matrix (N <= 4096 on all of these)."""
    import torch
    from qldpcsim_amd import decoders, dem as D, simulator, spacetime
    H, L, Hstab, Lop = half(name)
    m, n = H.shape
    model = D.phenomenological_dem(H, L, T, P_DATA, Q)
    ph = simulator.DevicePhenomHalf(H, L, T, _dev(), SEED, SHOT0)
    for bits in (False, True):
        ph.shot = SHOT0
        d0, E, f0 = ph.sample(P_DATA, Q, B, bits=bits, want_fired=True)
        d1, o1, f1 = _source(model).sample(B, bits=bits, want_fired=True)
        assert torch.equal(d0, d1) and torch.equal(f0, f1)
    Eb = pm.unpack_words(_u64(E), n)
    assert Eb.any() and np.array_equal(_u64(o1), pm.pack_words(pm.mod2(Eb, L % 2)))
    assert model.num_errors <= 4096
    S = H if T == 1 else spacetime.spacetime_matrix(H, T)
    ch = simulator.DeviceChannel(S, S, _dev(), SEED, SHOT0)
    ch.set_probs(np.stack([model.priors, np.zeros_like(model.priors), np.zeros_like(model.priors)]))
    assert torch.equal(ch.sample(0.0, B)[2], f1)
    # the counter, on estimates of every class
    fired = pm.unpack_words(_u64(f1), model.num_errors)
    rng = np.random.default_rng(17)
    ehat, rec = pm.craft(rng, H, Hstab, Lop, T, fired)
    t_eh = torch.as_tensor(ehat, device=_dev())
    t_it = torch.as_tensor(rng.integers(1, 60, B).astype(np.int32), device=_dev())
    for e_ in (t_eh, decoders.pack_bits(t_eh)):
        a0, c0, fl0, _ = ph.count_device(d0, E, e_, t_it, want_shots=True)
        a1, c1, fl1 = _source(model).count_device(d1, o1, e_, t_it, want_shots=True)
        assert torch.equal(c0, c1) and torch.equal(fl0, fl1) and a0.cpu().tolist() == a1.cpu().tolist()
    assert set(_np(c1)) == {0, 1, 2}


# ---------------------------------------------------------------------------
# simulate_dem against simulate_phenomenological's X half
# ---------------------------------------------------------------------------
SHOTS = 4096
CASES = {
    "ms_scalar": dict(q=0.02, kw=dict(decType="MS", decIterations=30)),
    "ms_vector": dict(q=0.01, kw=dict(decType="MS", decIterations=30)),
    "bp_layered": dict(q=0.01, kw=dict(decType="BP", decIterations=20, decSchedule="L")),
    "ms_osd0": dict(q=0.01, kw=dict(decType="MS", decIterations=4, OSDorder=0)),
    "ms_osd_cs10": dict(q=0.01, kw=dict(decType="MS", decIterations=4, OSDorder=10, osd_method="cs")),
}


def _x_half_dem(T, p, q):
    from qldpcsim_amd import codes, dem as D, logicals
    Hx, Hz = codes.load_code("LP04_0")
    return Hx, Hz, D.phenomenological_dem(Hz, logicals.css_logicals(Hx, Hz)[1], T, 2 * p / 3, q)


@pytest.mark.parametrize("T", (2, 3))
@pytest.mark.parametrize("case", sorted(CASES))
def test_simulate_dem_equals_the_x_half_of_simulate_phenomenological(case, T):
    """The X-half model (Hz, Lz, p_data = 2p/3) with the same rngSeed: the
    matrix, the prior row and the Philox key are simulate_phenomenological's,
    so DecFailures, logicalErrors and nIterAcc equal its _X counters exactly.
    q = 2p/3 takes the scalar entry point, q = 0.01 decode_vprior_kernel."""
    from qldpcsim_amd import simulator
    p, q, kw = 0.03, CASES[case]["q"], CASES[case]["kw"]
    Hx, Hz, model = _x_half_dem(T, p, q)
    assert (model.uniform_prior() is not None) == (case == "ms_scalar")
    common = dict(shots=SHOTS, rngSeed=11, sampler="device", verbose=False, **kw)
    want = simulator.simulate_phenomenological(Hx, Hz, p, q, T, **common)
    got = simulator.simulate_dem(model, **common)
    assert (got["DecFailures"], got["logicalErrors"], got["nIterAcc"]) == \
        (want["DecFailures_X"], want["logicalErrors_X"], want["nIterAccX"])
    assert got["decSuccess"] == SHOTS - got["DecFailures"] - got["logicalErrors"] and 0 < got["decSuccess"] < SHOTS
    assert got["nIterAcc"] > SHOTS
    assert got["logical_error_rate"] == 1. - got["decSuccess"] / SHOTS
    assert got["logical_error_rate_ci95"] == simulator.wilson_interval(SHOTS - got["decSuccess"], SHOTS)
    assert (got["detectors"], got["errors"], got["observables"]) == (*model.H.shape, model.L.shape[0])
    if "OSDorder" in kw:
        assert got["DecFailures"] == 0                       # OSD reproduces every detector
        plain = {k: v for k, v in common.items() if k not in ("OSDorder", "osd_method")}
        assert simulator.simulate_dem(model, **plain)["DecFailures"] > 0
    # the batching does not change a shot
    assert simulator.simulate_dem(model, batch_size=1000, **common) == got


def _host_decode(model, det, algo, iters):
    from qldpcsim_amd import decoders
    if model.uniform_prior() is not None:
        r = decoders.decode_batch(model.H, det, model.uniform_prior(), iters, algo=algo)
    else:
        r = decoders.decode_batch(model.H, det, None, iters, algo=algo, prior=model.priors)
    return r.ehat, r.iters


def test_simulate_dem_host_sampler_equals_a_model_loop():
    """sampler="host" on the steane X-half model, T = 2, 300 shots in batches
    of 128: a hand-written loop over the same generator, thresholds and
    classes from the model. The host decode entry stages through the device,
    hence the gpu mark."""
    from qldpcsim_amd import dem as D, simulator
    H, L = half("steane")[:2]
    model = D.phenomenological_dem(H, L, 2, 0.06, 0.03)
    shots, seed, bs = 300, 8, 128
    rng = np.random.default_rng([seed, 0])
    tot, done = np.zeros(4, np.int64), 0
    while done < shots:
        nb = min(bs, shots - done)
        u = rng.integers(0, 1 << 32, (nb, model.num_errors), dtype=np.uint64)
        fired = (u < dm.thresholds(model.priors)).astype(np.uint8)
        det, obs = pm.mod2(fired, model.H), pm.mod2(fired, model.L)
        ehat, it = _host_decode(model, det, "MS", 25)
        c = dm.counters(dm.classify(model.H, model.L, det, obs, ehat)[0], it)
        tot += (c["failures"], c["logical_errors"], c["successes"], c["iterations"])
        done += nb
    got = simulator.simulate_dem(model, shots=shots, decType="MS", decIterations=25, rngSeed=seed, batch_size=bs,
                                 sampler="host", verbose=False)
    assert [got[k] for k in simulator.DEM_KEYS] == tot.tolist()
    assert 0 < got["decSuccess"] < shots


def test_cli_two_ranks(tmp_path):
    """`torchrun -m qldpcsim_amd.simulator --dem model.npz` with two gloo ranks
    on the one GPU: the all-reduced counters equal a single-process loop over
    both ranks' shares (model sampler with each rank's key, host decode entry,
    model classes), and --results holds the one record."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from qldpcsim_amd import simulator
    _, _, model = _x_half_dem(2, 0.03, 0.01)
    f = tmp_path / "model.npz"
    np.savez(f, H=model.H, L=model.L, priors=model.priors)
    res = tmp_path / "res.json"
    shots, seed, it = 501, 9, 30
    env = dict(os.environ, QLDPC_SIM_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29551", "-m", "qldpcsim_amd.simulator",
                        "--dem", str(f), "--shots", str(shots), "--decIterations", str(it), "--rngSeed", str(seed),
                        "--batch", "100", "--results", str(res)], cwd=ROOT, capture_output=True, text=True,
                       timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("DETECTOR ERROR MODEL") == 1 and "SIMULATION RESULTS" not in r.stdout
    doc = json.loads(res.read_text())
    assert doc["meta"]["world"] == 2 and doc["meta"]["dem"] == str(f) and doc["meta"]["sampler"] == "device"
    tot = np.zeros(4, np.int64)
    for rank in range(2):
        my = shots // 2 + (1 if rank < shots % 2 else 0)
        det, obs, _ = dm.sample(model.H, model.L, model.priors, _key(seed, rank), 0, my)
        ehat, its = _host_decode(model, det, "MS", it)
        c = dm.counters(dm.classify(model.H, model.L, det, obs, ehat)[0], its)
        tot += (c["failures"], c["logical_errors"], c["successes"], c["iterations"])
    assert [doc["result"][k] for k in simulator.DEM_KEYS] == tot.tolist()
    assert doc["result"]["logical_error_rate"] == 1. - int(tot[2]) / shots


def test_vector_prior_refusal_draws_no_shot(monkeypatch):
    """MS under per-column priors takes rows of at most 32 entries: a model
    with a detector row of degree 33 raises NotImplementedError when the
    launch is planned, and the source's shot counter is still where it began.
    BP decodes the same model."""
    from qldpcsim_amd import dem as D, simulator
    rng = np.random.default_rng(5)
    H = np.zeros((12, 40), np.uint8)
    H[0, :33] = 1
    for j in range(40):
        H[1 + rng.choice(11, 2, replace=False), j] = 1
    L = np.zeros((1, 40), np.uint8)
    L[0, ::3] = 1
    model = D.Dem(H, L, np.linspace(0.001, 0.02, 40))
    made = []

    class Recording(simulator.DeviceDem):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)

    monkeypatch.setattr(simulator, "DeviceDem", Recording)
    with pytest.raises(NotImplementedError):
        simulator.simulate_dem(model, shots=64, decType="MS", decIterations=10, rngSeed=3, sampler="device",
                               verbose=False)
    assert len(made) == 1 and made[0].shot == 0
    got = simulator.simulate_dem(model, shots=64, decType="BP", decIterations=10, rngSeed=3, sampler="device",
                                 verbose=False)
    assert made[1].shot == 64 and got["DecFailures"] + got["logicalErrors"] + got["decSuccess"] == 64

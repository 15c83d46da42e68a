"""Phenomenological noise on the GPU: phenom_sample_kernel and
phenom_count_kernel (qldpc_phenom_sample / qldpc_phenom_count) bit for bit
against the independent NumPy model (tests/phenom_model.py) and against the
existing generic sampler on the materialised space-time matrix, then
simulate_phenomenological end to end. Every comparison is integer equality."""
import functools

import numpy as np
import pytest

import phenom_model as pm
from test_phenom_model import KERNEL_DEGREE, SHAPES, half

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
SHOT0 = 2 ** 32 - 100          # 257 shots from here cross shot_lo's wrap
B = 257
P_DATA, Q = 0.11, 0.07


def _dev():
    import torch
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _words(t, k):
    """int64 word tensor [B, W] -> uint8 [B, k]."""
    return pm.unpack_words(_np(t).view(np.uint64), k)


def _half_dev(name, T, seed=SEED, shot0=SHOT0):
    from qldpcsim_amd import simulator
    H, L = half(name)[:2]
    return simulator.DevicePhenomHalf(H, L, T, _dev(), seed, shot0)


@functools.lru_cache(maxsize=None)
def _model(name, T, p_data=P_DATA, q=Q):
    return pm.sample(half(name)[0], T, p_data, q, SEED, SHOT0, B)


@pytest.mark.parametrize("T", (1, 2, 3))
@pytest.mark.parametrize("name", SHAPES)
def test_sampler_equals_the_model(name, T):
    """Detectors (both formats), E and the fired row of 257 shots from shot
    2^32 - 100, bit for bit; one call equals calls of 100 + 157; p_data = 0
    gives E = 0 and q = 0 fires no measurement column."""
    import torch
    from qldpcsim_amd import _lib
    H = half(name)[0]
    m, n = H.shape
    assert _lib.phenom_kernel_name(H, "sample", 0) == f"phenom_sample_kernel<{KERNEL_DEGREE[name]}>"
    det, E, fired = _model(name, T)
    assert fired.any() and E.any() and (T == 1 or fired[:, ~pm.is_data(n, m, T)].any())
    for bits in (False, True):
        h = _half_dev(name, T)
        d, e, f = h.sample(P_DATA, Q, B, bits=bits, want_fired=True)
        assert d.dtype == (torch.int64 if bits else torch.uint8)
        gd = _words(d, T * m) if bits else _np(d)
        assert np.array_equal(gd, det), ("detectors", bits)
        assert np.array_equal(_np(e).view(np.uint64), pm.pack_words(E)), "E (padding bits zero)"
        assert np.array_equal(_np(f).view(np.uint64), pm.pack_words(fired)), "fired row (padding bits zero)"
        if bits:
            assert np.array_equal(_np(d).view(np.uint64), pm.pack_words(det)), "detector words (padding bits zero)"
        # the same shots in two calls, without the fired row
        h2 = _half_dev(name, T)
        d1, e1 = h2.sample(P_DATA, Q, 100, bits=bits)
        d2, e2 = h2.sample(P_DATA, Q, 157, bits=bits)
        assert torch.equal(torch.cat([d1, d2]), d) and torch.equal(torch.cat([e1, e2]), e)
    d, e, f = _half_dev(name, T).sample(0.0, Q, B, want_fired=True)
    got = _words(f, fired.shape[1])
    assert not _np(e).any() and not got[:, pm.is_data(n, m, T)].any()
    assert np.array_equal(_np(d), pm.sample(H, T, 0.0, Q, SEED, SHOT0, B)[0])
    d, e, f = _half_dev(name, T).sample(P_DATA, 0.0, B, want_fired=True)
    got = _words(f, fired.shape[1])
    assert not got[:, ~pm.is_data(n, m, T)].any() and got.any()
    assert np.array_equal(_np(d), pm.sample(H, T, P_DATA, 0.0, SEED, SHOT0, B)[0])


@pytest.mark.parametrize("T", (1, 2, 3))
@pytest.mark.parametrize("name", SHAPES)
def test_sampler_equals_the_generic_sampler_on_the_materialised_matrix(name, T):
    """qldpc_channel_sample_vec on the space-time matrix with (px, py, pz) =
    (prior, 0, 0) and the same key: its syndromes are the detectors, its errX
    the fired row (so its fold is E). With T = 1 that is the call on H."""
    from qldpcsim_amd import simulator, spacetime
    H = half(name)[0]
    m, n = H.shape
    S = spacetime.spacetime_matrix(H, T)
    if T == 1:
        S = H
    pr = spacetime.spacetime_prior(n, m, T, P_DATA, Q)
    ch = simulator.DeviceChannel(S, S, _dev(), SEED, SHOT0)
    ch.set_probs(np.stack([pr, np.zeros_like(pr), np.zeros_like(pr)]))
    sy_z, _, errX, _ = ch.sample(0.0, B)
    d, e, f = _half_dev(name, T).sample(P_DATA, Q, B, want_fired=True)
    assert np.array_equal(_np(d), _np(sy_z))
    assert np.array_equal(_np(f), _np(errX))
    assert np.array_equal(_words(e, n), spacetime.fold_data(_np(ch.unpack(errX)), n, m, T))


@functools.lru_cache(maxsize=None)
def _crafted(name, T):
    H, L, Hstab, Lop = half(name)
    det, E, fired = _model(name, T, 0.05, 0.04)
    rng = np.random.default_rng(17)
    ehat, rec = pm.craft(rng, H, Hstab, Lop, T, fired)
    iters = rng.integers(1, 60, B).astype(np.int32)
    cls, F, r = pm.classify(H, L, T, det, E, ehat)
    return det, E, ehat, rec, iters, cls, F, r


@pytest.mark.parametrize("T", (1, 2, 3))
@pytest.mark.parametrize("name", SHAPES)
def test_counter_equals_the_model(name, T):
    """Per-shot class, flip words and folded residual in both estimate and
    detector formats; the four counters equal the sums and accumulate over
    two calls. Every crafted case occurs with its class in the model."""
    import torch
    from qldpcsim_amd import _lib, decoders
    assert _lib.phenom_kernel_name(half(name)[0], "count", 0) == f"phenom_count_kernel<{KERNEL_DEGREE[name]}>"
    det, E, ehat, rec, iters, cls, F, r = _crafted(name, T)
    for i, want in enumerate((0, 0, 0, 1, 2, 2)):
        hit = cls[rec == i]
        assert (T == 1 and i in (2, 5)) or hit.size >= 20, (i, hit.size)
        assert (hit == want).all(), (pm.RECIPES[i], hit)
    h = _half_dev(name, T)
    dev = _dev()
    tn = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    t_det, t_eh, t_it = tn(det), tn(ehat), tn(iters)
    t_E = tn(pm.pack_words(E).view(np.int64))
    want = pm.counters(cls, iters)
    wv = [want["failures"], want["logical_errors"], want["successes"], want["iterations"]]
    for d_ in (t_det, decoders.pack_bits(t_det)):
        for e_ in (t_eh, decoders.pack_bits(t_eh)):
            acc, c, fl, rs = h.count_device(d_, t_E, e_, t_it, want_shots=True)
            assert np.array_equal(_np(c), cls)
            assert np.array_equal(_np(fl).view(np.uint64), pm.pack_words(F))
            assert np.array_equal(_np(rs).view(np.uint64), pm.pack_words(r))
            assert acc.cpu().tolist() == wv
            acc2 = h.count_device(d_[:100].contiguous(), t_E[:100].contiguous(), e_[:100].contiguous(),
                                  t_it[:100].contiguous())
            acc2 = h.count_device(d_[100:].contiguous(), t_E[100:].contiguous(), e_[100:].contiguous(),
                                  t_it[100:].contiguous(), acc2)
            assert acc2.cpu().tolist() == wv
            h.count_device(d_, t_E, e_, t_it, acc2)
            assert acc2.cpu().tolist() == [2 * v for v in wv]
    with pytest.raises(ValueError):
        h.count_device(t_det, t_E, t_eh[:, :-1].contiguous(), t_it)


# ---------------------------------------------------------------------------
# simulate_phenomenological end to end
# ---------------------------------------------------------------------------
def _key(seed, rank=0):
    return int(np.random.SeedSequence([seed, rank]).generate_state(1, np.uint64)[0])


def _decode_half(H, T, det, p_data, q, algo, sched, osd, iters):
    """decode_batch on the materialised matrix (host entry: NumPy in and
    out), then OSDdec shot by shot on the non-converged ones."""
    from qldpcsim_amd import decoders, schedule
    m, n = H.shape
    S = pm.dense_matrix(H, T)
    layers = None if sched == "F" else schedule.layerize(S, serial=sched == "S")
    if T == 1 or p_data == q:
        r = decoders.decode_batch(S, det, p_data, iters, layers=layers, algo=algo, want_post=osd >= 0)
    else:
        r = decoders.decode_batch(S, det, None, iters, layers=layers, algo=algo, want_post=osd >= 0,
                                  prior=np.where(pm.is_data(n, m, T), p_data, q))
    ehat = r.ehat.copy()
    bad = np.flatnonzero(~r.converged)
    if osd >= 0:
        for b in bad:
            decoders.OSDdec(S, ehat[b], det[b], r.post[b], osd)
    return ehat, r.iters, bad.size


def _count(tot, sfx, cls, iters):
    c = pm.counters(cls, iters)
    tot["DecFailures_" + sfx] += c["failures"]
    tot["logicalErrors_" + sfx] += c["logical_errors"]
    tot["nIterAcc" + sfx] += c["iterations"]


def _loop(Hx, Hz, p, q, T, shots, seed, algo="MS", sched="F", osd=-1, iters=30, ranks=1):
    """Model sampler -> decode_batch on the materialised matrix -> model
    counter, over every rank's contiguous share. Returns (counters, number of
    non-converged half-shots)."""
    from qldpcsim_amd import logicals, simulator
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    tot = {k: 0 for k in simulator.PHENOM_KEYS}
    nbad = 0
    for rank in range(ranks):
        my = shots // ranks + (1 if rank < shots % ranks else 0)
        cls = []
        for H, L, sfx, key in ((Hz, Lz, "X", _key(seed, rank)), (Hx, Lx, "Z", _key(seed, rank) ^ 0x9E3779B97F4A7C15)):
            det, E, _ = pm.sample(H, T, 2 * p / 3, q, key, 0, my)
            ehat, it, nb = _decode_half(H, T, det, 2 * p / 3, q, algo, sched, osd, iters)
            c = pm.classify(H, L, T, det, E, ehat)[0]
            _count(tot, sfx, c, it)
            cls.append(c)
            nbad += nb
        tot["decSuccessLogical"] += int(((cls[0] == 0) & (cls[1] == 0)).sum())
    return tot, nbad


def _check(got, want, shots, T, p, q):
    from qldpcsim_amd import simulator
    for k in simulator.PHENOM_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    ler = 1. - want["decSuccessLogical"] / shots
    assert got["logical_error_rate"] == ler
    assert got["logical_error_rate_ci95"] == simulator.wilson_interval(shots - want["decSuccessLogical"], shots)
    assert got["logical_error_rate_per_round"] == 1. - (1. - ler) ** (1. / T)
    assert (got["rounds"], got["q"], got["p_data"]) == (T, q, 2 * p / 3)


@pytest.mark.parametrize("q", (0.02, 0.01))
def test_simulate_phenomenological_lp04_ms_flooding(q):
    """LP04_0, T = 3, MS flooding, p = 0.03 (p_data = 0.02): q = 0.02 takes the
    scalar entry point, q = 0.01 decode_vprior_kernel. 600 shots in batches of
    256 and of 77 equal the model loop and each other."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    p, T, shots, seed = 0.03, 3, 600, 5
    assert (2 * p / 3 == q) == (q == 0.02)
    want, _ = _loop(Hx, Hz, p, q, T, shots, seed)
    assert want["decSuccessLogical"] > 0 and want["nIterAccX"] > shots
    assert want["DecFailures_X"] + want["logicalErrors_X"] + want["DecFailures_Z"] + want["logicalErrors_Z"] > 0
    kw = dict(shots=shots, decType="MS", decIterations=30, rngSeed=seed, sampler="device", verbose=False)
    got = simulator.simulate_phenomenological(Hx, Hz, p, q, T, batch_size=256, **kw)
    _check(got, want, shots, T, p, q)
    assert simulator.simulate_phenomenological(Hx, Hz, p, q, T, batch_size=77, **kw) == got


def test_simulate_phenomenological_bp_layered():
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    p, q, T, shots, seed = 0.03, 0.01, 3, 200, 6
    want, _ = _loop(Hx, Hz, p, q, T, shots, seed, algo="BP", sched="L", iters=20)
    got = simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=shots, decType="BP", decIterations=20,
                                              decSchedule="L", rngSeed=seed, batch_size=128, sampler="device",
                                              verbose=False)
    _check(got, want, shots, T, p, q)


def test_simulate_phenomenological_osd0_on_steane():
    """OSD-0 after a short min-sum on steane, T = 2, against the loop with
    OSDdec; some shots must reach OSD."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("steane")
    p, q, T, shots, seed = 0.12, 0.05, 2, 400, 7
    want, nbad = _loop(Hx, Hz, p, q, T, shots, seed, osd=0, iters=3)
    assert nbad >= 10
    got = simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=shots, decType="MS", decIterations=3, OSDorder=0,
                                              rngSeed=seed, batch_size=150, sampler="device", verbose=False)
    _check(got, want, shots, T, p, q)
    assert got["DecFailures_X"] == 0 and got["DecFailures_Z"] == 0       # OSD reproduces every detector


def test_simulate_phenomenological_host_sampler():
    """sampler="host" on steane, T = 2, 300 shots: counters equal a
    hand-written loop over the same generator (the X half draws first in
    every batch), thresholds and classes from the model. The host decode entry
    stages through the device, hence the gpu mark."""
    from qldpcsim_amd import codes, logicals, simulator
    Hx, Hz = codes.load_code("steane")
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    p, q, T, shots, seed, bs = 0.09, 0.03, 2, 300, 8, 128
    rng = np.random.default_rng([seed, 0])
    tot = {k: 0 for k in simulator.PHENOM_KEYS}
    done = 0
    while done < shots:
        nb = min(bs, shots - done)
        cls = []
        for H, L, sfx in ((Hz, Lz, "X"), (Hx, Lx, "Z")):
            m, n = H.shape
            S = pm.dense_matrix(H, T)
            thr = np.where(pm.is_data(n, m, T), pm.threshold(2 * p / 3), pm.threshold(q)).astype(np.uint64)
            fired = (rng.integers(0, 1 << 32, (nb, S.shape[1]), dtype=np.uint64) < thr).astype(np.uint8)
            det, E = pm.mod2(fired, S), pm.fold(fired, n, m, T)
            ehat, it, _ = _decode_half(H, T, det, 2 * p / 3, q, "MS", "F", -1, 25)
            c = pm.classify(H, L, T, det, E, ehat)[0]
            _count(tot, sfx, c, it)
            cls.append(c)
        tot["decSuccessLogical"] += int(((cls[0] == 0) & (cls[1] == 0)).sum())
        done += nb
    got = simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=shots, decType="MS", decIterations=25,
                                              rngSeed=seed, batch_size=bs, sampler="host", verbose=False)
    _check(got, tot, shots, T, p, q)
    assert 0 < tot["decSuccessLogical"] < shots


def test_cli_two_ranks(tmp_path):
    """`torchrun -m qldpcsim_amd.simulator --rounds 3 --meas-error 0.01` with
    two gloo ranks on the one GPU: the all-reduced counters equal the
    single-process loop over both ranks' shards."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP04_0")
    np.save(tmp_path / "Hx.npy", Hx.astype(np.int64))
    np.save(tmp_path / "Hz.npy", Hz.astype(np.int64))
    res = tmp_path / "res.json"
    shots, seed, p, q, T, it = 501, 9, 0.03, 0.01, 3, 30
    env = dict(os.environ, QLDPC_SIM_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", "-m", "qldpcsim_amd.simulator",
                        "--Hx", str(tmp_path / "Hx.npy"), "--Hz", str(tmp_path / "Hz.npy"), "--p", str(p),
                        "--shots", str(shots), "--decIterations", str(it), "--rngSeed", str(seed), "--batch", "100",
                        "--rounds", str(T), "--meas-error", str(q), "--results", str(res)], cwd=ROOT,
                       capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("PHENOMENOLOGICAL NOISE") == 1 and "SIMULATION RESULTS" not in r.stdout
    doc = json.loads(res.read_text())
    assert doc["meta"]["world"] == 2 and doc["meta"]["rounds"] == T and doc["meta"]["q"] == q
    want, _ = _loop(Hx, Hz, p, q, T, shots, seed, iters=it, ranks=2)
    _check(doc["results"][str(p)], want, shots, T, p, q)


def test_vector_prior_refusal_past_lds_and_the_scalar_path_at_the_same_shape():
    """LP118_0 at T = 5 (1200 x 3680) is past decode_vprior_kernel's LDS:
    p_data != q raises NotImplementedError when the launch is planned, before
    any shot is drawn; with p_data == q the same shape decodes through the
    scalar entry point."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP118_0")
    kw = dict(shots=64, decType="MS", decIterations=10, rngSeed=3, sampler="device", verbose=False)
    with pytest.raises(NotImplementedError, match="per-variable priors"):
        simulator.simulate_phenomenological(Hx, Hz, 0.003, 0.001, 5, **kw)
    got = simulator.simulate_phenomenological(Hx, Hz, 0.003, 0.002, 5, **kw)
    want, _ = _loop(Hx, Hz, 0.003, 0.002, 5, 64, 3, iters=10)
    _check(got, want, 64, 5, 0.003, 0.002)

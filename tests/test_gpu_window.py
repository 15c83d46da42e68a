"""Sliding-window decoding on the GPU: phenom_window_kernel
(qldpc_phenom_window, DevicePhenomHalf.advance) bit for bit against its NumPy
twin spacetime.window_advance in every combination of wire formats, then
simulate_phenomenological(window=) end to end against a model loop
(decode_batch per window, the twin between windows, the model counter at the
end). Every comparison is integer equality."""
import functools
import itertools

import numpy as np
import pytest

import phenom_model as pm
from test_gpu_phenom import _check, _count, _key
from test_phenom_model import half

pytestmark = pytest.mark.gpu

# shape, T, (W, F): many windows inside one 64-bit word (steane, n + m = 10);
# commits and cuts that straddle words at odd offsets (LP04_0, n + m = 259); every commit and cut on a word
# boundary (q8a-Hz of tests/channel_shape_codes.py, n + m = 192: shift 0, whole first and last words); m = 63
# beside n = 126 (q6b-Hz, n + m = 189)
KERNEL_CASES = [("steane", 9, (3, 1)), ("steane", 9, (3, 3)), ("steane", 9, (4, 2)),
                ("LP04_0", 6, (3, 1)), ("LP04_0", 6, (2, 2)), ("shor_x", 5, (2, 1)),
                ("q8a_hz", 5, (3, 1)), ("q8a_hz", 5, (2, 2)), ("q6b_hz", 4, (2, 1))]
FORMATS = list(itertools.product((False, True), repeat=3))      # (detectors, estimate, syndrome) packed?


def _dev():
    import torch
    return torch.device("cuda", 0)


def _grid_shots():
    """Shots one launch covers without a wave taking a second one: the launch
    code's grid is min(ceil(batch / 4), 8 workgroups per CU) workgroups of
    four waves, one shot per wave at a time."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4


def _to(a, packed):
    """uint8 [B, k] -> the device tensor of a wire format."""
    import torch
    from qldpcsim_amd import decoders
    t = torch.as_tensor(np.ascontiguousarray(a), device=_dev())
    return decoders.pack_bits(t) if packed else t


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _run_schedule(name, T, W, F, nb, d_bits, e_bits, s_bits, seed):
    """Every window of the schedule on the device and in the twin, from an
    estimate buffer of all ones, random rows as the windows' estimates (they
    alternate between the two formats). Compares after every step."""
    import torch
    from qldpcsim_amd import simulator, spacetime
    H, L = half(name)[:2]
    m, n = H.shape
    N = spacetime.spacetime_shape(n, m, T)[1]
    rng = np.random.default_rng(seed)
    det = rng.integers(0, 2, (nb, T * m), dtype=np.uint8)
    h = simulator.DevicePhenomHalf(H, L, T, _dev(), 1)
    t_det = _to(det, d_bits)
    t_eh = torch.full((nb, h.NW), -1, dtype=torch.int64, device=_dev()) if e_bits else \
        torch.ones((nb, N), dtype=torch.uint8, device=_dev())
    t_it = torch.full((nb,), 5, dtype=torch.int32, device=_dev())
    ehat, total = np.ones((nb, N), np.uint8), np.full(nb, 5, np.int32)
    last = west = wit = t_west = t_wit = None
    for k, w in enumerate(spacetime.window_schedule(T, W, F) + [None]):
        want = spacetime.window_advance(n, m, T, det, ehat, total, last, west, wit, w)
        got = h.advance(t_det, t_eh, t_it, last, t_west, t_wit, w, bits=s_bits)
        where = (name, T, W, F, nb, (d_bits, e_bits, s_bits), k)
        if w is None:
            assert got is None and want is None
        elif s_bits:
            assert got.dtype == torch.int64
            assert np.array_equal(_words(got), pm.pack_words(want)), ("syndrome words, padding included", where)
        else:
            assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want), ("syndrome", where)
        eh = pm.unpack_words(_words(t_eh), N) if e_bits else t_eh.cpu().numpy()
        assert np.array_equal(eh, ehat), ("estimate after the step", where)
        assert np.array_equal(t_it.cpu().numpy(), total), ("iterations", where)
        if w is None:
            break
        Nw = spacetime.window_shape(n, m, w[1], w[2])[1]
        west = rng.integers(0, 2, (nb, Nw), dtype=np.uint8)
        wit = rng.integers(1, 60, nb).astype(np.int32)
        t_west, t_wit = _to(west, (k + e_bits) % 2 == 1), torch.as_tensor(wit, device=_dev())
        last = w
    # overwrite safety: from all ones, exactly the assembled estimate is left, padding bits zero
    assert ehat.max() <= 1 and ehat.any() and not ehat.all()
    if e_bits:
        assert np.array_equal(_words(t_eh), pm.pack_words(ehat)), ("estimate words, padding included", where)


@pytest.mark.parametrize("name,T,WF", KERNEL_CASES)
def test_window_kernel_equals_the_twin(name, T, WF):
    """All 2 x 2 x 2 formats of detectors, estimate and syndrome, batches of 1
    and 257, every window of the schedule, from an estimate buffer of all
    ones: every syndrome, the estimate after every step (so merges keep their
    neighbours and every bit is written) and the summed iterations."""
    for i, (d_bits, e_bits, s_bits) in enumerate(FORMATS):
        for nb in (1, 257):
            _run_schedule(name, T, *WF, nb, d_bits, e_bits, s_bits, seed=100 * i + nb)


@pytest.mark.parametrize("fmt", [(True, True, True), (False, False, False), (True, False, True)])
def test_window_kernel_when_waves_take_a_second_shot(fmt):
    """steane, T = 9, (W, F) = (3, 1): one batch larger than the grid covers."""
    _run_schedule("steane", 9, 3, 1, _grid_shots() + 259, *fmt, seed=7)


def test_advance_refuses_buffers_that_do_not_match():
    import torch
    from qldpcsim_amd import simulator
    H, L = half("steane")[:2]
    h = simulator.DevicePhenomHalf(H, L, 5, _dev(), 1)
    det = torch.zeros((4, h.M), dtype=torch.uint8, device=_dev())
    eh = torch.zeros((4, h.N), dtype=torch.uint8, device=_dev())
    it = torch.zeros(4, dtype=torch.int32, device=_dev())
    west = torch.zeros((4, 20), dtype=torch.uint8, device=_dev())
    assert tuple(h.advance(det, eh, it, None, None, None, (0, 2, False, 1)).shape) == (4, 6)
    syn = h.advance(det, eh, it, (0, 2, False, 1), west, it.clone(), (1, 2, False, 1), bits=True)
    assert tuple(syn.shape) == (4, 1) and syn.dtype == torch.int64
    for bad in (dict(det=det[:, :-1].contiguous()), dict(ehat=eh[:, :-1].contiguous()), dict(iters=it.to(torch.int64)),
                dict(west=west[:, :-1].contiguous()), dict(witers=None), dict(west=west.cpu()),
                dict(done=(4, 2, False, 1)), dict(done=(3, 2, False, 1), nxt=None), dict(done=(0, 2, False, 3)),
                dict(nxt=(2, 2)), dict(nxt=(1, 5)), dict(done=(0, 2, True, 2))):
        kw = dict(det=det, ehat=eh, iters=it, done=(0, 2, False, 1), west=west, witers=it.clone(), nxt=(1, 2))
        with pytest.raises(ValueError):
            h.advance(**{**kw, **bad})
    with pytest.raises(ValueError):
        h.advance(det, eh, it)


# ---------------------------------------------------------------------------
# simulate_phenomenological(window=) end to end
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _window_record(name_H, R, closed, sched):
    """(window matrix, its layers) of a half, built once."""
    from qldpcsim_amd import codes, schedule, spacetime
    code, which = name_H
    H = codes.load_code(code)[which]
    Hw = spacetime.spacetime_matrix(H, R) if closed else spacetime.window_matrix(H, R)
    return Hw, (None if sched == "F" else schedule.layerize(Hw, serial=sched == "S"))


def _decode_windows(name_H, H, T, W, F, det, p_data, q, algo, sched, osd, iters):
    """The model loop of one half-batch: decode_batch's host entry on each
    window's matrix (OSDdec shot by shot on the non-converged ones), the NumPy
    twin between windows."""
    from qldpcsim_amd import decoders, spacetime
    m, n = H.shape
    nb = det.shape[0]
    ehat = np.zeros((nb, spacetime.spacetime_shape(n, m, T)[1]), np.uint8)
    total = np.zeros(nb, np.int32)
    last = west = wit = None
    nbad = 0
    for w in spacetime.window_schedule(T, W, F):
        syn = spacetime.window_advance(n, m, T, det, ehat, total, last, west, wit, w)
        Hw, layers = _window_record(name_H, w[1], w[2], sched)
        pr = (spacetime.spacetime_prior if w[2] else spacetime.window_prior)(n, m, w[1], p_data, q)
        if (pr == pr[0]).all():
            r = decoders.decode_batch(Hw, syn, float(pr[0]), iters, layers=layers, algo=algo, want_post=osd >= 0)
        else:
            r = decoders.decode_batch(Hw, syn, None, iters, layers=layers, algo=algo, want_post=osd >= 0, prior=pr)
        west, wit = r.ehat.copy(), r.iters
        bad = np.flatnonzero(~r.converged)
        nbad += bad.size
        if osd >= 0:
            for b in bad:
                decoders.OSDdec(Hw, west[b], syn[b], r.post[b], osd)
        last = w
    spacetime.window_advance(n, m, T, det, ehat, total, last, west, wit, None)
    return ehat, total, nbad


def _wloop(code, p, q, T, W, F, shots, seed, algo="MS", sched="F", osd=-1, iters=30, ranks=1):
    """Model sampler -> windowed decode -> model counter over every rank's
    contiguous share. Returns (counters, non-converged window decodes)."""
    from qldpcsim_amd import codes, logicals, simulator
    Hx, Hz = codes.load_code(code)
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    tot = {k: 0 for k in simulator.PHENOM_KEYS}
    nbad = 0
    for rank in range(ranks):
        my = shots // ranks + (1 if rank < shots % ranks else 0)
        cls = []
        for which, H, L, sfx, key in ((1, Hz, Lz, "X", _key(seed, rank)),
                                      (0, Hx, Lx, "Z", _key(seed, rank) ^ 0x9E3779B97F4A7C15)):
            det, E, _ = pm.sample(H, T, 2 * p / 3, q, key, 0, my)
            ehat, it, nb = _decode_windows((code, which), H, T, W, F, det, 2 * p / 3, q, algo, sched, osd, iters)
            c = pm.classify(H, L, T, det, E, ehat)[0]
            _count(tot, sfx, c, it)
            cls.append(c)
            nbad += nb
        tot["decSuccessLogical"] += int(((cls[0] == 0) & (cls[1] == 0)).sum())
    return tot, nbad


def _check_window(got, want, shots, T, p, q, W, F):
    from qldpcsim_amd import spacetime
    _check(got, want, shots, T, p, q)
    assert (got["window"], got["commit"], got["windows"]) == (W, F, len(spacetime.window_schedule(T, W, F)))


@pytest.mark.parametrize("T,W,F", [(3, 3, 1), (2, 4, 2), (3, 5, 5)])
def test_a_window_that_holds_every_round_is_the_whole_decode(T, W, F):
    """T <= W: one closed window of T rounds, the counters of the call without
    window= on the same seed (vector priors, two batches)."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    kw = dict(shots=300, decType="MS", decIterations=20, rngSeed=21, batch_size=160, sampler="device", verbose=False)
    whole = simulator.simulate_phenomenological(Hx, Hz, 0.03, 0.01, T, **kw)
    got = simulator.simulate_phenomenological(Hx, Hz, 0.03, 0.01, T, window=W, commit=F, **kw)
    assert (got.pop("window"), got.pop("commit"), got.pop("windows")) == (W, F, 1)
    assert got == whole and "window" not in whole
    assert whole["nIterAccX"] > 300


@pytest.mark.parametrize("q,algo,sched,osd,iters,p", [
    (0.02, "MS", "F", -1, 30, 0.03),        # p_data == q: the scalar entry point
    (0.01, "MS", "F", -1, 30, 0.03),        # decode_vprior_kernel
    (0.01, "BP", "L", -1, 20, 0.03),
    (0.03, "MS", "F", 0, 4, 0.06),          # OSD-0 after a short min-sum
], ids=["ms_scalar", "ms_vector", "bp_layered", "ms_osd0"])
def test_simulate_sliding_window_equals_the_model_loop(q, algo, sched, osd, iters, p):
    """LP04_0, T = 5, (W, F) = (3, 1): three windows per half-batch, batches of
    128 and of 77 equal the model loop and each other."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    T, W, F, shots, seed = 5, 3, 1, 300 if osd < 0 else 160, 31
    want, nbad = _wloop("LP04_0", p, q, T, W, F, shots, seed, algo=algo, sched=sched, osd=osd, iters=iters)
    assert want["nIterAccX"] > 3 * shots and want["decSuccessLogical"] < shots
    assert nbad >= 10 if osd >= 0 else want["decSuccessLogical"] > 0
    kw = dict(shots=shots, decType=algo, decIterations=iters, decSchedule=sched, OSDorder=osd, rngSeed=seed,
              sampler="device", verbose=False, window=W)
    got = simulator.simulate_phenomenological(Hx, Hz, p, q, T, batch_size=128, **kw)
    _check_window(got, want, shots, T, p, q, W, F)
    if osd >= 0:
        assert got["DecFailures_X"] == 0 and got["DecFailures_Z"] == 0   # OSD reproduces every window syndrome
    assert simulator.simulate_phenomenological(Hx, Hz, p, q, T, batch_size=77, commit=1, **kw) == got


def test_cli_two_ranks_sliding_window(tmp_path):
    """`torchrun -m qldpcsim_amd.simulator --rounds 5 --window 3 --commit 1`
    with two gloo ranks on the one GPU: the all-reduced counters equal the
    single-process model loop over both ranks' shards; W/F are in the meta."""
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
    shots, seed, p, q, T, it = 301, 9, 0.03, 0.01, 5, 30
    env = dict(os.environ, QLDPC_SIM_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29548", "-m", "qldpcsim_amd.simulator",
                        "--Hx", str(tmp_path / "Hx.npy"), "--Hz", str(tmp_path / "Hz.npy"), "--p", str(p),
                        "--shots", str(shots), "--decIterations", str(it), "--rngSeed", str(seed), "--batch", "100",
                        "--rounds", str(T), "--meas-error", str(q), "--window", "3", "--commit", "1",
                        "--results", str(res)], cwd=ROOT, capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("PHENOMENOLOGICAL NOISE") == 1 and "Window W/F" in r.stdout
    doc = json.loads(res.read_text())
    assert doc["meta"]["world"] == 2 and (doc["meta"]["window"], doc["meta"]["commit"]) == (3, 1)
    want, _ = _wloop("LP04_0", p, q, T, 3, 1, shots, seed, iters=it, ranks=2)
    _check_window(doc["results"][str(p)], want, shots, T, p, q, 3, 1)


def test_sliding_window_decodes_what_the_whole_matrix_refuses():
    """LP118_0, T = 8, p_data != q: past decode_vprior_kernel's LDS as a whole
    (NotImplementedError, the existing refusal); with window=3 the window
    matrices fit and all 512 shots are classified."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP118_0")
    shots = 512
    kw = dict(shots=shots, decType="MS", decIterations=10, rngSeed=3, sampler="device", verbose=False)
    with pytest.raises(NotImplementedError, match="per-variable priors"):
        simulator.simulate_phenomenological(Hx, Hz, 0.003, 0.001, 8, **kw)
    got = simulator.simulate_phenomenological(Hx, Hz, 0.003, 0.001, 8, window=3, **kw)
    assert (got["window"], got["commit"], got["windows"], got["rounds"]) == (3, 1, 6, 8)
    bad = [got["DecFailures_" + s] + got["logicalErrors_" + s] for s in "XZ"]
    # each half's three classes sum to the shot count, so the shots with both
    # halves class 0 lie between shots - bad_X - bad_Z and shots - max(bad)
    assert all(0 <= b <= shots for b in bad)
    assert shots - sum(bad) <= got["decSuccessLogical"] <= shots - max(bad)
    assert got["nIterAccX"] >= 6 * shots and got["nIterAccZ"] >= 6 * shots       # every window of every shot ran
    assert got["decSuccessLogical"] > shots // 2


def test_a_window_too_wide_for_the_vector_prior_kernel_is_still_refused(monkeypatch):
    """LP118_0, W = 5, p_data != q: the open window is past the kernel's LDS;
    NotImplementedError before any shot is drawn."""
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP118_0")

    def no_shots(*a, **k):
        raise AssertionError("a shot was drawn")

    monkeypatch.setattr(simulator.DevicePhenomHalf, "sample", no_shots)
    with pytest.raises(NotImplementedError, match="per-variable priors"):
        simulator.simulate_phenomenological(Hx, Hz, 0.003, 0.001, 8, shots=64, decType="MS", decIterations=10,
                                            rngSeed=3, sampler="device", verbose=False, window=5)

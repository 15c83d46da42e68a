"""Monte-Carlo driver with the reference simulator's API, batched on the GPU.

Same names, arguments, flags and counters as albertogp71/qLDPCsim
qLDPCsim/simulator.py:
    load_matrix(path)                                   simulator.py:20-35
    simulate_p(Hx, Hz, p, shots, decType, decIterations,
               decSchedule, OSDorder, rngSeed) -> dict  simulator.py:167-315
    simulate(HxFile, HzFile, p, shots, ...)             simulator.py:319-347
    main(argv)                                          simulator.py:351-373

What changes underneath: instead of a serial Python loop over shots
(simulator.py:244-304) the shots are processed in batches — one kernel
launch per half (X: Hz with the Hx-derived layers; Z: Hx with the
Hz-derived layers, the reference's cross-wiring, :278-282) — and the counters
are formed with array operations with the reference's exact definitions.
With torch.distributed initialised, shots shard across ranks and the six
counters are summed with one all_reduce (RCCL over xGMI on the GPU node);
`torchrun --nproc-per-node 8 -m qldpcsim_amd.simulator ...` sets that up
(one process per GPU).

Syndrome source: Stim is not available in this environment,
so shots come from a per-qubit Pauli sampler (X, Y, Z each p/3 — the
circuit's PAULI_CHANNEL_1(p/3,p/3,p/3), simulator.py:107) whose statistics
equal the circuit's: on the GPU a counter-based Philox
stream drawn by a HIP kernel next to the outcome counters (DeviceChannel,
channel_kernels.hip); on the host NumPy's generator (sample_channel). `rngSeed` seeds it (the reference
seeds np.random, which its unseeded Stim sampler never reads: runs there are
not reproducible; here they are).
"""
import argparse
import sys
import time
from dataclasses import dataclass
from typing import NamedTuple, Optional

# smallest tapered tail batch = batch_size // TAIL_DIV (see the tail tapering
# below; 32 vs 8: +0.5 % on configs[3] p = 0.1, profiles/r04bb/)
TAIL_DIV = 32

import numpy as np

from . import _lib, decoders, spacetime
from .schedule import layerize, select_layers, pack_layers  # noqa: F401  (re-exported)

__all__ = ["load_matrix", "simulate_p", "simulate", "main", "layerize", "sample_channel",
           "count_outcomes", "count_logical_outcomes", "wilson_interval", "simulate_phenomenological",
           "simulate_dem"]

COUNTER_KEYS = ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen",
                "nIterAccX", "nIterAccZ")
# the logical option's counters (class-1 half-shots per half; shots with both
# halves class 0), after COUNTER_KEYS in the device accumulator
LOGICAL_KEYS = ("logicalErrors_X", "logicalErrors_Z", "decSuccessLogical")
# simulate_phenomenological's counters (the all-reduced vector, in this order)
PHENOM_KEYS = ("DecFailures_X", "DecFailures_Z", "logicalErrors_X", "logicalErrors_Z", "nIterAccX", "nIterAccZ",
               "decSuccessLogical")
PHENOM_Z_KEY = 0x9E3779B97F4A7C15          # the Z half's Philox key is the X half's ^ this
# simulate_dem's counters (the all-reduced vector, in the device accumulator's order)
DEM_KEYS = ("DecFailures", "logicalErrors", "decSuccess", "nIterAcc")


def load_matrix(path: str) -> np.ndarray:
    """Load a binary matrix from .npy or whitespace text (simulator.py:20-35)."""
    if path.endswith(".npy"):
        mat = np.load(path, allow_pickle=False)
    else:
        mat = []
        with open(path, "rt") as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                mat.append([int(x) for x in line.split()])
        mat = np.array(mat, dtype=int)
    return (mat % 2).astype(np.int8)


def sample_channel(Hx, Hz, p, shots, rng):
    """Depolarizing-channel samples in the circuit's output layout.

    Returns (sy_z, sy_x, errX, errZ) as uint8 arrays ([shots, m_z], [shots, m_x],
    [shots, n], [shots, n]) — the slices simulator.py:249-252 takes of a Stim
    sample row [sy_z | sy_x | errX | errZ].
    """
    n = Hx.shape[1]
    u = rng.random((shots, n), dtype=np.float32)
    q = np.float32(p / 3)
    X = u < q
    Y = (u >= q) & (u < 2 * q)
    Z = (u >= 2 * q) & (u < np.float32(p))
    errX = (X | Y).astype(np.uint8)
    errZ = (Z | Y).astype(np.uint8)
    # H·e mod 2 via a float32 product (exact: row weights << 2^24)
    sy_z = (errX.astype(np.float32) @ Hz.T.astype(np.float32)).astype(np.int64) % 2
    sy_x = (errZ.astype(np.float32) @ Hx.T.astype(np.float32)).astype(np.int64) % 2
    return sy_z.astype(np.uint8), sy_x.astype(np.uint8), errX, errZ


def bias_weights(eta):
    """Channel weights (X, Y, Z) of a Z-biased Pauli channel with bias eta =
    pZ / (pX + pY), pX = pY: (1/(2(eta+1)), 1/(2(eta+1)), eta/(eta+1)); they sum
    to 1 and eta = 0.5 is the depolarizing channel."""
    eta = float(eta)
    if not (np.isfinite(eta) and eta >= 0.0):
        raise ValueError("bias must be a finite number >= 0")
    return np.array([1 / (2 * (eta + 1)), 1 / (2 * (eta + 1)), eta / (eta + 1)], np.float64)


def _weights_3n(channel_weights, n):
    """simulate_p's `channel_weights` ([3] or [3, n], rows X, Y, Z) as a
    validated float64 [3, n] array."""
    w = np.asarray(channel_weights, dtype=np.float64)
    if w.shape == (3,):
        w = np.repeat(w[:, None], n, axis=1)
    if w.shape != (3, n):
        raise ValueError(f"channel_weights must have shape [3] or [3, {n}] (rows X, Y, Z), got {list(w.shape)}")
    if not (np.isfinite(w).all() and (w >= 0).all()):
        raise ValueError("channel_weights must be finite and non-negative")
    return w


def channel_probs(p, channel_weights, n):
    """Per-qubit Pauli probabilities float64 [3, n] (rows X, Y, Z) of
    simulate_p's `channel_weights` at strength p: p * w[:, j]. ValueError
    unless every qubit's three sum to at most 1."""
    pr = float(p) * _weights_3n(channel_weights, n)
    if not ((pr[0] + pr[1]) + pr[2] <= 1.0).all():
        raise ValueError(f"p * sum(channel_weights) must be <= 1 on every qubit (p = {p})")
    return pr


def sample_channel_vec(Hx, Hz, probs, shots, rng):
    """sample_channel for per-qubit Pauli probabilities `probs` (float64 [3, n],
    rows X, Y, Z): one 32-bit draw per qubit against the device sampler's
    thresholds (qldpc_channel_table): X if u < T1_j, Y if T1_j <= u < T2_j, Z
    if T2_j <= u < T3_j. Same outputs as sample_channel."""
    n = Hx.shape[1]
    T = _lib.channel_table(probs[0], probs[1], probs[2])
    u = rng.integers(0, 1 << 32, (shots, n), dtype=np.uint64)
    errX = (u < T[1]).astype(np.uint8)                           # X | Y
    errZ = ((u >= T[0]) & (u < T[2])).astype(np.uint8)           # Y | Z
    sy_z = (errX.astype(np.float32) @ Hz.T.astype(np.float32)).astype(np.int64) % 2
    sy_x = (errZ.astype(np.float32) @ Hx.T.astype(np.float32)).astype(np.int64) % 2
    return sy_z.astype(np.uint8), sy_x.astype(np.uint8), errX, errZ


def _half_prior(q, hard):
    """decode_batch's (p, extra keywords) for a half whose qubits have the
    marginal error probabilities q [n]: the scalar entry point where they are
    all equal (the specialised kernels), else prior=q; NG / BF take no prior."""
    if hard:
        return 0.0, {}
    if q.size == 0 or (q == q[0]).all():
        return (float(q[0]) if q.size else 0.0), {}
    return None, {"prior": q}


def count_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ):
    """The reference's per-shot outcome counting (simulator.py:291-303), vectorised.

    exact:  errX == eX_hat and errZ == eZ_hat                       (:294-295)
    degen:  otherwise, Hz @ (errX ^ eX_hat) == 0 and Hx @ (errZ ^ eZ_hat) == 0
            over the integers, no mod 2 (:296-298; the reference also calls
            breakpoint() there)
    failX/Z: syndrome of the estimate differs from the measured one (:300-303)
    """
    return _count_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)[0]


def _count_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ):
    """count_outcomes' dict and the two failure masks (bool [B]) it counted,
    which count_logical_outcomes classifies by."""
    eX, eZ = np.asarray(eX), np.asarray(eZ)
    exact = np.all(errX == eX, axis=1) & np.all(errZ == eZ, axis=1)
    dX = (errX ^ eX).astype(np.float32)
    dZ = (errZ ^ eZ).astype(np.float32)
    degen = (~exact) & np.all(dX @ Hz.T.astype(np.float32) == 0, axis=1) & \
        np.all(dZ @ Hx.T.astype(np.float32) == 0, axis=1)
    sX = (eX.astype(np.float32) @ Hz.T.astype(np.float32)).astype(np.int64) % 2
    sZ = (eZ.astype(np.float32) @ Hx.T.astype(np.float32)).astype(np.int64) % 2
    failX = np.any(sX != sy_z, axis=1)
    failZ = np.any(sZ != sy_x, axis=1)
    return {
        "DecFailures_X": int(failX.sum()),
        "DecFailures_Z": int(failZ.sum()),
        "decSuccessExact": int(exact.sum()),
        "decSuccessDegen": int(degen.sum()),
        "nIterAccX": int(np.asarray(itX, dtype=np.int64).sum()),
        "nIterAccZ": int(np.asarray(itZ, dtype=np.int64).sum()),
    }, failX, failZ


def _pack_flips(F):
    """0/1 [B, k] -> uint64 [B, ceil(k/64)], bit i % 64 of word i / 64."""
    B, k = F.shape
    kw = (k + 63) // 64
    b = np.zeros((B, 8 * kw), dtype=np.uint8)
    if k:
        pk = np.packbits(F.astype(np.uint8), axis=1, bitorder="little")
        b[:, :pk.shape[1]] = pk
    return b.view("<u8").astype(np.uint64, copy=False).reshape(B, kw)


def count_logical_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ, logicals=None,
                           want_shots=False):
    """count_outcomes plus the stabiliser-group outcome of each half-shot
    (the NumPy twin of qldpc_count_logical_ex), vectorised over the batch.

    With rX = errX ^ eX, rZ = errZ ^ eZ and (Lx, Lz) = `logicals` (default:
    logicals.css_logicals(Hx, Hz)), the X half (the estimate that decodes Hz) is
        class 2  decoder failure: Hz·eX mod 2 != sy_z (the reference's test)
        class 1  logical error:   not 2, and Lz·rX mod 2 != 0
        class 0  success:         not 2, and Lz·rX mod 2 == 0 (rX is then an
                 X stabiliser; an exact match is class 0)
    and the Z half mirrors it with Hx, sy_x, Lx, rZ. The logical reading
    assumes sy = H·err: both shot sources guarantee it; for caller-supplied
    samples it is the caller's contract.

    Returns the six COUNTER_KEYS and the three LOGICAL_KEYS; with want_shots
    also (class_x, class_z uint8 [B], flip_x, flip_z uint64 [B, ceil(k/64)]):
    flip_x = Lz·rX mod 2, flip_z = Lx·rZ mod 2, bit i % 64 of word i / 64,
    as computed for every class."""
    if logicals is None:
        from .logicals import css_logicals
        logicals = css_logicals(Hx, Hz)
    Lx, Lz = logicals
    f32 = np.float32
    out, failX, failZ = _count_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
    fX = ((errX ^ eX).astype(f32) @ Lz.T.astype(f32)).astype(np.int64) % 2
    fZ = ((errZ ^ eZ).astype(f32) @ Lx.T.astype(f32)).astype(np.int64) % 2
    cX = np.where(failX, 2, np.any(fX != 0, axis=1).astype(np.uint8)).astype(np.uint8)
    cZ = np.where(failZ, 2, np.any(fZ != 0, axis=1).astype(np.uint8)).astype(np.uint8)
    out["logicalErrors_X"] = int((cX == 1).sum())
    out["logicalErrors_Z"] = int((cZ == 1).sum())
    out["decSuccessLogical"] = int(((cX == 0) & (cZ == 0)).sum())
    if want_shots:
        return out, (cX, cZ, _pack_flips(fX), _pack_flips(fZ))
    return out


def wilson_interval(successes, trials, z=1.959963984540054):
    """Wilson score interval [lo, hi] of a binomial proportion, clipped to
    [0, 1] (z = 1.959963984540054: 95 %)."""
    if trials <= 0:
        return [0.0, 1.0]
    ph = successes / trials
    den = 1.0 + z * z / trials
    mid = (ph + z * z / (2.0 * trials)) / den
    half = z * np.sqrt(ph * (1.0 - ph) / trials + z * z / (4.0 * trials * trials)) / den
    return [float(max(0.0, mid - half)), float(min(1.0, mid + half))]


def _fmt(bits):
    """The C ABI's buffer format of bit-packed words (`bits`) or byte rows."""
    return _lib.FMT_BITS if bits else _lib.FMT_BYTES


def _stream(dev):
    """torch's current HIP stream on `dev`, as the C ABI takes it."""
    import torch
    return torch.cuda.current_stream(dev).cuda_stream


class DeviceChannel:
    """Device-side shot source and outcome counters (channel_kernels.hip via
    the C ABI): the depolarizing draw of `sample_channel` as a counter-based
    Philox stream (qldpc_channel_sample: shot s of seed k is the same whatever
    the batching) and the counter definitions of `count_outcomes`
    (qldpc_count_outcomes), so a batch never leaves HBM.

    sample() returns (sy_z uint8 [B, m_z], sy_x uint8 [B, m_x], errX, errZ)
    with errX / errZ bit-packed as int64 [B, ceil(n/64)] words (bit j % 64 of
    word j / 64); `unpack` turns them into uint8 [B, n]."""

    def __init__(self, Hx, Hz, device, seed, shot0=0):
        import torch
        self.torch = torch
        self.dev = torch.device(device)
        self.n = Hx.shape[1]
        self.W = (self.n + 63) // 64
        with torch.cuda.device(self.dev):
            self.cx = _lib.code_for(Hx, self.dev.index)
            self.cz = _lib.code_for(Hz, self.dev.index)
        self.mx, self.mz = self.cx.m, self.cz.m
        self._Hx, self._Hz, self._lg = Hx, Hz, None
        self.seed = int(seed) & ((1 << 64) - 1)
        self.shot = int(shot0)
        self._vec = None

    def set_probs(self, probs):
        """Per-qubit Pauli probabilities float64 [3, n] (rows X, Y, Z): sample()
        then draws from them (qldpc_channel_sample_vec) and ignores its p."""
        with self.torch.cuda.device(self.dev):
            self._vec = _lib.Channel(self.cx, self.cz, probs[0], probs[1], probs[2])

    def sample(self, p, B, bits=False):
        """`bits`: syndromes as int64 words [B, ceil(m/64)] (decode_batch
        reads either format) instead of uint8 [B, m]."""
        torch = self.torch
        errX = torch.empty((B, self.W), dtype=torch.int64, device=self.dev)
        errZ = torch.empty((B, self.W), dtype=torch.int64, device=self.dev)
        if bits:
            sy_z = torch.empty((B, (self.mz + 63) // 64), dtype=torch.int64, device=self.dev)
            sy_x = torch.empty((B, (self.mx + 63) // 64), dtype=torch.int64, device=self.dev)
        else:
            sy_z = torch.empty((B, self.mz), dtype=torch.uint8, device=self.dev)
            sy_x = torch.empty((B, self.mx), dtype=torch.uint8, device=self.dev)
        if self._vec is not None:
            _lib.check(_lib.lib.qldpc_channel_sample_vec(
                self._vec.handle, self.seed, self.shot, int(B), errX.data_ptr(), errZ.data_ptr(), sy_z.data_ptr(),
                sy_x.data_ptr(), _fmt(bits), _stream(self.dev)))
        else:
            _lib.check(_lib.lib.qldpc_channel_sample_ex(
                self.cx.handle, self.cz.handle, float(p), self.seed, self.shot, int(B), errX.data_ptr(),
                errZ.data_ptr(), sy_z.data_ptr(), sy_x.data_ptr(), _fmt(bits), _stream(self.dev)))
        self.shot += int(B)
        return sy_z, sy_x, errX, errZ

    def unpack(self, words):
        """Packed int64 [B, W] error words -> uint8 [B, n] (device)."""
        torch = self.torch
        bits = torch.arange(64, device=words.device, dtype=torch.int64)
        return ((words.unsqueeze(-1) >> bits) & 1).to(torch.uint8).reshape(words.shape[0], -1)[:, :self.n]

    def count_device(self, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ, acc=None):
        """Adds the batch's six counters (COUNTER_KEYS order) to `acc`
        (int64 [6] device tensor, created if None) without a host sync."""
        torch = self.torch
        if acc is None:
            acc = torch.zeros(len(COUNTER_KEYS), dtype=torch.int64, device=self.dev)
        B, syn_fmt, e_fmt = self._layout("count_device", sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
        _lib.check(_lib.lib.qldpc_count_outcomes_ex(
            self.cx.handle, self.cz.handle, int(B), errX.data_ptr(), errZ.data_ptr(), sy_z.data_ptr(),
            sy_x.data_ptr(), syn_fmt, eX.data_ptr(), eZ.data_ptr(), e_fmt, itX.data_ptr(),
            itZ.data_ptr(), acc.data_ptr(), _stream(self.dev)))
        return acc

    def _layout(self, who, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ):
        """(B, syndrome format, estimate format) of one batch's buffers;
        ValueError if they do not match the batch layout."""
        torch = self.torch
        B = sy_z.shape[0]
        ts = (sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
        syn_bits = sy_z.dtype == torch.int64
        e_bits = eX.dtype == torch.int64
        e_shape = (B, self.W) if e_bits else (B, self.n)
        if not all(t.is_contiguous() and t.device == self.dev for t in ts) or \
                eX.shape != e_shape or eZ.shape != e_shape or errX.shape != (B, self.W) or \
                eX.dtype not in (torch.uint8, torch.int64) or eZ.dtype != eX.dtype or \
                sy_x.dtype != sy_z.dtype or itX.dtype != torch.int32 or itZ.dtype != torch.int32:
            raise ValueError(f"{who}: buffers do not match the batch layout")
        return B, _fmt(syn_bits), _fmt(e_bits)

    def count(self, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ):
        v = self.count_device(sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ).cpu().tolist()
        return dict(zip(COUNTER_KEYS, (int(x) for x in v)))

    def logicals(self):
        """The pair's logical operators on the device (built on first use from
        logicals.css_logicals, cached per pair and device)."""
        if self._lg is None:
            with self.torch.cuda.device(self.dev):
                self._lg = _lib.logicals_for(self._Hx, self._Hz, self.dev.index)
        return self._lg

    def count_logical_device(self, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ, acc=None, want_shots=False):
        """Adds the batch's nine counters (COUNTER_KEYS then LOGICAL_KEYS) to
        `acc` (int64 [9] device tensor, created if None) in one kernel, without
        a host sync. With want_shots returns (acc, class_x, class_z uint8 [B],
        flip_x, flip_z int64 [B, ceil(k/64)] words): see
        count_logical_outcomes."""
        torch = self.torch
        lg = self.logicals()
        if acc is None:
            acc = torch.zeros(len(COUNTER_KEYS) + len(LOGICAL_KEYS), dtype=torch.int64, device=self.dev)
        if acc.shape != (len(COUNTER_KEYS) + len(LOGICAL_KEYS),) or acc.dtype != torch.int64 or \
                acc.device != self.dev or not acc.is_contiguous():
            raise ValueError("count_logical_device: acc must be an int64 [9] tensor on the channel's device")
        B, syn_fmt, e_fmt = self._layout("count_logical_device", sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
        shots = None
        if want_shots:
            shots = (torch.empty(B, dtype=torch.uint8, device=self.dev),
                     torch.empty(B, dtype=torch.uint8, device=self.dev),
                     torch.empty((B, lg.kw), dtype=torch.int64, device=self.dev),
                     torch.empty((B, lg.kw), dtype=torch.int64, device=self.dev))
        sp = [t.data_ptr() if t.numel() else None for t in shots] if want_shots else [None] * 4
        _lib.check(_lib.lib.qldpc_count_logical_ex(
            self.cx.handle, self.cz.handle, lg.handle, int(B), errX.data_ptr(), errZ.data_ptr(), sy_z.data_ptr(),
            sy_x.data_ptr(), syn_fmt, eX.data_ptr(), eZ.data_ptr(), e_fmt, itX.data_ptr(), itZ.data_ptr(),
            acc.data_ptr(), sp[0], sp[1], sp[2], sp[3], _stream(self.dev)))
        return (acc,) + shots if want_shots else acc

    def count_logical(self, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ):
        v = self.count_logical_device(sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ).cpu().tolist()
        return dict(zip(COUNTER_KEYS + LOGICAL_KEYS, (int(x) for x in v)))


def _device_ok():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def _channel_ok(Hx, Hz):
    """The device sampler / counters handle n <= 4096 qubits (64 error words
    per shot, qldpc_channel_sample); larger codes use the host sampler."""
    return Hx.shape[1] <= 4096 and Hx.shape[1] == Hz.shape[1]


def _dist():
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized():
            return dist, dist.get_rank(), dist.get_world_size()
    except ImportError:
        pass
    return None, 0, 1


_WORKER = []


def _host_worker():
    """One background thread for the pipelined OSD's host work (waiting for a
    batch's device OSD, fetching the status-2 posteriors, NumPy's orders), so
    the main thread keeps queueing the next batch's GPU work."""
    from concurrent.futures import ThreadPoolExecutor
    if not _WORKER:
        _WORKER.append(ThreadPoolExecutor(1))
    return _WORKER[0]


def _host_orders_on(dev, staged):
    """decoders.osd_host_orders on the worker thread, with this rank's device
    current there too (the HIP current device is per thread)."""
    import torch
    torch.cuda.set_device(dev)
    return decoders.osd_host_orders(staged)


def _shard(shots, rngSeed):
    """This rank's contiguous share of the shots: (rank, its shots, its first
    shot's index, its seed pair [rngSeed, rank] or None)."""
    _, rank, world = _dist()
    my_shots = shots // world + (1 if rank < shots % world else 0)
    my_start = rank * (shots // world) + min(rank, shots % world)
    return rank, my_shots, my_start, None if rngSeed is None else [int(rngSeed), int(rank)]


def _device_key(seed):
    """The device samplers' Philox key of _shard's seed pair."""
    return int(np.random.SeedSequence(seed).generate_state(1, np.uint64)[0])


def _progress(label, my_shots, on, rates=False):
    """The progress line's printer show(done[, tot]), silent unless `on`.
    `rates`: the host path's line, with the failure rates so far from its
    counter dict `tot`."""
    t0 = time.time()

    def show(done, tot=None):
        if on:
            note = (f"Dec. failure rates (X,Z): {tot['DecFailures_X'] / done:.2e}, "
                    f"{tot['DecFailures_Z'] / done:.2e} ") if rates else ""
            print(f"\r{label} Decoding block n. {done:3}/{my_shots:4}... {note}"
                  f"({done / max(time.time() - t0, 1e-9):.3g} shots/s)", end="", flush=True)
    return show


def _all_reduce(tot, keys):
    """The counter dict `tot` summed over the ranks: a point's only collective
    (six values, nine with logical, seven phenomenological)."""
    dist, _, world = _dist()
    if dist is None or world == 1:
        return tot
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")
    t = torch.tensor([tot[k] for k in keys], dtype=torch.int64, device=dev)
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return dict(zip(keys, (int(v) for v in t.cpu().tolist())))


class _Half(NamedTuple):
    """One CSS half as decode_batch takes it, built once per call."""
    H: np.ndarray                # the matrix decoded (phenomenological: the half's space-time matrix)
    lp: np.ndarray               # its packed layers
    lr: np.ndarray
    p: Optional[float]           # decode_batch's p (None with prior=)
    kw: dict                     # relay= or prior=, if any
    code: tuple = None           # phenomenological: the code's (H, L), for the sampler and the counter


class _Decode(NamedTuple):
    """What every decode of a call shares."""
    algo: str
    iters: int
    osd: int                     # the effective OSD order (< 0: none)
    packed: bool                 # device path without OSD: bit-packed syndromes and estimates
    kw: dict                     # the path's keywords (_path_kw)
    masked: tuple = None         # correlated: (p, p_masked) of the second half
    osd_method: str = "ref"      # "cs": OSD-CS with lambda = osd (decoders.decode_batch)
    osd_cost: str = "hamming"    # "prior": OSD-CS prices candidates with each half's prior row


def _path_kw(use_dev, osd, osd_method="ref", osd_cost="hamming"):
    """decode_batch's keywords of a shot path -> (packed, keywords). Device:
    bit-packed syndromes and estimates (one bit per check / qubit in HBM)
    unless OSD needs posteriors and byte rows of the failing shots, and OSD
    is the caller's step; host: decode_batch applies OSD itself."""
    packed = use_dev and osd < 0
    host = {"osd_order": osd, **decoders._method_kw("osd_method", osd_method),
            **({} if osd_cost == "hamming" else {"osd_cost": osd_cost})}
    return packed, ({"want_post": osd >= 0, "ehat_bits": packed} if use_dev else host)


def _osd_method(osd_method, OSDorder, decType):
    """simulate_p's and simulate_phenomenological's osd_method, checked: "cs"
    needs decType MS (the only decoder whose shots get OSD here) and an
    OSDorder in 0..64."""
    if osd_method != "ref" and decType != "MS":
        decoders.osd_method_checked(osd_method, OSDorder)
        raise ValueError(f'osd_method="{osd_method}" needs decType MS: {decType} shots get no OSD step')
    return decoders.osd_method_checked(osd_method, OSDorder)


def _osd_cost(osd_cost, osd_method, rows):
    """osd_cost of a run, checked before a shot is drawn: "hamming", or "prior"
    with osd_method "cs" where every matrix that gets an OSD step decodes with a
    prior row (`rows`: each one's row or None). A half that decodes with one
    scalar prior has no row to weigh with: ValueError, as relay_cost="prior"."""
    if osd_cost not in decoders.OSD_COSTS:
        raise ValueError(f"osd_cost must be one of {decoders.OSD_COSTS}, got {osd_cost!r}")
    if osd_cost == "prior":
        decoders.osd_cost_checked(osd_cost, osd_method, True)
        if any(r is None for r in rows):
            raise ValueError('osd_cost="prior" weighs candidates by a prior row: this half decodes with one scalar '
                             "prior (uniform marginals); unequal priors give it a row")
    return osd_cost


def _osd_cost_kw(dec, half):
    """apply_osd_device's cost keywords for a half's OSD step (none with "hamming")."""
    return decoders._cost_kw(dec.osd_cost, half.kw.get("prior"))


def _relay_cost(cost, vector):
    """relay_cost of a half decoded with a prior row (`vector`) or one scalar
    prior: None is "prior" with a row and "hamming" without; "prior" without a
    row and anything unknown raise ValueError."""
    if cost not in (None,) + tuple(_lib.RELAY_COST):
        raise ValueError(f"relay_cost must be one of {tuple(_lib.RELAY_COST)} or None, got {cost!r}")
    if cost == "prior" and not vector:
        raise ValueError('relay_cost="prior" weighs solutions by a prior row: this half decodes with one scalar prior '
                         "(relay_priors and unequal priors give it a row)")
    return cost if cost is not None else ("prior" if vector else "hamming")


def _relay_config(leg_iters, gammas, sols, row, cost):
    """decode_batch's relay= of a half: the scalar relay's exactly as ever
    where `row` (the half's prior row) is None, else with the row and its cost."""
    if row is None:
        _relay_cost(cost, False)
        return decoders.RelayConfig(leg_iters, gammas, int(sols))
    return decoders.RelayConfig(leg_iters, gammas, int(sols), prior=row, cost=_relay_cost(cost, True))


def _decode_half(half, syn, dec, mask=None):
    """Decode one half's syndromes. `mask`: the other half's estimate, for the
    second half of a correlated decode (prior_mask=, p_masked=)."""
    kw = dec.kw if mask is None else dict(dec.kw, prior_mask=mask, p_masked=dec.masked[1])
    return decoders.decode_batch(half.H, syn, half.p if mask is None else dec.masked[0], dec.iters, algo=dec.algo,
                                 layer_ptr=half.lp, layer_rows=half.lr, **kw, **half.kw)


def _decode_pair(plan, sy_z, sy_x, finish=None):
    """Decode a batch's halves in the plan's order -> [rX, rZ]. Correlated: the
    second half gets the first one's final estimate as its prior mask, so
    `finish(H, syn, r)`, the device path's OSD, runs before the estimate is
    used (decoders.py:179-180)."""
    syn, res, mask = (sy_z, sy_x), [None, None], None
    for i in plan.order:
        res[i] = r = _decode_half(plan.halves[i], syn[i], plan.dec, mask)
        if finish is not None:
            finish(plan.halves[i].H, syn[i], r)
        if plan.dec.masked is not None:
            mask = r.ehat
    return res


class _Plan(NamedTuple):
    """simulate_p's checked arguments, as its loops use them."""
    halves: tuple                # (_Half X: Hz with Hx's layers, _Half Z: Hx with Hz's layers)
    order: tuple                 # the halves' indices in decode order
    dec: _Decode
    probs: Optional[np.ndarray]  # channel_weights: the samplers' per-qubit probabilities
    logicals: Optional[tuple]    # logical: the pair's (Lx, Lz)
    use_dev: bool


def _plan(Hx, Hz, p, decType, decIterations, decSchedule, OSDorder, rngSeed, samples, sampler, logical, correlated,
          correlated_q1, relay, channel_weights, osd_method="ref", osd_cost="hamming"):
    """simulate_p's argument checks, in the order they have always been made
    (all before a shot is drawn or the device is touched), and what they
    establish. `relay`: the six relay_* arguments by name."""
    n = Hx.shape[1]
    hard = decType in _lib.HARD_ALGOS
    _osd_method(osd_method, OSDorder, decType)
    probs = None
    priors = [(p / 3, {}), (p / 3, {})]           # decode_batch's p and prior= of the X and the Z half
    if channel_weights is not None:
        if correlated is not None:
            raise ValueError("channel_weights cannot be combined with correlated= (its second-half prior "
                             "assumes depolarizing noise)")
        probs = channel_probs(p, channel_weights, n)
        w = _weights_3n(channel_weights, n)
        priors = [_half_prior(float(p) * (w[0] + w[1]), hard), _half_prior(float(p) * (w[2] + w[1]), hard)]
        if decType == "RELAY" and (priors[0][1] or priors[1][1]) and not relay.get("priors"):
            raise ValueError("decType RELAY takes one scalar prior per half: channel_weights must give every "
                             "qubit the same marginals")
    if decType == "RELAY":
        if OSDorder >= 0:
            raise ValueError("decType RELAY has no OSD step (OSDorder must be < 0)")
        if correlated is not None:
            raise ValueError("decType RELAY cannot be combined with correlated=")
        if decSchedule != "F":
            raise ValueError("decType RELAY runs the flooding schedule only (decSchedule 'F')")
        if int(relay["legs"]) < 1 or int(relay["leg_iters"]) < 1 or int(relay["sols"]) < 1 or int(decIterations) < 1:
            raise ValueError("relay_legs, relay_leg_iters, relay_sols and decIterations must be >= 1")
        lo, hi = (float(x) for x in relay["gamma_range"])
        if not (np.isfinite([lo, hi, float(relay["gamma0"])]).all() and lo <= hi):
            raise ValueError("relay_gamma0 and relay_gamma_range (lo <= hi) must be finite")
        _relay_cost(relay.get("cost"), bool(priors[0][1]))
        _relay_cost(relay.get("cost"), bool(priors[1][1]))
    elif relay.get("priors") or relay.get("cost") is not None:
        raise ValueError("relay_priors and relay_cost go with decType RELAY")
    _osd_cost(osd_cost, osd_method, [kw.get("prior") for _, kw in priors])
    if rngSeed is not None:
        np.random.seed(rngSeed)                    # reference side effect (:187-188); it refuses a bad seed here
    if Hz.size and Hz.shape[1] != n:
        raise ValueError("Hx and Hz must have the same number of columns (physical qubits).")
    layersX, layersZ = select_layers(Hx, Hz, decSchedule)   # raises ValueError (:236)
    if decType not in _lib.ALGO and decType != "RELAY":
        raise ValueError("Unrecognized decoder type.")
    relays = [{}, {}]                              # decode_batch's relay= of each half
    if decType == "RELAY":
        leg_iters = [int(decIterations)] + [int(relay["leg_iters"])] * (int(relay["legs"]) - 1)
        grng = np.random.default_rng(relay["seed"])   # one generator: the Hz-decoded half draws first
        for i, kw in enumerate(relays):
            gammas = np.empty((len(leg_iters), n), np.float64)
            gammas[0] = relay["gamma0"]
            gammas[1:] = grng.uniform(lo, hi, (len(leg_iters) - 1, n))
            kw["relay"] = _relay_config(leg_iters, gammas, relay["sols"], priors[i][1].get("prior"), relay.get("cost"))
            if priors[i][1]:
                priors[i] = (None, {})             # relay_priors: the row travels in the RelayConfig, not as prior=
    if correlated not in (None, "XZ", "ZX"):
        raise ValueError("correlated must be 'XZ', 'ZX' or None")
    masked = None
    if correlated is not None:
        if hard:
            raise ValueError(f"correlated decoding needs a prior: {decType} is a hard-decision decoder")
        if not (0.0 < float(correlated_q1) <= 0.5):
            raise ValueError("correlated_q1 must lie in (0, 0.5]")
        # P(second component | no first component); correlated_q1 stands for the 1/2 given one
        masked = ((p / 3) / (1 - 2 * p / 3), float(correlated_q1))
    # the reference never passes OSDorder to BP_decoder (:281-282); NG and BF
    # get (H, syndrome) alone (:270-276): no prior, no decIterations (BF runs
    # its default 50), no OSD
    osd = OSDorder if decType == "MS" else -1
    halves = (_Half(Hz, *pack_layers(layersX, Hz.shape[0]), priors[0][0], {**relays[0], **priors[0][1]}),
              _Half(Hx, *pack_layers(layersZ, Hx.shape[0]), priors[1][0], {**relays[1], **priors[1][1]}))
    pair_logicals = None
    if logical:
        from .logicals import css_logicals
        pair_logicals = css_logicals(Hx, Hz)       # raises ValueError before any shot is drawn
    if sampler not in (None, "device", "host"):
        raise ValueError("sampler must be 'device', 'host' or None")
    if samples is not None and sampler == "device":
        raise ValueError("samples= decodes the given shots on the host path; it cannot be combined "
                         "with sampler='device' (which draws its own Philox shots)")
    use_dev = sampler == "device" or (sampler is None and samples is None and _device_ok()
                                      and _channel_ok(Hx, Hz))
    dec = _Decode(decType, 50 if hard else decIterations, osd, *_path_kw(use_dev, osd, osd_method, osd_cost), masked,
                  osd_method, osd_cost)
    return _Plan(halves, (1, 0) if correlated == "ZX" else (0, 1), dec, probs, pair_logicals, use_dev)


class _HostChannel:
    """The host path's shot source and counters, with DeviceChannel's two loop
    operations. sample() takes the next batch from `samples` (a tuple
    (sy_z, sy_x, errX, errZ), from row `start`) if given, else draws it from
    `rng`: per-qubit probabilities `probs` if given, else depolarizing.
    count() adds a batch's counters to a dict (nine with `logicals`)."""

    def __init__(self, Hx, Hz, rng, samples=None, probs=None, start=0, logicals=None):
        self.Hx, self.Hz, self.rng, self.samples, self.probs = Hx, Hz, rng, samples, probs
        self.at, self.logicals = start, logicals

    def sample(self, p, B, bits=False):
        if self.samples is not None:
            sl = slice(self.at, self.at + B)
            self.at += B
            return tuple(np.asarray(a)[sl].astype(np.uint8) for a in self.samples)
        if self.probs is not None:
            return sample_channel_vec(self.Hx, self.Hz, self.probs, B, self.rng)
        return sample_channel(self.Hx, self.Hz, p, B, self.rng)

    def count(self, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ, acc):
        if self.logicals is None:
            c = count_outcomes(self.Hx, self.Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
        else:
            c = count_logical_outcomes(self.Hx, self.Hz, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ,
                                       logicals=self.logicals)
        for k in acc:
            acc[k] += c[k]
        return acc


def _batch_loop(ch, count, acc, plan, p, my_shots, batch_size, show, finish=None):
    """The unpipelined loop of both paths: draw a batch, decode its halves
    (OSD inline: `finish` on the device, decode_batch's own on the host),
    count into `acc` (device: an int64 tensor, nothing syncs; host: a dict of
    ints). Returns acc."""
    done = 0
    while done < my_shots:
        B = min(batch_size, my_shots - done)
        sy_z, sy_x, errX, errZ = ch.sample(p, B, bits=plan.dec.packed)
        rX, rZ = _decode_pair(plan, sy_z, sy_x, finish)
        acc = count(sy_z, sy_x, errX, errZ, rX.ehat, rZ.ehat, rX.iters, rZ.iters, acc)
        done += B
        show(done, acc)
    return acc


@dataclass
class _Batch:
    """A batch in flight in the pipelined loop."""
    sy_z: object
    sy_x: object
    errX: object
    errZ: object
    rX: object
    rZ: object
    staged: object = None        # decoders.osd_device_stage's result, once the batch's OSD is queued
    orders: object = None        # the worker thread's future of its NumPy orders


def _pipelined_loop(ch, count, acc, plan, p, my_shots, batch_size, osd_flags, show):
    """Two-stage pipeline over batches: the host computes batch b-1's OSD
    reliability orders (NumPy, the shots the device order leaves) while the
    GPU runs batch b's decode and device OSD; counters accumulate on the device
    (one sync per batch, in the OSD staging; none without OSD until the end).
    `osd_flags` collects the IndexError flags, checked once at the end."""
    Hz, Hx = plan.halves[0].H, plan.halves[1].H
    osd, method = plan.dec.osd, plan.dec.osd_method
    cost = decoders._cost_kw(plan.dec.osd_cost, [h.kw.get("prior") for h in plan.halves])   # one row per half
    done = 0
    pending = None
    phase = 0
    stage_first = False                            # the last batch had device-ordered OSD shots
    tail_min = max(1, batch_size // TAIL_DIV)
    osd_frac = 0.0                                 # OSD shots / half-shots of the last staged batch

    def stage(b):
        """Queue b's device OSD (it waits for b's decode) and hand its NumPy
        orders to the worker thread."""
        nonlocal phase
        b.staged = decoders.osd_device_stage([(Hz, b.sy_z, b.rX), (Hx, b.sy_x, b.rZ)], slot0=2 * phase, order=osd,
                                              method=method, **cost)
        b.orders = _host_worker().submit(_host_orders_on, ch.dev, b.staged)
        phase ^= 1

    while done < my_shots or pending is not None:
        cur = None
        if done < my_shots:
            rem = my_shots - done
            B = min(batch_size, rem)
            if osd >= 0 and osd_frac > 0.2 and tail_min < rem <= batch_size:
                # the last batch's NumPy orders have no next batch to hide
                # behind (the GPU idles until they finish): when OSD is a
                # large share of the work, halve the tail batches, so the
                # final wait is a small batch's (LP118_2 MS-L p = 0.1:
                # +5 %; at low p the extra batches cost more than the
                # short drain saves). Shots keep their indices (the
                # sampler's counter): counters do not depend on batching.
                B = max(tail_min, rem // 2)
            sy_z, sy_x, errX, errZ = ch.sample(p, B, bits=plan.dec.packed)
            cur = _Batch(sy_z, sy_x, errX, errZ, *_decode_pair(plan, sy_z, sy_x))
            done += B
        if cur is not None and osd >= 0 and stage_first:
            # many OSD shots: this batch's device OSD is queued first
            # (staging waits for its decode), so the GPU runs it while the
            # worker thread finishes the previous batch's NumPy orders
            stage(cur)
        if pending is not None:
            b = pending
            items = [(Hz, b.sy_z, b.rX), (Hx, b.sy_x, b.rZ)]
            if osd >= 0:                               # (decoders.py:179-180), on the GPU
                # the status-2 shots' NumPy orders were computed on the
                # worker thread while the GPU decoded this batch
                decoders.osd_device_finish(items, b.staged, osd, host=b.orders.result(), method=method, **cost)
                decoders.osd_status_check(items, defer=osd_flags)
            count(b.sy_z, b.sy_x, b.errX, b.errZ, b.rX.ehat, b.rZ.ehat, b.rX.iters, b.rZ.iters, acc)
        if cur is not None and osd >= 0 and cur.staged is None:
            # few OSD shots: stage (and sync on) this batch's decode now
            stage(cur)
        if cur is not None and osd >= 0:
            stage_first = decoders.osd_staged_on_device(cur.staged)
            osd_frac = sum(sg.shots for sg in cur.staged if sg is not None) / (2.0 * B)
        pending = cur
        if cur is not None:
            show(done)


def simulate_p(Hx: np.ndarray, Hz: np.ndarray, p: float, shots: int = 1000, decType: str = "MS",
               decIterations: int = 99, decSchedule: str = "F", OSDorder: int = -1,
               rngSeed: Optional[int] = None, *, batch_size: Optional[int] = None,
               verbose: bool = True, samples=None, sampler: Optional[str] = None,
               logical: bool = False, correlated: Optional[str] = None, correlated_q1: float = 0.49,
               relay_legs: int = 11, relay_leg_iters: int = 60, relay_sols: int = 1, relay_gamma0: float = 0.125,
               relay_gamma_range=(-0.24, 0.66), relay_seed: int = 0, channel_weights=None,
               osd_method: str = "ref", relay_priors: bool = False, relay_cost: Optional[str] = None,
               osd_cost: str = "hamming") -> dict:
    """One depolarizing probability: sample, decode both halves, count.

    Returns the reference's dict (simulator.py:308-315). `samples`, if given,
    is a tuple (sy_z, sy_x, errX, errZ) to decode instead of sampling (used by
    the parity tests). `sampler`: "device" (HIP sampler + counters on the GPU,
    the default when a device is present), or "host" (NumPy). Extra keyword
    arguments default to reference behaviour.

    `osd_method` (extension; decType MS): "ref" is the reference's OSDdec of
    order OSDorder; "cs" is OSD-CS, the combination sweep with lambda =
    OSDorder in 0..64, on the device and on the host path.
    "cs" with OSDorder < 0, with another decType, or an unknown method raises
    ValueError. `osd_cost` (with "cs"): "hamming", or "prior" (DESIGN.md §3.19):
    OSD-CS keeps the candidate of least prior weight, each half priced with its
    own row of marginals (channel_weights). "prior" without "cs", and where a
    half decodes with one scalar prior (no channel_weights, or equal marginals
    on every qubit), raises ValueError before a shot is drawn.

    `logical` (extension): also test every residual against the pair's logical
    operators (count_logical_outcomes; on the device one counter kernel forms
    all nine counters). The dict then gains the three LOGICAL_KEYS,
    `logical_error_rate` = 1 - decSuccessLogical / shots and its 95 % Wilson
    interval `logical_error_rate_ci95` = [lo, hi]. Raises ValueError if
    (Hx, Hz) is not a CSS pair. With `samples`, sy = H·err is the caller's
    contract.

    `correlated` (extension; MS and BP): "XZ" or "ZX" decodes the halves in
    that order and gives the second one a two-level prior from the first one's
    final estimate (after OSD, if any): under depolarizing noise a qubit that
    carries an X component carries a Z component with probability 1/2 (a Y
    error), one that does not with (p/3)/(1 - 2p/3), and the same with X and Z
    exchanged. The first half is decoded exactly as without the option (prior
    p/3); the second with decode_batch(prior_mask=first estimate,
    p=(p/3)/(1 - 2p/3), p_masked=correlated_q1). `correlated_q1` (0 < q1 <=
    0.5) stands for the 1/2, whose LLR is exactly 0: BP then divides 0 by 0
    (allowed, flagged NONFINITE) and min-sum sets FLAG_MIN_ZERO on almost
    every shot, so the default is 0.49 (LLR 0.04), which decodes as well.
    The second half runs the generic LDS kernel's twin, and with OSD the two
    halves' OSD steps are not pipelined.

    `decType="RELAY"` (extension): relay min-sum, flooding
    only. `decIterations` is the first leg's iteration count and the other
    `relay_legs` - 1 legs run `relay_leg_iters` each; the first leg's memory
    strength is `relay_gamma0`, the later legs draw theirs uniformly from
    `relay_gamma_range` with np.random.default_rng(relay_seed), one table per
    half, the Hz-decoded half first; the decoder stops at `relay_sols`
    solutions. The defaults come from a CPU trial on LP04_0 / LP118_0 and are
    not tuned per code. OSDorder >= 0, correlated= and a decSchedule other than
    "F" raise ValueError.

    `channel_weights` (extension): a non-negative array of shape [3] or [3, n]
    (rows X, Y, Z): qubit j suffers X, Y, Z with probabilities p * w[:, j]
    (biased and inhomogeneous noise; p * sum(w) <= 1 on every qubit, else
    ValueError). The decoders get the true marginals as priors: the X half
    (decodes Hz) p (w_X + w_Y)_j, the Z half p (w_Z + w_Y)_j; a half whose
    marginals are equal on every qubit (uniform bias) calls the scalar entry
    point with that value and keeps the specialised kernels, any other runs
    decode_batch(prior=...) (decode_vprior_kernel). NG / BF
    take no prior: only the sampling changes. Not combinable with correlated=;
    decType "RELAY" needs uniform marginals in both halves (ValueError) unless
    `relay_priors` is set.

    `relay_priors`, `relay_cost` (extension; decType "RELAY"): with
    relay_priors=True a half whose marginals differ decodes with
    RelayConfig(prior=marginals) (relay_vprior_kernel); a half
    with equal marginals takes the scalar relay exactly as without the flag.
    relay_cost is "hamming", "prior" or None: None keeps the solution of least
    prior weight in a half decoded with a row and of least Hamming weight in a
    scalar half; an explicit "prior" on a scalar half raises ValueError.
    """
    plan = _plan(Hx, Hz, p, decType, decIterations, decSchedule, OSDorder, rngSeed, samples, sampler, logical,
                 correlated, correlated_q1,
                 dict(legs=relay_legs, leg_iters=relay_leg_iters, sols=relay_sols, gamma0=relay_gamma0,
                      gamma_range=relay_gamma_range, seed=relay_seed, priors=bool(relay_priors), cost=relay_cost),
                 channel_weights, osd_method, osd_cost)
    osd = plan.dec.osd
    rank, my_shots, my_start, seed = _shard(shots, rngSeed)
    keys = COUNTER_KEYS + LOGICAL_KEYS if logical else COUNTER_KEYS
    show = _progress(f"(p={p:5.2e})", my_shots, verbose and rank == 0, rates=not plan.use_dev)
    if batch_size is None:
        # shots per batch. Without OSD nothing syncs per batch, and 2^20-shot
        # batches amortise the per-batch host work (LP118_0 MS-F p = 0.01:
        # 107 -> 130 M shots/s vs 2^18); with OSD, 2^18 keeps the host's
        # reliability order of one batch overlapped with the next one's decode.
        batch_size = ((1 << 20) if osd < 0 else (1 << 18)) if plan.use_dev else (1 << 16)
    if plan.use_dev:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        ch = DeviceChannel(Hx, Hz, dev, _device_key(seed))
        if plan.probs is not None:
            ch.set_probs(plan.probs)
        count = ch.count_logical_device if logical else ch.count_device
        acc = torch.zeros(len(keys), dtype=torch.int64, device=dev)
        osd_flags = []                             # IndexError flags, checked once at the end
        if plan.dec.masked is None:
            _pipelined_loop(ch, count, acc, plan, p, my_shots, batch_size, osd_flags, show)
        else:
            # Correlated mode: the second half's decode waits for the first half's
            # final estimate, so each batch runs decode, (OSD,) decode, (OSD,)
            # count in stream order. Without OSD the mask is the first decode's
            # bit-packed estimate tensor itself: no kernel, copy or sync between.
            def osd_now(H, syn, r):
                items = [(H, syn, r)]
                decoders.osd_device_finish(items, decoders.osd_device_stage(items, order=osd, method=osd_method),
                                           osd, method=osd_method)
                decoders.osd_status_check(items, defer=osd_flags)
            _batch_loop(ch, count, acc, plan, p, my_shots, batch_size, show, osd_now if osd >= 0 else None)
        decoders.osd_status_raise(osd_flags)
        tot = dict(zip(keys, (int(x) for x in acc.cpu().tolist())))
    else:
        ch = _HostChannel(Hx, Hz, np.random.default_rng(seed), samples, plan.probs, my_start, plan.logicals)
        tot = _batch_loop(ch, ch.count, {k: 0 for k in keys}, plan, p, my_shots, batch_size, show)
    tot = _all_reduce(tot, keys)
    if verbose and rank == 0:
        print()
    res = {
        "DecFailures_X": tot["DecFailures_X"],
        "DecFailures_Z": tot["DecFailures_Z"],
        "decSuccessExact": tot["decSuccessExact"],
        "decSuccessDegen": tot["decSuccessDegen"],
        "Avg_number_of_iterations_X": tot["nIterAccX"] / float(shots),
        "Avg_number_of_iterations_Z": tot["nIterAccZ"] / float(shots),
    }
    if logical:
        for k in LOGICAL_KEYS:
            res[k] = tot[k]
        res["logical_error_rate"] = 1. - tot["decSuccessLogical"] / float(shots)
        res["logical_error_rate_ci95"] = wilson_interval(shots - tot["decSuccessLogical"], shots)
    return res


class DevicePhenomHalf:
    """Device-side shot source and outcome counter of one CSS half under
    phenomenological noise (phenom_kernels.hip via qldpc_phenom_sample /
    qldpc_phenom_count): `H` [m, n] detects the half's errors, `L` [k, n] is
    its logical table, `rounds` = T. Shot s of key k is the same whatever the
    batching. Packed outputs are int64 words, bit j % 64 of word j / 64."""

    def __init__(self, H, L, rounds, device, seed, shot0=0):
        import torch
        self.torch = torch
        self.dev = torch.device(device)
        self.T = int(rounds)
        self.m, self.n = H.shape
        self.M, self.N = spacetime.spacetime_shape(self.n, self.m, self.T)
        self.W, self.NW, self.MW = (self.n + 63) // 64, (self.N + 63) // 64, (self.M + 63) // 64
        with torch.cuda.device(self.dev):
            self.code = _lib.code_for(H, self.dev.index)
            self.table = _lib.PhenomTable(self.code, L)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.shot = int(shot0)

    def sample(self, p_data, q, B, bits=False, want_fired=False):
        """(det, E) of the next B shots: det uint8 [B, M] (bits: int64
        [B, ceil(M/64)]), E int64 [B, ceil(n/64)]; with want_fired also the
        fired rows int64 [B, ceil(N/64)]."""
        torch = self.torch
        det = torch.empty((B, self.MW), dtype=torch.int64, device=self.dev) if bits else \
            torch.empty((B, self.M), dtype=torch.uint8, device=self.dev)
        E = torch.empty((B, self.W), dtype=torch.int64, device=self.dev)
        fired = torch.empty((B, self.NW), dtype=torch.int64, device=self.dev) if want_fired else None
        _lib.phenom_sample(self.code, self.T, p_data, q, self.seed, self.shot, B, det.data_ptr(),
                           _fmt(bits), E.data_ptr(), fired.data_ptr() if want_fired else None, _stream(self.dev))
        self.shot += int(B)
        return (det, E, fired) if want_fired else (det, E)

    def count_device(self, det, E, ehat, iters, acc=None, want_shots=False, want_class=False):
        """Adds the batch's four counters (failures, logical errors, successes,
        iteration sum) to `acc` (int64 [4] device tensor, created if None),
        without a host sync. det as sample() wrote it; ehat uint8 [B, N] or
        int64 [B, ceil(N/64)]; iters int32 [B]. want_class: returns (acc,
        class uint8 [B]); want_shots: (acc, class, flip words int64
        [B, ceil(k/64)], residual words int64 [B, ceil(n/64)])."""
        torch = self.torch
        if acc is None:
            acc = torch.zeros(4, dtype=torch.int64, device=self.dev)
        B = det.shape[0]
        d_bits, e_bits = det.dtype == torch.int64, ehat.dtype == torch.int64
        ts = (det, E, ehat, iters, acc)
        if not all(t.is_contiguous() and t.device == self.dev for t in ts) or \
                tuple(det.shape) != ((B, self.MW) if d_bits else (B, self.M)) or \
                tuple(ehat.shape) != ((B, self.NW) if e_bits else (B, self.N)) or \
                det.dtype not in (torch.uint8, torch.int64) or ehat.dtype not in (torch.uint8, torch.int64) or \
                tuple(E.shape) != (B, self.W) or E.dtype != torch.int64 or tuple(iters.shape) != (B,) or \
                iters.dtype != torch.int32 or tuple(acc.shape) != (4,) or acc.dtype != torch.int64:
            raise ValueError("count_device: buffers do not match the batch layout")
        cls = torch.empty(B, dtype=torch.uint8, device=self.dev) if (want_shots or want_class) else None
        flips = torch.empty((B, self.table.kw), dtype=torch.int64, device=self.dev) if want_shots else None
        resid = torch.empty((B, self.W), dtype=torch.int64, device=self.dev) if want_shots else None
        P = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        _lib.phenom_count(self.code, self.table, self.T, B, det.data_ptr(), _fmt(d_bits), E.data_ptr(),
                          ehat.data_ptr(), _fmt(e_bits), iters.data_ptr(), acc.data_ptr(), P(cls), P(flips), P(resid),
                          _stream(self.dev))
        if want_shots:
            return acc, cls, flips, resid
        return (acc, cls) if want_class else acc

    def advance(self, det, ehat, iters, done=None, west=None, witers=None, nxt=None, bits=False):
        """The step between two windows of sliding-window decoding
        (spacetime.window_advance on the device, one launch of
        phenom_window_kernel, no host sync). `done` = (a, R, closed, C), the
        window just decoded, with its estimate `west` (uint8 [B, N_w] or int64
        [B, ceil(N_w/64)]) and iteration counts `witers` int32 [B]: its
        committed columns go into `ehat` (uint8 [B, N] or int64
        [B, ceil(N/64)], in place) and witers is added to `iters` (int32 [B], in
        place). `nxt` = (a', R', ..), the next window: returns its syndrome,
        uint8 [B, R' m] (bits: int64 [B, ceil(R' m / 64)]), cut from `det` (as
        sample() wrote it) and corrected by the committed measurement estimate.
        Each buffer's format is its own."""
        torch = self.torch
        B = det.shape[0]
        d_bits, e_bits = det.dtype == torch.int64, ehat.dtype == torch.int64
        ts = [det, ehat, iters]
        ok = det.dtype in (torch.uint8, torch.int64) and ehat.dtype in (torch.uint8, torch.int64) and \
            tuple(det.shape) == ((B, self.MW) if d_bits else (B, self.M)) and \
            tuple(ehat.shape) == ((B, self.NW) if e_bits else (B, self.N)) and \
            tuple(iters.shape) == (B,) and iters.dtype == torch.int32
        w_bits = False
        if done is not None:
            a, R, closed, C = (int(v) for v in done)
            if not (0 <= a and 1 <= R and a + R <= self.T and 1 <= C <= R) or \
                    (a + R == self.T) != bool(closed) or (closed and C != R):
                raise ValueError(f"window {tuple(done)} does not lie in [0, {self.T})")
            Nw = spacetime.window_shape(self.n, self.m, R, closed)[1]
            ok = ok and west is not None and witers is not None and west.dtype in (torch.uint8, torch.int64)
            if ok:
                w_bits = west.dtype == torch.int64
                ts += [west, witers]
                ok = tuple(west.shape) == ((B, (Nw + 63) // 64) if w_bits else (B, Nw)) and \
                    tuple(witers.shape) == (B,) and witers.dtype == torch.int32
        if nxt is not None:
            a2, R2 = int(nxt[0]), int(nxt[1])
            if not (0 <= a2 and 1 <= R2 and a2 + R2 <= self.T) or (done is not None and (closed or a2 != a + C)):
                raise ValueError(f"next window {tuple(nxt)} does not follow {done} in [0, {self.T})")
        elif done is None:
            raise ValueError("advance: neither a decoded window nor a next one")
        if not ok or not all(t.is_contiguous() and t.device == self.dev for t in ts):
            raise ValueError("advance: buffers do not match the batch layout")
        syn = None
        if nxt is not None:
            syn = torch.empty((B, (R2 * self.m + 63) // 64), dtype=torch.int64, device=self.dev) if bits else \
                torch.empty((B, R2 * self.m), dtype=torch.uint8, device=self.dev)
        if B == 0:
            return syn
        P = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        _lib.phenom_window(self.code, self.T, B, done, P(west) if done is not None else None, _fmt(w_bits),
                           P(witers) if done is not None else None, P(ehat), _fmt(e_bits), P(iters),
                           None if nxt is None else (a2, R2), P(det), _fmt(d_bits), P(syn), _fmt(bits),
                           _stream(self.dev))
        return syn


class _HostPhenomHalf:
    """DevicePhenomHalf's two loop operations on the host (the NumPy twins in
    spacetime.py): sample() draws from `rng`, which the halves share, and
    count_device() adds to an int64 [4] NumPy array."""

    def __init__(self, H, L, rounds, rng):
        self.H, self.L, self.T, self.rng = H, L, rounds, rng

    def sample(self, p_data, q, B, bits=False):
        return spacetime.sample_phenomenological(self.H, self.T, p_data, q, B, self.rng)

    def count_device(self, det, E, ehat, iters, acc, want_class=True):
        c, (cls, _, _) = spacetime.count_phenomenological(self.H, self.L, self.T, det, E, ehat, iters, want_shots=True)
        acc += (c["failures"], c["logical_errors"], c["successes"], c["iterations"])
        return acc, cls

    def advance(self, det, ehat, iters, done=None, west=None, witers=None, nxt=None, bits=False):
        m, n = self.H.shape
        return spacetime.window_advance(n, m, self.T, det, ehat, iters, done, west, witers, nxt)


def _hbm_priors_checked(hbm_priors):
    """hbm_priors= of simulate_phenomenological / simulate_dem / simulate as a
    bool (ValueError for anything else: a truthy path or number is a mistake)."""
    if not isinstance(hbm_priors, (bool, np.bool_)):
        raise ValueError("hbm_priors must be True or False")
    return bool(hbm_priors)


def _window_schedule(T, window, commit):
    """spacetime.window_schedule of window= / commit= (None without window=),
    with the ValueErrors every entry point raises."""
    if window is None:
        if commit is not None:
            raise ValueError("commit needs window (sliding-window decoding)")
        return None
    return spacetime.window_schedule(T, window, 1 if commit is None else commit)


def _decode_windows(recs, s, wins, det, dec, use_dev):
    """One half-batch window by window: advance (commit the last window, cut
    and correct the next syndrome), decode, OSD if asked; the last advance
    commits the closed window. Returns (the full estimate, summed iterations),
    in the decode path's formats. Nothing here syncs with the host."""
    B = det.shape[0]
    if use_dev:
        torch = s.torch
        ehat = torch.empty((B, s.NW), dtype=torch.int64, device=s.dev) if dec.packed else \
            torch.empty((B, s.N), dtype=torch.uint8, device=s.dev)
        iters = torch.zeros(B, dtype=torch.int32, device=s.dev)
    else:
        m, n = s.H.shape
        ehat = np.zeros((B, spacetime.spacetime_shape(n, m, s.T)[1]), np.uint8)
        iters = np.zeros(B, np.int32)
    last, r = None, None
    for w in wins:
        syn = s.advance(det, ehat, iters, last, None if r is None else r.ehat, None if r is None else r.iters, w,
                        bits=dec.packed)
        h = recs[w[1], w[2]]
        r = _decode_half(h, syn, dec)
        if use_dev and dec.osd >= 0:
            decoders.apply_osd_device(h.H, syn, r, dec.osd, method=dec.osd_method, **_osd_cost_kw(dec, h))
        last = w
    s.advance(det, ehat, iters, last, r.ehat, r.iters, None)
    return ehat, iters


def simulate_phenomenological(Hx: np.ndarray, Hz: np.ndarray, p: float, q: float, rounds: int, shots: int = 1000,
                              decType: str = "MS", decIterations: int = 99, decSchedule: str = "F",
                              OSDorder: int = -1, rngSeed: Optional[int] = None, *,
                              batch_size: Optional[int] = None, sampler: Optional[str] = None,
                              verbose: bool = True, window: Optional[int] = None, commit: Optional[int] = None,
                              osd_method: str = "ref", hbm_priors: bool = False, osd_cost: str = "hamming",
                              **unsupported) -> dict:
    """Phenomenological noise (extension; no reference counterpart): `rounds`
    = T rounds of syndrome extraction with measurement error probability `q`,
    the last round measured perfectly, decoded over each half's space-time
    check matrix (spacetime.spacetime_matrix).

    The two halves are independent channels: in every round each qubit carries
    an X component (detected by Hz, the X half) with probability p_data = 2p/3
    and a Z component (detected by Hx) with the same probability, the true
    marginals of depolarizing noise of strength p, as with --bias. The Y
    correlation between the halves is not modelled. Each half's detectors
    d_t = H e_t ^ u_t ^ u_{t-1} are decoded with the priors p_data on data
    columns and q on measurement columns: the scalar entry point when they are
    equal (every specialised kernel and the HBM-resident one apply, at any
    size), else decode_batch(prior=spacetime_prior(...)) with
    decode_vprior_kernel's limits (its NotImplementedError is passed on).
    `hbm_priors`: library option vprior_hbm is set around the whole run, so a
    matrix past those limits (windows included) decodes with
    hbm_tile_vprior_kernel at any size instead of raising;
    matrices within them decode as without it.

    decType "MS" or "BP"; decSchedule "F", or "L" / "S" with layers from
    schedule.layerize of the half's own space-time matrix (none of the
    reference's cross-wiring). OSDorder >= 0 (MS only, as in simulate_p) runs
    decoders.apply_osd_device per half after its decode, unpipelined;
    `osd_method` as in simulate_p ("cs": OSD-CS with lambda = OSDorder, on every
    window's decode too; on the device its limits are the block kernel's,
    m <= 512 and n <= 1087 of the matrix decoded, else NotImplementedError).
    `osd_cost` as in simulate_p: "prior" prices every decode's OSD-CS, each
    window's too, with the prior row of the matrix decoded; with p_data == q
    (or a matrix of data columns alone) the decode takes one scalar prior and
    "prior" raises ValueError before a shot is drawn.
    `sampler`: "device" (phenom_kernels.hip, the default with a device) or
    "host" (the NumPy twins in spacetime.py, drawn from
    np.random.default_rng([rngSeed, rank]), the X half first in every batch).
    On the device the X half's Philox key is simulate_p's
    (SeedSequence([rngSeed, rank])) and the Z half's is that ^
    0x9E3779B97F4A7C15. With torch.distributed initialised the shots shard as
    in simulate_p: contiguous shares, a key per rank, one all_reduce(SUM).

    A half-shot is class 2 (decoder failure) if the estimate does not
    reproduce the detectors, else class 1 (logical error) if L·(E ^ Ê) != 0
    with E / Ê the XOR of the true / estimated data errors over the rounds,
    else class 0. Returns DecFailures_X/Z, logicalErrors_X/Z, nIterAccX/Z,
    decSuccessLogical (shots with both halves class 0), logical_error_rate =
    1 - decSuccessLogical / shots, its 95 % Wilson interval
    logical_error_rate_ci95, logical_error_rate_per_round =
    1 - (1 - LER)^(1/rounds), and rounds, q, p_data.

    `window` = W, `commit` = F (default 1): sliding-window decoding (DESIGN.md
    §3.14). Each half is decoded W rounds at a time (spacetime.window_schedule):
    an open window (spacetime.window_matrix) commits its first F rounds into
    the full estimate, the next window's first detector round is corrected by
    the committed measurement estimate, and the last window is the closed
    space-time matrix of the rounds left. Between windows runs one launch of
    phenom_window_kernel (DevicePhenomHalf.advance); the host does nothing per
    window. Every decode path applies to the window matrices (at most two per
    half, each with its own layers and priors), so the decoder's state is
    bounded by W whatever T is; shots are sampled and scored at full T as
    without `window`, and the iterations are summed over the windows. T <= W is
    the whole-matrix decode. The results gain window, commit and windows (their
    number).

    ValueError: decType RELAY / NG / BF, correlated= and channel_weights= (not
    defined for this model), probabilities outside [0, 1), rounds < 1, a pair
    that is not CSS, window < 1, commit outside [1, window], either one not an
    integer, commit without window, hbm_priors not a bool."""
    from .logicals import css_logicals
    if _hbm_priors_checked(hbm_priors):
        with _lib.options(vprior_hbm=1):       # once around the run: an option change drops the cached launch plans
            return simulate_phenomenological(Hx, Hz, p, q, rounds, shots, decType, decIterations, decSchedule,
                                             OSDorder, rngSeed, batch_size=batch_size, sampler=sampler,
                                             verbose=verbose, window=window, commit=commit, osd_method=osd_method,
                                             osd_cost=osd_cost, **unsupported)
    for k_ in unsupported:
        if k_ in ("correlated", "channel_weights", "correlated_q1", "logical", "samples"):
            raise ValueError(f"simulate_phenomenological does not take {k_}=: the phenomenological model has "
                             "independent halves with uniform data noise")
        raise TypeError(f"simulate_phenomenological() got an unexpected keyword argument {k_!r}")
    if decType in ("RELAY",) + tuple(_lib.HARD_ALGOS):
        raise ValueError(f"decType {decType} is not available on space-time matrices (MS or BP)")
    if decType not in ("MS", "BP"):
        raise ValueError("Unrecognized decoder type.")
    if decSchedule not in ("F", "L", "S"):
        raise ValueError("Unrecognized decoder scheduling option.")
    _osd_method(osd_method, OSDorder, decType)
    T = int(rounds)
    if T < 1 or T != rounds:
        raise ValueError("rounds must be an integer >= 1")
    if not (0.0 <= float(p) < 1.0) or not (0.0 <= float(q) < 1.0):
        raise ValueError("p and q must lie in [0, 1)")
    wins = _window_schedule(T, window, commit)      # None without window=
    if sampler not in (None, "device", "host"):
        raise ValueError("sampler must be 'device', 'host' or None")
    if int(shots) < 0:
        raise ValueError("shots must be >= 0")
    Hx, Hz = np.asarray(Hx), np.asarray(Hz)
    n = Hx.shape[1]
    Lx, Lz = css_logicals(Hx, Hz)                  # ValueError unless (Hx, Hz) is a CSS pair
    p_data = 2.0 * float(p) / 3.0
    q = float(q)
    osd = OSDorder if decType == "MS" else -1      # as simulate_p
    rank, my_shots, _, seed = _shard(shots, rngSeed)
    use_dev = sampler == "device" or (sampler is None and _device_ok())
    if batch_size is None:
        # posteriors (OSD) and byte rows cost 9 N bytes per half-shot
        batch_size = ((1 << 18) if osd < 0 else (1 << 14)) if use_dev else (1 << 14)
    dec = _Decode(decType, decIterations, osd, *_path_kw(use_dev, osd, osd_method, osd_cost), osd_method=osd_method,
                  osd_cost=osd_cost)
    # the matrices decoded: (rounds, closed) -> a _Half per CSS half. Without
    # window= (and with T <= W) that is the closed matrix of all T rounds
    kinds = sorted({(R, closed) for _, R, closed, _ in (wins or [(0, T, True, T)])})
    halves = []                                    # X half: (Hz, Lz); Z half: (Hx, Lx)
    for H, L in ((Hz, Lz), (Hx, Lx)):
        recs = {}
        for R, closed in kinds:
            Hw = spacetime.spacetime_matrix(H, R) if closed else spacetime.window_matrix(H, R)
            pr = (spacetime.spacetime_prior if closed else spacetime.window_prior)(n, H.shape[0], R, p_data, q)
            layers = None if decSchedule == "F" else layerize(Hw, serial=decSchedule == "S")
            lp, lr = pack_layers(layers, Hw.shape[0])
            recs[R, closed] = _Half(Hw, lp, lr, *_half_prior(pr, False), (H, L))
        halves.append(recs)
    _osd_cost(osd_cost, osd_method, [h.kw.get("prior") for recs in halves for h in recs.values()])
    sliding = wins is not None and len(wins) > 1
    show = _progress(f"(p={p:5.2e}, q={q:5.2e}, T={T})", my_shots, verbose and rank == 0)
    if use_dev:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        key = _device_key(seed)
        src = [DevicePhenomHalf(*recs[kinds[0]].code, T, dev, k) for recs, k in zip(halves, (key, key ^ PHENOM_Z_KEY))]
        for recs in halves:
            for h in recs.values():
                if h.kw:
                    # the vector-prior kernel's limits are met when its launch is
                    # planned: one all-zero detector row per matrix, so a shape past
                    # them is refused (NotImplementedError) before any shot is drawn
                    _decode_half(h, torch.zeros((1, h.H.shape[0]), dtype=torch.uint8, device=dev),
                                 dec._replace(iters=1, kw={}))
        accs = [torch.zeros(k, dtype=torch.int64, device=dev) for k in (4, 4, 1)]
    else:
        rng = np.random.default_rng(seed)          # one generator: the X half draws first in every batch
        src = [_HostPhenomHalf(*recs[kinds[0]].code, T, rng) for recs in halves]
        accs = [np.zeros(k, np.int64) for k in (4, 4, 1)]
    both = accs[2]                                 # shots with both halves class 0
    done = 0
    while done < my_shots:
        B = min(batch_size, my_shots - done)
        cls = []
        for recs, s, acc in zip(halves, src, accs):  # (the two halves and their accumulators)
            det, E = s.sample(p_data, q, B, bits=dec.packed)
            if sliding:
                ehat, iters = _decode_windows(recs, s, wins, det, dec, use_dev)
            else:
                h = recs[kinds[0]]
                r = _decode_half(h, det, dec)
                if use_dev and osd >= 0:
                    decoders.apply_osd_device(h.H, det, r, osd, method=osd_method, **_osd_cost_kw(dec, h))
                ehat, iters = r.ehat, r.iters
            cls.append(s.count_device(det, E, ehat, iters, acc, want_class=True)[1])
        both += ((cls[0] | cls[1]) == 0).sum()
        done += B
        show(done)
    aX, aZ, ok = (a.cpu().tolist() if use_dev else a.tolist() for a in accs)
    tot = _all_reduce(dict(zip(PHENOM_KEYS, (aX[0], aZ[0], aX[1], aZ[1], aX[3], aZ[3], ok[0]))), PHENOM_KEYS)
    if verbose and rank == 0:
        print()
    res = dict(tot)
    ler = 1. - tot["decSuccessLogical"] / float(shots) if shots else 0.0
    res["logical_error_rate"] = ler
    res["logical_error_rate_ci95"] = wilson_interval(shots - tot["decSuccessLogical"], shots)
    res["logical_error_rate_per_round"] = 1. - (1. - ler) ** (1. / T)
    res["rounds"], res["q"], res["p_data"] = T, q, p_data
    if wins is not None:
        res["window"], res["commit"], res["windows"] = int(window), 1 if commit is None else int(commit), len(wins)
    return res


def format_phenomenological_results(p, results, shots):
    """The phenomenological mode's table."""
    lines = ["\n             ===          PHENOMENOLOGICAL NOISE: SPACE-TIME DECODING          ===\n",
             "   Depolarizing probability | Meas. error |  T  | Logical error rate (per round) |"
             "     95 % interval      | Failures (X,Z) | Logical errors (X,Z)",
             "----------------------------+-------------+-----+--------------------------------+"
             "------------------------+----------------+----------------------"]
    win = any("window" in r for r in results)      # sliding-window decoding: a W/F column
    if win:
        lines[1] += " | Window W/F"
        lines[2] += "-+-----------"
    for pT, r in zip(p, results):
        lo, hi = r["logical_error_rate_ci95"]
        lines.append(f"         {pT:10.2e}         |  {r['q']:9.2e}  | {r['rounds']:3} |      {r['logical_error_rate']:7.2e} "
                     f"({r['logical_error_rate_per_round']:7.2e})       |  [{lo:8.2e}, {hi:8.2e}]  |  "
                     f"{r['DecFailures_X']:6},{r['DecFailures_Z']:6} |     {r['logicalErrors_X']:6},"
                     f"{r['logicalErrors_Z']:6}")
        if win:
            lines[-1] += f"        |   {r['window']:3}/{r['commit']:<3}" if "window" in r else "        |"
    return "\n".join(lines)


class DeviceDem:
    """Device-side shot source and outcome counter of a detector error model
    (dem_kernels.hip via qldpc_dem_sample / qldpc_dem_count): DevicePhenomHalf's
    twin for a dem.Dem, without the sliding-window step. Shot s of key k is
    the same whatever the batching. Packed outputs are int64 words, bit j % 64
    of word j / 64."""

    def __init__(self, dem, device, seed, shot0=0):
        import torch
        self.torch = torch
        self.dev = torch.device(device)
        self.dem = dem
        self.M, self.K, self.N = dem.num_detectors, dem.num_observables, dem.num_errors
        self.MW, self.KW, self.NW = (self.M + 63) // 64, (self.K + 63) // 64, (self.N + 63) // 64
        with torch.cuda.device(self.dev):
            self.code = _lib.code_for(dem.H, self.dev.index)
            self.table = _lib.DemTable(self.code, dem.L, dem.priors)
        self.seed = int(seed) & ((1 << 64) - 1)
        self.shot = int(shot0)

    def sample(self, B, bits=False, want_fired=False):
        """(det, obs) of the next B shots: det uint8 [B, M] (bits: int64
        [B, ceil(M/64)]), obs int64 [B, ceil(K/64)]; with want_fired also the
        fired rows int64 [B, ceil(N/64)]."""
        torch = self.torch
        det = torch.empty((B, self.MW), dtype=torch.int64, device=self.dev) if bits else \
            torch.empty((B, self.M), dtype=torch.uint8, device=self.dev)
        obs = torch.empty((B, self.KW), dtype=torch.int64, device=self.dev)
        fired = torch.empty((B, self.NW), dtype=torch.int64, device=self.dev) if want_fired else None
        P = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        _lib.dem_sample(self.table, self.seed, self.shot, B, P(det), _fmt(bits), P(obs), P(fired), _stream(self.dev))
        self.shot += int(B)
        return (det, obs, fired) if want_fired else (det, obs)

    def count_device(self, det, obs, ehat, iters, acc=None, want_shots=False, want_class=False):
        """Adds the batch's four counters (failures, logical errors, successes,
        iteration sum) to `acc` (int64 [4] device tensor, created if None),
        without a host sync. det and obs as sample() wrote them; ehat uint8
        [B, N] or int64 [B, ceil(N/64)]; iters int32 [B]. want_class: returns
        (acc, class uint8 [B]); want_shots: (acc, class, flip words int64
        [B, ceil(K/64)] = L ehat ^ obs)."""
        torch = self.torch
        if acc is None:
            acc = torch.zeros(4, dtype=torch.int64, device=self.dev)
        B = det.shape[0]
        d_bits, e_bits = det.dtype == torch.int64, ehat.dtype == torch.int64
        ts = (det, obs, ehat, iters, acc)
        if not all(t.is_contiguous() and t.device == self.dev for t in ts) or \
                tuple(det.shape) != ((B, self.MW) if d_bits else (B, self.M)) or \
                tuple(ehat.shape) != ((B, self.NW) if e_bits else (B, self.N)) or \
                det.dtype not in (torch.uint8, torch.int64) or ehat.dtype not in (torch.uint8, torch.int64) or \
                tuple(obs.shape) != (B, self.KW) or obs.dtype != torch.int64 or tuple(iters.shape) != (B,) or \
                iters.dtype != torch.int32 or tuple(acc.shape) != (4,) or acc.dtype != torch.int64:
            raise ValueError("count_device: buffers do not match the batch layout")
        cls = torch.empty(B, dtype=torch.uint8, device=self.dev) if (want_shots or want_class) else None
        flips = torch.empty((B, self.KW), dtype=torch.int64, device=self.dev) if want_shots else None
        P = lambda t: t.data_ptr() if t is not None and t.numel() else None  # noqa: E731
        _lib.dem_count(self.table, B, P(det), _fmt(d_bits), P(obs), P(ehat), _fmt(e_bits), P(iters), acc.data_ptr(),
                       P(cls), P(flips), _stream(self.dev))
        if want_shots:
            return acc, cls, flips
        return (acc, cls) if want_class else acc


class _HostDem:
    """DeviceDem's two loop operations on the host (the NumPy twins in dem.py):
    sample() draws from `rng`, count_device() adds to an int64 [4] NumPy array."""

    def __init__(self, dem, rng):
        self.dem, self.rng, self.shot = dem, rng, 0

    def sample(self, B, bits=False):
        from .dem import sample_dem
        self.shot += int(B)
        return sample_dem(self.dem, B, self.rng)

    def count_device(self, det, obs, ehat, iters, acc):
        from .dem import count_dem
        c = count_dem(self.dem, det, obs, ehat, iters)
        acc += (c["failures"], c["logical_errors"], c["successes"], c["iterations"])
        return acc


def simulate_dem(dem, shots: int = 1000, decType: str = "MS", decIterations: int = 99, decSchedule: str = "F",
                 OSDorder: int = -1, rngSeed: Optional[int] = None, *, batch_size: Optional[int] = None,
                 sampler: Optional[str] = None, verbose: bool = True, osd_method: str = "ref",
                 hbm_priors: bool = False, relay_priors: bool = False, relay_cost: Optional[str] = None,
                 relay_legs: int = 11, relay_leg_iters: int = 60, relay_sols: int = 1, relay_gamma0: float = 0.125,
                 relay_gamma_range=(-0.24, 0.66), relay_seed: int = 0, osd_cost: str = "hamming") -> dict:
    """Monte-Carlo decoding of a detector error model (extension; no reference
    counterpart): `dem` is a dem.Dem (dem.load_dem reads Stim's .dem text).
    Each shot fires every mechanism independently with its own probability,
    the detectors H f are decoded over H with the mechanisms' probabilities as
    priors, and the estimate is scored against the observables L f (DESIGN.md
    §3.16).

    The decode takes the scalar entry point when every prior is equal (every
    specialised kernel and the HBM-resident one apply, at any size), else
    decode_batch(prior=dem.priors) with decode_vprior_kernel's limits: its
    NotImplementedError is raised when the launch is planned, before any shot
    is drawn. decType "MS" or "BP" (MS rows have at most 32 entries under
    per-column priors; detector rows of circuit-level models are often
    longer, and BP has no such limit). `hbm_priors`: library option vprior_hbm
    is set around the whole run, so a model past those limits decodes with
    hbm_tile_vprior_kernel at any size and row degree
    instead of raising; a model within them decodes as without it. decSchedule "F", or "L" / "S" with
    layers from schedule.layerize(dem.H). OSDorder >= 0 applies to MS and to
    BP here (decoders.apply_osd_device on the device path, decoders.apply_osd
    on the host), `osd_method` as in simulate_p; `osd_cost` "prior" (with "cs",
    DESIGN.md §3.19) prices OSD-CS's candidates with the mechanisms' own
    probabilities (ValueError where they are all equal). `sampler`: "device"
    (dem_kernels.hip, the default with a device; Philox key
    SeedSequence([rngSeed, rank]) as simulate_p) or "host" (dem.sample_dem
    from np.random.default_rng([rngSeed, rank])). With torch.distributed
    initialised the shots shard as in simulate_p: contiguous shares, a key per
    rank, one all_reduce(SUM).

    A shot is class 2 (decoder failure) if H ehat differs from the detectors,
    else class 1 (logical error) if L ehat differs from the observables, else
    class 0. Returns DecFailures, logicalErrors, decSuccess, nIterAcc,
    logical_error_rate = 1 - decSuccess / shots, its 95 % Wilson interval
    logical_error_rate_ci95, and detectors, errors, observables (M, N, K).

    decType "RELAY" with `relay_priors=True`: relay min-sum with the
    mechanisms' probabilities as its prior row (relay_vprior_kernel, DESIGN.md
    §3.18; the scalar relay when they are all equal). decIterations is the
    first leg's count and relay_legs, relay_leg_iters, relay_sols,
    relay_gamma0, relay_gamma_range, relay_seed and relay_cost are
    simulate_p's (one table of memory strengths; the defaults still come from
    the code-capacity trial). OSDorder >= 0, a decSchedule other than "F" and
    hbm_priors raise ValueError with it; a model past the relay's limits (a
    detector row of more than 32 entries, tables past 16 bits or the LDS)
    raises NotImplementedError before any shot is drawn.

    ValueError: decType RELAY without relay_priors, NG / BF or unknown, an
    unknown schedule or sampler, negative shots, an osd_method that does not
    fit, hbm_priors not a bool."""
    from .dem import Dem
    if not isinstance(dem, Dem):
        raise ValueError("dem must be a qldpcsim_amd.dem.Dem (dem.load_dem / dem.parse_dem make one)")
    relay_on = decType == "RELAY" and bool(relay_priors)
    if relay_on and _hbm_priors_checked(hbm_priors):
        raise ValueError("decType RELAY has no HBM-resident variant (hbm_priors)")
    if (relay_priors or relay_cost is not None) and decType != "RELAY":
        raise ValueError("relay_priors and relay_cost go with decType RELAY")
    if _hbm_priors_checked(hbm_priors):
        with _lib.options(vprior_hbm=1):       # once around the run: an option change drops the cached launch plans
            return simulate_dem(dem, shots, decType, decIterations, decSchedule, OSDorder, rngSeed,
                                batch_size=batch_size, sampler=sampler, verbose=verbose, osd_method=osd_method,
                                osd_cost=osd_cost)
    if decType in _lib.HARD_ALGOS or (decType == "RELAY" and not relay_on):
        raise ValueError(f"decType {decType} is not available on detector error models (MS or BP)")
    if decType not in ("MS", "BP", "RELAY"):
        raise ValueError("Unrecognized decoder type.")
    if decSchedule not in ("F", "L", "S"):
        raise ValueError("Unrecognized decoder scheduling option.")
    relay_kw = {}
    if relay_on:
        if OSDorder >= 0:
            raise ValueError("decType RELAY has no OSD step (OSDorder must be < 0)")
        if decSchedule != "F":
            raise ValueError("decType RELAY runs the flooding schedule only (decSchedule 'F')")
        if int(relay_legs) < 1 or int(relay_leg_iters) < 1 or int(relay_sols) < 1 or int(decIterations) < 1:
            raise ValueError("relay_legs, relay_leg_iters, relay_sols and decIterations must be >= 1")
        lo, hi = (float(x) for x in relay_gamma_range)
        if not (np.isfinite([lo, hi, float(relay_gamma0)]).all() and lo <= hi):
            raise ValueError("relay_gamma0 and relay_gamma_range (lo <= hi) must be finite")
        p_half, kw_half = _half_prior(dem.priors, False)
        leg_iters = [int(decIterations)] + [int(relay_leg_iters)] * (int(relay_legs) - 1)
        gammas = np.empty((len(leg_iters), dem.num_errors), np.float64)
        gammas[0] = relay_gamma0
        gammas[1:] = np.random.default_rng(relay_seed).uniform(lo, hi, (len(leg_iters) - 1, dem.num_errors))
        relay_kw = {"relay": _relay_config(leg_iters, gammas, relay_sols, kw_half.get("prior"), relay_cost)}
    decoders.osd_method_checked(osd_method, OSDorder, decType)
    _osd_cost(osd_cost, osd_method, [_half_prior(dem.priors, False)[1].get("prior")])
    if sampler not in (None, "device", "host"):
        raise ValueError("sampler must be 'device', 'host' or None")
    if int(shots) < 0:
        raise ValueError("shots must be >= 0")
    osd = int(OSDorder) if OSDorder >= 0 else -1   # MS and BP alike: there is no reference behaviour to mirror
    rank, my_shots, _, seed = _shard(shots, rngSeed)
    use_dev = sampler == "device" or (sampler is None and _device_ok())
    if batch_size is None:
        batch_size = ((1 << 18) if osd < 0 else (1 << 14)) if use_dev else (1 << 14)
    dec = _Decode(decType, decIterations, osd, *_path_kw(use_dev, osd, osd_method, osd_cost), osd_method=osd_method,
                  osd_cost=osd_cost)
    layers = None if decSchedule == "F" else layerize(dem.H, serial=decSchedule == "S")
    if relay_on:                                   # the row, if any, travels in the RelayConfig
        half = _Half(dem.H, *pack_layers(layers, dem.num_detectors), p_half, relay_kw)
    else:
        half = _Half(dem.H, *pack_layers(layers, dem.num_detectors), *_half_prior(dem.priors, False))
    show = _progress(f"(DEM {dem.num_detectors} x {dem.num_errors})", my_shots, verbose and rank == 0)
    if use_dev:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        src = DeviceDem(dem, dev, _device_key(seed))
        acc = torch.zeros(4, dtype=torch.int64, device=dev)
        zero = torch.zeros((1, dem.num_detectors), dtype=torch.uint8, device=dev)
    else:
        src = _HostDem(dem, np.random.default_rng(seed))
        acc = np.zeros(4, np.int64)
        zero = np.zeros((1, dem.num_detectors), np.uint8)
    if half.kw:
        # the vector-prior kernel's and the relay's limits are met when the
        # launch is planned: one all-zero detector row, so a model past them is
        # refused (NotImplementedError) before any shot is drawn
        _decode_half(half, zero, dec._replace(iters=1, kw={}))
    done = 0
    while done < my_shots:
        B = min(batch_size, my_shots - done)
        det, obs = src.sample(B, bits=dec.packed)
        r = _decode_half(half, det, dec)
        if use_dev and osd >= 0:
            decoders.apply_osd_device(half.H, det, r, osd, method=osd_method, **_osd_cost_kw(dec, half))
        src.count_device(det, obs, r.ehat, r.iters, acc)
        done += B
        show(done)
    tot = _all_reduce(dict(zip(DEM_KEYS, acc.cpu().tolist() if use_dev else acc.tolist())), DEM_KEYS)
    if verbose and rank == 0:
        print()
    res = dict(tot)
    res["logical_error_rate"] = 1. - tot["decSuccess"] / float(shots) if shots else 0.0
    res["logical_error_rate_ci95"] = wilson_interval(shots - tot["decSuccess"], shots)
    res["detectors"], res["errors"], res["observables"] = dem.num_detectors, dem.num_errors, dem.num_observables
    return res


def format_dem_results(name, r, shots):
    """The detector error model mode's table (one record)."""
    lo, hi = r["logical_error_rate_ci95"]
    return "\n".join([
        "\n             ===          DETECTOR ERROR MODEL          ===\n",
        "   Model (detectors x errors, observables) | Logical error rate |     95 % interval      | Failures | "
        "Logical errors | Average iterations",
        "-------------------------------------------+--------------------+------------------------+----------+-"
        "---------------+--------------------",
        f"   {name[-22:]:>22} ({r['detectors']} x {r['errors']}, {r['observables']})".ljust(43)
        + f"|      {r['logical_error_rate']:7.2e}      |  [{lo:8.2e}, {hi:8.2e}]  | {r['DecFailures']:8} | "
        f"{r['logicalErrors']:14} | {r['nIterAcc'] / max(shots, 1):10.3f}"])


def _run_dem(path, shots, decType, decIterations, decSchedule, OSDorder, rngSeed, batch_size, sampler, resultsFile,
             osd_method, hbm_priors=False, relay=None, osd_cost="hamming"):
    """The command line's --dem mode: load the model, simulate_dem, print the
    table; rank 0 writes the record (with the run's parameters; "hbm_priors"
    only when set; "osd_cost" only when it is "prior"; `relay`, simulate_dem's relay_* keywords under
    --relay-priors, only when given) to --results."""
    relay = dict(relay or {})
    from .dem import load_dem
    _, rank, world = _dist()
    dem = load_dem(path)
    if sampler is None:
        sampler = "device" if _device_ok() else "host"
    res = simulate_dem(dem, shots=shots, decType=decType, decIterations=decIterations, decSchedule=decSchedule,
                       OSDorder=OSDorder, rngSeed=rngSeed, batch_size=batch_size, sampler=sampler, verbose=True,
                       osd_method=osd_method, **({"hbm_priors": True} if _hbm_priors_checked(hbm_priors) else {}),
                       **({"osd_cost": osd_cost} if osd_cost != "hamming" else {}), **relay)
    if rank == 0:
        print(format_dem_results(path, res, shots))
        if resultsFile:
            meta = {"dem": path, "shots": shots, "decType": decType, "decIterations": decIterations,
                    "decSchedule": decSchedule, "OSDorder": OSDorder, "rngSeed": rngSeed, "world": world,
                    "sampler": sampler, **decoders._method_kw("osd_method", osd_method),
                    **({"osd_cost": osd_cost} if osd_cost != "hamming" else {}),
                    **({"hbm_priors": True} if hbm_priors else {}),
                    **{k: (list(v) if k == "relay_gamma_range" else v) for k, v in relay.items()}}
            import json
            import os
            with open(resultsFile + ".tmp", "w") as f:
                json.dump({"meta": meta, "result": res}, f, indent=1)
            os.replace(resultsFile + ".tmp", resultsFile)
    return res


def format_results(p, results, shots):
    """The reference's results table (simulator.py:342-347)."""
    lines = ["\n                             ===          SIMULATION RESULTS          ===\n",
             "   Depolarizing probability | qBlock error rate | Decoding failures (X,Z) | Average iterations (X,Z)",
             "----------------------------+-------------------+-------------------------+---------------------------"]
    for pT, r in zip(p, results):
        qbler = 1. - (r["decSuccessExact"] + r["decSuccessDegen"]) / shots
        lines.append(f"         {pT:10.2e}         |     {qbler:7.2e}      |       "
                     f"{r['DecFailures_X']:5},{r['DecFailures_Z']:5}       |      "
                     f"{r['Avg_number_of_iterations_X']:5.2f}, {r['Avg_number_of_iterations_Z']:5.2f}")
    return "\n".join(lines)


def format_logical_results(p, results, shots):
    """The logical option's table, printed after the reference's."""
    lines = ["\n                  ===          LOGICAL ERROR RATES          ===\n",
             "   Depolarizing probability | Logical block error rate |     95 % interval      | Logical errors (X,Z)",
             "----------------------------+--------------------------+------------------------+----------------------"]
    for pT, r in zip(p, results):
        lo, hi = r["logical_error_rate_ci95"]
        lines.append(f"         {pT:10.2e}         |         {r['logical_error_rate']:7.2e}         |  "
                     f"[{lo:8.2e}, {hi:8.2e}]  |     {r['logicalErrors_X']:6},{r['logicalErrors_Z']:6}")
    return "\n".join(lines)


def _load_results(path, meta):
    """Per-p results already in a resumable results file (JSON), if its
    run parameters match `meta`; else empty."""
    import json
    import os
    if not path or not os.path.exists(path):
        return {}
    with open(path) as f:
        doc = json.load(f)
    if doc.get("meta") != meta:
        raise ValueError(f"{path} holds results of a different run: {doc.get('meta')}")
    return {float(k): v for k, v in doc.get("results", {}).items()}


def _save_results(path, meta, done):
    import json
    import os
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump({"meta": meta, "results": {repr(k): v for k, v in sorted(done.items())}}, f, indent=1)
    os.replace(tmp, path)                      # atomic: a killed run leaves the last good file


def _sweep(p, meta, resultsFile, on_point, rank, point):
    """The resumable p-sweep: point(pT) for every pT the results file does not
    hold yet (its run parameters must equal `meta`), timed for on_point; rank 0
    saves the file after each. Returns every point's result, in p's order."""
    done = _load_results(resultsFile, meta)
    results = []
    for pT in p:
        if float(pT) in done:
            results.append(done[float(pT)])
            continue
        t0 = time.perf_counter()
        r = point(pT)
        if on_point is not None:
            on_point(pT, r, time.perf_counter() - t0)
        results.append(r)
        done[float(pT)] = r
        if resultsFile and rank == 0:
            _save_results(resultsFile, meta, done)
    return results


def simulate(HxFile: str, HzFile: str, p, shots: int = 1000, decType: str = "MS",
             decIterations: int = 99, decSchedule: str = "F", OSDorder: int = -1,
             rngSeed: Optional[int] = None, *, batch_size: Optional[int] = None, verbose: bool = True,
             return_results: bool = False, sampler: Optional[str] = None,
             resultsFile: Optional[str] = None, on_point=None, logical: bool = False,
             correlated: Optional[str] = None, correlated_q1: float = 0.49,
             relay_legs: int = 11, relay_leg_iters: int = 60, relay_sols: int = 1, relay_gamma0: float = 0.125,
             relay_gamma_range=(-0.24, 0.66), relay_seed: int = 0, bias: Optional[float] = None,
             channel_weights=None, rounds: Optional[int] = None, meas_error: Optional[float] = None,
             window: Optional[int] = None, commit: Optional[int] = None, osd_method: str = "ref",
             hbm_priors: bool = False, relay_priors: bool = False, relay_cost: Optional[str] = None,
             osd_cost: str = "hamming"):
    """p-sweep + results table (simulator.py:319-347). Returns None like the
    reference unless return_results=True.

    logical (extension): simulate_p(logical=True) for every point; a second
    table with the logical block error rate, its 95 % interval and the logical
    errors per half follows the reference's. The results file's meta then
    holds "logical": true (a file written without the option is refused).

    correlated, correlated_q1 (extension): simulate_p's correlated X/Z
    decoding for every point; both enter the results file's meta, so a sweep
    is never resumed across modes.

    relay_* (extension; decType "RELAY"): simulate_p's relay min-sum settings;
    all of them enter the results file's meta. relay_priors, relay_cost:
    simulate_p's, passed on and recorded ("relay_priors": true, "relay_cost")
    only when relay_priors is set; relay_cost without it, or either of them
    with rounds, raises ValueError.

    bias, channel_weights (extension; one of them at most): simulate_p's
    channel_weights for every point, given as a bias eta (bias_weights) or as
    the weights themselves ([3] or [3, n]). Both enter the results file's meta,
    the weights by a SHA-256 digest of their float64 bytes.

    rounds, meas_error (extension): phenomenological noise —
    simulate_phenomenological(rounds=rounds, q=meas_error) for every point
    (meas_error defaults to each point's 2p/3), with a results table of its
    own. "rounds" and "q" enter the results file's meta. meas_error without
    rounds, logical, correlated, bias and channel_weights raise ValueError.
    window, commit (extension; with rounds): simulate_phenomenological's
    sliding-window decoding; when given they enter the results file's meta (a
    resumed sweep with other values is a different sweep) and the table shows
    W/F. window without rounds, commit without window, window < 1, commit
    outside [1, window] and non-integers raise ValueError.
    hbm_priors (extension; with rounds): simulate_phenomenological's
    hbm_priors for every point; when set it enters the results file's meta as
    "hbm_priors": true. Without rounds it raises ValueError (the pair's own
    halves are always within decode_vprior_kernel's limits or refused alike).

    osd_method (extension; decType MS): simulate_p's / simulate_phenomenological's
    OSD method for every point, "ref" or "cs" (OSD-CS, lambda = OSDorder). A
    method other than "ref" enters the results file's meta as "osd_method" (a
    file without the key is a "ref" sweep), so a sweep is never resumed across
    methods. osd_cost (with osd_method "cs"): simulate_p's /
    simulate_phenomenological's cost for every point; "prior" enters the
    results file's meta as "osd_cost" (a file without the key is a "hamming"
    sweep) and is refused as there, before the first point runs.

    resultsFile (extension): a JSON file the sweep writes after every
    p-point; a rerun with the same arguments skips the points already there
    (resumable long sweeps). Only rank 0 writes it.
    on_point (extension): called as on_point(pT, result, seconds) after each
    p-point this call computed (bench.py times the sweep's points with it)."""
    Hx = load_matrix(HxFile)
    Hz = load_matrix(HzFile)
    assert max(p) <= 1. and min(p) >= 0.
    _, rank, world = _dist()
    method = {} if _osd_method(osd_method, OSDorder, decType) == "ref" else {"osd_method": osd_method}
    if osd_cost not in decoders.OSD_COSTS:
        raise ValueError(f"osd_cost must be one of {decoders.OSD_COSTS}, got {osd_cost!r}")
    if osd_cost == "prior":
        decoders.osd_cost_checked(osd_cost, osd_method, True)
        method["osd_cost"] = osd_cost
    if rounds is None and meas_error is not None:
        raise ValueError("meas_error needs rounds (the phenomenological model)")
    if rounds is None and (window is not None or commit is not None):
        raise ValueError("window / commit need rounds (the phenomenological model)")
    if _hbm_priors_checked(hbm_priors) and rounds is None:
        raise ValueError("hbm_priors needs rounds (the phenomenological model) or a detector error model")
    if relay_cost is not None and not relay_priors:
        raise ValueError("relay_cost needs relay_priors")
    if relay_priors and (decType != "RELAY" or rounds is not None):
        raise ValueError("relay_priors goes with decType RELAY, without rounds (a phenomenological model decodes "
                         "as a detector error model: simulate_dem)")
    if rounds is not None:
        if logical or correlated is not None or bias is not None or channel_weights is not None:
            raise ValueError("rounds= (phenomenological noise) cannot be combined with logical, correlated, bias or "
                             "channel_weights")
        if sampler is None:
            sampler = "device" if _device_ok() else "host"
        meta = {"Hx": HxFile, "Hz": HzFile, "shots": shots, "decType": decType, "decIterations": decIterations,
                "decSchedule": decSchedule, "OSDorder": OSDorder, "rngSeed": rngSeed, "world": world,
                "sampler": sampler, "rounds": int(rounds), "q": None if meas_error is None else float(meas_error)}
        win = {}                                   # window= / commit= / hbm_priors=: passed on and recorded only when given
        if _window_schedule(rounds, window, commit) is not None:
            win = {"window": int(window), "commit": 1 if commit is None else int(commit)}
            meta.update(win)
        if hbm_priors:
            win["hbm_priors"] = True
            meta["hbm_priors"] = True
        meta.update(method)
        results = _sweep(p, meta, resultsFile, on_point, rank, lambda pT: simulate_phenomenological(
            Hx, Hz, pT, 2 * pT / 3 if meas_error is None else meas_error, rounds, shots=shots, decType=decType,
            decIterations=decIterations, decSchedule=decSchedule, OSDorder=OSDorder, rngSeed=rngSeed,
            batch_size=batch_size, sampler=sampler, verbose=verbose, **win, **method))
        if rank == 0:
            print(format_phenomenological_results(p, results, shots))
        return results if return_results else None
    if sampler is None:                       # the resolved shot source is part of the run
        sampler = "device" if (_device_ok() and _channel_ok(Hx, Hz)) else "host"
    meta = {"Hx": HxFile, "Hz": HzFile, "shots": shots, "decType": decType,
            "decIterations": decIterations, "decSchedule": decSchedule, "OSDorder": OSDorder,
            "rngSeed": rngSeed, "world": world, "sampler": sampler, **method}
    extra = dict(method)
    if logical:
        meta["logical"] = True
        extra["logical"] = True
    if correlated is not None:
        meta["correlated"] = correlated
        meta["correlated_q1"] = correlated_q1
        extra["correlated"] = correlated
        extra["correlated_q1"] = correlated_q1
    if decType == "RELAY":
        extra.update(relay_legs=int(relay_legs), relay_leg_iters=int(relay_leg_iters), relay_sols=int(relay_sols),
                     relay_gamma0=float(relay_gamma0), relay_gamma_range=[float(x) for x in relay_gamma_range],
                     relay_seed=int(relay_seed))
        if relay_priors:
            extra.update(relay_priors=True, relay_cost=relay_cost)
        meta.update({k: v for k, v in extra.items() if k.startswith("relay_")})
    if bias is not None and channel_weights is not None:
        raise ValueError("give either bias or channel_weights, not both")
    if bias is not None:
        extra["channel_weights"] = bias_weights(bias)
        meta["bias"] = float(bias)
    elif channel_weights is not None:
        import hashlib
        w = np.ascontiguousarray(channel_weights, dtype=np.float64)
        extra["channel_weights"] = w
        meta["channel_weights"] = {"shape": list(w.shape), "sha256": hashlib.sha256(w.tobytes()).hexdigest()}
    if "channel_weights" in extra:
        for pT in p:                          # every point is checked before the first one runs
            channel_probs(pT, extra["channel_weights"], Hx.shape[1])
    results = _sweep(p, meta, resultsFile, on_point, rank, lambda pT: simulate_p(
        Hx, Hz, p=pT, shots=shots, rngSeed=rngSeed, decType=decType, decIterations=decIterations,
        decSchedule=decSchedule, OSDorder=OSDorder, batch_size=batch_size, verbose=verbose, sampler=sampler, **extra))
    if rank == 0:
        print(format_results(p, results, shots))
        if logical:
            print(format_logical_results(p, results, shots))
    return results if return_results else None


def _init_dist_from_env():
    """One process per GPU under torchrun (WORLD_SIZE > 1 in the environment):
    bind this rank to its device and join the process group (RCCL over xGMI;
    QLDPC_SIM_BACKEND=gloo to rehearse on CPU or with ranks sharing a GPU).
    Returns True if this call created the group."""
    import os
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world <= 1:
        return False
    import torch
    import torch.distributed as dist
    if dist.is_initialized():
        return False
    backend = os.environ.get("QLDPC_SIM_BACKEND", "nccl" if torch.cuda.is_available() else "gloo")
    if torch.cuda.is_available():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        ndev = torch.cuda.device_count()
        if local >= ndev:
            if backend == "nccl":
                # one process per GPU: under RCCL a second rank on a device is
                # a launch error, not something to fold silently (bench.py too)
                raise RuntimeError(f"LOCAL_RANK {local} but only {ndev} HIP device(s) visible: launch at "
                                   "most one rank per GPU (QLDPC_SIM_BACKEND=gloo rehearses more ranks)")
            local %= max(1, ndev)              # gloo rehearsal: ranks may share a device
        torch.cuda.set_device(local)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
            return True
    dist.init_process_group(backend)
    return True


def main(argv=None):
    parser = argparse.ArgumentParser(description="Stim-based QC-LDPC depolarizing-channel simulator.")
    # --dem replaces the code and the channel: only then are --Hx, --Hz and --p not required
    pair = not any(a == "--dem" or a.startswith("--dem=") for a in (sys.argv[1:] if argv is None else argv))
    parser.add_argument("--Hx", required=pair, help="Path to Hx parity-check matrix (.npy).")
    parser.add_argument("--Hz", required=pair, help="Path to Hz parity-check matrix (.npy).")
    parser.add_argument("--p", type=float, nargs="+", required=pair, help="Depolarizing probability.")
    parser.add_argument("--shots", type=int, default=1000, help="Number of Monte Carlo shots.")
    parser.add_argument("--rngSeed", type=int, default=None, help="RNG seed.")
    parser.add_argument("--decType", choices=["NG", "BF", "MS", "BP", "RELAY"], default="MS",
                        help="Decoder type: [NG] Naive Greedy; [BF] Bit Flipping; [MS] Min-Sum; "
                             "[BP] Belief Propagation; [RELAY] relay min-sum (extension: flooding min-sum with "
                             "memory in chained disordered legs; no OSD, --decIterations is the first leg's "
                             "count; the relay defaults come from a CPU trial and are not tuned per code).")
    parser.add_argument("--relay-legs", type=int, default=11, dest="relay_legs", help="RELAY: number of legs.")
    parser.add_argument("--relay-leg-iters", type=int, default=60, dest="relay_leg_iters",
                        help="RELAY: iterations of every leg after the first.")
    parser.add_argument("--relay-sols", type=int, default=1, dest="relay_sols",
                        help="RELAY: solutions to stop at (the lightest is kept).")
    parser.add_argument("--relay-gamma0", type=float, default=0.125, dest="relay_gamma0",
                        help="RELAY: memory strength of the first leg.")
    parser.add_argument("--relay-gamma-range", type=float, nargs=2, default=[-0.24, 0.66], metavar=("LO", "HI"),
                        dest="relay_gamma_range", help="RELAY: later legs draw their memory strengths from U(LO, HI).")
    parser.add_argument("--relay-seed", type=int, default=0, dest="relay_seed",
                        help="RELAY: seed of the memory-strength tables.")
    # (argparse.SUPPRESS: without the flags the printed namespace is what it was)
    parser.add_argument("--relay-priors", action="store_true", default=argparse.SUPPRESS, dest="relay_priors",
                        help="RELAY: decode unequal priors (--channel-weights marginals, a --dem model's mechanism "
                             "probabilities) with the per-variable-prior relay kernel instead of refusing them.")
    parser.add_argument("--relay-cost", choices=["hamming", "prior"], default=argparse.SUPPRESS, dest="relay_cost",
                        help="With --relay-priors: which of the solutions found is kept, the one of least Hamming "
                             "weight or of least prior weight (default: prior where a prior row decodes, else "
                             "hamming).")
    parser.add_argument("--decIterations", type=int, default=99, help="Number of decoding iterations.")
    parser.add_argument("--decSchedule", choices=["F", "L", "S"], default="F",
                        help="Decoder scheduling method: [F] flooding; [L] layered; [S] serial.")
    parser.add_argument("--OSDorder", type=int, default=-1, help="Ordered Statistics Decoding order.")
    parser.add_argument("--osd-method", dest="osd_method", choices=["ref", "cs"], default="ref",
                        help="OSD method (decType MS): ref = the reference's OSDdec of order --OSDorder; cs = OSD-CS, "
                             "the combination sweep with lambda = --OSDorder (0..64).")
    # (argparse.SUPPRESS: without the flag the printed namespace is what it was)
    parser.add_argument("--osd-cost", dest="osd_cost", choices=["hamming", "prior"], default=argparse.SUPPRESS,
                        help="With --osd-method cs: what OSD-CS minimises, the Hamming weight (default) or the prior "
                             "weight under the decode's per-column priors (--bias, --channel-weights, --rounds with "
                             "--meas-error, --dem).")
    parser.add_argument("--batch", type=int, default=None,
                        help="Shots per batch (default on the GPU: 2^20 without OSD, 2^18 with OSD; "
                             "2^16 on the host path).")
    parser.add_argument("--sampler", choices=["device", "host"], default=None,
                        help="Where shots are sampled and counted (default: device if present).")
    parser.add_argument("--results", default=None,
                        help="Resumable results file (JSON, written after every p-point).")
    parser.add_argument("--logical", action="store_true",
                        help="Also count logical errors (residuals tested against the CSS pair's logical "
                             "operators) and print the logical block error rate with its 95 %% interval.")
    parser.add_argument("--correlated", choices=["XZ", "ZX"], default=None,
                        help="Correlated X/Z decoding (MS, BP): decode the halves in this order and give the "
                             "second one a two-level prior from the first one's estimate.")
    parser.add_argument("--correlated-q1", type=float, default=0.49, dest="correlated_q1",
                        help="Prior of the second component on a qubit flagged by the first half (exactly 1/2 "
                             "in theory; its LLR 0 is degenerate for the decoders: default 0.49).")
    parser.add_argument("--bias", type=float, default=None, metavar="ETA",
                        help="Z-biased Pauli channel with pZ / (pX + pY) = ETA and pX = pY, at total error "
                             "probability p (0.5: depolarizing); the decoders get the true marginals as priors.")
    parser.add_argument("--channel-weights", default=None, dest="channel_weights", metavar="FILE.npy",
                        help="Pauli weights, shape [3] or [3, n] (rows X, Y, Z): qubit j suffers X, Y, Z with "
                             "probabilities p * w[:, j]; the decoders get each qubit's true marginal as its prior.")
    # (argparse.SUPPRESS: without the flags the printed namespace is what it was)
    parser.add_argument("--rounds", type=int, default=argparse.SUPPRESS, metavar="T",
                        help="Phenomenological noise: T rounds of syndrome extraction (the last one perfect), "
                             "decoded over each half's space-time check matrix (MS, BP); data errors 2p/3 per "
                             "half, qubit and round.")
    parser.add_argument("--meas-error", type=float, default=argparse.SUPPRESS, dest="meas_error", metavar="Q",
                        help="Phenomenological noise: measurement error probability per check and round "
                             "(default with --rounds: 2p/3).")
    parser.add_argument("--window", type=int, default=argparse.SUPPRESS, metavar="W",
                        help="With --rounds: sliding-window decoding, W rounds at a time (the decoder's state is "
                             "bounded by W whatever T is); T <= W is the whole-matrix decode.")
    parser.add_argument("--commit", type=int, default=argparse.SUPPRESS, metavar="F",
                        help="With --window: rounds committed per window, 1 <= F <= W (default 1).")
    parser.add_argument("--dem", default=argparse.SUPPRESS, metavar="FILE",
                        help="Decode a detector error model instead of a CSS pair: Stim's .dem text, or .npz with "
                             "H, L and priors (MS, BP; --OSDorder applies to both). Takes the place of --Hx, --Hz "
                             "and --p.")
    parser.add_argument("--hbm-priors", action="store_true", default=argparse.SUPPRESS, dest="hbm_priors",
                        help="With --rounds or --dem: decode unequal priors past the LDS kernel's limits (matrix "
                             "size, min-sum rows of more than 32 entries, state past the LDS) with the HBM-resident "
                             "per-variable-prior kernel instead of refusing them.")
    args = parser.parse_args(argv)
    osd_cost = getattr(args, "osd_cost", "hamming")
    if osd_cost == "prior" and args.osd_method != "cs":
        parser.error("--osd-cost prior needs --osd-method cs")
    relay_priors = getattr(args, "relay_priors", False)
    if hasattr(args, "relay_cost") and not relay_priors:
        parser.error("--relay-cost needs --relay-priors")
    if relay_priors and args.decType != "RELAY":
        parser.error("--relay-priors needs --decType RELAY")
    relay_names = ("relay_legs", "relay_leg_iters", "relay_sols", "relay_gamma0", "relay_gamma_range", "relay_seed")
    dem_file = getattr(args, "dem", None)
    if dem_file is not None:
        given = [f for f, v in (("--Hx", args.Hx), ("--Hz", args.Hz), ("--p", args.p),
                                ("--rounds", getattr(args, "rounds", None)),
                                ("--window", getattr(args, "window", None)), ("--logical", args.logical or None),
                                ("--correlated", args.correlated), ("--bias", args.bias),
                                ("--channel-weights", args.channel_weights)) if v is not None]
        if given:
            parser.error(f"--dem cannot be combined with {', '.join(given)}")
        if args.decType not in ("MS", "BP") and not (args.decType == "RELAY" and relay_priors):
            parser.error("--dem decodes with MS or BP")
        if relay_priors and getattr(args, "hbm_priors", False):
            parser.error("--relay-priors cannot be combined with --hbm-priors")
        if args.osd_method == "cs" and not 0 <= args.OSDorder <= decoders.OSD_CS_MAX_LAMBDA:
            parser.error(f"--osd-method cs takes its lambda from --OSDorder: 0..{decoders.OSD_CS_MAX_LAMBDA}")
        own_group = _init_dist_from_env()
        _, rank, _ = _dist()
        if rank == 0:
            print("\n   Command line arguments:")
            print(args)
            print("")
        try:
            _run_dem(dem_file, args.shots, args.decType, args.decIterations, args.decSchedule, args.OSDorder,
                     args.rngSeed, args.batch, args.sampler, args.results, args.osd_method,
                     hbm_priors=getattr(args, "hbm_priors", False), osd_cost=osd_cost,
                     relay=({**{k: getattr(args, k) for k in relay_names}, "relay_priors": True,
                             "relay_cost": getattr(args, "relay_cost", None)} if relay_priors else None))
        finally:
            if own_group:
                import torch.distributed as dist
                dist.destroy_process_group()
        return
    if args.bias is not None and args.channel_weights is not None:
        parser.error("--bias and --channel-weights exclude each other")
    rounds, meas_error = getattr(args, "rounds", None), getattr(args, "meas_error", None)
    if meas_error is not None and rounds is None:
        parser.error("--meas-error needs --rounds")
    window, commit = getattr(args, "window", None), getattr(args, "commit", None)
    if window is not None and rounds is None:
        parser.error("--window needs --rounds")
    if commit is not None and window is None:
        parser.error("--commit needs --window")
    if window is not None and window < 1:
        parser.error("--window must be >= 1")
    if commit is not None and not (1 <= commit <= window):
        parser.error("--commit must lie in [1, --window]")
    if getattr(args, "hbm_priors", False) and rounds is None:
        parser.error("--hbm-priors needs --rounds or --dem")
    if rounds is not None:
        if rounds < 1:
            parser.error("--rounds must be >= 1")
        if args.logical or args.correlated or args.bias is not None or args.channel_weights:
            parser.error("--rounds cannot be combined with --logical, --correlated, --bias or --channel-weights")
        if args.decType not in ("MS", "BP"):
            parser.error("--rounds decodes with MS or BP")
        if relay_priors:
            parser.error("--relay-priors cannot be combined with --rounds (decode the model as a --dem)")
    own_group = _init_dist_from_env()              # torchrun: shots shard over the ranks
    _, rank, _ = _dist()
    if rank == 0:
        print("\n   Command line arguments:")
        print(args)
        print("")
    try:
        simulate(HxFile=args.Hx, HzFile=args.Hz, p=args.p, shots=args.shots, decType=args.decType,
                 decIterations=args.decIterations, decSchedule=args.decSchedule,
                 OSDorder=args.OSDorder, rngSeed=args.rngSeed, batch_size=args.batch,
                 sampler=args.sampler, resultsFile=args.results, **({"logical": True} if args.logical else {}),
                 **({"correlated": args.correlated, "correlated_q1": args.correlated_q1} if args.correlated else {}),
                 **({"bias": args.bias} if args.bias is not None else {}),
                 **({"channel_weights": np.load(args.channel_weights)} if args.channel_weights else {}),
                 **({"rounds": rounds, "meas_error": meas_error} if rounds is not None else {}),
                 **({"window": window, "commit": commit} if window is not None else {}),
                 **({"hbm_priors": True} if getattr(args, "hbm_priors", False) else {}),
                 **({"osd_method": args.osd_method} if args.osd_method != "ref" else {}),
                 **({"osd_cost": osd_cost} if osd_cost != "hamming" else {}),
                 **({k: getattr(args, k) for k in relay_names} if args.decType == "RELAY" else {}),
                 **({"relay_priors": True, "relay_cost": getattr(args, "relay_cost", None)} if relay_priors else {}))
    finally:
        if own_group:
            import torch.distributed as dist
            dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1:])

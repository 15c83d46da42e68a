"""Phenomenological noise: the space-time check matrix of one CSS half and the
NumPy twins of the device kernels (phenom_kernels.hip). Pure NumPy.

A half is (H, L): H [m, n] detects this half's errors (the X half: Hz), L
[k, n] is the logical table logicals.css_logicals pairs with it (Lz). Over
T = rounds rounds of syndrome extraction, round t draws a fresh data error
e_t (probability p_data per qubit) and, unless it is the last round, a
measurement error u_t (probability q per check); the last round is measured
perfectly. The detectors are

    d_t = H e_t ^ u_t ^ u_{t-1},    u_{-1} = u_{T-1} = 0.

Columns (N = T n + (T-1) m, round-major): round t owns data columns
t (n+m) + j, j < n, and for t < T-1 measurement columns t (n+m) + n + c,
c < m. Rows (M = T m): row t m + c holds row c of H on round t's data
columns, measurement column (t, c) if t < T-1 and (t-1, c) if t >= 1. With
T = 1 the matrix is H.

Outcome of a shot, with E = XOR_t e_t, Ehat = XOR_t ehat_t (the fold of the
estimate's data blocks) and r = E ^ Ehat:
    class 2  decoder failure: H_st ehat != d
    class 1  logical error:   not 2, and L r mod 2 != 0
    class 0  success:         not 2, and L r mod 2 == 0
When the detectors match, H r = 0 follows by telescoping, so the test
against L decides membership in the stabiliser group.
"""
import numpy as np

__all__ = ["spacetime_shape", "spacetime_matrix", "spacetime_prior", "fold_data", "column_thresholds", "detectors",
           "sample_phenomenological", "count_phenomenological"]


def _rounds(rounds):
    T = int(rounds)
    if T < 1 or T != rounds:
        raise ValueError("rounds must be an integer >= 1")
    return T


def spacetime_shape(n, m, rounds):
    """(M, N) = (T m, T n + (T-1) m)."""
    T = _rounds(rounds)
    return T * m, T * n + (T - 1) * m


def spacetime_matrix(H, rounds):
    """The space-time check matrix int8 [T m, T n + (T-1) m] of H (see the
    module docstring for the layout)."""
    H = (np.asarray(H) % 2).astype(np.int8)
    if H.ndim != 2:
        raise ValueError("H must be a 2-D matrix")
    T = _rounds(rounds)
    m, n = H.shape
    M, N = spacetime_shape(n, m, T)
    S = np.zeros((M, N), np.int8)
    c = np.arange(m)
    for t in range(T):
        o = t * (n + m)
        S[t * m:(t + 1) * m, o:o + n] = H
        if t < T - 1:
            S[t * m + c, o + n + c] = 1
        if t >= 1:
            S[t * m + c, o - m + c] = 1
    return S


def _is_data(n, m, T):
    """bool [N]: True on data columns."""
    _, N = spacetime_shape(n, m, T)
    return (np.arange(N) % (n + m)) < n if N else np.zeros(0, bool)


def spacetime_prior(n, m, rounds, p_data, q):
    """The prior float64 [N] of the space-time matrix: p_data on data
    columns, q on measurement columns."""
    T = _rounds(rounds)
    for name, v in (("p_data", p_data), ("q", q)):
        if not (0.0 <= float(v) < 1.0):
            raise ValueError(f"{name} must lie in [0, 1) (got {v})")
    return np.where(_is_data(n, m, T), float(p_data), float(q)).astype(np.float64)


def fold_data(bits, n, m, rounds):
    """[B, N] 0/1 rows -> uint8 [B, n]: the XOR of the T data blocks."""
    T = _rounds(rounds)
    bits = np.asarray(bits)
    _, N = spacetime_shape(n, m, T)
    if bits.ndim != 2 or bits.shape[1] != N:
        raise ValueError(f"bits must be [B, {N}]")
    out = np.zeros((bits.shape[0], n), np.uint8)
    for t in range(T):
        o = t * (n + m)
        out ^= (bits[:, o:o + n] & 1).astype(np.uint8)
    return out


def column_thresholds(n, m, rounds, p_data, q):
    """uint64 [N]: column J fires iff its 32-bit draw u < thr_J, thr =
    min(2^32, floor(prob 2^32)) — what qldpc_channel_table(prob, 0, 0) yields."""
    pr = spacetime_prior(n, m, rounds, p_data, q)
    return np.minimum(2.0 ** 32, np.floor(pr * 2.0 ** 32)).astype(np.uint64)


def _mod2(A, Bt):
    """A·Btᵀ mod 2 for 0/1 arrays (float32 product, exact below 2^24 terms)."""
    return ((np.asarray(A).astype(np.float32) @ np.asarray(Bt).astype(np.float32).T).astype(np.int64) & 1).astype(np.uint8)


def detectors(H, rounds, fired):
    """uint8 [B, T m]: d_t = H e_t ^ u_t ^ u_{t-1} of fired rows [B, N], formed
    round by round from H (the materialised matrix is never built)."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    T = _rounds(rounds)
    m, n = H.shape
    fired = np.asarray(fired).astype(np.uint8) & 1
    det = np.zeros((fired.shape[0], T * m), np.uint8)
    for t in range(T):
        o = t * (n + m)
        d = _mod2(fired[:, o:o + n], H)
        if t < T - 1:
            d ^= fired[:, o + n:o + n + m]
        if t >= 1:
            d ^= fired[:, o - m:o]
        det[:, t * m:(t + 1) * m] = d
    return det


def sample_phenomenological(H, rounds, p_data, q, shots, rng, want_fired=False):
    """NumPy twin of qldpc_phenom_sample: one 32-bit integer per column drawn
    from `rng` against the device sampler's thresholds (column_thresholds).
    Returns (det uint8 [shots, T m], E uint8 [shots, n]); with want_fired also
    the fired rows uint8 [shots, N]."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    T = _rounds(rounds)
    m, n = H.shape
    thr = column_thresholds(n, m, T, p_data, q)
    u = rng.integers(0, 1 << 32, (int(shots), thr.size), dtype=np.uint64)
    fired = (u < thr).astype(np.uint8)
    det = detectors(H, T, fired)
    E = fold_data(fired, n, m, T)
    return (det, E, fired) if want_fired else (det, E)


def _pack_words(F):
    """0/1 [B, k] -> uint64 [B, ceil(k/64)], bit i % 64 of word i / 64."""
    B, k = F.shape
    kw = (k + 63) // 64
    b = np.zeros((B, 8 * kw), dtype=np.uint8)
    if k:
        pk = np.packbits(F.astype(np.uint8), axis=1, bitorder="little")
        b[:, :pk.shape[1]] = pk
    return b.view("<u8").astype(np.uint64, copy=False).reshape(B, kw)


def count_phenomenological(H, L, rounds, det, E, ehat, iters, want_shots=False):
    """NumPy twin of qldpc_phenom_count. det uint8 [B, T m], E uint8 [B, n],
    ehat uint8 [B, N] (the space-time estimate), iters [B]. Returns
    {"failures", "logical_errors", "successes", "iterations"}; with want_shots
    also (class uint8 [B], flip words uint64 [B, ceil(k/64)] = L r mod 2,
    residual r = E ^ fold(ehat) uint8 [B, n]), as computed for every class."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    L = (np.asarray(L) % 2).astype(np.uint8).reshape(-1, H.shape[1])
    T = _rounds(rounds)
    m, n = H.shape
    ehat = np.asarray(ehat).astype(np.uint8) & 1
    fail = np.any(detectors(H, T, ehat) != np.asarray(det), axis=1)
    r = (np.asarray(E).astype(np.uint8) & 1) ^ fold_data(ehat, n, m, T)
    F = _mod2(r, L) if L.shape[0] else np.zeros((r.shape[0], 0), np.uint8)
    cls = np.where(fail, 2, np.any(F != 0, axis=1).astype(np.uint8)).astype(np.uint8)
    out = {"failures": int((cls == 2).sum()), "logical_errors": int((cls == 1).sum()),
           "successes": int((cls == 0).sum()), "iterations": int(np.asarray(iters, dtype=np.int64).sum())}
    if want_shots:
        return out, (cls, _pack_words(F), r)
    return out

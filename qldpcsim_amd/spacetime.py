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

Sliding-window decoding (the window_* functions at the end): the decoder
works on W rounds at a time instead of the whole matrix; see there.
"""
import numpy as np

__all__ = ["spacetime_shape", "spacetime_matrix", "spacetime_prior", "fold_data", "column_thresholds", "detectors",
           "sample_phenomenological", "count_phenomenological", "window_matrix", "window_prior", "window_shape",
           "window_schedule", "window_advance"]


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


# ---------------------------------------------------------------------------
# Sliding-window decoding: the decoder works on a window of W
# rounds, commits its first F rounds into the full estimate, corrects the next
# window's first detector round by the committed measurement estimate, and
# moves on. The last window is the closed space-time matrix of the rounds
# left and commits all of them.
# ---------------------------------------------------------------------------
def _window(window, commit=None):
    """(W, F) of window= / commit= (commit None: 1), checked."""
    if isinstance(window, bool) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError("window must be an integer >= 1")
    F = 1 if commit is None else commit
    if isinstance(F, bool) or not isinstance(F, (int, np.integer)) or not (1 <= F <= window):
        raise ValueError("commit must be an integer in [1, window]")
    return int(window), int(F)


def window_shape(n, m, R, closed):
    """(rows, columns) of a window of R rounds: the closed one is the
    space-time matrix's, the open one has measurement columns in every round."""
    R = _rounds(R)
    return (R * m, R * n + (R - 1) * m) if closed else (R * m, R * (n + m))


def window_matrix(H, W):
    """The open window of W rounds, int8 [W m, W (n+m)]: the first W rounds of
    spacetime_matrix(H, W + 1), so every round has its measurement columns and
    the last round's have degree 1."""
    W = _rounds(W)
    H = np.asarray(H)
    if H.ndim != 2:
        raise ValueError("H must be a 2-D matrix")
    m, n = H.shape
    return np.ascontiguousarray(spacetime_matrix(H, W + 1)[:W * m, :W * (n + m)])


def window_prior(n, m, W, p_data, q):
    """The prior float64 [W (n+m)] of window_matrix: p_data on data columns, q
    on measurement columns (spacetime_prior's layout)."""
    W = _rounds(W)
    return np.ascontiguousarray(spacetime_prior(n, m, W + 1, p_data, q)[:W * (n + m)])


def window_schedule(rounds, window, commit=1):
    """The windows of T rounds decoded W at a time, F committed per window:
    a list of (start round a, rounds R, closed, commit rounds C). Window k
    starts at a = k F; if a + W >= T it is the last one: closed (the matrix
    spacetime_matrix(H, R) of the R = T - a rounds left) and commits all of
    them; else it is open (window_matrix(H, W)) and commits C = F. T <= W is
    one closed window of T rounds."""
    T = _rounds(rounds)
    W, F = _window(window, commit)
    out, a = [], 0
    while a + W < T:
        out.append((a, W, False, F))
        a += F
    out.append((a, T - a, True, T - a))
    return out


def window_advance(n, m, rounds, det, ehat, iters_total, done=None, west=None, witers=None, nxt=None):
    """NumPy twin of qldpc_phenom_window, the step between two windows.
    `done` = (a, R, closed, C) is the window just decoded, `west` uint8
    [B, N_w] its estimate and `witers` [B] its iteration counts: the committed
    columns west[:, :C (n+m)] (closed: all R n + (R-1) m) are copied to
    ehat[:, a (n+m) + .] (uint8 [B, N], in place; every other column stays) and
    witers is added to iters_total (int32 [B], in place). `nxt` = (a', R', ..)
    is the next window: returns its syndrome uint8 [B, R' m], det[:, a' m :
    (a' + R') m] with the first m entries XORed by the committed measurement
    estimate of window round C - 1 (d_a' ^ u_{a'-1}). done None: the plain cut
    (the first window); nxt None: returns None."""
    T = _rounds(rounds)
    nm = n + m
    det = np.asarray(det)
    C = None
    if done is not None:
        a, R, closed, C = (int(v) for v in done)
        if not (0 <= a and 1 <= R and a + R <= T and 1 <= C <= R) or (a + R == T) != bool(closed) or \
                (closed and C != R):
            raise ValueError(f"window {done} does not lie in [0, {T})")
        west = np.asarray(west).astype(np.uint8) & 1
        if west.shape != (ehat.shape[0], window_shape(n, m, R, closed)[1]):
            raise ValueError("west does not match the window")
        k = west.shape[1] if closed else C * nm
        ehat[:, a * nm:a * nm + k] = west[:, :k]
        iters_total += np.asarray(witers).astype(iters_total.dtype)
    if nxt is None:
        return None
    a2, R2 = int(nxt[0]), int(nxt[1])
    if not (0 <= a2 and 1 <= R2 and a2 + R2 <= T) or (done is not None and (closed or a2 != a + C)):
        raise ValueError(f"next window {nxt} does not follow {done} in [0, {T})")
    syn = (det[:, a2 * m:(a2 + R2) * m].astype(np.uint8) & 1).copy()
    if done is not None:
        o = (C - 1) * nm + n
        syn[:, :m] ^= west[:, o:o + m]
    return syn

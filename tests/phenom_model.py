"""Independent NumPy model of the phenomenological noise mode (tests only).

Restates, from the definition alone and with dense matrices: the space-time
check matrix, the Philox4x32-10 stream of the device sampler, the sampler's
outputs and the outcome classes. Nothing here imports qldpcsim_amd.spacetime.

Layout (one CSS half, H [m, n], T rounds): N = T n + (T-1) m columns,
round-major; round t owns data columns t (n+m) + j and, for t < T-1,
measurement columns t (n+m) + n + c. Detector row t m + c holds row c of H
on round t's data columns, measurement column (t, c) if t < T-1 and
(t-1, c) if t >= 1.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: ctr [..., 4], key
    [..., 2] (broadcastable), uint32 values held in uint64. Returns [..., 4]."""
    c = [np.asarray(ctr[..., i], dtype=np.uint64) & M32 for i in range(4)]
    k0 = np.asarray(key[..., 0], dtype=np.uint64) & M32
    k1 = np.asarray(key[..., 1], dtype=np.uint64) & M32
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for _ in range(10):
        p0 = m0 * c[0]                       # < 2^64: no overflow
        p1 = m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & M32, (p0 >> s32) ^ c[3] ^ k1, p0 & M32]
        k0 = (k0 + w0) & M32
        k1 = (k1 + w1) & M32
    return np.stack(c, axis=-1)


def draws(seed, shot0, shots, N):
    """uint64 [shots, N]: u(s, J) = Philox(key = seed, ctr = (J % 64,
    (J / 64) / 4, s_lo, s_hi))[(J / 64) % 4] for s = shot0 .. shot0+shots-1."""
    seed = int(seed) & (2 ** 64 - 1)
    J = np.arange(N, dtype=np.uint64)
    s = (np.arange(shots, dtype=object) + int(shot0)) % (2 ** 64)
    s = np.array([int(x) for x in s], dtype=np.uint64)
    ctr = np.zeros((shots, N, 4), np.uint64)
    ctr[..., 0] = J % np.uint64(64)
    ctr[..., 1] = (J // np.uint64(64)) // np.uint64(4)
    ctr[..., 2] = (s & M32)[:, None]
    ctr[..., 3] = (s >> np.uint64(32))[:, None]
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64)
    out = philox4x32_10(ctr, key)
    sel = ((J // np.uint64(64)) % np.uint64(4)).astype(np.int64)
    return np.take_along_axis(out, np.broadcast_to(sel[None, :, None], (shots, N, 1)), axis=2)[..., 0]


def threshold(prob):
    return int(min(2.0 ** 32, np.floor(float(prob) * 2.0 ** 32)))


def dense_matrix(H, T):
    """The space-time matrix, entry by entry from the definition."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    m, n = H.shape
    S = np.zeros((T * m, T * n + (T - 1) * m), np.uint8)
    for t in range(T):
        for c in range(m):
            for j in np.flatnonzero(H[c]):
                S[t * m + c, t * (n + m) + j] = 1
            if t < T - 1:
                S[t * m + c, t * (n + m) + n + c] = 1
            if t >= 1:
                S[t * m + c, (t - 1) * (n + m) + n + c] = 1
    return S


def is_data(n, m, T):
    N = T * n + (T - 1) * m
    return np.array([(J % (n + m)) < n for J in range(N)], bool)


def fold(bits, n, m, T):
    out = np.zeros((bits.shape[0], n), np.uint8)
    for t in range(T):
        out ^= bits[:, t * (n + m):t * (n + m) + n].astype(np.uint8)
    return out


def mod2(A, B):
    """A·Bᵀ mod 2 over the integers."""
    return ((np.asarray(A).astype(np.int64) @ np.asarray(B).astype(np.int64).T) % 2).astype(np.uint8)


def sample(H, T, p_data, q, seed, shot0, shots):
    """(det [shots, T m], E [shots, n], fired [shots, N]) of the device stream."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    m, n = H.shape
    S = dense_matrix(H, T)
    thr = np.where(is_data(n, m, T), threshold(p_data), threshold(q)).astype(np.uint64)
    fired = (draws(seed, shot0, shots, S.shape[1]) < thr).astype(np.uint8)
    return mod2(fired, S), fold(fired, n, m, T), fired


def classify(H, L, T, det, E, ehat):
    """(class uint8 [B], flips uint8 [B, k] = L r mod 2, r uint8 [B, n]) from
    the definition: class 2 if H_st ehat != det, else 1 if L r != 0, else 0."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    L = (np.asarray(L) % 2).astype(np.uint8).reshape(-1, H.shape[1])
    m, n = H.shape
    S = dense_matrix(H, T)
    fail = np.any(mod2(ehat, S) != det, axis=1)
    r = np.asarray(E).astype(np.uint8) ^ fold(np.asarray(ehat), n, m, T)
    F = mod2(r, L) if L.shape[0] else np.zeros((r.shape[0], 0), np.uint8)
    cls = np.where(fail, 2, np.any(F != 0, axis=1).astype(np.uint8)).astype(np.uint8)
    return cls, F, r


def counters(cls, iters):
    return {"failures": int((cls == 2).sum()), "logical_errors": int((cls == 1).sum()),
            "successes": int((cls == 0).sum()), "iterations": int(np.asarray(iters, np.int64).sum())}


def pack_words(bits):
    """0/1 [B, k] -> uint64 [B, ceil(k/64)], bit i % 64 of word i / 64."""
    bits = np.asarray(bits).astype(np.uint64)
    B, k = bits.shape
    out = np.zeros((B, (k + 63) // 64), np.uint64)
    for i in range(k):
        out[:, i // 64] |= bits[:, i] << np.uint64(i % 64)
    return out


def unpack_words(words, k):
    words = np.asarray(words).astype(np.uint64)
    out = np.zeros((words.shape[0], k), np.uint8)
    for i in range(k):
        out[:, i] = (words[:, i // 64] >> np.uint64(i % 64)) & np.uint64(1)
    return out


RECIPES = ("equal", "stabiliser", "moved", "logical", "data_flip", "meas_flip")


def craft(rng, H, Hstab, Lop, T, fired):
    """Estimates built from the fired rows [B, N]; shot b takes recipe b % 6:
      0  the fired row itself                                          (class 0)
      1  plus a stabiliser row `Hstab` on one round's data columns      (class 0)
      2  a data error moved from round t to t + 1, the measurement bits
         (t, c) of its checks flipped: same detectors                  (class 0)
      3  plus a logical operator `Lop` row of the half in one round    (class 1)
      4  one data bit flipped                                          (class 2)
      5  one measurement bit flipped                                   (class 2)
    `Hstab` are the stabilisers and `Lop` logical operators of the errors'
    own type (the X half, detected by H = Hz: rows of Hx and Lx; both lie in
    ker H, and a row of H itself does only for a self-orthogonal H): the
    table L the counter tests with detects Lop and not Hstab.
    Recipes 2 and 5 need T >= 2 and fall back to 0 and 4 at T = 1. Recipes 4
    and 5 pick a column in some check (a zero column of H would not change
    the detectors). Returns (ehat, recipe index per shot as applied)."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    m, n = H.shape
    B = fired.shape[0]
    e = fired.copy().astype(np.uint8)
    rec = np.arange(B) % 6
    used = np.flatnonzero(H.any(axis=0))
    for b in range(B):
        t = int(rng.integers(0, T))
        o = t * (n + m)
        if rec[b] == 1:
            e[b, o:o + n] ^= np.asarray(Hstab[int(rng.integers(0, len(Hstab)))]).astype(np.uint8) & 1
        elif rec[b] == 2:
            if T < 2:
                rec[b] = 0
                continue
            t = int(rng.integers(0, T - 1))
            o = t * (n + m)
            j = int(rng.choice(used))
            e[b, o + j] ^= 1
            e[b, o + (n + m) + j] ^= 1
            e[b, o + n:o + n + m] ^= H[:, j]
        elif rec[b] == 3:
            e[b, o:o + n] ^= np.asarray(Lop[int(rng.integers(0, len(Lop)))]).astype(np.uint8) & 1
        elif rec[b] == 4 or (rec[b] == 5 and T < 2):
            rec[b] = 4
            e[b, o + int(rng.choice(used))] ^= 1
        elif rec[b] == 5:
            t = int(rng.integers(0, T - 1))
            e[b, t * (n + m) + n + int(rng.integers(0, m))] ^= 1
    return e, rec

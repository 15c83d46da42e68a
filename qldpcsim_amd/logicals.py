"""Logical operators of a CSS pair (Hx, Hz), on the host.

`css_logicals(Hx, Hz)` returns a canonically paired basis (Lx, Lz) of the
k = n - rank(Hx) - rank(Hz) logical qubits:

    Hz·Lxᵀ = 0, Hx·Lzᵀ = 0            the logicals commute with every stabiliser
    span(Lx) ∩ rowspace(Hx) = {0}     none of them is a stabiliser
    span(Lz) ∩ rowspace(Hz) = {0}
    Lx·Lzᵀ = I_k                      bit i of a flip word is logical qubit i

all over GF(2). With these, a residual r = err ^ estimate whose syndrome is
zero is an X stabiliser exactly when Lz·r = 0 (simulator.count_logical_outcomes,
the device counters of channel_kernels.hip).

Construction. ker(Hz) ⊇ rowspace(Hx) (the pair commutes). Reduce a basis of
ker(Hz) by the reduced row-echelon form of Hx, so every vector is zero on Hx's
pivot columns: what is left spans a complement of rowspace(Hx) in ker(Hz),
and its echelon form has k rows (Lx candidates). The same with the roles
swapped gives Lz candidates; M = Lx·Lzᵀ is then invertible and
Lz <- (M⁻¹)ᵀ·Lz pairs them. Every elimination runs on bit-packed rows
(uint64 words, one vectorised XOR per pivot column); the products are float32
matrix products (exact: sums stay below 2^24).
"""
import threading

import numpy as np

__all__ = ["css_logicals", "gf2_rank"]


def _pack(M):
    """uint8 [r, n] (0/1) -> uint64 [r, ceil(n/64)], bit j % 64 of word j / 64."""
    M = np.ascontiguousarray(M, dtype=np.uint8)
    r, n = M.shape
    W = max(1, (n + 63) // 64)
    b = np.zeros((r, 8 * W), dtype=np.uint8)
    if n:
        pk = np.packbits(M, axis=1, bitorder="little")
        b[:, :pk.shape[1]] = pk
    return b.view("<u8").astype(np.uint64, copy=False).reshape(r, W)


def _unpack(P, n):
    """Inverse of _pack."""
    b = np.ascontiguousarray(P.astype("<u8", copy=False)).view(np.uint8).reshape(P.shape[0], 8 * P.shape[1])
    return np.unpackbits(b, axis=1, bitorder="little")[:, :n]


def _rref(P, n):
    """Reduced row-echelon form of bit-packed rows over the first n columns:
    (rows [rank, W], pivot columns). One XOR of the pivot row onto every other
    row that holds the pivot column, per pivot."""
    A = P.copy()
    piv = []
    r = 0
    rows = A.shape[0]
    for j in range(n):
        if r == rows:
            break
        w, sh = j >> 6, np.uint64(j & 63)
        col = ((A[:, w] >> sh) & np.uint64(1)).astype(bool)
        cand = np.flatnonzero(col[r:])
        if cand.size == 0:
            continue
        q = r + int(cand[0])
        if q != r:
            A[[r, q]] = A[[q, r]]
            col[q] = col[r]
        col[r] = False
        A[col] ^= A[r]
        piv.append(j)
        r += 1
    return A[:r], np.asarray(piv, dtype=np.int64)


def gf2_rank(H):
    H = (np.asarray(H) % 2).astype(np.uint8)
    if H.size == 0:
        return 0
    return int(_rref(_pack(H), H.shape[1])[0].shape[0])


def _mul(A, B):
    """A·B mod 2 for 0/1 arrays (float32 product, exact below 2^24 terms)."""
    return (A.astype(np.float32) @ B.astype(np.float32)).astype(np.int64) & 1


def _kernel(R, piv, n):
    """Basis [n - rank, n] (uint8) of {v : R·v = 0} from the RREF rows R
    (unpacked) and their pivots: one vector per free column f, with v[f] = 1
    and v[piv[i]] = R[i, f]."""
    free = np.setdiff1d(np.arange(n), piv)
    K = np.zeros((free.size, n), dtype=np.uint8)
    K[np.arange(free.size), free] = 1
    if piv.size:
        K[:, piv] = R[:, free].T
    return K


def _complement(Hstab, Hother, n):
    """Echelon basis (uint8 [k, n]) of a complement of rowspace(Hstab) in
    ker(Hother)."""
    Rs, ps = _rref(_pack(Hstab), n)
    Ro, po = _rref(_pack(Hother), n)
    K = _kernel(_unpack(Ro, n), po, n)
    if ps.size and K.shape[0]:
        K = K ^ _mul(K[:, ps], _unpack(Rs, n)).astype(np.uint8)   # zero on Hstab's pivots
    L, _ = _rref(_pack(K), n)
    return _unpack(L, n)


def _gf2_inverse(M):
    k = M.shape[0]
    R, piv = _rref(_pack(np.concatenate([M.astype(np.uint8), np.eye(k, dtype=np.uint8)], axis=1)), k)
    if piv.size != k:
        raise ValueError("the logical pairing matrix is singular (Hx and Hz do not form a CSS pair)")
    return _unpack(R, 2 * k)[:, k:]


def _compute(Hx, Hz):
    n = Hx.shape[1]
    Lx = _complement(Hx, Hz, n)         # in ker(Hz), outside rowspace(Hx)
    Lz = _complement(Hz, Hx, n)         # in ker(Hx), outside rowspace(Hz)
    k = Lx.shape[0]
    if Lz.shape[0] != k:
        raise ValueError("internal: the X and Z logical spaces differ in dimension")
    if k:
        Lz = _mul(_gf2_inverse(_mul(Lx, Lz.T)).T, Lz)
    return np.ascontiguousarray(Lx, dtype=np.int8), np.ascontiguousarray(Lz, dtype=np.int8)


_cache = {}
_lock = threading.Lock()


def css_logicals(Hx, Hz):
    """(Lx, Lz), int8 [k, n] each, for the CSS pair (Hx, Hz); see the module
    docstring for the identities. Deterministic; computed once per pair (cached
    by the matrices' bytes; treat the returned arrays as read-only).

    Raises ValueError if the column counts differ or Hx·Hzᵀ != 0 mod 2.
    k = 0 returns two (0, n) arrays."""
    Hx = np.asarray(Hx)
    Hz = np.asarray(Hz)
    if Hx.ndim != 2 or Hz.ndim != 2:
        raise ValueError("Hx and Hz must be 2-D matrices")
    if Hx.shape[1] != Hz.shape[1]:
        raise ValueError("Hx and Hz must have the same number of columns (physical qubits).")
    Hx = np.ascontiguousarray(Hx % 2, dtype=np.uint8)
    Hz = np.ascontiguousarray(Hz % 2, dtype=np.uint8)
    key = (Hx.shape, Hx.tobytes(), Hz.shape, Hz.tobytes())
    with _lock:
        hit = _cache.get(key)
    if hit is not None:
        return hit
    bad = int(_mul(Hx, Hz.T).sum())
    if bad:
        raise ValueError(f"Hx·Hzᵀ != 0 mod 2 ({bad} non-commuting entries): not a CSS pair")
    out = _compute(Hx, Hz)
    for a in out:
        a.setflags(write=False)
    with _lock:
        _cache.setdefault(key, out)
        return _cache[key]

"""Independent model of the logical outcome counters (tests only).

Decides "the residual r is a stabiliser" from the definition, with no logical
basis: r ∈ rowspace(H) ⇔ N·r = 0 mod 2 for a basis N of ker(H) (the row space
is the orthogonal complement of the kernel). N comes from this file's own
GF(2) elimination; qldpcsim_amd.logicals is not imported. For a half-shot
whose estimate reproduces the measured syndrome (and sy = H'·err), the
residual lies in ker(H'), so "not a stabiliser" is "a nontrivial logical":
this pins classes and counters whatever basis the package chose. Flip words
depend on the basis and are checked against L·r with the returned L.
"""
import numpy as np


def nullspace(H):
    """uint8 [n - rank, n]: a basis of {v : H·v = 0 mod 2} (Gauss-Jordan on
    0/1 rows held as 64-bit words, one row XOR per pivot)."""
    A = (np.asarray(H) % 2).astype(np.uint8)
    m, n = A.shape
    P = np.zeros((m, 8 * ((n + 63) // 64)), np.uint8)
    P[:, :(n + 7) // 8] = np.packbits(A, axis=1, bitorder="little")
    P = P.view("<u8")                       # bit j % 64 of word j / 64
    piv = []
    r = 0
    for j in range(n):
        if r == m:
            break
        w, sh = j >> 6, np.uint64(j & 63)
        rows = np.flatnonzero((P[r:, w] >> sh) & np.uint64(1)) + r
        if rows.size == 0:
            continue
        if rows[0] != r:
            P[[r, rows[0]]] = P[[rows[0], r]]
        hit = np.flatnonzero((P[:, w] >> sh) & np.uint64(1))
        hit = hit[hit != r]
        P[hit] ^= P[r]
        piv.append(j)
        r += 1
    A = np.unpackbits(P.view(np.uint8), axis=1, bitorder="little")[:, :n]
    pivset = set(piv)
    free = [j for j in range(n) if j not in pivset]
    N = np.zeros((len(free), n), dtype=np.uint8)
    for i, f in enumerate(free):            # v[f] = 1, v[pivot q] = A[q, f]
        N[i, f] = 1
        N[i, piv] = A[:r, f]
    assert not _mod2(A[:r], N).any()        # (float32 products of 0/1 rows: exact below 2^24 columns)
    return N


def _mod2(A, B):
    return (np.asarray(A).astype(np.float32) @ np.asarray(B).astype(np.float32).T).astype(np.int64) % 2


class Model:
    """Classes and the nine counters of one CSS pair."""

    def __init__(self, Hx, Hz):
        self.Hx = (np.asarray(Hx) % 2).astype(np.uint8)
        self.Hz = (np.asarray(Hz) % 2).astype(np.uint8)
        self.Nx = nullspace(self.Hx)        # rX ∈ rowspace(Hx) ⇔ Nx·rX = 0
        self.Nz = nullspace(self.Hz)

    def classes(self, sy_z, sy_x, errX, errZ, eX, eZ):
        failX = np.any(_mod2(eX, self.Hz) != sy_z, axis=1)
        failZ = np.any(_mod2(eZ, self.Hx) != sy_x, axis=1)
        stabX = ~np.any(_mod2(errX ^ eX, self.Nx), axis=1)
        stabZ = ~np.any(_mod2(errZ ^ eZ, self.Nz), axis=1)
        cX = np.where(failX, 2, np.where(stabX, 0, 1)).astype(np.uint8)
        cZ = np.where(failZ, 2, np.where(stabZ, 0, 1)).astype(np.uint8)
        return cX, cZ

    def counters(self, sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ):
        cX, cZ = self.classes(sy_z, sy_x, errX, errZ, eX, eZ)
        exact = np.all(errX == eX, axis=1) & np.all(errZ == eZ, axis=1)
        # the reference's integer test (no mod 2)
        iX = (errX ^ eX).astype(np.int64) @ self.Hz.T.astype(np.int64)
        iZ = (errZ ^ eZ).astype(np.int64) @ self.Hx.T.astype(np.int64)
        degen = ~exact & np.all(iX == 0, axis=1) & np.all(iZ == 0, axis=1)
        return {
            "DecFailures_X": int((cX == 2).sum()),
            "DecFailures_Z": int((cZ == 2).sum()),
            "decSuccessExact": int(exact.sum()),
            "decSuccessDegen": int(degen.sum()),
            "nIterAccX": int(np.asarray(itX, dtype=np.int64).sum()),
            "nIterAccZ": int(np.asarray(itZ, dtype=np.int64).sum()),
            "logicalErrors_X": int((cX == 1).sum()),
            "logicalErrors_Z": int((cZ == 1).sum()),
            "decSuccessLogical": int(((cX == 0) & (cZ == 0)).sum()),
        }


def flip_words(L, r):
    """uint64 [B, ceil(k/64)]: L·r mod 2, bit i % 64 of word i / 64."""
    L = np.asarray(L)
    B, k = r.shape[0], L.shape[0]
    kw = (k + 63) // 64
    out = np.zeros((B, kw), dtype=np.uint64)
    if k:
        F = _mod2(r, L)
        for i in range(k):
            out[:, i // 64] |= F[:, i].astype(np.uint64) << np.uint64(i % 64)
    return out


def check_invariants(c, shots):
    assert c["logicalErrors_X"] + c["DecFailures_X"] <= shots
    assert c["logicalErrors_Z"] + c["DecFailures_Z"] <= shots
    assert c["decSuccessLogical"] >= c["decSuccessExact"]
    assert c["decSuccessLogical"] + c["logicalErrors_X"] + c["logicalErrors_Z"] + c["DecFailures_X"] + \
        c["DecFailures_Z"] >= shots


def _combos(rng, rows, B, nonzero):
    """B random GF(2) combinations of `rows` ([r, n]); nonzero: at least one row each."""
    r = rows.shape[0]
    sel = rng.integers(0, 2, (B, r), dtype=np.uint8)
    if nonzero and r:
        sel[np.arange(B), rng.integers(0, r, B)] = 1
    return _mod2(sel, rows.T).astype(np.uint8)


RECIPES = ("exact", "stabiliser", "logical", "sparse")


def craft_half(rng, err, Hstab, Lsame, recipe):
    """Estimates of `err` ([B, n]) by recipe index per shot:
      0  err itself                                              (exact)
      1  err ^ nonzero combination of the stabiliser rows Hstab  (class 0, not exact)
      2  err ^ nonzero combination of the logical rows ^ stabiliser (class 1)
      3  err ^ one or two random bit flips                       (mostly class 2)
    Hstab: the half's own stabilisers (Hx for the X half); Lsame: its logical
    operators of the same type (Lx), which the other type's rows (Lz) detect."""
    B, n = err.shape
    e = err.copy()
    stab = _combos(rng, np.asarray(Hstab, dtype=np.uint8), B, True)
    logi = _combos(rng, np.asarray(Lsame, dtype=np.uint8), B, True)
    anyst = _combos(rng, np.asarray(Hstab, dtype=np.uint8), B, False)
    sparse = np.zeros((B, n), dtype=np.uint8)
    sparse[np.arange(B), rng.integers(0, n, B)] = 1
    second = rng.integers(0, 2, B).astype(bool)
    sparse[np.flatnonzero(second), rng.integers(0, n, int(second.sum()))] ^= 1
    e[recipe == 1] ^= stab[recipe == 1]
    e[recipe == 2] ^= logi[recipe == 2] ^ anyst[recipe == 2]
    e[recipe == 3] ^= sparse[recipe == 3]
    return e


def craft(rng, Hx, Hz, Lx, Lz, errX, errZ):
    """(eX, eZ, recipeX, recipeZ): every pair of recipes occurs (shot b takes
    recipe b % 4 in the X half and (b // 4) % 4 in the Z half)."""
    B = errX.shape[0]
    rX = np.arange(B) % 4
    rZ = (np.arange(B) // 4) % 4
    eX = craft_half(rng, errX, Hx, Lx, rX)
    eZ = craft_half(rng, errZ, Hz, Lz, rZ)
    for rec in (rX, rZ):
        share = np.bincount(rec, minlength=4) / B
        assert (share >= 0.1).all(), share      # by construction a quarter each
    return eX, eZ, rX, rZ

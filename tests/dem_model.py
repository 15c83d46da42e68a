"""Independent NumPy model of the detector error model mode (tests only).

Restates from the definition alone, with dense matrices: the sampler's
Philox stream and thresholds, its outputs, the outcome classes, and the
word-edge test models. Nothing here imports qldpcsim_amd.dem; the Philox
generator and the word packing are tests/phenom_model.py's.

A model is (H [M, N], L [K, N], priors [N]): column J fires iff
u(s, J) < floor(p_J 2^32); det = H f, obs = L f; an estimate ehat is class 2
if H ehat != det, else 1 if L ehat != obs, else 0.
"""
import numpy as np

from phenom_model import draws, mod2, pack_words, threshold, unpack_words  # noqa: F401


def thresholds(priors):
    return np.array([threshold(p) for p in priors], np.uint64)


def sample(H, L, priors, seed, shot0, shots):
    """(det [shots, M], obs [shots, K], fired [shots, N]) of the device stream."""
    N = len(priors)
    u = draws(seed, shot0, shots, N) if N else np.zeros((shots, 0), np.uint64)
    fired = (u < thresholds(priors)).astype(np.uint8)
    return _prod(fired, H), _prod(fired, L), fired


def _prod(x, A):
    A = np.asarray(A).astype(np.uint8)
    return mod2(x, A) if A.shape[0] else np.zeros((x.shape[0], 0), np.uint8)


def classify(H, L, det, obs, ehat):
    """(class uint8 [B], flips uint8 [B, K] = L ehat ^ obs), shot by shot."""
    B = len(ehat)
    H, L = np.asarray(H).astype(np.int64), np.asarray(L).astype(np.int64)
    cls = np.zeros(B, np.uint8)
    F = np.zeros((B, L.shape[0]), np.uint8)
    for b in range(B):
        s = (H @ ehat[b].astype(np.int64)) % 2
        o = (L @ ehat[b].astype(np.int64)) % 2
        F[b] = o ^ obs[b]
        cls[b] = 2 if np.any(s != det[b]) else (1 if F[b].any() else 0)
    return cls, F


def counters(cls, iters):
    return {"failures": int((cls == 2).sum()), "logical_errors": int((cls == 1).sum()),
            "successes": int((cls == 0).sum()), "iterations": int(np.asarray(iters, np.int64).sum())}


# (M, K, N) of the word-edge models: one word, a word's last bit, one past it,
# two words and a second observable word, more than 4096 columns
EDGE_SHAPES = ((1, 0, 1), (63, 1, 64), (64, 64, 65), (65, 65, 129), (130, 3, 4097))


def edge_dem(M, K, N, seed=0):
    """A fixed-seed random sparse model of that shape, (H, L, priors, where).
    From 64 columns up it holds, at the places `where` names: an all-zero
    column, an observable-only column (K > 0), a p = 0 column, a p = 1 - 2^-20
    column, an empty last detector row (M >= 3), a detector row and an
    observable row of degree min(300, N - 8), a pair of identical columns and
    (K > 0) a column that copies another one's detectors and differs in one
    observable; the other priors are log-uniform in [1e-6, 0.4]. Below 64
    columns it is the random matrix alone, every prior 0.4."""
    rng = np.random.default_rng([seed, M, K, N])
    H, L = np.zeros((M, N), np.uint8), np.zeros((K, N), np.uint8)
    for j in range(N):                                   # two or three detectors per column
        H[rng.choice(M, size=min(M, int(rng.integers(2, 4))), replace=False), j] = 1
    if K:
        L[rng.integers(0, K, N // 3), rng.choice(N, N // 3, replace=False)] = 1
    pr = np.exp(rng.uniform(np.log(1e-6), np.log(0.4), N))
    where = {}
    if N < 64:
        pr[:] = 0.4                                      # too few columns for the special ones: let them fire
        return H, L, pr, where
    cols = [int(c) for c in rng.choice(N, 8, replace=False)]
    zero, only, p0, p1, twin_a, twin_b, base, logi = cols
    free = np.setdiff1d(np.arange(N), cols)
    deg = min(300, free.size)
    # rows first (they clear whole rows), then the special columns
    if M >= 3:
        H[M - 1] = 0                                     # the last row is empty: M comes from a declaration
        H[0] = 0
        H[0, rng.choice(free, deg, replace=False)] = 1
        where.update(empty_row=M - 1, heavy_row=(0, deg))
    if K:
        L[K - 1] = 0
        L[K - 1, rng.choice(free, deg, replace=False)] = 1
        where["heavy_obs"] = (K - 1, deg)
    H[:, zero], H[:, only] = 0, 0
    pr[zero], pr[only], pr[p0], pr[p1] = 0.3, 0.3, 0.0, 1.0 - 2.0 ** -20
    where.update(zero=zero, p0=p0, p1=p1, twin=(twin_a, twin_b))
    H[:, twin_b] = H[:, twin_a]                          # twin_a ^ twin_b flips nothing: class 0 with both
    if K:
        L[:, zero], L[:, only] = 0, 0
        L[int(rng.integers(0, K)), only] = 1
        L[:, twin_b] = L[:, twin_a]
        # logi has base's detectors and one observable more or less: base ^ logi is a pure logical flip (class 1)
        H[:, logi], L[:, logi] = H[:, base], L[:, base]
        L[0, logi] ^= 1
        where.update(obs_only=only, base=base, logi=logi)
    return H, L, pr, where


def craft(rng, H, L, fired, where):
    """Estimates built from the fired rows [B, N]; shot b takes recipe b % 3:
      0  the fired row itself, plus the twin pair where the model has one (class 0)
      1  plus the (base, logi) pair: the same detectors, one observable
         flipped (class 1); without such a pair, plus an observable-only
         column if there is one, else recipe 0
      2  one column that some detector sees flipped (class 2)
    Returns (ehat, the class each shot must have)."""
    e = fired.copy().astype(np.uint8)
    B = e.shape[0]
    want = np.zeros(B, np.uint8)
    seen = np.flatnonzero(np.asarray(H).any(axis=0))
    for b in range(B):
        r = b % 3
        if r == 0 and "twin" in where:
            e[b, list(where["twin"])] ^= 1
        elif r == 1 and "logi" in where:
            e[b, [where["base"], where["logi"]]] ^= 1
            want[b] = 1
        elif r == 1 and "obs_only" in where:
            e[b, where["obs_only"]] ^= 1
            want[b] = 1
        elif r == 2 and seen.size:
            e[b, int(rng.choice(seen))] ^= 1
            want[b] = 2
    return e, want

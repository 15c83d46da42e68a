"""Comb-shaped parity-check matrices whose BP column sums reach every order
np.sum uses, and the HBM-resident kernels past 128 entries per column
(DESIGN.md sections 3.17 and 8).

np.sum of a 1-D float64 array (DOUBLE_pairwise_sum) adds in sequence from -0.0
below 8 terms; runs eight accumulators, a fixed tree over them and a sequential
remainder from 8 to 128 terms; and above 128 terms halves the range (the left
half a multiple of 8) and recurses. BP's posteriors equal the reference's bit
for bit only where every variable node follows the order of its own degree.
The bundled codes have columns of at most 5 entries and tests/shape_codes.py
stops at 36, so the shapes here carry a few heavy columns of prescribed degree
(the comb's teeth) over many light ones of degree 2 to 3, at least three in
every row (no decode is trivial). Row degrees stay at 32 or below, so that min-sum runs
on the LDS kernels as a control; W4 alone has one row past 64 entries.

As in tests/shape_codes.py everything is data: the matrices are deterministic
in their seed, write-protected and cached; tests/test_wide_column_codes.py
asserts on the references alone what the GPU tests rely on.
"""
import functools

import numpy as np

import shape_codes as sc
import tall_shape_codes as ts

LDS_COLUMN_MAX = 128  # the last BP column degree the LDS kernels take (capi_decode.cpp), np.sum's last unsplit length
MIN_LIGHT = 3         # fewest light entries of a row of a comb


def comb_code(m, heavy, n_light, seed, wide_row=0):
    """uint8 [m, len(heavy) + n_light]: one column of each degree in `heavy`
    over a random set of rows; light column k holds row k % m and one or two
    other random rows (n_light >= m: every row has a light entry); with
    `wide_row`, row 0 takes that many further entries in light columns that
    miss it; a row left with fewer than MIN_LIGHT light entries takes more in
    light columns of two entries. Columns are then shuffled."""
    assert n_light >= m and max(heavy) <= m
    rng = np.random.default_rng(seed)
    h = len(heavy)
    H = np.zeros((m, h + n_light), np.uint8)
    for j, d in enumerate(heavy):
        H[rng.choice(m, d, replace=False), j] = 1
    for k in range(n_light):
        r0 = k % m
        others = rng.choice(m - 1, 1 + int(rng.integers(0, 2)), replace=False)
        H[r0, h + k] = 1
        H[others + (others >= r0), h + k] = 1
    if wide_row:
        free = h + np.flatnonzero(H[0, h:] == 0)
        H[0, rng.choice(free, wide_row, replace=False)] = 1
    # Under a scalar prior a check whose other variables are all saturated (a heavy column soon is) but one
    # fresh one answers -L exactly: the posterior becomes 0 and the next tanh quotient 0 / 0. Three light
    # entries per row keep the references finite (a NaN's payload is not the reference's to pin). For the
    # same reason m lies well above the heaviest degree: two heavy columns over nearly the same rows drive
    # each other's posterior to 0.
    for r in np.flatnonzero(H[:, h:].sum(1) < MIN_LIGHT):
        two = h + np.flatnonzero((H[:, h:].sum(0) == 2) & (H[r, h:] == 0))
        H[r, rng.choice(two, MIN_LIGHT - int(H[r, h:].sum()), replace=False)] = 1
    return np.ascontiguousarray(H[:, rng.permutation(H.shape[1])])


# id -> how the matrix is made, the channel flip probability p (also the
# decoder's scalar prior) of its batch, and what the shape is for. p and the
# seeds were chosen so that tests/test_wide_column_codes.py's conditions on the
# references hold (finite posteriors, converged and full-length decodes, an
# estimate that sets a heavy variable).
SHAPES = {
    "W0": dict(kind="comb", m=192, heavy=(7, 8, 9, 15, 16, 17, 64, 127, 128), n_light=400, seed=3001, p=0.01,
               what="every form of the <= 128 rule: sequential, exactly one block, blocks plus a remainder of 1 "
                    "and of 7, the largest block; stays on the LDS kernels (decode_kernel<1, ...>, "
                    "decode_vprior_kernel)"),
    "W1": dict(kind="comb", m=200, heavy=(129, 128, 64), n_light=420, seed=3002, p=0.01,
               what="the routing boundary: scalar BP on hbm_tile_kernel<1, ...>, the LDS twins refuse; 129 = 64 + 65"),
    "W2": dict(kind="comb", m=520, heavy=(136, 255, 256, 257, 272, 513), n_light=1100, seed=3003, p=0.006,
               what="64 + 72; the unbalanced 120 + (64 + 71); 128 + 128; 128 + (64 + 65); two levels on both "
                    "sides; three levels"),
    "W3": dict(kind="comb", m=1536, heavy=(1025, 1024), n_light=3100, seed=3004, p=0.003,
               what="four levels: hbm_column_depth = 4, the largest dynamic LDS of the suite; min-sum column "
                    "degrees past the chunk_dmax clamp of 255 (capi_schedule.cpp)"),
    "W4": dict(kind="comb", m=300, heavy=(136, 255, 256, 257), n_light=640, seed=3005, p=0.008, wide_row=70,
               what="one row of more than 64 entries: the DCMAX = 64 instance and cn_wide beside wide columns"),
    "U8": dict(kind="degrees", m=192, dc=8, seed=3006, p=0.01,
               degrees=[(64, 1), (127, 1), (128, 1), (2, 101), (3, 205), (4, 100)],
               what="uniform row degree 8: the bp_team kernels (all-LDS: column degree > 31) and "
                    "decode_kernel<1, *, 8> under bp_wave=1 at the <= 128 rule's far end"),
}
IDS = tuple(SHAPES)
WIDE = tuple(s for s in IDS if max(SHAPES[s].get("heavy", (0,))) > LDS_COLUMN_MAX)     # a column past 128: W1 - W4
HEAVY_MIN = 7                                            # light columns have at most 4 entries


@functools.lru_cache(maxsize=None)
def matrix(sid):
    s = SHAPES[sid]
    if s["kind"] == "comb":
        H = comb_code(s["m"], s["heavy"], s["n_light"], s["seed"], s.get("wide_row", 0))
    else:
        H = sc.code_from_degrees(s["m"], s["dc"], s["degrees"], s["seed"])
    H.setflags(write=False)
    return H


def heavy_degrees(sid):
    s = SHAPES[sid]
    return tuple(sorted(s["heavy"] if s["kind"] == "comb" else [d for d, _ in s["degrees"] if d >= HEAVY_MIN]))


def heavy_columns(sid):
    """Indices of the heavy columns, ascending."""
    return np.flatnonzero(matrix(sid).sum(0) >= HEAVY_MIN)


# ---------------------------------------------------------------------------
# np.sum's splits and the HBM kernels' stack depth, restated
# ---------------------------------------------------------------------------
def splits(d):
    """The tree np.sum adds a column of d entries in: d itself up to 128 (one
    leaf), else (splits(left), splits(right)), left = d // 2 rounded down to a
    multiple of 8."""
    if d <= LDS_COLUMN_MAX:
        return d
    n2 = d // 2
    n2 -= n2 % 8
    return (splits(n2), splits(d - n2))


def column_depth(d):
    """hbm_kernels.h hbm_column_depth restated: levels below the root."""
    t = splits(d)

    def depth(t):
        return 0 if isinstance(t, int) else 1 + max(depth(t[0]), depth(t[1]))
    return depth(t)


def hbm_lds_bytes(H):
    """hbm_vprior_lds(deepest column): one float64 per level and lane, 256 lanes."""
    return max(column_depth(int(d)) for d in np.asarray(H).sum(0)) * 256 * 8


# ---------------------------------------------------------------------------
# schedules and batches
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layerized(sid):
    from qldpcsim_amd import schedule
    return schedule.layerize(matrix(sid))


STRIDE = 5


def layers(sid, sched):
    """"F": None (flooding); "L": schedule.layerize (a heavy column that holds
    every row leaves one row per layer); "S5": rows r = k mod 5 in layer k, so
    that in the first iteration the entries of a heavy column not yet reached
    lie between those that are."""
    m = matrix(sid).shape[0]
    return {"F": lambda: None, "L": lambda: layerized(sid),
            "S5": lambda: [np.arange(k, m, STRIDE) for k in range(STRIDE)]}[sched]()


def packed(sid, sched):
    """(layer_ptr, layer_rows) of layers(sid, sched)."""
    return sc.packed(layers(sid, sched), matrix(sid).shape[0])


GPU_SHOTS, GPU_RANDOM, GPU_MAX_ITER = 72, 12, 6
HEAVY_EVERY = 6       # every sixth channel shot also flips one heavy variable (each in turn)


@functools.lru_cache(maxsize=None)
def batch(sid):
    """The shape's fixed batch: 72 channel shots at the shape's p, every sixth
    with one more flip on a heavy column (a few heavy columns among hundreds
    are otherwise flipped in a shot or two), and 12 uniform-random syndromes,
    shuffled: 84 half-shots, more than one 64-slot tile."""
    H = matrix(sid)
    rng = np.random.default_rng(SHAPES[sid]["seed"] + 50000)
    e = (rng.random((GPU_SHOTS, H.shape[1])) < SHAPES[sid]["p"]).astype(np.int64)
    hv = heavy_columns(sid)
    for i, b in enumerate(range(0, GPU_SHOTS, HEAVY_EVERY)):
        e[b, hv[i % len(hv)]] ^= 1
    syn = np.concatenate([((e @ H.T.astype(np.int64)) % 2).astype(np.uint8),
                          rng.integers(0, 2, (GPU_RANDOM, H.shape[0]), dtype=np.uint8)])
    syn = np.ascontiguousarray(syn[rng.permutation(len(syn))])
    syn.setflags(write=False)
    return syn


@functools.lru_cache(maxsize=None)
def prior_row(sid):
    """tall_shape_codes.general_prior (log-uniform in [1e-4, 0.3], three
    entries above 0.5, none at 0.5) with 0.6 on the heaviest column."""
    H = matrix(sid)
    q = ts.general_prior(H.shape[1], SHAPES[sid]["seed"] + 7)
    q[int(np.argmax(H.sum(0)))] = 0.6
    q.setflags(write=False)
    return q

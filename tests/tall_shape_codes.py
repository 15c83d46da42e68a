"""Tall, sparse parity-check matrices past the generic LDS kernel's 2048-check
syndrome register, and uniform-degree-8 codes on either side of the fast
table's 16-bit limit.

The flooding branch of decode_kernel / decode_prior_kernel /
decode_vprior_kernel keeps a lane's syndrome bits in one 32-bit register: 32
passes of 64 lanes, 2048 checks. T0 is the last size that register holds; T1,
T2 and T3 lie one check, one pass and more than 64 passes beyond it. They are
shaped like a detector error model or a repetition-like space-time matrix: a
chain with a few extra entries, row weight 2 or 3, so that tables and a wave's
state fit the LDS easily. U0 and U1 are the largest row-degree-8 code with the
pre-scaled row table (8 * E < 65536, capi_internal.h fast_table_ok) and the
smallest without it.

As in tests/shape_codes.py everything is data: the matrices are deterministic
in their seed, write-protected and cached; tests/test_tall_shape_codes.py
asserts on the oracle alone what the GPU tests rely on.
"""
import functools
import os

import numpy as np

import shape_codes as sc

REG_CHECKS = 2048     # QLDPC_SYNREG_CHECKS (decoder_kernels.h): 32 register bits x 64 lanes


def chain_code(m, extra, seed):
    """uint8 [m, m + extra]: row r touches columns r and r + 1; a random third
    of the rows get a third entry in a random other column (never column 0,
    the chain's end, which keeps degree 1); rows and columns are then
    shuffled, with the chain's first row placed last: the check of highest
    index is the one a single flip (of column 0) fires alone."""
    rng = np.random.default_rng(seed)
    n = m + extra
    H = np.zeros((m, n), np.uint8)
    r = np.arange(m)
    H[r, r] = 1
    H[r, r + 1] = 1
    for row in np.flatnonzero(rng.random(m) < 1.0 / 3.0):
        c = int(rng.integers(1, n - 2))
        H[row, c + 2 * (c >= row)] = 1                   # any column but 0, row, row + 1
    rows = rng.permutation(m)
    H = H[np.concatenate([rows[rows != 0], [0]])][:, rng.permutation(n)]
    return np.ascontiguousarray(H)


def repetition_chain(m):
    """uint8 [m, m + 1]: row r touches columns r and r + 1, in that order."""
    H = np.zeros((m, m + 1), np.uint8)
    r = np.arange(m)
    H[r, r] = 1
    H[r, r + 1] = 1
    return H


# id -> how the matrix is made, the channel flip probability p (also the
# decoder's prior) of its batch, and what the shape is for
SHAPES = {
    "T0": dict(kind="chain", m=2048, extra=40, seed=2001, p=0.01,
               what="the last size the syndrome register holds: 32 full passes"),
    "T1": dict(kind="chain", m=2049, extra=40, seed=2002, p=0.01,
               what="one check in a 33rd pass (lane 0 only)"),
    "T2": dict(kind="chain", m=2113, extra=40, seed=2003, p=0.01,
               what="a full 33rd pass and one check of a 34th; m % 64 = 1, n % 64 != 0, a zero column, "
                    "column degrees up to about 6"),
    "T3": dict(kind="repetition", m=4100, p=0.01,
               what="more than 64 passes: a 64-bit register does not hold them either"),
    "U0": dict(kind="degrees", m=1023, dc=8, seed=2011, p=0.02, degrees=[(3, 500), (4, 1046), (5, 500)],
               what="largest row-degree-8 code with the fast table: the DC = 8 instances, relay_ms_kernel<8>"),
    "U1": dict(kind="degrees", m=1024, dc=8, seed=2012, p=0.02, degrees=[(3, 500), (4, 1048), (5, 500)],
               what="uniform degree 8 with 8 * E = 65536: the DC = 0 instances, relay_ms_kernel<0>"),
}
IDS = tuple(SHAPES)
TALL = ("T1", "T2", "T3")                                # past the register


@functools.lru_cache(maxsize=None)
def matrix(sid):
    s = SHAPES[sid]
    if s["kind"] == "chain":
        H = chain_code(s["m"], s["extra"], s["seed"])
    elif s["kind"] == "repetition":
        H = repetition_chain(s["m"])
    else:
        H = sc.code_from_degrees(s["m"], s["dc"], s["degrees"], s["seed"])
    H.setflags(write=False)
    return H


def fast_table_ok(H):
    """capi_internal.h fast_table_ok restated: uniform row degree 7 or 8 whose
    pre-scaled LDS byte offsets fit 16 bits."""
    H = np.asarray(H)
    deg = H.sum(1)
    E = int(deg.sum())
    return bool(deg.min() == deg.max() and deg[0] in (7, 8) and 8 * H.shape[1] < 65536 and 8 * E < 65536)


def dc_of(sid):
    """The DC template argument of the generic kernels on shape `sid`."""
    H = matrix(sid)
    return int(H[0].sum()) if fast_table_ok(H) else 0


@functools.lru_cache(maxsize=None)
def layerized(sid):
    from qldpcsim_amd import schedule
    return schedule.layerize(matrix(sid))


def packed(sid, layered):
    """(layer_ptr, layer_rows) of flooding or of schedule.layerize."""
    return sc.packed(layerized(sid) if layered else None, matrix(sid).shape[0])


GPU_SHOTS, GPU_RANDOM, GPU_MAX_ITER = 96, 16, 25


def high_pair(sid):
    """Two hand-made syndromes of a shape past the register: one whose only
    fired checks have index >= 2048 (every such check, so the 33rd pass and
    all beyond it are read), and its image folded to index - 2048, which is
    what a register of 32 bits read back for it."""
    m = matrix(sid).shape[0]
    assert m > REG_CHECKS
    hi = np.zeros(m, np.uint8)
    hi[REG_CHECKS:] = 1
    lo = np.zeros(m, np.uint8)
    lo[np.arange(m - REG_CHECKS) % REG_CHECKS] = 1
    return np.stack([hi, lo])


@functools.lru_cache(maxsize=None)
def batch(sid):
    """The shape's fixed batch: 96 channel shots at the shape's p and 16
    uniform-random syndromes, shuffled; for T1 - T3 the two shots of
    high_pair(sid) behind them (the last two rows). Where fewer than 64 checks
    lie past the register (T1: one), channel flips alone would fire them in a
    few shots of a hundred: every third shot also flips the last check's bit
    (in T1 the syndrome of one more flip, of the chain's end column)."""
    H = matrix(sid)
    seed = SHAPES[sid].get("seed", 2004)
    rng = np.random.default_rng(seed + 50000)
    syn = np.concatenate([sc.channel_syndromes(H, SHAPES[sid]["p"], GPU_SHOTS, rng),
                          rng.integers(0, 2, (GPU_RANDOM, H.shape[0]), dtype=np.uint8)])
    syn = syn[rng.permutation(len(syn))]
    if sid in TALL and H.shape[0] - REG_CHECKS < 64:
        syn[::3, -1] ^= 1
    if sid in TALL:
        syn = np.concatenate([syn, high_pair(sid)])
    syn = np.ascontiguousarray(syn)
    syn.setflags(write=False)
    return syn


MODEL_SHOTS = 32     # the leading shots where a NumPy model is the reference


def model_batch(sid):
    """The leading MODEL_SHOTS shots of the batch and, for T1 - T3, its two
    hand-made shots."""
    syn = batch(sid)
    return np.ascontiguousarray(np.concatenate([syn[:MODEL_SHOTS - 2], syn[-2:]]) if sid in TALL else syn[:MODEL_SHOTS])


def general_prior(n, seed):
    """log-uniform in [1e-4, 0.3] with three entries above 0.5 (negative
    LLRs); no entry is 0.5, so no LLR is exactly 0."""
    q = 10.0 ** np.random.default_rng(seed).uniform(-4, np.log10(0.3), n)
    q[0], q[n // 2], q[n - 1] = 0.7, 0.6, 0.9
    return q


# ---------------------------------------------------------------------------
# the reference's recorded outputs (tests/golden/gen_golden_tall.py)
# ---------------------------------------------------------------------------
GOLDEN_IDS = ("T2", "U1")
GOLDEN_ALGOS = (("MS", "F"), ("BP", "F"), ("MS", "L"))   # L: schedule.layerize


def golden_path(sid):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tall", f"tall_{sid}.npz")


@functools.lru_cache(maxsize=None)
def golden(sid):
    """(stored matrix uint8 [m, n], [(case dict, arrays dict), ...]) of
    tests/golden/tall/tall_<sid>.npz; the matrix is stored as its sorted
    (row, column) pairs."""
    import json
    with np.load(golden_path(sid), allow_pickle=False) as z:
        m, n = (int(x) for x in z["H_shape"])
        H = np.zeros((m, n), np.uint8)
        rc = z["H_pairs"]
        H[rc[:, 0], rc[:, 1]] = 1
        cases = json.loads(bytes(z["cases_json"]).decode())
        return H, [(c, {k.split("_", 1)[1]: z[k] for k in z.files if k.startswith(f"c{i}_")})
                   for i, c in enumerate(cases)]

"""Matrices and shots at the OSD kernels' selection boundaries.

The device OSD picks one of four column kernels (osd_kernel<4 | 9 | 17 | 33>),
six block kernels (osd_block_kernel<NW, SL, RT>, each with an OSD-CS twin) or
the HBM kernel from (m, n) alone. The bundled codes reach
three block instances and never osd_kernel<33>; the fourteen cases of CASES sit
on the edges in m (64 / 65 waves, 256 / 257 rows per thread, 512 / 513 and
1024 / 1025 hand-overs) and in n (the syndrome bit at bit 63 of the last row
word, or at bit 0 of a word the block loop never visits).

Everything is data: `gen` is deterministic in a seed derived from the case
name, the matrices are also stored bit-packed in tests/golden/osd_shapes/ and
tests/test_osd_shapes_host.py asserts the two agree. `shots` builds syndromes,
posteriors, incoming estimates and explicit permutations (np.argsort of
|post|, stable: nothing depends on the pinned NumPy order); where a matrix has
64 pairs of equal columns, shot 0 and the last shot carry a crafted
permutation that makes row word 1 a word without a pivot.
"""
import functools
import json
import os
import zlib

import numpy as np

import osd_ref_model

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "osd_shapes")
LAMBDAS = (0, 10, 64)
BLK, COL = "osd_block_kernel<%d, %d, %d>", "osd_kernel<%d>"

# id -> shape, recipe (r base rows, dup copied columns; or the space-time source),
# shots, the kernel of the reference method (None for OSD-CS: refused), rank(H)
# as the committed generator gives it, and what the case is for
CASES = {
    "b4w1": dict(m=64, n=255, r=60, dup=70, k=32, kernel=BLK % (4, 4, 1), rank=60,
                 what="one full wave; syndrome bit 63 of word 3; rank < 64"),
    "b9w3": dict(m=130, n=256, r=120, dup=70, k=32, kernel=BLK % (9, 4, 1), rank=120,
                 what="3 waves at RT = 1; first n of NW = 9; n a multiple of 64"),
    # (salt: a second draw of the shots; the first held no single-flip OSD-CS winner at lambda = 64)
    "b4r2": dict(m=300, n=250, r=180, dup=0, k=32, kernel=BLK % (4, 8, 2), rank=180, salt="-b",
                 what="tall (m > n); 3 waves at RT = 2; most words 64 pivots"),
    "b9r2": dict(m=257, n=575, r=230, dup=70, k=32, kernel=BLK % (9, 8, 2), rank=230,
                 what="smallest RT = 2; last n of NW = 9"),
    "b17r1": dict(m=256, n=576, r=256, dup=0, k=32, kernel=BLK % (17, 4, 1), rank=256,
                  what="last m of RT = 1; first n of NW = 17; full row rank"),
    "b17max": dict(m=512, n=1087, r=512, dup=0, k=32, kernel=BLK % (17, 8, 2), rank=512,
                   what="both block limits; syndrome bit 63 of word 16; full row rank"),
    "st3": dict(m=252, n=693, spacetime=3, k=32, kernel=BLK % (17, 4, 1), rank=246,
                what="spacetime_matrix(Hx of LP04_0, 3): a real workload shape"),
    "win3": dict(m=252, n=777, window=3, k=32, kernel=BLK % (17, 4, 1), rank=252,
                 what="window_matrix(Hx of LP04_0, 3): open window; full row rank"),
    "c17w9": dict(m=513, n=600, r=480, dup=0, k=32, kernel=COL % 17, rank=480,
                  what="first m past the block kernel; 9 waves"),
    "c33min": dict(m=100, n=1088, r=90, dup=0, k=32, kernel=COL % 33, rank=90,
                   what="first n of NW = 33; 2 waves"),
    "st5": dict(m=420, n=1211, spacetime=5, k=32, kernel=COL % 33, rank=414,
                what="spacetime_matrix(Hx of LP04_0, 5): a real workload shape"),
    "c33max": dict(m=1024, n=2111, r=1000, dup=0, k=8, kernel=COL % 33, rank=1000,
                   what="16 waves; every limit of the column kernel"),
    "h_m": dict(m=1025, n=1100, r=1000, dup=0, k=8, kernel="osd_hbm_kernel", rank=1000,
                what="first m on HBM"),
    "h_n": dict(m=200, n=2112, r=190, dup=0, k=8, kernel="osd_hbm_kernel", rank=190,
                what="first n on HBM (34 row words)"),
}
IDS = list(CASES)
BLOCK_IDS = [c for c in IDS if CASES[c]["kernel"].startswith("osd_block")]      # OSD-CS runs these alone
OTHER_IDS = [c for c in IDS if c not in BLOCK_IDS]
HBM_FORCED_IDS = ["b4w1", "b9r2", "st3", "c33min"]                              # also run with option osd_hbm
GOLDEN_EDGE = {"c33max": 2, "h_m": 2}                                           # golden shots at each end (else 4)


def cs_kernel(name):
    k = CASES[name]["kernel"]
    return k.replace("osd_block_kernel", "osd_block_cs_kernel") if name in BLOCK_IDS else None


def gen(name, m, n, r, dup):
    """uint8 [m, n] of rank <= r: r rows of weight 6 over n - dup columns (an
    all-zero column gets a single 1), dup copies of distinct columns appended,
    m - r rows that are each the XOR of three base rows, rows shuffled."""
    rng = np.random.default_rng(zlib.crc32(f"osd-shape-{name}".encode()))
    nb = n - dup
    B = np.zeros((r, nb), np.uint8)
    for i in range(r):
        B[i, rng.choice(nb, 6, replace=False)] = 1
    for j in np.flatnonzero(~B.any(axis=0)):
        B[rng.integers(0, r), j] = 1
    B = np.concatenate([B, B[:, rng.choice(nb, dup, replace=False)]], axis=1)
    extra = np.zeros((m - r, n), np.uint8)
    for i in range(m - r):
        extra[i] = B[rng.choice(r, 3, replace=False)].sum(axis=0) & 1
    H = np.concatenate([B, extra])[rng.permutation(m)]
    return np.ascontiguousarray(H)


@functools.lru_cache(maxsize=None)
def matrix(name):
    """The case's matrix from the committed generator (read-only uint8 [m, n])."""
    c = CASES[name]
    if "r" in c:
        H = gen(name, c["m"], c["n"], c["r"], c["dup"])
    else:
        from qldpcsim_amd import codes, spacetime
        Hx = codes.load_code("LP04_0")[0]
        if "spacetime" in c:
            H = spacetime.spacetime_matrix(Hx, c["spacetime"])
        else:
            H = spacetime.window_matrix(Hx, c["window"])
        H = np.ascontiguousarray(H % 2, dtype=np.uint8)
    assert H.shape == (c["m"], c["n"])
    assert H.any(axis=0).all(), f"{name}: an all-zero column would send the whole code to the column kernel"
    H.setflags(write=False)
    return H


def equal_column_pairs(H):
    """(originals, copies): one pair of equal columns from every class of equal
    columns that has two members, in order of the original's index."""
    seen, first, second = {}, [], []
    cols = np.packbits(H, axis=0).T
    for j in range(H.shape[1]):
        key = cols[j].tobytes()
        if key not in seen:
            seen[key] = j
        elif seen[key] >= 0:
            first.append(seen[key])
            second.append(j)
            seen[key] = -1
    return np.array(first, np.int64), np.array(second, np.int64)


def _independent_first(H, cols, order):
    """`order` (indices into cols) with a greedily chosen linearly independent
    set of H's columns first: where 64 of the originals are independent, word 0
    of the crafted order holds 64 pivots."""
    packed = np.packbits(H, axis=0).T
    basis, indep, dep = {}, [], []
    for i in order:
        v = int.from_bytes(packed[cols[i]].tobytes(), "big")
        while v and (v.bit_length() in basis):
            v ^= basis[v.bit_length()]
        if v:
            basis[v.bit_length()] = v
            indep.append(i)
        else:
            dep.append(i)
    return np.array(indep + dep, np.int64)


def crafted(name):
    """True where the case carries crafted permutations (>= 64 pairs of equal columns)."""
    return len(equal_column_pairs(matrix(name))[0]) >= 64


@functools.lru_cache(maxsize=None)
def shots(name):
    """(H, syn, post, e0, perms) of the case's k shots, as osd_cs_cases.shots
    builds them: the first half of the syndromes from errors of density 0.03
    and the rest uniform, the posteriors' mean moving with the shot (0, 3, 6),
    every third consistent shot nearly decoded, every fifth column tied at
    1.75, e0 = post < 0. perms = argsort(|post|), stable; shot 0 and shot k-1
    of a crafted case have 64 originals at positions 0..63, their copies at
    64..127 and the rest shuffled."""
    H = matrix(name)
    m, n = H.shape
    k = CASES[name]["k"]
    rng = np.random.default_rng(zlib.crc32(f"osd-shape-shots-{name}-{k}{CASES[name].get('salt', '')}".encode()))
    syn = rng.integers(0, 2, (k, m)).astype(np.uint8)
    err = (rng.random((k // 2, n)) < 0.03).astype(np.int64)
    syn[: k // 2] = (err @ H.T.astype(np.int64)) % 2
    post = rng.normal(0, 3, (k, n)) + 3.0 * (np.arange(k) % 3)[:, None]
    near = np.arange(2, k // 2, 3)
    post[near] = (np.abs(post[near]) + 0.5) * (1 - 2 * err[near])
    post[:, ::5] = 1.75
    e0 = (post < 0).astype(np.uint8)
    perms = np.argsort(np.abs(post), axis=1, kind="stable").astype(np.int32)
    a, b = equal_column_pairs(H)
    if len(a) >= 64:
        for i in (0, k - 1):
            pick = _independent_first(H, a, rng.permutation(len(a)))[:64]
            rest = np.setdiff1d(np.arange(n), np.concatenate([a[pick], b[pick]]))
            perms[i] = np.concatenate([a[pick], b[pick], rng.permutation(rest)])
    perms = np.ascontiguousarray(perms)
    for x in (syn, post, e0, perms):
        x.setflags(write=False)
    return H, syn, post, e0, perms


def golden_shots(name):
    """Indices of the shots the reference goldens cover: the first and the last few."""
    k, e = CASES[name]["k"], GOLDEN_EDGE.get(name, 4)
    return np.concatenate([np.arange(e), np.arange(k - e, k)])


def order_posteriors(perm, e0):
    """Posteriors whose reliability order under the reference's own argsort is
    `perm` with no ties (|L| grows by 0.004 per position, at most 8.5: every
    reliability differs from the next by more than 1e-7) and whose signs are
    e0's. What the reference's OSDdec and apply_osd_device are fed."""
    n = len(perm)
    L = np.empty(n, np.float64)
    L[perm] = 0.004 * (1 + np.arange(n))
    return np.where(np.asarray(e0) != 0, -L, L)


@functools.lru_cache(maxsize=None)
def golden(name):
    """tests/golden/osd_shapes/osd_<name>.npz -> dict of read-only arrays
    (H, shots, syn, post, e0, perms, ehat0, ehat1, raised0, raised1)."""
    with np.load(os.path.join(GOLDEN_DIR, f"osd_{name}.npz"), allow_pickle=False) as z:
        out = {k: z[k] for k in z.files}
    shape = tuple(int(x) for x in out.pop("H_shape"))
    out["H"] = np.unpackbits(out.pop("H_bits"), axis=1, bitorder="little")[:, :shape[1]]
    assert out["H"].shape == shape
    out["meta"] = json.loads(bytes(out.pop("meta_json")).decode())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ref_model(name):
    """osd_ref_model.osd_ref_batch on the case's shots: (J list, e_hat order 0,
    e_hat order 1, consistent), once per process."""
    H, syn, _, e0, perms = shots(name)
    out = osd_ref_model.osd_ref_batch(H, syn, perms, e0, CASES[name]["rank"])
    for x in out[1:]:
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _cs_reduced(name):
    """The OSD-CS model's own reduction of every shot (it does not depend on lambda)."""
    import osd_cs_model
    H, syn, _, _, perms = shots(name)
    return [osd_cs_model.reduce_shot(H, syn[i], perms[i], CASES[name]["rank"]) for i in range(len(syn))]


@functools.lru_cache(maxsize=None)
def cs_model(name, lam):
    """The OSD-CS model's (e_hat, winner kinds, consistent) on the case's shots."""
    import osd_cs_model
    H, syn, _, e0, perms = shots(name)
    rank, red = CASES[name]["rank"], _cs_reduced(name)
    out = [osd_cs_model.osd_cs_one(H, syn[i], perms[i], e0[i], lam, rank, red[i]) for i in range(len(e0))]
    out = (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], bool))
    for x in out:
        x.setflags(write=False)
    return out


def host_ref(H, syn, perms, e0, order, nthreads=4):
    """qldpc_osd_decode_batch (the host C++ OSD, reference method)."""
    from qldpcsim_amd import _lib
    e = np.array(e0, dtype=np.uint8)
    _lib.check(_lib.lib.qldpc_osd_decode_batch(_lib.code_for(H).handle, len(e), _lib.ptr(np.ascontiguousarray(syn)),
                                               _lib.ptr(np.ascontiguousarray(perms)), int(order), _lib.ptr(e),
                                               nthreads))
    return e


@functools.lru_cache(maxsize=None)
def host(name, order):
    H, syn, _, e0, perms = shots(name)
    e = host_ref(H, syn, perms, e0, order)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def host_cs(name, lam):
    import osd_cs_cases
    H, syn, _, e0, perms = shots(name)
    e = osd_cs_cases.host_cs(H, syn, perms, e0, lam, nthreads=4)
    e.setflags(write=False)
    return e

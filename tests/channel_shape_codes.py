"""CSS pairs at the selection and word edges of the channel and phenomenological
kernels (channel_kernels.hip, phenom_kernels.hip).

The launchers pick an instantiation from the row degree shared by every row of
both halves (6, 7, 8, else 0), from n % 4 with the estimates' alignment (VEC)
and from the logical tables' residency (TLDS). The bundled codes reach fewer
than half of the 40 instances and none of the word edges (n % 64 == 0,
m % 64 == 0, m = 63, W = 64, (n + m) % 64 == 0). The seven pairs of CASES do.

Each pair is the hypergraph product of two small classical matrices A
[ma, na] and B [mb, nb],
    Hx = [A (x) I_nb | I_ma (x) B^T],   Hz = [I_na (x) B | A^T (x) I_mb],
so Hx Hz^T = A (x) B^T + A (x) B^T = 0 by construction. circ(L, taps) is the
L x L circulant whose row i has ones at columns (i + t) % L; hamming() is the
3 x 7 matrix whose column j is j + 1 in binary. Everything is generated:
tests/test_channel_shape_codes.py pins the bits, the shapes and k.

`batch` is the one crafted counter batch of a case: the oracle's restatement
of the device stream (the GPU tests assert the device draws the same shots)
and logical_model.craft's estimates on it.
"""
import functools
import hashlib

import numpy as np

import logical_model as lm

SEED = 0x9E3779B97F4A7C15
SHOT0 = 2 ** 32 - 100          # 257 shots from here cross the wrap of the shot counter's low word
P = 0.06

# id -> factors (circulant: (L, taps); else a name), the halves' shapes, row
# degrees (x, z) as (min, max), the degree the launchers specialise on (0: the
# generic loop), W = ceil(n / 64), k, shots of the sampler test, and what the
# case reaches
CASES = {
    "q8a": dict(A=(8, (0, 1, 2, 4)), B=(8, (0, 1, 2, 4)), mx=64, mz=64, n=128, deg=((8, 8), (8, 8)), udeg=8, W=2, k=2,
                shots=257, what="<8, true>, no padding bits; m % 64 == 0; (n + m) % 64 == 0; misaligned: <8, false>"),
    "q6v": dict(A=(6, (0, 1, 2)), B=(6, (0, 1, 2)), mx=36, mz=36, n=72, deg=((6, 6), (6, 6)), udeg=6, W=2, k=8,
                shots=257, what="<6, true, *>; phenomenological <6>"),
    "q6b": dict(A=(7, (0, 1, 3)), B=(9, (0, 1, 2)), mx=63, mz=63, n=126, deg=((6, 6), (6, 6)), udeg=6, W=2, k=12,
                shots=257, what="<6, false, *>; m = 63; two padding bits"),
    "q7v": dict(A=(7, (0, 1, 3)), B=(6, (0, 1, 2, 3)), mx=42, mz=42, n=84, deg=((7, 7), (7, 7)), udeg=7, W=2, k=12,
                shots=257, what="<7, true, *>; misaligned: <7, false>"),
    "q8b": dict(A=(5, (0, 1, 2, 3)), B=(7, (0, 1, 2, 4)), mx=35, mz=35, n=70, deg=((8, 8), (8, 8)), udeg=8, W=2, k=8,
                shots=257, what="<8, false, *> by shape; phenomenological <8>"),
    "g0v": dict(A="hamming", B="ones3", mx=9, mz=7, n=24, deg=((5, 5), (4, 6)), udeg=0, W=1, k=8,
                shots=257, what="<0, true, *>; mx != mz; non-uniform rows"),
    "w64": dict(A=(45, (0, 1, 2)), B=(45, (0, 1, 2)), mx=2025, mz=2025, n=4050, deg=((6, 6), (6, 6)), udeg=6, W=64,
                k=8, shots=65, what="W = 64, the limit: wq reaches 15; 32 row words of syndrome; 24,300 column indices"),
}
IDS = list(CASES)
# the halves the phenomenological sampler and counter tests run ("<case>_hz":
# Hz detects), and the one more the window tests run (n + m = 189)
HALVES = ("q8a_hz", "q6v_hz", "q8b_hz", "g0v_hx")
WINDOW_HALF = "q6b_hz"
VEC_CASES = ("q8a", "q6b", "g0v", "q7v")   # the vector sampler test: every degree
MISALIGNED = ("q8a", "q7v", "g0v")         # VEC by shape: byte estimates at an odd base drop to the byte path
LDS_BYTES = 163840             # of a workgroup on the MI355X
LDS_TAB_BYTES = 64 * 1024      # automatic residency: the most table bytes staged

SHA256 = {
    "q8a": "a8fbbc4d322746adad36462992b2e9212b471bae801598e66a535764f344f86a",
    "q6v": "452f647263db7e7b4d120939d9d103c65993c9c5e545ad6e8f1f84ec01f7df6d",
    "q6b": "63258087e7b2b04b763776416618c05c6e04da26ad1e8ee7e998b503de22544d",
    "q7v": "63ee631edbfcfacf77e4db0544d2f3ebb3a664b869927a32d9f69a8b10e18f56",
    "q8b": "abe835cdabead7c42a707bce232efe948c85a1dccd2fa83077ab89e2e06b07e8",
    "g0v": "22cc1b0281a2d779810e928748bfc7e7208e347a59c8a659d3a616f52ec8ec22",
    "w64": "b89e2112e586118efad8508bc69565f87cee58ae4c64b4dd5aef8b8f86eb9da7",
}


def circ(L, taps):
    C = np.zeros((L, L), np.uint8)
    for i in range(L):
        for t in taps:
            C[i, (i + t) % L] = 1
    return C


def hamming():
    return np.array([[(j >> b) & 1 for j in range(1, 8)] for b in range(3)], np.uint8)


def _factor(f):
    if f == "hamming":
        return hamming()
    if f == "ones3":
        return np.ones((1, 3), np.uint8)
    return circ(*f)


def hgp(A, B):
    """(Hx, Hz) of the hypergraph product, uint8."""
    (ma, na), (mb, nb) = A.shape, B.shape
    eye = lambda k: np.eye(k, dtype=np.uint8)  # noqa: E731
    Hx = np.concatenate([np.kron(A, eye(nb)), np.kron(eye(ma), B.T)], axis=1)
    Hz = np.concatenate([np.kron(eye(na), B), np.kron(A.T, eye(mb))], axis=1)
    return np.ascontiguousarray(Hx, dtype=np.uint8), np.ascontiguousarray(Hz, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def pair(name):
    """(Hx, Hz) of a case, read-only uint8."""
    c = CASES[name]
    Hx, Hz = hgp(_factor(c["A"]), _factor(c["B"]))
    assert Hx.shape == (c["mx"], c["n"]) and Hz.shape == (c["mz"], c["n"])
    Hx.setflags(write=False)
    Hz.setflags(write=False)
    return Hx, Hz


def packed_sha256(name):
    """sha256 of both halves' bits (rows packed little-endian, Hx then Hz) and shapes."""
    h = hashlib.sha256()
    for H in pair(name):
        h.update(np.array(H.shape, "<i4").tobytes())
        h.update(np.packbits(H, axis=1, bitorder="little").tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def logicals(name):
    from qldpcsim_amd import logicals as lg
    return lg.css_logicals(*pair(name))


@functools.lru_cache(maxsize=None)
def half(name):
    """(H, L, Hstab, Lop) of "<case>_hz" (the X half: Hz detects, Lz tests, the
    errors' own stabilisers and logical operators are Hx and Lx) or
    "<case>_hx" (the Z half), as test_phenom_model.half."""
    case, _, which = name.partition("_")
    Hx, Hz = pair(case)
    Lx, Lz = logicals(case)
    return (Hz, Lz, Hx, Lx) if which == "hz" else (Hx, Lx, Hz, Lz)


def kernel(name, kind, aligned=True, tabs_lds=False):
    """The instance the launchers must pick for a case, from the table alone."""
    c = CASES[name]
    d, tf = c["udeg"], ("false", "true")
    vec = tf[c["n"] % 4 == 0 and aligned]
    return {"sample": f"channel_sample_kernel<{d}>", "sample_vec": f"channel_sample_vec_kernel<{d}>",
            "count": f"count_outcomes_kernel<{d}, {vec}>",
            "count_logical": f"count_logical_kernel<{d}, {vec}, {tf[bool(tabs_lds)]}>"}[kind]


def phenom_kernel(name, kind):
    H = half(name)[0]
    deg = np.unique(H.sum(axis=1))
    d = int(deg[0]) if deg.size == 1 and deg[0] in (6, 7, 8) else 0
    return f"phenom_{kind}_kernel<{d}>"


def logical_lds_bytes(name, tabs_lds):
    """count_logical_kernel's LDS for a case, restated from its carve: both
    CSR tables (32-bit row pointers, 16-bit column indices, 8-byte aligned),
    two column masks, nine counters per wave, the two logical tables if staged,
    four W-word slots per wave; four waves."""
    Hx, Hz = pair(name)
    c = CASES[name]
    W, kp = c["W"], (c["k"] + 63) // 64 * 64
    b = (4 * (c["mz"] + 1 + c["mx"] + 1) + 2 * int(Hz.sum() + Hx.sum()) + 7) // 8 * 8
    b += 8 * 2 * W + 8 * 9 * 4
    if tabs_lds:
        b += 2 * 8 * W * kp
    return b + 4 * 4 * W * 8


def tabs_lds(name, mode):
    """The residency option logical_tabs = mode gives a case on the MI355X
    (None: mode 1 is refused)."""
    fits = logical_lds_bytes(name, True) <= LDS_BYTES
    if mode == 1:
        return True if fits else None
    kp = (CASES[name]["k"] + 63) // 64 * 64
    return mode == 0 and fits and 2 * 8 * CASES[name]["W"] * kp <= LDS_TAB_BYTES


@functools.lru_cache(maxsize=None)
def model(name):
    return lm.Model(*pair(name))


@functools.lru_cache(maxsize=None)
def batch(name, B=257, craft_seed=7):
    """The crafted counter batch of a case, computed once: shots SHOT0 ..
    SHOT0 + B - 1 of the stream SEED at p = P from the oracle, estimates from
    logical_model.craft (shot b: recipe b % 4 in the X half, (b // 4) % 4 in
    the Z half), iteration counts, and the model's classes, flip words and
    nine counters."""
    from oracle import oracle
    Hx, Hz = pair(name)
    Lx, Lz = logicals(name)
    sy_z, sy_x, errX, errZ = oracle.channel_sample(Hx, Hz, P, SEED, SHOT0, B)
    rng = np.random.default_rng(craft_seed)
    eX, eZ, recX, recZ = lm.craft(rng, Hx, Hz, Lx, Lz, errX, errZ)
    itX = rng.integers(1, 60, B).astype(np.int32)
    itZ = rng.integers(1, 60, B).astype(np.int32)
    M = model(name)
    cX, cZ = M.classes(sy_z, sy_x, errX, errZ, eX, eZ)
    d = dict(sy_z=sy_z, sy_x=sy_x, errX=errX, errZ=errZ, eX=eX, eZ=eZ, recX=recX, recZ=recZ, itX=itX, itZ=itZ,
             cX=cX, cZ=cZ, want=M.counters(sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ),
             flipX=lm.flip_words(Lz, errX ^ eX), flipZ=lm.flip_words(Lx, errZ ^ eZ), k=Lx.shape[0])
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def check_batch(d):
    """The input conditions of a crafted batch: every recipe and every class
    occurs at least 20 times in each half, and the recipes give their classes."""
    for c, rec in ((d["cX"], d["recX"]), (d["cZ"], d["recZ"])):
        assert (np.bincount(rec, minlength=4) >= 20).all(), np.bincount(rec, minlength=4)
        assert (np.bincount(c, minlength=3) >= 20).all(), np.bincount(c, minlength=3)
        assert (c[rec <= 1] == 0).all() and (c[rec == 2] == 1).all() and (c[rec == 3] == 2).mean() > 0.5
    lm.check_invariants(d["want"], d["cX"].shape[0])


def vec_table(name):
    """float64 [3, n] per-qubit (px, py, pz) for the vector sampler: qubits
    that never err, that always err (a threshold of 2^32 in each of the three
    rows), one whose probabilities sum to 1, and generic rows; every kind
    occurs, in an order fixed by the case name."""
    n = CASES[name]["n"]
    rows = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.25, 0.25, 0.5],
                     [0.02, 0.01, 0.15], [0.2, 0.0, 0.0], [0.0, 0.05, 0.4], [0.11, 0.07, 0.03]])
    rng = np.random.default_rng(sum(name.encode()))
    pick = np.concatenate([np.arange(len(rows)), rng.integers(0, len(rows), n - len(rows))])
    return np.ascontiguousarray(rows[rng.permutation(pick)].T)


@functools.lru_cache(maxsize=None)
def reference_counters(name):
    """The six counters of the case's batch by the reference's per-shot loop
    (simulator.py:291-303), as test_gpu_simulator restates it; the products are
    float32 (exact: 0/1 entries, sums below 2^24)."""
    from qldpcsim_amd import simulator
    d = batch(name)
    Hx, Hz = (H.astype(np.float32) for H in pair(name))
    errX, errZ, eX, eZ = d["errX"], d["errZ"], d["eX"], d["eZ"]
    want = dict.fromkeys(simulator.COUNTER_KEYS, 0)
    for k in range(errX.shape[0]):
        if np.array_equal(errX[k], eX[k]) and np.array_equal(errZ[k], eZ[k]):
            want["decSuccessExact"] += 1
        elif ((Hz @ (errX[k] ^ eX[k]).astype(np.float32)) == 0).all() and \
                ((Hx @ (errZ[k] ^ eZ[k]).astype(np.float32)) == 0).all():
            want["decSuccessDegen"] += 1
        want["DecFailures_X"] += int(not np.array_equal(d["sy_z"][k], (Hz @ eX[k].astype(np.float32)) % 2))
        want["DecFailures_Z"] += int(not np.array_equal(d["sy_x"][k], (Hx @ eZ[k].astype(np.float32)) % 2))
    want["nIterAccX"] = int(d["itX"].sum())
    want["nIterAccZ"] = int(d["itZ"].sum())
    return want

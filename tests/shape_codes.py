"""Synthetic parity-check matrices at the kernel-selection boundaries.

The bundled library has four codes of uniform row degree 7 / 8, so the
specialised kernels (ms_flood_kernel, ms_layered_kernel, the BP team kernels
and the DC = 7 / 8 instances of decode_kernel) only ever met four shapes. The
eight matrices here are built from a column-degree prescription so that each
reaches a kernel instance, a host decision or a branch no bundled code does
(the right-hand column of SHAPES below).

Everything is data: `code_from_degrees` is deterministic in its seed, the
matrices it gives are also stored bit-packed in tests/golden/shapes/ and
tests/test_shape_codes.py asserts the two agree, so a NumPy change cannot move
the shapes silently. Layer partitions are contiguous cuts of the (already
random) row order, or schedule.layerize.
"""
import functools

import numpy as np

MAX_RUNS = 8          # QLDPC_MAX_RUNS (decoder_kernels.h): runs of equal column degree in ms_flood_kernel's header


def code_from_degrees(m, dc, column_degrees, seed):
    """uint8 [m, n] matrix with every row of weight `dc` and the multiset of
    column weights `column_degrees` ((degree, count) pairs, degree sum m * dc),
    rows and columns in a random order.

    Row by row, the `dc` columns with the most unfilled entries take a one
    (ties broken at random); then both orders are shuffled."""
    rng = np.random.default_rng(seed)
    want = np.concatenate([np.full(c, d, np.int64) for d, c in column_degrees])
    n = len(want)
    assert want.sum() == m * dc, f"degree sum {want.sum()} != m * dc = {m * dc}"
    assert want.max() <= m
    left = want.copy()
    H = np.zeros((m, n), np.uint8)
    for r in range(m):
        order = np.lexsort((rng.random(n), -left))      # most stubs first, random among equals
        take = order[:dc]
        assert left[take].min() >= 1, f"row {r}: fewer than {dc} columns have an entry left"
        H[r, take] = 1
        left[take] -= 1
    assert not left.any()
    H = H[rng.permutation(m)][:, rng.permutation(n)]
    assert (H.sum(1) == dc).all()
    assert np.array_equal(np.sort(H.sum(0)), np.sort(want))
    return np.ascontiguousarray(H)


# id -> m, dc, (degree, count) list, generator seed, channel flip probability p
# (also the decoder's prior) of the GPU batches and of the goldens, and what
# the shape is for
SHAPES = {
    "A": dict(m=128, dc=8, seed=1001, p=0.02,
              degrees=[(0, 1), (1, 64), (2, 129), (3, 66), (4, 78), (6, 20), (7, 9), (9, 1)],
              what="ms_flood_kernel<8, 2>; no pad check; 8 runs; run counts 1 / 64 / 129; vn_run<0,1,2,6>, "
                   "vn_run_any"),
    "B": dict(m=192, dc=7, seed=1002, p=0.02,
              degrees=[(2, 128), (3, 200), (4, 61), (6, 30), (32, 2)],
              what="ms_flood_kernel<7, 4>; run of 128; column degree 32: no layered images"),
    "C": dict(m=512, dc=7, seed=1003, p=0.04,
              degrees=[(1, 4), (3, 700), (5, 200), (6, 80)],
              what="ms_flood_kernel<7, 8>; all 512 checks live; long pair loop plus tail"),
    "D": dict(m=257, dc=8, seed=1004, p=0.02,
              degrees=[(2, 313), (3, 256), (4, 100), (5, 40), (31, 2)],
              what="ms_flood_kernel<8, 8> with 255 pad checks; column degree 31 keeps the layered images"),
    "E": dict(m=96, dc=8, seed=1005, p=0.02,
              degrees=[(1, 40), (2, 50), (3, 48), (4, 30), (5, 30), (6, 12), (7, 8), (8, 5), (10, 1), (36, 1)],
              what="10 runs: no flood image, decode_kernel<0, false, 8>"),
    "F": dict(m=640, dc=8, seed=1006, p=0.008,
              degrees=[(2, 1600), (3, 400), (4, 170), (5, 8)],
              what="m > 512 and n > 2048: generic kernels at DC = 8, all-LDS layered BP team by necessity"),
    "G": dict(m=96, dc=8, seed=1007, p=0.02,
              degrees=[(3, 128), (6, 64)],
              what="layered `two` bit with K = 6"),
    # (164 columns, not 132 of degrees 4 / 6 alone: each half of 48 rows must touch more than 128 variables)
    "H": dict(m=96, dc=7, seed=1008, p=0.04,
              degrees=[(3, 64), (4, 60), (6, 40)],
              what="layered `lo3` without `two`, dmax = 6 with a mid degree"),
}
IDS = tuple(SHAPES)


@functools.lru_cache(maxsize=None)
def matrix(sid):
    s = SHAPES[sid]
    H = code_from_degrees(s["m"], s["dc"], s["degrees"], s["seed"])
    H.setflags(write=False)          # no caller changes H (the zero column of A stays)
    return H


def degree_runs(H):
    """(degree, count) of each run of equal column degree after the library's
    stable relabeling by degree (capi_code.cpp): one entry per distinct degree."""
    d, c = np.unique(np.asarray(H).sum(0), return_counts=True)
    return list(zip(d.tolist(), c.tolist()))


def cut(m, sizes):
    """Contiguous layers of the given sizes over rows 0..m-1."""
    assert sum(sizes) == m
    b = np.concatenate([[0], np.cumsum(sizes)])
    return [np.arange(b[i], b[i + 1]) for i in range(len(sizes))]


def serial(m):
    return [np.array([r]) for r in range(m)]


def layerized(sid):
    from qldpcsim_amd import schedule
    return schedule.layerize(matrix(sid))


C_CUT = (1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 149)
D_CUT = (1, 8, 9, 16, 17, 32, 33, 64, 65, 12)
A_CUT70 = (2,) * 58 + (1,) * 12


@functools.lru_cache(maxsize=None)
def partitions(sid):
    """name -> list of row arrays: every layered / serial schedule the tests
    run on shape `sid`."""
    m = SHAPES[sid]["m"]
    if sid == "A":
        return {"cut70": cut(m, A_CUT70), "serial": serial(m)}
    if sid == "C":
        return {"cut": cut(m, C_CUT)}
    if sid == "D":
        return {"cut": cut(m, D_CUT)}
    if sid in ("G", "H"):
        out = {"halves": cut(m, (48, 48)), "layerized": layerized(sid)}
        if sid == "H":
            out["serial"] = serial(m)
        return out
    return {"layerized": layerized(sid), "quarters": cut(m, (m // 4,) * 4)}


# the few-layer partition whose reference outputs tests/golden/shapes/ records
# (the reference's layered BP is slow with many layers)
GOLDEN_PARTITION = {"A": "cut70", "B": "quarters", "C": "cut", "D": "cut", "E": "quarters", "F": "quarters",
                    "G": "halves", "H": "halves"}


def packed(layers, m):
    from qldpcsim_amd import schedule
    return schedule.pack_layers(layers, m)


def channel_syndromes(H, p, shots, rng):
    """Syndromes of independent bit flips of probability p."""
    e = (rng.random((shots, H.shape[1])) < p).astype(np.int64)
    return ((e @ H.T.astype(np.int64)) % 2).astype(np.uint8)


GPU_SHOTS, GPU_RANDOM, GPU_MAX_ITER = 128, 32, 25


@functools.lru_cache(maxsize=None)
def batch(sid, shots=GPU_SHOTS, n_random=GPU_RANDOM):
    """The mixed batch of the GPU tests: `shots` channel shots at the shape's
    p plus `n_random` uniform-random syndromes, shuffled (decodes of very
    different lengths side by side)."""
    H = matrix(sid)
    rng = np.random.default_rng(SHAPES[sid]["seed"] + 50000)
    syn = np.concatenate([channel_syndromes(H, SHAPES[sid]["p"], shots, rng),
                          rng.integers(0, 2, (n_random, H.shape[0]), dtype=np.uint8)])
    syn = np.ascontiguousarray(syn[rng.permutation(len(syn))])
    syn.setflags(write=False)
    return syn


def gpu_runs(sid):
    """(algo, partition name or None for flooding) of every full batch
    tests/test_gpu_shapes.py decodes on shape `sid`: min-sum on every
    schedule, BP on all but the serial ones."""
    names = list(partitions(sid))
    return ([("MS", None)] + [("MS", k) for k in names] +
            [("BP", None)] + [("BP", k) for k in names if k != "serial"])


def layer_words(H, layers):
    """What capi_schedule.cpp puts into adj_dmax for each layer, as dicts:
    dmax (bits 0-4), lo3 (bit 7), two (bit 8), lanes per check of the
    per-layer switch (bits 5-6), and the layer's adjacency size."""
    H = np.asarray(H)
    deg = H.sum(0)
    out = []
    for rows in layers:
        adj = np.flatnonzero(H[np.asarray(rows)].any(0))
        d = deg[adj]
        dmax, dmin = int(d.max()), int(d.min())
        lo3 = dmin >= 3
        two = lo3 and not np.any((d > 3) & (d < dmax))
        rows_n = len(rows)
        lanes = 8 if rows_n <= 8 else 4 if rows_n <= 16 else 1
        out.append(dict(dmax=dmax, lo3=lo3, two=two, lanes=lanes, rows=rows_n, adj=len(adj)))
    return out


def uniform_lanes(H, layers):
    """Lanes per check the host gives ms_layered_kernel's template (capi_decode.cpp):
    the per-layer width where every layer wants the same, else 0 (the
    per-layer switch)."""
    w = {x["lanes"] for x in layer_words(H, layers)}
    return w.pop() if len(w) == 1 else 0


def golden_path(sid):
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shapes", f"shape_{sid}.npz")


@functools.lru_cache(maxsize=None)
def golden(sid):
    """(stored matrix uint8 [m, n], [(case dict, arrays dict), ...]) of
    tests/golden/shapes/shape_<sid>.npz (gen_golden_shapes.py)."""
    import json
    with np.load(golden_path(sid), allow_pickle=False) as z:
        m, n = (int(x) for x in z["H_shape"])
        H = np.unpackbits(z["H_bits"], axis=1, bitorder="little", count=n)
        assert H.shape == (m, n)
        cases = json.loads(bytes(z["cases_json"]).decode())
        return H, [(c, {k.split("_", 1)[1]: z[k] for k in z.files if k.startswith(f"c{i}_")})
                   for i, c in enumerate(cases)]

"""The synthetic shapes of tests/shape_codes.py on the CPU: the generator
reproduces the stored matrices, each shape has the property it was built for
(what capi_schedule.cpp / capi_decode.cpp decide from, restated in NumPy), the
oracle equals the reference's recorded outputs on them bit for bit, and every
batch the GPU tests decode mixes short and full-length decodes."""
import numpy as np
import pytest

import shape_codes as sc


def _ids(sid):
    return [f"{sid}-{c['algo']}-{c['sched']}" for c, _ in sc.golden(sid)[1]]


GOLDEN_CASES = [(sid, i) for sid in sc.IDS for i in range(len(sc.golden(sid)[1]))]
GOLDEN_IDS = [x for sid in sc.IDS for x in _ids(sid)]


# ---------------------------------------------------------------------------
# generator and shape properties
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sid", sc.IDS)
def test_generator_reproduces_stored_matrix(sid):
    H = sc.matrix(sid)
    stored, _ = sc.golden(sid)
    assert H.dtype == np.uint8 and not H.flags.writeable
    np.testing.assert_array_equal(H, stored)
    again = sc.code_from_degrees(sc.SHAPES[sid]["m"], sc.SHAPES[sid]["dc"], sc.SHAPES[sid]["degrees"],
                                 sc.SHAPES[sid]["seed"])
    np.testing.assert_array_equal(H, again)


@pytest.mark.parametrize("sid", sc.IDS)
def test_declared_degrees(sid):
    s, H = sc.SHAPES[sid], sc.matrix(sid)
    m, n = H.shape
    assert m == s["m"] and n == sum(c for _, c in s["degrees"])
    assert (H.sum(1) == s["dc"]).all()
    assert sc.degree_runs(H) == sorted(s["degrees"])
    # the unrolled kernels' table format (capi_internal.h fast_table_ok) and the 16-bit LDS tables
    E = int(H.sum())
    assert s["dc"] in (7, 8) and 8 * n < 65536 and 8 * E < 65536


def _kc(sid):
    return (sc.SHAPES[sid]["m"] + 63) // 64


def test_flood_image_properties():
    """What decides the flooding min-sum kernel: checks per lane ceil(m / 64)
    (<= 2, <= 4, <= 8: the instantiated widths), at most 8 degree runs, and
    the run counts / degrees that take each variable-node path."""
    runs = {sid: sc.degree_runs(sc.matrix(sid)) for sid in sc.IDS}
    # A: <8, 2>, no pad check, exactly QLDPC_MAX_RUNS runs, counts 1 / 64 / 129, K = 0, 1, 2, 6 and K >= 7
    assert _kc("A") == 2 and sc.SHAPES["A"]["m"] % 64 == 0
    assert len(runs["A"]) == sc.MAX_RUNS
    assert {1, 64, 129} <= {c for _, c in runs["A"]}
    assert {0, 1, 2, 6} <= {d for d, _ in runs["A"]} and max(d for d, _ in runs["A"]) >= 7
    assert (sc.matrix("A").sum(0) == 0).sum() == 1             # the zero column is in the matrix the tests decode
    # B: <7, 4>, a run of exactly 128 (two-chunk loop, no tail)
    assert _kc("B") == 3 and sc.SHAPES["B"]["dc"] == 7 and 128 in {c for _, c in runs["B"]}
    # C: <7, 8>, every one of the 512 checks live, a run with several pair trips and a masked tail
    assert _kc("C") == 8 and sc.SHAPES["C"]["m"] == 512
    assert any(c > 256 and c % 64 != 0 for _, c in runs["C"])
    # D: <8, 8>, one live check in the fifth 64-row group: 255 pad checks
    assert _kc("D") == 5 and sc.SHAPES["D"]["m"] % 64 == 1 and 512 - sc.SHAPES["D"]["m"] == 255
    # G, H: the <dc, 2> instances
    assert _kc("G") == 2 and _kc("H") == 2
    for sid in "ABCDGH":
        assert len(runs[sid]) <= sc.MAX_RUNS and sc.SHAPES[sid]["m"] <= 512
    # E: more runs than the header holds; F: more checks than a lane owns: no flood image
    assert len(runs["E"]) >= sc.MAX_RUNS + 1 and sc.SHAPES["E"]["m"] <= 512
    assert sc.SHAPES["F"]["m"] > 512
    # BP team variable nodes: np.sum's order changes at 8 addends
    assert max(d for d, _ in runs["A"]) >= 8 and max(d for d, _ in runs["E"]) >= 8


def test_layered_image_conditions():
    """layered_ms / layered_bp exist for n <= 2048 and column degree <= 31."""
    have = {sid: sc.matrix(sid).shape[1] <= 2048 and sc.matrix(sid).sum(0).max() <= 31 for sid in sc.IDS}
    assert have == dict(A=True, B=False, C=True, D=True, E=False, F=False, G=True, H=True)
    assert sc.matrix("B").sum(0).max() == 32 and sc.matrix("D").sum(0).max() == 31
    assert sc.matrix("F").shape[1] > 2048 and sc.matrix("F").sum(0).max() <= 31


def test_partitions_cover_rows_once():
    for sid in sc.IDS:
        m = sc.SHAPES[sid]["m"]
        for name, layers in sc.partitions(sid).items():
            rows = np.concatenate(layers)
            np.testing.assert_array_equal(np.sort(rows), np.arange(m), err_msg=f"{sid} {name}")
            assert len(layers) > 1
    assert sc.GOLDEN_PARTITION.keys() == set(sc.IDS)
    assert all(sc.GOLDEN_PARTITION[s] in sc.partitions(s) for s in sc.IDS)


def test_partition_layer_sizes():
    """The per-layer lane-group switch at its edges (rows <= 8, <= 16, more),
    the pair path's 32 / 33, one or two check-node trips at 64 / 65, and
    schedules past the 64 layers whose bounds fit the wave's registers."""
    size = lambda sid, name: [len(l) for l in sc.partitions(sid)[name]]
    assert tuple(size("C", "cut")) == sc.C_CUT and tuple(size("D", "cut")) == sc.D_CUT
    for cutsz in (sc.C_CUT, sc.D_CUT):
        assert {8, 9, 16, 17, 32, 33, 64, 65} <= set(cutsz)
        assert len(cutsz) <= 64
    assert sc.uniform_lanes(sc.matrix("C"), sc.partitions("C")["cut"]) == 0
    assert sc.uniform_lanes(sc.matrix("D"), sc.partitions("D")["cut"]) == 0
    assert {x["lanes"] for x in sc.layer_words(sc.matrix("C"), sc.partitions("C")["cut"])} == {1, 4, 8}
    # A: 70 layers of one or two rows, and the serial schedules: lreg == false, 8 lanes per check
    assert size("A", "cut70") == [2] * 58 + [1] * 12
    for sid, name in (("A", "cut70"), ("A", "serial"), ("H", "serial")):
        assert len(sc.partitions(sid)[name]) > 64
        assert sc.uniform_lanes(sc.matrix(sid), sc.partitions(sid)[name]) == 8
    assert size("A", "serial") == [1] * 128 and size("H", "serial") == [1] * 96
    for sid in "GH":
        assert size(sid, "halves") == [48, 48]
        assert sc.uniform_lanes(sc.matrix(sid), sc.partitions(sid)["halves"]) == 1
    for sid in "BEF":
        m = sc.SHAPES[sid]["m"]
        assert size(sid, "quarters") == [m // 4] * 4


def _words(sid, name):
    return sc.layer_words(sc.matrix(sid), sc.partitions(sid)[name])


def test_layer_degree_words():
    """adj_dmax as capi_schedule.cpp builds it (dmax, lo3, two) and the
    adjacency sizes on either side of 128, per layer."""
    # G: `two` with K = 6 in every layer; halves above 128 adjacent variables, layerized below
    for name, big in (("halves", True), ("layerized", False)):
        for w in _words("G", name):
            assert (w["dmax"], w["lo3"], w["two"]) == (6, True, True), (name, w)
            assert (w["adj"] > 128) == big, (name, w)
    # H: lo3 without two at dmax = 6 (a degree-4 variable in the layer) in both halves ...
    for w in _words("H", "halves"):
        assert (w["dmax"], w["lo3"], w["two"]) == (6, True, False) and w["adj"] > 128, w
    # ... and small layers in every combination of {3, 4, 6}: dmax 4, and dmax 6 with and without two
    for name in ("layerized", "serial"):
        got = {(w["dmax"], w["lo3"], w["two"]) for w in _words("H", name)}
        assert got == {(4, True, True), (6, True, False), (6, True, True)}, (name, got)
        assert all(w["adj"] <= 128 for w in _words("H", name))
    # C and D: adjacencies on both sides of 128 within one schedule
    for sid in "CD":
        adj = [w["adj"] for w in _words(sid, "cut")]
        assert min(adj) <= 128 < max(adj)
    # C: dmax 6 with and without lo3; D: dmax 4 (two) and the default branch (31); A: 4, 6 and the default (7, 9)
    assert {(w["dmax"], w["lo3"]) for w in _words("C", "cut")} == {(6, False), (6, True)}
    assert {(4, True, True), (31, False, False)} <= {(w["dmax"], w["lo3"], w["two"]) for w in _words("D", "cut")}
    assert {4, 6, 7, 9} <= {w["dmax"] for w in _words("A", "cut70")}
    assert max(w["dmax"] for sid, name in (("A", "cut70"), ("C", "cut"), ("D", "cut")) for w in _words(sid, name)) <= 31


# ---------------------------------------------------------------------------
# the oracle against the reference's recorded outputs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sid,i", GOLDEN_CASES, ids=GOLDEN_IDS)
def test_oracle_equals_reference_golden(sid, i):
    from oracle import numpy_dense, oracle
    H = sc.matrix(sid)
    c, a = sc.golden(sid)[1][i]
    assert c["max_iter"] == 20 and len(a["syn"]) == 16
    layers = None if c["sched"] == "F" else sc.partitions(sid)[c["sched"]]
    lp, lr = sc.packed(layers, H.shape[0])
    np.testing.assert_array_equal(lp, a["layer_ptr"])
    np.testing.assert_array_equal(lr, a["layer_rows"])
    e, it, post, _ = oracle.decode_batch(c["algo"], H, a["syn"], c["p"], c["max_iter"], lp, lr)
    k = len(a["post"])
    assert k >= 8
    np.testing.assert_array_equal(it, a["iters"])
    np.testing.assert_array_equal(e, a["ehat"])
    np.testing.assert_array_equal(post[:k].view(np.uint64), a["post"].view(np.uint64))
    if c["algo"] == "MS":
        de, dit, dpost = numpy_dense.decode_batch_dense(H, a["syn"][:k], c["p"], c["max_iter"], layers)
        np.testing.assert_array_equal(dit, it[:k])
        np.testing.assert_array_equal(de, e[:k])
        np.testing.assert_array_equal(dpost.view(np.uint64), post[:k].view(np.uint64))


# ---------------------------------------------------------------------------
# the GPU batches mix short and full-length decodes
# ---------------------------------------------------------------------------
RUNS = [(sid, algo, name) for sid in sc.IDS for algo, name in sc.gpu_runs(sid)]


@pytest.mark.parametrize("sid,algo,name", RUNS, ids=[f"{s}-{a}-{n or 'flooding'}" for s, a, n in RUNS])
def test_batch_mixes_short_and_full_decodes(sid, algo, name):
    """Premise of every batch tests/test_gpu_shapes.py decodes (128 channel
    shots at the shape's p plus 32 random syndromes, max_iter 25), on the
    oracle alone: at least 8 half-shots stop within 4 iterations and at least
    8 run all of them, so waves pick up new half-shots at different times."""
    from oracle import oracle
    H = sc.matrix(sid)
    syn = sc.batch(sid)
    assert syn.shape == (sc.GPU_SHOTS + sc.GPU_RANDOM, H.shape[0])
    lp, lr = sc.packed(None if name is None else sc.partitions(sid)[name], H.shape[0])
    e, it, _, _ = oracle.decode_batch(algo, H, syn, sc.SHAPES[sid]["p"], sc.GPU_MAX_ITER, lp, lr, want_post=False)
    assert (it <= 4).sum() >= 8, (it <= 4).sum()
    assert (it == sc.GPU_MAX_ITER).sum() >= 8, (it == sc.GPU_MAX_ITER).sum()
    ok = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(1)
    assert ok[it < sc.GPU_MAX_ITER].all()              # an early stop reproduces its syndrome

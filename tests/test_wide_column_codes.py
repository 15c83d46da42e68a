"""The wide-column shapes of tests/wide_column_codes.py on the CPU: each matrix
has the degrees it was built for and each heavy column the np.sum split it
was chosen for; the batched column sum of tests/wide_column_model.py equals
np.sum of each contiguous column bit for bit; on every shape with a column
past 128 entries the old association (eight accumulators over the whole
column) gives other posterior bits than np.sum's on the shape's batch, so a
GPU comparison there can fail; and the references alone meet what the GPU
tests rely on: finite posteriors, converged and full-length decodes, an
estimate that sets a heavy variable, the C oracle and the NumPy model equal
under a uniform prior."""
import numpy as np
import pytest

import prior_model as pm
import wide_column_codes as wc
import wide_column_model as wm
from qldpcsim_amd import _lib

MAX_ITER = wc.GPU_MAX_ITER
SHAPE = dict(W0=(192, 409), W1=(200, 423), W2=(520, 1106), W3=(1536, 3102), W4=(300, 644), U8=(192, 409))
# the tree np.sum adds each heavy degree in (a leaf: 8 accumulators, or in sequence below 8)
SPLITS = {7: 7, 8: 8, 9: 9, 15: 15, 16: 16, 17: 17, 64: 64, 127: 127, 128: 128,
          129: (64, 65), 136: (64, 72), 255: (120, (64, 71)), 256: (128, 128), 257: (128, (64, 65)),
          272: ((64, 72), (64, 72)), 513: ((128, 128), (128, (64, 65))),
          1024: (((128, 128), (128, 128)), ((128, 128), (128, 128))),
          1025: (((128, 128), (128, 128)), ((128, 128), (128, (64, 65))))}
DEPTH = {129: 1, 136: 1, 255: 2, 256: 1, 257: 2, 272: 2, 513: 3, 1024: 3, 1025: 4}
SHAPE_DEPTH = dict(W0=0, W1=1, W2=3, W3=4, W4=2, U8=0)
FLOOD = lambda m: (np.array([0, m], np.int32), np.arange(m, dtype=np.int32))  # noqa: E731


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sid", wc.IDS)
def test_matrix_shapes_and_degrees(sid):
    H = wc.matrix(sid)
    s = wc.SHAPES[sid]
    assert H.shape == SHAPE[sid] and H.dtype == np.uint8 and not H.flags.writeable and s["what"]
    rows, cols = H.sum(1), H.sum(0)
    hv = wc.heavy_columns(sid)
    assert tuple(sorted(cols[hv].tolist())) == wc.heavy_degrees(sid)
    light = np.delete(cols, hv)
    # the LDS kernels' 16-bit tables hold it: only a degree sends a decode to the HBM kernels
    assert max(H.shape) <= 65535 and int(H.sum()) <= 65535
    if sid == "U8":
        assert (rows == 8).all() and set(light.tolist()) == {2, 3, 4} and wc.heavy_degrees(sid) == (64, 127, 128)
        return
    assert wc.heavy_degrees(sid) == tuple(sorted(s["heavy"]))
    assert set(light.tolist()) <= ({2, 3, 4} if sid == "W4" else {2, 3}) and (light >= 2).all()
    assert (np.delete(H, hv, axis=1).sum(1) >= wc.MIN_LIGHT).all()        # every row has light entries
    if sid == "W4":                                                       # one row past the 64-edge registers
        assert rows[0] > 64 and np.delete(rows, 0).max() <= 32
    else:
        assert rows.max() <= 32                                           # min-sum stays on the LDS kernels
    # no two heavy columns are near twins (their common flip would be almost undetected)
    big = H[:, hv[cols[hv] >= 64]].astype(np.int64)
    both = big.T @ big
    assert (both - np.diag(np.diag(both))).max() <= 0.95 * s["m"]


def test_matrices_and_batches_are_deterministic():
    for sid in wc.IDS:
        s = wc.SHAPES[sid]
        if s["kind"] == "comb":
            again = wc.comb_code(s["m"], s["heavy"], s["n_light"], s["seed"], s.get("wide_row", 0))
            np.testing.assert_array_equal(wc.matrix(sid), again)
        syn = wc.batch(sid)
        assert syn.shape == (wc.GPU_SHOTS + wc.GPU_RANDOM, s["m"]) and syn.dtype == np.uint8
        assert not syn.flags.writeable and syn.max() == 1 and len(syn) > 64        # more than one 64-slot tile
        q = wc.prior_row(sid)
        assert (q > 0.5).sum() >= 3 and not (q == 0.5).any() and q[int(np.argmax(wc.matrix(sid).sum(0)))] == 0.6


def test_heavy_degrees_reach_the_splits():
    """Every heavy degree of the table, its split sizes and its depth
    (hbm_kernels.h hbm_column_depth restated), and per shape the dynamic LDS
    the HBM kernels' BP instances get."""
    seen = set()
    for sid in wc.IDS:
        for d in wc.heavy_degrees(sid):
            assert wc.splits(d) == SPLITS[d], d
            assert wc.column_depth(d) == DEPTH.get(d, 0), d
            seen.add(d)
        assert wc.hbm_lds_bytes(wc.matrix(sid)) == SHAPE_DEPTH[sid] * 2048
    assert seen == set(SPLITS)
    # the <= 128 rule's forms on W0: sequential, one block, remainders of 1 and 7, the largest block
    assert [d % 8 for d in (9, 15, 17, 127)] == [1, 7, 1, 7] and {7, 8, 16, 64, 128} <= set(wc.heavy_degrees("W0"))
    assert wc.WIDE == ("W1", "W2", "W3", "W4")
    # past the chunk_dmax clamp (capi_schedule.cpp) for min-sum
    assert min(wc.heavy_degrees("W3")) > 255


def test_kernel_names_without_a_device(qopt):
    """The per-variable-prior names need no device: the LDS twin on W0 and U8,
    the refusal past 128 entries, and with option vprior_hbm the HBM instance
    by row degree (W4: 64). The two-level twin refuses W1."""
    for sid in wc.IDS:
        H = wc.matrix(sid)
        if sid in wc.WIDE:
            with pytest.raises(NotImplementedError, match=f"BP column degree {max(wc.heavy_degrees(sid))} > 128"):
                _lib.vprior_kernel_name(H, *FLOOD(H.shape[0]), "BP")
        else:
            dc = 8 if sid == "U8" else 0
            assert _lib.vprior_kernel_name(H, *FLOOD(H.shape[0]), "BP") == f"decode_vprior_kernel<1, false, {dc}>"
    with pytest.raises(NotImplementedError, match="two-level priors: BP column degree 129 > 128"):
        _lib.prior_kernel_name(wc.matrix("W1"), *FLOOD(200), "BP")
    qopt(vprior_hbm=1)
    for sid in wc.WIDE:
        H = wc.matrix(sid)
        d = int(H.sum(1).max())
        inst = 16 if d <= 16 else 32 if d <= 32 else 64
        assert 8 < d and _lib.vprior_kernel_name(H, *FLOOD(H.shape[0]), "BP") == f"hbm_tile_vprior_kernel<1, {inst}, 4>"
    assert int(wc.matrix("W4").sum(1).max()) > 64
    qopt(force_hbm=1)
    assert _lib.vprior_kernel_name(wc.matrix("W0"), *FLOOD(192), "BP") == "hbm_tile_vprior_kernel<1, 32, 4>"


# ---------------------------------------------------------------------------
# the model's batched column sum is np.sum's
# ---------------------------------------------------------------------------
def test_batched_column_sum_equals_np_sum():
    """pairwise_sum over [shots, variables, d] against np.sum of each
    contiguous 1-D column, bit for bit, at every heavy degree of the table and
    around each rule's edges; messages of both signs and very different sizes
    (any other association then rounds differently somewhere)."""
    rng = np.random.default_rng(11)
    for d in sorted(set(SPLITS) | {1, 2, 6, 10, 63, 65, 130, 143, 144, 1000}):
        M = rng.standard_normal((40, 3, d)) * 10.0 ** rng.integers(-3, 3, (40, 3, d))
        got = wm.pairwise_sum(M)
        want = np.array([[np.sum(np.ascontiguousarray(M[b, j])) for j in range(3)] for b in range(40)])
        np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64), err_msg=f"d = {d}")
        ctl = wm.pairwise_sum(M, "strided8")
        if d <= 128:
            np.testing.assert_array_equal(ctl.view(np.uint64), want.view(np.uint64))
        else:
            assert (ctl.view(np.uint64) != want.view(np.uint64)).any(), d
    # columns not yet reached read as +0.0: a column of zeros sums to +0.0 at every length
    for d in (3, 8, 129, 513):
        z = wm.pairwise_sum(np.zeros((2, 1, d)))
        assert not z.any() and not np.signbit(z).any()


# ---------------------------------------------------------------------------
# the batches tell the two associations apart
# ---------------------------------------------------------------------------
DISCRIMINATE = [(sid, sched) for sid in wc.WIDE for sched in ("F", "S5")]


@pytest.mark.parametrize("sid,sched", DISCRIMINATE, ids=[f"{s}-{k}" for s, k in DISCRIMINATE])
def test_old_association_changes_posterior_bits(sid, sched):
    """The control model (eight accumulators over the whole column) and the
    np.sum model differ in posterior bits on at least one shot of the batch,
    under the scalar prior and under the prior row: a kernel that keeps the
    old association fails the GPU comparison on this shape."""
    for want, ctl in ((wm.want_uniform(sid, sched), wm.want_uniform(sid, sched, "strided8")),
                      (wm.want_vprior(sid, sched), wm.want_vprior(sid, sched, "strided8"))):
        differ = (want[2].view(np.uint64) != ctl[2].view(np.uint64)).any(1)
        assert differ.sum() >= 8, differ.sum()


def test_shapes_within_128_do_not_discriminate():
    """W0 and U8 stay within the unsplit rule: both models agree there."""
    for sid in ("W0", "U8"):
        a, b = wm.want_uniform(sid, "F"), wm.want_uniform(sid, "F", "strided8")
        np.testing.assert_array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


# ---------------------------------------------------------------------------
# what the GPU tests rely on, on the references alone
# ---------------------------------------------------------------------------
def _conditions(sid, out, heavy=True):
    e, it, post, _ = out
    H = wc.matrix(sid)
    assert np.isfinite(post).all()
    assert (it < MAX_ITER).sum() >= 2 and (it == MAX_ITER).sum() >= 2, np.bincount(it)
    ok = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == wc.batch(sid)).all(1)
    assert ok[it < MAX_ITER].all()
    if heavy:
        assert e[:, wc.heavy_columns(sid)].any()


SCALAR = [(sid, sched) for sid in wc.IDS for sched in ("F", "L", "S5")] + [("W2", "NP")]


@pytest.mark.parametrize("sid,sched", SCALAR, ids=[f"{s}-{k}" for s, k in SCALAR])
def test_scalar_bp_reference(sid, sched):
    _conditions(sid, wm.want_scalar("BP", sid, sched))


VPRIOR = [(sid, sched) for sid in ("W0", "W1", "W2", "W3") for sched in ("F", "S5")]


@pytest.mark.parametrize("sid,sched", VPRIOR, ids=[f"{s}-{k}" for s, k in VPRIOR])
def test_vprior_bp_reference(sid, sched):
    L = wm.prior_llr(sid)
    assert (L < 0).sum() >= 3 and (L != 0).all() and np.isfinite(L).all()
    assert L[int(np.argmax(wc.matrix(sid).sum(0)))] < 0                    # an entry above 0.5 on the heaviest column
    out = wm.want_vprior(sid, sched)
    _conditions(sid, out)
    sat = ((out[0].astype(np.int64) @ wc.matrix(sid).T.astype(np.int64)) % 2 == wc.batch(sid)).all(1)
    np.testing.assert_array_equal((out[3] & wm.FLAG_CONVERGED) != 0, sat)


MIN_SUM = [("W2", "F"), ("W2", "L"), ("W3", "F"), ("W3", "S5"), ("W3", "L")]


@pytest.mark.parametrize("sid,sched", MIN_SUM, ids=[f"{s}-{k}" for s, k in MIN_SUM])
def test_min_sum_reference(sid, sched):
    _conditions(sid, wm.want_scalar("MS", sid, sched), heavy=False)


UNIFORM = [(sid, sched) for sid in wc.IDS for sched in ("F", "S5")] + [(sid, "L") for sid in ("W0", "W1", "U8")]


@pytest.mark.parametrize("sid,sched", UNIFORM, ids=[f"{s}-{k}" for s, k in UNIFORM])
def test_oracle_equals_the_numpy_model_under_a_uniform_prior(sid, sched):
    """oracle.decode_batch (C, np_pairwise recursing at any length) and
    decode_bp with L = llr(p) on every variable: iterations, estimates and
    posterior bits. (schedule.layerize on the small shapes only: the model
    spends its time per layer.)"""
    e, it, post, _ = wm.want_scalar("BP", sid, sched)
    me, mit, mpost, mfl = wm.want_uniform(sid, sched)
    np.testing.assert_array_equal(mit, it)
    np.testing.assert_array_equal(me, e)
    np.testing.assert_array_equal(mpost.view(np.uint64), post.view(np.uint64))


def test_model_equals_the_shot_by_shot_loop():
    """decode_bp against bp_flood_numpy (np.sum itself on every column) on
    the first shots of W1 with the prior row."""
    H, syn = wc.matrix("W1"), wc.batch("W1")[:6]
    e, it, post = wm.bp_flood_numpy(H, syn, wm.prior_llr("W1"), 3)
    me, mit, mpost, _ = wm.decode_bp(wm.graph("W1"), syn, wm.prior_llr("W1"), 3)
    np.testing.assert_array_equal(mit, it)
    np.testing.assert_array_equal(me, e)
    np.testing.assert_array_equal(mpost.view(np.uint64), post.view(np.uint64))
    assert pm.llr(0.6) < 0

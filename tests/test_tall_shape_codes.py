"""The tall shapes of tests/tall_shape_codes.py on the CPU: each matrix has the
shape and degree facts it was built for, every batch the GPU tests decode
exercises the checks past the generic kernel's 2048-check register and mixes
short and full-length decodes, the two hand-made shots decode differently,
the oracle equals the reference's recorded outputs on T2 and U1 bit for bit,
and the NumPy models the GPU tests use as references run in seconds. All of it
on the oracle alone, so that no GPU comparison passes vacuously."""
import time

import numpy as np
import pytest

import shape_codes as sc
import tall_shape_codes as ts

REG = ts.REG_CHECKS


# ---------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------
def test_matrix_shapes_and_degrees():
    want = dict(T0=(2048, 2088), T1=(2049, 2089), T2=(2113, 2153), T3=(4100, 4101), U0=(1023, 2046), U1=(1024, 2048))
    for sid in ts.IDS:
        H = ts.matrix(sid)
        assert H.shape == want[sid] and H.dtype == np.uint8 and not H.flags.writeable
        # the LDS kernels' 16-bit tables hold it (capi_code.cpp lds_ok)
        assert max(H.shape) <= 65535 and int(H.sum()) <= 65535
        # MS row degree <= 32, BP column degree <= 128: no HBM-resident plan for either reason; column
        # degree < 8: tests/prior_model.py's sequential BP column sums are np.sum's
        assert H.sum(1).max() <= 32 and H.sum(0).max() < 8
    assert ts.matrix("T0").shape[0] == REG                 # the last size the register holds
    for sid in ("T0", "T1", "T2"):
        H = ts.matrix(sid)
        rows, cols = H.sum(1), H.sum(0)
        assert set(rows.tolist()) == {2, 3}
        third = (rows == 3).mean()
        assert 0.28 < third < 0.39                         # a random third of the rows
        assert (cols == 1).sum() >= 1                      # the chain's end: column 0 before the shuffle
        # the chain's first row is the last check, and one column touches it alone
        assert (H[:, np.flatnonzero(H[-1])].sum(0) == 1).sum() == 1
        assert not ts.fast_table_ok(H)
    # T1: one check in a 33rd pass; T2: a full 33rd pass and one check of a 34th
    assert ts.matrix("T1").shape[0] - REG == 1
    m, n = ts.matrix("T2").shape
    assert m - REG == 65 and m % 64 == 1 and n % 64 != 0
    cols = ts.matrix("T2").sum(0)
    assert (cols == 0).sum() >= 1 and cols.max() in (5, 6, 7)       # a zero column, degrees up to about 6
    E2 = int(ts.matrix("T2").sum())
    assert 4800 < E2 < 5000
    # T3: the plain chain, more than 64 passes of 64 lanes
    H = ts.matrix("T3")
    assert int(H.sum()) == 8200 and (H.sum(1) == 2).all() and H.shape[0] > 64 * 64
    r = np.arange(H.shape[0])
    assert H[r, r].all() and H[r, r + 1].all()


def test_matrices_are_deterministic():
    for sid in ("T2", "U1"):
        s = ts.SHAPES[sid]
        again = ts.chain_code(s["m"], s["extra"], s["seed"]) if sid == "T2" else \
            sc.code_from_degrees(s["m"], s["dc"], s["degrees"], s["seed"])
        np.testing.assert_array_equal(ts.matrix(sid), again)
        stored, _ = ts.golden(sid)
        np.testing.assert_array_equal(ts.matrix(sid), stored)


def test_u_shapes_straddle_the_fast_table_limit():
    """fast_table_ok (capi_internal.h) restated: uniform row degree 7 or 8,
    8 * n < 65536 and 8 * E < 65536. U0 is the largest degree-8 code that has
    it, U1 the smallest that has not; only E decides."""
    for sid, E, fast in (("U0", 8184, True), ("U1", 8192, False)):
        H = ts.matrix(sid)
        m, n = H.shape
        assert (H.sum(1) == 8).all() and int(H.sum()) == E == 8 * m
        assert set(H.sum(0).tolist()) == {3, 4, 5}
        assert 8 * n < 65536                               # not the n edge
        ok = bool((H.sum(1) == 8).all()) and 8 * n < 65536 and 8 * E < 65536
        assert ok == fast == ts.fast_table_ok(H)
        assert ts.dc_of(sid) == (8 if fast else 0)
    assert 8 * 8184 == 65536 - 64 and 8 * 8192 == 65536


# ---------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ts.IDS)
def test_batch_layout(sid):
    syn = ts.batch(sid)
    m = ts.matrix(sid).shape[0]
    extra = 2 if sid in ts.TALL else 0
    assert syn.shape == (ts.GPU_SHOTS + ts.GPU_RANDOM + extra, m) and syn.dtype == np.uint8
    assert not syn.flags.writeable and syn.max() == 1
    assert ts.model_batch(sid).shape == (ts.MODEL_SHOTS, m)
    if extra:
        hi, lo = syn[-2], syn[-1]
        np.testing.assert_array_equal(ts.model_batch(sid)[-2:], syn[-2:])
        assert not hi[:REG].any() and hi[REG:].all()       # only checks of index >= 2048 fire, and all of them
        fired = np.flatnonzero(hi)
        np.testing.assert_array_equal(np.flatnonzero(lo), np.unique((fired - REG) % REG))
        assert not lo[REG:].any()


@pytest.mark.parametrize("sid", ts.TALL)
def test_fired_high_checks(sid):
    """At least a quarter of the shots fire a check past the register (T2: 92
    of 114), in the full batch and in the shots the NumPy models decode."""
    for syn in (ts.batch(sid), ts.model_batch(sid)):
        high = syn[:, REG:].any(1).sum()
        assert 4 * high >= len(syn), (sid, high, len(syn))


FLOODING = [(sid, algo) for sid in ts.IDS for algo in ("MS", "BP")]


@pytest.mark.parametrize("sid,algo", FLOODING, ids=[f"{s}-{a}" for s, a in FLOODING])
def test_batch_mixes_short_and_full_decodes(sid, algo):
    """oracle.decode_batch at 25 iterations: at least 8 shots stop after two
    or more iterations and at least 8 run to the end; an early stop
    reproduces its syndrome."""
    from oracle import oracle
    H, syn = ts.matrix(sid), ts.batch(sid)
    lp, lr = ts.packed(sid, False)
    e, it, _, _ = oracle.decode_batch(algo, H, syn, ts.SHAPES[sid]["p"], ts.GPU_MAX_ITER, lp, lr, want_post=False)
    stopped = (it >= 2) & (it < ts.GPU_MAX_ITER)
    assert stopped.sum() >= 8, stopped.sum()
    assert (it == ts.GPU_MAX_ITER).sum() >= 8, (it == ts.GPU_MAX_ITER).sum()
    ok = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(1)
    assert ok[it < ts.GPU_MAX_ITER].all()


@pytest.mark.parametrize("algo", ["MS", "BP"])
@pytest.mark.parametrize("sid", ts.TALL)
def test_hand_made_shots_decode_differently(sid, algo):
    """The shot fired past the register and its folded image give different
    estimates: a kernel that reads one for the other fails the comparison."""
    from oracle import oracle
    lp, lr = ts.packed(sid, False)
    e, _, _, _ = oracle.decode_batch(algo, ts.matrix(sid), ts.batch(sid)[-2:], ts.SHAPES[sid]["p"], ts.GPU_MAX_ITER,
                                     lp, lr, want_post=False)
    assert (e[0] != e[1]).any()


# ---------------------------------------------------------------------------
# the oracle against the reference's recorded outputs
# ---------------------------------------------------------------------------
GOLDEN_CASES = [(sid, i) for sid in ts.GOLDEN_IDS for i in range(len(ts.GOLDEN_ALGOS))]


@pytest.mark.parametrize("sid,i", GOLDEN_CASES,
                         ids=[f"{s}-{ts.GOLDEN_ALGOS[i][0]}-{ts.GOLDEN_ALGOS[i][1]}" for s, i in GOLDEN_CASES])
def test_oracle_equals_reference_golden(sid, i):
    from oracle import oracle
    H = ts.matrix(sid)
    c, a = ts.golden(sid)[1][i]
    assert (c["algo"], c["sched"]) == ts.GOLDEN_ALGOS[i] and c["max_iter"] == 20 and c["p"] == ts.SHAPES[sid]["p"]
    assert len(a["syn"]) == 8
    np.testing.assert_array_equal(a["syn"], ts.batch(sid)[:8])
    lp, lr = ts.packed(sid, c["sched"] == "L")
    np.testing.assert_array_equal(lp, a["layer_ptr"])
    np.testing.assert_array_equal(lr, a["layer_rows"])
    if c["sched"] == "L":
        assert len(lp) - 1 > 1
    e, it, post, _ = oracle.decode_batch(c["algo"], H, a["syn"], c["p"], c["max_iter"], lp, lr)
    np.testing.assert_array_equal(it, a["iters"])
    np.testing.assert_array_equal(e, a["ehat"])
    np.testing.assert_array_equal(post.view(np.uint64), a["post"].view(np.uint64))
    if sid in ts.TALL:                                     # the recorded shots reach past the register
        assert a["syn"][:, REG:].any()


def test_golden_files_are_small():
    import os
    for sid in ts.GOLDEN_IDS:
        assert os.path.getsize(ts.golden_path(sid)) < 404 * 1024


# ---------------------------------------------------------------------------
# the NumPy models on these shapes
# ---------------------------------------------------------------------------
def test_models_run_in_seconds():
    """prior_model.decode and relay_model.decode on 32 shots of T2, as the
    GPU tests call them."""
    import prior_model as pm
    import relay_model as rm
    H, syn = ts.matrix("T2"), ts.model_batch("T2")
    n = H.shape[1]
    L = np.array([pm.llr(x) for x in ts.general_prior(n, 21)])
    assert (L < 0).sum() == 3 and (L != 0).all() and np.isfinite(L).all()
    t0 = time.perf_counter()
    e, it, post, _ = pm.decode("MS", pm.Graph(H), syn, np.broadcast_to(L, (len(syn), n)), ts.GPU_MAX_ITER)
    t1 = time.perf_counter()
    assert t1 - t0 < 10.0 and e.shape == (len(syn), n) and (it == ts.GPU_MAX_ITER).any() and (it < 5).any()
    gam = np.random.default_rng(7).uniform(-0.24, 0.66, (2, n))
    out = rm.decode(H, syn, ts.SHAPES["T2"]["p"], [8, 6], gam, 2)
    assert time.perf_counter() - t1 < 20.0 and out[0].shape == (len(syn), n)

"""GPU parity on the wide-column shapes of tests/wide_column_codes.py: BP's
variable node at every order np.sum adds a column in. Up to 128 entries on the
LDS kernels, the team kernels and the HBM-resident kernels; past 128 entries
(np.sum halves the column and recurses) on hbm_tile_kernel, the default route
of such a code, and on hbm_tile_vprior_kernel, at one to four levels, balanced
and not, flooding, layered (the lazy first iteration: entries not yet reached
read as 0.0) and on a schedule that is no partition (DESIGN.md sections 3.17
and 8).

Scalar priors compare with the C oracle, per-variable priors with
tests/wide_column_model.py; tests/test_wide_column_codes.py shows on the CPU
that the two agree, that every posterior of the references is finite and that
the old association (eight accumulators over the whole column) changes
posterior bits on every batch past 128. Every test asserts the kernel's name
first; iterations, estimates, posteriors as 64-bit patterns and the CONVERGED
flag compare for equality on every shot."""
import numpy as np
import pytest

import shape_codes as sc
import wide_column_codes as wc
import wide_column_model as wm
from test_gpu_shapes import _check, _np, dec  # noqa: F401  (dec: the fixture)

pytestmark = pytest.mark.gpu

MAX_ITER = wc.GPU_MAX_ITER


@pytest.fixture
def fresh(qopt):
    """qopt, with the shapes' cached schedules (and their launch plans)
    forgotten around the test: options change which kernel a plan holds."""
    from qldpcsim_amd import _lib
    handles = [_lib.code_for(wc.matrix(sid)) for sid in wc.IDS]
    for h in handles:
        h._sched.clear()
    yield qopt
    for h in handles:
        h._sched.clear()


def _packed(sid, sched):
    return sc.packed(wm.schedule_of(sid, sched), wc.matrix(sid).shape[0])


def _hbm(sid, algo, kernel="hbm_tile_kernel"):
    """The HBM instance by the widest row, as select_hbm_kernel picks it."""
    d = int(wc.matrix(sid).sum(1).max())
    return f"{kernel}<{0 if algo == 'MS' else 1}, {8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64}, 4>"


def _scalar(dec, sid, algo, sched, expect, exact=True):
    """Assert the kernel's name, decode the shape's batch with the scalar
    prior and compare with the oracle."""
    from qldpcsim_amd import _lib
    H, syn = wc.matrix(sid), wc.batch(sid)
    lp, lr = _packed(sid, sched)
    nm = _lib.kernel_name(H, lp, lr, algo)
    assert (nm == expect) if exact else nm.startswith(expect), f"{sid} {algo} {sched}: {nm}, expected {expect}"
    r = dec.decode_batch(H, syn, wc.SHAPES[sid]["p"], MAX_ITER, algo=algo, want_post=True, layer_ptr=lp,
                         layer_rows=lr)
    want = wm.want_scalar(algo, sid, sched)
    assert np.isfinite(want[2]).all()
    _check(algo, H, syn, r, want)


def _vprior(dec, sid, sched, expect):
    """The same with the shape's prior row, against decode_bp."""
    from qldpcsim_amd import _lib
    H, syn = wc.matrix(sid), wc.batch(sid)
    lp, lr = _packed(sid, sched)
    assert _lib.vprior_kernel_name(H, lp, lr, "BP") == expect
    r = dec.decode_batch(H, syn, None, MAX_ITER, algo="BP", want_post=True, layer_ptr=lp, layer_rows=lr,
                         prior=np.array(wc.prior_row(sid)))
    want = wm.want_vprior(sid, sched)
    assert np.isfinite(want[2]).all() and (want[1] < MAX_ITER).any() and (want[1] == MAX_ITER).any()
    _check("BP", H, syn, r, want)


# ---------------------------------------------------------------------------
# scalar BP
# ---------------------------------------------------------------------------
def _default_bp_name(sid, sched):
    """W0: the generic LDS kernel (rows of several degrees); U8: the team
    kernels, all-LDS when layered (column degree > 31 leaves no global layer
    image); W1 - W4: a column past 128 entries, hbm_tile_kernel<1, D, 4>."""
    lay = "false" if sched == "F" else "true"
    if sid == "W0":
        return f"decode_kernel<1, {lay}, 0>", True
    if sid == "U8":
        return f"bp_team_kernel<{lay}, 8,", False
    return _hbm(sid, "BP"), True


DEFAULT = [(sid, sched) for sid in wc.IDS for sched in ("F", "L", "S5")]


@pytest.mark.parametrize("sid,sched", DEFAULT, ids=[f"{s}-{k}" for s, k in DEFAULT])
def test_scalar_bp_default_route(dec, sid, sched):
    """Flooding, schedule.layerize and five strided layers. On W1 - W4 this
    is the decode that kept the eight accumulators over the whole column."""
    expect, exact = _default_bp_name(sid, sched)
    if sid == "W4":
        assert expect == "hbm_tile_kernel<1, 64, 4>"
    _scalar(dec, sid, "BP", sched, expect, exact)


@pytest.mark.parametrize("sched", ["F", "S5"])
@pytest.mark.parametrize("sid", ["W0", "U8"])
def test_scalar_bp_forced_hbm(dec, sid, sched, fresh):
    """hbm_tile_kernel's forms up to 128 entries: columns of 7 .. 128 (W0) and
    of 64, 127, 128 (U8)."""
    fresh(force_hbm=1)
    _scalar(dec, sid, "BP", sched, _hbm(sid, "BP"))


@pytest.mark.parametrize("sched", ["F", "S5"])
@pytest.mark.parametrize("opt", ["bp_wave", "w4", "w8"])
def test_u8_team_options(dec, opt, sched, fresh):
    """U8 under bp_wave (decode_kernel<1, ., 8>) and at the forced team widths."""
    lay = "false" if sched == "F" else "true"
    if opt == "bp_wave":
        fresh(bp_wave=1)
        expect = f"decode_kernel<1, {lay}, 8>"
    else:
        fresh(bp_team_w=int(opt[1]))
        expect = f"bp_team_kernel<{lay}, 8, {opt[1]}>"
    _scalar(dec, "U8", "BP", sched, expect)


def test_non_partition_schedule_on_w2(dec):
    """Row 5 in two layers, row 10 in none: the HBM kernel initialises its
    state (lazy = 0) and sums columns of 136 .. 513 entries."""
    _scalar(dec, "W2", "BP", "NP", _hbm("W2", "BP"))


# ---------------------------------------------------------------------------
# per-variable priors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("sched", ["F", "S5"])
def test_vprior_w0_on_the_lds_twin_and_forced(dec, sched, fresh):
    _vprior(dec, "W0", sched, f"decode_vprior_kernel<1, {'false' if sched == 'F' else 'true'}, 0>")
    fresh(force_hbm=1, vprior_hbm=1)
    _vprior(dec, "W0", sched, _hbm("W0", "BP", "hbm_tile_vprior_kernel"))


@pytest.mark.parametrize("sched", ["F", "S5"])
@pytest.mark.parametrize("sid", ["W1", "W2", "W3"])
def test_vprior_past_128_entries(dec, sid, sched, fresh):
    """Refused without option vprior_hbm; with it np_pairwise_deep at one
    level (W1), at two and three levels and unbalanced (W2), at four (W3)."""
    H = wc.matrix(sid)
    lp, lr = _packed(sid, sched)
    with pytest.raises(NotImplementedError, match=f"BP column degree {max(wc.heavy_degrees(sid))} > 128"):
        dec.decode_batch(H, wc.batch(sid)[:1], None, MAX_ITER, algo="BP", layer_ptr=lp, layer_rows=lr,
                         prior=np.array(wc.prior_row(sid)))
    fresh(vprior_hbm=1)
    _vprior(dec, sid, sched, _hbm(sid, "BP", "hbm_tile_vprior_kernel"))


def test_two_level_twin_refuses_w1(dec, fresh):
    H = wc.matrix("W1")
    mask = np.zeros((1, H.shape[1]), np.uint8)
    for opts in ({}, dict(vprior_hbm=1)):
        fresh(**opts)
        with pytest.raises(NotImplementedError, match="two-level priors: BP column degree 129 > 128"):
            dec.decode_batch(H, wc.batch("W1")[:1], 0.01, MAX_ITER, algo="BP", prior_mask=mask, p_masked=0.2)


# ---------------------------------------------------------------------------
# min-sum controls: float32 sums of 513 and 1025 terms in sequence
# ---------------------------------------------------------------------------
MIN_SUM = [("W2", "F"), ("W2", "L"), ("W3", "F"), ("W3", "S5"), ("W3", "L")]


@pytest.mark.parametrize("sid,sched", MIN_SUM, ids=[f"{s}-{k}" for s, k in MIN_SUM])
def test_min_sum_default_route(dec, sid, sched):
    """decode_kernel<0, ., 0>: column degrees past the chunk_dmax clamp of
    255. (schedule.layerize cuts W3 into more than a thousand layers, whose
    tables the LDS does not hold: that decode takes the HBM kernel.)"""
    if (sid, sched) == ("W3", "L"):
        assert len(wc.layerized("W3")) > 1000
        return _scalar(dec, sid, "MS", sched, _hbm(sid, "MS"))
    _scalar(dec, sid, "MS", sched, f"decode_kernel<0, {'false' if sched == 'F' else 'true'}, 0>")


@pytest.mark.parametrize("sid", ["W2", "W3"])
def test_min_sum_forced_hbm(dec, sid, fresh):
    fresh(force_hbm=1)
    _scalar(dec, sid, "MS", "F", _hbm(sid, "MS"))


@pytest.mark.parametrize("sid", ["W2", "W3"])
def test_relay_one_leg_without_memory_is_min_sum(dec, sid):
    """Relay min-sum with one leg and gamma = 0 is algo="MS", bit for bit."""
    import torch
    H = wc.matrix(sid)
    syn = torch.as_tensor(np.array(wc.batch(sid)), device="cuda:0")      # (a copy: the batch is read-only)
    e, it, post, _ = wm.want_scalar("MS", sid, "F")
    r = dec.decode_batch(H, syn, wc.SHAPES[sid]["p"], 0, algo="RELAY", want_post=True,
                         relay=dec.RelayConfig([MAX_ITER], np.zeros((1, H.shape[1])), 1))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(r.iters), it)
    np.testing.assert_array_equal(_np(r.ehat), e)
    np.testing.assert_array_equal(_np(r.post).view(np.uint64), post.view(np.uint64))

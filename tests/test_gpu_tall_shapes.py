"""GPU parity on the tall shapes of tests/tall_shape_codes.py: the generic LDS
kernel body (decode_kernel, decode_prior_kernel, decode_vprior_kernel and their
*_tall instances) past the 2048 checks its flooding branch holds in a register,
and at the fast table's
16-bit limit, bit for bit against the CPU oracle and the test-side NumPy
models. The layered branch, the relay kernels, the hard-decision kernels and
the HBM-resident kernel keep syndrome bits elsewhere and decode the same
shapes as controls.

Every test first asserts the kernel's name, so the shape provably runs the
kernel it was built for; no comparison has a tolerance and no shot is left
out. tests/test_tall_shape_codes.py asserts, on the oracle alone, that the
batches fire the checks past the register and mix decode lengths."""
import functools

import numpy as np
import pytest

import hard_model as hm
import prior_model as pm
import relay_model as rm
import relay_vprior_model as vm
import shape_codes as sc
import tall_shape_codes as ts
from test_gpu_relay import _same as _relay_same
from test_gpu_shapes import _check, _decode, _np, dec  # noqa: F401  (dec: the fixture)

pytestmark = pytest.mark.gpu

MAX_ITER = ts.GPU_MAX_ITER
A = {"MS": 0, "BP": 1}


@pytest.fixture
def fresh(qopt):
    """qopt, with the tall shapes' cached schedules (and their launch plans)
    forgotten around the test: options change which kernel a plan holds."""
    from qldpcsim_amd import _lib
    handles = [_lib.code_for(ts.matrix(sid)) for sid in ts.IDS]
    for h in handles:
        h._sched.clear()
    yield qopt
    for h in handles:
        h._sched.clear()


@functools.lru_cache(maxsize=None)
def _want(algo, sid, layered):
    """The oracle on the shape's full batch, computed once and shared read-only."""
    from oracle import oracle
    lp, lr = ts.packed(sid, layered)
    out = oracle.decode_batch(algo, ts.matrix(sid), ts.batch(sid), ts.SHAPES[sid]["p"], MAX_ITER, lp, lr)
    for a in out:
        a.setflags(write=False)
    return out


def _generic(algo, layered, dc, kernel="decode_kernel"):
    return f"{kernel}<{A[algo]}, {'true' if layered else 'false'}, {dc}>"


def _flood(sid, algo, kernel="decode_kernel"):
    """The flooding instance of one of the three generic kernels on a tall
    shape: past the register's 2048 checks its *_tall kernel, else <., false, 0>."""
    return f"{kernel}_tall<{A[algo]}>" if sid in ts.TALL else _generic(algo, False, 0, kernel)


def _scalar(dec, algo, sid, layered, expect, B=None, bits=False, exact=True):
    """Assert the kernel's name, decode the first B shots (all: the hand-made
    pair included) and compare with the oracle."""
    from qldpcsim_amd import _lib
    H = ts.matrix(sid)
    lp, lr = ts.packed(sid, layered)
    nm = _lib.kernel_name(H, lp, lr, algo)
    assert (nm == expect) if exact else nm.startswith(expect), f"{sid} {algo}: {nm}, expected {expect}"
    syn = ts.batch(sid)[:B]
    r, e = _decode(dec, H, syn, ts.SHAPES[sid]["p"], algo, lp, lr, bits=bits)
    _check(algo, H, syn, r, _want(algo, sid, layered), ehat=e)


# ---------------------------------------------------------------------------
# scalar priors, against the oracle
# ---------------------------------------------------------------------------
def _flooding_name(sid, algo):
    """T0, U1: the DC = 0 instances; T1 - T3: decode_kernel_tall. U0 (DC = 8):
    no flood image at m > 512, so min-sum takes decode_kernel<0, false, 8>; BP
    its team kernel."""
    if sid == "U0":
        return ("bp_team_kernel<false, 8,", False) if algo == "BP" else (_generic(algo, False, 8), True)
    assert ts.dc_of(sid) == 0
    return _flood(sid, algo), True


@pytest.mark.parametrize("B", [1, None], ids=["B1", "full"])
@pytest.mark.parametrize("fmt", ["bytes", "bits"])
@pytest.mark.parametrize("algo", ["MS", "BP"])
@pytest.mark.parametrize("sid", ts.IDS)
def test_flooding(dec, sid, algo, fmt, B):
    expect, exact = _flooding_name(sid, algo)
    _scalar(dec, algo, sid, False, expect, B=B, bits=fmt == "bits", exact=exact)


@pytest.mark.parametrize("algo", ["MS", "BP"])
@pytest.mark.parametrize("sid", ["T2", "U1"])
def test_layered(dec, sid, algo):
    """schedule.layerize's layers: the branch of the body that keeps the
    syndrome in the slice's words (control)."""
    _scalar(dec, algo, sid, True, _generic(algo, True, 0))


@pytest.mark.parametrize("algo", ["MS", "BP"])
@pytest.mark.parametrize("sid", ["T2", "T3"])
def test_hbm_kernel(dec, sid, algo, fresh):
    """hbm_tile_kernel has no such register: the inputs are sound whatever
    the LDS kernels do with them (control)."""
    fresh(force_hbm=1)
    _scalar(dec, algo, sid, False, f"hbm_tile_kernel<{A[algo]}, 8, 4>")


@pytest.mark.parametrize("algo", ["MS", "BP"])
def test_dc8_instances_at_their_largest_row_table(dec, algo, fresh):
    """U0 under flood_generic and bp_wave: decode_kernel<., false, 8> with
    8 * E = 65472, the last row table whose byte offsets fit 16 bits."""
    fresh(flood_generic=1, bp_wave=1)
    _scalar(dec, algo, "U0", False, _generic(algo, False, 8))


# ---------------------------------------------------------------------------
# per-variable priors
# ---------------------------------------------------------------------------
def _model_check(algo, H, syn, r, want):
    """Result `r` against a NumPy model's (ehat, iters, post, flags): every
    output, posteriors as bit patterns (non-finite ones, BP's alone, in the
    same places with the same value; a NaN's payload is the platform's)."""
    from qldpcsim_amd import _lib
    e, it, post, fl = want
    got_e, got_post, flags = _np(r.ehat), _np(r.post), _np(r.flags)
    np.testing.assert_array_equal(_np(r.iters), it)
    np.testing.assert_array_equal(got_e, e)
    finite = np.isfinite(post)
    assert finite.all() or algo == "BP"
    np.testing.assert_array_equal(np.isfinite(got_post), finite)
    np.testing.assert_array_equal(got_post[~finite], post[~finite])
    np.testing.assert_array_equal(got_post[finite].view(np.uint64), post[finite].view(np.uint64))
    keep = pm.FLAG_CONVERGED | (pm.FLAG_MIN_ZERO if algo == "MS" else 0)
    np.testing.assert_array_equal(flags & keep, fl & keep)
    sat = ((got_e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(1)
    np.testing.assert_array_equal((flags & _lib.FLAG_CONVERGED) != 0, sat)


@functools.lru_cache(maxsize=None)
def _prior_row(n):
    q = ts.general_prior(n, 21)
    L = np.array([pm.llr(x) for x in q])
    assert (L < 0).sum() == 3 and (L != 0).all() and np.isfinite(L).all()
    q.setflags(write=False)
    L.setflags(write=False)
    return q, L


def _vprior_against_model(dec, H, syn, algo, layers, expect):
    from qldpcsim_amd import _lib
    m, n = H.shape
    lp, lr = sc.packed(layers, m)
    assert _lib.vprior_kernel_name(H, lp, lr, algo) == expect
    q, L = _prior_row(n)
    want = pm.decode(algo, H, syn, np.broadcast_to(L, (len(syn), n)), MAX_ITER, layers)
    assert (want[1] == MAX_ITER).any() and (want[1] < MAX_ITER).any()
    r, _ = _decode(dec, H, syn, None, algo, lp, lr, prior=q)
    _model_check(algo, H, syn, r, want)


VPRIOR = [(sid, algo, lay) for sid in ("T2", "U1") for algo, lay in (("MS", False), ("BP", False), ("MS", True))]


@pytest.mark.parametrize("sid,algo,layered", VPRIOR, ids=[f"{s}-{a}-{'L' if l else 'F'}" for s, a, l in VPRIOR])
def test_vprior_general_vector_against_the_model(dec, sid, algo, layered):
    """decode_vprior_kernel<., ., 0> (T2 flooding: decode_vprior_kernel_tall)
    with a log-uniform prior row in [1e-4, 0.3] and three entries above 0.5,
    against prior_model.decode."""
    expect = _generic(algo, True, 0, "decode_vprior_kernel") if layered else _flood(sid, algo, "decode_vprior_kernel")
    _vprior_against_model(dec, ts.matrix(sid), ts.model_batch(sid), algo, ts.layerized(sid) if layered else None,
                          expect)


UNIFORM = [(sid, algo) for sid in ("T0",) + ts.TALL for algo in ("MS", "BP") if (sid, algo) != ("T3", "BP")]


@pytest.mark.parametrize("sid,algo", UNIFORM, ids=[f"{s}-{a}" for s, a in UNIFORM])
def test_vprior_uniform_vector_equals_the_scalar_decode(dec, sid, algo):
    """prior = [p] * n through decode_vprior_kernel_tall (T0, at the register's
    last size: decode_vprior_kernel<., false, 0>) is the scalar decode (the
    oracle's) bit for bit. (T3 with BP: the prior row leaves no room for a
    wave's float64 state, see test_vprior_t3_bp_does_not_fit.)"""
    from qldpcsim_amd import _lib
    H, syn, p = ts.matrix(sid), ts.batch(sid), ts.SHAPES[sid]["p"]
    lp, lr = ts.packed(sid, False)
    assert _lib.vprior_kernel_name(H, lp, lr, algo) == _flood(sid, algo, "decode_vprior_kernel")
    r, _ = _decode(dec, H, syn, None, algo, lp, lr, prior=np.full(H.shape[1], p))
    _check(algo, H, syn, r, _want(algo, sid, False))


def test_vprior_t3_bp_does_not_fit(dec):
    """T3's tables (57 KB), prior row (33 KB) and one BP wave (99 KB) exceed
    the 160 KB of LDS: the decode is refused, not sent elsewhere."""
    H = ts.matrix("T3")
    lp, lr = ts.packed("T3", False)
    with pytest.raises(NotImplementedError, match="do not fit"):
        _decode(dec, H, ts.batch("T3")[:1], None, "BP", lp, lr, prior=np.full(H.shape[1], 0.01))


# ---------------------------------------------------------------------------
# two-level priors
# ---------------------------------------------------------------------------
PRIOR_EQ = [(sid, algo) for sid in ("T0",) + ts.TALL for algo in ("MS", "BP")]


@pytest.mark.parametrize("sid,algo", PRIOR_EQ, ids=[f"{s}-{a}" for s, a in PRIOR_EQ])
def test_prior_twin_with_equal_priors(dec, sid, algo):
    """decode_prior_kernel_tall (T0: decode_prior_kernel<., false, 0>) with
    p_masked == p is the scalar decode (the oracle's) whatever the masks hold."""
    from qldpcsim_amd import _lib
    H, syn, p = ts.matrix(sid), ts.batch(sid), ts.SHAPES[sid]["p"]
    lp, lr = ts.packed(sid, False)
    assert _lib.prior_kernel_name(H, lp, lr, algo) == _flood(sid, algo, "decode_prior_kernel")
    mask = np.random.default_rng(5).integers(0, 2, (len(syn), H.shape[1]), dtype=np.uint8)
    r, _ = _decode(dec, H, syn, p, algo, lp, lr, prior_mask=mask, p_masked=p)
    _check(algo, H, syn, r, _want(algo, sid, False))


@pytest.mark.parametrize("algo", ["MS", "BP"])
def test_two_level_rows_equal_the_per_variable_decode(dec, algo):
    """T2, a random 30 % mask per shot, p = 0.01 / p_masked = 0.2: each shot of
    decode_prior_kernel_tall equals decode_vprior_kernel_tall's decode of that
    syndrome with the mask row's indicator vector (itself compared with the
    model above)."""
    from qldpcsim_amd import _lib
    H, syn = ts.matrix("T2"), ts.model_batch("T2")
    n = H.shape[1]
    lp, lr = ts.packed("T2", False)
    assert _lib.prior_kernel_name(H, lp, lr, algo) == _flood("T2", algo, "decode_prior_kernel")
    p0, p1 = 0.01, 0.2
    mask = (np.random.default_rng(31).random((len(syn), n)) < 0.3).astype(np.uint8)
    two, _ = _decode(dec, H, syn, p0, algo, lp, lr, prior_mask=mask, p_masked=p1)
    cols = [_np(x) for x in (two.ehat, two.iters, two.post, two.flags)]
    assert (cols[1] == MAX_ITER).any() and (cols[1] < MAX_ITER).any()
    for b in range(len(syn)):
        one, _ = _decode(dec, H, syn[b:b + 1], None, algo, lp, lr, prior=np.where(mask[b] != 0, p1, p0))
        for got, ref in zip(cols, (one.ehat, one.iters, one.post, one.flags)):
            ref = _np(ref)
            if ref.dtype == np.float64:
                nan = np.isnan(ref[0])
                np.testing.assert_array_equal(np.isnan(got[b]), nan)
                np.testing.assert_array_equal(got[b][~nan].view(np.uint64), ref[0][~nan].view(np.uint64))
            else:
                np.testing.assert_array_equal(got[b], ref[0], err_msg=f"shot {b}")


# ---------------------------------------------------------------------------
# the per-variable-prior twin on the shapes of tests/shape_codes.py
# ---------------------------------------------------------------------------
OLD = [(sid, part) for sid in "ABEF" for part in (None, sc.GOLDEN_PARTITION[sid])]


@pytest.mark.parametrize("sid,part", OLD, ids=[f"{s}-{p or 'flooding'}" for s, p in OLD])
def test_vprior_on_the_synthetic_shapes(dec, sid, part):
    """decode_vprior_kernel<0, ., 8 | 7> against prior_model.decode on shapes
    A (a zero column), B (column degree 32), E (ten degree runs, column degree
    36) and F (n > 2048): min-sum, flooding and the golden partition."""
    H = sc.matrix(sid)
    layers = None if part is None else sc.partitions(sid)[part]
    _vprior_against_model(dec, H, sc.batch(sid)[:ts.MODEL_SHOTS], "MS", layers,
                          _generic("MS", part is not None, sc.SHAPES[sid]["dc"], "decode_vprior_kernel"))


# ---------------------------------------------------------------------------
# relay and hard-decision kernels (controls: syndrome bits in the slice's words)
# ---------------------------------------------------------------------------
RELAY_T = (8, 6)


def _relay_inputs(sid):
    from qldpcsim_amd import decoders
    H = ts.matrix(sid)
    return H, ts.model_batch(sid), list(RELAY_T), decoders.relay_gammas(H.shape[1], len(RELAY_T), seed=7)


@pytest.mark.parametrize("sid,kernel", [("T2", "relay_ms_kernel<0>"), ("U0", "relay_ms_kernel<8>"),
                                        ("U1", "relay_ms_kernel<0>")])
def test_relay_against_the_model(sid, kernel):
    """Two legs, sols = 2: relay_ms_kernel<0> past 2048 checks and at uniform
    degree 8 without the fast table, <8> at its largest row table."""
    import torch
    from qldpcsim_amd import _lib, decoders
    H, syn, T, G = _relay_inputs(sid)
    p = ts.SHAPES[sid]["p"]
    assert _lib.code_for(H, 0).relay(T, G, 2).kernel_name() == kernel
    want = rm.decode(H, syn, p, T, G, 2)
    assert len(np.unique(want[4])) >= 2                      # shots with and without a solution
    r = decoders.decode_batch(H, torch.as_tensor(np.array(syn), device="cuda:0"), p, 0, algo="RELAY",
                              relay=decoders.RelayConfig(T, G, 2), want_post=True)
    torch.cuda.synchronize()
    _relay_same(r, want, H.shape[1])


@pytest.mark.parametrize("cost", ["hamming", "prior"])
def test_relay_vprior_against_the_model(cost):
    import torch
    from qldpcsim_amd import _lib, decoders
    H, syn, T, G = _relay_inputs("T2")
    q, _ = _prior_row(H.shape[1])
    assert _lib.code_for(H, 0).relay(T, G, 2, prior=q).kernel_name() == "relay_vprior_kernel<0>"
    want = vm.decode(H, syn, q, T, G, 2, cost)
    assert len(np.unique(want[4])) >= 2
    r = decoders.decode_batch(H, torch.as_tensor(np.array(syn), device="cuda:0"), None, 0, algo="RELAY",
                              relay=decoders.RelayConfig(T, G, 2, prior=q, cost=cost), want_post=True)
    torch.cuda.synchronize()
    _relay_same(r, want, H.shape[1])


@pytest.mark.parametrize("algo,kernel", [("BF", "bf_kernel"), ("NG", "ng_kernel")])
def test_hard_decoders_against_the_model(algo, kernel):
    from qldpcsim_amd import _lib, decoders
    H, syn = ts.matrix("T2"), ts.model_batch("T2")
    assert _lib.kernel_name(H, None, None, algo, 0) == kernel
    if algo == "BF":
        e, it, conv = hm.bf_batch(H, syn, 50)
    else:
        e, it, info = hm.ng_batch(H, syn)
        conv = info["conv"]
    r = decoders.decode_batch(H, syn, 0.0, 50, algo=algo)
    np.testing.assert_array_equal(r.iters, it)
    np.testing.assert_array_equal(r.converged, conv)
    np.testing.assert_array_equal(r.ehat, e)

"""GPU parity on the synthetic shapes of tests/shape_codes.py: every kernel
instance, host decision and branch that no bundled code selects (DESIGN.md
section 8), bit for bit against the CPU oracle on the same syndromes — the
oracle itself is pinned to the reference's recorded outputs on these shapes by
tests/test_shape_codes.py, which also asserts that each batch here mixes short
and full-length decodes.

Every test first asserts the kernel's name, so the shape provably reaches the
kernel it was built for; no comparison has a tolerance."""
import functools

import numpy as np
import pytest

import shape_codes as sc

pytestmark = pytest.mark.gpu

MAX_ITER = sc.GPU_MAX_ITER


@pytest.fixture(scope="module")
def dec():
    from qldpcsim_amd import _lib, decoders
    if _lib.device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X box")
    return decoders


def _layers(sid, name):
    return sc.packed(None if name is None else sc.partitions(sid)[name], sc.SHAPES[sid]["m"])


@functools.lru_cache(maxsize=None)
def _want(algo, sid, name, p=None):
    """The oracle on the shape's full batch, computed once per (algo, shape,
    schedule, prior) and shared read-only: (ehat, iters, post, flags)."""
    from oracle import oracle
    H = sc.matrix(sid)
    lp, lr = _layers(sid, name)
    out = oracle.decode_batch(algo, H, sc.batch(sid), sc.SHAPES[sid]["p"] if p is None else p, MAX_ITER, lp, lr)
    for a in out:
        a.setflags(write=False)
    return out


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def _check(algo, H, syn, r, want, ehat=None, min_zero=True):
    """iters, hard decisions, posteriors as uint64, the min-sum zero-message
    flag and FLAG_CONVERGED of result `r` against the oracle's `want` on the
    leading len(syn) shots."""
    from qldpcsim_amd import _lib
    B = len(syn)
    e, it, post, fl = (a[:B] for a in want)
    got_e = _np(r.ehat) if ehat is None else ehat
    got_post, flags = _np(r.post), _np(r.flags)
    np.testing.assert_array_equal(_np(r.iters), it)
    np.testing.assert_array_equal(got_e, e)
    finite = np.isfinite(post)
    np.testing.assert_array_equal(np.isfinite(got_post), finite)   # non-finite only where the oracle's are
    if finite.all():
        np.testing.assert_array_equal(got_post.view(np.uint64), post.view(np.uint64))
    else:                                                          # NaN payloads are the platform's
        np.testing.assert_array_equal(got_post, post)
        np.testing.assert_array_equal(got_post[finite].view(np.uint64), post[finite].view(np.uint64))
    if algo == "MS" and min_zero:
        np.testing.assert_array_equal((flags & _lib.FLAG_MIN_ZERO) != 0, (fl & 1) != 0)
    sat = ((got_e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(1)
    np.testing.assert_array_equal((flags & _lib.FLAG_CONVERGED) != 0, sat)


def _decode(dec, H, syn, p, algo, lp, lr, bits=False, **kw):
    """decode_batch with posteriors: host byte syndromes, or (bits) device
    bit-packed syndromes and estimates; returns (result, ehat uint8 [B, n])."""
    if not bits:
        r = dec.decode_batch(H, syn, p, MAX_ITER, algo=algo, want_post=True, layer_ptr=lp, layer_rows=lr, **kw)
        return r, _np(r.ehat)
    import torch
    words = dec.pack_bits(torch.as_tensor(np.array(syn), device="cuda"))      # (a copy: the batch is read-only)
    r = dec.decode_batch(H, words, p, MAX_ITER, algo=algo, want_post=True, layer_ptr=lp, layer_rows=lr,
                         ehat_bits=True, **kw)
    torch.cuda.synchronize()
    return r, dec.unpack_bits(r.ehat, H.shape[1]).cpu().numpy()


def _run(dec, algo, sid, name, expect, B=None, bits=False, p=None, exact=True):
    """Assert the kernel's name, decode the first B shots of the shape's batch
    and compare with the oracle."""
    from qldpcsim_amd import _lib
    H = sc.matrix(sid)
    lp, lr = _layers(sid, name)
    nm = _lib.kernel_name(H, lp, lr, algo)
    assert (nm == expect) if exact else nm.startswith(expect), f"{sid} {algo} {name}: {nm}, expected {expect}"
    syn = sc.batch(sid)[:B]
    r, e = _decode(dec, H, syn, sc.SHAPES[sid]["p"] if p is None else p, algo, lp, lr, bits=bits)
    _check(algo, H, syn, r, _want(algo, sid, name, p), ehat=e)


@pytest.fixture
def fresh_schedules():
    """Forget the shapes' cached schedules around a test that changes how
    plans are chosen (as test_ms_layered_kernels_match_oracle does)."""
    from qldpcsim_amd import _lib
    handles = [_lib.code_for(sc.matrix(sid)) for sid in sc.IDS]
    for h in handles:
        h._sched.clear()
    yield
    for h in handles:
        h._sched.clear()


# ---------------------------------------------------------------------------
# flooding min-sum
# ---------------------------------------------------------------------------
FLOOD_MS = dict(A="ms_flood_kernel<8, 2>", B="ms_flood_kernel<7, 4>", C="ms_flood_kernel<7, 8>",
                D="ms_flood_kernel<8, 8>", G="ms_flood_kernel<8, 2>", H="ms_flood_kernel<7, 2>",
                E="decode_kernel<0, false, 8>", F="decode_kernel<0, false, 8>")


@pytest.mark.parametrize("B", [1, 3, None], ids=["B1", "B3", "full"])
@pytest.mark.parametrize("fmt", ["bytes", "bits"])
@pytest.mark.parametrize("sid", sc.IDS)
def test_flooding_ms(dec, sid, fmt, B):
    _run(dec, "MS", sid, None, FLOOD_MS[sid], B=B, bits=fmt == "bits")


@pytest.mark.parametrize("sid", list("ABCD"))
def test_flooding_ms_generic_kernel(dec, sid, qopt, fresh_schedules):
    """Option flood_generic: the generic kernel at DC = 7 / 8 on the shapes
    that have a flood image."""
    qopt(flood_generic=1)
    _run(dec, "MS", sid, None, f"decode_kernel<0, false, {sc.SHAPES[sid]['dc']}>")


@pytest.mark.parametrize("sid", ["A", "D"])
def test_flooding_ms_zero_prior(dec, sid):
    """p = 0.5: every message is zero and every half-shot is flagged
    FLAG_MIN_ZERO, exactly as the oracle flags it (pad checks included: D)."""
    want = _want("MS", sid, None, 0.5)
    assert (want[3] & 1).all()
    _run(dec, "MS", sid, None, FLOOD_MS[sid], p=0.5)


# ---------------------------------------------------------------------------
# layered and serial min-sum
# ---------------------------------------------------------------------------
def _layered_ms_name(sid, name):
    dc = sc.SHAPES[sid]["dc"]
    if sid in "BEF":                                      # no layered_ms image: column degree > 31 or n > 2048
        return f"decode_kernel<0, true, {dc}>"
    return f"ms_layered_kernel<{dc}, {sc.uniform_lanes(sc.matrix(sid), sc.partitions(sid)[name])}>"


LAYERED = [(sid, name) for sid in sc.IDS for name in sc.partitions(sid)]


@pytest.mark.parametrize("sid,name", LAYERED, ids=[f"{s}-{n}" for s, n in LAYERED])
def test_layered_ms(dec, sid, name):
    _run(dec, "MS", sid, name, _layered_ms_name(sid, name))


@pytest.mark.parametrize("lanes", [1, 2, 4, 8])
@pytest.mark.parametrize("sid", ["C", "D"])
def test_layered_ms_forced_lanes(dec, sid, lanes, qopt, fresh_schedules):
    """ms_layered_kernel at every forced lanes-per-check width over layers of
    1 .. 149 rows (the pair path's 32 / 33, one or two trips at 64 / 65)."""
    qopt(ms_lanes_per_check=lanes)
    _run(dec, "MS", sid, "cut", f"ms_layered_kernel<{sc.SHAPES[sid]['dc']}, {lanes}>")


# ---------------------------------------------------------------------------
# BP
# ---------------------------------------------------------------------------
BP_WIDTHS = [(sid, w) for sid in sc.IDS for w in ((0, 4, 8) if sid in "ABCD" else (0,))]


@pytest.mark.parametrize("sid,w", BP_WIDTHS, ids=[f"{s}-w{w}" for s, w in BP_WIDTHS])
def test_flooding_bp(dec, sid, w, qopt, fresh_schedules):
    dc = sc.SHAPES[sid]["dc"]
    if w:
        qopt(bp_team_w=w)
    _run(dec, "BP", sid, None, f"bp_team_kernel<false, {dc}, {w}>" if w else f"bp_team_kernel<false, {dc},",
         exact=bool(w))


LAYERED_BP = [(sid, name, w) for sid, name in LAYERED if name != "serial"
              for w in ((0, 4, 8) if sid in "ABCD" else (0,))]


@pytest.mark.parametrize("sid,name,w", LAYERED_BP, ids=[f"{s}-{n}-w{w}" for s, n, w in LAYERED_BP])
def test_layered_bp(dec, sid, name, w, qopt, fresh_schedules):
    """bp_team_lg_kernel where the schedule has the global layer image, the
    all-LDS bp_team_kernel<true, ..> where the code leaves none (B, E, F: no
    option set)."""
    dc = sc.SHAPES[sid]["dc"]
    if w:
        qopt(bp_team_w=w)
    if sid in "BEF":
        expect, exact = (f"bp_team_kernel<true, {dc}, {w}>", True) if w else (f"bp_team_kernel<true, {dc},", False)
    else:
        expect, exact = f"bp_team_lg_kernel<{dc}, {w or 4}>", True
    _run(dec, "BP", sid, name, expect, exact=exact)


# ---------------------------------------------------------------------------
# the reference's recorded outputs on the device
# ---------------------------------------------------------------------------
GOLDEN_CASES = [(sid, i) for sid in sc.IDS for i in range(len(sc.golden(sid)[1]))]


@pytest.mark.parametrize("sid,i", GOLDEN_CASES,
                         ids=[f"{s}-{sc.golden(s)[1][i][0]['algo']}-{sc.golden(s)[1][i][0]['sched']}"
                              for s, i in GOLDEN_CASES])
def test_reference_golden_on_device(dec, sid, i):
    H = sc.matrix(sid)
    c, a = sc.golden(sid)[1][i]
    r = dec.decode_batch(H, a["syn"], c["p"], c["max_iter"], algo=c["algo"], want_post=True,
                         layer_ptr=a["layer_ptr"], layer_rows=a["layer_rows"])
    k = len(a["post"])
    np.testing.assert_array_equal(r.iters, a["iters"])
    np.testing.assert_array_equal(r.ehat, a["ehat"])
    np.testing.assert_array_equal(r.post[:k].view(np.uint64), a["post"].view(np.uint64))


# ---------------------------------------------------------------------------
# twins, relay and the HBM-resident kernel
# ---------------------------------------------------------------------------
TWINS = [(sid, algo, name) for sid in "ADE" for algo in ("MS", "BP") for name in (None, sc.GOLDEN_PARTITION[sid])]


@pytest.mark.parametrize("sid,algo,name", TWINS, ids=[f"{s}-{a}-{n or 'flooding'}" for s, a, n in TWINS])
def test_prior_twins_with_equal_priors(dec, sid, algo, name):
    """decode_prior_kernel with p_masked == p and decode_vprior_kernel with a
    uniform vector give the scalar decode's result (the oracle's) bit for bit."""
    H = sc.matrix(sid)
    lp, lr = _layers(sid, name)
    syn, p, want = sc.batch(sid), sc.SHAPES[sid]["p"], _want(algo, sid, name)
    mask = np.random.default_rng(5).integers(0, 2, (len(syn), H.shape[1]), dtype=np.uint8)
    r, _ = _decode(dec, H, syn, p, algo, lp, lr, prior_mask=mask, p_masked=p)
    _check(algo, H, syn, r, want)
    r, _ = _decode(dec, H, syn, None, algo, lp, lr, prior=np.full(H.shape[1], p))
    _check(algo, H, syn, r, want)


@pytest.mark.parametrize("sid", list("ADE"))
def test_relay_one_leg_no_memory(dec, sid):
    """Relay min-sum with one leg and gamma = 0 is flooding min-sum (its
    MIN_ZERO flag may differ: no check pass runs after a solution)."""
    H = sc.matrix(sid)
    syn, p = sc.batch(sid), sc.SHAPES[sid]["p"]
    r = dec.decode_batch(H, syn, p, 0, algo="RELAY", want_post=True,
                         relay=dec.RelayConfig([MAX_ITER], np.zeros((1, H.shape[1])), 1))
    _check("MS", H, syn, r, _want("MS", sid, None), min_zero=False)


HBM = [(sid, algo, name) for sid in "AD" for algo in ("MS", "BP") for name in (None, sc.GOLDEN_PARTITION[sid])]


@pytest.mark.parametrize("sid,algo,name", HBM, ids=[f"{s}-{a}-{n or 'flooding'}" for s, a, n in HBM])
def test_hbm_kernel(dec, sid, algo, name, qopt, fresh_schedules):
    qopt(force_hbm=1)
    _run(dec, algo, sid, name, f"hbm_tile_kernel<{0 if algo == 'MS' else 1}, 8, 4>")

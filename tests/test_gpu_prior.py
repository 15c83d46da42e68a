"""decode_prior_kernel (two-level priors per half-shot) and simulate_p's
correlated X/Z mode on the GPU: against the scalar decode where the two priors
are equal, against the test-side NumPy model (tests/prior_model.py) where they
differ, and the simulator's counters against the host path, the model and the
uncorrelated run."""
import numpy as np
import pytest

import logical_model
import prior_model as pm
from qldpcsim_amd import _lib, codes, decoders, simulator

pytestmark = pytest.mark.gpu

GENERIC = dict(flood_generic=1, layered_generic=1, bp_wave=1)
_CACHE = {}


def _code(name):
    """steane: non-uniform degrees, n = 7; LP04_0: DC = 7, n = 175 (a partial
    last mask word); LP118_0: DC = 8; LP04_0z: LP04_0 with one column zeroed (a
    variable without checks)."""
    if name not in _CACHE:
        if name == "LP04_0z":
            H = codes.load_code("LP04_0")[0].copy()
            H[:, 70] = 0
        elif name == "LP118_0":
            H = codes.load_code(name)[1]
        else:
            H = codes.load_code(name)[0]
        _CACHE[name] = (np.ascontiguousarray(H), pm.Graph(H))
    return _CACHE[name]


def _layers(H, sched):
    return None if sched == "F" else simulator.layerize(H, serial=sched == "S")


def _syndromes(H, B, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "random":
        return rng.integers(0, 2, (B, H.shape[0]), dtype=np.uint8)
    e = (rng.random((B, H.shape[1])) < 0.05 * 2 / 3).astype(np.int64)
    return ((e @ H.T.astype(np.int64)) % 2).astype(np.uint8)


def _mask(B, n, density, seed):
    return (np.random.default_rng(seed).random((B, n)) < density).astype(np.uint8)


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _decode(H, syn, p, max_iter, algo, layers, mask=None, p1=None, **kw):
    kw.setdefault("want_post", True)
    if mask is not None:
        kw.update(prior_mask=mask, p_masked=p1)
    return decoders.decode_batch(H, syn, p, max_iter, layers=layers, algo=algo, **kw)


def _np(r, n=None):
    import torch
    torch.cuda.synchronize()
    e = r.ehat if r.ehat.dtype == torch.uint8 else decoders.unpack_bits(r.ehat, n)
    return (e.cpu().numpy(), r.iters.cpu().numpy(), None if r.post is None else r.post.cpu().numpy(),
            r.flags.cpu().numpy())


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: iterations"
    assert np.array_equal(a[0], b[0]), f"{what}: hard decisions"
    assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64)), f"{what}: posterior bits"
    assert np.array_equal(a[3], b[3]), f"{what}: flags"


ALGO_SCHED = [("MS", "F"), ("MS", "L"), ("MS", "S"), ("BP", "F"), ("BP", "L")]


@pytest.mark.parametrize("algo,sched", ALGO_SCHED)
@pytest.mark.parametrize("name", ["steane", "LP04_0", "LP118_0", "LP04_0z"])
def test_kernel_name(name, algo, sched):
    H, _ = _code(name)
    lp, lr = simulator.pack_layers(_layers(H, sched), H.shape[0])
    got = _lib.prior_kernel_name(H, lp, lr, algo, 0)
    dc = {"LP04_0": 7, "LP118_0": 8}.get(name, 0)
    assert got.startswith("decode_prior_kernel")
    assert got == f"decode_prior_kernel<{0 if algo == 'MS' else 1}, {'false' if sched == 'F' else 'true'}, {dc}>"


@pytest.mark.parametrize("algo,sched", ALGO_SCHED)
@pytest.mark.parametrize("name", ["steane", "LP04_0", "LP118_0", "LP04_0z"])
def test_equal_priors_equal_the_scalar_decode(name, algo, sched, qopt):
    """Any mask with p0 == p1 is the scalar decode bit for bit (ê, iterations,
    posterior bits, flags), through decode_kernel (the generic options) and
    through the default kernels; an all-zero mask decodes at p0 and an all-one
    mask at p1 when they differ. Batches of 1, 193 (a partly filled last
    workgroup) and 4096 (the queue under load)."""
    H, _ = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    mi = 12 if algo == "MS" else 8
    p0, p1 = 0.05 / 3, 0.3
    for B in (1, 193, 4096):
        syn = np.concatenate([_syndromes(H, B - B // 4, "channel", B), _syndromes(H, B // 4, "random", B + 1)])
        syn_d = _dev(syn)
        mask = _dev(_mask(B, n, 0.5, B + 2))
        prior = _np(_decode(H, syn_d, p0, mi, algo, layers, mask, p0))
        zeros = _np(_decode(H, syn_d, p0, mi, algo, layers, mask * 0, p1))
        ones = _np(_decode(H, syn_d, p0, mi, algo, layers, mask * 0 + 1, p1))
        for opts in (GENERIC, {}):
            qopt(**{k: opts.get(k, 0) for k in GENERIC})
            what = f"B={B} {'generic' if opts else 'default'} kernels"
            _same(prior, _np(_decode(H, syn_d, p0, mi, algo, layers)), what + ", random mask")
            _same(zeros, _np(_decode(H, syn_d, p0, mi, algo, layers)), what + ", zero mask")
            _same(ones, _np(_decode(H, syn_d, p1, mi, algo, layers)), what + ", one mask")


MODEL_CASES = [(name, "MS", s) for name in ("steane", "LP04_0", "LP118_0", "LP04_0z") for s in "FLS"] + \
              [(name, "BP", s) for name in ("steane", "LP04_0") for s in "FL"]


@pytest.mark.parametrize("name,algo,sched", MODEL_CASES)
def test_two_priors_against_the_model(name, algo, sched):
    """Random masks (5 % and 50 %) with p0 != p1 on channel syndromes (p = 0.05)
    and uniform random ones (these run to max_iter): ê, iterations, posterior
    bits and the CONVERGED / MIN_ZERO flags of the model."""
    H, g = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    big = n > 500
    # (the serial schedule is the model's slow case: one Python step per check)
    B = 4096 if n < 10 else 193 if sched != "S" else 16 if big else 96
    mi = (3 if sched == "S" else 6) if (big or sched == "S") else (10 if algo == "MS" else 6)
    p0, p1 = 0.05 / 3 / (1 - 2 * 0.05 / 3), 0.49
    for kind in ("channel", "random"):
        for density in (0.05, 0.5):
            syn = _syndromes(H, B, kind, 7)
            mask = _mask(B, n, density, 8)
            got = _np(_decode(H, _dev(syn), p0, mi, algo, layers, _dev(mask), p1))
            e, it, post, fl = pm.decode(algo, g, syn, pm.two_level(mask, p0, p1), mi, layers)
            what = f"{kind} syndromes, mask density {density}"
            assert np.array_equal(got[1], it), what + ": iterations"
            assert np.array_equal(got[0], e), what + ": hard decisions"
            assert np.array_equal(got[2].view(np.uint64), post.view(np.uint64)), what + ": posterior bits"
            assert np.array_equal(got[3] & 3, fl & 3), what + ": CONVERGED / MIN_ZERO"
            if kind == "random" and n > 7:
                assert (it == mi).any()
            # a single half-shot (one wave of one workgroup)
            one = _np(_decode(H, _dev(syn[:1]), p0, mi, algo, layers, _dev(mask[:1]), p1))
            assert np.array_equal(one[0], e[:1]) and np.array_equal(one[1], it[:1])
            assert np.array_equal(one[2].view(np.uint64), post[:1].view(np.uint64))


@pytest.mark.parametrize("sched", ["F", "L"])
def test_min_sum_with_a_zero_llr(sched):
    """p1 = 0.5 exactly: L1 = +0.0, min1 == 0 is common and flagged; the sparse
    semantics of the model hold."""
    H, g = _code("LP04_0")
    B, mi, p0, p1 = 193, 10, 0.02, 0.5
    syn = _syndromes(H, B, "channel", 3)
    mask = _mask(B, H.shape[1], 0.05, 4)
    got = _np(_decode(H, _dev(syn), p0, mi, "MS", _layers(H, sched), _dev(mask), p1))
    e, it, post, fl = pm.decode("MS", g, syn, pm.two_level(mask, p0, p1), mi, _layers(H, sched))
    assert np.array_equal(got[1], it) and np.array_equal(got[0], e)
    assert np.array_equal(got[2].view(np.uint64), post.view(np.uint64))
    assert np.array_equal(got[3] & 3, fl & 3)
    assert ((fl & pm.FLAG_MIN_ZERO) != 0).mean() > 0.5


@pytest.mark.parametrize("algo,sched", [("MS", "F"), ("BP", "L")])
def test_formats_buffers_and_static_schedule(algo, sched, qopt):
    """Mask format x syndrome format x ehat_bits give the same bits; a mask
    that is an earlier decode's ehat tensor; out= reuse across two calls with
    different masks; static_sched = 1 equals the queue."""
    H, _ = _code("LP04_0")
    m, n = H.shape
    layers = _layers(H, sched)
    B, mi, p0, p1 = 193, 8, 0.02, 0.45
    syn = _dev(_syndromes(H, B, "channel", 5))
    mask = _dev(_mask(B, n, 0.3, 6))
    want = _np(_decode(H, syn, p0, mi, algo, layers, mask, p1))
    for mk in (mask, decoders.pack_bits(mask)):
        for sy in (syn, decoders.pack_bits(syn)):
            for eb in (False, True):
                _same(want, _np(_decode(H, sy, p0, mi, algo, layers, mk, p1, ehat_bits=eb), n),
                      f"mask {mk.dtype} syndromes {sy.dtype} ehat_bits {eb}")
    # the first decode's estimate tensor itself is the second one's mask
    for eb in (False, True):
        first = _decode(H, syn, p0, mi, algo, layers, ehat_bits=eb)
        e1 = _np(first, n)[0]
        assert e1.any() and not e1.all()
        chained = _np(_decode(H, syn, p0, mi, algo, layers, first.ehat, p1), n)
        _same(chained, _np(_decode(H, syn, p0, mi, algo, layers, _dev(e1), p1)), f"aliased mask, ehat_bits {eb}")
    # out= written twice
    out = _decode(H, syn, p0, mi, algo, layers, mask, p1)
    other = 1 - mask
    want2 = _np(_decode(H, syn, p0, mi, algo, layers, other, p1))
    r = _decode(H, syn, p0, mi, algo, layers, other, p1, out=out)
    assert r.ehat.data_ptr() == out.ehat.data_ptr() and r.post.data_ptr() == out.post.data_ptr()
    _same(want2, _np(r), "out= second call")
    _same(want, _np(_decode(H, syn, p0, mi, algo, layers, mask, p1, out=out)), "out= third call")
    assert not np.array_equal(want[2], want2[2])
    qopt(static_sched=1)
    _same(want, _np(_decode(H, syn, p0, mi, algo, layers, mask, p1)), "static_sched")


def test_host_path_equals_the_device_path():
    H, _ = _code("LP04_0")
    B, mi, p0, p1 = 77, 8, 0.02, 0.45
    syn = _syndromes(H, B, "channel", 9)
    mask = _mask(B, H.shape[1], 0.3, 10)
    want = _np(_decode(H, _dev(syn), p0, mi, "MS", None, _dev(mask), p1))
    r = _decode(H, syn, p0, mi, "MS", None, mask, p1)
    _same(want, (r.ehat, r.iters, r.post, r.flags), "qldpc_decode_host_prior")
    # OSD on the host path reads the same posteriors afterwards
    r2 = _decode(H, syn, p0, mi, "MS", None, mask, p1, osd_order=0)
    bad = (r.flags & 1) == 0
    assert np.array_equal(r2.ehat[~bad], r.ehat[~bad])
    assert np.array_equal((r2.ehat[bad].astype(np.int64) @ H.T.astype(np.int64)) % 2, syn[bad])


def test_force_hbm_is_refused_and_restored():
    H, _ = _code("LP04_0")
    syn = _dev(_syndromes(H, 4, "channel", 1))
    mask = _dev(_mask(4, H.shape[1], 0.3, 2))
    before = _lib.get_option("force_hbm")
    with _lib.options(force_hbm=1):
        with pytest.raises(NotImplementedError, match="force_hbm"):
            _decode(H, syn, 0.02, 5, "MS", None, mask, 0.4)
        _decode(H, syn, 0.02, 5, "MS", None)                 # the scalar decode still takes the HBM kernel
    assert _lib.get_option("force_hbm") == before
    _decode(H, syn, 0.02, 5, "MS", None, mask, 0.4)


def _sim_shots(Hx, Hz, p, shots, seed):
    import torch
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), key)
    sy_z, sy_x, ewX, ewZ = ch.sample(p, shots)
    return (sy_z.cpu().numpy(), sy_x.cpu().numpy(), ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy())


def _result(c, shots):
    """simulate_p's dict from the nine counters."""
    r = {k: c[k] for k in ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen")}
    r["Avg_number_of_iterations_X"] = c["nIterAccX"] / float(shots)
    r["Avg_number_of_iterations_Z"] = c["nIterAccZ"] / float(shots)
    for k in simulator.LOGICAL_KEYS:
        r[k] = c[k]
    r["logical_error_rate"] = 1. - c["decSuccessLogical"] / float(shots)
    r["logical_error_rate_ci95"] = simulator.wilson_interval(shots - c["decSuccessLogical"], shots)
    return r


def _model_run(Hx, Hz, p, q1, order, decType, sched, mi, samples, osd=-1):
    """The reference's loop with the second half's prior taken from the first
    half's estimate, every decode on the model."""
    sy_z, sy_x, errX, errZ = samples
    layersX, layersZ = simulator.select_layers(Hx, Hz, sched)
    if sched == "F":
        layersX = layersZ = None
    halves = {"X": (Hz, sy_z, layersX), "Z": (Hx, sy_x, layersZ)}
    out, mask = {}, None
    for h in order:
        H, syn, layers = halves[h]
        L = np.full((len(syn), H.shape[1]), pm.llr(p / 3)) if mask is None else \
            pm.two_level(mask, (p / 3) / (1 - 2 * p / 3), q1)
        e, it, post, fl = pm.decode(decType, H, syn, L, mi, layers)
        if osd >= 0:                                         # (the library's host OSD on the model's posteriors)
            decoders.apply_osd(H, syn, e, post, fl, osd)
        out[h] = (e, it)
        mask = e
    c = logical_model.Model(Hx, Hz).counters(sy_z, sy_x, errX, errZ, out["X"][0], out["Z"][0], out["X"][1],
                                             out["Z"][1])
    return _result(c, len(sy_z))


@pytest.mark.parametrize("decType,sched,osd,p", [("MS", "F", -1, 0.06), ("BP", "L", -1, 0.06), ("MS", "L", 0, 0.1)])
@pytest.mark.parametrize("order", ["XZ", "ZX"])
def test_simulate_p_correlated(order, decType, sched, osd, p):
    """LP04_0, 330 shots in batches of 100 and 77, logical=True: the device
    pipeline equals (a) the host path on the same shots, (b) the reference's
    loop on the model, and (c) for the half decoded first, the uncorrelated
    run with the same seed."""
    Hx, Hz = codes.load_code("LP04_0")
    shots, seed, mi, q1 = 330, 11, 10, 0.49
    kw = dict(shots=shots, decType=decType, decIterations=mi, decSchedule=sched, OSDorder=osd, rngSeed=seed,
              verbose=False, logical=True)
    got = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="device", correlated=order, **kw)
    assert got == simulator.simulate_p(Hx, Hz, p, batch_size=77, sampler="device", correlated=order,
                                       correlated_q1=q1, **kw)
    samples = _sim_shots(Hx, Hz, p, shots, seed)
    host = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="host", samples=samples, correlated=order, **kw)
    assert got == host                                       # (a)
    want = _model_run(Hx, Hz, p, q1, order, decType, sched, mi, samples, osd)
    assert got == want                                       # (b)
    plain = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="device", **kw)
    f = order[0]
    for k in (f"DecFailures_{f}", f"Avg_number_of_iterations_{f}", f"logicalErrors_{f}"):
        assert got[k] == plain[k], k                         # (c)
    if osd >= 0:
        assert plain[f"Avg_number_of_iterations_{f}"] > 1 and decoders.OSD_STATS["osd_shots"] > 0


def test_the_gain_exists():
    """LP04_0 MS-F 30 iterations at p = 0.06, 20,000 shots, one seed: the Z
    half's logical errors + failures under "XZ" are below half of the
    uncorrelated run's (a float64 NumPy model predicted a ratio of 0.2-0.3 on
    roughly 900 events)."""
    Hx, Hz = codes.load_code("LP04_0")
    kw = dict(shots=20000, decType="MS", decIterations=30, decSchedule="F", rngSeed=5, verbose=False,
              logical=True, sampler="device")
    plain = simulator.simulate_p(Hx, Hz, 0.06, **kw)
    corr = simulator.simulate_p(Hx, Hz, 0.06, correlated="XZ", **kw)
    bad = lambda r: r["logicalErrors_Z"] + r["DecFailures_Z"]  # noqa: E731
    print(f"second-half events: independent {bad(plain)}, correlated {bad(corr)}; "
          f"logical error rate {plain['logical_error_rate']:.4f} -> {corr['logical_error_rate']:.4f}")
    assert bad(plain) > 300
    assert bad(corr) < 0.5 * bad(plain)
    assert corr["logicalErrors_X"] == plain["logicalErrors_X"] and corr["DecFailures_X"] == plain["DecFailures_X"]

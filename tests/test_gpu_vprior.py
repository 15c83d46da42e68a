"""decode_vprior_kernel (one prior per variable), the inhomogeneous Pauli
sampler and simulate_p's channel_weights on the GPU: against the scalar decode
where the vector is uniform, against decode_prior_kernel where it has two
values, against the test-side NumPy model (tests/prior_model.py) where it is
general; the sampler against the scalar sampler and the oracle's stream; the
simulator's counters against the reference's loop on the model."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import hard_model
import logical_model
import prior_model as pm
from oracle import oracle
from qldpcsim_amd import _lib, codes, decoders, simulator

pytestmark = pytest.mark.gpu

GENERIC = dict(flood_generic=1, layered_generic=1, bp_wave=1)
CODES = ["steane", "LP04_0", "LP118_0", "LP04_0z"]
ALGO_SCHED = [("MS", "F"), ("MS", "L"), ("MS", "S"), ("BP", "F"), ("BP", "L")]
_CACHE = {}


def _code(name):
    """steane: non-uniform degrees, n = 7, DC = 0; LP04_0: DC = 7, n = 175 (a
    partial last 64-bit word); LP118_0: DC = 8, several words; LP04_0z: LP04_0
    with one column zeroed (a variable without checks)."""
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


def _syndromes(H, B, seed):
    """Three quarters channel syndromes (p = 0.05), one quarter uniform random
    ones (these mostly run to max_iter)."""
    rng = np.random.default_rng(seed)
    nr = B // 4
    e = (rng.random((B - nr, H.shape[1])) < 0.05 * 2 / 3).astype(np.int64)
    ch = ((e @ H.T.astype(np.int64)) % 2).astype(np.uint8)
    return np.concatenate([ch, rng.integers(0, 2, (nr, H.shape[0]), dtype=np.uint8)])


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _decode(H, syn, p, max_iter, algo, layers, **kw):
    kw.setdefault("want_post", True)
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


@pytest.mark.parametrize("algo,sched", ALGO_SCHED)
@pytest.mark.parametrize("name", CODES)
def test_kernel_name(name, algo, sched):
    H, _ = _code(name)
    lp, lr = simulator.pack_layers(_layers(H, sched), H.shape[0])
    got = _lib.vprior_kernel_name(H, lp, lr, algo, 0)
    dc = {"LP04_0": 7, "LP118_0": 8}.get(name, 0)
    assert got == f"decode_vprior_kernel<{0 if algo == 'MS' else 1}, {'false' if sched == 'F' else 'true'}, {dc}>"
    assert got == _lib.prior_kernel_name(H, lp, lr, algo, 0).replace("decode_prior_kernel", "decode_vprior_kernel")


@pytest.mark.parametrize("algo,sched", ALGO_SCHED)
@pytest.mark.parametrize("name", CODES)
def test_uniform_vector_equals_the_scalar_decode(name, algo, sched, qopt):
    """prior = [p] * n is the scalar decode at p bit for bit (ê, iterations,
    posterior bits, flags), through decode_kernel (the generic options) and
    through the default kernels. Batches of 1, 300 and 512."""
    H, _ = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    mi = 12 if algo == "MS" else 8
    for B, p in ((1, 0.02), (300, 0.05 / 3), (512, 0.3)):
        syn = _dev(_syndromes(H, B, B))
        vec = _np(_decode(H, syn, None, mi, algo, layers, prior=np.full(n, p)))
        for opts in (GENERIC, {}):
            qopt(**{k: opts.get(k, 0) for k in GENERIC})
            _same(vec, _np(_decode(H, syn, p, mi, algo, layers)),
                  f"B={B} p={p} {'generic' if opts else 'default'} kernels")


@pytest.mark.parametrize("algo,sched", ALGO_SCHED)
@pytest.mark.parametrize("name", CODES)
def test_two_valued_vector_equals_the_two_level_kernel(name, algo, sched):
    """A vector with the values p0 and p1 is decode_prior_kernel's result when
    every mask row is the indicator of p1, bit for bit."""
    H, _ = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    mi = 12 if algo == "MS" else 8
    B, p0, p1 = 300, 0.05 / 3, 0.45
    ind = (np.random.default_rng(12).random(n) < 0.3).astype(np.uint8)
    ind[:2] = (0, 1)
    syn = _dev(_syndromes(H, B, 13))
    vec = _np(_decode(H, syn, None, mi, algo, layers, prior=np.where(ind != 0, p1, p0)))
    two = _np(_decode(H, syn, p0, mi, algo, layers, prior_mask=_dev(np.tile(ind, (B, 1))), p_masked=p1))
    _same(vec, two, "indicator mask")
    assert (two[1] == mi).any() or n < 10


def _general_vector(n, seed):
    """log-uniform in [1e-4, 0.3]; three entries above 0.5 (negative LLRs), one
    exactly 0 and one exactly 0.5 (none on column 70, LP04_0z's empty one)."""
    q = 10.0 ** np.random.default_rng(seed).uniform(-4, np.log10(0.3), n)
    q[0], q[n // 2], q[n - 1] = 0.7, 0.6, 0.9
    q[1], q[2] = 0.0, 0.5
    return q


MODEL_CASES = [(name, "MS", s) for name in CODES for s in "FLS"] + \
              [(name, "BP", s) for name in ("steane", "LP04_0") for s in "FL"]


@pytest.mark.parametrize("name,algo,sched", MODEL_CASES)
def test_general_vector_against_the_model(name, algo, sched):
    """ê, iterations, posterior bits and flags of prior_model.decode with the
    one row broadcast over the batch. The model raises CONVERGED and MIN_ZERO;
    NONFINITE is BP's alone and, with an LLR of exactly 0 on a variable that
    has checks, is raised by every shot's first check-node pass. BP's 0 / 0
    there is a NaN, whose sign and payload IEEE 754 leaves open: posteriors
    must be NaN in the same places and equal bit for bit everywhere else.
    (LP118_0 under the serial schedule, 240 one-row layers, is the model's slow
    case, one Python step per check: 32 half-shots there, 300 elsewhere.)"""
    H, g = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    big = n > 500
    B = 32 if (big and sched == "S") else 300
    mi = 3 if sched == "S" else 6 if big else (10 if algo == "MS" else 6)
    q = _general_vector(n, 21)
    L = np.array([pm.llr(x) for x in q])
    assert (L < 0).sum() == 3 and (L == 0).sum() == 1 and np.isfinite(L).all()
    syn = _syndromes(H, B, 22)
    got = _np(_decode(H, _dev(syn), None, mi, algo, layers, prior=q))
    e, it, post, fl = pm.decode(algo, g, syn, np.broadcast_to(L, (B, n)), mi, layers)
    assert np.array_equal(got[1], it), "iterations"
    assert np.array_equal(got[0], e), "hard decisions"
    if algo == "MS":
        assert np.array_equal(got[2].view(np.uint64), post.view(np.uint64)), "posterior bits"
        assert np.array_equal(got[3], fl), "flags"
        if sched == "F":                                         # (every check reads float32(L) in the first pass,
            assert (fl & pm.FLAG_MIN_ZERO).all()                 # and the zero LLR sits on a variable with checks)
    else:
        nan = np.isnan(post)
        assert np.array_equal(np.isnan(got[2]), nan), "NaN posteriors"
        assert np.array_equal(got[2].view(np.uint64)[~nan], post.view(np.uint64)[~nan]), "posterior bits"
        assert np.array_equal(got[3] & 3, fl & 3), "CONVERGED / MIN_ZERO"
        nonfinite = (got[3] & _lib.FLAG_NONFINITE) != 0
        assert nonfinite.all() if sched == "F" else nonfinite.any()   # (layered: a shot may stop before that check)
    assert (it == mi).any() or n < 10
    # a single half-shot (one wave of one workgroup)
    one = _np(_decode(H, _dev(syn[:1]), None, mi, algo, layers, prior=q))
    assert np.array_equal(one[0], e[:1]) and np.array_equal(one[1], it[:1])
    # without the degenerate entries BP's posteriors are finite and equal bit for bit
    if algo == "BP":
        q2 = q.copy()
        q2[2] = 0.2
        L2 = np.array([pm.llr(x) for x in q2])
        got = _np(_decode(H, _dev(syn), None, mi, algo, layers, prior=q2))
        e, it, post, fl = pm.decode(algo, g, syn, np.broadcast_to(L2, (B, n)), mi, layers)
        assert np.isfinite(post).all()
        _same(got, (e, it, post, fl), "finite priors")


@pytest.mark.parametrize("algo,sched", [("MS", "F"), ("BP", "L")])
def test_formats_buffers_streams_and_static_schedule(algo, sched, qopt):
    """Syndrome format x ehat_bits give the same bits; out= reuse across two
    calls with different vectors; a non-default stream; static_sched = 1
    equals the queue."""
    import torch
    H, _ = _code("LP04_0")
    n = H.shape[1]
    layers = _layers(H, sched)
    B, mi = 300, 8
    q = 10.0 ** np.random.default_rng(31).uniform(-3, np.log10(0.3), n)
    q[7] = 0.8
    syn = _dev(_syndromes(H, B, 32))
    want = _np(_decode(H, syn, None, mi, algo, layers, prior=q))
    for sy in (syn, decoders.pack_bits(syn)):
        for eb in (False, True):
            _same(want, _np(_decode(H, sy, None, mi, algo, layers, prior=q, ehat_bits=eb), n),
                  f"syndromes {sy.dtype} ehat_bits {eb}")
    out = _decode(H, syn, None, mi, algo, layers, prior=q)
    q2 = q[::-1].copy()
    want2 = _np(_decode(H, syn, None, mi, algo, layers, prior=q2))
    r = _decode(H, syn, None, mi, algo, layers, prior=q2, out=out)
    assert r.ehat.data_ptr() == out.ehat.data_ptr() and r.post.data_ptr() == out.post.data_ptr()
    _same(want2, _np(r), "out= second call")
    _same(want, _np(_decode(H, syn, None, mi, algo, layers, prior=q, out=out)), "out= third call")
    assert not np.array_equal(want[2], want2[2])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        r1 = _decode(H, syn, None, mi, algo, layers, prior=q)                       # torch's current stream
    r2 = _decode(H, syn, None, mi, algo, layers, prior=q, stream=st.cuda_stream)    # the raw handle
    st.synchronize()
    _same(want, _np(r1), "current stream")
    _same(want, _np(r2), "stream=")
    qopt(static_sched=1)
    _same(want, _np(_decode(H, syn, None, mi, algo, layers, prior=q)), "static_sched")


def test_host_path_handle_reuse_and_the_shims():
    H, _ = _code("LP04_0")
    n = H.shape[1]
    B, mi = 77, 8
    q = _general_vector(n, 41)
    syn = _syndromes(H, B, 42)
    code = _lib.code_for(H, 0)
    held = len(code._prior)
    for sched in ("F", "L"):                                     # one handle, two schedules of the code
        layers = _layers(H, sched)
        want = _np(_decode(H, _dev(syn), None, mi, "MS", layers, prior=q))
        r = _decode(H, syn, None, mi, "MS", layers, prior=q)
        _same(want, (r.ehat, r.iters, r.post, r.flags), f"qldpc_decode_host_vprior {sched}")
    assert len(code._prior) == held + 1                          # (the host path's code object is another one)
    # OSD on the host path reads the same posteriors afterwards
    r2 = _decode(H, syn, None, mi, "MS", None, prior=q, osd_order=0)
    r = _decode(H, syn, None, mi, "MS", None, prior=q)
    bad = (r.flags & 1) == 0
    assert bad.any() and np.array_equal(r2.ehat[~bad], r.ehat[~bad])
    fix = bad & (np.arange(B) < B - B // 4)                      # (a uniform random syndrome need not lie in H's image)
    assert fix.any()
    assert np.array_equal((r2.ehat[fix].astype(np.int64) @ H.T.astype(np.int64)) % 2, syn[fix])
    # the single-shot shims take an array for p
    for i in (0, B - 1):
        e, it = decoders.MS_decoder(H, syn[i], q, max_iter=mi)
        assert np.array_equal(e, r.ehat[i]) and it == r.iters[i] and e.dtype == np.int8
        e, it = decoders.MS_decoder(H, syn[i], q, max_iter=mi, OSDorder=0)
        assert np.array_equal(e, r2.ehat[i])
    rb = _decode(H, syn[:2], None, mi, "BP", None, prior=q)
    e, it = decoders.BP_decoder(H, syn[1], q, max_iter=mi)
    assert np.array_equal(e, rb.ehat[1]) and it == rb.iters[1]


def test_force_hbm_is_refused_and_restored():
    H, _ = _code("LP04_0")
    syn = _dev(_syndromes(H, 4, 1))
    q = np.full(H.shape[1], 0.02)
    q[3] = 0.2
    before = _lib.get_option("force_hbm")
    with _lib.options(force_hbm=1):
        with pytest.raises(NotImplementedError, match="force_hbm"):
            _decode(H, syn, None, 5, "MS", None, prior=q)
        _decode(H, syn, 0.02, 5, "MS", None)                     # the scalar decode still takes the HBM kernel
    assert _lib.get_option("force_hbm") == before
    _decode(H, syn, None, 5, "MS", None, prior=q)


# ---------------------------------------------------------------------------
# sampler
# ---------------------------------------------------------------------------
def _sample_vec(Hx, Hz, probs, seed, shot0, B, bits=False):
    import torch
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), seed, shot0)
    ch.set_probs(probs)
    sy_z, sy_x, ewX, ewZ = ch.sample(None, B, bits=bits)
    torch.cuda.synchronize()
    if bits:
        sy_z, sy_x = decoders.unpack_bits(sy_z, Hz.shape[0]), decoders.unpack_bits(sy_x, Hx.shape[0])
    return tuple(a.cpu().numpy() for a in (sy_z, sy_x, ch.unpack(ewX), ch.unpack(ewZ)))


@pytest.mark.parametrize("name", ["LP04_0", "LP118_0"])
def test_sampler_equals_the_scalar_sampler_on_a_depolarizing_table(name):
    import torch
    Hx, Hz = codes.load_code(name)
    n = Hx.shape[1]
    B, seed, shot0 = 300, 0x1234567890ABCDEF, (1 << 32) - 100    # (the shot counter crosses 2^32)
    for p in (0.1, 1.0, 0.0):
        probs = np.full((3, n), p / 3)
        for bits in (False, True):
            ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), seed, shot0)
            sy_z, sy_x, ewX, ewZ = ch.sample(p, B, bits=bits)
            torch.cuda.synchronize()
            if bits:
                sy_z, sy_x = decoders.unpack_bits(sy_z, Hz.shape[0]), decoders.unpack_bits(sy_x, Hx.shape[0])
            want = tuple(a.cpu().numpy() for a in (sy_z, sy_x, ch.unpack(ewX), ch.unpack(ewZ)))
            got = _sample_vec(Hx, Hz, probs, seed, shot0, B, bits)
            for g_, w_, what in zip(got, want, ("sy_z", "sy_x", "errX", "errZ")):
                assert np.array_equal(g_, w_), f"p={p} bits={bits}: {what}"
        if p == 0.1:
            assert want[2].any() and want[3].any()


def _oracle_sample(Hx, Hz, T, seed, shot0, B):
    """The oracle's stream with the thresholds (t1, t2, t3) on every qubit."""
    n = Hx.shape[1]
    rpx, cix = oracle.csr(Hx)
    rpz, ciz = oracle.csr(Hz)
    ex, ez = np.zeros((B, n), np.uint8), np.zeros((B, n), np.uint8)
    syz, syx = np.zeros((B, Hz.shape[0]), np.uint8), np.zeros((B, Hx.shape[0]), np.uint8)
    P = oracle._p
    oracle.lib().oracle_channel_sample(n, Hx.shape[0], P(rpx), P(cix), Hz.shape[0], P(rpz), P(ciz), int(T[0]),
                                       int(T[1]), int(T[2]), int(seed) & (2 ** 64 - 1), int(shot0), int(B), P(ex),
                                       P(ez), P(syz), P(syx))
    return ex, ez


def _expected_shots(Hx, Hz, probs, seed, shot0, B):
    """u(shot, j) depends on (shot, j) alone: column j's error bits are those of
    an oracle run with column j's thresholds everywhere (one run per distinct
    triple, columns merged); syndromes are H e mod 2."""
    n = Hx.shape[1]
    T = _lib.channel_table(probs[0], probs[1], probs[2])
    errX, errZ = np.zeros((B, n), np.uint8), np.zeros((B, n), np.uint8)
    triples = np.unique(T, axis=1)
    for k in range(triples.shape[1]):
        cols = (T == triples[:, k:k + 1]).all(0)
        ex, ez = _oracle_sample(Hx, Hz, triples[:, k], seed, shot0, B)
        errX[:, cols], errZ[:, cols] = ex[:, cols], ez[:, cols]
    sy_z = ((errX.astype(np.int64) @ Hz.T.astype(np.int64)) % 2).astype(np.uint8)
    sy_x = ((errZ.astype(np.int64) @ Hx.T.astype(np.int64)) % 2).astype(np.uint8)
    return sy_z, sy_x, errX, errZ, triples.shape[1]


def _three_triples(n, scale=1.0):
    """[3, n] probabilities with three distinct per-qubit triples."""
    tri = np.array([[0.02, 0.01, 0.15], [0.2, 0.0, 0.0], [0.0, 0.05, 0.4]]).T * scale
    return np.ascontiguousarray(tri[:, np.random.default_rng(51).integers(0, 3, n)])


@pytest.mark.parametrize("name", ["LP04_0", "LP118_0"])
def test_sampler_against_the_oracle_stream_and_batch_splits(name):
    Hx, Hz = codes.load_code(name)
    n = Hx.shape[1]
    probs = _three_triples(n)
    seed, shot0, B = 77, 1000, 300
    *want, k = _expected_shots(Hx, Hz, probs, seed, shot0, B)
    assert k == 3
    for bits in (False, True):
        got = _sample_vec(Hx, Hz, probs, seed, shot0, B, bits)
        for g_, w_, what in zip(got, want, ("sy_z", "sy_x", "errX", "errZ")):
            assert np.array_equal(g_, w_), f"bits={bits}: {what}"
    # one call of 300 shots against calls of 100 + 77 + 123
    parts, s0 = [], shot0
    for b in (100, 77, 123):
        parts.append(_sample_vec(Hx, Hz, probs, seed, s0, b))
        s0 += b
    for i, what in enumerate(("sy_z", "sy_x", "errX", "errZ")):
        assert np.array_equal(np.concatenate([p_[i] for p_ in parts]), want[i]), what
    # the three Paulis occur where, and only where, their probability is not zero
    X, Z = want[2].astype(bool), want[3].astype(bool)
    for pr, ev in ((probs[0], X & ~Z), (probs[1], X & Z), (probs[2], ~X & Z)):
        assert not ev[:, pr == 0].any() and ev[:, pr > 0].any()


# ---------------------------------------------------------------------------
# simulate_p(channel_weights=...)
# ---------------------------------------------------------------------------
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


def _model_counters(Hx, Hz, p, w, decType, sched, mi, samples, osd=-1):
    """The reference's per-shot loop, every decode on the model (NG: on the
    hard-decision model) with the true marginals as priors."""
    sy_z, sy_x, errX, errZ = samples
    layersX, layersZ = simulator.select_layers(Hx, Hz, sched)
    if sched == "F":
        layersX = layersZ = None
    out = {}
    for h, H, syn, layers, q in (("X", Hz, sy_z, layersX, p * (w[0] + w[1])),
                                 ("Z", Hx, sy_x, layersZ, p * (w[2] + w[1]))):
        if decType == "NG":
            e, it = hard_model.ng_batch(H, syn)[:2]
        else:
            L = np.array([pm.llr(x) for x in q])
            e, it, post, fl = pm.decode(decType, H, syn, np.broadcast_to(L, (len(syn), H.shape[1])), mi, layers)
            if osd >= 0:                                         # (the library's host OSD on the model's posteriors)
                decoders.apply_osd(H, syn, e, post, fl, osd)
        out[h] = (e, it)
    return logical_model.Model(Hx, Hz).counters(sy_z, sy_x, errX, errZ, out["X"][0], out["Z"][0], out["X"][1],
                                                out["Z"][1])


def _weights(n):
    """Inhomogeneous [3, n] weights: three triples, both halves' marginals non-uniform."""
    return _three_triples(n, scale=1.0)


@pytest.mark.parametrize("decType,sched,osd", [("MS", "F", -1), ("MS", "L", 0), ("BP", "L", -1), ("NG", "F", -1)])
def test_simulate_p_channel_weights(decType, sched, osd):
    """LP04_0, 330 shots in batches of 100 and 77, logical=True: the device
    pipeline equals the host path on the same shots and the reference's loop
    on the model; the shots are regenerated from the oracle's stream."""
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    shots, seed, mi, p = 330, 11, 10, 0.3
    w = _weights(n)
    kw = dict(shots=shots, decType=decType, decIterations=mi, decSchedule=sched, OSDorder=osd, rngSeed=seed,
              verbose=False, logical=True, channel_weights=w)
    got = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="device", **kw)
    assert got == simulator.simulate_p(Hx, Hz, p, batch_size=77, sampler="device", **kw)
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    samples = _expected_shots(Hx, Hz, simulator.channel_probs(p, w, n), int(key), 0, shots)[:4]
    host = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="host", samples=samples, **kw)
    assert got == host
    want = _result(_model_counters(Hx, Hz, p, w, decType, sched, mi, samples, osd), shots)
    assert got == want
    assert got["DecFailures_X"] + got["DecFailures_Z"] + got["logicalErrors_X"] + got["logicalErrors_Z"] > 0


def test_simulate_p_host_sampler_runs_the_vector_path():
    """sampler="host" without samples=: the NumPy sampler and
    qldpc_decode_host_vprior, counted against the model on the same draw."""
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    shots, seed, mi, p = 150, 5, 8, 0.3
    w = _weights(n)
    got = simulator.simulate_p(Hx, Hz, p, shots=shots, decType="MS", decIterations=mi, rngSeed=seed, verbose=False,
                               logical=True, channel_weights=w, sampler="host", batch_size=64)
    rng = np.random.default_rng([seed, 0])
    probs = simulator.channel_probs(p, w, n)
    parts = [simulator.sample_channel_vec(Hx, Hz, probs, b, rng) for b in (64, 64, 22)]
    samples = tuple(np.concatenate([q[i] for q in parts]) for i in range(4))
    assert got == _result(_model_counters(Hx, Hz, p, w, "MS", "F", mi, samples), shots)


def test_uniform_bias_runs_the_scalar_entry_point(monkeypatch):
    """--bias 10: both halves' marginals are uniform, so decode_batch is called
    with a scalar p and no prior=, and the counters are those of the same
    shots decoded with those scalars."""
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    shots, seed, mi, p = 330, 11, 10, 0.2
    w = simulator.bias_weights(10)
    calls = []
    real = decoders.decode_batch

    def spy(H, syn, p_, *a, **kw):
        calls.append((p_, kw.get("prior")))
        return real(H, syn, p_, *a, **kw)

    monkeypatch.setattr(decoders, "decode_batch", spy)
    kw = dict(shots=shots, decType="MS", decIterations=mi, rngSeed=seed, verbose=False, logical=True)
    got = simulator.simulate_p(Hx, Hz, p, batch_size=100, sampler="device", channel_weights=w, **kw)
    assert calls and all(pr is None for _, pr in calls)
    assert {c[0] for c in calls} == {p * (w[0] + w[1]), p * (w[2] + w[1])}
    monkeypatch.setattr(decoders, "decode_batch", real)
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    sy_z, sy_x, errX, errZ, k = _expected_shots(Hx, Hz, simulator.channel_probs(p, w, n), int(key), 0, shots)
    assert k == 1
    rX = real(Hz, sy_z, p * (w[0] + w[1]), mi)
    rZ = real(Hx, sy_x, p * (w[2] + w[1]), mi)
    c = simulator.count_logical_outcomes(Hx, Hz, sy_z, sy_x, errX, errZ, rX.ehat, rZ.ehat, rX.iters, rZ.iters)
    assert got == _result(c, shots)
    assert errZ.sum() > 3 * errX.sum() > 0                       # the bias is there


def test_cli_two_ranks_channel_weights(tmp_path):
    """`torchrun -m qldpcsim_amd.simulator --channel-weights` with two gloo
    ranks on the one GPU: the all-reduced counters equal the model's count
    over both ranks' shards (rank r's contiguous share from its Philox key)."""
    from conftest import ROOT
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    np.save(tmp_path / "Hx.npy", Hx.astype(np.int64))
    np.save(tmp_path / "Hz.npy", Hz.astype(np.int64))
    w = _weights(n)
    np.save(tmp_path / "w.npy", w)
    res = tmp_path / "res.json"
    shots, seed, p, it = 331, 4, 0.3, 10
    env = dict(os.environ, QLDPC_SIM_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29547", "-m", "qldpcsim_amd.simulator",
                        "--Hx", str(tmp_path / "Hx.npy"), "--Hz", str(tmp_path / "Hz.npy"), "--p", str(p),
                        "--shots", str(shots), "--decIterations", str(it), "--rngSeed", str(seed), "--batch", "100",
                        "--logical", "--channel-weights", str(tmp_path / "w.npy"), "--results", str(res)],
                       cwd=ROOT, capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.loads(res.read_text())
    assert doc["meta"]["world"] == 2 and doc["meta"]["channel_weights"]["shape"] == [3, n]
    got = doc["results"][str(p)]
    want = None
    for rank in range(2):
        my = shots // 2 + (1 if rank < shots % 2 else 0)
        key = np.random.SeedSequence([seed, rank]).generate_state(1, np.uint64)[0]
        samples = _expected_shots(Hx, Hz, simulator.channel_probs(p, w, n), int(key), 0, my)[:4]
        c = _model_counters(Hx, Hz, p, w, "MS", "F", it, samples)
        want = c if want is None else {k: want[k] + c[k] for k in c}
    for k in ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen") + tuple(simulator.LOGICAL_KEYS):
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["Avg_number_of_iterations_X"] - want["nIterAccX"] / shots) < 1e-9
    assert abs(got["Avg_number_of_iterations_Z"] - want["nIterAccZ"] / shots) < 1e-9


# ---------------------------------------------------------------------------
# the gain
# ---------------------------------------------------------------------------
def test_the_gain_exists():
    """LP04_0 Hz, a quarter of the qubits at marginal error probability 0.12
    and the rest at 0.004, 4000 shots drawn with NumPy, MS flooding, 30
    iterations: prior=q against p=q.mean(). The GPU's non-converged counts
    equal the model's exactly, and the per-qubit prior leaves fewer than a
    third of the scalar prior's (a CPU trial with another draw: 10 against
    92)."""
    _, Hz = codes.load_code("LP04_0")
    H = np.ascontiguousarray(Hz)
    n = H.shape[1]
    hot = np.random.default_rng(5).permutation(n)[:n // 4]
    q = np.full(n, 0.004)
    q[hot] = 0.12
    shots, mi = 4000, 30
    e = (np.random.default_rng(6).random((shots, n)) < q).astype(np.uint8)
    syn = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2).astype(np.uint8)
    g = pm.Graph(H)
    Lv = np.broadcast_to(np.array([pm.llr(x) for x in q]), (shots, n))
    Ls = np.full((shots, n), pm.llr(q.mean()))
    mv = pm.decode("MS", g, syn, Lv, mi)
    ms = pm.decode("MS", g, syn, Ls, mi)
    fails = lambda fl: int(((fl & 1) == 0).sum())                # noqa: E731
    gv = _np(_decode(H, _dev(syn), None, mi, "MS", None, prior=q))
    gs = _np(_decode(H, _dev(syn), float(q.mean()), mi, "MS", None))
    print(f"non-converged: model vector {fails(mv[3])} scalar {fails(ms[3])}; GPU vector {fails(gv[3])} "
          f"scalar {fails(gs[3])}; wrong estimates: vector {int((gv[0] != e).any(1).sum())} "
          f"scalar {int((gs[0] != e).any(1).sum())}")
    assert fails(gv[3]) == fails(mv[3]) and fails(gs[3]) == fails(ms[3])
    assert np.array_equal(gv[0], mv[0]) and np.array_equal(gs[0], ms[0])
    assert 3 * fails(gv[3]) < fails(gs[3])

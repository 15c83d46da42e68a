"""hbm_tile_vprior_kernel (library option vprior_hbm) on the
GPU: bit for bit against the LDS twin decode_vprior_kernel where that one
runs (force_hbm as well), against the scalar HBM kernel on a uniform vector,
against the test-side NumPy model (tests/prior_model.py) past each of the LDS
twin's limits, and through the simulator's drivers."""
import functools

import numpy as np
import pytest

import dem_model as dm
import prior_model as pm
from wide_column_model import bp_flood_numpy as _bp_flood_numpy   # (the NumPy loop this file held)
from qldpcsim_amd import _lib, codes, decoders, simulator

pytestmark = pytest.mark.gpu

HBM = dict(vprior_hbm=1, force_hbm=1)
ALGO_SCHED = [("MS", "F"), ("MS", "L"), ("MS", "S"), ("BP", "F"), ("BP", "L")]
CODES = ["steane", "LP04_0", "LP04_0z", "LP118_0"]
NAME = "hbm_tile_vprior_kernel<%d, %d, 4>"


@functools.lru_cache(maxsize=None)
def _code(name):
    """steane: non-uniform degrees, n = 7; LP04_0: n = 175 (a partial last
    64-bit word); LP04_0z: LP04_0 with column 70 zeroed (a variable without
    checks); LP118_0: Hz, several words."""
    if name == "LP04_0z":
        H = codes.load_code("LP04_0")[0].copy()
        H[:, 70] = 0
    else:
        H = codes.load_code(name)[1 if name == "LP118_0" else 0]
    return np.ascontiguousarray(H)


def _layers(H, sched):
    return None if sched == "F" else simulator.layerize(H, serial=sched == "S")


def _syndromes(H, B, seed, p=0.05 * 2 / 3):
    """Three quarters channel syndromes, one quarter uniform random ones
    (these mostly run to max_iter)."""
    rng = np.random.default_rng(seed)
    nr = B // 4
    e = (rng.random((B - nr, H.shape[1])) < p).astype(np.int64)
    ch = ((e @ H.T.astype(np.int64)) % 2).astype(np.uint8)
    return np.concatenate([ch, rng.integers(0, 2, (nr, H.shape[0]), dtype=np.uint8)])


def _general_vector(n, seed):
    """test_gpu_vprior.py's: log-uniform in [1e-4, 0.3]; three entries above
    0.5 (negative LLRs), one exactly 0 and one exactly 0.5."""
    q = 10.0 ** np.random.default_rng(seed).uniform(-4, np.log10(0.3), n)
    q[0], q[n // 2], q[n - 1] = 0.7, 0.6, 0.9
    q[1], q[2] = 0.0, 0.5
    return q


def _finite_vector(n, seed):
    """Log-uniform in [1e-3, 0.3] with two entries above 0.5 and none at 0.5:
    every LLR is finite and none is 0, so BP's posteriors are finite."""
    q = 10.0 ** np.random.default_rng(seed).uniform(-3, np.log10(0.3), n)
    q[0], q[n // 3] = 0.7, 0.6
    return q


def _llr(q):
    return np.array([pm.llr(x) for x in q])


def _dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")


def _decode(H, syn, max_iter, algo, layers, q, **kw):
    kw.setdefault("want_post", True)
    return decoders.decode_batch(H, syn, None, max_iter, layers=layers, algo=algo, prior=q, **kw)


def _np(r, n=None):
    import torch
    torch.cuda.synchronize()
    e = r.ehat if r.ehat.dtype == torch.uint8 else decoders.unpack_bits(r.ehat, n)
    return (e.cpu().numpy(), r.iters.cpu().numpy(), None if r.post is None else r.post.cpu().numpy(),
            r.flags.cpu().numpy())


def _same(a, b, what):
    """ê, iterations, posterior bits and the whole flag word. Posteriors that
    are NaN (BP with an LLR of exactly 0: 0 / 0, whose sign and payload IEEE
    754 leaves open) must be NaN in the same places."""
    assert np.array_equal(a[1], b[1]), f"{what}: iterations"
    assert np.array_equal(a[0], b[0]), f"{what}: hard decisions"
    nan = np.isnan(b[2])
    assert np.array_equal(np.isnan(a[2]), nan), f"{what}: NaN posteriors"
    assert np.array_equal(a[2].view(np.uint64)[~nan], b[2].view(np.uint64)[~nan]), f"{what}: posterior bits"
    assert np.array_equal(a[3], b[3]), f"{what}: flags"


def _name(H, layers, algo):
    lp, lr = simulator.pack_layers(layers, H.shape[0])
    return _lib.vprior_kernel_name(H, lp, lr, algo, 0)


def _inst(H, algo):
    d = int(H.sum(axis=1).max())
    return NAME % (_lib.ALGO[algo], 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64)


# ---------------------------------------------------------------------------
# 1. against the LDS twin, bit for bit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo,sched", ALGO_SCHED)
@pytest.mark.parametrize("name", CODES)
def test_equals_the_lds_twin(name, algo, sched, qopt):
    """The general vector (negative, zero and huge LLRs), B = 300: four full
    64-slot tiles and a ragged one, so slots recycle. ê, iterations, posterior
    bits (NaN in the same places) and the whole flag word equal
    decode_vprior_kernel's; steane and LP04_0 also equal the model directly
    (the model raises no NONFINITE: CONVERGED and MIN_ZERO there)."""
    H = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    big = n > 500
    mi = 3 if sched == "S" else 6 if big else (10 if algo == "MS" else 6)
    q = _general_vector(n, 21)
    syn = _syndromes(H, 300, 22)
    assert _name(H, layers, algo).startswith("decode_vprior_kernel<")
    want = _np(_decode(H, _dev(syn), mi, algo, layers, q))
    qopt(**HBM)
    assert _name(H, layers, algo) == _inst(H, algo)
    got = _np(_decode(H, _dev(syn), mi, algo, layers, q))
    _same(got, want, "against decode_vprior_kernel")
    assert (got[1] == mi).any() or n < 10
    if name in ("steane", "LP04_0"):
        e, it, post, fl = pm.decode(algo, H, syn, np.broadcast_to(_llr(q), (300, n)), mi, layers)
        _same((got[0], got[1], got[2], got[3] & 3), (e, it, post, fl), "against the model")


# ---------------------------------------------------------------------------
# 2. a uniform vector is the scalar HBM kernel's decode
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo,sched", [("MS", "L"), ("BP", "F")])
@pytest.mark.parametrize("name", ["LP04_0", "LP118_0"])
def test_uniform_vector_equals_the_scalar_hbm_kernel(name, algo, sched, qopt):
    H = _code(name)
    n = H.shape[1]
    layers = _layers(H, sched)
    lp, lr = simulator.pack_layers(layers, H.shape[0])
    mi = 12 if algo == "MS" else 8
    syn = _dev(_syndromes(H, 130, 5))
    qopt(**HBM)
    assert _lib.kernel_name(H, lp, lr, algo, 0) == _inst(H, algo).replace("_vprior", "")
    for p in (0.05 / 3, 0.6):                                     # (0.6: a negative LLR everywhere)
        want = _np(decoders.decode_batch(H, syn, p, mi, layers=layers, algo=algo, want_post=True))
        _same(_np(_decode(H, syn, mi, algo, layers, np.full(n, p))), want, f"p = {p}")


# ---------------------------------------------------------------------------
# 3. past each limit of the LDS twin, without force_hbm
# ---------------------------------------------------------------------------
def _refused(H, algo, layers, q, match):
    with pytest.raises(NotImplementedError, match=match):
        _decode(H, _dev(np.zeros((1, H.shape[0]), np.uint8)), 2, algo, layers, q)


@functools.lru_cache(maxsize=None)
def _wide_rows():
    """12 x 130: row 0 has 33 entries (the first degree past the LDS twin's
    min-sum limit), row 1 has 65 (the first past the HBM kernel's 64-edge
    registers: the two-pass check node), rows 2..11 have 6; column degrees 1
    and 2."""
    H = np.zeros((12, 130), np.uint8)
    H[0, :33] = 1
    H[1, 33:98] = 1
    for k in range(60):
        H[2 + k % 10, 98 + k if k < 32 else 3 * (k - 32)] = 1
    assert sorted(H.sum(1)) == [6] * 10 + [33, 65] and H.sum(0).min() == 1 and H.sum(0).max() == 2
    return H


@pytest.mark.parametrize("sched", ["F", "L"])
def test_ms_rows_of_33_and_65_entries(sched, qopt):
    H = _wide_rows()
    layers = _layers(H, sched)
    q = _finite_vector(130, 31)
    q[5] = 0.5                                                    # (an LLR of 0 on the 33-entry row)
    syn = _syndromes(H, 130, 32, p=0.01)
    _refused(H, "MS", layers, q, "MS row degree 65 > 32")
    qopt(vprior_hbm=1)
    assert _name(H, layers, "MS") == NAME % (0, 64)
    got = _np(_decode(H, _dev(syn), 10, "MS", layers, q))
    _same(got, pm.decode("MS", H, syn, np.broadcast_to(_llr(q), (130, 130)), 10, layers), "against the model")
    assert (got[1] < 10).any()


@pytest.mark.parametrize("sched", ["F", "L"])
def test_bp_rows_of_33_and_65_entries(sched, qopt):
    """BP has no row limit in the LDS twin: forced (both options), against
    the model and against the twin."""
    H = _wide_rows()
    layers = _layers(H, sched)
    q = _finite_vector(130, 33)
    syn = _syndromes(H, 130, 34, p=0.01)
    twin = _np(_decode(H, _dev(syn), 6, "BP", layers, q))
    qopt(**HBM)
    assert _name(H, layers, "BP") == NAME % (1, 64)
    got = _np(_decode(H, _dev(syn), 6, "BP", layers, q))
    want = pm.decode("BP", H, syn, np.broadcast_to(_llr(q), (130, 130)), 6, layers)
    assert np.isfinite(want[2]).all()
    _same(got, want, "against the model")
    _same(got, twin, "against decode_vprior_kernel")


def test_more_than_65535_edges(qopt):
    """64 x 65600, one entry per column (row degree 1025, E = n = 65600),
    bit-packed syndromes and estimates."""
    m, n, B = 64, 65600, 8
    H = np.zeros((m, n), np.uint8)
    H[np.arange(n) % m, np.arange(n)] = 1
    q = _finite_vector(n, 41)
    q[7] = 0.5
    syn = _syndromes(H, B, 42, p=0.0005)
    with pytest.raises(NotImplementedError, match="65535"):
        _name(H, None, "MS")
    qopt(vprior_hbm=1)
    assert _name(H, None, "MS") == NAME % (0, 64)
    got = _np(_decode(H, decoders.pack_bits(_dev(syn)), 4, "MS", None, q, ehat_bits=True), n)
    _same(got, pm.decode("MS", H, syn, np.broadcast_to(_llr(q), (B, n)), 4), "against the model")


def test_bp_column_of_129_entries(qopt):
    """m = 129, n = 4: column 0 holds every row (129 entries: np.sum splits it
    into 64 + 65), columns 1..3 hold 43 rows each. Not pm.decode's ground (it
    sums columns sequentially, degree < 8): a NumPy loop in this file."""
    m, n, B = 129, 4, 70
    H = np.zeros((m, n), np.uint8)
    H[:, 0] = 1
    H[np.arange(m), 1 + np.arange(m) % 3] = 1
    q = np.array([0.004, 0.2, 0.03, 0.6])
    rng = np.random.default_rng(51)
    e = (rng.random((B, n)) < 0.3).astype(np.int64)
    syn = ((e @ H.T.astype(np.int64)) % 2).astype(np.uint8)
    syn[B - 10:] = rng.integers(0, 2, (10, m), dtype=np.uint8)
    _refused(H, "BP", None, q, "BP column degree 129 > 128")
    qopt(vprior_hbm=1)
    assert _name(H, None, "BP") == NAME % (1, 8)
    got = _np(_decode(H, _dev(syn), 5, "BP", None, q))
    want_e, want_it, want_p = _bp_flood_numpy(H, syn, _llr(q), 5)
    assert np.isfinite(want_p).all() and (want_it < 5).any() and (want_it == 5).any()
    assert np.array_equal(got[1], want_it), "iterations"
    assert np.array_equal(got[0], want_e), "hard decisions"
    assert np.array_equal(got[2].view(np.uint64), want_p.view(np.uint64)), "posterior bits"
    ok = np.all((want_e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn, axis=1)
    assert np.array_equal((got[3] & _lib.FLAG_CONVERGED) != 0, ok), "CONVERGED"


def _regular_code(n, dv, dc, seed):
    """test_gpu_hbm.py's random (dv, dc)-regular matrix."""
    rng = np.random.default_rng(seed)
    m = n * dv // dc
    rows = rng.permutation(np.repeat(np.arange(m), dc))
    H = np.zeros((m, n), np.uint8)
    H[rows, np.repeat(np.arange(n), dv)] = 1
    return H


def test_state_past_the_lds(qopt):
    """The first (3, 6)-regular n of 3000, 4000, 5000, 6000 whose tables and
    one wave's state the LDS twin refuses ("do not fit"): min-sum flooding,
    B = 40, against the model."""
    for n in (3000, 4000, 5000, 6000):
        H = _regular_code(n, 3, 6, 1)
        q = _finite_vector(n, 61)
        try:
            _decode(H, _dev(np.zeros((1, H.shape[0]), np.uint8)), 1, "MS", None, q)
        except NotImplementedError as ex:
            assert "do not fit" in str(ex)
            break
    else:
        pytest.fail("every size up to n = 6000 fits the LDS twin")
    assert _name(H, None, "MS").startswith("decode_vprior_kernel<")   # (option off: the name asks no LDS size)
    qopt(vprior_hbm=1)
    assert _name(H, None, "MS") == NAME % (0, 8)
    syn = _syndromes(H, 40, 62, p=0.01)
    got = _np(_decode(H, _dev(syn), 5, "MS", None, q))
    _same(got, pm.decode("MS", H, syn, np.broadcast_to(_llr(q), (40, n)), 5), "against the model")
    assert (got[1] < 5).any() and (got[1] == 5).any()


# ---------------------------------------------------------------------------
# 4. a schedule that is not a partition of the rows: the initialising pass
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["MS", "BP"])
def test_non_partition_schedule(algo, qopt):
    """test_forced_hbm_non_partition_schedule's layers (row 5 in two layers,
    row 10 in none: hbm_lazy = 0, the state is initialised, BP's posteriors
    to Lv[v]) on LP04_0, max_iter 1 and 12, against the LDS twin."""
    H = _code("LP04_0")
    layers = [np.asarray(l) for l in simulator.layerize(H)]
    layers[-1] = np.append(layers[-1], 5)
    layers = [l[l != 10] for l in layers]
    assert any(5 in l for l in layers[:-1]) and not any(10 in l for l in layers)
    q = _general_vector(H.shape[1], 71)
    syn = _dev(_syndromes(H, 200, 72))
    for mi in (1, 12):
        qopt(vprior_hbm=0, force_hbm=0)
        want = _np(_decode(H, syn, mi, algo, layers, q))
        qopt(**HBM)
        assert _name(H, layers, algo) == NAME % (_lib.ALGO[algo], 8)
        _same(_np(_decode(H, syn, mi, algo, layers, q)), want, f"max_iter {mi}")


# ---------------------------------------------------------------------------
# 5. ragged batches, max_iter = 1, all-zero syndromes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 63, 65])
def test_ragged_batches_and_edge_cases(B, qopt):
    """Batches that do not fill a 64-slot tile, every third syndrome all zero,
    max_iter 1 and more, bit-packed I/O, flooding and layered, MS and BP:
    equal to the LDS twin. With every prior below 1/2 a zero syndrome
    converges at once; with the general vector (negative LLRs) it need not."""
    H = _code("LP04_0")
    n = H.shape[1]
    syn = np.random.default_rng(B).integers(0, 2, (B, H.shape[0]), dtype=np.uint8)
    syn[::3] = 0
    s = decoders.pack_bits(_dev(syn))
    pos = 10.0 ** np.random.default_rng(81).uniform(-3, np.log10(0.3), n)
    for q in (pos, _general_vector(n, 82)):
        for sched in ("F", "L"):
            layers = _layers(H, sched)
            for algo, mi in (("MS", 1), ("MS", 30), ("BP", 1), ("BP", 12)):
                qopt(vprior_hbm=0, force_hbm=0)
                want = _np(_decode(H, s, mi, algo, layers, q, ehat_bits=True), n)
                qopt(**HBM)
                got = _np(_decode(H, s, mi, algo, layers, q, ehat_bits=True), n)
                _same(got, want, f"{sched} {algo} max_iter {mi}")
                if q is pos:
                    assert (got[1][::3] == 1).all() and not got[0][::3].any()


# ---------------------------------------------------------------------------
# 6. drivers
# ---------------------------------------------------------------------------
def test_simulate_phenomenological_hbm_priors_equals_the_lds_run(qopt, monkeypatch):
    """LP04_0, T = 3, p_data != q: the same seed draws the same shots and the
    decode is bit-exact, so every counter equals the default (LDS twin) run's;
    sliding windows too."""
    Hx, Hz = codes.load_code("LP04_0")
    kw = dict(shots=300, decType="MS", decIterations=20, rngSeed=11, batch_size=128, sampler="device", verbose=False)
    for win in ({}, dict(window=2, commit=1)):
        want = simulator.simulate_phenomenological(Hx, Hz, 0.03, 0.01, 3, **kw, **win)
        assert 0 < want["decSuccessLogical"] < 300
        qopt(force_hbm=1)
        seen = []
        real = decoders.decode_batch

        def spy(H, *a, **k):
            lp, lr = k.get("layer_ptr"), k.get("layer_rows")
            if k.get("prior") is not None:
                seen.append(_lib.vprior_kernel_name(H, lp, lr, k.get("algo", "MS"), 0))
            return real(H, *a, **k)

        with monkeypatch.context() as mp:
            mp.setattr(decoders, "decode_batch", spy)
            got = simulator.simulate_phenomenological(Hx, Hz, 0.03, 0.01, 3, hbm_priors=True, **kw, **win)
        assert seen and all(s.startswith("hbm_tile_vprior_kernel<0, ") for s in seen)
        assert got == want
        assert _lib.get_option("vprior_hbm") == 0
        with pytest.raises(NotImplementedError, match="force_hbm"):   # (without the keyword: still refused)
            simulator.simulate_phenomenological(Hx, Hz, 0.03, 0.01, 3, **kw, **win)
        qopt(force_hbm=0)


def test_simulate_dem_hbm_priors_on_a_33_entry_detector_row():
    """test_vector_prior_refusal_draws_no_shot's model (a detector row of 33
    entries, min-sum): refused without the keyword, and with it the counters
    of a loop over the model's sampler and classes with pm.decode."""
    rng = np.random.default_rng(5)
    H = np.zeros((12, 40), np.uint8)
    H[0, :33] = 1
    for j in range(40):
        H[1 + rng.choice(11, 2, replace=False), j] = 1
    L = np.zeros((1, 40), np.uint8)
    L[0, ::3] = 1
    from qldpcsim_amd import dem as D
    model = D.Dem(H, L, np.linspace(0.001, 0.02, 40))
    shots, seed, mi = 400, 3, 10
    kw = dict(shots=shots, decType="MS", decIterations=mi, rngSeed=seed, sampler="device", verbose=False)
    with pytest.raises(NotImplementedError, match="row degree 33"):
        simulator.simulate_dem(model, **kw)
    got = simulator.simulate_dem(model, hbm_priors=True, batch_size=150, **kw)
    assert _lib.get_option("vprior_hbm") == 0
    key = int(np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0])
    det, obs, _ = dm.sample(model.H, model.L, model.priors, key, 0, shots)
    ehat, it, _, _ = pm.decode("MS", H, det, np.broadcast_to(_llr(model.priors), (shots, 40)), mi)
    c = dm.counters(dm.classify(model.H, model.L, det, obs, ehat)[0], it)
    assert [got[k] for k in simulator.DEM_KEYS] == [c["failures"], c["logical_errors"], c["successes"],
                                                    c["iterations"]]
    assert 0 < got["decSuccess"] <= shots and got["nIterAcc"] > shots
    # OSD after the decode reads out_post as for the scalar HBM kernel
    osd = simulator.simulate_dem(model, hbm_priors=True, OSDorder=0, **kw)
    assert osd["DecFailures"] == 0 and osd["decSuccess"] >= got["decSuccess"]

"""Per-variable priors and the inhomogeneous Pauli channel without a GPU: the
validation of every new C and Python entry point (decided before any HIP
call), the threshold table against the scalar thresholds, the bias weights,
the host sampler, the CLI and the results file's meta."""
import ctypes
import json

import numpy as np
import pytest

from qldpcsim_amd import _lib, codes, decoders, simulator


def _steane():
    Hx, _ = codes.load_code("steane")
    code = _lib.Code(Hx)
    sched = code.schedule(np.array([0, code.m], np.int32), np.arange(code.m, dtype=np.int32))
    return Hx, code, sched


def _prior_create(code, probs, eps=1e-9):
    h = ctypes.c_void_p()
    a = None if probs is None else np.ascontiguousarray(probs, np.float64)
    rc = _lib.lib.qldpc_prior_create(code.handle, _lib.ptr(a), eps, ctypes.byref(h))
    return rc, h


def test_prior_create_validates():
    _, code, _ = _steane()
    n = code.n
    ok = np.full(n, 0.01)
    rc, h = _prior_create(code, ok)
    assert rc == _lib.QLDPC_OK and h.value
    assert _lib.lib.qldpc_prior_destroy(h) == _lib.QLDPC_OK
    assert _lib.lib.qldpc_prior_destroy(None) == _lib.QLDPC_OK
    for bad in (-1e-9, 1.0, 1.5, float("nan"), float("inf")):
        for j in (0, n - 1):
            q = ok.copy()
            q[j] = bad
            rc, h = _prior_create(code, q)
            assert rc == _lib.QLDPC_EINVAL and not h.value, bad
            assert f"p[{j}]".encode() in _lib.lib.qldpc_last_error()
    for fine in (0.0, 0.5, 0.999999):
        q = ok.copy()
        q[3] = fine
        rc, h = _prior_create(code, q)
        assert rc == _lib.QLDPC_OK
        _lib.lib.qldpc_prior_destroy(h)
    # p = 0 with eps = 0 has no finite prior
    q = ok.copy()
    q[2] = 0.0
    assert _prior_create(code, q, eps=0.0)[0] == _lib.QLDPC_EINVAL
    assert _prior_create(code, None)[0] == _lib.QLDPC_EINVAL
    assert _lib.lib.qldpc_prior_create(None, _lib.ptr(ok), 1e-9, ctypes.byref(ctypes.c_void_p())) == _lib.QLDPC_EINVAL
    assert _lib.lib.qldpc_prior_create(code.handle, _lib.ptr(ok), 1e-9, None) == _lib.QLDPC_EINVAL
    # the Python handle: wrong length
    for shape in ((n - 1,), (n + 1,), (1, n)):
        with pytest.raises(ValueError, match="probabilities"):
            _lib.Prior(code, np.full(shape, 0.01), 1e-9)
    # cached per (bytes, eps)
    assert code.prior(ok, 1e-9) is code.prior(ok.copy(), 1e-9)
    assert code.prior(ok, 1e-9) is not code.prior(ok, 1e-8)
    assert code.prior(ok, 1e-9) is not code.prior(ok * 2, 1e-9)


def test_c_decode_entry_points_validate_before_any_hip_call():
    L = _lib.lib
    Hx, code, sched = _steane()
    m, n = code.m, code.n
    pr = code.prior(np.linspace(0.01, 0.2, n), 1e-9)
    syn = np.zeros((2, m), np.uint8)
    e = np.zeros((2, n), np.uint8)
    it = np.zeros(2, np.int32)
    P = _lib.ptr

    def dev(algo=0, sf=0, batch=2, prior=pr.handle, mi=5, ef=0, s=syn, eh=e, i=it, sc=sched.handle, c=code.handle):
        return L.qldpc_decode_device_vprior(c, sc, algo, P(s), sf, batch, prior, mi, 0.75, P(eh), ef, P(i), None,
                                            None, None)

    def host(algo=0, batch=2, prior=pr.handle, mi=5, s=syn, sc=sched.handle):
        return L.qldpc_decode_host_vprior(code.handle, sc, algo, P(s), batch, prior, mi, 0.75, P(e), P(it), None, None)

    EINVAL = _lib.QLDPC_EINVAL
    assert dev(prior=None) == EINVAL and b"prior" in L.qldpc_last_error()
    assert host(prior=None) == EINVAL
    assert dev(sf=2) == EINVAL and dev(ef=7) == EINVAL
    assert dev(algo=2) == EINVAL and dev(algo=3) == EINVAL   # NG / BF take no prior
    assert host(algo=2) == EINVAL and host(algo=3) == EINVAL
    assert dev(batch=-1) == EINVAL and dev(mi=0) == EINVAL and host(batch=-1) == EINVAL and host(mi=0) == EINVAL
    assert dev(s=None) == EINVAL and dev(eh=None) == EINVAL and dev(i=None) == EINVAL
    assert dev(sc=None) == EINVAL and dev(c=None) == EINVAL and host(sc=None) == EINVAL and host(s=None) == EINVAL
    assert dev(batch=0, s=None, eh=None, i=None) == _lib.QLDPC_OK
    assert host(batch=0, s=None) == _lib.QLDPC_OK
    # a handle made for another code, same n
    other = _lib.Code(np.roll(Hx, 1, axis=1))
    foreign = other.prior(np.full(n, 0.01), 1e-9)
    assert dev(prior=foreign.handle) == EINVAL and b"different code" in L.qldpc_last_error()
    assert host(prior=foreign.handle) == EINVAL
    assert dev(prior=foreign.handle, batch=0) == EINVAL
    # force_hbm: refused as unsupported, before the device is looked at
    buf = ctypes.create_string_buffer(64)
    with _lib.options(force_hbm=1):
        assert dev() == _lib.QLDPC_EUNSUP and b"force_hbm" in L.qldpc_last_error()
        assert host() == _lib.QLDPC_EUNSUP
        assert L.qldpc_decode_vprior_kernel_name(code.handle, sched.handle, 0, buf, 64) == _lib.QLDPC_EUNSUP
    assert _lib.get_option("force_hbm") == 0
    # the kernel's name needs no device; the instance is the two-level twin's
    for algo in ("MS", "BP"):
        a = _lib.ALGO[algo]
        assert _lib.vprior_kernel_name(Hx, sched.layer_ptr, sched.layer_rows, algo) == \
            f"decode_vprior_kernel<{a}, false, 0>"
    Hl = codes.load_code("LP04_0")[0]
    lp, lr = simulator.pack_layers(simulator.layerize(Hl), Hl.shape[0])
    assert _lib.vprior_kernel_name(Hl, lp, lr, "MS") == "decode_vprior_kernel<0, true, 7>"
    assert _lib.vprior_kernel_name(Hl, lp, lr, "MS") == \
        _lib.prior_kernel_name(Hl, lp, lr, "MS").replace("decode_prior_kernel", "decode_vprior_kernel")
    assert L.qldpc_decode_vprior_kernel_name(code.handle, sched.handle, 2, buf, 64) == EINVAL
    assert L.qldpc_decode_vprior_kernel_name(code.handle, None, 0, buf, 64) == EINVAL


def test_codes_past_the_lds_kernel_are_refused_before_any_launch():
    """m, n or E > 65535, MS row degree > 32, BP column degree > 128:
    NotImplementedError, no device needed."""
    H = np.zeros((1, 65536), np.uint8)
    H[0, :3] = 1
    with pytest.raises(NotImplementedError, match="65535"):
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), None, 5, prior=np.full(65536, 0.01))
    H = np.ones((1, 40), np.uint8)
    with pytest.raises(NotImplementedError, match="row degree"):
        decoders.decode_batch(H, np.zeros((1, 1), np.uint8), None, 5, prior=np.full(40, 0.01))
    H = np.ones((130, 2), np.uint8)
    with pytest.raises(NotImplementedError, match="column degree"):
        decoders.decode_batch(H, np.zeros((1, 130), np.uint8), None, 5, algo="BP", prior=np.full(2, 0.01))


def test_decode_batch_validates_prior():
    Hx, _ = codes.load_code("steane")
    m, n = Hx.shape
    syn = np.zeros((2, m), np.uint8)
    q = np.full(n, 0.01)
    with pytest.raises(ValueError, match="not both"):
        decoders.decode_batch(Hx, syn, 0.01, 5, prior=q)
    with pytest.raises(ValueError, match="prior_mask"):
        decoders.decode_batch(Hx, syn, None, 5, prior=q, prior_mask=np.zeros((2, n), np.uint8), p_masked=0.4)
    with pytest.raises(ValueError, match="relay"):
        decoders.decode_batch(Hx, syn, None, 5, algo="RELAY", prior=q,
                              relay=decoders.RelayConfig([5], np.zeros((1, n)), 1))
    for algo in ("NG", "BF"):
        with pytest.raises(ValueError, match="hard-decision"):
            decoders.decode_batch(Hx, syn, None, 5, algo=algo, prior=q)
    for bad in (q[:-1], np.append(q, 0.01), q.reshape(1, n)):
        with pytest.raises(ValueError, match="one per column"):
            decoders.decode_batch(Hx, syn, None, 5, prior=bad)
    for bad in (-0.1, 1.0, float("nan")):
        b = q.copy()
        b[4] = bad
        with pytest.raises(ValueError, match=r"p\[4\]"):
            decoders.decode_batch(Hx, syn, None, 5, prior=b)
        with pytest.raises(ValueError, match=r"p\[4\]"):
            decoders.MS_decoder(Hx, syn[0], b)
    with _lib.options(force_hbm=1):
        with pytest.raises(NotImplementedError, match="force_hbm"):
            decoders.decode_batch(Hx, syn, None, 5, prior=q)


def test_channel_table_equals_the_scalar_thresholds():
    """px = py = pz = p/3: q + q is exact and 2q + q rounds as 3q, so the table
    is qldpc_channel_thresholds(p), also where 3 (p/3) != p."""
    rng = np.random.default_rng(1)
    ps = np.concatenate([[0.0, 1.0, 0.1, 0.3, 0.7, 1e-12, 2.0 ** -33, 3 * 2.0 ** -32, 1 - 2.0 ** -53],
                         rng.random(2000), 10.0 ** rng.uniform(-12, 0, 2000)])
    assert (3 * (ps / 3) != ps).any()
    q = ps / 3
    T = _lib.channel_table(q, q, q)
    t = [ctypes.c_uint64() for _ in range(3)]
    for i, p in enumerate(ps):
        _lib.check(_lib.lib.qldpc_channel_thresholds(float(p), *(ctypes.byref(x) for x in t)))
        assert [int(T[k, i]) for k in range(3)] == [x.value for x in t], p
    assert int(T[2, 1]) == 1 << 32                               # p = 1: the table holds 2^32
    # the definition, in float64
    px, py, pz = rng.random(50) * 0.3, rng.random(50) * 0.3, rng.random(50) * 0.3
    T = _lib.channel_table(px, py, pz)
    two32 = 4294967296.0
    assert np.array_equal(T[0], np.minimum(two32, np.floor(px * two32)).astype(np.uint64))
    assert np.array_equal(T[1], np.minimum(two32, np.floor((px + py) * two32)).astype(np.uint64))
    assert np.array_equal(T[2], np.minimum(two32, np.floor(((px + py) + pz) * two32)).astype(np.uint64))
    assert int(_lib.channel_table([1.0], [0.0], [0.0])[0, 0]) == 1 << 32


def test_channel_entry_points_validate():
    L = _lib.lib
    Hx, Hz = codes.load_code("steane")
    cx, cz = _lib.Code(Hx), _lib.Code(Hz)
    n = cx.n
    ok = np.full(n, 0.1)
    for k in range(3):
        for bad in (-1e-12, float("nan"), 0.81):                 # 0.81 + 0.1 + 0.1 > 1
            a = [ok.copy(), ok.copy(), ok.copy()]
            a[k][n - 1] = bad
            with pytest.raises(ValueError, match=f"qubit {n - 1}"):
                _lib.channel_table(*a)
            with pytest.raises(ValueError, match=f"qubit {n - 1}"):
                _lib.Channel(cx, cz, *a)
    with pytest.raises(ValueError, match="one per qubit"):
        _lib.Channel(cx, cz, ok[:-1], ok[:-1], ok[:-1])
    with pytest.raises(ValueError, match="same length"):
        _lib.channel_table(ok, ok[:-1], ok)
    other = _lib.Code(np.ones((2, n + 1), np.uint8))
    with pytest.raises(ValueError, match="same number of columns"):
        _lib.Channel(cx, other, ok, ok, ok)
    h = ctypes.c_void_p()
    P = _lib.ptr
    assert L.qldpc_channel_create(None, cz.handle, P(ok), P(ok), P(ok), ctypes.byref(h)) == _lib.QLDPC_EINVAL
    assert L.qldpc_channel_create(cx.handle, cz.handle, None, P(ok), P(ok), ctypes.byref(h)) == _lib.QLDPC_EINVAL
    big = _lib.Code(np.ones((1, 4097), np.uint8))
    q = np.full(4097, 0.1)
    assert L.qldpc_channel_create(big.handle, big.handle, _lib.ptr(q), _lib.ptr(q), _lib.ptr(q),
                                  ctypes.byref(h)) == _lib.QLDPC_EUNSUP
    ch = _lib.Channel(cx, cz, ok, ok, ok)
    w = np.zeros((2, 1), np.uint64)
    s = np.zeros((2, 3), np.uint8)

    def sample(c=ch.handle, batch=2, ex=w, ez=w, sz=s, sx=s, fmt=0):
        return L.qldpc_channel_sample_vec(c, 1, 0, batch, P(ex), P(ez), P(sz), P(sx), fmt, None)

    assert sample(c=None) == _lib.QLDPC_EINVAL
    assert sample(fmt=2) == _lib.QLDPC_EINVAL
    assert sample(batch=-1) == _lib.QLDPC_EINVAL
    assert sample(ex=None) == _lib.QLDPC_EINVAL and sample(sz=None) == _lib.QLDPC_EINVAL
    assert sample(batch=0, ex=None, ez=None, sz=None, sx=None) == _lib.QLDPC_OK
    assert L.qldpc_channel_destroy(None) == _lib.QLDPC_OK


def test_bias_weights():
    for eta in (0.0, 0.5, 1.0, 10.0, 1e6):
        w = simulator.bias_weights(eta)
        assert w.shape == (3,) and w[0] == w[1] == 1 / (2 * (eta + 1)) and w[2] == eta / (eta + 1)
        assert abs(w.sum() - 1) < 1e-15
        if eta > 0:
            assert abs(w[2] / (w[0] + w[1]) - eta) < 1e-9 * eta
    assert np.allclose(simulator.bias_weights(0.5), 1 / 3, rtol=0, atol=1e-16)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bias"):
            simulator.bias_weights(bad)


def test_simulate_p_validates_channel_weights():
    Hx, Hz = codes.load_code("steane")
    n = Hx.shape[1]
    kw = dict(shots=4, sampler="host", verbose=False)
    with pytest.raises(ValueError, match="non-negative"):
        simulator.simulate_p(Hx, Hz, 0.05, channel_weights=[0.5, -0.1, 0.5], **kw)
    with pytest.raises(ValueError, match="non-negative"):
        simulator.simulate_p(Hx, Hz, 0.05, channel_weights=[0.5, float("nan"), 0.5], **kw)
    for shape in ((2,), (3, n - 1), (n, 3), (1, 3, n)):
        with pytest.raises(ValueError, match="shape"):
            simulator.simulate_p(Hx, Hz, 0.05, channel_weights=np.full(shape, 0.1), **kw)
    w = np.full((3, n), 1 / 3)
    w[2, 5] = 2.0
    with pytest.raises(ValueError, match="<= 1"):
        simulator.simulate_p(Hx, Hz, 0.5, channel_weights=w, **kw)
    with pytest.raises(ValueError, match="<= 1"):
        simulator.simulate_p(Hx, Hz, 0.5, channel_weights=[1.0, 1.0, 1.0], **kw)
    with pytest.raises(ValueError, match="correlated"):
        simulator.simulate_p(Hx, Hz, 0.05, channel_weights=[1 / 3] * 3, correlated="XZ", **kw)
    w = np.full((3, n), 1 / 3)
    w[0, 2] = 0.5
    with pytest.raises(ValueError, match="RELAY"):
        simulator.simulate_p(Hx, Hz, 0.05, channel_weights=w, decType="RELAY", **kw)
    # every p of a sweep is checked before the first point runs
    with pytest.raises(ValueError, match="<= 1"):
        simulator.channel_probs(0.6, [1.0, 0.5, 0.5], n)
    pr = simulator.channel_probs(0.3, [0.2, 0.3, 0.5], n)
    assert pr.shape == (3, n) and np.array_equal(pr[:, 0], 0.3 * np.array([0.2, 0.3, 0.5]))


def test_half_priors_pick_the_scalar_entry_point_for_uniform_marginals():
    q = 0.05 * (np.full(9, 0.2) + np.full(9, 0.3))
    assert simulator._half_prior(q, False) == (float(q[0]), {})
    q2 = q.copy()
    q2[3] *= 2
    p, kw = simulator._half_prior(q2, False)
    assert p is None and np.array_equal(kw["prior"], q2)
    assert simulator._half_prior(q2, True) == (0.0, {})          # NG / BF take no prior


def test_host_sampler_syndromes_and_frequencies():
    """sy = H e mod 2, and each qubit's X / Y / Z frequencies lie within 5
    binomial standard deviations of its probabilities at the shot count used
    (3 n = 525 comparisons: a false alarm has probability < 1e-3)."""
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    rng = np.random.default_rng(7)
    w = rng.random((3, n)) + 0.05
    w[:, :5] = [[0.0], [0.0], [1.0]]                             # pure Z
    w[:, 5:8] = 0.0                                              # no noise
    p = 0.3 / w.sum(0).max()
    probs = simulator.channel_probs(p, w, n)
    shots = 20000
    sy_z, sy_x, errX, errZ = simulator.sample_channel_vec(Hx, Hz, probs, shots, np.random.default_rng(3))
    assert sy_z.dtype == sy_x.dtype == errX.dtype == errZ.dtype == np.uint8
    assert np.array_equal(sy_z, (errX.astype(np.int64) @ Hz.T.astype(np.int64)) % 2)
    assert np.array_equal(sy_x, (errZ.astype(np.int64) @ Hx.T.astype(np.int64)) % 2)
    X = (errX == 1) & (errZ == 0)
    Y = (errX == 1) & (errZ == 1)
    Z = (errX == 0) & (errZ == 1)
    for got, want in ((X, probs[0]), (Y, probs[1]), (Z, probs[2])):
        sd = np.sqrt(want * (1 - want) / shots)
        assert (np.abs(got.mean(0) - want) <= 5 * sd + 2.0 ** -32).all()
    assert not errX[:, :8].any() and not errZ[:, 5:8].any()


def test_cli_parses_bias_and_weights(tmp_path, monkeypatch):
    Hx, Hz = codes.load_code("steane")
    n = Hx.shape[1]
    fx, fz, fw = str(tmp_path / "hx.npy"), str(tmp_path / "hz.npy"), str(tmp_path / "w.npy")
    np.save(fx, Hx)
    np.save(fz, Hz)
    w = np.full((3, n), 0.25)
    w[2, 1] = 0.5
    np.save(fw, w)
    seen = []
    monkeypatch.setattr(simulator, "simulate", lambda **kw: seen.append(kw))
    base = ["--Hx", fx, "--Hz", fz, "--p", "0.1"]
    simulator.main(base)
    assert "bias" not in seen[-1] and "channel_weights" not in seen[-1]
    simulator.main(base + ["--bias", "10"])
    assert seen[-1]["bias"] == 10.0 and "channel_weights" not in seen[-1]
    simulator.main(base + ["--channel-weights", fw])
    assert np.array_equal(seen[-1]["channel_weights"], w) and "bias" not in seen[-1]
    with pytest.raises(SystemExit):
        simulator.main(base + ["--bias", "10", "--channel-weights", fw])
    with pytest.raises(SystemExit):
        simulator.main(base + ["--bias", "x"])


def test_results_file_meta_holds_the_channel(tmp_path, monkeypatch):
    Hx, Hz = codes.load_code("steane")
    n = Hx.shape[1]
    fx, fz = str(tmp_path / "hx.npy"), str(tmp_path / "hz.npy")
    np.save(fx, Hx)
    np.save(fz, Hz)
    calls = []

    def fake(Hx, Hz, p, shots, **kw):
        calls.append(kw)
        return {"DecFailures_X": 0, "DecFailures_Z": 0, "decSuccessExact": shots, "decSuccessDegen": 0,
                "Avg_number_of_iterations_X": 1.0, "Avg_number_of_iterations_Z": 1.0}

    monkeypatch.setattr(simulator, "simulate_p", fake)
    rf = str(tmp_path / "res.json")
    run = lambda f=rf, **kw: simulator.simulate(fx, fz, [0.01], shots=4, verbose=False, sampler="host",  # noqa: E731
                                                resultsFile=f, **kw)
    run(bias=10)
    meta = json.load(open(rf))["meta"]
    assert meta["bias"] == 10.0 and "channel_weights" not in meta
    assert np.array_equal(calls[-1]["channel_weights"], simulator.bias_weights(10))
    run(bias=10)                                                 # same channel: resumed
    assert len(calls) == 1
    w = np.full((3, n), 0.25)
    for other in (dict(), dict(bias=5), dict(channel_weights=w)):
        with pytest.raises(ValueError, match="different run"):
            run(**other)
    rf2 = str(tmp_path / "w.json")
    run(rf2, channel_weights=w)
    meta = json.load(open(rf2))["meta"]
    assert meta["channel_weights"]["shape"] == [3, n] and len(meta["channel_weights"]["sha256"]) == 64
    w2 = w.copy()
    w2[0, 0] = 0.26
    with pytest.raises(ValueError, match="different run"):
        run(rf2, channel_weights=w2)
    with pytest.raises(ValueError, match="not both"):
        run(str(tmp_path / "x.json"), bias=1, channel_weights=w)
    with pytest.raises(ValueError, match="<= 1"):
        simulator.simulate(fx, fz, [0.01, 0.9], shots=4, verbose=False, sampler="host", channel_weights=w * 2)
    rf3 = str(tmp_path / "plain.json")
    run(rf3)
    meta = json.load(open(rf3))["meta"]
    assert "bias" not in meta and "channel_weights" not in meta and "channel_weights" not in calls[-1]

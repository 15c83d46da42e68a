"""The hard-decision decoders on the device (ng_kernel, bf_kernel): equal to the
reference's recorded outputs (tests/golden/hard/) and, on fresh inputs, to the
test-side model (tests/hard_model.py) — estimates, counts and flags, in both
wire formats, under the work queue and the static stride, through the
single-shot shims and through simulate_p."""
import functools

import numpy as np
import pytest

import hard_model as hm

pytestmark = pytest.mark.gpu

CASES = hm.golden_cases()


def _decode(H, syn, algo, max_iter=50, bits=False, out=None):
    """(ehat uint8 [B, n], iters, converged) from decode_batch on cuda:0."""
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(np.ascontiguousarray(syn, dtype=np.uint8), device="cuda:0")
    if bits:
        s = decoders.pack_bits(s)
    r = decoders.decode_batch(H, s, 0.3, max_iter, algo=algo, beta=0.1, eps=0.5, layers=[np.arange(1)],
                              ehat_bits=bits, out=out)
    assert r.post is None
    e = decoders.unpack_bits(r.ehat, H.shape[1]) if bits else r.ehat
    if bits:                                             # bits past n stay zero
        assert torch.equal(decoders.pack_bits(e), r.ehat)
    return e.cpu().numpy(), r.iters.cpu().numpy(), r.converged.cpu().numpy(), r


def _model(H, syn, algo, max_iter=50):
    if algo == "BF":
        return hm.bf_batch(H, syn, max_iter)
    e, it, info = hm.ng_batch(H, syn)
    return e, it, info["conv"]


def _same(got, want):
    assert np.array_equal(got[1], want[1])               # counts
    assert np.array_equal(got[2], want[2])               # the reference's own stop condition
    assert np.array_equal(got[0], want[0])               # estimates


@pytest.mark.parametrize("bits", [False, True], ids=["bytes", "bits"])
@pytest.mark.parametrize("c,a,H", CASES, ids=[hm.case_id(c) for c, _, _ in CASES])
def test_every_fixture_case_equals_the_reference(c, a, H, bits):
    """Steane / Shor: n < 64, m < 64 (tail lanes on both sides); LP118_2:
    m > 4 x 64; synthetic: zero row, zero column, a row of degree 100."""
    got = _decode(H, a["syn"], c["algo"], c["max_iter"] or 50, bits)
    _same(got, (a["ehat"], a["iters"], a["conv"].astype(bool)))


@pytest.mark.parametrize("code", ["steane", "shor", "LP04_0", "LP118_2", "synthetic"])
def test_single_shot_shims_return_the_reference_types(code):
    from qldpcsim_amd import decoders
    for c, a, H in CASES:
        if c["code"] != code or c["max_iter"] not in (0, 50, 3):
            continue
        for k in (0, 1, a["syn"].shape[0] // 2, a["syn"].shape[0] - 1):
            syn = a["syn"][k].astype(np.int64)
            if c["algo"] == "NG":
                e, it = decoders.NG_decoder(H, syn)
                assert e.dtype == np.int8
            else:
                e, it = decoders.BF_decoder(H, syn, c["max_iter"])
                assert e.dtype == np.bool_
            assert type(it) is int and it == a["iters"][k]
            assert e.shape == (H.shape[1],) and np.array_equal(e.astype(np.uint8), a["ehat"][k])
    if code == "steane":                                 # the default max_iter is the reference's 50
        c, a, H = next(x for x in CASES if x[0]["code"] == "steane" and x[0]["algo"] == "BF")
        k = int(np.flatnonzero(a["conv"] == 0)[0])
        assert decoders.BF_decoder(H, a["syn"][k])[1] == 50


@functools.lru_cache(maxsize=None)
def _fresh(code, algo):
    """Fresh random + channel syndromes and the model's outputs, computed once."""
    from qldpcsim_amd import codes
    H = hm.synthetic_matrix() if code == "synthetic" else codes.load_code(code)[1]
    m, n = H.shape
    B = 4096 if algo == "BF" else 512
    rng = np.random.default_rng(20251226 + m)
    syn = rng.integers(0, 2, (B, m), dtype=np.uint8)
    err = (rng.random((B // 2, n)) < np.linspace(0.002, 0.08, B // 2)[:, None]).astype(np.int64)
    syn[B // 2:] = (err @ (H % 2).T.astype(np.int64)) % 2
    return H, syn, _model(H, syn, algo)


@pytest.mark.parametrize("bits", [False, True], ids=["bytes", "bits"])
@pytest.mark.parametrize("code", ["LP118_0", "synthetic"])
@pytest.mark.parametrize("algo", ["BF", "NG"])
def test_fresh_inputs_equal_the_model(algo, code, bits):
    H, syn, want = _fresh(code, algo)
    _same(_decode(H, syn, algo, 50, bits), want)
    if algo == "NG":                                     # the batch spans 0 .. 2n steps
        assert want[1].min() < 8 and want[1].max() == 2 * H.shape[1]


def test_host_buffer_path_equals_the_device_path():
    from qldpcsim_amd import decoders
    for algo in ("BF", "NG"):
        H, syn, want = _fresh("synthetic", algo)
        r = decoders.decode_batch(H, syn[:300], 0.0, 50, algo=algo)
        assert isinstance(r.ehat, np.ndarray) and r.post is None
        _same((r.ehat, r.iters, r.converged), tuple(w[:300] for w in want))
        r = decoders.decode_batch(H, syn[:100], 0.0, 50, algo=algo)      # a smaller batch in the same workspace
        _same((r.ehat, r.iters, r.converged), tuple(w[:100] for w in want))


def test_queue_under_load_bf_steane():
    """2^16 half-shots, far more than the resident waves."""
    from qldpcsim_amd import codes
    H = codes.load_code("steane")[1]
    syn = np.random.default_rng(3).integers(0, 2, (1 << 16, H.shape[0]), dtype=np.uint8)
    _same(_decode(H, syn, "BF", 50, True), hm.bf_batch(H, syn, 50))


@pytest.mark.parametrize("static", [0, 1])
def test_ng_mixed_step_counts_static_and_queued_with_reused_out(static, qopt):
    """Zero-step and 2n-step shots in one batch; the same `out` buffers serve
    two launches, the second with the shots reversed."""
    import torch
    from qldpcsim_amd import codes, decoders
    qopt(static_sched=static)
    H = codes.load_code("LP04_0")[1]
    m, n = H.shape
    rng = np.random.default_rng(9)
    syn = rng.integers(0, 2, (6000, m), dtype=np.uint8)
    syn[rng.random(6000) < 0.5] = 0
    want = _model(H, syn, "NG")
    assert (want[1] == 0).sum() > 2000 and (want[1] == 2 * n).sum() > 2000
    out = decoders.DecodeResult(torch.full((6000, (n + 63) // 64), -1, dtype=torch.int64, device="cuda:0"),
                                torch.full((6000,), -1, dtype=torch.int32, device="cuda:0"), None,
                                torch.full((6000,), -1, dtype=torch.int32, device="cuda:0"))
    got = _decode(H, syn, "NG", bits=True, out=out)
    assert got[3].ehat is out.ehat and got[3].iters is out.iters
    _same(got, want)
    _same(_decode(H, syn[::-1], "NG", bits=True, out=out), tuple(w[::-1] for w in want))
    with pytest.raises(ValueError, match="out buffers"):
        _decode(H, syn[:10], "NG", bits=True, out=out)


def test_kernel_names_and_launch_info():
    from qldpcsim_amd import _lib, codes
    H = codes.load_code("LP118_0")[1]
    for algo, name in (("NG", "ng_kernel"), ("BF", "bf_kernel")):
        assert _lib.kernel_name(H, None, None, algo, 0) == name
        w, b, lds = _lib.launch_info(H, None, None, algo, 0)
        assert 1 <= w <= 8 and b >= 1 and 0 < lds <= 160 * 1024


def test_codes_past_the_16_bit_tables_are_refused_before_any_launch():
    import torch
    from qldpcsim_amd import decoders
    H = np.zeros((1, 65536), np.uint8)
    H[0, :3] = 1
    syn = torch.zeros((4, 1), dtype=torch.uint8, device="cuda:0")
    for algo in ("NG", "BF"):
        with pytest.raises(NotImplementedError, match="65535"):
            decoders.decode_batch(H, syn, 0.0, 50, algo=algo)


def _model_counters(Hx, Hz, decType, sy_z, sy_x, errX, errZ):
    """The reference's per-shot loop (simulator.py:270-303) on the model: both
    decoders get (H, syndrome) alone, BF its default 50 iterations; failures
    use the true parity."""
    (eX, itX, _), (eZ, itZ, _) = _model(Hz, sy_z, decType), _model(Hx, sy_x, decType)
    shots = sy_z.shape[0]
    want = dict(DecFailures_X=0, DecFailures_Z=0, decSuccessExact=0, decSuccessDegen=0)
    for k in range(shots):
        if np.array_equal(errX[k], eX[k]) and np.array_equal(errZ[k], eZ[k]):
            want["decSuccessExact"] += 1
        elif ((Hz.astype(int) @ (errX[k].astype(int) ^ eX[k])) == 0).all() and \
                ((Hx.astype(int) @ (errZ[k].astype(int) ^ eZ[k])) == 0).all():
            want["decSuccessDegen"] += 1
        want["DecFailures_X"] += int(not np.array_equal(sy_z[k], (Hz.astype(int) @ eX[k]) % 2))
        want["DecFailures_Z"] += int(not np.array_equal(sy_x[k], (Hx.astype(int) @ eZ[k]) % 2))
    want["Avg_number_of_iterations_X"] = itX.sum() / float(shots)
    want["Avg_number_of_iterations_Z"] = itZ.sum() / float(shots)
    return want


@pytest.mark.parametrize("decType", ["NG", "BF"])
def test_simulate_p_counters_equal_the_reference_loop_on_the_model(decType):
    """LP04_0, 330 shots in batches of 100 at p = 0.03: the device pipeline,
    the host path fed the same shots, and another batch size all give the
    counters of the reference's loop; decIterations and OSDorder are ignored."""
    import torch
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    p, shots, seed = 0.03, 330, 11
    got = simulator.simulate_p(Hx, Hz, p, shots=shots, decType=decType, decIterations=7, decSchedule="L",
                               OSDorder=0, rngSeed=seed, batch_size=100, sampler="device", verbose=False)
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), key)
    sy_z, sy_x, ewX, ewZ = ch.sample(p, shots)
    sy_z, sy_x = sy_z.cpu().numpy(), sy_x.cpu().numpy()
    errX, errZ = ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy()
    want = _model_counters(Hx, Hz, decType, sy_z, sy_x, errX, errZ)
    assert got == want
    assert want["DecFailures_X"] + want["DecFailures_Z"] > 0 and want["decSuccessExact"] > 0
    host = simulator.simulate_p(Hx, Hz, p, shots=shots, decType=decType, decIterations=3, OSDorder=2, rngSeed=seed,
                                batch_size=100, sampler="host", samples=(sy_z, sy_x, errX, errZ), verbose=False)
    assert host == want
    other = simulator.simulate_p(Hx, Hz, p, shots=shots, decType=decType, rngSeed=seed, batch_size=77,
                                 sampler="device", verbose=False)
    assert other == want
    with pytest.raises(ValueError):
        simulator.simulate_p(Hx, Hz, p, shots=4, decType=decType, decSchedule="Q", verbose=False)

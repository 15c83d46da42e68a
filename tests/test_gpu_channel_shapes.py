"""The shot source and the outcome counters on the GPU at the word and
kernel-selection edges (tests/channel_shape_codes.py): channel_sample_kernel,
channel_sample_vec_kernel, count_outcomes_kernel, count_logical_kernel and the
long-row trips of phenom_sample_kernel / phenom_count_kernel. Each test first
asserts the instance the launcher picks (qldpc_channel_kernel_name,
qldpc_phenom_kernel_name), then compares with the oracle stream, the models of
tests/logical_model.py and tests/phenom_model.py and the reference's per-shot
loop. Every comparison is integer equality. The inputs are pinned without a
GPU by tests/test_channel_shape_codes.py; the phenomenological sampler, counter
and window kernels run the new halves through the widened SHAPES /
KERNEL_CASES of test_gpu_phenom.py and test_gpu_window.py."""
import numpy as np
import pytest

import channel_shape_codes as csc
import logical_model as lm
import phenom_model as pm

pytestmark = pytest.mark.gpu

WHAT = ("sy_z", "sy_x", "errX", "errZ")


def _dev():
    import torch
    return torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy()


def _T(a):
    import torch
    return torch.as_tensor(np.array(a, order="C"), device=_dev())          # (a copy: the batches are read-only)


def _channel(name, shot0=csc.SHOT0):
    from qldpcsim_amd import simulator
    return simulator.DeviceChannel(*csc.pair(name), _dev(), csc.SEED, shot0)


def _kernel(name, kind, aligned=True, lds=False):
    from qldpcsim_amd import _lib
    return _lib.channel_kernel_name(*csc.pair(name), kind, aligned, lds, device_index=0)


def _check_shots(name, got, want, bits):
    """One sampler call (device tensors) against unpacked uint8 arrays: the
    syndromes in their format and the error words, padding bits included."""
    c = csc.CASES[name]
    for g, w, what, k in zip(got, want, WHAT, (c["mz"], c["mx"], c["n"], c["n"])):
        if what.startswith("err") or bits:
            words = _np(g).view(np.uint64)
            assert words.shape == (w.shape[0], (k + 63) // 64), what
            assert np.array_equal(words, pm.pack_words(w)), (name, what, "words, padding bits zero", bits)
            if k % 64:
                assert not (words[:, -1] >> np.uint64(k % 64)).any(), (name, what, "padding bits")
        else:
            assert np.array_equal(_np(g), w), (name, what, bits)


@pytest.mark.parametrize("name", csc.IDS)
def test_scalar_sampler_equals_the_oracle_stream(name):
    """257 shots (w64: 65) from shot 2^32 - 100, so the shot counter's low word
    wraps: both syndrome formats, errX and errZ against the oracle stream, one
    call and the same shots in two; p = 1 and p = 0 on q8a and w64."""
    import torch
    from oracle import oracle
    assert _kernel(name, "sample") == csc.kernel(name, "sample")
    Hx, Hz = csc.pair(name)
    c = csc.CASES[name]
    B = c["shots"]
    first = 100 if B == 257 else 30
    want = oracle.channel_sample(Hx, Hz, csc.P, csc.SEED, csc.SHOT0, B)
    assert all(w.any() for w in want)
    # a length that is a multiple of 64 has no padding bits: the last word is used up to bit 63
    assert all(w[:, -1].any() for w, k in zip(want, (c["mz"], c["mx"], c["n"], c["n"])) if k % 64 == 0)
    for bits in (False, True):
        ch = _channel(name)
        got = ch.sample(csc.P, B, bits=bits)
        assert got[0].dtype == (torch.int64 if bits else torch.uint8) and ch.shot == csc.SHOT0 + B
        _check_shots(name, got, want, bits)
        ch2 = _channel(name)
        a, b = ch2.sample(csc.P, first, bits=bits), ch2.sample(csc.P, B - first, bits=bits)
        for x, y, g, what in zip(a, b, got, WHAT):
            assert torch.equal(torch.cat([x, y]), g), (name, what, "split", bits)
    if name in ("q8a", "w64"):
        for p in (1.0, 0.0):
            want = oracle.channel_sample(Hx, Hz, p, csc.SEED, csc.SHOT0, B)
            assert (want[2] | want[3]).all() == (p == 1.0) and (want[2] | want[3]).any() == (p == 1.0)
            for bits in (False, True):
                _check_shots(name, _channel(name).sample(p, B, bits=bits), want, bits)


@pytest.mark.parametrize("name", csc.VEC_CASES)
def test_vector_sampler_equals_the_model_stream(name):
    """set_probs with per-qubit thresholds of 0 and 2^32, a qubit with
    px + py + pz = 1 and generic rows against the oracle stream column by
    column; a depolarizing table gives the scalar sampler's tensors."""
    import torch
    from test_gpu_vprior import _expected_shots
    assert _kernel(name, "sample_vec") == csc.kernel(name, "sample_vec")
    Hx, Hz = csc.pair(name)
    n, B = csc.CASES[name]["n"], 257
    probs = csc.vec_table(name)
    *want, triples = _expected_shots(Hx, Hz, probs, csc.SEED, csc.SHOT0, B)
    assert triples == 9
    X, Z = want[2].astype(bool), want[3].astype(bool)
    assert (X | Z)[:, probs.sum(0) == 1.0].all() and not (X | Z)[:, probs.sum(0) == 0.0].any()
    for pr, ev in ((probs[0], X & ~Z), (probs[1], X & Z), (probs[2], ~X & Z)):
        assert not ev[:, pr == 0].any() and ev[:, pr == 1.0].all() and ev[:, (pr > 0) & (pr < 1)].any()
    for bits in (False, True):
        ch = _channel(name)
        ch.set_probs(probs)
        _check_shots(name, ch.sample(None, B, bits=bits), want, bits)
        ch = _channel(name)
        ch.set_probs(probs)
        a, b = ch.sample(None, 100, bits=bits), ch.sample(None, 157, bits=bits)
        ch = _channel(name)
        ch.set_probs(probs)
        for x, y, g, what in zip(a, b, ch.sample(None, B, bits=bits), WHAT):
            assert torch.equal(torch.cat([x, y]), g), (name, what, "split", bits)
        ch = _channel(name)
        ch.set_probs(np.full((3, n), csc.P / 3))
        for g, w, what in zip(ch.sample(None, B, bits=bits), _channel(name).sample(csc.P, B, bits=bits), WHAT):
            assert torch.equal(g, w), (name, what, "depolarizing table", bits)


# ---------------------------------------------------------------------------
# counters
# ---------------------------------------------------------------------------
def _device_batch(name):
    """The case's crafted batch on the device: the shots are drawn there and
    must be the oracle's, on which logical_model.craft built the estimates."""
    from qldpcsim_amd import decoders
    d = csc.batch(name)
    ch = _channel(name)
    sy_z, sy_x, ewX, ewZ = ch.sample(csc.P, 257)
    for g, w, what in zip((sy_z, sy_x, ch.unpack(ewX), ch.unpack(ewZ)), (d["sy_z"], d["sy_x"], d["errX"], d["errZ"]),
                          WHAT):
        assert np.array_equal(_np(g), w), (name, what, "device-drawn shots")
    teX, teZ = _T(d["eX"]), _T(d["eZ"])
    return dict(d, ch=ch, err=(ewX, ewZ), it=(_T(d["itX"]), _T(d["itZ"])),
                syn={"bytes": (sy_z, sy_x), "bits": (decoders.pack_bits(sy_z), decoders.pack_bits(sy_x))},
                est={"bytes": (teX, teZ), "bits": (decoders.pack_bits(teX), decoders.pack_bits(teZ))})


def _check_logical(d, out, where):
    """Classes, flip words with their padding bits and all nine counters of
    one count_logical_device(want_shots=True) call against the model."""
    from qldpcsim_amd import simulator
    acc, cX, cZ, fX, fZ = (_np(t) for t in out)
    B, k = cX.shape[0], d["k"]
    assert np.array_equal(cX, d["cX"]) and np.array_equal(cZ, d["cZ"]), ("classes", where)
    fX, fZ = fX.view(np.uint64), fZ.view(np.uint64)
    assert fX.shape == fZ.shape == (B, (k + 63) // 64), where
    assert np.array_equal(fX, d["flipX"]) and np.array_equal(fZ, d["flipZ"]), ("flip words", where)
    if k % 64:
        pad = ~np.uint64((1 << (k % 64)) - 1)
        assert not (fX[:, -1] & pad).any() and not (fZ[:, -1] & pad).any(), ("flip padding bits", where)
    c = dict(zip(simulator.COUNTER_KEYS + simulator.LOGICAL_KEYS, (int(v) for v in acc)))
    assert c == d["want"], where
    lm.check_invariants(c, B)


@pytest.mark.parametrize("name", csc.IDS)
def test_counters_equal_the_model_and_the_reference_loop(name, qopt):
    """count_logical_kernel in both residencies and the automatic one and
    count_outcomes_kernel, in all four syndrome x estimate formats, on the
    crafted batch of 257: classes, flip words and nine counters against the
    model, six counters against the reference's per-shot loop."""
    from qldpcsim_amd import simulator
    d = _device_batch(name)
    csc.check_batch(d)
    ch = d["ch"]
    ref = csc.reference_counters(name)
    assert _kernel(name, "count") == csc.kernel(name, "count")
    for mode in (1, 2, 0):
        lds = csc.tabs_lds(name, mode)
        qopt(logical_tabs=mode)
        if lds is None:                                     # the tables do not fit: staging them is refused
            with pytest.raises(NotImplementedError, match="LDS"):
                ch.count_logical_device(*d["syn"]["bytes"], *d["err"], *d["est"]["bytes"], *d["it"])
            continue
        assert _kernel(name, "count_logical", True, lds) == csc.kernel(name, "count_logical", True, lds)
        for syn in ("bytes", "bits"):
            for est in ("bytes", "bits"):
                args = (*d["syn"][syn], *d["err"], *d["est"][est], *d["it"])
                _check_logical(d, ch.count_logical_device(*args, want_shots=True), (name, mode, syn, est))
                assert ch.count_logical(*args) == d["want"], (name, mode, syn, est)
                if mode == 0:
                    six = ch.count(*args)
                    assert six == ref == {k: d["want"][k] for k in simulator.COUNTER_KEYS}, (name, syn, est)


def _odd_base(t):
    """A contiguous copy of a uint8 [B, n] tensor one byte into a larger
    buffer: rows of n % 4 == 0 bytes at an odd base address."""
    import torch
    buf = torch.zeros(t.numel() + 8, dtype=torch.uint8, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 4 == 1 and t.data_ptr() % 4 == 0
    return v


@pytest.mark.parametrize("name", csc.MISALIGNED)
def test_misaligned_byte_estimates_take_the_byte_path(name, qopt):
    """n % 4 == 0, so aligned byte estimates are read by 32-bit loads; with
    either estimate at an odd base the launcher must pick the <.., false>
    instance, and the counters must be those of the aligned tensors."""
    from qldpcsim_amd import simulator
    d = _device_batch(name)
    ch = d["ch"]
    assert csc.CASES[name]["n"] % 4 == 0
    deg = csc.CASES[name]["udeg"]
    assert _kernel(name, "count", True) == f"count_outcomes_kernel<{deg}, true>"
    assert _kernel(name, "count", False) == f"count_outcomes_kernel<{deg}, false>"
    eX, eZ = d["est"]["bytes"]
    oX, oZ = _odd_base(eX), _odd_base(eZ)
    six = {k: d["want"][k] for k in simulator.COUNTER_KEYS}
    for mode in (1, 2):
        qopt(logical_tabs=mode)
        lds = "true" if mode == 1 else "false"
        assert _kernel(name, "count_logical", False, mode == 1) == f"count_logical_kernel<{deg}, false, {lds}>"
        assert _kernel(name, "count_logical", True, mode == 1) == f"count_logical_kernel<{deg}, true, {lds}>"
        for syn in ("bytes", "bits"):
            for x, z in ((oX, oZ), (oX, eZ), (eX, oZ)):
                args = (*d["syn"][syn], *d["err"], x, z, *d["it"])
                _check_logical(d, ch.count_logical_device(*args, want_shots=True), (name, mode, syn, "odd base"))
                assert ch.count(*args) == six == csc.reference_counters(name), (name, syn, "odd base")


def test_one_shape_past_the_grid():
    """q7v with more shots than one launch's waves (8 workgroups per CU, four
    waves each) plus 259: waves take a second shot in the sampler and in both
    counters."""
    from oracle import oracle
    from qldpcsim_amd import decoders, simulator
    from test_gpu_window import _grid_shots
    name = "q7v"
    Hx, Hz = csc.pair(name)
    Lx, Lz = csc.logicals(name)
    B = _grid_shots() + 259
    assert _kernel(name, "sample") == "channel_sample_kernel<7>"
    assert _kernel(name, "count") == "count_outcomes_kernel<7, true>"
    assert _kernel(name, "count_logical", True, True) == "count_logical_kernel<7, true, true>"
    want = oracle.channel_sample(Hx, Hz, csc.P, csc.SEED, csc.SHOT0, B)
    ch = _channel(name)
    sy_z, sy_x, ewX, ewZ = ch.sample(csc.P, B)
    _check_shots(name, (sy_z, sy_x, ewX, ewZ), want, False)
    _check_shots(name, _channel(name).sample(csc.P, B, bits=True), want, True)
    _, _, errX, errZ = want
    rng = np.random.default_rng(11)
    eX, eZ, recX, recZ = lm.craft(rng, Hx, Hz, Lx, Lz, errX, errZ)
    itX, itZ = rng.integers(1, 60, B).astype(np.int32), rng.integers(1, 60, B).astype(np.int32)
    M = csc.model(name)
    cX, cZ = M.classes(want[0], want[1], errX, errZ, eX, eZ)
    d = dict(cX=cX, cZ=cZ, recX=recX, recZ=recZ, k=Lx.shape[0], flipX=lm.flip_words(Lz, errX ^ eX),
             flipZ=lm.flip_words(Lx, errZ ^ eZ), want=M.counters(want[0], want[1], errX, errZ, eX, eZ, itX, itZ))
    csc.check_batch(d)
    for bits in (False, True):
        est = tuple(decoders.pack_bits(t) if bits else t for t in (_T(eX), _T(eZ)))
        syn = tuple(decoders.pack_bits(t) if bits else t for t in (sy_z, sy_x))
        args = (*syn, ewX, ewZ, *est, _T(itX), _T(itZ))
        _check_logical(d, ch.count_logical_device(*args, want_shots=True), (name, B, bits))
        assert ch.count(*args) == {k: d["want"][k] for k in simulator.COUNTER_KEYS}, (name, B, bits)


# ---------------------------------------------------------------------------
# phenomenological rows of more than 64 words
# ---------------------------------------------------------------------------
def test_phenomenological_rows_of_65_words():
    """q8a-Hz at T = 22, 65 shots: N = 4160 (NW = 65), M = 1408. The word
    loops of the sampler (fired-row write) and of the counter (estimate read)
    take a second trip; every round block and detector cut is word-aligned."""
    import torch
    from qldpcsim_amd import _lib, decoders
    from test_gpu_phenom import SEED, SHOT0, _half_dev, _words
    from test_phenom_model import half
    name, T, B = "q8a_hz", 22, 65
    H, L, Hstab, Lop = half(name)
    m, n = H.shape
    assert _lib.phenom_kernel_name(H, "sample", 0) == "phenom_sample_kernel<8>"
    assert _lib.phenom_kernel_name(H, "count", 0) == "phenom_count_kernel<8>"
    det, E, fired = pm.sample(H, T, 0.05, 0.04, SEED, SHOT0, B)
    assert fired.shape == (B, 4160) and det.shape == (B, 1408) and fired[:, 4096:].any()
    for bits in (False, True):
        h = _half_dev(name, T)
        assert (h.NW, h.MW, h.W) == (65, 22, 2)
        d, e, f = h.sample(0.05, 0.04, B, bits=bits, want_fired=True)
        gd = _words(d, T * m) if bits else _np(d)
        assert np.array_equal(gd, det), ("detectors", bits)
        assert np.array_equal(_np(e).view(np.uint64), pm.pack_words(E)), "E"
        assert np.array_equal(_np(f).view(np.uint64), pm.pack_words(fired)), "fired row"
        h2 = _half_dev(name, T)
        d1, e1 = h2.sample(0.05, 0.04, 30, bits=bits)
        d2, e2 = h2.sample(0.05, 0.04, 35, bits=bits)
        assert torch.equal(torch.cat([d1, d2]), d) and torch.equal(torch.cat([e1, e2]), e)
    rng = np.random.default_rng(17)
    ehat, rec = pm.craft(rng, H, Hstab, Lop, T, fired)
    iters = rng.integers(1, 60, B).astype(np.int32)
    cls, F, r = pm.classify(H, L, T, det, E, ehat)
    for i, want in enumerate((0, 0, 0, 1, 2, 2)):
        assert (rec == i).sum() >= 10 and (cls[rec == i] == want).all(), pm.RECIPES[i]
    want = pm.counters(cls, iters)
    wv = [want["failures"], want["logical_errors"], want["successes"], want["iterations"]]
    h = _half_dev(name, T)
    t_det, t_eh, t_it, t_E = _T(det), _T(ehat), _T(iters), _T(pm.pack_words(E).view(np.int64))
    for d_ in (t_det, decoders.pack_bits(t_det)):
        for e_ in (t_eh, decoders.pack_bits(t_eh)):
            acc, c, fl, rs = h.count_device(d_, t_E, e_, t_it, want_shots=True)
            assert np.array_equal(_np(c), cls)
            assert np.array_equal(_np(fl).view(np.uint64), pm.pack_words(F))
            assert np.array_equal(_np(rs).view(np.uint64), pm.pack_words(r))
            assert acc.cpu().tolist() == wv

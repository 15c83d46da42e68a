"""The seven pairs of tests/channel_shape_codes.py without a GPU: the generator's
bits, the table of shapes the cases were built for, the kernel instance
qldpc_channel_kernel_name / qldpc_phenom_kernel_name answer for every (kind,
alignment, residency), the n > 4096 refusal, the host paths against the models
on every case, and the input conditions of the batches the GPU tests run. With
these pinned, a disagreement in tests/test_gpu_channel_shapes.py is the
kernel's."""
import ctypes

import numpy as np
import pytest

import channel_shape_codes as csc
import logical_model as lm
import phenom_model as pm
from qldpcsim_amd import _lib

L = _lib.lib
OK, EINVAL, EUNSUP = _lib.QLDPC_OK, _lib.QLDPC_EINVAL, _lib.QLDPC_EUNSUP
MSG_N = "the channel kernels support n <= 4096 qubits (got 4097)"


def _err():
    return L.qldpc_last_error().decode()


# ---------------------------------------------------------------------------
# the generator and the table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", csc.IDS)
def test_generator_bits_are_pinned(name):
    Hx, Hz = csc.pair(name)
    assert Hx.dtype == np.uint8 and not Hx.flags.writeable and not Hz.flags.writeable
    assert csc.packed_sha256(name) == csc.SHA256[name]


def test_factors():
    C = csc.circ(5, (0, 1, 3))
    assert C[0].tolist() == [1, 1, 0, 1, 0] and C[4].tolist() == [1, 0, 1, 0, 1] and (C.sum(0) == 3).all()
    assert csc.hamming().T.tolist() == [[1, 0, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]]


@pytest.mark.parametrize("name", csc.IDS)
def test_table_columns(name):
    from qldpcsim_amd import logicals
    c = csc.CASES[name]
    Hx, Hz = csc.pair(name)
    f32 = np.float32
    assert not ((Hx.astype(f32) @ Hz.T.astype(f32)) % 2).any()                  # the pair commutes
    assert Hx.shape == (c["mx"], c["n"]) and Hz.shape == (c["mz"], c["n"])
    dx, dz = Hx.sum(axis=1), Hz.sum(axis=1)
    assert ((dx.min(), dx.max()), (dz.min(), dz.max())) == c["deg"]
    uniform = c["deg"][0][0] == c["deg"][0][1] == c["deg"][1][0] == c["deg"][1][1]
    assert c["udeg"] == (c["deg"][0][0] if uniform and c["deg"][0][0] in (6, 7, 8) else 0)
    assert c["W"] == (c["n"] + 63) // 64 <= 64
    Lx, Lz = csc.logicals(name)
    assert Lx.shape == Lz.shape == (c["k"], c["n"]) and c["k"] > 0
    assert c["k"] == c["n"] - logicals.gf2_rank(Hx) - logicals.gf2_rank(Hz)
    assert Hx.any(axis=0).all() and Hz.any(axis=0).all()


def test_the_edges_the_cases_were_built_for():
    C = csc.CASES
    rem = {k: (c["n"] % 4, c["n"] % 64) for k, c in C.items()}
    assert rem == {"q8a": (0, 0), "q6v": (0, 8), "q6b": (2, 62), "q7v": (0, 20), "q8b": (2, 6), "g0v": (0, 24),
                   "w64": (2, 18)}
    assert C["q8a"]["mz"] % 64 == 0 and (C["q8a"]["n"] + C["q8a"]["mz"]) % 64 == 0
    assert C["q6b"]["mx"] == C["q6b"]["mz"] == 63 and C["q6b"]["n"] + C["q6b"]["mz"] == 189
    assert C["g0v"]["mx"] != C["g0v"]["mz"]
    assert C["w64"]["W"] == 64 and (C["w64"]["W"] - 1) // 4 == 15 and (C["w64"]["mz"] + 63) // 64 == 32
    assert int(csc.pair("w64")[0].sum() + csc.pair("w64")[1].sum()) == 24300
    # q8a-Hz at T = 22: a second trip of every 64-word loop
    n, m, T = 128, 64, 22
    assert (T * n + (T - 1) * m, (T * n + (T - 1) * m + 63) // 64, T * m) == (4160, 65, 1408)
    # every degree and both VEC values by shape; every counter instance with the two misaligned cases
    assert {(c["udeg"], c["n"] % 4 == 0) for c in C.values()} == {(8, True), (6, True), (6, False), (7, True),
                                                                   (8, False), (0, True)}


# ---------------------------------------------------------------------------
# kernel names
# ---------------------------------------------------------------------------
def _name(hx, hz, kind, aligned, lds):
    buf = ctypes.create_string_buffer(128)
    rc = L.qldpc_channel_kernel_name(hx.handle if hx else None, hz.handle if hz else None, kind, aligned, lds, buf, 128)
    return (rc, buf.value.decode()) if rc == OK else (rc, _err())


@pytest.mark.parametrize("name", csc.IDS)
def test_channel_kernel_names(name):
    Hx, Hz = csc.pair(name)
    d = csc.CASES[name]["udeg"]
    vec = "true" if csc.CASES[name]["n"] % 4 == 0 else "false"
    for aligned in (True, False):
        for lds in (True, False):
            got = {k: _lib.channel_kernel_name(Hx, Hz, k, aligned, lds) for k in _lib.CHANNEL_KERNELS}
            assert got == {k: csc.kernel(name, k, aligned, lds) for k in _lib.CHANNEL_KERNELS}
            assert got["sample"] == f"channel_sample_kernel<{d}>"
            assert got["sample_vec"] == f"channel_sample_vec_kernel<{d}>"
            v = vec if aligned else "false"
            assert got["count"] == f"count_outcomes_kernel<{d}, {v}>"
            assert got["count_logical"] == f"count_logical_kernel<{d}, {v}, {'true' if lds else 'false'}>"


def test_the_cases_name_every_instance():
    """4 + 4 + 8 + 16 channel instances and 4 + 4 phenomenological ones: each
    is the answer for a case, alignment and residency that
    tests/test_gpu_channel_shapes.py or the phenomenological GPU tests assert
    and then compare with a model."""
    from test_phenom_model import KERNEL_DEGREE, SHAPES
    names = set()
    for name in csc.IDS:
        Hx, Hz = csc.pair(name)
        for aligned in ((True, False) if name in csc.MISALIGNED else (True,)):
            for mode in (1, 2):
                lds = csc.tabs_lds(name, mode)
                names |= {_lib.channel_kernel_name(Hx, Hz, k, aligned, lds) for k in ("count", "count_logical")}
        names.add(_lib.channel_kernel_name(Hx, Hz, "sample"))
        if name in csc.VEC_CASES:
            names.add(_lib.channel_kernel_name(Hx, Hz, "sample_vec"))
    assert set(csc.HALVES) <= set(SHAPES)
    names |= {f"phenom_{k}_kernel<{KERNEL_DEGREE[h]}>" for h in SHAPES for k in ("sample", "count")}
    tf = ("true", "false")
    want = {f"channel_sample_kernel<{d}>" for d in (0, 6, 7, 8)} | \
        {f"channel_sample_vec_kernel<{d}>" for d in (0, 6, 7, 8)} | \
        {f"count_outcomes_kernel<{d}, {v}>" for d in (0, 6, 7, 8) for v in tf} | \
        {f"count_logical_kernel<{d}, {v}, {t}>" for d in (0, 6, 7, 8) for v in tf for t in tf} | \
        {f"phenom_{k}_kernel<{d}>" for k in ("sample", "count") for d in (0, 6, 7, 8)}
    assert len(want) == 40 and names == want


def test_phenom_kernel_names():
    from test_phenom_model import KERNEL_DEGREE, half
    assert KERNEL_DEGREE == {"steane": 0, "shor_x": 0, "shor_z": 6, "LP04_0": 7, "q8a_hz": 8, "q6v_hz": 6, "q8b_hz": 8,
                             "g0v_hx": 0}
    for h, d in dict(KERNEL_DEGREE, q6b_hz=6).items():
        H = half(h)[0]
        assert _lib.phenom_kernel_name(H, "sample") == f"phenom_sample_kernel<{d}>"
        assert _lib.phenom_kernel_name(H, "count") == f"phenom_count_kernel<{d}>"
        if "_h" in h:
            assert csc.phenom_kernel(h, "sample") == f"phenom_sample_kernel<{d}>"
    # a uniform degree without an instance of its own: the generic loop
    assert _lib.phenom_kernel_name(np.kron(np.eye(3, dtype=np.uint8), np.ones((1, 5), np.uint8)), "count") == \
        "phenom_count_kernel<0>"


def test_kernel_name_arguments():
    Hx, Hz = csc.pair("q6v")
    cx, cz = _lib.Code(Hx), _lib.Code(Hz)
    assert _name(cx, cz, 3, 1, 1) == (OK, "count_logical_kernel<6, true, true>")
    assert _name(cx, cz, 4, 1, 1) == (EINVAL, "unknown channel kernel kind 4")
    assert _name(cx, cz, -1, 1, 1)[0] == EINVAL
    assert _name(None, cz, 0, 1, 1) == (EINVAL, "code is null") and _name(cx, None, 0, 1, 1) == (EINVAL, "code is null")
    other = _lib.Code(csc.pair("q7v")[1])
    assert _name(cx, other, 0, 1, 1)[0] == EINVAL and "same number of columns" in _err()
    assert L.qldpc_channel_kernel_name(cx.handle, cz.handle, 0, 1, 1, None, 128) == EINVAL and _err() == "null argument"
    assert L.qldpc_channel_kernel_name(cx.handle, cz.handle, 0, 1, 1, ctypes.create_string_buffer(8), 0) == EINVAL
    # different uniform degrees in the halves: the generic loop
    mixed = _lib.Code(np.kron(np.eye(12, dtype=np.uint8), np.ones((1, 6), np.uint8)))
    assert cx.n == mixed.n == 72 and _name(cx, mixed, 2, 1, 0) == (OK, "count_outcomes_kernel<6, true>")
    seven = _lib.Code(np.concatenate([np.kron(np.eye(10, dtype=np.uint8), np.ones((1, 7), np.uint8)),
                                      np.zeros((10, 2), np.uint8)], axis=1))
    assert _name(cx, seven, 2, 1, 0) == (OK, "count_outcomes_kernel<0, true>")
    buf = ctypes.create_string_buffer(128)
    assert L.qldpc_phenom_kernel_name(cz.handle, 2, buf, 128) == EINVAL
    assert _err() == "unknown phenomenological kernel kind 2"
    assert L.qldpc_phenom_kernel_name(None, 0, buf, 128) == EINVAL and _err() == "code is null"
    assert L.qldpc_phenom_kernel_name(cz.handle, 0, None, 128) == EINVAL and _err() == "null argument"


def test_pairs_past_4096_columns_are_refused():
    """The n <= 4096 limit (64 lanes, one per error word) on a 4097-column
    pair: the name query, the channel table and the logical tables refuse it
    without a device; n = 4096 is accepted."""
    big = _lib.Code(np.ones((1, 4097), np.uint8))
    assert _name(big, big, 0, 1, 0) == (EUNSUP, MSG_N)
    z = np.zeros(4097)
    with pytest.raises(NotImplementedError, match="n <= 4096 qubits .got 4097."):
        _lib.Channel(big, big, z, z, z)
    with pytest.raises(NotImplementedError, match="n <= 4096 qubits .got 4097."):
        _lib.Logicals(big, big, np.ones((1, 4097), np.uint8), np.ones((1, 4097), np.uint8))
    buf = ctypes.create_string_buffer(128)
    assert L.qldpc_phenom_kernel_name(big.handle, 0, buf, 128) == EUNSUP
    assert _err().startswith("the phenomenological kernels support n <= 4096 and m, E <= 65535 (got n = 4097")
    edge = _lib.Code(np.ones((1, 4096), np.uint8))
    assert _name(edge, edge, 0, 1, 0) == (OK, "channel_sample_kernel<0>")
    from qldpcsim_amd import simulator
    assert simulator._channel_ok(np.ones((1, 4096)), np.ones((1, 4096)))
    assert not simulator._channel_ok(np.ones((1, 4097)), np.ones((1, 4097)))


# ---------------------------------------------------------------------------
# host paths against the models
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", csc.IDS)
def test_oracle_stream_equals_the_philox_model(name):
    """oracle.channel_sample, the GPU sampler tests' reference, against the
    NumPy Philox of tests/phenom_model.py at the shots those tests draw: X if
    u < T1, Y if T1 <= u < T2, Z if T2 <= u < T3; syndromes are H e mod 2."""
    from oracle import oracle
    Hx, Hz = csc.pair(name)
    B, n = csc.CASES[name]["shots"], csc.CASES[name]["n"]
    u = pm.draws(csc.SEED, csc.SHOT0, B, n)
    for p in (csc.P, 1.0, 0.0) if name in ("q8a", "w64") else (csc.P,):
        t1, t2, t3 = (np.uint64(t) for t in oracle.channel_thresholds(p))
        errX, errZ = (u < t2).astype(np.uint8), ((u >= t1) & (u < t3)).astype(np.uint8)
        sy_z, sy_x, ex, ez = oracle.channel_sample(Hx, Hz, p, csc.SEED, csc.SHOT0, B)
        assert np.array_equal(ex, errX) and np.array_equal(ez, errZ)
        assert np.array_equal(sy_z, lm._mod2(errX, Hz)) and np.array_equal(sy_x, lm._mod2(errZ, Hx))
        if p == 1.0:                                        # T3 = 2^32: every qubit errs
            assert (errX | errZ).all() and not errX.all() and not errZ.all()
        else:
            assert (errX.any() and errZ.any()) == (p > 0) and (errX | errZ).any() == (p > 0)


@pytest.mark.parametrize("name", csc.IDS)
def test_counter_batch_conditions_and_host_counters(name):
    """Every recipe and every class at least 20 times in each half of the
    batch of 257; simulator.count_outcomes and count_logical_outcomes equal the
    model and the reference's per-shot loop on it."""
    from qldpcsim_amd import simulator
    d = csc.batch(name)
    assert d["errX"].shape == (257, csc.CASES[name]["n"]) and d["k"] == csc.CASES[name]["k"]
    csc.check_batch(d)
    Hx, Hz = csc.pair(name)
    args = (Hx, Hz, d["sy_z"], d["sy_x"], d["errX"], d["errZ"], d["eX"], d["eZ"], d["itX"], d["itZ"])
    six = simulator.count_outcomes(*args)
    assert six == csc.reference_counters(name) == {k: d["want"][k] for k in simulator.COUNTER_KEYS}
    assert 0 < six["decSuccessExact"] < 257 and six["DecFailures_X"] > 0 and six["DecFailures_Z"] > 0
    nine, (cX, cZ, fX, fZ) = simulator.count_logical_outcomes(*args, logicals=csc.logicals(name), want_shots=True)
    assert nine == d["want"]
    assert np.array_equal(cX, d["cX"]) and np.array_equal(cZ, d["cZ"])
    assert np.array_equal(fX, d["flipX"]) and np.array_equal(fZ, d["flipZ"])


def test_w64_tables_fit_in_lds():
    """W = 64, k = 8 (kp = 64): 2 x 32 KiB of tables beside 63 KiB of CSR fit a
    workgroup's LDS, so logical_tabs = 1 runs and the automatic choice stages
    them; the GPU test runs modes 1, 2 and 0."""
    assert csc.logical_lds_bytes("w64", True) == 139848 <= csc.LDS_BYTES
    assert csc.logical_lds_bytes("w64", False) == 139848 - 65536
    assert [csc.tabs_lds("w64", m) for m in (1, 2, 0)] == [True, False, True]
    for name in csc.IDS:
        assert [csc.tabs_lds(name, m) for m in (1, 2, 0)] == [True, False, True]


def test_vector_tables():
    """The per-qubit tables of the vector sampler test: thresholds 0 and 2^32,
    a row that sums to 1, generic rows."""
    for name in ("q8a", "q6b", "g0v"):
        pr = csc.vec_table(name)
        assert pr.shape == (3, csc.CASES[name]["n"])
        T = _lib.channel_table(*pr)
        assert (T[:, (pr == 0).all(0)] == 0).all() and (pr == 0).all(0).any()
        for r in range(3):
            assert (T[r:, pr[r] == 1.0] == 1 << 32).all() and (pr[r] == 1.0).any()
        full = (pr.sum(0) == 1.0) & (pr.max(0) < 1.0)
        assert full.any() and (T[2, full] == 1 << 32).all() and (T[0, full] > 0).all()
        generic = (pr.sum(0) < 1.0) & (pr.sum(0) > 0)
        assert generic.sum() >= 4 and (T[2, generic] < 1 << 32).all()
        assert np.unique(T, axis=1).shape[1] == 9


@pytest.mark.parametrize("T,W,F", [(5, 3, 1), (5, 2, 2)])
def test_window_twin_on_word_aligned_offsets(T, W, F):
    """q8a-Hz, n + m = 192: every commit and every cut of window_advance
    starts on a multiple of 64. The twin's properties on the schedules the
    window kernel test runs."""
    import test_window_model as tw
    tw.test_true_window_errors_reassemble_the_fired_row("q8a_hz", T, W, F)
    tw.test_any_window_estimates_telescope_to_the_detectors("q8a_hz", T, W, F)


def test_window_twin_on_q6b():
    import test_window_model as tw
    tw.test_true_window_errors_reassemble_the_fired_row(csc.WINDOW_HALF, 4, 2, 1)
    tw.test_any_window_estimates_telescope_to_the_detectors(csc.WINDOW_HALF, 4, 2, 1)


def test_long_row_model_inputs():
    """q8a-Hz at T = 22 (N = 4160: 65 words): the model's sample, the host
    detectors and fold on it, and the crafted estimates' classes."""
    from qldpcsim_amd import spacetime
    from test_phenom_model import half
    H, Lt, Hstab, Lop = half("q8a_hz")
    T, B = 22, 65
    det, E, fired = pm.sample(H, T, 0.05, 0.04, csc.SEED, csc.SHOT0, B)
    assert fired.shape == (B, 4160) and det.shape == (B, 1408) and fired[:, 4096:].any()
    assert np.array_equal(spacetime.detectors(H, T, fired), det)
    assert np.array_equal(spacetime.fold_data(fired, 128, 64, T), E)
    ehat, rec = pm.craft(np.random.default_rng(17), H, Hstab, Lop, T, fired)
    cls, F, r = pm.classify(H, Lt, T, det, E, ehat)
    for i, want in enumerate((0, 0, 0, 1, 2, 2)):
        assert (cls[rec == i] == want).all() and (rec == i).sum() >= 10
    got, (gc, gf, gr) = spacetime.count_phenomenological(H, Lt, T, det, E, ehat, np.ones(B, np.int32), want_shots=True)
    assert np.array_equal(gc, cls) and np.array_equal(gr, r) and np.array_equal(gf, pm.pack_words(F))

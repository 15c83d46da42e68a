"""The logical outcome counters on the GPU (count_logical_kernel through
qldpc_count_logical_ex): per-shot classes, flip words and all nine counters
against the independent model (tests/logical_model.py) on crafted estimates,
both table residencies, a k = 0 pair, and simulate_p(logical=True) on the
device pipeline and under two ranks. Every comparison is integer equality."""
import functools

import numpy as np
import pytest

import logical_model as lm

pytestmark = pytest.mark.gpu


def _synthetic():
    """n = 1500, one X check on columns 0-3, one Z check on 2-5 (overlap 2:
    they commute), k = 1498: tables far past any LDS."""
    Hx = np.zeros((1, 1500), np.int8)
    Hz = np.zeros((1, 1500), np.int8)
    Hx[0, 0:4] = 1
    Hz[0, 2:6] = 1
    return Hx, Hz


def _pair(name):
    from qldpcsim_amd import codes
    if name == "synthetic":
        return _synthetic()
    if name == "k0":
        return np.array([[1, 1]], np.int8), np.array([[1, 1]], np.int8)
    return codes.load_code(name)


@functools.lru_cache(maxsize=None)
def _case(name, B):
    """One crafted batch of a code and the model's answer, computed once:
    device tensors in both formats, and the expected classes / flips / counters."""
    import torch
    from qldpcsim_amd import decoders, logicals, simulator
    Hx, Hz = _pair(name)
    Lx, Lz = logicals.css_logicals(Hx, Hz)
    dev = torch.device("cuda", 0)
    ch = simulator.DeviceChannel(Hx, Hz, dev, 1234)
    sy_z, sy_x, ewX, ewZ = ch.sample(0.06, B)
    errX, errZ = ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy()
    rng = np.random.default_rng(7)
    eX, eZ, recX, recZ = lm.craft(rng, Hx, Hz, Lx, Lz, errX, errZ)
    itX = rng.integers(1, 60, B).astype(np.int32)
    itZ = rng.integers(1, 60, B).astype(np.int32)
    M = lm.Model(Hx, Hz)
    hz, hx = sy_z.cpu().numpy(), sy_x.cpu().numpy()
    cX, cZ = M.classes(hz, hx, errX, errZ, eX, eZ)
    want = M.counters(hz, hx, errX, errZ, eX, eZ, itX, itZ)
    T = lambda a: torch.as_tensor(np.ascontiguousarray(a), device=dev)  # noqa: E731
    teX, teZ = T(eX), T(eZ)
    d = dict(ch=ch, k=Lx.shape[0], rec=(recX, recZ), cls=(cX, cZ), want=want,
             flips=(lm.flip_words(Lz, errX ^ eX), lm.flip_words(Lx, errZ ^ eZ)),
             err=(ewX, ewZ), it=(T(itX), T(itZ)),
             syn={"bytes": (sy_z, sy_x), "bits": (decoders.pack_bits(sy_z), decoders.pack_bits(sy_x))},
             est={"bytes": (teX, teZ), "bits": (decoders.pack_bits(teX), decoders.pack_bits(teZ))})
    return d


def _run(d, syn="bytes", est="bytes", want_shots=True):
    ch = d["ch"]
    out = ch.count_logical_device(*d["syn"][syn], *d["err"], *d["est"][est], *d["it"], want_shots=want_shots)
    if not want_shots:
        return out.cpu().numpy()
    return tuple(t.cpu().numpy() for t in out)


def _check(d, got):
    from qldpcsim_amd import simulator
    acc, cX, cZ, fX, fZ = got
    keys = simulator.COUNTER_KEYS + simulator.LOGICAL_KEYS
    B, k = cX.shape[0], d["k"]
    assert np.array_equal(cX, d["cls"][0]) and np.array_equal(cZ, d["cls"][1])
    assert fX.shape == (B, (k + 63) // 64) and fZ.shape == fX.shape
    assert np.array_equal(fX.view(np.uint64), d["flips"][0]) and np.array_equal(fZ.view(np.uint64), d["flips"][1])
    if k % 64:                                              # padding bits of the last word
        pad = ~np.uint64((1 << (k % 64)) - 1)
        assert not (fX.view(np.uint64)[:, -1] & pad).any() and not (fZ.view(np.uint64)[:, -1] & pad).any()
    c = dict(zip(keys, (int(v) for v in acc)))
    assert c == d["want"]
    # the nine counters are the sums of the per-shot outputs
    assert c["DecFailures_X"] == (cX == 2).sum() and c["DecFailures_Z"] == (cZ == 2).sum()
    assert c["logicalErrors_X"] == (cX == 1).sum() and c["logicalErrors_Z"] == (cZ == 1).sum()
    assert c["decSuccessLogical"] == ((cX == 0) & (cZ == 0)).sum()
    assert ((fX != 0).any(axis=1) == (cX == 1))[cX != 2].all()
    lm.check_invariants(c, B)
    return c


# steane: n = 7, one word, byte loads; shor: m_x != m_z; LP04_0: n = 175, degree 7, k = 19;
# LP118_0: n = 544, 32-bit estimate loads, degree 8, k = 80 (two flip words); LP118_2: k = 136 (three)
@pytest.mark.parametrize("est", ["bytes", "bits"])
@pytest.mark.parametrize("syn", ["bytes", "bits"])
@pytest.mark.parametrize("name", ["steane", "shor", "LP04_0", "LP118_0", "LP118_2"])
def test_classes_flips_and_counters_equal_the_model(name, syn, est):
    from qldpcsim_amd import simulator
    d = _case(name, 2000)
    for c, rec in zip(d["cls"], d["rec"]):                  # every recipe, hence every class, is there
        assert (np.bincount(rec, minlength=4) >= 200).all()
        assert (c[rec <= 1] == 0).all() and (c[rec == 2] == 1).all() and (c[rec == 3] == 2).mean() > 0.5
        assert (np.bincount(c, minlength=3) >= 200).all()
    c = _check(d, _run(d, syn, est))
    # the first six are the six-counter kernel's on the same tensors
    old = d["ch"].count(*d["syn"][syn], *d["err"], *d["est"][est], *d["it"])
    assert old == {k: c[k] for k in simulator.COUNTER_KEYS}
    # with no per-shot output the counters are the same
    assert np.array_equal(_run(d, syn, est, want_shots=False), [c[k] for k in c])
    assert d["ch"].count_logical(*d["syn"][syn], *d["err"], *d["est"][est], *d["it"]) == c


def test_accumulates_into_a_given_accumulator():
    import torch
    d = _case("steane", 2000)
    acc = torch.full((9,), 5, dtype=torch.int64, device="cuda:0")
    out = d["ch"].count_logical_device(*d["syn"]["bytes"], *d["err"], *d["est"]["bytes"], *d["it"], acc=acc)
    assert out is acc
    assert (acc.cpu().numpy() - 5).tolist() == list(d["want"].values())


def test_global_memory_table_path_on_a_code_past_lds(qopt):
    """k = 1498 at n = 1500: 2 x 288 KB of tables, read from global memory."""
    d = _case("synthetic", 256)
    assert d["k"] == 1498
    assert (np.bincount(d["cls"][0], minlength=3)[:2] > 25).all()
    _check(d, _run(d))
    _check(d, _run(d, "bits", "bits"))
    qopt(logical_tabs=1)                                    # staging them is refused, not attempted
    with pytest.raises(NotImplementedError, match="LDS"):
        _run(d)


@pytest.mark.parametrize("name", ["LP04_0", "LP118_0"])
def test_both_table_residencies_agree(name, qopt):
    d = _case(name, 2000)
    outs = []
    for mode in (1, 2, 0):                                  # LDS, global memory, automatic
        qopt(logical_tabs=mode)
        outs.append(_run(d, "bits", "bytes"))
        _check(d, outs[-1])
    for o in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], o))


def test_k0_pair_has_no_logical_errors():
    d = _case("k0", 64)
    assert d["k"] == 0
    acc, cX, cZ, fX, fZ = _run(d)
    assert fX.shape == (64, 0) and fZ.shape == (64, 0)
    c = _check(d, (acc, cX, cZ, fX, fZ))
    assert not (cX == 1).any() and not (cZ == 1).any()
    assert c["logicalErrors_X"] == 0 and c["logicalErrors_Z"] == 0
    assert c["decSuccessLogical"] == ((cX != 2) & (cZ != 2)).sum() > 0
    assert (cX == 2).any() and (cZ == 2).any()


def _decode_reference(Hx, Hz, decType, sched, osd, p, max_iter, sy_z, sy_x):
    """Both halves decoded off the device: BF by the NumPy model of
    tests/hard_model.py, MS by the CPU oracle; OSD on every non-converged MS
    decode by the library's host OSD, with the oracle's OSDdec restatement
    checked on the first of them (it is a per-shot Python loop)."""
    from oracle import oracle
    import hard_model
    from qldpcsim_amd import decoders, schedule
    lx, lz = schedule.select_layers(Hx, Hz, sched)
    outs = []
    for H, layers, syn in ((Hz, lx, sy_z), (Hx, lz, sy_x)):
        if decType == "BF":
            e, it, _ = hard_model.bf_batch(H, syn, 50)
        else:
            lp, lr = schedule.pack_layers(layers, H.shape[0])
            e, it, post, fl = oracle.decode_batch(decType, H, syn, p / 3, max_iter, lp, lr)
            if osd >= 0:
                before = e.copy()
                decoders.apply_osd(H, syn, e, post, fl, osd)
                for i in np.flatnonzero((fl & 1) == 0)[:8]:
                    assert np.array_equal(e[i], oracle.osd_dec(H, before[i].astype(np.int64), syn[i].astype(np.int64),
                                                               post[i], osd))
        outs.append((e, it))
    return outs


@pytest.mark.parametrize("code,decType,sched,osd,p,max_iter", [
    ("steane", "BF", "F", -1, 0.05, 50),
    ("LP04_0", "MS", "L", 0, 0.1, 30),
])
def test_simulate_p_logical_on_the_device_pipeline(code, decType, sched, osd, p, max_iter):
    """simulate_p(logical=True) over several pipelined batches: all nine
    counters equal the model's on the same Philox shots (regenerated by the
    oracle) and decodes; they do not depend on the batch size; logical=False on
    the same seed returns the same six values and only six keys."""
    from oracle import oracle
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code(code)
    shots, seed = 20000, 21
    kw = dict(shots=shots, decType=decType, decIterations=max_iter, decSchedule=sched, OSDorder=osd, rngSeed=seed,
              sampler="device", verbose=False)
    got = simulator.simulate_p(Hx, Hz, p, batch_size=4096, logical=True, **kw)
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    sy_z, sy_x, errX, errZ = oracle.channel_sample(Hx, Hz, p, int(key), 0, shots)
    (eX, itX), (eZ, itZ) = _decode_reference(Hx, Hz, decType, sched, osd, p, max_iter, sy_z, sy_x)
    want = lm.Model(Hx, Hz).counters(sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
    for k in ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen") + simulator.LOGICAL_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert got["Avg_number_of_iterations_X"] == want["nIterAccX"] / float(shots)
    assert got["Avg_number_of_iterations_Z"] == want["nIterAccZ"] / float(shots)
    assert got["logical_error_rate"] == 1. - want["decSuccessLogical"] / shots
    assert got["logical_error_rate_ci95"] == simulator.wilson_interval(shots - want["decSuccessLogical"], shots)
    assert want["logicalErrors_X"] > 0 and want["logicalErrors_Z"] > 0 and want["decSuccessLogical"] > 0
    lm.check_invariants(want, shots)
    assert simulator.simulate_p(Hx, Hz, p, batch_size=7000, logical=True, **kw) == got
    off = simulator.simulate_p(Hx, Hz, p, batch_size=4096, **kw)
    assert len(off) == 6 and off == {k: got[k] for k in off}


def test_cli_two_ranks_logical(tmp_path):
    """`torchrun -m qldpcsim_amd.simulator --logical` with two gloo ranks on
    the one GPU: the all-reduced nine counters equal the model's count over
    both ranks' shards (rank r's contiguous share from its Philox key)."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    from oracle import oracle
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    np.save(tmp_path / "Hx.npy", Hx.astype(np.int64))
    np.save(tmp_path / "Hz.npy", Hz.astype(np.int64))
    res = tmp_path / "res.json"
    shots, seed, p, it = 20001, 4, 0.08, 30
    env = dict(os.environ, QLDPC_SIM_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29541", "-m", "qldpcsim_amd.simulator",
                        "--Hx", str(tmp_path / "Hx.npy"), "--Hz", str(tmp_path / "Hz.npy"), "--p", str(p),
                        "--shots", str(shots), "--decIterations", str(it), "--rngSeed", str(seed), "--batch", "4096",
                        "--logical", "--results", str(res)], cwd=ROOT, capture_output=True, text=True, timeout=110,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stdout.count("SIMULATION RESULTS") == 1 and r.stdout.count("LOGICAL ERROR RATES") == 1
    doc = json.loads(res.read_text())
    assert doc["meta"]["world"] == 2 and doc["meta"]["logical"] is True
    got = doc["results"][str(p)]
    M = lm.Model(Hx, Hz)
    want = None
    for rank in range(2):
        my = shots // 2 + (1 if rank < shots % 2 else 0)
        key = np.random.SeedSequence([seed, rank]).generate_state(1, np.uint64)[0]
        sy_z, sy_x, errX, errZ = oracle.channel_sample(Hx, Hz, p, int(key), 0, my)
        (eX, itX), (eZ, itZ) = _decode_reference(Hx, Hz, "MS", "F", -1, p, it, sy_z, sy_x)
        c = M.counters(sy_z, sy_x, errX, errZ, eX, eZ, itX, itZ)
        want = c if want is None else {k: want[k] + c[k] for k in c}
    for k in ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen") + simulator.LOGICAL_KEYS:
        assert got[k] == want[k], (k, got[k], want[k])
    assert abs(got["Avg_number_of_iterations_X"] - want["nIterAccX"] / shots) < 1e-9
    assert abs(got["Avg_number_of_iterations_Z"] - want["nIterAccZ"] / shots) < 1e-9
    assert got["logical_error_rate"] == 1. - want["decSuccessLogical"] / shots
    lm.check_invariants(want, shots)

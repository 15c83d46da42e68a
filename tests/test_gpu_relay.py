"""relay_ms_kernel on the device against tests/relay_model.py,
bit for bit: e_hat, iterations, posteriors as 64-bit patterns, flags, found and
best_leg; against the min-sum kernels where the relay has one leg and no
memory; through the simulator."""
import functools

import numpy as np
import pytest

import logical_model
import relay_model as rm
from test_relay_model import selection_batch

pytestmark = pytest.mark.gpu

FLAGS = rm.FLAG_CONVERGED | rm.FLAG_MIN_ZERO


@functools.lru_cache(maxsize=None)
def _H(name):
    from qldpcsim_amd import codes
    if name == "LP04_0_zero_col":
        Hz = codes.load_code("LP04_0")[1].copy()
        Hz[:, 70] = 0                                        # a variable without checks
        return Hz
    Hx, Hz = codes.load_code(name)
    return Hx if name == "steane" else Hz


def _channel(H, B, p, seed):
    """Syndromes of errors drawn at 2p/3 per variable (decoded with the prior p/3)."""
    err = (np.random.default_rng(seed).random((B, H.shape[1])) < 2 * p / 3).astype(np.int64)
    return ((err @ H.T) % 2).astype(np.uint8)


def _gpu(H, syn, p, T, G, S, bits_in=False, bits_out=False, want_post=True, out=None):
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(syn, device="cuda:0")
    if bits_in:
        s = decoders.pack_bits(s)
    r = decoders.decode_batch(H, s, p, 0, algo="RELAY", relay=decoders.RelayConfig(T, G, S), want_post=want_post,
                              ehat_bits=bits_out, out=out)
    torch.cuda.synchronize()
    return r


def _same(r, want, n, bits_out=False, want_post=True):
    from qldpcsim_amd import decoders
    e, it, post, fl, found, leg = want
    assert np.isfinite(post).all()                           # the model's inputs stay finite
    ge = decoders.unpack_bits(r.ehat, n) if bits_out else r.ehat
    np.testing.assert_array_equal(r.iters.cpu().numpy(), it)
    np.testing.assert_array_equal(ge.cpu().numpy(), e)
    if want_post:
        np.testing.assert_array_equal(r.post.cpu().numpy().view(np.uint64), post.view(np.uint64))
    else:
        assert r.post is None
    np.testing.assert_array_equal(r.flags.cpu().numpy() & FLAGS, fl)
    np.testing.assert_array_equal(r.found.cpu().numpy(), found)
    np.testing.assert_array_equal(r.best_leg.cpu().numpy(), leg)


@functools.lru_cache(maxsize=None)
def _selection_model(S):
    H, syn, p, T, G = selection_batch()
    return rm.decode(H, syn, p, T, G, S)


@pytest.mark.parametrize("name,kernel", [("steane", "relay_ms_kernel<0>"), ("LP04_0", "relay_ms_kernel<7>"),
                                         ("LP118_0", "relay_ms_kernel<8>")])
def test_kernel_names_and_launch_info(name, kernel):
    from qldpcsim_amd import _lib
    H = _H(name)
    rl = _lib.code_for(H, 0).relay([5], np.zeros((1, H.shape[1])), 1)
    assert rl.kernel_name() == kernel
    waves, wgs, lds = rl.launch_info()
    lay = rl.layout()
    assert waves >= 1 and wgs >= 1 and lds == lay["image"] + waves * lay["wave_bytes"]


@pytest.mark.parametrize("kind", ["channel", "random"])
@pytest.mark.parametrize("name", ["LP04_0", "LP118_0", "steane"])
def test_one_leg_without_memory_equals_the_min_sum_kernels(name, kind, qopt):
    """gamma = 0, one leg, S = 1 against decode_batch(algo="MS") through the
    default kernels and the generic LDS kernel: e_hat, iterations, posterior
    bits and CONVERGED (MIN_ZERO may differ: no check pass runs after a solution)."""
    import torch
    from qldpcsim_amd import _lib, decoders
    H = _H(name)
    m, n = H.shape
    it_max, p = 20, 0.05
    for B in (1, 3, 65, 1001):
        syn = _channel(H, B, p, 100 + B) if kind == "channel" else \
            np.random.default_rng(200 + B).integers(0, 2, (B, m), dtype=np.uint8)
        r = _gpu(H, syn, p / 3, [it_max], np.zeros((1, n)), 1)
        s = torch.as_tensor(syn, device="cuda:0")
        for generic in (0, 1):
            qopt(flood_generic=generic)
            w = decoders.decode_batch(H, s, p / 3, it_max, algo="MS", want_post=True)
            torch.cuda.synchronize()
            assert torch.equal(r.ehat, w.ehat) and torch.equal(r.iters, w.iters)
            assert torch.equal(r.post.view(torch.int64), w.post.view(torch.int64))
            assert torch.equal(r.flags & _lib.FLAG_CONVERGED, w.flags & _lib.FLAG_CONVERGED)
            conv = (w.flags & _lib.FLAG_CONVERGED) != 0
            assert torch.equal(r.found, conv.to(torch.int32))
            assert torch.equal(r.best_leg, torch.where(conv, 0, -1).to(torch.int32))
        qopt(flood_generic=0)


@pytest.mark.parametrize("S", [3, 1, 2])
def test_selection_batch_equals_the_model(S):
    """LP04_0 Hz, p = 0.08, 1,001 half-shots, T = [10, 6, 6, 6, 6]: every branch
    of the selection (test_relay_model.test_selection_reaches_every_branch)."""
    H, syn, p, T, G = selection_batch()
    want = _selection_model(S)
    if S == 3:
        np.testing.assert_array_equal(np.bincount(want[4], minlength=4), [206, 36, 44, 715])
    _same(_gpu(H, syn, p, T, G, S), want, H.shape[1])


def test_lp118_0_equals_the_model():
    """LP118_0 Hz, 130 half-shots at p = 0.07, T = [12, 8, 8, 8], S = 2:
    found 0 / 1 / 2 for 33 / 12 / 85 half-shots."""
    from qldpcsim_amd import decoders
    H = _H("LP118_0")
    n = H.shape[1]
    syn = _channel(H, 130, 0.07, 5)
    T, G = [12, 8, 8, 8], decoders.relay_gammas(n, 4, seed=7)
    want = rm.decode(H, syn, 0.07 / 3, T, G, 2)
    np.testing.assert_array_equal(np.bincount(want[4], minlength=3), [33, 12, 85])
    _same(_gpu(H, syn, 0.07 / 3, T, G, 2), want, n)


def test_one_iteration_legs():
    """T = [1] * 8 on LP04_0, S = 2: a leg boundary after every pass; found
    0 / 1 / 2 for 848 / 59 / 94 half-shots."""
    from qldpcsim_amd import decoders
    H, syn, p, _, _ = selection_batch()
    n = H.shape[1]
    G = decoders.relay_gammas(n, 8, seed=7)
    want = rm.decode(H, syn, p, [1] * 8, G, 2)
    np.testing.assert_array_equal(np.bincount(want[4], minlength=3), [848, 59, 94])
    _same(_gpu(H, syn, p, [1] * 8, G, 2), want, n)


@pytest.mark.parametrize("name", ["steane", "LP04_0_zero_col"])
def test_partial_chunk_and_a_variable_without_checks(name):
    """steane: n = 7, one partial chunk, pad lanes, relay_ms_kernel<0>; LP04_0
    with column 70 zeroed: non-uniform row degrees and an isolated variable."""
    from qldpcsim_amd import decoders
    H = _H(name)
    n = H.shape[1]
    syn = _channel(H, 257, 0.12 if name == "steane" else 0.08, 21)
    T, G = [5, 5, 5], decoders.relay_gammas(n, 3, seed=7)
    want = rm.decode(H, syn, 0.08 / 3, T, G, 2)
    if name == "steane":                                     # every syndrome is solved; both legs' solutions occur
        assert np.all(want[4] == 2) and len(np.unique(want[5])) == 2
    else:
        assert np.all(np.bincount(want[4], minlength=3) > 0)
    _same(_gpu(H, syn, 0.08 / 3, T, G, 2), want, n)


@pytest.mark.parametrize("bits_in,bits_out,want_post", [(True, True, False), (True, False, True), (False, True, True),
                                                        (False, False, False)])
def test_formats_and_out_reuse(bits_in, bits_out, want_post):
    """Both syndrome formats, bit-packed and byte estimates, posterior rows on
    and off; a second decode into the first one's buffers (out=)."""
    H, syn, p, T, G = selection_batch()
    n = H.shape[1]
    want = _selection_model(3)
    r = _gpu(H, syn, p, T, G, 3, bits_in, bits_out, want_post)
    _same(r, want, n, bits_out, want_post)
    keep = r.ehat.data_ptr(), r.info.data_ptr()
    r.ehat.fill_(1), r.iters.fill_(-1), r.flags.fill_(-1), r.info.fill_(-7)
    r2 = _gpu(H, syn, p, T, G, 3, bits_in, bits_out, want_post, out=r)
    assert (r2.ehat.data_ptr(), r2.info.data_ptr()) == keep
    _same(r2, want, n, bits_out, want_post)
    with pytest.raises(ValueError, match="out buffers"):
        _gpu(H, syn[:10], p, T, G, 3, bits_in, bits_out, want_post, out=r)


def test_host_path_equals_the_model():
    from qldpcsim_amd import decoders
    H, syn, p, T, G = selection_batch()
    want = _selection_model(3)
    for want_post in (True, False):
        r = decoders.decode_batch(H, syn, p, 0, algo="RELAY", relay=decoders.RelayConfig(T, G, 3), want_post=want_post)
        np.testing.assert_array_equal(r.ehat, want[0])
        np.testing.assert_array_equal(r.iters, want[1])
        if want_post:
            np.testing.assert_array_equal(r.post.view(np.uint64), want[2].view(np.uint64))
        np.testing.assert_array_equal(r.flags & FLAGS, want[3])
        np.testing.assert_array_equal(r.found, want[4])
        np.testing.assert_array_equal(r.best_leg, want[5])
    e, it = decoders.Relay_decoder(H, syn[5], p, T, G, sols=3)
    assert e.dtype == np.int8 and isinstance(it, int)
    np.testing.assert_array_equal(e, want[0][5])
    assert it == want[1][5]


@pytest.mark.parametrize("static", [0, 1])
def test_every_wave_restarts(static, qopt):
    """More than twice the half-shots the grid holds (one workgroup of one
    wave per CU): every wave decodes several, so a best solution, a weight or
    a `found` left over from the previous half-shot would show; queued and
    under static_sched."""
    import torch
    from qldpcsim_amd import _lib
    H, syn, p, T, G = selection_batch()
    n = H.shape[1]
    qopt(wg_per_cu=1, waves_per_wg=1, static_sched=static)
    waves, wgs, _ = _lib.code_for(H, 0).relay(T, G, 3).launch_info()
    assert (waves, wgs) == (1, 1)
    held = torch.cuda.get_device_properties(0).multi_processor_count
    assert len(syn) > 2 * held
    _same(_gpu(H, syn, p, T, G, 3), _selection_model(3), n)


def test_negative_prior():
    """p = 0.7: L < 0, almost every posterior starts negative; one leg pair."""
    from qldpcsim_amd import decoders
    H = _H("LP04_0")
    n = H.shape[1]
    err = (np.random.default_rng(31).random((65, n)) < 0.7).astype(np.int64)
    syn = ((err @ H.T) % 2).astype(np.uint8)
    T, G = [6, 6], decoders.relay_gammas(n, 2, seed=7)
    want = rm.decode(H, syn, 0.7, T, G, 1)
    assert np.isfinite(want[2]).all() and rm.llr(0.7) < 0
    _same(_gpu(H, syn, 0.7, T, G, 1), want, n)


def test_simulate_p_relay():
    """simulate_p(decType="RELAY") on LP04_0, 3,000 shots, fixed seed: the
    device pipeline, the host path fed the same shots and another batch size
    give equal counters; with logical=True they are logical_model's on the
    model's estimates. Refused combinations raise."""
    import torch
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("LP04_0")
    n = Hx.shape[1]
    p, shots, seed = 0.06, 3000, 11
    kw = dict(shots=shots, decType="RELAY", decIterations=10, relay_legs=4, relay_leg_iters=6, relay_sols=2,
              relay_seed=5, rngSeed=seed, verbose=False)
    got = simulator.simulate_p(Hx, Hz, p, batch_size=1000, sampler="device", logical=True, **kw)
    key = np.random.SeedSequence([seed, 0]).generate_state(1, np.uint64)[0]
    ch = simulator.DeviceChannel(Hx, Hz, torch.device("cuda", 0), key)
    sy_z, sy_x, ewX, ewZ = ch.sample(p, shots)
    sy_z, sy_x = sy_z.cpu().numpy(), sy_x.cpu().numpy()
    errX, errZ = ch.unpack(ewX).cpu().numpy(), ch.unpack(ewZ).cpu().numpy()
    grng = np.random.default_rng(5)                          # the Hz-decoded half draws first
    T = [10, 6, 6, 6]
    GX = np.vstack([np.full((1, n), 0.125), grng.uniform(-0.24, 0.66, (3, n))])
    GZ = np.vstack([np.full((1, n), 0.125), grng.uniform(-0.24, 0.66, (3, n))])
    mX = rm.decode(Hz, sy_z, p / 3, T, GX, 2)
    mZ = rm.decode(Hx, sy_x, p / 3, T, GZ, 2)
    c = logical_model.Model(Hx, Hz).counters(sy_z, sy_x, errX, errZ, mX[0], mZ[0], mX[1], mZ[1])
    assert c["DecFailures_X"] + c["DecFailures_Z"] > 0 and c["decSuccessLogical"] > 0
    for k in ("DecFailures_X", "DecFailures_Z", "decSuccessExact", "decSuccessDegen", "logicalErrors_X",
              "logicalErrors_Z", "decSuccessLogical"):
        assert got[k] == c[k], k
    assert got["Avg_number_of_iterations_X"] == c["nIterAccX"] / float(shots)
    assert got["Avg_number_of_iterations_Z"] == c["nIterAccZ"] / float(shots)
    plain = simulator.simulate_p(Hx, Hz, p, batch_size=1000, sampler="device", **kw)
    host = simulator.simulate_p(Hx, Hz, p, batch_size=1000, sampler="host", samples=(sy_z, sy_x, errX, errZ), **kw)
    other = simulator.simulate_p(Hx, Hz, p, batch_size=777, sampler="device", **kw)
    assert plain == host == other
    assert plain == {k: got[k] for k in plain}
    for bad in (dict(OSDorder=0), dict(correlated="XZ"), dict(decSchedule="L")):
        with pytest.raises(ValueError):
            simulator.simulate_p(Hx, Hz, p, sampler="device", **{**kw, **bad})

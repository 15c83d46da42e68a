"""The register-resident flooding min-sum kernel of the lift-16 QC codes
(ms_flood_kernel<8, 4> on LP118_0): bit for bit against the CPU
oracle and against its LDS twin (option flood_qc = 0), on channel syndromes
whose groups of four half-shots (the four DPP rows of a wave) converge at
different iterations, on the benchmark's uniform syndromes, on a zero prior,
on a code of the same shape that matches no generated table, and under both
work hand-outs."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC_KERNEL = "ms_flood_kernel<8, 4>"
LDS_TWIN = "ms_flood_lds_kernel<8, 4>"
P_MIX = 0.04          # LP118_0: most shots stop after 3-6 iterations, about 5 % run all 50
N_MIX = 1001
BATCHES = (1, 2, 3, 5, N_MIX)


def _half(which):
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP118_0")
    return Hx if which == "Hx" else Hz


@functools.lru_cache(maxsize=None)
def _channel_syndromes(which, count=N_MIX, seed=1234):
    H = _half(which)
    rng = np.random.default_rng(seed)
    e = (rng.random((count, H.shape[1])) < P_MIX).astype(np.uint8)
    syn = (e @ H.T % 2).astype(np.uint8)
    syn.setflags(write=False)
    return syn


def _oracle_decode(H, syn, p, max_iter):
    """(ehat, iters, post, flags) of the CPU oracle with the flags in the
    library's convention: FLAG_MIN_ZERO from the oracle's own flag, and
    FLAG_CONVERGED where the oracle's hard decisions reproduce the syndrome
    (the stop test of decoders.py:174-176 on its final posteriors)."""
    from oracle import oracle
    from qldpcsim_amd import _lib
    e, it, post, ofl = oracle.decode_batch("MS", H, syn, p, max_iter)
    conv = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(axis=1)
    fl = (np.where(conv, _lib.FLAG_CONVERGED, 0) | np.where(ofl & 1, _lib.FLAG_MIN_ZERO, 0)).astype(np.int32)
    assert conv[it < max_iter].all()
    return e, it, post, fl


@functools.lru_cache(maxsize=None)
def _oracle(which, max_iter, count=N_MIX, seed=1234):
    """The oracle's decode of the channel syndromes, computed once and shared;
    a smaller batch is a prefix (half-shots decode independently)."""
    out = _oracle_decode(_half(which), _channel_syndromes(which, count, seed), P_MIX, max_iter)
    for a in out:
        a.setflags(write=False)
    return out


def _decode(H, syn, p, max_iter, bits, want_post):
    """Device decode of uint8 syndromes; returns numpy (ehat uint8, iters, post | None, flags)."""
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(np.array(syn), device="cuda:0")
    r = decoders.decode_batch(H, decoders.pack_bits(s) if bits else s, p, max_iter, algo="MS",
                              want_post=want_post, ehat_bits=bits)
    torch.cuda.synchronize()
    e = decoders.unpack_bits(r.ehat, H.shape[1]) if bits else r.ehat
    return (e.cpu().numpy(), r.iters.cpu().numpy(), r.post.cpu().numpy() if want_post else None,
            r.flags.cpu().numpy())


def _assert_same(got, want, label):
    e, it, post, fl = got
    we, wit, wpost, wfl = want
    assert np.array_equal(it, wit), f"{label}: iterations"
    assert np.array_equal(fl, wfl), f"{label}: flags"
    assert np.array_equal(e, we), f"{label}: hard decisions"
    if post is not None:
        assert np.array_equal(post.view(np.uint64), wpost.view(np.uint64)), f"{label}: posteriors"


def _kernel(H):
    from qldpcsim_amd import _lib, schedule
    lp, lr = schedule.pack_layers(None, H.shape[0])           # flooding: one layer of every row
    return _lib.kernel_name(H, lp, lr, "MS", 0)


def test_chosen_p_mixes_early_and_late_rows():
    """The premise of the channel cases: inside groups of four consecutive
    half-shots (one wave's rows) some stop within 4 iterations while another
    runs all 50, in both halves, so rows finish and refill at different times."""
    for which in ("Hx", "Hz"):
        it = _oracle(which, 50)[1]
        g = it[:N_MIX - N_MIX % 4].reshape(-1, 4)
        mixed = int(((g.min(axis=1) <= 4) & (g.max(axis=1) == 50)).sum())
        assert mixed >= 3, (which, mixed)
        assert (it <= 3).sum() >= 20 and (it == 50).sum() >= 20, which


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_channel_syndromes_match_oracle_and_lds_twin(which, max_iter, qopt):
    H = _half(which)
    syn = _channel_syndromes(which)
    want = _oracle(which, max_iter)
    assert _kernel(H) == QC_KERNEL
    for B in BATCHES:
        w = tuple(a[:B] for a in want)
        for bits in (False, True):
            for want_post in (False, True):
                _assert_same(_decode(H, syn[:B], P_MIX, max_iter, bits, want_post), w,
                             f"{which} it={max_iter} B={B} bits={bits} post={want_post}")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    for B in BATCHES:
        w = tuple(a[:B] for a in want)
        for bits in (False, True):
            _assert_same(_decode(H, syn[:B], P_MIX, max_iter, bits, True), w,
                         f"twin {which} it={max_iter} B={B} bits={bits}")


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_uniform_syndromes_match_oracle_and_lds_twin(which, qopt):
    """The benchmark's input: uniform random syndromes, nothing converges."""
    H = _half(which)
    syn = np.random.default_rng(77).integers(0, 2, (256, H.shape[0]), dtype=np.uint8)
    want = _oracle_decode(H, syn, 0.05 / 3, 50)
    assert (want[1] == 50).all()
    assert _kernel(H) == QC_KERNEL
    for bits in (False, True):
        _assert_same(_decode(H, syn, 0.05 / 3, 50, bits, True), want, f"{which} uniform bits={bits}")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    _assert_same(_decode(H, syn, 0.05 / 3, 50, True, True), want, f"twin {which} uniform")


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_zero_prior_flags_min_zero(which, qopt):
    """p = 0.5: L = 0, every first minimum is zero (FLAG_MIN_ZERO)."""
    from qldpcsim_amd import _lib
    H = _half(which)
    syn = _channel_syndromes(which)[:37]
    want = _oracle_decode(H, syn, 0.5, 6)
    assert (want[3] & _lib.FLAG_MIN_ZERO).all()
    got = _decode(H, syn, 0.5, 6, True, True)
    _assert_same(got, want, f"{which} L=0")
    qopt(flood_qc=0)
    _assert_same(_decode(H, syn, 0.5, 6, True, True), got, f"twin {which} L=0")


def test_same_shape_unknown_code_runs_the_lds_twin():
    """Two rows of different blocks swapped: same shape and degrees, but no
    generated table expands to it."""
    H = _half("Hx").copy()
    H[[3, 40]] = H[[40, 3]]
    assert _kernel(H) == LDS_TWIN
    rng = np.random.default_rng(5)
    e = (rng.random((300, H.shape[1])) < P_MIX).astype(np.uint8)
    syn = (e @ H.T % 2).astype(np.uint8)
    want = _oracle_decode(H, syn, P_MIX, 50)
    for bits in (False, True):
        _assert_same(_decode(H, syn, P_MIX, 50, bits, True), want, f"swapped rows bits={bits}")


def test_work_queue_and_static_stride_agree_past_one_resident_pass(qopt):
    """More half-shots than the grid's rows hold at once (rows then refill from
    the ticket queue, or stride statically): both equal the oracle."""
    count = 20001
    H = _half("Hz")
    syn = _channel_syndromes("Hz", count, 99)
    want = _oracle("Hz", 50, count, 99)
    _assert_same(_decode(H, syn, P_MIX, 50, True, False), want, "queue")
    qopt(static_sched=1)
    _assert_same(_decode(H, syn, P_MIX, 50, True, False), want, "static stride")
    _assert_same(_decode(H, syn[:N_MIX], P_MIX, 50, False, True), tuple(a[:N_MIX] for a in want), "static, 1001")
    qopt(static_sched=0, wg_per_cu=1)                      # fewer rows: more refills per row
    _assert_same(_decode(H, syn, P_MIX, 50, False, True), want, "queue, one workgroup per CU")

"""The single-bit bookkeeping and the rare-path join of the register-resident
flooding min-sum kernel's check node (ms_flood_kernel<8, 4> on LP118_0,
DESIGN.md §3.1.1; switches QLDPC_QC_S31 and QLDPC_QC_RARE32 of ms_flood_qc.h).
Check block B's syndrome bit is carried at bit 31 as synreg << (31 - B), the
sign product, the stop test and the max_iter parity are read there, and the
wave-uniform rare branch (a zero or infinite minimum) redefines the two float32
words instead of the float64 minima. Syndromes that set one check block at a
time (blocks 0 and 14 are the ends of the shift), one check at either end of a
block, none and all; channel syndromes whose rows stop at different trips of one
wave; L = 0, where every check takes the rare branch, and a negative L; rows
that finish, write and restart. Everything bit for bit (posteriors as 64-bit
patterns) against the CPU oracle and the LDS twin (option flood_qc = 0)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC_KERNEL = "ms_flood_kernel<8, 4>"
LDS_TWIN = "ms_flood_lds_kernel<8, 4>"
P_ERR = 0.04          # the errors behind the channel syndromes; also the prior of most cases
N_ROWS = 67           # 16 groups of four and three: the last wave has an idle row
LIFT, MB = 16, 15     # LP118_0: 15 check blocks of 16 checks per half
N_RESTART = 2 * 4096 + N_ROWS


def _half(which):
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP118_0")
    return Hx if which == "Hx" else Hz


def _structured(m):
    """All-zero, all-one, the 15 patterns that set exactly one check block, and
    a single check at position 0 of a block and at position 15 of another."""
    assert m == LIFT * MB
    rows = [np.zeros(m, np.uint8), np.ones(m, np.uint8)]
    for b in range(MB):
        r = np.zeros(m, np.uint8)
        r[LIFT * b:LIFT * (b + 1)] = 1
        rows.append(r)
    for c in (LIFT * 7, LIFT * 14 + 15):
        r = np.zeros(m, np.uint8)
        r[c] = 1
        rows.append(r)
    return np.stack(rows)


def _channel(H, count, seed):
    e = (np.random.default_rng(seed).random((count, H.shape[1])) < P_ERR).astype(np.uint8)
    return (e @ H.T % 2).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _syndromes(which):
    """N_ROWS half-shots: channel rows first (so that every batch size starts
    with them), the structured ones from row N_CH on."""
    H = _half(which)
    st = _structured(H.shape[0])
    syn = np.concatenate([_channel(H, N_ROWS - len(st), 29), st])
    syn.setflags(write=False)
    return syn


N_CH = N_ROWS - (2 + MB + 2)


def _oracle_decode(H, syn, p, max_iter):
    """(ehat, iters, post, flags) of the CPU oracle, the flags in the library's
    convention (tests/test_gpu_flood_qc.py)."""
    from oracle import oracle
    from qldpcsim_amd import _lib
    e, it, post, ofl = oracle.decode_batch("MS", H, syn, p, max_iter)
    conv = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(axis=1)
    fl = (np.where(conv, _lib.FLAG_CONVERGED, 0) | np.where(ofl & 1, _lib.FLAG_MIN_ZERO, 0)).astype(np.int32)
    assert conv[it < max_iter].all()
    out = (e, it, post, fl)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(which, p, max_iter):
    return _oracle_decode(_half(which), _syndromes(which), p, max_iter)


def _decode(H, syn, p, max_iter, bits):
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(np.array(syn), device="cuda:0")
    r = decoders.decode_batch(H, decoders.pack_bits(s) if bits else s, p, max_iter, algo="MS",
                              want_post=True, ehat_bits=bits)
    torch.cuda.synchronize()
    e = decoders.unpack_bits(r.ehat, H.shape[1]) if bits else r.ehat
    return e.cpu().numpy(), r.iters.cpu().numpy(), r.post.cpu().numpy(), r.flags.cpu().numpy()


def _assert_same(got, want, label):
    e, it, post, fl = got
    we, wit, wpost, wfl = want
    assert np.array_equal(it, wit), f"{label}: iterations"
    assert np.array_equal(fl, wfl), f"{label}: flags"
    assert np.array_equal(e, we), f"{label}: hard decisions"
    assert np.array_equal(post.view(np.uint64), wpost.view(np.uint64)), f"{label}: posteriors"


def _kernel(H):
    from qldpcsim_amd import _lib, schedule
    lp, lr = schedule.pack_layers(None, H.shape[0])           # flooding: one layer of every row
    return _lib.kernel_name(H, lp, lr, "MS", 0)


def _check_slices(H, syn, want, p, max_iter, label):
    """Batches of 1, 3, 5 and N_ROWS, both formats; the small batches once on
    the leading channel rows and once on structured rows (all-one first, then
    the one-block patterns), which are decoded as batches of their own."""
    for lo, count in ((0, 1), (0, 3), (0, 5), (N_CH + 1, 1), (N_CH + 1, 3), (N_CH + 12, 5), (0, N_ROWS)):
        sl = slice(lo, lo + count)
        for bits in (True, False):
            _assert_same(_decode(H, syn[sl], p, max_iter, bits), tuple(a[sl] for a in want),
                         f"{label} rows {lo}+{count} it={max_iter} bits={bits}")


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_syndromes_exercise_what_they_are_chosen_for(which):
    """The premise of the cases below, from the oracle alone: among the channel
    rows some group of four (one wave) holds a half-shot that stops within 4
    iterations beside one that runs all 50; the all-zero row stops at its first
    stop test; every other structured row is undecodable and runs to max_iter,
    so the kernel tests its blocks' bits at every trip and in the final parity."""
    from qldpcsim_amd import _lib
    _, it, post, fl = _oracle(which, P_ERR, 50)
    groups = it[:N_CH - N_CH % 4].reshape(-1, 4)
    assert ((groups.min(axis=1) <= 4) & (groups.max(axis=1) == 50)).any(), it[:N_CH]
    assert it[N_CH] == 1 and fl[N_CH] & _lib.FLAG_CONVERGED
    assert (it[N_CH + 1:] == 50).all() and not (fl[N_CH + 1:] & _lib.FLAG_CONVERGED).any()
    assert np.isfinite(post).all()


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_block_and_channel_syndromes_match_oracle_and_lds_twin(which, max_iter, qopt):
    H = _half(which)
    syn = _syndromes(which)
    want = _oracle(which, P_ERR, max_iter)
    assert _kernel(H) == QC_KERNEL
    _check_slices(H, syn, want, P_ERR, max_iter, which)
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    _check_slices(H, syn, want, P_ERR, max_iter, f"twin {which}")


@pytest.mark.parametrize("max_iter", [1, 6])
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_zero_prior_takes_the_rare_branch_in_every_check(which, max_iter, qopt):
    """p = 0.5: L = 0, every first minimum is zero, so every check block of
    every trip runs the rare branch and every half-shot carries FLAG_MIN_ZERO."""
    from qldpcsim_amd import _lib
    H = _half(which)
    syn = _syndromes(which)
    want = _oracle(which, 0.5, max_iter)
    assert (want[3] & _lib.FLAG_MIN_ZERO).all()
    assert _kernel(H) == QC_KERNEL
    _check_slices(H, syn, want, 0.5, max_iter, f"{which} L=0")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    _check_slices(H, syn, want, 0.5, max_iter, f"twin {which} L=0")


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_negative_prior(which, qopt):
    """p = 0.7: L < 0, nearly every posterior negative, so the sign product and
    the parity words are mostly ones where they are mostly zeros otherwise."""
    H = _half(which)
    syn = _syndromes(which)
    for max_iter in (2, 50):
        want = _oracle(which, 0.7, max_iter)
        if max_iter == 50:
            assert (want[2] < 0).mean() > 0.8
        assert _kernel(H) == QC_KERNEL
        _check_slices(H, syn, want, 0.7, max_iter, f"{which} p=0.7")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    _check_slices(H, syn, _oracle(which, 0.7, 50), 0.7, 50, f"twin {which} p=0.7")


def test_rows_finish_write_and_restart(qopt):
    """More than twice the half-shots that one workgroup per CU holds at once
    (256 CUs x 16 rows): every row reads a new syndrome register and starts
    again beside rows that go on."""
    H = _half("Hz")
    syn = _channel(H, N_RESTART, 9731)
    want = _oracle_decode(H, syn, P_ERR, 50)
    assert (want[1] <= 3).sum() >= 100 and (want[1] == 50).sum() >= 100
    qopt(wg_per_cu=1)
    assert _kernel(H) == QC_KERNEL
    _assert_same(_decode(H, syn, P_ERR, 50, True), want, "Hz restart, bits")
    _assert_same(_decode(H, syn, P_ERR, 50, False), want, "Hz restart, bytes")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    _assert_same(_decode(H, syn, P_ERR, 50, True), want, "twin Hz restart, bits")

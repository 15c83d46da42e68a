"""The per-variable float64 posteriors of the register-resident flooding
min-sum kernel (ms_flood_kernel<8, 4> on LP118_0): the VN
pass forms P = L + (double)S once per variable block and a check reads it by
rotating its low and high word. Priors at which the float64 posterior carries
more than the float32 column sum (negative L, |L| near 20.7, a small positive
L), a batch whose last wave has an idle row, and rows that finish, write
float64 posterior rows and restart many times; everything bit for bit
(posteriors as 64-bit patterns, which see a low word rotated by the wrong
amount) against the CPU oracle and the LDS twin (option flood_qc = 0)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC_KERNEL = "ms_flood_kernel<8, 4>"
LDS_TWIN = "ms_flood_lds_kernel<8, 4>"
P_ERR = 0.04          # the errors behind the syndromes, whatever prior decodes them
N_ROWS = 67           # 16 groups of four and three: the last wave has an idle row
PRIORS = (0.7, 1e-9, 0.3)   # L = -0.85 (96 % of posteriors negative), 20.7, 0.85
N_REFILL = 1001


def _half(which):
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP118_0")
    return Hx if which == "Hx" else Hz


@functools.lru_cache(maxsize=None)
def _syndromes(which):
    H = _half(which)
    e = (np.random.default_rng(11).random((N_ROWS, H.shape[1])) < P_ERR).astype(np.uint8)
    syn = (e @ H.T % 2).astype(np.uint8)
    syn.setflags(write=False)
    return syn


def _oracle_decode(H, syn, p, max_iter):
    """(ehat, iters, post, flags, oracle flags) of the CPU oracle, the flags in
    the library's convention (tests/test_gpu_flood_qc.py)."""
    from oracle import oracle
    from qldpcsim_amd import _lib
    e, it, post, ofl = oracle.decode_batch("MS", H, syn, p, max_iter)
    conv = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(axis=1)
    fl = (np.where(conv, _lib.FLAG_CONVERGED, 0) | np.where(ofl & 1, _lib.FLAG_MIN_ZERO, 0)).astype(np.int32)
    assert conv[it < max_iter].all()
    out = (e, it, post, fl, np.asarray(ofl))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(which, p, max_iter):
    return _oracle_decode(_half(which), _syndromes(which), p, max_iter)


def _decode(H, syn, p, max_iter, bits, want_post=True):
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(np.array(syn), device="cuda:0")
    r = decoders.decode_batch(H, decoders.pack_bits(s) if bits else s, p, max_iter, algo="MS",
                              want_post=want_post, ehat_bits=bits)
    torch.cuda.synchronize()
    e = decoders.unpack_bits(r.ehat, H.shape[1]) if bits else r.ehat
    return e.cpu().numpy(), r.iters.cpu().numpy(), r.post.cpu().numpy(), r.flags.cpu().numpy()


def _assert_same(got, want, label):
    e, it, post, fl = got
    we, wit, wpost, wfl = want[:4]
    assert np.array_equal(it, wit), f"{label}: iterations"
    assert np.array_equal(fl, wfl), f"{label}: flags"
    assert np.array_equal(e, we), f"{label}: hard decisions"
    assert np.array_equal(post.view(np.uint64), wpost.view(np.uint64)), f"{label}: posteriors"


def _kernel(H):
    from qldpcsim_amd import _lib, schedule
    lp, lr = schedule.pack_layers(None, H.shape[0])           # flooding: one layer of every row
    return _lib.kernel_name(H, lp, lr, "MS", 0)


@pytest.mark.parametrize("p", PRIORS)
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_priors_exercise_what_they_are_chosen_for(which, p):
    """The premise of the cases below, from the oracle alone: half-shots of 2
    to 5 iterations beside some that run all 50, finite posteriors, no oracle
    flag; at p = 0.7 nearly every posterior is negative."""
    _, it, post, _, ofl = _oracle(which, p, 50)
    assert ((it >= 2) & (it <= 5)).sum() >= 20 and 3 <= (it == 50).sum() <= 10, (which, p, np.bincount(it))
    assert np.isfinite(post).all()
    assert not ofl.any()
    if p == 0.7:
        assert (post < 0).mean() > 0.9


@pytest.mark.parametrize("max_iter", [50, 1])
@pytest.mark.parametrize("p", PRIORS)
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_posteriors_match_oracle_and_lds_twin(which, p, max_iter, qopt):
    H = _half(which)
    syn = _syndromes(which)
    want = _oracle(which, p, max_iter)
    assert _kernel(H) == QC_KERNEL
    for bits in (True, False):
        _assert_same(_decode(H, syn, p, max_iter, bits), want, f"{which} p={p} it={max_iter} bits={bits}")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    for bits in (True, False):
        _assert_same(_decode(H, syn, p, max_iter, bits), want, f"twin {which} p={p} it={max_iter} bits={bits}")


def _channel(H, count, seed):
    e = (np.random.default_rng(seed).random((count, H.shape[1])) < P_ERR).astype(np.uint8)
    return (e @ H.T % 2).astype(np.uint8)


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_posterior_rows_with_one_workgroup_per_cu(which, qopt):
    """1,001 half-shots of mixed iteration counts, bytes, posteriors on, one
    workgroup per CU: rows finish at different trips and write their float64
    rows from P while their neighbours go on."""
    H = _half(which)
    syn = _channel(H, N_REFILL, 1234)
    want = _oracle_decode(H, syn, P_ERR, 50)
    assert (want[1] <= 3).sum() >= 20 and (want[1] == 50).sum() >= 20
    qopt(wg_per_cu=1)
    assert _kernel(H) == QC_KERNEL
    _assert_same(_decode(H, syn, P_ERR, 50, False), want, f"{which} one workgroup per CU")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    _assert_same(_decode(H, syn, P_ERR, 50, False), want, f"twin {which}")


def test_rows_restart_with_posterior_rows(qopt):
    """More than twice the half-shots that one workgroup per CU holds at once
    (256 CUs x 16 rows): every row writes float64 rows from P and restarts
    (the Hz counterpart is tests/test_gpu_flood_qc.py's queue case)."""
    H = _half("Hx")
    syn = _channel(H, 2 * 4096 + N_ROWS, 4321)
    want = _oracle_decode(H, syn, P_ERR, 50)
    qopt(wg_per_cu=1)
    assert _kernel(H) == QC_KERNEL
    _assert_same(_decode(H, syn, P_ERR, 50, False), want, "Hx restart, bytes")
    _assert_same(_decode(H, syn, P_ERR, 50, True), want, "Hx restart, bits")

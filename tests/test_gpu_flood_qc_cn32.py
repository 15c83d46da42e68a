"""The float32-domain check node of the register-resident flooding min-sum
kernel (ms_flood_kernel<8, 4> on LP118_0): the minimum and
the select are taken on bits(fl32(beta * |v|)) as unsigned integers, and a wave
with a zero or non-finite float32 minimum takes the float64 check node. Bit
for bit (iterations, flags, hard decisions, float64 posterior rows as 64-bit
patterns) against the CPU oracle and the LDS twin (option flood_qc = 0), which
keeps the float64 arithmetic: 67 half-shots per half (the last wave has an
idle row) at four priors, max_iter 1, 2 and 50, both I/O formats, beta = 0.75
and the non-dyadic 0.8 (fl64(beta * x) rounds); L = 0, where every check takes
the float64 path and sets FLAG_MIN_ZERO; and 8,259 half-shots with one
workgroup per CU, more than twice what the grid holds at once, so rows finish,
write their posterior rows and restart on further half-shots. The messages of the first
iterations are massive exact ties (every v2c = L)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC_KERNEL = "ms_flood_kernel<8, 4>"
LDS_TWIN = "ms_flood_lds_kernel<8, 4>"
P_ERR = 0.04          # the errors behind the syndromes, whatever prior decodes them
N_ROWS = 67           # 16 groups of four and three: the last wave has an idle row
PRIORS = (0.04, 0.3, 0.7, 1e-9)
BETAS = (0.75, 0.8)
N_REFILL = 2 * 4096 + 67   # more than twice what one workgroup per CU holds at once (256 CUs x 16 rows)


def _half(which):
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP118_0")
    return Hx if which == "Hx" else Hz


@functools.lru_cache(maxsize=None)
def _syndromes(which, count=N_ROWS, seed=11):
    H = _half(which)
    e = (np.random.default_rng(seed).random((count, H.shape[1])) < P_ERR).astype(np.uint8)
    syn = (e @ H.T % 2).astype(np.uint8)
    syn.setflags(write=False)
    return syn


@functools.lru_cache(maxsize=None)
def _oracle(which, p, max_iter, beta, count=N_ROWS, seed=11):
    """(ehat, iters, post, flags) of the CPU oracle, the flags in the library's
    convention (tests/test_gpu_flood_qc.py); computed once per case and shared."""
    from oracle import oracle
    from qldpcsim_amd import _lib
    H, syn = _half(which), _syndromes(which, count, seed)
    e, it, post, ofl = oracle.decode_batch("MS", H, syn, p, max_iter, beta=beta)
    conv = ((e.astype(np.int64) @ H.T.astype(np.int64)) % 2 == syn).all(axis=1)
    fl = (np.where(conv, _lib.FLAG_CONVERGED, 0) | np.where(ofl & 1, _lib.FLAG_MIN_ZERO, 0)).astype(np.int32)
    assert conv[it < max_iter].all()
    out = (e, it, post, fl)
    for a in out:
        a.setflags(write=False)
    return out


def _decode(H, syn, p, max_iter, beta, bits):
    import torch
    from qldpcsim_amd import decoders
    s = torch.as_tensor(np.array(syn), device="cuda:0")
    r = decoders.decode_batch(H, decoders.pack_bits(s) if bits else s, p, max_iter, algo="MS", beta=beta,
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


def _both_kernels_both_formats(which, p, max_iter, beta, qopt, count=N_ROWS, seed=11, formats=(True, False)):
    H = _half(which)
    syn = _syndromes(which, count, seed)
    want = _oracle(which, p, max_iter, beta, count, seed)
    label = f"{which} p={p} it={max_iter} beta={beta}"
    assert _kernel(H) == QC_KERNEL
    for bits in formats:
        _assert_same(_decode(H, syn, p, max_iter, beta, bits), want, f"{label} bits={bits}")
    qopt(flood_qc=0)
    assert _kernel(H) == LDS_TWIN
    for bits in formats:
        _assert_same(_decode(H, syn, p, max_iter, beta, bits), want, f"twin {label} bits={bits}")
    return want


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("p", PRIORS)
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_check_node_matches_oracle_and_lds_twin(which, p, max_iter, beta, qopt):
    _both_kernels_both_formats(which, p, max_iter, beta, qopt)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_zero_prior_takes_the_float64_path_and_flags_min_zero(which, beta, qopt):
    """p = 0.5: L = 0, every v is 0, every check of every iteration has w1 == 0."""
    from qldpcsim_amd import _lib
    want = _both_kernels_both_formats(which, 0.5, 6, beta, qopt)
    assert (want[3] & _lib.FLAG_MIN_ZERO).all()


@pytest.mark.parametrize("which,beta", [("Hx", 0.8), ("Hz", 0.75)])
def test_rows_restart_with_one_workgroup_per_cu(which, beta, qopt):
    """8,259 half-shots of mixed iteration counts, bytes, float64 posterior
    rows, one workgroup per CU: the grid then holds 256 CUs x 16 rows = 4,096
    half-shots at once, less than half the batch, so rows finish at different
    trips, write their rows and take further half-shots from the queue while
    their neighbours go on (a quick row many, a 50-iteration row perhaps none)."""
    import torch
    from qldpcsim_amd import _lib, schedule
    want = _oracle(which, P_ERR, 50, beta, N_REFILL, 1234)
    assert (want[1] <= 3).sum() >= 20 and (want[1] == 50).sum() >= 20
    qopt(wg_per_cu=1)
    H = _half(which)
    waves, wgs, _ = _lib.launch_info(H, *schedule.pack_layers(None, H.shape[0]), "MS", 0)
    resident = torch.cuda.get_device_properties(0).multi_processor_count * wgs * waves * 4
    assert N_REFILL > 2 * resident, (waves, wgs, resident)
    _both_kernels_both_formats(which, P_ERR, 50, beta, qopt, N_REFILL, 1234, formats=(False,))

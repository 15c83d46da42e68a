"""The 32-bit leave-one-out check node of the register-resident flooding
min-sum kernel (ms_flood_kernel<8, 4> on LP118_0; switch
QLDPC_QC_LOO = 2 of ms_flood_qc.h): per edge w_e = bits(fl32(bs * |v_e|)) first,
then the leave-one-out minima of the words as unsigned integers; a wave with a
zero or infinite float32 word among the network's mA, mB and oA takes the
float64 select form. Bit for bit (iterations, flags, hard decisions, float64
posterior rows as 64-bit patterns) against the CPU oracle and the LDS twin
(option flood_qc = 0), on the shapes of test_gpu_flood_qc_loo.py: both halves;
channel syndromes at priors 0.04, 0.5 (L = 0: every check of every trip takes
the fallback and every half-shot carries FLAG_MIN_ZERO), 0.7 and 1e-9, and
uniform syndromes; max_iter 1, 2 and 50; beta 0.75 and 0.8; batches of 1, 3, 5
and 67; both I/O formats; 8,259 half-shots with one workgroup per CU. And one
case that only the 32-bit test can get wrong: beta = 1e-47 at prior 0.04, where
every product beta * |v_e| rounds to float32 zero while the float64 minima are
not zero, so every check takes the fallback on words that are all zero and no
half-shot may carry FLAG_MIN_ZERO."""
import numpy as np
import pytest

from test_gpu_flood_qc_loo import (BATCHES, BETAS, CASES, N_RESTART, N_ROWS, P_ERR, QC_KERNEL, _both_kernels, _half,
                                   _launch, _oracle)

pytestmark = pytest.mark.gpu

TINY_BETA = 1e-47     # beta * |L| = 3.2e-47 is below half the smallest float32 subnormal (7.0e-46)


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_launch_geometry_is_unchanged(which):
    """four waves per workgroup, two workgroups per CU (two waves per SIMD), no LDS"""
    assert _launch(_half(which)) == (QC_KERNEL, (4, 2, 0))


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_check_node_matches_oracle_and_lds_twin(which, case, max_iter):
    from qldpcsim_amd import _lib
    kind, p = CASES[case]
    for beta in BETAS:
        want = _both_kernels(which, kind, p, max_iter, beta, BATCHES)
        flagged = (want[3] & _lib.FLAG_MIN_ZERO) != 0
        assert flagged.all() if case == "zero_prior" else not flagged.any(), (case, beta)


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_products_that_round_to_float32_zero(which, max_iter):
    """beta = 1e-47: every message is +-0 in float32, every posterior stays L and
    every |v_e| is |L| = 3.18, so the float64 minima are not zero (the oracle
    flags nothing) while every word of the 32-bit network is: the class test
    fires on every check and the fallback must not raise FLAG_MIN_ZERO."""
    from qldpcsim_amd import _lib
    L = np.log((1 - 0.04) / 0.04)
    assert np.float32(TINY_BETA * L) == 0.0 and TINY_BETA * L > 0.0
    e, it, post, fl = _oracle(which, "channel", 0.04, max_iter, TINY_BETA)
    assert not (fl & _lib.FLAG_MIN_ZERO).any()
    assert (post == post[0, 0]).all() and abs(post[0, 0] - L) < 1e-12     # no message ever moved a posterior
    _both_kernels(which, "channel", 0.04, max_iter, TINY_BETA, BATCHES)


@pytest.mark.parametrize("which,beta", [("Hx", 0.8), ("Hz", 0.75)])
def test_rows_restart_with_one_workgroup_per_cu(which, beta, qopt):
    """8,259 half-shots of mixed iteration counts, float64 posterior rows, one
    workgroup per CU: less than half the batch is resident at once, so rows
    finish at different trips, write their rows and take further half-shots
    while their neighbours go on."""
    import torch
    from qldpcsim_amd import _lib, schedule
    want = _oracle(which, "channel", P_ERR, 50, beta, N_RESTART, 4321)
    assert (want[1] <= 3).sum() >= 20 and (want[1] == 50).sum() >= 20
    qopt(wg_per_cu=1)
    H = _half(which)
    waves, wgs, _ = _lib.launch_info(H, *schedule.pack_layers(None, H.shape[0]), "MS", 0)
    resident = torch.cuda.get_device_properties(0).multi_processor_count * wgs * waves * 4
    assert N_RESTART > 2 * resident, (waves, wgs, resident)
    _both_kernels(which, "channel", P_ERR, 50, beta, (N_RESTART,), formats=(False, True), count=N_RESTART,
                  seed=4321)
    assert N_ROWS % 4 == 3                                   # (the small batches end on a wave with an idle row)

"""The leave-one-out check node of the register-resident flooding min-sum
kernel (ms_flood_kernel<8, 4> on LP118_0; switch QLDPC_QC_LOO
of ms_flood_qc.h): per edge the minimum over the other edges and fl32(beta *
that), beta carrying the check's sign, in place of min1 / min2 and a compare and
select; a wave with a zero or infinite top minimum takes the select form. Bit
for bit (iterations, flags, hard decisions, float64 posterior rows as 64-bit
patterns) against the CPU oracle and the LDS twin (option flood_qc = 0), which
keeps min1 / min2: both halves; channel syndromes at priors 0.04 (rows of one
wave stop at different trips), 0.5 (L = 0: every check of every trip takes the
select form and every half-shot carries FLAG_MIN_ZERO), 0.7 (L < 0) and 1e-9,
and uniform random syndromes (the headline's, which run to max_iter); max_iter
1, 2 and 50; beta 0.75 and the non-dyadic 0.8; batches of 1, 3, 5 and 67 (the
last wave has an idle row); both I/O formats; and 8,259 half-shots with one
workgroup per CU, more than twice what the grid holds at once, so rows finish,
write their posterior rows and restart. Iteration 1 of every decode has all
eight |v_e| equal (every v2c = L), so full ties are in every case."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

QC_KERNEL = "ms_flood_kernel<8, 4>"
LDS_TWIN = "ms_flood_lds_kernel<8, 4>"
P_ERR = 0.04          # the errors behind the channel syndromes, whatever prior decodes them
N_ROWS = 67           # 16 groups of four and three: the last wave has an idle row
BATCHES = (1, 3, 5, N_ROWS)
BETAS = (0.75, 0.8)
# (name, syndromes, prior)
CASES = {
    "channel_p04": ("channel", 0.04),
    "uniform": ("uniform", 0.05 / 3),
    "zero_prior": ("channel", 0.5),
    "negative_prior": ("channel", 0.7),
    "tiny_prior": ("channel", 1e-9),
}
N_RESTART = 2 * 4096 + 67   # more than twice what one workgroup per CU holds at once (256 CUs x 16 rows)


def _half(which):
    from qldpcsim_amd import codes
    Hx, Hz = codes.load_code("LP118_0")
    return Hx if which == "Hx" else Hz


@functools.lru_cache(maxsize=None)
def _syndromes(which, kind, count=N_ROWS, seed=23):
    H = _half(which)
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        syn = rng.integers(0, 2, (count, H.shape[0]), dtype=np.uint8)
    else:
        e = (rng.random((count, H.shape[1])) < P_ERR).astype(np.uint8)
        syn = (e @ H.T % 2).astype(np.uint8)
    syn.setflags(write=False)
    return syn


@functools.lru_cache(maxsize=None)
def _oracle(which, kind, p, max_iter, beta, count=N_ROWS, seed=23):
    """(ehat, iters, post, flags) of the CPU oracle, the flags in the library's
    convention (tests/test_gpu_flood_qc.py); computed once per case and shared."""
    from oracle import oracle
    from qldpcsim_amd import _lib
    H, syn = _half(which), _syndromes(which, kind, count, seed)
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


def _launch(H):
    from qldpcsim_amd import _lib, schedule
    lp, lr = schedule.pack_layers(None, H.shape[0])           # flooding: one layer of every row
    return _lib.kernel_name(H, lp, lr, "MS", 0), tuple(_lib.launch_info(H, lp, lr, "MS", 0))


def _both_kernels(which, kind, p, max_iter, beta, batches, formats=(True, False), count=N_ROWS, seed=23):
    from qldpcsim_amd import _lib
    H = _half(which)
    syn = _syndromes(which, kind, count, seed)
    want = _oracle(which, kind, p, max_iter, beta, count, seed)
    label = f"{which} {kind} p={p} it={max_iter} beta={beta}"
    for kernel, opts in ((QC_KERNEL, {}), (LDS_TWIN, {"flood_qc": 0})):
        with _lib.options(**opts):
            assert _launch(H)[0] == kernel
            for b in batches:
                for bits in formats:
                    _assert_same(_decode(H, syn[:b], p, max_iter, beta, bits), tuple(a[:b] for a in want),
                                 f"{kernel} {label} batch={b} bits={bits}")
    return want


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_launch_geometry_is_unchanged(which):
    """four waves per workgroup, two workgroups per CU (two waves per SIMD), no LDS"""
    assert _launch(_half(which)) == (QC_KERNEL, (4, 2, 0))


@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_syndromes_exercise_what_they_are_chosen_for(which):
    """The premise of the cases below, from the oracle alone: at p = 0.04 some
    group of four channel rows (one wave) holds a half-shot that stops within 4
    iterations beside one that runs longer than 20; the uniform syndromes run to
    max_iter; L = 0 flags every half-shot and no other prior flags any; L < 0
    leaves most posteriors negative."""
    from qldpcsim_amd import _lib
    it = _oracle(which, "channel", 0.04, 50, 0.75)[1]
    groups = it[:N_ROWS - N_ROWS % 4].reshape(-1, 4)
    assert ((groups.min(axis=1) <= 4) & (groups.max(axis=1) > 20)).any(), it
    assert (_oracle(which, "uniform", 0.05 / 3, 50, 0.75)[1] == 50).all()
    assert (_oracle(which, "channel", 0.5, 2, 0.75)[3] & _lib.FLAG_MIN_ZERO).all()
    for kind, p in (("channel", 0.04), ("uniform", 0.05 / 3), ("channel", 0.7), ("channel", 1e-9)):
        assert not (_oracle(which, kind, p, 50, 0.8)[3] & _lib.FLAG_MIN_ZERO).any(), (kind, p)
    assert (_oracle(which, "channel", 0.7, 50, 0.75)[2] < 0).mean() > 0.8


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("which", ["Hx", "Hz"])
def test_check_node_matches_oracle_and_lds_twin(which, case, max_iter):
    kind, p = CASES[case]
    for beta in BETAS:
        want = _both_kernels(which, kind, p, max_iter, beta, BATCHES)
    if case == "zero_prior":
        from qldpcsim_amd import _lib
        assert (want[3] & _lib.FLAG_MIN_ZERO).all()


@pytest.mark.parametrize("which,beta", [("Hx", 0.8), ("Hz", 0.75)])
def test_rows_restart_with_one_workgroup_per_cu(which, beta, qopt):
    """8,259 half-shots of mixed iteration counts, float64 posterior rows, one
    workgroup per CU: the grid then holds 256 CUs x 16 rows = 4,096 half-shots
    at once, less than half the batch, so rows finish at different trips, write
    their rows and take further half-shots while their neighbours go on."""
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

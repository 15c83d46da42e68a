"""The host path the generic kernel's two prior twins share (capi_decode.cpp),
pinned without a GPU: the exact kernel names the three *_kernel_name entry
points answer for row degree 7, row degree 8 and neither, both algorithms and
both schedules, and the error code and message of every refusal that twin_limits
and the validators make before any HIP call."""
import ctypes

import numpy as np
import pytest

from qldpcsim_amd import _lib, codes, simulator

L = _lib.lib
P = _lib.ptr
EINVAL, EUNSUP, EHIP = _lib.QLDPC_EINVAL, _lib.QLDPC_EUNSUP, _lib.QLDPC_EHIP
NO_DEVICE = _lib.device_count() == 0

# code -> the DC template argument of the generic kernels (uniform row degree 7 / 8, else 0)
CODES = {"LP04_0": 7, "LP118_0": 8, "steane": 0}

NAMES = {
    ("prior", "LP04_0"): ["decode_prior_kernel<0, false, 7>", "decode_prior_kernel<0, true, 7>",
                          "decode_prior_kernel<1, false, 7>", "decode_prior_kernel<1, true, 7>"],
    ("prior", "LP118_0"): ["decode_prior_kernel<0, false, 8>", "decode_prior_kernel<0, true, 8>",
                           "decode_prior_kernel<1, false, 8>", "decode_prior_kernel<1, true, 8>"],
    ("prior", "steane"): ["decode_prior_kernel<0, false, 0>", "decode_prior_kernel<0, true, 0>",
                          "decode_prior_kernel<1, false, 0>", "decode_prior_kernel<1, true, 0>"],
    ("vprior", "LP04_0"): ["decode_vprior_kernel<0, false, 7>", "decode_vprior_kernel<0, true, 7>",
                           "decode_vprior_kernel<1, false, 7>", "decode_vprior_kernel<1, true, 7>"],
    ("vprior", "LP118_0"): ["decode_vprior_kernel<0, false, 8>", "decode_vprior_kernel<0, true, 8>",
                            "decode_vprior_kernel<1, false, 8>", "decode_vprior_kernel<1, true, 8>"],
    ("vprior", "steane"): ["decode_vprior_kernel<0, false, 0>", "decode_vprior_kernel<0, true, 0>",
                           "decode_vprior_kernel<1, false, 0>", "decode_vprior_kernel<1, true, 0>"],
}

MSG_NO_DEVICE = "no HIP device was visible when the code/schedule was created"
MSG_NO_DEVICE_HOST = "no HIP device was visible when the code was created"
MSG_ALGO = "Unrecognized decoder type."
MSG_MAX_ITER = "max_iter must be >= 1 (the reference leaves e_hat unbound)"
MSG_PROB = "two-level priors: p0 and p1 must be probabilities (0 <= p <= 1)"
MSG_FOREIGN = "prior handle was built for a different code"
MSG_HBM = {"prior": "two-level priors: option force_hbm is set and there is no HBM-resident variant",
           "vprior": "per-variable priors: option force_hbm is set and there is no HBM-resident variant"}


def _err():
    return L.qldpc_last_error().decode()


def _schedules(H):
    m = H.shape[0]
    flooding = (np.array([0, m], np.int32), np.arange(m, dtype=np.int32))
    layered = simulator.pack_layers(simulator.layerize(H), m)
    return flooding, layered


def _name(fn, code, sched, algo):
    buf = ctypes.create_string_buffer(128)
    rc = fn(code.handle if code else None, sched.handle if sched else None, algo, buf, 128)
    return rc, buf.value.decode()


@pytest.mark.parametrize("name", sorted(CODES))
def test_kernel_names(name):
    H = codes.load_code(name)[0]
    code = _lib.Code(H)
    assert (H.sum(1) == CODES[name]).all() or CODES[name] == 0
    got = {"prior": [], "vprior": []}
    for algo in (0, 1):
        for lp, lr in _schedules(H):
            sched = code.schedule(lp, lr)
            got["prior"].append(_name(L.qldpc_decode_prior_kernel_name, code, sched, algo))
            got["vprior"].append(_name(L.qldpc_decode_vprior_kernel_name, code, sched, algo))
            # the scalar entry resolves a launch plan: past its argument checks it needs a device
            rc, s = _name(L.qldpc_decode_kernel_name, code, sched, algo)
            if NO_DEVICE:
                assert (rc, _err()) == (EHIP, MSG_NO_DEVICE)
            else:
                assert rc == _lib.QLDPC_OK and s
    for kind in ("prior", "vprior"):
        assert got[kind] == [(_lib.QLDPC_OK, s) for s in NAMES[(kind, name)]]


def test_kernel_name_argument_checks():
    H = codes.load_code("steane")[0]
    code = _lib.Code(H)
    other = _lib.Code(np.roll(H, 1, axis=1))
    sched = code.schedule(*_schedules(H)[0])
    for fn in (L.qldpc_decode_prior_kernel_name, L.qldpc_decode_vprior_kernel_name, L.qldpc_decode_kernel_name):
        assert _name(fn, None, sched, 0)[0] == EINVAL and _err() == "null argument"
        assert _name(fn, code, None, 0)[0] == EINVAL and _err() == "null argument"
        assert fn(code.handle, sched.handle, 0, None, 128) == EINVAL and _err() == "null argument"
        assert fn(code.handle, sched.handle, 0, ctypes.create_string_buffer(8), 0) == EINVAL
        assert _err() == "null argument"
        for algo in (2, 3, -1):
            assert _name(fn, code, sched, algo)[0] == EINVAL and _err() == MSG_ALGO
    for fn in (L.qldpc_decode_prior_kernel_name, L.qldpc_decode_vprior_kernel_name):
        assert _name(fn, other, sched, 0)[0] == EINVAL and _err() == "schedule was built for a different code"
    with _lib.options(force_hbm=1):
        assert _name(L.qldpc_decode_prior_kernel_name, code, sched, 0)[0] == EUNSUP and _err() == MSG_HBM["prior"]
        assert _name(L.qldpc_decode_vprior_kernel_name, code, sched, 1)[0] == EUNSUP and _err() == MSG_HBM["vprior"]
    assert _lib.get_option("force_hbm") == 0


def test_refusals_of_the_decode_entry_points():
    H = codes.load_code("steane")[0]
    code = _lib.Code(H)
    m, n = code.m, code.n
    sched = code.schedule(*_schedules(H)[0])
    vp = code.prior(np.linspace(0.01, 0.2, n), 1e-9)
    foreign = _lib.Code(np.roll(H, 1, axis=1)).prior(np.full(n, 0.01), 1e-9)
    syn, mask = np.zeros((2, m), np.uint8), np.zeros((2, n), np.uint8)
    e, it = np.zeros((2, n), np.uint8), np.zeros(2, np.int32)

    def dev_prior(p0=0.01, p1=0.4, mk=mask, mi=5):
        return L.qldpc_decode_device_prior(code.handle, sched.handle, 0, P(syn), 0, 2, p0, p1, P(mk), 0, mi, 0.75,
                                           1e-9, P(e), 0, P(it), None, None, None)

    def host_prior(p0=0.01, p1=0.4, mk=mask, mi=5):
        return L.qldpc_decode_host_prior(code.handle, sched.handle, 0, P(syn), 2, p0, p1, P(mk), mi, 0.75, 1e-9,
                                         P(e), P(it), None, None)

    def dev_vprior(prior=vp.handle, mi=5, batch=2):
        return L.qldpc_decode_device_vprior(code.handle, sched.handle, 0, P(syn), 0, batch, prior, mi, 0.75, P(e), 0,
                                            P(it), None, None, None)

    def host_vprior(prior=vp.handle, mi=5):
        return L.qldpc_decode_host_vprior(code.handle, sched.handle, 0, P(syn), 2, prior, mi, 0.75, P(e), P(it),
                                          None, None)

    def host_plain(mi=5):
        return L.qldpc_decode_host(code.handle, sched.handle, 0, P(syn), 2, 0.01, mi, 0.75, 1e-9, P(e), P(it),
                                   None, None)

    # option force_hbm: neither twin has an HBM-resident variant
    with _lib.options(force_hbm=1):
        for call, kind in ((dev_prior, "prior"), (host_prior, "prior"), (dev_vprior, "vprior"),
                           (host_vprior, "vprior")):
            assert (call(), _err()) == (EUNSUP, MSG_HBM[kind])
    assert _lib.get_option("force_hbm") == 0
    # null mask
    for call in (dev_prior, host_prior):
        assert (call(mk=None), _err()) == (EINVAL, "null mask")
    # p outside [0, 1]
    for bad in (-1e-3, 1.0001, float("nan")):
        for call in (dev_prior, host_prior):
            assert (call(p0=bad), _err()) == (EINVAL, MSG_PROB)
            assert (call(p1=bad), _err()) == (EINVAL, MSG_PROB)
    # a prior handle of another code (also for an empty batch), and none
    for call in (dev_vprior, host_vprior):
        assert (call(prior=foreign.handle), _err()) == (EINVAL, MSG_FOREIGN)
        assert (call(prior=None), _err()) == (EINVAL, "prior handle is null")
    assert (dev_vprior(prior=foreign.handle, batch=0), _err()) == (EINVAL, MSG_FOREIGN)
    # max_iter = 0. The device entries and the per-variable host entry refuse it
    # before any HIP call; the scalar and the two-level host entries reach that
    # check only behind their staging copies, so without a device they report the
    # missing device first
    for call in (dev_prior, dev_vprior, host_vprior):
        assert (call(mi=0), _err()) == (EINVAL, MSG_MAX_ITER)
    late = (EHIP, MSG_NO_DEVICE_HOST) if NO_DEVICE else (EINVAL, MSG_MAX_ITER)
    for call in (host_plain, host_prior):
        assert (call(mi=0), _err()) == late
    # the two-level host entry reports its prior's errors ahead of max_iter
    assert (host_prior(mi=0, mk=None), _err()) == (EINVAL, "null mask")
    assert (host_prior(mi=0, p1=2.0), _err()) == (EINVAL, MSG_PROB)
    assert (dev_prior(mi=0, mk=None), _err()) == (EINVAL, MSG_MAX_ITER)

"""OSD-CS with the prior-weighted cost on the host (qldpc_osd_decode_batch_cs_prior,
osd_cost="prior") against the dense NumPy model of tests/osd_cs_weighted_model.py,
bit for bit, on the shots of tests/osd_cs_cases.py and five prior rows."""
import ctypes

import numpy as np
import pytest

import osd_cs_cases as cases
import osd_cs_prior_cases as pc
import osd_cs_weighted_model as wm

# (matrix, shots): the bundled codes, then the generated 40 x 128 and 40 x 127 matrices
BUNDLED = [("steane:x", 24), ("shor:x", 24), ("LP04_0:x", 64), ("LP04_0:z", 64), ("LP118_2:x", 16)]
GENERATED = [("gen128", 16), ("gen127", 16)]


@pytest.mark.parametrize("row", pc.ROWS)
@pytest.mark.parametrize("name,k", BUNDLED + GENERATED, ids=[c for c, _ in BUNDLED + GENERATED])
def test_host_equals_model(name, k, row):
    H, syn, _, e0, perms = cases.shots(name, k)
    q, eps = pc.prior_row(name, row)
    W = wm.weights(q, eps)
    Hi = H.astype(np.int64)
    base = cases.host_order0(H, syn, perms, e0)
    wide = False
    for lam in cases.LAMBDAS:
        want, _, consistent, c_base, c_best = pc.model(name, k, lam, row)
        got = pc.host_cs_prior(H, syn, perms, e0, lam, q, eps)
        np.testing.assert_array_equal(got, want, err_msg=f"lambda {lam}")
        ok = np.flatnonzero(consistent)
        # consistent syndromes are satisfied; a syndrome outside H's column space gives the order-0 result
        np.testing.assert_array_equal((got[ok].astype(np.int64) @ Hi.T) % 2, syn[ok])
        np.testing.assert_array_equal(got[~consistent], base[~consistent])
        # the prior weight under "prior" is at most that under "hamming": Hamming's winner is a candidate
        ham = cases.host_cs(H, syn, perms, e0, lam)
        cp, ch = wm.cost(got, W), wm.cost(ham, W)
        assert all(a <= b for a, b in zip(cp, ch)), f"lambda {lam}"
        assert cp == c_best
        wide = wide or any(abs(c) > 2 ** 31 for c in c_base + c_best)
        if row == "uniform":                            # a positive multiple of the Hamming weight: same ties
            assert got.tobytes() == ham.tobytes(), f"lambda {lam}"
    if row == "wide" and H.shape[1] > 64:
        # the case a 32-bit accumulator gets wrong
        assert wide


@pytest.mark.parametrize("name,k", BUNDLED, ids=[c for c, _ in BUNDLED])
def test_costs_disagree_and_every_winner_kind_occurs(name, k):
    H, syn, _, e0, perms = cases.shots(name, k)
    kinds = set()
    for row in ("two_level", "random", "negative"):
        differ = 0
        for lam in (10, 64):
            got, kd, consistent, _, _ = pc.model(name, k, lam, row)
            differ += int(np.any(got != cases.model(name, k, lam)[0], axis=1).sum())
            kinds |= set(kd[consistent].tolist())
        assert differ > 0, row
    assert kinds == {wm.BASE, wm.SINGLE, wm.PAIR}
    assert not np.any(pc.model(name, k, 1, "random")[1] == wm.PAIR)      # pairs need lambda >= 2


def test_negative_row_has_negative_weights_and_wide_row_is_wide():
    n = cases.matrix("LP04_0:x").shape[1]
    assert (wm.weights(*pc.prior_row("LP04_0:x", "negative"))[::7] < 0).all()
    W = wm.weights(*pc.prior_row("LP04_0:x", "wide"))
    assert W.max() > 400 * 2 ** 20 and int(W.sum()) > 2 ** 31 and W.shape == (n,)


def test_keyword_paths_equal_the_entry_point():
    from qldpcsim_amd import decoders
    name, k, lam = "LP04_0:x", 64, 10
    H, syn, post, e0, perms = cases.shots(name, k)
    q, eps = pc.prior_row(name, "random")
    want = pc.model(name, k, lam, "random")[0]
    flags = np.zeros(k, np.int32)                       # every shot unconverged
    got = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, lam, method="cs", cost="prior",
                             prior=q, eps=eps)
    np.testing.assert_array_equal(got, want)
    for i in (0, 3, 40):
        one = decoders.OSDdec(H, np.array(e0[i], np.int8), syn[i], post[i], lam, osd_method="cs", osd_cost="prior",
                              prior=q, eps=eps)
        np.testing.assert_array_equal(one, want[i])
    # the wide row goes with eps = 0
    qd, epsd = pc.prior_row(name, "wide")
    got = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, lam, method="cs", cost="prior",
                             prior=qd, eps=epsd)
    np.testing.assert_array_equal(got, pc.model(name, k, lam, "wide")[0])


def test_without_the_keyword_nothing_changes():
    from qldpcsim_amd import decoders
    for name, k in (("LP04_0:x", 64), ("gen128", 16)):
        H, syn, post, e0, perms = cases.shots(name, k)
        q, eps = pc.prior_row(name, "random")
        flags = np.zeros(k, np.int32)
        for method, order in (("ref", 0), ("ref", 1), ("cs", 10)):
            a = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, order, method=method)
            b = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, order, method=method,
                                   cost="hamming")
            c = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, order, method=method,
                                   cost="hamming", prior=q)     # a row the Hamming cost does not read
            assert a.tobytes() == b.tobytes() == c.tobytes()
        i = 3
        assert (decoders.OSDdec(H, np.array(e0[i], np.int8), syn[i], post[i], 10, osd_method="cs").tobytes()
                == decoders.OSDdec(H, np.array(e0[i], np.int8), syn[i], post[i], 10, osd_method="cs",
                                   osd_cost="hamming").tobytes())
        np.testing.assert_array_equal(decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, 10,
                                                         method="cs"), cases.model(name, k, 10)[0])


def test_refusals():
    from qldpcsim_amd import _lib, decoders
    name, k = "LP04_0:x", 64
    H, syn, post, e0, perms = cases.shots(name, k)
    n = H.shape[1]
    q, eps = pc.prior_row(name, "random")
    flags = np.zeros(k, np.int32)
    args = (H, np.array(syn), np.array(e0), np.array(post), flags)
    with pytest.raises(ValueError, match='osd_method="cs"'):
        decoders.apply_osd(*args, 0, method="ref", cost="prior", prior=q)
    with pytest.raises(ValueError, match="prior row"):
        decoders.apply_osd(*args, 10, method="cs", cost="prior")
    with pytest.raises(ValueError):
        decoders.apply_osd(*args, 10, method="cs", cost="llr", prior=q)
    with pytest.raises(ValueError, match=str(n)):
        decoders.apply_osd(*args, 10, method="cs", cost="prior", prior=q[:-1])
    for lam in (-1, 65):
        with pytest.raises(ValueError):
            decoders.apply_osd(*args, lam, method="cs", cost="prior", prior=q)
        with pytest.raises(ValueError):
            decoders.OSDdec(H, np.array(e0[0], np.int8), syn[0], post[0], lam, osd_method="cs", osd_cost="prior",
                            prior=q)
    with pytest.raises(ValueError):
        decoders.OSDdec(H, np.array(e0[0], np.int8), syn[0], post[0], 0, osd_cost="prior", prior=q)
    with pytest.raises(ValueError):
        decoders.OSDdec(H, np.array(e0[0], np.int8), syn[0], post[0], 10, osd_method="cs", osd_cost="prior")
    for kw in (dict(osd_order=0, osd_cost="prior", prior=q), dict(osd_order=10, osd_method="cs", osd_cost="prior"),
               dict(osd_order=10, osd_method="cs", osd_cost="other", prior=q)):
        with pytest.raises(ValueError):
            decoders.decode_batch(H, np.array(syn), None if "prior" in kw else 0.05, 3, **kw)
    with pytest.raises(ValueError):                     # one scalar prior: no row to weigh with
        decoders.MS_decoder(H, syn[1], 0.05, 5, OSDorder=10, osd_method="cs", osd_cost="prior")
    with pytest.raises(ValueError):
        decoders.BP_decoder(H, syn[1], q, 5, OSDorder=0, osd_cost="prior")
    # the C ABI: a null handle, a handle of another code, lambda out of range; e_hat untouched
    code, other = _lib.code_for(H), _lib.code_for(cases.matrix("LP04_0:z"))
    assert other.n == n
    e = np.array(e0)
    call = lambda handle, lam: _lib.lib.qldpc_osd_decode_batch_cs_prior(      # noqa: E731
        code.handle, k, _lib.ptr(np.ascontiguousarray(syn)), _lib.ptr(np.ascontiguousarray(perms)), lam, handle,
        _lib.ptr(e), 1)
    assert call(None, 10) == _lib.QLDPC_EINVAL
    assert call(other.prior(q, eps).handle, 10) == _lib.QLDPC_EINVAL
    assert b"another code" in _lib.lib.qldpc_last_error()
    for lam in (-1, 65):
        assert call(code.prior(q, eps).handle, lam) == _lib.QLDPC_EINVAL
    np.testing.assert_array_equal(e, e0)
    assert call(code.prior(q, eps).handle, 10) == _lib.QLDPC_OK
    np.testing.assert_array_equal(e, pc.model(name, k, 10, "random")[0])


def test_kernel_name_takes_the_third_kind():
    from qldpcsim_amd import _lib
    H = cases.matrix("LP118_2:x")
    names = []
    for cs in (0, 1, 2):
        buf = ctypes.create_string_buffer(128)
        _lib.check(_lib.lib.qldpc_osd_kernel_name(_lib.code_for(H).handle, cs, buf, 128))
        names.append(buf.value.decode())
    assert names == ["osd_block_kernel<17, 8, 2>", "osd_block_cs_kernel<17, 8, 2>",
                     "osd_block_cs_prior_kernel<17, 8, 2>"]


def test_simulators_refuse_before_any_shot():
    from qldpcsim_amd import codes, dem, simulator
    Hx, Hz = codes.load_code("steane")
    n = Hx.shape[1]
    kw = dict(shots=4, verbose=False, sampler="host")
    w = np.ones((3, n))
    w[:, ::2] = 3.0
    for bad in (dict(OSDorder=10, osd_method="cs", osd_cost="prior"),                       # one scalar prior per half
                dict(OSDorder=0, osd_cost="prior", channel_weights=w),                     # not OSD-CS
                dict(OSDorder=10, osd_method="cs", osd_cost="llr", channel_weights=w),
                dict(OSDorder=10, osd_method="cs", osd_cost="prior", channel_weights=np.ones((3, n)))):   # uniform marginals
        with pytest.raises(ValueError):
            simulator.simulate_p(Hx, Hz, 0.05, **kw, **bad)
    with pytest.raises(ValueError, match="scalar prior"):
        simulator.simulate_p(Hx, Hz, 0.05, OSDorder=10, osd_method="cs", osd_cost="prior", **kw)
    with pytest.raises(ValueError):                     # p_data == Q: uniform
        simulator.simulate_phenomenological(Hx, Hz, 0.01, 2.0 * 0.01 / 3.0, 2, OSDorder=2, osd_method="cs",
                                            osd_cost="prior", **kw)
    with pytest.raises(ValueError):
        simulator.simulate_phenomenological(Hx, Hz, 0.01, 0.02, 2, OSDorder=2, osd_cost="prior", **kw)
    model = dem.parse_dem("error(0.1) D0 D1 L0\nerror(0.05) D1 D2\nerror(0.02) D2 D0 L1\n")
    with pytest.raises(ValueError):
        simulator.simulate_dem(model, shots=4, OSDorder=0, osd_cost="prior", verbose=False, sampler="host")


def test_command_line_takes_the_cost():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "qldpcsim_amd.simulator", "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--osd-cost" in r.stdout

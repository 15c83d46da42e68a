"""OSD-CS on the host (qldpc_osd_decode_batch_cs, osd_method="cs") against the
dense NumPy model of tests/osd_cs_model.py, bit for bit."""
import numpy as np
import pytest

import osd_cs_cases as cases
import osd_cs_model

# (matrix, shots): the bundled codes (LP04_0: 64 shots per half; steane: its 8
# syndromes three times over, one per posterior mean), then the generated ones
BUNDLED = [("steane:x", 24), ("steane:z", 24), ("shor:x", 24), ("shor:z", 24), ("LP04_0:x", 64), ("LP04_0:z", 64),
           ("LP118_2:x", 16)]
GENERATED = [("fullrank", 12), ("t3", 24), ("gen128", 16), ("gen127", 16)]


@pytest.mark.parametrize("lam", cases.LAMBDAS)
@pytest.mark.parametrize("name,k", BUNDLED + GENERATED, ids=[c for c, _ in BUNDLED + GENERATED])
def test_host_cs_equals_model(name, k, lam):
    H, syn, _, e0, perms = cases.shots(name, k)
    want, _, consistent = cases.model(name, k, lam)
    got = cases.host_cs(H, syn, perms, e0, lam)
    np.testing.assert_array_equal(got, want)
    base = cases.host_order0(H, syn, perms, e0)
    Hi = H.astype(np.int64)
    # consistent syndromes are satisfied, at no more than the order-0 weight
    ok = np.flatnonzero(consistent)
    np.testing.assert_array_equal((got[ok].astype(np.int64) @ Hi.T) % 2, syn[ok])
    assert np.all(got[ok].sum(axis=1) <= base[ok].sum(axis=1))
    # a syndrome outside H's column space: the order-0 result
    np.testing.assert_array_equal(got[~consistent], base[~consistent])
    # (a full-row-rank H has no inconsistent syndrome; every other case must hold some)
    assert name.startswith("steane") or consistent[: k // 2].all()
    assert (~consistent).any() == (osd_cs_model.gf2_rank(H) < H.shape[0])


@pytest.mark.parametrize("name,k", BUNDLED, ids=[c for c, _ in BUNDLED])
def test_every_winner_kind_occurs(name, k):
    # the tie rule and all three candidate kinds are exercised: over the case's
    # shots the model names the base, a single flip and a pair as winners
    _, kinds, consistent = cases.model(name, k, 10)
    counts = [int(np.sum(kinds[consistent] == kind)) for kind in (osd_cs_model.BASE, osd_cs_model.SINGLE,
                                                                   osd_cs_model.PAIR)]
    assert all(c > 0 for c in counts), counts
    # pairs need lambda >= 2
    assert not np.any(cases.model(name, k, 1)[1] == osd_cs_model.PAIR)


def test_lambda_grows_the_search():
    # more pairs never cost more
    name, k = "LP04_0:x", 64
    w = [cases.model(name, k, lam)[0].sum(axis=1) for lam in cases.LAMBDAS]
    for a, b in zip(w, w[1:]):
        assert np.all(b <= a)
    assert np.any(w[-1] < w[0])


def test_tmax_empty_and_small():
    # |T| = 0: only the base; |T| = 3 < lambda: three singles and three pairs
    H, syn, _, e0, perms = cases.shots("fullrank", 12)
    assert osd_cs_model.gf2_rank(H) == H.shape[1]
    np.testing.assert_array_equal(cases.host_cs(H, syn, perms, e0, 10), cases.host_order0(H, syn, perms, e0))
    H = cases.matrix("t3")
    assert H.shape[1] - osd_cs_model.gf2_rank(H) == 3


def test_zero_first_column_is_order0():
    # an all-zero column perm[0]: J's unconditional first entry is no pivot, the result is order 0's
    H = cases.matrix("gen127").copy()
    H[:, 5] = 0
    rng = np.random.default_rng(5)
    post = rng.normal(0, 3, (6, H.shape[1]))
    post[:, 5] = 0.0                                    # least reliable: perm[0] = 5
    from qldpcsim_amd import decoders
    perms = np.ascontiguousarray(decoders.osd_perms(post), np.int32)
    assert np.all(perms[:, 0] == 5)
    e0 = (post < 0).astype(np.uint8)
    syn = ((rng.random((6, H.shape[1])) < 0.05).astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.uint8)
    np.testing.assert_array_equal(cases.host_cs(H, syn, perms, e0, 10), cases.host_order0(H, syn, perms, e0))


def test_index_error_case_unchanged():
    from qldpcsim_amd import decoders
    H = np.array([[1, 1, 0, 1], [1, 1, 0, 1]], np.int8)
    post = np.array([0.1, 5.0, 6.0, 7.0])
    for method in ("ref", "cs"):
        with pytest.raises(IndexError):
            decoders.OSDdec(H, np.zeros(4, np.int8), np.array([1, 1]), post, 0, osd_method=method)
    with pytest.raises(IndexError):
        osd_cs_model.osd_cs_one(H, [1, 1], decoders.osd_perm(post), np.zeros(4, np.uint8), 0)


@pytest.mark.parametrize("lam", [-1, 65])
def test_lambda_out_of_range_is_refused(lam):
    from qldpcsim_amd import _lib, decoders
    H, syn, post, e0, perms = cases.shots("steane:x", 24)
    e = np.array(e0)
    rc = _lib.lib.qldpc_osd_decode_batch_cs(_lib.code_for(H).handle, len(e), _lib.ptr(np.ascontiguousarray(syn)),
                                            _lib.ptr(np.ascontiguousarray(perms)), lam, _lib.ptr(e), 1)
    assert rc == _lib.QLDPC_EINVAL
    np.testing.assert_array_equal(e, e0)
    flags = np.zeros(len(e), np.int32)
    with pytest.raises(ValueError):
        decoders.apply_osd(H, np.array(syn), e, np.array(post), flags, lam, method="cs")
    with pytest.raises(ValueError):
        decoders.OSDdec(H, e[0].astype(np.int8), syn[0], post[0], lam, osd_method="cs")


def test_method_keyword_checks():
    from qldpcsim_amd import decoders
    H, syn, post, e0, perms = cases.shots("steane:x", 24)
    with pytest.raises(ValueError):
        decoders.osd_method_checked("osd-e", 0)
    for algo in ("RELAY", "NG", "BF"):
        with pytest.raises(ValueError):
            decoders.decode_batch(H, np.array(syn), 0.05, 5, algo=algo, osd_order=10, osd_method="cs")
    with pytest.raises(ValueError):
        decoders.decode_batch(H, np.array(syn), 0.05, 5, osd_order=-1, osd_method="cs")
    with pytest.raises(ValueError):
        decoders.decode_batch(H, np.array(syn), 0.05, 5, osd_order=0, osd_method="other")
    with pytest.raises(ValueError):
        decoders.MS_decoder(H, syn[1], 0.05, 5, OSDorder=-1, osd_method="cs")


def test_ref_is_the_call_without_keyword():
    from qldpcsim_amd import decoders
    for name, k in (("LP04_0:x", 64), ("gen128", 16)):
        H, syn, post, e0, perms = cases.shots(name, k)
        flags = np.zeros(k, np.int32)                   # every shot unconverged
        for order in (0, 1, 2):
            a = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, order)
            b = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, order, method="ref")
            assert a.tobytes() == b.tobytes()
            np.testing.assert_array_equal(a, cases.host_order0(H, syn, perms, e0) if order != 1 else a)
        c = decoders.apply_osd(H, np.array(syn), np.array(e0), np.array(post), flags, 10, method="cs")
        np.testing.assert_array_equal(c, cases.model(name, k, 10)[0])
        i = 3
        one = decoders.OSDdec(H, np.array(e0[i], np.int8), syn[i], post[i], 10, osd_method="cs")
        np.testing.assert_array_equal(one, c[i])
        assert (decoders.OSDdec(H, np.array(e0[i], np.int8), syn[i], post[i], 2).tobytes()
                == decoders.OSDdec(H, np.array(e0[i], np.int8), syn[i], post[i], 2, osd_method="ref").tobytes())


def test_simulators_refuse_before_any_shot():
    # checked with the other arguments, before a shot is drawn or a device is touched
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code("steane")
    kw = dict(shots=4, verbose=False, sampler="host")
    for bad in (dict(OSDorder=-1, osd_method="cs"), dict(OSDorder=65, osd_method="cs"),
                dict(OSDorder=0, osd_method="osd-e"), dict(OSDorder=3, osd_method="cs", decType="BP"),
                dict(OSDorder=3, osd_method="cs", decType="NG"), dict(OSDorder=3, osd_method="cs", decType="RELAY")):
        with pytest.raises(ValueError):
            simulator.simulate_p(Hx, Hz, 0.05, **kw, **bad)
    with pytest.raises(ValueError):
        simulator.simulate_phenomenological(Hx, Hz, 0.01, 0.01, 2, OSDorder=-1, osd_method="cs", **kw)
    with pytest.raises(ValueError):
        simulator.simulate_phenomenological(Hx, Hz, 0.01, 0.01, 2, OSDorder=2, osd_method="cs", decType="BP", **kw)


def test_command_line_takes_the_method():
    import subprocess
    import sys
    r = subprocess.run([sys.executable, "-m", "qldpcsim_amd.simulator", "--help"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and "--osd-method" in r.stdout

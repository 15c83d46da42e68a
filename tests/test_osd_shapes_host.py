"""The OSD shape cases (tests/osd_shape_codes.py) on the host: the generator
against the stored bits, the conditions the inputs must meet (asserted on the
model alone), and the host C++ OSD (reference method, orders 0 and 1, and
OSD-CS) against the dense NumPy models and the reference's goldens, bit for
bit. No GPU."""
import numpy as np
import pytest

import osd_cs_model
import osd_ref_model
import osd_shape_codes as sc


def _rank(H):
    return len(osd_ref_model.reduce_shot(H, np.zeros(H.shape[0], np.uint8), np.arange(H.shape[1]), min(H.shape))[1])


@pytest.mark.parametrize("name", sc.IDS)
def test_generator_equals_stored_bits(name):
    H, g, c = sc.matrix(name), sc.golden(name), sc.CASES[name]
    assert H.shape == (c["m"], c["n"]) and H.dtype == np.uint8
    np.testing.assert_array_equal(H, g["H"])
    assert int((~H.any(axis=0)).sum()) == 0            # (else the launcher picks the column kernel for the whole code)
    assert _rank(H) == c["rank"]
    assert g["meta"]["crafted"] == sc.crafted(name)


@pytest.mark.parametrize("name", sc.IDS)
def test_shots_equal_stored_shots(name):
    # the committed shot builder gives the inputs the reference was run on
    _, syn, _, e0, perms = sc.shots(name)
    g, idx = sc.golden(name), sc.golden_shots(name)
    k = sc.CASES[name]["k"]
    assert k == (8 if name in ("c33max", "h_m", "h_n") else 32) and len(syn) == k
    np.testing.assert_array_equal(g["shots"], idx)
    np.testing.assert_array_equal(g["syn"], syn[idx])
    np.testing.assert_array_equal(g["e0"], e0[idx])
    np.testing.assert_array_equal(g["perms"], perms[idx])
    np.testing.assert_array_equal(np.sort(perms, axis=1), np.broadcast_to(np.arange(perms.shape[1]), perms.shape))
    for j, i in enumerate(idx):
        want = sc.order_posteriors(perms[i], e0[i])
        assert want.tobytes() == g["post"][j].tobytes()
        # the reference's own order of these posteriors (decoders.py:320-325) is the permutation, without ties
        prob = 1.0 / (1.0 + np.exp(want))
        rel = np.where(prob > 0.5, prob, 1 - prob)
        np.testing.assert_array_equal(np.argsort(rel, kind="stable"), perms[i])
        assert np.all(np.diff(rel[perms[i]]) > 0)
        np.testing.assert_array_equal(want < 0, e0[i] != 0)
    assert not g["raised0"].any() and not g["raised1"].any()


@pytest.mark.parametrize("name", sc.IDS)
def test_host_osd_equals_model_and_goldens(name):
    J, e0h, e1h, consistent = sc.ref_model(name)
    g, idx = sc.golden(name), sc.golden_shots(name)
    for order, want in ((0, e0h), (1, e1h)):
        got = sc.host(name, order)
        np.testing.assert_array_equal(got, want, err_msg=f"order {order}")
        np.testing.assert_array_equal(got[idx], g[f"ehat{order}"], err_msg=f"order {order}: reference golden")
        np.testing.assert_array_equal(want[idx], g[f"ehat{order}"], err_msg=f"order {order}: model against golden")
    H, syn = sc.shots(name)[:2]
    ok = np.flatnonzero(consistent)
    np.testing.assert_array_equal((e0h[ok].astype(np.int64) @ H.T.astype(np.int64)) % 2, syn[ok])
    assert all(len(j) == sc.CASES[name]["rank"] for j in J)


@pytest.mark.parametrize("name", sc.IDS)
def test_inconsistent_syndromes_occur(name):
    # every rank-deficient case: at least a quarter of the shots inconsistent and a quarter consistent
    c = sc.CASES[name]
    consistent = sc.ref_model(name)[3]
    k = c["k"]
    assert consistent[: k // 2].all()                   # the first half comes from errors
    if c["rank"] < c["m"]:
        assert 4 * int(consistent.sum()) >= k and 4 * int((~consistent).sum()) >= k, consistent
    else:
        assert consistent.all()
    # the golden shots: half from errors, half arbitrary
    assert list(sc.golden_shots(name) < k // 2).count(True) * 2 == len(sc.golden_shots(name))


CRAFTED = ["b4w1", "b9w3", "b9r2", "c33min", "c33max", "h_n"]


def test_crafted_cases_are_the_ones_with_64_pairs():
    assert [n for n in sc.IDS if sc.crafted(n)] == CRAFTED


@pytest.mark.parametrize("name", CRAFTED)
def test_crafted_shots_have_an_empty_and_a_full_word(name):
    H, syn, _, _, perms = sc.shots(name)
    J, _, _, consistent = sc.ref_model(name)
    k, n = sc.CASES[name]["k"], H.shape[1]
    a, b = sc.equal_column_pairs(H)
    pair = dict(zip(a.tolist(), b.tolist()))
    assert consistent[0] and not consistent[k - 1]      # one consistent and one arbitrary syndrome
    for i in (0, k - 1):
        assert i in sc.golden_shots(name)
        assert [pair[int(c)] for c in perms[i, :64]] == perms[i, 64:128].tolist()
        w = osd_ref_model.pivots_per_word(J[i], n)
        last = int(np.flatnonzero(w)[-1])
        assert last > 1 and w[1] == 0, w                # word 1: no pivot before the rank is reached
        if name != "b4w1":                              # (rank 60: its fullest word cannot hold 64)
            assert w.max() == 64, w


@pytest.mark.parametrize("lam", sc.LAMBDAS)
@pytest.mark.parametrize("name", sc.BLOCK_IDS)
def test_host_cs_equals_model(name, lam):
    want, _, consistent = sc.cs_model(name, lam)
    got = sc.host_cs(name, lam)
    np.testing.assert_array_equal(got, want)
    base = sc.host(name, 0)
    np.testing.assert_array_equal(got[~consistent], base[~consistent])
    assert np.all(got[consistent].sum(axis=1) <= base[consistent].sum(axis=1))
    np.testing.assert_array_equal(consistent, sc.ref_model(name)[3])
    if lam == 0:                                        # no pairs: singles alone
        assert not np.any(sc.cs_model(name, 0)[1] == osd_cs_model.PAIR)


@pytest.mark.parametrize("name", sc.BLOCK_IDS)
def test_every_winner_kind_occurs_at_lambda_64(name):
    _, kinds, consistent = sc.cs_model(name, 64)
    counts = [int(np.sum(kinds[consistent] == kind)) for kind in (osd_cs_model.BASE, osd_cs_model.SINGLE,
                                                                   osd_cs_model.PAIR)]
    assert all(c > 0 for c in counts), counts


def test_model_orders_agree_with_the_cs_model_and_the_oracle():
    # the two models share no code: order 0 is OSD-CS's base candidate (lambda 0 picks
    # it or a single flip), and order 1 is the oracle's restatement of OSDdec
    from oracle import oracle
    name = "b4w1"
    H, syn, _, e0, perms = sc.shots(name)
    _, e0h, e1h, _ = sc.ref_model(name)
    cs, kinds, _ = sc.cs_model(name, 0)
    base = kinds == osd_cs_model.BASE
    assert base.any()
    np.testing.assert_array_equal(cs[base], e0h[base])
    for i in sc.golden_shots(name):
        post = sc.order_posteriors(perms[i], e0[i])
        for order, want in ((0, e0h), (1, e1h)):
            got = oracle.osd_dec(H.astype(np.int64), e0[i].astype(np.int64), syn[i].astype(np.int64), post, order)
            np.testing.assert_array_equal(got, want[i])

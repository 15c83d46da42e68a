"""The identity behind the float32-domain check node of the register-resident
flooding min-sum kernel (ms_flood_qc.h), restated in
NumPy on degree-8 checks and compared as 32-bit patterns.

Float64 form (cn_ms_compute): min1 / min2 the smallest and second smallest
|v_e| (with multiplicity), c1 = fl32(beta * min1), c2 = fl32(beta * min2), edge
e takes (|v_e| == min1 ? c2 : c1).

Float32-domain form: w_e = bits(fl32(beta * |v_e|)) as unsigned integers, w1 /
w2 their smallest and second smallest by the kernel's network
(min12_tree_u32<8>: groups 3 + 3 + 2, one three-way merge), edge e takes
(w_e == w1 ? w2 : w1), or without a compare med3(w_e, w1, w2) ^ (w1 ^ w2).

Rounding and multiplying by beta > 0 are monotone, so both give the same bits;
the reference's substitutions for zero and infinite float64 minima are outside
the identity, and every check they apply to is one the kernel's trigger (w1 ==
0 or w2 not finite) sends to the float64 code."""
import numpy as np
import pytest

BETAS = (0.75, 0.8, 0.625, 0.9)
DEG = 8
ROWS = 20000
INF32 = np.uint32(0x7F800000)


def _f64_form(v, beta):
    a = np.abs(v)
    s = np.sort(a, axis=1)
    min1, min2 = s[:, 0], s[:, 1]
    with np.errstate(over="ignore", under="ignore"):
        c1 = (beta * min1).astype(np.float32).view(np.uint32)
        c2 = (beta * min2).astype(np.float32).view(np.uint32)
    return np.where(a == min1[:, None], c2[:, None], c1[:, None]), min1, min2


def _med3(x, y, z):
    return np.maximum(np.minimum(x, y), np.minimum(np.maximum(x, y), z))


def _min3(x, y, z):
    return np.minimum(np.minimum(x, y), z)


def _tree_u32(w):
    """min12_tree_u32<8>: (min3, med3) of w[0:3] and of w[3:6], (min, max) of
    w[6:8], then lo = min3(l), hi = min(med3(l), min3(h))."""
    l1, h1 = _min3(w[:, 0], w[:, 1], w[:, 2]), _med3(w[:, 0], w[:, 1], w[:, 2])
    l2, h2 = _min3(w[:, 3], w[:, 4], w[:, 5]), _med3(w[:, 3], w[:, 4], w[:, 5])
    l3, h3 = np.minimum(w[:, 6], w[:, 7]), np.maximum(w[:, 6], w[:, 7])
    return _min3(l1, l2, l3), np.minimum(_med3(l1, l2, l3), _min3(h1, h2, h3))


def _f32_forms(v, beta):
    with np.errstate(over="ignore", under="ignore"):
        w = (beta * np.abs(v)).astype(np.float32).view(np.uint32)
    w1, w2 = _tree_u32(w)
    s = np.sort(w, axis=1)
    assert np.array_equal(w1, s[:, 0]) and np.array_equal(w2, s[:, 1]), "network: not the two smallest"
    cmp_form = np.where(w == w1[:, None], w2[:, None], w1[:, None])
    med_form = _med3(w, w1[:, None], w2[:, None]) ^ (w1 ^ w2)[:, None]
    return cmp_form, med_form, w1, w2


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _random(rng):
    """magnitudes log-uniform over 1e-3 .. 1e2"""
    return _signs(rng, (ROWS, DEG)) * 10.0 ** rng.uniform(-3, 2, (ROWS, DEG))


def _exact_ties(rng):
    """two to eight edges share one magnitude, often the smallest"""
    v = _random(rng)
    k = rng.integers(2, DEG + 1, ROWS)
    shared = np.abs(v[:, 0]) * np.where(rng.random(ROWS) < 0.7, 1e-3, 1.0)
    for j in range(DEG):
        v[:, j] = np.where(j < k, np.sign(v[:, j]) * shared, v[:, j])
    return rng.permuted(v, axis=1)


def _near_ties(rng, beta):
    """magnitudes a few float64 ulps apart: equal after rounding to float32,
    different before, placed at the minimum and away from it"""
    v = _random(rng)
    base = np.abs(v[:, 0]) * np.where(rng.random(ROWS) < 0.7, 1e-3, 1.0)
    k = rng.integers(2, 5, ROWS)
    for j in range(1, 4):
        near = base * (1.0 + rng.integers(1, 1 << 20, ROWS) * 2.0 ** -52)
        v[:, j] = np.where(j < k, np.sign(v[:, j]) * near, v[:, j])
    v[:, 0] = np.sign(v[:, 0]) * base
    a = np.abs(v[:, :2])
    with np.errstate(over="ignore", under="ignore"):
        w = (beta * a).astype(np.float32)
    assert ((a[:, 0] != a[:, 1]) & (w[:, 0] == w[:, 1])).mean() > 0.9
    return rng.permuted(v, axis=1)


def _zeros(rng):
    v = _random(rng)
    v[rng.random((ROWS, DEG)) < 0.2] = 0.0
    v[rng.random((ROWS, DEG)) < 0.05] = -0.0
    return v


def _underflow(rng):
    """beta * |v| around the smallest float32 subnormal (2^-149) and normal (2^-126)"""
    return _signs(rng, (ROWS, DEG)) * 2.0 ** rng.uniform(-153, -120, (ROWS, DEG))


def _overflow(rng):
    """beta * |v| around the largest float32 (2^128 rounds to inf), some infinite"""
    v = _signs(rng, (ROWS, DEG)) * 2.0 ** (rng.uniform(126, 129.5, (ROWS, 1)) + rng.uniform(-0.5, 0.5, (ROWS, DEG)))
    v[rng.random((ROWS, DEG)) < 0.1] = np.inf
    return v


FAMILIES = {
    "random": lambda rng, beta: _random(rng),
    "exact_ties": lambda rng, beta: _exact_ties(rng),
    "near_ties": _near_ties,
    "zeros": lambda rng, beta: _zeros(rng),
    "underflow": lambda rng, beta: _underflow(rng),
    "overflow": lambda rng, beta: _overflow(rng),
}


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_float32_domain_select_has_the_float64_bits(family, beta):
    rng = np.random.default_rng([sorted(FAMILIES).index(family), int(beta * 1000)])
    scale = 10.0 ** rng.integers(-3, 3) if family in ("random", "exact_ties", "near_ties", "zeros") else 1.0
    v = FAMILIES[family](rng, beta) * scale
    want, min1, min2 = _f64_form(v, beta)
    cmp_form, med_form, w1, w2 = _f32_forms(v, beta)
    assert np.array_equal(cmp_form, want), f"{family} beta={beta}: compare form"
    assert np.array_equal(med_form, want), f"{family} beta={beta}: median form"
    # the checks the reference's :165-166 rules and FLAG_MIN_ZERO apply to are
    # among those the kernel sends to its float64 code
    f64_rare = (min1 == 0.0) | np.isinf(min2)
    trigger = (w1 == 0) | (w2 >= INF32)
    assert not (f64_rare & ~trigger).any()
    if family in ("zeros", "underflow", "overflow"):
        assert trigger.mean() > 0.05, "the family does not reach the trigger"
    if family in ("underflow", "overflow"):
        assert (trigger & ~f64_rare).any(), "no float32-only underflow / overflow"


def test_near_ties_put_a_float32_tie_on_a_float64_non_argmin():
    """The case the argument needs: an edge with w_e == w1 that is not the
    float64 argmin; then w2 == w1 and either choice has the same bits."""
    rng = np.random.default_rng(5)
    v = _near_ties(rng, 0.8)
    a = np.abs(v)
    _, _, w1, w2 = _f32_forms(v, 0.8)
    with np.errstate(over="ignore", under="ignore"):
        w = (0.8 * a).astype(np.float32).view(np.uint32)
    fake = (w == w1[:, None]) & (a != a.min(axis=1)[:, None])
    assert fake.any(axis=1).mean() > 0.5
    assert (w1 == w2)[fake.any(axis=1)].all()

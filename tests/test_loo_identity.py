"""The identity behind the leave-one-out check node of the register-resident
flooding min-sum kernel (ms_flood_qc.h's qc_loo_f64 and decoder_common.h's
loo_min_tree), restated in NumPy for checks of degree 2 to 9
and compared as 32-bit patterns.

Select form (cn_ms_compute, decoders.py:160-169): min1 / min2 the smallest and
second smallest |v_e| (with multiplicity), c1 = fl32(beta * min1), c2 =
fl32(beta * min2), edge e takes (|v_e| == min1 ? c2 : c1) with the sign
npm ^ sign(v_e).

Leave-one-out form: loo_e = min over e' != e of |v_e'| by the kernel's tree (a
recursion over halves, each subtree's minimum formed once, a subtree handed the
minimum of everything outside it), edge e takes fl32(bs * loo_e) ^ sign(v_e),
bs = beta with npm in its sign bit.

loo_e is min2 where |v_e| == min1 and min1 elsewhere, and rounding is symmetric,
so both give the same bits wherever the reference's substitutions for a zero
min1 and an infinite min2 do not apply; every check they apply to is one the
kernel's class test on the tree's two top minima (zero or infinite) sends to the
select form."""
import numpy as np
import pytest

BETAS = (0.75, 0.8, 0.625, 1.0)
DEGREES = tuple(range(2, 10))
ROWS = 6000
SIGN = np.uint32(0x80000000)


def _select_form(v, npm, beta):
    a = np.abs(v)
    s = np.sort(a, axis=1)
    min1, min2 = s[:, 0], s[:, 1]
    with np.errstate(over="ignore", under="ignore"):
        c1 = (beta * min1).astype(np.float32).view(np.uint32)
        c2 = (beta * min2).astype(np.float32).view(np.uint32)
    c = np.where(a == min1[:, None], c2[:, None], c1[:, None])
    return c ^ npm[:, None] ^ np.where(np.signbit(v), SIGN, np.uint32(0)), min1, min2


class _Tree:
    """loo_min_tree<N>: the split of min12_tree (3 -> 2 + 1, 5 -> 2 + 3, 6 -> 4 + 2,
    7 -> 4 + 3, 8 -> 4 + 4), every np.minimum one v_min_f64."""

    def __init__(self, a):
        self.a, self.ops = a, 0

    def _min(self, x, y):
        self.ops += 1
        return np.minimum(x, y)

    @staticmethod
    def split(n):
        h = (n // 2 + 1) & ~1
        return h if h < n else n - 1

    def up(self, lo, n, sub):
        """minimum of columns lo .. lo + n, n >= 2; sub[(lo, n)] for every inner node"""
        k = self.split(n)
        left = self.a[:, lo] if k == 1 else self.up(lo, k, sub)
        right = self.a[:, lo + k] if n - k == 1 else self.up(lo + k, n - k, sub)
        sub[(lo, n)] = self._min(left, right)
        return sub[(lo, n)]

    def down(self, lo, n, sub, out, loo):
        if n == 1:
            loo[:, lo] = out
            return
        k = self.split(n)
        left = self.a[:, lo] if k == 1 else sub[(lo, k)]
        right = self.a[:, lo + k] if n - k == 1 else sub[(lo + k, n - k)]
        self.down(lo, k, sub, self._min(right, out), loo)
        self.down(lo + k, n - k, sub, self._min(left, out), loo)

    def run(self):
        n = self.a.shape[1]
        k, sub, loo = self.split(n), {}, np.empty_like(self.a)
        top0 = self.a[:, 0] if k == 1 else self.up(0, k, sub)
        top1 = self.a[:, k] if n - k == 1 else self.up(k, n - k, sub)
        self.down(0, k, sub, top1, loo)
        self.down(k, n - k, sub, top0, loo)
        return loo, top0, top1


def _loo_form(v, npm, beta):
    tree = _Tree(np.abs(v))
    loo, top0, top1 = tree.run()
    bs = np.where(npm != 0, -beta, beta)[:, None]
    with np.errstate(over="ignore", under="ignore"):
        c = (bs * loo).astype(np.float32).view(np.uint32)
    return c ^ np.where(np.signbit(v), SIGN, np.uint32(0)), loo, top0, top1, tree.ops


def _signs(rng, shape):
    return np.where(rng.random(shape) < 0.5, -1.0, 1.0)


def _random(rng, n):
    """magnitudes log-uniform over 1e-3 .. 1e2"""
    return _signs(rng, (ROWS, n)) * 10.0 ** rng.uniform(-3, 2, (ROWS, n))


def _all_tied(rng, n):
    """iteration 1 of every decode: one magnitude on every edge"""
    return _signs(rng, (ROWS, n)) * 10.0 ** rng.uniform(-3, 2, (ROWS, 1))


def _two_tied(rng, n):
    """exactly two edges share the smallest magnitude (all of them for n = 2)"""
    v = _random(rng, n)
    lo = np.abs(v).min(axis=1) * 0.5
    v[:, 0], v[:, 1] = np.sign(v[:, 0]) * lo, np.sign(v[:, 1]) * lo
    return rng.permuted(v, axis=1)


def _near_ties(rng, n, beta):
    """two or three magnitudes a few float64 ulps apart, equal after rounding to
    float32, at the minimum and away from it"""
    v = _random(rng, n)
    base = np.abs(v[:, 0]) * np.where(rng.random(ROWS) < 0.7, 1e-3, 1.0)
    for j in range(1, min(n, 3)):
        v[:, j] = np.sign(v[:, j]) * base * (1.0 + rng.integers(1, 1 << 20, ROWS) * 2.0 ** -52)
    v[:, 0] = np.sign(v[:, 0]) * base
    a = np.abs(v[:, :2])
    with np.errstate(over="ignore", under="ignore"):
        w = (beta * a).astype(np.float32)
    assert ((a[:, 0] != a[:, 1]) & (w[:, 0] == w[:, 1])).mean() > 0.9
    return rng.permuted(v, axis=1)


def _zeros(rng, n):
    v = _random(rng, n)
    v[rng.random((ROWS, n)) < 0.2] = 0.0
    v[rng.random((ROWS, n)) < 0.05] = -0.0
    return v


def _few_finite(rng, n):
    """one finite value (min2 infinite) or two (min2 finite, whole subtrees
    infinite) among infinities of either sign"""
    v = _signs(rng, (ROWS, n)) * np.inf
    keep = np.zeros((ROWS, n), bool)
    keep[:, 0] = True
    keep[:, 1] = rng.random(ROWS) < 0.5
    keep = rng.permuted(keep, axis=1)
    return np.where(keep, _random(rng, n), v)


def _underflow(rng, n):
    """beta * |v| around the smallest float32 subnormal (2^-149) and normal (2^-126)"""
    return _signs(rng, (ROWS, n)) * 2.0 ** rng.uniform(-153, -120, (ROWS, n))


def _overflow(rng, n):
    """beta * |v| around the largest float32 (2^128 rounds to inf), some infinite"""
    v = _signs(rng, (ROWS, n)) * 2.0 ** (rng.uniform(126, 129.5, (ROWS, 1)) + rng.uniform(-0.5, 0.5, (ROWS, n)))
    v[rng.random((ROWS, n)) < 0.1] = np.inf
    return v


FAMILIES = {
    "random": lambda rng, n, beta: _random(rng, n),
    "all_tied": lambda rng, n, beta: _all_tied(rng, n),
    "two_tied": lambda rng, n, beta: _two_tied(rng, n),
    "near_ties": _near_ties,
    "zeros": lambda rng, n, beta: _zeros(rng, n),
    "few_finite": lambda rng, n, beta: _few_finite(rng, n),
    "underflow": lambda rng, n, beta: _underflow(rng, n),
    "overflow": lambda rng, n, beta: _overflow(rng, n),
}


def _zero_or_inf(x):
    return (x == 0.0) | np.isinf(x)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_leave_one_out_form_has_the_select_bits(family, beta):
    for n in DEGREES:
        rng = np.random.default_rng([sorted(FAMILIES).index(family), int(beta * 1000), n])
        scale = 10.0 ** rng.integers(-3, 3) if family in ("random", "all_tied", "two_tied", "near_ties", "zeros") \
            else 1.0
        v = FAMILIES[family](rng, n, beta) * scale
        npm = np.where(rng.random(ROWS) < 0.5, SIGN, np.uint32(0))
        label = f"{family} beta={beta} n={n}"
        want, min1, min2 = _select_form(v, npm, beta)
        got, loo, top0, top1, _ = _loo_form(v, npm, beta)
        # the tree: every loo_e is the minimum of the others
        a = np.abs(v)
        for e in range(n):
            assert np.array_equal(loo[:, e], np.delete(a, e, axis=1).min(axis=1)), f"{label}: loo of edge {e}"
        assert np.array_equal(np.minimum(top0, top1), min1), f"{label}: top minima"
        # the checks the reference's :165-166 rules and FLAG_MIN_ZERO apply to
        # are among those the class test sends to the select form; min1 == 0 exactly
        rare = (min1 == 0.0) | np.isinf(min2)
        trigger = _zero_or_inf(top0) | _zero_or_inf(top1)
        assert not (rare & ~trigger).any(), f"{label}: a rare check passes the class test"
        assert np.array_equal((top0 == 0.0) | (top1 == 0.0), min1 == 0.0), f"{label}: zero test"
        # the identity, wherever the substitutions do not apply (the kernel uses
        # it on the checks that pass the class test, a subset)
        assert np.array_equal(got[~rare], want[~rare]), f"{label}: bits differ"
        if family in ("zeros", "few_finite"):
            assert rare.mean() > 0.2, f"{label}: the family does not reach the rare rules"
        if family == "few_finite" and n >= 4:
            assert (trigger & ~rare).any(), f"{label}: no infinite subtree beside a finite min2"
        if family in ("random", "all_tied", "two_tied", "near_ties"):
            assert not trigger.any(), f"{label}: the hot path is not what is compared"
        if family == "underflow":
            assert (got[~rare] << 1 == 0).any() and (got[~rare] << 1 != 0).any(), f"{label}: no underflow to zero"
        if family == "overflow":
            inf32 = (got[~rare] & ~SIGN) == np.uint32(0x7F800000)
            assert inf32.any() and (~inf32).any(), f"{label}: no overflow to infinity"


def test_tie_families_are_what_they_say():
    rng = np.random.default_rng(11)
    for n in DEGREES:
        a = np.abs(_all_tied(rng, n))
        assert (a == a[:, :1]).all()
        a = np.abs(_two_tied(rng, n))
        assert ((a == a.min(axis=1)[:, None]).sum(axis=1) == 2).all()
    # an edge equal to min1 in float32 only is not tied: its loo is min1
    v = _near_ties(rng, 8, 0.8)
    a = np.abs(v)
    loo = _Tree(a).run()[0]
    arg = a == a.min(axis=1)[:, None]
    assert (arg.sum(axis=1) == 1).all()
    assert np.array_equal(loo[~arg], np.broadcast_to(a.min(axis=1)[:, None], a.shape)[~arg])


@pytest.mark.parametrize("n", DEGREES)
def test_tree_instruction_count(n):
    """3 N - 6 minima: one per inner node below the root going up (N - 2), one
    per node below the root's halves going down (2 N - 4); 18 at N = 8, where
    min12_tree takes 20 and two multiplies and conversions more."""
    assert _loo_form(np.ones((1, n)), np.zeros(1, np.uint32), 0.75)[4] == 3 * n - 6

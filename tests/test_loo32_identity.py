"""The identity behind the 32-bit leave-one-out check node of the
register-resident flooding min-sum kernel (ms_flood_qc.h's qc_loo_u32 and
decoder_common.h's loo_min_tree_u32), restated in NumPy for
checks of degree 2 to 9 and compared as 32-bit patterns.

Float64 form (qc_loo_f64's hot path): loo_e = min over e' != e of |v_e'|, edge e
takes fl32(bs * loo_e) ^ sign(v_e), bs = beta with the check's sign npm.

32-bit form: w_e = bits(fl32(bs * |v_e|)) first, then loo_w[e] = the unsigned
minimum over e' != e of w_e' by the kernel's network (groups of three, min3),
edge e takes loo_w[e] ^ sign(v_e). x -> fl32(bs * x) is monotone in magnitude on
x >= 0 and every word of a lane carries npm's sign bit, so the unsigned order of
the words is the order of the magnitudes and loo_w[e] == bits(fl32(bs * loo_e)).

The kernel's rare test is a float32 class test (+-0, +-inf) on three words of
the network (top0, top1, out0: mA, mB and oA at degree 8); a lane it fires on
takes the select form (decoders.py:160-169) instead. It must fire wherever the
reference's substitutions apply (min1 == 0 or min2 infinite), and it also fires
where a finite non-zero product underflows to zero or overflows float32 there;
it must not fire on ordinary inputs, or the hot path is not the hot path."""
import os
import re

import numpy as np
import pytest

from test_loo_identity import FAMILIES, ROWS, SIGN, _loo_form, _select_form

BETAS = (0.75, 0.8, 1.0, 0.3)
DEGREES = tuple(range(2, 10))
HOT = ("random", "all_tied", "two_tied", "near_ties")       # families no lane of which may fire the rare test
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "qldpcsim_amd", "csrc", "decoder_common.h")


class _Net:
    """loo_min_tree_u32<N>: up to four values directly; more as N // 3 groups of
    three and N % 3 single values, the groups' minima and the single values the
    items of the same problem one level up. Every minimum of two or three is one
    instruction (v_min_u32 / v_min3_u32)."""

    def __init__(self):
        self.ops = 0

    def _min(self, *x):
        assert 2 <= len(x) <= 3
        self.ops += 1
        out = x[0]
        for y in x[1:]:
            out = np.minimum(out, y)
        return out

    def run(self, w):
        """w: list of N columns -> (loo columns, top0, top1, out0)"""
        n = len(w)
        assert n >= 2
        if n <= 4:
            loo = [w[1], w[0]] if n == 2 else [self._min(*(w[j] for j in range(n) if j != e)) for e in range(n)]
            return loo, w[0], w[1], loo[0]
        g, r = n // 3, n % 3
        t = [self._min(w[3 * k], w[3 * k + 1], w[3 * k + 2]) for k in range(g)] + [w[3 * g + k] for k in range(r)]
        o = self.run(t)[0]
        loo = []
        for k in range(g):
            a, b, c = w[3 * k:3 * k + 3]
            loo += [self._min(b, c, o[k]), self._min(a, c, o[k]), self._min(a, b, o[k])]
        loo += o[g:]
        return loo, t[0], t[1], o[0]


def _u32_form(v, npm, beta):
    """(message bits, loo words, rare-test lanes, instructions)"""
    bs = np.where(npm != 0, -beta, beta)[:, None]
    with np.errstate(over="ignore", under="ignore"):
        w = (bs * np.abs(v)).astype(np.float32).view(np.uint32)
    net = _Net()
    loo, top0, top1, out0 = net.run([w[:, e] for e in range(w.shape[1])])
    loo = np.stack(loo, axis=1)
    fire = _class_zero_or_inf(top0) | _class_zero_or_inf(top1) | _class_zero_or_inf(out0)
    return loo ^ np.where(np.signbit(v), SIGN, np.uint32(0)), loo, w, fire, net.ops


def _class_zero_or_inf(x):
    """v_cmp_class_f32 with the mask 0x264 on a word: +-0, +-inf"""
    mag = x & ~SIGN
    return (mag == 0) | (mag == np.uint32(0x7F800000))


def _case(family, beta, n):
    rng = np.random.default_rng([sorted(FAMILIES).index(family), int(beta * 1000), n, 32])
    scale = 10.0 ** rng.integers(-3, 3) if family in HOT + ("zeros",) else 1.0
    v = FAMILIES[family](rng, n, beta) * scale
    npm = np.where(rng.random(ROWS) < 0.5, SIGN, np.uint32(0))
    return v, npm


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_u32_form_has_the_float64_forms_bits(family, beta):
    for n in DEGREES:
        v, npm = _case(family, beta, n)
        assert (npm != 0).any() and (npm == 0).any()
        label = f"{family} beta={beta} n={n}"
        want, min1, min2 = _select_form(v, npm, beta)
        hot64 = _loo_form(v, npm, beta)[0]
        got, loo_w, w, fire, _ = _u32_form(v, npm, beta)
        # the network: every loo_w[e] is the unsigned minimum of the other words
        for e in range(n):
            assert np.array_equal(loo_w[:, e], np.delete(w, e, axis=1).min(axis=1)), f"{label}: loo of edge {e}"
        # the rare test fires wherever the reference's :165-166 rules apply
        rare = (min1 == 0.0) | np.isinf(min2)
        assert not (rare & ~fire).any(), f"{label}: a rare check passes the class test"
        # the identity on every lane, fired or not, against qc_loo_f64's hot path,
        # and against the select form wherever its substitutions do not apply
        assert np.array_equal(got, hot64), f"{label}: bits differ from the float64 leave-one-out form"
        assert np.array_equal(got[~rare], want[~rare]), f"{label}: bits differ from the select form"
        if family in HOT:
            assert not fire.any(), f"{label}: the rare test fires on {int(fire.sum())} ordinary lanes"
        if family in ("zeros", "few_finite"):
            assert rare.mean() > 0.2, f"{label}: the family does not reach the rare rules"
        if family == "underflow":
            # a product that rounds to float32 zero fires the test although min1 != 0
            assert (fire & ~rare).any() and (~fire).any(), f"{label}: no underflow on either side of the test"
            assert ((got[~fire] & ~SIGN) < np.uint32(0x00800000)).any(), f"{label}: no float32 denormal on the hot path"
        if family == "overflow":
            assert (fire & ~rare).any() and (~fire).any(), f"{label}: no overflow on either side of the test"


def test_near_ties_are_equal_in_float32_only():
    """the family behind 'equal in float32 only': distinct |v_e| whose words are
    equal, so the word minimum ties where the float64 minimum does not"""
    rng = np.random.default_rng(5)
    v = FAMILIES["near_ties"](rng, 8, 0.8)
    a = np.abs(v)
    w = (0.8 * a).astype(np.float32).view(np.uint32)
    assert ((a == a.min(axis=1)[:, None]).sum(axis=1) == 1).all()
    assert ((w == w.min(axis=1)[:, None]).sum(axis=1) >= 2).mean() > 0.5


def _header_ops():
    """decoder_common.h's constexpr loo_min_tree_u32_ops as a Python function"""
    txt = open(HEADER).read()
    expr = re.search(r"constexpr int loo_min_tree_u32_ops\(int n\) \{[^\n]*\n\s*return ([^;]+);", txt).group(1)

    def tern(s):
        if "?" not in s:
            return s
        cond, rest = s.split("?", 1)
        a, b = rest.split(":", 1)
        return f"(({a}) if ({cond}) else {tern(b)})"

    code = tern(expr.replace("/", "//"))

    def ops(n):
        return eval(code, {"loo_min_tree_u32_ops": ops, "n": n})   # noqa: S307  (the project's own header)
    return ops


@pytest.mark.parametrize("n", DEGREES)
def test_network_instruction_count(n):
    """the NumPy network's count equals the header's constexpr; 12 at N = 8
    (the float64 tree: 18)"""
    ops = _u32_form(np.ones((1, n)), np.zeros(1, np.uint32), 0.75)[4]
    assert ops == _header_ops()(n)
    if n == 8:
        assert ops == 12

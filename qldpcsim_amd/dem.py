"""Detector error models: the object, the reader of Stim's .dem text and the
NumPy twins of the device kernels (dem_kernels.hip). Pure NumPy, no Stim.

A detector error model (DEM) is a list of N independent error mechanisms.
Mechanism J fires with probability priors[J]; when it fires it flips the
detectors of column J of H [M, N] and the logical observables of column J of
L [K, N]. A shot is the fired row f; the decoder sees det = H f and answers
with an estimate ehat; the shot is

    class 2  decoder failure: H ehat != det
    class 1  logical error:   not 2, and L ehat != L f
    class 0  success:         not 2, and L ehat == L f

so scoring needs the detectors and the K observable bits alone, never f.

The text grammar is Stim's (https://github.com/quantumlib/Stim, the
detector error model file format): `error(p) D3 D7 ^ D9 L0`,
`detector(coords) D5`, `logical_observable L2`, `shift_detectors(coords) k`,
`repeat n { ... }`, `#` comments and an optional `[tag]` after the
instruction's name. `^` separates the parts of a suggested decomposition and
means nothing here: the mechanism flips the XOR of all its targets.
"""
import re

import numpy as np

from . import spacetime

__all__ = ["Dem", "parse_dem", "load_dem", "dem_text", "phenomenological_dem", "sample_dem", "count_dem"]


class Dem:
    """H uint8 [M, N] (detector x mechanism), L uint8 [K, N] (observable x
    mechanism; K may be 0), priors float64 [N], each in [0, 1)."""

    def __init__(self, H, L, priors):
        H, L = np.asarray(H), np.asarray(L)
        pr = np.asarray(priors, dtype=np.float64)
        if H.ndim != 2 or pr.ndim != 1 or pr.shape[0] != H.shape[1]:
            raise ValueError("H must be [M, N] and priors [N]")
        if L.ndim == 1 and L.size == 0:
            L = np.zeros((0, H.shape[1]), np.uint8)             # K = 0 spelt as an empty list
        if L.ndim != 2 or L.shape[1] != H.shape[1]:
            raise ValueError(f"L must be [K, {H.shape[1]}]")
        for name, A in (("H", H), ("L", L)):
            if A.dtype == object or not np.isin(A, (0, 1)).all():
                raise ValueError(f"{name} must hold only 0 and 1")
        if not np.all((pr >= 0.0) & (pr < 1.0)):                # NaN fails both comparisons
            raise ValueError("every prior must lie in [0, 1)")
        self.H = np.ascontiguousarray(H, dtype=np.uint8)
        self.L = np.ascontiguousarray(L, dtype=np.uint8)
        self.priors = np.ascontiguousarray(pr)

    @property
    def num_detectors(self):
        return self.H.shape[0]

    @property
    def num_observables(self):
        return self.L.shape[0]

    @property
    def num_errors(self):
        return self.H.shape[1]

    def thresholds(self):
        """uint64 [N]: column J fires iff its 32-bit draw u < thr_J, thr =
        min(2^32, floor(p 2^32)) — what qldpc_channel_table(p, 0, 0) yields."""
        return np.minimum(2.0 ** 32, np.floor(self.priors * 2.0 ** 32)).astype(np.uint64)

    def uniform_prior(self):
        """The one probability every column has, else None."""
        pr = self.priors
        return float(pr[0]) if pr.size and np.all(pr == pr[0]) else None

    def __eq__(self, other):
        return isinstance(other, Dem) and self.H.shape == other.H.shape and self.L.shape == other.L.shape and \
            np.array_equal(self.H, other.H) and np.array_equal(self.L, other.L) and \
            np.array_equal(self.priors, other.priors)

    __hash__ = None

    def __repr__(self):
        return f"Dem(detectors={self.num_detectors}, observables={self.num_observables}, errors={self.num_errors})"


# name, optional [tag], optional (arguments), targets
_INSTR = re.compile(r"^([A-Za-z_][A-Za-z_0-9]*)\s*(\[[^\]]*\])?\s*(?:\(([^)]*)\))?\s*(.*)$")
_TARGET = re.compile(r"^([DL])(\d+)$")


def _fail(ln, msg):
    raise ValueError(f"line {ln}: {msg}")


def _blocks(text):
    """The text as nested blocks: a list of (line number, name, arguments or
    None, target words) and, for a repeat, (line number, "repeat", count,
    block)."""
    root = []
    stack = [(root, 0)]
    for ln, raw in enumerate(text.splitlines(), 1):
        line = raw.split("#", 1)[0].strip()
        if not line:
            continue
        if line == "}":
            if len(stack) == 1:
                _fail(ln, "'}' without a repeat block")
            stack.pop()
            continue
        m = _INSTR.match(line)
        if not m:
            _fail(ln, f"cannot read {line!r}")
        name, args, rest = m.group(1).lower(), m.group(3), m.group(4).split()
        if name == "repeat":
            if args is not None or len(rest) != 2 or rest[1] != "{" or not rest[0].isdigit():
                _fail(ln, "expected 'repeat N {'")
            body = []
            stack[-1][0].append((ln, "repeat", int(rest[0]), body))
            stack.append((body, ln))
            continue
        if "{" in rest or "}" in rest:
            _fail(ln, "a brace belongs to a repeat block, on a line of its own")
        stack[-1][0].append((ln, name, args, rest))
    if len(stack) > 1:
        _fail(stack[-1][1], "repeat block is never closed")
    return root


def _targets(ln, words, kinds, shift):
    """(detector indices, observable indices) of target words, detectors
    shifted; `kinds`: the letters this instruction takes."""
    det, obs = [], []
    for w in words:
        if w == "^" and "^" in kinds:
            continue
        m = _TARGET.match(w)
        if not m or m.group(1) not in kinds:
            _fail(ln, f"malformed target {w!r}")
        (det if m.group(1) == "D" else obs).append(int(m.group(2)) + (shift if m.group(1) == "D" else 0))
    return det, obs


def _odd(idx):
    """The indices named an odd number of times, ascending."""
    u, c = np.unique(np.asarray(idx, dtype=np.int64), return_counts=True)
    return tuple(int(x) for x in u[c % 2 == 1])


def parse_dem(text, merge=True):
    """Stim detector error model text -> Dem. M = 1 + the largest absolute
    detector index seen (in an error or a declaration), K likewise for the
    observables. A target named an even number of times in one instruction
    cancels. merge: mechanisms with identical (detector set, observable set)
    combine into one column at the first one's position, p <- p1 (1 - p2) +
    p2 (1 - p1); columns that differ only in their observables stay separate,
    and so do columns without a detector (an undetectable logical error is
    still sampled). ValueError names the line."""
    cols, where = [], {}                        # [p, detectors, observables]; (detectors, observables) -> column
    top = {"D": -1, "L": -1}
    state = {"shift": 0}

    def run(block):
        for ln, name, args, rest in block:
            if name == "repeat":
                for _ in range(args):
                    run(rest)
            elif name == "error":
                try:
                    p = float(args)
                except (TypeError, ValueError):
                    _fail(ln, "error needs one probability: error(p) targets")
                if not (0.0 <= p < 1.0):
                    _fail(ln, f"probability {args.strip()} outside [0, 1)")
                det, obs = _targets(ln, rest, "DL^", state["shift"])
                top["D"], top["L"] = max([top["D"]] + det), max([top["L"]] + obs)
                key = (_odd(det), _odd(obs))
                if merge and key in where:
                    c = cols[where[key]]
                    c[0] = c[0] * (1.0 - p) + p * (1.0 - c[0])
                else:
                    where.setdefault(key, len(cols))
                    cols.append([p, key[0], key[1]])
            elif name == "detector":
                top["D"] = max([top["D"]] + _targets(ln, rest, "D", state["shift"])[0])
            elif name == "logical_observable":
                if args is not None:
                    _fail(ln, "logical_observable takes no arguments")
                top["L"] = max([top["L"]] + _targets(ln, rest, "L", 0)[1])
            elif name == "shift_detectors":
                if len(rest) > 1 or (rest and not rest[0].isdigit()):
                    _fail(ln, "expected 'shift_detectors(coords) k'")
                state["shift"] += int(rest[0]) if rest else 0
            else:
                _fail(ln, f"unknown instruction {name!r}")

    run(_blocks(text))
    M, K, N = top["D"] + 1, top["L"] + 1, len(cols)
    H, L = np.zeros((M, N), np.uint8), np.zeros((K, N), np.uint8)
    for j, (_, det, obs) in enumerate(cols):
        H[list(det), j] = 1
        L[list(obs), j] = 1
    return Dem(H, L, np.array([c[0] for c in cols], np.float64))


def load_dem(path, merge=True):
    """A Dem from a file: .npz with keys H, L, priors, else .dem text."""
    path = str(path)
    if path.endswith(".npz"):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("H", "L", "priors") if k not in z.files]
            if missing:
                raise ValueError(f"{path}: no key {missing[0]!r} (a model holds H, L and priors)")
            return Dem(z["H"], z["L"], z["priors"])
    with open(path, "rt") as f:
        return parse_dem(f.read(), merge=merge)


def dem_text(dem):
    """The model as .dem text: one `error` line per column with a %.17g
    probability, and a declaration where the last detector or observable is
    in no column. parse_dem(dem_text(d), merge=False) == d."""
    lines = []
    for j in range(dem.num_errors):
        t = [f"D{i}" for i in np.flatnonzero(dem.H[:, j])] + [f"L{i}" for i in np.flatnonzero(dem.L[:, j])]
        lines.append(" ".join(["error(%.17g)" % dem.priors[j]] + t))
    M, K = dem.num_detectors, dem.num_observables
    if M and not dem.H[M - 1].any():
        lines.append(f"detector D{M - 1}")
    if K and not dem.L[K - 1].any():
        lines.append(f"logical_observable L{K - 1}")
    return "\n".join(lines) + "\n"


def phenomenological_dem(H, L, rounds, p_data, q):
    """The phenomenological model of one CSS half (spacetime.py) as a Dem:
    spacetime_matrix(H, T), L on every round's data columns and zero on the
    measurement columns, spacetime_prior. The column order is
    spacetime_matrix's, so L_st ehat = L fold_data(ehat)."""
    H = (np.asarray(H) % 2).astype(np.uint8)
    m, n = H.shape
    L = (np.asarray(L) % 2).astype(np.uint8).reshape(-1, n)
    S = spacetime.spacetime_matrix(H, rounds).astype(np.uint8)
    T = int(rounds)
    Lst = np.zeros((L.shape[0], S.shape[1]), np.uint8)
    for t in range(T):
        Lst[:, t * (n + m):t * (n + m) + n] = L
    return Dem(S, Lst, spacetime.spacetime_prior(n, m, T, p_data, q))


def sample_dem(dem, shots, rng, want_fired=False):
    """NumPy twin of qldpc_dem_sample: one 32-bit integer per column drawn from
    `rng` against the device sampler's thresholds. Returns (det uint8
    [shots, M], obs uint8 [shots, K]); with want_fired also the fired rows
    uint8 [shots, N]."""
    thr = dem.thresholds()
    u = rng.integers(0, 1 << 32, (int(shots), thr.size), dtype=np.uint64)
    fired = (u < thr).astype(np.uint8)
    det, obs = spacetime._mod2(fired, dem.H), spacetime._mod2(fired, dem.L)
    return (det, obs, fired) if want_fired else (det, obs)


def count_dem(dem, det, obs, ehat, iters, want_shots=False):
    """NumPy twin of qldpc_dem_count. det uint8 [B, M], obs uint8 [B, K], ehat
    uint8 [B, N], iters [B]. Returns {"failures", "logical_errors",
    "successes", "iterations"}; with want_shots also (class uint8 [B], flip
    words uint64 [B, ceil(K/64)] = L ehat ^ obs, as computed for every
    class)."""
    ehat = np.asarray(ehat).astype(np.uint8) & 1
    fail = np.any(spacetime._mod2(ehat, dem.H) != (np.asarray(det) & 1), axis=1)
    F = spacetime._mod2(ehat, dem.L) ^ (np.asarray(obs).astype(np.uint8) & 1)
    cls = np.where(fail, 2, np.any(F != 0, axis=1).astype(np.uint8)).astype(np.uint8)
    out = {"failures": int((cls == 2).sum()), "logical_errors": int((cls == 1).sum()),
           "successes": int((cls == 0).sum()), "iterations": int(np.asarray(iters, dtype=np.int64).sum())}
    if want_shots:
        return out, (cls, spacetime._pack_words(F))
    return out

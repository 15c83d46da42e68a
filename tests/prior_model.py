"""NumPy model of min-sum and BP decoding with a prior per shot and variable —
TEST INFRASTRUCTURE ONLY. It restates SURVEY.md App. A.1 (MS) and A.2 (BP)
and DESIGN.md §3.10 with `L` replaced by `L[b, j]`, shares no code with the
library or the oracle, and is what tests/test_gpu_prior.py compares
decode_prior_kernel with. With every prior equal it is the scalar contract,
which tests/test_prior_model.py pins to the reference's goldens.

Contract restated:
  MS  c2v float32 (0 at the start), S float32 summed in ascending check order,
      post = fl64(L_j + (f64)S_j). A check node reads v_e = post_j - (f64)c2v_e,
      except in the first layer of the first iteration, which reads
      (f64)(f32)L_j. sign(0) = +1; min1 / first argmin / min2 (inf -> 0);
      every edge with |v_e| == min1 gets min2, the others min1;
      c2v_e = +-fl32(beta * m_e), sign = syndrome * prod(sign) * sign_e.
      Sparse semantics: the reference's dense "leak" of a zero min1 is not
      emulated, it raises FLAG_MIN_ZERO.
  BP  float64; post_j = L_j at the start and for a variable without checks,
      else L_j + S_j (sequential sum, column degree < 8); t_e = tanh(v_e / 2),
      P = left fold of the product, th = P / t_e, |th| >= 1 - eps moves by eps
      towards 0, c2v_e = 2 atanh(th), negated where the syndrome bit is set.
  Stop test H e == s (mod 2) after every layer's variable pass; iterations
  as the reference returns them.
  Flags as the kernels raise them: CONVERGED = the last stop test held;
  MIN_ZERO = some check node pass met min1 == 0. A flooding decode runs the
  check nodes of iteration k + 1 before it learns that iteration k converged
  (the parity test rides on that pass), so that pass's MIN_ZERO counts too —
  unless k is max_iter, whose last test is a parity test alone.
"""
import numpy as np

FLAG_CONVERGED, FLAG_MIN_ZERO = 1, 2


def llr(p, eps=1e-9):
    return np.log((1 - p) / max(p, eps))               # np.float64 (decoders.py:147)


def two_level(mask, p0, p1, eps=1e-9):
    """L[B, n] of a 0/1 mask: llr(p0) where 0, llr(p1) where 1."""
    return np.where(np.asarray(mask) != 0, llr(p1, eps), llr(p0, eps)).astype(np.float64)


class Graph:
    def __init__(self, H):
        H = (np.asarray(H) % 2).astype(np.int64)
        self.H = H
        self.m, self.n = H.shape
        r, c = np.nonzero(H)                            # row-major: ascending variable within a check
        self.er, self.ec = r, c
        self.E = len(r)
        dr = H.sum(1)
        dc = H.sum(0)
        self.R = -np.ones((self.m, max(1, dr.max(initial=0))), np.int64)   # edge ids per check
        fill = np.zeros(self.m, np.int64)
        for e in range(self.E):
            self.R[r[e], fill[r[e]]] = e
            fill[r[e]] += 1
        self.C = -np.ones((self.n, max(1, dc.max(initial=0))), np.int64)   # per variable, ascending check
        fill = np.zeros(self.n, np.int64)
        for e in range(self.E):                         # e ascends with the check
            self.C[c[e], fill[c[e]]] = e
            fill[c[e]] += 1
        self.dc = dc


def _cn_ms(V, valid, syn, beta):
    """V [b, r, d] float64, valid [r, d], syn [b, r] -> (c2v float32 [b, r, d], min1 == 0 [b, r])."""
    A = np.where(valid, np.abs(V), np.inf)
    k = np.argmin(A, axis=2)                            # first argmin
    min1 = np.take_along_axis(A, k[..., None], 2)[..., 0]
    A2 = A.copy()
    np.put_along_axis(A2, k[..., None], np.inf, 2)
    min2 = A2.min(axis=2)
    m1 = np.where(np.isinf(min1), 0.0, min1)
    m2 = np.where(np.isinf(min2), 0.0, min2)
    neg = (V < 0) & valid                               # sign(0) = +1
    flip = ((neg.sum(2) & 1) ^ syn).astype(bool)        # syndrome * prod of the signs < 0
    mag = np.where(np.abs(V) == min1[..., None], m2[..., None], m1[..., None])
    c = (beta * mag).astype(np.float32)                 # float64 product, rounded once
    c = np.where(neg ^ flip[..., None], -c, c)
    has = valid.any(1)
    return c.astype(np.float32), (m1 == 0.0) & has


def _cn_bp(V, valid, syn, eps):
    with np.errstate(all="ignore"):
        T = np.tanh(V / 2.0)
        P = np.ones(V.shape[:2])
        for k in range(V.shape[2]):                     # np.prod: sequential fold
            P = np.where(valid[:, k], P * T[:, :, k], P)
        th = P[..., None] / T
        big = np.abs(th) >= 1.0 - eps
        th = np.where(big, th - eps * np.sign(th), th)
        val = 2.0 * np.arctanh(th)
    return np.where(syn[..., None].astype(bool), -val, val)


def decode(algo, H, syn, L, max_iter, layers=None, beta=0.75, eps=1e-9):
    """-> (ehat uint8 [B, n], iters int32 [B], post float64 [B, n], flags int32 [B]).
    L: float64 [B, n] priors (LLRs); layers: list of row lists, None = flooding."""
    g = H if isinstance(H, Graph) else Graph(H)
    syn = np.asarray(syn).astype(np.int64)
    L = np.ascontiguousarray(L, np.float64)
    B = syn.shape[0]
    ms = algo == "MS"
    if not ms:
        assert g.dc.max(initial=0) < 8, "the BP model sums columns sequentially (np.sum below 8 terms)"
    flooding = layers is None
    lay = [np.arange(g.m)] if flooding else [np.asarray(r, np.int64) for r in layers]
    post = L.copy()
    c2v = np.zeros((B, g.E + 1), np.float32 if ms else np.float64)    # [E]: the pad entry of absent edges
    iters = np.full(B, max_iter, np.int32)
    flags = np.zeros(B, np.int32)
    act = np.ones(B, bool)
    L32 = L.astype(np.float32).astype(np.float64)
    Cv = g.C >= 0

    def check_pass(idx, rows, first):
        Re = g.R[rows]
        valid = Re >= 0
        cols = g.ec[np.where(valid, Re, 0)]
        src = L32 if (ms and first) else post
        V = src[idx][:, cols]
        if not (ms and first):
            V = V - c2v[idx][:, np.where(valid, Re, g.E)].astype(np.float64)
        if ms:
            c, z = _cn_ms(V, valid, syn[idx][:, rows], beta)
            flags[idx[z.any(1)]] |= FLAG_MIN_ZERO
        else:
            c = _cn_bp(V, valid, syn[idx][:, rows], eps)
        sub = c2v[idx]
        sub[:, Re[valid]] = c[:, valid]
        c2v[idx] = sub

    def var_pass(idx, rows):
        # the variables of the layer's checks (the others' sums are unchanged:
        # recomputing every column, as the reference does, gives the same bits)
        Re = g.R[rows]
        js = np.unique(g.ec[Re[Re >= 0]])
        if idx.size == 0 or js.size == 0:
            return
        sub = c2v[idx]
        Cj, Cvj = g.C[js], Cv[js]
        S = np.zeros((len(idx), len(js)), sub.dtype)
        for t in range(g.C.shape[1]):                   # ascending check order, sequential
            S = S + np.where(Cvj[:, t], sub[:, np.where(Cvj[:, t], Cj[:, t], g.E)], 0).astype(sub.dtype)
        Lj = L[np.ix_(idx, js)]
        post[np.ix_(idx, js)] = Lj + S.astype(np.float64) if ms else Lj + S

    Rv = g.R >= 0
    Rcols = g.ec[np.where(Rv, g.R, 0)]                  # [m, d] variable of each check's edges

    def satisfied(idx):
        # H e == s (mod 2) edge by edge (a dense product per layer is what a
        # schedule of many layers on a matrix of thousands of rows spends its time in)
        e = post[idx] < 0
        par = (e[:, Rcols] & Rv).sum(2) & 1
        return np.all(par == syn[idx], axis=1)

    first = True
    for it in range(max_iter):
        for rows in lay:
            idx = np.flatnonzero(act)
            if idx.size == 0:
                break
            check_pass(idx, rows, first)
            first = False
            if flooding and it > 0:                     # the pass's parity result: iteration `it` converged
                ok = satisfied(idx)
                iters[idx[ok]] = it
                flags[idx[ok]] |= FLAG_CONVERGED
                act[idx[ok]] = False
                idx = idx[~ok]
            var_pass(idx, rows)
            if not flooding or it + 1 == max_iter:
                ok = satisfied(idx)
                iters[idx[ok]] = it + 1
                flags[idx[ok]] |= FLAG_CONVERGED
                act[idx[ok]] = False
    return (post < 0).astype(np.uint8), iters, post, flags

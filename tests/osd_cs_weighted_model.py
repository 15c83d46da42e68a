"""Dense NumPy model of OSD-CS with the prior-weighted cost,
written from its definition and sharing nothing with the C++ or the kernels.

Everything of tests/osd_cs_model.py's definition stays (perm, J, T, the base
estimate e0, the candidates and their order, lambda, the cases that fall back
to order 0) except the cost: with a prior row q and eps,
  L_j = np.log((1 - q_j) / max(q_j, eps)),  W_j = round-half-even(L_j 2^20),
and the cost of an estimate e is sum_j e_j W_j, an integer (W_j < 0 where
q_j > 1/2). The first candidate of strictly smallest cost wins, the base wins
ties. Costs are Python ints; the column sums are formed in int64, which is
exact because sum |W_j| < 2^62 is asserted.
"""
import numpy as np

from osd_cs_model import BASE, PAIR, SINGLE, gf2_rank, reduce_shot  # noqa: F401  (re-exported)


def weights(q, eps=1e-9):
    """W int64 [n] of a prior row (every |W_j| < 2^30)."""
    q = np.asarray(q, np.float64)
    L = np.log((1 - q) / np.maximum(q, eps))
    W = np.rint(L * 2.0 ** 20).astype(np.int64)        # (the scaling is exact)
    assert sum(abs(int(w)) for w in W) < 2 ** 62
    return W


def cost(e, W):
    """Prior weight of the rows of e (uint8 [k, n] or [n]) as Python ints."""
    e = np.atleast_2d(np.asarray(e))
    return [sum(int(w) for w in np.asarray(W)[np.flatnonzero(row)]) for row in e]


def osd_cs_one(H, syn, perm, e_in, lam, W, rank=None, reduced=None):
    """-> (e_hat uint8 [n], winner kind, consistent, base cost, winning cost)."""
    H = np.asarray(H, dtype=np.uint8) & 1
    m, n = H.shape
    perm = np.asarray(perm)
    rank = gf2_rank(H) if rank is None else rank
    if rank <= 1:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (n, n))
    Wp = np.asarray(W, np.int64)[perm]                  # weight of each perm position
    ep = (np.asarray(e_in, dtype=np.uint8) & 1)[perm]
    A, J = reduce_shot(H, syn, perm, rank) if reduced is None else reduced
    nJ = len(J)
    inJ = np.zeros(n, bool)
    inJ[J] = True
    T = np.flatnonzero(~inJ)
    consistent = not A[nJ:, n].any()
    M = A[:nJ][:, T].astype(np.int64)                   # B^-1 H_T
    e_T = ep[T].astype(np.int64)
    e0_J = (A[:nJ, n].astype(np.int64) + M @ e_T) % 2
    WJ, WT = Wp[J], Wp[T]
    base = int((e0_J * WJ).sum()) + int((e_T * WT).sum())
    best_cost, best, kind = base, (), BASE
    if consistent:
        L = min(int(lam), len(T))
        sw = WJ * (1 - 2 * e0_J)                        # cost change of flipping e0_J[r]
        fl = WT * (1 - 2 * e_T)                         # and of flipping T[k]
        cands = [(k,) for k in range(len(T))]
        costs = [base + int(fl[k]) + int(sw[M[:, k] != 0].sum()) for k in range(len(T))]
        for a in range(L):
            for b in range(a + 1, L):
                x = M[:, a] ^ M[:, b]
                cands.append((a, b))
                costs.append(base + int(fl[a]) + int(fl[b]) + int(sw[x != 0].sum()))
        for F, c in zip(cands, costs):                  # the first of strictly smallest cost
            if c < best_cost:
                best_cost, best, kind = c, F, len(F)
    eJ, eT = e0_J.copy(), e_T.copy()
    for k in best:
        eJ = (eJ + M[:, k]) % 2
        eT[k] ^= 1
    ep = ep.copy()
    ep[J] = eJ
    ep[T] = eT
    out = np.zeros(n, np.uint8)
    out[perm] = ep
    return out, kind, consistent, base, best_cost


def osd_cs_batch(H, syn, perms, e_in, lam, W, reduced=None):
    """Row-wise osd_cs_one -> (e_hat [k, n], kinds [k], consistent [k], base costs, winning costs: lists of int).
    `reduced`: one reduce_shot result per shot, where a caller runs several lambdas or rows on the same shots."""
    rank = gf2_rank(H)
    out = [osd_cs_one(H, syn[i], perms[i], e_in[i], lam, W, rank, None if reduced is None else reduced[i])
           for i in range(len(e_in))]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], bool),
            [o[3] for o in out], [o[4] for o in out])

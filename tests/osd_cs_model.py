"""Dense NumPy model of OSD-CS (combination sweep), written from its definition
 and sharing nothing with the C++ or the kernels.

For one shot, with `perm` the reliability order:
  * Hp = H[:, perm]; J = the greedy information-complement set of
    decoders.py:329-342 (position 0, then every position whose column raises
    the rank, until rank(H)); T = the other positions, ascending.
  * Base estimate e0 = the order-0 OSD result: e0_T is the incoming hard
    decision on T, e0_J = B^-1 (s + H_T e0_T), B = Hp[:, J].
  * Candidates in order: e0; for k in 0 .. |T|-1 the flip of T[k]; for
    a < b < min(lam, |T|), lexicographic, the flips of T[a] and T[b]. A flip
    set F gives e_J = e0_J + sum over F of the column B^-1 H_T[:, k].
  * Cost = Hamming weight of all n bits; the first candidate of strictly
    smallest cost wins.
  * A syndrome outside H's column space: the order-0 result, computed as the
    reference does: e_J[k] = (T sJ)[k] with T the row operations of
    REF(Hp[:, J], reduced=True) (gf2math.py:139-187, pivot = first row at or
    below the current one).
  * rank(H) <= 1 with a nonzero first column: the reference's IndexError.
The model does not cover an all-zero column perm[0] (the tests give it none).
"""
import numpy as np

BASE, SINGLE, PAIR = 0, 1, 2


def gf2_rank(A):
    A = np.array(A, dtype=np.uint8) & 1
    r = 0
    for j in range(A.shape[1]):
        rows = np.flatnonzero(A[r:, j]) + r
        if rows.size == 0:
            continue
        A[[r, rows[0]]] = A[[rows[0], r]]
        rows = np.flatnonzero(A[:, j])
        A[rows[rows != r]] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def reduce_shot(H, syn, perm, rank):
    """-> (A, J): the full reduction of [Hp | s] with REF's pivot rule, stopping
    at rank(H), and the pivot positions. It does not depend on lambda."""
    H = np.asarray(H, dtype=np.uint8) & 1
    m, n = H.shape
    Hp = H[:, np.asarray(perm)]
    assert Hp[:, 0].any(), "the model does not cover an all-zero first column"
    A = np.concatenate([Hp, (np.asarray(syn, dtype=np.uint8) & 1).reshape(m, 1)], axis=1)
    J, r = [], 0
    for j in range(n):
        if r == rank:
            break
        rows = np.flatnonzero(A[r:, j]) + r
        if rows.size == 0:
            continue
        A[[r, rows[0]]] = A[[rows[0], r]]
        rows = np.flatnonzero(A[:, j])
        A[rows[rows != r]] ^= A[r]                      # (one vectorised update per pivot)
        J.append(j)
        r += 1
    return A, J


def osd_cs_one(H, syn, perm, e_in, lam, rank=None, reduced=None):
    """-> (e_hat uint8 [n], winner kind, consistent). Raises IndexError where
    the reference's OSDdec does. `reduced`: this shot's reduce_shot result,
    where a caller runs several lambdas on the same shot."""
    H = np.asarray(H, dtype=np.uint8) & 1
    m, n = H.shape
    perm = np.asarray(perm)
    rank = gf2_rank(H) if rank is None else rank
    assert H[:, perm[0]].any(), "the model does not cover an all-zero first column"
    if rank <= 1:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (n, n))
    ep = (np.asarray(e_in, dtype=np.uint8) & 1)[perm]
    A, J = reduce_shot(H, syn, perm, rank) if reduced is None else reduced
    nJ = len(J)
    inJ = np.zeros(n, bool)
    inJ[J] = True
    T = np.flatnonzero(~inJ)
    consistent = not A[nJ:, n].any()
    M = A[:nJ][:, T].astype(np.int64)                   # B^-1 H_T (rows of T sJ where inconsistent)
    e_T = ep[T].astype(np.int64)
    e0_J = (A[:nJ, n].astype(np.int64) + M @ e_T) % 2
    best_cost, best, kind = int(e0_J.sum() + e_T.sum()), (), BASE
    if consistent:
        L = min(int(lam), len(T))
        # every candidate's full weight, a block of candidates at a time: the
        # weight of its e_J plus the weight of its e_T (np.argmin: first minimum)
        wT = int(e_T.sum())
        flipT = 1 - 2 * e_T                             # weight change of flipping T[k]
        blocks = [([(k,) for k in range(len(T))], ((e0_J[:, None] + M) % 2).sum(axis=0) + wT + flipT)]
        for a in range(L - 1):
            eJ = (e0_J[:, None] + M[:, a:a + 1] + M[:, a + 1:L]) % 2
            blocks.append(([(a, b) for b in range(a + 1, L)], eJ.sum(axis=0) + wT + flipT[a] + flipT[a + 1:L]))
        for F, cost in blocks:
            if len(F) and int(cost.min()) < best_cost:
                i = int(np.argmin(cost))
                best_cost, best, kind = int(cost[i]), F[i], len(F[i])
    eJ, eT = e0_J.copy(), e_T.copy()
    for k in best:
        eJ = (eJ + M[:, k]) % 2
        eT[k] ^= 1
    ep = ep.copy()
    ep[J] = eJ
    ep[T] = eT
    out = np.zeros(n, np.uint8)
    out[perm] = ep
    return out, kind, consistent


def osd_cs_batch(H, syn, perms, e_in, lam):
    """Row-wise osd_cs_one -> (e_hat [k, n], kinds [k], consistent [k])."""
    rank = gf2_rank(H)
    out = [osd_cs_one(H, syn[i], perms[i], e_in[i], lam, rank) for i in range(len(e_in))]
    return (np.stack([o[0] for o in out]), np.array([o[1] for o in out]),
            np.array([o[2] for o in out], bool))

"""Dense NumPy model of the reference-method OSD, orders 0 and 1, beside the
OSD-CS model of tests/osd_cs_model.py (same definitions) and
sharing nothing with the C++ or the kernels.

For one shot, with `perm` the reliability order and Hp = H[:, perm]:
  * J = position 0, then every position whose column raises the rank, until
    rank(H) (decoders.py:329-342); T = the other positions.
  * The row operations are those of REF(Hp[:, J], reduced=True)
    (gf2math.py:139-187, pivot = first row at or below the current one),
    applied to [Hp | s] whole: columns outside J never hold a pivot, so the
    operations are the same. With A the reduced matrix, e_J = A[:|J|, n] +
    A[:|J|, T] e_T, for consistent and inconsistent syndromes alike.
  * Order 0: e_T is the incoming estimate on T.
  * Order 1: the reference's loop aliases its candidate arrays, so its result
    is the second candidate whatever the weights: e_T with the bit at
    infoSet[0] flipped, infoSet = list(set(range(n)) - set(J)) taken literally
    with CPython's set (decoders.py:344-368).
The model does not cover an all-zero column perm[0] (the tests give it none).
"""
import numpy as np


def reduce_shot(H, syn, perm, rank):
    """-> (A, J): [Hp | s] after REF's row operations through the first `rank`
    pivot columns, and those columns' positions. Row updates are one
    vectorised XOR per pivot, on rows packed eight columns to the byte (at
    1024 x 2111 a shot takes about 0.2 s instead of a second)."""
    H = np.asarray(H, dtype=np.uint8) & 1
    m, n = H.shape
    A = np.concatenate([H[:, np.asarray(perm)], (np.asarray(syn, dtype=np.uint8) & 1).reshape(m, 1)], axis=1)
    assert A[:, 0].any(), "the model does not cover an all-zero first column"
    P = np.packbits(A, axis=1)                          # column j: bit 7 - j % 8 of byte j // 8
    J, r = [], 0
    for j in range(n):
        if r == rank:
            break
        col = (P[:, j >> 3] >> (7 - (j & 7))) & 1
        below = np.flatnonzero(col[r:])
        if below.size == 0:
            continue
        p = r + int(below[0])
        if p != r:
            P[[r, p]] = P[[p, r]]
            col[[r, p]] = col[[p, r]]
        rows = np.flatnonzero(col)
        rows = rows[rows != r]
        P[rows] ^= P[r]
        J.append(j)
        r += 1
    return np.unpackbits(P, axis=1)[:, :n + 1], J


def osd_ref_one(H, syn, perm, e_in, rank):
    """-> (J, e_hat order 0, e_hat order 1, consistent), e_hat uint8 [n]."""
    n = np.asarray(H).shape[1]
    perm = np.asarray(perm)
    if rank <= 1:
        raise IndexError("index %d is out of bounds for axis 1 with size %d" % (n, n))
    A, J = reduce_shot(H, syn, perm, rank)
    nJ = len(J)
    consistent = not A[nJ:, n].any()
    info = list(set(range(n)) - set(J))                 # the reference's infoSet, CPython's order
    T = np.array(sorted(info), np.int64)
    M = A[:nJ][:, T].astype(np.int64)
    ep = (np.asarray(e_in, dtype=np.uint8) & 1)[perm]
    out = []
    for order in (0, 1):
        if order == 1 and info:
            ep = ep.copy()
            ep[info[0]] ^= 1
        cand = ep.copy()
        cand[J] = (A[:nJ, n].astype(np.int64) + M @ ep[T].astype(np.int64)) % 2
        e = np.zeros(n, np.uint8)
        e[perm] = cand
        out.append(e)
    return J, out[0], out[1], consistent


def osd_ref_batch(H, syn, perms, e_in, rank):
    """Row-wise osd_ref_one -> (list of J, e_hat0 [k, n], e_hat1 [k, n], consistent [k])."""
    out = [osd_ref_one(H, syn[i], perms[i], e_in[i], rank) for i in range(len(e_in))]
    return ([o[0] for o in out], np.stack([o[1] for o in out]), np.stack([o[2] for o in out]),
            np.array([o[3] for o in out], bool))


def pivots_per_word(J, n):
    """Number of pivot positions in each 64-column word of the permuted order."""
    return np.bincount(np.asarray(J, np.int64) // 64, minlength=(n + 63) // 64)

"""NumPy models of BP decoding with one prior per variable on columns of any
degree — TEST INFRASTRUCTURE ONLY. tests/prior_model.py sums BP columns in
sequence (np.sum below 8 terms); here every column is summed in np.sum's own
order at its length (DOUBLE_pairwise_sum: sequential below 8 terms, eight
accumulators up to 128, halved and recursed above), flooding and layered.

  bp_flood_numpy   the shot-by-shot loop tests/test_gpu_vprior_hbm.py has used
                   at 129 entries: every column through np.sum itself.
  decode_bp        the same decode vectorised over shots (seconds, not
                   minutes): the column sum is pairwise_sum below, which adds
                   whole vectors of shots in np.sum's order, so each shot's
                   sum has np.sum's bits (tests/test_wide_column_codes.py
                   compares it with np.sum of each contiguous 1-D column; an
                   axis reduction of NumPy's does not associate like a 1-D sum
                   unless the reduced axis is the contiguous one). A layered
                   schedule runs layer by layer, the messages of rows not yet
                   visited at zero, with the stop test after every layer, as
                   the reference does.
  colsum="strided8"  the control: eight accumulators over the whole column at
                   any length, what hbm_tile_kernel did past 128 entries. Used
                   only to show that a batch tells the two orders apart.
"""
import functools

import numpy as np

import prior_model as pm
import shape_codes as sc
import wide_column_codes as wc

FLAG_CONVERGED = pm.FLAG_CONVERGED


def bp_flood_numpy(H, syn, L, max_iter, eps=1e-9):
    """The reference's flooding BP with L_j per variable, shot by shot, every
    column summed with np.sum on a contiguous float64 vector (NumPy's pairwise
    summation at any length). -> (ehat, iters, post)."""
    m, n = H.shape
    rows = [np.flatnonzero(H[c]) for c in range(m)]
    cols = [np.flatnonzero(H[:, j]) for j in range(n)]
    out_e, out_it, out_p = [], [], []
    for s in syn:
        c2v = np.zeros((m, n))
        post = L.copy()
        iters = max_iter
        for it in range(max_iter):
            new = np.zeros((m, n))
            for c in range(m):
                t = np.tanh((post[rows[c]] - c2v[c, rows[c]]) / 2.0)
                prod = np.float64(1.0)
                for x in t:
                    prod = prod * x
                for k, j in enumerate(rows[c]):
                    th2 = prod / t[k]
                    if np.abs(th2) >= 1 - eps:
                        th2 = th2 - eps * np.sign(th2)
                    val = 2 * np.arctanh(th2)
                    new[c, j] = -val if s[c] else val
            c2v = new
            for j in range(n):
                post[j] = L[j] + np.sum(np.ascontiguousarray(c2v[cols[j], j])) if len(cols[j]) else L[j]
            if np.array_equal((H.astype(np.int64) @ (post < 0)) % 2, s):
                iters = it + 1
                break
        out_e.append((post < 0).astype(np.uint8))
        out_it.append(iters)
        out_p.append(post.copy())
    return np.array(out_e), np.array(out_it, np.int32), np.array(out_p)


def _block8(M):
    """DOUBLE_pairwise_sum's unsplit form on M [..., d], 8 <= d: eight
    accumulators over the blocks of 8, the fixed tree, the remainder in
    sequence. Every add is elementwise over the leading axes."""
    d = M.shape[-1]
    r = [M[..., k] for k in range(8)]
    nb = d - d % 8
    for i in range(8, nb, 8):
        r = [r[k] + M[..., i + k] for k in range(8)]
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for i in range(nb, d):
        res = res + M[..., i]
    return res


def pairwise_sum(M, colsum="numpy"):
    """np.sum along the last axis of M [..., d] in the order np.sum adds a
    contiguous 1-D array of d float64 (colsum="numpy"), or with the eight
    accumulators over the whole length (colsum="strided8")."""
    d = M.shape[-1]
    if d < 8:
        res = np.full(M.shape[:-1], -0.0)
        for i in range(d):
            res = res + M[..., i]
        return res
    if d <= 128 or colsum == "strided8":
        return _block8(M)
    assert colsum == "numpy"
    n2 = d // 2
    n2 -= n2 % 8
    return pairwise_sum(M[..., :n2]) + pairwise_sum(M[..., n2:])


def decode_bp(H, syn, L, max_iter, layers=None, eps=1e-9, colsum="numpy"):
    """BP with prior LLRs L [n] (or [B, n]), flooding (layers None) or layered.
    -> (ehat uint8 [B, n], iters int32 [B], post float64 [B, n], flags int32
    [B]: FLAG_CONVERGED where the last stop test held)."""
    g = H if isinstance(H, pm.Graph) else pm.Graph(H)
    syn = np.asarray(syn).astype(np.int64)
    B = syn.shape[0]
    L = np.ascontiguousarray(np.broadcast_to(np.asarray(L, np.float64), (B, g.n)))
    lay = [np.arange(g.m)] if layers is None else [np.asarray(r, np.int64) for r in layers]
    post = L.copy()
    c2v = np.zeros((B, g.E + 1))                         # [E]: the pad entry of absent edges, always 0
    iters = np.full(B, max_iter, np.int32)
    flags = np.zeros(B, np.int32)
    act = np.ones(B, bool)
    Rv = g.R >= 0
    Rcols = g.ec[np.where(Rv, g.R, 0)]

    def satisfied(idx):
        e = post[idx] < 0
        return np.all(((e[:, Rcols] & Rv).sum(2) & 1) == syn[idx], axis=1)

    for it in range(max_iter):
        for rows in lay:
            idx = np.flatnonzero(act)
            if idx.size == 0 or rows.size == 0:
                continue
            Re = g.R[rows]
            valid = Re >= 0
            V = post[idx][:, g.ec[np.where(valid, Re, 0)]] - c2v[idx][:, np.where(valid, Re, g.E)]
            c = pm._cn_bp(V, valid, syn[idx][:, rows], eps)
            sub = c2v[idx]
            sub[:, Re[valid]] = c[:, valid]
            c2v[idx] = sub
            # the variables of the layer's checks, grouped by degree: one pairwise sum per group
            js = np.unique(g.ec[Re[valid]])
            for d in np.unique(g.dc[js]):
                jd = js[g.dc[js] == d]
                S = pairwise_sum(sub[:, g.C[jd, :d]], colsum)          # [shots, variables, d], ascending check
                post[np.ix_(idx, jd)] = L[np.ix_(idx, jd)] + S
            ok = satisfied(idx)
            iters[idx[ok]] = it + 1
            flags[idx[ok]] |= FLAG_CONVERGED
            act[idx[ok]] = False
    return (post < 0).astype(np.uint8), iters, post, flags


# ---------------------------------------------------------------------------
# the references on the shapes of tests/wide_column_codes.py, computed once
# and shared read-only by the CPU and the GPU tests
# ---------------------------------------------------------------------------
def _frozen(out):
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def graph(sid):
    return pm.Graph(wc.matrix(sid))


def non_partition(sid):
    """The "S5" layers with row 5 once more in the last layer and row 10 in
    none (test_forced_hbm_non_partition_schedule's change): no partition of
    the rows, so the HBM kernels initialise their state (lazy = 0)."""
    lay = [np.asarray(l) for l in wc.layers(sid, "S5")]
    lay[-1] = np.append(lay[-1], 5)
    lay = [l[l != 10] for l in lay]
    assert any(5 in l for l in lay[:-1]) and not any(10 in l for l in lay)
    return lay


def schedule_of(sid, sched):
    return non_partition(sid) if sched == "NP" else wc.layers(sid, sched)


@functools.lru_cache(maxsize=None)
def want_scalar(algo, sid, sched):
    """oracle.decode_batch (its np_pairwise recurses at any length) on the
    shape's batch with the scalar prior p: (ehat, iters, post, flags)."""
    from oracle import oracle
    H = wc.matrix(sid)
    lp, lr = sc.packed(schedule_of(sid, sched), H.shape[0])
    return _frozen(oracle.decode_batch(algo, H, wc.batch(sid), wc.SHAPES[sid]["p"], wc.GPU_MAX_ITER, lp, lr))


def prior_llr(sid):
    return np.array([pm.llr(x) for x in wc.prior_row(sid)])


@functools.lru_cache(maxsize=None)
def want_vprior(sid, sched, colsum="numpy"):
    """decode_bp on the shape's batch with the shape's prior row."""
    return _frozen(decode_bp(graph(sid), wc.batch(sid), prior_llr(sid), wc.GPU_MAX_ITER, schedule_of(sid, sched),
                             colsum=colsum))


@functools.lru_cache(maxsize=None)
def want_uniform(sid, sched, colsum="numpy"):
    """decode_bp with the scalar prior's LLR on every variable."""
    L = np.full(wc.matrix(sid).shape[1], pm.llr(wc.SHAPES[sid]["p"]))
    return _frozen(decode_bp(graph(sid), wc.batch(sid), L, wc.GPU_MAX_ITER, schedule_of(sid, sched), colsum=colsum))

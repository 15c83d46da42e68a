"""NumPy model of relay min-sum with one prior per variable —
TEST INFRASTRUCTURE ONLY. It shares no code with the library and builds on
prior_model's Graph and check node, as relay_model does;
tests/test_gpu_relay_vprior.py compares relay_vprior_kernel with it bit for
bit, and tests/test_relay_vprior_model.py pins it to relay_model (a uniform
row) and to prior_model's min-sum (gamma = 0, one leg).

Per half-shot (q_j the prior probabilities, gamma[r][j] the memory strengths):
  L_j = np.log((1 - q_j) / max(q_j, eps));  W_j = np.rint(L_j 2^20) as int64
  M = L; for each leg r: c2v = 0, S = 0; for t < T[r]:
    Lam = fl((1 - gamma) L) + fl(gamma M)
    check nodes read (f64)(f32)Lam at t = 0, fl(fl(Lam + (f64)S) - (f64)c2v) after
    S = float32 column sums in ascending check order from +0.0f
    M = Lam + (f64)S; e = M < 0; if H e == s: a solution, the leg ends
  the decoder stops after `sols` solutions and keeps the lightest (ties: the
  earlier): cost "hamming" weighs a solution sum_j e_j, cost "prior"
  sum_j e_j W_j (exact integers; W_j < 0 where q_j > 1/2). Without a solution
  e_hat is the last pass's M < 0.
Flags as relay_model's.
"""
import numpy as np

from prior_model import FLAG_CONVERGED, FLAG_MIN_ZERO, Graph, _cn_ms  # noqa: F401

COSTS = ("hamming", "prior")


def llr_row(q, eps=1e-9):
    q = np.asarray(q, np.float64)
    return np.log((1 - q) / np.maximum(q, eps))


def weights(L):
    """W_j = round-half-even of L_j 2^20 (the scaling is exact)."""
    return np.rint(np.asarray(L, np.float64) * 2.0 ** 20).astype(np.int64)


def decode(H, syn, q, leg_iters, gammas, sols=1, cost="hamming", beta=0.75, eps=1e-9):
    """-> (ehat uint8 [B, n], iters int32 [B], post float64 [B, n], flags int32 [B],
    found int32 [B], best_leg int32 [B])."""
    assert cost in COSTS
    g = H if isinstance(H, Graph) else Graph(H)
    syn = np.asarray(syn).astype(np.int64)
    B = syn.shape[0]
    L = llr_row(q, eps)
    assert L.shape == (g.n,) and np.isfinite(L).all()
    W = weights(L) if cost == "prior" else np.ones(g.n, np.int64)
    T = [int(t) for t in np.asarray(leg_iters).reshape(-1)]
    G = np.ascontiguousarray(gammas, np.float64)
    assert G.shape == (len(T), g.n) and min(T) >= 1 and sols >= 1
    M = np.tile(L, (B, 1))
    c2v = np.zeros((B, g.E + 1), np.float32)                 # [E]: the pad entry of absent edges
    S = np.zeros((B, g.n), np.float32)
    iters = np.zeros(B, np.int32)
    flags = np.zeros(B, np.int32)
    found = np.zeros(B, np.int32)
    best = np.zeros((B, g.n), np.uint8)
    best_w = np.full(B, np.iinfo(np.int64).max, np.int64)
    best_leg = -np.ones(B, np.int32)
    alive = np.ones(B, bool)
    valid = g.R >= 0
    Re = np.where(valid, g.R, g.E)
    cols = g.ec[np.where(valid, g.R, 0)] if g.E else np.zeros_like(g.R)
    Cv = g.C >= 0
    Ce = np.where(Cv, g.C, g.E)
    for r, Tr in enumerate(T):
        gam = G[r]
        act = alive.copy()
        c2v[act] = 0
        S[act] = 0
        for t in range(Tr):
            idx = np.flatnonzero(act)
            if idx.size == 0:
                break
            Lam = (1 - gam) * L + gam * M[idx]               # two products, one add
            if t == 0:
                V = (Lam.astype(np.float32).astype(np.float64) + 0.0)[:, cols]
            else:
                V = (Lam + S[idx].astype(np.float64))[:, cols] - c2v[idx][:, Re].astype(np.float64)
            c, z = _cn_ms(V, valid, syn[idx], beta)
            flags[idx[z.any(1)]] |= FLAG_MIN_ZERO
            sub = c2v[idx]
            sub[:, g.R[valid]] = c[:, valid]
            c2v[idx] = sub
            s = np.zeros((len(idx), g.n), np.float32)
            for k in range(g.C.shape[1]):                    # ascending check order, sequential
                s = s + np.where(Cv[:, k], sub[:, Ce[:, k]], np.float32(0)).astype(np.float32)
            S[idx] = s
            Mn = Lam + s.astype(np.float64)
            M[idx] = Mn
            iters[idx] += 1
            e = (Mn < 0)
            ok = np.all((e.astype(np.int64) @ g.H.T) % 2 == syn[idx], axis=1)
            hit = idx[ok]
            found[hit] += 1
            w = e[ok].astype(np.int64) @ W                   # exact: int64
            better = w < best_w[hit]                         # ties keep the earlier one
            best[hit[better]] = e[ok][better]
            best_w[hit[better]] = w[better]
            best_leg[hit[better]] = r
            act[hit] = False
        alive &= found < sols
    ehat = np.where((found > 0)[:, None], best, (M < 0).astype(np.uint8)).astype(np.uint8)
    flags[found > 0] |= FLAG_CONVERGED
    return ehat, iters, M, flags, found, best_leg

"""Batch NumPy model of the two hard-decision decoders (NG, BF), written from
their stated semantics, not from the reference's text. The
fixture test pins it to the reference's recorded outputs; the GPU tests then
use it on fresh inputs, where the reference does not exist.

    bf_batch(H, syn, max_iter=50) -> (e uint8 [B, n], iters int32 [B], conv bool [B])
    ng_batch(H, syn)              -> (e uint8 [B, n], steps int32 [B], info)
        info: dict of bool [B] arrays
          conv       residual all zero on exit
          zero_stop  ended because the largest score was 0 (that step is counted)
          tied       some step's largest score was attained by several variables
    true_syndrome(H, e)           -> H e mod 2, uint8 [B, m]
"""
import numpy as np


def _graph(H):
    H = (np.asarray(H) % 2).astype(np.int64)
    return H, H.shape[0], H.shape[1]


def true_syndrome(H, e):
    H, _, _ = _graph(H)
    return ((np.asarray(e).astype(np.int64) @ H.T) % 2).astype(np.uint8)


def bf_batch(H, syn, max_iter=50):
    """Bit flipping. Per iteration: nuc[v] = failing checks at v; flip e[v]
    where 2 nuc[v] > deg(v); r[c] = (row c holds a set e bit) XOR syn[c] — a
    non-zero count, not a parity. Stops when r is all zero (1-based count);
    otherwise the count is max_iter."""
    H, m, n = _graph(H)
    syn = np.asarray(syn).astype(np.int64)
    B = syn.shape[0]
    deg = H.sum(axis=0)
    Hf = H.astype(np.float32)                         # BLAS products; exact, every count is far below 2^24
    e = np.zeros((B, n), bool)
    r = syn.copy()
    iters = np.full(B, max_iter, np.int32)
    conv = np.zeros(B, bool)
    live = np.arange(B)
    for it in range(1, max_iter + 1):
        if live.size == 0:
            break
        nuc = (r[live].astype(np.float32) @ Hf).astype(np.int64)
        e[live] ^= 2 * nuc > deg
        r[live] = ((e[live].astype(np.float32) @ Hf.T) != 0) ^ (syn[live] != 0)
        done = ~r[live].any(axis=1)
        iters[live[done]] = it
        conv[live[done]] = True
        live = live[~done]
    return e.astype(np.uint8), iters, conv


def ng_batch(H, syn):
    """Naive greedy. While the residual is non-zero and steps < 2n: count the
    step; score[v] = failing checks at v; stop if the largest score is 0; else
    flip the lowest-index variable with the largest score and toggle the
    residual of its checks."""
    H, m, n = _graph(H)
    syn = np.asarray(syn).astype(np.int64)
    B = syn.shape[0]
    # padded adjacency: check m and variable n are dummies that absorb the padding
    dv = max(int(H.sum(axis=0).max(initial=0)), 1)
    dc = max(int(H.sum(axis=1).max(initial=0)), 1)
    col_chk = np.full((n + 1, dv), m, np.int64)
    row_var = np.full((m + 1, dc), n, np.int64)
    for v in range(n):
        c = np.flatnonzero(H[:, v])
        col_chk[v, :c.size] = c
    for c in range(m):
        v = np.flatnonzero(H[c])
        row_var[c, :v.size] = v
    res = np.zeros((B, m + 1), np.int64)
    res[:, :m] = syn
    score = np.zeros((B, n + 1), np.int64)
    score[:, :n] = syn @ H
    e = np.zeros((B, n), np.uint8)
    steps = np.zeros(B, np.int32)
    zero_stop = np.zeros(B, bool)
    tied = np.zeros(B, bool)
    live = np.flatnonzero(res[:, :m].any(axis=1))
    for _ in range(2 * n):
        if live.size == 0:
            break
        steps[live] += 1
        s = score[live, :n]
        best = s.max(axis=1)
        stop = best == 0
        zero_stop[live[stop]] = True
        live, s, best = live[~stop], s[~stop], best[~stop]
        if live.size == 0:
            break
        tied[live] |= (s == best[:, None]).sum(axis=1) > 1
        v = s.argmax(axis=1)                          # lowest index among equals
        e[live, v] ^= 1
        for k in range(dv):                           # check by check
            c = col_chk[v, k]
            res[live, c] ^= 1
            res[:, m] = 0
            delta = 2 * res[live, c] - 1              # +1 if the check now fails, else -1
            delta[c == m] = 0
            score[live[:, None], row_var[c]] += delta[:, None]
        score[:, n] = 0
        live = live[res[live, :m].any(axis=1)]
    conv = ~res[:, :m].any(axis=1)
    return e, steps, {"conv": conv, "zero_stop": zero_stop, "tied": tied}


def golden_cases():
    """[(case dict, arrays dict, H)] of every tests/golden/hard/*.npz case: the
    reference's recorded NG / BF outputs (tests/golden/gen_golden_hard.py)."""
    import json
    import os
    from qldpcsim_amd import codes
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hard")
    out = []
    for f in sorted(os.listdir(root)):
        if not f.endswith(".npz"):
            continue
        with np.load(os.path.join(root, f), allow_pickle=False) as z:
            cases = json.loads(bytes(z["cases_json"]).decode())
            for i, c in enumerate(cases):
                a = {k.split("_", 1)[1]: z[k] for k in z.files if k.startswith(f"c{i}_")}
                if "H" in a:
                    H = a["H"]
                else:
                    Hx, Hz = codes.load_code(c["code"])
                    H = Hz if c["half"] == "X" else Hx
                out.append((c, a, np.asarray(H)))
    return out


def case_id(c):
    return f"{c['code']}-{c['half']}-{c['kind']}-{c['algo']}{c['max_iter'] or ''}"


def synthetic_matrix():
    return next(H for c, _, H in golden_cases() if c["code"] == "synthetic")

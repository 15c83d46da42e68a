"""Golden vectors of the tall shapes (tests/tall_shape_codes.py) from the
UNMODIFIED reference decoders (same method as gen_golden_shapes.py: stub-package
import, settrace capture of the final posteriors; build container only).

One file per shape of tall_shape_codes.GOLDEN_IDS (T2: past the generic
kernel's 2048-check register; U1: uniform degree 8 without the fast table),
tests/golden/tall/tall_<id>.npz: the matrix as its sorted (row, column) pairs
(`H_pairs`, `H_shape`) and, for flooding min-sum, flooding BP and min-sum on
schedule.layerize's layers, the first 8 half-shots of the shape's GPU batch at
max_iter = 20 with the prior p of the shape. Per case the syndromes, hard
decisions, iteration counts, float64 posteriors and the layer arrays.

Usage:  python tests/golden/gen_golden_tall.py   (6 procs, a few minutes)
"""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import gen_golden as g  # noqa: E402
import shape_codes as sc  # noqa: E402
import tall_shape_codes as ts  # noqa: E402

OUT = os.path.join(HERE, "tall")
SHOTS, MAX_ITER = 8, 20


def build_cases():
    return [dict(shape=sid, algo=algo, sched=sched, p=ts.SHAPES[sid]["p"], max_iter=MAX_ITER, shots=SHOTS, id=i)
            for i, (sid, (algo, sched)) in enumerate((s, a) for s in ts.GOLDEN_IDS for a in ts.GOLDEN_ALGOS)]


def run_case(case):
    dec = g.ref_decoders()
    H = np.array(ts.matrix(case["shape"]))
    m, n = H.shape
    layers = [np.arange(m)] if case["sched"] == "F" else ts.layerized(case["shape"])
    syn = np.array(ts.batch(case["shape"])[:case["shots"]])
    K = len(syn)
    ehat = np.zeros((K, n), np.uint8)
    iters = np.zeros(K, np.int32)
    post = np.zeros((K, n), np.float64)
    fn, name = (dec.MS_decoder, "posteriorLLRs") if case["algo"] == "MS" else (dec.BP_decoder, "L_post")
    for k in range(K):
        (e, it), pst = g.run_capture(fn, name, H, syn[k].astype(int), p=case["p"], max_iter=case["max_iter"],
                                     layers=layers, OSDorder=-1)
        ehat[k] = np.asarray(e).astype(np.uint8)
        iters[k] = it
        post[k] = pst
    lp, lr = sc.packed(None if case["sched"] == "F" else layers, m)
    return case, dict(syn=syn, ehat=ehat, iters=iters, post=post, layer_ptr=lp, layer_rows=lr)


def main():
    cases = build_cases()
    results = {}
    with Pool(int(os.environ.get("GOLDEN_PROCS", "6"))) as pool:
        for case, arrs in pool.imap_unordered(run_case, cases):
            results[case["id"]] = (case, arrs)
            print(f"[{len(results)}/{len(cases)}] {case['shape']} {case['algo']} {case['sched']} "
                  f"iters={arrs['iters'].tolist()}", flush=True)
    os.makedirs(OUT, exist_ok=True)
    for sid in ts.GOLDEN_IDS:
        H = ts.matrix(sid)
        out = dict(H_pairs=np.argwhere(H).astype(np.int32), H_shape=np.array(H.shape, np.int32))
        meta = []
        for cid in sorted(results):
            case, arrs = results[cid]
            if case["shape"] != sid:
                continue
            for name, a in arrs.items():
                out[f"c{len(meta)}_{name}"] = a
            meta.append(case)
        out["cases_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(OUT, f"tall_{sid}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, len(meta), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

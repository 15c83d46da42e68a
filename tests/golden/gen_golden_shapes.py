"""Golden vectors of the synthetic shapes (tests/shape_codes.py) from the
UNMODIFIED reference decoders (same method as gen_golden.py: stub-package
import, settrace capture of the final posteriors; build container only).

One file per shape, tests/golden/shapes/shape_<id>.npz (a sub-directory, so
conftest.golden_files() does not sweep them into the bundled codes'
parametrisations): the matrix bit-packed (`H_bits`, `H_shape`) and, for MS and
BP, flooding and the shape's few-layer partition (shape_codes.GOLDEN_PARTITION),
16 half-shots at max_iter = 20: 12 channel shots (independent flips of
probability p, prior p) and 4 uniform-random syndromes. Per case the
syndromes, hard decisions, iteration counts, float64 posteriors and the layer
arrays. Shape F keeps the posteriors of the first 8 shots (file size).

Usage:  python tests/golden/gen_golden_shapes.py   (8 procs, about a minute)
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

OUT = os.path.join(HERE, "shapes")
CHANNEL_SHOTS, RANDOM_SHOTS, MAX_ITER = 12, 4, 20
POST_SHOTS = {"F": 8}


def build_cases():
    cases = []
    for sid in sc.IDS:
        for algo in ("MS", "BP"):
            for sched in ("F", sc.GOLDEN_PARTITION[sid]):
                cases.append(dict(shape=sid, algo=algo, sched=sched, p=sc.SHAPES[sid]["p"], max_iter=MAX_ITER,
                                  channel_shots=CHANNEL_SHOTS, random_shots=RANDOM_SHOTS,
                                  seed=20261020 + 7 * sc.IDS.index(sid), id=len(cases)))
    return cases


def run_case(case):
    dec = g.ref_decoders()
    H = np.array(sc.matrix(case["shape"]))
    m, n = H.shape
    layers = [np.arange(m)] if case["sched"] == "F" else sc.partitions(case["shape"])[case["sched"]]
    rng = np.random.default_rng(case["seed"])           # per shape: its four cases share the syndromes
    syn = np.concatenate([sc.channel_syndromes(H, case["p"], case["channel_shots"], rng),
                          rng.integers(0, 2, (case["random_shots"], m), dtype=np.uint8)])
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
    lp, lr = sc.packed(layers, m)
    return case, dict(syn=syn, ehat=ehat, iters=iters, post=post[:POST_SHOTS.get(case["shape"], K)],
                      layer_ptr=lp, layer_rows=lr)


def main():
    cases = build_cases()
    results = {}
    heavy = lambda c: sc.SHAPES[c["shape"]]["m"] * (20 if c["algo"] == "BP" else 1) * (3 if c["sched"] != "F" else 1)
    with Pool(int(os.environ.get("GOLDEN_PROCS", "8"))) as pool:
        for case, arrs in pool.imap_unordered(run_case, sorted(cases, key=heavy, reverse=True)):
            results[case["id"]] = (case, arrs)
            print(f"[{len(results)}/{len(cases)}] {case['shape']} {case['algo']} {case['sched']} "
                  f"iters={arrs['iters'].tolist()}", flush=True)
    os.makedirs(OUT, exist_ok=True)
    for sid in sc.IDS:
        H = sc.matrix(sid)
        out = dict(H_bits=np.packbits(H, axis=1, bitorder="little"), H_shape=np.array(H.shape, np.int32))
        meta = []
        for cid in sorted(results):
            case, arrs = results[cid]
            if case["shape"] != sid:
                continue
            for name, a in arrs.items():
                out[f"c{len(meta)}_{name}"] = a
            meta.append(case)
        out["cases_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(OUT, f"shape_{sid}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, len(meta), "cases", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

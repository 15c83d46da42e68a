"""Golden OSD estimates of the OSD shape cases (tests/osd_shape_codes.py) from
the UNMODIFIED reference's OSDdec (same method as gen_golden.py: stub-package
import; build container only).

One file per case, tests/golden/osd_shapes/osd_<id>.npz (a sub-directory, so
conftest.golden_files() does not sweep them into the bundled codes'
parametrisations): the matrix bit-packed (`H_bits`, `H_shape`) and, for the
first and the last 4 shots of the case (2 and 2 for c33max and h_m: 4
consistent and 4 arbitrary syndromes, both crafted shots among them), the shot
indices, syndromes, incoming estimates, permutations, the posteriors OSDdec was
fed (osd_shape_codes.order_posteriors: their NumPy order is the committed
permutation, without ties) and the reference's e_hat at orders 0 and 1
(`ehat0`, `ehat1`; `raised0` / `raised1` mark an IndexError, none expected).

Usage:  python tests/golden/gen_golden_osd_shapes.py [id ...]   (8 procs, about 12 minutes;
        OSDdec takes 0.1 s per call at 64 x 255 and minutes at 1024 x 2111)
"""
import json
import os
import sys
import time
from multiprocessing import Pool

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, ".."))
import gen_golden as g  # noqa: E402
import osd_shape_codes as sc  # noqa: E402

OUT = sc.GOLDEN_DIR
ORDERS = (0, 1)


def run_unit(unit):
    name, i, order = unit
    dec = g.ref_decoders()
    H, syn, _, e0, perms = sc.shots(name)
    post = sc.order_posteriors(perms[i], e0[i])
    t0 = time.time()
    try:
        e = dec.OSDdec(np.array(H, dtype=int), np.array(e0[i], dtype=int), np.array(syn[i], dtype=int), post, order)
        e, raised = np.asarray(e).astype(np.uint8), 0
    except IndexError:
        e, raised = np.array(e0[i], np.uint8), 1
    return unit, e, raised, time.time() - t0


def main():
    ids = sys.argv[1:] or sc.IDS                      # (case ids: regenerate those files alone)
    units = [(name, int(i), o) for name in ids for i in sc.golden_shots(name) for o in ORDERS]
    heavy = lambda u: sc.CASES[u[0]]["m"] ** 2 * sc.CASES[u[0]]["n"]          # noqa: E731
    done, t0 = {}, time.time()
    with Pool(int(os.environ.get("GOLDEN_PROCS", "8"))) as pool:
        for unit, e, raised, dt in pool.imap_unordered(run_unit, sorted(units, key=heavy, reverse=True)):
            done[unit] = (e, raised, dt)
            print(f"[{len(done)}/{len(units)}] {unit[0]} shot {unit[1]} order {unit[2]}: {dt:.1f} s"
                  f"{' IndexError' if raised else ''}", flush=True)
    os.makedirs(OUT, exist_ok=True)
    for name in ids:
        H, syn, _, e0, perms = sc.shots(name)
        idx = sc.golden_shots(name)
        out = dict(H_bits=np.packbits(H, axis=1, bitorder="little"), H_shape=np.array(H.shape, np.int32),
                   shots=idx.astype(np.int32), syn=syn[idx], e0=e0[idx], perms=perms[idx],
                   post=np.stack([sc.order_posteriors(perms[i], e0[i]) for i in idx]))
        secs = 0.0
        for o in ORDERS:
            out[f"ehat{o}"] = np.stack([done[(name, int(i), o)][0] for i in idx])
            out[f"raised{o}"] = np.array([done[(name, int(i), o)][1] for i in idx], np.uint8)
            secs += sum(done[(name, int(i), o)][2] for i in idx)
        meta = dict(id=name, crafted=bool(sc.crafted(name)), reference_seconds=round(secs, 1),
                    **{k: v for k, v in sc.CASES[name].items()})
        out["meta_json"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
        path = os.path.join(OUT, f"osd_{name}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")
    print(f"total {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()

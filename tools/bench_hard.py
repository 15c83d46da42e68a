"""Rates of the hard-decision decoders (ng_kernel, bf_kernel) on one GPU:
decoded half-shots/s from kernel time (HIP events, qldpc_timing) over repeated
launches on device-sampled channel syndromes, and end-to-end simulate_p
shots/s for the same setting. One JSON line per setting.

    python tools/bench_hard.py [--code LP118_0] [--batch 262144] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SETTINGS = (("BF", 0.05), ("NG", 0.01), ("NG", 0.05))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", default="LP118_0")
    ap.add_argument("--batch", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sim-shots", type=int, default=1 << 20)
    args = ap.parse_args(argv)
    import torch
    from qldpcsim_amd import _lib, codes, decoders, simulator
    Hx, Hz = codes.load_code(args.code)
    dev = torch.device("cuda", 0)
    for algo, p in SETTINGS:
        ch = simulator.DeviceChannel(Hx, Hz, dev, 20251226)
        sy_z, _, _, _ = ch.sample(p, args.batch, bits=True)
        out = decoders.decode_batch(Hz, sy_z, p / 3, 50, algo=algo, ehat_bits=True)      # warm-up: plan, tables
        torch.cuda.synchronize()
        _lib.timing_enable(True)
        _lib.timing_reset()
        for _ in range(args.reps):
            decoders.decode_batch(Hz, sy_z, p / 3, 50, algo=algo, ehat_bits=True, out=out)
        torch.cuda.synchronize()
        ms, launches = _lib.timing_read()
        _lib.timing_enable(False)
        iters = float(out.iters.double().mean())
        w, b, lds = _lib.launch_info(Hz, None, None, algo, 0)
        simulator.simulate_p(Hx, Hz, p, shots=args.sim_shots // 8, decType=algo, rngSeed=1, verbose=False)   # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = simulator.simulate_p(Hx, Hz, p, shots=args.sim_shots, decType=algo, rngSeed=1, verbose=False)
        dt = time.perf_counter() - t0
        hs_per_s = args.batch * launches / (ms * 1e-3)
        print(json.dumps({
            "code": args.code, "algo": algo, "p": p, "kernel": _lib.kernel_name(Hz, None, None, algo, 0),
            "batch": args.batch, "launches": launches, "kernel_ms_per_launch": round(ms / launches, 4),
            "halfshots_per_s": round(hs_per_s), "mean_count": round(iters, 3),
            "halfshot_counts_per_s": round(hs_per_s * iters),
            "waves_per_wg": w, "wg_per_cu": b, "lds_bytes": lds,
            "simulate_shots": args.sim_shots, "simulate_shots_per_s": round(args.sim_shots / dt),
            "avg_iters_x": r["Avg_number_of_iterations_X"]}), flush=True)


if __name__ == "__main__":
    main()

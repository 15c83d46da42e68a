#!/usr/bin/env python3
"""Measure the phenomenological noise mode on the GPU.

For each (code, rounds) with MS flooding and p_data = q (the scalar decode
entry point):
  - shots/s of simulate_phenomenological (both halves, end to end);
  - phenom_sample_kernel's and phenom_count_kernel's ms per 2^18 shots of the
    X half (HIP events around the launches, bit-packed formats as the
    simulator uses them) and their share of that half-batch's
    sample + decode + count;
  - the logical error rate and its per-round value;
  - where N <= 4096, the ms of the existing generic sampler
    (qldpc_channel_sample_vec) on the materialised space-time matrix for the
    same shots: it draws the same stream, and it walks the matrix twice (its
    X and Z sides; the Z side never fires here).
`--limits` also reports, per (code, rounds) of LP118_0 and LP118_2, whether the
vector-prior path (p_data != q) accepts the shape, and launch_info of the
scalar plan at that shape.

    python tools/bench_phenom.py [--shots 262144] [--p 0.015] [--limits]

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np  # noqa: E402


def _ms(fn, reps=3):
    """Median milliseconds of fn() between HIP events, after one warm-up."""
    import torch
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out))


def measure(name, T, p, shots, iters):
    import torch
    from qldpcsim_amd import _lib, codes, decoders, logicals, simulator, spacetime
    Hx, Hz = codes.load_code(name)
    Lz = logicals.css_logicals(Hx, Hz)[1]
    m, n = Hz.shape
    p_data = q = 2 * p / 3
    dev = torch.device("cuda", 0)
    B = 1 << 18
    half = simulator.DevicePhenomHalf(Hz, Lz, T, dev, 1)
    S = spacetime.spacetime_matrix(Hz, T)
    lp, lr = decoders.pack_layers(None, S.shape[0])
    det, E = half.sample(p_data, q, B, bits=True)
    r = decoders.decode_batch(S, det, p_data, iters, algo="MS", layer_ptr=lp, layer_rows=lr, ehat_bits=True)
    acc = torch.zeros(4, dtype=torch.int64, device=dev)
    t_s = _ms(lambda: half.sample(p_data, q, B, bits=True))
    t_d = _ms(lambda: decoders.decode_batch(S, det, p_data, iters, algo="MS", layer_ptr=lp, layer_rows=lr,
                                            ehat_bits=True, out=r))
    t_c = _ms(lambda: half.count_device(det, E, r.ehat, r.iters, acc))
    row = {"code": name, "rounds": T, "N": half.N, "M": half.M, "p": p, "p_data": p_data, "q": q, "iters": iters,
           "kernel": _lib.kernel_name(S, lp, lr, "MS", 0), "launch_info": _lib.launch_info(S, lp, lr, "MS", 0),
           "sample_ms_per_2^18": round(t_s, 3), "count_ms_per_2^18": round(t_c, 3),
           "decode_ms_per_2^18": round(t_d, 3), "sample_share": round(t_s / (t_s + t_d + t_c), 4),
           "count_share": round(t_c / (t_s + t_d + t_c), 4)}
    if half.N <= 4096:
        ch = simulator.DeviceChannel(S, S, dev, 1)
        pr = spacetime.spacetime_prior(n, m, T, p_data, q)
        ch.set_probs(np.stack([pr, np.zeros_like(pr), np.zeros_like(pr)]))
        row["generic_sample_ms_per_2^18"] = round(_ms(lambda: ch.sample(0.0, B, bits=True)), 3)
    simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=min(shots, 4096), decIterations=iters, rngSeed=1,
                                        verbose=False)                       # warm-up: plans, tables
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=shots, decIterations=iters, rngSeed=1,
                                              verbose=False)
    dt = time.perf_counter() - t0
    row.update(shots=shots, shots_per_s=round(shots / dt, 1), logical_error_rate=res["logical_error_rate"],
               logical_error_rate_per_round=res["logical_error_rate_per_round"],
               failures=[res["DecFailures_X"], res["DecFailures_Z"]],
               logical_errors=[res["logicalErrors_X"], res["logicalErrors_Z"]])
    return row


def limits():
    """Which (code, rounds) the vector-prior path accepts, and the scalar plan's launch_info there."""
    import torch
    from qldpcsim_amd import _lib, codes, decoders, spacetime
    dev = torch.device("cuda", 0)
    for name in ("LP118_0", "LP118_2"):
        Hz = codes.load_code(name)[1]
        m, n = Hz.shape
        for T in (2, 3, 4, 5):
            S = spacetime.spacetime_matrix(Hz, T)
            lp, lr = decoders.pack_layers(None, S.shape[0])
            syn = torch.zeros((1, S.shape[0]), dtype=torch.uint8, device=dev)
            row = {"limits": name, "rounds": T, "shape": list(S.shape)}
            for algo in ("MS", "BP"):
                try:
                    decoders.decode_batch(S, syn, None, 1, algo=algo, prior=spacetime.spacetime_prior(n, m, T, .02, .01))
                    row[algo + "_vprior"] = "accepted"
                except NotImplementedError as e:
                    row[algo + "_vprior"] = "refused: " + str(e)
                row[algo + "_scalar"] = [_lib.kernel_name(S, lp, lr, algo, 0), _lib.launch_info(S, lp, lr, algo, 0)]
            print(json.dumps(row), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codes", nargs="+", default=["LP04_0", "LP118_0"])
    ap.add_argument("--rounds", type=int, nargs="+", default=[1, 3, 5])
    ap.add_argument("--p", type=float, default=0.015, help="depolarizing strength (p_data = q = 2p/3)")
    ap.add_argument("--shots", type=int, default=1 << 18)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--limits", action="store_true")
    a = ap.parse_args(argv)
    for name in a.codes:
        for T in a.rounds:
            print(json.dumps(measure(name, T, a.p, a.shots, a.iters)), flush=True)
    if a.limits:
        limits()


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measure sliding-window decoding of the phenomenological noise mode on the
GPU.

Workload: MS flooding, 50 iterations, p_data = q = 0.01 (the scalar decode
entry point), LP04_0 and LP118_0 at T = 5, 10 and 20 with (W, F) = (3, 1) and
(4, 2), and the whole-matrix decode at T = 5 as the reference point. Per
configuration:
  - shots/s of simulate_phenomenological (both halves, end to end);
  - the logical error rate with its 95 % interval and the failures and
    logical errors per half;
  - kernel_name / launch_info of the window matrices' decode plans;
  - phenom_window_kernel's ms per launch at 2^18 shots of the X half (HIP
    events; the first cut, a middle step and the last commit, bit-packed
    formats as the simulator uses them) and the share of all of a
    half-batch's window steps in its sample + windows + count.
`--unequal` runs the same at LP118_0, T = 8 with p_data = 0.01, q = 0.005 (the
vector-prior path, which refuses the whole matrix at that T).

`--converge` reports instead, for the first window of T = 6 on 2^15 shots of the
X half: min-sum's mean iterations and converged fraction on the open window of
3 and 4 rounds and on the closed matrix of 3 rounds, the mean iterations of
the converged shots, and the shots with an unsatisfied check per window round.

    python tools/bench_window.py [--shots 262144] [--unequal] [--converge]

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np  # noqa: E402

from bench_phenom import _ms  # noqa: E402


def _plans(Hz, T, wins, p_data, q, algo="MS"):
    """kernel name and launch_info of each matrix the schedule decodes."""
    from qldpcsim_amd import _lib, decoders, spacetime
    m, n = Hz.shape
    out = {}
    for R, closed in sorted({(w[1], w[2]) for w in wins}):
        S = spacetime.spacetime_matrix(Hz, R) if closed else spacetime.window_matrix(Hz, R)
        lp, lr = decoders.pack_layers(None, S.shape[0])
        key = f"{'closed' if closed else 'open'}_{R}"
        if p_data == q:
            out[key] = {"shape": list(S.shape), "kernel": _lib.kernel_name(S, lp, lr, algo, 0),
                        "launch_info": _lib.launch_info(S, lp, lr, algo, 0)}
        else:
            out[key] = {"shape": list(S.shape), "kernel": _lib.vprior_kernel_name(S, lp, lr, algo, 0)}
    return out


def _advance_times(Hx, Hz, T, W, F, p_data, q, iters, B):
    """ms per launch of phenom_window_kernel on the X half (first cut, middle
    step, last commit) and the share of a half-batch's window steps."""
    import torch
    from qldpcsim_amd import logicals, simulator, spacetime
    Lz = logicals.css_logicals(Hx, Hz)[1]
    m, n = Hz.shape
    dev = torch.device("cuda", 0)
    s = simulator.DevicePhenomHalf(Hz, Lz, T, dev, 1)
    wins = spacetime.window_schedule(T, W, F)
    recs = {}
    for R, closed in {(w[1], w[2]) for w in wins}:
        S = spacetime.spacetime_matrix(Hz, R) if closed else spacetime.window_matrix(Hz, R)
        pr = (spacetime.spacetime_prior if closed else spacetime.window_prior)(n, m, R, p_data, q)
        recs[R, closed] = simulator._Half(S, *simulator.pack_layers(None, S.shape[0]),
                                          *simulator._half_prior(pr, False), (Hz, Lz))
    dec = simulator._Decode("MS", iters, -1, *simulator._path_kw(True, -1))
    det, E = s.sample(p_data, q, B, bits=True)
    acc = torch.zeros(4, dtype=torch.int64, device=dev)

    def half_batch():
        d, e = s.sample(p_data, q, B, bits=True)
        ehat, it = simulator._decode_windows(recs, s, wins, d, dec, True)
        s.count_device(d, e, ehat, it, acc)

    ehat = torch.zeros((B, s.NW), dtype=torch.int64, device=dev)
    it = torch.zeros(B, dtype=torch.int32, device=dev)
    west = torch.zeros((B, (spacetime.window_shape(n, m, wins[0][1], wins[0][2])[1] + 63) // 64), dtype=torch.int64,
                       device=dev)
    last = torch.zeros((B, (spacetime.window_shape(n, m, wins[-1][1], True)[1] + 63) // 64), dtype=torch.int64,
                       device=dev)
    t = {"first": _ms(lambda: s.advance(det, ehat, it, None, None, None, wins[0], bits=True)),
         "last": _ms(lambda: s.advance(det, ehat, it, wins[-1], last, it.clone(), None))}
    if len(wins) > 1:
        t["middle"] = _ms(lambda: s.advance(det, ehat, it, wins[0], west, it.clone(), wins[1], bits=True))
    total = t["first"] + t["last"] + (len(wins) - 1) * t.get("middle", 0.0)
    t_half = _ms(half_batch)
    return {"advance_ms_per_launch": {k: round(v, 4) for k, v in t.items()}, "advance_launches": len(wins) + 1,
            "half_batch_ms": round(t_half, 3), "advance_share": round(total / t_half, 4)}


def measure(name, T, WF, p_data, q, shots, iters, B):
    import torch
    from qldpcsim_amd import codes, simulator, spacetime
    Hx, Hz = codes.load_code(name)
    p = 1.5 * p_data
    kw = {} if WF is None else {"window": WF[0], "commit": WF[1]}
    wins = [(0, T, True, T)] if WF is None else spacetime.window_schedule(T, *WF)
    row = {"code": name, "rounds": T, "window": None if WF is None else list(WF), "windows": len(wins),
           "p_data": p_data, "q": q, "iters": iters, "shots": shots}
    try:
        simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=min(shots, 4096), decIterations=iters, rngSeed=1,
                                            verbose=False, **kw)                  # warm-up: plans, tables
    except NotImplementedError as e:
        row["refused"] = str(e)
        return row
    row["plans"] = _plans(Hz, T, wins, p_data, q)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = simulator.simulate_phenomenological(Hx, Hz, p, q, T, shots=shots, decIterations=iters, rngSeed=1,
                                              verbose=False, **kw)
    dt = time.perf_counter() - t0
    row.update(shots_per_s=round(shots / dt, 1), logical_error_rate=res["logical_error_rate"],
               logical_error_rate_ci95=list(res["logical_error_rate_ci95"]),
               logical_error_rate_per_round=res["logical_error_rate_per_round"],
               failures=[res["DecFailures_X"], res["DecFailures_Z"]],
               logical_errors=[res["logicalErrors_X"], res["logicalErrors_Z"]],
               mean_iterations=[round(res["nIterAccX"] / shots, 3), round(res["nIterAccZ"] / shots, 3)])
    if WF is not None:
        row.update(_advance_times(Hx, Hz, T, *WF, p_data, q, iters, B))
    return row


def converge(name, iters, B=1 << 15):
    """Where min-sum's iterations go on an open window (see the module docstring)."""
    import torch
    from qldpcsim_amd import codes, decoders, logicals, simulator, spacetime
    Hx, Hz = codes.load_code(name)
    Lz = logicals.css_logicals(Hx, Hz)[1]
    m = Hz.shape[0]
    dev = torch.device("cuda", 0)
    det = simulator.DevicePhenomHalf(Hz, Lz, 6, dev, 1).sample(0.01, 0.01, B)[0]
    for W, closed in ((3, False), (4, False), (3, True)):
        if closed:                                  # the closed matrix decodes its own consistent detectors
            S = spacetime.spacetime_matrix(Hz, W)
            syn = simulator.DevicePhenomHalf(Hz, Lz, W, dev, 1).sample(0.01, 0.01, B)[0]
        else:
            S = spacetime.window_matrix(Hz, W)
            syn = det[:, :W * m].contiguous()
        r = decoders.decode_batch(S, syn, 0.01, iters, algo="MS")
        torch.cuda.synchronize()
        it, conv = r.iters.cpu().numpy(), r.converged.cpu().numpy()
        resid = ((r.ehat.cpu().numpy().astype(np.float32) @ S.T.astype(np.float32)).astype(np.int64) & 1) ^ \
            syn.cpu().numpy()
        print(json.dumps({"converge": name, "rounds": W, "closed": closed, "shots": B, "iters": iters,
                          "mean_iterations": round(float(it.mean()), 3), "converged": round(float(conv.mean()), 4),
                          "mean_iterations_converged": round(float(it[conv].mean()), 3),
                          "shots_unsatisfied_by_round": [int(resid[:, t * m:(t + 1) * m].any(axis=1).sum())
                                                         for t in range(W)]}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codes", nargs="+", default=["LP04_0", "LP118_0"])
    ap.add_argument("--rounds", type=int, nargs="+", default=[5, 10, 20])
    ap.add_argument("--shots", type=int, default=1 << 18)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--batch", type=int, default=1 << 18, help="shots of the advance kernel's timing")
    ap.add_argument("--unequal", action="store_true", help="LP118_0, T = 8, p_data = 0.01, q = 0.005")
    ap.add_argument("--converge", action="store_true", help="only: where the iterations of an open window go")
    a = ap.parse_args(argv)
    if a.converge:
        for name in a.codes:
            converge(name, a.iters)
        return
    for name in a.codes:
        print(json.dumps(measure(name, 5, None, 0.01, 0.01, a.shots, a.iters, a.batch)), flush=True)
        for T in a.rounds:
            for WF in ((3, 1), (4, 2)):
                print(json.dumps(measure(name, T, WF, 0.01, 0.01, a.shots, a.iters, a.batch)), flush=True)
    if a.unequal:
        for WF in (None, (3, 1), (4, 2)):
            print(json.dumps(measure("LP118_0", 8, WF, 0.01, 0.005, a.shots, a.iters, a.batch)), flush=True)


if __name__ == "__main__":
    main()

"""Cost and gain of relay min-sum (relay_ms_kernel, simulate_p(decType="RELAY"))
on one GPU.

Kernel side (--kernels): one batch of 2^18 half-shots of LP118_0 Hz, uniform
random syndromes (fixed work), 50 iterations, decoded by
    relay    relay_ms_kernel<8>, one leg, gamma = 0, S = 1 (the same results)
    generic  decode_kernel<0, false, 8>, the generic LDS kernel (flood_generic)
    default  the kernel the min-sum decode takes by default
alternating in one process (the library's HIP events around each launch, after
a warm-up of all three). One JSON line: ms per launch of every repeat, relay /
generic and generic / default of the best ones, and every kernel's launch
geometry (waves per workgroup, workgroups per CU, LDS bytes).

End to end (default): simulate_p shots/s, logical=True, a baseline and RELAY
with the simulator's defaults (decIterations = the baseline's), interleaved,
twice each after a warm-up of both, on
    LP118_0  MS flooding, 50 iterations, p = 0.05 and p = 0.07
    LP118_2  MS layered + OSD-0, 50 iterations, p = 0.05
with both sides' failures per half, logical_error_rate and 95 % Wilson interval.

    python tools/bench_relay.py [--kernels] [--only N] [--scale S] [--batch B] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WORKLOADS = (
    dict(code="LP118_0", decType="MS", decSchedule="F", decIterations=50, OSDorder=-1, p=0.05, shots=1 << 21),
    dict(code="LP118_0", decType="MS", decSchedule="F", decIterations=50, OSDorder=-1, p=0.07, shots=1 << 20),
    dict(code="LP118_2", decType="MS", decSchedule="L", decIterations=50, OSDorder=0, p=0.05, shots=1 << 20),
)


def _rate(simulator, Hx, Hz, w, shots, relay):
    import torch
    kw = dict(decType="RELAY", decSchedule="F", OSDorder=-1) if relay else \
        dict(decType=w["decType"], decSchedule=w["decSchedule"], OSDorder=w["OSDorder"])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = simulator.simulate_p(Hx, Hz, w["p"], shots=shots, decIterations=w["decIterations"], rngSeed=1, verbose=False,
                             logical=True, **kw)
    return shots / (time.perf_counter() - t0), r


def end_to_end(args):
    from qldpcsim_amd import codes, simulator
    for i, w in enumerate(WORKLOADS):
        if args.only is not None and i != args.only:
            continue
        Hx, Hz = codes.load_code(w["code"])
        shots = max(1, int(w["shots"] * args.scale))
        sides = (False, True)
        for s in sides:                                    # warm-up: plans, tables, logical operators
            _rate(simulator, Hx, Hz, w, max(1, shots // 8), s)
        runs, last = {s: [] for s in sides}, {}
        for _ in range(2):
            for s in sides:
                rate, last[s] = _rate(simulator, Hx, Hz, w, shots, s)
                runs[s].append(round(rate))
        out = dict(w, shots=shots, baseline_shots_per_s=runs[False], relay_shots_per_s=runs[True],
                   relay_over_baseline=round(max(runs[True]) / max(runs[False]), 4))
        for s, name in ((False, "baseline"), (True, "relay")):
            r = last[s]
            out[f"{name}_failures_XZ"] = [r["DecFailures_X"], r["DecFailures_Z"]]
            out[f"{name}_avg_iterations_XZ"] = [r["Avg_number_of_iterations_X"], r["Avg_number_of_iterations_Z"]]
            out[f"{name}_logical_error_rate"] = r["logical_error_rate"]
            out[f"{name}_ci95"] = r["logical_error_rate_ci95"]
        print(json.dumps(out), flush=True)


def kernels(args):
    import numpy as np
    import torch
    from qldpcsim_amd import _lib, codes, decoders, simulator
    dev = torch.device("cuda", 0)
    B = args.batch
    Hx, Hz = codes.load_code("LP118_0")
    m, n = Hz.shape
    lp, lr = simulator.pack_layers(None, m)
    g = torch.Generator(device=dev).manual_seed(20251226)
    syn = decoders.pack_bits(torch.randint(0, 2, (B, m), dtype=torch.uint8, device=dev, generator=g))
    p, iters = 0.05 / 3, 50
    cfg = decoders.RelayConfig([iters], np.zeros((1, n)), 1)
    outs = {}

    def run(side):
        # the library's own launch timing (HIP events around the kernel alone)
        _lib.timing_reset()
        if side == "relay":
            r = decoders.decode_batch(Hz, syn, p, 0, algo="RELAY", relay=cfg, ehat_bits=True, out=outs.get(side))
        elif side == "generic":
            with _lib.options(flood_generic=1):
                r = decoders.decode_batch(Hz, syn, p, iters, algo="MS", ehat_bits=True, out=outs.get(side))
        else:
            r = decoders.decode_batch(Hz, syn, p, iters, algo="MS", ehat_bits=True, out=outs.get(side))
        torch.cuda.synchronize()
        outs[side] = r
        return round(_lib.timing_read()[0], 4)
    _lib.timing_enable(True)
    sides = ("relay", "generic", "default")
    for s in sides:
        run(s)
    ms = {s: [] for s in sides}
    for _ in range(args.reps):
        for s in sides:
            ms[s].append(run(s))
    _lib.timing_enable(False)
    same = all(torch.equal(outs["relay"].ehat, outs[s].ehat) and torch.equal(outs["relay"].iters, outs[s].iters)
               for s in sides)
    rl = _lib.code_for(Hz, 0).relay(cfg.leg_iters, cfg.gammas, 1)
    with _lib.options(flood_generic=1):
        generic = (_lib.kernel_name(Hz, lp, lr, "MS", 0), _lib.launch_info(Hz, lp, lr, "MS", 0))
    default = (_lib.kernel_name(Hz, lp, lr, "MS", 0), _lib.launch_info(Hz, lp, lr, "MS", 0))
    out = dict(code="LP118_0", syndromes="random", iterations=iters, batch=B,
               kernels=dict(relay=rl.kernel_name(), generic=generic[0], default=default[0]),
               waves_wgs_lds=dict(relay=rl.launch_info(), generic=generic[1], default=default[1]),
               ms=ms, relay_over_generic=round(min(ms["relay"]) / min(ms["generic"]), 4),
               generic_over_default=round(min(ms["generic"]) / min(ms["default"]), 4), same_results=same,
               mean_iterations=float(outs["relay"].iters.double().mean()))
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="index of the one end-to-end workload to run")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every end-to-end workload's shots")
    ap.add_argument("--batch", type=int, default=1 << 18, help="half-shots of the kernel-side batch")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    return kernels(args) if args.kernels else end_to_end(args)


if __name__ == "__main__":
    main()

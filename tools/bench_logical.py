"""Cost of the logical outcome counters (simulate_p(logical=True)) on one GPU.

End to end: simulate_p with `logical` off and on, interleaved, twice each
(after one warm-up of both), on
    LP118_0  MS flooding, 50 iterations, p = 0.01   (the counters weigh most here)
    LP118_2  MS layered + OSD-0, 50 iterations, p = 0.05
One JSON line per workload: shots/s of every run and the on/off ratio of the
best runs. Kernel side (--kernels): the counter kernels alone on one
device-sampled batch (HIP events over repeated launches): count_outcomes_kernel
against count_logical_kernel with its tables in LDS and in global memory.

    python tools/bench_logical.py [--tabs 0|1|2] [--off-only] [--kernels] [--only N]

--off-only times the `logical=False` runs alone (also against a library built
without the option: QLDPC_LIB=...).
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WORKLOADS = (
    dict(code="LP118_0", decType="MS", decSchedule="F", decIterations=50, OSDorder=-1, p=0.01, shots=1 << 25),
    dict(code="LP118_2", decType="MS", decSchedule="L", decIterations=50, OSDorder=0, p=0.05, shots=1 << 21),
)


def _rate(simulator, Hx, Hz, w, shots, logical):
    import torch
    kw = {"logical": True} if logical else {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = simulator.simulate_p(Hx, Hz, w["p"], shots=shots, decType=w["decType"], decIterations=w["decIterations"],
                             decSchedule=w["decSchedule"], OSDorder=w["OSDorder"], rngSeed=1, verbose=False, **kw)
    return shots / (time.perf_counter() - t0), r


def end_to_end(args):
    from qldpcsim_amd import codes, simulator
    for i, w in enumerate(WORKLOADS):
        if args.only is not None and i != args.only:
            continue
        Hx, Hz = codes.load_code(w["code"])
        shots = max(1, int(w["shots"] * args.scale))
        modes = (False,) if args.off_only else (False, True)
        for m in modes:                                    # warm-up: plans, tables, logical operators
            _rate(simulator, Hx, Hz, w, max(1, shots // 8), m)
        runs = {m: [] for m in modes}
        last = {}
        for _ in range(2):
            for m in modes:
                rate, last[m] = _rate(simulator, Hx, Hz, w, shots, m)
                runs[m].append(round(rate))
        out = dict(w, shots=shots, tabs=args.tabs, off_shots_per_s=runs[False])
        if True in runs:
            out.update(on_shots_per_s=runs[True], on_over_off=round(max(runs[True]) / max(runs[False]), 4),
                       logical_error_rate=last[True]["logical_error_rate"],
                       reference_block_error_rate=1. - (last[True]["decSuccessExact"]
                                                        + last[True]["decSuccessDegen"]) / shots)
        print(json.dumps(out), flush=True)


def kernels(args):
    """ms per launch of the counter kernels on one bit-packed batch."""
    import torch
    from qldpcsim_amd import _lib, codes, decoders, simulator
    dev = torch.device("cuda", 0)
    for code in ("LP118_0", "LP118_2"):
        Hx, Hz = codes.load_code(code)
        ch = simulator.DeviceChannel(Hx, Hz, dev, 20251226)
        B = args.batch
        sy_z, sy_x, errX, errZ = ch.sample(0.01, B, bits=True)
        rX = decoders.decode_batch(Hz, sy_z, 0.01 / 3, 50, algo="MS", ehat_bits=True)
        rZ = decoders.decode_batch(Hx, sy_x, 0.01 / 3, 50, algo="MS", ehat_bits=True)
        a = (sy_z, sy_x, errX, errZ, rX.ehat, rZ.ehat, rX.iters, rZ.iters)

        def timed(fn):
            fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return round(e0.elapsed_time(e1) / args.reps, 4)
        out = {"code": code, "batch": B, "k": ch.logicals().k,
               "count_outcomes_ms": timed(lambda: ch.count_device(*a))}
        for name, mode in (("lds", 1), ("global", 2)):
            with _lib.options(logical_tabs=mode):
                try:
                    out[f"count_logical_{name}_ms"] = timed(lambda: ch.count_logical_device(*a))
                except NotImplementedError as e:           # the tables do not fit this device's LDS
                    out[f"count_logical_{name}_ms"] = None
                    out["note"] = str(e)
        print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tabs", type=int, default=0, help="library option logical_tabs for the end-to-end runs")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="index of the one workload to run")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every workload's shots")
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args(argv)
    from qldpcsim_amd import _lib
    if args.kernels:
        return kernels(args)
    if args.off_only:
        return end_to_end(args)
    with _lib.options(logical_tabs=args.tabs):
        end_to_end(args)


if __name__ == "__main__":
    main()

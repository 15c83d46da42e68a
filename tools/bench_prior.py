"""Cost and gain of two-level priors (decode_prior_kernel, simulate_p(correlated=))
on one GPU.

Kernel side (--kernels): one batch of 2^18 half-shots decoded by
    prior    decode_prior_kernel, a random 5 % mask with p0 == p1 (the same
             arithmetic and results as the scalar decode)
    generic  decode_kernel, its parent (options flood_generic / layered_generic)
    default  the specialised kernel the scalar decode takes by default
alternating in one process (the library's HIP events around each launch,
after a warm-up of all three), on
    LP118_0  MS flooding, 50 iterations, uniform random syndromes (fixed work)
    LP118_2  MS layered, 50 iterations, channel syndromes at p = 0.05
One JSON line per workload: ms per launch of every repeat, prior / generic and
generic / default of the best ones. The second ratio is the known price of
routing the second half through the generic kernel.

End to end (default): simulate_p shots/s with correlated=None and "XZ",
interleaved, twice each after a warm-up of both, logical=True, on
    LP118_0  MS flooding, 50 iterations, p = 0.01 and p = 0.05
    LP118_2  MS layered + OSD-0, 50 iterations, p = 0.05
with both modes' logical_error_rate and 95 % Wilson interval.

    python tools/bench_prior.py [--kernels] [--only N] [--scale S] [--batch B] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

WORKLOADS = (
    dict(code="LP118_0", decType="MS", decSchedule="F", decIterations=50, OSDorder=-1, p=0.01, shots=1 << 24),
    dict(code="LP118_0", decType="MS", decSchedule="F", decIterations=50, OSDorder=-1, p=0.05, shots=1 << 22),
    dict(code="LP118_2", decType="MS", decSchedule="L", decIterations=50, OSDorder=0, p=0.05, shots=1 << 20),
)
KERNEL_WORKLOADS = (
    dict(code="LP118_0", decSchedule="F", syndromes="random", p=0.05),
    dict(code="LP118_2", decSchedule="L", syndromes="channel", p=0.05),
)
GENERIC = dict(flood_generic=1, layered_generic=1)


def _rate(simulator, Hx, Hz, w, shots, correlated):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = simulator.simulate_p(Hx, Hz, w["p"], shots=shots, decType=w["decType"], decIterations=w["decIterations"],
                             decSchedule=w["decSchedule"], OSDorder=w["OSDorder"], rngSeed=1, verbose=False,
                             logical=True, correlated=correlated)
    return shots / (time.perf_counter() - t0), r


def end_to_end(args):
    from qldpcsim_amd import codes, simulator
    for i, w in enumerate(WORKLOADS):
        if args.only is not None and i != args.only:
            continue
        Hx, Hz = codes.load_code(w["code"])
        shots = max(1, int(w["shots"] * args.scale))
        modes = (None, "XZ")
        for m in modes:                                    # warm-up: plans, tables, logical operators
            _rate(simulator, Hx, Hz, w, max(1, shots // 8), m)
        runs, last = {m: [] for m in modes}, {}
        for _ in range(2):
            for m in modes:
                rate, last[m] = _rate(simulator, Hx, Hz, w, shots, m)
                runs[m].append(round(rate))
        out = dict(w, shots=shots, independent_shots_per_s=runs[None], correlated_shots_per_s=runs["XZ"],
                   correlated_over_independent=round(max(runs["XZ"]) / max(runs[None]), 4))
        for m, name in ((None, "independent"), ("XZ", "correlated")):
            out[f"{name}_logical_error_rate"] = last[m]["logical_error_rate"]
            out[f"{name}_ci95"] = last[m]["logical_error_rate_ci95"]
            out[f"{name}_second_half_events"] = last[m]["logicalErrors_Z"] + last[m]["DecFailures_Z"]
        print(json.dumps(out), flush=True)


def kernels(args):
    import numpy as np
    import torch
    from qldpcsim_amd import _lib, codes, decoders, simulator
    dev = torch.device("cuda", 0)
    B = args.batch
    for i, w in enumerate(KERNEL_WORKLOADS):
        if args.only is not None and i != args.only:
            continue
        Hx, Hz = codes.load_code(w["code"])
        layers = simulator.select_layers(Hx, Hz, w["decSchedule"])[0]
        lp, lr = simulator.pack_layers(layers, Hz.shape[0])
        if w["syndromes"] == "random":
            g = torch.Generator(device=dev).manual_seed(20251226)
            syn = decoders.pack_bits(torch.randint(0, 2, (B, Hz.shape[0]), dtype=torch.uint8, device=dev, generator=g))
        else:
            syn = simulator.DeviceChannel(Hx, Hz, dev, 20251226).sample(w["p"], B, bits=True)[0]
        mask = decoders.pack_bits(torch.as_tensor(
            (np.random.default_rng(1).random((B, Hz.shape[1])) < 0.05).astype(np.uint8), device=dev))
        p = w["p"] / 3
        kw = dict(algo="MS", layer_ptr=lp, layer_rows=lr, ehat_bits=True)
        outs = {}

        def run(side):
            # the library's own launch timing (HIP events around the kernel
            # alone: switching options rebuilds the launch plan on the host)
            _lib.timing_reset()
            if side == "prior":
                r = decoders.decode_batch(Hz, syn, p, 50, prior_mask=mask, p_masked=p, out=outs.get(side), **kw)
            elif side == "generic":
                with _lib.options(**GENERIC):
                    r = decoders.decode_batch(Hz, syn, p, 50, out=outs.get(side), **kw)
            else:
                r = decoders.decode_batch(Hz, syn, p, 50, out=outs.get(side), **kw)
            torch.cuda.synchronize()
            outs[side] = r
            return round(_lib.timing_read()[0], 4)
        _lib.timing_enable(True)
        sides = ("prior", "generic", "default")
        for s in sides:
            run(s)
        ms = {s: [] for s in sides}
        for _ in range(args.reps):
            for s in sides:
                ms[s].append(run(s))
        same = all(torch.equal(outs["prior"].ehat, outs[s].ehat) and torch.equal(outs["prior"].iters, outs[s].iters)
                   for s in sides)
        with _lib.options(**GENERIC):
            generic_name = _lib.kernel_name(Hz, lp, lr, "MS", 0)
        out = dict(w, batch=B, kernels=dict(prior=_lib.prior_kernel_name(Hz, lp, lr, "MS", 0), generic=generic_name,
                                            default=_lib.kernel_name(Hz, lp, lr, "MS", 0)),
                   ms=ms, prior_over_generic=round(min(ms["prior"]) / min(ms["generic"]), 4),
                   generic_over_default=round(min(ms["generic"]) / min(ms["default"]), 4), same_results=same,
                   mean_iterations=float(outs["prior"].iters.double().mean()))
        print(json.dumps(out), flush=True)
    _lib.timing_enable(False)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="index of the one workload to run")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every end-to-end workload's shots")
    ap.add_argument("--batch", type=int, default=1 << 18, help="half-shots of the kernel-side batch")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    return kernels(args) if args.kernels else end_to_end(args)


if __name__ == "__main__":
    main()

"""Cost and gain of per-qubit priors (decode_vprior_kernel,
simulate_p(channel_weights=)) on one GPU.

Kernel side (--kernels): one batch of 2^18 half-shots decoded by
    vprior   decode_vprior_kernel, a uniform vector (the same arithmetic and
             results as the scalar decode)
    prior    decode_prior_kernel, a random 5 % mask with p0 == p1
    generic  decode_kernel, their parent (options flood_generic / layered_generic)
    default  the specialised kernel the scalar decode takes by default
alternating in one process (the library's HIP events around each launch,
after a warm-up of all four), on
    LP118_0  MS flooding, 50 iterations, uniform random syndromes (fixed work)
    LP118_2  MS layered, 50 iterations, channel syndromes at p = 0.05
One JSON line per workload: ms per launch of every repeat, the spread
(max / min - 1) of each side, and vprior / prior, vprior / generic of the best.

End to end (default): simulate_p shots/s, logical=True, LP118_0 MS flooding,
50 iterations, p = 0.05, interleaved, twice each after a warm-up of all:
    depolarizing     no channel_weights (the parent commit's path)
    bias0.5          channel_weights = bias_weights(0.5): the same channel and
                     shots through the per-qubit sampler, decoded with the scalar
                     prior 2p/3 (the sampler twin's own cost)
    bias10           channel_weights = bias_weights(10): uniform marginals, the
                     scalar entry point and the specialised kernels
    inhomogeneous    a quarter of the qubits five times as noisy as the rest
                     (same mean): the vector entry point
    inhomogeneous_mean  the same channel decoded with each half's mean marginal
                     as a scalar prior (what a caller without prior= does)
with each one's logical_error_rate and 95 % Wilson interval.

    python tools/bench_vprior.py [--kernels] [--only N] [--scale S] [--batch B] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

E2E = dict(code="LP118_0", decType="MS", decSchedule="F", decIterations=50, p=0.05, shots=1 << 22)
KERNEL_WORKLOADS = (
    dict(code="LP118_0", decSchedule="F", syndromes="random", p=0.05),
    dict(code="LP118_2", decSchedule="L", syndromes="channel", p=0.05),
)
GENERIC = dict(flood_generic=1, layered_generic=1)


def inhomogeneous_weights(n):
    """[3, n]: X, Y, Z equally likely on every qubit; a quarter of the qubits
    (a fixed random choice) five times as noisy as the rest, mean total 1."""
    import numpy as np
    hot = np.random.default_rng(5).permutation(n)[:n // 4]
    t = np.full(n, 1.0)
    t[hot] = 5.0
    t /= t.mean()
    return np.tile(t / 3, (3, 1))


def _rate(simulator, Hx, Hz, shots, weights, mean_prior=False):
    import numpy as np
    import torch
    from qldpcsim_amd import decoders
    real = decoders.decode_batch
    if mean_prior:
        # the vector channel, decoded with the mean of the half's marginals
        def scalar(H, syn, p, *a, prior=None, **kw):
            return real(H, syn, float(np.mean(prior)) if prior is not None else p, *a, **kw)
        decoders.decode_batch = scalar
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = simulator.simulate_p(Hx, Hz, E2E["p"], shots=shots, decType=E2E["decType"],
                                 decIterations=E2E["decIterations"], decSchedule=E2E["decSchedule"], rngSeed=1,
                                 verbose=False, logical=True, channel_weights=weights)
        return shots / (time.perf_counter() - t0), r
    finally:
        decoders.decode_batch = real


def end_to_end(args):
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code(E2E["code"])
    shots = max(1, int(E2E["shots"] * args.scale))
    w_in = inhomogeneous_weights(Hx.shape[1])
    modes = {"depolarizing": (None, False), "bias0.5": (simulator.bias_weights(0.5), False),
             "bias10": (simulator.bias_weights(10), False), "inhomogeneous": (w_in, False),
             "inhomogeneous_mean": (w_in, True)}
    for w, mp in modes.values():                             # warm-up: plans, tables, logical operators
        _rate(simulator, Hx, Hz, max(1, shots // 8), w, mp)
    runs, last = {m: [] for m in modes}, {}
    for _ in range(2):
        for m, (w, mp) in modes.items():
            rate, last[m] = _rate(simulator, Hx, Hz, shots, w, mp)
            runs[m].append(round(rate))
    out = dict(E2E, shots=shots)
    for m in modes:
        out[m] = dict(shots_per_s=runs[m], logical_error_rate=last[m]["logical_error_rate"],
                      ci95=last[m]["logical_error_rate_ci95"],
                      failures=last[m]["DecFailures_X"] + last[m]["DecFailures_Z"])
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
        vec = np.full(Hz.shape[1], p)
        kw = dict(algo="MS", layer_ptr=lp, layer_rows=lr, ehat_bits=True)
        outs = {}

        def run(side):
            # the library's own launch timing (HIP events around the kernel
            # alone: switching options rebuilds the launch plan on the host)
            _lib.timing_reset()
            if side == "vprior":
                r = decoders.decode_batch(Hz, syn, None, 50, prior=vec, out=outs.get(side), **kw)
            elif side == "prior":
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
        sides = ("vprior", "prior", "generic", "default")
        for s in sides:
            run(s)
        ms = {s: [] for s in sides}
        for _ in range(args.reps):
            for s in sides:
                ms[s].append(run(s))
        same = all(torch.equal(outs["vprior"].ehat, outs[s].ehat) and torch.equal(outs["vprior"].iters, outs[s].iters)
                   for s in sides)
        with _lib.options(**GENERIC):
            generic_name = _lib.kernel_name(Hz, lp, lr, "MS", 0)
        out = dict(w, batch=B, kernels=dict(vprior=_lib.vprior_kernel_name(Hz, lp, lr, "MS", 0),
                                            prior=_lib.prior_kernel_name(Hz, lp, lr, "MS", 0), generic=generic_name,
                                            default=_lib.kernel_name(Hz, lp, lr, "MS", 0)),
                   ms=ms, spread={s: round(max(ms[s]) / min(ms[s]) - 1, 4) for s in sides},
                   vprior_over_prior=round(min(ms["vprior"]) / min(ms["prior"]), 4),
                   vprior_over_generic=round(min(ms["vprior"]) / min(ms["generic"]), 4),
                   generic_over_default=round(min(ms["generic"]) / min(ms["default"]), 4), same_results=same,
                   mean_iterations=float(outs["vprior"].iters.double().mean()))
        print(json.dumps(out), flush=True)
    _lib.timing_enable(False)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--only", type=int, default=None, help="index of the one kernel-side workload to run")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the end-to-end workload's shots")
    ap.add_argument("--batch", type=int, default=1 << 18, help="half-shots of the kernel-side batch")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    return kernels(args) if args.kernels else end_to_end(args)


if __name__ == "__main__":
    main()

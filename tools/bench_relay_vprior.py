"""Cost and gain of relay min-sum with per-variable priors
(relay_vprior_kernel, simulate_p / simulate_dem with relay_priors=True;
DESIGN.md §3.18) on one GPU.

Kernel side (--kernels): one batch of 2^20 LP118_0 Hz half-shots, channel
syndromes at p = 0.05, the simulator's default legs (T = [50] + [60] * 10,
relay_gammas), S = 1, decoded by
    vector   relay_vprior_kernel<8>, a uniform row, cost "hamming" (the same
             arithmetic and results as the scalar relay)
    scalar   relay_ms_kernel<8>
alternating in one process (the library's HIP events around each launch, after
a warm-up of both). One JSON line: ms per launch of every repeat, each side's
spread (max / min - 1), vector / scalar of the best ones, and both kernels'
launch geometry (waves per workgroup, workgroups per CU, LDS bytes).

End to end (default): simulate_p shots/s and logical error rate, logical=True,
LP118_0, p = 0.05, a quarter of the qubits five times as noisy as the rest
(bench_vprior.py's inhomogeneous channel), 50 iterations (RELAY: the first
leg; --sols solutions, 3 by default, so that the cost has a choice: with the
simulator's default of 1 both costs return the first solution), 2^23 shots,
interleaved, twice each after a warm-up of all:
    ms_vector        decType MS, decode_batch(prior=marginals)
    relay_mean       RELAY, the same channel decoded with each half's mean
                     marginal as its scalar prior
    relay_hamming    RELAY, relay_priors=True, relay_cost="hamming"
    relay_prior      RELAY, relay_priors=True, relay_cost="prior"

Detector error model (--dem): simulate_dem on the X-half phenomenological
model of LP04_0 (3 rounds, p = 0.03, q = 0.01: 252 detectors, 693 mechanisms,
rows of at most 9 entries), 30 iterations (RELAY: the first leg), MS against
RELAY with relay_priors=True under both costs (--sols solutions), 2^21 shots,
shots/s and logical error rate.

    python tools/bench_relay_vprior.py [--kernels | --dem] [--scale S] [--sols N] [--batch B] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from bench_vprior import inhomogeneous_weights  # noqa: E402

E2E = dict(code="LP118_0", decIterations=50, p=0.05, shots=1 << 23)
DEM = dict(code="LP04_0", rounds=3, p=0.03, q=0.01, decIterations=30, shots=1 << 21)
MODES = {"ms_vector": dict(decType="MS"),
         "relay_mean": dict(decType="RELAY", relay_priors=True, relay_cost="hamming"),
         "relay_hamming": dict(decType="RELAY", relay_priors=True, relay_cost="hamming"),
         "relay_prior": dict(decType="RELAY", relay_priors=True, relay_cost="prior")}


def _rate(simulator, Hx, Hz, shots, weights, mode, sols):
    import numpy as np
    import torch
    from qldpcsim_amd import decoders
    real = decoders.decode_batch
    if mode == "relay_mean":
        # the vector channel, decoded with the mean of the half's marginals
        def scalar(H, syn, p, *a, relay=None, **kw):
            cfg = decoders.RelayConfig(relay.leg_iters, relay.gammas, relay.sols)
            return real(H, syn, float(np.mean(relay.prior)), *a, relay=cfg, **kw)
        decoders.decode_batch = scalar
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = simulator.simulate_p(Hx, Hz, E2E["p"], shots=shots, decIterations=E2E["decIterations"], rngSeed=1,
                                 verbose=False, logical=True, channel_weights=weights, **MODES[mode],
                                 **({} if mode == "ms_vector" else {"relay_sols": sols}))
        return shots / (time.perf_counter() - t0), r
    finally:
        decoders.decode_batch = real


def end_to_end(args):
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code(E2E["code"])
    shots = max(1, int(E2E["shots"] * args.scale))
    w = inhomogeneous_weights(Hx.shape[1])
    for m in MODES:                                          # warm-up: plans, tables, logical operators
        _rate(simulator, Hx, Hz, max(1, shots // 8), w, m, args.sols)
    runs, last = {m: [] for m in MODES}, {}
    for _ in range(2):
        for m in MODES:
            rate, last[m] = _rate(simulator, Hx, Hz, shots, w, m, args.sols)
            runs[m].append(round(rate))
    out = dict(E2E, shots=shots, relay_sols=args.sols)
    for m in MODES:
        out[m] = dict(shots_per_s=runs[m], logical_error_rate=last[m]["logical_error_rate"],
                      ci95=last[m]["logical_error_rate_ci95"],
                      failures=last[m]["DecFailures_X"] + last[m]["DecFailures_Z"],
                      avg_iterations_XZ=[last[m]["Avg_number_of_iterations_X"], last[m]["Avg_number_of_iterations_Z"]])
    print(json.dumps(out), flush=True)


def dem_run(args):
    import torch
    from qldpcsim_amd import codes, dem, logicals, simulator
    Hx, Hz = codes.load_code(DEM["code"])
    model = dem.phenomenological_dem(Hz, logicals.css_logicals(Hx, Hz)[1], DEM["rounds"], 2 * DEM["p"] / 3, DEM["q"])
    shots = max(1, int(DEM["shots"] * args.scale))
    modes = {"ms": dict(decType="MS"),
             "relay_hamming": dict(decType="RELAY", relay_priors=True, relay_cost="hamming"),
             "relay_prior": dict(decType="RELAY", relay_priors=True, relay_cost="prior")}

    def rate(m, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = simulator.simulate_dem(model, shots=n, decIterations=DEM["decIterations"], rngSeed=1, verbose=False,
                                   sampler="device", **modes[m], **({} if m == "ms" else {"relay_sols": args.sols}))
        return n / (time.perf_counter() - t0), r
    for m in modes:
        rate(m, max(1, shots // 8))
    runs, last = {m: [] for m in modes}, {}
    for _ in range(2):
        for m in modes:
            x, last[m] = rate(m, shots)
            runs[m].append(round(x))
    out = dict(DEM, shots=shots, relay_sols=args.sols, detectors=model.num_detectors, errors=model.num_errors,
               max_row=int(model.H.sum(1).max()))
    for m in modes:
        out[m] = dict(shots_per_s=runs[m], logical_error_rate=last[m]["logical_error_rate"],
                      ci95=last[m]["logical_error_rate_ci95"], failures=last[m]["DecFailures"],
                      avg_iterations=last[m]["nIterAcc"] / shots)
    print(json.dumps(out), flush=True)


def kernels(args):
    import numpy as np
    import torch
    from qldpcsim_amd import _lib, codes, decoders, simulator
    dev = torch.device("cuda", 0)
    B = args.batch
    Hx, Hz = codes.load_code("LP118_0")
    n = Hz.shape[1]
    p = 0.05
    syn = simulator.DeviceChannel(Hx, Hz, dev, 20251226).sample(p, B, bits=True)[0]
    T = [50] + [60] * 10
    G = decoders.relay_gammas(n, len(T))
    cfg = {"scalar": decoders.RelayConfig(T, G, 1),
           "vector": decoders.RelayConfig(T, G, 1, prior=np.full(n, p / 3), cost="hamming")}
    outs = {}

    def run(side):
        # the library's own launch timing (HIP events around the kernel alone)
        _lib.timing_reset()
        r = decoders.decode_batch(Hz, syn, p / 3 if side == "scalar" else None, 0, algo="RELAY", relay=cfg[side],
                                  ehat_bits=True, out=outs.get(side))
        torch.cuda.synchronize()
        outs[side] = r
        return round(_lib.timing_read()[0], 4)
    _lib.timing_enable(True)
    sides = ("vector", "scalar")
    for s in sides:
        run(s)
    ms = {s: [] for s in sides}
    for _ in range(args.reps):
        for s in sides:
            ms[s].append(run(s))
    _lib.timing_enable(False)
    a, b = outs["vector"], outs["scalar"]
    same = all(torch.equal(getattr(a, k), getattr(b, k)) for k in ("ehat", "iters", "flags", "info"))
    code = _lib.code_for(Hz, 0)
    rl = {"scalar": code.relay(T, G, 1), "vector": code.relay(T, G, 1, prior=cfg["vector"].prior)}
    out = dict(code="LP118_0", syndromes="channel", p=p, leg_iters=T, batch=B,
               kernels={s: rl[s].kernel_name() for s in sides},
               waves_wgs_lds={s: rl[s].launch_info() for s in sides}, layout={s: rl[s].layout() for s in sides},
               ms=ms, spread={s: round(max(ms[s]) / min(ms[s]) - 1, 4) for s in sides},
               vector_over_scalar=round(min(ms["vector"]) / min(ms["scalar"]), 4), same_results=same,
               mean_iterations=float(a.iters.double().mean()),
               solved=float((a.found > 0).double().mean()))
    print(json.dumps(out), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--dem", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the end-to-end / --dem workload's shots")
    ap.add_argument("--sols", type=int, default=3, help="relay_sols of every RELAY run (end to end, --dem)")
    ap.add_argument("--batch", type=int, default=1 << 20, help="half-shots of the kernel-side batch")
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args(argv)
    return kernels(args) if args.kernels else dem_run(args) if args.dem else end_to_end(args)


if __name__ == "__main__":
    main()

"""Cost of per-variable priors on the HBM-resident kernel
(hbm_tile_vprior_kernel, library option vprior_hbm) on one GPU, and what the
option makes decodable.

Kernel side (--kernels): one batch of 2^18 fixed-work half-shots (uniform
random syndromes) of LP118_0, decoded by
    vprior_hbm  hbm_tile_vprior_kernel, a uniform vector (options vprior_hbm,
                force_hbm): the same arithmetic and results as the scalar decode
    scalar_hbm  hbm_tile_kernel, the scalar prior (option force_hbm): its twin
    vprior_lds  decode_vprior_kernel, the same vector (no option)
alternating in one process (the library's HIP events around each launch, after
a warm-up of all three; an option change only rebuilds the launch plan on the
host), for MS flooding 50 iterations and BP flooding 12. One JSON line per
workload: ms per launch of every repeat, each side's spread (max / min - 1),
and vprior_hbm / scalar_hbm, vprior_hbm / vprior_lds of the best.
(hbm_tile_kernel against another build of the library: tools/ab_libs.py with
--cfg "--path hbm".)

End to end (default): shots/s and logical error rate of
    phenom T=5, T=8      LP118_0, p_data != q, MS flooding 30 iterations, the
                         whole space-time matrix (hbm_priors=True; refused
                         without it), and at T = 8 the sliding window
                         (W, F) = (4, 1) on the LDS twin beside it
    dem                  a random detector error model, 600 detectors x 6000
                         mechanisms of weight 3 (detector rows of ~30 entries,
                         the longest past 32), 8 observables, MS flooding 30
                         iterations, hbm_priors=True (refused without it)
one JSON line each.

    python tools/bench_vprior_hbm.py [--kernels] [--scale S] [--batch B] [--reps R]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

KERNEL_WORKLOADS = (dict(code="LP118_0", algo="MS", iters=50, p=0.05), dict(code="LP118_0", algo="BP", iters=12, p=0.05))
PHENOM = dict(code="LP118_0", p=0.01, q=0.02, decType="MS", decIterations=30, shots=1 << 16)
DEM = dict(detectors=600, errors=6000, weight=3, observables=8, decType="MS", decIterations=30, shots=1 << 17)


def kernels(args):
    import numpy as np
    import torch
    from qldpcsim_amd import _lib, codes, decoders, simulator
    dev = torch.device("cuda", 0)
    B = args.batch
    sides = {"vprior_hbm": dict(vprior_hbm=1, force_hbm=1), "scalar_hbm": dict(force_hbm=1), "vprior_lds": {}}
    _lib.timing_enable(True)
    for w in KERNEL_WORKLOADS:
        Hz = codes.load_code(w["code"])[1]
        lp, lr = simulator.pack_layers(None, Hz.shape[0])
        g = torch.Generator(device=dev).manual_seed(20251226)
        syn = decoders.pack_bits(torch.randint(0, 2, (B, Hz.shape[0]), dtype=torch.uint8, device=dev, generator=g))
        p = w["p"] / 3
        vec = np.full(Hz.shape[1], p)
        kw = dict(algo=w["algo"], layer_ptr=lp, layer_rows=lr, ehat_bits=True)
        outs, names = {}, {}

        def run(side):
            with _lib.options(**sides[side]):
                _lib.timing_reset()
                if side == "scalar_hbm":
                    r = decoders.decode_batch(Hz, syn, p, w["iters"], out=outs.get(side), **kw)
                    names[side] = _lib.kernel_name(Hz, lp, lr, w["algo"], 0)
                else:
                    r = decoders.decode_batch(Hz, syn, None, w["iters"], prior=vec, out=outs.get(side), **kw)
                    names[side] = _lib.vprior_kernel_name(Hz, lp, lr, w["algo"], 0)
                torch.cuda.synchronize()
                outs[side] = r
                return round(_lib.timing_read()[0], 4)
        for s in sides:
            run(s)
        ms = {s: [] for s in sides}
        for _ in range(args.reps):
            for s in sides:
                ms[s].append(run(s))
        same = all(torch.equal(outs["vprior_hbm"].ehat, outs[s].ehat) and
                   torch.equal(outs["vprior_hbm"].iters, outs[s].iters) for s in sides)
        print(json.dumps(dict(w, batch=B, kernels=names, ms=ms,
                              spread={s: round(max(ms[s]) / min(ms[s]) - 1, 4) for s in sides},
                              vprior_hbm_over_scalar_hbm=round(min(ms["vprior_hbm"]) / min(ms["scalar_hbm"]), 4),
                              vprior_hbm_over_vprior_lds=round(min(ms["vprior_hbm"]) / min(ms["vprior_lds"]), 4),
                              same_results=same, mean_iterations=float(outs["vprior_hbm"].iters.double().mean()))),
              flush=True)
    _lib.timing_enable(False)


def random_dem():
    """DEM's model: every mechanism flips `weight` random detectors and each
    observable with probability 1/4; priors log-uniform in [1e-4, 5e-3]."""
    import numpy as np
    from qldpcsim_amd import dem as D
    rng = np.random.default_rng(7)
    M, N = DEM["detectors"], DEM["errors"]
    H = np.zeros((M, N), np.uint8)
    for j in range(N):
        H[rng.choice(M, DEM["weight"], replace=False), j] = 1
    L = (rng.random((DEM["observables"], N)) < 0.25).astype(np.uint8)
    return D.Dem(H, L, 10.0 ** rng.uniform(-4, np.log10(5e-3), N))


def _timed(fn, warm):
    import torch
    warm()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def end_to_end(args):
    from qldpcsim_amd import codes, simulator
    Hx, Hz = codes.load_code(PHENOM["code"])
    shots = max(64, int(PHENOM["shots"] * args.scale))
    kw = dict(decType=PHENOM["decType"], decIterations=PHENOM["decIterations"], rngSeed=1, verbose=False,
              sampler="device")
    runs = [(5, dict(hbm_priors=True)), (8, dict(hbm_priors=True)), (8, dict(window=4, commit=1))]
    for T, extra in runs:
        refused = None
        if "hbm_priors" in extra:
            try:
                simulator.simulate_phenomenological(Hx, Hz, PHENOM["p"], PHENOM["q"], T, shots=64, **kw)
            except NotImplementedError as ex:
                refused = str(ex)
        call = lambda n: simulator.simulate_phenomenological(Hx, Hz, PHENOM["p"], PHENOM["q"], T, shots=n,  # noqa: E731
                                                             **kw, **extra)
        dt, r = _timed(lambda: call(shots), lambda: call(max(64, shots // 8)))
        print(json.dumps(dict(PHENOM, mode="phenom", rounds=T, shots=shots, **extra, refused_without=refused,
                              shots_per_s=round(shots / dt, 1), logical_error_rate=r["logical_error_rate"],
                              ci95=r["logical_error_rate_ci95"],
                              failures=r["DecFailures_X"] + r["DecFailures_Z"],
                              mean_iterations=(r["nIterAccX"] + r["nIterAccZ"]) / (2.0 * shots))), flush=True)
    model = random_dem()
    shots = max(64, int(DEM["shots"] * args.scale))
    kw = dict(decType=DEM["decType"], decIterations=DEM["decIterations"], rngSeed=1, verbose=False, sampler="device")
    refused = None
    try:
        simulator.simulate_dem(model, shots=64, **kw)
    except NotImplementedError as ex:
        refused = str(ex)
    call = lambda n: simulator.simulate_dem(model, shots=n, hbm_priors=True, **kw)  # noqa: E731
    dt, r = _timed(lambda: call(shots), lambda: call(max(64, shots // 8)))
    print(json.dumps(dict(DEM, mode="dem", shots=shots, max_row_degree=int(model.H.sum(axis=1).max()),
                          refused_without=refused, shots_per_s=round(shots / dt, 1),
                          logical_error_rate=r["logical_error_rate"], ci95=r["logical_error_rate_ci95"],
                          failures=r["DecFailures"], mean_iterations=r["nIterAcc"] / float(shots))), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the end-to-end workloads' shots")
    ap.add_argument("--batch", type=int, default=1 << 18, help="half-shots of the kernel-side batch")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args(argv)
    return kernels(args) if args.kernels else end_to_end(args)


if __name__ == "__main__":
    main()

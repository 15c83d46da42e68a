"""Cost and gain of OSD-CS (osd_block_cs_kernel, osd_method="cs") and of its
prior-weighted cost (osd_block_cs_prior_kernel, osd_cost="prior") on one GPU
(DESIGN.md §3.15, §3.19).

OSD call (--call, one process per library build): the non-converged shots of
one configs[3] batch (LP118_2 Hz, MS layered, 50 iterations, p = 0.1, device
sampler), then qldpc_osd_device_ordered (device order + elimination) timed
with HIP events over repeats after a warm-up: order 0, and with a library
that has them the OSD-CS calls at lambda = 0 / 10 / 60 on the same shots,
interleaved. One JSON line: ms per call of every repeat, the CS results'
mean weight saved against order 0. With --cost prior the weighted calls
(qldpc_osd_device_ordered_cs_prior, "csw<lambda>") run on the same shots and
lambdas beside them, priced with a fixed non-uniform row (the decode's p / 3,
five times that on every fourth column), and the line gains each weighted
median over its Hamming-CS median.

Order-0 regression (--regress PARENT.so): --call as fresh processes (QLDPC_LIB
selects the build) in the order parent, this, parent, this, ...; the parent is
the library tools/build_variants.sh builds from the parent commit (`name
HEAD` before the change is committed). One JSON line: every process's median
order-0 ms, the parent-versus-parent spread (max - min of its medians) and
this build's slowdown against the parent's best; the same for every Hamming-CS
call both libraries have (medians, spreads and whether this build's medians lie
inside the parent's range widened by its spread).

Logical error rate (default): simulate_p(logical=True) shots/s, logical error
rate and its 95 % Wilson interval for OSD-0, CS-10, CS-60 and RELAY on
    LP118_2  MS layered, 50 iterations, p = 0.05 and p = 0.1
    LP118_0  MS flooding, 50 iterations, p = 0.05
one JSON line per workload and side, after a warm-up of that side.
With --cost prior instead: CS-hamming against CS-prior at lambda = 10 and 60 on
the two workloads quoted for per-variable priors,
    LP118_0  MS flooding, 50 iterations, p = 0.05, a quarter of the qubits
             five times as noisy (bench_vprior.py's inhomogeneous channel)
    LP04_0   the X half's 3-round detector error model (p = 0.03, q = 0.01:
             252 x 693), MS, 30 iterations
one JSON line per workload, side and lambda.

    python tools/bench_osd_cs.py [--call | --regress PARENT.so] [--cost prior] [--only N] [--scale S] [--batch B]
                                 [--reps R] [--rounds N]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WORKLOADS = (
    dict(code="LP118_2", decSchedule="L", decIterations=50, p=0.05, shots=1 << 18),
    dict(code="LP118_2", decSchedule="L", decIterations=50, p=0.1, shots=1 << 16),
    dict(code="LP118_0", decSchedule="F", decIterations=50, p=0.05, shots=1 << 21),
)
SIDES = (("osd0", dict(decType="MS", OSDorder=0)),
         ("cs10", dict(decType="MS", OSDorder=10, osd_method="cs")),
         ("cs60", dict(decType="MS", OSDorder=60, osd_method="cs")),
         ("relay", dict(decType="RELAY", OSDorder=-1, decSchedule="F")))


def call(args):
    import numpy as np
    import torch
    from qldpcsim_amd import _lib, codes, decoders, schedule, simulator
    Hx, Hz = codes.load_code("LP118_2")
    lx, _ = schedule.select_layers(Hx, Hz, "L")
    lp, lr = schedule.pack_layers(lx, Hz.shape[0])
    dev = torch.device("cuda", 0)
    p = 0.1
    sy_z = simulator.DeviceChannel(Hx, Hz, dev, 1).sample(p, args.batch)[0]
    r = decoders.decode_batch(Hz, sy_z, p / 3, 50, algo="MS", want_post=True, layer_ptr=lp, layer_rows=lr)
    bad = ((r.flags & _lib.FLAG_CONVERGED) == 0).nonzero().flatten()
    k, n = int(bad.numel()), Hz.shape[1]
    post, syn, e0 = (x.index_select(0, bad).contiguous() for x in (r.post, sy_z, r.ehat))
    h = _lib.code_for(Hz, 0)
    perm = torch.empty((k, n), dtype=torch.int32, device=dev)
    tie = torch.empty(k, dtype=torch.int32, device=dev)
    status = torch.empty(k, dtype=torch.int32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    sides = {"order0": (_lib.lib.qldpc_osd_device_ordered, 0, ())}
    if hasattr(_lib.lib, "qldpc_osd_device_ordered_cs"):
        for lam in (0, 10, 60):
            sides[f"cs{lam}"] = (_lib.lib.qldpc_osd_device_ordered_cs, lam, ())
    if args.cost == "prior":
        row = np.full(n, p / 3)
        row[::4] *= 5.0
        weights = h.prior(row, 1e-9)
        for lam in (0, 10, 60):
            sides[f"csw{lam}"] = (_lib.lib.qldpc_osd_device_ordered_cs_prior, lam, (weights.handle,))
    ms, weight = {s: [] for s in sides}, {}
    for rep in range(args.reps + 1):
        for s, (fn, order, extra) in sides.items():
            e = e0.clone()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            _lib.check(fn(h.handle, k, syn.data_ptr(), post.data_ptr(), order, *extra, e.data_ptr(),
                          status.data_ptr(), perm.data_ptr(), tie.data_ptr(), st))
            t1.record()
            torch.cuda.synchronize()
            if rep:
                ms[s].append(round(t0.elapsed_time(t1), 4))
            weight[s] = float(e.sum(dim=1, dtype=torch.float64).mean())
    med = {s: float(np.median(v)) for s, v in ms.items()}
    ratio = {f"csw{lam}_over_cs{lam}": round(med[f"csw{lam}"] / med[f"cs{lam}"], 4) for lam in (0, 10, 60)
             if f"csw{lam}" in med}
    print(json.dumps(dict(lib=os.path.basename(_lib.LIB_PATH), code="LP118_2", p=p, batch=args.batch, osd_shots=k,
                          status_hist=np.bincount(status.cpu().numpy(), minlength=4).tolist(), ms=ms,
                          median_ms=med, mean_weight=weight, **ratio)), flush=True)


def regress(args):
    from qldpcsim_amd import _lib
    libs = [("parent", os.path.abspath(args.regress)), ("this", _lib.LIB_PATH)]
    med = {name: [] for name, _ in libs}
    med_cs = {name: {} for name, _ in libs}       # Hamming-CS side -> every process's median
    cs = None
    for _ in range(args.rounds):
        for name, path in libs:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--call", "--batch", str(args.batch),
                                  "--reps", str(args.reps)] + (["--cost", "prior"] if args.cost == "prior" and
                                                                name == "this" else []), env=dict(os.environ, QLDPC_LIB=path),
                                 capture_output=True, text=True, timeout=600)
            line = [x for x in out.stdout.splitlines() if x.startswith("{")]
            if out.returncode or not line:
                print(out.stderr[-3000:], flush=True)
                raise SystemExit(1)
            d = json.loads(line[-1])
            med[name].append(d["median_ms"]["order0"])
            for side, v in d["median_ms"].items():
                if side.startswith("cs") and not side.startswith("csw"):
                    med_cs[name].setdefault(side, []).append(v)
            if name == "this":
                cs = d
    spread = max(med["parent"]) - min(med["parent"])
    cs_sides = {}
    for side, pv in med_cs["parent"].items():
        tv = med_cs["this"].get(side)
        if tv:
            sp = max(pv) - min(pv)
            cs_sides[side] = dict(parent=pv, this=tv, parent_spread_ms=round(sp, 4), this_spread_ms=round(max(tv) - min(tv), 4),
                                  this_minus_parent_best_ms=round(min(tv) - min(pv), 4),
                                  within_spread=min(tv) - min(pv) <= sp)
    print(json.dumps(dict(order0_median_ms=med, osd_shots=cs["osd_shots"], parent_spread_ms=round(spread, 4),
                          this_spread_ms=round(max(med["this"]) - min(med["this"]), 4), hamming_cs=cs_sides,
                          this_minus_parent_best_ms=round(min(med["this"]) - min(med["parent"]), 4),
                          within_spread=min(med["this"]) - min(med["parent"]) <= spread,
                          cs_median_ms=cs["median_ms"], mean_weight=cs["mean_weight"])), flush=True)


def logical(args):
    import torch
    from qldpcsim_amd import codes, simulator
    for i, w in enumerate(WORKLOADS):
        if args.only is not None and i != args.only:
            continue
        Hx, Hz = codes.load_code(w["code"])
        shots = max(1, int(w["shots"] * args.scale))
        for name, side in SIDES:
            kw = dict(decSchedule=w["decSchedule"], decIterations=w["decIterations"], rngSeed=1, verbose=False,
                      logical=True)
            kw.update(side)
            simulator.simulate_p(Hx, Hz, w["p"], shots=max(1, shots // 8), **kw)     # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = simulator.simulate_p(Hx, Hz, w["p"], shots=shots, **kw)
            dt = time.perf_counter() - t0
            print(json.dumps(dict(code=w["code"], p=w["p"], side=name, shots=shots, shots_per_s=round(shots / dt),
                                  failures_XZ=[r["DecFailures_X"], r["DecFailures_Z"]],
                                  logical_error_rate=r["logical_error_rate"], ci95=r["logical_error_rate_ci95"])),
                  flush=True)


def logical_prior(args):
    """CS-hamming against CS-prior, lambda = 10 and 60, on the two per-variable-prior workloads."""
    import torch
    from bench_vprior import inhomogeneous_weights
    from qldpcsim_amd import codes, dem, logicals, simulator
    costs = (("cs_hamming", {}), ("cs_prior", dict(osd_cost="prior")))

    def report(name, shots, lam, side, dt, r, failures):
        print(json.dumps(dict(workload=name, side=side, osd_lambda=lam, shots=shots, shots_per_s=round(shots / dt),
                              failures=failures, logical_error_rate=r["logical_error_rate"],
                              ci95=r["logical_error_rate_ci95"])), flush=True)

    if args.only in (None, 0):
        Hx, Hz = codes.load_code("LP118_0")
        shots = max(1, int((1 << 21) * args.scale))
        w = inhomogeneous_weights(Hx.shape[1])
        for lam in (10, 60):
            for side, kw in costs:
                run = lambda n: simulator.simulate_p(Hx, Hz, 0.05, shots=n, decType="MS", decIterations=50,   # noqa: E731
                                                     decSchedule="F", OSDorder=lam, osd_method="cs", rngSeed=1,
                                                     verbose=False, logical=True, channel_weights=w, **kw)
                run(max(1, shots // 8))                                                  # warm-up
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = run(shots)
                report("LP118_0 p=0.05 inhomogeneous", shots, lam, side, time.perf_counter() - t0, r,
                       [r["DecFailures_X"], r["DecFailures_Z"]])
    if args.only in (None, 1):
        Hx, Hz = codes.load_code("LP04_0")
        model = dem.phenomenological_dem(Hz, logicals.css_logicals(Hx, Hz)[1], 3, 2 * 0.03 / 3, 0.01)
        shots = max(1, int((1 << 21) * args.scale))
        for lam in (10, 60):
            for side, kw in costs:
                run = lambda n: simulator.simulate_dem(model, shots=n, decType="MS", decIterations=30, OSDorder=lam,   # noqa: E731
                                                       osd_method="cs", rngSeed=1, verbose=False, sampler="device", **kw)
                run(max(1, shots // 8))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = run(shots)
                report(f"LP04_0 3-round DEM {model.num_detectors} x {model.num_errors}", shots, lam, side,
                       time.perf_counter() - t0, r, r["DecFailures"])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--call", action="store_true")
    ap.add_argument("--regress", default=None, help="the parent commit's library (tools/build_variants.sh)")
    ap.add_argument("--rounds", type=int, default=3, help="--regress: processes per library")
    ap.add_argument("--only", type=int, default=None, help="index of the one logical-error-rate workload to run")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies every workload's shots")
    ap.add_argument("--batch", type=int, default=1 << 15, help="shots of the --call batch")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cost", choices=["hamming", "prior"], default="hamming",
                    help="prior: --call / --regress time the weighted calls too; alone, the CS-hamming against "
                         "CS-prior logical-error-rate legs")
    args = ap.parse_args(argv)
    return (call(args) if args.call else regress(args) if args.regress else
            logical_prior(args) if args.cost == "prior" else logical(args))


if __name__ == "__main__":
    main()

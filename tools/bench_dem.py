#!/usr/bin/env python3
"""Measure the detector error model mode on the GPU.

For the phenomenological model of each (code, rounds) with p_data = q (the
scalar decode entry point), MS flooding, on the X half:
  - dem_sample_kernel's, dem_count_kernel's and the decode's ms per 2^18
    shots (medians of three launches between HIP events, bit-packed formats
    as the simulator uses them) and the sampler's and the counter's share of
    that batch's sample + decode + count;
  - the ratio to phenom_sample_kernel / phenom_count_kernel on the same
    shape, key and shots (the same stream; those kernels walk H's own CSR and
    have two thresholds, these read a threshold per column and the
    materialised matrix column by column);
  - where N <= 4096, the ratio to the generic sampler
    (qldpc_channel_sample_vec) on the materialised matrix, which writes 2N
    error bits per shot where this one writes M + K;
  - the mean number of fired columns per shot, which is what the sampler's
    walk scales with.

    python tools/bench_dem.py [--codes LP04_0 LP118_0] [--rounds 1 3 5] [--p 0.015]

Prints one JSON line per measurement.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.abspath(os.path.join(os.path.dirname(__file__), "..")))

import numpy as np  # noqa: E402

from bench_phenom import _ms  # noqa: E402


def measure(name, T, p, iters):
    import torch
    from qldpcsim_amd import _lib, codes, decoders, dem as D, logicals, simulator
    Hx, Hz = codes.load_code(name)
    Lz = logicals.css_logicals(Hx, Hz)[1]
    p_data = q = 2 * p / 3
    dev = torch.device("cuda", 0)
    B = 1 << 18
    model = D.phenomenological_dem(Hz, Lz, T, p_data, q)
    src = simulator.DeviceDem(model, dev, 1)
    half = simulator.DevicePhenomHalf(Hz, Lz, T, dev, 1)
    S = model.H
    lp, lr = decoders.pack_layers(None, S.shape[0])
    det, obs = src.sample(B, bits=True)
    r = decoders.decode_batch(S, det, p_data, iters, algo="MS", layer_ptr=lp, layer_rows=lr, ehat_bits=True)
    acc = torch.zeros(4, dtype=torch.int64, device=dev)
    t_s = _ms(lambda: src.sample(B, bits=True))
    t_d = _ms(lambda: decoders.decode_batch(S, det, p_data, iters, algo="MS", layer_ptr=lp, layer_rows=lr,
                                            ehat_bits=True, out=r))
    t_c = _ms(lambda: src.count_device(det, obs, r.ehat, r.iters, acc))
    pdet, E = half.sample(p_data, q, B, bits=True)
    p_s = _ms(lambda: half.sample(p_data, q, B, bits=True))
    p_c = _ms(lambda: half.count_device(pdet, E, r.ehat, r.iters, acc))
    fired = src.sample(4096, want_fired=True)[2]
    weight = float(np.unpackbits(fired.cpu().numpy().view(np.uint8), axis=1).sum(axis=1).mean())
    row = {"code": name, "rounds": T, "M": src.M, "K": src.K, "N": src.N, "p_data": p_data, "q": q, "iters": iters,
           "fired_per_shot": round(weight, 2), "decode_kernel": _lib.kernel_name(S, lp, lr, "MS", 0),
           "kernels": [_lib.dem_kernel_name(src.table, k) for k in ("sample", "count")],
           "sample_ms_per_2^18": round(t_s, 3), "count_ms_per_2^18": round(t_c, 3),
           "decode_ms_per_2^18": round(t_d, 3), "sample_share": round(t_s / (t_s + t_d + t_c), 4),
           "count_share": round(t_c / (t_s + t_d + t_c), 4),
           "phenom_sample_ms_per_2^18": round(p_s, 3), "phenom_count_ms_per_2^18": round(p_c, 3),
           "sample_vs_phenom": round(t_s / p_s, 3), "count_vs_phenom": round(t_c / p_c, 3)}
    if src.N <= 4096:
        ch = simulator.DeviceChannel(S, S, dev, 1)
        ch.set_probs(np.stack([model.priors, np.zeros_like(model.priors), np.zeros_like(model.priors)]))
        g = _ms(lambda: ch.sample(0.0, B, bits=True))
        row.update({"generic_sample_ms_per_2^18": round(g, 3), "sample_vs_generic": round(t_s / g, 3)})
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--codes", nargs="+", default=["LP04_0", "LP118_0"])
    ap.add_argument("--rounds", type=int, nargs="+", default=[1, 3, 5])
    ap.add_argument("--p", type=float, default=0.015, help="depolarizing strength (p_data = q = 2p/3 = 0.01)")
    ap.add_argument("--iters", type=int, default=50)
    a = ap.parse_args(argv)
    for name in a.codes:
        for T in a.rounds:
            print(json.dumps(measure(name, T, a.p, a.iters)), flush=True)


if __name__ == "__main__":
    main()

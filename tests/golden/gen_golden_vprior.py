"""Writes tests/golden/vprior/vprior_LP04_0.npz: 48 half-shots of LP04_0's Hz decoded
by tests/prior_model.py (min-sum, flooding, 20 iterations) with one prior per
variable, the expectation __graft_entry__.smoke() holds decode_vprior_kernel
to. Run from the repository root: python tests/golden/gen_golden_vprior.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import prior_model as pm  # noqa: E402
from qldpcsim_amd import codes  # noqa: E402

H = np.ascontiguousarray(codes.load_code("LP04_0")[1])
n = H.shape[1]
rng = np.random.default_rng(20261019)
q = 10.0 ** rng.uniform(-4, np.log10(0.3), n)               # log-uniform in [1e-4, 0.3]
q[5], q[90] = 0.7, 0.0                                      # a negative LLR, a zero probability
B, max_iter = 48, 20
e = (rng.random((B - 8, n)) < q).astype(np.int64)
syn = np.concatenate([(e @ H.T.astype(np.int64)) % 2, rng.integers(0, 2, (8, H.shape[0]))]).astype(np.uint8)
L = np.array([pm.llr(x) for x in q])
ehat, iters, post, flags = pm.decode("MS", H, syn, np.broadcast_to(L, (B, n)), max_iter)
np.savez_compressed(os.path.join(HERE, "vprior", "vprior_LP04_0.npz"), q=q, syn=syn, ehat=ehat, iters=iters, post=post,
                    flags=flags, max_iter=np.int32(max_iter))
print(f"{B} half-shots, {(flags & 1).sum()} converged, iterations {iters.min()}..{iters.max()}")

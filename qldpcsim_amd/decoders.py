"""Drop-in decoders: the reference's decoders.py surface on the MI355X kernels.

    MS_decoder(H, syndrome, p, max_iter=99, layers=None, beta=0.75, OSDorder=-1, eps=1e-9)
        reference qLDPCsim/decoders.py:110-182  -> (e_hat int8[n], n_iter)
    BP_decoder(H, syndrome, p, max_iter=99, layers=None, OSDorder=-1, eps=1e-9)
        reference qLDPCsim/decoders.py:189-290  -> (e_hat int64[n], n_iter)
    OSDdec(H, e_hat, syndrome, posteriorLLRs, order=0)
        reference qLDPCsim/decoders.py:299-370  -> e_hat (updated in place)
    NG_decoder(H, syndrome)
        reference qLDPCsim/decoders.py:27-66    -> (e_hat int8[n], steps)
    BF_decoder(H, syndrome, max_iter=50)
        reference qLDPCsim/decoders.py:74-102   -> (e_hat bool[n], n_iter)

plus the batched entry point the simulator uses, `decode_batch`, which decodes
many syndromes of one matrix in one kernel launch.

All decoding runs through the HIP kernels (libqldpc_hip.so via the C ABI);
there is no CPU fallback. OSD of the non-converged shots runs on the device
(osd_kernels.hip: NumPy's reliability order of decoders.py:320-325 — SVML's
exp and x86-simd-sort's argsort restated, ties included — and a block GF(2)
elimination); the rare shots the device order leaves to NumPy (a NaN
posterior, x86-simd-sort's std::sort fallback) get NumPy's own order on the
host and the device elimination again. `OSDdec` / `apply_osd` are the
single-shot and host entry points (host C++ elimination).

The restated order is NumPy 2.2.6's on x86-64 AVX512_SKX (the reference's
capture host). At first use, `numpy_order_pinned()` compares it with the running
NumPy on a fixed set of tie-heavy rows; if they differ (another NumPy build
or ISA dispatch), every OSD order is NumPy's own, computed on the host, and a
RuntimeWarning says why. `numpy_libm_pinned()` does the same for the tanh /
arctanh / log / exp restated for BP and the priors (BP is bit-exact only where
it holds; checked at the first BP decode); `parity_pins()` reports both.

Deviations from the reference (documented in DESIGN.md §7):
  * layers=None means flooding (the reference raises AttributeError on
    `np.range`, decoders.py:144 / :221).
  * H entries are reduced mod 2 (as load_matrix does, simulator.py:35);
    syndrome entries must be 0/1 (ValueError otherwise).
  * The min-sum "leak" case (a v2c message exactly 0.0, App. A.1.6) is
    flagged (FLAG_MIN_ZERO) but not emulated.
"""
import contextlib
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, hostcores
from .schedule import pack_layers

__all__ = ["MS_decoder", "BP_decoder", "NG_decoder", "BF_decoder", "OSDdec", "decode_batch", "DecodeResult",
           "Relay_decoder", "RelayConfig", "relay_gammas",
           "osd_perm", "pack_bits", "unpack_bits",
           "osd_perms", "apply_osd", "apply_osd_device", "apply_osd_device_many", "osd_device_stage",
           "osd_device_finish", "osd_host_orders", "osd_status_check", "osd_method_checked", "osd_cost_checked", "numpy_order_pinned",
           "numpy_libm_pinned", "parity_pins"]


@dataclass
class DecodeResult:
    ehat: object          # uint8 [B, n]   (numpy, or torch on the device path)
    iters: object         # int32 [B]
    post: object          # float64 [B, n] or None
    flags: object         # int32 [B]
    info: object = None   # algo "RELAY": int32 [B, 2] (solutions found, leg of the one returned or -1)
    osd_status: object = None   # after the device OSD: int32 per OSD shot, 1 = the reference's IndexError case
    osd_host_order: int = 0     # after the device OSD: shots whose reliability order the host computed

    @property
    def converged(self):
        return (self.flags & _lib.FLAG_CONVERGED) != 0

    @property
    def found(self):
        return None if self.info is None else self.info[:, 0]

    @property
    def best_leg(self):
        return None if self.info is None else self.info[:, 1]


@dataclass
class RelayConfig:
    """Settings of decode_batch(algo="RELAY"): iterations per leg, the memory
    strengths float64 [legs, n] in original column order (relay_gammas), and
    the number of solutions to stop at. `prior`: one error
    probability per column of H, float64 [n] in original column order, every
    0 <= q_j < 1, in place of decode_batch's scalar `p` (which must then be
    None). `cost`: which of the solutions found is kept, "hamming" (the fewest
    set bits) or "prior" (the smallest sum of the set bits' prior weights
    llrint(L_j 2^20); needs `prior`); ties keep the earlier one."""
    leg_iters: object
    gammas: object
    sols: int = 1
    prior: object = None
    cost: str = "hamming"


def relay_gammas(n, legs, gamma0=0.125, lo=-0.24, hi=0.66, seed=0):
    """Memory strengths float64 [legs, n] of a relay decoder: row 0 is gamma0
    for every variable, rows 1.. are np.random.default_rng(seed).uniform(lo, hi,
    (legs - 1, n)) (Relay-BP's disordered legs, some strengths negative)."""
    g = np.empty((int(legs), int(n)), np.float64)
    g[0] = gamma0
    g[1:] = np.random.default_rng(seed).uniform(lo, hi, (int(legs) - 1, int(n)))
    return g


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def pack_bits(bits):
    """uint8 [B, k] 0/1 tensor -> int64 [B, ceil(k/64)] words, bit j % 64 of
    word j / 64 (the bit-packed syndrome / estimate format, QLDPC_FMT_BITS)."""
    import torch
    B, k = bits.shape
    W = (k + 63) // 64
    x = torch.zeros((B, 64 * W), dtype=torch.int64, device=bits.device)
    x[:, :k] = bits.to(torch.int64) & 1
    sh = torch.arange(64, device=bits.device, dtype=torch.int64)
    return (x.view(B, W, 64) << sh).sum(dim=2)


def unpack_bits(words, k):
    """int64 [B, W] words -> uint8 [B, k] (inverse of pack_bits)."""
    import torch
    sh = torch.arange(64, device=words.device, dtype=torch.int64)
    return ((words.unsqueeze(-1) >> sh) & 1).to(torch.uint8).reshape(words.shape[0], -1)[:, :k]


def decode_batch(H, syndromes, p, max_iter, layers=None, algo="MS", beta=0.75, eps=1e-9,
                 want_post=False, osd_order=-1, layer_ptr=None, layer_rows=None, stream=None,
                 out=None, ehat_bits=False, prior_mask=None, p_masked=None, relay=None, prior=None, osd_method="ref",
                 osd_cost="hamming"):
    """Decode a batch of syndromes of one matrix on the GPU.

    syndromes: uint8 [B, m] NumPy array (host; staged, synchronous) or a
    torch tensor on a HIP device (asynchronous on `stream` or torch's current
    stream; outputs are device tensors, OSD is not applied): uint8 [B, m] one
    byte per check, or int64 [B, ceil(m/64)] bit-packed words (pack_bits).
    `ehat_bits` (device path): hard decisions as int64 [B, ceil(n/64)] words
    instead of uint8 [B, n].
    `p` is the decoder prior (simulate passes p/3, simulator.py:278-282).
    `out` (device path): a DecodeResult of matching device tensors to write
    into instead of allocating (steady-state loops allocate nothing).
    `algo`: "MS", "BP", or the hard-decision "NG" / "BF", which take only H,
    the syndromes and (BF) `max_iter`: p, layers, beta and eps are ignored,
    want_post / osd_order >= 0 raise ValueError, and the result's post is None.
    `prior_mask`, `p_masked` (MS / BP; both or neither): a two-level prior per
    shot. Variable j of shot b decodes with the prior of `p_masked` where
    prior_mask[b, j] is set and with the prior of `p` elsewhere (correlated
    X/Z decoding: the other half's estimate is the mask). Device path: a
    tensor on the syndromes' device, uint8 [B, n] or int64 words
    [B, ceil(n/64)] (an earlier decode's ehat as it is; not this call's out);
    host path: a uint8 [B, n] array. Runs decode_prior_kernel, the generic LDS
    kernel's twin: NotImplementedError for a code it cannot hold or with
    option force_hbm. With p_masked == p the result is the scalar decode's.
    `prior` (MS / BP): one prior probability per column of H, a float64
    array-like of n values in [0, 1) (the `channel_probs` of other BP
    packages), shared by every shot of the batch; `p` must then be None. Runs
    decode_vprior_kernel on both paths, with the limits of
    the prior_mask kernel; not combinable with prior_mask, relay= or NG / BF.
    A uniform vector gives the scalar decode's result bit for bit. There is
    no keyword for the HBM-resident variant: library option vprior_hbm is its
    switch (`with _lib.options(vprior_hbm=1): ...`, set once around a run, since
    every option change invalidates the cached launch plans). With it a code
    past those limits decodes with hbm_tile_vprior_kernel at
    any size and degree instead of raising, and with force_hbm=1 as well every
    prior= decode does; prior_mask stays refused there.
    `osd_method` (with osd_order >= 0): "ref" is the reference's OSDdec of that
    order (order 1 flips one bit, orders >= 2 equal order 0); "cs" is OSD-CS,
    the combination sweep with lambda = osd_order in 0..64:
    every single flip of an information position and every pair among the
    first lambda, lowest Hamming weight wins. MS / BP only: "cs" with
    osd_order < 0, with RELAY, NG or BF, or an unknown method raises ValueError.
    `osd_cost` (with osd_method="cs"): "hamming", or "prior" (DESIGN.md §3.19):
    the candidate of least prior weight wins, sum over its support of
    llrint(L_j 2^20) with L_j the prior LLR of column j, an exact int64. The
    row is this decode's `prior=`; "prior" without osd_method="cs" or without
    `prior=` raises ValueError. A uniform row with p < 1/2 gives the "hamming"
    result bit for bit.
    `algo="RELAY"` with `relay=RelayConfig(...)`: relay min-sum (DESIGN.md
    §3.11), flooding only. `max_iter` is ignored: the legs carry their own
    counts (relay.leg_iters). layers other than flooding, prior_mask and
    osd_order >= 0 raise ValueError (post is returned with want_post, so a
    caller can run OSDdec on the failures). The result's `info` (`found`,
    `best_leg`) says how many solutions each shot met and which leg's was kept.
    With `relay.prior` (one probability per column; `p` must be None) the
    blend takes each variable's own prior and relay_vprior_kernel runs
    (DESIGN.md §3.18); `relay.cost="prior"` keeps the solution of least prior
    weight instead of least Hamming weight. A uniform row with cost "hamming"
    gives the scalar relay's result bit for bit. The top-level `prior=` stays
    refused with RELAY.
    """
    osd_method_checked(osd_method, osd_order, algo)
    osd_cost_checked(osd_cost, osd_method, prior, "prior=")
    if prior is not None:
        if p is not None:
            raise ValueError("give either p (one scalar prior) or prior (one per column), not both")
        if prior_mask is not None or p_masked is not None:
            raise ValueError("prior (per-column) and prior_mask (two-level, per shot) cannot be combined")
        if relay is not None or algo == "RELAY":
            raise ValueError("relay min-sum takes no per-column prior")
        if algo in _lib.HARD_ALGOS:
            raise ValueError(f"{algo} is a hard-decision decoder: it takes no prior")
        prior = np.ascontiguousarray(prior, dtype=np.float64)
        if prior.shape != (np.asarray(H).shape[1],):
            raise ValueError(f"prior must hold {np.asarray(H).shape[1]} probabilities (one per column of H), got "
                             f"shape {prior.shape}")
    if algo == "RELAY":
        return _decode_batch_relay(H, syndromes, p, relay, layers, beta, eps, want_post, osd_order, layer_ptr,
                                   layer_rows, stream, out, ehat_bits, prior_mask, p_masked)
    if relay is not None:
        raise ValueError('relay= goes with algo="RELAY"')
    if algo not in _lib.ALGO:
        raise ValueError("Unrecognized decoder type.")
    if (prior_mask is None) != (p_masked is None):
        raise ValueError("prior_mask and p_masked go together: give both or neither")
    if algo in _lib.HARD_ALGOS:
        if prior_mask is not None:
            raise ValueError(f"{algo} is a hard-decision decoder: it takes no prior (prior_mask)")
        return _decode_batch_hard(H, syndromes, max_iter, algo, want_post, osd_order, stream, out, ehat_bits)
    if algo == "BP" and "libm" not in _PINNED:
        numpy_libm_pinned()                   # once: warns if BP cannot be bit-exact on this NumPy
    H = np.asarray(H)
    m, n = H.shape
    if layer_ptr is None:
        layer_ptr, layer_rows = pack_layers(layers, m)
    if int(max_iter) < 1:
        raise ValueError("max_iter must be >= 1")
    host = not _is_torch(syndromes)
    code, sched, res, ins, mask, outs, held = (_host_batch if host else _device_batch)(
        H, syndromes, _lib.Code.schedule, (layer_ptr, layer_rows), want_post, osd=osd_order >= 0,
        prior_mask=prior_mask, out=out, stream=stream, ehat_bits=ehat_bits)
    L = _lib.lib
    head = (code.handle, sched.handle, _lib.ALGO[algo])
    if prior is not None:
        _lib.check((L.qldpc_decode_host_vprior if host else L.qldpc_decode_device_vprior)(
            *head, *ins, code.prior(prior, eps).handle, int(max_iter), float(beta), *outs))
    elif prior_mask is not None:
        _lib.check((L.qldpc_decode_host_prior if host else L.qldpc_decode_device_prior)(
            *head, *ins, float(p), float(p_masked), *mask, int(max_iter), float(beta), float(eps), *outs))
    else:
        _lib.check((L.qldpc_decode_host if host else L.qldpc_decode_device_ex)(
            *head, *ins, float(p), int(max_iter), float(beta), float(eps), *outs))
    if host and osd_order >= 0:
        syn, post = held[:2]
        apply_osd(H, syn, res.ehat, post, res.flags, osd_order, **_method_kw("method", osd_method),
                  **_cost_kw(osd_cost, prior, eps))
    return res


def _decode_batch_relay(H, syndromes, p, relay, layers, beta, eps, want_post, osd_order, layer_ptr, layer_rows,
                        stream, out, ehat_bits, prior_mask, p_masked):
    """decode_batch for algo "RELAY" (relay_ms_kernel; with relay.prior
    relay_vprior_kernel)."""
    if not isinstance(relay, RelayConfig):
        raise ValueError('algo="RELAY" needs relay=RelayConfig(leg_iters, gammas, sols)')
    if relay.cost not in _lib.RELAY_COST:
        raise ValueError(f"relay.cost must be one of {tuple(_lib.RELAY_COST)}, got {relay.cost!r}")
    if relay.prior is None and relay.cost == "prior":
        raise ValueError('relay.cost="prior" weighs solutions by relay.prior: give the prior row')
    if relay.prior is not None and p is not None:
        raise ValueError("give either p (one scalar prior) or relay.prior (one per column), not both")
    if prior_mask is not None or p_masked is not None:
        raise ValueError("relay min-sum takes no two-level prior (prior_mask)")
    if osd_order >= 0:
        raise ValueError("relay min-sum has no OSD step (decode with want_post and run OSDdec on the failures)")
    H = np.asarray(H)
    if H.ndim != 2:
        raise ValueError("H must be a 2-D matrix")
    m, n = H.shape
    if layer_ptr is None:
        layer_ptr, layer_rows = pack_layers(layers, m)
    if not (len(layer_ptr) == 2 and np.array_equal(np.sort(np.asarray(layer_rows)), np.arange(m))):
        raise ValueError("relay min-sum runs the flooding schedule only (layers=None)")
    T = np.asarray(relay.leg_iters, np.int64).reshape(-1)
    G = np.asarray(relay.gammas, np.float64)
    if G.shape != (len(T), n):
        raise ValueError(f"relay.gammas must be float64 [{len(T)}, {n}] (one row per leg, one entry per variable)")
    host = not _is_torch(syndromes)
    make = _lib.Code.relay
    if relay.prior is not None:
        q = np.ascontiguousarray(relay.prior, dtype=np.float64)
        if q.shape != (n,):
            raise ValueError(f"relay.prior must hold {n} probabilities (one per column of H), got shape {q.shape}")

        def make(code, *made_from):
            return code.relay(*made_from, prior=q, eps=eps)
    code, rl, res, ins, _, outs, held = (_host_batch if host else _device_batch)(
        H, syndromes, make, (T, G, relay.sols), want_post, out=out, stream=stream, ehat_bits=ehat_bits,
        has_info=True)
    L = _lib.lib
    if relay.prior is not None:
        _lib.check((L.qldpc_decode_host_relay_vprior if host else L.qldpc_decode_device_relay_vprior)(
            code.handle, rl.handle, rl.prior.handle, _lib.RELAY_COST[relay.cost], *ins, float(beta), float(eps), *outs))
        return res
    _lib.check((L.qldpc_decode_host_relay if host else L.qldpc_decode_device_relay)(
        code.handle, rl.handle, *ins, float(p), float(beta), float(eps), *outs))
    return res


def _decode_batch_hard(H, syndromes, max_iter, algo, want_post, osd_order, stream, out, ehat_bits):
    """decode_batch for algo "NG" / "BF" (ng_kernel / bf_kernel): no schedule,
    prior or posteriors; `max_iter` is BF's and NG ignores it. DecodeResult.post
    is None; `converged` is the reference's own stop condition (BF: its
    non-zero-count residual all zero, which the true parity may contradict)."""
    if want_post or osd_order >= 0:
        raise ValueError(f"{algo} is a hard-decision decoder: it has no posteriors (want_post) and no OSD step")
    H = np.asarray(H)
    if H.ndim != 2 or H.size == 0:
        raise ValueError("H must be a non-empty 2-D matrix")
    max_iter = int(max_iter) if algo == "BF" else 1
    if max_iter < 1:
        raise ValueError("max_iter must be >= 1")
    host = not _is_torch(syndromes)
    code, _, res, ins, _, outs, held = (_host_batch if host else _device_batch)(
        H, syndromes, None, (), False, out=out, stream=stream, ehat_bits=ehat_bits, has_post=False)
    L = _lib.lib
    _lib.check((L.qldpc_hard_decode_host if host else L.qldpc_hard_decode_device)(
        code.handle, _lib.ALGO[algo], *ins, max_iter, *outs))
    return res


# _host_batch and _device_batch: what every decode_batch family does alike on its path. They take the same
# arguments (each ignores the other path's) and return (code, handle, res, ins, mask, outs, held):
#   code, handle  the _lib.Code of H and the family's handle on it, `make`(code, *made_from) (_lib.Code.schedule /
#                 .relay; None: no handle)
#   res           the DecodeResult, outputs in place
#   ins, mask, outs   the runs of an entry's arguments that every family shares, around its own handles and scalars,
#                 as addresses; post only where the entry has the slot (`has_post`; None where no posteriors are
#                 kept), info likewise (`has_info`):
#                     host    ins (syndromes, B)          mask (mask,)         outs (ehat, iters, post, flags, info)
#                     device  ins (syndromes, format, B)  mask (mask, format)  outs (ehat, format, iters, post, flags,
#                                                                                    info, stream)
#   held          the (syndromes, posteriors, mask) those addresses point into, to be kept until the entry returns
def _host_batch(H, syndromes, make, made_from, want_post, osd=False, prior_mask=None, out=None, stream=None,
                ehat_bits=False, has_post=True, has_info=False):
    """Staged and synchronous. The syndromes and the mask are looked at before
    the code and the handle are made; posteriors are kept for OSD (`osd`) even
    where the result returns none."""
    ptr = _lib.ptr
    m, n = H.shape
    syn = np.ascontiguousarray(syndromes)
    if syn.ndim != 2 or syn.shape[1] != m:
        raise ValueError(f"syndromes must be [B, {m}]")
    if syn.size and (syn.min() < 0 or syn.max() > 1):
        raise ValueError("syndrome entries must be 0 or 1")
    syn = syn.astype(np.uint8, copy=False)
    B = syn.shape[0]
    mask = ()
    if prior_mask is not None:
        if _is_torch(prior_mask):
            raise ValueError("prior_mask must be a NumPy array on the host path (the syndromes are)")
        prior_mask = np.ascontiguousarray(prior_mask)
        if prior_mask.shape != (B, n):
            raise ValueError(f"prior_mask must be [{B}, {n}]")
        if prior_mask.size and (prior_mask.min() < 0 or prior_mask.max() > 1):
            raise ValueError("prior_mask entries must be 0 or 1")
        prior_mask = prior_mask.astype(np.uint8, copy=False)
        mask = (ptr(prior_mask),)
    code = _lib.code_for(H)
    handle = make(code, *made_from) if make is not None else None
    post = np.zeros((B, n), np.float64) if want_post or osd else None
    res = DecodeResult(np.zeros((B, n), np.uint8), np.zeros(B, np.int32), post if want_post else None,
                       np.zeros(B, np.int32), np.zeros((B, 2), np.int32) if has_info else None)
    if has_info:
        outs = (ptr(res.ehat), ptr(res.iters), ptr(post), ptr(res.flags), ptr(res.info))
    elif has_post:
        outs = (ptr(res.ehat), ptr(res.iters), ptr(post), ptr(res.flags))
    else:
        outs = (ptr(res.ehat), ptr(res.iters), ptr(res.flags))
    return code, handle, res, (ptr(syn), B), mask, outs, (syn, post, prior_mask)


def _device_batch(H, syndromes, make, made_from, want_post, osd=False, prior_mask=None, out=None, stream=None,
                  ehat_bits=False, has_post=True, has_info=False):
    """Asynchronous on `stream` (or torch's current one); it syncs on nothing.
    The code and the handle are made before the syndromes are looked at; with
    out= nothing is allocated."""
    import torch
    m, n = H.shape
    dev = syndromes.device
    code = _lib.code_for(H, dev.index)
    handle = make(code, *made_from) if make is not None else None
    syn = syndromes.contiguous()
    wm, wn = (m + 63) // 64, (n + 63) // 64
    if syn.dim() == 2 and syn.dtype == torch.uint8 and syn.shape[1] == m:
        syn_fmt = _lib.FMT_BYTES
    elif syn.dim() == 2 and syn.dtype == torch.int64 and syn.shape[1] == wm:
        syn_fmt = _lib.FMT_BITS
    else:
        raise ValueError(f"syndromes must be uint8 [B, {m}] or int64 words [B, {wm}]")
    B = syn.shape[0]
    mask = ()
    if prior_mask is not None:
        if not (_is_torch(prior_mask) and prior_mask.device == dev and prior_mask.dim() == 2):
            raise ValueError("prior_mask must be a 2-D tensor on the syndromes' device")
        prior_mask = prior_mask.contiguous()
        if prior_mask.dtype == torch.uint8 and tuple(prior_mask.shape) == (B, n):
            mask = (prior_mask.data_ptr(), _lib.FMT_BYTES)
        elif prior_mask.dtype == torch.int64 and tuple(prior_mask.shape) == (B, wn):
            mask = (prior_mask.data_ptr(), _lib.FMT_BITS)
        else:
            raise ValueError(f"prior_mask must be uint8 [{B}, {n}] or int64 words [{B}, {wn}]")
    want = {"ehat": ((B, wn), torch.int64) if ehat_bits else ((B, n), torch.uint8),
            "iters": ((B,), torch.int32), "flags": ((B,), torch.int32)}
    if has_info:
        want["info"] = ((B, 2), torch.int32)
    if want_post:
        want["post"] = ((B, n), torch.float64)
    if out is not None:
        t = {k: getattr(out, k) for k in want}
        if not all(x is not None and x.shape == shape and x.dtype == dtype and x.device == dev and x.is_contiguous()
                   for x, (shape, dtype) in zip(t.values(), want.values())):
            raise ValueError("out buffers do not match the batch (uint8 [B, n] or int64 [B, ceil(n/64)], int32 [B], "
                             "int32 [B]" + (", int32 info [B, 2]" if has_info else "")
                             + (", float64 [B, n] if want_post" if has_post else "") + ") on the syndromes' device")
    else:
        t = {k: torch.empty(shape, dtype=dtype, device=dev) for k, (shape, dtype) in want.items()}
    res = DecodeResult(t["ehat"], t["iters"], t.get("post"), t["flags"], t.get("info"))
    st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
    post_p = (res.post.data_ptr() if want_post else None,) if has_post else ()
    info_p = (res.info.data_ptr(),) if has_info else ()
    outs = (res.ehat.data_ptr(), _lib.FMT_BITS if ehat_bits else _lib.FMT_BYTES, res.iters.data_ptr(), *post_p,
            res.flags.data_ptr(), *info_p, st)
    return code, handle, res, (syn.data_ptr(), syn_fmt, B), mask, outs, (syn, res.post, prior_mask)


OSD_METHODS = ("ref", "cs")
OSD_CS_MAX_LAMBDA = 64       # QLDPC_OSD_CS_MAX_LAMBDA


def osd_method_checked(method, order, algo="MS"):
    """The OSD method of a call, checked: "ref" (the reference's OSDdec) or "cs"
    (OSD-CS, `order` = lambda). ValueError for an unknown method, and for "cs"
    without an order in 0..64 or with a decoder that has no OSD step."""
    if method not in OSD_METHODS:
        raise ValueError(f"osd_method must be one of {OSD_METHODS}, got {method!r}")
    if method == "cs":
        if algo not in ("MS", "BP"):
            raise ValueError(f'osd_method="cs" needs a decoder with posteriors (MS or BP), not {algo}')
        if not 0 <= int(order) <= OSD_CS_MAX_LAMBDA:
            raise ValueError(f'osd_method="cs" takes its lambda from the OSD order: 0..{OSD_CS_MAX_LAMBDA}, '
                             f"got {order}")
    return method


OSD_COSTS = ("hamming", "prior")


def osd_cost_checked(cost, method, prior=None, where="prior="):
    """The OSD-CS cost of a call, checked: "hamming" or "prior" (DESIGN.md
    §3.19). ValueError for an unknown cost, and for "prior" without method
    "cs" or without a prior row (`where` names the argument that gives it)."""
    if cost not in OSD_COSTS:
        raise ValueError(f"osd_cost must be one of {OSD_COSTS}, got {cost!r}")
    if cost == "prior":
        if method != "cs":
            raise ValueError(f'osd_cost="prior" is OSD-CS\'s cost: it needs osd_method="cs", not {method!r}')
        if prior is None:
            raise ValueError(f'osd_cost="prior" weighs candidates by a prior row: give it ({where})')
    return cost


def _cost_kw(cost, prior, eps=1e-9, name="cost"):
    """The OSD-CS cost with its row and eps as keywords, given only for
    "prior": a "hamming" call is the call earlier releases made."""
    return {} if cost == "hamming" else {name: cost, "prior": prior, "eps": eps}


def _osd_prior_handle(code, cost, prior, eps):
    """The qldpc_prior handle of an OSD call's row, or None with cost "hamming"."""
    return None if cost == "hamming" else code.prior(prior, eps).handle


def _method_kw(name, method):
    """The OSD method as a keyword of that name, given only when it is not the
    default: a "ref" call is the call earlier releases made."""
    return {} if method == "ref" else {name: method}


def osd_perm(posteriorLLRs):
    """Reliability order of decoders.py:320-325, computed with NumPy itself."""
    posteriorLLRs = np.asarray(posteriorLLRs)
    posteriorLLRsat = np.where(np.abs(posteriorLLRs) < 100.0, posteriorLLRs,
                               100.0 * np.sign(posteriorLLRs))
    posteriorProb = 1. / (1. + np.exp(posteriorLLRsat))
    reliability = np.where(posteriorProb > 0.5, posteriorProb, 1 - posteriorProb)
    return np.argsort(reliability)


def _pin_rows():
    """Fixed posterior rows for numpy_order_pinned: saturated (long runs of
    keys equal to 1.0), min-sum-quantised (many exact ties), +-x pairs, the
    clip edges, and sizes on both sides of the 256-key network."""
    rng = np.random.default_rng(20251226)
    rows = []
    L = np.log((1 - 0.1 / 3) / (0.1 / 3))
    for n in (7, 175, 256, 257, 544, 1020, 2047):
        P = rng.normal(0, 6, n)
        P[rng.random(n) < 0.7] *= 1e3
        rows.append(P)
        rows.append(L + rng.integers(-6, 7, n).astype(np.float32) * np.float32(0.975))
        Q = rng.normal(0, 2, n)
        Q[1::4] = -Q[::4][:Q[1::4].size]
        Q[:6] = [0.0, -0.0, 100.0, -100.0, 36.7, -36.7][:min(6, n)]
        rows.append(Q)
    return rows


_PINNED = {}                 # "order" / "libm" -> (bool, reason)


def _pin_warn(what, reason):
    import warnings
    warnings.warn(f"qldpcsim_amd: {what} not pinned to the running NumPy {np.__version__} ({reason}); "
                  + ("every OSD reliability order is computed by NumPy on the host (slower, same results)"
                     if what == "reliability order" else
                     "BP decodes follow the 1e-5 posterior contract instead of bit-exact parity"),
                  RuntimeWarning, stacklevel=3)


def numpy_order_pinned():
    """Whether the running NumPy's reliability order (np.exp, np.argsort)
    equals the restatement the device and the host library run
    (qldpc_osd_order_host): checked once, on _pin_rows(), bit for bit. When it
    does not, a RuntimeWarning says why (missing library symbol, or the first
    pin row whose order differs) and every OSD order is computed by NumPy on
    the host; parity_pins() reports the reason."""
    if "order" not in _PINNED:
        ok, why = True, "equal on every pin row"
        try:
            for r, P in enumerate(_pin_rows()):
                P = np.ascontiguousarray(P, np.float64)
                n = P.size
                perm = np.empty(n, np.int32)
                st = np.empty(1, np.int32)
                _lib.check(_lib.lib.qldpc_osd_order_host(_lib.ptr(P), 1, n, _lib.ptr(perm), _lib.ptr(st), 1))
                if st[0] != 0 or not np.array_equal(perm, osd_perm(P)):
                    ok, why = False, f"pin row {r} (n = {n}) orders differently"
                    break
        except (OSError, AttributeError, RuntimeError) as e:
            ok, why = False, f"{type(e).__name__}: {e}"
        _PINNED["order"] = (ok, why)
        if not ok:
            _pin_warn("reliability order", why)
    return _PINNED["order"][0]


def _libm_pin_args():
    """Fixed arguments for numpy_libm_pinned, over the ranges BP and the
    priors feed each function (decoders.py:147, :232, :254-259, :322)."""
    rng = np.random.default_rng(20251226)
    t = np.concatenate([rng.uniform(-40, 40, 6000), rng.uniform(-1, 1, 3000), rng.normal(0, 1e-4, 500),
                        np.linspace(19.0, 20.0, 257), -np.linspace(19.0, 20.0, 257),
                        [0.0, -0.0, 1e-300, -1e-300, 0.5, 24.0, 710.0, -710.0]])
    a = np.concatenate([rng.uniform(-1, 1, 6000), 1 - rng.uniform(0, 1e-6, 500), -1 + rng.uniform(0, 1e-6, 500),
                        [1 - 1e-9, -(1 - 1e-9), 0.0, -0.0, 1e-300, 0.5, -0.5]])
    pr = rng.uniform(1e-5, 0.4, 3000)
    lg = np.concatenate([(1 - pr) / pr, rng.uniform(1e-3, 1e3, 3000), np.exp(rng.uniform(-700, 700, 500))])
    ex = np.concatenate([rng.uniform(-100, 100, 6000), rng.uniform(-706, 706, 1000), [0.0, -0.0, 100.0, -100.0]])
    return {"tanh": (0, t, np.tanh), "atanh": (1, a, np.arctanh), "log": (2, lg, np.log), "exp": (3, ex, np.exp)}


def numpy_libm_pinned():
    """Whether the running NumPy's tanh / arctanh / log / exp equal the
    restatement BP's kernels and the priors run (include/qldpc_libm.h, through
    qldpc_libm_eval_host): checked once, bit for bit, on _libm_pin_args(). BP is
    bit-exact against the reference only where this holds;
    otherwise a RuntimeWarning says which function differs and parity_pins()
    reports it."""
    if "libm" not in _PINNED:
        ok, why = True, "equal on every pin argument"
        try:
            for name, (fn, x, ref) in _libm_pin_args().items():
                x = np.ascontiguousarray(x, np.float64)
                y = np.empty_like(x)
                _lib.check(_lib.lib.qldpc_libm_eval_host(fn, _lib.ptr(x), x.size, _lib.ptr(y)))
                with np.errstate(all="ignore"):
                    want = ref(x)
                bad = np.flatnonzero(y.view(np.uint64) != want.view(np.uint64))
                if bad.size:
                    ok, why = False, f"np.{ref.__name__} differs on {bad.size} of {x.size} arguments (x = {x[bad[0]]!r})"
                    break
        except (OSError, AttributeError, RuntimeError) as e:
            ok, why = False, f"{type(e).__name__}: {e}"
        _PINNED["libm"] = (ok, why)
        if not ok:
            _pin_warn("the restated libm", why)
    return _PINNED["libm"][0]


def parity_pins():
    """{"order": bool, "libm": bool, "numpy": version, "reasons": {...}}: the
    run-time pins parity depends on (smoke() and bench.py report them)."""
    numpy_order_pinned()
    numpy_libm_pinned()
    return {"order": _PINNED["order"][0], "libm": _PINNED["libm"][0], "numpy": np.__version__,
            "reasons": {k: v[1] for k, v in _PINNED.items()}}


def osd_perms(post, nthreads=None):
    """Row-wise reliability orders (decoders.py:320-325) of a [k, n] posterior
    block. When the running NumPy is the pinned one (numpy_order_pinned), the
    host library's restatement computes them (C++ threads, no GIL), and
    NumPy only the rows it leaves (NaN, std::sort fallback); otherwise NumPy's
    own exp / argsort, chunked over host threads (identical to per-row calls;
    NumPy releases the GIL in these loops)."""
    post = np.asarray(post)
    if post.shape[0] == 0:
        return np.zeros((0, post.shape[1]), np.int32)
    if numpy_order_pinned() and post.dtype == np.float64:
        P = np.ascontiguousarray(post)
        k, n = P.shape
        out = np.empty((k, n), np.int32)
        st = np.empty(k, np.int32)
        _lib.check(_lib.lib.qldpc_osd_order_host(_lib.ptr(P), k, n, _lib.ptr(out), _lib.ptr(st),
                                                 int(nthreads or hostcores.rank_cores())))
        for r in np.flatnonzero(st):
            out[r] = osd_perm(P[r])
        return out

    def one(P):
        # the reference's reliability, element for element (tests pin the bits):
        #   np.where(|P| < 100, P, 100 sign P)  ==  np.clip(P, -100, 100)
        #   1 / (1 + exp(sat))                  (same ufuncs, in place)
        #   np.where(prob > 0.5, prob, 1-prob)  ==  np.maximum(prob, 1-prob)
        #     (1 - prob is exact for prob > 0.5, and >= 0.5 >= prob otherwise)
        # 4x fewer passes over the block than the literal form, then NumPy's own
        # argsort decides the order (and its ties) exactly as the reference's.
        out = np.empty((P.shape[0], P.shape[1]), np.int32)
        for r0 in range(0, P.shape[0], 64):          # cache-sized row blocks
            t = np.clip(P[r0:r0 + 64], -100.0, 100.0)
            np.exp(t, out=t)
            np.add(t, 1.0, out=t)
            np.divide(1.0, t, out=t)
            np.maximum(t, np.subtract(1.0, t), out=t)
            out[r0:r0 + 64] = np.argsort(t, axis=1)
        return out

    nthreads = nthreads or hostcores.rank_cores()
    if post.shape[0] < 256 or nthreads <= 1:
        return one(post)
    # a persistent pool (starting 16 threads per call had cost ~4 ms, more than
    # the sorts of a few hundred rows) and chunks of >= 64 rows
    chunks = max(1, min(4 * nthreads, post.shape[0] // 64))
    return np.concatenate(list(_thread_pool(nthreads).map(one, np.array_split(post, chunks))))


_POOL = {}
_SIDE = {}


def _side_stream(dev):
    import torch
    if dev.index not in _SIDE:
        _SIDE[dev.index] = torch.cuda.Stream(dev)
    return _SIDE[dev.index]


def _thread_pool(n):
    from concurrent.futures import ThreadPoolExecutor
    if n not in _POOL:
        _POOL[n] = ThreadPoolExecutor(n)
    return _POOL[n]


_PINNED_BUF = {}             # key -> page-locked staging tensor (release_workspaces frees them)


def _pinned(key, shape, dtype):
    """Grow-only page-locked host staging buffers (D2H of posteriors, H2D of
    reliability orders run at DMA speed instead of through pageable copies)."""
    import torch
    need = int(np.prod(shape))
    buf = _PINNED_BUF.get(key)
    if buf is None or buf.numel() < need or buf.dtype != dtype:
        # page-locking is slow (ms per call): grow geometrically, start at 1 MiB
        old = 0 if buf is None or buf.dtype != dtype else buf.numel()
        cap = max(need, 2 * old, (1 << 20) // torch.empty((), dtype=dtype).element_size())
        buf = torch.empty(cap, dtype=dtype, pin_memory=True)
        _PINNED_BUF[key] = buf
    return buf[:need].view(*shape)


def apply_osd_device(H, syn, res, order, stream=None, method="ref", cost="hamming", prior=None, eps=1e-9):
    """GPU OSD for the non-converged shots of a device decode `res`
    (DecodeResult of torch tensors, with posteriors). The reliability order is
    NumPy's, computed on the device (qldpc_osd_device_ordered); only the shots
    it leaves to NumPy (NaN posteriors, x86-simd-sort's std::sort fallback)
    have their posteriors copied to the host. Updates res.ehat in place. See
    apply_osd_device_many for several decodes at once. `method`: "ref", or "cs"
    for OSD-CS with lambda = `order` (decode_batch's osd_method); `cost`:
    decode_batch's osd_cost, with "prior" the row `prior` (one probability per
    column of H) and the `eps` of its LLRs."""
    return apply_osd_device_many([(H, syn, res)], order, stream, method, cost, None if prior is None else [prior],
                                 eps)[0]


def apply_osd_device_many(items, order, stream=None, method="ref", cost="hamming", prior=None, eps=1e-9):
    """apply_osd_device for several (H, syn, res) decodes (the X and Z halves
    of a batch): every device order and elimination is queued first. `prior`
    (cost "prior"): one row per item, in the items' order."""
    staged = osd_device_stage(items, stream, order=order, method=method, cost=cost, prior=prior, eps=eps)
    osd_device_finish(items, staged, order, stream, method=method, cost=cost, prior=prior, eps=eps)
    with _on_stream(stream):                      # the status check reads on the same stream
        osd_status_check(items)
    return [r.ehat for _, _, r in items]


# Where the OSD reliability order comes from (decoders.py:320-325):
#   device_min  fewest non-converged shots of one decode for which the order
#               is computed on the device (below it: on the host, after a copy
#               of their posteriors); the device order is NumPy's exact order,
#               so the default is every decode;
#   host_order  the host computes every OSD shot's order (A/B reference, and
#               the setting whenever the running NumPy is not the pinned one:
#               numpy_order_pinned() False).
# Read once at import from QLDPC_OSD_DEVICE_MIN / QLDPC_OSD_HOST_ORDER (tools
# start one process per setting); set_osd_policy / osd_policy change it.
OSD_POLICY = {"device_min": int(os.environ.get("QLDPC_OSD_DEVICE_MIN", "1")),
              "host_order": os.environ.get("QLDPC_OSD_HOST_ORDER", "") == "1"}


def set_osd_policy(device_min=None, host_order=None):
    if device_min is not None:
        OSD_POLICY["device_min"] = int(device_min)
    if host_order is not None:
        OSD_POLICY["host_order"] = bool(host_order)


@contextlib.contextmanager
def osd_policy(**kw):
    """`with osd_policy(device_min=1): ...` — the previous policy comes back after."""
    old = dict(OSD_POLICY)
    try:
        set_osd_policy(**kw)
        yield
    finally:
        OSD_POLICY.update(old)


# OSD shots of this process since reset_osd_stats(): every non-converged shot
# OSD saw, and those whose reliability order the host computed (NumPy or the
# host restatement: policy, n > 2048, or the device's NaN / fallback shots)
OSD_STATS = {"osd_shots": 0, "host_order_shots": 0}


def reset_osd_stats():
    OSD_STATS.update(osd_shots=0, host_order_shots=0)


def _on_stream(stream):
    """Context that makes `stream` (a raw HIP stream handle, or None = torch's
    current stream) the current stream, so every kernel, copy and event of
    one OSD stage is ordered on it."""
    import torch
    if stream is None:
        return contextlib.nullcontext()
    return torch.cuda.stream(torch.cuda.ExternalStream(stream))


def release_workspaces():
    """Free the grow-only device OSD spill workspaces and pinned staging
    buffers (they are reused across batches while a sweep runs), and the HBM
    workspaces of every cached schedule (hbm_tile_kernel's message state:
    up to half the free device memory per schedule, kept between launches)."""
    _DEVBUF.clear()
    _PINNED_BUF.clear()
    _lib.release_hbm_workspaces()


def _item_priors(items, method, cost, prior):
    """osd_cost_checked for every item of a staged call -> one row (or None) per item."""
    if osd_cost_checked(cost, method, prior, "prior=, one row per item") == "hamming":
        return [None] * len(items)
    rows = list(prior)
    if len(rows) != len(items):
        raise ValueError(f"prior must hold one row per item: {len(items)} items, {len(rows)} rows")
    for row in rows:
        osd_cost_checked(cost, method, row, "prior=, one row per item")
    return rows


def osd_device_stage(items, stream=None, slot0=0, order=0, method="ref", cost="hamming", prior=None, eps=1e-9):
    """First half of the device OSD: find each decode's non-converged shots
    (one device sync), then queue asynchronously on the device: the
    reliability order (decoders.py:320-325) and the elimination of every shot
    whose result the device order decides, with its status copied into a
    pinned host buffer. Shots that need NumPy's order (status 2) are finished
    by osd_device_finish. `slot0` selects the pinned buffer set (pipelined
    callers alternate). OSD_POLICY["host_order"] (A/B, or an unpinned NumPy)
    or n > 2048 sends every shot through the host order (osd_perms).
    `method`, `cost`, `prior` (one row per item) and `eps` as
    apply_osd_device_many's; osd_device_finish takes the same ones."""
    osd_method_checked(method, order)
    rows = _item_priors(items, method, cost, prior)
    staged = []
    with _on_stream(stream):
        for slot, ((H, syn, res), row) in enumerate(zip(items, rows)):
            staged.append(_osd_stage_one(H, syn, res, slot0 + slot, order, method, cost, row, eps))
    return staged


@dataclass
class _Staged:
    """One decode's OSD work as osd_device_stage queued it, for
    osd_host_orders and osd_device_finish."""
    bad: object           # int64 [shots]: the batch's non-converged shots (device)
    post_b: object        # their posteriors, syndromes and estimates, gathered (device)
    syn_b: object
    e_b: object
    status: object        # int32 [shots] (device): 0 done, 1 the IndexError case, 2 needs NumPy's order
    status_h: object      # its pinned host copy, valid after `ev`
    ev: object            # recorded on the launch stream after everything queued here
    slot: int             # the pinned / spill buffer set
    on_dev: bool          # the device computed the reliability order (else every shot has status 2)
    shots: int
    # on_dev: the posteriors of the status-2 shots as the kernels spilled them, their shot indices, the pinned
    # copy of their count (valid after `ev`), and the rows the spill buffers hold
    sp_post: object = None
    sp_idx: object = None
    cnt_h: object = None
    cap: int = 0


def _osd_stage_one(H, syn, res, slot, order, method="ref", cost="hamming", prior=None, eps=1e-9):
    import torch
    if res.post is None:
        raise ValueError("apply_osd_device needs the decode's posteriors (want_post=True)")
    m, n = np.shape(H)
    B = res.post.shape[0]
    # the OSD kernels read one byte per check / variable: bit-packed decodes
    # (ehat_bits, int64 word syndromes) must be unpacked first
    if not (syn.dtype == torch.uint8 and tuple(syn.shape) == (B, m)):
        raise ValueError(f"OSD needs uint8 [B, {m}] syndromes (unpack_bits a word batch first)")
    if not (res.ehat.dtype == torch.uint8 and tuple(res.ehat.shape) == (B, n)):
        raise ValueError(f"OSD needs uint8 [B, {n}] estimates (decode without ehat_bits)")
    dev = res.ehat.device
    bad = ((res.flags & _lib.FLAG_CONVERGED) == 0).nonzero().flatten()
    k = int(bad.numel())
    if k == 0:
        return None
    OSD_STATS["osd_shots"] += k
    code = _lib.code_for(H, dev.index)
    weights = _osd_prior_handle(code, cost, prior, eps)
    post_b = res.post.index_select(0, bad)
    syn_b = syn.index_select(0, bad)
    e_b = res.ehat.index_select(0, bad)
    status = torch.empty(k, dtype=torch.int32, device=dev)
    cs = torch.cuda.current_stream(dev)
    st = cs.cuda_stream
    status_h = _pinned(("status", slot), (k,), torch.int32)
    on_dev = (n <= 2048 and k >= OSD_POLICY["device_min"] and not OSD_POLICY["host_order"]
              and numpy_order_pinned())
    spill = ()
    if on_dev:
        perm = torch.empty((k, n), dtype=torch.int32, device=dev)
        tie = torch.empty(k, dtype=torch.int32, device=dev)
        # the shots left to NumPy's order copy their posteriors into a
        # spill buffer (one DMA copy for the host later, no gather kernel);
        # at most 256 MiB per buffer — a batch that spills more takes the
        # gather path in osd_device_finish
        cap = min(k // 2 + 1024, max(1024, (256 << 20) // (8 * n)))
        sp_post = _device_buf(("spill_post", slot), (cap, n), torch.float64, dev)
        sp_idx = _device_buf(("spill_idx", slot), (cap,), torch.int32, dev)
        sp_cnt = _device_buf(("spill_cnt", slot), (1,), torch.int32, dev)
        sp_cnt.zero_()
        ordered = (_lib.lib.qldpc_osd_device_ordered_ex_cs_prior if weights is not None else
                   _lib.lib.qldpc_osd_device_ordered_ex_cs if method == "cs" else _lib.lib.qldpc_osd_device_ordered_ex)
        _lib.check(ordered(
            code.handle, k, syn_b.data_ptr(), post_b.data_ptr(), int(order),
            *(() if weights is None else (weights,)), e_b.data_ptr(), status.data_ptr(), perm.data_ptr(), tie.data_ptr(), sp_post.data_ptr(), sp_idx.data_ptr(),
            sp_cnt.data_ptr(), cap, st))
        cnt_h = _pinned(("spill_cnt", slot), (1,), torch.int32)
        cnt_h.copy_(sp_cnt, non_blocking=True)
        spill = (sp_post, sp_idx, cnt_h, cap)
    else:
        status.fill_(2)                            # every shot takes NumPy's order
    status_h.copy_(status, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record(cs)
    return _Staged(bad, post_b, syn_b, e_b, status, status_h, ev, slot, on_dev, k, *spill)


def osd_staged_on_device(staged):
    """Whether osd_device_stage queued any decode's shots with the device
    reliability order (rather than leaving them all to NumPy's)."""
    return any(sg is not None and sg.on_dev for sg in staged)


_DEVBUF = {}


def _device_buf(key, shape, dtype, dev):
    """Grow-only device workspaces reused across batches (per pipeline slot)."""
    import torch
    need = int(np.prod(shape))
    buf = _DEVBUF.get(key)
    if buf is None or buf.numel() < need or buf.dtype != dtype or buf.device != dev:
        buf = torch.empty(max(need, 1), dtype=dtype, device=dev)
        _DEVBUF[key] = buf
    return buf[:need].view(shape)


def osd_device_finish(items, staged, order, stream=None, host=None, method="ref", cost="hamming", prior=None,
                      eps=1e-9):
    """Second half: for each staged decode, the shots the device order could
    not decide (status 2) get NumPy's reliability order on the host (their
    posteriors only, pinned copies) and the GPU elimination; then the
    corrected estimates are scattered back, all queued asynchronously.
    `host` = the result of osd_host_orders(staged) if the caller already ran
    it (e.g. on a worker thread while the GPU ran the next batch); otherwise
    it runs here. res.osd_status keeps 0 / 1 per shot (1: the reference's
    IndexError case, raised by osd_status_check)."""
    rows = _item_priors(items, method, cost, prior)
    if host is None:
        host = osd_host_orders(staged)
    with _on_stream(stream):
        for (H, syn, res), sg, hr, row in zip(items, staged, host, rows):
            if sg is not None:
                _osd_finish_device(H, syn, res, sg, hr, order, method, cost, row, eps)
    return staged


def osd_host_orders(staged):
    """The host part of osd_device_finish, for every staged decode: wait for
    its device OSD (its event only), fetch the status-2 shots' posteriors and
    compute NumPy's reliability orders (decoders.py:320-325) for all of them
    in one pass over the host threads. Blocking, touches no launch stream, so
    a pipelined caller runs it on a worker thread while the GPU decodes the
    next batch. Returns per decode None (no staging) or (redo, perms_pinned)."""
    import torch
    out, blocks = [], []
    for sg in staged:
        if sg is None:
            out.append(None)
            continue
        post_b, ev, slot = sg.post_b, sg.ev, sg.slot
        dev = post_b.device
        ev.synchronize()
        redo = (sg.status_h.numpy() == 2).nonzero()[0]
        if redo.size == 0:
            out.append((redo, None))
            continue
        k2 = int(redo.size)
        hostp = _pinned(("post", slot), (k2, post_b.shape[1]), torch.float64)
        # fetch these posteriors on a side stream, with copies that wait only
        # for this decode's OSD (its event): the launch stream's next batch
        # (decode, device OSD) keeps running
        side = _side_stream(dev)
        side.wait_event(ev)
        if sg.on_dev and k2 <= sg.cap and int(sg.cnt_h[0]) == k2:
            # the kernels spilled exactly these rows: one contiguous DMA copy
            # (no gather kernel waiting for free CUs behind other work)
            idx_h = _pinned(("spill_idx", slot), (k2,), torch.int32)
            with torch.cuda.stream(side):
                hostp.copy_(sg.sp_post[:k2], non_blocking=True)
                idx_h.copy_(sg.sp_idx[:k2], non_blocking=True)
            side.synchronize()
            redo = idx_h.numpy().astype(np.int64)
        else:
            with torch.cuda.stream(side):
                idx_s = torch.as_tensor(redo, device=dev)
                hostp.copy_(post_b.index_select(0, idx_s), non_blocking=True)
            side.synchronize()
        out.append((redo, _pinned(("perm", slot), (k2, post_b.shape[1]), torch.int32)))
        blocks.append((len(out) - 1, hostp.numpy()))
    if blocks:
        # every decode's rows in one threaded pass (better parallel efficiency
        # than one pass per decode)
        if len(blocks) == 1 or len({b.shape[1] for _, b in blocks}) > 1:
            for i, P in blocks:
                out[i][1].numpy()[...] = osd_perms(P)
        else:
            perms = osd_perms(np.concatenate([P for _, P in blocks]))
            r0 = 0
            for i, P in blocks:
                out[i][1].numpy()[...] = perms[r0:r0 + P.shape[0]]
                r0 += P.shape[0]
    return out


def _osd_finish_device(H, syn, res, sg, hr, order, method="ref", cost="hamming", prior=None, eps=1e-9):
    import torch
    e_b, status = sg.e_b, sg.status
    dev = res.ehat.device
    code = _lib.code_for(H, dev.index)
    redo, perm_h = hr
    res.osd_host_order = int(redo.size)
    OSD_STATS["host_order_shots"] += int(redo.size)
    if redo.size:
        k2 = int(redo.size)
        idx = torch.as_tensor(redo, device=dev)
        perms = perm_h.to(dev, non_blocking=True)
        syn_r = sg.syn_b.index_select(0, idx)
        e_r = e_b.index_select(0, idx)
        st2 = torch.empty(k2, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        weights = _osd_prior_handle(code, cost, prior, eps)
        device = (_lib.lib.qldpc_osd_device_cs_prior if weights is not None else
                  _lib.lib.qldpc_osd_device_cs if method == "cs" else _lib.lib.qldpc_osd_device)
        _lib.check(device(code.handle, k2, syn_r.data_ptr(), perms.data_ptr(), int(order),
                          *(() if weights is None else (weights,)), e_r.data_ptr(), st2.data_ptr(), st))
        e_b.index_copy_(0, idx, e_r)
        status.index_copy_(0, idx, st2)
    res.ehat.index_copy_(0, sg.bad, e_b)
    res.osd_status = status      # checked by the caller (raises IndexError like the reference)


def osd_status_check(items, defer=None):
    """Raise the reference's IndexError if any OSD of these decodes ran its
    greedy basis loop past the last column (decoders.py:333-342). With a
    `defer` list, the per-decode flags are appended there as device tensors
    instead (no sync; the caller checks them with osd_status_raise)."""
    for _, _, res in items:
        st = res.osd_status
        if st is None:
            continue
        if defer is not None:
            defer.append((st != 0).any())
        elif bool((st != 0).any()):
            raise IndexError("OSD: column basis search ran past the last column")


def osd_status_raise(flags):
    """osd_status_check's deferred flags: one sync for all of them."""
    import torch
    if flags and bool(torch.stack(flags).any()):
        raise IndexError("OSD: column basis search ran past the last column")


def apply_osd(H, syn, ehat, post, flags, order, nthreads=None, method="ref", cost="hamming", prior=None, eps=1e-9):
    """OSD post-step for every non-converged row (decoders.py:179-180, :287-288).

    ehat (uint8 [B, n]) is updated in place. `method`: "ref", or "cs" for
    OSD-CS with lambda = `order` (decode_batch's osd_method); `cost`:
    decode_batch's osd_cost, with "prior" the row `prior` (one probability per
    column of H) and the `eps` of its LLRs.
    """
    osd_method_checked(method, order)
    osd_cost_checked(cost, method, prior)
    if cost == "prior":
        _lib.code_for(H).prior(prior, eps)         # a bad row is refused whether or not a shot needs OSD
    idx = np.flatnonzero((np.asarray(flags) & _lib.FLAG_CONVERGED) == 0)
    if idx.size == 0:
        return ehat
    OSD_STATS["osd_shots"] += int(idx.size)
    OSD_STATS["host_order_shots"] += int(idx.size)
    code = _lib.code_for(H)
    perms = np.ascontiguousarray(osd_perms(post[idx]), dtype=np.int32)
    sub_syn = np.ascontiguousarray(syn[idx], dtype=np.uint8)
    sub_e = np.ascontiguousarray(ehat[idx], dtype=np.uint8)
    weights = _osd_prior_handle(code, cost, prior, eps)
    batch = (_lib.lib.qldpc_osd_decode_batch_cs_prior if weights is not None else
             _lib.lib.qldpc_osd_decode_batch_cs if method == "cs" else _lib.lib.qldpc_osd_decode_batch)
    _lib.check(batch(code.handle, idx.size, _lib.ptr(sub_syn), _lib.ptr(perms), int(order),
                     *(() if weights is None else (weights,)), _lib.ptr(sub_e),
                     int(nthreads or hostcores.rank_cores())))
    ehat[idx] = sub_e
    return ehat


def _shot(H, syndrome):
    """A single-shot wrapper's (H, syndrome) as arrays, and the reference's
    answer where either is empty: a bare int8 array, no tuple (decoders.py:86-87,
    :138-139, :215-216; NG and relay do as MS / BP / BF), else None."""
    H, syndrome = np.asarray(H), np.asarray(syndrome)
    empty = H.size == 0 or syndrome.size == 0
    return H, syndrome, np.zeros(H.shape[1] if H.size else 0, dtype=np.int8) if empty else None


def _row(H, syndrome):
    """The syndrome as a batch of one."""
    m, n = H.shape
    if syndrome.shape != (m,):
        raise ValueError(f"syndrome must have shape ({m},), got {syndrome.shape}")
    return syndrome.reshape(1, m)


def _soft(H, syndrome, p, max_iter, layers, algo, beta, eps, OSDorder, dtype, osd_method="ref", osd_cost="hamming"):
    """MS_decoder / BP_decoder of a non-empty shot: (e_hat of `dtype`, n_iter)."""
    row = _row(H, syndrome)
    if osd_method != "ref" or OSDorder >= 0:
        osd_method_checked(osd_method, OSDorder, algo)
    vec = np.ndim(p) > 0
    osd_cost_checked(osd_cost, osd_method, p if vec else None, "an array of n probabilities for p")
    if int(max_iter) < 1:
        # the reference's iteration loop never binds e_hat (decoders.py:153/:182)
        raise UnboundLocalError("local variable 'e_hat' referenced before assignment")
    lp, lr = pack_layers(layers, H.shape[0])
    # p may be an array of n probabilities, one per column (the reference
    # raises on max(array, eps) there: DESIGN.md §7)
    r = decode_batch(H, row, None if vec else p, max_iter, algo=algo, beta=beta, eps=eps,
                     want_post=True, layer_ptr=lp, layer_rows=lr, prior=p if vec else None)
    e_hat = r.ehat[0].astype(dtype)
    if OSDorder >= 0 and not r.converged[0]:       # (:179-180, :287-288)
        e_hat = OSDdec(H, e_hat, syndrome, r.post[0], OSDorder, **_method_kw("osd_method", osd_method),
                       **_cost_kw(osd_cost, p, eps, "osd_cost"))
    return e_hat, int(r.iters[0])


def MS_decoder(H: np.ndarray, syndrome: np.ndarray, p: float, max_iter: int = 99,
               layers: Optional[list] = None, beta: float = 0.75, OSDorder: int = -1,
               eps: float = 1e-9, osd_method: str = "ref", osd_cost: str = "hamming"):
    """Normalized min-sum (reference decoders.py:110-182) on the GPU.
    osd_method="cs": OSD-CS with lambda = OSDorder (decode_batch);
    osd_cost="prior" with it and an array for `p`: that row prices the candidates."""
    H, syndrome, bare = _shot(H, syndrome)
    if bare is not None:
        return bare
    return _soft(H, syndrome, p, max_iter, layers, "MS", beta, eps, OSDorder, np.int8, osd_method, osd_cost)


def BP_decoder(H: np.ndarray, syndrome: np.ndarray, p: float, max_iter: int = 99,
               layers: Optional[list] = None, OSDorder: int = -1, eps: float = 1e-9,
               osd_method: str = "ref", osd_cost: str = "hamming"):
    """Sum-product BP (reference decoders.py:189-290) on the GPU.
    osd_method="cs": OSD-CS with lambda = OSDorder (decode_batch);
    osd_cost="prior" with it and an array for `p`: that row prices the candidates."""
    H, syndrome, bare = _shot(H, syndrome)
    if bare is not None:
        return bare
    # dtype int: (L_post < 0).astype(int) (:280)
    return _soft(H, syndrome, p, max_iter, layers, "BP", 0.75, eps, OSDorder, int, osd_method, osd_cost)


def Relay_decoder(H: np.ndarray, syndrome: np.ndarray, p: float, leg_iters, gammas, sols: int = 1,
                  beta: float = 0.75, eps: float = 1e-9, cost: str = "hamming"):
    """Relay min-sum of one syndrome on the GPU, in the style
    of MS_decoder: (e_hat int8 [n], passes run over all legs). `gammas` is
    float64 [len(leg_iters), n] (relay_gammas). `p` may be an array of n
    probabilities, one per column, as MS_decoder's (RelayConfig.prior, §3.18);
    `cost` is RelayConfig.cost ("prior" needs the array)."""
    H, syndrome, bare = _shot(H, syndrome)
    if bare is not None:
        return bare
    vec = np.ndim(p) > 0
    r = decode_batch(H, _row(H, syndrome), None if vec else p, 0, algo="RELAY", beta=beta, eps=eps,
                     relay=RelayConfig(leg_iters, gammas, sols, prior=p if vec else None, cost=cost))
    return r.ehat[0].astype(np.int8), int(r.iters[0])


def NG_decoder(H: np.ndarray, syndrome: np.ndarray):
    """Naive greedy (reference decoders.py:27-66) on the GPU: (int8 [n], steps)."""
    H, syndrome, bare = _shot(H, syndrome)
    if bare is not None:
        return bare
    r = decode_batch(H, _row(H, syndrome), 0.0, 1, algo="NG")
    return r.ehat[0].astype(np.int8), int(r.iters[0])


def BF_decoder(H: np.ndarray, syndrome: np.ndarray, max_iter: int = 50):
    """Bit flipping (reference decoders.py:74-102) on the GPU: (bool [n], iterations)."""
    H, syndrome, bare = _shot(H, syndrome)
    if bare is not None:
        return bare
    if max_iter < 1:                               # the loop does not run (:89, :102): float zeros
        return np.zeros(H.shape[1]), max_iter
    r = decode_batch(H, _row(H, syndrome), 0.0, max_iter, algo="BF")
    return r.ehat[0].astype(bool), int(r.iters[0])


def OSDdec(H: np.ndarray, e_hat: np.ndarray, syndrome: np.ndarray, posteriorLLRs: np.ndarray,
           order: int = 0, osd_method: str = "ref", osd_cost: str = "hamming", prior=None,
           eps: float = 1e-9) -> np.ndarray:
    """OSD post-decoder (reference decoders.py:299-370), host C++ GF(2).

    Mutates and returns `e_hat`, like the reference's `e_hat[perm] = ...`.
    osd_method="cs": OSD-CS with lambda = `order`;
    osd_cost="prior" with it: the candidates are priced with the row `prior`
    (one probability per column of H; `eps` as the decoders') instead of by
    Hamming weight.
    """
    osd_method_checked(osd_method, order)
    osd_cost_checked(osd_cost, osd_method, prior)
    H = np.asarray(H)
    m, n = H.shape
    perm = np.ascontiguousarray(osd_perm(posteriorLLRs), dtype=np.int32)
    syn = np.ascontiguousarray(np.asarray(syndrome) % 2, dtype=np.uint8)
    e = np.ascontiguousarray(np.asarray(e_hat) & 1, dtype=np.uint8)
    code = _lib.code_for(H)
    if osd_cost == "prior":
        _lib.check(_lib.lib.qldpc_osd_decode_batch_cs_prior(code.handle, 1, _lib.ptr(syn), _lib.ptr(perm), int(order),
                                                            code.prior(prior, eps).handle, _lib.ptr(e), 1))
    elif osd_method == "cs":
        _lib.check(_lib.lib.qldpc_osd_decode_batch_cs(code.handle, 1, _lib.ptr(syn), _lib.ptr(perm), int(order),
                                                      _lib.ptr(e), 1))
    else:
        _lib.check(_lib.lib.qldpc_osd_decode(code.handle, _lib.ptr(syn), _lib.ptr(perm), int(order),
                                             _lib.ptr(e), None, None, -1))
    e_hat[...] = e.astype(e_hat.dtype)
    return e_hat

"""decode_batch's route from Python to the C ABI, pinned without a GPU: which
of the ten decode entries a call reaches, every scalar it passes, which
tensor's or array's address lands in each pointer slot, what the result
holds, and which exception a refused call raises (and which of two, where two
things are wrong at once). The ten entries are replaced by recorders that
return 0; code, schedule, prior and relay handles are the real library's (they
need no device). The device branch is reached with CPU torch tensors and an
explicit stream. The literals were recorded before decode_batch's three
copies were folded into one host and one device path: they hold for any
decode_batch that keeps the calls, the results and the refusals."""
import ctypes

import numpy as np
import pytest
import torch

from qldpcsim_amd import _lib, codes, decoders
from qldpcsim_amd.decoders import DecodeResult, RelayConfig
from qldpcsim_amd.schedule import pack_layers

ENTRIES = ("qldpc_decode_device_ex", "qldpc_decode_device_prior", "qldpc_decode_device_vprior",
           "qldpc_decode_host", "qldpc_decode_host_prior", "qldpc_decode_host_vprior",
           "qldpc_decode_device_relay", "qldpc_decode_host_relay",
           "qldpc_hard_decode_device", "qldpc_hard_decode_host")
ST = 77                                        # the explicit stream handle of every device-path call
LAYERS = [[0], [1, 2]]                         # a two-layer schedule of Steane's three checks


class _Env:
    """Inputs shared by every case (never written: the entries are recorders)."""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.H = np.array(codes.load_code("steane")[0])                     # 3 x 7
        self.syn = rng.integers(0, 2, (3, 3), dtype=np.uint8)
        self.syn_t = torch.as_tensor(self.syn.copy())
        self.syn_w = decoders.pack_bits(self.syn_t)                         # int64 [3, 1]
        self.mask = rng.integers(0, 2, (3, 7), dtype=np.uint8)
        self.mask_t = torch.as_tensor(self.mask.copy())
        self.mask_w = decoders.pack_bits(self.mask_t)
        self.prior = np.linspace(0.01, 0.2, 7)
        self.relay = RelayConfig([5, 4], decoders.relay_gammas(7, 2), 2)
        self.lp, self.lr = pack_layers(LAYERS, 3)
        self.H2 = np.array(codes.load_code("LP04_0")[1])                    # 84 x 175: two words of checks, three of bits
        self.syn2 = rng.integers(0, 2, (3, 84), dtype=np.uint8)
        self.syn2_t = torch.as_tensor(self.syn2.copy())
        self.syn2_w = decoders.pack_bits(self.syn2_t)                       # int64 [3, 2]
        self.mask2_w = decoders.pack_bits(torch.as_tensor(rng.integers(0, 2, (3, 175), dtype=np.uint8)))
        self.relay2 = RelayConfig([3], decoders.relay_gammas(175, 1), 1)

    def host(self, **kw):
        return dict(dict(H=self.H, syndromes=self.syn, p=0.05, max_iter=20), **kw)

    def dev(self, **kw):
        return dict(dict(H=self.H, syndromes=self.syn_t, p=0.05, max_iter=20, stream=ST), **kw)

    def dev2(self, **kw):
        return dict(dict(H=self.H2, syndromes=self.syn2_w, p=0.05, max_iter=20, stream=ST), **kw)

    @staticmethod
    def out(bits=False, post=True, info=False, B=3, n=7):
        return DecodeResult(torch.empty((B, (n + 63) // 64), dtype=torch.int64) if bits
                            else torch.empty((B, n), dtype=torch.uint8),
                            torch.empty(B, dtype=torch.int32),
                            torch.empty((B, n), dtype=torch.float64) if post else None,
                            torch.empty(B, dtype=torch.int32),
                            torch.empty((B, 2), dtype=torch.int32) if info else None)


_ENV = []


def _env():
    if not _ENV:
        _ENV.append(_Env())
    return _ENV[0]


def _prev_ehat(e):
    """An earlier device decode's bit-packed estimate, as the correlated decode
    passes it on as prior_mask."""
    return decoders.decode_batch(e.H, e.syn_t, 0.05, 20, stream=ST, ehat_bits=True).ehat


# name -> keyword arguments of decode_batch, built from the shared inputs
CALLS = {
    # host path (NumPy arrays)
    "h_ms": lambda e: e.host(),
    "h_ms_post": lambda e: e.host(want_post=True),
    "h_bp_layers": lambda e: e.host(algo="BP", layers=LAYERS, p=0.01, max_iter=7),
    "h_ms_layer_ptr": lambda e: e.host(layer_ptr=e.lp, layer_rows=e.lr, beta=0.8, eps=1e-6),
    "h_ms_osd0": lambda e: e.host(osd_order=0),
    "h_ms_osd2_post": lambda e: e.host(osd_order=2, want_post=True),
    "h_ms_device_only_options": lambda e: e.host(ehat_bits=True, stream=5, out=e.out()),
    "h_ms_int64_syndromes": lambda e: e.host(syndromes=e.syn.astype(np.int64)),
    "h_mask": lambda e: e.host(prior_mask=e.mask, p_masked=0.3),
    "h_mask_bp_post_osd": lambda e: e.host(algo="BP", prior_mask=e.mask, p_masked=0.3, want_post=True, osd_order=0,
                                           layers=LAYERS),
    "h_vprior_post": lambda e: e.host(p=None, prior=e.prior, want_post=True),
    "h_vprior_bp_osd": lambda e: e.host(algo="BP", p=None, prior=list(e.prior), osd_order=0, eps=1e-7),
    "h_relay": lambda e: e.host(algo="RELAY", relay=e.relay, max_iter=0),
    "h_relay_post": lambda e: e.host(algo="RELAY", relay=e.relay, want_post=True, beta=0.9, eps=1e-6),
    "h_ng": lambda e: e.host(algo="NG", max_iter=9),
    "h_bf": lambda e: e.host(algo="BF", max_iter=9),
    "h_lp04": lambda e: e.host(H=e.H2, syndromes=e.syn2, want_post=True),
    # device path (torch tensors, explicit stream)
    "d_ms": lambda e: e.dev(),
    "d_ms_post": lambda e: e.dev(want_post=True),
    "d_ms_words": lambda e: e.dev(syndromes=e.syn_w),
    "d_ms_bits": lambda e: e.dev(ehat_bits=True),
    "d_ms_words_bits_post": lambda e: e.dev(syndromes=e.syn_w, ehat_bits=True, want_post=True),
    "d_bp_layer_ptr": lambda e: e.dev(algo="BP", layer_ptr=e.lp, layer_rows=e.lr, p=0.01, max_iter=7, eps=1e-6),
    "d_ms_layers": lambda e: e.dev(layers=LAYERS, beta=0.8),
    "d_ms_osd_ignored": lambda e: e.dev(osd_order=0),
    "d_ms_copied_syndromes": lambda e: e.dev(syndromes=e.syn_t.t().contiguous().t()),
    "d_ms_out": lambda e: e.dev(out=e.out()),
    "d_ms_out_post": lambda e: e.dev(out=e.out(), want_post=True),
    "d_ms_out_bits": lambda e: e.dev(out=e.out(bits=True, post=False), ehat_bits=True),
    "d_mask_bytes": lambda e: e.dev(prior_mask=e.mask_t, p_masked=0.3),
    "d_mask_words_post": lambda e: e.dev(prior_mask=e.mask_w, p_masked=0.3, want_post=True, algo="BP"),
    "d_mask_earlier_ehat": lambda e: e.dev(prior_mask=_prev_ehat(e), p_masked=0.3, ehat_bits=True),
    "d_mask_out_post": lambda e: e.dev(prior_mask=e.mask_t, p_masked=0.3, out=e.out(), want_post=True,
                                       layers=LAYERS),
    "d_vprior": lambda e: e.dev(p=None, prior=e.prior),
    "d_vprior_bits_post": lambda e: e.dev(p=None, prior=e.prior, ehat_bits=True, want_post=True, algo="BP",
                                          syndromes=e.syn_w, eps=1e-7),
    "d_vprior_out": lambda e: e.dev(p=None, prior=e.prior, out=e.out(post=False)),
    "d_relay": lambda e: e.dev(algo="RELAY", relay=e.relay, max_iter=0),
    "d_relay_words_bits_post": lambda e: e.dev(algo="RELAY", relay=e.relay, syndromes=e.syn_w, ehat_bits=True,
                                               want_post=True, beta=0.9),
    "d_relay_out": lambda e: e.dev(algo="RELAY", relay=e.relay, out=e.out(info=True)),
    "d_relay_out_post": lambda e: e.dev(algo="RELAY", relay=e.relay, out=e.out(info=True), want_post=True),
    "d_ng": lambda e: e.dev(algo="NG", max_iter=9),
    "d_bf_words_bits": lambda e: e.dev(algo="BF", max_iter=9, syndromes=e.syn_w, ehat_bits=True),
    "d_bf_out": lambda e: e.dev(algo="BF", max_iter=4, out=e.out(post=False)),
    "d_lp04_words_bits_post": lambda e: e.dev2(ehat_bits=True, want_post=True),
    "d_lp04_mask_words": lambda e: e.dev2(prior_mask=e.mask2_w, p_masked=0.2, ehat_bits=True),
    "d_lp04_bytes_out_bits": lambda e: e.dev2(syndromes=e.syn2_t, ehat_bits=True,
                                              out=e.out(bits=True, post=False, n=175)),
    "d_lp04_relay_bits": lambda e: e.dev2(algo="RELAY", relay=e.relay2, ehat_bits=True),
    "d_lp04_ng_bits": lambda e: e.dev2(algo="NG", ehat_bits=True),
}

# what each call hands to the library and returns, recorded on the three-copy decode_batch:
#   the C-ABI entry reached;
#   its arguments in order: scalars as they are; handles and addresses by the name of the object they belong to
#     (result fields, "syn" / "mask" = the call's own syndromes / prior_mask, "?" = a copy made inside);
#   per field of the DecodeResult (ehat, iters, post, flags, info): None, or container (N NumPy, T torch):dtype:shape;
#   the arguments code_for got after H (the device path keys the code by the device's index);
#   "out", with out=: whether ehat, iters, post, flags, info of the result are out's own tensors;
#   "osd": apply_osd's arguments, where the host path calls it
N7 = ["N:uint8:3x7", "N:int32:3", None, "N:int32:3", None]
N7P = ["N:uint8:3x7", "N:int32:3", "N:float64:3x7", "N:int32:3", None]
T7 = ["T:uint8:3x7", "T:int32:3", None, "T:int32:3", None]
T7P = ["T:uint8:3x7", "T:int32:3", "T:float64:3x7", "T:int32:3", None]
T7W = ["T:int64:3x1", "T:int32:3", None, "T:int32:3", None]
T7WP = ["T:int64:3x1", "T:int32:3", "T:float64:3x7", "T:int32:3", None]
T175W = ["T:int64:3x3", "T:int32:3", None, "T:int32:3", None]
HOST, DEV = [[]], [[None]]
OSD0 = {"osd": ["H", "syn", "ehat", "post", "flags", 0]}
ALL_OUT = {"out": [True, True, True, True, True]}
OUT_BUT_POST = {"out": [True, True, False, True, True]}
EXPECT = {
    "h_ms": ("qldpc_decode_host",
             ["code", "sched:F", 0, "syn", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", None, "flags"], N7, HOST, {}),
    "h_ms_post": ("qldpc_decode_host",
                  ["code", "sched:F", 0, "syn", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", "post", "flags"],
                  N7P, HOST, {}),
    "h_bp_layers": ("qldpc_decode_host",
                    ["code", "sched:L", 1, "syn", 3, 0.01, 7, 0.75, 1e-09, "ehat", "iters", None, "flags"],
                    N7, HOST, {}),
    "h_ms_layer_ptr": ("qldpc_decode_host",
                       ["code", "sched:L", 0, "syn", 3, 0.05, 20, 0.8, 1e-06, "ehat", "iters", None, "flags"],
                       N7, HOST, {}),
    "h_ms_osd0": ("qldpc_decode_host",
                  ["code", "sched:F", 0, "syn", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", "post", "flags"],
                  N7, HOST, OSD0),
    "h_ms_osd2_post": ("qldpc_decode_host",
                       ["code", "sched:F", 0, "syn", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", "post", "flags"],
                       N7P, HOST, {"osd": ["H", "syn", "ehat", "post", "flags", 2]}),
    "h_ms_device_only_options": ("qldpc_decode_host",
                                 ["code", "sched:F", 0, "syn", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", None,
                                  "flags"], N7, HOST, {"out": [False, False, False, False, True]}),
    "h_ms_int64_syndromes": ("qldpc_decode_host",
                             ["code", "sched:F", 0, "?", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", None, "flags"],
                             N7, HOST, {}),
    "h_mask": ("qldpc_decode_host_prior",
               ["code", "sched:F", 0, "syn", 3, 0.05, 0.3, "mask", 20, 0.75, 1e-09, "ehat", "iters", None, "flags"],
               N7, HOST, {}),
    "h_mask_bp_post_osd": ("qldpc_decode_host_prior",
                           ["code", "sched:L", 1, "syn", 3, 0.05, 0.3, "mask", 20, 0.75, 1e-09, "ehat", "iters",
                            "post", "flags"], N7P, HOST, OSD0),
    "h_vprior_post": ("qldpc_decode_host_vprior",
                      ["code", "sched:F", 0, "syn", 3, "prior", 20, 0.75, "ehat", "iters", "post", "flags"],
                      N7P, HOST, {}),
    "h_vprior_bp_osd": ("qldpc_decode_host_vprior",
                        ["code", "sched:F", 1, "syn", 3, "prior", 20, 0.75, "ehat", "iters", "post", "flags"],
                        N7, HOST, OSD0),
    "h_relay": ("qldpc_decode_host_relay",
                ["code", "relay", "syn", 3, 0.05, 0.75, 1e-09, "ehat", "iters", None, "flags", "info"],
                ["N:uint8:3x7", "N:int32:3", None, "N:int32:3", "N:int32:3x2"], HOST, {}),
    "h_relay_post": ("qldpc_decode_host_relay",
                     ["code", "relay", "syn", 3, 0.05, 0.9, 1e-06, "ehat", "iters", "post", "flags", "info"],
                     ["N:uint8:3x7", "N:int32:3", "N:float64:3x7", "N:int32:3", "N:int32:3x2"], HOST, {}),
    "h_ng": ("qldpc_hard_decode_host", ["code", 2, "syn", 3, 1, "ehat", "iters", "flags"], N7, HOST, {}),
    "h_bf": ("qldpc_hard_decode_host", ["code", 3, "syn", 3, 9, "ehat", "iters", "flags"], N7, HOST, {}),
    "h_lp04": ("qldpc_decode_host",
               ["code", "sched:F", 0, "syn", 3, 0.05, 20, 0.75, 1e-09, "ehat", "iters", "post", "flags"],
               ["N:uint8:3x175", "N:int32:3", "N:float64:3x175", "N:int32:3", None], HOST, {}),
    "d_ms": ("qldpc_decode_device_ex",
             ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", None, "flags", 77],
             T7, DEV, {}),
    "d_ms_post": ("qldpc_decode_device_ex",
                  ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", "post", "flags", 77],
                  T7P, DEV, {}),
    "d_ms_words": ("qldpc_decode_device_ex",
                   ["code", "sched:F", 0, "syn", 1, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", None, "flags", 77],
                   T7, DEV, {}),
    "d_ms_bits": ("qldpc_decode_device_ex",
                  ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 1, "iters", None, "flags", 77],
                  T7W, DEV, {}),
    "d_ms_words_bits_post": ("qldpc_decode_device_ex",
                             ["code", "sched:F", 0, "syn", 1, 3, 0.05, 20, 0.75, 1e-09, "ehat", 1, "iters", "post",
                              "flags", 77], T7WP, DEV, {}),
    "d_bp_layer_ptr": ("qldpc_decode_device_ex",
                       ["code", "sched:L", 1, "syn", 0, 3, 0.01, 7, 0.75, 1e-06, "ehat", 0, "iters", None, "flags",
                        77], T7, DEV, {}),
    "d_ms_layers": ("qldpc_decode_device_ex",
                    ["code", "sched:L", 0, "syn", 0, 3, 0.05, 20, 0.8, 1e-09, "ehat", 0, "iters", None, "flags", 77],
                    T7, DEV, {}),
    "d_ms_osd_ignored": ("qldpc_decode_device_ex",
                         ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", None, "flags",
                          77], T7, DEV, {}),
    "d_ms_copied_syndromes": ("qldpc_decode_device_ex",
                              ["code", "sched:F", 0, "?", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", None,
                               "flags", 77], T7, DEV, {}),
    "d_ms_out": ("qldpc_decode_device_ex",
                 ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", None, "flags", 77],
                 T7, DEV, OUT_BUT_POST),
    "d_ms_out_post": ("qldpc_decode_device_ex",
                      ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 0, "iters", "post", "flags",
                       77], T7P, DEV, ALL_OUT),
    "d_ms_out_bits": ("qldpc_decode_device_ex",
                      ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 1, "iters", None, "flags",
                       77], T7W, DEV, ALL_OUT),
    "d_mask_bytes": ("qldpc_decode_device_prior",
                     ["code", "sched:F", 0, "syn", 0, 3, 0.05, 0.3, "mask", 0, 20, 0.75, 1e-09, "ehat", 0, "iters",
                      None, "flags", 77], T7, DEV, {}),
    "d_mask_words_post": ("qldpc_decode_device_prior",
                          ["code", "sched:F", 1, "syn", 0, 3, 0.05, 0.3, "mask", 1, 20, 0.75, 1e-09, "ehat", 0,
                           "iters", "post", "flags", 77], T7P, DEV, {}),
    "d_mask_earlier_ehat": ("qldpc_decode_device_prior",
                            ["code", "sched:F", 0, "syn", 0, 3, 0.05, 0.3, "mask", 1, 20, 0.75, 1e-09, "ehat", 1,
                             "iters", None, "flags", 77], T7W, DEV, {}),
    "d_mask_out_post": ("qldpc_decode_device_prior",
                        ["code", "sched:L", 0, "syn", 0, 3, 0.05, 0.3, "mask", 0, 20, 0.75, 1e-09, "ehat", 0, "iters",
                         "post", "flags", 77], T7P, DEV, ALL_OUT),
    "d_vprior": ("qldpc_decode_device_vprior",
                 ["code", "sched:F", 0, "syn", 0, 3, "prior", 20, 0.75, "ehat", 0, "iters", None, "flags", 77],
                 T7, DEV, {}),
    "d_vprior_bits_post": ("qldpc_decode_device_vprior",
                           ["code", "sched:F", 1, "syn", 1, 3, "prior", 20, 0.75, "ehat", 1, "iters", "post", "flags",
                            77], T7WP, DEV, {}),
    "d_vprior_out": ("qldpc_decode_device_vprior",
                     ["code", "sched:F", 0, "syn", 0, 3, "prior", 20, 0.75, "ehat", 0, "iters", None, "flags", 77],
                     T7, DEV, ALL_OUT),
    "d_relay": ("qldpc_decode_device_relay",
                ["code", "relay", "syn", 0, 3, 0.05, 0.75, 1e-09, "ehat", 0, "iters", None, "flags", "info", 77],
                ["T:uint8:3x7", "T:int32:3", None, "T:int32:3", "T:int32:3x2"], DEV, {}),
    "d_relay_words_bits_post": ("qldpc_decode_device_relay",
                                ["code", "relay", "syn", 1, 3, 0.05, 0.9, 1e-09, "ehat", 1, "iters", "post", "flags",
                                 "info", 77],
                                ["T:int64:3x1", "T:int32:3", "T:float64:3x7", "T:int32:3", "T:int32:3x2"], DEV, {}),
    "d_relay_out": ("qldpc_decode_device_relay",
                    ["code", "relay", "syn", 0, 3, 0.05, 0.75, 1e-09, "ehat", 0, "iters", None, "flags", "info", 77],
                    ["T:uint8:3x7", "T:int32:3", None, "T:int32:3", "T:int32:3x2"], DEV, OUT_BUT_POST),
    "d_relay_out_post": ("qldpc_decode_device_relay",
                         ["code", "relay", "syn", 0, 3, 0.05, 0.75, 1e-09, "ehat", 0, "iters", "post", "flags", "info",
                          77], ["T:uint8:3x7", "T:int32:3", "T:float64:3x7", "T:int32:3", "T:int32:3x2"], DEV, ALL_OUT),
    "d_ng": ("qldpc_hard_decode_device", ["code", 2, "syn", 0, 3, 1, "ehat", 0, "iters", "flags", 77], T7, DEV, {}),
    "d_bf_words_bits": ("qldpc_hard_decode_device", ["code", 3, "syn", 1, 3, 9, "ehat", 1, "iters", "flags", 77],
                        T7W, DEV, {}),
    "d_bf_out": ("qldpc_hard_decode_device", ["code", 3, "syn", 0, 3, 4, "ehat", 0, "iters", "flags", 77],
                 T7, DEV, ALL_OUT),
    "d_lp04_words_bits_post": ("qldpc_decode_device_ex",
                               ["code", "sched:F", 0, "syn", 1, 3, 0.05, 20, 0.75, 1e-09, "ehat", 1, "iters", "post",
                                "flags", 77],
                               ["T:int64:3x3", "T:int32:3", "T:float64:3x175", "T:int32:3", None], DEV, {}),
    "d_lp04_mask_words": ("qldpc_decode_device_prior",
                          ["code", "sched:F", 0, "syn", 1, 3, 0.05, 0.2, "mask", 1, 20, 0.75, 1e-09, "ehat", 1,
                           "iters", None, "flags", 77], T175W, DEV, {}),
    "d_lp04_bytes_out_bits": ("qldpc_decode_device_ex",
                              ["code", "sched:F", 0, "syn", 0, 3, 0.05, 20, 0.75, 1e-09, "ehat", 1, "iters", None,
                               "flags", 77], T175W, DEV, ALL_OUT),
    "d_lp04_relay_bits": ("qldpc_decode_device_relay",
                          ["code", "relay", "syn", 1, 3, 0.05, 0.75, 1e-09, "ehat", 1, "iters", None, "flags", "info",
                           77], ["T:int64:3x3", "T:int32:3", None, "T:int32:3", "T:int32:3x2"], DEV, {}),
    "d_lp04_ng_bits": ("qldpc_hard_decode_device", ["code", 2, "syn", 1, 3, 1, "ehat", 1, "iters", "flags", 77],
                       T175W, DEV, {}),
}


def _addr(x):
    return x.data_ptr() if isinstance(x, torch.Tensor) else x.ctypes.data


def _field(x):
    if x is None:
        return None
    kind = "T" if isinstance(x, torch.Tensor) else "N"
    return f"{kind}:{str(x.dtype).replace('torch.', '')}:{'x'.join(str(int(s)) for s in x.shape)}"


class _Spy:
    """The ten entries and apply_osd as recorders; code_for passes through and
    notes its key arguments."""

    def __init__(self, monkeypatch):
        self.calls, self.osd, self.code_keys = [], [], []
        for name in ENTRIES:
            monkeypatch.setattr(_lib.lib, name, lambda *a, _n=name: self.calls.append((_n, a)) or 0)
        monkeypatch.setattr(decoders, "apply_osd", lambda *a: self.osd.append(a))
        self.code_for = _lib.code_for
        monkeypatch.setattr(_lib, "code_for", lambda H, *a: self.code_keys.append(list(a)) or self.code_for(H, *a))


@pytest.fixture
def spy(monkeypatch):
    return _Spy(monkeypatch)


def _describe(spy, kw, r):
    (entry, args), = spy.calls
    H = kw["H"]
    code = spy.code_for(H, None)
    names = {code.handle.value: "code",
             code.schedule(*pack_layers(None, H.shape[0])).handle.value: "sched:F"}
    if H is _env().H:
        names[code.schedule(*pack_layers(LAYERS, 3)).handle.value] = "sched:L"
    if kw.get("relay") is not None:
        rl = kw["relay"]
        names[code.relay(np.asarray(rl.leg_iters, np.int64), np.asarray(rl.gammas, np.float64),
                         rl.sols).handle.value] = "relay"
    if kw.get("prior") is not None:
        names[code.prior(kw["prior"], kw.get("eps", 1e-9)).handle.value] = "prior"
    if spy.osd:
        names[_addr(spy.osd[0][3])] = "post"
    for label, x in (("syn", kw["syndromes"]), ("mask", kw.get("prior_mask")), ("ehat", r.ehat), ("iters", r.iters),
                     ("post", r.post), ("flags", r.flags), ("info", r.info)):
        if x is not None:
            names[_addr(x)] = label

    def sym(a):
        if isinstance(a, ctypes.c_void_p):
            return names.get(a.value, "?")
        if isinstance(a, int) and a in names:
            return names[a]
        return "?" if isinstance(a, int) and a > 1 << 20 else a

    more = {}
    out = kw.get("out")
    if out is not None:
        more["out"] = [getattr(r, f) is getattr(out, f) for f in ("ehat", "iters", "post", "flags", "info")]
    if spy.osd:
        (a,) = spy.osd
        more["osd"] = ["H" if a[0] is H else "?", *(sym(_addr(x)) for x in a[1:5]), a[5]]
    return (entry, [sym(a) for a in args], [_field(x) for x in (r.ehat, r.iters, r.post, r.flags, r.info)],
            spy.code_keys, more)


@pytest.mark.parametrize("name", list(CALLS))
def test_call(name, spy):
    kw = CALLS[name](_env())
    spy.calls.clear()                           # a case may decode once before (an earlier ehat as the mask)
    spy.code_keys.clear()
    r = decoders.decode_batch(**kw)
    assert isinstance(r, DecodeResult)
    assert _describe(spy, kw, r) == EXPECT[name]


def test_out_allocates_nothing(spy, monkeypatch):
    """With out= the device path allocates no tensor (steady-state loops)."""
    e = _env()
    made = []
    empty = torch.empty
    for kw in (e.dev(out=e.out(), want_post=True), e.dev(out=e.out(), prior_mask=e.mask_t, p_masked=0.3),
               e.dev(algo="RELAY", relay=e.relay, out=e.out(info=True), want_post=True),
               e.dev(algo="BF", out=e.out(post=False))):
        with monkeypatch.context() as mp:
            mp.setattr(torch, "empty", lambda *a, **k: made.append(a) or empty(*a, **k))
            decoders.decode_batch(**kw)
    assert made == [] and len(spy.calls) == 4


def test_libm_pin_runs_at_the_first_bp_decode_only(spy, monkeypatch):
    """numpy_libm_pinned() runs at a BP decode while "libm" is not in _PINNED:
    not for MS, relay or NG / BF, and not before the dispatch and pairing checks."""
    e = _env()
    ran = []
    monkeypatch.delitem(decoders._PINNED, "libm", raising=False)
    monkeypatch.setattr(decoders, "numpy_libm_pinned", lambda: ran.append(1))
    decoders.decode_batch(**e.host())
    decoders.decode_batch(**e.dev(algo="RELAY", relay=e.relay))
    decoders.decode_batch(**e.host(algo="BF"))
    for bad in (dict(algo="BP", relay=e.relay), dict(algo="BP", prior_mask=e.mask), dict(algo="BP?")):
        with pytest.raises(ValueError):
            decoders.decode_batch(**e.host(**bad))
    assert ran == []
    with pytest.raises(ValueError, match="max_iter must be >= 1"):
        decoders.decode_batch(**e.host(algo="BP", max_iter=0))          # the pin comes before the argument checks
    assert ran == [1]
    decoders.decode_batch(**e.dev(algo="BP"))
    assert ran == [1, 1]                                                 # the stand-in does not fill _PINNED
    monkeypatch.setitem(decoders._PINNED, "libm", (True, "test"))
    decoders.decode_batch(**e.host(algo="BP"))
    assert ran == [1, 1]


def _bad_out(**change):
    out = _Env.out(info=True)
    for k, v in change.items():
        setattr(out, k, v)
    return out


BAD_SCHED = dict(layer_ptr=[0, 3], layer_rows=[0, 1, 5])                  # the library refuses row 5
BAD_SYN = np.zeros((3, 4), np.uint8)
BAD_SYN_T = torch.zeros((3, 4), dtype=torch.uint8)
NO_LEGS = RelayConfig([0], np.zeros((1, 7)), 1)                           # the library refuses a leg of 0 iterations

# name -> keyword arguments of a refused call. The second block has two things wrong at once.
REFUSALS = {
    "prior_and_p": lambda e: e.host(prior=e.prior),
    "prior_and_mask": lambda e: e.host(p=None, prior=e.prior, prior_mask=e.mask, p_masked=0.3),
    "prior_and_p_masked": lambda e: e.host(p=None, prior=e.prior, p_masked=0.3),
    "prior_and_relay": lambda e: e.host(p=None, prior=e.prior, relay=e.relay),
    "prior_and_algo_relay": lambda e: e.host(p=None, prior=e.prior, algo="RELAY"),
    "prior_and_ng": lambda e: e.host(p=None, prior=e.prior, algo="NG"),
    "prior_shape": lambda e: e.dev(p=None, prior=e.prior[:6]),
    "prior_2d": lambda e: e.host(p=None, prior=e.prior.reshape(1, 7)),
    "prior_not_a_probability": lambda e: e.host(p=None, prior=np.full(7, 1.0)),
    "relay_without_algo": lambda e: e.host(relay=e.relay),
    "unknown_algo": lambda e: e.host(algo="OSD"),
    "mask_without_p_masked": lambda e: e.host(prior_mask=e.mask),
    "p_masked_without_mask": lambda e: e.dev(p_masked=0.3),
    "ng_with_mask": lambda e: e.host(algo="NG", prior_mask=e.mask, p_masked=0.3),
    "max_iter_0": lambda e: e.host(max_iter=0),
    "max_iter_0_device": lambda e: e.dev(algo="BP", max_iter=0),
    "H_1d": lambda e: e.host(H=e.H[0]),
    "H_3d": lambda e: e.dev(H=e.H.reshape(3, 7, 1)),
    "p_missing": lambda e: e.host(p=None),
    "p_missing_device": lambda e: e.dev(p=None),
    "p_missing_mask": lambda e: e.dev(p=None, prior_mask=e.mask_t, p_masked=0.3),
    "p_missing_relay": lambda e: e.host(p=None, algo="RELAY", relay=e.relay),
    "d_syn_shape": lambda e: e.dev(syndromes=BAD_SYN_T),
    "d_syn_1d": lambda e: e.dev(syndromes=e.syn_t[0]),
    "d_syn_dtype": lambda e: e.dev(syndromes=e.syn_t.to(torch.int32)),
    "d_syn_words_of_lp04": lambda e: e.dev2(syndromes=e.syn2_w[:, :1]),
    "d_mask_numpy": lambda e: e.dev(prior_mask=e.mask, p_masked=0.3),
    "d_mask_1d": lambda e: e.dev(prior_mask=e.mask_t[0], p_masked=0.3),
    "d_mask_shape": lambda e: e.dev(prior_mask=e.mask_t[:2], p_masked=0.3),
    "d_mask_dtype": lambda e: e.dev(prior_mask=e.mask_t.to(torch.int32), p_masked=0.3),
    "d_mask_words_of_lp04": lambda e: e.dev2(prior_mask=e.mask2_w[:, :2], p_masked=0.3),
    "d_out_ehat_shape": lambda e: e.dev(out=e.out(n=8)),
    "d_out_ehat_not_bits": lambda e: e.dev(out=e.out(), ehat_bits=True),
    "d_out_iters_dtype": lambda e: e.dev(out=_bad_out(iters=torch.empty(3, dtype=torch.int64))),
    "d_out_flags_shape": lambda e: e.dev(out=_bad_out(flags=torch.empty(4, dtype=torch.int32))),
    "d_out_not_contiguous": lambda e: e.dev(out=_bad_out(ehat=torch.empty((7, 3), dtype=torch.uint8).t())),
    "d_out_no_post": lambda e: e.dev(out=e.out(post=False), want_post=True),
    "d_out_post_dtype": lambda e: e.dev(out=_bad_out(post=torch.empty((3, 7), dtype=torch.float32)), want_post=True),
    "d_out_mask": lambda e: e.dev(out=e.out(n=8), prior_mask=e.mask_t, p_masked=0.3),
    "d_out_vprior": lambda e: e.dev(p=None, prior=e.prior, out=e.out(B=2)),
    "h_syn_shape": lambda e: e.host(syndromes=BAD_SYN),
    "h_syn_1d": lambda e: e.host(syndromes=e.syn[0]),
    "h_syn_entries": lambda e: e.host(syndromes=e.syn * 2),
    "h_syn_negative": lambda e: e.host(syndromes=e.syn.astype(np.int64) - 1),
    "h_mask_torch": lambda e: e.host(prior_mask=e.mask_t, p_masked=0.3),
    "h_mask_shape": lambda e: e.host(prior_mask=e.mask[:2], p_masked=0.3),
    "h_mask_entries": lambda e: e.host(prior_mask=e.mask * 3, p_masked=0.3),
    "relay_no_config": lambda e: e.host(algo="RELAY"),
    "relay_config_is_a_tuple": lambda e: e.dev(algo="RELAY", relay=([5], np.zeros((1, 7)), 1)),
    "relay_mask": lambda e: e.host(algo="RELAY", relay=e.relay, prior_mask=e.mask, p_masked=0.3),
    "relay_p_masked": lambda e: e.host(algo="RELAY", relay=e.relay, p_masked=0.3),
    "relay_osd": lambda e: e.host(algo="RELAY", relay=e.relay, osd_order=0),
    "relay_H_1d": lambda e: e.host(algo="RELAY", relay=e.relay, H=e.H[0]),
    "relay_layers": lambda e: e.host(algo="RELAY", relay=e.relay, layers=LAYERS),
    "relay_layer_ptr": lambda e: e.dev(algo="RELAY", relay=e.relay, layer_ptr=e.lp, layer_rows=e.lr),
    "relay_gammas_shape": lambda e: e.host(algo="RELAY", relay=RelayConfig([5, 4, 3], e.relay.gammas, 1)),
    "relay_d_syn": lambda e: e.dev(algo="RELAY", relay=e.relay, syndromes=BAD_SYN_T),
    "relay_h_syn_shape": lambda e: e.host(algo="RELAY", relay=e.relay, syndromes=BAD_SYN),
    "relay_h_syn_entries": lambda e: e.host(algo="RELAY", relay=e.relay, syndromes=e.syn + 1),
    "relay_out_no_info": lambda e: e.dev(algo="RELAY", relay=e.relay, out=e.out()),
    "relay_out_info_shape": lambda e: e.dev(algo="RELAY", relay=e.relay,
                                            out=_bad_out(info=torch.empty((3, 3), dtype=torch.int32))),
    "relay_out_no_post": lambda e: e.dev(algo="RELAY", relay=e.relay, out=e.out(post=False, info=True),
                                         want_post=True),
    "hard_want_post": lambda e: e.host(algo="NG", want_post=True),
    "hard_osd": lambda e: e.dev(algo="BF", osd_order=0),
    "hard_H_empty": lambda e: e.host(algo="NG", H=np.zeros((0, 7), np.uint8), syndromes=np.zeros((3, 0), np.uint8)),
    "hard_H_1d": lambda e: e.dev(algo="BF", H=e.H[0]),
    "bf_max_iter_0": lambda e: e.host(algo="BF", max_iter=0),
    "hard_d_syn": lambda e: e.dev(algo="NG", syndromes=BAD_SYN_T),
    "hard_h_syn_shape": lambda e: e.host(algo="BF", syndromes=BAD_SYN),
    "hard_h_syn_entries": lambda e: e.host(algo="NG", syndromes=e.syn * 2),
    "hard_out_ehat": lambda e: e.dev(algo="NG", out=e.out(n=8)),
    "hard_out_flags_dtype": lambda e: e.dev(algo="BF", out=_bad_out(flags=torch.empty(3, dtype=torch.int64))),

    # precedence: prior= first of all
    "first_prior_then_algo": lambda e: e.host(prior=e.prior, algo="OSD"),
    "first_prior_shape_then_max_iter": lambda e: e.host(p=None, prior=e.prior[:6], max_iter=0),
    # the dispatch: relay, the algorithm's name, the pairing, then the hard decoders' own checks
    "first_relay_config_then_H": lambda e: e.host(algo="RELAY", H=e.H[0]),
    "first_relay_arg_then_algo": lambda e: e.host(algo="OSD", relay=e.relay),
    "first_algo_then_pairing": lambda e: e.host(algo="OSD", prior_mask=e.mask),
    "first_pairing_then_hard": lambda e: e.host(algo="NG", prior_mask=e.mask, want_post=True),
    "first_hard_mask_then_want_post": lambda e: e.host(algo="NG", prior_mask=e.mask, p_masked=0.3, want_post=True),
    "first_hard_want_post_then_H": lambda e: e.host(algo="BF", want_post=True, H=e.H[0]),
    "first_hard_H_then_max_iter": lambda e: e.host(algo="BF", max_iter=0, H=np.zeros((3, 0), np.uint8)),
    "first_hard_max_iter_then_syn": lambda e: e.dev(algo="BF", max_iter=0, syndromes=BAD_SYN_T),
    # MS / BP: H, the schedule's packing, max_iter, then the branch
    "first_H_then_max_iter": lambda e: e.host(H=e.H[0], max_iter=0),
    "first_max_iter_then_syn": lambda e: e.host(max_iter=0, syndromes=BAD_SYN),
    "first_max_iter_then_sched_device": lambda e: e.dev(max_iter=0, **BAD_SCHED),
    # the device branch builds the code and the schedule or relay handle before it looks at the syndromes;
    # the prior handle is made last, as the entry's argument
    "d_first_sched_then_syn": lambda e: e.dev(syndromes=BAD_SYN_T, **BAD_SCHED),
    "d_first_syn_then_mask": lambda e: e.dev(syndromes=BAD_SYN_T, prior_mask=e.mask, p_masked=0.3),
    "d_first_mask_then_out": lambda e: e.dev(prior_mask=e.mask_t[:2], p_masked=0.3, out=e.out(n=8)),
    "d_first_syn_then_out": lambda e: e.dev(syndromes=BAD_SYN_T, out=e.out(n=8)),
    "d_first_out_then_p": lambda e: e.dev(p=None, out=e.out(n=8)),
    "d_first_syn_then_prior_handle": lambda e: e.dev(p=None, prior=np.full(7, 1.0), syndromes=BAD_SYN_T),
    "d_first_out_then_prior_handle": lambda e: e.dev(p=None, prior=np.full(7, 1.0), out=e.out(n=8)),
    "d_relay_first_handle_then_syn": lambda e: e.dev(algo="RELAY", relay=NO_LEGS, syndromes=BAD_SYN_T),
    "d_relay_first_syn_then_out": lambda e: e.dev(algo="RELAY", relay=e.relay, syndromes=BAD_SYN_T, out=e.out()),
    "d_hard_first_syn_then_out": lambda e: e.dev(algo="NG", syndromes=BAD_SYN_T, out=e.out(n=8)),
    # the host branch looks at the syndromes and the mask first
    "h_first_syn_then_sched": lambda e: e.host(syndromes=BAD_SYN, **BAD_SCHED),
    "h_first_syn_shape_then_entries": lambda e: e.host(syndromes=BAD_SYN + 2),
    "h_first_syn_then_mask": lambda e: e.host(syndromes=e.syn * 2, prior_mask=e.mask_t, p_masked=0.3),
    "h_first_mask_then_sched": lambda e: e.host(prior_mask=e.mask[:2], p_masked=0.3, **BAD_SCHED),
    "h_first_mask_shape_then_entries": lambda e: e.host(prior_mask=e.mask[:2] * 2, p_masked=0.3),
    "h_first_sched_then_p": lambda e: e.host(p=None, **BAD_SCHED),
    "h_first_sched_then_prior_handle": lambda e: e.host(p=None, prior=np.full(7, 1.0), **BAD_SCHED),
    "h_relay_first_syn_then_handle": lambda e: e.host(algo="RELAY", relay=NO_LEGS, syndromes=BAD_SYN),
    # relay: its own checks in order
    "relay_first_mask_then_osd": lambda e: e.host(algo="RELAY", relay=e.relay, p_masked=0.3, osd_order=0),
    "relay_first_osd_then_H": lambda e: e.host(algo="RELAY", relay=e.relay, osd_order=0, H=e.H[0]),
    "relay_first_H_then_layers": lambda e: e.host(algo="RELAY", relay=e.relay, H=e.H[0], layers=LAYERS),
    "relay_first_layers_then_gammas": lambda e: e.host(algo="RELAY", relay=RelayConfig([5], e.relay.gammas, 1),
                                                       layers=LAYERS),
    "relay_first_gammas_then_syn": lambda e: e.dev(algo="RELAY", relay=RelayConfig([5], e.relay.gammas, 1),
                                                   syndromes=BAD_SYN_T),
}

def _out_msg(more):
    return ("out buffers do not match the batch (uint8 [B, n] or int64 [B, ceil(n/64)], int32 [B], int32 [B]" + more
            + ") on the syndromes' device")


V = "ValueError"
OUT_SOFT = (V, _out_msg(", float64 [B, n] if want_post"))
OUT_RELAY = (V, _out_msg(", int32 info [B, 2], float64 [B, n] if want_post"))
OUT_HARD = (V, _out_msg(""))
PRIOR_P = (V, "give either p (one scalar prior) or prior (one per column), not both")
PRIOR_MASK = (V, "prior (per-column) and prior_mask (two-level, per shot) cannot be combined")
PRIOR_RELAY = (V, "relay min-sum takes no per-column prior")
PRIOR_6 = (V, "prior must hold 7 probabilities (one per column of H), got shape (6,)")
PAIRING = (V, "prior_mask and p_masked go together: give both or neither")
MAX_ITER = (V, "max_iter must be >= 1")
UNPACK_1 = (V, "not enough values to unpack*")
NO_P = ("TypeError", "float() argument must be a string or a*")
SYN_D = (V, "syndromes must be uint8 [B, 3] or int64 words [B, 1]")
SYN_H = (V, "syndromes must be [B, 3]")
SYN_01 = (V, "syndrome entries must be 0 or 1")
MASK_D = (V, "prior_mask must be a 2-D tensor on the syndromes' device")
MASK_D_SHAPE = (V, "prior_mask must be uint8 [3, 7] or int64 words [3, 1]")
MASK_H_SHAPE = (V, "prior_mask must be [3, 7]")
ROW_5 = ("IndexError", "index 5 is out of bounds*")
RELAY_CONFIG = (V, 'algo="RELAY" needs relay=RelayConfig(leg_iters, gammas, sols)')
RELAY_MASK = (V, "relay min-sum takes no two-level prior (prior_mask)")
RELAY_OSD = (V, "relay min-sum has no OSD step (decode with want_post and run OSDdec on the failures)")
RELAY_H = (V, "H must be a 2-D matrix")
RELAY_FLOOD = (V, "relay min-sum runs the flooding schedule only (layers=None)")
HARD_MASK = (V, "NG is a hard-decision decoder: it takes no prior (prior_mask)")
HARD_POST = "{} is a hard-decision decoder: it has no posteriors (want_post) and no OSD step"
HARD_H = (V, "H must be a non-empty 2-D matrix")

# exception and message of each refused call, recorded on the three-copy decode_batch
# (a message ending in "*" is Python's or NumPy's own and is compared up to there)
REFUSED = {
    "prior_and_p": PRIOR_P,
    "prior_and_mask": PRIOR_MASK,
    "prior_and_p_masked": PRIOR_MASK,
    "prior_and_relay": PRIOR_RELAY,
    "prior_and_algo_relay": PRIOR_RELAY,
    "prior_and_ng": (V, "NG is a hard-decision decoder: it takes no prior"),
    "prior_shape": PRIOR_6,
    "prior_2d": (V, "prior must hold 7 probabilities (one per column of H), got shape (1, 7)"),
    "prior_not_a_probability": (V, "per-variable priors: p[0] = 1 is not a probability in [0, 1)"),
    "relay_without_algo": (V, 'relay= goes with algo="RELAY"'),
    "unknown_algo": (V, "Unrecognized decoder type."),
    "mask_without_p_masked": PAIRING,
    "p_masked_without_mask": PAIRING,
    "ng_with_mask": HARD_MASK,
    "max_iter_0": MAX_ITER,
    "max_iter_0_device": MAX_ITER,
    "H_1d": UNPACK_1,
    "H_3d": (V, "too many values to unpack*"),
    "p_missing": NO_P,
    "p_missing_device": NO_P,
    "p_missing_mask": NO_P,
    "p_missing_relay": NO_P,
    "d_syn_shape": SYN_D,
    "d_syn_1d": SYN_D,
    "d_syn_dtype": SYN_D,
    "d_syn_words_of_lp04": (V, "syndromes must be uint8 [B, 84] or int64 words [B, 2]"),
    "d_mask_numpy": MASK_D,
    "d_mask_1d": MASK_D,
    "d_mask_shape": MASK_D_SHAPE,
    "d_mask_dtype": MASK_D_SHAPE,
    "d_mask_words_of_lp04": (V, "prior_mask must be uint8 [3, 175] or int64 words [3, 3]"),
    "d_out_ehat_shape": OUT_SOFT,
    "d_out_ehat_not_bits": OUT_SOFT,
    "d_out_iters_dtype": OUT_SOFT,
    "d_out_flags_shape": OUT_SOFT,
    "d_out_not_contiguous": OUT_SOFT,
    "d_out_no_post": OUT_SOFT,
    "d_out_post_dtype": OUT_SOFT,
    "d_out_mask": OUT_SOFT,
    "d_out_vprior": OUT_SOFT,
    "h_syn_shape": SYN_H,
    "h_syn_1d": SYN_H,
    "h_syn_entries": SYN_01,
    "h_syn_negative": SYN_01,
    "h_mask_torch": (V, "prior_mask must be a NumPy array on the host path (the syndromes are)"),
    "h_mask_shape": MASK_H_SHAPE,
    "h_mask_entries": (V, "prior_mask entries must be 0 or 1"),
    "relay_no_config": RELAY_CONFIG,
    "relay_config_is_a_tuple": RELAY_CONFIG,
    "relay_mask": RELAY_MASK,
    "relay_p_masked": RELAY_MASK,
    "relay_osd": RELAY_OSD,
    "relay_H_1d": RELAY_H,
    "relay_layers": RELAY_FLOOD,
    "relay_layer_ptr": RELAY_FLOOD,
    "relay_gammas_shape": (V, "relay.gammas must be float64 [3, 7] (one row per leg, one entry per variable)"),
    "relay_d_syn": SYN_D,
    "relay_h_syn_shape": SYN_H,
    "relay_h_syn_entries": SYN_01,
    "relay_out_no_info": OUT_RELAY,
    "relay_out_info_shape": OUT_RELAY,
    "relay_out_no_post": OUT_RELAY,
    "hard_want_post": (V, HARD_POST.format("NG")),
    "hard_osd": (V, HARD_POST.format("BF")),
    "hard_H_empty": HARD_H,
    "hard_H_1d": HARD_H,
    "bf_max_iter_0": MAX_ITER,
    "hard_d_syn": SYN_D,
    "hard_h_syn_shape": SYN_H,
    "hard_h_syn_entries": SYN_01,
    "hard_out_ehat": OUT_HARD,
    "hard_out_flags_dtype": OUT_HARD,
    "first_prior_then_algo": PRIOR_P,
    "first_prior_shape_then_max_iter": PRIOR_6,
    "first_relay_config_then_H": RELAY_CONFIG,
    "first_relay_arg_then_algo": (V, 'relay= goes with algo="RELAY"'),
    "first_algo_then_pairing": (V, "Unrecognized decoder type."),
    "first_pairing_then_hard": PAIRING,
    "first_hard_mask_then_want_post": HARD_MASK,
    "first_hard_want_post_then_H": (V, HARD_POST.format("BF")),
    "first_hard_H_then_max_iter": HARD_H,
    "first_hard_max_iter_then_syn": MAX_ITER,
    "first_H_then_max_iter": UNPACK_1,
    "first_max_iter_then_syn": MAX_ITER,
    "first_max_iter_then_sched_device": MAX_ITER,
    "d_first_sched_then_syn": ROW_5,
    "d_first_syn_then_mask": SYN_D,
    "d_first_mask_then_out": MASK_D_SHAPE,
    "d_first_syn_then_out": SYN_D,
    "d_first_out_then_p": OUT_SOFT,
    "d_first_syn_then_prior_handle": SYN_D,
    "d_first_out_then_prior_handle": OUT_SOFT,
    "d_relay_first_handle_then_syn": (V, "relay min-sum: leg 0 has 0 iterations (>= 1)"),
    "d_relay_first_syn_then_out": SYN_D,
    "d_hard_first_syn_then_out": SYN_D,
    "h_first_syn_then_sched": SYN_H,
    "h_first_syn_shape_then_entries": SYN_H,
    "h_first_syn_then_mask": SYN_01,
    "h_first_mask_then_sched": MASK_H_SHAPE,
    "h_first_mask_shape_then_entries": MASK_H_SHAPE,
    "h_first_sched_then_p": ROW_5,
    "h_first_sched_then_prior_handle": ROW_5,
    "h_relay_first_syn_then_handle": SYN_H,
    "relay_first_mask_then_osd": RELAY_MASK,
    "relay_first_osd_then_H": RELAY_OSD,
    "relay_first_H_then_layers": RELAY_H,
    "relay_first_layers_then_gammas": RELAY_FLOOD,
    "relay_first_gammas_then_syn": (V, "relay.gammas must be float64 [1, 7] (one row per leg, one entry per variable)"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refusal(name, spy):
    kw = REFUSALS[name](_env())
    with pytest.raises(Exception) as ei:
        decoders.decode_batch(**kw)
    exc, msg = REFUSED[name]
    assert type(ei.value).__name__ == exc
    assert str(ei.value) == msg or (msg.endswith("*") and str(ei.value).startswith(msg[:-1]))
    assert spy.calls == [] and spy.osd == []


# the single-shot wrappers over decode_batch: what they refuse, what they return for an empty H or syndrome and for
# BF's max_iter < 1, the entry each reaches, and their return types (the recorders leave zeros: not converged)
def _wrappers(e):
    g = e.relay.gammas
    return {"MS": lambda H, s, **k: decoders.MS_decoder(H, s, 0.05, **k),
            "BP": lambda H, s, **k: decoders.BP_decoder(H, s, 0.05, **k),
            "RELAY": lambda H, s, **k: decoders.Relay_decoder(H, s, 0.05, [5, 4], g, **k),
            "NG": lambda H, s, **k: decoders.NG_decoder(H, s, **k),
            "BF": lambda H, s, **k: decoders.BF_decoder(H, s, **k)}


@pytest.mark.parametrize("algo", ["MS", "BP", "RELAY", "NG", "BF"])
def test_single_shot_wrapper(algo, spy, monkeypatch):
    e = _env()
    f = _wrappers(e)[algo]
    osd = []
    monkeypatch.setattr(decoders, "OSDdec", lambda *a: osd.append(a) or a[1])
    for H, s, n in ((np.zeros((0, 7)), e.syn[0], 0), (e.H, np.zeros(0), 7), ([[]], [1, 0, 1], 0)):
        bare = f(H, s)                                                   # a bare array, no tuple
        assert isinstance(bare, np.ndarray) and bare.dtype == np.int8 and bare.shape == (n,) and not bare.any()
    if algo == "BF":
        z, it = decoders.BF_decoder(e.H, e.syn, max_iter=0)              # before the shape check: float zeros
        assert z.dtype == np.float64 and z.shape == (7,) and not z.any() and it == 0
    with pytest.raises(ValueError) as ei:
        f(e.H, e.syn, **({"max_iter": 0} if algo in ("MS", "BP") else {}))
    assert str(ei.value) == "syndrome must have shape (3,), got (3, 3)"
    if algo in ("MS", "BP"):
        with pytest.raises(UnboundLocalError) as ei:
            f(e.H, e.syn[0], max_iter=0, layers=[[0, 0, 7]])
        assert str(ei.value) == "local variable 'e_hat' referenced before assignment"
    assert spy.calls == []
    e_hat, it = f(e.H, list(e.syn[0]))
    (entry, args), = spy.calls
    want = {"MS": ("qldpc_decode_host", np.int8), "BP": ("qldpc_decode_host", np.dtype(int)),
            "RELAY": ("qldpc_decode_host_relay", np.int8), "NG": ("qldpc_hard_decode_host", np.int8),
            "BF": ("qldpc_hard_decode_host", np.bool_)}[algo]
    assert (entry, e_hat.dtype, e_hat.shape, type(it), it) == (want[0], want[1], (7,), int, 0)
    scalars = [a for a in args if isinstance(a, (int, float))]
    assert scalars == {"MS": [0, 1, 0.05, 99, 0.75, 1e-09], "BP": [1, 1, 0.05, 99, 0.75, 1e-09],
                       "RELAY": [1, 0.05, 0.75, 1e-09], "NG": [2, 1, 1], "BF": [3, 1, 50]}[algo]
    if algo in ("MS", "BP"):
        assert args[-2] is not None and osd == []                        # posteriors are always asked for
        spy.calls.clear()
        row = e.syn[0]
        out, it = f(e.H, row, OSDorder=2, layers=LAYERS, max_iter=5, eps=1e-6)
        (H, eh, s, post, order), = osd                                   # not converged: OSDdec on this shot
        assert H is e.H and out is eh and eh.dtype == want[1] and s is row and order == 2
        assert post.shape == (7,) and post.dtype == np.float64
        spy.calls.clear()
        e_hat, it = (decoders.MS_decoder if algo == "MS" else decoders.BP_decoder)(e.H, e.syn[0], e.prior)
        assert spy.calls[0][0] == "qldpc_decode_host_vprior" and e_hat.dtype == want[1]

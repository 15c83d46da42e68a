"""ctypes binding of the C ABI in include/qldpc_decoder.h (libqldpc_hip.so).

The product path has no CPU fallback: if the HIP library is missing this
module raises on import, and every decode entry point fails loudly when no
HIP device is visible.
"""
import contextlib
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QLDPC_LIB", os.path.join(_HERE, "_build", "libqldpc_hip.so"))

QLDPC_OK, QLDPC_EINVAL, QLDPC_ERANGE, QLDPC_EUNSUP, QLDPC_EHIP, QLDPC_ENOMEM = 0, -1, -2, -3, -4, -5
ALGO = {"MS": 0, "BP": 1, "NG": 2, "BF": 3}
HARD_ALGOS = ("NG", "BF")            # no schedule, prior or posteriors (qldpc_hard_decode_*)
FLAG_CONVERGED, FLAG_MIN_ZERO, FLAG_NONFINITE = 1, 2, 4
FMT_BYTES, FMT_BITS = 0, 1          # syndrome / estimate formats (QLDPC_FMT_*)
RELAY_COST = {"hamming": 0, "prior": 1}   # what "lightest solution" means (QLDPC_RELAY_COST_*)

# every symbol include/qldpc_decoder.h declares
EXPORTS = (
    "qldpc_last_error", "qldpc_version", "qldpc_device_count",
    "qldpc_code_create", "qldpc_code_destroy", "qldpc_code_shape",
    "qldpc_schedule_create", "qldpc_schedule_destroy", "qldpc_schedule_release_workspace",
    "qldpc_decode_device", "qldpc_decode_device_ex", "qldpc_decode_host", "qldpc_decode_kernel_name",
    "qldpc_decode_launch_info",
    "qldpc_decode_device_prior", "qldpc_decode_host_prior", "qldpc_decode_prior_kernel_name",
    "qldpc_prior_create", "qldpc_prior_destroy", "qldpc_decode_device_vprior", "qldpc_decode_host_vprior",
    "qldpc_decode_vprior_kernel_name",
    "qldpc_relay_create", "qldpc_relay_destroy", "qldpc_relay_layout", "qldpc_decode_device_relay",
    "qldpc_decode_host_relay", "qldpc_decode_relay_kernel_name", "qldpc_decode_relay_launch_info",
    "qldpc_decode_device_relay_vprior", "qldpc_decode_host_relay_vprior", "qldpc_decode_relay_vprior_kernel_name",
    "qldpc_decode_relay_vprior_launch_info", "qldpc_relay_vprior_layout",
    "qldpc_hard_decode_device", "qldpc_hard_decode_host", "qldpc_hard_kernel_name", "qldpc_hard_launch_info",
    "qldpc_osd_decode", "qldpc_osd_decode_batch", "qldpc_osd_device", "qldpc_osd_order_device",
    "qldpc_osd_device_ordered", "qldpc_osd_device_ordered_ex", "qldpc_cpython_setdiff_first",
    "qldpc_osd_decode_batch_cs", "qldpc_osd_device_cs", "qldpc_osd_device_ordered_cs",
    "qldpc_osd_device_ordered_ex_cs", "qldpc_osd_kernel_name",
    "qldpc_osd_decode_batch_cs_prior", "qldpc_osd_device_cs_prior", "qldpc_osd_device_ordered_cs_prior",
    "qldpc_osd_device_ordered_ex_cs_prior",
    "qldpc_osd_order_host", "qldpc_np_argsort_host", "qldpc_osd_keys_host", "qldpc_libm_eval_host",
    "qldpc_channel_thresholds", "qldpc_channel_sample", "qldpc_channel_sample_ex", "qldpc_count_outcomes",
    "qldpc_count_outcomes_ex",
    "qldpc_channel_table", "qldpc_channel_create", "qldpc_channel_destroy", "qldpc_channel_sample_vec",
    "qldpc_channel_kernel_name",
    "qldpc_logicals_create", "qldpc_logicals_destroy", "qldpc_count_logical_ex",
    "qldpc_phenom_kernel_name", "qldpc_phenom_create", "qldpc_phenom_destroy", "qldpc_phenom_sample", "qldpc_phenom_count",
    "qldpc_phenom_window",
    "qldpc_dem_create", "qldpc_dem_destroy", "qldpc_dem_sample", "qldpc_dem_count", "qldpc_dem_kernel_name",
    "qldpc_timing_enable", "qldpc_timing_reset", "qldpc_timing_read",
    "qldpc_set_option", "qldpc_get_option",
)


class HIPLibraryMissing(ImportError):
    pass


def _load():
    # PyTorch-ROCm ships its own libamdhip64.so (SONAME libamdhip64.so.7, the
    # same as /opt/rocm's). Load it first when torch is present so this
    # library binds to the very same HIP runtime instance; loading ours first
    # would bring in a second runtime and torch then sees no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise HIPLibraryMissing(
            f"{LIB_PATH} not found: build the HIP extension first "
            "(`python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C qldpcsim_amd/csrc`). There is no CPU fallback.")
    L = ctypes.CDLL(LIB_PATH)
    P, I, D, I64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int64
    PP = ctypes.POINTER(ctypes.c_void_p)
    sig = {
        "qldpc_last_error": ([], ctypes.c_char_p),
        "qldpc_version": ([], ctypes.c_char_p),
        "qldpc_device_count": ([], I),
        "qldpc_code_create": ([P, I, I, PP], I),
        "qldpc_code_destroy": ([P], I),
        "qldpc_code_shape": ([P, P, P, P], I),
        "qldpc_schedule_create": ([P, I, P, P, PP], I),
        "qldpc_schedule_destroy": ([P], I),
        "qldpc_schedule_release_workspace": ([P], I),
        "qldpc_decode_device": ([P, P, I, P, I64, D, I, D, D, P, P, P, P, P], I),
        "qldpc_decode_device_ex": ([P, P, I, P, I, I64, D, I, D, D, P, I, P, P, P, P], I),
        "qldpc_decode_host": ([P, P, I, P, I64, D, I, D, D, P, P, P, P], I),
        "qldpc_decode_kernel_name": ([P, P, I, ctypes.c_char_p, I], I),
        "qldpc_decode_launch_info": ([P, P, I, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)], I),
        "qldpc_decode_device_prior": ([P, P, I, P, I, I64, D, D, P, I, I, D, D, P, I, P, P, P, P], I),
        "qldpc_decode_host_prior": ([P, P, I, P, I64, D, D, P, I, D, D, P, P, P, P], I),
        "qldpc_decode_prior_kernel_name": ([P, P, I, ctypes.c_char_p, I], I),
        "qldpc_prior_create": ([P, P, D, PP], I),
        "qldpc_prior_destroy": ([P], I),
        "qldpc_decode_device_vprior": ([P, P, I, P, I, I64, P, I, D, P, I, P, P, P, P], I),
        "qldpc_decode_host_vprior": ([P, P, I, P, I64, P, I, D, P, P, P, P], I),
        "qldpc_decode_vprior_kernel_name": ([P, P, I, ctypes.c_char_p, I], I),
        "qldpc_relay_create": ([P, I, P, P, I, I, PP], I),
        "qldpc_relay_destroy": ([P], I),
        "qldpc_relay_layout": ([P, P], I),
        "qldpc_decode_device_relay": ([P, P, P, I, I64, D, D, D, P, I, P, P, P, P, P], I),
        "qldpc_decode_host_relay": ([P, P, P, I64, D, D, D, P, P, P, P, P], I),
        "qldpc_decode_relay_kernel_name": ([P, P, ctypes.c_char_p, I], I),
        "qldpc_decode_relay_launch_info": ([P, P, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)], I),
        "qldpc_decode_device_relay_vprior": ([P, P, P, I, P, I, I64, D, D, P, I, P, P, P, P, P], I),
        "qldpc_decode_host_relay_vprior": ([P, P, P, I, P, I64, D, D, P, P, P, P, P], I),
        "qldpc_decode_relay_vprior_kernel_name": ([P, P, ctypes.c_char_p, I], I),
        "qldpc_decode_relay_vprior_launch_info": ([P, P, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)], I),
        "qldpc_relay_vprior_layout": ([P, P], I),
        "qldpc_hard_decode_device": ([P, I, P, I, I64, I, P, I, P, P, P], I),
        "qldpc_hard_decode_host": ([P, I, P, I64, I, P, P, P], I),
        "qldpc_hard_kernel_name": ([P, I, ctypes.c_char_p, I], I),
        "qldpc_hard_launch_info": ([P, I, ctypes.POINTER(I), ctypes.POINTER(I), ctypes.POINTER(I)], I),
        "qldpc_osd_decode": ([P, P, P, I, P, P, P, I], I),
        "qldpc_osd_decode_batch": ([P, I64, P, P, I, P, I], I),
        "qldpc_osd_device": ([P, I64, P, P, I, P, P, P], I),
        "qldpc_osd_order_device": ([P, I64, P, P, P, P], I),
        "qldpc_osd_device_ordered": ([P, I64, P, P, I, P, P, P, P, P], I),
        "qldpc_osd_device_ordered_ex": ([P, I64, P, P, I, P, P, P, P, P, P, P, I64, P], I),
        "qldpc_osd_decode_batch_cs": ([P, I64, P, P, I, P, I], I),
        "qldpc_osd_device_cs": ([P, I64, P, P, I, P, P, P], I),
        "qldpc_osd_device_ordered_cs": ([P, I64, P, P, I, P, P, P, P, P], I),
        "qldpc_osd_device_ordered_ex_cs": ([P, I64, P, P, I, P, P, P, P, P, P, P, I64, P], I),
        "qldpc_osd_decode_batch_cs_prior": ([P, I64, P, P, I, P, P, I], I),
        "qldpc_osd_device_cs_prior": ([P, I64, P, P, I, P, P, P, P], I),
        "qldpc_osd_device_ordered_cs_prior": ([P, I64, P, P, I, P, P, P, P, P, P], I),
        "qldpc_osd_device_ordered_ex_cs_prior": ([P, I64, P, P, I, P, P, P, P, P, P, P, P, I64, P], I),
        "qldpc_osd_kernel_name": ([P, I, ctypes.c_char_p, I], I),
        "qldpc_cpython_setdiff_first": ([I, P, I], I),
        "qldpc_osd_order_host": ([P, I64, I, P, P, I], I),
        "qldpc_np_argsort_host": ([P, I, P], I),
        "qldpc_osd_keys_host": ([P, I64, P, I], None),
        "qldpc_libm_eval_host": ([I, P, I64, P], I),
        "qldpc_channel_thresholds": ([D, P, P, P], I),
        "qldpc_channel_sample": ([P, P, D, ctypes.c_uint64, ctypes.c_uint64, I64, P, P, P, P, P], I),
        "qldpc_channel_sample_ex": ([P, P, D, ctypes.c_uint64, ctypes.c_uint64, I64, P, P, P, P, I, P], I),
        "qldpc_count_outcomes": ([P, P, I64, P, P, P, P, P, P, P, P, P, P], I),
        "qldpc_count_outcomes_ex": ([P, P, I64, P, P, P, P, I, P, P, I, P, P, P, P], I),
        "qldpc_channel_table": ([P, P, P, I, P], I),
        "qldpc_channel_create": ([P, P, P, P, P, PP], I),
        "qldpc_channel_destroy": ([P], I),
        "qldpc_channel_sample_vec": ([P, ctypes.c_uint64, ctypes.c_uint64, I64, P, P, P, P, I, P], I),
        "qldpc_channel_kernel_name": ([P, P, I, I, I, ctypes.c_char_p, I], I),
        "qldpc_logicals_create": ([P, P, P, P, I, PP], I),
        "qldpc_logicals_destroy": ([P], I),
        "qldpc_count_logical_ex": ([P, P, P, I64, P, P, P, P, I, P, P, I, P, P, P, P, P, P, P, P], I),
        "qldpc_phenom_kernel_name": ([P, I, ctypes.c_char_p, I], I),
        "qldpc_phenom_create": ([P, P, I, PP], I),
        "qldpc_phenom_destroy": ([P], I),
        "qldpc_phenom_sample": ([P, I, D, D, ctypes.c_uint64, ctypes.c_uint64, I64, P, I, P, P, P], I),
        "qldpc_phenom_count": ([P, P, I, I64, P, I, P, P, I, P, P, P, P, P, P], I),
        "qldpc_phenom_window": ([P, I, I64, I, I, I, I, P, I, P, P, I, P, I, I, P, I, P, I, P], I),
        "qldpc_dem_create": ([P, P, I, P, PP], I),
        "qldpc_dem_destroy": ([P], I),
        "qldpc_dem_sample": ([P, ctypes.c_uint64, ctypes.c_uint64, I64, P, I, P, P, P], I),
        "qldpc_dem_count": ([P, I64, P, I, P, P, I, P, P, P, P, P], I),
        "qldpc_dem_kernel_name": ([P, I, ctypes.c_char_p, I], I),
        "qldpc_timing_enable": ([I], I),
        "qldpc_timing_reset": ([], I),
        "qldpc_timing_read": ([P, P], I),
        "qldpc_set_option": ([ctypes.c_char_p, I64], I),
        "qldpc_get_option": ([ctypes.c_char_p, P], I),
    }
    for name, (args, res) in sig.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            if "QLDPC_LIB" in os.environ:       # an older A/B build (tools/build_variants.sh HEAD)
                continue
            raise
        fn.argtypes = args
        fn.restype = res
    return L


lib = _load()


def ptr(a):
    """Raw address of a NumPy array (or None)."""
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data)


def check(rc):
    if rc == QLDPC_OK:
        return
    msg = lib.qldpc_last_error().decode(errors="replace")
    if rc == QLDPC_EINVAL:
        raise ValueError(msg)
    if rc == QLDPC_ERANGE:
        raise IndexError(msg)
    if rc == QLDPC_EUNSUP:
        raise NotImplementedError(msg)
    raise RuntimeError(f"qldpc error {rc}: {msg}")


def device_count():
    return int(lib.qldpc_device_count())


class Schedule:
    """A layer partition bound to a Code (qldpc_schedule)."""

    def __init__(self, code, layer_ptr, layer_rows):
        self.code = code
        self.layer_ptr = np.ascontiguousarray(layer_ptr, dtype=np.int32)
        self.layer_rows = np.ascontiguousarray(layer_rows, dtype=np.int32)
        h = ctypes.c_void_p()
        check(lib.qldpc_schedule_create(code.handle, len(self.layer_ptr) - 1, ptr(self.layer_ptr),
                                        ptr(self.layer_rows), ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_schedule_destroy(h)
            self.handle = None


class Relay:
    """Legs, memory strengths and solution count of a relay min-sum decoder
    bound to a Code (qldpc_relay). `gammas` is float64 [legs, n] in original
    column order. `prior` (a Prior of the same code, or None): the handle
    decodes with relay_vprior_kernel and that row, and
    layout(), kernel_name() and launch_info() describe that kernel."""

    def __init__(self, code, leg_iters, gammas, sols, prior=None):
        self.code = code
        self.prior = prior
        self.leg_iters = np.ascontiguousarray(leg_iters, dtype=np.int32).reshape(-1)
        g = np.ascontiguousarray(gammas, dtype=np.float64)
        if g.ndim != 2 or g.shape[0] != len(self.leg_iters):
            raise ValueError(f"gammas must be float64 [{len(self.leg_iters)}, {code.n}] (one row per leg)")
        self.gammas = g
        self.sols = int(sols)
        h = ctypes.c_void_p()
        check(lib.qldpc_relay_create(code.handle, len(self.leg_iters), ptr(self.leg_iters), ptr(g), g.shape[1],
                                     self.sols, ctypes.byref(h)))
        self.handle = h

    def layout(self):
        """Per-wave LDS layout of the relay kernel (no device needed): bytes of
        the graph image and of a wave's slice, and the offsets inside it."""
        out = np.zeros(7, np.int32)
        check((lib.qldpc_relay_layout if self.prior is None else lib.qldpc_relay_vprior_layout)(self.handle, ptr(out)))
        return dict(zip(("image", "wave_bytes", "off_c2v", "off_synw", "off_m", "off_ew", "off_best"),
                        (int(x) for x in out)))

    def kernel_name(self):
        buf = ctypes.create_string_buffer(128)
        check((lib.qldpc_decode_relay_kernel_name if self.prior is None else
               lib.qldpc_decode_relay_vprior_kernel_name)(self.code.handle, self.handle, buf, 128))
        return buf.value.decode()

    def launch_info(self):
        """(waves per workgroup, workgroups per CU, LDS bytes per workgroup)"""
        w, b, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        check((lib.qldpc_decode_relay_launch_info if self.prior is None else
               lib.qldpc_decode_relay_vprior_launch_info)(self.code.handle, self.handle, ctypes.byref(w),
                                                          ctypes.byref(b), ctypes.byref(l)))
        return w.value, b.value, l.value

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_relay_destroy(h)
            self.handle = None


class Prior:
    """One prior error probability per variable of a Code (qldpc_prior):
    `probs` is float64 [n] in original column order, every 0 <= p_j < 1."""

    def __init__(self, code, probs, eps):
        self.code = code
        self.probs = np.ascontiguousarray(probs, dtype=np.float64)
        if self.probs.shape != (code.n,):
            raise ValueError(f"prior must hold {code.n} probabilities (one per column of H), got shape "
                             f"{self.probs.shape}")
        self.eps = float(eps)
        h = ctypes.c_void_p()
        check(lib.qldpc_prior_create(code.handle, ptr(self.probs), self.eps, ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_prior_destroy(h)
            self.handle = None


class Code:
    """Tanner graph of one parity-check matrix, resident on the current device."""

    def __init__(self, H):
        H = np.asarray(H)
        if H.ndim != 2:
            raise ValueError("H must be a 2-D matrix")
        self.H = (H % 2).astype(np.uint8)
        self.m, self.n = self.H.shape
        h = ctypes.c_void_p()
        Hc = np.ascontiguousarray(self.H)
        check(lib.qldpc_code_create(ptr(Hc), self.m, self.n, ctypes.byref(h)))
        self.handle = h
        self._sched = {}
        self._relay = {}
        self._prior = {}
        self._lock = threading.Lock()

    def prior(self, probs, eps):
        """Cached Prior handle per (probability bytes, eps), as schedules are."""
        a = np.ascontiguousarray(probs, dtype=np.float64)
        key = (a.tobytes(), float(eps))
        with self._lock:
            r = self._prior.get(key)
            if r is None:
                r = Prior(self, a, eps)
                self._prior[key] = r
            return r

    def relay(self, leg_iters, gammas, sols, *, prior=None, eps=1e-9):
        """Cached Relay handle per (leg counts, table bytes, sols), as schedules
        are. `prior` (float64 [n] probabilities, original column order) with
        `eps`: a handle of its own per prior row, bound to self.prior(prior, eps)."""
        key = (np.asarray(leg_iters, np.int32).tobytes(), np.ascontiguousarray(gammas, np.float64).tobytes(),
               int(sols))
        pr = None
        if prior is not None:
            pr = self.prior(prior, eps)
            key += (pr.probs.tobytes(), pr.eps)
        with self._lock:
            r = self._relay.get(key)
            if r is None:
                r = Relay(self, leg_iters, gammas, sols, pr)
                self._relay[key] = r
            return r

    def schedule(self, layer_ptr, layer_rows):
        key = (np.asarray(layer_ptr, np.int32).tobytes(), np.asarray(layer_rows, np.int32).tobytes())
        with self._lock:
            s = self._sched.get(key)
            if s is None:
                s = Schedule(self, layer_ptr, layer_rows)
                self._sched[key] = s
            return s

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            self._sched = {}
            self._relay = {}
            self._prior = {}
            lib.qldpc_code_destroy(h)
            self.handle = None


_code_cache = {}
_code_lock = threading.Lock()


def code_for(H, device_index=None):
    """Cached Code for a matrix (keyed by its bytes and the current device).
    Repeat calls with the same contiguous array hit a cache keyed by a 128-bit
    xxh3 of its raw bytes (~30 us for LP118_2) before the normalising copy
    (mod 2, uint8, tobytes: ~0.7 ms per call, paid per decode launch)."""
    a = np.asarray(H)
    fk = None
    if _xxh is not None and a.flags.c_contiguous:
        fk = (a.shape, a.dtype.str, _xxh.xxh3_128_digest(a), device_index)
        c = _code_fast.get(fk)
        if c is not None:
            return c
    H = np.ascontiguousarray((a % 2).astype(np.uint8))
    key = (H.shape, H.tobytes(), device_index)
    with _code_lock:
        c = _code_cache.get(key)
        if c is None:
            c = Code(H)
            _code_cache[key] = c
        if fk is not None:
            _code_fast[fk] = c
        return c


try:
    import xxhash as _xxh
except ImportError:                                     # the normalising path alone
    _xxh = None
_code_fast = {}


class Logicals:
    """Logical operators (Lx, Lz) of the pair (cx, cz) on the codes' device
    (qldpc_logicals). Keeps both Codes alive."""

    def __init__(self, cx, cz, Lx, Lz):
        self.cx, self.cz = cx, cz
        Lx = np.ascontiguousarray(Lx, dtype=np.uint8)
        Lz = np.ascontiguousarray(Lz, dtype=np.uint8)
        if Lx.ndim != 2 or Lx.shape != Lz.shape or (Lx.shape[0] and Lx.shape[1] != cx.n):
            raise ValueError(f"logical operators must be two [k, {cx.n}] matrices")
        self.k = int(Lx.shape[0])
        self.kw = (self.k + 63) // 64
        h = ctypes.c_void_p()
        check(lib.qldpc_logicals_create(cx.handle, cz.handle, ptr(Lx) if self.k else None,
                                        ptr(Lz) if self.k else None, self.k, ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_logicals_destroy(h)
            self.handle = None


_logicals_cache = {}


def channel_table(px, py, pz):
    """qldpc_channel_table: the draw thresholds uint64 [3, n] of per-qubit
    Pauli probabilities (ValueError unless each is >= 0 and their sum <= 1)."""
    px, py, pz = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (px, py, pz))
    if not (px.shape == py.shape == pz.shape):
        raise ValueError("px, py and pz must have the same length")
    t = np.zeros((3, px.size), np.uint64)
    check(lib.qldpc_channel_table(ptr(px), ptr(py), ptr(pz), px.size, ptr(t)))
    return t


class Channel:
    """Per-qubit Pauli probabilities of the pair (cx, cz) on the codes' device
    (qldpc_channel). Keeps both Codes alive."""

    def __init__(self, cx, cz, px, py, pz):
        self.cx, self.cz = cx, cz
        px, py, pz = (np.ascontiguousarray(a, dtype=np.float64) for a in (px, py, pz))
        if not (px.shape == py.shape == pz.shape == (cx.n,)):
            raise ValueError(f"px, py and pz must each hold {cx.n} probabilities (one per qubit)")
        h = ctypes.c_void_p()
        check(lib.qldpc_channel_create(cx.handle, cz.handle, ptr(px), ptr(py), ptr(pz), ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_channel_destroy(h)
            self.handle = None


class PhenomTable:
    """Logical table L [k, n] of one CSS half on the code's device
    (qldpc_phenom), for qldpc_phenom_count. Keeps the Code alive."""

    def __init__(self, code, L):
        self.code = code
        L = np.ascontiguousarray(np.asarray(L) % 2, dtype=np.uint8)
        if L.ndim != 2 or (L.shape[0] and L.shape[1] != code.n):
            raise ValueError(f"the logical table must be a [k, {code.n}] matrix")
        self.k = int(L.shape[0])
        self.kw = (self.k + 63) // 64
        h = ctypes.c_void_p()
        check(lib.qldpc_phenom_create(code.handle, ptr(L) if self.k else None, self.k, ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_phenom_destroy(h)
            self.handle = None


def phenom_sample(code, rounds, p_data, q, seed, shot0, batch, det, det_fmt, E, fired=None, stream=None):
    """qldpc_phenom_sample on raw device addresses (ints; `fired` may be None)."""
    check(lib.qldpc_phenom_sample(code.handle, int(rounds), float(p_data), float(q), int(seed) & ((1 << 64) - 1),
                                  int(shot0) & ((1 << 64) - 1), int(batch), det, int(det_fmt), E, fired, stream))


def phenom_count(code, table, rounds, batch, det, det_fmt, E, ehat, e_fmt, iters, acc, cls=None, flips=None,
                 resid=None, stream=None):
    """qldpc_phenom_count on raw device addresses (ints; the three per-shot
    outputs may be None)."""
    check(lib.qldpc_phenom_count(code.handle, table.handle, int(rounds), int(batch), det, int(det_fmt), E, ehat,
                                 int(e_fmt), iters, acc, cls, flips, resid, stream))


def phenom_window(code, rounds, batch, done, west, w_fmt, witers, ehat, e_fmt, iters, nxt, det, det_fmt, syn, syn_fmt,
                  stream=None):
    """qldpc_phenom_window on raw device addresses (ints). `done` = (start,
    rounds, closed, commit) of the window just decoded or None; `nxt` = (start,
    rounds) of the next one or None; a window's buffers may be None with it."""
    a, R, closed, C = (int(v) for v in done) if done is not None else (0, 0, 0, 0)
    a2, R2 = (int(nxt[0]), int(nxt[1])) if nxt is not None else (0, 0)
    check(lib.qldpc_phenom_window(code.handle, int(rounds), int(batch), a, R, int(bool(closed)), C, west, int(w_fmt),
                                  witers, ehat, int(e_fmt), iters, a2, R2, det, int(det_fmt), syn, int(syn_fmt),
                                  stream))


class DemTable:
    """A detector error model on the code's device (qldpc_dem): `code` is H's
    Code, L uint8 [K, N] the observables, priors float64 [N]. Keeps the Code
    alive."""

    def __init__(self, code, L, priors):
        self.code = code
        L = np.ascontiguousarray(np.asarray(L) % 2, dtype=np.uint8)
        pr = np.ascontiguousarray(priors, dtype=np.float64)
        if L.ndim != 2 or (L.shape[0] and L.shape[1] != code.n):
            raise ValueError(f"the observable matrix must be a [K, {code.n}] matrix")
        if pr.shape != (code.n,):
            raise ValueError(f"priors must hold {code.n} probabilities (one per column)")
        self.k = int(L.shape[0])
        self.kw = (self.k + 63) // 64
        h = ctypes.c_void_p()
        check(lib.qldpc_dem_create(code.handle, ptr(L) if L.size else None, self.k, ptr(pr) if pr.size else None,
                                   ctypes.byref(h)))
        self.handle = h

    def __del__(self):
        h = getattr(self, "handle", None)
        if h and lib is not None:
            lib.qldpc_dem_destroy(h)
            self.handle = None


def dem_sample(table, seed, shot0, batch, det, det_fmt, obs, fired=None, stream=None):
    """qldpc_dem_sample on raw device addresses (ints; `fired` may be None, and
    `obs` with no observable)."""
    check(lib.qldpc_dem_sample(table.handle, int(seed) & ((1 << 64) - 1), int(shot0) & ((1 << 64) - 1), int(batch),
                               det, int(det_fmt), obs, fired, stream))


def dem_count(table, batch, det, det_fmt, obs, ehat, e_fmt, iters, acc, cls=None, flips=None, stream=None):
    """qldpc_dem_count on raw device addresses (ints; the two per-shot outputs
    may be None)."""
    check(lib.qldpc_dem_count(table.handle, int(batch), det, int(det_fmt), obs, ehat, int(e_fmt), iters, acc, cls,
                              flips, stream))


def dem_kernel_name(table, kind):
    """Name of the detector error model sampler's ("sample") or counter's
    ("count") instance for a DemTable. Needs no device."""
    buf = ctypes.create_string_buffer(128)
    check(lib.qldpc_dem_kernel_name(table.handle, DEM_KERNELS[kind], buf, 128))
    return buf.value.decode()


def logicals_for(Hx, Hz, device_index=None):
    """Cached Logicals of a CSS pair on a device: the operators come from
    logicals.css_logicals, computed and uploaded once per pair."""
    from . import logicals
    cx, cz = code_for(Hx, device_index), code_for(Hz, device_index)
    key = (id(cx), id(cz))
    with _code_lock:
        lg = _logicals_cache.get(key)
    if lg is None:
        Lx, Lz = logicals.css_logicals(Hx, Hz)
        lg = Logicals(cx, cz, Lx, Lz)
        with _code_lock:
            lg = _logicals_cache.setdefault(key, lg)
    return lg


def release_hbm_workspaces():
    """qldpc_schedule_release_workspace on every cached schedule."""
    with _code_lock:
        codes_ = list({id(c): c for c in list(_code_cache.values()) + list(_code_fast.values())}.values())
    for c in codes_:
        with c._lock:
            scheds = list(c._sched.values())
        for s in scheds:
            check(lib.qldpc_schedule_release_workspace(s.handle))


def kernel_name(H, layer_ptr, layer_rows, algo, device_index=None):
    """Name of the decode kernel a launch for (H, schedule, algo) uses (NG /
    BF: the schedule is ignored)."""
    code = code_for(H, device_index)
    if algo in HARD_ALGOS:
        buf = ctypes.create_string_buffer(128)
        check(lib.qldpc_hard_kernel_name(code.handle, ALGO[algo], buf, 128))
        return buf.value.decode()
    sched = code.schedule(layer_ptr, layer_rows)
    buf = ctypes.create_string_buffer(128)
    check(lib.qldpc_decode_kernel_name(code.handle, sched.handle, ALGO[algo], buf, 128))
    return buf.value.decode()


def prior_kernel_name(H, layer_ptr, layer_rows, algo, device_index=None):
    """Name of the kernel a decode with prior_mask launches for (H, schedule,
    algo): decode_prior_kernel<...> (NotImplementedError where it cannot run)."""
    code = code_for(H, device_index)
    sched = code.schedule(layer_ptr, layer_rows)
    buf = ctypes.create_string_buffer(128)
    check(lib.qldpc_decode_prior_kernel_name(code.handle, sched.handle, ALGO[algo], buf, 128))
    return buf.value.decode()


def vprior_kernel_name(H, layer_ptr, layer_rows, algo, device_index=None):
    """Name of the kernel a decode with prior= launches for (H, schedule,
    algo): decode_vprior_kernel<...> (NotImplementedError where it cannot run);
    with option vprior_hbm, hbm_tile_vprior_kernel<...> where that one cannot."""
    code = code_for(H, device_index)
    sched = code.schedule(layer_ptr, layer_rows)
    buf = ctypes.create_string_buffer(128)
    check(lib.qldpc_decode_vprior_kernel_name(code.handle, sched.handle, ALGO[algo], buf, 128))
    return buf.value.decode()


CHANNEL_KERNELS = {"sample": 0, "sample_vec": 1, "count": 2, "count_logical": 3}     # QLDPC_CHANNEL_*
PHENOM_KERNELS = {"sample": 0, "count": 1}                                            # QLDPC_PHENOM_*
DEM_KERNELS = {"sample": 0, "count": 1}                                               # QLDPC_DEM_*


def channel_kernel_name(Hx, Hz, kind, est_aligned=True, tabs_lds=False, device_index=None):
    """Name of the kernel instance the device sampler ("sample", with
    per-qubit thresholds "sample_vec") or an outcome counter ("count",
    "count_logical") launches for the pair. est_aligned: both byte-estimate
    bases are 4-byte aligned; tabs_lds: the logical tables' residency. Needs
    no device."""
    cx, cz = code_for(Hx, device_index), code_for(Hz, device_index)
    buf = ctypes.create_string_buffer(128)
    check(lib.qldpc_channel_kernel_name(cx.handle, cz.handle, CHANNEL_KERNELS[kind], int(bool(est_aligned)),
                                        int(bool(tabs_lds)), buf, 128))
    return buf.value.decode()


def phenom_kernel_name(H, kind, device_index=None):
    """Name of the phenomenological sampler's ("sample") or counter's
    ("count") instance for the half H. Needs no device."""
    buf = ctypes.create_string_buffer(128)
    check(lib.qldpc_phenom_kernel_name(code_for(H, device_index).handle, PHENOM_KERNELS[kind], buf, 128))
    return buf.value.decode()


def launch_info(H, layer_ptr, layer_rows, algo, device_index=None):
    """(waves per workgroup, workgroups per CU, LDS bytes per workgroup) of
    that kernel's launch; zeros for the HBM-resident kernel."""
    code = code_for(H, device_index)
    w, b, l = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if algo in HARD_ALGOS:
        check(lib.qldpc_hard_launch_info(code.handle, ALGO[algo], ctypes.byref(w), ctypes.byref(b), ctypes.byref(l)))
        return w.value, b.value, l.value
    sched = code.schedule(layer_ptr, layer_rows)
    check(lib.qldpc_decode_launch_info(code.handle, sched.handle, ALGO[algo], ctypes.byref(w), ctypes.byref(b),
                                       ctypes.byref(l)))
    return w.value, b.value, l.value


def timing_enable(on=True):
    check(lib.qldpc_timing_enable(1 if on else 0))


def timing_reset():
    check(lib.qldpc_timing_reset())


def timing_read():
    ms = ctypes.c_double()
    n = ctypes.c_int64()
    check(lib.qldpc_timing_read(ctypes.byref(ms), ctypes.byref(n)))
    return ms.value, n.value


# ---------------------------------------------------------------------------
# library options (qldpc_set_option): which kernel family decodes. The
# library never reads the environment; QLDPC_OPTIONS="name=value,..." is
# applied once here, at import (A/B tools start one process per setting).
# ---------------------------------------------------------------------------
def set_option(name, value):
    check(lib.qldpc_set_option(name.encode(), int(value)))


def get_option(name):
    v = ctypes.c_int64()
    check(lib.qldpc_get_option(name.encode(), ctypes.byref(v)))
    return v.value


@contextlib.contextmanager
def options(**kw):
    """Set library options for the duration of a block, e.g.
    `with options(force_hbm=1): ...`; the previous values come back after."""
    old = {k: get_option(k) for k in kw}
    try:
        for k, v in kw.items():
            set_option(k, v)
        yield
    finally:
        for k, v in old.items():
            set_option(k, v)


for _kv in filter(None, os.environ.get("QLDPC_OPTIONS", "").split(",")):
    _k, _, _v = _kv.partition("=")
    set_option(_k.strip(), int(_v or 1))

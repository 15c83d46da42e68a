"""The host path of the device OSD (capi_osd_device.cpp), pinned without a GPU:
the kernel name qldpc_osd_kernel_name answers for the fourteen matrices of
osd_shape_codes (both methods, options osd_column and osd_hbm), the code and
message of every refusal the eight entry points make before their first HIP
call, in the order they make them, and the LDS size functions of osd_kernels.h
against integers recorded from the sums they replaced."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import osd_shape_codes as S
from qldpcsim_amd import _lib

L = _lib.lib
P = _lib.ptr
OK, EINVAL, EUNSUP, EHIP = _lib.QLDPC_OK, _lib.QLDPC_EINVAL, _lib.QLDPC_EUNSUP, _lib.QLDPC_EHIP
NO_DEVICE = _lib.device_count() == 0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MSG_NO_DEVICE = "no HIP device was visible when the code was created"
MSG_CS = "OSD-CS on the device needs "
WHY_RANGE = MSG_CS + "m <= 512 and n <= 1087 (the block kernel's range)"
WHY_ZERO = MSG_CS + "an H without all-zero columns"
WHY_OPTS = MSG_CS + "options osd_column and osd_hbm off"
MSG_ORDER_N = "the device reliability order supports 1 <= n <= 2048 (got %d)"

# id -> NW of the instance (0: more than 33 row words), the block kernel's row
# slots as the launcher formed them, CPython's set table for n keys (ints), and
# the launcher's hand-written sums before they became osd_column_lds (col),
# osd_block_lds (blk) and osd_block_cs_room (room), for orders 0 and 1
LDS = {
    "b4w1": dict(nw=4, mr=64, table=640, col0=2816, blk0=7280, col1=5376, blk1=9840, room=4608),
    "b9w3": dict(nw=9, mr=192, table=640, col0=4472, blk0=15000, col1=7032, blk1=17560, room=10496),
    "b4r2": dict(nw=4, mr=384, table=640, col0=3728, blk0=17152, col1=6288, blk1=19712, room=9728),
    "b9r2": dict(nw=9, mr=384, table=2560, col0=6584, blk0=22488, col1=16824, blk1=32728, room=13568),
    "b17r1": dict(nw=17, mr=256, table=2560, col0=8824, blk0=25112, col1=19064, blk1=35352, room=17664),
    "b17max": dict(nw=17, mr=512, table=2560, col0=12408, blk0=35864, col1=22648, blk1=46104, room=21760),
    "st3": dict(nw=17, mr=256, table=2560, col0=9400, blk0=25688, col1=19640, blk1=35928, room=17664),
    "win3": dict(nw=17, mr=256, table=2560, col0=9816, blk0=26104, col1=20056, blk1=36344, room=17664),
    "c17w9": dict(nw=17, mr=640, table=2560, col0=9976, blk0=37016, col1=20216, blk1=47256, room=23808),
    "c33min": dict(nw=33, mr=128, table=2560, col0=15240, blk0=35880, col1=25480, blk1=46120, room=27904),
    "st5": dict(nw=33, mr=448, table=2560, col0=17128, blk0=46728, col1=27368, blk1=56968, room=33024),
    "c33max": dict(nw=33, mr=1024, table=10240, col0=24056, blk0=69784, col1=65016, blk1=110744, room=42240),
    "h_m": dict(nw=33, mr=1088, table=2560, col0=19000, blk0=66520, col1=29240, blk1=76760, room=43264),
    "h_n": dict(nw=0, mr=256, table=10240, col0=11520, blk0=19376, col1=52480, blk1=60336, room=4608),
}


def _err():
    return L.qldpc_last_error().decode()


def _name(code, cs):
    buf = ctypes.create_string_buffer(128)
    rc = L.qldpc_osd_kernel_name(code.handle if code else None, cs, buf, 128)
    return (rc, buf.value.decode()) if rc == OK else (rc, _err())


def _zero_col():
    H = np.array(S.matrix("b4w1"))
    H[:, 7] = 0
    return H


@pytest.mark.parametrize("name", S.IDS)
def test_kernel_names(name):
    code = _lib.Code(S.matrix(name))
    block, hbm = name in S.BLOCK_IDS, S.CASES[name]["kernel"] == "osd_hbm_kernel"
    assert _name(code, 0) == (OK, S.CASES[name]["kernel"])
    assert _name(code, 1) == ((OK, S.cs_kernel(name)) if block else (EUNSUP, WHY_RANGE))
    with _lib.options(osd_column=1):
        assert _name(code, 0) == (OK, "osd_hbm_kernel" if hbm else S.COL % LDS[name]["nw"])
        assert _name(code, 1) == (EUNSUP, WHY_OPTS if block else WHY_RANGE)
    with _lib.options(osd_hbm=1):
        assert _name(code, 0) == (OK, "osd_hbm_kernel")
        assert _name(code, 1) == (EUNSUP, WHY_OPTS if block else WHY_RANGE)
    assert _lib.get_option("osd_column") == 0 and _lib.get_option("osd_hbm") == 0


def test_kernel_name_arguments_and_zero_column():
    code = _lib.Code(_zero_col())
    assert _name(code, 0) == (OK, "osd_kernel<4>")         # (b4w1 is osd_block_kernel<4, 4, 1> otherwise)
    assert _name(code, 1) == (EUNSUP, WHY_ZERO)
    with _lib.options(osd_column=1):                       # the zero column is reported ahead of the options
        assert _name(code, 1) == (EUNSUP, WHY_ZERO)
    assert _name(None, 0) == (EINVAL, "null argument")
    assert L.qldpc_osd_kernel_name(code.handle, 0, None, 128) == EINVAL and _err() == "null argument"
    assert L.qldpc_osd_kernel_name(code.handle, 0, ctypes.create_string_buffer(8), 0) == EINVAL
    assert _err() == "null argument"


class _Entries:
    """The seven launching entry points on one code with null device buffers
    (every call here is refused, or has nothing to do, before a launch)."""

    def __init__(self, code):
        self.code = code                                     # (keeps the handle alive)
        self.h = code.handle if code is not None else None

    def device(self, count=1, order=0):
        return L.qldpc_osd_device(self.h, count, None, None, order, None, None, None)

    def device_cs(self, count=1, lam=10):
        return L.qldpc_osd_device_cs(self.h, count, None, None, lam, None, None, None)

    def order(self, count=1, bufs=(None, None, None)):
        return L.qldpc_osd_order_device(self.h, count, *bufs, None)

    def ordered(self, count=1, order=0):
        return L.qldpc_osd_device_ordered(self.h, count, None, None, order, None, None, None, None, None)

    def ordered_cs(self, count=1, lam=10):
        return L.qldpc_osd_device_ordered_cs(self.h, count, None, None, lam, None, None, None, None, None)

    def ordered_ex(self, count=1, spill=(None, None, None, 0)):
        return L.qldpc_osd_device_ordered_ex(self.h, count, None, None, 0, None, None, None, None, *spill, None)

    def ordered_ex_cs(self, count=1, lam=10, spill=(None, None, None, 0)):
        return L.qldpc_osd_device_ordered_ex_cs(self.h, count, None, None, lam, None, None, None, None, *spill, None)

    def plain(self):
        return (self.device, self.order, self.ordered, self.ordered_ex)

    def cs(self):
        return (self.device_cs, self.ordered_cs, self.ordered_ex_cs)


def test_refusals_null_code_lambda_count():
    e, none = _Entries(_lib.Code(S.matrix("b4w1"))), _Entries(None)
    for call in none.plain() + none.cs():
        assert (call(), _err()) == (EINVAL, "code is null")
        assert (call(count=-1), _err()) == (EINVAL, "code is null")
    # lambda outside 0..64: ahead of the null code, the OSD-CS refusal and the counts
    big = _Entries(_lib.Code(S.matrix("c17w9")))
    for lam in (-1, -7, 65, 1 << 20):
        for who in (e, none, big):
            for call in who.cs():
                for count in (1, 0, -1):
                    assert (call(count=count, lam=lam), _err()) == \
                        (EINVAL, f"OSD-CS lambda must lie in 0..64 (got {lam})")
    for call in e.plain() + e.cs():
        assert (call(count=-1), _err()) == (EINVAL, "negative count")
        assert call(count=0) == OK
    for lam in (0, 64):
        for call in e.cs():
            assert call(count=0, lam=lam) == OK
    # past the counts: the device the code was created on, then the buffers
    late = (EHIP, MSG_NO_DEVICE) if NO_DEVICE else (EINVAL, "null device buffer")
    for call in e.plain() + e.cs():
        assert (call(), _err()) == late


def test_refusals_osd_cs():
    """m > 512, n > 1087, a zero column and each option: before the counts, and
    in the _ordered entries before the order kernel's own checks."""
    cases = [(_lib.Code(S.matrix("c17w9")), {}, WHY_RANGE), (_lib.Code(S.matrix("c33min")), {}, WHY_RANGE),
             (_lib.Code(_zero_col()), {}, WHY_ZERO), (_lib.Code(S.matrix("b4w1")), dict(osd_column=1), WHY_OPTS),
             (_lib.Code(S.matrix("b4w1")), dict(osd_hbm=1), WHY_OPTS),
             (_lib.Code(S.matrix("h_n")), dict(osd_hbm=1), WHY_RANGE)]
    for code, opts, why in cases:
        e = _Entries(code)
        with _lib.options(**opts):
            for call in e.cs():
                for count in (1, 0, -1):
                    assert (call(count=count), _err()) == (EUNSUP, why)
            # the reference method is not refused: the same codes and options have a kernel
            for call in e.plain():
                assert call(count=0) == OK
    assert _lib.get_option("osd_column") == 0 and _lib.get_option("osd_hbm") == 0


def test_refusals_spill_and_order_range():
    cnt, post, idx = np.zeros(1, np.int32), np.zeros(4, np.float64), np.zeros(4, np.int32)
    big = _lib.Code(S.matrix("c17w9"))
    for who in (_Entries(_lib.Code(S.matrix("b4w1"))), _Entries(None), _Entries(big)):
        for call in (who.ordered_ex, who.ordered_ex_cs):
            # incomplete spill buffers: ahead of the null code and the OSD-CS refusal
            for spill in ((None, P(idx), P(cnt), 4), (P(post), None, P(cnt), 4), (P(post), P(idx), P(cnt), -1)):
                for count in (1, 0, -1):
                    assert (call(count=count, spill=spill), _err()) == (EINVAL, "spill buffers incomplete")
            assert (call(count=1 << 31, spill=(P(post), P(idx), P(cnt), 4)), _err()) == \
                (EINVAL, "spill indices are int32")
        # the lambda range comes first of all
        assert (who.ordered_ex_cs(lam=65, spill=(None, None, P(cnt), 4)), _err()) == \
            (EINVAL, "OSD-CS lambda must lie in 0..64 (got 65)")
    # n > 2048: the order entries refuse behind the device and buffer checks,
    # before any launch (the buffers only have to be non-null)
    wide = _Entries(_lib.Code(S.matrix("h_n")))
    late = (EHIP, MSG_NO_DEVICE) if NO_DEVICE else (EUNSUP, MSG_ORDER_N % 2112)
    assert (wide.order(bufs=(P(post), P(idx), P(cnt))), _err()) == late
    assert wide.order(count=0) == OK and wide.ordered(count=0) == OK
    assert (wide.order(count=-1), _err()) == (EINVAL, "negative count")


@pytest.fixture(scope="module")
def lds_lib(tmp_path_factory):
    """osd_kernels.h's inline size functions behind a C ABI (host compiler, no device code)."""
    d = tmp_path_factory.mktemp("osd_lds")
    src, so = d / "osd_lds.cpp", d / "osd_lds.so"
    src.write_text('#include "osd_kernels.h"\n'
                   'extern "C" {\n'
                   "long long col(int m, int n, int nw, int t) { return (long long)qldpc::osd_column_lds(m, n, nw, t); }\n"
                   "long long blk(int m, int n, int nw, int mr, int t) { return (long long)qldpc::osd_block_lds(m, n, nw, mr, t); }\n"
                   "long long room(int nw, int mr) { return (long long)qldpc::osd_block_cs_room(nw, mr); }\n"
                   "long long cs(int nw, int mr) { return (long long)qldpc::osd_cs_lds(nw, mr); }\n"
                   "}\n")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "qldpcsim_amd", "csrc"),
                    str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    for f in (lib.col, lib.blk, lib.room, lib.cs):
        f.restype = ctypes.c_longlong
    return lib


@pytest.mark.parametrize("name", S.IDS)
def test_lds_sizes(lds_lib, name):
    c, w = S.CASES[name], LDS[name]
    for order in (0, 1):
        t = w["table"] if order == 1 else 0
        assert lds_lib.col(c["m"], c["n"], w["nw"], t) == w[f"col{order}"]
        assert lds_lib.blk(c["m"], c["n"], w["nw"], w["mr"], t) == w[f"blk{order}"]
    assert lds_lib.room(w["nw"], w["mr"]) == w["room"]
    # the OSD-CS epilogue fits the room it is given (the launcher's check)
    assert lds_lib.cs(w["nw"], w["mr"]) <= w["room"]

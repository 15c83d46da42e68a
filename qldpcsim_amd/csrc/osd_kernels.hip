// osd_kernels.hip — batched OSD post-decoding on MI355X (gfx950).
//
// Replaces OSDdec (qLDPCsim/decoders.py:299-370) with its gf2math.rank /
// gf2math.REF calls (gf2math.py:91-187) for a batch of non-converged shots.
// One workgroup = one shot; thread t owns row t of the column-permuted matrix
// Hp = H[:, perm] (perm = the reliability order, computed by the caller with
// NumPy exactly as decoders.py:320-325), held bit-packed in VGPRs, with the
// syndrome as an augmented column.
//
// Equivalences used (OSD):
//  * Gaussian elimination over the columns of Hp in order, pivot = first row at
//    or below the current pivot row holding a 1 (gf2math.REF's rule), finds a
//    pivot exactly in the columns that raise the rank — the greedy
//    complementary information set J of decoders.py:329-342 (plus column 0,
//    which the reference takes unconditionally).
//  * Non-pivot columns cause no row operation, so the row operations equal
//    those of REF(Hp[:, J], reduced=True); applied to the augmented syndrome
//    they give T @ s. With R = T @ Hp: T @ sJ = T @ s + R[:, I] @ e_I (mod 2),
//    so e_J = (T @ sJ)[:|J|] (decoders.py:352-358) needs one elimination.
//  * Order semantics with the reference's aliasing: order 1
//    flips e_perm[infoSet[0]] (CPython set order, emulated), order >= 2 is
//    order 0.
//
// One translation unit for every OSD kernel, one header per family over
// osd_common.h; here the selectors (pointer and name, as rocprofv3 prints it)
// and the order kernel's launcher. capi_osd_device.cpp chooses (choose_osd_kernel).
#include "osd_column.h"
#include "osd_block.h"
#include "osd_order.h"
#include "osd_hbm.h"
#include "wave_common.h"

namespace qldpc {
size_t osd_order_lds(int n) { return (size_t)8 * n + 96 * 4 + 512 * 2 + 16; }

hipError_t launch_osd_order(const OrderArgs& a, long long count, hipStream_t stream) {
  const void* k = a.n <= 256 ? (const void*)&osd_order_kernel<4>
                : a.n <= 512 ? (const void*)&osd_order_kernel<8>
                : a.n <= 1024 ? (const void*)&osd_order_kernel<16>
                : (const void*)&osd_order_kernel<32>;
  long long done = 0;
  while (done < count) {
    const long long g = count - done < (1ll << 30) ? count - done : (1ll << 30);
    OrderArgs ai = a;
    ai.post = a.post + done * a.n;
    ai.perm = a.perm + done * a.n;
    ai.tiepos = a.tiepos + done;
    void* params[] = {(void*)&ai};
    hipError_t e = hipLaunchKernel(k, dim3((unsigned)g), dim3(64), params, osd_order_lds(a.n), stream);
    if (e != hipSuccess) return e;
    done += g;
  }
  return hipSuccess;
}

int osd_nw_of(int words) { return words <= 4 ? 4 : words <= 9 ? 9 : words <= 17 ? 17 : words <= 33 ? 33 : 0; }

const void* select_osd_kernel(int nw, const char** name) {
#define QLDPC_OSD_COL(NW) if (nw > 0 && nw <= NW) QLDPC_NAMED((&osd_kernel<NW>), "osd_kernel<" #NW ">");
  QLDPC_OSD_COL(4) QLDPC_OSD_COL(9) QLDPC_OSD_COL(17) QLDPC_OSD_COL(33)
#undef QLDPC_OSD_COL
  return nullptr;                                   // (osd_nw_of: more than 33 words)
}

const void* osd_hbm_kernel_ptr(const char** name) { QLDPC_NAMED((&osd_hbm_kernel), "osd_hbm_kernel"); }

// block kernel configurations whose state fits the VGPR budget without
// spills (m <= 512 rows, n <= 1087 columns): SL = 4 engine slots and one row
// per thread up to 256 rows, SL = 8 and two rows per thread up to 512; null ->
// osd_kernel (the engine state would spill). cs: the OSD-CS instance of the
// same configuration, with the Hamming (kOsdCsHamming) or the prior cost (kOsdCsPrior)
const void* select_osd_block_kernel(int nw, int m, int cs, int* rows_per_thread, const char** name) {
#define QLDPC_OSD_BLK(NW, SL, RT)                                                                                 \
  if (nw > 0 && nw <= NW && m <= 64 * SL) {                                                                       \
    *rows_per_thread = RT;                                                                                        \
    if (cs == kOsdCsPrior)                                                                                        \
      QLDPC_NAMED((&osd_block_cs_prior_kernel<NW, SL, RT>), "osd_block_cs_prior_kernel<" #NW ", " #SL ", " #RT ">"); \
    if (cs) QLDPC_NAMED((&osd_block_cs_kernel<NW, SL, RT>), "osd_block_cs_kernel<" #NW ", " #SL ", " #RT ">");    \
    QLDPC_NAMED((&osd_block_kernel<NW, SL, RT>), "osd_block_kernel<" #NW ", " #SL ", " #RT ">");                  \
  }
  QLDPC_OSD_BLK(4, 4, 1) QLDPC_OSD_BLK(4, 8, 2)
  QLDPC_OSD_BLK(9, 4, 1) QLDPC_OSD_BLK(9, 8, 2)
  QLDPC_OSD_BLK(17, 4, 1) QLDPC_OSD_BLK(17, 8, 2)
#undef QLDPC_OSD_BLK
  return nullptr;
}

}  // namespace qldpc

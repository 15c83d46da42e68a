// ms_flood_kernels.hip — the flooding min-sum kernel (ms_flood_kernel,
// ms_flood.h; the headline decoder) instantiated in a translation
// unit of its own, built with the AMDGPU max-ILP machine scheduler
// (-mllvm -amdgpu-sched-strategy=max-ilp, Makefile): 46.66 -> 46.04 ms per
// LP118_0 fixed-work launch; the same strategy slows the layered min-sum
// (+1.3 %), BP (+0.4 / +3.6 %) and OSD (+0.2 %) kernels, which keep the
// default. profiles/r06/r06p_ab_sched_strategies.json. Re-examined for the
// register-resident body (ms_flood_qc.h): 33.59 ms with max-ilp against 33.81
// with the default scheduler (make FLOOD_SCHED=; profiles/r07a/); and for its
// per-variable float64 posteriors: 30.94 against 30.97 ms (medians of 5, the
// ranges overlap; profiles/r08a/); and with the check node's sign word formed
// ahead of the tournament: 30.53 against 31.09 ms (profiles/r09a/), so
// max-ilp stays. (The float32-domain check node, -DQLDPC_QC_CN32, spills
// under it and was timed with the default scheduler, make FLOOD_SCHED=.)
#include "ms_flood.h"

namespace qldpc {

const void* select_ms_flood_kernel(int dc, int kc, const char** name) {
  // instantiated (DC, KC) shapes; the host passes ceil(m/64) checks per lane
  if (dc == 7 && kc <= 2) QLDPC_NAMED((&ms_flood_kernel<7, 2>), "ms_flood_kernel<7, 2>");
  if (dc == 8 && kc <= 2) QLDPC_NAMED((&ms_flood_kernel<8, 2>), "ms_flood_kernel<8, 2>");
  if (dc == 7 && kc <= 4) QLDPC_NAMED((&ms_flood_kernel<7, 4>), "ms_flood_kernel<7, 4>");
  if (dc == 8 && kc <= 4) QLDPC_NAMED((&ms_flood_kernel<8, 4>), "ms_flood_kernel<8, 4>");
  if (dc == 7 && kc <= 8) QLDPC_NAMED((&ms_flood_kernel<7, 8>), "ms_flood_kernel<7, 8>");
  if (dc == 8 && kc <= 8) QLDPC_NAMED((&ms_flood_kernel<8, 8>), "ms_flood_kernel<8, 8>");
  return nullptr;
}

bool ms_flood_kernel_is_qc(int dc, int kc) {
  if (dc == 7) return kc <= 2 ? ms_flood_is_qc<7, 2>() : kc <= 4 ? ms_flood_is_qc<7, 4>() : ms_flood_is_qc<7, 8>();
  if (dc == 8) return kc <= 2 ? ms_flood_is_qc<8, 2>() : kc <= 4 ? ms_flood_is_qc<8, 4>() : ms_flood_is_qc<8, 8>();
  return false;
}

const void* select_ms_flood_lds_kernel(int dc, int kc, const char** name) {
  // the LDS twins of the register-resident shapes
  if (dc == 8 && kc > 2 && kc <= 4) QLDPC_NAMED((&ms_flood_lds_kernel<8, 4>), "ms_flood_lds_kernel<8, 4>");
  return nullptr;
}

}  // namespace qldpc

// bp_team_kernels.hip — the sum-product team kernels (bp_team_kernel,
// bp_team_lg_kernel, bp_team.h) instantiated in a translation unit
// of their own, built with -fno-slp-vectorize (Makefile): the SLP vectorizer
// packed pairs of their float64 / index operations with register moves
// between, measured 1.4 % slower per LP118_2 BP-L launch and 1.2 % per LP118_0
// BP-F launch; the min-sum kernels keep it (the layered one is 0.3 % faster
// with it). profiles/r06/r06l_ab_noslp.json.
#include "bp_team.h"

namespace qldpc {

const void* select_bp_team_kernel(bool layered, int dc, int w, const char** name) {
#define QLDPC_BPT(L, D, Wn) \
  if (layered == L && dc == D && w == Wn) QLDPC_NAMED((&bp_team_kernel<L, D, Wn>), "bp_team_kernel<" #L ", " #D ", " #Wn ">");
  QLDPC_BPT(false, 7, 4) QLDPC_BPT(false, 8, 4) QLDPC_BPT(true, 7, 4) QLDPC_BPT(true, 8, 4)
  QLDPC_BPT(false, 7, 8) QLDPC_BPT(false, 8, 8) QLDPC_BPT(true, 7, 8) QLDPC_BPT(true, 8, 8)
#undef QLDPC_BPT
  return nullptr;
}

const void* select_bp_team_lg_kernel(int dc, int w, const char** name) {
  if (dc == 7 && w == 4) QLDPC_NAMED((&bp_team_lg_kernel<7, 4>), "bp_team_lg_kernel<7, 4>");
  if (dc == 8 && w == 4) QLDPC_NAMED((&bp_team_lg_kernel<8, 4>), "bp_team_lg_kernel<8, 4>");
  if (dc == 7 && w == 8) QLDPC_NAMED((&bp_team_lg_kernel<7, 8>), "bp_team_lg_kernel<7, 8>");
  if (dc == 8 && w == 8) QLDPC_NAMED((&bp_team_lg_kernel<8, 8>), "bp_team_lg_kernel<8, 8>");
  return nullptr;
}

}  // namespace qldpc

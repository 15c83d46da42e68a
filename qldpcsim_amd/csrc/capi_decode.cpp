// capi_decode.cpp — the soft decoders (MS, BP): kernel choice, LDS layouts and
// launch plans, the decode entry points (scalar, two-level and per-variable
// priors; device and host buffers) and the HBM-resident path. The plumbing
// shared with the other families is in capi_launch.h.

#include <cmath>
#include <cstdio>
#include <memory>

#include "capi_launch.h"
#include "../../include/qldpc_libm.h"   // after hip_runtime.h
#include "qc_tables.h"
#include "tuning.h"

using namespace capi;
using qldpc::DecodeArgs;

// ---------------------------------------------------------------------------
// launch plan, device-free half: which kernel, and its static arguments
// ---------------------------------------------------------------------------
// per-wave state slice: post f64[n] | c2v (f32|f64)[E] | syn words | parity words
// (flooding: no parity words, and syndrome words only past the register of the
// generic kernels, QLDPC_SYNREG_CHECKS;
// ms_layered_kernel, colsum_f32: the "parity words" slot holds the syndrome
// bits in layer order instead, 2 ceil(synl_rows / 64) words; the lane-group
// instance <DC, 0> only; decode_prior_kernel: selector words behind them)
static void wave_layout(const qldpc_code* c, bool layered, int algo, bool colsum_f32, int synl_rows, bool prior,
                        DecodeArgs* a) {
  int off = align16((colsum_f32 ? 4 : 8) * c->n);   // post f64, or ms_layered_kernel's float32 sums
  a->off_c2v = off;
  off = align16(off + (algo == QLDPC_ALGO_MS ? 4 : 8) * (c->E + 8));  // +8: VN over-read pad
  const int words = 2 * ((c->m + 63) / 64);
  a->off_synw = off;
  // (flooding: the generic kernels hold the bits in a register up to
  // QLDPC_SYNREG_CHECKS checks, so no existing slice grows; the *_tall ones read these)
  if (layered || c->m > QLDPC_SYNREG_CHECKS) off = align16(off + 4 * words);
  a->off_parw = off;
  if (layered && !colsum_f32) off = align16(off + 4 * words);
  if (layered && colsum_f32) off = align16(off + 4 * 2 * ((synl_rows + 63) / 64));
  a->off_selw = off;
  if (prior) off = align16(off + 4 * 2 * ((c->n + 63) / 64));
  a->wave_bytes = std::max(off, 16);
}

// bp_team_kernel's slice: post f64[n] | c2v f64[E + 8] | syn words | parity
// words | reduction slots ([2][W] any-flags, [2][2] tickets)
static void team_layout(const qldpc_code* c, int w, DecodeArgs* a) {
  int off = align16(8 * c->n);
  a->off_c2v = off;
  off = align16(off + 8 * (c->E + 8));
  const int words = 2 * ((c->m + 63) / 64);
  a->off_synw = off;
  off = align16(off + 4 * words);
  a->off_parw = off;
  off = align16(off + 4 * words);
  a->off_red = off;
  off = align16(off + 4 * (3 * w + 4));   // + [W] filter words (layered stop test)
  a->wave_bytes = off;
}

// H's CSR (np.where order: ascending columns within a row) against table T
// expanded: row 16 b + r holds columns 16 cvar[b][e] + (r + cshift[b][e]) % 16
template <typename T>
static bool qc_table_matches(const qldpc_code* c) {
  constexpr int lift = qldpc::qc::kLift;
  if (c->m != lift * T::MB || c->n != lift * T::NB || c->E != lift * T::MB * T::DC) return false;
  for (int b = 0; b < T::MB; ++b)
    for (int r = 0; r < lift; ++r) {
      const int row = lift * b + r;
      if (c->row_ptr[row + 1] - c->row_ptr[row] != T::DC) return false;
      int cols[T::DC];
      for (int e = 0; e < T::DC; ++e) cols[e] = lift * T::cvar[b][e] + (r + T::cshift[b][e]) % lift;
      std::sort(cols, cols + T::DC);
      for (int e = 0; e < T::DC; ++e)
        if (c->col_idx[c->row_ptr[row] + e] != cols[e]) return false;
    }
  return true;
}

int capi::qc_table_of(const qldpc_code* c) {
#define QLDPC_QC_MATCH(ID, T, NAME) \
  if (qc_table_matches<T>(c)) return ID;
  QLDPC_QC_TABLES(QLDPC_QC_MATCH)
#undef QLDPC_QC_MATCH
  return -1;
}

// flooding past the syndrome register of the generic LDS kernels: the *_tall
// instances (such a code has no fast table: 8 E < 65536 caps it at 1170 checks)
static bool flooding_tall(const qldpc_schedule* s) { return !s->layered && s->code->m > QLDPC_SYNREG_CHECKS; }

KernelChoice capi::choose_kernel(const qldpc_schedule* s, int algo) {
  const qldpc_code* c = s->code;
  const int dc = fast_table_ok(c) ? c->uniform_deg : 0;
  KernelChoice k;
  k.max_waves = QLDPC_MAX_THREADS / 64;
  if (algo == QLDPC_ALGO_MS && !s->layered && dc > 0 && !s->flood_ms.empty() && !opt(&Options::flood_generic)) {
    const int kc = (c->m + 63) / 64;
    k.kernel = qldpc::select_ms_flood_kernel(dc, kc, &k.name);
    if (k.kernel) {
      k.family = FAM_MS_FLOOD;
      k.max_waves = qldpc::ms_flood_max_waves(kc);
    }
    if (k.kernel && qldpc::ms_flood_kernel_is_qc(dc, kc)) {
      // this shape's ms_flood_kernel is the register-resident kernel of the
      // generated tables: for a code that is exactly one of them (option
      // flood_qc = 0: never); every other code of the shape runs the LDS twin
      k.qc_table = opt(&Options::flood_qc) ? qc_table_of(c) : -1;
      if (k.qc_table >= 0) {
        k.family = FAM_MS_FLOOD_QC;
      } else {
        k.kernel = qldpc::select_ms_flood_lds_kernel(dc, kc, &k.name);
        if (!k.kernel) k.family = FAM_GENERIC, k.max_waves = QLDPC_MAX_THREADS / 64;
      }
    }
  }
  if (!k.kernel && algo == QLDPC_ALGO_MS && s->layered && dc > 0 && !s->layered_ms.empty() &&
      !opt(&Options::layered_generic)) {
    // lanes per check: one template width when every layer wants the same
    // (8 for one- or two-row layers of serial schedules, else one: interleaved
    // A/B, DESIGN.md §3.2: wider groups lost on 7-60-row layers), else chosen
    // per layer (the runtime switch costs ~5 % where it is not needed)
    k.lanes = s->layer_g > 0 ? s->layer_g : 0;
    if (const int64_t og = opt(&Options::ms_lanes_per_check)) k.lanes = (int)og;
    // (several half-shots per wave, ms_layered_grp_kernel, measured 2x slower
    // in round 2: at a fixed LDS budget it halves the waves per CU; removed)
    k.kernel = qldpc::select_ms_layered_kernel(dc, k.lanes, &k.name);
    if (k.kernel) k.family = FAM_MS_LAYERED;
  }
  if (!k.kernel && algo == QLDPC_ALGO_BP && dc > 0 && !opt(&Options::bp_wave)) {
    // 4 waves per half-shot; 8 when a team's LDS footprint leaves at most 3
    // teams per CU (LP118_2: 67 KB), so a CU still runs >= 16 waves
    DecodeArgs t4{};
    team_layout(c, 4, &t4);
    k.team = (s->generic.lds_bytes + t4.wave_bytes > 48 * 1024) ? 8 : 4;
    // Layered: 4-wave teams with every graph table in global memory
    // (bp_team_lg_kernel): LDS holds only the team's state, so a CU runs 4
    // teams (the VGPR cap of 16 team waves) — LP118_2: 2 teams with all-LDS
    // tables, 3 with the row table alone global; the kernel is barrier /
    // latency-bound and BP-L p = 0.1 ran 175 -> 132 -> 108 ms per launch.
    // Schedules without the global image (n > 2048, a column degree > 31) run
    // the all-LDS team kernel; option bp_lg = 0 forces it (tests).
    const bool tlg = s->layered && !s->layered_bp.empty() && opt(&Options::bp_lg) != 0;
    if (tlg) k.team = 4;
    if (const int64_t ow = opt(&Options::bp_team_w)) k.team = (int)ow;
    if (tlg) {
      k.kernel = qldpc::select_bp_team_lg_kernel(dc, k.team, &k.name);
      if (k.kernel) k.family = FAM_BP_TEAM_LG;
    }
    if (!k.kernel) {
      k.kernel = qldpc::select_bp_team_kernel(s->layered, dc, k.team, &k.name);
      if (k.kernel) k.family = FAM_BP_TEAM;
    }
    if (!k.kernel) k.team = 0;
  }
  if (!k.kernel) k.kernel = qldpc::select_kernel(algo, s->layered, dc, flooding_tall(s), &k.name);
  return k;
}

// what both prior twins of the generic LDS kernel refuse (`what` names the caller's feature)
static int twin_limits(const qldpc_schedule* s, int algo, const char* what) {
  const qldpc_code* c = s->code;
  const LdsLimit l = lds_limit(s->lds_ok, c, algo);
  if (l == LDS_TABLES16)
    return fail(QLDPC_EUNSUP, "%s: %d x %d with %d edges is past the LDS kernels' 16-bit tables "
                "(m, n, edges, layer rows <= 65535); there is no HBM-resident variant", what, c->m, c->n, c->E);
  if (l == LDS_MS_ROW_DEG) return fail(QLDPC_EUNSUP, "%s: MS row degree %d > 32 has no LDS kernel", what, c->max_row_deg);
  if (l == LDS_BP_COL_DEG)
    return fail(QLDPC_EUNSUP, "%s: BP column degree %d > 128 has no LDS kernel", what, c->max_col_deg);
  if (l == LDS_FORCE_HBM)
    return fail(QLDPC_EUNSUP, "%s: option force_hbm is set and there is no HBM-resident variant", what);
  return QLDPC_OK;
}

// the feature's name in messages (kind: PLAN_PRIOR or PLAN_VPRIOR)
static const char* twin_name(PlanKind kind) { return kind == PLAN_PRIOR ? "two-level priors" : "per-variable priors"; }

// PLAN_VPRIOR under option vprior_hbm: what the LDS twin refuses decodes with
// hbm_tile_vprior_kernel (the two-level twin has no HBM-resident variant)
static bool vprior_hbm_on(PlanKind kind) { return kind == PLAN_VPRIOR && opt(&Options::vprior_hbm) != 0; }

// twin_limits without the message: no LDS kernel runs this (schedule, algo)
static bool past_lds_limits(const qldpc_schedule* s, int algo) { return lds_limit(s->lds_ok, s->code, algo) != LDS_FITS; }

uint32_t capi::prior_filter_word(const qldpc_code* c, const std::vector<double>& L) {
  uint32_t f = 0;
  const size_t n = std::min(L.size(), c->avar.size());
  for (size_t v = 0; v < n; ++v)
    if (L[v] < 0.0) f ^= c->avar[v];
  return f;
}

int capi::choose_twin_kernel(const qldpc_schedule* s, int algo, PlanKind kind, KernelChoice* k) {
  const qldpc_code* c = s->code;
  *k = KernelChoice{};
  k->max_waves = QLDPC_MAX_THREADS / 64;
  k->kind = kind;
  if (vprior_hbm_on(kind) && past_lds_limits(s, algo)) {
    k->hbm = true;
    k->kernel = qldpc::select_hbm_vprior_kernel(algo, c->max_row_deg, &k->name);
    return QLDPC_OK;
  }
  if (int rc = twin_limits(s, algo, twin_name(kind))) return rc;
  const auto select = kind == PLAN_PRIOR ? qldpc::select_prior_kernel : qldpc::select_vprior_kernel;
  k->kernel = select(algo, s->layered, fast_table_ok(c) ? c->uniform_deg : 0, flooding_tall(s), &k->name);
  return QLDPC_OK;
}

int capi::plan_static(const qldpc_schedule* s, int algo, const KernelChoice& k, DecodeArgs* a) {
  const qldpc_code* c = s->code;
  if (k.family == FAM_MS_FLOOD_QC) {
    // no tables and no LDS: the graph is compiled into the kernel, the state lives in registers
    a->qc_table = k.qc_table;
    a->m = c->m, a->n = c->n, a->E = c->E, a->n_layers = s->n_layers;
    a->wm = (c->m + 63) / 64, a->wn = (c->n + 63) / 64;
    a->vinv = c->d_vinv;                              // (unread: outputs are in original order)
    a->wave_bytes = 0;
    return 0;
  }
  const TableImage& t = k.family == FAM_MS_FLOOD     ? s->flood_ms
                        : k.family == FAM_MS_LAYERED ? s->layered_ms
                        : k.family == FAM_BP_TEAM_LG ? s->layered_bp
                                                     : s->generic;
  int image_lds = t.lds_bytes;
  a->blob = t.dev;
  a->blob_bytes = k.family == FAM_MS_FLOOD ? 0 : t.lds_bytes;   // what the kernel's staging loop copies
  a->lds_skip = t.lds_skip;
  if (QLDPC_MSL_GT && k.family == FAM_MS_LAYERED && k.lanes == 1) {
    // ms_layered_kernel<DC, 1>: the leading row table and the trailing filter
    // words are read from global memory; the LDS image is what lies between
    a->lds_skip = t.off.lay_rows;
    a->blob_bytes = image_lds = t.off.vn_chk - t.off.lay_rows;
  }
  a->off_cn_tab = t.off.cn_tab, a->off_row_ptr = t.off.row_ptr, a->off_vn_ptr = t.off.vn_ptr;
  a->off_vn_chk = t.off.vn_chk, a->off_lay_ptr = t.off.lay_ptr, a->off_lay_rows = t.off.lay_rows;
  a->off_adj_ptr = t.off.adj_ptr, a->off_adj_vars = t.off.adj_vars, a->off_chunk_dmax = t.off.chunk_dmax;
  const bool msl = k.family == FAM_MS_LAYERED;
  wave_layout(c, s->layered, algo, msl, msl && k.lanes == 0 ? (int)s->h_lay_rows.size() : 0, k.kind == PLAN_PRIOR,
              a);
  if (k.kind == PLAN_VPRIOR) {
    // decode_vprior_kernel: the prior row f64[n] between the image and the slices
    a->vprior_bytes = align16(8 * c->n);
    image_lds += a->vprior_bytes;
  }
  if (k.team) team_layout(c, k.team, a);
  a->m = c->m, a->n = c->n, a->E = c->E, a->n_layers = s->n_layers;
  a->wm = (c->m + 63) / 64, a->wn = (c->n + 63) / 64;
  a->vinv = c->d_vinv, a->wc = c->d_wc, a->rtab = c->d_rtab, a->avar = c->d_avar;
  a->vperm = c->d_vperm;
  a->filt_all = c->filt_all;
  return image_lds;
}

// [table image][one slice per wave, or one per team][BP: NumPy's libm tables]
int capi::plan_lds(int algo, int image_lds, int team, int waves, DecodeArgs* a) {
  const int libm = algo == QLDPC_ALGO_BP ? (int)sizeof(qldpc_libm_tab) : 0;
  const int lds = image_lds + (team ? 1 : waves) * a->wave_bytes + libm;
  a->off_libm = libm ? lds - libm : 0;
  return lds;
}

void capi::plan_static_hbm(const qldpc_schedule* s, qldpc::HbmArgs* a) {
  const qldpc_code* c = s->code;
  a->row_ptr = c->d_row_ptr, a->row_var = c->d_row_var, a->row_pos = c->d_row_pos, a->col_ptr = c->d_col_ptr;
  a->vinv = c->d_vinv32, a->wc = c->d_wc, a->avar = c->d_avar, a->filt_all = c->filt_all;
  a->lay_ptr = s->d_h_lay_ptr, a->lay_rows = s->d_h_lay_rows;
  a->adj_ptr = s->d_h_adj_ptr, a->adj_vars = s->d_h_adj_vars;
  a->n_layers = s->n_layers, a->m = c->m, a->n = c->n, a->E = c->E;
  a->wm = (c->m + 63) / 64, a->wn = (c->n + 63) / 64;
}

// ---------------------------------------------------------------------------
// launch plan, device half: occupancy, and the cache under the schedule's lock
// ---------------------------------------------------------------------------
static int build_plan(qldpc_schedule* s, int algo, PlanKind kind, LaunchPlan* p) {
  const bool prior = kind != PLAN_SCALAR;             // a twin of the generic LDS kernel, or nothing
  const qldpc_code* c = s->code;
  int max_lds = 0;
  if (int rc = device_limits(&max_lds, &p->cus)) return rc;
  // The LDS-resident kernels when their tables and per-half-shot state fit,
  // else the HBM-resident kernel (hbm_kernels.hip). Option force_hbm takes the
  // HBM kernel for any code (tests: the two families agree bit for bit).
  p->hbm = past_lds_limits(s, algo);
  KernelChoice pk;
  if (prior) {
    if (int rc = choose_twin_kernel(s, algo, kind, &pk)) return rc;
    p->hbm = pk.hbm;
  }
  if (!p->hbm) {
    const KernelChoice k = prior ? pk : choose_kernel(s, algo);
    p->kernel = k.kernel, p->name = k.name, p->team = k.team;
    p->hs_per_wave = k.family == FAM_MS_FLOOD_QC ? 4 : 1;
    const int image_lds = plan_static(s, algo, k, &p->args);
    HIP_TRY(qldpc::configure_kernel(k.kernel, max_lds));
    auto lds_of = [&](int w) { return plan_lds(algo, image_lds, k.team, w, &p->args); };
    // wave kernels: any width the kernel was compiled for; a team (one workgroup of `team` waves per
    // half-shot) has that one width, so no search and no waves_per_wg, while wg_per_cu still applies
    WaveChoice wc;
    HIP_TRY(wave_search(k.team ? k.team : 1, k.team ? k.team : k.max_waves, max_lds, lds_of, occupancy_of(k.kernel), true,
                        &wc));
    p->waves = wc.waves, p->blocks_per_cu = wc.blocks_per_cu, p->lds = wc.lds;
    (void)lds_of(p->waves);                           // off_libm of the chosen width
    // no LDS kernel holds the graph's per-half-shot state and tables: the
    // HBM-resident kernel decodes it; decided once per plan, not per launch
    p->hbm = wc.waves == 0;
    if (prior && p->hbm && !vprior_hbm_on(kind))
      return fail(QLDPC_EUNSUP, "%s: the tables and one wave's state (%d + %d B) do not fit the %d B "
                  "of LDS; there is no HBM-resident variant", twin_name(kind), image_lds, p->args.wave_bytes, max_lds);
  }
  if (p->hbm) {
    p->kernel = (kind == PLAN_VPRIOR ? qldpc::select_hbm_vprior_kernel : qldpc::select_hbm_kernel)(
        algo, c->max_row_deg, &p->name);
    p->waves = p->blocks_per_cu = p->lds = p->team = 0;
    plan_static_hbm(s, &p->hargs);
    if (algo == QLDPC_ALGO_BP && c->max_col_deg > 128) {
      // np.sum splits a column of more than 128 entries: one pending sum per
      // level and lane, for the deepest column the code has (both kernels)
      int depth = 0;
      for (int v = 0; v < c->n; ++v) depth = std::max(depth, qldpc::hbm_column_depth(c->csc_ptr[v + 1] - c->csc_ptr[v]));
      p->hbm_lds = qldpc::hbm_vprior_lds(depth);
      if (p->hbm_lds > (size_t)max_lds / 2)
        return fail(QLDPC_EUNSUP, "%s: BP column degree %d needs %zu B of LDS for its column sums",
                    kind == PLAN_SCALAR ? "HBM decode" : twin_name(kind), c->max_col_deg, p->hbm_lds);
      HIP_TRY(qldpc::configure_kernel(p->kernel, max_lds / 2));   // (beside 6.4 KB of static LDS)
    }
    int per_cu = 0;                                  // resident tiles at the kernel's register use
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p->kernel, 64 * qldpc::kHbmWaves, p->hbm_lds));
    p->hbm_tiles_cap = p->cus * std::max(per_cu, 1);
  }
  return QLDPC_OK;
}

// The one validating way to a plan (cached_plan, under the schedule's lock)
static int resolve_plan(const qldpc_code* code, qldpc_schedule* s, int algo, LaunchPlan* out,
                        PlanKind kind = PLAN_SCALAR) {
  if (algo != QLDPC_ALGO_MS && algo != QLDPC_ALGO_BP) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  if (code->device < 0 || !s->generic.dev)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code/schedule was created");
  return cached_plan(s->mu, s->plan[kind][algo], out, [&](LaunchPlan* p) { return build_plan(s, algo, kind, p); });
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
// One decode call's arguments, as qldpc_decode_device_ex lists them (host entries: host buffers in io, st unread)
struct DecodeCall {
  const qldpc_code* code;
  const qldpc_schedule* sched;
  int algo;
  CallIO io;
  double p;
  int max_iter;
  double beta, eps;
  hipStream_t st;
};
// hbm_tile_kernel's workspace for t tiles of 64 half-shot slots
struct HbmLayout { size_t off_post, off_syn, bytes; };
static HbmLayout hbm_layout(const qldpc_code* c, size_t w, int64_t t) {
  HbmLayout l;
  l.off_post = ((size_t)t * c->E * w * 64 + 255) & ~(size_t)255;
  l.off_syn = (l.off_post + (size_t)t * c->n * w * 64 + 255) & ~(size_t)255;
  l.bytes = l.off_syn + (size_t)t * c->m * 64 + 256;
  return l;
}

// The HBM-resident decode: tiles of 64 half-shot slots, one workgroup each,
// tiles = min(what the batch fills, the workgroups a CU holds at the kernel's
// register use, what a 64 GiB (or half the free memory) workspace holds); the
// workspace belongs to the schedule and an event orders launches that share it.
// With `vp` (hbm_tile_vprior_kernel) the priors come from the handle's row and
// its filter word; q.p is unread.
static int decode_hbm(qldpc_schedule* s, const LaunchPlan& plan, const DecodeCall& q, const qldpc_prior* vp) {
  const qldpc_code* code = q.code;
  if (vp && !vp->d_L.p) return fail(QLDPC_EHIP, "no HIP device was visible when the prior handle was created");
  const size_t w = q.algo == QLDPC_ALGO_MS ? 4 : 8;   // message / posterior row element (MS: f32 S)
  const size_t per_tile = ((size_t)code->E * w + (size_t)code->n * w + (size_t)code->m) * 64;
  std::lock_guard<std::mutex> lk(s->mu);
  int64_t tiles = std::min<int64_t>((q.io.batch + 63) / 64, (int64_t)plan.hbm_tiles_cap);
  // the workspace those tiles need; grown (never shrunk: qldpc_schedule_release_workspace
  // frees it) within half of the free device memory, at most 64 GiB
  if (hbm_layout(code, w, tiles).bytes > s->hbm_ws_bytes) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = std::min<size_t>(free_b / 2 + s->hbm_ws_bytes, (size_t)64 << 30);
    tiles = std::min<int64_t>(tiles, (int64_t)(budget / per_tile));
  }
  if (tiles < 1) return fail(QLDPC_EUNSUP, "HBM decode needs %zu B per 64-slot tile: device memory too small", per_tile);
  const HbmLayout lay = hbm_layout(code, w, tiles);
  if (!s->hbm_ev) HIP_TRY(hipEventCreateWithFlags(&s->hbm_ev, hipEventDisableTiming));
  if (lay.bytes > s->hbm_ws_bytes) {
    if (s->hbm_ws) {
      HIP_TRY(hipEventSynchronize(s->hbm_ev));      // last launch done with the old workspace
      HIP_TRY(hipFree(s->hbm_ws));
      s->hbm_ws = nullptr;
      s->hbm_ws_bytes = 0;
    }
    HIP_TRY(hipMalloc(&s->hbm_ws, lay.bytes));
    s->hbm_ws_bytes = lay.bytes;
  }
  HIP_TRY(hipStreamWaitEvent(q.st, s->hbm_ev, 0));  // a launch on another stream may still use it
  qldpc::HbmArgs a = plan.hargs;
  a.c2v = s->hbm_ws;
  a.post = (char*)s->hbm_ws + lay.off_post;
  a.synT = (uint8_t*)s->hbm_ws + lay.off_syn;
  a.syn = (const uint8_t*)q.io.syn, a.ehat = (uint8_t*)q.io.ehat;
  a.iters = q.io.iters, a.out_post = q.io.post, a.flags = q.io.flags;
  a.syn_bits = q.io.syn_format == QLDPC_FMT_BITS, a.eh_bits = q.io.ehat_format == QLDPC_FMT_BITS;
  a.batch = q.io.batch;
  if (vp) {
    a.L = 0.0, a.L32 = 0.0f;                        // (unread: every prior comes from the handle's row)
  } else {
    a.L = qldpc_prior_llr(q.p, q.eps);              // np.log prior (decoders.py:147, :232)
    a.L32 = (float)a.L;
  }
  a.beta = q.beta, a.eps = q.eps, a.max_iter = q.max_iter;
  if (int rc = s->queue.claim(q.st, &a.queue)) return rc;   // (always: this kernel has no static schedule)
  TimedLaunch t;
  if (int rc = timing_begin(&t, q.st)) return rc;
  if (vp)
    HIP_TRY(qldpc::launch_hbm_vprior(plan.kernel, a, qldpc::HbmPrior{vp->d_L, vp->filt0}, (int)tiles, s->d_h_fl_var,
                                     s->d_h_fl_pos, s->hbm_lazy ? 1 : 0, plan.hbm_lds, q.st));
  else
    HIP_TRY(qldpc::launch_hbm(plan.kernel, a, (int)tiles, s->d_h_fl_var, s->d_h_fl_pos, s->hbm_lazy ? 1 : 0,
                              plan.hbm_lds, q.st));
  if (int rc = timing_end(&t, q.st)) return rc;
  HIP_TRY(hipEventRecord(s->hbm_ev, q.st));
  return QLDPC_OK;
}

extern "C" int qldpc_decode_device(const qldpc_code* code, const qldpc_schedule* sched_c, int algo,
                                   const uint8_t* d_syn, int64_t batch, double p, int max_iter,
                                   double beta, double eps, uint8_t* d_ehat, int32_t* d_iters,
                                   double* d_post, int32_t* d_flags, void* stream) {
  return qldpc_decode_device_ex(code, sched_c, algo, d_syn, QLDPC_FMT_BYTES, batch, p, max_iter, beta, eps, d_ehat,
                                QLDPC_FMT_BYTES, d_iters, d_post, d_flags, stream);
}

// The BP check node's saturated value (bp_team.h, cn_bp_word): at
// |th2| = 1 the reference clips th2 to +-(1 - eps) (decoders.py:256-258), so
// c2v = +-2 atanh(1 - eps) — computed here by the restated SVML atanh the
// kernels and the oracle share (include/qldpc_libm.h), the same expression
// as the full path; not finite (eps <= 0) turns the fast path off.
static void bp_saturation(double eps, double* csat, uint32_t* sat_hi) {
  double th2 = 1.0;
  th2 = (std::fabs(th2) >= 1.0 - eps) ? std::copysign(std::fabs(th2) - eps, th2) : th2;
  const double v = 2.0 * qldpc_atanh(th2);
  const bool on = std::isfinite(v);
  *csat = on ? v : 0.0;
  *sat_hi = on ? 0x40338000u : 0x7ff00000u;            // |x| >= 19.5 (high word, sign cleared)
}

// the two-level prior of qldpc_decode_device_prior: variables whose mask bit is
// set take p1 (the others the call's p)
struct PriorCall {
  double p1;
  const void* mask;
  int mask_format;
};

// A decode call carries at most one of pr, the two-level prior of
// qldpc_decode_device_prior, and vp, the per-variable priors of
// qldpc_decode_device_vprior (p is then unread)
static PlanKind kind_of(const PriorCall* pr, const qldpc_prior* vp) {
  return vp ? PLAN_VPRIOR : pr ? PLAN_PRIOR : PLAN_SCALAR;
}

// what a call with `pr` or `vp` checks on top of the scalar entry, before any
// HIP call: its own arguments, then what the twin kernel refuses
static int validate_twin(const qldpc_code* code, const qldpc_schedule* sched, int algo, int64_t batch, double p0,
                         const PriorCall* pr, const qldpc_prior* vp) {
  if (pr) {
    if (pr->mask_format != QLDPC_FMT_BYTES && pr->mask_format != QLDPC_FMT_BITS)
      return fail(QLDPC_EINVAL, "unknown mask format");
    if (!(p0 >= 0.0 && p0 <= 1.0) || !(pr->p1 >= 0.0 && pr->p1 <= 1.0))
      return fail(QLDPC_EINVAL, "two-level priors: p0 and p1 must be probabilities (0 <= p <= 1)");
    if (batch > 0 && !pr->mask) return fail(QLDPC_EINVAL, "null mask");
  }
  if (vp && code && (vp->code != code || vp->n != code->n || vp->m != code->m || vp->E != code->E))
    return fail(QLDPC_EINVAL, "prior handle was built for a different code");
  if ((pr || vp) && code && sched && sched->code == code && (algo == QLDPC_ALGO_MS || algo == QLDPC_ALGO_BP)) {
    KernelChoice k;
    if (int rc = choose_twin_kernel(sched, algo, kind_of(pr, vp), &k)) return rc;
  }
  return QLDPC_OK;
}

// The device-free checks of a decode call, in the order decode_device reports
// them (decode_host makes them before its staging copies where it can)
static int validate_call(const DecodeCall& q, const PriorCall* pr, const qldpc_prior* vp) {
  if ((q.io.syn_format != QLDPC_FMT_BYTES && q.io.syn_format != QLDPC_FMT_BITS) ||
      (q.io.ehat_format != QLDPC_FMT_BYTES && q.io.ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  if (!q.code || !q.sched) return fail(QLDPC_EINVAL, "code/schedule is null");
  if (q.sched->code != q.code) return fail(QLDPC_EINVAL, "schedule was built for a different code");
  if (q.algo != QLDPC_ALGO_MS && q.algo != QLDPC_ALGO_BP) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  if (q.io.batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (q.max_iter < 1) return fail(QLDPC_EINVAL, "max_iter must be >= 1 (the reference leaves e_hat unbound)");
  return validate_twin(q.code, q.sched, q.algo, q.io.batch, q.p, pr, vp);
}

static int decode_device(const DecodeCall& q, const PriorCall* pr, const qldpc_prior* vp = nullptr) {
  if (int rc = validate_call(q, pr, vp)) return rc;
  const qldpc_code* code = q.code;
  auto* sched = const_cast<qldpc_schedule*>(q.sched);
  const double eps = q.eps;
  if (q.io.batch == 0) return QLDPC_OK;
  if (!q.io.syn || !q.io.ehat || !q.io.iters) return fail(QLDPC_EINVAL, "null device buffer");
  if (code->device < 0 || !sched->generic.dev)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code/schedule was created");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != code->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", code->device, dev);
  LaunchPlan plan;
  if (int rc = resolve_plan(code, sched, q.algo, &plan, kind_of(pr, vp))) return rc;
  hipStream_t st = q.st;
  if (plan.hbm) return decode_hbm(sched, plan, q, vp);

  DecodeArgs a = plan.args;
  set_call_io(&a, q.io);
  // L_ch = np.log((1 - p) / max(p, eps))   (decoders.py:147, :232), with
  // NumPy's own log (SVML log8_ha, include/qldpc_libm.h): glibc's differs in
  // the last bit for ~0.2 % of priors
  a.L = qldpc_prior_llr(q.p, eps);
  a.L32 = (float)a.L;
  if (pr) {
    a.L1 = qldpc_prior_llr(pr->p1, eps);
    a.pmask = pr->mask;
    a.pmask_bits = pr->mask_format == QLDPC_FMT_BITS;
  }
  if (vp) {
    if (!vp->d_L.p) return fail(QLDPC_EHIP, "no HIP device was visible when the prior handle was created");
    a.vprior = vp->d_L;
    a.L = 0.0, a.L32 = 0.0f;                          // (unread: every prior comes from the row)
  }
  a.beta = q.beta, a.eps = eps;
  bp_saturation(eps, &a.bp_csat, &a.bp_sat_hi);
  a.max_iter = q.max_iter;
  {
    // (L + (double)S < 0) == (S < hd_thresh) for every float S: the float at
    // or below -L, nudged up one step when -L is not a float
    const double t = -a.L;
    float f = (float)t;
    if ((double)f > t) f = std::nextafter(f, -INFINITY);
    a.hd_thresh = ((double)f == t) ? f : std::nextafter(f, INFINITY);
  }
  a.queue = nullptr;
  if (!opt(&Options::static_sched))
    if (int rc = sched->queue.claim(st, &a.queue)) return rc;
  const int grid = launch_grid(q.io.batch, plan.team ? 1 : (int64_t)plan.waves * plan.hs_per_wave, plan.blocks_per_cu,
                               plan.cus);
  TimedLaunch t;
  if (int rc = timing_begin(&t, st)) return rc;
  HIP_TRY(qldpc::launch_decode(plan.kernel, a, grid, 64 * plan.waves, plan.lds, st));
  return timing_end(&t, st);
}

extern "C" int qldpc_decode_device_ex(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                      const void* d_syn, int syn_format, int64_t batch, double p, int max_iter,
                                      double beta, double eps, void* d_ehat, int ehat_format, int32_t* d_iters,
                                      double* d_post, int32_t* d_flags, void* stream) {
  const DecodeCall q{code, sched, algo, {d_syn, syn_format, batch, d_ehat, ehat_format, d_iters, d_flags, d_post}, p,
                     max_iter, beta, eps, (hipStream_t)stream};
  return decode_device(q, nullptr);
}

extern "C" int qldpc_decode_device_prior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                         const void* d_syn, int syn_format, int64_t batch, double p0, double p1,
                                         const void* d_mask, int mask_format, int max_iter, double beta, double eps,
                                         void* d_ehat, int ehat_format, int32_t* d_iters, double* d_post,
                                         int32_t* d_flags, void* stream) {
  const PriorCall pr{p1, d_mask, mask_format};
  const DecodeCall q{code, sched, algo, {d_syn, syn_format, batch, d_ehat, ehat_format, d_iters, d_flags, d_post}, p0,
                     max_iter, beta, eps, (hipStream_t)stream};
  return decode_device(q, &pr);
}

static int twin_kernel_name(const qldpc_code* code, const qldpc_schedule* sched, int algo, PlanKind kind, char* buf,
                            int len) {
  if (!code || !sched || !buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  if (sched->code != code) return fail(QLDPC_EINVAL, "schedule was built for a different code");
  if (algo != QLDPC_ALGO_MS && algo != QLDPC_ALGO_BP) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  KernelChoice k;                                     // (no device needed: the name depends on the code alone)
  if (int rc = choose_twin_kernel(sched, algo, kind, &k)) return rc;
  if (vprior_hbm_on(kind) && !k.hbm && code->device >= 0 && sched->generic.dev) {
    // option vprior_hbm: whether the LDS twin or hbm_tile_vprior_kernel runs is
    // then a question of the device's LDS size, answered by the launch plan
    LaunchPlan plan;
    if (int rc = resolve_plan(code, const_cast<qldpc_schedule*>(sched), algo, &plan, kind)) return rc;
    k.name = plan.name;
  }
  snprintf(buf, (size_t)len, "%s", k.name);
  return QLDPC_OK;
}

extern "C" int qldpc_decode_prior_kernel_name(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                              char* buf, int len) {
  return twin_kernel_name(code, sched, algo, PLAN_PRIOR, buf, len);
}

extern "C" int qldpc_decode_kernel_name(const qldpc_code* code, const qldpc_schedule* sched_c, int algo,
                                        char* buf, int len) {
  auto* sched = const_cast<qldpc_schedule*>(sched_c);
  if (!code || !sched || !buf || len <= 0) return fail(QLDPC_EINVAL, "null argument");
  LaunchPlan plan;
  if (int rc = resolve_plan(code, sched, algo, &plan)) return rc;
  snprintf(buf, (size_t)len, "%s", plan.name);
  return QLDPC_OK;
}

extern "C" int qldpc_decode_launch_info(const qldpc_code* code, const qldpc_schedule* sched_c, int algo,
                                        int* waves_per_wg, int* wg_per_cu, int* lds_bytes) {
  auto* sched = const_cast<qldpc_schedule*>(sched_c);
  if (!code || !sched || !waves_per_wg || !wg_per_cu || !lds_bytes) return fail(QLDPC_EINVAL, "null argument");
  LaunchPlan plan;
  if (int rc = resolve_plan(code, sched, algo, &plan)) return rc;
  *waves_per_wg = plan.waves;                         // all three 0 on the HBM path
  *wg_per_cu = plan.blocks_per_cu;
  *lds_bytes = plan.lds;
  return QLDPC_OK;
}

// qldpc_decode_host, with `pr` (a host byte mask) qldpc_decode_host_prior, and
// with `vp` qldpc_decode_host_vprior
static int decode_host(const DecodeCall& q, const PriorCall* pr, const qldpc_prior* vp = nullptr) {
  auto* code = const_cast<qldpc_code*>(q.code);
  const int64_t batch = q.io.batch;
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  // Before the staging copies: with `vp` every check decode_device makes
  // before its first HIP call; with `pr` the prior's own part alone, so its
  // errors come ahead of the schedule / algo / max_iter ones, which this entry
  // and the scalar one report from decode_device, behind the copies.
  if (vp) {
    if (int rc = validate_call(q, nullptr, vp)) return rc;
  } else if (pr) {
    if (!q.sched) return fail(QLDPC_EINVAL, "code/schedule is null");
    if (int rc = validate_twin(code, q.sched, q.algo, batch, q.p, pr, nullptr)) return rc;
  }
  if (batch == 0) return QLDPC_OK;
  if (!q.io.syn || !q.io.ehat || !q.io.iters) return fail(QLDPC_EINVAL, "null host buffer");
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  return staged_call(code, q.io, [&](const CallIO& d, hipStream_t st) {
    DecodeCall dq = q;
    dq.io = d, dq.st = st;
    if (!pr) return decode_device(dq, nullptr, vp);
    // the mask goes through the workspace's mask buffers, grown with it
    const int64_t bn = batch * code->n;
    if (code->ws_mask_cap < code->ws_cap) {
      const size_t cn = std::max<int64_t>(1, code->ws_cap * code->n);
      HIP_TRY(code->ws_mask.alloc(cn));
      HIP_TRY(code->hp_mask.alloc(cn));
      code->ws_mask_cap = code->ws_cap;
    }
    if (bn) {
      memcpy(code->hp_mask, pr->mask, bn);
      HIP_TRY(hipMemcpyAsync(code->ws_mask, code->hp_mask, bn, hipMemcpyHostToDevice, st));
    }
    const PriorCall dpr{pr->p1, code->ws_mask.p, QLDPC_FMT_BYTES};
    return decode_device(dq, &dpr, vp);
  });
}

extern "C" int qldpc_decode_host(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                 const uint8_t* h_syn, int64_t batch, double p, int max_iter,
                                 double beta, double eps, uint8_t* h_ehat, int32_t* h_iters,
                                 double* h_post, int32_t* h_flags) {
  const DecodeCall q{code, sched, algo, host_io(h_syn, batch, h_ehat, h_iters, h_post, h_flags), p, max_iter, beta,
                     eps, nullptr};
  return decode_host(q, nullptr);
}

extern "C" int qldpc_decode_host_prior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                       const uint8_t* h_syn, int64_t batch, double p0, double p1,
                                       const uint8_t* h_mask, int max_iter, double beta, double eps,
                                       uint8_t* h_ehat, int32_t* h_iters, double* h_post, int32_t* h_flags) {
  const PriorCall pr{p1, h_mask, QLDPC_FMT_BYTES};
  const DecodeCall q{code, sched, algo, host_io(h_syn, batch, h_ehat, h_iters, h_post, h_flags), p0, max_iter, beta,
                     eps, nullptr};
  return decode_host(q, &pr);
}

// ---------------------------------------------------------------------------
// per-variable priors: the qldpc_prior handle and its decode entry points
// ---------------------------------------------------------------------------
extern "C" int qldpc_prior_create(const qldpc_code* code, const double* h_p, double eps, qldpc_prior** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (code->n > 0 && !h_p) return fail(QLDPC_EINVAL, "per-variable priors: null probability vector");
  const int n = code->n;
  for (int j = 0; j < n; ++j)
    if (!(h_p[j] >= 0.0 && h_p[j] < 1.0))             // (NaN fails both)
      return fail(QLDPC_EINVAL, "per-variable priors: p[%d] = %g is not a probability in [0, 1)", j, h_p[j]);
  std::unique_ptr<qldpc_prior> pr(new qldpc_prior());
  pr->code = code;
  pr->m = code->m, pr->n = n, pr->E = code->E;
  pr->eps = eps;
  pr->L.resize(n);
  for (int j = 0; j < n; ++j) {                       // relabeled variable j is original column vperm[j]
    pr->L[j] = qldpc_prior_llr(h_p[code->vperm[j]], eps);
    if (!std::isfinite(pr->L[j]))
      return fail(QLDPC_EINVAL, "per-variable priors: p[%d] = %g with eps = %g has no finite prior", code->vperm[j],
                  h_p[code->vperm[j]], eps);
  }
  pr->W.resize(n);                                    // |L_j| < 750: L_j 2^20 is exact and fits; round-half-even
  for (int j = 0; j < n; ++j) pr->W[j] = (int64_t)std::llrint(std::ldexp(pr->L[j], 20));
  pr->Wo.resize(n);
  for (int j = 0; j < n; ++j) pr->Wo[code->vperm[j]] = pr->W[j];
  if (code->device >= 0) {
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev != code->device)
      return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", code->device, dev);
    HIP_TRY(pr->d_L.upload(pr->L));
    HIP_TRY(pr->d_W.upload(pr->W));
    HIP_TRY(pr->d_Wo.upload(pr->Wo));
  }
  pr->filt0 = prior_filter_word(code, pr->L);
  *out = pr.release();
  return QLDPC_OK;
}

extern "C" int qldpc_prior_destroy(qldpc_prior* prior) {
  delete prior;
  return QLDPC_OK;
}

extern "C" int qldpc_decode_device_vprior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                          const void* d_syn, int syn_format, int64_t batch, const qldpc_prior* prior,
                                          int max_iter, double beta, void* d_ehat, int ehat_format, int32_t* d_iters,
                                          double* d_post, int32_t* d_flags, void* stream) {
  if (!prior) return fail(QLDPC_EINVAL, "prior handle is null");
  const DecodeCall q{code, sched, algo, {d_syn, syn_format, batch, d_ehat, ehat_format, d_iters, d_flags, d_post},
                     0.0, max_iter, beta, prior->eps, (hipStream_t)stream};
  return decode_device(q, nullptr, prior);
}

extern "C" int qldpc_decode_host_vprior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                        const uint8_t* h_syn, int64_t batch, const qldpc_prior* prior, int max_iter,
                                        double beta, uint8_t* h_ehat, int32_t* h_iters, double* h_post,
                                        int32_t* h_flags) {
  if (!prior) return fail(QLDPC_EINVAL, "prior handle is null");
  const DecodeCall q{code, sched, algo, host_io(h_syn, batch, h_ehat, h_iters, h_post, h_flags), 0.0, max_iter, beta,
                     prior->eps, nullptr};
  return decode_host(q, nullptr, prior);
}

extern "C" int qldpc_decode_vprior_kernel_name(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                               char* buf, int len) {
  return twin_kernel_name(code, sched, algo, PLAN_VPRIOR, buf, len);
}

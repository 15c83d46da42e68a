// capi_decode.cpp — launch plans, the decode entry points, launch timing, the
// HBM-resident path and the host staging entry point.

#include <cmath>
#include <cstdio>
#include <memory>

#include "capi_internal.h"
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
  if (!s->lds_ok)
    return fail(QLDPC_EUNSUP, "%s: %d x %d with %d edges is past the LDS kernels' 16-bit tables "
                "(m, n, edges, layer rows <= 65535); there is no HBM-resident variant", what, c->m, c->n, c->E);
  if (algo == QLDPC_ALGO_MS && c->max_row_deg > 32)
    return fail(QLDPC_EUNSUP, "%s: MS row degree %d > 32 has no LDS kernel", what, c->max_row_deg);
  if (algo == QLDPC_ALGO_BP && c->max_col_deg > 128)
    return fail(QLDPC_EUNSUP, "%s: BP column degree %d > 128 has no LDS kernel", what, c->max_col_deg);
  if (opt(&Options::force_hbm) != 0)
    return fail(QLDPC_EUNSUP, "%s: option force_hbm is set and there is no HBM-resident variant", what);
  return QLDPC_OK;
}

// the feature's name in messages (kind: PLAN_PRIOR or PLAN_VPRIOR)
static const char* twin_name(PlanKind kind) { return kind == PLAN_PRIOR ? "two-level priors" : "per-variable priors"; }

// PLAN_VPRIOR under option vprior_hbm: what the LDS twin refuses decodes with
// hbm_tile_vprior_kernel (the two-level twin has no HBM-resident variant)
static bool vprior_hbm_on(PlanKind kind) { return kind == PLAN_VPRIOR && opt(&Options::vprior_hbm) != 0; }

// twin_limits without the message: no LDS twin runs this (schedule, algo)
static bool past_twin_limits(const qldpc_schedule* s, int algo) {
  const qldpc_code* c = s->code;
  return !s->lds_ok || (algo == QLDPC_ALGO_MS && c->max_row_deg > 32) ||
         (algo == QLDPC_ALGO_BP && c->max_col_deg > 128) || opt(&Options::force_hbm) != 0;
}

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
  if (vprior_hbm_on(kind) && past_twin_limits(s, algo)) {
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
  int dev = 0, max_lds = 0;
  HIP_TRY(hipGetDevice(&dev));
  HIP_TRY(hipDeviceGetAttribute(&max_lds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
  HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, dev));
  // The LDS-resident kernels when their tables and per-half-shot state fit,
  // else the HBM-resident kernel (hbm_kernels.hip). Option force_hbm takes the
  // HBM kernel for any code (tests: the two families agree bit for bit).
  p->hbm = !s->lds_ok || opt(&Options::force_hbm) != 0 || (algo == QLDPC_ALGO_MS && c->max_row_deg > 32) ||
           (algo == QLDPC_ALGO_BP && c->max_col_deg > 128);
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
    int best_waves = 0, max_waves = k.max_waves;
    auto occupancy = [&](int w, int lds, int* nb) {
      return hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, k.kernel, 64 * w, (size_t)lds);
    };
    auto take = [&](int w, int nb, int lds) { p->waves = w, p->blocks_per_cu = nb, p->lds = lds, best_waves = nb * w; };
    if (k.team) {  // one team (workgroup of `team` waves) per half-shot
      const int lds = plan_lds(algo, image_lds, k.team, k.team, &p->args);
      int nb = 0;
      if (lds <= max_lds) HIP_TRY(occupancy(k.team, lds, &nb));
      take(k.team, nb, lds);
      max_waves = 0;  // skip the wave-kernel search below
    }
    for (int w = max_waves; w >= 1; --w) {
      const int lds = plan_lds(algo, image_lds, 0, w, &p->args);
      if (lds > max_lds) continue;
      int nb = 0;
      HIP_TRY(occupancy(w, lds, &nb));
      if (nb * w > best_waves) take(w, nb, lds);
    }
    // Tuning overrides (experiments only): options waves_per_wg, wg_per_cu.
    if (const int64_t ow = k.team ? 0 : opt(&Options::waves_per_wg)) {
      const int w = (int)ow;
      const int lds = plan_lds(algo, image_lds, 0, w, &p->args);
      int nb = 0;
      if (w >= 1 && w <= max_waves && lds <= max_lds && occupancy(w, lds, &nb) == hipSuccess && nb > 0)
        take(w, nb, lds);
    }
    if (const int64_t ok = opt(&Options::wg_per_cu)) {
      const int k2 = (int)ok;
      if (k2 >= 1 && k2 < p->blocks_per_cu) p->blocks_per_cu = k2;
    }
    (void)plan_lds(algo, image_lds, k.team, p->waves, &p->args);   // off_libm of the chosen width
    // no LDS kernel holds the graph's per-half-shot state and tables: the
    // HBM-resident kernel decodes it; decided once per plan, not per launch
    p->hbm = best_waves == 0;
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

// The one validating way to a plan: copied into *out under the schedule's
// lock, so a launch keeps its own consistent snapshot even if an option change
// (qldpc_set_option) rebuilds the cached one meanwhile.
static int resolve_plan(const qldpc_code* code, qldpc_schedule* s, int algo, LaunchPlan* out,
                        PlanKind kind = PLAN_SCALAR) {
  if (algo != QLDPC_ALGO_MS && algo != QLDPC_ALGO_BP) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  if (code->device < 0 || !s->generic.dev)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code/schedule was created");
  std::lock_guard<std::mutex> lk(s->mu);
  const uint32_t gen = g_opt.gen.load();
  LaunchPlan& slot = s->plan[kind][algo];
  if (!slot.ok || slot.gen != gen) {
    LaunchPlan p{};                                   // built aside, published whole
    const int rc = build_plan(s, algo, kind, &p);
    if (rc) return rc;
    p.ok = true;
    p.gen = gen;
    slot = p;
  }
  *out = slot;
  return QLDPC_OK;
}

// ---------------------------------------------------------------------------
// timing
// ---------------------------------------------------------------------------
static std::mutex g_tmu;
static bool g_timing = false;
static std::vector<std::pair<hipEvent_t, hipEvent_t>> g_events;
static double g_total_ms = 0.0;
static int64_t g_launches = 0;

extern "C" int qldpc_timing_enable(int on) {
  std::lock_guard<std::mutex> lk(g_tmu);
  g_timing = on != 0;
  return QLDPC_OK;
}

static int drain_events_locked() {
  for (auto& ev : g_events) {
    HIP_TRY(hipEventSynchronize(ev.second));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, ev.first, ev.second));
    g_total_ms += ms;
    g_launches++;
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  g_events.clear();
  return QLDPC_OK;
}

extern "C" int qldpc_timing_reset(void) {
  std::lock_guard<std::mutex> lk(g_tmu);
  int rc = drain_events_locked();
  g_total_ms = 0.0;
  g_launches = 0;
  return rc;
}

extern "C" int qldpc_timing_read(double* total_ms, int64_t* launches) {
  std::lock_guard<std::mutex> lk(g_tmu);
  int rc = drain_events_locked();
  if (total_ms) *total_ms = g_total_ms;
  if (launches) *launches = g_launches;
  return rc;
}

// A timed launch: timing_begin before the kernel is enqueued, timing_end
// after. The event pair goes to g_events; drain_events_locked destroys it.
int capi::timing_begin(TimedLaunch* t, hipStream_t st) {
  {
    std::lock_guard<std::mutex> lk(g_tmu);
    if (!g_timing) return QLDPC_OK;
  }
  HIP_TRY(hipEventCreate(&t->e0));
  HIP_TRY(hipEventCreate(&t->e1));
  HIP_TRY(hipEventRecord(t->e0, st));
  return QLDPC_OK;
}

int capi::timing_end(TimedLaunch* t, hipStream_t st) {
  if (!t->e0) return QLDPC_OK;
  HIP_TRY(hipEventRecord(t->e1, st));
  std::lock_guard<std::mutex> lk(g_tmu);
  g_events.emplace_back(t->e0, t->e1);
  return QLDPC_OK;
}

// ---------------------------------------------------------------------------
// decode
// ---------------------------------------------------------------------------
struct DecodeCall {  // the per-call arguments of qldpc_decode_device_ex
  const void* syn;
  void* ehat;
  int syn_format, ehat_format, max_iter;
  int64_t batch;
  double p, beta, eps;
  int32_t *iters, *flags;
  double* post;
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
static int decode_hbm(const qldpc_code* code, qldpc_schedule* s, int algo, const LaunchPlan& plan,
                      const DecodeCall& q, const qldpc_prior* vp) {
  if (vp && !vp->d_L.p) return fail(QLDPC_EHIP, "no HIP device was visible when the prior handle was created");
  const size_t w = algo == QLDPC_ALGO_MS ? 4 : 8;   // message / posterior row element (MS: f32 S)
  const size_t per_tile = ((size_t)code->E * w + (size_t)code->n * w + (size_t)code->m) * 64;
  std::lock_guard<std::mutex> lk(s->mu);
  int64_t tiles = std::min<int64_t>((q.batch + 63) / 64, (int64_t)plan.hbm_tiles_cap);
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
  a.syn = (const uint8_t*)q.syn, a.ehat = (uint8_t*)q.ehat;
  a.iters = q.iters, a.out_post = q.post, a.flags = q.flags;
  a.syn_bits = q.syn_format == QLDPC_FMT_BITS, a.eh_bits = q.ehat_format == QLDPC_FMT_BITS;
  a.batch = q.batch;
  a.queue = s->d_queue + (s->qnext.fetch_add(1) % qldpc_schedule::kQueueSlots);
  if (vp) {
    a.L = 0.0, a.L32 = 0.0f;                        // (unread: every prior comes from the handle's row)
  } else {
    a.L = qldpc_prior_llr(q.p, q.eps);              // np.log prior (decoders.py:147, :232)
    a.L32 = (float)a.L;
  }
  a.beta = q.beta, a.eps = q.eps, a.max_iter = q.max_iter;
  HIP_TRY(hipMemsetAsync(a.queue, 0, sizeof(uint32_t), q.st));
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
static int validate_call(const qldpc_code* code, const qldpc_schedule* sched, int algo, int syn_format,
                         int ehat_format, int64_t batch, double p, int max_iter, const PriorCall* pr,
                         const qldpc_prior* vp) {
  if ((syn_format != QLDPC_FMT_BYTES && syn_format != QLDPC_FMT_BITS) ||
      (ehat_format != QLDPC_FMT_BYTES && ehat_format != QLDPC_FMT_BITS))
    return fail(QLDPC_EINVAL, "unknown syndrome / estimate format");
  if (!code || !sched) return fail(QLDPC_EINVAL, "code/schedule is null");
  if (sched->code != code) return fail(QLDPC_EINVAL, "schedule was built for a different code");
  if (algo != QLDPC_ALGO_MS && algo != QLDPC_ALGO_BP) return fail(QLDPC_EINVAL, "Unrecognized decoder type.");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  if (max_iter < 1) return fail(QLDPC_EINVAL, "max_iter must be >= 1 (the reference leaves e_hat unbound)");
  return validate_twin(code, sched, algo, batch, p, pr, vp);
}

static int decode_device(const qldpc_code* code, const qldpc_schedule* sched_c, int algo,
                         const void* d_syn, int syn_format, int64_t batch, double p, int max_iter,
                         double beta, double eps, void* d_ehat, int ehat_format, int32_t* d_iters,
                         double* d_post, int32_t* d_flags, void* stream, const PriorCall* pr,
                         const qldpc_prior* vp = nullptr) {
  auto* sched = const_cast<qldpc_schedule*>(sched_c);
  if (int rc = validate_call(code, sched, algo, syn_format, ehat_format, batch, p, max_iter, pr, vp)) return rc;
  if (batch == 0) return QLDPC_OK;
  if (!d_syn || !d_ehat || !d_iters) return fail(QLDPC_EINVAL, "null device buffer");
  if (code->device < 0 || !sched->generic.dev)
    return fail(QLDPC_EHIP, "no HIP device was visible when the code/schedule was created");
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev != code->device) return fail(QLDPC_EINVAL, "code lives on device %d, current device is %d", code->device, dev);
  LaunchPlan plan;
  if (int rc = resolve_plan(code, sched, algo, &plan, kind_of(pr, vp))) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (plan.hbm)
    return decode_hbm(code, sched, algo, plan,
                      DecodeCall{d_syn, d_ehat, syn_format, ehat_format, max_iter, batch, p, beta, eps, d_iters,
                                 d_flags, d_post, st},
                      vp);

  DecodeArgs a = plan.args;
  a.syn = (const uint8_t*)d_syn, a.ehat = (uint8_t*)d_ehat;
  a.syn_bits = syn_format == QLDPC_FMT_BITS, a.eh_bits = ehat_format == QLDPC_FMT_BITS;
  a.iters = d_iters, a.post = d_post, a.flags = d_flags;
  a.batch = batch;
  // L_ch = np.log((1 - p) / max(p, eps))   (decoders.py:147, :232), with
  // NumPy's own log (SVML log8_ha, include/qldpc_libm.h): glibc's differs in
  // the last bit for ~0.2 % of priors
  a.L = qldpc_prior_llr(p, eps);
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
  a.beta = beta, a.eps = eps;
  bp_saturation(eps, &a.bp_csat, &a.bp_sat_hi);
  a.max_iter = max_iter;
  {
    // (L + (double)S < 0) == (S < hd_thresh) for every float S: the float at
    // or below -L, nudged up one step when -L is not a float
    const double t = -a.L;
    float f = (float)t;
    if ((double)f > t) f = std::nextafter(f, -INFINITY);
    a.hd_thresh = ((double)f == t) ? f : std::nextafter(f, INFINITY);
  }
  a.queue = nullptr;
  if (!opt(&Options::static_sched)) {
    a.queue = sched->d_queue + (sched->qnext.fetch_add(1) % qldpc_schedule::kQueueSlots);
    HIP_TRY(hipMemsetAsync(a.queue, 0, sizeof(uint32_t), st));
  }
  const int64_t per_block = plan.team ? 1 : (int64_t)plan.waves * plan.hs_per_wave;
  const int64_t need = (batch + per_block - 1) / per_block;
  const int64_t resident = (int64_t)plan.blocks_per_cu * plan.cus;
  const int grid = (int)std::max<int64_t>(1, std::min(need, resident));
  TimedLaunch t;
  if (int rc = timing_begin(&t, st)) return rc;
  HIP_TRY(qldpc::launch_decode(plan.kernel, a, grid, 64 * plan.waves, plan.lds, st));
  return timing_end(&t, st);
}

extern "C" int qldpc_decode_device_ex(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                      const void* d_syn, int syn_format, int64_t batch, double p, int max_iter,
                                      double beta, double eps, void* d_ehat, int ehat_format, int32_t* d_iters,
                                      double* d_post, int32_t* d_flags, void* stream) {
  return decode_device(code, sched, algo, d_syn, syn_format, batch, p, max_iter, beta, eps, d_ehat, ehat_format,
                       d_iters, d_post, d_flags, stream, nullptr);
}

extern "C" int qldpc_decode_device_prior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                         const void* d_syn, int syn_format, int64_t batch, double p0, double p1,
                                         const void* d_mask, int mask_format, int max_iter, double beta, double eps,
                                         void* d_ehat, int ehat_format, int32_t* d_iters, double* d_post,
                                         int32_t* d_flags, void* stream) {
  const PriorCall pr{p1, d_mask, mask_format};
  return decode_device(code, sched, algo, d_syn, syn_format, batch, p0, max_iter, beta, eps, d_ehat, ehat_format,
                       d_iters, d_post, d_flags, stream, &pr);
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

// The code's host staging workspace (under ws_mu), grown to hold `batch`
// half-shots; the posterior buffers only once a caller wants posteriors.
int capi::ws_reserve(qldpc_code* code, int64_t batch, bool want_post) {
  const int m = code->m, n = code->n;
  if (!code->ws_stream) HIP_TRY(hipStreamCreateWithFlags(&code->ws_stream, hipStreamNonBlocking));
  if (batch > code->ws_cap) {
    code->ws_cap = 0;
    code->ws_post_cap = 0;
    const int64_t cap = std::max<int64_t>(batch, 64);
    const size_t cm = std::max<int64_t>(1, cap * m), cn = std::max<int64_t>(1, cap * n);
    HIP_TRY(code->ws_syn.alloc(cm));
    HIP_TRY(code->ws_ehat.alloc(cn));
    HIP_TRY(code->ws_iters.alloc(cap));
    HIP_TRY(code->ws_flags.alloc(cap));
    HIP_TRY(code->hp_syn.alloc(cm));
    HIP_TRY(code->hp_ehat.alloc(cn));
    HIP_TRY(code->hp_iters.alloc(cap));
    HIP_TRY(code->hp_flags.alloc(cap));
    code->ws_cap = cap;
  }
  if (want_post && code->ws_post_cap < code->ws_cap) {
    const size_t cn = std::max<int64_t>(1, code->ws_cap * n);
    HIP_TRY(code->ws_post.alloc(cn));
    HIP_TRY(code->hp_post.alloc(cn));
    code->ws_post_cap = code->ws_cap;
  }
  return QLDPC_OK;
}

// qldpc_decode_host, with `pr` (a host byte mask) qldpc_decode_host_prior, and
// with `vp` qldpc_decode_host_vprior
static int decode_host(const qldpc_code* code_c, const qldpc_schedule* sched, int algo,
                       const uint8_t* h_syn, int64_t batch, double p, int max_iter,
                       double beta, double eps, uint8_t* h_ehat, int32_t* h_iters,
                       double* h_post, int32_t* h_flags, const PriorCall* pr, const qldpc_prior* vp = nullptr) {
  auto* code = const_cast<qldpc_code*>(code_c);
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (batch < 0) return fail(QLDPC_EINVAL, "negative batch");
  // Before the staging copies: with `vp` every check decode_device makes
  // before its first HIP call; with `pr` the prior's own part alone, so its
  // errors come ahead of the schedule / algo / max_iter ones, which this entry
  // and the scalar one report from decode_device, behind the copies.
  if (vp) {
    if (int rc = validate_call(code, sched, algo, QLDPC_FMT_BYTES, QLDPC_FMT_BYTES, batch, p, max_iter, nullptr, vp))
      return rc;
  } else if (pr) {
    if (!sched) return fail(QLDPC_EINVAL, "code/schedule is null");
    if (int rc = validate_twin(code, sched, algo, batch, p, pr, nullptr)) return rc;
  }
  if (batch == 0) return QLDPC_OK;
  if (!h_syn || !h_ehat || !h_iters) return fail(QLDPC_EINVAL, "null host buffer");
  if (code->device < 0) return fail(QLDPC_EHIP, "no HIP device was visible when the code was created");
  std::lock_guard<std::mutex> lk(code->ws_mu);
  const int m = code->m, n = code->n;
  if (int rc = ws_reserve(code, batch, h_post != nullptr)) return rc;
  hipStream_t st = code->ws_stream;
  if (batch * m) {
    memcpy(code->hp_syn, h_syn, batch * m);
    HIP_TRY(hipMemcpyAsync(code->ws_syn, code->hp_syn, batch * m, hipMemcpyHostToDevice, st));
  }
  PriorCall dpr{};
  if (pr) {
    // the mask goes through the workspace's mask buffers, grown with it
    if (code->ws_mask_cap < code->ws_cap) {
      const size_t cn = std::max<int64_t>(1, code->ws_cap * n);
      HIP_TRY(code->ws_mask.alloc(cn));
      HIP_TRY(code->hp_mask.alloc(cn));
      code->ws_mask_cap = code->ws_cap;
    }
    if (batch * n) {
      memcpy(code->hp_mask, pr->mask, batch * n);
      HIP_TRY(hipMemcpyAsync(code->ws_mask, code->hp_mask, batch * n, hipMemcpyHostToDevice, st));
    }
    dpr = PriorCall{pr->p1, code->ws_mask.p, QLDPC_FMT_BYTES};
  }
  int rc = decode_device(code, sched, algo, code->ws_syn, QLDPC_FMT_BYTES, batch, p, max_iter, beta, eps,
                         code->ws_ehat, QLDPC_FMT_BYTES, code->ws_iters, h_post ? code->ws_post.p : nullptr,
                         code->ws_flags, st, pr ? &dpr : nullptr, vp);
  if (rc) return rc;
  if (batch * n) HIP_TRY(hipMemcpyAsync(code->hp_ehat, code->ws_ehat, batch * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_iters, code->ws_iters, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(code->hp_flags, code->ws_flags, sizeof(int32_t) * batch, hipMemcpyDeviceToHost, st));
  if (h_post && batch * n)
    HIP_TRY(hipMemcpyAsync(code->hp_post, code->ws_post, sizeof(double) * batch * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));                  // this stream only
  if (batch * n) memcpy(h_ehat, code->hp_ehat, batch * n);
  memcpy(h_iters, code->hp_iters, sizeof(int32_t) * batch);
  if (h_flags) memcpy(h_flags, code->hp_flags, sizeof(int32_t) * batch);
  if (h_post && batch * n) memcpy(h_post, code->hp_post, sizeof(double) * batch * n);
  return QLDPC_OK;
}

extern "C" int qldpc_decode_host(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                 const uint8_t* h_syn, int64_t batch, double p, int max_iter,
                                 double beta, double eps, uint8_t* h_ehat, int32_t* h_iters,
                                 double* h_post, int32_t* h_flags) {
  return decode_host(code, sched, algo, h_syn, batch, p, max_iter, beta, eps, h_ehat, h_iters, h_post, h_flags,
                     nullptr);
}

extern "C" int qldpc_decode_host_prior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                       const uint8_t* h_syn, int64_t batch, double p0, double p1,
                                       const uint8_t* h_mask, int max_iter, double beta, double eps,
                                       uint8_t* h_ehat, int32_t* h_iters, double* h_post, int32_t* h_flags) {
  const PriorCall pr{p1, h_mask, QLDPC_FMT_BYTES};
  return decode_host(code, sched, algo, h_syn, batch, p0, max_iter, beta, eps, h_ehat, h_iters, h_post, h_flags,
                     &pr);
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
  return decode_device(code, sched, algo, d_syn, syn_format, batch, 0.0, max_iter, beta, prior->eps, d_ehat,
                       ehat_format, d_iters, d_post, d_flags, stream, nullptr, prior);
}

extern "C" int qldpc_decode_host_vprior(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                        const uint8_t* h_syn, int64_t batch, const qldpc_prior* prior, int max_iter,
                                        double beta, uint8_t* h_ehat, int32_t* h_iters, double* h_post,
                                        int32_t* h_flags) {
  if (!prior) return fail(QLDPC_EINVAL, "prior handle is null");
  return decode_host(code, sched, algo, h_syn, batch, 0.0, max_iter, beta, prior->eps, h_ehat, h_iters, h_post,
                     h_flags, nullptr, prior);
}

extern "C" int qldpc_decode_vprior_kernel_name(const qldpc_code* code, const qldpc_schedule* sched, int algo,
                                               char* buf, int len) {
  return twin_kernel_name(code, sched, algo, PLAN_VPRIOR, buf, len);
}

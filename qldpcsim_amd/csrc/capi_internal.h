// capi_internal.h — private to the host translation units of the C ABI
// (capi*.cpp): errors, options, owning device buffers, the part every launch
// plan shares, the half-shot queue ring, and the definitions of qldpc_code /
// qldpc_schedule. What a launch does with them is in capi_launch.h. Nothing
// declared in namespace capi is exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qldpc_decoder.h"
#include "decoder_kernels.h"
#include "hard_kernels.h"
#include "hbm_kernels.h"

#pragma GCC visibility push(hidden)
namespace capi {

// ---------------------------------------------------------------------------
// errors (capi.cpp)
// ---------------------------------------------------------------------------
extern thread_local std::string g_err;
int fail(int code, const char* fmt, ...);

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t _e = (expr);                                                                 \
    if (_e != hipSuccess)                                                                   \
      return capi::fail(QLDPC_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),  \
                        __FILE__, __LINE__);                                                \
  } while (0)

// ---------------------------------------------------------------------------
// options (include/qldpc_decoder.h; capi.cpp): read at launch, never from the
// environment; `gen` changes with every set so cached launch plans are rebuilt
// ---------------------------------------------------------------------------
struct Options {
  std::atomic<int64_t> force_hbm{0}, flood_generic{0}, layered_generic{0}, ms_lanes_per_check{0}, bp_wave{0},
      bp_lg{1}, bp_team_w{0}, static_sched{0}, waves_per_wg{0}, wg_per_cu{0}, osd_column{0}, osd_tickets{1},
      osd_prof{0}, osd_hbm{0}, logical_tabs{0}, flood_qc{1}, vprior_hbm{0};
  std::atomic<uint32_t> gen{1};
};
extern Options g_opt;
inline int64_t opt(std::atomic<int64_t> Options::*slot) { return (g_opt.*slot).load(std::memory_order_relaxed); }

// ---------------------------------------------------------------------------
// Owning device buffer (kPinned: page-locked host memory instead). Move-only;
// freed by the destructor, so a create that fails half way leaks nothing.
// ---------------------------------------------------------------------------
template <typename T, bool kPinned = false>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
  }
  hipError_t alloc(size_t count) {
    reset();
    return kPinned ? hipHostMalloc((void**)&p, sizeof(T) * count) : hipMalloc((void**)&p, sizeof(T) * count);
  }
  // an empty table still gets one element, so its pointer is never null
  hipError_t upload(const std::vector<T>& h) {
    hipError_t e = alloc(std::max<size_t>(h.size(), 1));
    if (e == hipSuccess && !h.empty()) e = hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice);
    return e;
  }
  operator T*() const { return p; }
};
template <typename T>
using PinBuf = DevBuf<T, true>;

inline int align16(int x) { return (x + 15) & ~15; }

// ---------------------------------------------------------------------------
// One table image of a schedule: the bytes a kernel family reads its graph
// tables from, and where each table starts, named as DecodeArgs names them.
// A family that gives a DecodeArgs field another meaning says so where its
// image is built (capi_schedule.cpp); fields it does not read keep the
// generic image's values.
// ---------------------------------------------------------------------------
struct TableOffsets {  // DecodeArgs::off_<name>
  int cn_tab = 0, row_ptr = 0, vn_ptr = 0, vn_chk = 0, lay_ptr = 0, lay_rows = 0, adj_ptr = 0, adj_vars = 0,
      chunk_dmax = 0;
};
struct TableImage {
  std::vector<uint8_t> bytes;      // host copy
  DevBuf<unsigned char> dev;       // device copy (DecodeArgs::blob)
  int lds_bytes = 0;               // bytes [lds_skip, lds_skip + lds_bytes) are staged into LDS
  int lds_skip = 0;
  TableOffsets off;

  bool empty() const { return bytes.empty(); }
  template <typename T>
  int put(const std::vector<T>& v) {               // append at the next multiple of 16; returns the offset
    const int off = align16((int)bytes.size());
    bytes.resize(off + sizeof(T) * v.size());
    if (!v.empty()) memcpy(bytes.data() + off, v.data(), sizeof(T) * v.size());
    return off;
  }
  int seal() {                                     // pad to a multiple of 16, never empty; returns the size
    bytes.resize(align16((int)bytes.size() + 1));
    return (int)bytes.size();
  }
};

// What every family's launch plan starts with: the kernel, its geometry and the option generation (cached_plan)
struct PlanBase {
  const void* kernel = nullptr;
  const char* name = "";    // as rocprofv3 reports it
  int waves = 0, blocks_per_cu = 0, lds = 0;   // waves per workgroup, workgroups per CU, LDS bytes
  int cus = 0;              // compute units of the device
  uint32_t gen = 0;         // g_opt.gen the plan was built under
  bool ok = false;
};

// Half-shot work-queue counters: concurrent launches take different slots, each zeroed on the launch stream
struct QueueRing {
  static constexpr int kSlots = 64;
  DevBuf<uint32_t> buf;     // [kSlots], allocated and zeroed by the owner
  std::atomic<uint32_t> next{0};
  int claim(hipStream_t st, uint32_t** slot);   // capi_launch.cpp
};

// ---------------------------------------------------------------------------
// Launch plan of (schedule, algo) under one option generation: everything a
// decode launch needs that does not depend on the call (capi_decode.cpp)
// ---------------------------------------------------------------------------
enum KernelFamily { FAM_GENERIC, FAM_MS_FLOOD, FAM_MS_FLOOD_QC, FAM_MS_LAYERED, FAM_BP_TEAM, FAM_BP_TEAM_LG };
// Which priors a launch takes: one scalar, or one of the generic LDS kernel's
// twins (decode_prior_kernel, decode_vprior_kernel). Indexes qldpc_schedule::plan.
enum PlanKind { PLAN_SCALAR = 0, PLAN_PRIOR = 1, PLAN_VPRIOR = 2 };

struct KernelChoice {
  const void* kernel = nullptr;
  const char* name = "";    // as rocprofv3 reports it
  KernelFamily family = FAM_GENERIC;
  int team = 0;             // BP teams: waves per half-shot (one workgroup), 0 = wave kernels
  int lanes = 0;            // ms_layered_kernel: lanes per check, 0 = chosen per layer
  int max_waves = 0;        // most waves per workgroup the kernel was compiled for
  int qc_table = -1;        // FAM_MS_FLOOD_QC: the generated table H expands from (qc_tables.h)
  // PLAN_PRIOR (decode_prior_kernel): the wave slice also holds the selector
  // bits; PLAN_VPRIOR (decode_vprior_kernel): the prior row lies behind the graph image
  PlanKind kind = PLAN_SCALAR;
  // PLAN_VPRIOR under option vprior_hbm, past the LDS twin's limits (or with
  // force_hbm): hbm_tile_vprior_kernel; `kernel` and `name` are that instance's
  bool hbm = false;
};

struct LaunchPlan : PlanBase {   // (waves, blocks_per_cu, lds: the LDS kernels'; 0 on the HBM path)
  // hbm_tile_kernel (PLAN_VPRIOR: hbm_tile_vprior_kernel) decodes: the LDS
  // kernels cannot hold this schedule, or force_hbm
  bool hbm = false;
  int team = 0;             // BP teams: waves per half-shot
  int hs_per_wave = 1;      // half-shots a wave decodes at a time (register-resident ms_flood_kernel: 4)
  qldpc::DecodeArgs args{};  // every static field filled (LDS kernels)
  qldpc::HbmArgs hargs{};    // the same for hbm_tile_kernel
  int hbm_tiles_cap = 0;    // CUs x resident 64-slot tiles per CU
  size_t hbm_lds = 0;       // hbm_tile_kernel / hbm_tile_vprior_kernel, BP: dynamic LDS bytes (qldpc::hbm_vprior_lds; 0 up to 128 entries per column)
};

// Launch plan of (code, NG | BF) under one option generation (capi_hard.cpp):
// the hard-decision kernels need no schedule, so the plan belongs to the code
struct HardPlan : PlanBase {
  qldpc::HardArgs args{};    // every static field filled
};

}  // namespace capi
#pragma GCC visibility pop

// ---------------------------------------------------------------------------
// code (Tanner graph; capi_code.cpp)
// ---------------------------------------------------------------------------
struct qldpc_code {
  int m = 0, n = 0, E = 0, device = 0;
  int uniform_deg = 0;  // row degree if every row has it, else 0
  int max_row_deg = 0, max_col_deg = 0;
  // GF(2) rank of H (gf2math.rank) and column bit-vectors, for OSD only:
  // built on first use (code_osd_prep), a large code may never need them
  mutable std::once_flag osd_once;
  mutable int rank = -1;
  bool zero_col = false;  // H has an all-zero column (GPU OSD: exact REF kernel only)
  // the LDS-resident kernels' 16-bit tables hold this code (m, n, E <= 65535);
  // otherwise every decode takes the HBM-resident kernel
  bool lds_ok = true;
  std::vector<int32_t> row_ptr, col_idx;     // CSR, np.where(H) order
  std::vector<int32_t> vperm, vinv;          // relabeled -> original, original -> relabeled
  std::vector<int32_t> csc_ptr, csc_edge;    // relabeled-variable CSC: CSR edge ids, ascending check
  std::vector<int32_t> edge_pos;             // CSR edge -> CSC position
  int mw = 0;                                // 64-bit words per column bit-vector
  mutable std::vector<uint64_t> col_bits;    // [n][mw] column j of H (OSD)
  capi::DevBuf<uint16_t> d_vinv;
  capi::DevBuf<uint16_t> d_vperm;            // relabeled -> original (decode_prior_kernel's mask gather)
  // HBM-resident kernel: 32-bit graph tables (relabeled variables)
  capi::DevBuf<int32_t> d_row_var, d_row_pos, d_col_ptr, d_vinv32;
  capi::DevBuf<int32_t> d_row_ptr, d_col_idx;  // CSR for the GPU OSD
  // layered MS stop-test filters (ms_layered_kernel): 32 fixed random parity
  // checks of H's rows; wc[c] bit k = row c in check k, avar[v] bit k = parity
  // of the rows of check k that hold relabeled variable v
  std::vector<uint32_t> wc, avar;
  uint32_t filt_all = 0;
  capi::DevBuf<uint32_t> d_wc, d_rtab;  // rtab: [m][8] relabeled variables per row
  capi::DevBuf<uint32_t> d_avar;        // [n] filter word per relabeled variable (layered BP)
  // host staging workspace of every *_host entry (staged_call, capi_launch.h): device buffers,
  // page-locked host mirrors (DMA copies) and a stream of its own (no device-wide sync)
  std::mutex ws_mu;
  int64_t ws_cap = 0, ws_post_cap = 0;   // half-shots held; of those, with posterior buffers
  capi::DevBuf<uint8_t> ws_syn, ws_ehat;
  capi::DevBuf<int32_t> ws_iters, ws_flags;
  capi::DevBuf<double> ws_post;
  capi::PinBuf<uint8_t> hp_syn, hp_ehat;
  capi::PinBuf<int32_t> hp_iters, hp_flags;
  capi::PinBuf<double> hp_post;
  int64_t ws_mask_cap = 0;               // half-shots the mask buffers hold (qldpc_decode_host_prior)
  capi::DevBuf<uint8_t> ws_mask;
  capi::PinBuf<uint8_t> hp_mask;
  hipStream_t ws_stream = nullptr;
  // hard-decision decoders (capi_hard.cpp), under hard_mu: 16-bit CSR / CSC
  // tables in original variable labels (row_ell | col_ell | row_ptr | row_var |
  // col_ptr | col_chk),
  // uploaded on first use; the launch plans per algo; a half-shot queue ring
  // as qldpc_schedule's
  std::mutex hard_mu;
  capi::DevBuf<uint16_t> d_hard_tab;
  capi::QueueRing hard_queue;
  capi::HardPlan hard_plan[2];   // [algo - QLDPC_ALGO_NG]
};

// ---------------------------------------------------------------------------
// per-variable priors of one code (capi_decode.cpp)
// ---------------------------------------------------------------------------
struct qldpc_prior {
  const qldpc_code* code = nullptr;
  int m = 0, n = 0, E = 0;       // the code's shape when the row was formed
  double eps = 0.0;
  std::vector<double> L;         // [n] L_j = log((1 - p_j) / max(p_j, eps)), relabeled variable order
  capi::DevBuf<double> d_L;
  std::vector<int64_t> W;        // [n] llrint(L_j 2^20): relay_vprior_kernel's solution weights
  capi::DevBuf<int64_t> d_W;
  std::vector<int64_t> Wo;       // [n] the same weights by original column: OSD-CS's prior cost indexes them
  capi::DevBuf<int64_t> d_Wo;    // through perm
  uint32_t filt0 = 0;           // prior_filter_word(code, L): hbm_tile_vprior_kernel's filter word at start
};

// ---------------------------------------------------------------------------
// schedule (layers) and its table images (capi_schedule.cpp)
// ---------------------------------------------------------------------------
struct qldpc_schedule {
  const qldpc_code* code = nullptr;
  bool layered = false;
  int n_layers = 0;
  int layer_g = 0;            // lanes per check shared by every layer, 0 = chosen per layer
  capi::TableImage generic;      // every wave kernel and bp_team_kernel: the whole image in LDS
  capi::TableImage layered_ms;   // ms_layered_kernel, uniform degree: layer-ordered tables
  capi::TableImage layered_bp;   // bp_team_lg_kernel: layer pointers in LDS, every table global
  capi::TableImage flood_ms;     // ms_flood_kernel, uniform degree: global tables, no LDS image
  capi::LaunchPlan plan[3][2];   // [PlanKind][algo], under mu
  std::mutex mu;
  // HBM-resident kernel (hbm_kernels.hip): 32-bit layer tables and a grow-only
  // slot-major workspace; hbm_ev orders launches that share the workspace
  bool lds_ok = true;         // the LDS kernels' 16-bit layer tables hold this schedule
  bool hbm_lazy = false;      // every row in exactly one layer (no state init pass)
  std::vector<int32_t> h_lay_ptr, h_lay_rows, h_adj_ptr, h_adj_vars, h_fl_var, h_fl_pos;
  capi::DevBuf<int32_t> d_h_lay_ptr, d_h_lay_rows, d_h_adj_ptr, d_h_adj_vars, d_h_fl_var, d_h_fl_pos;
  void* hbm_ws = nullptr;
  size_t hbm_ws_bytes = 0;
  hipEvent_t hbm_ev = nullptr;
  capi::QueueRing queue;      // half-shot work-queue counters
};

#pragma GCC visibility push(hidden)
namespace capi {

// Uniform row degree 7 or 8 with LDS offsets that fit 16 bits -> the
// unrolled kernel instantiation and its pre-scaled table format.
inline bool fast_table_ok(const qldpc_code* c) {
  return (c->uniform_deg == 7 || c->uniform_deg == 8) && 8 * c->n < 65536 && 8 * c->E < 65536;
}

// capi_code.cpp: OSD's column bit-vectors and rank(H), built once on first OSD use
void code_osd_prep(const qldpc_code* c);

// capi_osd_host.cpp
struct Gf2Basis {
  int mw;
  std::vector<uint64_t> vec;  // [m][mw], slot b holds a vector whose lowest set bit is b
  std::vector<char> has;
  Gf2Basis(int m, int mw_) : mw(mw_), vec((size_t)std::max(m, 1) * std::max(mw_, 1), 0), has(std::max(m, 1), 0) {}
  bool insert(uint64_t* x);   // true if x (modified) was independent and got inserted
};
// QLDPC_EINVAL unless `prior` is a handle built for `code` (the _cs_prior entry points, host and device)
int osd_cs_prior_checked(const qldpc_code* code, const qldpc_prior* prior);

// capi_decode.cpp. choose_kernel and plan_static call no HIP function: the
// static kernel arguments can be checked on a machine without a device.
KernelChoice choose_kernel(const qldpc_schedule* s, int algo);
// decode_prior_kernel (PLAN_PRIOR) or decode_vprior_kernel (PLAN_VPRIOR) for
// (schedule, algo): QLDPC_EUNSUP where the generic LDS kernel cannot run the
// code (16-bit tables, MS row degree > 32, BP column degree > 128) or option
// force_hbm is set; calls no HIP function. PLAN_VPRIOR with option vprior_hbm
// set: those cases take hbm_tile_vprior_kernel instead (k->hbm)
int choose_twin_kernel(const qldpc_schedule* s, int algo, PlanKind kind, KernelChoice* k);
// The generated protograph table (qc_tables.h) whose expansion is exactly the
// code's H, or -1: compared entry by entry, not by shape or hash
int qc_table_of(const qldpc_code* c);
// Fills every static DecodeArgs field but off_libm (plan_lds); returns the
// LDS bytes the kernel keeps in front of the state slices.
int plan_static(const qldpc_schedule* s, int algo, const KernelChoice& k, qldpc::DecodeArgs* a);
// LDS bytes of a workgroup of `waves` waves; sets a->off_libm
int plan_lds(int algo, int image_lds, int team, int waves, qldpc::DecodeArgs* a);
void plan_static_hbm(const qldpc_schedule* s, qldpc::HbmArgs* a);
// XOR of the stop-test filter words avar[v] over the relabeled variables whose
// prior L[v] is negative: the filters of a decode whose posteriors all stand at
// their priors (hbm_tile_vprior_kernel's HbmArgs::filt0); calls no HIP function
uint32_t prior_filter_word(const qldpc_code* c, const std::vector<double>& L);

// capi_hard.cpp. Calls no HIP function: the per-wave LDS layout of the
// hard-decision kernels (every HardArgs field that depends on the code's
// shape alone); returns QLDPC_EUNSUP past the 16-bit tables.
int hard_layout(const qldpc_code* c, int algo, qldpc::HardArgs* a);

}  // namespace capi
#pragma GCC visibility pop

// launch_host_check.cpp — the launch plumbing every decoder family shares
// (qldpcsim_amd/csrc/capi_launch.h) under a sanitizer, without a device and
// without Python: the occupancy search over workgroup widths driven by fake
// occupancy tables, the launch-plan cache with a counting builder, the grid
// size and the LDS-limit predicate. Built as relay_vprior_host_check.cpp is,
// from the library's own translation units, the kernel units compiled once
// without the sanitizer (objects first on the line):
//   cd qldpcsim_amd/csrc && for f in *_kernels.hip; do hipcc --offload-arch=gfx950 -O1 -std=c++17 -fPIC \
//     -ffp-contract=off -c $f -o /tmp/$f.o; done && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -ffp-contract=off -Xarch_host -fsanitize=address,undefined /tmp/*_kernels.hip.o \
//     ../../tools/probe/launch_host_check.cpp capi*.cpp np_order.cpp -o launch_host_check && \
//     ./launch_host_check
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <map>
#include <vector>

#include "../../qldpcsim_amd/csrc/capi_launch.h"

using namespace capi;

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, qldpc_last_error()); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

// A fake device: blocks per CU by width (absent: 0), widths whose query fails,
// and every width that was asked
struct FakeDevice {
  std::map<int, int> blocks;
  std::vector<int> failing, asked;
  hipError_t operator()(int w, int lds, int* nb) {
    (void)lds;
    asked.push_back(w);
    for (int f : failing)
      if (f == w) return hipErrorInvalidValue;
    *nb = blocks.count(w) ? blocks[w] : 0;
    return hipSuccess;
  }
};

static void set_opts(int64_t waves_per_wg, int64_t wg_per_cu) {
  CHECK(qldpc_set_option("waves_per_wg", waves_per_wg) == QLDPC_OK);
  CHECK(qldpc_set_option("wg_per_cu", wg_per_cu) == QLDPC_OK);
}

static WaveChoice search(FakeDevice& dev, int lo, int hi, int max_lds, bool overrides, hipError_t want = hipSuccess) {
  WaveChoice wc{7, 7, 7};
  dev.asked.clear();
  CHECK(wave_search(lo, hi, max_lds, [](int w) { return 100 + 1000 * w; }, std::ref(dev), overrides, &wc) == want);
  return wc;
}

static void check_wave_search() {
  // most resident waves wins; on a tie (4 x 2 = 8 x 1 = 2 x 4) the wider workgroup
  FakeDevice dev;
  dev.blocks = {{8, 1}, {4, 2}, {2, 4}, {1, 5}, {3, 2}};
  WaveChoice wc = search(dev, 1, 8, 1 << 20, true);
  CHECK(wc.waves == 8 && wc.blocks_per_cu == 1 && wc.lds == 8100);
  CHECK((dev.asked == std::vector<int>{8, 7, 6, 5, 4, 3, 2, 1}));
  dev.blocks[1] = 9;
  wc = search(dev, 1, 8, 1 << 20, true);
  CHECK(wc.waves == 1 && wc.blocks_per_cu == 9 && wc.lds == 1100);
  // a width past the LDS limit is never asked about
  wc = search(dev, 1, 8, 4100, true);
  CHECK((dev.asked == std::vector<int>{4, 3, 2, 1}) && wc.waves == 1);
  dev.blocks[1] = 5;
  wc = search(dev, 1, 8, 4100, true);
  CHECK(wc.waves == 4 && wc.blocks_per_cu == 2 && wc.lds == 4100);
  // nothing fits, or nothing is resident: zeros
  wc = search(dev, 1, 8, 1099, true);
  CHECK(dev.asked.empty() && wc.waves == 0 && wc.blocks_per_cu == 0 && wc.lds == 0);
  FakeDevice none;
  wc = search(none, 1, 8, 1 << 20, true);
  CHECK(none.asked.size() == 8 && wc.waves == 0 && wc.blocks_per_cu == 0 && wc.lds == 0);
  // a failing query ends the search with its error
  FakeDevice bad = dev;
  bad.failing = {5};
  (void)search(bad, 1, 8, 1 << 20, true, hipErrorInvalidValue);
  CHECK((bad.asked == std::vector<int>{8, 7, 6, 5}));
  // one width (a team): that width or nothing
  wc = search(dev, 4, 4, 1 << 20, true);
  CHECK((dev.asked == std::vector<int>{4}) && wc.waves == 4 && wc.blocks_per_cu == 2);
  wc = search(dev, 6, 6, 1 << 20, true);
  CHECK(wc.waves == 0 && wc.blocks_per_cu == 0 && wc.lds == 0);

  // waves_per_wg: taken when in range, fitting, answered and resident
  set_opts(2, 0);
  wc = search(dev, 1, 8, 1 << 20, true);
  CHECK(wc.waves == 2 && wc.blocks_per_cu == 4 && wc.lds == 2100);
  wc = search(dev, 1, 8, 1 << 20, false);               // the flag switches it off
  CHECK(wc.waves == 8 && wc.blocks_per_cu == 1);
  wc = search(dev, 4, 4, 1 << 20, true);                // out of a team's range
  CHECK(wc.waves == 4 && wc.blocks_per_cu == 2);
  for (int64_t w : {-1, 9, 99}) {                       // out of range
    set_opts(w, 0);
    wc = search(dev, 1, 8, 1 << 20, true);
    CHECK(wc.waves == 8 && wc.blocks_per_cu == 1 && dev.asked.size() == 8);
  }
  set_opts(8, 0);                                       // does not fit
  wc = search(dev, 1, 8, 4100, true);
  CHECK(wc.waves == 4 && dev.asked.size() == 4);
  set_opts(6, 0);                                       // nb == 0
  wc = search(dev, 1, 8, 1 << 20, true);
  CHECK(wc.waves == 8 && wc.blocks_per_cu == 1);
  // its own query fails (the search's query of that width did not): ignored
  struct FailSecond {
    FakeDevice* d;
    int seen = 0;
    hipError_t operator()(int w, int lds, int* nb) { return w == 3 && seen++ ? hipErrorInvalidValue : (*d)(w, lds, nb); }
  } second{&dev};
  set_opts(3, 0);
  wc = WaveChoice{};
  CHECK(wave_search(1, 8, 1 << 20, [](int w) { return 100 + 1000 * w; }, std::ref(second), true, &wc) == hipSuccess);
  CHECK(second.seen == 2 && wc.waves == 8 && wc.blocks_per_cu == 1);

  // wg_per_cu only lowers blocks_per_cu, never below 1
  dev.blocks[1] = 9;
  for (int64_t k : {0, -3, 9, 10, 1000}) {
    set_opts(0, k);
    wc = search(dev, 1, 8, 1 << 20, true);
    CHECK(wc.waves == 1 && wc.blocks_per_cu == 9);
  }
  for (int64_t k : {1, 4, 8}) {
    set_opts(0, k);
    wc = search(dev, 1, 8, 1 << 20, true);
    CHECK(wc.waves == 1 && wc.blocks_per_cu == (int)k && wc.lds == 1100);
    wc = search(dev, 1, 8, 1 << 20, false);
    CHECK(wc.waves == 1 && wc.blocks_per_cu == 9);
  }
  set_opts(2, 3);                                       // both: the width, then the cap on its blocks
  wc = search(dev, 1, 8, 1 << 20, true);
  CHECK(wc.waves == 2 && wc.blocks_per_cu == 3 && wc.lds == 2100);
  wc = search(dev, 1, 8, 1 << 20, false);
  CHECK(wc.waves == 1 && wc.blocks_per_cu == 9);
  set_opts(0, 0);
}

struct CountedPlan : PlanBase {
  int payload = 0;
};

static void check_plan_cache() {
  std::mutex mu;
  CountedPlan slot, out;
  int builds = 0, rc = QLDPC_OK;
  auto build = [&](CountedPlan* p) {
    p->payload = ++builds;
    p->waves = 4;
    return rc;
  };
  CHECK(cached_plan(mu, slot, &out, build) == QLDPC_OK && builds == 1 && out.payload == 1 && out.ok && out.waves == 4);
  CHECK(cached_plan(mu, slot, &out, build) == QLDPC_OK && builds == 1 && out.payload == 1);
  const uint32_t gen = out.gen;
  CHECK(qldpc_set_option("bp_wave", 1) == QLDPC_OK);
  CHECK(cached_plan(mu, slot, &out, build) == QLDPC_OK && builds == 2 && out.payload == 2 && out.gen != gen);
  CHECK(cached_plan(mu, slot, &out, build) == QLDPC_OK && builds == 2);
  // a failing build: its code comes back, neither the slot nor *out changes,
  // and the next call builds again
  CHECK(qldpc_set_option("bp_wave", 0) == QLDPC_OK);
  rc = QLDPC_EUNSUP;
  CHECK(cached_plan(mu, slot, &out, build) == QLDPC_EUNSUP && builds == 3 && slot.payload == 2 && out.payload == 2);
  rc = QLDPC_OK;
  CHECK(cached_plan(mu, slot, &out, build) == QLDPC_OK && builds == 4 && slot.payload == 4 && out.payload == 4);
  CountedPlan fresh, none;
  rc = QLDPC_EHIP;
  CHECK(cached_plan(mu, fresh, &none, build) == QLDPC_EHIP && !fresh.ok && fresh.payload == 0 && !none.ok);
}

static void check_launch_grid() {
  CHECK(launch_grid(0, 4, 2, 256) == 1);
  CHECK(launch_grid(1, 4, 2, 256) == 1);
  CHECK(launch_grid(4, 4, 2, 256) == 1 && launch_grid(5, 4, 2, 256) == 2 && launch_grid(8, 4, 2, 256) == 2);
  CHECK(launch_grid(2048, 4, 2, 256) == 512 && launch_grid(2047, 4, 2, 256) == 512 && launch_grid(2044, 4, 2, 256) == 511);
  CHECK(launch_grid(2049, 4, 2, 256) == 512 && launch_grid((int64_t)1 << 40, 1, 2, 256) == 512);
  CHECK(launch_grid(7, 1, 3, 5) == 7 && launch_grid(16, 1, 3, 5) == 15);
  CHECK(launch_grid(100, 4, 0, 256) == 1);              // (no resident block: still one workgroup)
}

// m x n with row 0 and column 0 full: row degree n, column degree m
static qldpc_code* cross(int m, int n) {
  std::vector<uint8_t> H((size_t)m * n, 0);
  for (int j = 0; j < n; ++j) H[j] = 1;
  for (int i = 0; i < m; ++i) H[(size_t)i * n] = 1;
  qldpc_code* c = nullptr;
  CHECK(qldpc_code_create(H.data(), m, n, &c) == QLDPC_OK);
  CHECK(c->max_row_deg == n && c->max_col_deg == m);
  return c;
}

static void check_lds_limit() {
  const uint8_t H[3 * 7] = {0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1};
  qldpc_code* code = nullptr;
  CHECK(qldpc_code_create(H, 3, 7, &code) == QLDPC_OK);
  for (int algo : {QLDPC_ALGO_MS, QLDPC_ALGO_BP}) {
    CHECK(lds_limit(code->lds_ok, code, algo) == LDS_FITS);
    CHECK(lds_limit(false, code, algo) == LDS_TABLES16);
    CHECK(qldpc_set_option("force_hbm", 1) == QLDPC_OK);
    CHECK(lds_limit(true, code, algo) == LDS_FORCE_HBM);
    CHECK(lds_limit(false, code, algo) == LDS_TABLES16);  // the tables come first
    CHECK(qldpc_set_option("force_hbm", 0) == QLDPC_OK);
  }
  CHECK(qldpc_code_destroy(code) == QLDPC_OK);
  // the row limit is min-sum's, the column limit BP's
  struct { int m, n; LdsLimit ms, bp; } shapes[] = {{2, 32, LDS_FITS, LDS_FITS},
                                                   {2, 33, LDS_MS_ROW_DEG, LDS_FITS},
                                                   {128, 2, LDS_FITS, LDS_FITS},
                                                   {129, 2, LDS_FITS, LDS_BP_COL_DEG},
                                                   {129, 33, LDS_MS_ROW_DEG, LDS_BP_COL_DEG}};
  for (const auto& s : shapes) {
    qldpc_code* c = cross(s.m, s.n);
    CHECK(lds_limit(c->lds_ok, c, QLDPC_ALGO_MS) == s.ms && lds_limit(c->lds_ok, c, QLDPC_ALGO_BP) == s.bp);
    CHECK(qldpc_set_option("force_hbm", 1) == QLDPC_OK);  // a degree limit is named ahead of the option
    CHECK(lds_limit(c->lds_ok, c, QLDPC_ALGO_MS) == (s.ms ? s.ms : LDS_FORCE_HBM));
    CHECK(lds_limit(c->lds_ok, c, QLDPC_ALGO_BP) == (s.bp ? s.bp : LDS_FORCE_HBM));
    CHECK(qldpc_set_option("force_hbm", 0) == QLDPC_OK);
    CHECK(qldpc_code_destroy(c) == QLDPC_OK);
  }
}

int main() {
  check_wave_search();
  check_plan_cache();
  check_launch_grid();
  check_lds_limit();
  std::puts("launch_host_check OK");
  return 0;
}

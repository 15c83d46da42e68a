// capi.cpp — C ABI (include/qldpc_decoder.h): errors, version and options.
// The rest of the host layer, one translation unit per concern:
//   capi_code.cpp        Tanner graph of one H, built and uploaded once
//   capi_schedule.cpp    layer schedules and their table images
//   capi_decode.cpp      launch plans, decode entry points, timing, HBM path
//   capi_osd_host.cpp    host OSD (bit-packed GF(2))
//   capi_osd_device.cpp  GPU OSD launchers
//   capi_channel.cpp     channel sampler, outcome counters, logical operators
// capi_internal.h holds what they share.

#include <cstdarg>
#include <cstdio>

#include "capi_internal.h"

namespace capi {
thread_local std::string g_err;
Options g_opt;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
}  // namespace capi
using namespace capi;

extern "C" const char* qldpc_last_error(void) { return g_err.c_str(); }
extern "C" const char* qldpc_version(void) { return "qldpcsim_amd 0.1.0 (gfx950)"; }

extern "C" int qldpc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

static std::atomic<int64_t>* option_slot(const char* name) {
  if (!name) return nullptr;
  static const struct {
    const char* name;
    std::atomic<int64_t> Options::*slot;
  } table[] = {{"force_hbm", &Options::force_hbm},     {"flood_generic", &Options::flood_generic},
               {"layered_generic", &Options::layered_generic},
               {"ms_lanes_per_check", &Options::ms_lanes_per_check},
               {"bp_wave", &Options::bp_wave},         {"bp_lg", &Options::bp_lg},
               {"bp_team_w", &Options::bp_team_w},     {"static_sched", &Options::static_sched},
               {"waves_per_wg", &Options::waves_per_wg}, {"wg_per_cu", &Options::wg_per_cu},
               {"osd_column", &Options::osd_column},   {"osd_tickets", &Options::osd_tickets},
               {"osd_prof", &Options::osd_prof},       {"osd_hbm", &Options::osd_hbm},
               {"logical_tabs", &Options::logical_tabs}, {"flood_qc", &Options::flood_qc},
               {"vprior_hbm", &Options::vprior_hbm}};
  for (const auto& e : table)
    if (strcmp(e.name, name) == 0) return &(g_opt.*(e.slot));
  return nullptr;
}

extern "C" int qldpc_set_option(const char* name, int64_t value) {
  std::atomic<int64_t>* o = option_slot(name);
  if (!o) return fail(QLDPC_EINVAL, "unknown option %s", name ? name : "(null)");
  o->store(value);
  g_opt.gen.fetch_add(1);
  return QLDPC_OK;
}

extern "C" int qldpc_get_option(const char* name, int64_t* value) {
  std::atomic<int64_t>* o = option_slot(name);
  if (!o || !value) return fail(QLDPC_EINVAL, "unknown option %s", name ? name : "(null)");
  *value = o->load();
  return QLDPC_OK;
}

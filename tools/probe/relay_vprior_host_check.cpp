// relay_vprior_host_check.cpp — the host side of relay min-sum with
// per-variable priors under a sanitizer, without a device
// and without Python: the weight row formed with the prior handle
// (W_j = llrint(L_j 2^20), relabeled order), relay_vprior_kernel's name and
// LDS layout (neither needs a device), and every validation path of the two
// decode entry points that returns before a HIP call. Built as
// vprior_hbm_host_check.cpp is, from the library's own translation units, the
// kernel units compiled once without the sanitizer (objects first on the line):
//   cd qldpcsim_amd/csrc && for f in *_kernels.hip; do hipcc --offload-arch=gfx950 -O1 -std=c++17 -fPIC \
//     -ffp-contract=off -c $f -o /tmp/$f.o; done && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -ffp-contract=off -Xarch_host -fsanitize=address,undefined /tmp/*_kernels.hip.o \
//     ../../tools/probe/relay_vprior_host_check.cpp capi*.cpp np_order.cpp -o relay_vprior_host_check && \
//     ./relay_vprior_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../qldpcsim_amd/csrc/capi_internal.h"

#define CHECK(cond)                                                       \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "%s:%d: %s failed (%s)\n", __FILE__, __LINE__, #cond, qldpc_last_error()); \
      std::exit(1);                                                       \
    }                                                                     \
  } while (0)

int main() {
  const uint8_t H[3 * 7] = {0, 0, 0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 0, 1, 0, 1, 0, 1};
  qldpc_code *code = nullptr, *other = nullptr;
  CHECK(qldpc_code_create(H, 3, 7, &code) == QLDPC_OK);
  CHECK(qldpc_code_create(H, 3, 7, &other) == QLDPC_OK);
  const int n = 7;

  // the weight row: one int64 per relabeled variable, round-half-even of
  // L_j 2^20 (exact scaling), negative where p_j > 1/2
  const double p[n] = {0.01, 0.6, 0.2, 0.0, 0.5, 0.999, 0.03};
  qldpc_prior *pr = nullptr, *pr_other = nullptr, *pr_eps = nullptr;
  CHECK(qldpc_prior_create(code, p, 1e-9, &pr) == QLDPC_OK);
  CHECK(qldpc_prior_create(other, p, 1e-9, &pr_other) == QLDPC_OK);
  CHECK(qldpc_prior_create(code, p, 1e-6, &pr_eps) == QLDPC_OK);
  CHECK((int)pr->W.size() == n && (int)pr->L.size() == n);
  for (int j = 0; j < n; ++j) {
    const double scaled = pr->L[j] * 1048576.0;
    CHECK(pr->W[j] == (int64_t)std::nearbyint(scaled));
    CHECK(std::fabs((double)pr->W[j] - scaled) <= 0.5);
    CHECK((pr->W[j] < 0) == (p[code->vperm[j]] > 0.5));
  }
  CHECK(pr_eps->W != pr->W);                             // p = 0: the row depends on eps

  // the relay handle, the kernel's name and its layout: the scalar image plus
  // the row, the same slice
  const int32_t T[2] = {3, 4};
  std::vector<double> G(2 * n, 0.1);
  qldpc_relay* rl = nullptr;
  CHECK(qldpc_relay_create(code, 2, T, G.data(), n, 2, &rl) == QLDPC_OK);
  char name[64] = "";
  CHECK(qldpc_decode_relay_vprior_kernel_name(code, rl, name, 64) == QLDPC_OK);
  CHECK(std::strcmp(name, "relay_vprior_kernel<0>") == 0);
  CHECK(qldpc_decode_relay_kernel_name(code, rl, name, 64) == QLDPC_OK);
  CHECK(std::strcmp(name, "relay_ms_kernel<0>") == 0);
  CHECK(qldpc_decode_relay_vprior_kernel_name(other, rl, name, 64) == QLDPC_EINVAL);
  CHECK(qldpc_decode_relay_vprior_kernel_name(code, nullptr, name, 64) == QLDPC_EINVAL);
  int32_t a[7], b[7];
  CHECK(qldpc_relay_layout(rl, a) == QLDPC_OK && qldpc_relay_vprior_layout(rl, b) == QLDPC_OK);
  CHECK(b[0] == a[0] + ((8 * n + 15) & ~15));
  for (int k = 1; k < 7; ++k) CHECK(a[k] == b[k]);
  CHECK(qldpc_relay_vprior_layout(nullptr, b) == QLDPC_EINVAL && qldpc_relay_vprior_layout(rl, nullptr) == QLDPC_EINVAL);
  int w = 0;
  CHECK(qldpc_decode_relay_vprior_launch_info(code, nullptr, &w, &w, &w) == QLDPC_EINVAL);
  CHECK(qldpc_decode_relay_vprior_launch_info(code, rl, &w, &w, nullptr) == QLDPC_EINVAL);

  // the decode entry points: everything refused before a HIP call
  std::vector<uint8_t> syn(2 * 3, 0), e(2 * n, 0);
  std::vector<int32_t> it(2, 0);
  auto dev = [&](const qldpc_code* c, const qldpc_relay* r, const qldpc_prior* v, int cost, int sf, int64_t batch,
                 double eps, const void* s, void* eh, int32_t* i) {
    return qldpc_decode_device_relay_vprior(c, r, v, cost, s, sf, batch, 0.75, eps, eh, 0, i, nullptr, nullptr, nullptr,
                                            nullptr);
  };
  auto host = [&](const qldpc_prior* v, int cost, int64_t batch, double eps, const uint8_t* s) {
    return qldpc_decode_host_relay_vprior(code, rl, v, cost, s, batch, 0.75, eps, e.data(), it.data(), nullptr, nullptr,
                                          nullptr);
  };
  CHECK(dev(code, rl, pr, 0, 2, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);        // format
  CHECK(dev(nullptr, rl, pr, 0, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(dev(code, nullptr, pr, 0, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(dev(other, rl, pr_other, 0, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);  // relay of another code
  CHECK(dev(code, rl, nullptr, 0, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(dev(code, rl, pr_other, 0, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(std::strstr(qldpc_last_error(), "different code") != nullptr);
  CHECK(dev(code, rl, pr, 0, 0, 2, 1e-6, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(std::strstr(qldpc_last_error(), "eps") != nullptr);
  CHECK(dev(code, rl, pr_eps, 1, 0, 0, 1e-6, nullptr, nullptr, nullptr) == QLDPC_OK);              // its own eps; nothing to launch
  for (int cost : {-1, 2, 7}) CHECK(dev(code, rl, pr, cost, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(dev(code, rl, pr, 1, 0, -1, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(dev(code, rl, pr, 1, 0, 2, 1e-9, nullptr, e.data(), it.data()) == QLDPC_EINVAL);
  CHECK(dev(code, rl, pr, 1, 0, 2, 1e-9, syn.data(), nullptr, it.data()) == QLDPC_EINVAL);
  CHECK(dev(code, rl, pr, 1, 0, 2, 1e-9, syn.data(), e.data(), nullptr) == QLDPC_EINVAL);
  CHECK(dev(code, rl, pr, 1, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EHIP);           // no device here
  CHECK(host(nullptr, 0, 2, 1e-9, syn.data()) == QLDPC_EINVAL);
  CHECK(host(pr, 3, 2, 1e-9, syn.data()) == QLDPC_EINVAL);
  CHECK(host(pr, 0, 2, 1e-7, syn.data()) == QLDPC_EINVAL);
  CHECK(host(pr, 0, -1, 1e-9, syn.data()) == QLDPC_EINVAL);
  CHECK(host(pr, 0, 2, 1e-9, nullptr) == QLDPC_EINVAL);
  CHECK(host(pr, 1, 0, 1e-9, nullptr) == QLDPC_OK);
  CHECK(host(pr, 1, 2, 1e-9, syn.data()) == QLDPC_EHIP);
  CHECK(qldpc_set_option("force_hbm", 1) == QLDPC_OK);
  CHECK(dev(code, rl, pr, 1, 0, 2, 1e-9, syn.data(), e.data(), it.data()) == QLDPC_EUNSUP);
  CHECK(host(pr, 1, 2, 1e-9, syn.data()) == QLDPC_EUNSUP);
  CHECK(qldpc_relay_vprior_layout(rl, b) == QLDPC_EUNSUP);
  CHECK(qldpc_decode_relay_vprior_kernel_name(code, rl, name, 64) == QLDPC_EUNSUP);
  CHECK(qldpc_set_option("force_hbm", 0) == QLDPC_OK);

  CHECK(qldpc_relay_destroy(rl) == QLDPC_OK);
  for (qldpc_prior* x : {pr, pr_other, pr_eps}) CHECK(qldpc_prior_destroy(x) == QLDPC_OK);
  CHECK(qldpc_code_destroy(code) == QLDPC_OK && qldpc_code_destroy(other) == QLDPC_OK);
  std::puts("relay_vprior_host_check OK");
  return 0;
}

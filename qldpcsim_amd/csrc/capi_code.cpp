// capi_code.cpp — the Tanner graph of one H (qldpc_code).
//
// Replaces the per-call setup the reference repeats for every shot:
//   BP_decoder's edge lists   np.where(H) + per-check/per-var lists  decoders.py:224-229
//   MS_decoder's dense masks  H == 1 over m x n                       decoders.py:148-169
// Here the graph is built once per H, bit-exactly ordered (CSR edges in
// np.where(H) order; CSC lists in ascending check order), relabeled so that
// variables of equal degree share wavefront passes, and uploaded once.

#include "capi_internal.h"

using namespace capi;

extern "C" int qldpc_code_create(const uint8_t* h_H, int m, int n, qldpc_code** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (m < 0 || n < 0 || (m * (int64_t)n > 0 && !h_H)) return fail(QLDPC_EINVAL, "bad shape %d x %d", m, n);
  auto* c = new qldpc_code();
  c->m = m;
  c->n = n;
  // No visible device (e.g. the CPU build container): the graph is still built
  // so host-side services (OSD) work; decode entry points then fail loudly.
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || hipGetDevice(&c->device) != hipSuccess)
    c->device = -1;
  c->row_ptr.assign(m + 1, 0);
  for (int r = 0; r < m; ++r) {
    for (int j = 0; j < n; ++j)
      if (h_H[(size_t)r * n + j] & 1) c->col_idx.push_back(j);  // (mat % 2) (simulator.py:35)
    c->row_ptr[r + 1] = (int32_t)c->col_idx.size();
  }
  c->E = (int)c->col_idx.size();
  c->lds_ok = m <= 65535 && n <= 65535 && c->E <= 65535;
  std::vector<int> cdeg(n, 0);
  for (int e = 0; e < c->E; ++e) cdeg[c->col_idx[e]]++;
  for (int r = 0; r < m; ++r) c->max_row_deg = std::max(c->max_row_deg, c->row_ptr[r + 1] - c->row_ptr[r]);
  for (int j = 0; j < n; ++j) c->max_col_deg = std::max(c->max_col_deg, cdeg[j]);
  c->uniform_deg = m > 0 ? c->row_ptr[1] : 0;
  for (int r = 0; r < m; ++r)
    if (c->row_ptr[r + 1] - c->row_ptr[r] != c->uniform_deg) c->uniform_deg = 0;
  // Relabel variables by degree (stable) so a wavefront pass over 64
  // consecutive relabeled variables has (nearly) one loop trip count.
  c->vperm.resize(n);
  for (int j = 0; j < n; ++j) c->vperm[j] = j;
  std::stable_sort(c->vperm.begin(), c->vperm.end(), [&](int a, int b) { return cdeg[a] < cdeg[b]; });
  c->vinv.resize(n);
  for (int r = 0; r < n; ++r) c->vinv[c->vperm[r]] = r;
  // CSC over relabeled variables; CSR traversal in ascending row keeps each
  // column's list in ascending check order (np.sum axis=0 order).
  c->csc_ptr.assign(n + 1, 0);
  for (int r = 0; r < n; ++r) c->csc_ptr[r + 1] = c->csc_ptr[r] + cdeg[c->vperm[r]];
  c->csc_edge.assign(c->E, 0);
  c->edge_pos.assign(c->E, 0);
  std::vector<int32_t> fill(c->csc_ptr.begin(), c->csc_ptr.end() - 1);
  for (int r = 0; r < m; ++r)
    for (int e = c->row_ptr[r]; e < c->row_ptr[r + 1]; ++e) {
      const int pos = fill[c->vinv[c->col_idx[e]]]++;
      c->csc_edge[pos] = e;
      c->edge_pos[e] = pos;
    }
  c->mw = (m + 63) / 64;
  for (int j = 0; j < n && !c->zero_col; ++j) c->zero_col = cdeg[j] == 0;
  c->wc.resize(m);
  for (int r = 0; r < m; ++r) {
    uint64_t z = 0x9E3779B97F4A7C15ull * (uint64_t)(r + 1) + 0xD1B54A32D192ED03ull;   // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    c->wc[r] = (uint32_t)((z ^ (z >> 31)) >> 16);
  }
  c->avar.assign(n, 0);
  for (int r = 0; r < m; ++r)
    for (int e = c->row_ptr[r]; e < c->row_ptr[r + 1]; ++e) c->avar[c->vinv[c->col_idx[e]]] ^= c->wc[r];
  for (int v = 0; v < n; ++v) c->filt_all ^= c->avar[v];
  if (n > 0 && c->device >= 0) {
    hipError_t e1 = hipSuccess;
    auto up = [&](auto& d, const auto& h) { e1 = e1 == hipSuccess ? d.upload(h) : e1; };
    if (c->lds_ok) up(c->d_vinv, std::vector<uint16_t>(c->vinv.begin(), c->vinv.end()));
    if (c->lds_ok) up(c->d_vperm, std::vector<uint16_t>(c->vperm.begin(), c->vperm.end()));
    {  // HBM-resident kernel tables
      std::vector<int32_t> rv(c->E), rp(c->E);
      for (int e = 0; e < c->E; ++e) {
        rv[e] = c->vinv[c->col_idx[e]];
        rp[e] = c->edge_pos[e];
      }
      up(c->d_row_var, rv);
      up(c->d_row_pos, rp);
      up(c->d_col_ptr, c->csc_ptr);
      up(c->d_vinv32, c->vinv);
    }
    up(c->d_row_ptr, c->row_ptr);
    up(c->d_col_idx, c->col_idx);
    if (m > 0) {
      std::vector<uint32_t> rtab((size_t)8 * m, 0);
      for (int r = 0; r < m; ++r)
        for (int e = c->row_ptr[r], k = 0; e < c->row_ptr[r + 1] && k < 8; ++e, ++k)
          rtab[(size_t)8 * r + k] = (uint32_t)c->vinv[c->col_idx[e]];
      up(c->d_wc, c->wc);
      up(c->d_rtab, rtab);
      up(c->d_avar, c->avar);
    }
    if (e1 != hipSuccess) {
      delete c;                                      // frees what was uploaded
      return fail(QLDPC_EHIP, "uploading the graph failed: %s", hipGetErrorString(e1));
    }
  }
  *out = c;
  return QLDPC_OK;
}

extern "C" int qldpc_code_destroy(qldpc_code* code) {
  if (!code) return QLDPC_OK;
  if (code->ws_stream) (void)hipStreamDestroy(code->ws_stream);
  delete code;                                       // every table and workspace buffer owns itself
  return QLDPC_OK;
}

extern "C" int qldpc_code_shape(const qldpc_code* code, int* m, int* n, int* n_edges) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (m) *m = code->m;
  if (n) *n = code->n;
  if (n_edges) *n_edges = code->E;
  return QLDPC_OK;
}

// ---------------------------------------------------------------------------
// GF(2) rank of H by XOR-basis insertion of its columns (gf2math.rank,
// gf2math.py:91-135 — rank is basis independent).
// ---------------------------------------------------------------------------
static int gf2_rank_cols(const std::vector<uint64_t>& cols, int n, int mw) {
  if (mw == 0) return 0;
  Gf2Basis B(mw * 64, mw);
  std::vector<uint64_t> x(mw);
  int r = 0;
  for (int j = 0; j < n; ++j) {
    memcpy(x.data(), &cols[(size_t)j * mw], sizeof(uint64_t) * mw);
    r += B.insert(x.data());
  }
  return r;
}

// OSD's column bit-vectors and rank(H), built once on first OSD use
void capi::code_osd_prep(const qldpc_code* c) {
  std::call_once(c->osd_once, [c] {
    c->col_bits.assign((size_t)c->n * std::max(c->mw, 1), 0);
    for (int r = 0; r < c->m; ++r)
      for (int e = c->row_ptr[r]; e < c->row_ptr[r + 1]; ++e)
        c->col_bits[(size_t)c->col_idx[e] * c->mw + (r >> 6)] |= 1ull << (r & 63);
    c->rank = gf2_rank_cols(c->col_bits, c->n, c->mw);
  });
}

// capi_schedule.cpp — layer schedules (qldpc_schedule) and the table images
// the kernels read their graph from. Each image is laid out here, once, and
// each of its offsets is named as the kernel's DecodeArgs names it.

#include "capi_internal.h"

using namespace capi;

extern "C" int qldpc_schedule_create(const qldpc_code* code, int n_layers, const int32_t* h_layer_ptr,
                                     const int32_t* h_layer_rows, qldpc_schedule** out) {
  if (!out) return fail(QLDPC_EINVAL, "out is null");
  *out = nullptr;
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (n_layers < 0 || (n_layers > 0 && !h_layer_ptr)) return fail(QLDPC_EINVAL, "bad layer list");
  const int m = code->m, n = code->n;
  std::vector<std::vector<int>> layers(n_layers);
  std::vector<int> seen(m, -1);
  for (int l = 0; l < n_layers; ++l) {
    const int a = h_layer_ptr[l], b = h_layer_ptr[l + 1];
    if (a < 0 || b < a) return fail(QLDPC_EINVAL, "layer_ptr is not non-decreasing at layer %d", l);
    for (int q = a; q < b; ++q) {
      const int r = h_layer_rows[q];
      if (r < 0 || r >= m)
        return fail(QLDPC_ERANGE, "index %d is out of bounds for axis 0 with size %d", r, m);
      if (seen[r] != l) {  // duplicates inside a layer: same Jacobi inputs, same outputs
        seen[r] = l;
        layers[l].push_back(r);
      }
    }
  }
  auto* s = new qldpc_schedule();
  TableImage& gen = s->generic;
  s->code = code;
  s->n_layers = n_layers;
  // One layer holding every row exactly once == flooding (decoders.py:122).
  s->layered = !(n_layers == 1 && (int)layers[0].size() == m);

  // HBM-resident kernel tables (32-bit, every schedule): layer rows, each
  // layer's adjacent variables (ascending), and for the no-init first
  // iteration the first layer that reaches each variable / CSC position
  {
    s->h_lay_ptr.assign(n_layers + 1, 0);
    s->h_adj_ptr.assign(n_layers + 1, 0);
    s->h_fl_var.assign(std::max(n, 1), n_layers);
    s->h_fl_pos.assign(std::max(code->E, 1), n_layers);
    std::vector<int> row_layer(m, -1), mark(n, -1);
    bool part = true;
    for (int l = 0; l < n_layers; ++l) {
      std::vector<int> adj;
      for (int r : layers[l]) {
        s->h_lay_rows.push_back(r);
        if (row_layer[r] >= 0) part = false;          // a row in two layers
        row_layer[r] = l;
        for (int e = code->row_ptr[r]; e < code->row_ptr[r + 1]; ++e) {
          const int v = code->vinv[code->col_idx[e]];
          if (mark[v] != l) {
            mark[v] = l;
            adj.push_back(v);
          }
        }
      }
      std::sort(adj.begin(), adj.end());
      for (int v : adj) {
        s->h_adj_vars.push_back(v);
        s->h_fl_var[v] = std::min(s->h_fl_var[v], l);
      }
      s->h_lay_ptr[l + 1] = (int32_t)s->h_lay_rows.size();
      s->h_adj_ptr[l + 1] = (int32_t)s->h_adj_vars.size();
    }
    for (int r = 0; r < m; ++r) {
      if (row_layer[r] < 0) part = false;             // a row no layer updates
      for (int e = code->row_ptr[r]; e < code->row_ptr[r + 1]; ++e) s->h_fl_pos[code->edge_pos[e]] = row_layer[r];
    }
    s->hbm_lazy = part;
  }
  s->lds_ok = code->lds_ok && s->h_lay_rows.size() <= 65535 && s->h_adj_vars.size() <= 65535;

  if (s->lds_ok) {
  std::vector<uint32_t> cn_tab;
  if (fast_table_ok(code)) {
    // uniform row degree: rows padded to 8 entries, pre-scaled LDS byte offsets
    // (4 * csc position) << 16 | (8 * relabeled variable)
    cn_tab.assign((size_t)8 * m, 0);
    for (int r = 0; r < m; ++r)
      for (int e = code->row_ptr[r], k = 0; e < code->row_ptr[r + 1]; ++e, ++k)
        cn_tab[(size_t)8 * r + k] = ((uint32_t)(4 * code->edge_pos[e]) << 16) |
                                    (uint32_t)(8 * code->vinv[code->col_idx[e]]);
  } else {
    cn_tab.resize(code->E);
    for (int e = 0; e < code->E; ++e)
      cn_tab[e] = ((uint32_t)code->vinv[code->col_idx[e]] << 16) | (uint32_t)code->edge_pos[e];
  }
  std::vector<uint16_t> row_ptr(code->row_ptr.begin(), code->row_ptr.end());
  std::vector<uint32_t> vn_ptr(n);  // csc start | degree << 16
  for (int j = 0; j < n; ++j)
    vn_ptr[j] = (uint32_t)code->csc_ptr[j] | ((uint32_t)(code->csc_ptr[j + 1] - code->csc_ptr[j]) << 16);
  gen.off.cn_tab = gen.put(cn_tab);
  gen.off.row_ptr = gen.put(row_ptr);
  gen.off.vn_ptr = gen.put(vn_ptr);
  std::vector<uint8_t> chunk_dmax((n + 63) / 64, 0);   // VN passes unroll to this (<= 255)
  for (int j = 0; j < n; ++j)
    chunk_dmax[j >> 6] = (uint8_t)std::min(255, std::max<int>(chunk_dmax[j >> 6], code->csc_ptr[j + 1] - code->csc_ptr[j]));
  gen.off.chunk_dmax = gen.put(chunk_dmax);
  if (s->layered) {
    std::vector<uint16_t> vn_chk(code->E), lay_ptr(n_layers + 1, 0), lay_rows, adj_ptr(n_layers + 1, 0), adj_vars;
    for (int p = 0; p < code->E; ++p) {
      // CSR edge -> its check (row)
      const int e = code->csc_edge[p];
      const int r = (int)(std::upper_bound(code->row_ptr.begin(), code->row_ptr.end(), e) - code->row_ptr.begin()) - 1;
      vn_chk[p] = (uint16_t)r;
    }
    std::vector<int> mark(n, -1);
    for (int l = 0; l < n_layers; ++l) {
      std::vector<int> adj;
      for (int r : layers[l]) {
        lay_rows.push_back((uint16_t)r);
        for (int e = code->row_ptr[r]; e < code->row_ptr[r + 1]; ++e) {
          const int v = code->vinv[code->col_idx[e]];
          if (mark[v] != l) {
            mark[v] = l;
            adj.push_back(v);
          }
        }
      }
      std::sort(adj.begin(), adj.end());
      for (int v : adj) adj_vars.push_back((uint16_t)v);
      lay_ptr[l + 1] = (uint16_t)lay_rows.size();
      adj_ptr[l + 1] = (uint16_t)adj_vars.size();
    }
    gen.off.vn_chk = gen.put(vn_chk);
    gen.off.lay_ptr = gen.put(lay_ptr);
    gen.off.lay_rows = gen.put(lay_rows);
    gen.off.adj_ptr = gen.put(adj_ptr);
    gen.off.adj_vars = gen.put(adj_vars);
    if (fast_table_ok(code) && n <= 2048 && code->max_col_deg <= 31) {
      std::vector<uint32_t> ltab((size_t)8 * lay_rows.size(), 0), adj_info(adj_vars.size());
      for (size_t q = 0; q < lay_rows.size(); ++q) {
        const int r = lay_rows[q];
        for (int e = code->row_ptr[r], k = 0; e < code->row_ptr[r + 1]; ++e, ++k)
          ltab[8 * q + k] = ((uint32_t)(4 * code->edge_pos[e]) << 16) | (uint32_t)(4 * code->vinv[code->col_idx[e]]);
      }
      std::vector<uint16_t> adj_dmax(std::max(n_layers, 1), 0);
      for (int l = 0; l < n_layers; ++l) {
        int dmin = 32;
        bool mid = false;                                   // a degree strictly between 3 and dmax
        for (int q = adj_ptr[l]; q < adj_ptr[l + 1]; ++q) {
          const int v = adj_vars[q], d = code->csc_ptr[v + 1] - code->csc_ptr[v];
          adj_info[q] = ((uint32_t)v << 21) | ((uint32_t)d << 16) | (uint32_t)code->csc_ptr[v];
          adj_dmax[l] = (uint16_t)std::max<int>(adj_dmax[l], d);   // d <= 31 here
          dmin = std::min(dmin, d);
        }
        for (int q = adj_ptr[l]; q < adj_ptr[l + 1]; ++q) {
          const int v = adj_vars[q], d = code->csc_ptr[v + 1] - code->csc_ptr[v];
          mid |= d > 3 && d < adj_dmax[l];
        }
        // bit 7: every adjacent variable has degree >= 3 (vn_layer's LO = 3);
        // bit 8: and every degree is 3 or the layer's maximum (vn_layer's TWO)
        if (dmin >= 3 && adj_ptr[l + 1] > adj_ptr[l]) {
          adj_dmax[l] = (uint16_t)(adj_dmax[l] | 0x80);
          if (!mid) adj_dmax[l] = (uint16_t)(adj_dmax[l] | 0x100);
        }
      }
      // bits 5-6: log2 of the layer's lanes per check (ms_layered_kernel<DC, 0>):
      // one lane per check for long layers, a lane group when the layer leaves
      // most of the wave idle (rows <= 8: 8 lanes, <= 16: 4)
      // (two lanes per check on 17-64-row layers measured 5-12 % slower, round 2)
      s->layer_g = -2;
      for (int l = 0; l < n_layers; ++l) {
        const int rows = lay_ptr[l + 1] - lay_ptr[l];
        const int gl = rows <= 8 ? 3 : (rows <= 16 ? 2 : 0);
        adj_dmax[l] = (uint16_t)(adj_dmax[l] | (gl << 5));
        s->layer_g = (s->layer_g == -2 || s->layer_g == (1 << gl)) ? (1 << gl) : 0;
      }
      {
        std::vector<uint32_t> btab((size_t)8 * lay_rows.size(), 0);   // cn_tab words (BP format), layer order
        for (size_t q = 0; q < lay_rows.size(); ++q)
          for (int k = 0; k < 8; ++k) btab[8 * q + k] = cn_tab[(size_t)8 * lay_rows[q] + k];
        // bp_team_lg_kernel: the layer pointers are the LDS image, the
        // tables behind them stay global
        TableImage& lg = s->layered_bp;
        lg.off = gen.off;
        lg.off.lay_ptr = lg.put(lay_ptr);
        lg.off.adj_ptr = lg.put(adj_ptr);
        lg.lds_bytes = lg.seal();
        lg.off.cn_tab = lg.put(btab);        // rows in layer order
        lg.off.lay_rows = lg.put(lay_rows);
        lg.off.row_ptr = lg.put(adj_info);   // carries the adjacency words, not row pointers
        lg.seal();
      }
      // ms_layered_kernel: the whole image in LDS (the <DC, 1> instance built
      // with QLDPC_MSL_GT stages a window of it, plan_static)
      TableImage& lm = s->layered_ms;
      lm.off = gen.off;
      lm.off.cn_tab = lm.put(ltab);          // rows in layer order, 4-byte variable offsets
      lm.off.lay_rows = lm.put(lay_rows);
      lm.off.lay_ptr = lm.put(lay_ptr);
      lm.off.adj_ptr = lm.put(adj_ptr);
      lm.off.adj_vars = 0;                   // not read: adjacency comes from off_row_ptr
      lm.off.row_ptr = lm.put(adj_info);     // carries the adjacency words, not row pointers
      lm.off.chunk_dmax = lm.put(adj_dmax);  // carries the per-layer degree / lane-group words
      lm.off.vn_chk = lm.put(code->avar);    // carries the filter word per relabeled variable
      lm.lds_bytes = lm.seal();
    }
  }
  if (!s->layered && fast_table_ok(code) && m <= 8 * 64) {
    // ms_flood_kernel's global image: FloodRuns header (runs of equal column
    // degree over the relabeled variables), then per check c = lane + 64 i the
    // words [8c, 8c+8): (4 * csc position) << 16 | (8 * relabeled variable).
    // Pad checks write the pad floats E..E+7 behind c2v and read post[0].
    std::vector<int32_t> hdr(1 + 4 * QLDPC_MAX_RUNS, 0);
    int nr = 0;
    bool ok = true;
    for (int j = 0; j < n;) {
      const int d = code->csc_ptr[j + 1] - code->csc_ptr[j];
      int e = j;
      while (e < n && code->csc_ptr[e + 1] - code->csc_ptr[e] == d) ++e;
      if (nr == QLDPC_MAX_RUNS) { ok = false; break; }
      hdr[1 + nr] = j;                                   // start
      hdr[1 + QLDPC_MAX_RUNS + nr] = e - j;              // count
      hdr[1 + 2 * QLDPC_MAX_RUNS + nr] = d;              // degree
      hdr[1 + 3 * QLDPC_MAX_RUNS + nr] = code->csc_ptr[j];  // csc start
      ++nr;
      j = e;
    }
    hdr[0] = nr;
    if (ok) {
      std::vector<uint32_t> ftab((size_t)8 * 64 * 8, 0);
      for (int r = 0; r < 8 * 64; ++r)
        for (int k = 0; k < 8; ++k) {
          const int e = r < m ? code->row_ptr[r] + k : -1;
          if (r < m && e < code->row_ptr[r + 1])
            ftab[(size_t)8 * r + k] = ((uint32_t)(4 * code->edge_pos[e]) << 16) |
                                      (uint32_t)(8 * code->vinv[code->col_idx[e]]);
          else if (r >= m)
            ftab[(size_t)8 * r + k] = (uint32_t)(4 * (code->E + k)) << 16;
        }
      TableImage& fl = s->flood_ms;
      fl.off = gen.off;
      (void)fl.put(hdr);
      fl.off.cn_tab = fl.put(ftab);
      fl.seal();
      fl.lds_bytes = QLDPC_FLOOD_HDR;   // the kernel keeps the runs header in LDS, loaded by itself
    }
  }
  }  // s->lds_ok
  gen.lds_bytes = gen.seal();
  if (code->device < 0) {  // no device: keep the host images only
    *out = s;
    return QLDPC_OK;
  }
  hipError_t e1 = s->queue.buf.alloc(QueueRing::kSlots);
  for (TableImage* t : {&s->generic, &s->flood_ms, &s->layered_bp, &s->layered_ms})
    if (e1 == hipSuccess && !t->empty()) e1 = t->dev.upload(t->bytes);
  auto up = [&](DevBuf<int32_t>& d, const std::vector<int32_t>& h) { e1 = e1 == hipSuccess ? d.upload(h) : e1; };
  up(s->d_h_lay_ptr, s->h_lay_ptr), up(s->d_h_lay_rows, s->h_lay_rows);
  up(s->d_h_adj_ptr, s->h_adj_ptr), up(s->d_h_adj_vars, s->h_adj_vars);
  up(s->d_h_fl_var, s->h_fl_var), up(s->d_h_fl_pos, s->h_fl_pos);
  if (e1 != hipSuccess) {
    qldpc_schedule_destroy(s);                       // frees what was uploaded
    return fail(QLDPC_EHIP, "uploading the schedule failed: %s", hipGetErrorString(e1));
  }
  *out = s;
  return QLDPC_OK;
}

extern "C" int qldpc_schedule_destroy(qldpc_schedule* s) {
  if (!s) return QLDPC_OK;
  (void)hipFree(s->hbm_ws);
  if (s->hbm_ev) (void)hipEventDestroy(s->hbm_ev);
  delete s;                                          // every table owns its device buffer
  return QLDPC_OK;
}

extern "C" int qldpc_schedule_release_workspace(qldpc_schedule* s) {
  if (!s) return fail(QLDPC_EINVAL, "schedule is null");
  std::lock_guard<std::mutex> lk(s->mu);
  if (s->hbm_ws) {
    if (s->hbm_ev) HIP_TRY(hipEventSynchronize(s->hbm_ev));   // the last launch that used it is done
    HIP_TRY(hipFree(s->hbm_ws));
    s->hbm_ws = nullptr;
    s->hbm_ws_bytes = 0;
  }
  return QLDPC_OK;
}

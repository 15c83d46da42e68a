// capi_osd_host.cpp — host OSD (decoders.py:299-370): bit-packed GF(2)
// elimination, one shot or a threaded batch.

#include <thread>

#include "capi_internal.h"

using namespace capi;

// XOR-basis insertion (also gf2math.rank for capi_code.cpp, gf2math.py:91-135)
bool Gf2Basis::insert(uint64_t* x) {
  for (int w = 0; w < mw; ++w) {
    while (x[w]) {
      const int b = w * 64 + __builtin_ctzll(x[w]);
      if (!has[b]) {
        memcpy(&vec[(size_t)b * mw], x, sizeof(uint64_t) * mw);
        has[b] = 1;
        return true;
      }
      const uint64_t* v = &vec[(size_t)b * mw];
      for (int k = w; k < mw; ++k) x[k] ^= v[k];
    }
  }
  return false;
}

// Order of iteration of CPython's `set(range(n)) - set(J)` (the reference's
// infoSet, decoders.py:344): returns its first element. Emulates
// setobject.c (set_difference -> set_add_entry / set_table_resize /
// set_insert_clean; LINEAR_PROBES 9, PERTURB_SHIFT 5) for small-int keys
// (hash(i) == i). Verified against the interpreter in tests.
static int cpython_setdiff_first(int n, const std::vector<char>& inJ, int nJ) {
  if (nJ == n) return -1;
  if ((n >> 2) > nJ) {
    // set_copy_and_difference: a copy of set(range(n)) (ascending slots)
    for (int i = 0; i < n; ++i)
      if (!inJ[i]) return i;
    return -1;
  }
  size_t mask = 7;
  std::vector<int64_t> table(8, -1);
  size_t fill = 0, used = 0;
  auto insert_clean = [](std::vector<int64_t>& t, size_t msk, int64_t key) {
    size_t perturb = (size_t)key, i = (size_t)key & msk;
    while (true) {
      if (t[i] < 0) { t[i] = key; return; }
      if (i + 9 <= msk) {
        for (int j = 0; j < 9; ++j) {
          ++i;
          if (t[i] < 0) { t[i] = key; return; }
        }
      }
      perturb >>= 5;
      i = (i * 5 + 1 + perturb) & msk;
    }
  };
  for (int key = 0; key < n; ++key) {
    if (inJ[key]) continue;
    // set_add_entry (new key, no dummies)
    size_t perturb = (size_t)key, i = (size_t)key & mask;
    while (true) {
      size_t probes = (i + 9 <= mask) ? 9 : 0;
      size_t k = i;
      bool placed = false;
      while (true) {
        if (table[k] < 0) {
          table[k] = key;
          placed = true;
          break;
        }
        if (probes-- == 0) break;
        ++k;
      }
      if (placed) break;
      perturb >>= 5;
      i = (i * 5 + 1 + perturb) & mask;
    }
    ++fill;
    ++used;
    if (fill * 5 >= mask * 3) {
      const size_t minused = used > 50000 ? used * 2 : used * 4;
      size_t newsize = 8;
      while (newsize <= minused) newsize <<= 1;
      std::vector<int64_t> nt(newsize, -1);
      for (size_t s2 = 0; s2 <= mask; ++s2)
        if (table[s2] >= 0) insert_clean(nt, newsize - 1, table[s2]);
      table.swap(nt);
      mask = newsize - 1;
    }
  }
  for (size_t s2 = 0; s2 <= mask; ++s2)
    if (table[s2] >= 0) return (int)table[s2];
  return -1;
}

extern "C" int qldpc_cpython_setdiff_first(int n, const int32_t* J, int nJ) {
  std::vector<char> inJ(std::max(n, 1), 0);
  int cnt = 0;
  for (int k = 0; k < nJ; ++k)
    if (J[k] >= 0 && J[k] < n && !inJ[J[k]]) inJ[J[k]] = 1, ++cnt;
  return cpython_setdiff_first(n, inJ, cnt);
}

// ---------------------------------------------------------------------------
// OSD (decoders.py:299-370), given the caller's reliability order `perm`
// (np.argsort of decoders.py:320-325 — NumPy's own exp/argsort decide ties).
// ---------------------------------------------------------------------------
static int osd_one(const qldpc_code* c, const uint8_t* syn, const int32_t* perm, int order, uint8_t* ehat,
                   int32_t* J_out, int32_t* J_size, int first_info_index) {
  const int m = c->m, n = c->n, mw = c->mw;
  if (n == 0) return QLDPC_OK;
  code_osd_prep(c);
  // (1) least reliable basis J (decoders.py:329-342): index 0 unconditionally,
  //     then every column (in perm order) that raises the rank, until rank(H).
  Gf2Basis B(std::max(mw * 64, 1), mw);
  std::vector<uint64_t> x(std::max(mw, 1));
  std::vector<int> J;
  std::vector<char> inJ(n, 0);
  auto col = [&](int i) { return &c->col_bits[(size_t)perm[i] * mw]; };
  if (mw) memcpy(x.data(), col(0), sizeof(uint64_t) * mw);
  int rank = mw ? (int)B.insert(x.data()) : 0;
  J.push_back(0);
  inJ[0] = 1;
  if (rank >= c->rank)
    return fail(QLDPC_ERANGE, "index %d is out of bounds for axis 1 with size %d", n, n);  // reference IndexError
  int next = 1;
  while (true) {
    if (next >= n) return fail(QLDPC_ERANGE, "index %d is out of bounds for axis 1 with size %d", n, n);
    memcpy(x.data(), col(next), sizeof(uint64_t) * mw);
    if (B.insert(x.data())) {
      J.push_back(next);
      inJ[next] = 1;
      if (++rank >= c->rank) break;
    }
    ++next;
  }
  const int nJ = (int)J.size();
  if (J_out)
    for (int k = 0; k < nJ; ++k) J_out[k] = J[k];
  if (J_size) *J_size = nJ;
  // (2) e_hat_perm = e_hat[perm]; order-k loop with aliasing:
  //     the cumulative flip is I[0] for order 1 and nothing otherwise.
  std::vector<uint8_t> ep(n);
  for (int i = 0; i < n; ++i) ep[i] = ehat[perm[i]] & 1;
  if (order == 1 && nJ < n) {
    int i0 = first_info_index >= 0 ? first_info_index : cpython_setdiff_first(n, inJ, nJ);
    if (i0 < 0 || i0 >= n || inJ[i0]) return fail(QLDPC_EINVAL, "bad first_info_index %d", i0);
    ep[i0] ^= 1;
  }
  // (3) sJ = (syndrome + Hp[:, I] @ e_I) % 2
  std::vector<uint64_t> sJ(std::max(mw, 1), 0);
  for (int r = 0; r < m; ++r)
    if (syn[r] & 1) sJ[r >> 6] |= 1ull << (r & 63);
  for (int i = 0; i < n; ++i)
    if (!inJ[i] && ep[i]) {
      const uint64_t* cb = col(i);
      for (int w = 0; w < mw; ++w) sJ[w] ^= cb[w];
    }
  // (4) (T @ sJ) % 2 with T from REF(Hp[:, J], reduced=True) (gf2math.py:139-187):
  //     the same row operations applied to sJ as an augmented column.
  const int rw = (nJ + 63) / 64;
  std::vector<uint64_t> rows((size_t)m * rw, 0);
  for (int k = 0; k < nJ; ++k) {
    const uint64_t* cb = col(J[k]);
    for (int w = 0; w < mw; ++w) {
      uint64_t bits = cb[w];
      while (bits) {
        const int r = w * 64 + __builtin_ctzll(bits);
        bits &= bits - 1;
        rows[(size_t)r * rw + (k >> 6)] |= 1ull << (k & 63);
      }
    }
  }
  std::vector<uint8_t> s(m);
  for (int r = 0; r < m; ++r) s[r] = (sJ[r >> 6] >> (r & 63)) & 1;
  auto bit = [&](int r, int k) { return (rows[(size_t)r * rw + (k >> 6)] >> (k & 63)) & 1; };
  auto xor_row = [&](int dst, int src) {
    for (int w = 0; w < rw; ++w) rows[(size_t)dst * rw + w] ^= rows[(size_t)src * rw + w];
    s[dst] ^= s[src];
  };
  int xr = 0;
  for (int k = 0; k < nJ && m > 0; ++k) {
    int r = xr;
    while (r < m && !bit(r, k)) ++r;
    if (r == m) continue;
    if (r != xr) {
      for (int w = 0; w < rw; ++w) std::swap(rows[(size_t)xr * rw + w], rows[(size_t)r * rw + w]);
      std::swap(s[xr], s[r]);
    }
    for (int t = r + 1; t < m; ++t)
      if (bit(t, k)) xor_row(t, xr);
    for (int t = 0; t < xr; ++t)
      if (bit(t, k)) xor_row(t, xr);
    if (++xr >= m) break;
  }
  for (int k = 0; k < nJ; ++k) ep[J[k]] = k < m ? s[k] : 0;
  for (int i = 0; i < n; ++i) ehat[perm[i]] = ep[i];  // e_hat[perm] = ... (:368)
  return QLDPC_OK;
}

static int osd_check_perm(const qldpc_code* code, const int32_t* h_perm) {
  std::vector<char> seen(code->n, 0);
  for (int i = 0; i < code->n; ++i) {
    if (h_perm[i] < 0 || h_perm[i] >= code->n || seen[h_perm[i]])
      return fail(QLDPC_EINVAL, "perm is not a permutation");
    seen[h_perm[i]] = 1;
  }
  return QLDPC_OK;
}

extern "C" int qldpc_osd_decode(const qldpc_code* code, const uint8_t* h_syn, const int32_t* h_perm, int order,
                                uint8_t* h_ehat, int32_t* h_J, int32_t* h_J_size, int first_info_index) {
  if (!code || !h_perm || !h_ehat || (!h_syn && code->m)) return fail(QLDPC_EINVAL, "null argument");
  if (const int rc = osd_check_perm(code, h_perm)) return rc;
  return osd_one(code, h_syn, h_perm, order, h_ehat, h_J, h_J_size, first_info_index);
}

// ---------------------------------------------------------------------------
// OSD-CS (combination sweep), the device epilogue's host
// twin. One elimination of [H[:, perm] | s] with REF's pivot rule gives J (the
// pivot columns, the greedy set of decoders.py:329-342), T (the rest,
// ascending) and, in pivot row k, column k of B^-1 H_T and of B^-1 s. The base
// estimate e0 is the order-0 result; candidates, in order: e0, every single
// flip of T[k], every pair T[a], T[b] with a < b < min(lambda, |T|); the first
// of strictly smallest cost wins. The cost is the Hamming weight, or with a
// weight row Wo (one int64 per original column, qldpc_prior::Wo; DESIGN.md
// §3.19) the exact sum of Wo over the estimate's support. Three cases have no
// B^-1 and return the order-0 result of osd_one: an all-zero column perm[0]
// (J's unconditional first entry is no pivot), a syndrome outside H's column
// space, and rank(H) <= 1 (the reference's IndexError case, QLDPC_ERANGE).
// ---------------------------------------------------------------------------
static int osd_cs_one(const qldpc_code* c, const uint8_t* syn, const int32_t* perm, int lambda, uint8_t* ehat,
                      const int64_t* Wo = nullptr) {
  const int m = c->m, n = c->n, mw = c->mw;
  if (n == 0) return QLDPC_OK;
  code_osd_prep(c);
  const int nw = (n + 1 + 63) / 64;                   // row words, syndrome bit at column n
  std::vector<uint64_t> R((size_t)std::max(m, 1) * nw, 0);
  bool col0 = false;
  for (int i = 0; i < n; ++i) {
    const uint64_t* cb = &c->col_bits[(size_t)perm[i] * mw];
    for (int w = 0; w < mw; ++w) {
      uint64_t bits = cb[w];
      if (i == 0 && bits) col0 = true;
      while (bits) {
        const int r = w * 64 + __builtin_ctzll(bits);
        bits &= bits - 1;
        R[(size_t)r * nw + (i >> 6)] |= 1ull << (i & 63);
      }
    }
  }
  for (int r = 0; r < m; ++r)
    if (syn[r] & 1) R[(size_t)r * nw + (n >> 6)] |= 1ull << (n & 63);
  auto order0 = [&]() { return osd_one(c, syn, perm, 0, ehat, nullptr, nullptr, -1); };
  if (!col0 || c->rank <= 1) return order0();
  std::vector<int> J;
  std::vector<char> inJ(n, 0);
  int xr = 0;
  for (int i = 0; i < n && xr < c->rank; ++i) {
    int r = xr;
    while (r < m && !((R[(size_t)r * nw + (i >> 6)] >> (i & 63)) & 1)) ++r;
    if (r == m) continue;
    for (int w = 0; w < nw; ++w) std::swap(R[(size_t)xr * nw + w], R[(size_t)r * nw + w]);
    const uint64_t* pr = &R[(size_t)xr * nw];
    for (int t = 0; t < m; ++t)
      if (t != xr && ((R[(size_t)t * nw + (i >> 6)] >> (i & 63)) & 1))
        for (int w = i >> 6; w < nw; ++w) R[(size_t)t * nw + w] ^= pr[w];
    J.push_back(i);
    inJ[i] = 1;
    ++xr;
  }
  const int nJ = xr;
  for (int r = nJ; r < m; ++r)
    if ((R[(size_t)r * nw + (n >> 6)] >> (n & 63)) & 1) return order0();   // s outside H's column space
  // e_T as a row mask; e0_J[k] = (B^-1 s)[k] + (B^-1 H_T e_T)[k]
  std::vector<uint64_t> eT(nw, 0);
  std::vector<int> T;
  for (int i = 0; i < n; ++i)
    if (!inJ[i]) {
      T.push_back(i);
      if (ehat[perm[i]] & 1) eT[i >> 6] |= 1ull << (i & 63);
    }
  const int kw = (nJ + 63) / 64, nT = (int)T.size();
  std::vector<uint64_t> eJ(kw, 0);
  for (int k = 0; k < nJ; ++k) {
    const uint64_t* row = &R[(size_t)k * nw];
    uint64_t acc = (row[n >> 6] >> (n & 63)) & 1;
    for (int w = 0; w < nw; ++w) acc ^= (uint64_t)(__builtin_popcountll(row[w] & eT[w]) & 1);
    if (acc) eJ[k >> 6] |= 1ull << (k & 63);
  }
  // column T[k] of B^-1 H_T over the pivot rows, bit-packed
  auto column = [&](int i, uint64_t* out) {
    for (int w = 0; w < kw; ++w) out[w] = 0;
    for (int k = 0; k < nJ; ++k)
      if ((R[(size_t)k * nw + (i >> 6)] >> (i & 63)) & 1) out[k >> 6] |= 1ull << (k & 63);
  };
  // signed weight of pivot row k: what flipping e0_J[k] adds to the cost
  std::vector<int64_t> sw(Wo ? nJ : 0);
  for (int k = 0; k < (int)sw.size(); ++k) sw[k] = ((eJ[k >> 6] >> (k & 63)) & 1) ? -Wo[perm[J[k]]] : Wo[perm[J[k]]];
  // cost change of XOR-ing `col` into e_J: +1 (+W) per 0 it sets, -1 (-W) per 1 it clears
  auto delta = [&](const uint64_t* col) {
    int64_t d = 0;
    for (int w = 0; w < kw; ++w) {
      if (!Wo) {
        d += __builtin_popcountll(col[w]) - 2 * __builtin_popcountll(col[w] & eJ[w]);
        continue;
      }
      for (uint64_t bits = col[w]; bits; bits &= bits - 1) d += sw[64 * w + __builtin_ctzll(bits)];
    }
    return d;
  };
  auto flip_cost = [&](int i) -> int64_t {
    const int64_t wt = Wo ? Wo[perm[i]] : 1;
    return ((eT[i >> 6] >> (i & 63)) & 1) ? -wt : wt;
  };
  const int L = std::min(lambda, nT);
  std::vector<uint64_t> first((size_t)std::max(L, 1) * std::max(kw, 1)), col(std::max(kw, 1));
  int64_t best = 0;                                   // strictly below the base's 0, first such
  int ba = -1, bb = -1;
  for (int k = 0; k < nT; ++k) {
    uint64_t* dst = k < L ? &first[(size_t)k * kw] : col.data();
    column(T[k], dst);
    const int64_t d = flip_cost(T[k]) + delta(dst);
    if (d < best) best = d, ba = k, bb = -1;
  }
  for (int a = 0; a < L; ++a)
    for (int b = a + 1; b < L; ++b) {
      for (int w = 0; w < kw; ++w) col[w] = first[(size_t)a * kw + w] ^ first[(size_t)b * kw + w];
      const int64_t d = flip_cost(T[a]) + flip_cost(T[b]) + delta(col.data());
      if (d < best) best = d, ba = a, bb = b;
    }
  for (int f : {ba, bb})
    if (f >= 0) {
      column(T[f], col.data());
      for (int w = 0; w < kw; ++w) eJ[w] ^= col[w];
      ehat[perm[T[f]]] ^= 1;
    }
  for (int k = 0; k < nJ; ++k) ehat[perm[J[k]]] = (uint8_t)((eJ[k >> 6] >> (k & 63)) & 1);
  return QLDPC_OK;
}

int qldpc_host_thread_budget();                         // np_order.cpp

// lambda < 0: the reference's OSD of `order`; else OSD-CS with that lambda, and with the weight row Wo if given
static int osd_batch(const qldpc_code* code, int64_t count, const uint8_t* h_syn, const int32_t* h_perm, int order,
                     int lambda, uint8_t* h_ehat, int nthreads, const int64_t* Wo = nullptr) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (count <= 0) return QLDPC_OK;
  if (nthreads <= 0) nthreads = qldpc_host_thread_budget();
  nthreads = (int)std::min<int64_t>(nthreads, count);
  const int m = code->m, n = code->n;
  std::atomic<int64_t> next{0};
  std::atomic<int> rc{QLDPC_OK};
  std::string err;
  std::mutex emu;
  auto worker = [&]() {
    while (true) {
      const int64_t b = next.fetch_add(1);
      if (b >= count || rc.load() != QLDPC_OK) return;
      int r;
      if (lambda < 0) {
        r = qldpc_osd_decode(code, h_syn + b * m, h_perm + b * n, order, h_ehat + b * n, nullptr, nullptr, -1);
      } else {
        r = osd_check_perm(code, h_perm + b * n);
        if (r == QLDPC_OK) r = osd_cs_one(code, h_syn + b * m, h_perm + b * n, lambda, h_ehat + b * n, Wo);
      }
      if (r != QLDPC_OK) {
        std::lock_guard<std::mutex> lk(emu);
        if (rc.load() == QLDPC_OK) err = g_err;
        rc = r;
      }
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < nthreads; ++t) th.emplace_back(worker);
  worker();
  for (auto& t : th) t.join();
  if (rc.load() != QLDPC_OK) g_err = err;
  return rc.load();
}

extern "C" int qldpc_osd_decode_batch(const qldpc_code* code, int64_t count, const uint8_t* h_syn,
                                      const int32_t* h_perm, int order, uint8_t* h_ehat, int nthreads) {
  return osd_batch(code, count, h_syn, h_perm, order, -1, h_ehat, nthreads);
}

// the prior handle of an OSD-CS call with the weighted cost: built for this code
int capi::osd_cs_prior_checked(const qldpc_code* code, const qldpc_prior* prior) {
  if (!code) return fail(QLDPC_EINVAL, "code is null");
  if (!prior) return fail(QLDPC_EINVAL, "OSD-CS with the prior cost needs a prior handle (null)");
  if (prior->code != code || prior->n != code->n || (int)prior->Wo.size() != code->n)
    return fail(QLDPC_EINVAL, "the prior handle was built for another code");
  return QLDPC_OK;
}

static int osd_batch_cs(const qldpc_code* code, int64_t count, const uint8_t* h_syn, const int32_t* h_perm,
                        int lambda, const int64_t* Wo, uint8_t* h_ehat, int nthreads) {
  if (lambda < 0 || lambda > QLDPC_OSD_CS_MAX_LAMBDA)
    return fail(QLDPC_EINVAL, "OSD-CS lambda must lie in 0..%d (got %d)", QLDPC_OSD_CS_MAX_LAMBDA, lambda);
  if (count > 0 && (!h_perm || !h_ehat || (!h_syn && code && code->m))) return fail(QLDPC_EINVAL, "null argument");
  return osd_batch(code, count, h_syn, h_perm, 0, lambda, h_ehat, nthreads, Wo);
}

extern "C" int qldpc_osd_decode_batch_cs(const qldpc_code* code, int64_t count, const uint8_t* h_syn,
                                         const int32_t* h_perm, int lambda, uint8_t* h_ehat, int nthreads) {
  return osd_batch_cs(code, count, h_syn, h_perm, lambda, nullptr, h_ehat, nthreads);
}

extern "C" int qldpc_osd_decode_batch_cs_prior(const qldpc_code* code, int64_t count, const uint8_t* h_syn,
                                               const int32_t* h_perm, int lambda, const qldpc_prior* prior,
                                               uint8_t* h_ehat, int nthreads) {
  if (const int rc = osd_cs_prior_checked(code, prior)) return rc;
  return osd_batch_cs(code, count, h_syn, h_perm, lambda, prior->Wo.data(), h_ehat, nthreads);
}

/*
 * qldpc_decoder.h — C ABI of the MI355X (gfx950) batched BP / Min-Sum decoder.
 *
 * This is the drop-in boundary for qLDPCsim's Monte-Carlo hot path
 * (albertogp71/qLDPCsim @ 2025-12-26). The reference has no FFI: its boundary
 * is the Python call dispatched per shot by simulate_p
 * (qLDPCsim/simulator.py:270-284) into
 *     MS_decoder(H, syndrome, p, max_iter=99, layers=None, beta=0.75,
 *                OSDorder=-1, eps=1e-9) -> (e_hat int8[n], n_iter)   decoders.py:110-182
 *     BP_decoder(H, syndrome, p, max_iter=99, layers=None, OSDorder=-1,
 *                eps=1e-9) -> (e_hat int64[n], n_iter)               decoders.py:189-290
 *     OSDdec(H, e_hat, syndrome, posteriorLLRs, order=0) -> e_hat      decoders.py:299-370
 * Each entry point below names the reference interface it replaces. The
 * Python package `qldpcsim_amd` binds these with ctypes and
 * re-exposes the reference signatures unchanged.
 *
 * Conventions
 *  - Plain C types only. Every function returns QLDPC_OK (0) or a negative
 *    QLDPC_E* code; qldpc_last_error() gives a message (thread-local).
 *  - "d_" pointers are device (HBM) pointers; "h_" pointers are host memory.
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *    Device entry points are asynchronous on that stream. In the steady state
 *    they do no allocation, copy or synchronisation (hipGraph-capturable),
 *    with these exceptions:
 *     - the first decode of a (schedule, algo) after creation or after a
 *       qldpc_set_option queries the device (occupancy) to build its launch
 *       plan; no allocation, no synchronisation;
 *     - a decode that takes the HBM-resident kernel (codes past the LDS
 *       kernels, option force_hbm) grows the schedule's workspace when the
 *       batch needs more tiles than it holds: hipMemGetInfo, then a wait for
 *       the last launch that used the old workspace, hipFree and hipMalloc.
 *       It never shrinks; qldpc_schedule_release_workspace frees it;
 *     - the GPU OSD whose working matrix lives in global memory (m > 1024,
 *       n > 2111 or option osd_hbm) takes its scratch with hipMallocAsync /
 *       hipFreeAsync on `stream`, every call;
 *     - the first OSD call for a code builds rank(H) and its column
 *       bit-vectors on the host, and the first GPU OSD on a device allocates
 *       and zeroes a small per-device ticket array (hipMalloc, hipMemset);
 *     - option osd_prof synchronises `stream` and copies counters, every call.
 *  - Decodes of one schedule take their half-shot queue counter from a ring
 *    of 64 slots: at most 64 launches of one schedule may be in flight at
 *    once across all streams.
 *  - Results are bit-exact with the reference for MS (hard decisions,
 *    iteration counts, float64 posteriors) and for BP,
 *    whose tanh / arctanh / log restate the NumPy 2.2.6 / SVML functions the
 *    reference runs on the capture host (include/qldpc_libm.h); against other
 *    NumPy builds the north star's 1e-5 relative contract on BP posteriors
 *    (App. A.2) is what holds.
 */
#ifndef QLDPC_DECODER_H
#define QLDPC_DECODER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLDPC_OK 0
#define QLDPC_EINVAL -1   /* bad argument / shape / option   (reference: ValueError)  */
#define QLDPC_ERANGE -2   /* index out of range               (reference: IndexError)  */
#define QLDPC_EUNSUP -3   /* graph outside the kernel's limits (degree, size, LDS)     */
#define QLDPC_EHIP -4     /* a HIP runtime call failed          (raised as RuntimeError) */
#define QLDPC_ENOMEM -5

#define QLDPC_ALGO_MS 0   /* normalized min-sum, decoders.py:110-182 */
#define QLDPC_ALGO_BP 1   /* sum-product (tanh rule), decoders.py:189-290 */
#define QLDPC_ALGO_NG 2   /* naive greedy, decoders.py:27-66     (qldpc_hard_decode_* only) */
#define QLDPC_ALGO_BF 3   /* bit flipping, decoders.py:74-102    (qldpc_hard_decode_* only) */

/* Bit formats of syndromes and hard decisions on the device (the *_ex entry
 * points): one byte per bit, or 64-bit words with bit j % 64 of word j / 64
 * (rows of ceil(len / 64) words; the layout of the sampler's error vectors,
 * the reference's sample row bits packed, simulator.py:246-252). */
#define QLDPC_FMT_BYTES 0
#define QLDPC_FMT_BITS 1

/* per-shot flag bits written to d_flags */
#define QLDPC_FLAG_CONVERGED 1 /* a syndrome check passed (decoders.py:175-176 / :283-285) */
#define QLDPC_FLAG_MIN_ZERO 2  /* MS: a check saw min|v|==0 (not emulated) */
#define QLDPC_FLAG_NONFINITE 4 /* BP: tanh(v/2)==0 or a non-finite message */

typedef struct qldpc_code qldpc_code;         /* Tanner graph of one H, resident in HBM */
typedef struct qldpc_schedule qldpc_schedule; /* layer partition bound to one code     */
typedef struct qldpc_logicals qldpc_logicals; /* logical operators of a CSS pair, in HBM */
typedef struct qldpc_relay qldpc_relay;       /* relay min-sum: legs and memory strengths of one code */
typedef struct qldpc_prior qldpc_prior;       /* one prior probability per variable of one code */
typedef struct qldpc_channel qldpc_channel;   /* per-qubit Pauli probabilities of a CSS pair */
typedef struct qldpc_phenom qldpc_phenom;     /* logical table of one CSS half (phenomenological noise) */
typedef struct qldpc_dem qldpc_dem;           /* detector error model: thresholds and [H; L] by column */

const char *qldpc_last_error(void);
const char *qldpc_version(void);

/* Number of visible HIP devices (0 if none; never fails). */
int qldpc_device_count(void);

/* Build the Tanner graph of H (row-major uint8 m x n, entries taken mod 2,
 * as load_matrix's `(mat % 2)`, simulator.py:35; any size) and upload it to
 * the current device. Replaces the per-call `np.where(H)` edge construction of
 * BP_decoder (decoders.py:224-229) and MS_decoder's dense H masks
 * (decoders.py:148-169). */
int qldpc_code_create(const uint8_t *h_H, int m, int n, qldpc_code **out);
int qldpc_code_destroy(qldpc_code *code);
int qldpc_code_shape(const qldpc_code *code, int *m, int *n, int *n_edges);

/* Bind a layer partition to a code: layer l holds rows
 * h_layer_rows[h_layer_ptr[l] .. h_layer_ptr[l+1]). Replaces MS_decoder's /
 * BP_decoder's `layers` list (decoders.py:114, :193, consumed at :154 / :247).
 * One layer holding every row = flooding. Rows out of range -> QLDPC_ERANGE
 * (reference: IndexError at decoders.py:156 / :250). Duplicate rows inside a
 * layer are dropped (the reference's Jacobi update makes them idempotent). */
int qldpc_schedule_create(const qldpc_code *code, int n_layers, const int32_t *h_layer_ptr,
                          const int32_t *h_layer_rows, qldpc_schedule **out);
int qldpc_schedule_destroy(qldpc_schedule *sched);
/* Frees the schedule's HBM-resident-kernel workspace (grown on demand, up to
 * half of the free device memory; kept between launches otherwise), after
 * the last launch that used it has finished. The next HBM decode allocates
 * it again. */
int qldpc_schedule_release_workspace(qldpc_schedule *sched);

/* Batched decode, device pointers, asynchronous on `stream`.
 * Replaces `batch` calls of MS_decoder / BP_decoder (without the OSD
 * post-step, which the host applies to non-converged shots via
 * qldpc_osd_decode) — the inner loop of simulate_p (simulator.py:244-304).
 *   d_syn   uint8 [batch][m]   syndrome bits (0/1)
 *   p       prior error probability as passed to MS_decoder (simulate uses p/3)
 *   beta    MS normalisation (0.75 default; ignored by BP)
 *   eps     decoders.py's eps (1e-9)
 *   d_ehat  uint8 [batch][n]   hard decisions, original column order
 *   d_iters int32 [batch]      iterations as returned by the reference
 *   d_post  double[batch][n]   final posterior LLRs (nullable)
 *   d_flags int32 [batch]      QLDPC_FLAG_* (nullable)
 * Any size of H decodes: codes whose per-half-shot state fits a CU's LDS
 * (and whose tables fit 16 bits) run the LDS-resident kernels, others the
 * HBM-resident kernel (row degree <= 64), with identical results. The
 * prior L = log((1-p)/max(p, eps)) is NumPy's log (decoders.py:147, :232). */
int qldpc_decode_device(const qldpc_code *code, const qldpc_schedule *sched, int algo,
                        const uint8_t *d_syn, int64_t batch, double p, int max_iter, double beta,
                        double eps, uint8_t *d_ehat, int32_t *d_iters, double *d_post,
                        int32_t *d_flags, void *stream);

/* Name of the kernel qldpc_decode_device launches for (code, sched, algo),
 * as rocprofv3 reports it (e.g. "ms_flood_kernel<8, 4>"): lets a benchmark
 * match its live timings to a committed counter profile. No reference
 * counterpart (measurement only). */
int qldpc_decode_kernel_name(const qldpc_code *code, const qldpc_schedule *sched, int algo,
                             char *buf, int len);

/* The launch geometry of that kernel: waves per workgroup, resident
 * workgroups per CU and LDS bytes per workgroup (0, 0, 0 for the
 * HBM-resident kernel, whose geometry is fixed). Measurement only. */
int qldpc_decode_launch_info(const qldpc_code *code, const qldpc_schedule *sched, int algo,
                             int *waves_per_wg, int *wg_per_cu, int *lds_bytes);

/* qldpc_decode_device with a choice of formats: d_syn uint8 [batch][m]
 * (QLDPC_FMT_BYTES) or uint64 [batch][ceil(m/64)] (QLDPC_FMT_BITS); d_ehat
 * uint8 [batch][n] or uint64 [batch][ceil(n/64)]. Bit-packed I/O cuts the
 * kernel's HBM bytes per half-shot from m + n to 8 (ceil(m/64) + ceil(n/64)). */
int qldpc_decode_device_ex(const qldpc_code *code, const qldpc_schedule *sched, int algo, const void *d_syn,
                           int syn_format, int64_t batch, double p, int max_iter, double beta, double eps,
                           void *d_ehat, int ehat_format, int32_t *d_iters, double *d_post, int32_t *d_flags,
                           void *stream);

/* Same with host buffers: stages through page-locked host memory and device
 * memory on a stream of its own (asynchronous DMA copies, then a wait on that
 * stream only).
 * This is what the single-shot drop-in shims (MS_decoder / BP_decoder) use. */
int qldpc_decode_host(const qldpc_code *code, const qldpc_schedule *sched, int algo,
                      const uint8_t *h_syn, int64_t batch, double p, int max_iter, double beta,
                      double eps, uint8_t *h_ehat, int32_t *h_iters, double *h_post,
                      int32_t *h_flags);

/* qldpc_decode_device_ex with a two-level prior per half-shot (correlated
 * X/Z decoding of depolarizing noise: the first half's estimate is the second
 * half's mask). No reference counterpart.
 *   d_mask   one bit per variable, original column order, in mask_format:
 *            uint8 [batch][n] (0/1) or uint64 [batch][ceil(n/64)], the layouts
 *            of d_ehat; it may be an earlier decode's d_ehat, not this call's
 *   p0, p1   variable j decodes with the prior L0 = log((1-p0)/max(p0, eps))
 *            where its mask bit is 0 and L1 (of p1) where it is 1; both must
 *            lie in [0, 1] (QLDPC_EINVAL otherwise; p1 = 0.5 gives L1 = +0.0:
 *            min-sum then sets QLDPC_FLAG_MIN_ZERO, BP divides 0 by 0 as the
 *            reference would and sets QLDPC_FLAG_NONFINITE)
 * The arithmetic is the scalar decode's with L replaced by the variable's own
 * L_j everywhere (the float32(L_j) first pass of min-sum included); with
 * p0 == p1 every output equals the scalar decode's bit for bit, whatever the
 * mask. Runs decode_prior_kernel, the generic LDS kernel's twin: QLDPC_EUNSUP,
 * before any launch, for a code that kernel cannot hold (m, n or edges >
 * 65535, MS row degree > 32, BP column degree > 128, state past the LDS) or
 * with option "force_hbm" set; there is no HBM-resident variant. Arguments are
 * checked before any HIP call. */
int qldpc_decode_device_prior(const qldpc_code *code, const qldpc_schedule *sched, int algo, const void *d_syn,
                              int syn_format, int64_t batch, double p0, double p1, const void *d_mask,
                              int mask_format, int max_iter, double beta, double eps, void *d_ehat,
                              int ehat_format, int32_t *d_iters, double *d_post, int32_t *d_flags, void *stream);

/* Same with host buffers and a byte mask (uint8 [batch][n]), staged like
 * qldpc_decode_host. */
int qldpc_decode_host_prior(const qldpc_code *code, const qldpc_schedule *sched, int algo, const uint8_t *h_syn,
                            int64_t batch, double p0, double p1, const uint8_t *h_mask, int max_iter,
                            double beta, double eps, uint8_t *h_ehat, int32_t *h_iters, double *h_post,
                            int32_t *h_flags);

/* Name of the kernel qldpc_decode_device_prior launches, as rocprofv3 reports
 * it (e.g. "decode_prior_kernel<0, false, 8>"); needs no device. */
int qldpc_decode_prior_kernel_name(const qldpc_code *code, const qldpc_schedule *sched, int algo, char *buf,
                                   int len);

/* Per-variable priors: one error probability per column of
 * H, the `channel_probs` vector of other BP / BP-OSD packages. No reference
 * counterpart (the reference's decoders take a scalar p).
 *   h_p   float64 [n], original column order, every 0 <= p_j < 1 (anything
 *         else, NaN included: QLDPC_EINVAL)
 *   eps   decoders.py's eps (1e-9); it belongs to the handle
 * Creation forms L_j = log((1 - p_j) / max(p_j, eps)) with NumPy's log, as the
 * scalar entry forms L (an L_j that is not finite: QLDPC_EINVAL), permutes the
 * row to the kernels' variable order and uploads it once (one hipMalloc, one
 * synchronous copy). The code must outlive the handle. Without a visible
 * device the handle is still made (as qldpc_code_create); decoding then fails
 * with QLDPC_EHIP. A handle serves every schedule of its code. */
int qldpc_prior_create(const qldpc_code *code, const double *h_p, double eps, qldpc_prior **out);
int qldpc_prior_destroy(qldpc_prior *prior);

/* qldpc_decode_device_ex with the handle's prior row in place of p and eps:
 * the scalar decode's arithmetic with L replaced by the variable's own L_j
 * everywhere (min-sum's first check-node pass reads float32(L_j) per edge;
 * the layered schedules' initial check parities follow L_j < 0 per variable).
 * With every p_j equal the outputs equal the scalar decode's bit for bit, and
 * with two distinct values qldpc_decode_device_prior's whose mask rows are
 * the indicator of the second. p_j = 0.5 behaves as p1 = 0.5 there
 * (QLDPC_FLAG_MIN_ZERO / QLDPC_FLAG_NONFINITE). Runs decode_vprior_kernel, the
 * generic LDS kernel's second twin, which keeps the row in LDS (8 n bytes per
 * workgroup): QLDPC_EUNSUP, before any launch, under the conditions of
 * qldpc_decode_device_prior (m, n or edges > 65535, MS row degree > 32, BP
 * column degree > 128, state past the LDS, option "force_hbm"). With option
 * "vprior_hbm" set those cases decode instead, with hbm_tile_vprior_kernel:
 * the HBM-resident kernel reading L_j from the handle's row, at any size and
 * degree, bit for bit with decode_vprior_kernel where both run ("force_hbm"
 * as well: every call takes it). A handle made
 * for another code: QLDPC_EINVAL. Arguments are checked before any HIP call;
 * asynchronous on `stream`, a launch plan of its own per (schedule, algo). */
int qldpc_decode_device_vprior(const qldpc_code *code, const qldpc_schedule *sched, int algo, const void *d_syn,
                               int syn_format, int64_t batch, const qldpc_prior *prior, int max_iter, double beta,
                               void *d_ehat, int ehat_format, int32_t *d_iters, double *d_post, int32_t *d_flags,
                               void *stream);

/* Same with host buffers (one byte per bit), staged like qldpc_decode_host. */
int qldpc_decode_host_vprior(const qldpc_code *code, const qldpc_schedule *sched, int algo, const uint8_t *h_syn,
                             int64_t batch, const qldpc_prior *prior, int max_iter, double beta, uint8_t *h_ehat,
                             int32_t *h_iters, double *h_post, int32_t *h_flags);

/* Name of the kernel qldpc_decode_device_vprior launches, as rocprofv3 reports
 * it (e.g. "decode_vprior_kernel<0, false, 8>"); needs no device. With option
 * "vprior_hbm": "hbm_tile_vprior_kernel<0, 8, 4>" (algo, row-degree bound 8 /
 * 16 / 32 / 64, waves) where the LDS kernel cannot run; that needs no device
 * either unless the LDS size decides (state past the LDS: asked of the launch
 * plan when the code has a device, else the LDS kernel's name). */
int qldpc_decode_vprior_kernel_name(const qldpc_code *code, const qldpc_schedule *sched, int algo, char *buf,
                                    int len);

/* Relay min-sum (Relay-BP, Mueller et al. 2025): flooding
 * min-sum whose prior is blended with each variable's own previous posterior,
 *   Lam_j = fl((1 - gamma[r][j]) L) + fl(gamma[r][j] M_j),   M_j = Lam_j + S_j,
 * run as `legs` chained legs of leg_iters[r] iterations: leg 0 starts from
 * M = L, every later leg from the previous leg's M with c2v = 0; a leg ends at
 * its first pass whose hard decisions (M < 0) satisfy the syndrome, and the
 * decoder stops after `sols` such solutions, keeping the lightest (ties: the
 * earlier). No reference counterpart; with one leg, gamma = 0 and sols = 1 it
 * is min-sum flooding bit for bit (e_hat, iterations, posteriors, CONVERGED).
 *   h_leg_iters  int32 [legs], each >= 1, their sum <= 2^20
 *   h_gamma      float64 [legs][n_gamma], original column order, finite;
 *                n_gamma must be the code's n
 *   sols         >= 1
 * Anything else is QLDPC_EINVAL. Limits are the generic LDS kernel's: m, n and
 * edges <= 65535, row degree <= 32, tables and one wave's state within the
 * LDS; past them, and with option "force_hbm" set, QLDPC_EUNSUP (there is no
 * HBM-resident variant). Creation needs no device (decoding does). */
int qldpc_relay_create(const qldpc_code *code, int legs, const int32_t *h_leg_iters, const double *h_gamma,
                       int n_gamma, int sols, qldpc_relay **out);
int qldpc_relay_destroy(qldpc_relay *relay);

/* The per-wave LDS layout of the relay kernel (no device needed), bytes:
 * out7 = {graph image, wave slice, offsets inside the slice of c2v, the
 * syndrome words, the posterior row M, the hard-decision words, the
 * best-solution words}; the row the check nodes read is at offset 0. */
int qldpc_relay_layout(const qldpc_relay *relay, int32_t *out7);

/* Decode `batch` syndromes with the handle's legs; device pointers,
 * asynchronous on `stream`. Buffers and formats as qldpc_decode_device_ex;
 * the prior is L = log((1-p)/max(p, eps)), beta the min-sum normalisation.
 *   d_iters  int32 [batch]  passes run over all legs
 *   d_post   float64 [batch][n] (nullable) the last pass's M
 *   d_flags  int32 [batch] (nullable) QLDPC_FLAG_CONVERGED iff a solution was
 *            found; QLDPC_FLAG_MIN_ZERO if a check-node pass met a zero minimum
 *   d_info   int32 [batch][2] (nullable) solutions found, and the leg of the
 *            one returned (-1: none; e_hat is then the last pass's M < 0)
 * Arguments are checked before any HIP call. Options "static_sched",
 * "waves_per_wg" and "wg_per_cu" apply as for qldpc_decode_device. */
int qldpc_decode_device_relay(const qldpc_code *code, const qldpc_relay *relay, const void *d_syn, int syn_format,
                              int64_t batch, double p, double beta, double eps, void *d_ehat, int ehat_format,
                              int32_t *d_iters, double *d_post, int32_t *d_flags, int32_t *d_info, void *stream);

/* Same with host buffers (one byte per bit), staged like qldpc_decode_host. */
int qldpc_decode_host_relay(const qldpc_code *code, const qldpc_relay *relay, const uint8_t *h_syn, int64_t batch,
                            double p, double beta, double eps, uint8_t *h_ehat, int32_t *h_iters, double *h_post,
                            int32_t *h_flags, int32_t *h_info);

/* Name of the kernel qldpc_decode_device_relay launches ("relay_ms_kernel<8>";
 * needs no device) and its launch geometry (as qldpc_decode_launch_info). */
int qldpc_decode_relay_kernel_name(const qldpc_code *code, const qldpc_relay *relay, char *buf, int len);
int qldpc_decode_relay_launch_info(const qldpc_code *code, const qldpc_relay *relay, int *waves_per_wg,
                                   int *wg_per_cu, int *lds_bytes);

/* Relay min-sum with one prior per variable:
 * qldpc_decode_device_relay with the prior handle's row in place of p, so
 *   Lam_j = fl((1 - gamma[r][j]) L_j) + fl(gamma[r][j] M_j),   leg 0 starts from M_j = L_j,
 * and everything else as there. `prior` is a qldpc_prior of the same code
 * (another code's: QLDPC_EINVAL) and `eps` must be the eps its row was formed
 * with (QLDPC_EINVAL otherwise: the row cannot be re-formed per call).
 * `cost` chooses what "lightest" means among the solutions found:
 *   QLDPC_RELAY_COST_HAMMING  the number of set bits, as qldpc_decode_device_relay
 *   QLDPC_RELAY_COST_PRIOR    sum of W_j over the set bits, W_j = llrint(L_j 2^20)
 *                             (int64, round-half-even; exact, so independent of
 *                             the order of summation; W_j < 0 where p_j > 1/2)
 * ties keep the earlier solution under both; any other value is QLDPC_EINVAL.
 * With every p_j equal and QLDPC_RELAY_COST_HAMMING the outputs equal
 * qldpc_decode_device_relay's bit for bit. Runs relay_vprior_kernel, which
 * keeps the row in LDS behind the graph image (8 n bytes, rounded up to 16,
 * per workgroup); the limits are qldpc_relay_create's, QLDPC_EUNSUP where the
 * image, the row and one wave's state pass the LDS. Arguments are checked
 * before any HIP call; a launch plan of its own per relay handle. */
#define QLDPC_RELAY_COST_HAMMING 0
#define QLDPC_RELAY_COST_PRIOR 1
int qldpc_decode_device_relay_vprior(const qldpc_code *code, const qldpc_relay *relay, const qldpc_prior *prior,
                                     int cost, const void *d_syn, int syn_format, int64_t batch, double beta,
                                     double eps, void *d_ehat, int ehat_format, int32_t *d_iters, double *d_post,
                                     int32_t *d_flags, int32_t *d_info, void *stream);

/* Same with host buffers (one byte per bit), staged like qldpc_decode_host. */
int qldpc_decode_host_relay_vprior(const qldpc_code *code, const qldpc_relay *relay, const qldpc_prior *prior,
                                   int cost, const uint8_t *h_syn, int64_t batch, double beta, double eps,
                                   uint8_t *h_ehat, int32_t *h_iters, double *h_post, int32_t *h_flags,
                                   int32_t *h_info);

/* Name of the kernel qldpc_decode_device_relay_vprior launches
 * ("relay_vprior_kernel<8>", the instance chosen as relay_ms_kernel's; needs
 * no device), its launch geometry, and its LDS layout (no device needed):
 * qldpc_relay_layout's with the prior row counted in out7[0], the slice and
 * its offsets unchanged. */
int qldpc_decode_relay_vprior_kernel_name(const qldpc_code *code, const qldpc_relay *relay, char *buf, int len);
int qldpc_decode_relay_vprior_launch_info(const qldpc_code *code, const qldpc_relay *relay, int *waves_per_wg,
                                          int *wg_per_cu, int *lds_bytes);
int qldpc_relay_vprior_layout(const qldpc_relay *relay, int32_t *out7);

/* The hard-decision decoders, batched, device pointers, asynchronous on
 * `stream`. Replaces `batch` calls of NG_decoder(H, syndrome)
 * (decoders.py:27-66) or BF_decoder(H, syndrome, max_iter) (:74-102) — what
 * simulate_p runs for decType NG / BF (simulator.py:270-276). They take no
 * schedule, prior or posteriors; results equal the reference's bit for bit
 * (integer arithmetic only), its quirks included: BF's residual is "row holds
 * a set estimate bit" XOR syndrome, a non-zero count and not a parity
 * (:97-98), and NG flips the lowest-index variable among equal scores (:59).
 *   algo     QLDPC_ALGO_NG or QLDPC_ALGO_BF (anything else: QLDPC_EINVAL; the
 *            qldpc_decode_* functions answer QLDPC_EINVAL for these two)
 *   d_syn    uint8 [batch][m] or uint64 [batch][ceil(m/64)]  (syn_format)
 *   max_iter BF's iteration limit, >= 1 (the reference's default is 50);
 *            ignored for NG, whose limit is 2n steps
 *   d_ehat   uint8 [batch][n] or uint64 [batch][ceil(n/64)]  (ehat_format)
 *   d_iters  int32 [batch]  BF: iterations as returned; NG: steps
 *   d_flags  int32 [batch]  (nullable) QLDPC_FLAG_CONVERGED when the
 *            reference's own stop condition held: BF's residual above all
 *            zero (the true parity may still differ), NG's residual all zero
 * Limits: m, n and the number of edges <= 65535 (16-bit tables; every such
 * code's per-wave state fits a CU's LDS); past that, QLDPC_EUNSUP. An empty
 * matrix is QLDPC_EINVAL. Arguments are checked before any HIP call. The
 * first decode of a (code, algo) after creation or a qldpc_set_option uploads
 * the code's tables (once) and queries the device for its launch plan; later
 * ones only launch. Option "static_sched" applies as for qldpc_decode_device;
 * at most 64 launches of one code may be in flight at once. */
int qldpc_hard_decode_device(const qldpc_code *code, int algo, const void *d_syn, int syn_format,
                             int64_t batch, int max_iter, void *d_ehat, int ehat_format, int32_t *d_iters,
                             int32_t *d_flags, void *stream);

/* Same with host buffers (one byte per bit), staged through the code's
 * page-locked workspace, the one qldpc_decode_host uses. What the single-shot
 * shims NG_decoder / BF_decoder call. */
int qldpc_hard_decode_host(const qldpc_code *code, int algo, const uint8_t *h_syn, int64_t batch,
                           int max_iter, uint8_t *h_ehat, int32_t *h_iters, int32_t *h_flags);

/* Name of the kernel qldpc_hard_decode_device launches ("ng_kernel",
 * "bf_kernel"), as rocprofv3 reports it, and its launch geometry (as
 * qldpc_decode_launch_info). Measurement only. */
int qldpc_hard_kernel_name(const qldpc_code *code, int algo, char *buf, int len);
int qldpc_hard_launch_info(const qldpc_code *code, int algo, int *waves_per_wg, int *wg_per_cu,
                           int *lds_bytes);

/* OSD post-decoder, host. Replaces OSDdec (decoders.py:299-370) including its
 * aliasing semantics: order 0 -> solve;
 * order 1 -> flip the first information-set position, then solve;
 * order >= 2 -> identical to order 0. `h_ehat` (uint8[n]) is updated in place
 * like the reference's `e_hat[perm] = ...` (decoders.py:368).
 *   h_perm   int32[n]: np.argsort(reliability) as decoders.py:320-325 computes
 *            it (NumPy itself, or qldpc_osd_order_host).
 *   h_J / h_J_size (nullable): the complementary information set (positions
 *            in perm order, decoders.py:329-342), h_J sized n.
 *   first_info_index: position the order-1 flip applies to (infoSet[0]);
 *            -1 = emulate CPython's `list(set(range(n)) - set(J))[0]`.
 * Errors: QLDPC_ERANGE where the reference raises IndexError (the greedy basis
 * loop runs past column n-1). */
int qldpc_osd_decode(const qldpc_code *code, const uint8_t *h_syn, const int32_t *h_perm, int order,
                     uint8_t *h_ehat, int32_t *h_J, int32_t *h_J_size, int first_info_index);

/* Batched OSD over `count` shots (syn uint8[count][m], perm int32[count][n],
 * ehat uint8[count][n] in/out), `nthreads` host threads (<= 0: the process's
 * budget — affinity mask, cgroup cpu.max quota, OMP_NUM_THREADS). */
int qldpc_osd_decode_batch(const qldpc_code *code, int64_t count, const uint8_t *h_syn,
                           const int32_t *h_perm, int order, uint8_t *h_ehat, int nthreads);

/* Batched OSD on the device: one workgroup per shot, asynchronous on `stream`.
 * Same semantics as qldpc_osd_decode (orders 0, 1, >= 2) for `count` shots:
 * d_syn uint8[count][m], d_perm int32[count][n] (NumPy's reliability order),
 * d_ehat uint8[count][n] in/out, d_status int32[count] (0 ok; 1 = the
 * reference's IndexError case, e_hat left unchanged). Any size: m <= 1024 and
 * n <= 2111 run in registers / LDS, larger codes with each shot's working
 * matrix in device memory (osd_hbm_kernel; LDS holds one 64-bit word per row,
 * so m is bounded by the LDS size, about 19,000 rows: QLDPC_EUNSUP past it). */
int qldpc_osd_device(const qldpc_code *code, int64_t count, const uint8_t *d_syn,
                     const int32_t *d_perm, int order, uint8_t *d_ehat, int32_t *d_status,
                     void *stream);

/* The reliability order of decoders.py:320-325 on the device, for `count`
 * posterior rows d_post double[count][n] (n <= 2048): d_perm int32[count][n]
 * = np.argsort of the keys max(prob, 1 - prob), prob = 1/(1 + np.exp(
 * clip(post, +-100))), exactly as NumPy 2.2.6 computes them on x86-64
 * AVX512_SKX: the key through SVML's exp8_ha (include/qldpc_libm.h), the order
 * through x86-simd-sort's argsort, equal keys included (np_order.cpp states
 * the algorithm). d_tiepos[row] = n for an exact order; -1 where this order
 * leaves the row to NumPy itself (a NaN posterior, or x86-simd-sort's
 * std::sort fallback after 2 floor(log2 n) partition levels). No reference
 * counterpart as an entry point (it replaces the np.argsort call inside
 * OSDdec, decoders.py:325). */
int qldpc_osd_order_device(const qldpc_code *code, int64_t count, const double *d_post, int32_t *d_perm,
                           int32_t *d_tiepos, void *stream);

/* The same order on the host (C++, `nthreads` threads, <= 0: the process's
 * budget as qldpc_osd_decode_batch): h_perm int32[count][n],
 * h_status int32[count] = 0 exact, 1 left to NumPy (as tiepos -1 above).
 * Used to check at import that the running NumPy dispatches to the restated
 * functions (qldpcsim_amd/decoders.py), and by the host OSD path. */
int qldpc_osd_order_host(const double *h_post, int64_t count, int n, int32_t *h_perm, int32_t *h_status,
                         int nthreads);

/* x86-simd-sort's argsort (np.argsort, default kind, float64) of n keys into
 * h_perm; returns 0, or 1 for a case left to NumPy (NaN, std::sort fallback). */
int qldpc_np_argsort_host(const double *h_key, int n, int32_t *h_perm);

/* The reliability keys themselves (qldpc_osd_key), element-wise; exp_only != 0:
 * np.exp alone (SVML exp8_ha restated, |x| < 707). */
void qldpc_osd_keys_host(const double *h_post, int64_t count, double *h_key, int exp_only);

/* The restated NumPy libm (include/qldpc_libm.h: the code the BP kernels and
 * the priors run), element-wise on the host: y[i] = f(x[i]) with f = np.tanh
 * (QLDPC_LIBM_TANH, decoders.py:254), np.arctanh (QLDPC_LIBM_ATANH, :259),
 * np.log (QLDPC_LIBM_LOG, :147, :232) or np.exp (QLDPC_LIBM_EXP, :322).
 * Replaces no reference interface: it lets a caller check at run time that
 * the NumPy it runs computes the same bits (decoders.numpy_libm_pinned). */
#define QLDPC_LIBM_TANH 0
#define QLDPC_LIBM_ATANH 1
#define QLDPC_LIBM_LOG 2
#define QLDPC_LIBM_EXP 3
int qldpc_libm_eval_host(int fn, const double *h_x, int64_t count, double *h_y);

/* qldpc_osd_device with the order computed on the device
 * (qldpc_osd_order_device into the caller's workspaces d_perm / d_tiepos):
 * a shot whose order the device leaves to NumPy (tiepos -1) gets d_status 2
 * and its e_hat is left unchanged: the caller decides it with NumPy's order
 * (qldpc_osd_device). Status 0 / 1 as qldpc_osd_device. */
int qldpc_osd_device_ordered(const qldpc_code *code, int64_t count, const uint8_t *d_syn, const double *d_post,
                             int order, uint8_t *d_ehat, int32_t *d_status, int32_t *d_perm, int32_t *d_tiepos,
                             void *stream);

/* qldpc_osd_device_ordered plus a spill of the shots it leaves to the host:
 * each status-2 shot also copies its posterior row to d_spill_post[slot]
 * (double[spill_cap][n]) and its index (0 .. count-1) to d_spill_idx[slot],
 * slot = the next value of *d_spill_count (int32, zeroed by the caller), for
 * slot < spill_cap; *d_spill_count ends as the number of status-2 shots. The
 * host then fetches exactly those posteriors with one copy (no gather
 * kernel queued behind other work). */
int qldpc_osd_device_ordered_ex(const qldpc_code *code, int64_t count, const uint8_t *d_syn, const double *d_post,
                                int order, uint8_t *d_ehat, int32_t *d_status, int32_t *d_perm, int32_t *d_tiepos,
                                double *d_spill_post, int32_t *d_spill_idx, int32_t *d_spill_count,
                                int64_t spill_cap, void *stream);

/* OSD-CS: combination-sweep OSD, the higher-order search the
 * reference's OSDdec does not have (its order 1 flips one bit, orders >= 2
 * equal order 0). No reference counterpart. With perm, J (the greedy set of
 * decoders.py:329-342, in perm positions) and T (the other positions,
 * ascending) as in qldpc_osd_decode, the candidates are, in this order:
 *   the order-0 result e0;
 *   for k = 0 .. |T|-1: e0 with position T[k] flipped and e_J solved again;
 *   for a < b < min(lambda, |T|), lexicographic: the same with T[a] and T[b].
 * The result is the first candidate of strictly smallest Hamming weight (all n
 * bits). The order-0 result is returned as it is where the syndrome lies
 * outside H's column space, and (host) where column perm[0] of H is all-zero.
 * 0 <= lambda <= QLDPC_OSD_CS_MAX_LAMBDA, else QLDPC_EINVAL. Errors and
 * status values otherwise as the entry point each one is named after.
 * The host form takes any code. The device forms run osd_block_kernel's range
 * only: m <= 512, n <= 1087 and no all-zero column in H; any other code, and
 * options osd_column / osd_hbm, give QLDPC_EUNSUP before any launch. Shots
 * that qldpc_osd_device_ordered(_ex)_cs leaves to NumPy's order (status 2)
 * are finished with qldpc_osd_device_cs. */
#define QLDPC_OSD_CS_MAX_LAMBDA 64
int qldpc_osd_decode_batch_cs(const qldpc_code *code, int64_t count, const uint8_t *h_syn,
                              const int32_t *h_perm, int lambda, uint8_t *h_ehat, int nthreads);
int qldpc_osd_device_cs(const qldpc_code *code, int64_t count, const uint8_t *d_syn, const int32_t *d_perm,
                        int lambda, uint8_t *d_ehat, int32_t *d_status, void *stream);
int qldpc_osd_device_ordered_cs(const qldpc_code *code, int64_t count, const uint8_t *d_syn, const double *d_post,
                                int lambda, uint8_t *d_ehat, int32_t *d_status, int32_t *d_perm,
                                int32_t *d_tiepos, void *stream);
int qldpc_osd_device_ordered_ex_cs(const qldpc_code *code, int64_t count, const uint8_t *d_syn,
                                   const double *d_post, int lambda, uint8_t *d_ehat, int32_t *d_status,
                                   int32_t *d_perm, int32_t *d_tiepos, double *d_spill_post,
                                   int32_t *d_spill_idx, int32_t *d_spill_count, int64_t spill_cap, void *stream);
/* OSD-CS with the prior-weighted cost: the same candidates in
 * the same order, but the cost of an estimate e is sum_j e_j W_j with W_j =
 * llrint(L_j 2^20), L_j the prior LLR of column j as `prior` holds it (exact
 * int64; W_j < 0 where p_j > 1/2). The first candidate of strictly smallest
 * cost wins, the base wins ties. `prior` must come from qldpc_prior_create for
 * this very code: a null handle or another code's gives QLDPC_EINVAL. A
 * uniform row with p < 1/2 gives the Hamming-cost result bit for bit. All else
 * (lambda, limits, errors, status values, the order-0 cases) as the _cs entry
 * point each one is named after; status-2 shots of the ordered forms are
 * finished with qldpc_osd_device_cs_prior. */
int qldpc_osd_decode_batch_cs_prior(const qldpc_code *code, int64_t count, const uint8_t *h_syn,
                                    const int32_t *h_perm, int lambda, const qldpc_prior *prior, uint8_t *h_ehat,
                                    int nthreads);
int qldpc_osd_device_cs_prior(const qldpc_code *code, int64_t count, const uint8_t *d_syn, const int32_t *d_perm,
                              int lambda, const qldpc_prior *prior, uint8_t *d_ehat, int32_t *d_status,
                              void *stream);
int qldpc_osd_device_ordered_cs_prior(const qldpc_code *code, int64_t count, const uint8_t *d_syn,
                                      const double *d_post, int lambda, const qldpc_prior *prior, uint8_t *d_ehat,
                                      int32_t *d_status, int32_t *d_perm, int32_t *d_tiepos, void *stream);
int qldpc_osd_device_ordered_ex_cs_prior(const qldpc_code *code, int64_t count, const uint8_t *d_syn,
                                         const double *d_post, int lambda, const qldpc_prior *prior,
                                         uint8_t *d_ehat, int32_t *d_status, int32_t *d_perm, int32_t *d_tiepos,
                                         double *d_spill_post, int32_t *d_spill_idx, int32_t *d_spill_count,
                                         int64_t spill_cap, void *stream);
/* The name of the kernel qldpc_osd_device(_cs, _cs_prior) launches for this code, into buf: cs = 0
 * ("osd_block_kernel<17, 8, 2>", ...), 1 ("osd_block_cs_kernel<17, 8, 2>") or 2, the prior-weighted cost
 * ("osd_block_cs_prior_kernel<17, 8, 2>"). Measurement and tests. */
int qldpc_osd_kernel_name(const qldpc_code *code, int cs, char *buf, int len);

/* First element of CPython's `set(range(n)) - set(J)` iteration order
 * (the reference's infoSet[0], decoders.py:344); -1 if empty. */
int qldpc_cpython_setdiff_first(int n, const int32_t *J, int nJ);

/* ---- Monte-Carlo shot source and counters on the device -----------------
 * Replace simulate_p's shot source and per-shot bookkeeping
 * (simulator.py:196-197 Stim sample, :249-252 row slicing, :291-303 outcome
 * counting) so that a batch never leaves HBM. hx / hz are the two codes of
 * the pair (same n), created on the current device.
 *
 * qldpc_channel_thresholds: the 32-bit draw thresholds of the depolarizing
 * channel, T_k = floor(k * (p/3) * 2^32) (k = 1, 2, 3); p outside [0, 1]
 * -> QLDPC_EINVAL (reference: assert at simulator.py:332).
 *
 * qldpc_channel_sample: shots shot0 .. shot0+batch-1 of the stream `seed`.
 * Per qubit j of shot s: u = Philox4x32-10(key = seed, counter = (j % 64,
 * (j / 64) / 4, s mod 2^32, s >> 32))[(j / 64) % 4]; X if u < T1, Y if
 * T1 <= u < T2, Z if T2 <= u < T3 (PAULI_CHANNEL_1(p/3,p/3,p/3),
 * simulator.py:107); errX = X|Y, errZ = Z|Y; sy_z = Hz errX mod 2,
 * sy_x = Hx errZ mod 2 (the circuit's detector layout, :249-252).
 *   d_errx, d_errz  uint64 [batch][ceil(n/64)]  bit j%64 of word j/64
 *   d_syn_z uint8 [batch][m_z],  d_syn_x uint8 [batch][m_x]
 *
 * qldpc_count_outcomes: adds this batch's outcomes to d_counters int64[6] =
 * {DecFailures_X, DecFailures_Z, decSuccessExact, decSuccessDegen,
 *  sum of iterations X, sum of iterations Z} with the reference's exact
 * definitions (simulator.py:291-303; "degen" is the integer, not mod-2,
 * product of :296-298). d_ehat_x: uint8 [batch][n] estimate of errX (the
 * decode of Hz / sy_z); d_ehat_z: estimate of errZ (Hx / sy_x); d_iters_*
 * int32 [batch]. Asynchronous on `stream`, no host synchronisation. */
int qldpc_channel_thresholds(double p, uint64_t *t1, uint64_t *t2, uint64_t *t3);
/* _ex forms: syndromes (and, for the counters, estimates) in either
 * QLDPC_FMT_* format. */
int qldpc_channel_sample_ex(const qldpc_code *hx, const qldpc_code *hz, double p, uint64_t seed,
                            uint64_t shot0, int64_t batch, uint64_t *d_errx, uint64_t *d_errz,
                            void *d_syn_z, void *d_syn_x, int syn_format, void *stream);
int qldpc_count_outcomes_ex(const qldpc_code *hx, const qldpc_code *hz, int64_t batch,
                            const uint64_t *d_errx, const uint64_t *d_errz, const void *d_syn_z,
                            const void *d_syn_x, int syn_format, const void *d_ehat_x, const void *d_ehat_z,
                            int ehat_format, const int32_t *d_iters_x, const int32_t *d_iters_z,
                            int64_t *d_counters, void *stream);
int qldpc_channel_sample(const qldpc_code *hx, const qldpc_code *hz, double p, uint64_t seed,
                         uint64_t shot0, int64_t batch, uint64_t *d_errx, uint64_t *d_errz,
                         uint8_t *d_syn_z, uint8_t *d_syn_x, void *stream);
int qldpc_count_outcomes(const qldpc_code *hx, const qldpc_code *hz, int64_t batch,
                         const uint64_t *d_errx, const uint64_t *d_errz, const uint8_t *d_syn_z,
                         const uint8_t *d_syn_x, const uint8_t *d_ehat_x, const uint8_t *d_ehat_z,
                         const int32_t *d_iters_x, const int32_t *d_iters_z, int64_t *d_counters,
                         void *stream);

/* ---- Inhomogeneous / biased Pauli channel --------------------------------
 * qldpc_channel_sample_ex with probabilities per qubit. No reference
 * counterpart (the reference's circuit is depolarizing, simulator.py:107).
 *
 * qldpc_channel_table (host only): the draw thresholds of n qubits into
 * t = uint64 [3][n], in float64:
 *   t[0][j] = min(2^32, floor(px_j 2^32)),
 *   t[1][j] = min(2^32, floor((px_j + py_j) 2^32)),
 *   t[2][j] = min(2^32, floor(((px_j + py_j) + pz_j) 2^32));
 * every px_j, py_j, pz_j >= 0 and (px_j + py_j) + pz_j <= 1, else QLDPC_EINVAL
 * (NaN included). With px = py = pz = p/3 the three are exactly
 * qldpc_channel_thresholds(p).
 *
 * qldpc_channel_create: validates as above, forms the table and uploads it
 * once to the codes' device; h_px, h_py, h_pz are float64 [n]. hx / hz must
 * outlive the handle; n <= 4096 (QLDPC_EUNSUP past it). Without a visible
 * device the handle is still made.
 *
 * qldpc_channel_sample_vec: the stream of qldpc_channel_sample — u(shot, j) is
 * the same Philox draw — with qubit j's own thresholds: X if u < t[0][j], Y if
 * t[0][j] <= u < t[1][j], Z if t[1][j] <= u < t[2][j]. Outputs and formats as
 * qldpc_channel_sample_ex; with a uniform depolarizing table they are that
 * call's bit for bit. Asynchronous on `stream`; arguments are checked before
 * any HIP call. */
int qldpc_channel_table(const double *px, const double *py, const double *pz, int n, uint64_t *t);
int qldpc_channel_create(const qldpc_code *hx, const qldpc_code *hz, const double *h_px, const double *h_py,
                         const double *h_pz, qldpc_channel **out);
int qldpc_channel_destroy(qldpc_channel *ch);
int qldpc_channel_sample_vec(const qldpc_channel *ch, uint64_t seed, uint64_t shot0, int64_t batch,
                             uint64_t *d_errx, uint64_t *d_errz, void *d_syn_z, void *d_syn_x, int syn_format,
                             void *stream);

/* ---- Logical error counting of a CSS pair -------------------------------
 * The reference's "degen" counter is an integer product that real codes never
 * satisfy (simulator.py:296), so it reports 1 - exact / shots. These entry
 * points add the stabiliser-group test: with Lx, Lz a paired basis of the
 * pair's logical operators (Hz Lx^T = 0, Hx Lz^T = 0, Lx Lz^T = I; the
 * package computes one in qldpcsim_amd/logicals.py), a residual
 * rX = errX ^ ehat_x whose syndrome is zero is an X stabiliser exactly when
 * Lz rX = 0 mod 2.
 *
 * qldpc_logicals_create: h_Lx, h_Lz are host uint8 [k][n] (0/1), 0 <= k <= n
 * (k = 0: both may be NULL). Validates the shapes, packs both tables
 * word-major (uint64 [ceil(n/64)][k padded to 64]) and uploads them to the
 * codes' device: two hipMalloc and two synchronous copies, once; a failure
 * frees what was uploaded. hx / hz must outlive the handle. Without a
 * visible device the handle is still made (as qldpc_code_create).
 * qldpc_logicals_destroy: hipFree of both tables; NULL is accepted.
 *
 * qldpc_count_logical_ex: qldpc_count_outcomes_ex and the logical test in one
 * kernel (one pass over the batch's rows; the six-counter kernel is not
 * launched). Per half-shot class: 2 decoder failure (H ehat != syndrome, the
 * reference's test, :300-303), 1 logical error (not 2 and L r != 0), 0 success
 * (not 2 and L r == 0; an exact match is class 0), L = Lz for the X half, Lx
 * for the Z half. The logical reading assumes syndrome = H err.
 *   d_counters  int64 [9], added to: the six of qldpc_count_outcomes, then
 *               {logicalErrors_X, logicalErrors_Z (class-1 half-shots),
 *                decSuccessLogical (shots with both halves class 0)}
 *   d_class_x, d_class_z  uint8 [batch]                     (NULL: not written)
 *   d_flip_x   uint64 [batch][ceil(k/64)]  Lz rX mod 2, bit i % 64 of word i / 64,
 *   d_flip_z   the same for Lx rZ; written as computed for every class,
 *              padding bits zero, nothing for k = 0            (NULL: not written)
 * Every argument check (null handles, a handle built for another pair or
 * device, unknown formats, negative batch, null required buffers) returns
 * before any HIP call; batch == 0 returns QLDPC_OK. Asynchronous on `stream`:
 * no allocation, no copy, no synchronisation. Option "logical_tabs" picks the
 * table residency (LDS / global memory). */
int qldpc_logicals_create(const qldpc_code *hx, const qldpc_code *hz, const uint8_t *h_Lx, const uint8_t *h_Lz,
                          int k, qldpc_logicals **out);
int qldpc_logicals_destroy(qldpc_logicals *lg);
int qldpc_count_logical_ex(const qldpc_code *hx, const qldpc_code *hz, const qldpc_logicals *lg, int64_t batch,
                           const uint64_t *d_errx, const uint64_t *d_errz, const void *d_syn_z,
                           const void *d_syn_x, int syn_format, const void *d_ehat_x, const void *d_ehat_z,
                           int ehat_format, const int32_t *d_iters_x, const int32_t *d_iters_z,
                           int64_t *d_counters, uint8_t *d_class_x, uint8_t *d_class_z, uint64_t *d_flip_x,
                           uint64_t *d_flip_z, void *stream);

/* The name of the kernel instance a launch for this pair uses
 * ("channel_sample_kernel<8>", "channel_sample_vec_kernel<0>",
 * "count_outcomes_kernel<7, true>", "count_logical_kernel<6, true, false>"),
 * into buf. kind: QLDPC_CHANNEL_*. est_aligned: both byte-estimate bases are
 * 4-byte aligned (the counters; word estimates always are); tabs_lds: the
 * residency qldpc_count_logical_ex picks (option "logical_tabs", the device's
 * LDS). The samplers ignore both, qldpc_count_outcomes_ex ignores tabs_lds.
 * Needs no device; n > 4096: QLDPC_EUNSUP. Measurement and tests. */
#define QLDPC_CHANNEL_SAMPLE 0
#define QLDPC_CHANNEL_SAMPLE_VEC 1
#define QLDPC_CHANNEL_COUNT 2
#define QLDPC_CHANNEL_COUNT_LOGICAL 3
int qldpc_channel_kernel_name(const qldpc_code *hx, const qldpc_code *hz, int kind, int est_aligned, int tabs_lds,
                              char *buf, int len);

/* ---- Phenomenological noise: multi-round space-time decoding -------------
 * T = rounds rounds of syndrome extraction of one CSS half: `code` is the
 * half's H [m][n] (the X half: Hz), L [k][n] its logical table (Lz). Round t
 * draws a data error e_t (probability p_data per qubit) and, for t < T-1, a
 * measurement error u_t (probability q per check); the last round is measured
 * perfectly. Detectors d_t = H e_t ^ u_t ^ u_{t-1} (u_{-1} = u_{T-1} = 0).
 * Space-time columns, round-major, N = T n + (T-1) m: round t owns data
 * columns t (n+m) + j and, for t < T-1, measurement columns t (n+m) + n + c;
 * detector rows M = T m, row t m + c. With T = 1 this is H itself. No
 * reference counterpart.
 *
 * qldpc_phenom_sample: shots shot0 .. shot0+batch-1 of the stream `seed`.
 * Column J of shot s fires iff u < thr_J with qldpc_channel_sample's draw,
 * u = Philox4x32-10(key = seed, counter = (J % 64, (J / 64) / 4, s mod 2^32,
 * s >> 32))[(J / 64) % 4], and thr_J = floor(prob 2^32), prob = p_data on
 * data and q on measurement columns: bit for bit qldpc_channel_sample_vec on
 * the materialised matrix with (px, py, pz) = (prior, 0, 0).
 *   d_det    uint8 [batch][M] (QLDPC_FMT_BYTES) or uint64 [batch][ceil(M/64)]
 *   d_E      uint64 [batch][ceil(n/64)]   XOR_t e_t, bit j % 64 of word j / 64
 *   d_fired  uint64 [batch][ceil(N/64)]   the whole fired row (NULL: not written)
 *
 * qldpc_phenom_create: h_L is host uint8 [k][n] (0/1), 0 <= k <= n (k = 0: may
 * be NULL); packs it word-major and uploads it once to the code's device.
 * `code` must outlive the handle. Without a visible device the handle is
 * still made. qldpc_phenom_destroy: NULL is accepted.
 *
 * qldpc_phenom_count: with Ehat the XOR of the estimate's T data blocks and
 * r = E ^ Ehat, a shot is class 2 (decoder failure) if H_st ehat != d, else
 * class 1 (logical error) if L r != 0 mod 2, else class 0 (success).
 *   d_ehat      uint8 [batch][N] or uint64 [batch][ceil(N/64)] (ehat_format)
 *   d_iters     int32 [batch]
 *   d_counters  int64 [4], added to: failures, logical errors, successes,
 *               sum of iterations
 *   d_class     uint8 [batch]                                (NULL: not written)
 *   d_flips     uint64 [batch][ceil(k/64)]  L r mod 2, as computed for every
 *               class, nothing for k = 0                     (NULL: not written)
 *   d_resid     uint64 [batch][ceil(n/64)]  r                (NULL: not written)
 *
 * Both: rounds < 1, a probability outside [0, 1), an unknown format, a
 * negative batch, a null handle or required buffer -> QLDPC_EINVAL, before any
 * HIP call. Limits (QLDPC_EUNSUP, before any launch): n <= 4096, m and E <=
 * 65535, and N bounded by a wave's LDS slice (H's CSR, for the counter L's
 * table up to 64 KiB, and 8 (ceil(N/64) + 1) bytes per wave, four waves).
 * Asynchronous on `stream`: no allocation, copy or synchronisation. */
int qldpc_phenom_create(const qldpc_code *code, const uint8_t *h_L, int k, qldpc_phenom **out);
int qldpc_phenom_destroy(qldpc_phenom *ph);
int qldpc_phenom_sample(const qldpc_code *code, int rounds, double p_data, double q, uint64_t seed, uint64_t shot0,
                        int64_t batch, void *d_det, int det_format, uint64_t *d_E, uint64_t *d_fired, void *stream);
int qldpc_phenom_count(const qldpc_code *code, const qldpc_phenom *ph, int rounds, int64_t batch, const void *d_det,
                       int det_format, const uint64_t *d_E, const void *d_ehat, int ehat_format,
                       const int32_t *d_iters, int64_t *d_counters, uint8_t *d_class, uint64_t *d_flips,
                       uint64_t *d_resid, void *stream);

/* The name of the sampler's or the counter's instance for this half
 * ("phenom_sample_kernel<8>", "phenom_count_kernel<0>"), into buf. kind:
 * QLDPC_PHENOM_*. phenom_window_kernel has one instance. Needs no device;
 * the code's limits as above. Measurement and tests. */
#define QLDPC_PHENOM_SAMPLE 0
#define QLDPC_PHENOM_COUNT 1
int qldpc_phenom_kernel_name(const qldpc_code *code, int kind, char *buf, int len);

/* qldpc_phenom_window: the step between two windows of sliding-window
 * decoding, one launch of phenom_window_kernel. A window (start a, rounds R)
 * covers rounds [a, a + R) of [0, T). An open window's matrix has R (n+m)
 * columns (every round has its measurement columns); a closed one ends at
 * round T, has the space-time matrix's R n + (R-1) m columns and commits all
 * of its rounds. Each of the four rows is QLDPC_FMT_BYTES or QLDPC_FMT_BITS on
 * its own format argument.
 *   done_*   the window just decoded (done_rounds = 0: none, the first step):
 *            its first done_commit (n+m) columns of d_west (closed: all) are
 *            copied to columns done_start (n+m) + . of d_ehat, the other
 *            columns of d_ehat stay as they are, and d_witers is added to
 *            d_iters.
 *     d_west    uint8 [batch][N_w] or uint64 [batch][ceil(N_w/64)]
 *     d_witers  int32 [batch]
 *     d_ehat    uint8 [batch][N] or uint64 [batch][ceil(N/64)], read and
 *               written; in words the padding bits past N are cleared by the
 *               step that commits column N - 1
 *     d_iters   int32 [batch], added to
 *   next_*   the window decoded next (next_rounds = 0: none, the last step;
 *            with a decoded window next_start = done_start + done_commit):
 *            d_syn = detectors next_start m .. (next_start + next_rounds) m of
 *            d_det, the first m of them XORed with the committed measurement
 *            estimate, columns (done_commit - 1) (n+m) + n + c of d_west.
 *     d_det     as qldpc_phenom_sample wrote it
 *     d_syn     uint8 [batch][next_rounds m] or uint64 words, padding bits zero
 * QLDPC_EINVAL, before any HIP call: a window outside [0, T), done_commit
 * outside [1, done_rounds], a closed window that does not end at T, commit all
 * its rounds or has a successor, an open window that ends at T (its last
 * round has measurement columns), neither window, an unknown format, a null
 * buffer of a window that is given, a negative batch. The code's limits are
 * those of qldpc_phenom_sample (QLDPC_EUNSUP); the kernel uses no LDS. The
 * wave that owns a shot's row merges the first and last word of a commit, so
 * successive windows are successive launches on one stream. Asynchronous on
 * `stream`: no allocation, copy or synchronisation. */
int qldpc_phenom_window(const qldpc_code *code, int rounds, int64_t batch, int done_start, int done_rounds,
                        int done_closed, int done_commit, const void *d_west, int west_format,
                        const int32_t *d_witers, void *d_ehat, int ehat_format, int32_t *d_iters, int next_start,
                        int next_rounds, const void *d_det, int det_format, void *d_syn, int syn_format,
                        void *stream);

/* ---- Detector error models ------------------------------------------------
 * A detector error model is N independent error mechanisms: mechanism J
 * fires with probability p_J and flips the detectors of column J of H [M][N]
 * and the logical observables of column J of L [K][N]. It is what a
 * circuit-level noise simulation yields (Stim's .dem files; the package reads
 * them in qldpcsim_amd/dem.py), and the phenomenological model above is the
 * special case (space-time matrix, folded logical table, prior row). The
 * decoders take H and the priors as any other matrix (qldpc_decode_device,
 * qldpc_decode_device_vprior); these entry points are the shot source and the
 * outcome counter around them. No reference counterpart.
 *
 * qldpc_dem_create: `code` is H's handle, h_L host uint8 [k][N] (0/1; k = 0:
 * may be NULL), h_priors host double [N], each in [0, 1). Forms the
 * thresholds thr_J = floor(p_J 2^32) (what qldpc_channel_table(p, 0, 0)
 * yields) and the stacked matrix [H; L] column by column, and uploads them
 * once to the code's device. `code` must outlive the handle. Without a
 * visible device the handle is still made. qldpc_dem_destroy: NULL is
 * accepted.
 *
 * qldpc_dem_sample: shots shot0 .. shot0+batch-1 of the stream `seed`. Column
 * J of shot s fires iff u < thr_J with qldpc_phenom_sample's draw, u =
 * Philox4x32-10(key = seed, counter = (J % 64, (J / 64) / 4, s mod 2^32,
 * s >> 32))[(J / 64) % 4]: on a phenomenological model bit for bit that
 * sampler's fired row, and on any matrix qldpc_channel_sample_vec's errX with
 * (px, py, pz) = (p, 0, 0).
 *   d_det    uint8 [batch][M] (QLDPC_FMT_BYTES) or uint64 [batch][ceil(M/64)]
 *   d_obs    uint64 [batch][ceil(K/64)]   L e mod 2, bit i % 64 of word i / 64,
 *            nothing for K = 0 (may be NULL then)
 *   d_fired  uint64 [batch][ceil(N/64)]   the fired row (NULL: not written)
 * Per shot it writes O(M + K) bits, never the N error bits.
 *
 * qldpc_dem_count: a shot is class 2 (decoder failure) if H ehat != d, else
 * class 1 (logical error) if L ehat != obs, else class 0 (success). It needs
 * no error vector.
 *   d_ehat      uint8 [batch][N] or uint64 [batch][ceil(N/64)] (ehat_format)
 *   d_iters     int32 [batch]
 *   d_counters  int64 [4], added to: failures, logical errors, successes,
 *               sum of iterations
 *   d_class     uint8 [batch]                                (NULL: not written)
 *   d_flips     uint64 [batch][ceil(K/64)]  L ehat ^ obs, as computed for every
 *               class, nothing for K = 0                     (NULL: not written)
 *
 * QLDPC_EINVAL, before any HIP call: a null handle or required buffer, a
 * handle whose code changed, a prior outside [0, 1) or NaN, an unknown
 * format, a negative batch. Limits (QLDPC_EUNSUP, before any launch):
 * ceil(M/64) + ceil(K/64) <= 4096 words (a wave's LDS row; four waves and 128
 * bytes of partial sums per workgroup must fit the device's LDS), N <= 2^24,
 * fewer than 2^31 entries in [H; L]. The tables are read from global memory:
 * no row or column degree is bounded, and the limits lie past every decode
 * kernel's under per-variable priors (m, n, E <= 65535). batch == 0 returns
 * QLDPC_OK. Asynchronous on `stream`: no allocation, copy or synchronisation. */
int qldpc_dem_create(const qldpc_code *code, const uint8_t *h_L, int k, const double *h_priors, qldpc_dem **out);
int qldpc_dem_destroy(qldpc_dem *dem);
int qldpc_dem_sample(const qldpc_dem *dem, uint64_t seed, uint64_t shot0, int64_t batch, void *d_det, int det_format,
                     uint64_t *d_obs, uint64_t *d_fired, void *stream);
int qldpc_dem_count(const qldpc_dem *dem, int64_t batch, const void *d_det, int det_format, const uint64_t *d_obs,
                    const void *d_ehat, int ehat_format, const int32_t *d_iters, int64_t *d_counters,
                    uint8_t *d_class, uint64_t *d_flips, void *stream);

/* The name of the sampler's or the counter's instance for this model
 * ("dem_sample_kernel<16>", "dem_count_kernel<32>": the width of an entry of
 * the column lists, 16 bits while 64 (ceil(M/64) + ceil(K/64)) <= 65536), into
 * buf. kind: QLDPC_DEM_*. Needs no device. Measurement and tests. */
#define QLDPC_DEM_SAMPLE 0
#define QLDPC_DEM_COUNT 1
int qldpc_dem_kernel_name(const qldpc_dem *dem, int kind, char *buf, int len);

/* Kernel timing (HIP events around each decode kernel launch, on the launch
 * stream). Enabled by qldpc_timing_enable(1); qldpc_timing_read returns the
 * summed kernel milliseconds and launch count since the last reset. */
int qldpc_timing_enable(int on);
int qldpc_timing_reset(void);
int qldpc_timing_read(double *total_ms, int64_t *launches);

/* Library options: which kernel family decodes, for tests (every variant is
 * checked against the oracle), A/B experiments and diagnostics. The defaults
 * are the measured best and what the product runs; the library never reads
 * the environment. A change applies from the next launch on, for every
 * schedule. Names (default):
 *   "force_hbm" (0)           every code through the HBM-resident kernel
 *   "flood_generic" (0)       flooding MS through decode_kernel, not ms_flood_kernel
 *   "flood_qc" (1)            flooding MS of a lift-16 QC code with generated tables: the
 *                             register-resident ms_flood_kernel (0: its LDS twin, ms_flood_lds_kernel)
 *   "layered_generic" (0)     layered MS through decode_kernel, not ms_layered_kernel
 *   "ms_lanes_per_check" (0)  layered MS: one lanes-per-check width for every layer (0: per layer)
 *   "bp_wave" (0)             BP through the one-wave decode_kernel, not the team kernels
 *   "bp_lg" (1)               layered BP: the global-table team kernel (0: tables in LDS)
 *   "bp_team_w" (0)           BP team width in waves (0: automatic)
 *   "static_sched" (0)        static half-shot striding instead of the work queue
 *   "waves_per_wg" (0), "wg_per_cu" (0)   occupancy overrides of the wave kernels
 *   "osd_column" (0)          GPU OSD through the exact-REF column kernel only
 *   "osd_tickets" (1)         GPU OSD engine wave placed by per-CU SIMD tickets
 *   "osd_prof" (0)            print per-phase OSD cycles (builds with QLDPC_OSD_TIMING)
 *   "osd_hbm" (0)             GPU OSD through the device-memory kernel at any size (tests)
 *   "logical_tabs" (0)        qldpc_count_logical_ex: logical tables staged in LDS (1), read from
 *                             global memory (2), or chosen by size (0)
 *   "vprior_hbm" (0)          qldpc_decode_*_vprior: what decode_vprior_kernel refuses decodes with the
 *                             HBM-resident hbm_tile_vprior_kernel (with "force_hbm": every call); 0: refused
 * Unknown name: QLDPC_EINVAL. */
int qldpc_set_option(const char *name, int64_t value);
int qldpc_get_option(const char *name, int64_t *value);

#ifdef __cplusplus
}
#endif
#endif /* QLDPC_DECODER_H */

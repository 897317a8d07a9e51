// Shared host-side helpers for libflgp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>
#include "../../include/flgp_hip.h"
#include "worker_pool.h"

namespace flgp {

void set_error(const char *fmt, ...);
int tuning(const char *key, int dflt);

// the current device's multiprocessor count and maximum LDS per block (bytes), asked once per device (core.hip); a figure
// whose query failed is 0
struct DeviceFigures { int cus, lds_per_block; };
DeviceFigures device_figures();

// optional per-launch HIP-event timing (core.hip); work = algorithmic flops or bytes of the launch
int prof_begin(const char *name, hipStream_t st, double work);
void prof_end(int idx, hipStream_t st);
struct ProfScope {
  int idx; hipStream_t st;
  ProfScope(const char *name, hipStream_t s, double work) : idx(prof_begin(name, s, work)), st(s) {}
  ~ProfScope() { prof_end(idx, st); }
};

inline int hip_fail(hipError_t e, const char *what, const char *file, int line) {
  set_error("HIP error %s (%d) in %s at %s:%d", hipGetErrorString(e), (int)e, what, file, line);
  return FLGP_ERR_HIP;
}

#define FLGP_HIP(call)                                                         \
  do {                                                                         \
    hipError_t e_ = (call);                                                    \
    if (e_ != hipSuccess) return ::flgp::hip_fail(e_, #call, __FILE__, __LINE__); \
  } while (0)

#define FLGP_TRY(call)            \
  do {                            \
    int rc_ = (call);             \
    if (rc_ != FLGP_OK) return rc_; \
  } while (0)

#define FLGP_REQUIRE(cond, ...)      \
  do {                               \
    if (!(cond)) {                   \
      ::flgp::set_error(__VA_ARGS__); \
      return FLGP_ERR_INVALID;       \
    }                                \
  } while (0)

inline int ceil_div(long a, long b) { return (int)((a + b - 1) / b); }

// Device memory of the entry points comes from a small cache (core.hip): hipMalloc / hipFree cost 50-500 us each and an
// entry point makes dozens (2.7 ms of a 34 ms call at BASELINE configs[2]); a block that is given back is kept, up to
// `pool_max_mb` (default 16 GB) per process, and handed to the next request of the same size on the same device.  Giving
// back synchronises the device first -- exactly what the hipFree it replaces did -- so nothing in flight can still use
// the block when its next owner writes to it.  Blocks above 4 GB bypass the cache.  flgp_dev_pool_release() empties it.
void *pool_take(int dev, size_t bytes);                 // nullptr: nothing of that size cached
bool pool_give(int dev, void *p, size_t bytes);         // false: not kept (the caller frees)

// RAII device buffer for the host-pointer entry points
struct DevBuf {
  void *p = nullptr;
  bool owned = true;
  size_t cap = 0;       // bytes as allocated (rounded), for the cache
  int dev = -1;
  ~DevBuf() { release(); }
  void release() {
    if (p && owned) {
      bool kept = false;
      if (cap && dev >= 0) {
        // the hipFree this replaces waited for the OWNING device; the caller may be on another one by now (a rank's thread of
        // the multi-GPU entry, a flgp_set_device in between)
        int cur = -1;
        const bool here = hipGetDevice(&cur) == hipSuccess && cur == dev;
        if (here || hipSetDevice(dev) == hipSuccess) {
          (void)hipDeviceSynchronize();
          kept = pool_give(dev, p, cap);
          if (!here && cur >= 0) (void)hipSetDevice(cur);
        }
      }
      if (!kept) (void)hipFree(p);
    }
    p = nullptr; cap = 0; dev = -1;
  }
  void borrow(const void *q) { release(); p = (void *)q; owned = false; }   // the caller's device memory: never freed here
  int alloc(size_t bytes) {
    if (bytes == 0) bytes = 8;
    release();
    owned = true;
    bytes = (bytes + 255) / 256 * 256;
    int d = 0;
    if (hipGetDevice(&d) == hipSuccess && bytes <= ((size_t)4 << 30)) {
      p = pool_take(d, bytes);
      if (p) { cap = bytes; dev = d; return FLGP_OK; }
    }
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) {       // the memory may be parked in the cache under other sizes: empty it and ask once more
      (void)hipGetLastError();
      if (flgp_dev_pool_release() > 0) e = hipMalloc(&p, bytes);
    }
    if (e != hipSuccess) { p = nullptr; set_error("hipMalloc of %zu bytes failed: %s", bytes, hipGetErrorString(e)); return FLGP_ERR_NOMEM; }
    if (bytes <= ((size_t)4 << 30)) { cap = bytes; dev = d; }
    return FLGP_OK;
  }
  template <class T> T *as() { return (T *)p; }
};

inline int check_launch(const char *what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) { set_error("launch of %s failed: %s", what, hipGetErrorString(e)); return FLGP_ERR_HIP; }
  return FLGP_OK;
}

// the host entry points' own stream, destroyed on every way out
struct Stream {
  hipStream_t s = nullptr;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  int create() { FLGP_HIP(hipStreamCreate(&s)); return FLGP_OK; }
};

// The worker pool (worker_pool.h) on the current device.  plan(): the worker count, capped by the free memory where
// bytes_per_worker > 0.  run<Own>(): setup(Own &) makes what a worker owns, item(stream, Own &, i) runs item i on
// it.  A single worker runs on the calling thread and on `st`; several have a host thread and a stream each.
struct DevicePool {
  int dev = 0, workers = 1;
  int plan(int max_parallel, int items, double bytes_per_worker) {
    FLGP_HIP(hipGetDevice(&dev));
    size_t free_b = 0, total_b = 0;
    if (bytes_per_worker > 0.0 && plan_workers(max_parallel, items, 0.0, 0.0) > 1) FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
    workers = plan_workers(max_parallel, items, (double)free_b, bytes_per_worker);
    return FLGP_OK;
  }
  template <class Own, class Setup, class Item>
  PoolFailure run(hipStream_t st, int items, Setup setup, Item item) const {
    struct State { Stream own; hipStream_t st = nullptr; Own a; };     // `a` goes before its stream does
    return run_strided<State>(
        items, workers,
        [&](int, State &S) -> int {
          if (workers == 1) {
            S.st = st;
          } else {
            FLGP_HIP(hipSetDevice(dev));
            FLGP_TRY(S.own.create());
            S.st = S.own.s;
          }
          return setup(S.a);
        },
        [&](State &S, int i) -> int { return item(S.st, S.a, i); }, [] { return std::string(flgp_last_error()); });
  }
};
// how the bandwidth grids report what their pool found
inline int bandwidth_failure(const PoolFailure &f, const double *a2s) {
  if (f.item >= 0) set_error("bandwidth %d (a2=%g): %s", f.item, a2s[f.item], f.message.c_str());
  return f.status;
}

inline int h2d(void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (bytes) FLGP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st));
  return FLGP_OK;
}
inline int d2h(void *dst, const void *src, size_t bytes, hipStream_t st) {
  if (bytes) FLGP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
  return FLGP_OK;
}
// *h = the device int at d_flag once everything queued on `st` has run (synchronises the stream)
inline int read_flag(hipStream_t st, const void *d_flag, int *h) {
  FLGP_HIP(hipMemcpyAsync(h, d_flag, sizeof(int), hipMemcpyDeviceToHost, st));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

inline bool is_range(const int *idx, int cnt) {
  for (int i = 1; i < cnt; ++i)
    if (idx[i] != idx[0] + i) return false;
  return true;
}

// C(i,j) = alpha * sum_k A(i,k) B(k,j) + beta * E(i,j) + gamma * E2(i,j)   (gemm.hip)
int gemm_launch(hipStream_t st, int M, int N, int Kd, double alpha, const double *A, long a_is, long a_ks,
                const double *B, long b_ks, long b_js, double beta, const double *E, long e_is, long e_js,
                double *C, long c_is, long c_js, double *work, size_t work_elems, double gamma,
                const double *E2, struct GemmFusedReduce *fused = nullptr,
                const struct GemmPair *pair = nullptr, int force_split = 0, int *planes_out = nullptr,
                const struct GemmBatch *batch = nullptr);
// The number of split-K planes gemm_launch chooses for this shape and workspace.  `force_split` > 0 makes a launch take
// that number instead (the workspace must hold it): a row block of a product then adds every element's terms in the
// order the whole product does, whatever the block's own tile count would have chosen.  `planes_out` (optional) receives the
// number of planes a launch took.
int gemm_plan_split(int M, int N, int Kd, size_t work_elems);
// `pair`: a second product C2 = alpha A2 B2 of the same shape and strides in the same launch (no E / E2, never split):
// two of the solver's s x b rotations fill the chip where one leaves its fixed costs exposed.
struct GemmPair { const double *A2, *B2; double *C2; };
// `batch`: `count` products of this shape and these element strides in one launch (and one reduction launch when split).
// Problem q reads the device int slots[q] and takes A + slot a_bs, B + slot b_bs, C + slot c_bs, E + slot e_bs and its
// split-K planes at work + slot part_bs (work_elems: the planes of ONE problem); a stride of 0 shares the operand.  No pair,
// E2 or fused reduction.  The tiles, the k ranges and the reduction order of a problem are those of a launch of that
// problem alone with the same split, so with force_split = that launch's gemm_plan_split every problem keeps its bits.
constexpr int GEMM_BATCH_MAX = 32768;     // (the reduction kernel carries the problem in gridDim.y)
// a_slots (optional device list of `count` ints): A of problem q at a_slots[q] a_bs instead, for an operand that belongs to
// something several problems share without sharing the rest (the rows of a pair under many x).
struct GemmBatch { int count; const int *slots; long a_bs, b_bs, c_bs, e_bs, part_bs; const int *a_slots = nullptr; };
int gemm_reduce_square(hipStream_t st, int b, const double *part, int nsplit, double *C, GemmFusedReduce *fused);
// The eigensolver's b x b Gram product out = Xa^T Xb (Xa, Xb: s x b column-major) on its own kernel (rot.hip): split over the
// rows, planes reduced by gemm.hip's reduction kernels (with the fused extras).  false: not this shape, nothing was launched.
int gemm_split_limit(int Kd, int ntiles, int gk, bool tile64);
bool gramk_applicable(int s, int b, const double *Xa, const double *Xb, size_t work_elems);
int gramk_launch(hipStream_t st, int s, int b, const double *Xa, const double *Xb, double *out, double *work, size_t work_elems,
                 GemmFusedReduce *fused);
// The eigensolver's rotation out = alpha X W + beta E on its own kernel (rot.hip): W k-major, WT[k * b + j] = W(k, j)
bool rot_applicable(int s, int b, const double *X, const double *X2, const double *WT, const double *out, const double *out2);
int rot_launch(hipStream_t st, int s, int b, double alpha, const double *X, const double *X2, const double *WT, double beta,
               const double *E, const double *E2, double *out, double *out2);
// Optional extra work for the split-K reduction kernel of a SQUARE product S (M == N, alpha = 1, no E / E2), so that the
// eigensolver's small matrices need no kernels of their own behind the product:
//   mode bit 0: S <- D S D with D = diag(1 / sqrt(S_jj)) (0 where S_jj <= 0), D stored in dinv;
//        bit 1: only the strictly upper triangle (row < column) of S is kept, the rest zero (bit 3: the strictly lower one);
//               rows and columns are the caller's own, for a column-major and a row-major C alike;
//        bit 2: |S - I|_F^2 (after bits 0 / 1) as GEMM_DIST_PARTS partial sums in a fixed order into dist[] (may be host memory).
// `scratch` holds one double per 16 x 16 tile of S, `counter` one int that is zero between launches.  `done` tells the caller
// whether the reduction kernel ran (the product was split) -- if not, S is the plain product and the caller runs its own kernels.
constexpr int GEMM_DIST_PARTS = 32;
struct GemmFusedReduce {
  int mode;
  double *dinv, *dist, *scratch;
  int *counter;
  bool done;
};

// heat-kernel contraction on LDS-resident panels of V (hk.hip); d_vw holds hk_panel_vw_elems(n1, K) doubles
bool hk_panel_applicable(int n0, int n1, int K, long ldh);
bool hk_panel2_applicable(int n0, int n1, int K, long ldh);    // hk2.hip: the same with the k loop unrolled (K in 89..112, 185..208)
int hk2_nks(int K);                                            // hk2.hip: the k steps of its instance for K (it pads K to 4 of them each), 0: none
// the larger of the two layouts for every K: n1 padded to 32 rows x max(K padded to 16, hk2.hip's 4 hk2_nks(K)) columns
size_t hk_panel_vw_elems(int n1, int K);
// Vw(b, k) = exp(-t (1 - values_k)) V1(row(b), k), b-contiguous: d_vw[b + k n1] (gemm.hip; row(b) = d_idx1[b] or row0_1 + b)
int hk_scale_launch(hipStream_t st, const double *d_values, int K, double t, const double *dV1, int ld1, const int *d_idx1,
                    int row0_1, int n1, double *d_vw);
int hk_panel2_launch(hipStream_t st, const double *d_values, int K, double t, const double *V0, long ld0, int n0,
                     const double *dV1, int ld1, const int *d_idx1, int row0_1, int n1, double *dH, long ldh,
                     double *d_vw);
int hk_panel_launch(hipStream_t st, const double *d_values, int K, double t, const double *V0, long ld0, int n0,
                    const double *dV1, int ld1, const int *d_idx1, int row0_1, int n1, double *dH, long ldh,
                    double *d_vw);

// Pipelined copies to the caller's pageable memory through the pinned rings (hostcopy.hip); both synchronise `st`.
// hk_ranges_to_host: H (host, ld n0) = HK of rows [row0_0, row0_0 + n0) of V against rows [row0_1, row0_1 + n1).
// d2h_cols_pipelined: a device matrix (rows x cols, column-major, ld = rows) with column c to H + c * ldh (ldh >= rows: a
// rank's row block of the whole H).
int hk_ranges_to_host(hipStream_t st, const double *d_values, int K, double t, const double *d_vectors, int ldv,
                      int row0_0, int n0, int row0_1, int n1, double *H);
int d2h_cols_pipelined(hipStream_t st, const double *dM, long rows, int cols, double *H, long ldh, int rings_at_least);

// dense algebra of the regression consumers of an EigenPair (gpr.hip)
int chol_solve(hipStream_t st, double *dA, int N, double *dB, int nrhs, int *d_flag);
int gpr_weights(hipStream_t st, const double *d_values, int K, double t, double *d_ls, double *d_l);
int gpr_q(hipStream_t st, const double *dVtV, const double *d_ls, int K, double c, double *dQ);
int gpr_scale(hipStream_t st, const double *dM, const double *d_a, const double *d_b, int rows, int cols, double *d_out);
int gpr_diff(hipStream_t st, const double *dX, const double *dY, double alpha, long count, double *d_out);
int gpr_add_diag(hipStream_t st, double *dA, int N, double c);
int gpr_add_diag_vec(hipStream_t st, double *dA, int N, const double *d_v);
int gpr_rowscale_ld(hipStream_t st, const double *dM, long ldm, const double *d_a, int rows, int cols, double *d_out);
int gpr_zinv(hipStream_t st, const double *d_noise, double sigma, int m, double *d_zinv);
int gpr_scalar_mul(hipStream_t st, const double *d_x, double s, int n, double *d_out);   // out = s x
int gpr_rowquad(hipStream_t st, const double *dV2, long ld2, const double *dW, int mnew, int K, const double *d_l, double c,
                double *d_cov);
int gpr_rowdot(hipStream_t st, const double *dC21, const double *dAl, int mnew, int m, const double *dV2, long ld2, int K,
               const double *d_l, double c, double *d_cov);

// Laplace approximation of the logit GP on the device (gpc.hip)
int chol_blocked(hipStream_t st, double *dA, long lda, int m, int *d_flag);       // flag: first bad pivot + 1
// mode bit 0: L y = b, bit 1: L^T x = y; one workgroup per right-hand side
int chol_trsv(hipStream_t st, const double *dL, long lda, int m, double *dB, long ldb, int nrhs, int mode, const int *d_flag);
int chol_logdet(hipStream_t st, const double *dL, long lda, int m, double *d_out);
int gpc_scale2(hipStream_t st, const double *dM, long ldm, const double *d_a, const double *d_b, int rows, int cols, double *d_out);
int gpc_bmat(hipStream_t st, const double *dC, const double *d_sW, int m, double *dB);      // B = sW C sW + I (m x m)
int gpc_gemv(hipStream_t st, const double *dC, int m, const double *d_x, const double *d_s, double *d_y);   // y = s .* (C x)
// The state of one Newton loop (GPML Alg. 3.1) on an m x m covariance C.  dN = nullptr: the posterior's N = 1 form.
struct GpcNewton {
  DevBuf B, f, fnew, sW, b, a, r, resid, scal, flag;
  int m = 0;
  int alloc(int m_);
  // pi, sqrt(W), b (and resid = Y - pi) from f; B = sW C sW + I factored in place
  int weights(hipStream_t st, const double *dC, const double *dY, const double *dN);
  int run(hipStream_t st, const double *dC, const double *dY, const double *dN, double tol, int max_iter, const char *who,
          int *iters);
  int amll(hipStream_t st, const double *dY, const double *dN, double *out);   // synchronises
  static int pivot_error(int bad, const char *who, int iter);   // iter 0: the factorisation at the final f
};
// The low-rank Newton loop of the logit training objective (m > K) for a chunk of independent problems in the same
// launches (gpc.hip, the loop itself in eigenpair_internal.h: LrBatch).  A problem owns one slot of every buffer below for the whole call; the kernels take a device list `act`
// of A slot numbers (the problems still iterating) and carry its index in the grid, so a step is one launch whatever A is
// and a slot that left the list is not written again.  The strides are doubles between two slots; Y, N, V1 are shared.
// `pair` (nullptr: one pair, V1 shared): a device list with the pair of every SLOT, for a chunk whose problems
// sit on several pairs; slot s then reads its rows at V1 + pair[s] s1 and its eigenvalues at values + pair[s] sk.
struct LrChunk {
  int m, K, slots;
  long sv, sk, sx, sq;                                          // of the m-vectors, the K-vectors, X (m x K) and Q (K x K)
  double *f, *fnew, *sW, *b, *a, *D, *dh, *xs, *c, *g, *Xv;    // m each
  double *u, *l, *ls;                                           // K each; l and ls are the slot's spectrum weights
  double *X, *Q;                                                // Q holds the factor L_Q after lrb_chol
  const double *Y; long ldy; const int *ycol;                   // slot s's responses: Y + ycol[s] ldy (ycol on the device)
  const double *N, *V1; long ld1;
  double sigma;
  int *flag;                                                    // one pivot flag per slot (chol_blocked's)
  double *amll;                                                 // one result per slot
  const int *pair = nullptr; long s1 = 0;                       // the slot's pair and the doubles between two pairs' rows
};
// lrb_weights: l = exp(-t (1 - values)) and ls = l^1/2 for slot s at t = d_ts[s], s < slots (d_pair, or nullptr: LrChunk's
// `pair`, the values of pair p at d_values + p sk).  On the listed slots: lrb_w:
// sW and b from f, Y, N; lrb_d: D = 1 + sigma sW^2, dh = D^-1/2, xs = sW dh; lrb_scale2: X = diag(xs) V1 diag(ls) (V1 of the slot's pair);
// lrb_add_diag: Q += I; lrb_mul: out = a .* x, lrb_axpy: out = x + c z (n elements, a stride per operand, 0 = shared);
// lrb_a: a = b - sW .* (dh .* (g - Xv)).  lrb_step: |f - f_new|_1 in a fixed order and f <- f_new per listed problem,
// d_stat[q] = the norm of act[q] and ((int *)(d_stat + A))[q] = its pivot flag: 12 A bytes for the host.  lrb_chol:
// chol_blocked of every listed Q; lrb_trsv: u <- Q^-1 u per listed slot; lrb_amll, for every slot of the chunk: amll[slot] =
// -0.5 a^T f + sum Y log pi + sum (N - Y) log(1 - pi) - 0.5 sum log D - sum log (L_Q)_kk (the K x K factor).
int lrb_weights(hipStream_t st, const double *d_values, const int *d_pair, int K, const double *d_ts, int slots, long sk,
                double *d_ls, double *d_l);
int lrb_w(hipStream_t st, const LrChunk &c, const int *act, int A);
int lrb_d(hipStream_t st, const LrChunk &c, const int *act, int A);
int lrb_scale2(hipStream_t st, const LrChunk &c, const int *act, int A);
int lrb_add_diag(hipStream_t st, const LrChunk &c, const int *act, int A);
int lrb_mul(hipStream_t st, int n, const double *a, long sa, const double *x, long sx, double *out, long so, const int *act, int A);
int lrb_axpy(hipStream_t st, int n, const double *x, long sx, double c, const double *z, long sz, double *out, long so,
             const int *act, int A);
int lrb_a(hipStream_t st, const LrChunk &c, const int *act, int A);
int lrb_step(hipStream_t st, const LrChunk &c, const int *act, int A, double *d_stat);
int lrb_chol(hipStream_t st, const LrChunk &c, const int *act, int A);
int lrb_trsv(hipStream_t st, const LrChunk &c, const int *act, int A);
// lrb_trsv's q-column form: the q columns of R (K x q per slot at stride sr) <- Q^-1 (.), a workgroup per column
int lrb_trsv_cols(hipStream_t st, const LrChunk &c, const int *act, int A, double *R, long sr, int q);
int lrb_amll(hipStream_t st, const LrChunk &c);
// The predictive rows of the logit posterior for m > K (gpc.hip; the loop is in eigenpair_logit.hip: WsBatch).
// gpc_predict_rows_multi: mean_i = u^T v_i and cov_i = c + |G v_i|^2 for the mnew rows v_i = V(rows_i, 0:K) of the pair, read
// in place (d_idx, or row0 + i when it is nullptr), against J operands [G ; u^T] (G K x K lower triangular, u K) stored
// back to back in d_Gf, gpc_predict_operand_elems(K) doubles each as wsb_predict_prep writes them: the rows are staged once
// and column j of d_mean / d_cov (ldo) depends on operand j alone.  One fused MFMA kernel, for K <= GPC_PREDICT_KMAX on a
// device whose LDS holds 16 rows (gpc_predict_rows_applicable); wider K takes gemm + gpc_rowsumsq_add
// (out[i] = c + |Z(i, :)|^2) in the caller.  gpc_class_indicator: out = (labels == j), a column of the one-vs-rest matrix.
constexpr int GPC_PREDICT_KMAX = 1024;
size_t gpc_predict_operand_elems(int K);
bool gpc_predict_rows_applicable(int K);
int gpc_class_indicator(hipStream_t st, const double *d_labels, int m, int j, double *d_out);
int gpc_predict_rows_multi(hipStream_t st, const double *dV, long ld, const int *d_idx, int row0, int mnew, int K, int J,
                           const double *d_Gf, double c, double *d_mean, double *d_cov, long ldo);
int gpc_rowsumsq_add(hipStream_t st, const double *dZ, long ldz, int rows, int cols, double c, double *d_out);
// The weight-space loop and the predictive operands for a chunk of problems in the same launches (gpc.hip,
// the loop in eigenpair_logit.hip: WsBatch), on LrChunk's slots and lists, beside the lrb_* steps it shares.  On the listed
// slots: wsb_w: sW and b from f and Y with N = 1 (gpc_w_kernel's form without N); wsb_bd: c = b / D; wsb_fnew:
// f_new = g + sigma (b - sW^2 g) / D; wsb_scale_cols: M(i, j) *= ls(j) on the K x K matrix at Q's stride;
// wsb_predict_prep: the operand [G ; u^T] of (dG at Q's stride, u) into operand s of d_Gf.  wsb_tri_inverse: tri_inverse of the
// factor in Q for every slot 0 .. A-1 (`all` lists them), dX at Q's stride, dT 64 x K per slot at stride st_, the split
// planes of a slot at part + slot sp (pe doubles each, at least wsb_tri_inverse_planes(K, we)); `we` is the workspace whose
// plan an unbatched tri_inverse would take.
int wsb_w(hipStream_t st, const LrChunk &c, const int *act, int A);
int wsb_bd(hipStream_t st, const LrChunk &c, const int *act, int A);
int wsb_fnew(hipStream_t st, const LrChunk &c, const int *act, int A);
int wsb_scale_cols(hipStream_t st, const LrChunk &c, const int *act, int A, double *dM);
int wsb_predict_prep(hipStream_t st, const LrChunk &c, const int *act, int A, const double *dG, double *d_Gf);
size_t wsb_tri_inverse_planes(int K, size_t we);
int wsb_tri_inverse(hipStream_t st, const LrChunk &c, const int *all, int A, double *dX, double *dT, long st_, double *part,
                    size_t pe, long sp, size_t we);
// The rows of the regression posterior for m > K (gpc.hip, beside the kernels above whose staging and row
// sums they share): mean(i, 0:q) = U^T v_i (d_mean column-major at ldo) and cov_i = c + |G v_i|^2, the operand
// Gp = [G ; U^T] ((K + q) x K; U K x q at ld K) written once by gpr_predict_prep into gpr_predict_operand_elems(K, q)
// doubles.  dG == nullptr writes zeros for G; d_cov == nullptr skips the triangle's tiles: the mean rows only.  A mean's
// bits do not depend on either.  For K <= GPC_PREDICT_KMAX and q <= GPR_PREDICT_QMAX on a device whose LDS holds 16 rows
// (gpr_predict_rows_applicable); beyond, the caller takes the GEMM route.
constexpr int GPR_PREDICT_QMAX = 64;
size_t gpr_predict_operand_elems(int K, int q);
bool gpr_predict_rows_applicable(int K, int q);
int gpr_predict_prep(hipStream_t st, int K, int q, const double *dG, const double *dU, double *d_Gf);
int gpr_predict_rows(hipStream_t st, const double *dV, long ld, const int *d_idx, int row0, int mnew, int K, int q,
                     const double *d_Gf, double c, double *d_mean, long ldo, double *d_cov);

// The regression training objectives on the device (gpr_grad.hip).  tri_inverse: X = L^-1 (m x m, upper triangle zeroed)
// for a lower factor of chol_blocked; dT holds 64 x m doubles, `work` (we doubles) bounds the GEMM's k-split.
int tri_inverse(hipStream_t st, const double *dL, long lda, int m, double *dX, long ldx, double *dT, double *work, size_t we,
                const int *d_flag);
int rg_colsumsq(hipStream_t st, const double *dX, long ldx, int rows, int cols, double *d_out);   // out[j] = |X(:, j)|^2
// The pieces of one evaluation (device pointers) and where its value and gradient go: out = [value, grad_0 .. grad_{nx-1}].
// direct (m <= K): d = diag C^-1 (m), s = |columns of L^-1 V|^2 (K).  Woodbury: M = V^T V ("same") or V^T Z^-1 V, Qinv = Q^-1,
// M1 = Q^-1 Ls M (K x K), ls = exp(-t lambda / 2); "different": d = |rows of V Ls L_Q^-T|^2 (m).  Vta = V^T alpha (K x q).
struct RgTerms {
  int m, q, K, direct, different, posterior, grad;
  double sigma, c;            // c = x1 + sigma ("same")
  double prior[5];            // p, q, tau, alpha, beta
  const double *x;            // nx
  const double *Y, *alpha;    // m x q
  const double *logdet;       // sum log(L_ii + 1e-9) of the factor
  const double *values, *ls;
  const double *Vta, *d, *s, *M, *Qinv, *M1;
  double *out;
};
int rg_assemble(hipStream_t st, const RgTerms &T);
// The Woodbury route (m > K) of the same objective for a chunk of problems in the same launches (the steps in
// eigenpair_regression.hip: RgBatch).  Problem s of the chunk owns slot s of every buffer below and the kernels carry the slot in
// gridDim.y (rgb_assemble: one workgroup per slot), so a step is one launch whatever the chunk holds.  The strides are
// doubles between two slots.  What belongs to a pair and not to a problem (its eigenvalues, its gathered rows V and, for
// "same", M0 = V^T V) is stored once per distinct pair and found through pair[s] (on the device).  Y is shared.
struct RgbChunk {
  int m, q, K, nx, different, posterior, grad;
  double sigma, prior[5];
  long sv, sk, skq, smq, sq, sx, sxn;      // of an m-vector, a K-vector, K x q, m x q, K x K, m x K and x (nx)
  const int *pair;
  const double *values, *V, *M0;          // per pair at sk, sx (ld m) and sq
  const double *Y;
  double *x, *c, *ci;                      // x per slot; c[s] = x1 + sigma or 1, ci[s] = gpr_diff's factor (1 / c or 1)
  double *ls;                              // K: exp(-t lambda / 2) + 0.0 at t = x[0]
  double *alpha, *Tq;                      // m x q
  double *R, *Vta;                         // K x q
  double *M, *Q, *Li, *Qinv, *LsM, *M1;    // K x K; M is written for "different" only ("same" reads M0)
  double *d;                               // m
  double *ZV, *P;                          // m x K, "different" only
  double *logdet;                          // one per slot
  int *flag;                               // one pivot flag per slot (chol_blocked's)
  double *out;                             // slots x (1 + nx) doubles [value, grad], then one int per slot: its flag
};
// Each is its gpr_* / rg_* namesake on every slot, expression for expression.  rgb_weights: ls from values[pair[s]] at
// x[s][0]; rgb_q: Q from M (or M0[pair[s]]), ls and c[s]; rgb_scale: out = diag(a) M diag(b) (a, b optional; `list`
// optional: M of slot s at list[s] sm); rgb_diff: out = f[s] (X - Z); rgb_zinv: d = 1 / (x[1..m] + sigma);
// rgb_rowscale: out(i, j) = a(i) M(i, j), M at ldm; rgb_rowsumsq: out[i] = |X(i, :)|^2, k ascending.  rgb_assemble: the
// log-determinant of the factor in Q (chol_logdet's sum), then rg_assemble's value and gradient of the slot into out.
int rgb_weights(hipStream_t st, const RgbChunk &c, int slots);
int rgb_q(hipStream_t st, const RgbChunk &c, int slots);
int rgb_scale(hipStream_t st, int slots, int rows, int cols, const double *M, long sm, const int *list, const double *a, long sa,
              const double *b, long sb, double *out, long so);
int rgb_diff(hipStream_t st, int slots, long count, const double *X, long sx, const double *Z, long sz, const double *f,
             double *out, long so);
int rgb_zinv(hipStream_t st, const RgbChunk &c, int slots);
int rgb_rowscale(hipStream_t st, int slots, int rows, int cols, const double *M, long ldm, long sm, const int *list,
                 const double *a, long sa, double *out, long so);
int rgb_rowsumsq(hipStream_t st, int slots, const double *X, long sx, long ldx, int rows, int cols, double *out, long so);
int rgb_assemble(hipStream_t st, const RgbChunk &c, int slots);

// The Polya-Gamma Gibbs sampler (pg.hip; its random-number layout is documented there).  pg_stream_base: the base of
// stream `stream` under `seed`, as flgp_amd/synth.py's _stream_base.
unsigned long long pg_stream_base(unsigned long long seed, unsigned long long stream);
int pg_draw_launch(hipStream_t st, const double *d_b, const double *d_c, long n, unsigned long long base, double *d_out);
int pg_normals(hipStream_t st, unsigned long long seed, int sweep, int K, int m, double *d_out);   // K + 2m normals
int pg_f0r(hipStream_t st, int m, const double *Vz, const double *z2, double ss, const double *z3, const double *kappa,
           const double *omega, double *f0, double *r, double *sw);
int pg_dvec(hipStream_t st, int m, const double *omega, double sigma, double *sw, double *dh, double *a);
int pg_mul(hipStream_t st, int m, const double *a, const double *x, const double *b, double *out);
int pg_axpy3(hipStream_t st, int m, const double *x, const double *y, double c, const double *z, double *out);
int pg_trmv(hipStream_t st, const double *dL, long lda, int m, const double *z, double *y, const int *d_flag);
int pg_pi(hipStream_t st, long n, const double *mean, double sigma_nv, const long *ptr, const int *list, const double *w,
          double *pi, long ld, double *y);
int pg_argmax(hipStream_t st, long n, int J, const double *probs, double *labels);
int pg_init(hipStream_t st, int m, const double *Y, double *kappa, double *omega, double *f);
// The Woodbury sweep (m > K) for a chunk of chains in the same launches (pg.hip, the sweep itself in
// eigenpair_pg.hip: PgBatch).  A chain owns slot s of every buffer below for the whole chunk and the kernels carry the slot in
// gridDim.y, so a step is one launch whatever the chunk holds.  sv and sz are the doubles between two slots of an
// m-vector and of z; Y is shared, chain s reading column ycol[s] and drawing from seed[s] (both on the device).  The K x K
// pieces (X, Q, u, l, ls, the pivot flags) are LrChunk's, on the lrb_* kernels.
struct PgChunk {
  int m, K, slots;
  long sv, sz;
  double *kappa, *omega, *f, *f0, *r, *sw, *x, *t1, *t2, *dh, *a;   // m each
  double *z;                                                         // z1 (K), z2 (m), z3 (m) of the sweep
  const double *Y; long ldy; const int *ycol;
  const unsigned long long *seed;
  double sigma;
};
// Each is its pg_* namesake on every slot, expression for expression: pgb_init (column ycol[s] of Y), pgb_normals (the three
// stream bases of (seed[s], sweep) made on the device), pgb_f0r (Vz = t2), pgb_dvec, pgb_draw (omega ~ PG(1, f) on stream
// 4 sweep + 3 of seed[s]); pgb_wb_out: out = sw .* dh .* (t1 - t2); pgb_axpy3: out = x + y + c z, a missing term left out
// (the operands at stride sv); pgb_pi: column s of pi and y (n x slots at ldo) from the slot's mean (stride smean) and
// its w = x (stride sv) over the shared match list.
int pgb_init(hipStream_t st, const PgChunk &c);
int pgb_normals(hipStream_t st, const PgChunk &c, int sweep);
int pgb_f0r(hipStream_t st, const PgChunk &c, double ss);
int pgb_dvec(hipStream_t st, const PgChunk &c);
int pgb_wb_out(hipStream_t st, const PgChunk &c, double *out);
int pgb_axpy3(hipStream_t st, const PgChunk &c, const double *x, const double *y, double cz, const double *z, double *out);
int pgb_draw(hipStream_t st, const PgChunk &c, int sweep);
int pgb_pi(hipStream_t st, long n, int slots, const double *mean, long smean, double sigma_nv, const long *ptr, const int *list,
           const double *w, long sw, double *pi, double *y, long ldo);

// The multinomial label check of the host entries (nll.hip): v[i] an integer in [0, J), as "<who>: <name>[i]=.. is not a
// class label in 0 .. J-1"; with all_named also max(v) + 1 == J, under negative_log_likelihood's message.
int check_class_labels(const char *who, const char *name, const double *v, long n, int J, bool all_named);

// host wait for a stream that polls an event instead of sleeping in hipStreamSynchronize (eig.hip)
hipError_t stream_wait(hipStream_t st);

// Register-resident LAE kernels (lae_reg*.hip).  Returns FLGP_LAE_REG_NONE when no kernel of the family
// is built for (r, d) and the caller falls through to the LDS kernels of lae.hip.
#define FLGP_LAE_REG_NONE 1
int launch_lae_reg(hipStream_t st, const double *dX, int n, int ldx, int d, const double *dUt, int dpad, int r,
                   const int *d_knn, int ldk, int *d_ei, double *d_ev);

}  // namespace flgp

// device-resident EigenPair (include/flgp_hip.h): made in capi.hip, consumed there (H, copied out by hostcopy.hip) and in eigenpair*.hip
struct flgp_eigenpair {
  flgp::DevBuf values, vectors;   // K, n x K column-major
  int n = 0, K = 0, device = 0;
};

// fitted spectrum model (include/flgp_hip.h): made in capi.hip (the fit), consumed in model.hip (the extension)
struct flgp_spectrum_model {
  flgp::DevBuf Ut, uu;                              // the k-NN / LAE panel of the anchors
  flgp::DevBuf V, eig, values;                      // s x K (ld s), K (the solver's), K (as the pair's)
  flgp::DevBuf colsum_gl, colsum_spectrum, sizes;   // s each; colsum_gl unset for "rw", sizes unless cluster-normalized
  int n_fit = 0, d = 0, s = 0, r = 0, K = 0, kernel_se = 0, gl = 0, root = 0, device = 0;
  double epsilon = 0.0;
};
namespace flgp {
// FLGP_ERR_INVALID with the host entries' message where d_x holds a non-finite value (capi.hip; synchronises `st`)
int check_finite_on_device(hipStream_t st, const double *d_x, long count, const char *who);
// out(a, k) = V(idx[a], k) into a matrix of leading dimension ldo (gemm.hip)
int gather_rows_ld(hipStream_t st, const double *dV, int ld, const int *d_idx, int n0, int K, double *d_out, int ldo);
// The model's row chain up to the weights (model.hip): k-NN -> LAE / SE weights -> flgp_dev_extend_scale for rows [0, nb) of
// dX (ldx) into W.ell_idx / W.ell_val (nb x r); asynchronous on `st`.  ModelRowWork: its workspaces for a block of at most
// `rows` rows.  model_block_rows: the block of the knob model_extend_block.
struct ModelRowWork {
  DevBuf knn_idx, knn_dist, ell_idx, ell_val;
  int alloc(const flgp_spectrum_model *m, int rows);
};
int model_block_rows();
int model_rows(hipStream_t st, const flgp_spectrum_model *m, ModelRowWork &W, const double *dX, int nb, int ldx);
// The rows an entry serves: the caller's device rows (dX, ldx), or host rows X (column-major, ld n) with the block they are
// staged in, which lives as long as the entry's other workspaces do.
struct RowPoints {
  const double *dX = nullptr;
  int ldx = 0;
  const double *X = nullptr;
  DevBuf staged;
};
// Rows [0, n) of `points` (d columns) in blocks of B: block(i0, rows, nb, ld) on the nb device rows from i0, asynchronous on
// `st`.  Host rows are uploaded and screened ("points") block by block.  Stops at the first failure and returns its code; the
// final synchronise and the copies down are the caller's.
template <class Block>
int for_row_blocks(hipStream_t st, RowPoints &points, int n, int d, int B, Block block) {
  if (points.X) FLGP_TRY(points.staged.alloc(sizeof(double) * (size_t)std::min(B, n) * d));
  for (long i0 = 0; i0 < n; i0 += B) {
    const int nb = (int)std::min<long>(B, n - i0);
    if (!points.X) {
      FLGP_TRY(block(i0, points.dX + i0, nb, points.ldx));
      continue;
    }
    double *rows = points.staged.as<double>();
    FLGP_HIP(hipMemcpy2DAsync(rows, sizeof(double) * (size_t)nb, points.X + i0, sizeof(double) * (size_t)n, sizeof(double) * (size_t)nb, d,
                              hipMemcpyHostToDevice, st));
    FLGP_TRY(check_finite_on_device(st, rows, (long)nb * d, "points"));
    FLGP_TRY(block(i0, rows, nb, nb));
  }
  return FLGP_OK;
}
// The way out of an entry that queued row blocks: `st` is idle before the workspaces die, whether rc is a failure or not
inline int settle(hipStream_t st, int rc) {
  if (rc != FLGP_OK) { (void)hipStreamSynchronize(st); return rc; }
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}
// The update of a regression handle (predictor_update.hip).  predictor_gram: flgp_dev_predictor_gram's two
// launches on d_part (predictor_gram_bytes(n, K, q) bytes); `first` starts every element from 0.0, otherwise from S as it stands,
// so the chunk partials of successive row blocks -- each a multiple of predictor_gram_chunk() rows -- form one ascending chain.
// predictor_update_system: M = I + S[:K, :K] (ld K) and R = S[:K, K:] (ld K) of S at ld K + q.
size_t predictor_gram_bytes(long n, int K, int q);
int predictor_gram_chunk();
int predictor_gram(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P, long ldp, int K,
                   int q, const double *d_w, const double *d_Y, long ldy, double *d_S, long lds, double *d_part, bool first);
int predictor_update_system(hipStream_t st, const double *d_S, int K, int q, double *d_M, double *d_R);
// The greedy design loop (predictor_design.hip): flgp_dev_predictor_design_rows' launches on d_work
// (predictor_design_bytes(n, r, s, K, B) bytes), shapes already checked; asynchronous on `st`.
size_t predictor_design_bytes(int n, int r, int s, int K, int B);
int predictor_design_rows(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P, long ldp,
                          int s, int K, double d, int B, int *d_picks, double *d_gain, double *d_score, void *d_work);
// B(j, k) = Vs(j, k) q_k, q_k = scale / sigma_k (0 where sigma_k = 0): the anchor side of flgp_dev_hk_rows (sparse.hip)
int hk_rows_b(hipStream_t st, const double *dVs, int ldv, int s, const double *d_eig, int K, double scale, double *dB);
// The trained operands of the posteriors for the predictor (predictor.hip), by the weight-space route whatever m is, on
// the launches of the m > K bodies of the entries they mirror (eigenpair_regression.hip, eigenpair_logit.hip).  *_check: that entry's refusals under `who`,
// before any device work.  The sink receives the operands of problems [p0, p0 + S) while they are valid: G (K x K, ld K)
// of problem p0 + a at G + a sg and U (K x q, ld K) at U + a su, with var_i = c + |G u_i|^2 and mean_i = U^T u_i; it queues
// its work on `st`.  Both synchronise `st` and return the mirrored entry's verdict.
using OperandSink = std::function<int(int p0, int S, const double *G, long sg, const double *U, long su)>;
int regression_operands_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int q,
                              double t, const double *noise, int n_noise, double sigma);
int regression_operands(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y,
                        int q, double t, const double *noise, int n_noise, double sigma, const OperandSink &sink);
int logit_operands_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol,
                         const int *col, const double *ts, int B, double sigma11, double sigma22, int max_iter);
int logit_operands(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y,
                   int ncol, const int *col, const double *ts, int B, double sigma11, double tol, int max_iter, int max_parallel,
                   int *its, const OperandSink &sink);
// The trained state of B Polya-Gamma chains (f-22): flgp_eigenpair_pg_predict_batch's chains on its own launches, both
// sides of m = K.  pg_operands_check: that entry's refusals that concern the chains alone, in its order and wording;
// `also`: a further variance screened with sigma (the entry's sigma_nv).  The sink receives u = L (V1^T w) (K doubles) of
// chain p0 + a at U + a su while it is valid -- the latent mean of a row with eigenvector entries v is v . u -- and queues
// its work on the stream it is handed: `st`, or for m <= K the stream of the pool worker that ran the chain (from that
// worker's thread, one chain per call).  omega_out / f_out (m x B or NULL): the chains' final state, the entry's bits.
// Synchronises `st`; a pivot <= 0 gives FLGP_ERR_NOCONV under the entry's "chain b (t=.., seed=..): .." message.
using PgSink = std::function<int(hipStream_t st, int p0, int S, const double *U, long su)>;
int pg_operands_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol,
                      const int *col, const double *ts, const unsigned long long *seeds, int B, double sigma, int n_sample,
                      double also = 0.0);
int pg_operands(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol,
                const int *col, const double *ts, const unsigned long long *seeds, int B, double sigma, int n_sample,
                int max_parallel, double *omega_out, double *f_out, const PgSink &sink);
// The Nystrom predictor's mean-only route on a P of q columns alone (nystrom_predictor.hip; f-22): flgp_dev_nystrom_predictor_rows
// with groups = 1 and no K columns, unchanged in its arithmetic.  The workspace is that entry's, sized by the first.
size_t nystrom_mean_workspace(int n, int s, int q);
int nystrom_mean_rows(hipStream_t st, const double *dX, int n, int ldx, int d, const double *dUt, const double *duu, const double *dU,
                      int ldu, int s, double inv_c, const double *d_w, const double *d_P, long ldp, int q, double *d_mean, long ldm,
                      void *d_work, size_t work_bytes);
// The Nystrom predictor's columns-out route (nystrom_predictor.hip; f-23): out(i, c) = f_i sum_j Z(i, j) P(j, c0 + c), c < nc, with
// Z and f made and stored as the variance route makes them, T = Z P(:, a chunk of columns) one j-ascending chain per element
// (gemm_launch without a workspace; chunks under nystrom_predictor_t_mb) and out = f T.  out n x nc column-major (ldo).
size_t nystrom_cols_workspace(int n, int s, int nc);
int nystrom_cols_rows(hipStream_t st, const double *dX, int n, int ldx, int d, const double *dUt, const double *duu, const double *dU,
                      int ldu, int s, double inv_c, const double *d_w, const double *d_P, long ldp, int c0, int nc, double *d_out,
                      long ldo, void *d_work, size_t work_bytes);
// The draws handle's kernels (predictor_cols.hip; f-23).  draws_normals_fill: xi(k, col) at d_xi[k ncol + col], normal p = k of
// stream (col / S) 2^32 + col % S under seed.  draws_fold: P_draw(j, (g q + c) S + t) = P(j, g (K + q) + K + c) + the k-ascending
// chain of P(j, g (K + q) + k) xi(k, col).  sym_mirror: the strict upper triangle of C (n x n, ldc) takes the lower one's bits.
int draws_normals_fill(hipStream_t st, unsigned long long seed, int K, int S, long ncol, double *d_xi);
int draws_fold(hipStream_t st, const double *d_P, long ldp, int s, int groups, int K, int q, int S, const double *d_xi, double *d_Pd,
               long ldd);
int sym_mirror(hipStream_t st, double *d_C, int n, long ldc);
}  // namespace flgp

struct flgp_nystrom_grid;
namespace flgp {
// Nystrom extension from a grid's anchor side (nystrom.hip); both synchronise `st`.  d_vectors[i] (extend_all): the n x K
// block of bandwidth i (ldv).
int nystrom_grid_extend(hipStream_t st, const flgp_nystrom_grid *G, int i, const double *dX, int n, int ldx, double *d_vectors,
                        int ldv);
int nystrom_grid_extend_all(hipStream_t st, const flgp_nystrom_grid *G, const double *dX, int n, int ldx,
                            double *const *d_vectors, int ldv);
// "bandwidth %d (a2=%g): <who>: a2 must be positive and finite" for the first of the l bandwidths that is not
int check_bandwidths(const char *who, const double *a2s, int l);
// The steps of the anchor side that the GLGP grid (glgp.hip) shares: see nystrom.hip.  The void ones only launch.
// What nys_self_distances needs beside its result: the partial and whole row sums (rsx is part of the result), the squared
// norms and, for a caller that does not keep one (with_panel), the padded panel of the s points (flgp_dev_anchor_prep)
struct NysScratch {
  DevBuf p1, xx, rsx, Ut, uu;
  int alloc(int s, int dpad, bool with_panel) {
    FLGP_TRY(p1.alloc(sizeof(double) * (size_t)ceil_div(s, 64) * s));
    FLGP_TRY(xx.alloc(sizeof(double) * (size_t)s));
    FLGP_TRY(rsx.alloc(sizeof(double) * (size_t)s));
    if (!with_panel) return FLGP_OK;
    const size_t rows = (size_t)flgp_dev_anchor_rows(s);
    FLGP_TRY(Ut.alloc(sizeof(double) * rows * dpad));
    return uu.alloc(sizeof(double) * rows);
  }
};
int nys_self_distances(hipStream_t st, const double *dU, int s, int ldu, int d, int dpad, const double *Ut, const double *uu,
                       double *D, NysScratch &T);
// W = exp(-D inv_c) (s x s), its first scaling (rs) and second factor (sd), W <- diag(sd) W diag(sd)
void nys_normalised_w(hipStream_t st, const double *D, double *W, int s, double inv_c, double *rs, double *sd);
void nys_colsum(hipStream_t st, const double *M, int s, long ld, double *colsum);
void nys_first_scaling(hipStream_t st, double *W, int s, double *rs, bool have_sums = false);
void nys_second_factor(hipStream_t st, const double *W, int s, double *sd);
void nys_vector_norms(hipStream_t st, double *V, int s, int K, const double *sd, double *nrm);
// For the Nystrom predictor: R(1), the rows per block of the single-bandwidth extension (at most n), and whether the dot
// products of a row block come from the GEMM (the knob nystrom_dot_gemm; always for dpad > 64, which has no register kernel)
int nys_row_block(int s, int K, int n);
bool nys_dots_via_gemm(int dpad);
}  // namespace flgp

// anchor side of the Nystrom bandwidth grid (include/flgp_hip.h): made and consumed in nystrom.hip
struct flgp_nystrom_grid {
  flgp::DevBuf U, Ut, uu;         // the anchors (s x d column-major, ld s) and their padded panel
  flgp::DevBuf values, rsu, eigv; // per bandwidth: K values, s factors 1 / (rs_U + 1e-9), s x K pre-scaled eigenvectors
  std::vector<double> a2s, inv_c; // l bandwidths and 1 / (a2 mean)
  double mean = 0.0;
  int s = 0, d = 0, dpad = 0, l = 0, K = 0, device = 0, workers = 0;
  // bandwidth i's block starts at i * vs / i * rs / i * es doubles: strides rounded up to 256 bytes, so that every
  // block is aligned like an allocation of its own (what the single-bandwidth entry handed to the eigensolver)
  size_t vs = 0, rs = 0, es = 0;
  const double *values_of(int i) const { return (const double *)values.p + (size_t)i * vs; }
  const double *rsu_of(int i) const { return (const double *)rsu.p + (size_t)i * rs; }
  const double *eigv_of(int i) const { return (const double *)eigv.p + (size_t)i * es; }
};

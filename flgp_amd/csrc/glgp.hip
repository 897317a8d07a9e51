// the bandwidth-grid spectra of the fit_gl_* drivers (GLGP; reference src/Fit.cpp:361-449, the same block at
// :1166-1260 and :1340-1415), for n <= FLGP_SMAX with W dense on the device.  Per bandwidth a2:
//   dense:   Z = exp(-D / (a2 mean(D)))
//   sparse:  each point keeps its r nearest of all n rows (itself included), mean = mean of the kept distances,
//            Z = (Z_kept + Z_kept^T) / 2
//   rs = rowsum(Z) + 1e-9;  A = Z / (rs rs^T);  sd = 1/sqrt(rowsum(A) + 1e-9);  W = sd A sd
//   (values, V) = top-K eigenpairs of W;  V <- sd V, columns rescaled to norm sqrt(n) (+1e-9 guard)
// The dense route IS the anchor side of the Nystrom grid with U = X_all, up to the last kernel: both go through
// nys_self_distances and nys_normalised_w (nystrom.hip).  The sparsified W is indefinite (eigenvalues down to about -0.33) and the eigensolver damps [0, cut], so the sparse
// route hands it W' = (W + I) / 2, whose spectrum lies in (0, 1), and returns 2 lambda' - 1.
// The kept set of point i is never stored as an index list: it is {j : D < tau_i or (D == tau_i and j <= jcut_i)} with
// tau_i the r-th smallest of the list and jcut_i the column of the last kept one among those equal to it (ties go to the
// lower column: the reference's ascending scan with strict <).
#include "common.h"
#include <climits>
#include <cmath>
#include <memory>
#include <mutex>

namespace flgp {

// order-preserving key of a double; -0.0 and +0.0 share one
__device__ __forceinline__ unsigned long long glgp_key(double v) {
  if (v == 0.0) v = 0.0;
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double glgp_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// One workgroup per point: radix select of the r-th smallest key of its list (column i of Dt) in six passes over the
// list, digits of 11 bits (the last one 9) counted in LDS; then wave 0 walks the list once more in column order for jcut
// and the sum of the kept entries, added one by one in ascending column order.  Exact for any 1 <= r <= n.
constexpr int GLGP_BINS = 2048;
__global__ __launch_bounds__(256) void glgp_select_kernel(const double *__restrict__ Dt, int n, long ldd, int r,
                                                          double *__restrict__ tau, int *__restrict__ jcut,
                                                          double *__restrict__ sum) {
  __shared__ unsigned hist[GLGP_BINS];
  __shared__ unsigned part[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_k;
  const double *col = Dt + (size_t)blockIdx.x * ldd;
  const int t = threadIdx.x;
  unsigned long long prefix = 0;
  unsigned k = (unsigned)r;                  // rank (from 1) among the entries that share the prefix
  for (int p = 0; p < 6; ++p) {
    const int sh = p < 5 ? 53 - 11 * p : 0;
    const unsigned dmask = p < 5 ? 0x7ffu : 0x1ffu;
    const unsigned long long himask = p == 0 ? 0ull : ~0ull << (p < 5 ? sh + 11 : 9);
    for (int b = t; b < GLGP_BINS; b += 256) hist[b] = 0;
    __syncthreads();
    for (int j = t; j < n; j += 256) {
      const unsigned long long key = glgp_key(col[j]);
      if ((key & himask) == prefix) atomicAdd(&hist[(unsigned)(key >> sh) & dmask], 1u);
    }
    __syncthreads();
    unsigned c = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) c += hist[8 * t + q];
    part[t] = c;
    __syncthreads();
    if (t == 0) {
      unsigned acc = 0;
      int g = 0;
      for (; g < 255; ++g) {
        if (acc + part[g] >= k) break;
        acc += part[g];
      }
      int b = 8 * g;
      for (; b < 8 * g + 7; ++b) {
        if (acc + hist[b] >= k) break;
        acc += hist[b];
      }
      s_prefix = prefix | ((unsigned long long)b << sh);
      s_k = k - acc;
    }
    __syncthreads();
    prefix = s_prefix;
    k = s_k;
  }
  if (t >= 64) return;
  // k: how many of the entries equal to tau are kept
  const double tv = glgp_unkey(prefix);
  unsigned eq_seen = 0;
  int jc = -1;
  double acc = 0.0;
  const unsigned long long below = (1ull << t) - 1ull;
  for (int base = 0; base < n; base += 256) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + u * 64 + t;
      v[u] = j < n ? col[j] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = base + u * 64 + t;
      const bool in = j < n;
      const bool eq = in && v[u] == tv;
      const unsigned long long eqm = __ballot(eq);
      const unsigned ord = eq_seen + (unsigned)__popcll(eqm & below) + 1u;
      const bool keep = (in && v[u] < tv) || (eq && ord <= k);
      const unsigned long long hit = __ballot(eq && ord == k);
      if (hit) jc = base + u * 64 + (__ffsll((long long)hit) - 1);
      eq_seen += (unsigned)__popcll(eqm);
      unsigned long long km = __ballot(keep);
      while (km) {
        const int lane = __ffsll((long long)km) - 1;
        acc += __shfl(v[u], lane);
        km &= km - 1ull;
      }
    }
  }
  if (t == 0) {
    tau[blockIdx.x] = tv;
    jcut[blockIdx.x] = jc;
    sum[blockIdx.x] = acc;
  }
}

// Z(i, j) = (a(i, j) + a(j, i)) / 2 with a(i, j) = exp(-Dt(j, i) inv_c) where point i keeps j, else 0.  The workgroup of the
// tile pair (I, J), I <= J, reads tile (J of list I) and tile (I of list J) through LDS, both along the lists, and writes
// Z's tiles (I, J) and (J, I), both along Z's columns; the addition commutes, so Z is symmetric to the bit.
constexpr int GLGP_T = 32;
__global__ __launch_bounds__(256) void glgp_similarity_kernel(const double *__restrict__ Dt, int n, long ldd,
                                                              const double *__restrict__ tau, const int *__restrict__ jcut,
                                                              double inv_c, double *__restrict__ Z, long ldz) {
  const int I = blockIdx.x, J = blockIdx.y;
  if (I > J) return;
  __shared__ double sA[GLGP_T][GLGP_T + 1], sB[GLGP_T][GLGP_T + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = I * GLGP_T, j0 = J * GLGP_T;
  for (int q = ty; q < GLGP_T; q += 8) {
    {   // sA[il][jl] = a(i0 + il, j0 + jl)
      const int i = i0 + q, j = j0 + tx;
      double a = 0.0;
      if (i < n && j < n) {
        const double D = Dt[(size_t)i * ldd + j], tv = tau[i];
        if (D < tv || (D == tv && j <= jcut[i])) a = exp(-D * inv_c);
      }
      sA[q][tx] = a;
    }
    {   // sB[jl][il] = a(j0 + jl, i0 + il)
      const int j = j0 + q, i = i0 + tx;
      double b = 0.0;
      if (i < n && j < n) {
        const double D = Dt[(size_t)j * ldd + i], tv = tau[j];
        if (D < tv || (D == tv && i <= jcut[j])) b = exp(-D * inv_c);
      }
      sB[q][tx] = b;
    }
  }
  __syncthreads();
  for (int q = ty; q < GLGP_T; q += 8) {
    {
      const int i = i0 + tx, j = j0 + q;
      if (i < n && j < n) Z[(size_t)j * ldz + i] = 0.5 * (sA[tx][q] + sB[q][tx]);
    }
    if (I != J) {
      const int j = j0 + tx, i = i0 + q;
      if (i < n && j < n) Z[(size_t)i * ldz + j] = 0.5 * (sB[tx][q] + sA[q][tx]);
    }
  }
}

// out(j, i) = in(i, j): the Nystrom distance kernel writes D(x, j) = fma(-2, dot, |x|^2) + |u_j|^2 down column j; point i's
// list wants |x_i|^2 inside the fma along its own column
__global__ __launch_bounds__(256) void glgp_transpose_kernel(const double *__restrict__ in, int n, double *__restrict__ out,
                                                             long ldo) {
  __shared__ double tile[GLGP_T][GLGP_T + 1];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = blockIdx.x * GLGP_T, j0 = blockIdx.y * GLGP_T;
  for (int q = ty; q < GLGP_T; q += 8) {
    const int i = i0 + tx, j = j0 + q;
    tile[q][tx] = (i < n && j < n) ? in[(size_t)j * n + i] : 0.0;
  }
  __syncthreads();
  for (int q = ty; q < GLGP_T; q += 8) {
    const int j = j0 + tx, i = i0 + q;
    if (i < n && j < n) out[(size_t)i * ldo + j] = tile[tx][q];
  }
}

// the second scaling of the sparse route with the shift: M(i, j) <- ((M(i, j) a[i]) a[j] + [i == j]) / 2
__global__ void glgp_symscale_shift_kernel(double *__restrict__ M, int s, const double *__restrict__ a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)s * s) return;
  const int i = (int)(e % s), j = (int)(e / s);
  M[e] = 0.5 * ((M[e] * a[i]) * a[j] + (i == j ? 1.0 : 0.0));
}

// V(j, k) <- V(j, k) sqrt(n) / (nrm_k + 1e-9); with `shifted`, val_k <- 2 val_k - 1
__global__ void glgp_vfinal_kernel(double *__restrict__ V, int n, int K, const double *__restrict__ nrm, double sqrt_n,
                                   double *__restrict__ val, int shifted) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)n * K) return;
  const int k = (int)(e / n);
  V[e] = V[e] * (sqrt_n / (nrm[k] + 1e-9));
  if (shifted && e < K) val[e] = 2.0 * val[e] - 1.0;
}

}  // namespace flgp

using namespace flgp;

extern "C" int flgp_glgp_neighbours(double threshold, int n) {
  const double x = std::floor(threshold * (double)n + 0.5);
  if (!(x >= 3.0)) return 3;
  if (x >= 2147483647.0) return INT_MAX;
  return (int)x;
}

extern "C" int flgp_dev_glgp_select(void *stream, const double *dDt, int n, int ldd, int r, double *d_tau, int *d_jcut,
                                    double *d_sum) {
  FLGP_REQUIRE(dDt && d_tau && d_jcut && d_sum, "glgp_select: null pointer");
  FLGP_REQUIRE(n >= 1 && ldd >= n, "glgp_select: need n >= 1 and ldd >= n (n=%d, ldd=%d)", n, ldd);
  FLGP_REQUIRE(r >= 1 && r <= n, "glgp_select: need 1 <= r <= n (r=%d, n=%d)", r, n);
  hipLaunchKernelGGL(glgp_select_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, dDt, n, (long)ldd, r, d_tau, d_jcut, d_sum);
  return check_launch("glgp_select_kernel");
}

extern "C" int flgp_dev_glgp_similarity(void *stream, const double *dDt, int n, int ldd, const double *d_tau, const int *d_jcut,
                                        double inv_c, double *dZ, int ldz, double *d_rowsum) {
  FLGP_REQUIRE(dDt && d_tau && d_jcut && dZ, "glgp_similarity: null pointer");
  FLGP_REQUIRE(n >= 1 && ldd >= n && ldz >= n, "glgp_similarity: need n >= 1 and leading dimensions >= n (n=%d, ldd=%d, ldz=%d)",
               n, ldd, ldz);
  const int T = ceil_div(n, GLGP_T);
  hipLaunchKernelGGL(glgp_similarity_kernel, dim3(T, T), dim3(256), 0, (hipStream_t)stream, dDt, n, (long)ldd, d_tau, d_jcut,
                     inv_c, dZ, (long)ldz);
  if (d_rowsum) nys_colsum((hipStream_t)stream, dZ, n, ldz, d_rowsum);     // Z is symmetric: column sums are row sums
  return check_launch("glgp_similarity_kernel");
}

namespace {

// what every entry refuses before any device work
int glgp_check(const void *X, int n, int d, int K, const double *a2s, int l, int sparse, double threshold, bool any_out) {
  FLGP_REQUIRE(X && a2s, "glgp: null pointer");
  FLGP_REQUIRE(any_out, "glgp: nothing to return (values, vectors and pairs are all NULL)");
  FLGP_REQUIRE(n >= 3 && n <= FLGP_SMAX, "glgp: need 3 <= n <= %d, W is held dense (n=%d)", FLGP_SMAX, n);
  FLGP_REQUIRE(d >= 1 && flgp_dev_anchor_dpad(d) > 0, "glgp: kernels are built for 1 <= d <= %d (got %d)", FLGP_DMAX, d);
  FLGP_REQUIRE(K >= 1 && K <= n, "glgp: need 1 <= K <= n (K=%d, n=%d)", K, n);
  FLGP_REQUIRE(l >= 1, "glgp: need at least one bandwidth (l=%d)", l);
  FLGP_TRY(check_bandwidths("glgp", a2s, l));
  if (sparse) {
    FLGP_REQUIRE(std::isfinite(threshold) && threshold > 0.0, "glgp: threshold must be positive and finite (got %g)", threshold);
    FLGP_REQUIRE(threshold * (double)n + 0.5 < (double)n + 1.0, "glgp: threshold %g asks for more than n = %d neighbours", threshold, n);
  }
  return FLGP_OK;
}

// what one worker owns: W, the eigensolver's workspace and results, three vectors
struct GlgpWorker {
  DevBuf W, work, rs, sd, nrm, val, V;
  size_t wb = 0;
  int alloc(int n, int K) {
    wb = flgp_dev_eig_workspace(n, K);
    FLGP_TRY(W.alloc(sizeof(double) * (size_t)n * n));
    FLGP_TRY(work.alloc(wb));
    FLGP_TRY(rs.alloc(sizeof(double) * (size_t)n));
    FLGP_TRY(sd.alloc(sizeof(double) * (size_t)n));
    FLGP_TRY(nrm.alloc(sizeof(double) * (size_t)K));
    FLGP_TRY(val.alloc(sizeof(double) * (size_t)K));
    return V.alloc(sizeof(double) * (size_t)n * K);
  }
};

// outer iterations of each bandwidth's eigensolve in the last grid of this process (-1: not solved), for the timing script
std::mutex g_iters_mu;
std::vector<int> g_iters;

struct GlgpGrid {
  int n, K, sparse;
  const double *D;        // dense: D(x, j) as the Nystrom grid holds it; sparse: Dt, column i = point i's list
  const double *tau; const int *jcut;
  std::vector<double> inv_c;
};

// bandwidth i into out_val (K, or NULL) and out_vec (n x K at ld n, or NULL); synchronises `st`
int glgp_bandwidth(hipStream_t st, const GlgpGrid &G, int i, GlgpWorker &A, double *out_val, double *out_vec) {
  const int n = G.n, K = G.K;
  double *W = A.W.as<double>(), *rs = A.rs.as<double>(), *sd = A.sd.as<double>(), *nrm = A.nrm.as<double>();
  double *val = A.val.as<double>(), *V = A.V.as<double>();
  int info[4] = {-1, -1, -1, -1};
  {
    ProfScope prof("glgp_similarity_norm", st, 8.0 * n * (double)n);
    if (G.sparse) {      // Z and its row sums; W' = (sd A sd + I) / 2
      FLGP_TRY(flgp_dev_glgp_similarity(st, G.D, n, n, G.tau, G.jcut, G.inv_c[i], W, n, rs));
      nys_first_scaling(st, W, n, rs, true);
      nys_second_factor(st, W, n, sd);
      hipLaunchKernelGGL(glgp_symscale_shift_kernel, dim3(ceil_div((long)n * n, 256)), dim3(256), 0, st, W, n, sd);
    } else {             // the Nystrom grid's anchor side
      nys_normalised_w(st, G.D, W, n, G.inv_c[i], rs, sd);
    }
    FLGP_TRY(check_launch("glgp W"));
  }
  {
    ProfScope prof("glgp_eigensolve", st, 0.0);
    const int rc = flgp_dev_eig_topk(st, W, n, n, K, 0.0, val, V, n, A.work.p, A.wb, info);
    {
      std::lock_guard<std::mutex> lk(g_iters_mu);
      if (i < (int)g_iters.size()) g_iters[i] = rc == FLGP_OK ? info[0] : -1;
    }
    FLGP_TRY(rc);
  }
  {
    ProfScope prof("glgp_final", st, 16.0 * n * (double)K);
    nys_vector_norms(st, V, n, K, sd, nrm);
    hipLaunchKernelGGL(glgp_vfinal_kernel, dim3(ceil_div((long)n * K, 256)), dim3(256), 0, st, V, n, K, nrm, std::sqrt((double)n),
                       val, G.sparse);
    FLGP_TRY(check_launch("glgp V"));
  }
  if (out_val) FLGP_HIP(hipMemcpyAsync(out_val, val, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, st));
  if (out_vec) FLGP_HIP(hipMemcpyAsync(out_vec, V, sizeof(double) * (size_t)n * K, hipMemcpyDeviceToDevice, st));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// Dt (ldd): column i = point i's list, D = fma(-2, dot_ij, |x_i|^2) + |x_j|^2 at row j -- the transpose of what the Nystrom
// distance step leaves in D0 (n x n)
int glgp_lists(hipStream_t st, const double *dX, int n, int ldx, int d, int dpad, NysScratch &S, double *D0, double *Dt, long ldd) {
  FLGP_TRY(nys_self_distances(st, dX, n, ldx, d, dpad, S.Ut.as<double>(), S.uu.as<double>(), D0, S));
  const int T = ceil_div(n, GLGP_T);
  hipLaunchKernelGGL(glgp_transpose_kernel, dim3(T, T), dim3(256), 0, st, D0, n, Dt, ldd);
  return check_launch("glgp_transpose_kernel");
}

// the grid on device points; out_val[i] / out_vec[i]: where bandwidth i goes (either array may be NULL)
int glgp_grid(hipStream_t st, const double *dX, int n, int ldx, int d, int K, const double *a2s, int l, int sparse,
              double threshold, int max_parallel, double *const *out_val, double *const *out_vec, double *mean_out, int *r_out) {
  const int dpad = flgp_dev_anchor_dpad(d);
  const int r = sparse ? flgp_glgp_neighbours(threshold, n) : n;
  FLGP_REQUIRE(r <= n, "glgp: threshold %g asks for %d of n = %d neighbours", threshold, r, n);
  if (ldx == n) FLGP_TRY(check_finite_on_device(st, dX, (long)n * d, "glgp"));
  else for (int k = 0; k < d; ++k) FLGP_TRY(check_finite_on_device(st, dX + (size_t)k * ldx, n, "glgp"));
  GlgpGrid G;
  G.n = n; G.K = K; G.sparse = sparse ? 1 : 0; G.tau = nullptr; G.jcut = nullptr;
  DevBuf D, tau, jcut;
  double total = 0.0;
  {
    NysScratch T;
    DevBuf D0;
    FLGP_TRY(T.alloc(n, dpad, true));
    FLGP_TRY(D.alloc(sizeof(double) * (size_t)n * n));
    FLGP_TRY(flgp_dev_anchor_prep(st, dX, n, ldx, d, T.Ut.as<double>(), T.uu.as<double>()));
    std::vector<double> hrow(n);
    if (!sparse) {      // D and mean(D) as the Nystrom grid takes them (src/Fit.cpp:383,394)
      ProfScope prof("glgp_distances", st, 8.0 * n * (double)n);
      FLGP_TRY(nys_self_distances(st, dX, n, ldx, d, dpad, T.Ut.as<double>(), T.uu.as<double>(), D.as<double>(), T));
      FLGP_TRY(d2h(hrow.data(), T.rsx.p, sizeof(double) * n, st));
    } else {            // the lists, their r-th smallest and the kept sums (:396-428)
      FLGP_TRY(D0.alloc(sizeof(double) * (size_t)n * n));
      FLGP_TRY(tau.alloc(sizeof(double) * (size_t)n));
      FLGP_TRY(jcut.alloc(sizeof(int) * (size_t)n));
      {
        ProfScope prof("glgp_distances", st, 24.0 * n * (double)n);
        FLGP_TRY(glgp_lists(st, dX, n, ldx, d, dpad, T, D0.as<double>(), D.as<double>(), n));
      }
      ProfScope prof("glgp_select", st, 8.0 * n * (double)n);
      FLGP_TRY(flgp_dev_glgp_select(st, D.as<double>(), n, n, r, tau.as<double>(), jcut.as<int>(), T.rsx.as<double>()));
      FLGP_TRY(d2h(hrow.data(), T.rsx.p, sizeof(double) * n, st));
      G.tau = tau.as<double>(); G.jcut = jcut.as<int>();
    }
    FLGP_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < n; ++i) total += hrow[i];
  }
  G.D = D.as<double>();
  const double mean = total / ((double)n * (double)r);
  FLGP_REQUIRE(mean > 0.0 && std::isfinite(mean), "glgp: the points coincide (mean squared distance %g)", mean);
  if (mean_out) *mean_out = mean;
  if (r_out) *r_out = r;
  G.inv_c.resize(l);
  for (int i = 0; i < l; ++i) G.inv_c[i] = 1.0 / (a2s[i] * mean);
  {
    std::lock_guard<std::mutex> lk(g_iters_mu);
    g_iters.assign(l, -1);
  }
  // ---- workers as the Nystrom grid's (worker_pool.h); one owns W, the eigensolver's workspace and an n x K block
  DevicePool pool;
  FLGP_TRY(pool.plan(max_parallel, l,
                     8.0 * n * (double)n + (double)flgp_dev_eig_workspace(n, K) + 8.0 * (2.0 * n + 2.0 * K + (double)n * K)));
  return bandwidth_failure(pool.run<GlgpWorker>(
                               st, l, [&](GlgpWorker &A) { return A.alloc(n, K); },
                               [&](hipStream_t ws, GlgpWorker &A, int i) {
                                 return glgp_bandwidth(ws, G, i, A, out_val ? out_val[i] : nullptr, out_vec ? out_vec[i] : nullptr);
                               }),
                           a2s);
}

}  // namespace

extern "C" int flgp_glgp_last_iterations(int *iters, int l) {
  FLGP_REQUIRE(iters && l >= 0, "glgp_last_iterations: null pointer");
  std::lock_guard<std::mutex> lk(g_iters_mu);
  for (int i = 0; i < l; ++i) iters[i] = i < (int)g_iters.size() ? g_iters[i] : -1;
  return FLGP_OK;
}

// the lists the sparse route selects from, for the tests: dDt column-major n x n (ldd)
extern "C" int flgp_dev_glgp_distances(void *stream, const double *dX, int n, int ldx, int d, double *dDt, int ldd) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(dX && dDt, "glgp_distances: null pointer");
  FLGP_REQUIRE(n >= 1 && n <= FLGP_SMAX && ldx >= n && ldd >= n, "glgp_distances: need 1 <= n <= %d and leading dimensions >= n (n=%d)",
               FLGP_SMAX, n);
  const int dpad = flgp_dev_anchor_dpad(d);
  FLGP_REQUIRE(d >= 1 && dpad > 0, "glgp_distances: kernels are built for 1 <= d <= %d (got %d)", FLGP_DMAX, d);
  NysScratch T;
  DevBuf D0;
  FLGP_TRY(T.alloc(n, dpad, true));
  FLGP_TRY(D0.alloc(sizeof(double) * (size_t)n * n));
  FLGP_TRY(flgp_dev_anchor_prep(st, dX, n, ldx, d, T.Ut.as<double>(), T.uu.as<double>()));
  FLGP_TRY(glgp_lists(st, dX, n, ldx, d, dpad, T, D0.as<double>(), dDt, ldd));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// dX: n x d column-major (ldx); a2s: host.  d_values: l x K (or NULL); d_vectors: l blocks n x K column-major (or NULL).
extern "C" int flgp_dev_glgp_spectrum_grid(void *stream, const double *dX, int n, int ldx, int d, int K, const double *a2s, int l,
                                           int sparse, double threshold, int max_parallel, double *d_values, double *d_vectors,
                                           double *distances_mean_out, int *r_out) {
  FLGP_TRY(glgp_check(dX, n, d, K, a2s, l, sparse, threshold, d_values || d_vectors));
  FLGP_REQUIRE(ldx >= n, "glgp: leading dimension too small (ldx=%d, n=%d)", ldx, n);
  std::vector<double *> pv(l), pV(l);
  for (int i = 0; i < l; ++i) {
    pv[i] = d_values ? d_values + (size_t)i * K : nullptr;
    pV[i] = d_vectors ? d_vectors + (size_t)i * n * K : nullptr;
  }
  return glgp_grid((hipStream_t)stream, dX, n, ldx, d, K, a2s, l, sparse, threshold, max_parallel, d_values ? pv.data() : nullptr,
                   d_vectors ? pV.data() : nullptr, distances_mean_out, r_out);
}

// X_all: n x d column-major (host).  values: l x K | NULL, vectors: l blocks n x K | NULL, pairs: l handles | NULL.
extern "C" int flgp_glgp_spectrum_grid(const double *X_all, int n, int d, int K, const double *a2s, int l, int sparse,
                                       double threshold, int max_parallel, double *values, double *vectors,
                                       flgp_eigenpair **pairs, double *distances_mean_out, int *r_out) {
  if (pairs && l >= 1 && l <= (1 << 20))
    for (int i = 0; i < l; ++i) pairs[i] = nullptr;
  FLGP_TRY(glgp_check(X_all, n, d, K, a2s, l, sparse, threshold, values || vectors || pairs));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dX;
  FLGP_TRY(dX.alloc(sizeof(double) * (size_t)n * d));
  FLGP_TRY(h2d(dX.p, X_all, sizeof(double) * (size_t)n * d, st.s));
  // the results stay where a pair would hold them; host copies are taken from there
  std::vector<std::unique_ptr<flgp_eigenpair>> eps(l);
  std::vector<double *> pv(l), pV(l);
  for (int i = 0; i < l; ++i) {
    eps[i].reset(new flgp_eigenpair());
    eps[i]->n = n; eps[i]->K = K;
    FLGP_HIP(hipGetDevice(&eps[i]->device));
    FLGP_TRY(eps[i]->values.alloc(sizeof(double) * (size_t)K));
    FLGP_TRY(eps[i]->vectors.alloc(sizeof(double) * (size_t)n * K));
    pv[i] = eps[i]->values.as<double>();
    pV[i] = eps[i]->vectors.as<double>();
  }
  FLGP_TRY(glgp_grid(st.s, dX.as<double>(), n, n, d, K, a2s, l, sparse, threshold, max_parallel, pv.data(), pV.data(),
                     distances_mean_out, r_out));
  for (int i = 0; i < l; ++i) {
    if (values) FLGP_TRY(d2h(values + (size_t)i * K, pv[i], sizeof(double) * (size_t)K, st.s));
    if (vectors) FLGP_TRY(d2h(vectors + (size_t)i * n * K, pV[i], sizeof(double) * (size_t)n * K, st.s));
  }
  FLGP_HIP(hipStreamSynchronize(st.s));
  if (pairs)
    for (int i = 0; i < l; ++i) pairs[i] = eps[i].release();
  return FLGP_OK;
}

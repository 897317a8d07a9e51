// The classification consumers of an EigenPair, on the device: the Laplace approximation of the logit GP.
//   marginal_log_likelihood_logit_la_cpp (reference src/train.cpp:716-760): Newton's method for the posterior mode
//     (GPML Alg. 3.1) with one m x m Cholesky factorisation per iteration, then the approximate marginal likelihood;
//   posterior_distribution_classification (src/Utils.cpp:252-299): the same loop with N = 1, then the predictive mean and
//     variance (Alg. 3.2) in the low-rank form C21 = V2 L V1^T, never forming the m_new x m matrix C21.
// The Newton loop factors an m x m matrix (m = 1000 at BASELINE configs[2]) every iteration, so the factorisation here is
// blocked and right-looking: a 64-column diagonal panel factored in the registers of one wave, the panel column solved
// by a grid of waves, the trailing update through the MFMA GEMM.  gpr.hip's one-workgroup chol_solve stays as it is for
// the regression entries (their bits do not change).  Everything is fixed-order: two calls give the same bits.
// The fused predictive rows of the logit posterior are here too, and beside them the rows of the
// regression posterior (f-13), which share their staging and row sums.
#include "common.h"

namespace flgp {

constexpr int CNB = 64;   // panel width = one wave

__device__ __forceinline__ double readlane_d(double x, int l) {
  const long long v = __double_as_longlong(x);
  const int lo = __builtin_amdgcn_readlane((int)v, l);
  const int hi = __builtin_amdgcn_readlane((int)(v >> 32), l);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}

// Lower Cholesky factor of the diagonal block A(k0:k0+nb, k0:k0+nb) in place, one wave: lane i holds row i of the block
// in registers (rows past nb are padded with the identity), column j's pivot and multipliers are read across lanes with
// readlane.  flag[0] = (global index + 1) of the first pivot that is not positive; a set flag turns later steps off.
// (the steps are written once, for this kernel and the one-wave-per-problem kernel of the batched loop below)
__device__ __forceinline__ void chol_panel_body(double *__restrict__ A, long lda, int m, int k0, int *__restrict__ flag) {
  if (flag[0]) return;
  const int lane = threadIdx.x;
  const int nb = min(CNB, m - k0);
  double r[CNB];
#pragma unroll
  for (int k = 0; k < CNB; ++k) {
    double v = (lane >= nb && k == lane) ? 1.0 : 0.0;
    if (lane < nb && k <= lane) v = A[(size_t)(k0 + k) * lda + k0 + lane];
    r[k] = v;
  }
  int bad = 0;
#pragma unroll
  for (int j = 0; j < CNB; ++j) {
    double d = readlane_d(r[j], j);
    if (!(d > 0.0)) {
      if (!bad) bad = k0 + j + 1;
      d = 1.0;
    }
    const double ljj = __builtin_sqrt(d);
    const double lij = lane > j ? r[j] / ljj : (lane == j ? ljj : r[j]);
    r[j] = lij;
#pragma unroll
    for (int k = j + 1; k < CNB; ++k) {
      const double lkj = readlane_d(lij, k);
      if (lane >= k) r[k] -= lij * lkj;
    }
  }
#pragma unroll
  for (int k = 0; k < CNB; ++k)
    if (lane < nb && k <= lane) A[(size_t)(k0 + k) * lda + k0 + lane] = r[k];
  if (bad && lane == 0) flag[0] = bad;
}
__global__ __launch_bounds__(64) void chol_panel_kernel(double *__restrict__ A, long lda, int m, int k0, int *__restrict__ flag) {
  chol_panel_body(A, lda, m, k0, flag);
}

// Panel column: L21 = A21 L11^-T for the rows below the diagonal block, a thread per row (x L11^T = a by forward
// substitution), L11 in LDS (identity-padded past nb; every lane reads the same element: a broadcast), the row's
// unknowns in LDS as well (a register array of 64 unrolled twice over spills).
__device__ __forceinline__ void chol_trsm_body(double *__restrict__ A, long lda, int m, int k0, const int *__restrict__ flag,
                                               int rowblock) {
  if (flag[0]) return;
  __shared__ double Ls[CNB][CNB];   // Ls[k][j] = L11(j, k)
  __shared__ double xs[CNB][64];    // xs[j][lane] = x_j of this lane's row
  const int tid = threadIdx.x;
  const int nb = min(CNB, m - k0);
  for (int e = tid; e < CNB * CNB; e += 64) {
    const int j = e % CNB, k = e / CNB;
    double v = (j == k) ? 1.0 : 0.0;
    if (j < nb && k <= j) v = A[(size_t)(k0 + k) * lda + k0 + j];
    Ls[k][j] = v;
  }
  __syncthreads();
  const int i = k0 + nb + rowblock * 64 + tid;
  if (i >= m) return;
  for (int j = 0; j < nb; ++j) {
    double acc = A[(size_t)(k0 + j) * lda + i];
    for (int k = 0; k < j; ++k) acc -= xs[k][tid] * Ls[k][j];
    acc = acc / Ls[j][j];
    xs[j][tid] = acc;
    A[(size_t)(k0 + j) * lda + i] = acc;
  }
}
__global__ __launch_bounds__(64) void chol_trsm_kernel(double *__restrict__ A, long lda, int m, int k0, const int *__restrict__ flag) {
  chol_trsm_body(A, lda, m, k0, flag, blockIdx.x);
}

// In-place lower Cholesky factor of the SPD m x m matrix A (column-major, leading dimension lda).  Only the lower triangle
// is read and only the lower triangle of the result is the factor (the trailing GEMM also rewrites the upper one).
int chol_blocked(hipStream_t st, double *dA, long lda, int m, int *d_flag) {
  ProfScope ps("chol_blocked", st, (double)m * m * m / 3.0);
  for (int k0 = 0; k0 < m; k0 += CNB) {
    const int nb = std::min(CNB, m - k0), rem = m - k0 - nb;
    hipLaunchKernelGGL(chol_panel_kernel, dim3(1), dim3(64), 0, st, dA, lda, m, k0, d_flag);
    FLGP_TRY(check_launch("chol_panel_kernel"));
    if (rem <= 0) break;
    hipLaunchKernelGGL(chol_trsm_kernel, dim3(ceil_div(rem, 64)), dim3(64), 0, st, dA, lda, m, k0, d_flag);
    FLGP_TRY(check_launch("chol_trsm_kernel"));
    // A22 <- A22 - L21 L21^T
    const double *L21 = dA + (size_t)k0 * lda + k0 + nb;
    double *A22 = dA + (size_t)(k0 + nb) * lda + k0 + nb;
    FLGP_TRY(gemm_launch(st, rem, rem, nb, -1.0, L21, 1, lda, L21, lda, 1, 1.0, A22, 1, lda, A22, 1, lda, nullptr, 0, 0.0,
                         nullptr));
  }
  return FLGP_OK;
}

// Triangular solves with the factor chol_blocked left in L, one workgroup per right-hand side (column c of B, leading
// dimension ldb), in place: mode bit 0 solves L y = b, bit 1 then L^T x = y.  Blocks of 64 unknowns: the triangle of a
// block is solved by one wave in registers, the rest of the rows by the whole workgroup (forward: an axpy per row,
// backward: a dot product along a column of L per row, reduced in a fixed order).
// (b: the workgroup's right-hand side)
__device__ __forceinline__ void chol_trsv_body(const double *__restrict__ L, long lda, int m, double *__restrict__ b, int mode,
                                               const int *__restrict__ flag) {
  if (flag[0]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ double ys[CNB];
  if (mode & 1) {
    for (int b0 = 0; b0 < m; b0 += CNB) {
      const int nb = min(CNB, m - b0);
      if (wave == 0) {
        double yi = lane < nb ? b[b0 + lane] : 0.0;
#pragma unroll
        for (int j = 0; j < CNB; ++j) {
          if (j < nb) {
            const double yj = readlane_d(yi, j) / L[(size_t)(b0 + j) * lda + b0 + j];
            if (lane == j) yi = yj;
            if (lane > j && lane < nb) yi -= L[(size_t)(b0 + j) * lda + b0 + lane] * yj;
          }
        }
        if (lane < nb) b[b0 + lane] = yi;
        ys[lane] = yi;
      }
      __syncthreads();
      for (int i = b0 + nb + tid; i < m; i += 256) {
        double acc = b[i];
        for (int j = 0; j < nb; ++j) acc -= L[(size_t)(b0 + j) * lda + i] * ys[j];
        b[i] = acc;
      }
      __syncthreads();
    }
  }
  if (mode & 2) {
    for (int b0 = ((m - 1) / CNB) * CNB; b0 >= 0; b0 -= CNB) {
      const int nb = min(CNB, m - b0), e = b0 + nb;
      for (int rr = wave; rr < nb; rr += 4) {
        const double *li = L + (size_t)(b0 + rr) * lda;   // column b0+rr of L = row b0+rr of L^T
        double acc = 0.0;
        for (int k = e + lane; k < m; k += 64) acc += li[k] * b[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) ys[rr] = acc;
      }
      __syncthreads();
      if (wave == 0) {
        double xi = lane < nb ? b[b0 + lane] - ys[lane] : 0.0;
#pragma unroll
        for (int j = CNB - 1; j >= 0; --j) {
          if (j < nb) {
            const double xj = readlane_d(xi, j) / L[(size_t)(b0 + j) * lda + b0 + j];
            if (lane == j) xi = xj;
            if (lane < j) xi -= L[(size_t)(b0 + lane) * lda + b0 + j] * xj;
          }
        }
        if (lane < nb) b[b0 + lane] = xi;
      }
      __syncthreads();
    }
  }
}
__global__ __launch_bounds__(256) void chol_trsv_kernel(const double *__restrict__ L, long lda, int m, double *__restrict__ B,
                                                        long ldb, int mode, const int *__restrict__ flag) {
  chol_trsv_body(L, lda, m, B + (size_t)blockIdx.x * ldb, mode, flag);
}

int chol_trsv(hipStream_t st, const double *dL, long lda, int m, double *dB, long ldb, int nrhs, int mode, const int *d_flag) {
  if (nrhs <= 0) return FLGP_OK;
  hipLaunchKernelGGL(chol_trsv_kernel, dim3(nrhs), dim3(256), 0, st, dL, lda, m, dB, ldb, mode, d_flag);
  return check_launch("chol_trsv_kernel");
}

// sum(log(L_ii + 1e-9)) in a fixed order (one workgroup)
__device__ __forceinline__ double block_sum_1024(double v, double *red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
  for (int off = 512; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  const double s = red[0];
  __syncthreads();
  return s;
}

__global__ __launch_bounds__(1024) void chol_logdet_kernel(const double *__restrict__ L, long lda, int m, double *__restrict__ out) {
  __shared__ double red[1024];
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += 1024) s += log(L[(size_t)i * lda + i] + 1e-9);
  s = block_sum_1024(s, red);
  if (threadIdx.x == 0) out[0] = s;
}

int chol_logdet(hipStream_t st, const double *dL, long lda, int m, double *d_out) {
  hipLaunchKernelGGL(chol_logdet_kernel, dim3(1), dim3(1024), 0, st, dL, lda, m, d_out);
  return check_launch("chol_logdet_kernel");
}

// ---- Newton's method for the posterior mode (GPML Alg. 3.1) ----------------------------------------------------------

// pi = 1 / (1 + exp(-f)); with N (marginal likelihood, src/train.cpp:737-743): W = N pi (1 - pi),
// b = W f + Y (1 - pi) + (N - Y)(-pi); without (posterior, src/Utils.cpp:269-276): W = pi (1 - pi), b = W f + (Y - pi).
// sW = sqrt(W); resid (optional) = Y - pi.
__global__ void gpc_w_kernel(const double *__restrict__ f, const double *__restrict__ Y, const double *__restrict__ N, int m,
                             double *__restrict__ sW, double *__restrict__ b, double *__restrict__ resid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double fi = f[i], yi = Y[i];
  const double pi = 1.0 / (1.0 + exp(-fi));
  double W, bi;
  if (N) {
    const double ni = N[i];
    W = ni * pi * (1.0 - pi);
    bi = W * fi + yi * (1.0 - pi) + (ni - yi) * (-pi);
  } else {
    W = pi * (1.0 - pi);
    bi = W * fi + (yi - pi);
  }
  sW[i] = __builtin_sqrt(W);
  if (b) b[i] = bi;
  if (resid) resid[i] = yi - pi;
}

// B = sW C sW + I   (column-major m x m)
__global__ void gpc_b_kernel(const double *__restrict__ C, const double *__restrict__ sW, int m, double *__restrict__ B) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)m * m) return;
  const int i = (int)(e % m), j = (int)(e / m);
  B[e] = sW[i] * C[e] * sW[j] + (i == j ? 1.0 : 0.0);
}

// y = s .* (C x) (s optional), C m x m column-major: 64 rows per workgroup, the columns split over 16 waves, the 16
// partial sums added in a fixed order
__global__ __launch_bounds__(1024) void gpc_gemv_kernel(const double *__restrict__ C, int m, const double *__restrict__ x,
                                                        const double *__restrict__ s, double *__restrict__ y) {
  __shared__ double part[16][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane;
  const int chunk = (m + 15) / 16, k0 = wave * chunk, k1 = min(m, k0 + chunk);
  double acc = 0.0;
  if (i < m)
    for (int k = k0; k < k1; ++k) acc += C[(size_t)k * m + i] * x[k];
  part[wave][lane] = acc;
  __syncthreads();
  if (wave == 0 && i < m) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += part[w][lane];
    y[i] = s ? s[i] * t : t;
  }
}

// a = b - sW .* r
__global__ void gpc_a_kernel(const double *__restrict__ b, const double *__restrict__ sW, const double *__restrict__ r, int m,
                             double *__restrict__ a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) a[i] = b[i] - sW[i] * r[i];
}

// diff = |f - f_new|_1 (fixed order), then f <- f_new
__global__ __launch_bounds__(1024) void gpc_step_kernel(double *__restrict__ f, const double *__restrict__ fnew, int m,
                                                        double *__restrict__ diff) {
  __shared__ double red[1024];
  double s = 0.0;
  for (int i = threadIdx.x; i < m; i += 1024) {
    const double fn = fnew[i];
    s += __builtin_fabs(f[i] - fn);
    f[i] = fn;
  }
  s = block_sum_1024(s, red);
  if (threadIdx.x == 0) diff[0] = s;
}

// amll = -0.5 sum(a f) + (sum(Y log pi) + sum((N - Y) log(1 - pi))) - sum(log(L_ii + 1e-9))   (src/train.cpp:753-757)
__global__ __launch_bounds__(1024) void gpc_amll_kernel(const double *__restrict__ f, const double *__restrict__ a,
                                                        const double *__restrict__ Y, const double *__restrict__ N,
                                                        const double *__restrict__ L, long lda, int m, double *__restrict__ out) {
  __shared__ double red[1024];
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
  for (int i = threadIdx.x; i < m; i += 1024) {
    const double pi = 1.0 / (1.0 + exp(-f[i]));
    s1 += a[i] * f[i];
    s2 += Y[i] * log(pi);
    s3 += (N[i] - Y[i]) * log(1.0 - pi);
    s4 += log(L[(size_t)i * lda + i] + 1e-9);
  }
  s1 = block_sum_1024(s1, red);
  s2 = block_sum_1024(s2, red);
  s3 = block_sum_1024(s3, red);
  s4 = block_sum_1024(s4, red);
  if (threadIdx.x == 0) {
    double amll = -0.5 * s1;
    amll += s2 + s3;
    amll -= s4;
    out[0] = amll;
  }
}

// out(i, j) = a(i) * M(i, j) * b(j): M rows x cols with leading dimension ldm, out contiguous
__global__ void gpc_scale2_kernel(const double *__restrict__ M, long ldm, const double *__restrict__ a, const double *__restrict__ b,
                                  int rows, int cols, double *__restrict__ out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)rows * cols) return;
  const int i = (int)(e % rows), j = (int)(e / rows);
  out[e] = a[i] * M[(size_t)j * ldm + i] * b[j];
}

int gpc_scale2(hipStream_t st, const double *dM, long ldm, const double *d_a, const double *d_b, int rows, int cols, double *d_out) {
  hipLaunchKernelGGL(gpc_scale2_kernel, dim3(ceil_div((long)rows * cols, 256)), dim3(256), 0, st, dM, ldm, d_a, d_b, rows, cols, d_out);
  return check_launch("gpc_scale2_kernel");
}

int gpc_bmat(hipStream_t st, const double *dC, const double *d_sW, int m, double *dB) {
  hipLaunchKernelGGL(gpc_b_kernel, dim3(ceil_div((long)m * m, 256)), dim3(256), 0, st, dC, d_sW, m, dB);
  return check_launch("gpc_b_kernel");
}

int gpc_gemv(hipStream_t st, const double *dC, int m, const double *d_x, const double *d_s, double *d_y) {
  hipLaunchKernelGGL(gpc_gemv_kernel, dim3(ceil_div(m, 64)), dim3(1024), 0, st, dC, m, d_x, d_s, d_y);
  return check_launch("gpc_gemv_kernel");
}

int GpcNewton::alloc(int m_) {
  m = m_;
  const size_t v = sizeof(double) * (size_t)m;
  FLGP_TRY(B.alloc(v * m));
  FLGP_TRY(f.alloc(v)); FLGP_TRY(fnew.alloc(v)); FLGP_TRY(sW.alloc(v)); FLGP_TRY(b.alloc(v));
  FLGP_TRY(a.alloc(v)); FLGP_TRY(r.alloc(v)); FLGP_TRY(resid.alloc(v));
  FLGP_TRY(scal.alloc(sizeof(double) * 4)); FLGP_TRY(flag.alloc(sizeof(int)));
  return FLGP_OK;
}

int GpcNewton::weights(hipStream_t st, const double *dC, const double *dY, const double *dN) {
  hipLaunchKernelGGL(gpc_w_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, f.as<double>(), dY, dN, m, sW.as<double>(),
                     b.as<double>(), resid.as<double>());
  FLGP_TRY(check_launch("gpc_w_kernel"));
  hipLaunchKernelGGL(gpc_b_kernel, dim3(ceil_div((long)m * m, 256)), dim3(256), 0, st, dC, sW.as<double>(), m, B.as<double>());
  FLGP_TRY(check_launch("gpc_b_kernel"));
  return chol_blocked(st, B.as<double>(), m, m, flag.as<int>());
}

// Alg. 3.1 from f = 0.  The host reads |f - f_new|_1 and the pivot flag back after every iteration (8 + 4 bytes) and
// decides; the loop's state never leaves the device.  Afterwards B holds the factor and a the vector of the LAST
// iteration, f the final mode -- what the reference's final sums use (src/train.cpp:753-757).
int GpcNewton::run(hipStream_t st, const double *dC, const double *dY, const double *dN, double tol, int max_iter,
                   const char *who, int *iters) {
  FLGP_HIP(hipMemsetAsync(f.p, 0, sizeof(double) * (size_t)m, st));
  FLGP_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
  *iters = 0;
  for (int it = 0; it < max_iter; ++it) {
    {
      ProfScope ps("logit_la_newton_iter", st, 0.0);      // the device time of one iteration, without the host's read-back
      FLGP_TRY(weights(st, dC, dY, dN));
      hipLaunchKernelGGL(gpc_gemv_kernel, dim3(ceil_div(m, 64)), dim3(1024), 0, st, dC, m, b.as<double>(), sW.as<double>(), r.as<double>());
      FLGP_TRY(check_launch("gpc_gemv_kernel"));                                                  // sW (C b)
      FLGP_TRY(chol_trsv(st, B.as<double>(), m, m, r.as<double>(), m, 1, 3, flag.as<int>()));      // B^-1 (.)
      hipLaunchKernelGGL(gpc_a_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, b.as<double>(), sW.as<double>(), r.as<double>(), m,
                         a.as<double>());
      FLGP_TRY(check_launch("gpc_a_kernel"));
      hipLaunchKernelGGL(gpc_gemv_kernel, dim3(ceil_div(m, 64)), dim3(1024), 0, st, dC, m, a.as<double>(), (const double *)nullptr,
                         fnew.as<double>());
      FLGP_TRY(check_launch("gpc_gemv_kernel"));                                                  // f_new = C a
      hipLaunchKernelGGL(gpc_step_kernel, dim3(1), dim3(1024), 0, st, f.as<double>(), fnew.as<double>(), m, scal.as<double>());
      FLGP_TRY(check_launch("gpc_step_kernel"));
    }
    double diff = 0.0;
    int bad = 0;
    FLGP_HIP(hipMemcpyAsync(&diff, scal.p, sizeof(double), hipMemcpyDeviceToHost, st));
    FLGP_HIP(hipMemcpyAsync(&bad, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    FLGP_HIP(hipStreamSynchronize(st));
    *iters = it + 1;
    FLGP_TRY(pivot_error(bad, who, it + 1));
    if (diff < tol) break;
  }
  return FLGP_OK;
}

int GpcNewton::pivot_error(int bad, const char *who, int iter) {
  if (!bad) return FLGP_OK;
  if (iter > 0)
    set_error("%s: B = sqrt(W) C sqrt(W) + I is not positive definite (Cholesky pivot %d <= 0 in Newton iteration %d)", who,
              bad - 1, iter);
  else
    set_error("%s: B = sqrt(W) C sqrt(W) + I is not positive definite at the mode (Cholesky pivot %d <= 0)", who, bad - 1);
  return FLGP_ERR_NOCONV;
}

int GpcNewton::amll(hipStream_t st, const double *dY, const double *dN, double *out) {
  hipLaunchKernelGGL(gpc_amll_kernel, dim3(1), dim3(1024), 0, st, f.as<double>(), a.as<double>(), dY, dN, B.as<double>(), (long)m,
                     m, scal.as<double>() + 1);
  FLGP_TRY(check_launch("gpc_amll_kernel"));
  FLGP_HIP(hipMemcpyAsync(out, scal.as<double>() + 1, sizeof(double), hipMemcpyDeviceToHost, st));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// ---- the low-rank Newton loop for a chunk of independent problems (the loop is in eigenpair_internal.h)
// The elementwise steps, the K x K factorisation and the final sums of Alg. 3.1 on C = V1 L V1^T + sigma I (LrBatch,
// eigenpair_internal.h), with the problem in the grid (blockIdx.y, or blockIdx.x where a workgroup takes a whole problem): entry q
// of the device list `act` names the slot whose buffers the workgroups of row q use (LrChunk, common.h).  A workgroup reads
// and writes its own slot only and every sum is in a fixed order, so a slot's bits do not depend on the list.

// the slot's spectrum weights at its t: l = exp(-t (1 - values)), ls = l^1/2

__global__ void lrb_weights_kernel(const double *__restrict__ values, const int *__restrict__ pair, int K,
                                   const double *__restrict__ ts, long sk, double *__restrict__ ls, double *__restrict__ l) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const long s = blockIdx.y;
  const double t = ts[s];
  if (pair) values += (long)pair[s] * sk;                 // the slot's pair (every slot is listed here: s is the slot)
  const double lam = 1.0 - values[k];
  ls[s * sk + k] = exp(-0.5 * t * lam) + 0.0;
  l[s * sk + k] = exp(-t * lam);
}

// pi = logistic(f), W = N pi (1 - pi): sW = W^1/2, b = W f + (Y - N pi), the latter as Y (1 - pi) - (N - Y) pi
__global__ void lrb_w_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long s = act[blockIdx.y], o = s * c.sv + i;
  const double fi = c.f[o], yi = c.Y[(size_t)c.ycol[s] * c.ldy + i];
  const double pi = 1.0 / (1.0 + exp(-fi));
  const double ni = c.N[i];
  const double W = ni * pi * (1.0 - pi);
  const double bi = W * fi + yi * (1.0 - pi) + (ni - yi) * (-pi);
  c.sW[o] = __builtin_sqrt(W);
  c.b[o] = bi;
}

// W = sW^2: D = 1 + sigma W, dh = D^-1/2, xs = sW dh (the row scaling of X)
__global__ void lrb_d_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long o = (long)act[blockIdx.y] * c.sv + i;
  const double s = c.sW[o], d = 1.0 + c.sigma * (s * s), h = 1.0 / __builtin_sqrt(d);
  c.D[o] = d; c.dh[o] = h; c.xs[o] = s * h;
}

// X = diag(xs) V1 diag(ls), V1 the shared one or that of the SLOT's pair (c.pair is indexed by the slot, not by the
// position in `act`: the two part as soon as a slot has left the list)
__global__ void lrb_scale2_kernel(LrChunk c, const int *__restrict__ act) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)c.m * c.K) return;
  const long s = act[blockIdx.y];
  const int i = (int)(e % c.m), j = (int)(e / c.m);
  const double *V1 = c.pair ? c.V1 + (long)c.pair[s] * c.s1 : c.V1;
  c.X[s * c.sx + e] = c.xs[s * c.sv + i] * V1[(size_t)j * c.ld1 + i] * c.ls[s * c.sk + j];
}

// Q(i, i) += 1
__global__ void lrb_add_diag_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < c.K) c.Q[(long)act[blockIdx.y] * c.sq + (size_t)i * c.K + i] += 1.0;
}

// out = a .* x; a stride of 0 shares the vector
__global__ void lrb_mul_kernel(int n, const double *__restrict__ a, long sa, const double *__restrict__ x, long sx,
                               double *__restrict__ out, long so, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long s = act[blockIdx.y];
  out[s * so + i] = a[s * sa + i] * x[s * sx + i];
}

// out = x + c z
__global__ void lrb_axpy_kernel(int n, const double *__restrict__ x, long sx, double c, const double *__restrict__ z, long sz,
                                double *__restrict__ out, long so, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long s = act[blockIdx.y];
  double v = x[s * sx + i];
  v = v + c * z[s * sz + i];
  out[s * so + i] = v;
}

// a = b - sW .* r with r = B^-1 (sW .* c) = dh .* (g - Xv), g = dh .* sW .* c, Xv = X Q^-1 X^T g
__global__ void lrb_a_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long o = (long)act[blockIdx.y] * c.sv + i;
  c.a[o] = c.b[o] - c.sW[o] * (c.dh[o] * (c.g[o] - c.Xv[o]));
}

// One workgroup per problem: stat[q] = |f - f_new|_1 in a fixed order, f <- f_new, and behind the A norms the A pivot
// flags of the same problems, so that the host reads both in one copy
__global__ __launch_bounds__(1024) void lrb_step_kernel(LrChunk c, const int *__restrict__ act, int A, double *__restrict__ stat) {
  __shared__ double red[1024];
  const long s = act[blockIdx.x];
  double *f = c.f + s * c.sv;
  const double *fnew = c.fnew + s * c.sv;
  double sum = 0.0;
  for (int i = threadIdx.x; i < c.m; i += 1024) {
    const double fn = fnew[i];
    sum += __builtin_fabs(f[i] - fn);
    f[i] = fn;
  }
  sum = block_sum_1024(sum, red);
  if (threadIdx.x == 0) {
    stat[blockIdx.x] = sum;
    ((int *)(stat + A))[blockIdx.x] = c.flag[s];
  }
}

// the panel and the row-block steps of chol_blocked on the slot's Q
__global__ __launch_bounds__(64) void lrb_chol_panel_kernel(LrChunk c, const int *__restrict__ act, int k0) {
  const long s = act[blockIdx.x];
  chol_panel_body(c.Q + s * c.sq, c.K, c.K, k0, c.flag + s);
}
__global__ __launch_bounds__(64) void lrb_chol_trsm_kernel(LrChunk c, const int *__restrict__ act, int k0) {
  const long s = act[blockIdx.y];
  chol_trsm_body(c.Q + s * c.sq, c.K, c.K, k0, c.flag + s, blockIdx.x);
}
// u <- Q^-1 u with the slot's factor, one workgroup per problem
__global__ __launch_bounds__(256) void lrb_trsv_kernel(LrChunk c, const int *__restrict__ act) {
  const long s = act[blockIdx.x];
  chol_trsv_body(c.Q + s * c.sq, c.K, c.K, c.u + s * c.sk, 3, c.flag + s);
}
// The final sums of every slot of the chunk (no list: a problem that left the loop kept its f, a, D and L_Q), one workgroup
// per slot: amll = -0.5 sum(a f) + (sum(Y log pi) + sum((N - Y) log(1 - pi))) - 0.5 sum(log D_i) - sum(log (L_Q)_kk).
// log det B = log det D + log det Q exactly (no 1e-9 on the pivots: the one departure from gpc_amll_kernel,
// include/flgp_hip.h).
__global__ __launch_bounds__(1024) void lrb_amll_kernel(LrChunk c) {
  __shared__ double red[1024];
  const long s = blockIdx.x;
  const double *__restrict__ f = c.f + s * c.sv, *__restrict__ a = c.a + s * c.sv, *__restrict__ D = c.D + s * c.sv;
  const double *__restrict__ Y = c.Y + (size_t)c.ycol[s] * c.ldy, *__restrict__ N = c.N, *__restrict__ LQ = c.Q + s * c.sq;
  const int K = c.K;
  double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0, s5 = 0.0;
  for (int i = threadIdx.x; i < c.m; i += 1024) {
    const double pi = 1.0 / (1.0 + exp(-f[i]));
    s1 += a[i] * f[i];
    s2 += Y[i] * log(pi);
    s3 += (N[i] - Y[i]) * log(1.0 - pi);
    s4 += log(D[i]);
  }
  for (int k = threadIdx.x; k < K; k += 1024) s5 += log(LQ[(size_t)k * K + k]);
  s1 = block_sum_1024(s1, red);
  s2 = block_sum_1024(s2, red);
  s3 = block_sum_1024(s3, red);
  s4 = block_sum_1024(s4, red);
  s5 = block_sum_1024(s5, red);
  if (threadIdx.x == 0) {
    double amll = -0.5 * s1;
    amll += s2 + s3;
    amll -= 0.5 * s4;
    amll -= s5;
    c.amll[s] = amll;
  }
}

int lrb_weights(hipStream_t st, const double *d_values, const int *d_pair, int K, const double *d_ts, int slots, long sk,
                double *d_ls, double *d_l) {
  hipLaunchKernelGGL(lrb_weights_kernel, dim3(ceil_div(K, 256), slots), dim3(256), 0, st, d_values, d_pair, K, d_ts, sk, d_ls,
                     d_l);
  return check_launch("lrb_weights_kernel");
}
int lrb_w(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(lrb_w_kernel, dim3(ceil_div(c.m, 256), A), dim3(256), 0, st, c, act);
  return check_launch("lrb_w_kernel");
}
int lrb_d(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(lrb_d_kernel, dim3(ceil_div(c.m, 256), A), dim3(256), 0, st, c, act);
  return check_launch("lrb_d_kernel");
}
int lrb_scale2(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(lrb_scale2_kernel, dim3(ceil_div((long)c.m * c.K, 256), A), dim3(256), 0, st, c, act);
  return check_launch("lrb_scale2_kernel");
}
int lrb_add_diag(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(lrb_add_diag_kernel, dim3(ceil_div(c.K, 256), A), dim3(256), 0, st, c, act);
  return check_launch("lrb_add_diag_kernel");
}
int lrb_mul(hipStream_t st, int n, const double *a, long sa, const double *x, long sx, double *out, long so, const int *act, int A) {
  hipLaunchKernelGGL(lrb_mul_kernel, dim3(ceil_div(n, 256), A), dim3(256), 0, st, n, a, sa, x, sx, out, so, act);
  return check_launch("lrb_mul_kernel");
}
int lrb_axpy(hipStream_t st, int n, const double *x, long sx, double c, const double *z, long sz, double *out, long so,
             const int *act, int A) {
  hipLaunchKernelGGL(lrb_axpy_kernel, dim3(ceil_div(n, 256), A), dim3(256), 0, st, n, x, sx, c, z, sz, out, so, act);
  return check_launch("lrb_axpy_kernel");
}
int lrb_a(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(lrb_a_kernel, dim3(ceil_div(c.m, 256), A), dim3(256), 0, st, c, act);
  return check_launch("lrb_a_kernel");
}
int lrb_step(hipStream_t st, const LrChunk &c, const int *act, int A, double *d_stat) {
  hipLaunchKernelGGL(lrb_step_kernel, dim3(A), dim3(1024), 0, st, c, act, A, d_stat);
  return check_launch("lrb_step_kernel");
}
// Q = L_Q L_Q^T in place for every listed slot: chol_blocked's panels in its order, one launch per step whatever A is
int lrb_chol(hipStream_t st, const LrChunk &c, const int *act, int A) {
  ProfScope ps("chol_blocked_batch", st, (double)A * c.K * c.K * c.K / 3.0);
  const int m = c.K;
  const long lda = c.K;
  for (int k0 = 0; k0 < m; k0 += CNB) {
    const int nb = std::min(CNB, m - k0), rem = m - k0 - nb;
    hipLaunchKernelGGL(lrb_chol_panel_kernel, dim3(A), dim3(64), 0, st, c, act, k0);
    FLGP_TRY(check_launch("lrb_chol_panel_kernel"));
    if (rem <= 0) break;
    hipLaunchKernelGGL(lrb_chol_trsm_kernel, dim3(ceil_div(rem, 64), A), dim3(64), 0, st, c, act, k0);
    FLGP_TRY(check_launch("lrb_chol_trsm_kernel"));
    const double *L21 = c.Q + (size_t)k0 * lda + k0 + nb;
    double *A22 = c.Q + (size_t)(k0 + nb) * lda + k0 + nb;
    const GemmBatch gb{A, act, c.sq, c.sq, c.sq, c.sq, 0};
    FLGP_TRY(gemm_launch(st, rem, rem, nb, -1.0, L21, 1, lda, L21, lda, 1, 1.0, A22, 1, lda, A22, 1, lda, nullptr, 0, 0.0,
                         nullptr, nullptr, nullptr, 0, nullptr, &gb));
  }
  return FLGP_OK;
}
int lrb_trsv(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(lrb_trsv_kernel, dim3(A), dim3(256), 0, st, c, act);
  return check_launch("lrb_trsv_kernel");
}
// column blockIdx.x of the slot's K x q right-hand sides: chol_trsv's workgroup per column on the slot's factor
__global__ __launch_bounds__(256) void lrb_trsv_cols_kernel(LrChunk c, const int *__restrict__ act, double *__restrict__ R, long sr) {
  const long s = act[blockIdx.y];
  chol_trsv_body(c.Q + s * c.sq, c.K, c.K, R + s * sr + (size_t)blockIdx.x * c.K, 3, c.flag + s);
}
int lrb_trsv_cols(hipStream_t st, const LrChunk &c, const int *act, int A, double *R, long sr, int q) {
  hipLaunchKernelGGL(lrb_trsv_cols_kernel, dim3(q, A), dim3(256), 0, st, c, act, R, sr);
  return check_launch("lrb_trsv_cols_kernel");
}
int lrb_amll(hipStream_t st, const LrChunk &c) {
  hipLaunchKernelGGL(lrb_amll_kernel, dim3(c.slots), dim3(1024), 0, st, c);
  return check_launch("lrb_amll_kernel");
}

// ---- the one-vs-rest indicator and the fused predictive rows of the logit posterior (m > K) ------------------

// out = (labels == j): column j of the one-vs-rest indicator matrix, never stored as a matrix
__global__ void gpc_class_indicator_kernel(const double *__restrict__ labels, int m, double j, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = labels[i] == j ? 1.0 : 0.0;
}

int gpc_class_indicator(hipStream_t st, const double *d_labels, int m, int j, double *d_out) {
  hipLaunchKernelGGL(gpc_class_indicator_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, d_labels, m, (double)j, d_out);
  return check_launch("gpc_class_indicator_kernel");
}

// The predictive operand Gp = [G ; u^T] ((K + 1) x K: G = L_Q^-1 L^1/2 lower triangular at ld K, u = L^1/2 beta) in the
// order the kernel below loads it (wsb_predict_prep_kernel writes it): Gf[(jt * nks + ks) * 64 + lane] =
// Gp(16 jt + (lane & 15), 4 ks + (lane >> 4)), the A fragment of one v_mfma_f64_16x16x4_f64, zero past row K and past
// column K - 1.  A wave's fragment is 512 contiguous bytes and the k steps of a j-tile follow each other.

typedef double gd4 __attribute__((ext_vector_type(4)));

constexpr int PR_WAVES = 8;                  // waves per workgroup of gpc_predict_rows_multi_kernel
constexpr int PR_THREADS = 64 * PR_WAVES;
// LDS row stride (doubles) of a block of R rows: 16 (mod 32), so that the two k of a 32-lane group of ds_read_b64 fall
// into different halves of the 64 banks
__host__ __device__ constexpr int pr_stride(int R) { return R == 16 ? 16 : R + 16; }

// mean_i = z_K, cov_i = c + sum_{j < K} z_j^2 with z = Gp v_i, for the rows v_i = V(rows_i, 0:K) of the pair read in place
// (rows_i = idx[i], or row0 + i when idx is nullptr; V column-major at ld).  A workgroup stages R = 16 RT rows in LDS
// (vs[k][r], zero past K and past mnew), then its waves split the j-tiles of 16 outputs: D(16 j x 16 rows) +=
// A(16 j x 4 k) B(4 k x 16 rows), A streamed from Gf (L2), B from LDS.  Tile jt runs the k steps below 4 (jt + 1) only
// (Gp's first K rows are lower triangular); the last tile, which holds u, runs all nks.  The tiles go to the waves in
// descending cost, back and forth over the waves.  C/D: lane l holds rows j = (l >> 4) + 4 reg of new row l & 15, so a
// lane squares and adds its four results (reg ascending), the four lane groups meet through two xor exchanges
// ((g0 + g1) + (g2 + g3) on every lane) and the tiles of a row are added in ascending jt by one thread: the bits of a
// row depend on that row and Gp alone -- not on mnew, the grid, the row's position or its neighbours.
// The three steps are written once, for the kernel below and the regression posterior's (gpr_predict_rows_kernel).

// vs[k][r] = V(rows_{base + r}, k) for the block's R rows, zero past K and past mnew
template <int RT>
__device__ __forceinline__ void pr_stage(const double *__restrict__ V, long ld, const int *__restrict__ idx, int row0, int mnew,
                                         int K, int nks, long base, double *__restrict__ vs) {
  constexpr int R = 16 * RT, RS = pr_stride(R), KSTEP = PR_THREADS / R;
  const int tid = threadIdx.x;
  // every load is unconditional (row and k clamped into the block's live part) so that four are in flight per thread;
  // the zero padding is applied on the way into LDS
  const int r = tid % R;
  const long i = base + r;
  const bool live = i < mnew;
  const long ic = live ? i : (long)mnew - 1;
  const double *src = V + (idx ? (long)idx[ic] : (long)row0 + ic);
  for (int k0 = tid / R; k0 < 4 * nks; k0 += 4 * KSTEP) {
    double v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = src[(size_t)min(k0 + u * KSTEP, K - 1) * ld];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * KSTEP;
      if (k < 4 * nks) vs[(size_t)k * RS + r] = (live && k < K) ? v[u] : 0.0;
    }
  }
}

// the j-tiles of one operand Gf against the staged rows: ts[jt][r] = the tile's sum of squares, mean[base + r] = z_K
template <int RT>
__device__ __forceinline__ void pr_tiles(const double *__restrict__ Gf, const double *__restrict__ vs, double *__restrict__ ts,
                                         int K, int nks, int njt, long base, int mnew, double *__restrict__ mean) {
  constexpr int R = 16 * RT, RS = pr_stride(R);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int jlast = njt - 1, qK = (K & 15) >> 2, gK = K & 3;      // z_K: tile jlast, lane group gK, register qK
  for (int round = 0; round * PR_WAVES < njt; ++round) {
    const int d = round * PR_WAVES + ((round & 1) ? PR_WAVES - 1 - wave : wave);
    if (d >= njt) continue;
    const int jt = jlast - d;
    const int steps = jt == jlast ? nks : min(4 * (jt + 1), nks);
    const double *A = Gf + (size_t)jt * nks * 64 + lane;
    const double *B = vs + (size_t)g * RS + col;
    gd4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = gd4{0.0, 0.0, 0.0, 0.0};
    // four A fragments ahead of the four being multiplied (the loads clamped into the tile, the steps guarded)
    double a[4], an[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = A[(size_t)min(u, steps - 1) * 64];
    for (int ks = 0; ks < steps; ks += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) an[u] = A[(size_t)min(ks + 4 + u, steps - 1) * 64];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ks + u < steps) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
            acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], B[(size_t)(ks + u) * 4 * RS + rt * 16], acc[rt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = an[u];
    }
    const int j0 = 16 * jt + g;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const gd4 z = acc[rt];
      double s = j0 < K ? z.x * z.x : 0.0;
      s += j0 + 4 < K ? z.y * z.y : 0.0;
      s += j0 + 8 < K ? z.z * z.z : 0.0;
      s += j0 + 12 < K ? z.w * z.w : 0.0;
      s += __shfl_xor(s, 16, 64);
      s += __shfl_xor(s, 32, 64);
      if (g == 0) ts[(size_t)jt * R + rt * 16 + col] = s;
      if (jt == jlast && g == gK) {
        const long i = base + rt * 16 + col;
        const double zK = qK == 0 ? z.x : (qK == 1 ? z.y : (qK == 2 ? z.z : z.w));
        if (i < mnew) mean[i] = zK;
      }
    }
  }
}

// cov[base + r] = c + the row's tiles in ascending jt, one thread per row
template <int RT>
__device__ __forceinline__ void pr_rowsum(const double *__restrict__ ts, int njt, long base, int mnew, double c,
                                          double *__restrict__ cov) {
  constexpr int R = 16 * RT;
  const int tid = threadIdx.x;
  if (tid < R && base + tid < mnew) {
    double s = 0.0;
    for (int jt = 0; jt < njt; ++jt) s += ts[(size_t)jt * R + tid];
    cov[base + tid] = c + s;
  }
}

// J operands stored back to back (operand j at Gf + j * gf_elems, each written by wsb_predict_prep) into column j of
// mean / cov (column-major at ldo): the block's rows are staged once and every operand is multiplied against them, so the
// pair is read once, not J times.  Per (row, operand) the steps are the three above, so column j depends on operand j
// alone.  The workgroups walk the operands in the same order, so the one in use stays in L2.  One ts scratch: a barrier
// after an operand's tiles and one after its row sums.
template <int RT>
__global__ __launch_bounds__(PR_THREADS) void gpc_predict_rows_multi_kernel(const double *__restrict__ V, long ld,
                                                                            const int *__restrict__ idx, int row0, int mnew,
                                                                            int K, int nks, int njt, int J,
                                                                            const double *__restrict__ Gf, long gf_elems,
                                                                            double c, double *__restrict__ mean,
                                                                            double *__restrict__ cov, long ldo) {
  constexpr int R = 16 * RT, RS = pr_stride(R);
  extern __shared__ double pr_lds[];
  double *vs = pr_lds;                         // [4 nks][RS]
  double *ts = pr_lds + (size_t)4 * nks * RS;  // [njt][R]
  const long base = (long)blockIdx.x * R;
  pr_stage<RT>(V, ld, idx, row0, mnew, K, nks, base, vs);
  __syncthreads();
  for (int j = 0; j < J; ++j) {
    pr_tiles<RT>(Gf + (size_t)j * gf_elems, vs, ts, K, nks, njt, base, mnew, mean + (size_t)j * ldo);
    __syncthreads();
    pr_rowsum<RT>(ts, njt, base, mnew, c, cov + (size_t)j * ldo);
    if (j + 1 < J) __syncthreads();
  }
}

// dynamic LDS of a block of R rows
static size_t pr_lds_bytes(int R, int nks, int njt) { return sizeof(double) * ((size_t)4 * nks * pr_stride(R) + (size_t)njt * R); }

size_t gpc_predict_operand_elems(int K) { return (size_t)ceil_div(K + 1, 16) * ceil_div(K, 4) * 64; }

// Block of rows: the largest of 64, 32, 16 that leaves room for two workgroups per CU (one stages while the other
// multiplies), otherwise the largest that fits at all.  K <= GPC_PREDICT_KMAX always fits 16 rows in 160 KB.
static int pr_rows(int nks, int njt, int lds_max) {
  for (int R = 64; R >= 16; R >>= 1)
    if (2 * pr_lds_bytes(R, nks, njt) <= (size_t)lds_max) return R;
  for (int R = 64; R >= 16; R >>= 1)
    if (pr_lds_bytes(R, nks, njt) <= (size_t)lds_max) return R;
  return 0;
}

bool gpc_predict_rows_applicable(int K) {
  if (K > GPC_PREDICT_KMAX) return false;
  const int lds = device_figures().lds_per_block;
  return pr_rows(ceil_div(K, 4), ceil_div(K + 1, 16), lds > 0 ? lds : 65536) != 0;
}

// the block of rows and the dynamic LDS of the kernel at this K; 0 rows: K does not fit the device's LDS
static int pr_shape(const char *who, int K, int *nks, int *njt, size_t *lds) {
  *nks = ceil_div(K, 4); *njt = ceil_div(K + 1, 16);
  const int lds_dev = device_figures().lds_per_block;
  const int R = pr_rows(*nks, *njt, lds_dev > 0 ? lds_dev : 65536);
  if (!R) { set_error("%s: K=%d does not fit the device's LDS", who, K); return 0; }
  *lds = pr_lds_bytes(R, *nks, *njt);
  return R;
}

int gpc_predict_rows_multi(hipStream_t st, const double *dV, long ld, const int *d_idx, int row0, int mnew, int K, int J,
                           const double *d_Gf, double c, double *d_mean, double *d_cov, long ldo) {
  int nks, njt;
  size_t lds;
  const int R = pr_shape("gpc_predict_rows_multi", K, &nks, &njt, &lds);
  if (!R) return FLGP_ERR_UNSUPPORTED;
  ProfScope ps("gpc_predict_rows_multi", st, (double)J * mnew * K * (K + 1));
  const long gf_elems = (long)gpc_predict_operand_elems(K);
  const dim3 grid(ceil_div(mnew, R)), block(PR_THREADS);
  auto launch = [&](auto kfn) -> int {
    if (lds > 48 * 1024) FLGP_HIP(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kfn, grid, block, lds, st, dV, ld, d_idx, row0, mnew, K, nks, njt, J, d_Gf, gf_elems, c, d_mean, d_cov, ldo);
    return check_launch("gpc_predict_rows_multi_kernel");
  };
  if (R == 64) return launch(gpc_predict_rows_multi_kernel<4>);
  if (R == 32) return launch(gpc_predict_rows_multi_kernel<2>);
  return launch(gpc_predict_rows_multi_kernel<1>);
}

// ---- the weight-space Newton loop and the predictive operands for a chunk of problems (WsBatch, eigenpair_logit.hip)
// The steps of the weight-space loop that the lrb_* kernels above do not already have, in their form: the slot in
// blockIdx.y through the device list, a workgroup on its own slot only.  Each keeps the expression tree of the unbatched
// kernel it stands beside where there is one (gpc_w_kernel without N, tri_inv_diag_kernel, gpr_scale_kernel's column
// scaling), so a slot's bits do not depend on its chunk.  bd = b / D sits in the chunk's c, p in its g.

// pi = logistic(f), W = pi (1 - pi): sW = W^1/2, b = W f + (Y - pi)   (N = 1, src/Utils.cpp:269-276)
__global__ void wsb_w_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long s = act[blockIdx.y], o = s * c.sv + i;
  const double fi = c.f[o], yi = c.Y[(size_t)c.ycol[s] * c.ldy + i];
  const double pi = 1.0 / (1.0 + exp(-fi));
  const double W = pi * (1.0 - pi);
  const double bi = W * fi + (yi - pi);
  c.sW[o] = __builtin_sqrt(W);
  c.b[o] = bi;
}

// c = b / D
__global__ void wsb_bd_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long o = (long)act[blockIdx.y] * c.sv + i;
  c.c[o] = c.b[o] / c.D[o];
}

// f_new = p + sigma (b - W p) / D with W = sW^2 and p = g
__global__ void wsb_fnew_kernel(LrChunk c, const int *__restrict__ act) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long o = (long)act[blockIdx.y] * c.sv + i;
  const double s = c.sW[o], pi = c.g[o];
  c.fnew[o] = pi + c.sigma * ((c.b[o] - (s * s) * pi) / c.D[o]);
}

// tri_inv_diag_kernel on the slot's factor: X(b0:b0+nb, b0:b0+nb) = L_Q(b0:b0+nb, b0:b0+nb)^-1 for block b0 = 64 blockIdx.x,
// lane c one column by forward substitution (the block width is tri_inverse's, which is the factorisation's panel width)
__global__ __launch_bounds__(64) void wsb_tri_inv_diag_kernel(LrChunk ch, const int *__restrict__ act, double *__restrict__ Xall) {
  const long s = act[blockIdx.y];
  if (ch.flag[s]) return;
  const double *__restrict__ L = ch.Q + s * ch.sq;
  double *__restrict__ X = Xall + s * ch.sq;
  const int m = ch.K;
  const long lda = ch.K, ldx = ch.K;
  __shared__ double Lt[CNB][CNB];       // Lt[k][i] = L(b0 + i, b0 + k)
  __shared__ double xs[CNB][CNB + 1];   // xs[i][c] = X(b0 + i, b0 + c)
  const int c = threadIdx.x, b0 = blockIdx.x * CNB, nb = min(CNB, m - b0);
  for (int e = c; e < CNB * CNB; e += CNB) {
    const int i = e % CNB, k = e / CNB;
    Lt[k][i] = (i < nb && k <= i) ? L[(size_t)(b0 + k) * lda + b0 + i] : (i == k ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    double acc = (i == c) ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k) acc -= Lt[k][i] * xs[k][c];
    xs[i][c] = acc / Lt[i][i];
  }
  __syncthreads();
  for (int e = c; e < nb * nb; e += CNB) {
    const int i = e % nb, k = e / nb;
    X[(size_t)(b0 + k) * ldx + b0 + i] = xs[i][k];
  }
}

// M(i, j) *= ls(j) on the slot's K x K matrix
__global__ void wsb_scale_cols_kernel(LrChunk c, const int *__restrict__ act, double *__restrict__ M) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)c.K * c.K) return;
  const long s = act[blockIdx.y];
  const int j = (int)(e / c.K);
  double v = M[s * c.sq + e];
  v *= c.ls[s * c.sk + j];
  M[s * c.sq + e] = v;
}

// the predictive operand [G ; u^T] of the slot's G and u in the fused kernel's fragment order: operand s at Gf + s total
__global__ void wsb_predict_prep_kernel(LrChunk c, const int *__restrict__ act, const double *__restrict__ Gall, int nks, long total,
                                        double *__restrict__ Gf) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long s = act[blockIdx.y];
  const double *__restrict__ G = Gall + s * c.sq, *__restrict__ u = c.u + s * c.sk;
  const int K = c.K;
  const int lane = (int)(e & 63);
  const long f = e >> 6;
  const int ks = (int)(f % nks), jt = (int)(f / nks);
  const int j = 16 * jt + (lane & 15), k = 4 * ks + (lane >> 4);
  double v = 0.0;
  if (k < K) {
    if (j < K) v = k <= j ? G[(size_t)k * K + j] : 0.0;
    else if (j == K) v = u[k];
  }
  Gf[s * total + e] = v;
}

int wsb_w(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(wsb_w_kernel, dim3(ceil_div(c.m, 256), A), dim3(256), 0, st, c, act);
  return check_launch("wsb_w_kernel");
}
int wsb_bd(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(wsb_bd_kernel, dim3(ceil_div(c.m, 256), A), dim3(256), 0, st, c, act);
  return check_launch("wsb_bd_kernel");
}
int wsb_fnew(hipStream_t st, const LrChunk &c, const int *act, int A) {
  hipLaunchKernelGGL(wsb_fnew_kernel, dim3(ceil_div(c.m, 256), A), dim3(256), 0, st, c, act);
  return check_launch("wsb_fnew_kernel");
}
int wsb_scale_cols(hipStream_t st, const LrChunk &c, const int *act, int A, double *dM) {
  hipLaunchKernelGGL(wsb_scale_cols_kernel, dim3(ceil_div((long)c.K * c.K, 256), A), dim3(256), 0, st, c, act, dM);
  return check_launch("wsb_scale_cols_kernel");
}
int wsb_predict_prep(hipStream_t st, const LrChunk &c, const int *act, int A, const double *dG, double *d_Gf) {
  const long total = (long)gpc_predict_operand_elems(c.K);
  hipLaunchKernelGGL(wsb_predict_prep_kernel, dim3(ceil_div(total, 256), A), dim3(256), 0, st, c, act, dG, ceil_div(c.K, 4), total,
                     d_Gf);
  return check_launch("wsb_predict_prep_kernel");
}

// the planes one slot needs for the split products of wsb_tri_inverse: the largest over its block rows
size_t wsb_tri_inverse_planes(int K, size_t we) {
  size_t pe = 0;
  for (int r0 = CNB; r0 < K; r0 += CNB) {
    const int nb = std::min(CNB, K - r0);
    pe = std::max(pe, (size_t)gemm_plan_split(nb, r0, r0, we) * nb * r0);
  }
  return pe;
}

// tri_inverse (gpr_grad.hip) on the factor in Q of every slot 0 .. A-1 (`all`: the device list 0, 1, ..), X = L_Q^-1 at Q's
// stride: one memset, the diagonal blocks of every slot in one launch, then per block row its two products for all slots
// in one launch each.  The first takes the split an unbatched tri_inverse with a workspace of `we` doubles chooses, on the
// slot's own planes (part at stride sp, pe >= wsb_tri_inverse_planes(K, we) doubles each); T holds 64 x K per slot at stride st_.
int wsb_tri_inverse(hipStream_t st, const LrChunk &c, const int *all, int A, double *dX, double *dT, long st_, double *part,
                    size_t pe, long sp, size_t we) {
  const int m = c.K;
  const long lda = c.K, ldx = c.K;
  ProfScope ps("tri_inverse_batch", st, (double)A * m * m * m / 3.0);
  FLGP_HIP(hipMemsetAsync(dX, 0, sizeof(double) * (size_t)A * c.sq, st));
  const int nblk = ceil_div(m, CNB);
  hipLaunchKernelGGL(wsb_tri_inv_diag_kernel, dim3(nblk, A), dim3(CNB), 0, st, c, all, dX);
  FLGP_TRY(check_launch("wsb_tri_inv_diag_kernel"));
  for (int r = 1; r < nblk; ++r) {
    const int r0 = r * CNB, nb = std::min(CNB, m - r0);
    const GemmBatch g1{A, all, c.sq, c.sq, st_, 0, sp};
    FLGP_TRY(gemm_launch(st, nb, r0, r0, 1.0, c.Q + r0, 1, lda, dX, 1, ldx, 0.0, nullptr, 0, 0, dT, 1, CNB, part, pe, 0.0, nullptr,
                         nullptr, nullptr, gemm_plan_split(nb, r0, r0, we), nullptr, &g1));
    const GemmBatch g2{A, all, c.sq, st_, c.sq, 0, 0};
    FLGP_TRY(gemm_launch(st, nb, r0, nb, -1.0, dX + (size_t)r0 * ldx + r0, 1, ldx, dT, 1, CNB, 0.0, nullptr, 0, 0, dX + r0, 1, ldx,
                         nullptr, 0, 0.0, nullptr, nullptr, nullptr, 0, nullptr, &g2));
  }
  return FLGP_OK;
}

// ---- the regression posterior's rows: q mean rows under the triangle ------------------------------------
// The operand Gp = [G ; U^T] ((K + q) x K: G lower triangular at ld K, or nullptr for zeros when no variance is wanted;
// U K x q at ld K) in the fragment order of wsb_predict_prep_kernel, njt = ceil((K + q) / 16) j-tiles.
__global__ void gpr_predict_prep_kernel(const double *__restrict__ G, const double *__restrict__ U, int K, int q, int nks,
                                        long total, double *__restrict__ Gf) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int lane = (int)(e & 63);
  const long f = e >> 6;
  const int ks = (int)(f % nks), jt = (int)(f / nks);
  const int j = 16 * jt + (lane & 15), k = 4 * ks + (lane >> 4);
  double v = 0.0;
  if (k < K) {
    if (j < K) v = (G && k <= j) ? G[(size_t)k * K + j] : 0.0;
    else if (j < K + q) v = U[(size_t)(j - K) * K + k];
  }
  Gf[e] = v;
}

// pr_tiles for that operand, the tiles jt0 .. njt - 1: a tile wholly inside the triangle (16 (jt + 1) <= K) runs the k steps
// below 4 (jt + 1), every tile that holds a mean row runs all nks.  Rows j < K are squared into ts as in pr_tiles (skipped
// when ts is nullptr: no variance is wanted and jt0 = K / 16, the first tile with a mean row); mean row K + col comes from
// tile (K + col) / 16, lane group (K + col) & 3, register ((K + col) & 15) >> 2 and goes to mean[col * ldo + i].  For q = 1
// the steps, the sums and the stored mean are pr_tiles' own.
template <int RT>
__device__ __forceinline__ void pr_tiles_q(const double *__restrict__ Gf, const double *__restrict__ vs, double *__restrict__ ts,
                                           int K, int q, int nks, int njt, int jt0, long base, int mnew,
                                           double *__restrict__ mean, long ldo) {
  constexpr int R = 16 * RT, RS = pr_stride(R);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int jlast = njt - 1, ntiles = njt - jt0;
  for (int round = 0; round * PR_WAVES < ntiles; ++round) {
    const int d = round * PR_WAVES + ((round & 1) ? PR_WAVES - 1 - wave : wave);
    if (d >= ntiles) continue;
    const int jt = jlast - d;
    const int steps = 16 * (jt + 1) <= K ? min(4 * (jt + 1), nks) : nks;
    const double *A = Gf + (size_t)jt * nks * 64 + lane;
    const double *B = vs + (size_t)g * RS + col;
    gd4 acc[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) acc[rt] = gd4{0.0, 0.0, 0.0, 0.0};
    double a[4], an[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) a[u] = A[(size_t)min(u, steps - 1) * 64];
    for (int ks = 0; ks < steps; ks += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) an[u] = A[(size_t)min(ks + 4 + u, steps - 1) * 64];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (ks + u < steps) {
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
            acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], B[(size_t)(ks + u) * 4 * RS + rt * 16], acc[rt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) a[u] = an[u];
    }
    const int j0 = 16 * jt + g;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
      const gd4 z = acc[rt];
      if (ts) {
        double s = j0 < K ? z.x * z.x : 0.0;
        s += j0 + 4 < K ? z.y * z.y : 0.0;
        s += j0 + 8 < K ? z.z * z.z : 0.0;
        s += j0 + 12 < K ? z.w * z.w : 0.0;
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (g == 0) ts[(size_t)jt * R + rt * 16 + col] = s;
      }
      const long i = base + rt * 16 + col;
      if (j0 + 12 >= K && i < mnew) {
        const int c0 = j0 - K;                              // the mean column of register 0; registers are 4 rows apart
        if (c0 >= 0 && c0 < q) mean[(size_t)c0 * ldo + i] = z.x;
        if (c0 + 4 >= 0 && c0 + 4 < q) mean[(size_t)(c0 + 4) * ldo + i] = z.y;
        if (c0 + 8 >= 0 && c0 + 8 < q) mean[(size_t)(c0 + 8) * ldo + i] = z.z;
        if (c0 + 12 >= 0 && c0 + 12 < q) mean[(size_t)(c0 + 12) * ldo + i] = z.w;
      }
    }
  }
}

// mean(i, 0:q) = U^T v_i and, with cov, cov_i = c + |G v_i|^2 for the rows v_i of the pair read in place: the staging and the
// row sums of gpc_predict_rows_multi_kernel, pr_tiles_q between them.  cov == nullptr: the mean rows only (the training rows).
template <int RT>
__global__ __launch_bounds__(PR_THREADS) void gpr_predict_rows_kernel(const double *__restrict__ V, long ld,
                                                                      const int *__restrict__ idx, int row0, int mnew, int K,
                                                                      int q, int nks, int njt, const double *__restrict__ Gf,
                                                                      double c, double *__restrict__ mean, long ldo,
                                                                      double *__restrict__ cov) {
  constexpr int R = 16 * RT, RS = pr_stride(R);
  extern __shared__ double pr_lds[];
  double *vs = pr_lds;                         // [4 nks][RS]
  double *ts = pr_lds + (size_t)4 * nks * RS;  // [njt][R]
  const long base = (long)blockIdx.x * R;
  pr_stage<RT>(V, ld, idx, row0, mnew, K, nks, base, vs);
  __syncthreads();
  pr_tiles_q<RT>(Gf, vs, cov ? ts : nullptr, K, q, nks, njt, cov ? 0 : K / 16, base, mnew, mean, ldo);
  if (!cov) return;
  __syncthreads();
  pr_rowsum<RT>(ts, njt, base, mnew, c, cov);
}

size_t gpr_predict_operand_elems(int K, int q) { return (size_t)ceil_div(K + q, 16) * ceil_div(K, 4) * 64; }

bool gpr_predict_rows_applicable(int K, int q) {
  if (K > GPC_PREDICT_KMAX || q > GPR_PREDICT_QMAX) return false;
  const int lds = device_figures().lds_per_block;
  return pr_rows(ceil_div(K, 4), ceil_div(K + q, 16), lds > 0 ? lds : 65536) != 0;
}

int gpr_predict_prep(hipStream_t st, int K, int q, const double *dG, const double *dU, double *d_Gf) {
  const long total = (long)gpr_predict_operand_elems(K, q);
  hipLaunchKernelGGL(gpr_predict_prep_kernel, dim3(ceil_div(total, 256)), dim3(256), 0, st, dG, dU, K, q, ceil_div(K, 4), total, d_Gf);
  return check_launch("gpr_predict_prep_kernel");
}

int gpr_predict_rows(hipStream_t st, const double *dV, long ld, const int *d_idx, int row0, int mnew, int K, int q,
                     const double *d_Gf, double c, double *d_mean, long ldo, double *d_cov) {
  const int nks = ceil_div(K, 4), njt = ceil_div(K + q, 16);
  const int lds_dev = device_figures().lds_per_block;
  const int R = pr_rows(nks, njt, lds_dev > 0 ? lds_dev : 65536);
  if (!R) { set_error("gpr_predict_rows: K=%d, q=%d do not fit the device's LDS", K, q); return FLGP_ERR_UNSUPPORTED; }
  const size_t lds = pr_lds_bytes(R, nks, njt);
  ProfScope ps("gpr_predict_rows", st, (double)mnew * K * (d_cov ? K + 2 * q : 2 * q));
  const dim3 grid(ceil_div(mnew, R)), block(PR_THREADS);
  auto launch = [&](auto kfn) -> int {
    if (lds > 48 * 1024) FLGP_HIP(hipFuncSetAttribute((const void *)kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kfn, grid, block, lds, st, dV, ld, d_idx, row0, mnew, K, q, nks, njt, d_Gf, c, d_mean, ldo, d_cov);
    return check_launch("gpr_predict_rows_kernel");
  };
  if (R == 64) return launch(gpr_predict_rows_kernel<4>);
  if (R == 32) return launch(gpr_predict_rows_kernel<2>);
  return launch(gpr_predict_rows_kernel<1>);
}

// out[i] = c + sum_k Z(i, k)^2, k ascending, a thread per row (the K > GPC_PREDICT_KMAX route of the predictive rows)
__global__ void gpc_rowsumsq_add_kernel(const double *__restrict__ Z, long ldz, int rows, int cols, double c,
                                        double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  double s = 0.0;
  for (int k = 0; k < cols; ++k) { const double v = Z[(size_t)k * ldz + i]; s += v * v; }
  out[i] = c + s;
}

int gpc_rowsumsq_add(hipStream_t st, const double *dZ, long ldz, int rows, int cols, double c, double *d_out) {
  hipLaunchKernelGGL(gpc_rowsumsq_add_kernel, dim3(ceil_div(rows, 256)), dim3(256), 0, st, dZ, ldz, rows, cols, c, d_out);
  return check_launch("gpc_rowsumsq_add_kernel");
}

}  // namespace flgp

using namespace flgp;

extern "C" int flgp_dev_cholesky(void *stream, double *d_A, int m, int single_workgroup, int *d_flag) {
  FLGP_REQUIRE(d_A && d_flag && m >= 1, "cholesky: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  if (single_workgroup) return chol_solve(st, d_A, m, nullptr, 0, d_flag);
  return chol_blocked(st, d_A, m, m, d_flag);
}

extern "C" int flgp_dev_chol_solve(void *stream, const double *d_L, int m, double *d_B, int nrhs, int mode, const int *d_flag) {
  FLGP_REQUIRE(d_L && d_B && d_flag && m >= 1 && nrhs >= 0 && mode >= 1 && mode <= 3, "chol_solve: bad arguments");
  return chol_trsv((hipStream_t)stream, d_L, m, m, d_B, m, nrhs, mode, d_flag);
}

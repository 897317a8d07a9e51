// The regression training objectives on the device: value and gradient of the negative marginal likelihood
// and the negative log posterior of train_regression_gp_cpp (reference src/train.cpp:333-555), for noise = "same" and
// "different", without forming the m x m matrices U, C^-1 or G = V diag(A) V^T the reference builds:
//   (C^-1)_ii     = |column i of L^-1|^2                 tr(C^-1 G) = sum_k A_k |column k of L^-1 V|^2
//   alpha^T G alpha = sum_k A_k |row k of V^T alpha|^2   z_i^-2 (v_i Ls) Q^-1 (Ls v_i^T) = z_i^-2 |row i of V Ls L_Q^-T|^2
// Here: the blocked lower-triangular inverse, the column / row sums of squares, and one assembly kernel that turns the
// pieces into the value and the gradient (clipping and prior terms included).  Every sum runs in a fixed order.
#include "common.h"

namespace flgp {

constexpr int TNB = 64;   // diagonal block of the triangular inverse (the factorisation's panel width)

// X(b0:b0+nb, b0:b0+nb) = L(b0:b0+nb, b0:b0+nb)^-1 for block b0 = 64 blockIdx.x: lane c solves column c of the block by
// forward substitution.  L's block sits in LDS and is read as a broadcast (every lane the same element); the unknowns of
// the lane's column sit in LDS too, a column per lane.
__global__ __launch_bounds__(64) void tri_inv_diag_kernel(const double *__restrict__ L, long lda, int m, double *__restrict__ X,
                                                          long ldx, const int *__restrict__ flag) {
  if (flag[0]) return;
  __shared__ double Lt[TNB][TNB];       // Lt[k][i] = L(b0 + i, b0 + k)
  __shared__ double xs[TNB][TNB + 1];   // xs[i][c] = X(b0 + i, b0 + c)
  const int c = threadIdx.x, b0 = blockIdx.x * TNB, nb = min(TNB, m - b0);
  for (int e = c; e < TNB * TNB; e += TNB) {
    const int i = e % TNB, k = e / TNB;
    Lt[k][i] = (i < nb && k <= i) ? L[(size_t)(b0 + k) * lda + b0 + i] : (i == k ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int i = 0; i < nb; ++i) {
    double acc = (i == c) ? 1.0 : 0.0;
    for (int k = 0; k < i; ++k) acc -= Lt[k][i] * xs[k][c];
    xs[i][c] = acc / Lt[i][i];
  }
  __syncthreads();
  for (int e = c; e < nb * nb; e += TNB) {
    const int i = e % nb, k = e / nb;
    X[(size_t)(b0 + k) * ldx + b0 + i] = xs[i][k];
  }
}

// X = L^-1 (m x m, lower; the upper triangle is zeroed) for the lower factor chol_blocked left in L.  The diagonal blocks
// are inverted in parallel, then block row r (r0 = 64 r) is filled left-looking through the MFMA GEMM:
//   X(r0:, 0:r0) = -X(r0:, r0:) [L(r0:, 0:r0) X(0:r0, 0:r0)]
// with the product in T (64 x m).  `work` (we doubles) bounds the GEMM's k-split.  A set flag leaves X = 0.
int tri_inverse(hipStream_t st, const double *dL, long lda, int m, double *dX, long ldx, double *dT, double *work, size_t we,
                const int *d_flag) {
  ProfScope ps("tri_inverse", st, (double)m * m * m / 3.0);
  FLGP_HIP(hipMemsetAsync(dX, 0, sizeof(double) * (size_t)ldx * m, st));
  const int nblk = ceil_div(m, TNB);
  hipLaunchKernelGGL(tri_inv_diag_kernel, dim3(nblk), dim3(TNB), 0, st, dL, lda, m, dX, ldx, d_flag);
  FLGP_TRY(check_launch("tri_inv_diag_kernel"));
  for (int r = 1; r < nblk; ++r) {
    const int r0 = r * TNB, nb = std::min(TNB, m - r0);
    FLGP_TRY(gemm_launch(st, nb, r0, r0, 1.0, dL + r0, 1, lda, dX, 1, ldx, 0.0, nullptr, 0, 0, dT, 1, TNB, work, we, 0.0,
                         nullptr));
    FLGP_TRY(gemm_launch(st, nb, r0, nb, -1.0, dX + (size_t)r0 * ldx + r0, 1, ldx, dT, 1, TNB, 0.0, nullptr, 0, 0, dX + r0, 1,
                         ldx, nullptr, 0, 0.0, nullptr));
  }
  return FLGP_OK;
}

// out[j] = sum_i X(i, j)^2 for the cols columns of X (rows x cols, leading dimension ldx): a workgroup per column, a fixed
// tree over its 256 threads
__global__ __launch_bounds__(256) void rg_colsumsq_kernel(const double *__restrict__ X, long ldx, int rows, double *__restrict__ out) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  const double *x = X + (size_t)blockIdx.x * ldx;
  double s = 0.0;
  for (int i = tid; i < rows; i += 256) s += x[i] * x[i];
  red[tid] = s;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) red[tid] += red[tid + off];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = red[0];
}

int rg_colsumsq(hipStream_t st, const double *dX, long ldx, int rows, int cols, double *d_out) {
  hipLaunchKernelGGL(rg_colsumsq_kernel, dim3(cols), dim3(256), 0, st, dX, ldx, rows, d_out);
  return check_launch("rg_colsumsq_kernel");
}

__device__ __forceinline__ double rg_block_sum(double v, double *red) {
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

__device__ __forceinline__ double rg_clip(double g, double thr) { return __builtin_fabs(g) >= thr ? g / __builtin_fabs(g) * thr : g; }

// A_k = -lambda_k exp(-t lambda_k), lambda_k = 1 - values_k        (src/train.cpp:376-378, 409, 519)
__device__ __forceinline__ double rg_a(const double *values, int k, double t) {
  const double lam = 1.0 - values[k];
  return -lam * (exp(-t * lam) + 0.0);
}

// value and gradient from the pieces RgTerms names (one workgroup); out = [value, grad_0 .. grad_{nx-1}]
// (written once, for the kernel of one evaluation and the one-workgroup-per-slot kernel of the batch below)
__device__ __forceinline__ void rg_assemble_body(const RgTerms &T, double *red) {
  const int tid = threadIdx.x, m = T.m, q = T.q, K = T.K;
  const double *x = T.x, sigma = T.sigma;
  const long mq = (long)m * q;
  double s = 0.0;
  for (long e = tid; e < mq; e += 1024) s += T.Y[e] * T.alpha[e];
  const double sya = rg_block_sum(s, red);
  double lz = 0.0;
  if (!T.direct && T.different) {
    s = 0.0;
    for (int i = tid; i < m; i += 1024) s += log(x[1 + i] + sigma + 1e-9);
    lz = rg_block_sum(s, red);
  }
  // prior (src/train.cpp:337-338, 444-451): pa = alpha + 1, pb = beta
  const double pp = T.prior[0], pq = T.prior[1], ptau = T.prior[2], pa = T.prior[3] + 1.0, pb = T.prior[4];
  const double t = x[0];
  double pr1 = 0.0;
  if (T.posterior && T.different) {
    s = 0.0;
    for (int i = tid; i < m; i += 1024) {
      const double z = x[1 + i] + sigma;
      s += (pa * log(z) + pb / z) / m;
    }
    pr1 = rg_block_sum(s, red);
  }
  if (tid == 0) {
    double v = 0.5 * sya / q;
    v += T.logdet[0];
    if (!T.direct) v += T.different ? 0.5 * lz : 0.5 * (m - K) * log(T.c);
    if (T.posterior) {
      const double pr0 = pp * log(t + 1e-9) + pow(t / ptau, -pq);
      if (!T.different) pr1 = pa * log(x[1] + sigma) + pb / (x[1] + sigma);
      v = v + pr0 + pr1;
    }
    T.out[0] = v;
  }
  if (!T.grad) return;

  // grad_0: -0.5 (sum_k A_k r_k / q - tr(C^-1 G)), r_k = |row k of V^T alpha|^2
  s = 0.0;
  for (int k = tid; k < K; k += 1024) {
    double r = 0.0;
    for (int c = 0; c < q; ++c) { const double u = T.Vta[(size_t)c * K + k]; r += u * u; }
    s += rg_a(T.values, k, t) * r;
  }
  const double sr = rg_block_sum(s, red);
  double g0a = 0.0, g0b = 0.0, t3 = 0.0;
  if (T.direct) {
    s = 0.0;
    for (int k = tid; k < K; k += 1024) s += rg_a(T.values, k, t) * T.s[k];          // s_k = |column k of L^-1 V|^2
    g0a = rg_block_sum(s, red);
  } else {
    // M = V^T V or V^T Z^-1 V (symmetric), M1 = Q^-1 Ls M:  sum_k A_k M_kk  and  sum_ij M1_ij (A M Ls)_ji   (:411-413, :521-523)
    s = 0.0;
    for (int k = tid; k < K; k += 1024) s += rg_a(T.values, k, t) * T.M[(size_t)k * K + k];
    g0a = rg_block_sum(s, red);
    s = 0.0;
    double s3 = 0.0;
    const long KK = (long)K * K;
    for (long e = tid; e < KK; e += 1024) {
      const int i = (int)(e % K), j = (int)(e / K);
      const double mij = T.M[e];
      s += T.M1[e] * (rg_a(T.values, j, t) * mij * T.ls[i]);
      if (!T.different) s3 += T.Qinv[e] * (T.ls[j] * mij * T.ls[i]);
    }
    g0b = rg_block_sum(s, red);
    if (!T.different) t3 = rg_block_sum(s3, red);
  }
  // "same": grad_1 = -0.5 tr U  (:380, :417-418)
  double sa2 = 0.0, sd = 0.0;
  if (!T.different) {
    s = 0.0;
    for (long e = tid; e < mq; e += 1024) s += T.alpha[e] * T.alpha[e];
    sa2 = rg_block_sum(s, red);
    if (T.direct) {
      s = 0.0;
      for (int i = tid; i < m; i += 1024) s += T.d[i];
      sd = rg_block_sum(s, red);
    }
  }
  if (tid == 0) {
    double g0;
    if (T.direct) {
      g0 = -0.5 * (sr / q - g0a);
    } else {
      const double ci = T.different ? 1.0 : 1.0 / T.c;
      g0 = -0.5 * sr / q;
      g0 += 0.5 * ci * g0a;
      g0 += -0.5 * ci * g0b;
    }
    if (T.posterior) g0 += pp / (t + 1e-9) - (pq / ptau) * pow(t / ptau, -pq - 1.0);
    T.out[1] = g0;
    if (!T.different) {
      double g1 = T.direct ? -0.5 * (sa2 / q - sd) : -0.5 * sa2 / q + 0.5 / T.c * (m - t3);
      g1 = rg_clip(g1, 10.0);
      if (T.posterior) { const double z = x[1] + sigma; g1 += pa / z - pb / (z * z); }
      T.out[2] = g1;
    }
  }
  if (T.different) {
    // grad_i = -0.5 U_ii (direct, :481-483) or -0.5 |alpha_i|^2 / q + 0.5 (z_i^-1 - z_i^-2 p_i) clipped at 1 (:531-548)
    for (int i = tid; i < m; i += 1024) {
      double a2 = 0.0;
      for (int c = 0; c < q; ++c) { const double u = T.alpha[(size_t)c * m + i]; a2 += u * u; }
      const double z = x[1 + i] + sigma;
      double g;
      if (T.direct) {
        g = -0.5 * (a2 / q - T.d[i]);
      } else {
        const double zi = 1.0 / z;
        g = -0.5 * a2 / q;
        g += 0.5 * (zi - zi * zi * T.d[i]);
        g = rg_clip(g, 1.0);
      }
      if (T.posterior) g += (pa / z - pb / (z * z)) / m;
      T.out[2 + i] = g;
    }
  }
}
__global__ __launch_bounds__(1024) void rg_assemble_kernel(RgTerms T) {
  __shared__ double red[1024];
  rg_assemble_body(T, red);
}

int rg_assemble(hipStream_t st, const RgTerms &T) {
  hipLaunchKernelGGL(rg_assemble_kernel, dim3(1), dim3(1024), 0, st, T);
  return check_launch("rg_assemble_kernel");
}

// ---- the same for a chunk of problems (RgbChunk, common.h) ---------------------------------------------
// out[i] = sum_k X(i, k)^2 on the slot's X (rows x cols, leading dimension ldx), k ascending, a thread per row
__global__ void rgb_rowsumsq_kernel(const double *__restrict__ X, long sx, long ldx, int rows, int cols, double *__restrict__ out,
                                    long so) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows) return;
  const long sl = blockIdx.y;
  const double *x = X + sl * sx;
  double s = 0.0;
  for (int k = 0; k < cols; ++k) { const double v = x[(size_t)k * ldx + i]; s += v * v; }
  out[sl * so + i] = s;
}
int rgb_rowsumsq(hipStream_t st, int slots, const double *X, long sx, long ldx, int rows, int cols, double *out, long so) {
  hipLaunchKernelGGL(rgb_rowsumsq_kernel, dim3(ceil_div(rows, 256), slots), dim3(256), 0, st, X, sx, ldx, rows, cols, out, so);
  return check_launch("rgb_rowsumsq_kernel");
}

// One workgroup per slot: chol_logdet_kernel's sum over the factor in Q (gpc.hip: a stride of 1024, the same tree), then
// rg_assemble_body on the slot's pieces, and the slot's pivot flag behind the chunk's results for the host's one copy.
__global__ __launch_bounds__(1024) void rgb_assemble_kernel(RgbChunk c) {
  __shared__ double red[1024];
  const long s = blockIdx.x;
  const int K = c.K;
  const double *LQ = c.Q + s * c.sq;
  double ld = 0.0;
  for (int i = threadIdx.x; i < K; i += 1024) ld += log(LQ[(size_t)i * K + i] + 1e-9);
  ld = rg_block_sum(ld, red);
  if (threadIdx.x == 0) {
    c.logdet[s] = ld;
    ((int *)(c.out + (size_t)gridDim.x * (1 + c.nx)))[s] = c.flag[s];
  }
  RgTerms T;
  T.m = c.m; T.q = c.q; T.K = K; T.direct = 0; T.different = c.different; T.posterior = c.posterior; T.grad = c.grad;
  T.sigma = c.sigma; T.c = c.c[s];
  for (int a = 0; a < 5; ++a) T.prior[a] = c.prior[a];
  T.x = c.x + s * c.sxn;
  T.Y = c.Y; T.alpha = c.alpha + s * c.smq;
  T.logdet = c.logdet + s;
  T.values = c.values + c.pair[s] * c.sk; T.ls = c.ls + s * c.sk;
  T.Vta = c.Vta + s * c.skq; T.d = c.d + s * c.sv; T.s = nullptr;
  T.M = c.different ? c.M + s * c.sq : c.M0 + c.pair[s] * c.sq;
  T.Qinv = c.Qinv + s * c.sq; T.M1 = c.M1 + s * c.sq;
  T.out = c.out + s * (1 + c.nx);
  rg_assemble_body(T, red);
}
int rgb_assemble(hipStream_t st, const RgbChunk &c, int slots) {
  hipLaunchKernelGGL(rgb_assemble_kernel, dim3(slots), dim3(1024), 0, st, c);
  return check_launch("rgb_assemble_kernel");
}

}  // namespace flgp

using namespace flgp;

// T (64 x m) and the k-split planes, sized as the direct branch of the regression objective sizes them (eigenpair_regression.hip)
extern "C" size_t flgp_dev_tri_inverse_workspace(int m) {
  return m < 1 ? 0 : sizeof(double) * ((size_t)TNB * m + (size_t)32 * TNB * m);
}

extern "C" int flgp_dev_tri_inverse(void *stream, const double *d_L, int m, double *d_X, void *d_work, size_t work_bytes,
                                    const int *d_flag) {
  FLGP_REQUIRE(d_L && d_X && d_work && d_flag && m >= 1, "tri_inverse: bad arguments");
  FLGP_REQUIRE(work_bytes >= flgp_dev_tri_inverse_workspace(m), "tri_inverse: workspace of %zu bytes, %zu needed", work_bytes,
               flgp_dev_tri_inverse_workspace(m));
  double *T = (double *)d_work;
  return tri_inverse((hipStream_t)stream, d_L, m, m, d_X, m, T, T + (size_t)TNB * m, (size_t)32 * TNB * m, d_flag);
}

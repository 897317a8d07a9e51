// the Nystrom-extension spectrum of the fit_nystrom_* drivers (reference src/Fit.cpp:244-289, the same
// block in :399-441, :918-960, :1063-1105, :1222-1264, :1379-1421), per bandwidth a2:
//   D_UU, D_XU squared distances;  mean = sum(D_UU)/s^2;  Z = exp(-D/(a2 mean))
//   rs_U = rowsum(Z_UU) + 1e-9;  A_UU = Z_UU / (rs_U rs_U^T);  sd = 1/sqrt(rowsum(A_UU) + 1e-9);  W_UU = sd A_UU sd
//   (values, V) = top-K eigenpairs of W_UU;  V <- sd V, columns rescaled to norm sqrt(s) (+1e-9 guards)
//   rs_X = rowsum(Z_XU) + 1e-9;  A_XU = Z_XU / (rs_X rs_U^T);  W_XU = A_XU / (rowsum(A_XU) + 1e-9)
//   vectors = W_XU V diag(1/(|values| + 1e-9))
// The n x s similarity (400 GB at C5) is never materialised: row blocks of Z_XU are produced together with their row
// sums, multiplied with the (pre-scaled) anchor eigenvectors by the MFMA GEMM, and rescaled.  W_UU is dense
// (every anchor sees every other one), so its eigensolve takes the dense-product path of eig.hip.
// Distances use the k-NN arithmetic (k-ascending FMA chain); the reference's come out of an Eigen GEMM whose
// summation order is unspecified, so this stage is compared at rounding level, not bit for bit.
#include "common.h"
#include <cmath>
#include <memory>

namespace flgp {

// MODE 0: out(x, j) = D(x, u_j), acc1 = sum_j D.   MODE 1: out = exp(-D inv_c), acc1 = sum_j out, acc2 = sum_j out w_j.
// Thread x owns one point (coordinates in registers); blockIdx.y owns a chunk of 64 anchors (wave-uniform operands:
// scalar loads of the padded panel).  Partial sums go to part1/part2[chunk][x] and are added in chunk order later.
template <int DP, int MODE>
__global__ __launch_bounds__(256) void nys_sim_kernel(const double *__restrict__ X, int nb, int ldx, int d,
                                                      const double *__restrict__ Ut, const double *__restrict__ uu, int s,
                                                      double inv_c, const double *__restrict__ w, double *__restrict__ out,
                                                      int ldo, double *__restrict__ part1, double *__restrict__ part2) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int xc = x < nb ? x : nb - 1;
  double xv[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xv[k] = (k < d) ? X[(size_t)k * ldx + xc] : 0.0;
  double xx = xv[0] * xv[0];
#pragma unroll
  for (int k = 1; k < DP; ++k) xx = __builtin_fma(xv[k], xv[k], xx);
  const int j0 = blockIdx.y * 64, j1 = (j0 + 64 < s) ? j0 + 64 : s;
  double a1 = 0.0, a2 = 0.0;
  for (int j = j0; j < j1; ++j) {
    const double *u = Ut + (size_t)j * DP;
    double dot = xv[0] * u[0];
#pragma unroll
    for (int k = 1; k < DP; ++k) dot = __builtin_fma(xv[k], u[k], dot);
    const double D = __builtin_fma(-2.0, dot, xx) + uu[j];
    double v = D;
    if (MODE == 1) v = exp(-D * inv_c);
    if (x < nb) out[(size_t)j * ldo + x] = v;
    a1 += v;
    if (MODE == 1) a2 += v * w[j];
  }
  if (x < nb) {
    part1[(size_t)blockIdx.y * nb + x] = a1;
    if (MODE == 1) part2[(size_t)blockIdx.y * nb + x] = a2;
  }
}

// d > 32: the dot products come from the MFMA GEMM (a k-ascending FMA chain from 0, the same bits as the chain
// above); the 64 anchor coordinates of the scalar-operand kernel no longer fit the SGPR file and its loads stall.
__global__ void nys_sqnorm_kernel(const double *__restrict__ X, int nb, int ldx, int d, double *__restrict__ xx) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nb) return;
  double a = X[x] * X[x];
  for (int k = 1; k < d; ++k) a = __builtin_fma(X[(size_t)k * ldx + x], X[(size_t)k * ldx + x], a);
  xx[x] = a;
}
// in place on the dot products: Z(x, j) = exp(-(fma(-2, dot, xx) + uu_j) inv_c), with the two partial row sums
__global__ __launch_bounds__(256) void nys_exp_rows_kernel(double *__restrict__ Z, int nb, int s, const double *__restrict__ xx,
                                                           const double *__restrict__ uu, double inv_c,
                                                           const double *__restrict__ w, double *__restrict__ part1,
                                                           double *__restrict__ part2) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= nb) return;
  const double xn = xx[x];
  const int j0 = blockIdx.y * 64, j1 = (j0 + 64 < s) ? j0 + 64 : s;
  double a1 = 0.0, a2 = 0.0;
#pragma unroll 8
  for (int j = j0; j < j1; ++j) {
    const double D = __builtin_fma(-2.0, Z[(size_t)j * nb + x], xn) + uu[j];
    const double v = exp(-D * inv_c);
    Z[(size_t)j * nb + x] = v;
    a1 += v;
    a2 += v * w[j];
  }
  part1[(size_t)blockIdx.y * nb + x] = a1;
  part2[(size_t)blockIdx.y * nb + x] = a2;
}

// the same on the dot products of the anchors with themselves: Z(x, j) = D(x, j), row sums in part1 (MODE 0 of nys_sim_kernel)
__global__ __launch_bounds__(256) void nys_dist_rows_kernel(double *__restrict__ Z, int nb, int s, const double *__restrict__ xx,
                                                            const double *__restrict__ uu, double *__restrict__ part1) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= nb) return;
  const double xn = xx[x];
  const int j0 = blockIdx.y * 64, j1 = (j0 + 64 < s) ? j0 + 64 : s;
  double a1 = 0.0;
  for (int j = j0; j < j1; ++j) {
    const double D = __builtin_fma(-2.0, Z[(size_t)j * nb + x], xn) + uu[j];
    Z[(size_t)j * nb + x] = D;
    a1 += D;
  }
  part1[(size_t)blockIdx.y * nb + x] = a1;
}

// r1[x] = sum over chunks (ascending) of part1[chunk][x] (+ add1); same for r2
__global__ void nys_reduce_kernel(const double *__restrict__ part1, const double *__restrict__ part2, int nchunk, int nb,
                                  double add1, double *__restrict__ r1, double *__restrict__ r2) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nb) return;
  double a = 0.0, b = 0.0;
  for (int c = 0; c < nchunk; ++c) {
    a += part1[(size_t)c * nb + x];
    if (part2) b += part2[(size_t)c * nb + x];
  }
  r1[x] = a + add1;
  if (r2) r2[x] = b;
}

__global__ void nys_exp_kernel(double *__restrict__ M, long count, double inv_c) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < count) M[e] = exp(-M[e] * inv_c);
}
// colsum[j] = sum_i M(i, j) (rows ascending, one workgroup per column, fixed tree); M column-major at ld
__global__ __launch_bounds__(256) void nys_colsum_kernel(const double *__restrict__ M, int s, long ld, double *__restrict__ colsum) {
  __shared__ double red[256];
  const int j = blockIdx.x;
  double a = 0.0;
  for (int i = threadIdx.x; i < s; i += 256) a += M[(size_t)j * ld + i];
  red[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) colsum[j] = red[0];
}
// mode 0: v[j] = 1 / (v[j] + 1e-9);  mode 1: v[j] = 1 / sqrt(v[j] + 1e-9)
__global__ void nys_vec_kernel(double *__restrict__ v, int s, int mode) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= s) return;
  v[j] = mode == 0 ? 1.0 / (v[j] + 1e-9) : 1.0 / __builtin_sqrt(v[j] + 1e-9);
}
// M(i, j) <- (M(i, j) a[i]) a[j]
__global__ void nys_symscale_kernel(double *__restrict__ M, int s, const double *__restrict__ a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)s * s) return;
  const int i = (int)(e % s), j = (int)(e / s);
  M[e] = (M[e] * a[i]) * a[j];
}
// anchor eigenvectors: V(j,k) <- sd[j] V(j,k); norms per column; then the column and row factors of the extension
__global__ void nys_rowscale_kernel(double *__restrict__ V, int rows, int cols, int ld, const double *__restrict__ f) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)rows * cols) return;
  const int i = (int)(e % rows), k = (int)(e / rows);
  V[(size_t)k * ld + i] *= f[i];
}
__global__ __launch_bounds__(256) void nys_colnorm_kernel(const double *__restrict__ V, int s, double *__restrict__ nrm) {
  __shared__ double red[256];
  const int k = blockIdx.x;
  double a = 0.0;
  for (int i = threadIdx.x; i < s; i += 256) { const double v = V[(size_t)k * s + i]; a = __builtin_fma(v, v, a); }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) nrm[k] = __builtin_sqrt(red[0]);
}
// V(j,k) <- V(j,k) * sqrt(s)/(nrm_k + 1e-9) * rsu_inv[j] / (|val_k| + 1e-9)
__global__ void nys_vfinal_kernel(double *__restrict__ V, int s, int K, const double *__restrict__ nrm,
                                  const double *__restrict__ rsu_inv, const double *__restrict__ val, double sqrt_s) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)s * K) return;
  const int j = (int)(e % s), k = (int)(e / s);
  V[e] = ((V[e] * (sqrt_s / (nrm[k] + 1e-9))) * rsu_inv[j]) / (__builtin_fabs(val[k]) + 1e-9);
}
// f[x] = (1/rsx[x]) / (s1[x]/rsx[x] + 1e-9)
__global__ void nys_factor_kernel(const double *__restrict__ rsx, const double *__restrict__ s1, int nb, double *__restrict__ f) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nb) return;
  const double inv = 1.0 / rsx[x];
  f[x] = inv / (s1[x] * inv + 1e-9);
}

// ---- the bandwidth grid: one distance, FLGP_NYSTROM_GRID_BATCH similarities.  Per bandwidth the arithmetic, the chunk order
// and the order inside a chunk are those of nys_sim_kernel<DP, 1> / nys_exp_rows_kernel, so block b holds the same bits.
constexpr int NYS_BATCH = FLGP_NYSTROM_GRID_BATCH;
struct NysBatch {
  int cnt;                        // bandwidths in this launch (1 .. NYS_BATCH)
  double inv_c[NYS_BATCH];
  const double *w[NYS_BATCH];     // 1 / (rs_U + 1e-9) of the bandwidth
  double *out[NYS_BATCH];         // its nb x s block of Z_XU (ld nb)
};
// partial sums of bandwidth b go to part1/part2[(b nchunk + chunk) nb + x]
template <int DP>
__global__ __launch_bounds__(256) void nys_sim_grid_kernel(const double *__restrict__ X, int nb, int ldx, int d,
                                                           const double *__restrict__ Ut, const double *__restrict__ uu, int s,
                                                           NysBatch B, double *__restrict__ part1, double *__restrict__ part2) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  const int xc = x < nb ? x : nb - 1;
  double xv[DP];
#pragma unroll
  for (int k = 0; k < DP; ++k) xv[k] = (k < d) ? X[(size_t)k * ldx + xc] : 0.0;
  double xx = xv[0] * xv[0];
#pragma unroll
  for (int k = 1; k < DP; ++k) xx = __builtin_fma(xv[k], xv[k], xx);
  const int j0 = blockIdx.y * 64, j1 = (j0 + 64 < s) ? j0 + 64 : s;
  double a1[NYS_BATCH], a2[NYS_BATCH];
#pragma unroll
  for (int b = 0; b < NYS_BATCH; ++b) a1[b] = a2[b] = 0.0;
  for (int j = j0; j < j1; ++j) {
    const double *u = Ut + (size_t)j * DP;
    double dot = xv[0] * u[0];
#pragma unroll
    for (int k = 1; k < DP; ++k) dot = __builtin_fma(xv[k], u[k], dot);
    const double D = __builtin_fma(-2.0, dot, xx) + uu[j];
#pragma unroll
    for (int b = 0; b < NYS_BATCH; ++b) {
      if (b < B.cnt) {
        const double v = exp(-D * B.inv_c[b]);
        if (x < nb) B.out[b][(size_t)j * nb + x] = v;
        a1[b] += v;
        a2[b] += v * B.w[b][j];
      }
    }
  }
  if (x < nb) {
    const size_t nchunk = gridDim.y;
#pragma unroll
    for (int b = 0; b < NYS_BATCH; ++b) {
      if (b < B.cnt) {
        part1[((size_t)b * nchunk + blockIdx.y) * nb + x] = a1[b];
        part2[((size_t)b * nchunk + blockIdx.y) * nb + x] = a2[b];
      }
    }
  }
}

// the d > 32 route: `dots` (nb x s, ld nb) holds the GEMM's dot products and may be the last block of the batch, which
// is why neither it nor the blocks are __restrict__: an element is read before any block's copy of it is written
__global__ __launch_bounds__(256) void nys_exp_rows_grid_kernel(const double *dots, int nb, int s, const double *__restrict__ xx,
                                                                const double *__restrict__ uu, NysBatch B,
                                                                double *__restrict__ part1, double *__restrict__ part2) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= nb) return;
  const double xn = xx[x];
  const int j0 = blockIdx.y * 64, j1 = (j0 + 64 < s) ? j0 + 64 : s;
  double a1[NYS_BATCH], a2[NYS_BATCH];
#pragma unroll
  for (int b = 0; b < NYS_BATCH; ++b) a1[b] = a2[b] = 0.0;
  for (int j = j0; j < j1; ++j) {
    const double D = __builtin_fma(-2.0, dots[(size_t)j * nb + x], xn) + uu[j];
    double v[NYS_BATCH];
#pragma unroll
    for (int b = 0; b < NYS_BATCH; ++b)
      if (b < B.cnt) v[b] = exp(-D * B.inv_c[b]);
#pragma unroll
    for (int b = 0; b < NYS_BATCH; ++b) {
      if (b < B.cnt) {
        B.out[b][(size_t)j * nb + x] = v[b];
        a1[b] += v[b];
        a2[b] += v[b] * B.w[b][j];
      }
    }
  }
  const size_t nchunk = gridDim.y;
#pragma unroll
  for (int b = 0; b < NYS_BATCH; ++b) {
    if (b < B.cnt) {
      part1[((size_t)b * nchunk + blockIdx.y) * nb + x] = a1[b];
      part2[((size_t)b * nchunk + blockIdx.y) * nb + x] = a2[b];
    }
  }
}

// W = exp(-D inv_c), out of place: the l bandwidths share one D_UU
__global__ void nys_exp_from_kernel(const double *__restrict__ D, double *__restrict__ W, long count, double inv_c) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < count) W[e] = exp(-D[e] * inv_c);
}

template <int MODE>
static int launch_sim(hipStream_t st, int dpad, const double *X, int nb, int ldx, int d, const double *Ut, const double *uu,
                      int s, double inv_c, const double *w, double *out, int ldo, double *p1, double *p2) {
  const dim3 grid(ceil_div(nb, 256), ceil_div(s, 64));
#define NYS_CASE(DPv) if (dpad == DPv) hipLaunchKernelGGL((nys_sim_kernel<DPv, MODE>), grid, dim3(256), 0, st, X, nb, ldx, d, Ut, uu, s, inv_c, w, out, ldo, p1, p2);
  NYS_CASE(4) NYS_CASE(8) NYS_CASE(16) NYS_CASE(32) NYS_CASE(64)
#undef NYS_CASE
  FLGP_REQUIRE(dpad <= 64, "nystrom: no register kernel for dpad = %d (the GEMM route serves d > 64)", dpad);
  return check_launch("nys_sim_kernel");
}

static int launch_sim_grid(hipStream_t st, int dpad, const double *X, int nb, int ldx, int d, const double *Ut, const double *uu,
                           int s, const NysBatch &B, double *p1, double *p2) {
  const dim3 grid(ceil_div(nb, 256), ceil_div(s, 64));
#define NYS_CASE(DPv) if (dpad == DPv) hipLaunchKernelGGL((nys_sim_grid_kernel<DPv>), grid, dim3(256), 0, st, X, nb, ldx, d, Ut, uu, s, B, p1, p2);
  NYS_CASE(4) NYS_CASE(8) NYS_CASE(16) NYS_CASE(32) NYS_CASE(64)
#undef NYS_CASE
  FLGP_REQUIRE(dpad <= 64, "nystrom: no register kernel for dpad = %d (the GEMM route serves d > 64)", dpad);
  return check_launch("nys_sim_grid_kernel");
}

// ---- the steps of the anchor side that the GLGP grid (glgp.hip) takes as well: the same kernels in the same order
// D(x, j) = fma(-2, dot, |u_x|^2) + |u_j|^2 of the points with themselves (s x s, ld s) and its row sums in rsx; p1 holds
// ceil(s / 64) x s doubles, xx s (read for dpad > 64 only)
int nys_self_distances(hipStream_t st, const double *dU, int s, int ldu, int d, int dpad, const double *Ut, const double *uu,
                       double *D, NysScratch &T) {
  const int nchunk = ceil_div(s, 64);
  double *p1 = T.p1.as<double>(), *xx = T.xx.as<double>(), *rsx = T.rsx.as<double>();
  if (dpad > 64) {   // no register kernel beyond d = 64: dot products by the GEMM (one chain per element, the same bits)
    hipLaunchKernelGGL(nys_sqnorm_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, dU, s, ldu, d, xx);
    FLGP_TRY(check_launch("nys_sqnorm_kernel"));
    FLGP_TRY(gemm_launch(st, s, s, d, 1.0, dU, 1, ldu, dU, ldu, 1, 0.0, nullptr, 0, 0, D, 1, s, nullptr, 0, 0.0, nullptr));
    hipLaunchKernelGGL(nys_dist_rows_kernel, dim3(ceil_div(s, 256), nchunk), dim3(256), 0, st, D, s, s, xx, uu, p1);
    FLGP_TRY(check_launch("nys_dist_rows_kernel"));
  } else {
    FLGP_TRY((launch_sim<0>(st, dpad, dU, s, ldu, d, Ut, uu, s, 0.0, nullptr, D, s, p1, nullptr)));
  }
  hipLaunchKernelGGL(nys_reduce_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, p1, nullptr, nchunk, s, 0.0, rsx, nullptr);
  return check_launch("nys_reduce_kernel");
}
void nys_exp_from(hipStream_t st, const double *D, double *W, long count, double inv_c) {
  hipLaunchKernelGGL(nys_exp_from_kernel, dim3(ceil_div(count, 256)), dim3(256), 0, st, D, W, count, inv_c);
}
void nys_colsum(hipStream_t st, const double *M, int s, long ld, double *colsum) {
  hipLaunchKernelGGL(nys_colsum_kernel, dim3(s), dim3(256), 0, st, M, s, ld, colsum);
}
void nys_symscale(hipStream_t st, double *W, int s, const double *a) {
  hipLaunchKernelGGL(nys_symscale_kernel, dim3(ceil_div((long)s * s, 256)), dim3(256), 0, st, W, s, a);
}
// rs = 1 / (rowsum(W) + 1e-9), or from the sums already in rs (have_sums);  W <- diag(rs) W diag(rs)
void nys_first_scaling(hipStream_t st, double *W, int s, double *rs, bool have_sums) {
  if (!have_sums) nys_colsum(st, W, s, s, rs);
  hipLaunchKernelGGL(nys_vec_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, rs, s, 0);      // 1/(rs + 1e-9)
  nys_symscale(st, W, s, rs);
}
// sd = 1 / sqrt(rowsum(W) + 1e-9); the caller scales with it
void nys_second_factor(hipStream_t st, const double *W, int s, double *sd) {
  nys_colsum(st, W, s, s, sd);
  hipLaunchKernelGGL(nys_vec_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, sd, s, 1);       // 1/sqrt(. + 1e-9)
}
// W is symmetric, so column sums are row sums
void nys_normalised_w(hipStream_t st, const double *D, double *W, int s, double inv_c, double *rs, double *sd) {
  nys_exp_from(st, D, W, (long)s * s, inv_c);
  nys_first_scaling(st, W, s, rs);
  nys_second_factor(st, W, s, sd);
  nys_symscale(st, W, s, sd);
}
// V(j, k) <- sd[j] V(j, k) (s x K, ld s) and the column norms
void nys_vector_norms(hipStream_t st, double *V, int s, int K, const double *sd, double *nrm) {
  hipLaunchKernelGGL(nys_rowscale_kernel, dim3(ceil_div((long)s * K, 256)), dim3(256), 0, st, V, s, K, s, sd);
  hipLaunchKernelGGL(nys_colnorm_kernel, dim3(K), dim3(256), 0, st, V, s, nrm);
}

// Rows of X per block of the extension with `nz` blocks of Z_XU (rows x s each) resident: whole rounds of the GEMM grid
// (128 x 128 tiles, two co-resident workgroups per CU, 256 CUs) while the nz blocks together stay under 2 GB; below one
// round a multiple of 256, and never fewer than 256.  (include/flgp_hip.h states this rule for the callers.)
static int row_block(int s, int K, int n, int nz) {
  const long round_rows = 128L * 512 / ceil_div(K, 128);
  const long cap_rows = ((long)256 << 20) / s / nz;
  long nb_max = cap_rows / round_rows * round_rows;
  if (nb_max < round_rows) nb_max = cap_rows / 256 * 256;
  if (nb_max < 256) nb_max = 256;
  if (nb_max > n) nb_max = n;
  return (int)nb_max;
}

static bool dots_via_gemm(int dpad) {
  const int t = tuning("nystrom_dot_gemm", -1);
  return t == 1 || (t < 0 && dpad > 32);
}

// the temporaries of an extension with row blocks of NB rows and nz bandwidths per launch
struct ExtendBufs {
  DevBuf Zb, p1, p2, rsx, s1, fac, xx, gws;
  size_t gws_elems = 0;
  int alloc(int s, int K, int NB, int nz, int NB_plan) {
    const int nchunk = ceil_div(s, 64);
    FLGP_TRY(Zb.alloc(sizeof(double) * (size_t)NB * s * nz));
    FLGP_TRY(p1.alloc(sizeof(double) * (size_t)nchunk * NB * nz));
    FLGP_TRY(p2.alloc(sizeof(double) * (size_t)nchunk * NB * nz));
    FLGP_TRY(rsx.alloc(sizeof(double) * (size_t)NB));
    FLGP_TRY(s1.alloc(sizeof(double) * (size_t)NB));
    FLGP_TRY(fac.alloc(sizeof(double) * (size_t)NB));
    FLGP_TRY(xx.alloc(sizeof(double) * (size_t)NB));
    gws_elems = (size_t)8 * NB_plan * K;      // (of the single-bandwidth row block: the split-k plan is made for that one)
    return gws.alloc(sizeof(double) * gws_elems);
  }
};

// row sums -> row factor -> out(x, k) = f[x] sum_j Z(x, j) V'(j, k) for one bandwidth's block of Z
static int extend_finish(hipStream_t st, const flgp_nystrom_grid *G, int i, ExtendBufs &T, const double *Z, const double *p1,
                         const double *p2, int nb, double *out, int ldv, int split) {
  const int s = G->s, K = G->K, nchunk = ceil_div(s, 64);
  hipLaunchKernelGGL(nys_reduce_kernel, dim3(ceil_div(nb, 256)), dim3(256), 0, st, p1, p2, nchunk, nb, 1e-9, T.rsx.as<double>(),
                     T.s1.as<double>());
  hipLaunchKernelGGL(nys_factor_kernel, dim3(ceil_div(nb, 256)), dim3(256), 0, st, T.rsx.as<double>(), T.s1.as<double>(), nb,
                     T.fac.as<double>());
  FLGP_TRY(check_launch("nystrom block sums"));
  FLGP_TRY(gemm_launch(st, nb, K, s, 1.0, Z, 1, nb, G->eigv_of(i), 1, s, 0.0, nullptr, 0, 0, out, 1,
                       ldv, T.gws.as<double>(), T.gws_elems, 0.0, nullptr, nullptr, nullptr, split));
  hipLaunchKernelGGL(nys_rowscale_kernel, dim3(ceil_div((long)nb * K, 256)), dim3(256), 0, st, out, nb, K, ldv, T.fac.as<double>());
  return check_launch("nys_rowscale_kernel");
}

// Nystrom extension of the rows of X for bandwidth i (src/Fit.cpp:283-289 and :321-325), row block by row block
int nystrom_grid_extend(hipStream_t st, const flgp_nystrom_grid *G, int i, const double *dX, int n, int ldx, double *d_vectors,
                        int ldv) {
  const int s = G->s, d = G->d, K = G->K, dpad = G->dpad, nchunk = ceil_div(s, 64);
  const int NB = row_block(s, K, n, 1);
  ExtendBufs T;
  FLGP_TRY(T.alloc(s, K, NB, 1, NB));
  const double *Ut = (const double *)G->Ut.p, *uu = (const double *)G->uu.p, *dU = (const double *)G->U.p;
  const double *rsu = G->rsu_of(i);
  const double inv_c = G->inv_c[i];
  // without a workspace gemm_launch cannot split k, so every dot product is one whole chain
  const bool via_gemm = dots_via_gemm(dpad);
  for (int x0 = 0; x0 < n; x0 += NB) {
    const int nb = (n - x0 < NB) ? n - x0 : NB;
    if (via_gemm) {
      hipLaunchKernelGGL(nys_sqnorm_kernel, dim3(ceil_div(nb, 256)), dim3(256), 0, st, dX + x0, nb, ldx, d, T.xx.as<double>());
      FLGP_TRY(check_launch("nys_sqnorm_kernel"));
      FLGP_TRY(gemm_launch(st, nb, s, d, 1.0, dX + x0, 1, ldx, dU, s, 1, 0.0, nullptr, 0, 0, T.Zb.as<double>(), 1, nb, nullptr, 0,
                           0.0, nullptr));
      hipLaunchKernelGGL(nys_exp_rows_kernel, dim3(ceil_div(nb, 256), nchunk), dim3(256), 0, st, T.Zb.as<double>(), nb, s,
                         T.xx.as<double>(), uu, inv_c, rsu, T.p1.as<double>(), T.p2.as<double>());
      FLGP_TRY(check_launch("nys_exp_rows_kernel"));
    } else {
      FLGP_TRY((launch_sim<1>(st, dpad, dX + x0, nb, ldx, d, Ut, uu, s, inv_c, rsu, T.Zb.as<double>(), nb, T.p1.as<double>(),
                              T.p2.as<double>())));
    }
    FLGP_TRY(extend_finish(st, G, i, T, T.Zb.as<double>(), T.p1.as<double>(), T.p2.as<double>(), nb, d_vectors + x0, ldv, 0));
  }
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// The same for all l bandwidths: the distance of a row to an anchor is computed once per batch of NYS_BATCH bandwidths.
// The row block shrinks with the Z blocks held at once; the extension GEMM of a shrunken block takes the split-k plan of the
// single-bandwidth block that its rows lie in, so every element is added up exactly as nystrom_grid_extend adds it.
int nystrom_grid_extend_all(hipStream_t st, const flgp_nystrom_grid *G, const double *dX, int n, int ldx,
                            double *const *d_vectors, int ldv) {
  const int s = G->s, d = G->d, K = G->K, l = G->l, dpad = G->dpad, nchunk = ceil_div(s, 64);
  const int nz = l < NYS_BATCH ? l : NYS_BATCH;
  const int NB1 = row_block(s, K, n, 1), NB = row_block(s, K, n, nz);
  ExtendBufs T;
  FLGP_TRY(T.alloc(s, K, NB, nz, NB1));
  const double *Ut = (const double *)G->Ut.p, *uu = (const double *)G->uu.p, *dU = (const double *)G->U.p;
  const bool via_gemm = dots_via_gemm(dpad);
  for (int y0 = 0; y0 < n; y0 += NB1) {          // the single-bandwidth blocks: they fix the plan
    const int nb1 = (n - y0 < NB1) ? n - y0 : NB1;
    const int split = gemm_plan_split(nb1, K, s, T.gws_elems);
    for (int x0 = y0; x0 < y0 + nb1; x0 += NB) {
      const int nb = (y0 + nb1 - x0 < NB) ? y0 + nb1 - x0 : NB;
      if (via_gemm) {
        hipLaunchKernelGGL(nys_sqnorm_kernel, dim3(ceil_div(nb, 256)), dim3(256), 0, st, dX + x0, nb, ldx, d, T.xx.as<double>());
        FLGP_TRY(check_launch("nys_sqnorm_kernel"));
      }
      for (int b0 = 0; b0 < l; b0 += NYS_BATCH) {
        NysBatch B;
        B.cnt = (l - b0 < NYS_BATCH) ? l - b0 : NYS_BATCH;
        for (int b = 0; b < NYS_BATCH; ++b) {
          const int i = b0 + (b < B.cnt ? b : 0);
          B.inv_c[b] = G->inv_c[i];
          B.w[b] = G->rsu_of(i);
          B.out[b] = T.Zb.as<double>() + (size_t)(b < B.cnt ? b : 0) * nb * s;
        }
        if (via_gemm) {
          double *dots = B.out[B.cnt - 1];
          FLGP_TRY(gemm_launch(st, nb, s, d, 1.0, dX + x0, 1, ldx, dU, s, 1, 0.0, nullptr, 0, 0, dots, 1, nb, nullptr, 0, 0.0,
                               nullptr));
          hipLaunchKernelGGL(nys_exp_rows_grid_kernel, dim3(ceil_div(nb, 256), nchunk), dim3(256), 0, st, dots, nb, s,
                             T.xx.as<double>(), uu, B, T.p1.as<double>(), T.p2.as<double>());
          FLGP_TRY(check_launch("nys_exp_rows_grid_kernel"));
        } else {
          FLGP_TRY(launch_sim_grid(st, dpad, dX + x0, nb, ldx, d, Ut, uu, s, B, T.p1.as<double>(), T.p2.as<double>()));
        }
        for (int b = 0; b < B.cnt; ++b)
          FLGP_TRY(extend_finish(st, G, b0 + b, T, B.out[b], T.p1.as<double>() + (size_t)b * nchunk * nb,
                                 T.p2.as<double>() + (size_t)b * nchunk * nb, nb, d_vectors[b0 + b] + x0, ldv, split));
      }
    }
  }
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

int check_bandwidths(const char *who, const double *a2s, int l) {
  for (int i = 0; i < l; ++i)
    if (!(a2s[i] > 0.0) || !std::isfinite(a2s[i])) {
      set_error("bandwidth %d (a2=%g): %s: a2 must be positive and finite", i, a2s[i], who);
      return FLGP_ERR_INVALID;
    }
  return FLGP_OK;
}

// what the Nystrom predictor (nystrom_predictor.hip, predictor.hip) shares with the extension: its single-bandwidth row
// block R(1) and its choice of the dot-product route
int nys_row_block(int s, int K, int n) { return row_block(s, K, n, 1); }
bool nys_dots_via_gemm(int dpad) { return dpad > 64 || dots_via_gemm(dpad); }

}  // namespace flgp

using namespace flgp;

namespace {

// what one worker of the anchor side owns: W_UU, the eigensolver's workspace, two vectors
struct AnchorWorker {
  DevBuf W, work, sd, nrm;
  size_t wb = 0;
  int alloc(int s, int K) {
    wb = flgp_dev_eig_workspace(s, K);
    FLGP_TRY(W.alloc(sizeof(double) * (size_t)s * s));
    FLGP_TRY(work.alloc(wb));
    FLGP_TRY(sd.alloc(sizeof(double) * (size_t)s));
    return nrm.alloc(sizeof(double) * (size_t)K);
  }
};

// bandwidth i: Z_UU, rs_U, A_UU, sd, W_UU (src/Fit.cpp:266-270), its top-K eigenpairs (:272-276), V <- sd V with columns of
// norm sqrt(s) (:278-280) and the two diagonal factors of the extension folded in
int anchor_side(hipStream_t st, flgp_nystrom_grid *G, int i, const double *D, AnchorWorker &A) {
  const int s = G->s, K = G->K;
  double *W = A.W.as<double>(), *sd = A.sd.as<double>(), *nrm = A.nrm.as<double>();
  double *rsu = (double *)G->rsu_of(i), *values = (double *)G->values_of(i), *eigv = (double *)G->eigv_of(i);
  nys_normalised_w(st, D, W, s, G->inv_c[i], rsu, sd);
  FLGP_TRY(check_launch("nystrom W_UU"));
  FLGP_TRY(flgp_dev_eig_topk(st, W, s, s, K, 0.0, values, eigv, s, A.work.p, A.wb, nullptr));
  nys_vector_norms(st, eigv, s, K, sd, nrm);
  hipLaunchKernelGGL(nys_vfinal_kernel, dim3(ceil_div((long)s * K, 256)), dim3(256), 0, st, eigv, s, K, nrm, rsu, values,
                     std::sqrt((double)s));
  FLGP_TRY(check_launch("nystrom V_UU"));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

}  // namespace

// dU: s x d column-major (ldu); a2s: l bandwidths (host).  Synchronous.
extern "C" int flgp_dev_nystrom_grid_create(void *stream, const double *dU, int s, int ldu, int d, const double *a2s, int l,
                                            int K, int max_parallel, flgp_nystrom_grid **out) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(out, "nystrom_grid_create: null pointer");
  *out = nullptr;
  FLGP_REQUIRE(dU && a2s, "nystrom_grid_create: null pointer");
  FLGP_REQUIRE(l >= 1, "nystrom_grid_create: need at least one bandwidth (l=%d)", l);
  const int dpad = flgp_dev_anchor_dpad(d);
  FLGP_REQUIRE(dpad > 0 && d >= 1, "nystrom: kernels are built for 1 <= d <= %d (got %d)", FLGP_DMAX, d);
  FLGP_REQUIRE(s >= 2 && K >= 1 && K <= s, "nystrom: need 1 <= K <= s, s >= 2 (K=%d, s=%d)", K, s);
  FLGP_REQUIRE(ldu >= s, "nystrom: leading dimensions too small");
  FLGP_TRY(check_bandwidths("nystrom", a2s, l));
  std::unique_ptr<flgp_nystrom_grid> G(new flgp_nystrom_grid());
  G->s = s; G->d = d; G->dpad = dpad; G->l = l; G->K = K;
  G->a2s.assign(a2s, a2s + l);
  FLGP_HIP(hipGetDevice(&G->device));
  const int rows = flgp_dev_anchor_rows(s);
  DevBuf D;
  NysScratch T;
  FLGP_TRY(G->U.alloc(sizeof(double) * (size_t)s * d));
  FLGP_TRY(G->Ut.alloc(sizeof(double) * (size_t)rows * dpad));
  FLGP_TRY(G->uu.alloc(sizeof(double) * (size_t)rows));
  G->vs = ((size_t)K + 31) / 32 * 32; G->rs = ((size_t)s + 31) / 32 * 32; G->es = ((size_t)s * K + 31) / 32 * 32;
  FLGP_TRY(G->values.alloc(sizeof(double) * l * G->vs));
  FLGP_TRY(G->rsu.alloc(sizeof(double) * l * G->rs));
  FLGP_TRY(G->eigv.alloc(sizeof(double) * l * G->es));
  FLGP_TRY(D.alloc(sizeof(double) * (size_t)s * s));
  FLGP_TRY(T.alloc(s, dpad, false));
  FLGP_HIP(hipMemcpy2DAsync(G->U.p, sizeof(double) * (size_t)s, dU, sizeof(double) * (size_t)ldu, sizeof(double) * (size_t)s, d,
                            hipMemcpyDeviceToDevice, st));
  FLGP_TRY(flgp_dev_anchor_prep(st, dU, s, ldu, d, G->Ut.as<double>(), G->uu.as<double>()));
  // ---- D_UU and its mean (src/Fit.cpp:244,248), once for the grid
  FLGP_TRY(nys_self_distances(st, dU, s, ldu, d, dpad, G->Ut.as<double>(), G->uu.as<double>(), D.as<double>(), T));
  std::vector<double> hrow(s);
  FLGP_HIP(hipMemcpyAsync(hrow.data(), T.rsx.p,sizeof(double) * s, hipMemcpyDeviceToHost, st));
  FLGP_HIP(hipStreamSynchronize(st));
  double total = 0.0;
  for (int i = 0; i < s; ++i) total += hrow[i];
  const double mean = total / ((double)s * (double)s);
  FLGP_REQUIRE(mean > 0.0 && std::isfinite(mean), "nystrom: the anchors coincide (mean squared distance %g)", mean);
  G->mean = mean;
  G->inv_c.resize(l);
  for (int i = 0; i < l; ++i) G->inv_c[i] = 1.0 / (a2s[i] * mean);
  // ---- workers: at most max_parallel, at most l, and no more than fit into 90 % of the free memory (worker_pool.h)
  DevicePool pool;
  FLGP_TRY(pool.plan(max_parallel, l, 8.0 * s * (double)s + (double)flgp_dev_eig_workspace(s, K) + 8.0 * (s + K)));
  G->workers = pool.workers;
  flgp_nystrom_grid *Gp = G.get();
  const double *Dp = D.as<double>();
  FLGP_TRY(bandwidth_failure(pool.run<AnchorWorker>(
                                 st, l, [&](AnchorWorker &A) { return A.alloc(s, K); },
                                 [&](hipStream_t ws, AnchorWorker &A, int i) { return anchor_side(ws, Gp, i, Dp, A); }),
                             a2s));
  *out = G.release();
  return FLGP_OK;
}

static int grid_usable(const flgp_nystrom_grid *G, const char *who) {
  FLGP_REQUIRE(G, "%s: null handle", who);
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == G->device, "%s: the grid lives on device %d, the current device is %d", who, G->device, dev);
  return FLGP_OK;
}

// dX: n x d column-major (ldx); d_values: K (or NULL); d_vectors: n x K column-major (ldv).  Synchronous.
extern "C" int flgp_dev_nystrom_grid_extend(void *stream, const flgp_nystrom_grid *grid, int i, const double *dX, int n, int ldx,
                                            double *d_values, double *d_vectors, int ldv) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_TRY(grid_usable(grid, "nystrom_grid_extend"));
  FLGP_REQUIRE(i >= 0 && i < grid->l, "nystrom_grid_extend: bandwidth %d outside 0..%d", i, grid->l - 1);
  FLGP_REQUIRE(dX && d_vectors, "nystrom_grid_extend: null pointer");
  FLGP_REQUIRE(n >= 1 && ldx >= n && ldv >= n, "nystrom_grid_extend: need n >= 1 and leading dimensions >= n");
  if (d_values)
    FLGP_HIP(hipMemcpyAsync(d_values, grid->values_of(i), sizeof(double) * (size_t)grid->K, hipMemcpyDeviceToDevice, st));
  return nystrom_grid_extend(st, grid, i, dX, n, ldx, d_vectors, ldv);
}

// d_values: l x K (or NULL); d_vectors: l blocks of ldv x K doubles, block i = the n x K vectors of bandwidth i (ldv)
extern "C" int flgp_dev_nystrom_grid_extend_all(void *stream, const flgp_nystrom_grid *grid, const double *dX, int n, int ldx,
                                                double *d_values, double *d_vectors, int ldv) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_TRY(grid_usable(grid, "nystrom_grid_extend_all"));
  FLGP_REQUIRE(dX && d_vectors, "nystrom_grid_extend_all: null pointer");
  FLGP_REQUIRE(n >= 1 && ldx >= n && ldv >= n, "nystrom_grid_extend_all: need n >= 1 and leading dimensions >= n");
  if (d_values)
    FLGP_HIP(hipMemcpy2DAsync(d_values, sizeof(double) * (size_t)grid->K, grid->values.p, sizeof(double) * grid->vs,
                              sizeof(double) * (size_t)grid->K, grid->l, hipMemcpyDeviceToDevice, st));
  std::vector<double *> blocks(grid->l);
  for (int i = 0; i < grid->l; ++i) blocks[i] = d_vectors + (size_t)i * ldv * grid->K;
  return nystrom_grid_extend_all(st, grid, dX, n, ldx, blocks.data(), ldv);
}

// dX: n x d column-major (ldx), dU: s x d column-major (ldu); d_values: K, d_vectors: n x K column-major (ldv).
// A grid of one bandwidth, its extension to the rows of X, and the grid given back.
extern "C" int flgp_dev_nystrom_eigenpair(void *stream, const double *dX, int n, int ldx, int d, const double *dU, int s,
                                          int ldu, double a2, int K, double *d_values, double *d_vectors, int ldv) {
  const int dpad = flgp_dev_anchor_dpad(d);
  FLGP_REQUIRE(dpad > 0 && d >= 1, "nystrom: kernels are built for 1 <= d <= %d (got %d)", FLGP_DMAX, d);
  FLGP_REQUIRE(n >= 1 && s >= 2 && K >= 1 && K <= s && a2 > 0.0, "nystrom: need n >= 1, 1 <= K <= s, a2 > 0");
  FLGP_REQUIRE(ldx >= n && ldu >= s && ldv >= n, "nystrom: leading dimensions too small");
  flgp_nystrom_grid *g = nullptr;
  FLGP_TRY(flgp_dev_nystrom_grid_create(stream, dU, s, ldu, d, &a2, 1, K, 1, &g));
  std::unique_ptr<flgp_nystrom_grid> G(g);
  return flgp_dev_nystrom_grid_extend(stream, g, 0, dX, n, ldx, d_values, d_vectors, ldv);
}

// The row path of the Nystrom predictor (include/flgp_hip.h).  A row's extended eigenvector entries are
//   u_i = f_i sum_j Z_ij V'_j,   Z_ij = exp(-D(x_i, u_j) inv_c),   f_i the row factor of nys_factor_kernel (nystrom.hip),
// and with the folded operand P = V' Gp^T (s x (K + q) per group, predictor.hip) the posterior of the row is
//   z_i = f_i sum_j Z_ij P_j:   its last q entries the mean, cg plus the squares of its first K entries the variance.
// Mean: the similarity kernels of nystrom.hip with up to NP_CM accumulators a_c += v Pm(j, c) beside the two partial row
// sums -- the value v never goes to memory unless a variance is asked for.  Pm is a packed copy of the mean columns of P, a
// row of NP_CM doubles per (pass, anchor): one 64-byte scalar load.  A second kernel adds the chunk partials in ascending
// chunk order, makes f as nys_reduce_kernel + nys_factor_kernel make it, and writes mean = f sum.
// Variance: Z is stored, T = Z P(:, the columns of a chunk of groups) is one j-ascending MFMA chain per element (gemm_launch
// without a workspace), and var = cg + sum_k (f T_k)^2 with k ascending from 0.0.
#include "common.h"
#include <algorithm>

using namespace flgp;

namespace flgp {

constexpr int NP_CM = 8;                              // mean columns per pass (register figures: DESIGN f-21)
// bytes of T = Z P held at once: groups are chunked under it (knob nystrom_predictor_t_mb, default 256, at least 1; every
// element of T is one chain whatever the chunk, so the knob changes no bit)
static size_t np_t_cap() { return (size_t)std::max(1, tuning("nystrom_predictor_t_mb", 256)) << 20; }

// column m = g q + c of the mean sits at column g (K + q) + K + c of P; columns past groups q are zero
__global__ void np_pack_kernel(const double *__restrict__ P, long ldp, int s, int K, int q, int gq, int npass,
                               double *__restrict__ Pm) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)npass * s * NP_CM) return;
  const int c = (int)(e % NP_CM);
  const long jp = e / NP_CM;
  const int j = (int)(jp % s), pass = (int)(jp / s);
  const int m = pass * NP_CM + c;
  Pm[e] = m < gq ? P[(long)j * ldp + (long)(m / q) * (K + q) + K + m % q] : 0.0;
}

// nys_sim_kernel<DP, 1> (nystrom.hip) with the mean accumulators.  Thread x owns a row (coordinates in registers), blockIdx.y
// a chunk of 64 anchors; the anchor panel, uu, w and the Pm rows are wave-uniform: scalar loads.  v, a1 and a2 are that
// kernel's expressions in its order.  STORE: Z(x, j) = v is written (ld nb).  sums: part1 / part2[chunk][x] are written (the
// first pass).  NC = NP_CM: pm[(chunk NP_CM + c) nb + x] = sum over the chunk's anchors, ascending, of v Pm(j, c) from 0.0,
// multiply then add.  NC = 0: no mean.
template <int DP, int NC, int STORE>
__global__ __launch_bounds__(256) void np_sim_kernel(const double *__restrict__ X, int nb, int ldx, int d,
                                                     const double *__restrict__ Ut, const double *__restrict__ uu, int s,
                                                     double inv_c, const double *__restrict__ w, const double *__restrict__ Pm,
                                                     double *__restrict__ Z, int sums, double *__restrict__ part1,
                                                     double *__restrict__ part2, double *__restrict__ pm) {
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
  double am[NC > 0 ? NC : 1];
#pragma unroll
  for (int c = 0; c < NC; ++c) am[c] = 0.0;
  for (int j = j0; j < j1; ++j) {
    const double *u = Ut + (size_t)j * DP;
    double dot = xv[0] * u[0];
#pragma unroll
    for (int k = 1; k < DP; ++k) dot = __builtin_fma(xv[k], u[k], dot);
    const double D = __builtin_fma(-2.0, dot, xx) + uu[j];
    const double v = exp(-D * inv_c);
    if (STORE && x < nb) Z[(size_t)j * nb + x] = v;
    a1 += v;
    a2 += v * w[j];
    const double *pj = Pm + (size_t)j * NP_CM;
#pragma unroll
    for (int c = 0; c < NC; ++c) am[c] = am[c] + v * pj[c];
  }
  if (x < nb) {
    if (sums) {
      part1[(size_t)blockIdx.y * nb + x] = a1;
      part2[(size_t)blockIdx.y * nb + x] = a2;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) pm[((size_t)blockIdx.y * NP_CM + c) * nb + x] = am[c];
  }
}

// |x|^2 as nys_sqnorm_kernel makes it
__global__ void np_sqnorm_kernel(const double *__restrict__ X, int nb, int ldx, int d, double *__restrict__ xx) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= nb) return;
  double a = X[x] * X[x];
  for (int k = 1; k < d; ++k) a = __builtin_fma(X[(size_t)k * ldx + x], X[(size_t)k * ldx + x], a);
  xx[x] = a;
}

// nys_exp_rows_kernel (nystrom.hip) with the mean accumulators, on the GEMM's dot products in Z (nb x s, ld nb).
// MODE 0: v from the dot product, Z left as it is; MODE 1: v written back in place; MODE 2: Z already holds v (a further
// pass of mean columns after a MODE 1 pass).  MODE 0 and 1 write the partial row sums.
template <int NC, int MODE>
__global__ __launch_bounds__(256) void np_exp_rows_kernel(double *__restrict__ Z, int nb, int s, const double *__restrict__ xx,
                                                          const double *__restrict__ uu, double inv_c,
                                                          const double *__restrict__ w, const double *__restrict__ Pm,
                                                          double *__restrict__ part1, double *__restrict__ part2,
                                                          double *__restrict__ pm) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= nb) return;
  const double xn = MODE == 2 ? 0.0 : xx[x];
  const int j0 = blockIdx.y * 64, j1 = (j0 + 64 < s) ? j0 + 64 : s;
  double a1 = 0.0, a2 = 0.0;
  double am[NC > 0 ? NC : 1];
#pragma unroll
  for (int c = 0; c < NC; ++c) am[c] = 0.0;
#pragma unroll 4
  for (int j = j0; j < j1; ++j) {
    double v = Z[(size_t)j * nb + x];
    if (MODE != 2) {
      const double D = __builtin_fma(-2.0, v, xn) + uu[j];
      v = exp(-D * inv_c);
      if (MODE == 1) Z[(size_t)j * nb + x] = v;
      a1 += v;
      a2 += v * w[j];
    }
    const double *pj = Pm + (size_t)j * NP_CM;
#pragma unroll
    for (int c = 0; c < NC; ++c) am[c] = am[c] + v * pj[c];
  }
  if (MODE != 2) {
    part1[(size_t)blockIdx.y * nb + x] = a1;
    part2[(size_t)blockIdx.y * nb + x] = a2;
  }
#pragma unroll
  for (int c = 0; c < NC; ++c) pm[((size_t)blockIdx.y * NP_CM + c) * nb + x] = am[c];
}

// make_f: rs = (sum over chunks, ascending from 0.0, of part1) + 1e-9 and s1 = the same sum of part2, as nys_reduce_kernel;
// f = (1 / rs) / (s1 / rs + 1e-9) as nys_factor_kernel; fac[x] = f.  Otherwise f = fac[x].  Then for the nc columns of the
// pass: mean(x, c) = f * (sum over chunks, ascending from 0.0, of pm[chunk][c][x]).
__global__ __launch_bounds__(64) void np_finish_kernel(const double *__restrict__ part1, const double *__restrict__ part2,
                                                       const double *__restrict__ pm, int nchunk, int nb, int nc, int make_f,
                                                       double *__restrict__ fac, double *__restrict__ mean, long ldm) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= nb) return;
  double f;
  if (make_f) {
    double a = 0.0, b = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      a += part1[(size_t)c * nb + x];
      b += part2[(size_t)c * nb + x];
    }
    const double inv = 1.0 / (a + 1e-9);
    f = inv / (b * inv + 1e-9);
    fac[x] = f;
  } else {
    f = fac[x];
  }
  for (int c = 0; c < nc; ++c) {
    double a = 0.0;
    for (int ch = 0; ch < nchunk; ++ch) a += pm[((size_t)ch * NP_CM + c) * nb + x];
    mean[(long)c * ldm + x] = f * a;
  }
}

// var(x, g) = cg[g] + sum_k (f_x T(x, g w + k))^2 over k = 0 .. K-1 in that order from 0.0, multiply then add; T nb x (gc w),
// ld nb.  The order is a function of (K, k) alone and every term is a square: var >= cg bit for bit.
__global__ __launch_bounds__(256) void np_var_kernel(const double *__restrict__ T, int nb, int K, int w, int gc,
                                                     const double *__restrict__ fac, const double *__restrict__ cg,
                                                     double *__restrict__ var, long ldv) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= nb) return;
  const double f = fac[x];
  for (int g = blockIdx.y; g < gc; g += gridDim.y) {
    const double *Tg = T + (size_t)g * w * nb + x;
    double sq = 0.0;
    for (int k = 0; k < K; ++k) {
      const double t = f * Tg[(size_t)k * nb];
      sq = sq + t * t;
    }
    var[(long)g * ldv + x] = cg[g] + sq;
  }
}

// out(x, c) = f_x T(x, c) for the nc columns of a chunk: the product np_var_kernel squares (T nb x nc, ld nb)
__global__ __launch_bounds__(256) void np_scale_kernel(const double *__restrict__ T, int nb, int nc, const double *__restrict__ fac,
                                                       double *__restrict__ out, long ldo) {
  const int x = blockIdx.x * 256 + threadIdx.x;
  if (x >= nb) return;
  const double f = fac[x];
  for (int c = blockIdx.y; c < nc; c += gridDim.y) out[(long)c * ldo + x] = f * T[(size_t)c * nb + x];
}

template <int NC, int STORE>
static int np_launch_sim(hipStream_t st, int dpad, const double *X, int nb, int ldx, int d, const double *Ut, const double *uu, int s,
                         double inv_c, const double *w, const double *Pm, double *Z, int sums, double *p1, double *p2, double *pm) {
  const dim3 grid(ceil_div(nb, 256), ceil_div(s, 64));
#define NP_CASE(DPv) if (dpad == DPv) hipLaunchKernelGGL((np_sim_kernel<DPv, NC, STORE>), grid, dim3(256), 0, st, X, nb, ldx, d, Ut, uu, s, inv_c, w, Pm, Z, sums, p1, p2, pm);
  NP_CASE(4) NP_CASE(8) NP_CASE(16) NP_CASE(32) NP_CASE(64)
#undef NP_CASE
  return check_launch("np_sim_kernel");
}

// the doubles of the workspace, in the order they are laid out
struct NpLayout {
  size_t Z, p1, p2, pm, fac, xx, Pm, T, total;
  int nchunk, npass, gc;
  NpLayout(int n, int s, int groups, int K, int q, int want_var) {
    nchunk = ceil_div(s, 64);
    npass = ceil_div((long)groups * q, NP_CM);
    const size_t per_group = sizeof(double) * (size_t)n * ((size_t)K + q);
    gc = (int)std::max<size_t>(1, std::min<size_t>((size_t)groups, np_t_cap() / per_group));
    size_t o = 0;
    auto take = [&](size_t count) { const size_t at = o; o += (count + 31) / 32 * 32; return at; };     // 256-byte pieces
    Z = take((size_t)n * s);
    p1 = take((size_t)nchunk * n);
    p2 = take((size_t)nchunk * n);
    pm = take((size_t)nchunk * NP_CM * n);
    fac = take((size_t)n);
    xx = take((size_t)n);
    Pm = take((size_t)npass * s * NP_CM);
    T = take(want_var ? (size_t)gc * ((size_t)K + q) * n : 0);
    total = o;
  }
};

}  // namespace flgp

static int np_rows_body(const char *who, hipStream_t st, const double *dX, int n, int ldx, int d, int dpad, const double *dUt,
                        const double *duu, const double *dU, int ldu, int s, double inv_c, const double *d_w, const double *d_P,
                        long ldp, int groups, int K, int q, const double *d_cg, double *d_mean, long ldm, double *d_var, long ldv,
                        void *d_work, size_t work_bytes);

extern "C" size_t flgp_dev_nystrom_predictor_workspace(int n, int s, int groups, int K, int q, int want_var) {
  if (n < 1 || s < 1 || groups < 1 || K < 1 || q < 0) return 0;
  return sizeof(double) * NpLayout(n, s, groups, K, q, want_var).total;
}

extern "C" int flgp_dev_nystrom_predictor_rows(void *stream, const double *dX, int n, int ldx, int d, const double *dUt,
                                               const double *duu, const double *dU, int ldu, int s, double inv_c, const double *d_w,
                                               const double *d_P, long ldp, int groups, int K, int q, const double *d_cg,
                                               double *d_mean, long ldm, double *d_var, long ldv, void *d_work, size_t work_bytes) {
  const char *who = "nystrom_predictor_rows";
  FLGP_REQUIRE(dX && dUt && duu && dU && d_w && d_P && d_work, "%s: null pointer", who);
  FLGP_REQUIRE(d_mean || d_var, "%s: null pointer (no output is wanted)", who);
  FLGP_REQUIRE(!d_var || d_cg, "%s: null pointer (the variance needs cg)", who);
  const int dpad = flgp_dev_anchor_dpad(d);
  FLGP_REQUIRE(dpad > 0 && d >= 1, "%s: kernels are built for 1 <= d <= %d (got %d)", who, FLGP_DMAX, d);
  FLGP_REQUIRE(n >= 1 && s >= 1 && groups >= 1 && K >= 1 && q >= 0, "%s: bad shape (n=%d, s=%d, groups=%d, K=%d, q=%d)", who, n, s,
               groups, K, q);
  FLGP_REQUIRE(!d_mean || q >= 1, "%s: a mean needs q >= 1 (q=%d)", who, q);
  FLGP_REQUIRE(inv_c > 0.0 && inv_c < HUGE_VAL, "%s: inv_c=%g must be positive and finite", who, inv_c);
  FLGP_REQUIRE(ldp >= (long)groups * ((long)K + q), "%s: ldp=%ld is below groups (K + q) = %ld", who, ldp,
               (long)groups * ((long)K + q));
  FLGP_REQUIRE(ldx >= n && ldu >= s && (!d_mean || ldm >= n) && (!d_var || ldv >= n),
               "%s: a leading dimension is too small (n=%d, s=%d)", who, n, s);
  FLGP_REQUIRE((long)groups * ((long)K + q) < (1L << 31) && (long)n * s < (1L << 40), "%s: the operand is too wide", who);
  return np_rows_body(who, (hipStream_t)stream, dX, n, ldx, d, dpad, dUt, duu, dU, ldu, s, inv_c, d_w, d_P, ldp, groups, K, q, d_cg, d_mean,
                      ldm, d_var, ldv, d_work, work_bytes);
}

// what follows the refusals; K = 0 is a P of mean columns alone (nystrom_mean_rows)
static int np_rows_body(const char *who, hipStream_t st, const double *dX, int n, int ldx, int d, int dpad, const double *dUt,
                        const double *duu, const double *dU, int ldu, int s, double inv_c, const double *d_w, const double *d_P,
                        long ldp, int groups, int K, int q, const double *d_cg, double *d_mean, long ldm, double *d_var, long ldv,
                        void *d_work, size_t work_bytes) {
  const NpLayout L(n, s, groups, K, q, d_var != nullptr);
  FLGP_REQUIRE(work_bytes >= sizeof(double) * L.total, "%s: the workspace holds %zu bytes, %zu are needed", who, work_bytes,
               sizeof(double) * L.total);
  double *W = (double *)d_work;
  double *Z = W + L.Z, *p1 = W + L.p1, *p2 = W + L.p2, *pm = W + L.pm, *fac = W + L.fac, *xx = W + L.xx, *Pm = W + L.Pm, *T = W + L.T;
  const int gq = d_mean ? groups * q : 0, npass = d_mean ? L.npass : 0, nchunk = L.nchunk, w = K + q;
  const bool want_var = d_var != nullptr, via_gemm = nys_dots_via_gemm(dpad);
  ProfScope ps("nystrom_predictor_rows", st,
               (double)n * s * (2.0 * dpad + 4.0 + 2.0 * gq) + (want_var ? 2.0 * (double)n * s * groups * w : 0.0));
  if (npass) {
    hipLaunchKernelGGL(np_pack_kernel, dim3(ceil_div((long)npass * s * NP_CM, 256)), dim3(256), 0, st, d_P, ldp, s, K, q, gq, npass, Pm);
    FLGP_TRY(check_launch("np_pack_kernel"));
  }
  const dim3 grid(ceil_div(n, 256), nchunk);
  // the first pass makes the row sums (and Z where it is wanted); a call without a mean is that pass without columns
  for (int pass = 0; pass < std::max(npass, 1); ++pass) {
    const double *Pp = Pm + (size_t)pass * s * NP_CM;
    const bool first = pass == 0, cols = npass > 0;
    if (via_gemm) {
      if (first) {
        hipLaunchKernelGGL(np_sqnorm_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, dX, n, ldx, d, xx);
        FLGP_TRY(check_launch("np_sqnorm_kernel"));
        // no workspace: the GEMM cannot split k, so every dot product is one whole chain (as nystrom_grid_extend's)
        FLGP_TRY(gemm_launch(st, n, s, d, 1.0, dX, 1, ldx, dU, ldu, 1, 0.0, nullptr, 0, 0, Z, 1, n, nullptr, 0, 0.0, nullptr));
        const bool keep = want_var || npass > 1;
#define NP_EXP(NCv, MODEv) hipLaunchKernelGGL((np_exp_rows_kernel<NCv, MODEv>), grid, dim3(256), 0, st, Z, n, s, xx, duu, inv_c, d_w, Pp, p1, p2, pm)
        if (cols && keep) NP_EXP(NP_CM, 1);
        else if (cols) NP_EXP(NP_CM, 0);
        else NP_EXP(0, 1);
      } else {
        NP_EXP(NP_CM, 2);
      }
#undef NP_EXP
      FLGP_TRY(check_launch("np_exp_rows_kernel"));
    } else if (first && want_var) {
      if (cols) FLGP_TRY((np_launch_sim<NP_CM, 1>(st, dpad, dX, n, ldx, d, dUt, duu, s, inv_c, d_w, Pp, Z, 1, p1, p2, pm)));
      else FLGP_TRY((np_launch_sim<0, 1>(st, dpad, dX, n, ldx, d, dUt, duu, s, inv_c, d_w, Pp, Z, 1, p1, p2, pm)));
    } else {
      FLGP_TRY((np_launch_sim<NP_CM, 0>(st, dpad, dX, n, ldx, d, dUt, duu, s, inv_c, d_w, Pp, Z, first ? 1 : 0, p1, p2, pm)));
    }
    const int nc = cols ? std::min(NP_CM, gq - pass * NP_CM) : 0;
    hipLaunchKernelGGL(np_finish_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, st, p1, p2, pm, nchunk, n, nc, first ? 1 : 0, fac,
                       cols ? d_mean + (long)pass * NP_CM * ldm : nullptr, ldm);
    FLGP_TRY(check_launch("np_finish_kernel"));
  }
  if (want_var) {
    for (int g0 = 0; g0 < groups; g0 += L.gc) {
      const int gc = std::min(L.gc, groups - g0);
      FLGP_TRY(gemm_launch(st, n, gc * w, s, 1.0, Z, 1, n, d_P + (long)g0 * w, ldp, 1, 0.0, nullptr, 0, 0, T, 1, n, nullptr, 0, 0.0,
                           nullptr));
      hipLaunchKernelGGL(np_var_kernel, dim3(ceil_div(n, 256), std::min(gc, 65535)), dim3(256), 0, st, T, n, K, w, gc, fac, d_cg + g0,
                         d_var + (long)g0 * ldv, ldv);
      FLGP_TRY(check_launch("np_var_kernel"));
    }
  }
  return FLGP_OK;
}

size_t flgp::nystrom_mean_workspace(int n, int s, int q) {
  if (n < 1 || s < 1 || q < 1) return 0;
  return sizeof(double) * NpLayout(n, s, 1, 0, q, 0).total;
}

int flgp::nystrom_mean_rows(hipStream_t st, const double *dX, int n, int ldx, int d, const double *dUt, const double *duu,
                            const double *dU, int ldu, int s, double inv_c, const double *d_w, const double *d_P, long ldp, int q,
                            double *d_mean, long ldm, void *d_work, size_t work_bytes) {
  const char *who = "nystrom_mean_rows";
  FLGP_REQUIRE(dX && dUt && duu && dU && d_w && d_P && d_mean && d_work, "%s: null pointer", who);
  const int dpad = flgp_dev_anchor_dpad(d);
  FLGP_REQUIRE(dpad > 0 && d >= 1, "%s: kernels are built for 1 <= d <= %d (got %d)", who, FLGP_DMAX, d);
  FLGP_REQUIRE(n >= 1 && s >= 1 && q >= 1 && ldp >= q && ldx >= n && ldu >= s && ldm >= n && (long)n * s < (1L << 40),
               "%s: bad shape (n=%d, s=%d, q=%d)", who, n, s, q);
  return np_rows_body(who, st, dX, n, ldx, d, dpad, dUt, duu, dU, ldu, s, inv_c, d_w, d_P, ldp, 1, 0, q, nullptr, d_mean, ldm, nullptr, 0,
                      d_work, work_bytes);
}

// ---- the columns-out route (f-23).  The workspace: the pieces of the variance route without a mean (NpLayout of one mean
// column, which is never packed), then T for a chunk of columns
namespace {
struct NpColsLayout {
  NpLayout L;
  size_t T, total;
  int cc;                                               // columns of T held at once
  NpColsLayout(int n, int s, int nc) : L(n, s, 1, 0, 1, 0) {
    const size_t cap = np_t_cap() / sizeof(double);
    cc = (int)std::max<size_t>(1, std::min<size_t>((size_t)nc, cap / (size_t)n));
    T = L.total;
    // cc n <= min(nc n, max(n, cap)), which grows with n: the workspace of a block holds every shorter block
    total = T + (std::min((size_t)nc * n, std::max((size_t)n, cap)) + 31) / 32 * 32;
  }
};
}  // namespace

size_t flgp::nystrom_cols_workspace(int n, int s, int nc) {
  if (n < 1 || s < 1 || nc < 1) return 0;
  return sizeof(double) * NpColsLayout(n, s, nc).total;
}

int flgp::nystrom_cols_rows(hipStream_t st, const double *dX, int n, int ldx, int d, const double *dUt, const double *duu,
                            const double *dU, int ldu, int s, double inv_c, const double *d_w, const double *d_P, long ldp, int c0,
                            int nc, double *d_out, long ldo, void *d_work, size_t work_bytes) {
  const char *who = "nystrom_cols_rows";
  FLGP_REQUIRE(dX && dUt && duu && dU && d_w && d_P && d_out && d_work, "%s: null pointer", who);
  const int dpad = flgp_dev_anchor_dpad(d);
  FLGP_REQUIRE(dpad > 0 && d >= 1, "%s: kernels are built for 1 <= d <= %d (got %d)", who, FLGP_DMAX, d);
  FLGP_REQUIRE(n >= 1 && s >= 1 && nc >= 1 && c0 >= 0 && (long)c0 + nc <= ldp && ldx >= n && ldu >= s && ldo >= n &&
                   (long)n * s < (1L << 40),
               "%s: bad shape (n=%d, s=%d, c0=%d, nc=%d)", who, n, s, c0, nc);
  const NpColsLayout C(n, s, nc);
  FLGP_REQUIRE(work_bytes >= sizeof(double) * C.total, "%s: the workspace holds %zu bytes, %zu are needed", who, work_bytes,
               sizeof(double) * C.total);
  const NpLayout &L = C.L;
  double *W = (double *)d_work;
  double *Z = W + L.Z, *p1 = W + L.p1, *p2 = W + L.p2, *pm = W + L.pm, *fac = W + L.fac, *xx = W + L.xx, *Pm = W + L.Pm, *T = W + C.T;
  ProfScope ps("nystrom_cols_rows", st, (double)n * s * (2.0 * dpad + 4.0 + 2.0 * nc));
  // Z and the row factor: the launches of the variance route where no mean is asked for
  if (nys_dots_via_gemm(dpad)) {
    hipLaunchKernelGGL(np_sqnorm_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, dX, n, ldx, d, xx);
    FLGP_TRY(check_launch("np_sqnorm_kernel"));
    FLGP_TRY(gemm_launch(st, n, s, d, 1.0, dX, 1, ldx, dU, ldu, 1, 0.0, nullptr, 0, 0, Z, 1, n, nullptr, 0, 0.0, nullptr));
    hipLaunchKernelGGL((np_exp_rows_kernel<0, 1>), dim3(ceil_div(n, 256), L.nchunk), dim3(256), 0, st, Z, n, s, xx, duu, inv_c, d_w, Pm, p1,
                       p2, pm);
    FLGP_TRY(check_launch("np_exp_rows_kernel"));
  } else {
    FLGP_TRY((np_launch_sim<0, 1>(st, dpad, dX, n, ldx, d, dUt, duu, s, inv_c, d_w, Pm, Z, 1, p1, p2, pm)));
  }
  hipLaunchKernelGGL(np_finish_kernel, dim3(ceil_div(n, 64)), dim3(64), 0, st, p1, p2, pm, L.nchunk, n, 0, 1, fac, (double *)nullptr,
                     (long)0);
  FLGP_TRY(check_launch("np_finish_kernel"));
  for (int b0 = 0; b0 < nc; b0 += C.cc) {
    const int bc = std::min(C.cc, nc - b0);
    FLGP_TRY(gemm_launch(st, n, bc, s, 1.0, Z, 1, n, d_P + c0 + b0, ldp, 1, 0.0, nullptr, 0, 0, T, 1, n, nullptr, 0, 0.0, nullptr));
    hipLaunchKernelGGL(np_scale_kernel, dim3(ceil_div(n, 256), std::min(bc, 65535)), dim3(256), 0, st, T, n, bc, fac,
                       d_out + (long)b0 * ldo, ldo);
    FLGP_TRY(check_launch("np_scale_kernel"));
  }
  return FLGP_OK;
}

// The row kernels of the fitted predictor (include/flgp_hip.h) and their flgp_dev_* entries: a served
// row's posterior z_i = a_i P from its r scaled anchor weights (predictor_rows_kernel), the Polya-Gamma handle's latent, pi, y
// and label (predictor_pg_rows_kernel) and the link on a latent that exists (pg_link_kernel).  predictor.hip holds the handle
// and the host routes that run them block by block.
#include "common.h"
#include <algorithm>

using namespace flgp;

namespace flgp {

// One wave per (row, group).  Lane l of column chunk c holds column j = 64 c + l of the group's K + q: z is the chain over
// a ascending, multiply then add, from 0.0.  A column j >= K is the mean's entry j - K.  For j < K the lane adds z^2 to its
// own sum, so lane l holds S_l = the squares of k = l, l + 64, l + 128, .. added in that order from 0.0 (0.0 where K <= l);
// then six butterfly steps S_l <- S_l + S_(l xor o), o = 32, 16, 8, 4, 2, 1, leave the same total in every lane and
// var = cg + S_0.  The order is a function of (K, k) alone, every term is a square, and nothing depends on the grid.
// The row's r (index, value) pairs sit in lanes 0 .. r-1 and are broadcast from there: they are wave-uniform, so a row of P
// is one coalesced load per chunk.
constexpr int PRED_WAVES = 4;
__global__ __launch_bounds__(PRED_WAVES * 64) void predictor_rows_kernel(const int *__restrict__ ell_idx,
                                                                          const double *__restrict__ ell_val, int n, int r,
                                                                          const double *__restrict__ P, long ldp, int groups,
                                                                          int K, int q, const double *__restrict__ cg,
                                                                          double *__restrict__ mean, long ldm,
                                                                          double *__restrict__ var, long ldv) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = K + q;
  // the columns a call needs: the mean's alone where var is skipped, the squares' alone where the mean is
  const int j_lo = var ? 0 : K, j_hi = mean ? w : K;
  const int c_lo = j_lo / 64, c_hi = (j_hi + 63) / 64;
  for (long i = (long)blockIdx.x * PRED_WAVES + wave; i < n; i += (long)gridDim.x * PRED_WAVES) {
    int my_idx = 0;
    double my_val = 0.0;
    if (lane < r) { my_idx = ell_idx[i * r + lane]; my_val = ell_val[i * r + lane]; }
    for (int g = blockIdx.y; g < groups; g += gridDim.y) {
      const double *__restrict__ Pg = P + (long)g * w;
      double sq = 0.0;
      for (int c = c_lo; c < c_hi; ++c) {
        const int j = c * 64 + lane;
        const bool on = j >= j_lo && j < j_hi;
        double z = 0.0;
        for (int a = 0; a < r; ++a) {           // every lane takes the broadcast; a lane past the columns loads nothing
          const long ja = __builtin_amdgcn_readlane(my_idx, a);
          const double va = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_val), a),
                                             __builtin_amdgcn_readlane(__double2loint(my_val), a));
          if (on) z = z + va * Pg[ja * ldp + j];
        }
        if (on) {
          if (j < K) sq = sq + z * z;
          else mean[((long)g * q + (j - K)) * ldm + i] = z;
        }
      }
      if (var) {
        for (int o = 32; o >= 1; o >>= 1) sq = sq + __shfl_xor(sq, o);
        if (lane == 0) var[(long)g * ldv + i] = cg[g] + sq;
      }
    }
  }
}

// The Polya-Gamma handle's rows (f-22): P holds the B mean columns alone, column b chain b.  One wave per row; lane l of
// chunk c owns chain b = 64 c + l: f is the chain over a ascending, multiply then add, from 0.0 (predictor_rows_kernel's
// mean column), pi = 1 / (1 + exp(-f)) and y = (pi > 0.5) are pg_pi_kernel's expressions.  label: every lane keeps the
// (largest pi, its first chain) of its own chunks -- a later chunk replaces only on a strictly larger value -- and six
// butterfly steps combine (value, chain) pairs: the larger value wins, at equal values the lower chain, so every lane ends
// with the first chain of maximal pi, pg_argmax_kernel's answer (a NaN is never larger; a NaN in chain 0 gives 0 as there).
// Any output may be nullptr; the exponential is skipped where f alone is wanted.
__global__ __launch_bounds__(PRED_WAVES * 64) void predictor_pg_rows_kernel(const int *__restrict__ ell_idx,
                                                                             const double *__restrict__ ell_val, int n, int r,
                                                                             const double *__restrict__ P, long ldp, int B,
                                                                             double *__restrict__ f, long ldf,
                                                                             double *__restrict__ pi, long ldpi,
                                                                             double *__restrict__ y, long ldy,
                                                                             double *__restrict__ label) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c_hi = (B + 63) / 64;
  const bool link = pi || y || label;
  for (long i = (long)blockIdx.x * PRED_WAVES + wave; i < n; i += (long)gridDim.x * PRED_WAVES) {
    int my_idx = 0;
    double my_val = 0.0;
    if (lane < r) { my_idx = ell_idx[i * r + lane]; my_val = ell_val[i * r + lane]; }
    double best = -1.0, first = 0.0;            // pi >= 0: any chain beats a lane without one
    int loc = 0x7fffffff;
    for (int c = 0; c < c_hi; ++c) {
      const int b = c * 64 + lane;
      const bool on = b < B;
      double z = 0.0;
      for (int a = 0; a < r; ++a) {
        const long ja = __builtin_amdgcn_readlane(my_idx, a);
        const double va = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_val), a),
                                           __builtin_amdgcn_readlane(__double2loint(my_val), a));
        if (on) z = z + va * P[ja * ldp + b];
      }
      if (on) {
        if (f) f[(long)b * ldf + i] = z;
        if (link) {
          const double v = 1.0 / (1.0 + exp(-z));
          if (pi) pi[(long)b * ldpi + i] = v;
          if (y) y[(long)b * ldy + i] = v > 0.5 ? 1.0 : 0.0;
          if (c == 0) first = v;
          if (v > best) { best = v; loc = b; }
        }
      }
    }
    if (label) {
      for (int o = 32; o >= 1; o >>= 1) {
        const double ob = __shfl_xor(best, o);
        const int ol = __shfl_xor(loc, o);
        if (ob > best || (ob == best && ol < loc)) { best = ob; loc = ol; }
      }
      if (lane == 0) label[i] = (first != first || loc == 0x7fffffff) ? 0.0 : (double)loc;
    }
  }
}

// the same three expressions on a latent that exists: a thread per row, the chains ascending (pg_argmax_kernel's loop)
__global__ void pg_link_kernel(long n, int B, const double *__restrict__ f, long ldf, double *__restrict__ pi, long ldpi,
                               double *__restrict__ y, long ldy, double *__restrict__ label) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double best = 0.0;
  int loc = 0;
  for (int b = 0; b < B; ++b) {
    const double v = 1.0 / (1.0 + exp(-f[(long)b * ldf + i]));
    if (pi) pi[(long)b * ldpi + i] = v;
    if (y) y[(long)b * ldy + i] = v > 0.5 ? 1.0 : 0.0;
    if (b == 0) best = v;
    else if (v > best) { best = v; loc = b; }
  }
  if (label) label[i] = (double)loc;
}

}  // namespace flgp

extern "C" int flgp_dev_predictor_pg_rows(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P,
                                          long ldp, int s, int B, double *d_f, long ldf, double *d_pi, long ldpi, double *d_y, long ldy,
                                          double *d_label) {
  const char *who = "predictor_pg_rows";
  FLGP_REQUIRE(d_ell_idx && d_ell_val && d_P, "%s: null pointer", who);
  FLGP_REQUIRE(d_f || d_pi || d_y || d_label, "%s: null pointer (no output is wanted)", who);
  FLGP_REQUIRE(n >= 1 && r >= 1 && r <= FLGP_RMAX && s >= 1 && B >= 1, "%s: bad shape (n=%d, r=%d, s=%d, B=%d)", who, n, r, s, B);
  FLGP_REQUIRE(ldp >= B, "%s: ldp=%ld is below B = %d", who, ldp, B);
  FLGP_REQUIRE((!d_f || ldf >= n) && (!d_pi || ldpi >= n) && (!d_y || ldy >= n), "%s: a leading dimension is below n = %d", who, n);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("predictor_pg_rows", st, 2.0 * (double)n * r * B);
  hipLaunchKernelGGL(predictor_pg_rows_kernel, dim3(std::min(ceil_div(n, PRED_WAVES), 1 << 20)), dim3(PRED_WAVES * 64), 0, st, d_ell_idx,
                     d_ell_val, n, r, d_P, ldp, B, d_f, ldf, d_pi, ldpi, d_y, ldy, d_label);
  return check_launch("predictor_pg_rows_kernel");
}

extern "C" int flgp_dev_pg_link(void *stream, const double *d_f, long ldf, int n, int B, double *d_pi, long ldpi, double *d_y, long ldy,
                                double *d_label) {
  const char *who = "pg_link";
  FLGP_REQUIRE(d_f, "%s: null pointer", who);
  FLGP_REQUIRE(d_pi || d_y || d_label, "%s: null pointer (no output is wanted)", who);
  FLGP_REQUIRE(n >= 1 && B >= 1, "%s: bad shape (n=%d, B=%d)", who, n, B);
  FLGP_REQUIRE(ldf >= n && (!d_pi || ldpi >= n) && (!d_y || ldy >= n), "%s: a leading dimension is below n = %d", who, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(pg_link_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, (long)n, B, d_f, ldf, d_pi, ldpi, d_y, ldy, d_label);
  return check_launch("pg_link_kernel");
}

extern "C" int flgp_dev_predictor_rows(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r,
                                       const double *d_P, long ldp, int s, int groups, int K, int q, const double *d_cg,
                                       double *d_mean, long ldm, double *d_var, long ldv) {
  const char *who = "predictor_rows";
  FLGP_REQUIRE(d_ell_idx && d_ell_val && d_P, "%s: null pointer", who);
  FLGP_REQUIRE(d_mean || d_var, "%s: null pointer (no output is wanted)", who);
  FLGP_REQUIRE(!d_var || d_cg, "%s: null pointer (the variance needs cg)", who);
  FLGP_REQUIRE(n >= 1 && r >= 1 && r <= FLGP_RMAX && s >= 1 && groups >= 1 && K >= 1 && q >= 0,
               "%s: bad shape (n=%d, r=%d, s=%d, groups=%d, K=%d, q=%d)", who, n, r, s, groups, K, q);
  FLGP_REQUIRE(!d_mean || q >= 1, "%s: a mean needs q >= 1 (q=%d)", who, q);
  FLGP_REQUIRE(ldp >= (long)groups * ((long)K + q), "%s: ldp=%ld is below groups (K + q) = %ld", who, ldp,
               (long)groups * ((long)K + q));
  FLGP_REQUIRE((!d_mean || ldm >= n) && (!d_var || ldv >= n), "%s: a leading dimension is below n = %d", who, n);
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps("predictor_rows", st, 2.0 * (double)n * r * groups * ((double)K + q));
  const dim3 grid(std::min(ceil_div(n, PRED_WAVES), 1 << 20), std::min(groups, 65535));
  hipLaunchKernelGGL(predictor_rows_kernel, grid, dim3(PRED_WAVES * 64), 0, st, d_ell_idx, d_ell_val, n, r, d_P, ldp, groups, K, q,
                     d_cg, d_mean, ldm, d_var, ldv);
  return check_launch("predictor_rows_kernel");
}

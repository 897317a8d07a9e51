// The fitted predictor (include/flgp_hip.h): a trained posterior folded into the anchor side of a fitted
// spectrum model once,
//   P = Bq Gp^T   (s x (K + q) per group),   Bq(j, k) = Vs(j, k) sqrt(n_fit) / sigma_k,   Gp = [G ; U^T],
// so that the posterior of a row that arrives later is z_i = a_i P on the row's r scaled anchor weights: its last q entries
// the mean, c plus the squares of its first K entries the variance.  No n_new x K array exists.  The trained operands come
// from the bodies of the entries the handle mirrors (eigenpair.hip: regression_operands, logit_operands); the row chain up
// to the weights is the model's (model.hip: model_rows).
// The same handle over one bandwidth of a Nystrom grid (f-21): the anchor side is the grid's pre-scaled eigenvectors V', the
// weights are dense and the row path is nystrom_predictor.hip's.
// A Polya-Gamma handle (f-22) keeps the B mean columns alone, P(:, b) = B u_b with u_b = L (V1^T w_b) of chain b (eigenpair.hip:
// pg_operands): a served row's latent is a_i P, its pi, y and label the link's (predictor_pg_rows_kernel, pg_link_kernel).
// The joint posterior of served rows (f-23): the K columns of a group are the features z_i, z_i . z_j the latent covariance of
// two rows, and a draws handle keeps P_draw(:, col) = P_mean(:, c) + P_K xi_col, mean columns alone, served like any mean
// (predictor_cols.hip: the wide row kernel, the normals and the fold; nystrom_predictor.hip: the columns-out route).
#include "common.h"
#include <algorithm>
#include <cmath>
#include <memory>

using namespace flgp;

struct flgp_predictor {
  const flgp_spectrum_model *model = nullptr;   // borrowed: a spectrum model, or
  const flgp_nystrom_grid *grid = nullptr;      // bandwidth gi of a Nystrom grid (f-21: dense weights, nystrom_predictor.hip)
  int gi = 0, s = 0, d = 0;
  DevBuf P, cg;                                 // s x ldp row-major, groups
  DevBuf xi;                                    // a draws handle (f-23): the normals, xi(k, col) at k q + col
  std::vector<int> iters;                       // logit: one count per group
  int K = 0, groups = 0, q = 0, kind = 0, device = 0;
  long ldp = 0;
  // a regression handle (f-24): the nugget and noise[0] it was created with, and whether its K columns are the covariance of
  // its mean ("same" noise, or the result of an update) -- what flgp_predictor_update conditions on
  double sigma = 0.0, noise0 = 0.0;
  bool consistent = false;
};

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

namespace {

// what a create entry checks about the model (not null: looked at first) and the pair after its mirrored entry's checks; the
// comparison of the values is the first device work
int check_model(const char *who, const flgp_spectrum_model *model, const flgp_eigenpair *ep) {
  FLGP_REQUIRE(ep->K == model->K, "%s: the pair has K = %d, the model K = %d", who, ep->K, model->K);
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == model->device && dev == ep->device, "%s: the model lives on device %d, the pair on device %d, the current device is %d",
               who, model->device, ep->device, dev);
  std::vector<double> a((size_t)ep->K), b((size_t)ep->K);
  FLGP_HIP(hipMemcpy(a.data(), ep->values.p, sizeof(double) * a.size(), hipMemcpyDeviceToHost));
  FLGP_HIP(hipMemcpy(b.data(), model->values.p, sizeof(double) * b.size(), hipMemcpyDeviceToHost));
  FLGP_REQUIRE(std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0,
               "%s: the pair's values are not the model's (a pair from another fit)", who);
  return FLGP_OK;
}

// The handle's P zeroed and the anchor side B (s x K, ld s) chosen: for a model Bq, written here; for a Nystrom grid the
// bandwidth's pre-scaled eigenvectors V', which carry every scaling already.  Then fold() per chunk of operands
struct Folder {
  flgp_predictor *h;
  DevBuf Bq;
  const double *B = nullptr;
  int shape(hipStream_t st, int s, int d, int device, int K, int groups, int q, int kind) {
    h->s = s; h->d = d; h->K = K; h->groups = groups; h->q = q; h->kind = kind; h->device = device;
    // a Polya-Gamma handle's P holds the q mean columns alone, and so does a draws handle's (f-23)
    const bool mean_only = kind == FLGP_PREDICTOR_PG || kind == FLGP_PREDICTOR_DRAWS;
    h->ldp = ((mean_only ? (long)q : (long)groups * (K + q)) + 15) / 16 * 16;
    FLGP_TRY(h->P.alloc(sizeof(double) * (size_t)s * h->ldp));
    FLGP_TRY(h->cg.alloc(sizeof(double) * (size_t)groups));
    FLGP_HIP(hipMemsetAsync(h->cg.p, 0, sizeof(double) * (size_t)groups, st));
    FLGP_HIP(hipMemsetAsync(h->P.p, 0, sizeof(double) * (size_t)s * h->ldp, st));
    return FLGP_OK;
  }
  int begin(hipStream_t st, const flgp_spectrum_model *model, int K, int groups, int q, int kind) {
    h->model = model;
    FLGP_TRY(shape(st, model->s, model->d, model->device, K, groups, q, kind));
    FLGP_TRY(Bq.alloc(sizeof(double) * (size_t)model->s * K));
    B = Bq.as<double>();
    return hk_rows_b(st, (const double *)model->V.p, model->s, model->s, (const double *)model->eig.p, K,
                     std::sqrt((double)model->n_fit), Bq.as<double>());
  }
  int begin(hipStream_t st, const flgp_nystrom_grid *grid, int i, int K, int groups, int q, int kind) {
    h->grid = grid; h->gi = i;
    B = grid->eigv_of(i);
    return shape(st, grid->s, grid->d, grid->device, K, groups, q, kind);
  }
  // groups [p0, p0 + S): P(:, g (K + q) + k') = sum_k Bq(:, k) G_g(k', k), P(:, g (K + q) + K + c) = sum_k Bq(:, k) U_g(k, c); no
  // workspace, so each element is one k-ascending chain
  int fold(hipStream_t st, int p0, int S, const double *G, long sg, const double *U, long su) {
    const int s = h->s, K = h->K, q = h->q;
    for (int a = 0; a < S; ++a) {
      double *Pg = h->P.as<double>() + (long)(p0 + a) * (K + q);
      FLGP_TRY(flgp_dev_gemm(st, s, K, K, 1.0, B, 1, s, G + a * sg, K, 1, 0.0, nullptr, 0, 0, Pg, h->ldp, 1, nullptr, 0));
      FLGP_TRY(flgp_dev_gemm(st, s, q, K, 1.0, B, 1, s, U + a * su, 1, K, 0.0, nullptr, 0, 0, Pg + K, h->ldp, 1, nullptr, 0));
    }
    return FLGP_OK;
  }
  // Polya-Gamma chains [p0, p0 + S): P(:, b) = sum_k B(:, k) u_b(k), a column per N = 1 product whatever shares the call
  int fold_pg(hipStream_t st, int p0, int S, const double *U, long su) {
    for (int a = 0; a < S; ++a)
      FLGP_TRY(flgp_dev_gemm(st, h->s, 1, h->K, 1.0, B, 1, h->s, U + a * su, 1, h->K, 0.0, nullptr, 0, 0, h->P.as<double>() + p0 + a,
                             h->ldp, 1, nullptr, 0));
    return FLGP_OK;
  }
};

int on_handle_device(const flgp_predictor *h, const char *who) {
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == h->device, "%s: the predictor lives on device %d, the current device is %d", who, h->device, dev);
  return FLGP_OK;
}

// rows [0, nb) of dX (ldx): the model's row chain up to the weights, then the row kernel; asynchronous on `st`
int apply_block(hipStream_t st, const flgp_predictor *h, ModelRowWork &W, const double *dX, int nb, int ldx, double *d_mean, long ldm,
                double *d_var, long ldv) {
  const flgp_spectrum_model *m = h->model;
  FLGP_TRY(model_rows(st, m, W, dX, nb, ldx));
  return flgp_dev_predictor_rows(st, W.ell_idx.as<int>(), W.ell_val.as<double>(), nb, m->r, (const double *)h->P.p, h->ldp, m->s, h->groups,
                                 h->K, h->q, (const double *)h->cg.p, d_mean, ldm, d_var, ldv);
}

// ---- a Nystrom handle (f-21): what create checks after the mirrored entry's checks, and the row blocks of apply
int check_grid(const char *who, const flgp_nystrom_grid *grid, int i, const flgp_eigenpair *ep) {
  FLGP_REQUIRE(ep->K == grid->K, "%s: the pair has K = %d, the grid K = %d", who, ep->K, grid->K);
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == grid->device && dev == ep->device, "%s: the grid lives on device %d, the pair on device %d, the current device is %d",
               who, grid->device, ep->device, dev);
  std::vector<double> a((size_t)ep->K), b((size_t)ep->K);
  FLGP_HIP(hipMemcpy(a.data(), ep->values.p, sizeof(double) * a.size(), hipMemcpyDeviceToHost));
  FLGP_HIP(hipMemcpy(b.data(), grid->values_of(i), sizeof(double) * b.size(), hipMemcpyDeviceToHost));
  FLGP_REQUIRE(std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0,
               "%s: the pair's values are not those of bandwidth %d (a pair from another bandwidth or grid)", who, i);
  return FLGP_OK;
}

// rows per block: min(R(1) of the extension, model_extend_block), and the workspace of one block
struct NystromRowWork {
  DevBuf work;
  size_t bytes = 0;
  int B = 0;
  int alloc(const flgp_predictor *h, int n_new, bool want_var) {
    B = std::min(nys_row_block(h->s, h->K, n_new), std::min(model_block_rows(), n_new));
    bytes = flgp_dev_nystrom_predictor_workspace(B, h->s, h->groups, h->K, h->q, want_var ? 1 : 0);
    return work.alloc(bytes);
  }
};
int nystrom_apply_block(hipStream_t st, const flgp_predictor *h, NystromRowWork &W, const double *dX, int nb, int ldx, double *d_mean,
                        long ldm, double *d_var, long ldv) {
  const flgp_nystrom_grid *G = h->grid;
  return flgp_dev_nystrom_predictor_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p,
                                         G->s, G->s, G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, h->groups, h->K,
                                         h->q, (const double *)h->cg.p, d_mean, ldm, d_var, ldv, W.work.p, W.bytes);
}

// The create entries: one body per kind of posterior, shared by the two kinds of handle.  `check` is what the handle refuses
// after the mirrored entry's checks (its last part the first device work), `begin` its Folder::begin.
template <class Check, class Begin>
int create_regression(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int q, double t,
                      const double *noise, int n_noise, double sigma, flgp_predictor **out, Check check, Begin begin) {
  FLGP_TRY(regression_operands_check(who, ep, K, idx0, m, Y, q, t, noise, n_noise, sigma));
  FLGP_TRY(check());
  Stream st;
  FLGP_TRY(st.create());
  std::unique_ptr<flgp_predictor> h(new flgp_predictor());
  Folder F{h.get()};
  FLGP_TRY(begin(F, st.s));
  const double c = noise[0] + sigma;
  h->sigma = sigma; h->noise0 = noise[0]; h->consistent = n_noise == 1;
  FLGP_TRY(h2d(h->cg.p, &c, sizeof(double), st.s));
  FLGP_TRY(regression_operands(st.s, who, ep, K, idx0, m, Y, q, t, noise, n_noise, sigma,
                               [&](int p0, int S, const double *G, long sg, const double *U, long su) {
                                 return F.fold(st.s, p0, S, G, sg, U, su);
                               }));
  FLGP_HIP(hipStreamSynchronize(st.s));
  *out = h.release();
  return FLGP_OK;
}

template <class Check, class Begin>
int create_logit(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol, const int *col,
                 const double *ts, int B, double sigma11, double sigma22, double tol, int max_iter, int max_parallel, int *iters,
                 flgp_predictor **out, Check check, Begin begin) {
  FLGP_TRY(logit_operands_check(who, ep, K, idx0, m, Y, ncol, col, ts, B, sigma11, sigma22, max_iter));
  FLGP_TRY(check());
  Stream st;
  FLGP_TRY(st.create());
  std::unique_ptr<flgp_predictor> h(new flgp_predictor());
  Folder F{h.get()};
  FLGP_TRY(begin(F, st.s));
  const std::vector<double> cg((size_t)B, sigma22);
  FLGP_TRY(h2d(h->cg.p, cg.data(), sizeof(double) * (size_t)B, st.s));
  h->iters.assign((size_t)B, 0);
  const int rc = logit_operands(st.s, who, ep, K, idx0, m, Y, ncol, col, ts, B, sigma11, tol, max_iter, max_parallel, h->iters.data(),
                                [&](int p0, int S, const double *G, long sg, const double *U, long su) {
                                  return F.fold(st.s, p0, S, G, sg, U, su);
                                });
  if (rc != FLGP_OK) { (void)hipStreamSynchronize(st.s); return rc; }
  FLGP_HIP(hipStreamSynchronize(st.s));
  if (iters) std::copy(h->iters.begin(), h->iters.end(), iters);
  *out = h.release();
  return FLGP_OK;
}

template <class Check, class Begin>
int create_pg(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol, const int *col,
              const double *ts, const unsigned long long *seeds, int B, double sigma, int n_sample, int max_parallel, double *omega_out,
              double *f_out, flgp_predictor **out, Check check, Begin begin) {
  FLGP_TRY(pg_operands_check(who, ep, K, idx0, m, Y, ncol, col, ts, seeds, B, sigma, n_sample));
  FLGP_TRY(check());
  Stream st;
  FLGP_TRY(st.create());
  std::unique_ptr<flgp_predictor> h(new flgp_predictor());
  Folder F{h.get()};
  FLGP_TRY(begin(F, st.s));
  const int rc = pg_operands(st.s, who, ep, K, idx0, m, Y, ncol, col, ts, seeds, B, sigma, n_sample, max_parallel, omega_out, f_out,
                             [&](hipStream_t ws, int p0, int S, const double *U, long su) { return F.fold_pg(ws, p0, S, U, su); });
  if (rc != FLGP_OK) { (void)hipStreamSynchronize(st.s); return rc; }
  FLGP_HIP(hipStreamSynchronize(st.s));
  *out = h.release();
  return FLGP_OK;
}

// ---- apply on a Polya-Gamma handle: the latent of a block, then the link
int pg_apply_block(hipStream_t st, const flgp_predictor *h, ModelRowWork &W, const double *dX, int nb, int ldx, double *d_f, long ldf,
                   double *d_pi, long ldpi, double *d_y, long ldy, double *d_label) {
  const flgp_spectrum_model *m = h->model;
  FLGP_TRY(model_rows(st, m, W, dX, nb, ldx));
  return flgp_dev_predictor_pg_rows(st, W.ell_idx.as<int>(), W.ell_val.as<double>(), nb, m->r, (const double *)h->P.p, h->ldp, m->s, h->q,
                                    d_f, ldf, d_pi, ldpi, d_y, ldy, d_label);
}
// a Nystrom handle: the mean-only route writes the block's latent (the caller's f, or `lat`: nb x q at ld nb), then the link
struct NystromPgWork {
  DevBuf work, lat;
  size_t bytes = 0;
  int B = 0;
  int alloc(const flgp_predictor *h, int n_new, bool own_latent) {
    B = std::min(nys_row_block(h->s, h->K, n_new), std::min(model_block_rows(), n_new));
    bytes = nystrom_mean_workspace(B, h->s, h->q);
    FLGP_TRY(work.alloc(bytes));
    return own_latent ? lat.alloc(sizeof(double) * (size_t)B * h->q) : FLGP_OK;
  }
};
int nystrom_pg_apply_block(hipStream_t st, const flgp_predictor *h, NystromPgWork &W, const double *dX, int nb, int ldx, double *d_f,
                           long ldf, double *d_pi, long ldpi, double *d_y, long ldy, double *d_label) {
  const flgp_nystrom_grid *G = h->grid;
  double *lat = d_f ? d_f : W.lat.as<double>();
  const long ldl = d_f ? ldf : nb;
  FLGP_TRY(nystrom_mean_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p, G->s, G->s,
                             G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, h->q, lat, ldl, W.work.p, W.bytes));
  if (!(d_pi || d_y || d_label)) return FLGP_OK;
  return flgp_dev_pg_link(st, lat, ldl, nb, h->q, d_pi, ldpi, d_y, ldy, d_label);
}

}  // namespace

extern "C" int flgp_predictor_pg_create(const flgp_spectrum_model *model, const flgp_eigenpair *ep, int K, const int *idx0, int m,
                                        const double *Y, int ncol, const int *col, const double *ts, const unsigned long long *seeds,
                                        int B, double sigma, int n_sample, int max_parallel, double *omega_out, double *f_out,
                                        flgp_predictor **out) {
  const char *who = "predictor_pg";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(model, "%s: null model", who);
  return create_pg(who, ep, K, idx0, m, Y, ncol, col, ts, seeds, B, sigma, n_sample, max_parallel, omega_out, f_out, out,
                   [&] { return check_model(who, model, ep); },
                   [&](Folder &F, hipStream_t st) { return F.begin(st, model, K, 1, B, FLGP_PREDICTOR_PG); });
}

extern "C" int flgp_predictor_nystrom_pg_create(const flgp_nystrom_grid *grid, int i, const flgp_eigenpair *ep, int K, const int *idx0,
                                                int m, const double *Y, int ncol, const int *col, const double *ts,
                                                const unsigned long long *seeds, int B, double sigma, int n_sample, int max_parallel,
                                                double *omega_out, double *f_out, flgp_predictor **out) {
  const char *who = "predictor_nystrom_pg";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(grid, "%s: null grid", who);
  FLGP_REQUIRE(i >= 0 && i < grid->l, "%s: bandwidth %d outside 0..%d", who, i, grid->l - 1);
  return create_pg(who, ep, K, idx0, m, Y, ncol, col, ts, seeds, B, sigma, n_sample, max_parallel, omega_out, f_out, out,
                   [&] { return check_grid(who, grid, i, ep); },
                   [&](Folder &F, hipStream_t st) { return F.begin(st, grid, i, K, 1, B, FLGP_PREDICTOR_PG); });
}

extern "C" int flgp_dev_predictor_pg_apply(void *stream, const flgp_predictor *h, const double *dX, int n_new, int ldx, double *d_f,
                                           long ldf, double *d_pi, long ldpi, double *d_y, long ldy, double *d_label) {
  const char *who = "predictor_pg_apply";
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(dX && (d_f || d_pi || d_y || d_label), "%s: null pointer", who);
  FLGP_REQUIRE(n_new >= 1, "%s: need n_new >= 1 (n_new=%d)", who, n_new);
  FLGP_REQUIRE(ldx >= n_new && (!d_f || ldf >= n_new) && (!d_pi || ldpi >= n_new) && (!d_y || ldy >= n_new),
               "%s: a leading dimension is below n_new = %d", who, n_new);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(h->kind == FLGP_PREDICTOR_PG, "%s: the handle is not a Polya-Gamma one (kind %d)", who, h->kind);
  FLGP_TRY(on_handle_device(h, who));
  auto at = [](double *p, long i0) { return p ? p + i0 : nullptr; };
  if (h->grid) {
    NystromPgWork W;
    FLGP_TRY(W.alloc(h, n_new, d_f == nullptr));
    for (long i0 = 0; i0 < n_new; i0 += W.B)
      FLGP_TRY(nystrom_pg_apply_block(st, h, W, dX + i0, (int)std::min<long>(W.B, n_new - i0), ldx, at(d_f, i0), ldf, at(d_pi, i0), ldpi,
                                      at(d_y, i0), ldy, at(d_label, i0)));
    FLGP_HIP(hipStreamSynchronize(st));
    return FLGP_OK;
  }
  const int B = std::min(model_block_rows(), n_new);
  ModelRowWork W;
  FLGP_TRY(W.alloc(h->model, B));
  for (long i0 = 0; i0 < n_new; i0 += B)
    FLGP_TRY(pg_apply_block(st, h, W, dX + i0, (int)std::min<long>(B, n_new - i0), ldx, at(d_f, i0), ldf, at(d_pi, i0), ldpi, at(d_y, i0),
                            ldy, at(d_label, i0)));
  FLGP_HIP(hipStreamSynchronize(st));     // (the workspaces die here)
  return FLGP_OK;
}

extern "C" int flgp_predictor_pg_apply(const flgp_predictor *h, const double *X, int n_new, double *f, double *pi, double *y,
                                       double *label) {
  const char *who = "predictor_pg_apply";
  FLGP_REQUIRE(X && (f || pi || y || label), "%s: null pointer", who);
  FLGP_REQUIRE(n_new >= 1, "%s: need n_new >= 1 (n_new=%d)", who, n_new);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(h->kind == FLGP_PREDICTOR_PG, "%s: the handle is not a Polya-Gamma one (kind %d)", who, h->kind);
  FLGP_TRY(on_handle_device(h, who));
  const flgp_spectrum_model *m = h->model;
  const int d = h->d, q = h->q;
  Stream st;
  FLGP_TRY(st.create());
  ModelRowWork W;
  NystromPgWork NW;
  DevBuf dX, df, dpi, dy, dlab;
  if (h->grid) FLGP_TRY(NW.alloc(h, n_new, f == nullptr));
  const int B = h->grid ? NW.B : std::min(model_block_rows(), n_new);
  if (m) FLGP_TRY(W.alloc(m, B));
  const size_t nq = sizeof(double) * (size_t)n_new * q;
  FLGP_TRY(dX.alloc(sizeof(double) * (size_t)B * d));
  if (f) FLGP_TRY(df.alloc(nq));
  if (pi) FLGP_TRY(dpi.alloc(nq));
  if (y) FLGP_TRY(dy.alloc(nq));
  if (label) FLGP_TRY(dlab.alloc(sizeof(double) * (size_t)n_new));
  auto at = [](DevBuf &b, bool want, long i0) { return want ? b.as<double>() + i0 : nullptr; };
  for (long i0 = 0; i0 < n_new; i0 += B) {
    const int nb = (int)std::min<long>(B, n_new - i0);
    FLGP_HIP(hipMemcpy2DAsync(dX.p, sizeof(double) * (size_t)nb, X + i0, sizeof(double) * (size_t)n_new, sizeof(double) * (size_t)nb, d,
                              hipMemcpyHostToDevice, st.s));
    FLGP_TRY(check_finite_on_device(st.s, dX.as<double>(), (long)nb * d, "points"));
    if (h->grid)
      FLGP_TRY(nystrom_pg_apply_block(st.s, h, NW, dX.as<double>(), nb, nb, at(df, f, i0), n_new, at(dpi, pi, i0), n_new, at(dy, y, i0),
                                      n_new, at(dlab, label, i0)));
    else
      FLGP_TRY(pg_apply_block(st.s, h, W, dX.as<double>(), nb, nb, at(df, f, i0), n_new, at(dpi, pi, i0), n_new, at(dy, y, i0), n_new,
                              at(dlab, label, i0)));
  }
  if (f) FLGP_TRY(d2h(f, df.p, nq, st.s));
  if (pi) FLGP_TRY(d2h(pi, dpi.p, nq, st.s));
  if (y) FLGP_TRY(d2h(y, dy.p, nq, st.s));
  if (label) FLGP_TRY(d2h(label, dlab.p, sizeof(double) * (size_t)n_new, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" int flgp_predictor_regression_create(const flgp_spectrum_model *model, const flgp_eigenpair *ep, int K, const int *idx0,
                                                int m, const double *Y, int q, double t, const double *noise, int n_noise,
                                                double sigma, flgp_predictor **out) {
  const char *who = "predictor_regression";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(model, "%s: null model", who);
  return create_regression(who, ep, K, idx0, m, Y, q, t, noise, n_noise, sigma, out, [&] { return check_model(who, model, ep); },
                           [&](Folder &F, hipStream_t st) { return F.begin(st, model, K, 1, q, FLGP_PREDICTOR_REGRESSION); });
}

extern "C" int flgp_predictor_logit_create(const flgp_spectrum_model *model, const flgp_eigenpair *ep, int K, const int *idx0, int m,
                                           const double *Y, int ncol, const int *col, const double *ts, int B, double sigma11,
                                           double sigma22, double tol, int max_iter, int max_parallel, int *iters,
                                           flgp_predictor **out) {
  const char *who = "predictor_logit";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(model, "%s: null model", who);
  return create_logit(who, ep, K, idx0, m, Y, ncol, col, ts, B, sigma11, sigma22, tol, max_iter, max_parallel, iters, out,
                      [&] { return check_model(who, model, ep); },
                      [&](Folder &F, hipStream_t st) { return F.begin(st, model, K, B, 1, FLGP_PREDICTOR_LOGIT); });
}

// the Nystrom creates: a null out, a null grid and the bandwidth index come before the mirrored entry's refusals
extern "C" int flgp_predictor_nystrom_regression_create(const flgp_nystrom_grid *grid, int i, const flgp_eigenpair *ep, int K,
                                                        const int *idx0, int m, const double *Y, int q, double t,
                                                        const double *noise, int n_noise, double sigma, flgp_predictor **out) {
  const char *who = "predictor_nystrom_regression";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(grid, "%s: null grid", who);
  FLGP_REQUIRE(i >= 0 && i < grid->l, "%s: bandwidth %d outside 0..%d", who, i, grid->l - 1);
  return create_regression(who, ep, K, idx0, m, Y, q, t, noise, n_noise, sigma, out, [&] { return check_grid(who, grid, i, ep); },
                           [&](Folder &F, hipStream_t st) { return F.begin(st, grid, i, K, 1, q, FLGP_PREDICTOR_REGRESSION); });
}

extern "C" int flgp_predictor_nystrom_logit_create(const flgp_nystrom_grid *grid, int i, const flgp_eigenpair *ep, int K,
                                                   const int *idx0, int m, const double *Y, int ncol, const int *col,
                                                   const double *ts, int B, double sigma11, double sigma22, double tol, int max_iter,
                                                   int max_parallel, int *iters, flgp_predictor **out) {
  const char *who = "predictor_nystrom_logit";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(grid, "%s: null grid", who);
  FLGP_REQUIRE(i >= 0 && i < grid->l, "%s: bandwidth %d outside 0..%d", who, i, grid->l - 1);
  return create_logit(who, ep, K, idx0, m, Y, ncol, col, ts, B, sigma11, sigma22, tol, max_iter, max_parallel, iters, out,
                      [&] { return check_grid(who, grid, i, ep); },
                      [&](Folder &F, hipStream_t st) { return F.begin(st, grid, i, K, B, 1, FLGP_PREDICTOR_LOGIT); });
}

// ---- f-23: columns [c0, c0 + nc) of z_i = a_i P (model) or f_i sum_j Z_ij P_j (Nystrom) for the rows of a block, as they are:
// the features of a regression / logit handle (the K columns of a group) and the draws of a draws handle (all of P_draw).
namespace {

bool has_covariance_operand(const flgp_predictor *h) {
  return h->kind == FLGP_PREDICTOR_REGRESSION || h->kind == FLGP_PREDICTOR_LOGIT;
}

// "<who>: <what> of <bytes> bytes does not fit 90 % of the <free> bytes free" (the memory query is the first device call)
int fits_free_memory(const char *who, const char *what, double bytes) {
  size_t free_b = 0, total_b = 0;
  FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
  FLGP_REQUIRE(bytes <= 0.9 * (double)free_b, "%s: %s of %.0f bytes does not fit 90 %% of the %zu bytes free", who, what, bytes, free_b);
  return FLGP_OK;
}

// the rows per block and the workspaces of one block.  `mean_route`: a Nystrom draws handle of at most 8 columns takes the
// mean-only route (nystrom_mean_rows); every other Nystrom call the columns-out route
struct ColsWork {
  ModelRowWork M;
  DevBuf nys;
  size_t nys_bytes = 0;
  int B = 0;
  bool mean_route = false;
  static int rows(const flgp_predictor *h, int n) {
    const int B = std::min(model_block_rows(), n);
    return h->grid ? std::min(nys_row_block(h->s, h->K, n), B) : B;
  }
  static size_t bytes(const flgp_predictor *h, int B, int nc, bool mean_route) {
    if (!h->grid) return (sizeof(int) + sizeof(double)) * (size_t)B * (size_t)(2 * h->model->r);
    return mean_route ? nystrom_mean_workspace(B, h->s, nc) : nystrom_cols_workspace(B, h->s, nc);
  }
  int alloc(const flgp_predictor *h, int n, int nc, bool mean) {
    B = rows(h, n);
    mean_route = mean;
    if (!h->grid) return M.alloc(h->model, B);
    nys_bytes = bytes(h, B, nc, mean);
    return nys.alloc(nys_bytes);
  }
};

int cols_block(hipStream_t st, const flgp_predictor *h, ColsWork &W, const double *dX, int nb, int ldx, int c0, int nc, double *d_out,
               long ldo) {
  if (!h->grid) {
    const flgp_spectrum_model *m = h->model;
    FLGP_TRY(model_rows(st, m, W.M, dX, nb, ldx));
    return flgp_dev_predictor_cols(st, W.M.ell_idx.as<int>(), W.M.ell_val.as<double>(), nb, m->r, (const double *)h->P.p, h->ldp, m->s, c0,
                                   nc, d_out, ldo);
  }
  const flgp_nystrom_grid *G = h->grid;
  if (W.mean_route) {      // a draws handle's whole P_draw: the mean-only route takes its columns from 0
    FLGP_REQUIRE(c0 == 0, "predictor: the mean-only route serves columns from 0 (c0=%d)", c0);
    return nystrom_mean_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p, G->s, G->s,
                             G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, nc, d_out, ldo, W.nys.p, W.nys_bytes);
  }
  return nystrom_cols_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p, G->s, G->s,
                           G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, c0, nc, d_out, ldo, W.nys.p, W.nys_bytes);
}

bool draws_mean_route(const flgp_predictor *h) { return h->grid && h->kind == FLGP_PREDICTOR_DRAWS && h->q <= 8; }

// device rows: block by block on `st`, which is synchronised before the workspaces die
int cols_from_device(const char *who, hipStream_t st, const flgp_predictor *h, const double *dX, int n, int ldx, int c0, int nc,
                     double *d_out, long ldo) {
  const bool mean = draws_mean_route(h);
  const int B = ColsWork::rows(h, n);
  FLGP_TRY(fits_free_memory(who, "the workspace of a row block", (double)ColsWork::bytes(h, B, nc, mean)));
  ColsWork W;
  FLGP_TRY(W.alloc(h, n, nc, mean));
  for (long i0 = 0; i0 < n; i0 += W.B)
    FLGP_TRY(cols_block(st, h, W, dX + i0, (int)std::min<long>(W.B, n - i0), ldx, c0, nc, d_out + i0, ldo));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// host rows: uploaded and screened block by block; the result stays on the device (d_out n x nc, ldo)
int cols_from_host(const char *who, hipStream_t st, const flgp_predictor *h, const double *X, int n, int c0, int nc, double *d_out,
                   long ldo) {
  const bool mean = draws_mean_route(h);
  const int B = ColsWork::rows(h, n), d = h->d;
  FLGP_TRY(fits_free_memory(who, "a row block and its workspace",
                            (double)ColsWork::bytes(h, B, nc, mean) + sizeof(double) * (double)B * d));
  ColsWork W;
  DevBuf dX;
  FLGP_TRY(W.alloc(h, n, nc, mean));
  FLGP_TRY(dX.alloc(sizeof(double) * (size_t)W.B * d));
  for (long i0 = 0; i0 < n; i0 += W.B) {
    const int nb = (int)std::min<long>(W.B, n - i0);
    FLGP_HIP(hipMemcpy2DAsync(dX.p, sizeof(double) * (size_t)nb, X + i0, sizeof(double) * (size_t)n, sizeof(double) * (size_t)nb, d,
                              hipMemcpyHostToDevice, st));
    FLGP_TRY(check_finite_on_device(st, dX.as<double>(), (long)nb * d, "points"));
    FLGP_TRY(cols_block(st, h, W, dX.as<double>(), nb, nb, c0, nc, d_out + i0, ldo));
  }
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// the same, down to the host (out n x nc column-major)
int cols_to_host(const char *who, const flgp_predictor *h, const double *X, int n, int c0, int nc, double *out) {
  const double bytes = sizeof(double) * (double)n * nc;
  FLGP_TRY(fits_free_memory(who, "the n x nc result", bytes));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf d_out;
  FLGP_TRY(d_out.alloc((size_t)bytes));
  FLGP_TRY(cols_from_host(who, st.s, h, X, n, c0, nc, d_out.as<double>(), n));
  FLGP_TRY(d2h(out, d_out.p, (size_t)bytes, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

// what features and covariance refuse about the handle, after their own pointers and shapes
int check_features(const char *who, const flgp_predictor *h, int g) {
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(has_covariance_operand(h), "%s: a handle of kind %d has no covariance operand", who, h->kind);
  FLGP_REQUIRE(g >= 0 && g < h->groups, "%s: group %d outside 0..%d", who, g, h->groups - 1);
  return on_handle_device(h, who);
}

}  // namespace

extern "C" int flgp_predictor_draws_create(const flgp_predictor *h, int S, unsigned long long seed, flgp_predictor **out) {
  const char *who = "predictor_draws";
  FLGP_REQUIRE(out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(has_covariance_operand(h), "%s: a handle of kind %d has no covariance operand", who, h->kind);
  FLGP_REQUIRE(S >= 1, "%s: need S >= 1 (S=%d)", who, S);
  const long ncol = (long)h->groups * h->q * S;
  FLGP_REQUIRE(ncol <= 0x7fffffffL - 15, "%s: groups q S = %ld columns overflow an int", who, ncol);
  FLGP_TRY(on_handle_device(h, who));
  const long ldd = (ncol + 15) / 16 * 16;
  FLGP_TRY(fits_free_memory(who, "P_draw and the normals", sizeof(double) * ((double)h->s * ldd + (double)h->K * ncol)));
  Stream st;
  FLGP_TRY(st.create());
  std::unique_ptr<flgp_predictor> o(new flgp_predictor());
  o->model = h->model; o->grid = h->grid; o->gi = h->gi;       // what h borrows, not h
  Folder F{o.get()};
  FLGP_TRY(F.shape(st.s, h->s, h->d, h->device, h->K, 1, (int)ncol, FLGP_PREDICTOR_DRAWS));
  FLGP_TRY(o->xi.alloc(sizeof(double) * (size_t)h->K * (size_t)ncol));
  FLGP_TRY(flgp_dev_predictor_draws_fold(st.s, (const double *)h->P.p, h->ldp, h->s, h->groups, h->K, h->q, S, seed, o->xi.as<double>(),
                                         o->P.as<double>(), o->ldp));
  FLGP_HIP(hipStreamSynchronize(st.s));
  *out = o.release();
  return FLGP_OK;
}

extern "C" int flgp_predictor_draws_normals(const flgp_predictor *h, double *xi) {
  const char *who = "predictor_draws_normals";
  FLGP_REQUIRE(xi, "%s: null pointer", who);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(h->kind == FLGP_PREDICTOR_DRAWS, "%s: the handle is not a draws one (kind %d)", who, h->kind);
  FLGP_TRY(on_handle_device(h, who));
  const size_t K = (size_t)h->K, ncol = (size_t)h->q;
  std::vector<double> rows(K * ncol);
  Stream st;
  FLGP_TRY(st.create());
  FLGP_TRY(d2h(rows.data(), h->xi.p, sizeof(double) * rows.size(), st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  for (size_t k = 0; k < K; ++k)
    for (size_t c = 0; c < ncol; ++c) xi[c * K + k] = rows[k * ncol + c];
  return FLGP_OK;
}

extern "C" int flgp_dev_predictor_features(void *stream, const flgp_predictor *h, int g, const double *dX, int n, int ldx, double *dZ,
                                           long ldz) {
  const char *who = "predictor_features";
  FLGP_REQUIRE(dX && dZ, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: need n >= 1 (n=%d)", who, n);
  FLGP_REQUIRE(ldx >= n && ldz >= n, "%s: a leading dimension is below n = %d", who, n);
  FLGP_TRY(check_features(who, h, g));
  return cols_from_device(who, (hipStream_t)stream, h, dX, n, ldx, g * (h->K + h->q), h->K, dZ, ldz);
}

extern "C" int flgp_predictor_features(const flgp_predictor *h, int g, const double *X, int n, double *Z) {
  const char *who = "predictor_features";
  FLGP_REQUIRE(X && Z, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: need n >= 1 (n=%d)", who, n);
  FLGP_TRY(check_features(who, h, g));
  return cols_to_host(who, h, X, n, g * (h->K + h->q), h->K, Z);
}

extern "C" int flgp_predictor_covariance(const flgp_predictor *h, int g, const double *Xa, int na, const double *Xb, int nb, double *C) {
  const char *who = "predictor_covariance";
  FLGP_REQUIRE(Xa && C, "%s: null pointer", who);
  FLGP_REQUIRE(na >= 1 && (!Xb || nb >= 1), "%s: need na >= 1 and nb >= 1 (na=%d, nb=%d)", who, na, nb);
  FLGP_TRY(check_features(who, h, g));
  if (!Xb) nb = na;
  const int K = h->K, c0 = g * (h->K + h->q);
  const double bytes = sizeof(double) * ((double)na * K + (Xb ? (double)nb * K : 0.0) + (double)na * nb);
  FLGP_TRY(fits_free_memory(who, "the features and the na x nb block", bytes));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf Za, Zb, dC;
  FLGP_TRY(Za.alloc(sizeof(double) * (size_t)na * K));
  FLGP_TRY(dC.alloc(sizeof(double) * (size_t)na * nb));
  FLGP_TRY(cols_from_host(who, st.s, h, Xa, na, c0, K, Za.as<double>(), na));
  if (Xb) {
    FLGP_TRY(Zb.alloc(sizeof(double) * (size_t)nb * K));
    FLGP_TRY(cols_from_host(who, st.s, h, Xb, nb, c0, K, Zb.as<double>(), nb));
  }
  const double *B = Xb ? Zb.as<double>() : Za.as<double>();
  FLGP_TRY(flgp_dev_gemm(st.s, na, nb, K, 1.0, Za.as<double>(), 1, na, B, nb, 1, 0.0, nullptr, 0, 0, dC.as<double>(), 1, na, nullptr, 0));
  if (!Xb) FLGP_TRY(sym_mirror(st.s, dC.as<double>(), na, na));
  FLGP_TRY(d2h(C, dC.p, sizeof(double) * (size_t)na * nb, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

// ---- f-24: a regression handle conditioned on newly labelled rows.  With f_i = mean_i + z_i . xi, xi ~ N(0, I_K), observing
// y_i = f_i + N(0, d_i) on n_b rows is a K x K problem in xi: M = I + sum_i z_i z_i^T / d_i = L L^T, xi* = M^-1 sum_i z_i
// (y_i - mean_i)^T / d_i, and the new handle is P_mean' = P_mean + P_K xi*, P_K' = P_K L^-T.  S = sum_i e_i e_i^T / d_i with
// e_i = [z_i ; y_i - mean_i] comes from predictor_update.hip; the fold is the pieces the creates run on.
namespace {

// refusals 1 to 3 of the update entries come before these; then the handle (4 to 7)
int update_check_handle(const char *who, const flgp_predictor *h) {
  FLGP_REQUIRE(h->kind != FLGP_PREDICTOR_LOGIT,
               "%s: a logit handle cannot be updated (a Laplace posterior is not closed under conditioning)", who);
  FLGP_REQUIRE(h->kind != FLGP_PREDICTOR_PG, "%s: a Polya-Gamma handle cannot be updated (it holds the chains' mean columns alone)", who);
  FLGP_REQUIRE(h->kind != FLGP_PREDICTOR_DRAWS,
               "%s: a draws handle cannot be updated (update the regression handle it was made from and make the draws again)", who);
  FLGP_REQUIRE(h->kind == FLGP_PREDICTOR_REGRESSION, "%s: the handle is not a regression one (kind %d)", who, h->kind);
  FLGP_REQUIRE(!h->grid, "%s: a Nystrom handle cannot be updated (only a handle over a spectrum model)", who);
  FLGP_REQUIRE(h->consistent,
               "%s: the handle was created with per-row noise: its variance operand is built at noise[0] and is not the covariance "
               "of its mean, so conditioning it is not a posterior of anything",
               who);
  return on_handle_device(h, who);
}

// w_i = 1 / (noise_i + sigma) on the host; noise NULL: the create's noise[0]
int update_weights(const char *who, const flgp_predictor *h, const double *noise, int n_noise, int n_b, std::vector<double> &w) {
  for (int a = 0; a < n_noise; ++a) {
    FLGP_REQUIRE(std::isfinite(noise[a]), "%s: noise[%d] must be finite", who, a);
    FLGP_REQUIRE(noise[a] + h->sigma > 0.0, "%s: noise[%d] + sigma must be positive", who, a);
  }
  w.resize((size_t)n_b);
  for (int i = 0; i < n_b; ++i) w[(size_t)i] = 1.0 / ((n_noise == 0 ? h->noise0 : noise[n_noise == 1 ? 0 : i]) + h->sigma);
  return FLGP_OK;
}

struct UpdateRun {
  const flgp_predictor *h;
  ModelRowWork M;
  DevBuf S, dW, part;
  int B = 0;                                    // rows per block: a multiple of the Gram kernel's chunk
  // the block: model_extend_block rounded down to a multiple of the chunk, at least one chunk -- any multiple gives the same chain
  static int rows(const flgp_predictor *) {
    const int gc = predictor_gram_chunk();
    return std::max(gc, model_block_rows() / gc * gc);
  }
  int begin(hipStream_t st, int n_b, const std::vector<double> &w) {
    const int Wd = h->K + h->q;
    B = rows(h);
    FLGP_TRY(M.alloc(h->model, std::min(B, n_b)));
    FLGP_TRY(S.alloc(sizeof(double) * (size_t)Wd * Wd));
    FLGP_TRY(part.alloc(predictor_gram_bytes(std::min(B, n_b), h->K, h->q)));
    FLGP_TRY(dW.alloc(sizeof(double) * (size_t)n_b));
    return h2d(dW.p, w.data(), sizeof(double) * (size_t)n_b, st);
  }
  // rows [i0, i0 + nb) of the call: dX their points (ldx), dY their responses (ldy)
  int block(hipStream_t st, long i0, const double *dX, int nb, int ldx, const double *dY, long ldy) {
    const flgp_spectrum_model *m = h->model;
    FLGP_TRY(model_rows(st, m, M, dX, nb, ldx));
    return predictor_gram(st, M.ell_idx.as<int>(), M.ell_val.as<double>(), nb, m->r, (const double *)h->P.p, h->ldp, h->K, h->q,
                          dW.as<double>() + i0, dY, ldy, S.as<double>(), h->K + h->q, part.as<double>(), i0 == 0);
  }
  // the fold; synchronises `st`
  int finish(hipStream_t st, const char *who, flgp_predictor **out) {
    const int K = h->K, q = h->q, s = h->s;
    const size_t wi = (size_t)32 * 64 * K;
    DevBuf Mk, R, Li, Tb, wt, flag;
    FLGP_TRY(Mk.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(R.alloc(sizeof(double) * (size_t)K * q));
    FLGP_TRY(Li.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(Tb.alloc(sizeof(double) * (size_t)64 * K));
    FLGP_TRY(wt.alloc(sizeof(double) * wi)); FLGP_TRY(flag.alloc(sizeof(int)));
    FLGP_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    std::unique_ptr<flgp_predictor> o(new flgp_predictor());
    o->model = h->model;                        // what h borrows, not h
    Folder F{o.get()};
    FLGP_TRY(F.shape(st, s, h->d, h->device, K, 1, q, FLGP_PREDICTOR_REGRESSION));
    o->sigma = h->sigma; o->noise0 = h->noise0; o->consistent = true;
    FLGP_HIP(hipMemcpyAsync(o->cg.p, h->cg.p, sizeof(double), hipMemcpyDeviceToDevice, st));
    FLGP_TRY(predictor_update_system(st, S.as<double>(), K, q, Mk.as<double>(), R.as<double>()));
    FLGP_TRY(chol_blocked(st, Mk.as<double>(), K, K, flag.as<int>()));
    FLGP_TRY(chol_trsv(st, Mk.as<double>(), K, K, R.as<double>(), K, q, 3, flag.as<int>()));              // xi*
    FLGP_TRY(tri_inverse(st, Mk.as<double>(), K, K, Li.as<double>(), K, Tb.as<double>(), wt.as<double>(), wi, flag.as<int>()));
    const double *Ph = (const double *)h->P.p;
    double *Po = o->P.as<double>();
    // P_K'(j, k') = sum_k P_K(j, k) Linv(k', k);  P_mean' = P_mean + P_K xi*: no workspace, each element one k-ascending chain
    FLGP_TRY(flgp_dev_gemm(st, s, K, K, 1.0, Ph, h->ldp, 1, Li.as<double>(), K, 1, 0.0, nullptr, 0, 0, Po, o->ldp, 1, nullptr, 0));
    FLGP_TRY(flgp_dev_gemm(st, s, q, K, 1.0, Ph, h->ldp, 1, R.as<double>(), 1, K, 1.0, Ph + K, h->ldp, 1, Po + K, o->ldp, 1, nullptr, 0));
    int bad = 0;
    FLGP_TRY(read_flag(st, flag.p, &bad));
    if (bad) {
      set_error("%s: I + Z^T D^-1 Z is not positive definite (pivot %d <= 0)", who, bad - 1);
      return FLGP_ERR_NOCONV;
    }
    *out = o.release();
    return FLGP_OK;
  }
};

// a non-finite response: the q columns of dY (ldy) on the device
int update_check_responses(hipStream_t st, const double *dY, long ldy, int n_b, int q) {
  for (int c = 0; c < q; ++c) FLGP_TRY(check_finite_on_device(st, dY + (long)c * ldy, n_b, "predictor_update: the responses Y"));
  return FLGP_OK;
}

}  // namespace

extern "C" int flgp_dev_predictor_update(void *stream, const flgp_predictor *h, const double *dX, int n_b, int ldx, const double *dY,
                                         long ldy, const double *d_noise, int n_noise, flgp_predictor **out) {
  const char *who = "predictor_update";
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(out, "%s: null pointer (out)", who);
  *out = nullptr;
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(dX && dY, "%s: null pointer", who);
  FLGP_REQUIRE(n_b >= 1, "%s: need n_b >= 1 (n_b=%d)", who, n_b);
  FLGP_REQUIRE(d_noise ? (n_noise == 1 || n_noise == n_b) : n_noise == 0,
               "%s: n_noise=%d must be 0 with a NULL noise, 1 or n_b=%d", who, n_noise, n_b);
  FLGP_REQUIRE(ldx >= n_b && ldy >= n_b, "%s: a leading dimension is below n_b = %d", who, n_b);
  FLGP_TRY(update_check_handle(who, h));
  std::vector<double> noise((size_t)n_noise), w;
  if (n_noise) {
    FLGP_TRY(d2h(noise.data(), d_noise, sizeof(double) * (size_t)n_noise, st));
    FLGP_HIP(hipStreamSynchronize(st));
  }
  FLGP_TRY(update_check_responses(st, dY, ldy, n_b, h->q));
  FLGP_TRY(update_weights(who, h, noise.data(), n_noise, n_b, w));
  UpdateRun U{h};
  FLGP_TRY(U.begin(st, n_b, w));
  int rc = FLGP_OK;
  for (long i0 = 0; i0 < n_b && rc == FLGP_OK; i0 += U.B)
    rc = U.block(st, i0, dX + i0, (int)std::min<long>(U.B, n_b - i0), ldx, dY + i0, ldy);
  if (rc == FLGP_OK) rc = U.finish(st, who, out);
  (void)hipStreamSynchronize(st);               // (the workspaces die here)
  return rc;
}

extern "C" int flgp_predictor_update(const flgp_predictor *h, const double *X, int n_b, const double *Y, const double *noise,
                                     int n_noise, flgp_predictor **out) {
  const char *who = "predictor_update";
  FLGP_REQUIRE(out, "%s: null pointer (out)", who);
  *out = nullptr;
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(X && Y, "%s: null pointer", who);
  FLGP_REQUIRE(n_b >= 1, "%s: need n_b >= 1 (n_b=%d)", who, n_b);
  FLGP_REQUIRE(noise ? (n_noise == 1 || n_noise == n_b) : n_noise == 0, "%s: n_noise=%d must be 0 with a NULL noise, 1 or n_b=%d", who,
               n_noise, n_b);
  FLGP_TRY(update_check_handle(who, h));
  const int d = h->d, q = h->q;
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dX, dY;
  FLGP_TRY(dY.alloc(sizeof(double) * (size_t)n_b * q));
  FLGP_TRY(h2d(dY.p, Y, sizeof(double) * (size_t)n_b * q, st.s));
  FLGP_TRY(update_check_responses(st.s, dY.as<double>(), n_b, n_b, q));
  std::vector<double> w;
  FLGP_TRY(update_weights(who, h, noise, n_noise, n_b, w));
  UpdateRun U{h};
  FLGP_TRY(U.begin(st.s, n_b, w));
  const int B = std::min(U.B, n_b);
  FLGP_TRY(dX.alloc(sizeof(double) * (size_t)B * d));
  int rc = FLGP_OK;
  for (long i0 = 0; i0 < n_b && rc == FLGP_OK; i0 += B) {
    const int nb = (int)std::min<long>(B, n_b - i0);
    FLGP_HIP(hipMemcpy2DAsync(dX.p, sizeof(double) * (size_t)nb, X + i0, sizeof(double) * (size_t)n_b, sizeof(double) * (size_t)nb, d,
                              hipMemcpyHostToDevice, st.s));
    rc = check_finite_on_device(st.s, dX.as<double>(), (long)nb * d, "points");
    if (rc == FLGP_OK) rc = U.block(st.s, i0, dX.as<double>(), nb, nb, dY.as<double>() + i0, n_b);
  }
  if (rc == FLGP_OK) rc = U.finish(st.s, who, out);
  (void)hipStreamSynchronize(st.s);
  return rc;
}

// ---- f-25: which rows to label next.  The pool's rows go through the model's row chain block by block into n x r arrays; the
// greedy loop (predictor_design.hip) runs once on them.
namespace {

// refusals 1 to 3 of the design entries come before these; then the handle (4 to 7), in update's words
int design_check_handle(const char *who, const flgp_predictor *h) {
  FLGP_REQUIRE(h->kind != FLGP_PREDICTOR_LOGIT,
               "%s: a logit handle has no design (the observation variance of a new label is not a constant)", who);
  FLGP_REQUIRE(h->kind != FLGP_PREDICTOR_PG, "%s: a Polya-Gamma handle has no design (it holds the chains' mean columns alone)", who);
  FLGP_REQUIRE(h->kind != FLGP_PREDICTOR_DRAWS, "%s: a draws handle has no design (design on the regression handle it was made from)", who);
  FLGP_REQUIRE(h->kind == FLGP_PREDICTOR_REGRESSION, "%s: the handle is not a regression one (kind %d)", who, h->kind);
  FLGP_REQUIRE(!h->grid, "%s: a Nystrom handle has no design (only a handle over a spectrum model)", who);
  FLGP_REQUIRE(h->consistent,
               "%s: the handle was created with per-row noise: its variance operand is built at noise[0] and is not the covariance "
               "of its mean, so the variance a design would reduce is not a posterior's",
               who);
  return on_handle_device(h, who);
}

// refusal 8: d = noise + sigma, noise NULL = the create's noise[0]
int design_variance(const char *who, const flgp_predictor *h, const double *noise, double *d) {
  const double nz = noise ? noise[0] : h->noise0;
  FLGP_REQUIRE(std::isfinite(nz), "%s: the noise must be finite", who);
  FLGP_REQUIRE(nz + h->sigma > 0.0, "%s: noise + sigma must be positive", who);
  *d = nz + h->sigma;
  return FLGP_OK;
}

struct DesignRun {
  const flgp_predictor *h;
  ModelRowWork M;
  DevBuf idx, val, work;
  int n = 0, Bd = 0, blk = 0;
  size_t work_bytes = 0;
  // the pool's rows, the workspace and the row chain's block, against the free memory; `extra`: what the entry holds besides
  int begin(const char *who, int n_, int B, double extra) {
    const flgp_spectrum_model *m = h->model;
    n = n_; Bd = B;
    blk = std::min(model_block_rows(), n);
    work_bytes = predictor_design_bytes(n, m->r, h->s, h->K, B);
    FLGP_REQUIRE(work_bytes > 0, "%s: bad shape (n=%d, r=%d, s=%d, K=%d, B=%d)", who, n, m->r, h->s, h->K, B);
    const double rows = (sizeof(int) + sizeof(double)) * (double)n * m->r;
    const double chain = (sizeof(int) + sizeof(double)) * (double)blk * (2.0 * m->r);
    size_t free_b = 0, total_b = 0;
    FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
    FLGP_REQUIRE(rows + (double)work_bytes + chain + extra <= 0.9 * (double)free_b,
                 "%s: the pool's rows of %.0f bytes and the workspace of %zu bytes (n=%d, B=%d) do not fit 90 %% of the %zu bytes free", who,
                 rows + chain + extra, work_bytes, n, B, free_b);
    FLGP_TRY(M.alloc(m, blk));
    FLGP_TRY(idx.alloc(sizeof(int) * (size_t)n * m->r));
    FLGP_TRY(val.alloc(sizeof(double) * (size_t)n * m->r));
    return work.alloc(work_bytes);
  }
  // rows [i0, i0 + nb) of the call: dX their points (ldx)
  int block(hipStream_t st, long i0, const double *dX, int nb, int ldx) {
    const flgp_spectrum_model *m = h->model;
    FLGP_TRY(model_rows(st, m, M, dX, nb, ldx));
    FLGP_HIP(hipMemcpyAsync(idx.as<int>() + i0 * m->r, M.ell_idx.p, sizeof(int) * (size_t)nb * m->r, hipMemcpyDeviceToDevice, st));
    FLGP_HIP(hipMemcpyAsync(val.as<double>() + i0 * m->r, M.ell_val.p, sizeof(double) * (size_t)nb * m->r, hipMemcpyDeviceToDevice, st));
    return FLGP_OK;
  }
  int loop(hipStream_t st, double d, int *d_picks, double *d_gain, double *d_score) {
    return predictor_design_rows(st, idx.as<int>(), val.as<double>(), n, h->model->r, (const double *)h->P.p, h->ldp, h->s, h->K, d, Bd,
                                 d_picks, d_gain, d_score, work.p);
  }
};

}  // namespace

extern "C" int flgp_dev_predictor_design(void *stream, const flgp_predictor *h, const double *dX, int n, int ldx, int B,
                                         const double *noise, int *d_picks, double *d_gain, double *d_score) {
  const char *who = "predictor_design";
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(d_picks, "%s: null pointer (picks)", who);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(dX, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: need n >= 1 (n=%d)", who, n);
  FLGP_REQUIRE(B >= 1 && B <= n, "%s: need 1 <= B <= n (B=%d, n=%d)", who, B, n);
  FLGP_REQUIRE(ldx >= n, "%s: a leading dimension is below n = %d", who, n);
  FLGP_TRY(design_check_handle(who, h));
  double d = 0.0;
  FLGP_TRY(design_variance(who, h, noise, &d));
  DesignRun R{h};
  FLGP_TRY(R.begin(who, n, B, 0.0));
  int rc = FLGP_OK;
  for (long i0 = 0; i0 < n && rc == FLGP_OK; i0 += R.blk) rc = R.block(st, i0, dX + i0, (int)std::min<long>(R.blk, n - i0), ldx);
  if (rc == FLGP_OK) rc = R.loop(st, d, d_picks, d_gain, d_score);
  (void)hipStreamSynchronize(st);               // (the workspaces die here)
  return rc;
}

extern "C" int flgp_predictor_design(const flgp_predictor *h, const double *X, int n, int B, const double *noise, int *picks,
                                     double *gain, double *score) {
  const char *who = "predictor_design";
  FLGP_REQUIRE(picks, "%s: null pointer (picks)", who);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(X, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: need n >= 1 (n=%d)", who, n);
  FLGP_REQUIRE(B >= 1 && B <= n, "%s: need 1 <= B <= n (B=%d, n=%d)", who, B, n);
  FLGP_TRY(design_check_handle(who, h));
  double d = 0.0;
  FLGP_TRY(design_variance(who, h, noise, &d));
  const int dim = h->d;
  Stream st;
  FLGP_TRY(st.create());
  DesignRun R{h};
  const double out_bytes = sizeof(int) * (double)B + sizeof(double) * ((double)B + n);
  FLGP_TRY(R.begin(who, n, B, out_bytes + sizeof(double) * (double)std::min(model_block_rows(), n) * dim));
  DevBuf dX, d_picks, d_gain, d_score;
  FLGP_TRY(dX.alloc(sizeof(double) * (size_t)R.blk * dim));
  FLGP_TRY(d_picks.alloc(sizeof(int) * (size_t)B));
  if (gain) FLGP_TRY(d_gain.alloc(sizeof(double) * (size_t)B));
  if (score) FLGP_TRY(d_score.alloc(sizeof(double) * (size_t)n));
  int rc = FLGP_OK;
  for (long i0 = 0; i0 < n && rc == FLGP_OK; i0 += R.blk) {
    const int nb = (int)std::min<long>(R.blk, n - i0);
    FLGP_HIP(hipMemcpy2DAsync(dX.p, sizeof(double) * (size_t)nb, X + i0, sizeof(double) * (size_t)n, sizeof(double) * (size_t)nb, dim,
                              hipMemcpyHostToDevice, st.s));
    rc = check_finite_on_device(st.s, dX.as<double>(), (long)nb * dim, "points");
    if (rc == FLGP_OK) rc = R.block(st.s, i0, dX.as<double>(), nb, nb);
  }
  if (rc == FLGP_OK) rc = R.loop(st.s, d, d_picks.as<int>(), gain ? d_gain.as<double>() : nullptr, score ? d_score.as<double>() : nullptr);
  if (rc == FLGP_OK) rc = d2h(picks, d_picks.p, sizeof(int) * (size_t)B, st.s);
  if (rc == FLGP_OK && gain) rc = d2h(gain, d_gain.p, sizeof(double) * (size_t)B, st.s);
  if (rc == FLGP_OK && score) rc = d2h(score, d_score.p, sizeof(double) * (size_t)n, st.s);
  (void)hipStreamSynchronize(st.s);
  return rc;
}

extern "C" int flgp_predictor_dims(const flgp_predictor *h, int *d, int *s, int *r, int *K, int *groups, int *q, int *kind, long *ldp) {
  FLGP_REQUIRE(h, "predictor_dims: null handle");
  if (d) *d = h->d;
  if (s) *s = h->s;
  if (r) *r = h->model ? h->model->r : 0;     // a Nystrom handle's weights are dense
  if (K) *K = h->K;
  if (groups) *groups = h->groups;
  if (q) *q = h->q;
  if (kind) *kind = h->kind;
  if (ldp) *ldp = h->ldp;
  return FLGP_OK;
}

extern "C" int flgp_predictor_to_host(const flgp_predictor *h, double *P, double *cg) {
  FLGP_REQUIRE(h, "predictor_to_host: null handle");
  FLGP_TRY(on_handle_device(h, "predictor_to_host"));
  Stream st;
  FLGP_TRY(st.create());
  if (P) FLGP_TRY(d2h(P, h->P.p, sizeof(double) * (size_t)h->s * h->ldp, st.s));
  if (cg) FLGP_TRY(d2h(cg, h->cg.p, sizeof(double) * (size_t)h->groups, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" int flgp_dev_predictor_apply(void *stream, const flgp_predictor *h, const double *dX, int n_new, int ldx, double *d_mean,
                                        long ldm, double *d_var, long ldv) {
  const char *who = "predictor_apply";
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(dX && (d_mean || d_var), "%s: null pointer", who);
  FLGP_REQUIRE(n_new >= 1, "%s: need n_new >= 1 (n_new=%d)", who, n_new);
  FLGP_REQUIRE(ldx >= n_new && (!d_mean || ldm >= n_new) && (!d_var || ldv >= n_new), "%s: a leading dimension is below n_new = %d", who,
               n_new);
  FLGP_REQUIRE(h, "%s: null handle", who);
  if (h->kind == FLGP_PREDICTOR_PG) {
    FLGP_REQUIRE(!d_var, "%s: a Polya-Gamma handle has no variance", who);
    return flgp_dev_predictor_pg_apply(stream, h, dX, n_new, ldx, d_mean, ldm, nullptr, 0, nullptr, 0, nullptr);
  }
  if (h->kind == FLGP_PREDICTOR_DRAWS) {
    FLGP_REQUIRE(!d_var, "%s: a draws handle has no variance", who);
    FLGP_TRY(on_handle_device(h, who));
    return cols_from_device(who, st, h, dX, n_new, ldx, 0, h->q, d_mean, ldm);
  }
  FLGP_TRY(on_handle_device(h, who));
  if (h->grid) {
    NystromRowWork W;
    FLGP_TRY(W.alloc(h, n_new, d_var != nullptr));
    for (long i0 = 0; i0 < n_new; i0 += W.B)
      FLGP_TRY(nystrom_apply_block(st, h, W, dX + i0, (int)std::min<long>(W.B, n_new - i0), ldx, d_mean ? d_mean + i0 : nullptr, ldm,
                                   d_var ? d_var + i0 : nullptr, ldv));
    FLGP_HIP(hipStreamSynchronize(st));
    return FLGP_OK;
  }
  const int B = std::min(model_block_rows(), n_new);
  ModelRowWork W;
  FLGP_TRY(W.alloc(h->model, B));
  for (long i0 = 0; i0 < n_new; i0 += B)
    FLGP_TRY(apply_block(st, h, W, dX + i0, (int)std::min<long>(B, n_new - i0), ldx, d_mean ? d_mean + i0 : nullptr, ldm,
                         d_var ? d_var + i0 : nullptr, ldv));
  FLGP_HIP(hipStreamSynchronize(st));     // (the workspaces die here)
  return FLGP_OK;
}

extern "C" int flgp_predictor_apply(const flgp_predictor *h, const double *X, int n_new, double *mean, double *var) {
  const char *who = "predictor_apply";
  FLGP_REQUIRE(X && (mean || var), "%s: null pointer", who);
  FLGP_REQUIRE(n_new >= 1, "%s: need n_new >= 1 (n_new=%d)", who, n_new);
  FLGP_REQUIRE(h, "%s: null handle", who);
  if (h->kind == FLGP_PREDICTOR_PG) {
    FLGP_REQUIRE(!var, "%s: a Polya-Gamma handle has no variance", who);
    return flgp_predictor_pg_apply(h, X, n_new, mean, nullptr, nullptr, nullptr);
  }
  if (h->kind == FLGP_PREDICTOR_DRAWS) {
    FLGP_REQUIRE(!var, "%s: a draws handle has no variance", who);
    FLGP_TRY(on_handle_device(h, who));
    return cols_to_host(who, h, X, n_new, 0, h->q, mean);
  }
  FLGP_TRY(on_handle_device(h, who));
  const flgp_spectrum_model *m = h->model;
  const int d = h->d, gq = h->groups * h->q;
  Stream st;
  FLGP_TRY(st.create());
  ModelRowWork W;
  NystromRowWork NW;
  DevBuf dX, dmean, dvar;
  if (h->grid) FLGP_TRY(NW.alloc(h, n_new, var != nullptr));
  const int B = h->grid ? NW.B : std::min(model_block_rows(), n_new);
  if (m) FLGP_TRY(W.alloc(m, B));
  FLGP_TRY(dX.alloc(sizeof(double) * (size_t)B * d));
  if (mean) FLGP_TRY(dmean.alloc(sizeof(double) * (size_t)n_new * gq));
  if (var) FLGP_TRY(dvar.alloc(sizeof(double) * (size_t)n_new * h->groups));
  for (long i0 = 0; i0 < n_new; i0 += B) {
    const int nb = (int)std::min<long>(B, n_new - i0);
    FLGP_HIP(hipMemcpy2DAsync(dX.p, sizeof(double) * (size_t)nb, X + i0, sizeof(double) * (size_t)n_new, sizeof(double) * (size_t)nb, d,
                              hipMemcpyHostToDevice, st.s));
    FLGP_TRY(check_finite_on_device(st.s, dX.as<double>(), (long)nb * d, "points"));
    if (h->grid)
      FLGP_TRY(nystrom_apply_block(st.s, h, NW, dX.as<double>(), nb, nb, mean ? dmean.as<double>() + i0 : nullptr, n_new,
                                   var ? dvar.as<double>() + i0 : nullptr, n_new));
    else
      FLGP_TRY(apply_block(st.s, h, W, dX.as<double>(), nb, nb, mean ? dmean.as<double>() + i0 : nullptr, n_new,
                           var ? dvar.as<double>() + i0 : nullptr, n_new));
  }
  if (mean) FLGP_TRY(d2h(mean, dmean.p, sizeof(double) * (size_t)n_new * gq, st.s));
  if (var) FLGP_TRY(d2h(var, dvar.p, sizeof(double) * (size_t)n_new * h->groups, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" void flgp_predictor_free(flgp_predictor *h) { delete h; }

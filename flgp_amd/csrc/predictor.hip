// The fitted predictor (include/flgp_hip.h): a trained posterior folded into the anchor side of a fitted
// spectrum model once,
//   P = Bq Gp^T   (s x (K + q) per group),   Bq(j, k) = Vs(j, k) sqrt(n_fit) / sigma_k,   Gp = [G ; U^T],
// so that the posterior of a row that arrives later is z_i = a_i P on the row's r scaled anchor weights: its last q entries
// the mean, c plus the squares of its first K entries the variance.  No n_new x K array exists.  The trained operands come
// from the bodies of the entries the handle mirrors (eigenpair_regression.hip: regression_operands; eigenpair_logit.hip: logit_operands); the row chain up
// to the weights is the model's (model.hip: model_rows); the row kernels are predictor_rows.hip's.
// The same handle over one bandwidth of a Nystrom grid (f-21): the anchor side is the grid's pre-scaled eigenvectors V', the
// weights are dense and the row path is nystrom_predictor.hip's.
// A Polya-Gamma handle (f-22) keeps the B mean columns alone, P(:, b) = B u_b with u_b = L (V1^T w_b) of chain b (eigenpair_pg.hip:
// pg_operands): a served row's latent is a_i P, its pi, y and label the link's (predictor_rows.hip: predictor_pg_rows_kernel,
// pg_link_kernel).
// The joint posterior of served rows (f-23): the K columns of a group are the features z_i, z_i . z_j the latent covariance of
// two rows, and a draws handle keeps P_draw(:, col) = P_mean(:, c) + P_K xi_col, mean columns alone, served like any mean
// (predictor_cols.hip: the wide row kernel, the normals and the fold; nystrom_predictor.hip: the columns-out route).
// This file holds the handle and the host routes.  Every entry over served rows is one walk of common.h's for_row_blocks with
// its block body over a RowWork; its host and its device entry share that walk and one argument check.
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

namespace {

// whether the pair's K values are the K device values at d_values, bit for bit: the first device work of a create
int same_values(const flgp_eigenpair *ep, const double *d_values, bool &same) {
  std::vector<double> a((size_t)ep->K), b((size_t)ep->K);
  FLGP_HIP(hipMemcpy(a.data(), ep->values.p, sizeof(double) * a.size(), hipMemcpyDeviceToHost));
  FLGP_HIP(hipMemcpy(b.data(), d_values, sizeof(double) * b.size(), hipMemcpyDeviceToHost));
  same = std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0;
  return FLGP_OK;
}

// what a create entry checks about the model (not null: looked at first) and the pair after its mirrored entry's checks
int check_model(const char *who, const flgp_spectrum_model *model, const flgp_eigenpair *ep) {
  FLGP_REQUIRE(ep->K == model->K, "%s: the pair has K = %d, the model K = %d", who, ep->K, model->K);
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == model->device && dev == ep->device, "%s: the model lives on device %d, the pair on device %d, the current device is %d",
               who, model->device, ep->device, dev);
  bool same = false;
  FLGP_TRY(same_values(ep, (const double *)model->values.p, same));
  FLGP_REQUIRE(same, "%s: the pair's values are not the model's (a pair from another fit)", who);
  return FLGP_OK;
}

// the same about bandwidth i of a Nystrom grid (f-21)
int check_grid(const char *who, const flgp_nystrom_grid *grid, int i, const flgp_eigenpair *ep) {
  FLGP_REQUIRE(ep->K == grid->K, "%s: the pair has K = %d, the grid K = %d", who, ep->K, grid->K);
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == grid->device && dev == ep->device, "%s: the grid lives on device %d, the pair on device %d, the current device is %d",
               who, grid->device, ep->device, dev);
  bool same = false;
  FLGP_TRY(same_values(ep, grid->values_of(i), same));
  FLGP_REQUIRE(same, "%s: the pair's values are not those of bandwidth %d (a pair from another bandwidth or grid)", who, i);
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

// What serving a block of rows takes from a handle: the rows per block, the block's workspaces and the way from a block's
// points to the operands of its row kernel -- for a model handle the row chain up to the weights (ell), for a Nystrom handle
// the grid's anchor side in front of the three row routes of nystrom_predictor.hip.
struct RowWork {
  const flgp_predictor *h;
  ModelRowWork M;
  DevBuf nys, lat;                              // a Nystrom block's workspace; the PG route's own latent (nb x q at ld nb)
  size_t nys_bytes = 0;
  // rows per block: model_extend_block, and for a Nystrom handle R(1) of the extension where that is smaller
  int rows(int n) const {
    const int B = std::min(model_block_rows(), n);
    return h->grid ? std::min(nys_row_block(h->s, h->K, n), B) : B;
  }
  // update's block: model_extend_block rounded down to a multiple of the Gram kernel's chunk, at least one chunk -- any
  // multiple gives the same chain
  static int update_rows() {
    const int gc = predictor_gram_chunk();
    return std::max(gc, model_block_rows() / gc * gc);
  }
  // a block of at most B rows: the row chain's workspaces of a model handle; `bytes` for the route a Nystrom handle is served by
  int alloc(int B, size_t bytes = 0, bool own_latent = false) {
    if (!h->grid) return M.alloc(h->model, B);
    nys_bytes = bytes;
    FLGP_TRY(nys.alloc(bytes));
    return own_latent ? lat.alloc(sizeof(double) * (size_t)B * h->q) : FLGP_OK;
  }
  // rows [0, nb) of dX (ldx) through the model's row chain: their weights (nb x r); asynchronous on `st`
  int ell(hipStream_t st, const double *dX, int nb, int ldx, const int *&idx, const double *&val) {
    FLGP_TRY(model_rows(st, h->model, M, dX, nb, ldx));
    idx = M.ell_idx.as<int>();
    val = M.ell_val.as<double>();
    return FLGP_OK;
  }
  int nystrom_rows(hipStream_t st, const double *dX, int nb, int ldx, double *d_mean, long ldm, double *d_var, long ldv) {
    const flgp_nystrom_grid *G = h->grid;
    return flgp_dev_nystrom_predictor_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p,
                                           G->s, G->s, G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, h->groups, h->K,
                                           h->q, (const double *)h->cg.p, d_mean, ldm, d_var, ldv, nys.p, nys_bytes);
  }
  int nystrom_mean(hipStream_t st, const double *dX, int nb, int ldx, int nc, double *d_out, long ldo) {
    const flgp_nystrom_grid *G = h->grid;
    return nystrom_mean_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p, G->s, G->s,
                             G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, nc, d_out, ldo, nys.p, nys_bytes);
  }
  int nystrom_cols(hipStream_t st, const double *dX, int nb, int ldx, int c0, int nc, double *d_out, long ldo) {
    const flgp_nystrom_grid *G = h->grid;
    return nystrom_cols_rows(st, dX, nb, ldx, G->d, (const double *)G->Ut.p, (const double *)G->uu.p, (const double *)G->U.p, G->s, G->s,
                             G->inv_c[h->gi], G->rsu_of(h->gi), (const double *)h->P.p, h->ldp, c0, nc, d_out, ldo, nys.p, nys_bytes);
  }
};

double *at(double *p, long i0) { return p ? p + i0 : nullptr; }

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

// ---- apply on a Polya-Gamma handle (f-22): the latent of a block, then the link.  What both entries refuse; `ld_ok`: the
// device entry's leading dimensions, refused before the handle is looked at
int pg_apply_check(const char *who, const flgp_predictor *h, const double *X, bool any_output, int n_new, bool ld_ok) {
  FLGP_REQUIRE(X && any_output, "%s: null pointer", who);
  FLGP_REQUIRE(n_new >= 1, "%s: need n_new >= 1 (n_new=%d)", who, n_new);
  FLGP_REQUIRE(ld_ok, "%s: a leading dimension is below n_new = %d", who, n_new);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(h->kind == FLGP_PREDICTOR_PG, "%s: the handle is not a Polya-Gamma one (kind %d)", who, h->kind);
  return on_handle_device(h, who);
}

// the n rows of `points` into the device outputs that are wanted; synchronises `st`.  A Nystrom handle: the mean-only route
// writes the block's latent (the caller's f, or W.lat), then the link
int pg_apply_rows(hipStream_t st, const flgp_predictor *h, RowPoints &points, int n, double *d_f, long ldf, double *d_pi, long ldpi,
                  double *d_y, long ldy, double *d_label) {
  RowWork W{h};
  const int B = W.rows(n);
  FLGP_TRY(W.alloc(B, h->grid ? nystrom_mean_workspace(B, h->s, h->q) : 0, d_f == nullptr));
  const int rc = for_row_blocks(st, points, n, h->d, B, [&](long i0, const double *dX, int nb, int ldx) -> int {
    double *f = at(d_f, i0), *pi = at(d_pi, i0), *y = at(d_y, i0), *label = at(d_label, i0);
    if (!h->grid) {
      const int *idx;
      const double *val;
      FLGP_TRY(W.ell(st, dX, nb, ldx, idx, val));
      return flgp_dev_predictor_pg_rows(st, idx, val, nb, h->model->r, (const double *)h->P.p, h->ldp, h->s, h->q, f, ldf, pi, ldpi, y, ldy,
                                        label);
    }
    double *lat = f ? f : W.lat.as<double>();
    const long ldl = f ? ldf : nb;
    FLGP_TRY(W.nystrom_mean(st, dX, nb, ldx, h->q, lat, ldl));
    if (!(pi || y || label)) return FLGP_OK;
    return flgp_dev_pg_link(st, lat, ldl, nb, h->q, pi, ldpi, y, ldy, label);
  });
  return settle(st, rc);                        // (the workspaces die here)
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
  FLGP_TRY(pg_apply_check("predictor_pg_apply", h, dX, d_f || d_pi || d_y || d_label, n_new,
                          ldx >= n_new && (!d_f || ldf >= n_new) && (!d_pi || ldpi >= n_new) && (!d_y || ldy >= n_new)));
  RowPoints points{dX, ldx};
  return pg_apply_rows((hipStream_t)stream, h, points, n_new, d_f, ldf, d_pi, ldpi, d_y, ldy, d_label);
}

extern "C" int flgp_predictor_pg_apply(const flgp_predictor *h, const double *X, int n_new, double *f, double *pi, double *y,
                                       double *label) {
  FLGP_TRY(pg_apply_check("predictor_pg_apply", h, X, f || pi || y || label, n_new, true));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf df, dpi, dy, dlab;
  RowPoints points{nullptr, 0, X};
  const size_t nq = sizeof(double) * (size_t)n_new * h->q;
  if (f) FLGP_TRY(df.alloc(nq));
  if (pi) FLGP_TRY(dpi.alloc(nq));
  if (y) FLGP_TRY(dy.alloc(nq));
  if (label) FLGP_TRY(dlab.alloc(sizeof(double) * (size_t)n_new));
  FLGP_TRY(pg_apply_rows(st.s, h, points, n_new, f ? df.as<double>() : nullptr, n_new, pi ? dpi.as<double>() : nullptr, n_new,
                         y ? dy.as<double>() : nullptr, n_new, label ? dlab.as<double>() : nullptr));
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

// the n rows of `points` into d_out (n x nc, ldo), which stays on the device; synchronises `st`.  A Nystrom draws handle of at
// most 8 columns takes the mean-only route (nystrom_mean_rows); every other Nystrom call the columns-out route
int cols_rows(const char *who, hipStream_t st, const flgp_predictor *h, RowPoints &points, int n, int c0, int nc, double *d_out,
              long ldo) {
  const bool mean_route = h->grid && h->kind == FLGP_PREDICTOR_DRAWS && h->q <= 8;
  RowWork W{h};
  const int B = W.rows(n);
  const size_t bytes = !h->grid      ? (sizeof(int) + sizeof(double)) * (size_t)B * (size_t)(2 * h->model->r)
                       : mean_route ? nystrom_mean_workspace(B, h->s, nc)
                                    : nystrom_cols_workspace(B, h->s, nc);
  if (points.X)
    FLGP_TRY(fits_free_memory(who, "a row block and its workspace", (double)bytes + sizeof(double) * (double)B * h->d));
  else
    FLGP_TRY(fits_free_memory(who, "the workspace of a row block", (double)bytes));
  FLGP_TRY(W.alloc(B, bytes));
  const int rc = for_row_blocks(st, points, n, h->d, B, [&](long i0, const double *dX, int nb, int ldx) -> int {
    if (!h->grid) {
      const int *idx;
      const double *val;
      FLGP_TRY(W.ell(st, dX, nb, ldx, idx, val));
      return flgp_dev_predictor_cols(st, idx, val, nb, h->model->r, (const double *)h->P.p, h->ldp, h->s, c0, nc, d_out + i0, ldo);
    }
    if (!mean_route) return W.nystrom_cols(st, dX, nb, ldx, c0, nc, d_out + i0, ldo);
    // a draws handle's whole P_draw: the mean-only route takes its columns from 0
    FLGP_REQUIRE(c0 == 0, "predictor: the mean-only route serves columns from 0 (c0=%d)", c0);
    return W.nystrom_mean(st, dX, nb, ldx, nc, d_out + i0, ldo);
  });
  return settle(st, rc);                        // (the workspaces die here)
}

// host rows, down to the host (out n x nc column-major)
int cols_to_host(const char *who, const flgp_predictor *h, const double *X, int n, int c0, int nc, double *out) {
  const double bytes = sizeof(double) * (double)n * nc;
  FLGP_TRY(fits_free_memory(who, "the n x nc result", bytes));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf d_out;
  RowPoints points{nullptr, 0, X};
  FLGP_TRY(d_out.alloc((size_t)bytes));
  FLGP_TRY(cols_rows(who, st.s, h, points, n, c0, nc, d_out.as<double>(), n));
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

// what both features entries refuse; `ld_ok`: the device entry's leading dimensions
int features_check(const char *who, const flgp_predictor *h, int g, const double *X, const double *Z, int n, bool ld_ok) {
  FLGP_REQUIRE(X && Z, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: need n >= 1 (n=%d)", who, n);
  FLGP_REQUIRE(ld_ok, "%s: a leading dimension is below n = %d", who, n);
  return check_features(who, h, g);
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
  FLGP_TRY(features_check(who, h, g, dX, dZ, n, ldx >= n && ldz >= n));
  RowPoints points{dX, ldx};
  return cols_rows(who, (hipStream_t)stream, h, points, n, g * (h->K + h->q), h->K, dZ, ldz);
}

extern "C" int flgp_predictor_features(const flgp_predictor *h, int g, const double *X, int n, double *Z) {
  const char *who = "predictor_features";
  FLGP_TRY(features_check(who, h, g, X, Z, n, true));
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
  RowPoints rows_a{nullptr, 0, Xa}, rows_b{nullptr, 0, Xb};
  FLGP_TRY(Za.alloc(sizeof(double) * (size_t)na * K));
  FLGP_TRY(dC.alloc(sizeof(double) * (size_t)na * nb));
  FLGP_TRY(cols_rows(who, st.s, h, rows_a, na, c0, K, Za.as<double>(), na));
  if (Xb) {
    FLGP_TRY(Zb.alloc(sizeof(double) * (size_t)nb * K));
    FLGP_TRY(cols_rows(who, st.s, h, rows_b, nb, c0, K, Zb.as<double>(), nb));
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

// what both update entries refuse before any device work, in the header's order; `ld_ok`: the device entry's leading dimensions
int update_check(const char *who, const flgp_predictor *h, const double *X, const double *Y, int n_b, const double *noise, int n_noise,
                 flgp_predictor **out, bool ld_ok) {
  FLGP_REQUIRE(out, "%s: null pointer (out)", who);
  *out = nullptr;
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(X && Y, "%s: null pointer", who);
  FLGP_REQUIRE(n_b >= 1, "%s: need n_b >= 1 (n_b=%d)", who, n_b);
  FLGP_REQUIRE(noise ? (n_noise == 1 || n_noise == n_b) : n_noise == 0, "%s: n_noise=%d must be 0 with a NULL noise, 1 or n_b=%d", who,
               n_noise, n_b);
  FLGP_REQUIRE(ld_ok, "%s: a leading dimension is below n_b = %d", who, n_b);
  return update_check_handle(who, h);
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
  RowWork W;
  DevBuf S, dW, part;
  int B = 0;                                    // rows per block: a multiple of the Gram kernel's chunk
  int begin(hipStream_t st, int n_b, const std::vector<double> &w) {
    const flgp_predictor *h = W.h;
    const int Wd = h->K + h->q;
    B = RowWork::update_rows();
    FLGP_TRY(W.alloc(std::min(B, n_b)));
    FLGP_TRY(S.alloc(sizeof(double) * (size_t)Wd * Wd));
    FLGP_TRY(part.alloc(predictor_gram_bytes(std::min(B, n_b), h->K, h->q)));
    FLGP_TRY(dW.alloc(sizeof(double) * (size_t)n_b));
    return h2d(dW.p, w.data(), sizeof(double) * (size_t)n_b, st);
  }
  // rows [i0, i0 + nb) of the call: dX their points (ldx), dY their responses (ldy)
  int block(hipStream_t st, long i0, const double *dX, int nb, int ldx, const double *dY, long ldy) {
    const flgp_predictor *h = W.h;
    const int *idx;
    const double *val;
    FLGP_TRY(W.ell(st, dX, nb, ldx, idx, val));
    return predictor_gram(st, idx, val, nb, h->model->r, (const double *)h->P.p, h->ldp, h->K, h->q, dW.as<double>() + i0, dY, ldy,
                          S.as<double>(), h->K + h->q, part.as<double>(), i0 == 0);
  }
  // the fold; synchronises `st`
  int finish(hipStream_t st, const char *who, flgp_predictor **out) {
    const flgp_predictor *h = W.h;
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

// The checked call once its responses dY (ldy) are on the device and its noise on the host: the responses' screen, the weights,
// the row blocks and the fold; synchronises `st`
int update_run(const char *who, hipStream_t st, const flgp_predictor *h, RowPoints &points, int n_b, const double *dY, long ldy,
               const double *noise, int n_noise, flgp_predictor **out) {
  for (int c = 0; c < h->q; ++c) FLGP_TRY(check_finite_on_device(st, dY + (long)c * ldy, n_b, "predictor_update: the responses Y"));
  std::vector<double> w;
  FLGP_TRY(update_weights(who, h, noise, n_noise, n_b, w));
  UpdateRun U{{h}};
  FLGP_TRY(U.begin(st, n_b, w));
  int rc = for_row_blocks(st, points, n_b, h->d, U.B, [&](long i0, const double *dX, int nb, int ldx) -> int {
    return U.block(st, i0, dX, nb, ldx, dY + i0, ldy);
  });
  if (rc == FLGP_OK) rc = U.finish(st, who, out);
  return settle(st, rc);                        // (the workspaces die here)
}

}  // namespace

extern "C" int flgp_dev_predictor_update(void *stream, const flgp_predictor *h, const double *dX, int n_b, int ldx, const double *dY,
                                         long ldy, const double *d_noise, int n_noise, flgp_predictor **out) {
  const char *who = "predictor_update";
  hipStream_t st = (hipStream_t)stream;
  FLGP_TRY(update_check(who, h, dX, dY, n_b, d_noise, n_noise, out, ldx >= n_b && ldy >= n_b));
  std::vector<double> noise((size_t)n_noise);
  if (n_noise) {
    FLGP_TRY(d2h(noise.data(), d_noise, sizeof(double) * (size_t)n_noise, st));
    FLGP_HIP(hipStreamSynchronize(st));
  }
  RowPoints points{dX, ldx};
  return update_run(who, st, h, points, n_b, dY, ldy, noise.data(), n_noise, out);
}

extern "C" int flgp_predictor_update(const flgp_predictor *h, const double *X, int n_b, const double *Y, const double *noise,
                                     int n_noise, flgp_predictor **out) {
  const char *who = "predictor_update";
  FLGP_TRY(update_check(who, h, X, Y, n_b, noise, n_noise, out, true));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dY;
  RowPoints points{nullptr, 0, X};
  FLGP_TRY(dY.alloc(sizeof(double) * (size_t)n_b * h->q));
  FLGP_TRY(h2d(dY.p, Y, sizeof(double) * (size_t)n_b * h->q, st.s));
  return update_run(who, st.s, h, points, n_b, dY.as<double>(), n_b, noise, n_noise, out);
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

// What both design entries refuse before any device work, in the header's order; `ld_ok`: the device entry's leading dimension.
// Refusal 8 last: *d = noise + sigma, noise NULL = the create's noise[0]
int design_check(const char *who, const flgp_predictor *h, const double *X, int n, int B, const double *noise, const int *picks, bool ld_ok,
                 double *d) {
  FLGP_REQUIRE(picks, "%s: null pointer (picks)", who);
  FLGP_REQUIRE(h, "%s: null handle", who);
  FLGP_REQUIRE(X, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: need n >= 1 (n=%d)", who, n);
  FLGP_REQUIRE(B >= 1 && B <= n, "%s: need 1 <= B <= n (B=%d, n=%d)", who, B, n);
  FLGP_REQUIRE(ld_ok, "%s: a leading dimension is below n = %d", who, n);
  FLGP_TRY(design_check_handle(who, h));
  const double nz = noise ? noise[0] : h->noise0;
  FLGP_REQUIRE(std::isfinite(nz), "%s: the noise must be finite", who);
  FLGP_REQUIRE(nz + h->sigma > 0.0, "%s: noise + sigma must be positive", who);
  *d = nz + h->sigma;
  return FLGP_OK;
}

struct DesignRun {
  RowWork W;
  DevBuf idx, val, work;
  int n = 0, Bd = 0, blk = 0;
  size_t work_bytes = 0;
  // the pool's rows, the workspace and the row chain's block, against the free memory; `extra`: what the entry holds besides
  int begin(const char *who, int n_, int B, double extra) {
    const flgp_predictor *h = W.h;
    const flgp_spectrum_model *m = h->model;
    n = n_; Bd = B;
    blk = W.rows(n);
    work_bytes = predictor_design_bytes(n, m->r, h->s, h->K, B);
    FLGP_REQUIRE(work_bytes > 0, "%s: bad shape (n=%d, r=%d, s=%d, K=%d, B=%d)", who, n, m->r, h->s, h->K, B);
    const double rows = (sizeof(int) + sizeof(double)) * (double)n * m->r;
    const double chain = (sizeof(int) + sizeof(double)) * (double)blk * (2.0 * m->r);
    size_t free_b = 0, total_b = 0;
    FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
    FLGP_REQUIRE(rows + (double)work_bytes + chain + extra <= 0.9 * (double)free_b,
                 "%s: the pool's rows of %.0f bytes and the workspace of %zu bytes (n=%d, B=%d) do not fit 90 %% of the %zu bytes free", who,
                 rows + chain + extra, work_bytes, n, B, free_b);
    FLGP_TRY(W.alloc(blk));
    FLGP_TRY(idx.alloc(sizeof(int) * (size_t)n * m->r));
    FLGP_TRY(val.alloc(sizeof(double) * (size_t)n * m->r));
    return work.alloc(work_bytes);
  }
  // rows [i0, i0 + nb) of the call: dX their points (ldx)
  int block(hipStream_t st, long i0, const double *dX, int nb, int ldx) {
    const int r = W.h->model->r;
    const int *bi;
    const double *bv;
    FLGP_TRY(W.ell(st, dX, nb, ldx, bi, bv));
    FLGP_HIP(hipMemcpyAsync(idx.as<int>() + i0 * r, bi, sizeof(int) * (size_t)nb * r, hipMemcpyDeviceToDevice, st));
    FLGP_HIP(hipMemcpyAsync(val.as<double>() + i0 * r, bv, sizeof(double) * (size_t)nb * r, hipMemcpyDeviceToDevice, st));
    return FLGP_OK;
  }
  // every block of `points`, then the greedy loop on the pool's rows; asynchronous on `st` but for the screen of host rows
  int loop(hipStream_t st, RowPoints &points, double d, int *d_picks, double *d_gain, double *d_score) {
    const flgp_predictor *h = W.h;
    FLGP_TRY(for_row_blocks(st, points, n, h->d, blk,
                            [&](long i0, const double *dX, int nb, int ldx) -> int { return block(st, i0, dX, nb, ldx); }));
    return predictor_design_rows(st, idx.as<int>(), val.as<double>(), n, h->model->r, (const double *)h->P.p, h->ldp, h->s, h->K, d, Bd,
                                 d_picks, d_gain, d_score, work.p);
  }
};

}  // namespace

extern "C" int flgp_dev_predictor_design(void *stream, const flgp_predictor *h, const double *dX, int n, int ldx, int B,
                                         const double *noise, int *d_picks, double *d_gain, double *d_score) {
  const char *who = "predictor_design";
  hipStream_t st = (hipStream_t)stream;
  double d = 0.0;
  FLGP_TRY(design_check(who, h, dX, n, B, noise, d_picks, ldx >= n, &d));
  DesignRun R{{h}};
  RowPoints points{dX, ldx};
  FLGP_TRY(R.begin(who, n, B, 0.0));
  return settle(st, R.loop(st, points, d, d_picks, d_gain, d_score));     // (the workspaces die here)
}

extern "C" int flgp_predictor_design(const flgp_predictor *h, const double *X, int n, int B, const double *noise, int *picks,
                                     double *gain, double *score) {
  const char *who = "predictor_design";
  double d = 0.0;
  FLGP_TRY(design_check(who, h, X, n, B, noise, picks, true, &d));
  Stream st;
  FLGP_TRY(st.create());
  DesignRun R{{h}};
  RowPoints points{nullptr, 0, X};
  const double out_bytes = sizeof(int) * (double)B + sizeof(double) * ((double)B + n);
  FLGP_TRY(R.begin(who, n, B, out_bytes + sizeof(double) * (double)R.W.rows(n) * h->d));
  DevBuf d_picks, d_gain, d_score;
  FLGP_TRY(d_picks.alloc(sizeof(int) * (size_t)B));
  if (gain) FLGP_TRY(d_gain.alloc(sizeof(double) * (size_t)B));
  if (score) FLGP_TRY(d_score.alloc(sizeof(double) * (size_t)n));
  int rc = R.loop(st.s, points, d, d_picks.as<int>(), gain ? d_gain.as<double>() : nullptr, score ? d_score.as<double>() : nullptr);
  if (rc == FLGP_OK) rc = d2h(picks, d_picks.p, sizeof(int) * (size_t)B, st.s);
  if (rc == FLGP_OK && gain) rc = d2h(gain, d_gain.p, sizeof(double) * (size_t)B, st.s);
  if (rc == FLGP_OK && score) rc = d2h(score, d_score.p, sizeof(double) * (size_t)n, st.s);
  return settle(st.s, rc);
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

// ---- apply (f-20, f-21): mean and variance of served rows; a Polya-Gamma handle goes to pg_apply, a draws handle to the columns
namespace {

// what both apply entries refuse; `ld_ok`: the device entry's leading dimensions, refused before the handle is looked at.  A
// Polya-Gamma handle's device is pg_apply's to check, under its own name
int apply_check(const char *who, const flgp_predictor *h, const double *X, const double *mean, const double *var, int n_new, bool ld_ok) {
  FLGP_REQUIRE(X && (mean || var), "%s: null pointer", who);
  FLGP_REQUIRE(n_new >= 1, "%s: need n_new >= 1 (n_new=%d)", who, n_new);
  FLGP_REQUIRE(ld_ok, "%s: a leading dimension is below n_new = %d", who, n_new);
  FLGP_REQUIRE(h, "%s: null handle", who);
  if (h->kind == FLGP_PREDICTOR_PG) {
    FLGP_REQUIRE(!var, "%s: a Polya-Gamma handle has no variance", who);
    return FLGP_OK;
  }
  if (h->kind == FLGP_PREDICTOR_DRAWS) FLGP_REQUIRE(!var, "%s: a draws handle has no variance", who);
  return on_handle_device(h, who);
}

// the n rows of `points` of a regression or logit handle into the device outputs that are wanted; synchronises `st`
int apply_rows(hipStream_t st, const flgp_predictor *h, RowPoints &points, int n, double *d_mean, long ldm, double *d_var, long ldv) {
  RowWork W{h};
  const int B = W.rows(n);
  FLGP_TRY(W.alloc(B, h->grid ? flgp_dev_nystrom_predictor_workspace(B, h->s, h->groups, h->K, h->q, d_var ? 1 : 0) : 0));
  const int rc = for_row_blocks(st, points, n, h->d, B, [&](long i0, const double *dX, int nb, int ldx) -> int {
    double *mean = at(d_mean, i0), *var = at(d_var, i0);
    if (h->grid) return W.nystrom_rows(st, dX, nb, ldx, mean, ldm, var, ldv);
    const int *idx;
    const double *val;
    FLGP_TRY(W.ell(st, dX, nb, ldx, idx, val));
    return flgp_dev_predictor_rows(st, idx, val, nb, h->model->r, (const double *)h->P.p, h->ldp, h->s, h->groups, h->K, h->q,
                                   (const double *)h->cg.p, mean, ldm, var, ldv);
  });
  return settle(st, rc);                        // (the workspaces die here)
}

}  // namespace

extern "C" int flgp_dev_predictor_apply(void *stream, const flgp_predictor *h, const double *dX, int n_new, int ldx, double *d_mean,
                                        long ldm, double *d_var, long ldv) {
  const char *who = "predictor_apply";
  hipStream_t st = (hipStream_t)stream;
  FLGP_TRY(apply_check(who, h, dX, d_mean, d_var, n_new, ldx >= n_new && (!d_mean || ldm >= n_new) && (!d_var || ldv >= n_new)));
  if (h->kind == FLGP_PREDICTOR_PG)
    return flgp_dev_predictor_pg_apply(stream, h, dX, n_new, ldx, d_mean, ldm, nullptr, 0, nullptr, 0, nullptr);
  RowPoints points{dX, ldx};
  if (h->kind == FLGP_PREDICTOR_DRAWS) return cols_rows(who, st, h, points, n_new, 0, h->q, d_mean, ldm);
  return apply_rows(st, h, points, n_new, d_mean, ldm, d_var, ldv);
}

extern "C" int flgp_predictor_apply(const flgp_predictor *h, const double *X, int n_new, double *mean, double *var) {
  const char *who = "predictor_apply";
  FLGP_TRY(apply_check(who, h, X, mean, var, n_new, true));
  if (h->kind == FLGP_PREDICTOR_PG) return flgp_predictor_pg_apply(h, X, n_new, mean, nullptr, nullptr, nullptr);
  if (h->kind == FLGP_PREDICTOR_DRAWS) return cols_to_host(who, h, X, n_new, 0, h->q, mean);
  const size_t gq = (size_t)h->groups * h->q;
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dmean, dvar;
  RowPoints points{nullptr, 0, X};
  if (mean) FLGP_TRY(dmean.alloc(sizeof(double) * (size_t)n_new * gq));
  if (var) FLGP_TRY(dvar.alloc(sizeof(double) * (size_t)n_new * h->groups));
  FLGP_TRY(apply_rows(st.s, h, points, n_new, mean ? dmean.as<double>() : nullptr, n_new, var ? dvar.as<double>() : nullptr, n_new));
  if (mean) FLGP_TRY(d2h(mean, dmean.p, sizeof(double) * (size_t)n_new * gq, st.s));
  if (var) FLGP_TRY(d2h(var, dvar.p, sizeof(double) * (size_t)n_new * h->groups, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" void flgp_predictor_free(flgp_predictor *h) { delete h; }

// The fitted spectrum model's extension (include/flgp_hip.h): the fit's row chain
//   k-NN -> LAE / SE weights -> the three scalings under the fit's column sums -> u = a V / sigma * sqrt(n_fit)
// for rows that were not in the fit, on the stage entries the fit itself runs (knn.hip, lae.hip, sparse.hip).  The fit
// that makes the handle is capi.hip's flgp_heat_kernel_spectrum_model.  The chain up to the weights (model_rows) is shared
// with the fitted predictor (predictor.hip, f-20), which puts its row kernel (predictor_rows.hip) in the place of U-recovery.
// Both walk their rows through common.h's for_row_blocks.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <memory>

using namespace flgp;

namespace flgp {

int model_block_rows() { return std::max(256, tuning("model_extend_block", 1 << 20)); }

int ModelRowWork::alloc(const flgp_spectrum_model *m, int rows) {
  FLGP_TRY(knn_idx.alloc(sizeof(int) * (size_t)rows * m->r));
  if (m->kernel_se) FLGP_TRY(knn_dist.alloc(sizeof(double) * (size_t)rows * m->r));
  FLGP_TRY(ell_idx.alloc(sizeof(int) * (size_t)rows * m->r));
  return ell_val.alloc(sizeof(double) * (size_t)rows * m->r);
}

// The row chain up to the scaled anchor weights, for the extension below and the predictor (predictor.hip)
int model_rows(hipStream_t st, const flgp_spectrum_model *m, ModelRowWork &W, const double *dX, int nb, int ldx) {
  const int r = m->r, s = m->s;
  const double *Ut = (const double *)m->Ut.p;
  FLGP_TRY(flgp_dev_knn(st, dX, nb, ldx, m->d, Ut, (const double *)m->uu.p, s, r, W.knn_idx.as<int>(),
                        m->kernel_se ? W.knn_dist.as<double>() : nullptr, nb));
  if (m->kernel_se)
    FLGP_TRY(flgp_dev_se_weights(st, W.knn_idx.as<int>(), W.knn_dist.as<double>(), nb, nb, r, m->epsilon, W.ell_idx.as<int>(),
                                 W.ell_val.as<double>()));
  else
    FLGP_TRY(flgp_dev_lae(st, dX, nb, ldx, m->d, Ut, s, r, W.knn_idx.as<int>(), nb, W.ell_idx.as<int>(), W.ell_val.as<double>()));
  return flgp_dev_extend_scale(st, W.ell_idx.as<int>(), W.ell_val.as<double>(), nb, r,
                               m->gl == FLGP_GL_RW ? nullptr : (const double *)m->colsum_gl.p,
                               m->gl == FLGP_GL_CLUSTER_NORMALIZED ? (const double *)m->sizes.p : nullptr,
                               (const double *)m->colsum_spectrum.p);
}

}  // namespace flgp

namespace {

int on_model_device(const flgp_spectrum_model *m, const char *who) {
  int dev = -1;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == m->device, "%s: the model lives on device %d, the current device is %d", who, m->device, dev);
  return FLGP_OK;
}

// the workspaces of one block of at most `rows` rows
struct ExtendWork : ModelRowWork {
  DevBuf uwork;
  int alloc(const flgp_spectrum_model *m, int rows) {
    FLGP_TRY(ModelRowWork::alloc(m, rows));
    return uwork.alloc(flgp_dev_u_recover_workspace(m->s, m->K));
  }
};

// the n_new rows of `points` block by block into d_out (+ row offset already applied, ldo): synchronises `st`
int extend_rows(hipStream_t st, const flgp_spectrum_model *m, RowPoints &points, int n_new, double *d_out, int ldo) {
  const int B = std::min(model_block_rows(), n_new);
  ExtendWork W;
  FLGP_TRY(W.alloc(m, B));
  const int rc = for_row_blocks(st, points, n_new, m->d, B, [&](long i0, const double *dX, int nb, int ldx) -> int {
    FLGP_TRY(model_rows(st, m, W, dX, nb, ldx));
    // sqrt(n_fit): the scale of the fit's rows, whatever the number of new ones
    return flgp_dev_u_recover(st, W.ell_idx.as<int>(), W.ell_val.as<double>(), nb, m->r, (const double *)m->V.p, m->s, m->s,
                              (const double *)m->eig.p, m->K, std::sqrt((double)m->n_fit), m->root, d_out + i0, ldo, nullptr,
                              W.uwork.as<double>());
  });
  return settle(st, rc);                  // (the workspaces die here)
}

}  // namespace

extern "C" int flgp_dev_spectrum_model_extend(void *stream, const flgp_spectrum_model *m, const double *dX, int n_new, int ldx,
                                              double *d_vectors, int ldv) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(dX && d_vectors, "spectrum_model_extend: null pointer");
  FLGP_REQUIRE(n_new >= 1, "spectrum_model_extend: need n_new >= 1 (n_new=%d)", n_new);
  FLGP_REQUIRE(ldx >= n_new && ldv >= n_new, "spectrum_model_extend: a leading dimension is below n_new = %d", n_new);
  FLGP_REQUIRE(m, "spectrum_model_extend: null handle");
  FLGP_TRY(on_model_device(m, "spectrum_model_extend"));
  RowPoints points{dX, ldx};
  return extend_rows(st, m, points, n_new, d_vectors, ldv);
}

extern "C" int flgp_spectrum_model_dims(const flgp_spectrum_model *m, int *n_fit, int *d, int *s, int *r, int *K, int *kernel_se,
                                        int *gl, int *root) {
  FLGP_REQUIRE(m, "spectrum_model_dims: null handle");
  if (n_fit) *n_fit = m->n_fit;
  if (d) *d = m->d;
  if (s) *s = m->s;
  if (r) *r = m->r;
  if (K) *K = m->K;
  if (kernel_se) *kernel_se = m->kernel_se;
  if (gl) *gl = m->gl;
  if (root) *root = m->root;
  return FLGP_OK;
}

extern "C" int flgp_spectrum_model_to_host(const flgp_spectrum_model *m, double *values, double *eig, double *V, double *colsum_gl,
                                           double *colsum_spectrum, double *sizes) {
  FLGP_REQUIRE(m, "spectrum_model_to_host: null handle");
  FLGP_TRY(on_model_device(m, "spectrum_model_to_host"));
  Stream st;
  FLGP_TRY(st.create());
  const size_t s = (size_t)m->s, K = (size_t)m->K;
  // a vector the fit did not use ("rw": no Laplacian column sums; no cluster sizes) reads as zeros
  auto out = [&](double *h, const DevBuf &b, size_t cnt) -> int {
    if (!h) return FLGP_OK;
    if (!b.p) { std::fill(h, h + cnt, 0.0); return FLGP_OK; }
    return d2h(h, b.p, sizeof(double) * cnt, st.s);
  };
  FLGP_TRY(out(values, m->values, K));
  FLGP_TRY(out(eig, m->eig, K));
  FLGP_TRY(out(V, m->V, s * K));
  FLGP_TRY(out(colsum_gl, m->colsum_gl, s));
  FLGP_TRY(out(colsum_spectrum, m->colsum_spectrum, s));
  FLGP_TRY(out(sizes, m->sizes, s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" int flgp_spectrum_model_extend(const flgp_spectrum_model *m, const double *X, int n_new, double *vectors) {
  FLGP_REQUIRE(X && vectors, "spectrum_model_extend: null pointer");
  FLGP_REQUIRE(n_new >= 1, "spectrum_model_extend: need n_new >= 1 (n_new=%d)", n_new);
  FLGP_REQUIRE(m, "spectrum_model_extend: null handle");
  FLGP_TRY(on_model_device(m, "spectrum_model_extend"));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dvec;
  RowPoints points{nullptr, 0, X};
  FLGP_TRY(dvec.alloc(sizeof(double) * (size_t)n_new * m->K));
  FLGP_TRY(extend_rows(st.s, m, points, n_new, dvec.as<double>(), n_new));
  FLGP_TRY(d2h(vectors, dvec.p, sizeof(double) * (size_t)n_new * m->K, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" int flgp_spectrum_model_extend_resident(const flgp_spectrum_model *m, const double *X, int n_new,
                                                   const flgp_eigenpair *head, const int *head_rows, int n_head,
                                                   flgp_eigenpair **out) {
  FLGP_REQUIRE(out, "spectrum_model_extend_resident: null pointer");
  *out = nullptr;
  FLGP_REQUIRE(X, "spectrum_model_extend_resident: null pointer");
  FLGP_REQUIRE(n_new >= 1, "spectrum_model_extend_resident: need n_new >= 1 (n_new=%d)", n_new);
  FLGP_REQUIRE(n_head >= 0, "spectrum_model_extend_resident: need n_head >= 0 (n_head=%d)", n_head);
  FLGP_REQUIRE(m, "spectrum_model_extend_resident: null handle");
  if (!head) n_head = 0;
  if (n_head > 0) {
    FLGP_REQUIRE(head_rows, "spectrum_model_extend_resident: head without head_rows");
    FLGP_REQUIRE(head->K == m->K, "spectrum_model_extend_resident: the head pair has K = %d, the model K = %d", head->K, m->K);
    FLGP_REQUIRE(head->device == m->device, "spectrum_model_extend_resident: the head pair lives on device %d, the model on device %d",
                 head->device, m->device);
    for (int a = 0; a < n_head; ++a)
      FLGP_REQUIRE(head_rows[a] >= 0 && head_rows[a] < head->n, "spectrum_model_extend_resident: head_rows[%d]=%d out of range", a, head_rows[a]);
  }
  FLGP_REQUIRE((long)n_head + n_new <= 2147483647L, "spectrum_model_extend_resident: n_head + n_new exceeds the int range");
  FLGP_TRY(on_model_device(m, "spectrum_model_extend_resident"));
  const int K = m->K, n = n_head + n_new;
  Stream st;
  FLGP_TRY(st.create());
  std::unique_ptr<flgp_eigenpair> ep(new flgp_eigenpair());
  ep->n = n; ep->K = K; ep->device = m->device;
  FLGP_TRY(ep->values.alloc(sizeof(double) * (size_t)K));
  FLGP_TRY(ep->vectors.alloc(sizeof(double) * (size_t)n * K));
  FLGP_HIP(hipMemcpyAsync(ep->values.p, m->values.p, sizeof(double) * (size_t)K, hipMemcpyDeviceToDevice, st.s));
  DevBuf drows;
  if (n_head > 0) {
    FLGP_TRY(drows.alloc(sizeof(int) * (size_t)n_head));
    FLGP_TRY(h2d(drows.p, head_rows, sizeof(int) * (size_t)n_head, st.s));
    FLGP_TRY(gather_rows_ld(st.s, (const double *)head->vectors.p, head->n, drows.as<int>(), n_head, K, ep->vectors.as<double>(), n));
  }
  RowPoints points{nullptr, 0, X};
  FLGP_TRY(extend_rows(st.s, m, points, n_new, ep->vectors.as<double>() + n_head, n));
  *out = ep.release();
  return FLGP_OK;
}

extern "C" void flgp_spectrum_model_free(flgp_spectrum_model *m) { delete m; }

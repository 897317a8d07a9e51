// Consumers of the device-resident EigenPair (include/flgp_hip.h; the pair itself is made in capi.hip): the V products;
// regression prediction, posterior variance and the training objectives with their gradients (kernels in
// gpr.hip and gpr_grad.hip; the drivers' whole testing step in one call, in weight space for m > K: DESIGN 8 f-13); the
// Laplace approximation of the logit GP, its posterior and its training objective (SURVEY
// 8f-5, gpc.hip; the posterior's route for m > K, B problems in shared launches: DESIGN 8 f-11; the binary entry is its
// batch of one, the J one-vs-rest posteriors its batch of J: f-12; any response matrix in one call: f-17; the
// training objective for B problems in one call: f-15; the regression objective for B (pair, x) problems through a training
// context: f-18; the trained operands of both posteriors for the fitted predictor of predictor.hip: f-20);
// Polya-Gamma Gibbs prediction (pg.hip; B chains in one call, the binary entry its batch of one and the
// one-vs-rest entry its batch of J: DESIGN 8 f-16).  The algebra they share is written once: woodbury_step (regression,
// m > K) and LrBatch (the K x K solve against B = sW C sW + I, for the Newton loop and, through PgBatch, the Gibbs sweep).
// Each entry checks its arguments on the host, then runs on one stream of its own.
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

using namespace flgp;

namespace {

// X = the host's `bytes` at `host`, allocated and copied on `st`
int upload(DevBuf &X, const void *host, size_t bytes, hipStream_t st) {
  FLGP_TRY(X.alloc(bytes));
  return h2d(X.p, host, bytes, st);
}

// One index array into the pair's rows.  check() refuses a row outside [0, n) before any device work, as
// "<who>: <name>[<a>]=<v> out of range".  At first use (resolve) a contiguous range is taken in place (row0) and any other
// set is uploaded once (d): the scan runs beside the device work queued by then.  gather() makes V = vectors[rows, 0:K]
// (m x K at ld; a range is read in place).
struct Rows {
  const int *idx = nullptr;
  int m = 0, row0 = 0;
  bool resolved = false;
  const int *d = nullptr;        // flgp_dev_hk's index argument: nullptr for a range
  const double *V = nullptr;
  long ld = 0;
  int gathered_K = 0;            // the K of the last gather(): asking again for it does nothing
  DevBuf didx, vbuf;
  int check(const flgp_eigenpair *ep, const int *idx_, int m_, const char *who, const char *name) {
    for (int a = 0; a < m_; ++a) FLGP_REQUIRE(idx_[a] >= 0 && idx_[a] < ep->n, "%s: %s[%d]=%d out of range", who, name, a, idx_[a]);
    idx = idx_; m = m_;
    return FLGP_OK;
  }
  int resolve(hipStream_t st) {
    if (resolved) return FLGP_OK;
    resolved = true;
    if (is_range(idx, m)) { row0 = idx[0]; return FLGP_OK; }
    FLGP_TRY(upload(didx, idx, sizeof(int) * (size_t)m, st));
    d = didx.as<int>();
    return FLGP_OK;
  }
  int gather(hipStream_t st, const flgp_eigenpair *ep, int K) {
    FLGP_TRY(resolve(st));
    if (gathered_K == K) return FLGP_OK;
    if (!d) { V = (const double *)ep->vectors.p + row0; ld = ep->n; gathered_K = K; return FLGP_OK; }
    FLGP_TRY(vbuf.alloc(sizeof(double) * (size_t)m * K));
    FLGP_TRY(flgp_dev_gather_rows(st, (const double *)ep->vectors.p, ep->n, d, m, K, vbuf.as<double>()));
    V = vbuf.as<double>(); ld = m; gathered_K = K;
    return FLGP_OK;
  }
};

// H = HK(a, b) from the first K pairs (a.m x b.m, ld a.m); both row sets uploaded, `work` sized by the caller
int hk(hipStream_t st, const flgp_eigenpair *ep, int K, double t, const Rows &a, const Rows &b, double *H, double *work) {
  const double *dvec = (const double *)ep->vectors.p;
  return flgp_dev_hk(st, (const double *)ep->values.p, K, t, dvec, ep->n, a.d, a.row0, a.m, dvec, ep->n, b.d, b.row0, b.m, H,
                     a.m, work);
}
// C = C11 = HK(r, r) + sigma I (r.m x r.m), with `work` of work_bytes for it and the caller's later contractions.  A zero
// sigma launches nothing: the diagonal of HK(r, r) is a sum of squares, never -0.
int hk_c11(hipStream_t st, const flgp_eigenpair *ep, int K, double t, Rows &r, double sigma, DevBuf &C, DevBuf &work,
           size_t work_bytes) {
  FLGP_TRY(r.resolve(st));
  FLGP_TRY(C.alloc(sizeof(double) * (size_t)r.m * r.m));
  FLGP_TRY(work.alloc(work_bytes));
  FLGP_TRY(hk(st, ep, K, t, r, r, C.as<double>(), work.as<double>()));
  return sigma != 0.0 ? gpr_add_diag(st, C.as<double>(), r.m, sigma) : FLGP_OK;
}

// Column-major products, C (M x N, ld M) = A^T B with A k x M, or = A B with A M x k; B k x N.  `work` / `we` go to
// gemm_launch unchanged: they bound its k-split, so they decide the bits.  vt_work_elems: the `we` of the consumers that
// form a K x K and a K x q product V^T (.) from one workspace.
size_t vt_work_elems(int K, int q) { return (size_t)128 * K * K + (size_t)64 * K * q + 1024; }
int gemm_tn(hipStream_t st, int M, int N, int k, const double *A, long lda, const double *B, long ldb, double *C, double *work,
            size_t we) {
  return gemm_launch(st, M, N, k, 1.0, A, lda, 1, B, 1, ldb, 0.0, nullptr, 0, 0, C, 1, M, work, we, 0.0, nullptr);
}
int gemm_nn(hipStream_t st, int M, int N, int k, const double *A, long lda, const double *B, long ldb, double *C, double *work,
            size_t we) {
  return gemm_launch(st, M, N, k, 1.0, A, 1, lda, B, 1, ldb, 0.0, nullptr, 0, 0, C, 1, M, work, we, 0.0, nullptr);
}

// The V products: out (host) = V^T B (tn, K x q) or V B (m x q) with V = vectors[idx, 0:K] and B the caller's (m or K rows,
// q columns; nullptr: V itself).  `we` is the workspace of the V^T B product.
int v_product(const flgp_eigenpair *ep, int K, const int *idx, int m, const double *B, int q, bool tn, size_t we, double *out_h) {
  FLGP_REQUIRE(ep && idx, "eigenpair: null pointer");
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1, "eigenpair: need 1 <= K <= %d and m >= 1", ep->K);
  Rows R;
  FLGP_TRY(R.check(ep, idx, m, "eigenpair", "idx"));
  Stream st;
  FLGP_TRY(st.create());
  FLGP_TRY(R.gather(st.s, ep, K));
  const int brows = tn ? m : K, orows = tn ? K : m;
  DevBuf dB, out, work;
  FLGP_TRY(out.alloc(sizeof(double) * (size_t)orows * q));
  if (tn) FLGP_TRY(work.alloc(sizeof(double) * we));
  if (B) FLGP_TRY(upload(dB, B, sizeof(double) * (size_t)brows * q, st.s));
  const double *b = B ? dB.as<double>() : R.V;
  const long ldb = B ? brows : R.ld;
  FLGP_TRY(tn ? gemm_tn(st.s, K, q, m, R.V, R.ld, b, ldb, out.as<double>(), work.as<double>(), we)
              : gemm_nn(st.s, m, q, K, R.V, R.ld, b, ldb, out.as<double>(), nullptr, 0));
  FLGP_TRY(d2h(out_h, out.p, sizeof(double) * (size_t)orows * q, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

}  // namespace

extern "C" int flgp_eigenpair_vtv(const flgp_eigenpair *ep, int K, const int *idx, int m, double *VtV) {
  FLGP_REQUIRE(VtV, "eigenpair_vtv: null pointer");
  return v_product(ep, K, idx, m, nullptr, K, true, (size_t)128 * K * K, VtV);
}

extern "C" int flgp_eigenpair_vty(const flgp_eigenpair *ep, int K, const int *idx, int m, const double *Y, int q,
                                  double *VtY) {
  FLGP_REQUIRE(Y && VtY && q >= 1, "eigenpair_vty: bad arguments");
  return v_product(ep, K, idx, m, Y, q, true, (size_t)64 * K * q + 1024, VtY);
}

extern "C" int flgp_eigenpair_vc(const flgp_eigenpair *ep, int K, const int *idx, int m, const double *C, int q,
                                 double *VC) {
  FLGP_REQUIRE(C && VC && q >= 1, "eigenpair_vc: bad arguments");
  return v_product(ep, K, idx, m, C, q, false, 0, VC);
}

// ---- regression consumers of the resident pair: the Woodbury algebra stays on the device --------------
namespace {
// the two verdicts on a system matrix that did not factor, under the entry's name, and how one is returned
std::string not_positive_definite(const char *who) {
  return std::string(who) + ": the system matrix is not positive definite (Cholesky pivot <= 0)";
}
std::string not_finite(const char *who) {
  return std::string(who) + ": the objective is not finite (the system matrix is numerically singular)";
}
int noconv(const std::string &verdict) { set_error("%s", verdict.c_str()); return FLGP_ERR_NOCONV; }
struct GprCtx {
  DevBuf ls, l, flag;
  int prepare(hipStream_t st, const flgp_eigenpair *ep, int K, double t) {
    FLGP_TRY(ls.alloc(sizeof(double) * (size_t)K)); FLGP_TRY(l.alloc(sizeof(double) * (size_t)K));
    FLGP_TRY(flag.alloc(sizeof(int)));
    FLGP_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st));
    return gpr_weights(st, (const double *)ep->values.p, K, t, ls.as<double>(), l.as<double>());
  }
  int verdict(hipStream_t st, const char *who) {   // synchronises
    int h = 0;
    FLGP_TRY(read_flag(st, flag.p, &h));
    return h ? noconv(not_positive_definite(who)) : FLGP_OK;
  }
};

// The regression Woodbury step (m > K) on M = V^T Z^-1 V (K x K) and the right-hand side S = V^T Z^-1 Y (K x q), both the
// caller's:  Q = Ls M Ls + c I,  T1 = (S - M Ls Q^-1 Ls S) * scale.  noisepar "same" (src/Predict.cpp:59-74) has Z = I,
// c = noise + sigma and scale = 1 / c; "different" (:92-110) has Z = diag(noise_i + sigma) and c = scale = 1.  T1 is then
// V^T alpha: the m x q alpha is never formed.  The posterior variance (src/Utils.cpp:238-246) passes M as its own S.
// Q (K x K) and R (K x q) are scratch.  No GEMM here splits its k, so the step takes no workspace: the V^T products that
// do, and their `we`, stay with the callers.
int woodbury_step(hipStream_t st, GprCtx &G, int K, int q, const double *M, const double *S, double c, double scale, double *Q,
                  double *R, double *T1) {
  FLGP_TRY(gpr_q(st, M, G.ls.as<double>(), K, c, Q));
  FLGP_TRY(gpr_scale(st, S, G.ls.as<double>(), nullptr, K, q, R));          // Ls S
  FLGP_TRY(chol_solve(st, Q, K, R, q, G.flag.as<int>()));                    // Q^-1 (.)
  FLGP_TRY(gpr_scale(st, R, G.ls.as<double>(), nullptr, K, q, R));          // Ls (.)
  FLGP_TRY(gemm_nn(st, K, q, K, M, K, R, K, T1, nullptr, 0));
  return gpr_diff(st, S, T1, scale, (long)K * q, T1);
}

// predict_regression_cpp (reference src/Predict.cpp:40-110): noise_vec == nullptr is noisepar = "same" (one variance
// `noise` for every training row), otherwise "different" (noise_vec[a] for row a, the reference's pars[1..m]).
// `who` names the entry in every message (the regression posterior runs this body for m <= K).
int predict_regression(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1, int mnew,
                       const double *Y, int q, double t, double noise, const double *noise_vec, double sigma, double *Y_pred) {
  FLGP_REQUIRE(ep && idx0 && idx1 && Y && Y_pred, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && mnew >= 1 && q >= 1, "%s: bad shape (K=%d m=%d m_new=%d q=%d)", who, K, m, mnew, q);
  if (noise_vec)
    for (int a = 0; a < m; ++a) FLGP_REQUIRE(noise_vec[a] + sigma > 0.0, "%s: noise[%d] + sigma must be positive", who, a);
  else
    FLGP_REQUIRE(noise + sigma > 0.0, "%s: noise + sigma must be positive", who);
  Rows r0, r1;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  FLGP_TRY(r1.check(ep, idx1, mnew, who, "idx1"));
  Stream st;
  FLGP_TRY(st.create());
  GprCtx G;
  FLGP_TRY(G.prepare(st.s, ep, K, t));
  DevBuf dY, out, dnoise;
  FLGP_TRY(out.alloc(sizeof(double) * (size_t)mnew * q));
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m * q, st.s));
  if (noise_vec) FLGP_TRY(upload(dnoise, noise_vec, sizeof(double) * (size_t)m, st.s));
  if (m <= K) {
    // Cvv + sigma I + (noise I or diag(noise)), Cholesky, alpha = C^-1 Y, Y_pred = Cnv alpha   (src/Predict.cpp:48-58, 78-91)
    DevBuf C, Cnv, work;
    FLGP_TRY(r1.resolve(st.s));
    FLGP_TRY(Cnv.alloc(sizeof(double) * (size_t)mnew * m));
    FLGP_TRY(hk_c11(st.s, ep, K, t, r0, sigma, C, work, flgp_dev_hk_workspace(std::max(m, mnew), m, K, 1)));
    FLGP_TRY(noise_vec ? gpr_add_diag_vec(st.s, C.as<double>(), m, dnoise.as<double>()) : gpr_add_diag(st.s, C.as<double>(), m, noise));
    FLGP_TRY(hk(st.s, ep, K, t, r1, r0, Cnv.as<double>(), work.as<double>()));
    FLGP_TRY(chol_solve(st.s, C.as<double>(), m, dY.as<double>(), q, G.flag.as<int>()));
    FLGP_TRY(gemm_nn(st.s, mnew, q, m, Cnv.as<double>(), mnew, dY.as<double>(), m, out.as<double>(), nullptr, 0));
  } else {
    // V^T alpha by the Woodbury step, then Y_pred = V2 exp(-t lam) V^T alpha                   (src/Predict.cpp:59-75, 92-110)
    FLGP_TRY(r0.gather(st.s, ep, K));
    FLGP_TRY(r1.gather(st.s, ep, K));
    DevBuf zinv, ZV, ZY, M, S, Q, R, T1, work;
    const size_t we = vt_work_elems(K, q);
    FLGP_TRY(M.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(Q.alloc(sizeof(double) * (size_t)K * K));
    FLGP_TRY(S.alloc(sizeof(double) * (size_t)K * q)); FLGP_TRY(R.alloc(sizeof(double) * (size_t)K * q));
    FLGP_TRY(T1.alloc(sizeof(double) * (size_t)K * q)); FLGP_TRY(work.alloc(sizeof(double) * we));
    const double *Vz = r0.V, *Yz = dY.as<double>();                                               // Z^-1 V, Z^-1 Y: "same" has Z = I
    long ldz = r0.ld;
    double c = noise + sigma, scale = 1.0 / c;
    if (noise_vec) {
      FLGP_TRY(zinv.alloc(sizeof(double) * (size_t)m));
      FLGP_TRY(ZV.alloc(sizeof(double) * (size_t)m * K)); FLGP_TRY(ZY.alloc(sizeof(double) * (size_t)m * q));
      FLGP_TRY(gpr_zinv(st.s, dnoise.as<double>(), sigma, m, zinv.as<double>()));                // :98-101
      FLGP_TRY(gpr_rowscale_ld(st.s, r0.V, r0.ld, zinv.as<double>(), m, K, ZV.as<double>()));
      FLGP_TRY(gpr_rowscale_ld(st.s, dY.as<double>(), m, zinv.as<double>(), m, q, ZY.as<double>()));
      Vz = ZV.as<double>(); ldz = m; Yz = ZY.as<double>(); c = scale = 1.0;
    }
    FLGP_TRY(gemm_tn(st.s, K, K, m, r0.V, r0.ld, Vz, ldz, M.as<double>(), work.as<double>(), we));    // V^T Z^-1 V   :102
    FLGP_TRY(gemm_tn(st.s, K, q, m, r0.V, r0.ld, Yz, m, S.as<double>(), work.as<double>(), we));      // V^T Z^-1 Y
    FLGP_TRY(woodbury_step(st.s, G, K, q, M.as<double>(), S.as<double>(), c, scale, Q.as<double>(), R.as<double>(), T1.as<double>()));
    FLGP_TRY(gpr_scale(st.s, T1.as<double>(), G.l.as<double>(), nullptr, K, q, T1.as<double>()));          // exp(-t lam) (.)
    FLGP_TRY(gemm_nn(st.s, mnew, q, K, r1.V, r1.ld, T1.as<double>(), K, out.as<double>(), nullptr, 0));    // :108-109
  }
  FLGP_TRY(d2h(Y_pred, out.p, sizeof(double) * (size_t)mnew * q, st.s));
  return G.verdict(st.s, who);
}
}  // namespace

extern "C" int flgp_eigenpair_predict_regression(const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1,
                                                 int mnew, const double *Y, int q, double t, double noise, double sigma,
                                                 double *Y_pred) {
  return predict_regression("predict_regression", ep, K, idx0, m, idx1, mnew, Y, q, t, noise, nullptr, sigma, Y_pred);
}

extern "C" int flgp_eigenpair_predict_regression_different(const flgp_eigenpair *ep, int K, const int *idx0, int m,
                                                           const int *idx1, int mnew, const double *Y, int q, double t,
                                                           const double *noise, double sigma, double *Y_pred) {
  FLGP_REQUIRE(noise, "predict_regression: null pointer");
  return predict_regression("predict_regression", ep, K, idx0, m, idx1, mnew, Y, q, t, 0.0, noise, sigma, Y_pred);
}

namespace {
// posterior_covariance_regression (reference src/Utils.cpp:214-250), under the caller's name as predict_regression
int posterior_variance(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1, int mnew,
                       double t, double var, double sigma, double *cov) {
  FLGP_REQUIRE(ep && idx0 && idx1 && cov, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && mnew >= 1, "%s: bad shape (K=%d m=%d m_new=%d)", who, K, m, mnew);
  const double c = var + sigma;
  FLGP_REQUIRE(c > 0.0, "%s: var + sigma must be positive", who);
  Rows r0, r1;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  FLGP_TRY(r1.check(ep, idx1, mnew, who, "idx1"));
  Stream st;
  FLGP_TRY(st.create());
  GprCtx G;
  FLGP_TRY(G.prepare(st.s, ep, K, t));
  FLGP_TRY(r1.gather(st.s, ep, K));
  DevBuf out;
  FLGP_TRY(out.alloc(sizeof(double) * (size_t)mnew));
  if (m <= K) {
    // K11 = C11 + (var + sigma) I; alpha = C21 K11^-1; beta = rowsum(C21 .* alpha)          (src/Utils.cpp:227-237)
    DevBuf C, C12, X, work;
    FLGP_TRY(C12.alloc(sizeof(double) * (size_t)m * mnew)); FLGP_TRY(X.alloc(sizeof(double) * (size_t)m * mnew));
    FLGP_TRY(hk_c11(st.s, ep, K, t, r0, c, C, work, flgp_dev_hk_workspace(m, std::max(m, mnew), K, 1)));
    FLGP_TRY(hk(st.s, ep, K, t, r0, r1, C12.as<double>(), work.as<double>()));
    FLGP_HIP(hipMemcpyAsync(X.p, C12.p, sizeof(double) * (size_t)m * mnew, hipMemcpyDeviceToDevice, st.s));
    FLGP_TRY(chol_solve(st.s, C.as<double>(), m, X.as<double>(), mnew, G.flag.as<int>()));
    FLGP_TRY(gpr_rowdot(st.s, C12.as<double>(), X.as<double>(), mnew, m, r1.V, r1.ld, K, G.l.as<double>(), c, out.as<double>()));
  } else {
    // alpha = 1/(var+sigma) L V1^T (V1 - V1 Ls Q^-1 Ls V1^T V1) L; beta_i = V2(i,:) alpha V2(i,:)^T  (src/Utils.cpp:238-246)
    FLGP_TRY(r0.gather(st.s, ep, K));
    DevBuf VtV, Q, R, T1, W, work;
    const size_t we = (size_t)128 * K * K + 1024;
    FLGP_TRY(VtV.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(Q.alloc(sizeof(double) * (size_t)K * K));
    FLGP_TRY(R.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(T1.alloc(sizeof(double) * (size_t)K * K));
    FLGP_TRY(W.alloc(sizeof(double) * (size_t)mnew * K)); FLGP_TRY(work.alloc(sizeof(double) * we));
    FLGP_TRY(gemm_tn(st.s, K, K, m, r0.V, r0.ld, r0.V, r0.ld, VtV.as<double>(), work.as<double>(), we));
    FLGP_TRY(woodbury_step(st.s, G, K, K, VtV.as<double>(), VtV.as<double>(), c, 1.0 / c, Q.as<double>(), R.as<double>(),
                           T1.as<double>()));                                                              // (VtV - ...)/(var+sigma)
    FLGP_TRY(gpr_scale(st.s, T1.as<double>(), G.l.as<double>(), G.l.as<double>(), K, K, T1.as<double>()));   // L (.) L
    FLGP_TRY(gemm_nn(st.s, mnew, K, K, r1.V, r1.ld, T1.as<double>(), K, W.as<double>(), nullptr, 0));      // V2 alpha
    FLGP_TRY(gpr_rowquad(st.s, r1.V, r1.ld, W.as<double>(), mnew, K, G.l.as<double>(), c, out.as<double>()));
  }
  FLGP_TRY(d2h(cov, out.p, sizeof(double) * (size_t)mnew, st.s));
  return G.verdict(st.s, who);
}
}  // namespace

extern "C" int flgp_eigenpair_posterior_variance(const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1,
                                                 int mnew, double t, double var, double sigma, double *cov) {
  return posterior_variance("posterior_variance", ep, K, idx0, m, idx1, mnew, t, var, sigma, cov);
}

// ---- classification consumers: the Laplace approximation of the logit GP on the device (gpc.hip) ---------
namespace {
int check_labels(const double *Y, const double *N, int m, const char *who) {
  for (int a = 0; a < m; ++a) {
    const double n = N ? N[a] : 1.0;
    FLGP_REQUIRE(n > 0.0 && n < HUGE_VAL, "%s: N[%d]=%g must be positive", who, a, n);
    FLGP_REQUIRE(Y[a] >= 0.0 && Y[a] <= n, "%s: Y[%d]=%g is outside [0, N[%d]=%g]", who, a, Y[a], a, n);
  }
  return FLGP_OK;
}
// Newton loop + final sums on the device-resident C (m x m); only the scalar comes down
int logit_la_on_device(hipStream_t st, const double *dC, int m, const double *Y, const double *N, double tol, int max_iter,
                       double *amll, int *iters, const char *who) {
  DevBuf dY, dN;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m, st));
  FLGP_TRY(upload(dN, N, sizeof(double) * (size_t)m, st));
  GpcNewton S;
  FLGP_TRY(S.alloc(m));
  int it = 0;
  FLGP_TRY(S.run(st, dC, dY.as<double>(), dN.as<double>(), tol, max_iter, who, &it));
  if (iters) *iters = it;
  return S.amll(st, dY.as<double>(), dN.as<double>(), amll);
}
}  // namespace

extern "C" int flgp_logit_la_marginal_likelihood(const double *C, int m, const double *Y, const double *N, double tol,
                                                 int max_iter, double *amll, int *iters) {
  FLGP_REQUIRE(C && Y && N && amll, "logit_la_marginal_likelihood: null pointer");
  FLGP_REQUIRE(m >= 1 && max_iter >= 1, "logit_la_marginal_likelihood: bad shape (m=%d max_iter=%d)", m, max_iter);
  FLGP_TRY(check_labels(Y, N, m, "logit_la_marginal_likelihood"));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dC;
  FLGP_TRY(upload(dC, C, sizeof(double) * (size_t)m * m, st.s));
  return logit_la_on_device(st.s, dC.as<double>(), m, Y, N, tol, max_iter, amll, iters, "logit_la_marginal_likelihood");
}

extern "C" int flgp_eigenpair_logit_marginal_likelihood(const flgp_eigenpair *ep, int K, double t, double sigma, const int *idx,
                                                        int m, const double *Y, const double *N, double tol, int max_iter,
                                                        double *amll, int *iters) {
  FLGP_REQUIRE(ep && idx && Y && N && amll, "logit_marginal_likelihood: null pointer");
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && max_iter >= 1, "logit_marginal_likelihood: bad shape (K=%d of %d, m=%d, max_iter=%d)",
               K, ep->K, m, max_iter);
  Rows r0;
  FLGP_TRY(r0.check(ep, idx, m, "logit_marginal_likelihood", "idx"));
  FLGP_TRY(check_labels(Y, N, m, "logit_marginal_likelihood"));
  Stream st;
  FLGP_TRY(st.create());
  // C = HK(idx, idx) + sigma I       (src/train.cpp:30-31)
  DevBuf C, work;
  FLGP_TRY(hk_c11(st.s, ep, K, t, r0, sigma, C, work, flgp_dev_hk_workspace(m, m, K, 1)));
  return logit_la_on_device(st.s, C.as<double>(), m, Y, N, tol, max_iter, amll, iters, "logit_marginal_likelihood");
}

namespace {
// The argument checks the posterior entries share, under the caller's name; r0 / r1 take the row sets.  `others`: the
// entry's remaining pointers are there.
int posterior_check_rows(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1, int mnew,
                         int max_iter, bool others, Rows &r0, Rows &r1) {
  FLGP_REQUIRE(ep && idx0 && idx1 && others, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && mnew >= 1 && max_iter >= 1,
               "%s: bad shape (K=%d of %d, m=%d, m_new=%d, max_iter=%d)", who, K, ep->K, m, mnew, max_iter);
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  return r1.check(ep, idx1, mnew, who, "idx1");
}
int posterior_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, const int *idx1,
                    int mnew, int max_iter, const double *mean, const double *cov, Rows &r0, Rows &r1) {
  FLGP_TRY(posterior_check_rows(who, ep, K, idx0, m, idx1, mnew, max_iter, Y && mean && cov, r0, r1));
  return check_labels(Y, nullptr, m, who);
}
int posterior_check_sigmas(const char *who, double sigma11, double sigma22) {
  FLGP_REQUIRE(sigma11 >= 0.0 && std::isfinite(sigma11), "%s: sigma11=%g must be finite and >= 0", who, sigma11);
  FLGP_REQUIRE(sigma22 >= 0.0 && std::isfinite(sigma22), "%s: sigma22=%g must be finite and >= 0", who, sigma22);
  return FLGP_OK;
}

// posterior_distribution_classification (src/Utils.cpp:252-299) with C11 = HK(idx0, idx0) + sigma11 I,
// C21 = HK(idx1, idx0) = V2 L V1^T, C22 = rowsum(V2 L .* V2) + sigma22.  mean = V2 L V1^T (Y - pi);
// var_i = C22_i - v2_i^T M v2_i with M = X^T X, X = L_B^-1 sqrt(W) V1 L: O(m_new K^2), C21 is never formed.
// The dense route of the posterior entries: the m x m C11 and B, whatever m is.  On the caller's stream, Y and the two
// results (m_new each) on the device; synchronises.
int posterior_dense_on(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, double t, double sigma11, double sigma22,
                       Rows &r0, int m, const double *dY, Rows &r1, int mnew, double tol, int max_iter, double *dmean,
                       double *dcov, int *iters) {
  GprCtx G;
  FLGP_TRY(G.prepare(st, ep, K, t));                    // G.l = exp(-t (1 - values))
  DevBuf C, work;
  FLGP_TRY(hk_c11(st, ep, K, t, r0, sigma11, C, work, flgp_dev_hk_workspace(m, m, K, 1)));
  // the mode (N = 1), then B factored again at the final f          (src/Utils.cpp:268-293)
  GpcNewton S;
  FLGP_TRY(S.alloc(m));
  int it = 0;
  FLGP_TRY(S.run(st, C.as<double>(), dY, nullptr, tol, max_iter, who, &it));
  if (iters) *iters = it;
  FLGP_TRY(S.weights(st, C.as<double>(), dY, nullptr));
  FLGP_TRY(r0.gather(st, ep, K));
  FLGP_TRY(r1.gather(st, ep, K));
  DevBuf X, Mp, u, Wp, gw;
  const size_t we = (size_t)128 * K * K + 1024;
  FLGP_TRY(X.alloc(sizeof(double) * (size_t)m * K));
  FLGP_TRY(Mp.alloc(sizeof(double) * (size_t)K * (K + 1)));
  FLGP_TRY(u.alloc(sizeof(double) * (size_t)K));
  FLGP_TRY(Wp.alloc(sizeof(double) * (size_t)mnew * (K + 1)));
  FLGP_TRY(gw.alloc(sizeof(double) * we));
  FLGP_TRY(gpc_scale2(st, r0.V, r0.ld, S.sW.as<double>(), G.l.as<double>(), m, K, X.as<double>()));     // sqrt(W) V1 L
  FLGP_TRY(chol_trsv(st, S.B.as<double>(), m, m, X.as<double>(), m, K, 1, S.flag.as<int>()));         // L_B^-1 (.)
  FLGP_TRY(gemm_tn(st, K, K, m, X.as<double>(), m, X.as<double>(), m, Mp.as<double>(), gw.as<double>(), we));        // M = X^T X
  FLGP_TRY(gemm_tn(st, K, 1, m, r0.V, r0.ld, S.resid.as<double>(), m, u.as<double>(), gw.as<double>(), we));         // V1^T (Y - pi)
  FLGP_TRY(gpr_scale(st, u.as<double>(), G.l.as<double>(), nullptr, K, 1, Mp.as<double>() + (size_t)K * K));  // column K: L (.)
  {
    ProfScope ps("posterior_dense_predict", st, 2.0 * mnew * K * (K + 1));
    FLGP_TRY(gemm_nn(st, mnew, K + 1, K, r1.V, r1.ld, Mp.as<double>(), K, Wp.as<double>(), nullptr, 0));        // V2 [M | u]
    FLGP_TRY(gpr_rowquad(st, r1.V, r1.ld, Wp.as<double>(), mnew, K, G.l.as<double>(), sigma22, dcov));
  }
  FLGP_HIP(hipMemcpyAsync(dmean, Wp.as<double>() + (size_t)K * mnew, sizeof(double) * (size_t)mnew, hipMemcpyDeviceToDevice, st));
  int bad = 0;
  FLGP_TRY(read_flag(st, S.flag.p, &bad));
  return GpcNewton::pivot_error(bad, who, 0);      // the loop checked its own factorisations: this is the one at the mode
}

// the binary entries' call of it: a stream of its own, Y up, mean and cov down
int posterior_dense(const char *who, const flgp_eigenpair *ep, int K, double t, double sigma11, double sigma22, Rows &r0, int m,
                    const double *Y, Rows &r1, int mnew, double tol, int max_iter, double *mean, double *cov, int *iters) {
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dY, dmean, dcov;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m, st.s));
  FLGP_TRY(dmean.alloc(sizeof(double) * (size_t)mnew)); FLGP_TRY(dcov.alloc(sizeof(double) * (size_t)mnew));
  FLGP_TRY(posterior_dense_on(st.s, who, ep, K, t, sigma11, sigma22, r0, m, dY.as<double>(), r1, mnew, tol, max_iter,
                              dmean.as<double>(), dcov.as<double>(), iters));
  FLGP_TRY(d2h(mean, dmean.p, sizeof(double) * (size_t)mnew, st.s));
  FLGP_TRY(d2h(cov, dcov.p, sizeof(double) * (size_t)mnew, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}
}  // namespace

extern "C" int flgp_eigenpair_posterior_classification(const flgp_eigenpair *ep, int K, double t, double sigma11, double sigma22,
                                                       const int *idx0, int m, const double *Y, const int *idx1, int mnew,
                                                       double tol, int max_iter, double *mean, double *cov) {
  const char *who = "posterior_classification";
  Rows r0, r1;
  FLGP_TRY(posterior_check(who, ep, K, idx0, m, Y, idx1, mnew, max_iter, mean, cov, r0, r1));
  return posterior_dense(who, ep, K, t, sigma11, sigma22, r0, m, Y, r1, mnew, tol, max_iter, mean, cov, nullptr);
}

// ---- regression training objectives: train_regression_gp_cpp's four objectives on the resident pair.  The
// entries and the Woodbury route (m > K) are with the training context at the end of this file -------------
namespace {
bool all_finite(const double *v, int cnt) {
  for (int a = 0; a < cnt; ++a)
    if (!std::isfinite(v[a])) return false;
  return true;
}
// One evaluation on the direct route (m <= K), on the caller's stream.  It owns every device buffer that RgTerms points
// into, and the steps' scratch, until the result has come down: a step leaves pointers behind, so none of them is a step's
// local.  The caller (flgp_regression_batch::direct_one) fills it.
struct RgDirect {
  hipStream_t st = nullptr;
  const flgp_eigenpair *ep = nullptr;
  Rows r;
  GprCtx G;                                                     // ls = exp(-t lambda / 2) + 0.0
  RgTerms T{};
  const double *x = nullptr;                                    // the host's: t = x[0]; "same": noise = x[1]
  DevBuf dY, dx, alpha, out, ld, Vta, d, s, work;
  DevBuf C, hw, Li, Tb, W;

  // C = HK(idx, idx) + sigma I + (x1 I or diag(x[1..m])), factored; alpha = C^-1 Y        (:362-369, :469-477)
  int terms() {
    const int m = T.m, q = T.q, K = T.K;
    FLGP_TRY(hk_c11(st, ep, K, x[0], r, T.sigma, C, hw, flgp_dev_hk_workspace(m, m, K, 1)));
    FLGP_TRY(T.different ? gpr_add_diag_vec(st, C.as<double>(), m, dx.as<double>() + 1) : gpr_add_diag(st, C.as<double>(), m, x[1]));
    FLGP_TRY(chol_blocked(st, C.as<double>(), m, m, G.flag.as<int>()));
    FLGP_HIP(hipMemcpyAsync(alpha.p, dY.p, sizeof(double) * (size_t)m * q, hipMemcpyDeviceToDevice, st));
    FLGP_TRY(chol_trsv(st, C.as<double>(), m, m, alpha.as<double>(), m, q, 3, G.flag.as<int>()));
    FLGP_TRY(chol_logdet(st, C.as<double>(), m, m, ld.as<double>()));
    if (!T.grad) return FLGP_OK;
    // d_i = (C^-1)_ii, s_k = |(L^-1 V)_{:,k}|^2, V^T alpha
    const size_t wi = (size_t)32 * 64 * m, we = vt_work_elems(K, q);
    FLGP_TRY(Li.alloc(sizeof(double) * (size_t)m * m)); FLGP_TRY(Tb.alloc(sizeof(double) * (size_t)64 * m));
    FLGP_TRY(W.alloc(sizeof(double) * (size_t)m * K)); FLGP_TRY(s.alloc(sizeof(double) * (size_t)K));
    FLGP_TRY(work.alloc(sizeof(double) * std::max(wi, we)));
    FLGP_TRY(tri_inverse(st, C.as<double>(), m, m, Li.as<double>(), m, Tb.as<double>(), work.as<double>(), wi, G.flag.as<int>()));
    FLGP_TRY(rg_colsumsq(st, Li.as<double>(), m, m, m, d.as<double>()));
    FLGP_TRY(r.gather(st, ep, K));
    FLGP_TRY(gemm_nn(st, m, K, m, Li.as<double>(), m, r.V, r.ld, W.as<double>(), nullptr, 0));
    FLGP_TRY(rg_colsumsq(st, W.as<double>(), m, m, K, s.as<double>()));
    return gemm_tn(st, K, q, m, r.V, r.ld, alpha.as<double>(), m, Vta.as<double>(), work.as<double>(), we);
  }
  // rg_assemble on what the steps left, then [value, grad] down
  int finish(const char *who, int nx, double *value, double *grad) {
    T.x = dx.as<double>(); T.Y = dY.as<double>(); T.alpha = alpha.as<double>(); T.logdet = ld.as<double>();
    T.values = (const double *)ep->values.p; T.ls = G.ls.as<double>();
    T.Vta = Vta.as<double>(); T.d = d.as<double>(); T.s = s.as<double>();
    T.out = out.as<double>();
    FLGP_TRY(rg_assemble(st, T));
    std::vector<double> h((size_t)nx + 1);
    FLGP_TRY(d2h(h.data(), out.p, sizeof(double) * h.size(), st));
    FLGP_TRY(G.verdict(st, who));
    if (!all_finite(h.data(), T.grad ? nx + 1 : 1)) return noconv(not_finite(who));
    *value = h[0];
    if (T.grad) std::memcpy(grad, h.data() + 1, sizeof(double) * (size_t)nx);
    return FLGP_OK;
  }
};
}  // namespace

// ---- logit training objective: what train_lae_logit_gp_cpp's COBYLA minimises, on the
// resident pair, for B problems (labels, t) in one call; the single entry is the batch of one ------------------------------
namespace {
inline long pad32(long n) { return (n + 31) / 32 * 32; }     // a slot starts 256-byte aligned, like an allocation of its own

// Alg. 3.1 for m > K on C = V1 L V1^T + sigma I, O(m K^2) per iteration, never an m x m matrix, for a chunk of problems.
// With D = 1 + sigma W and U = sW V1, B = sW C sW + I = D + U L U^T, so with xs = D^-1/2 sW, X = diag(xs) V1 L^1/2 and
// Q = I + X^T X (K x K):  B^-1 y = D^-1 y - D^-1/2 X Q^-1 X^T D^-1/2 y,  det B = det D det Q.  Per iteration:
// sW, b from f; D, X, Q factored (K x K); c = C b; g = xs c; r = B^-1 (sW c) = D^-1/2 (g - X Q^-1 X^T g); a = b - sW r;
// f_new = C a.  As in GpcNewton, a, D and L_Q stay those of the LAST iteration and f is the final mode; everything is
// fixed-order.  Slot s of every buffer belongs to problem p0 + s for the whole chunk, the device list `act` names the slots
// still iterating and every step of an iteration is one launch over that list (gpc.hip, LrChunk), so a problem's bits
// depend on nothing that shares its chunk.  The split products take, per problem, the plan of an unbatched product with a
// workspace of vt_work_elems(K, 1) doubles (planQ for Q = X^T X, planU for the two K x 1 products) on planes of the
// slot's own.  A chunk on several pairs (C.pair, pair_h its host copy) keeps, behind `act`, the pair of every
// listed POSITION for the four products against V1: the batched GEMM finds an operand of a list of its own by position.
struct LrBatch {
  LrChunk C;
  DevBuf vec, kv, X, Q, part, stat, flag, amll, act;
  const int *pair_h = nullptr;   // slot -> pair, where C.pair is set
  std::vector<int> apair;        // the host's side of act_pair()
  int planQ = 1, planU = 1;
  size_t pe = 0;                 // doubles of one slot's planes
  long sp = 0;

  static void plans(int m, int K, int *planQ, int *planU, size_t *pe) {
    const size_t we = vt_work_elems(K, 1);
    *planQ = gemm_plan_split(K, K, m, we);
    *planU = gemm_plan_split(K, 1, m, we);
    *pe = std::max((size_t)*planQ * K * K, (size_t)*planU * K);
  }
  // device bytes of one problem: X, Q, eleven m-vectors, u, l, ls, its planes and its scalars
  static double bytes(int m, int K) {
    int a, b;
    size_t pe;
    plans(m, K, &a, &b, &pe);
    return 8.0 * ((double)pad32((long)m * K) + pad32((long)K * K) + 11.0 * pad32(m) + 3.0 * pad32(K) + pad32((long)pe)) + 32.0;
  }
  int alloc(int m, int K, int slots) {
    C.m = m; C.K = K; C.slots = slots;
    C.sv = pad32(m); C.sk = pad32(K); C.sx = pad32((long)m * K); C.sq = pad32((long)K * K);
    plans(m, K, &planQ, &planU, &pe);
    sp = pad32((long)pe);
    const size_t S = (size_t)slots;
    FLGP_TRY(vec.alloc(sizeof(double) * 11 * S * C.sv)); FLGP_TRY(kv.alloc(sizeof(double) * 3 * S * C.sk));
    FLGP_TRY(X.alloc(sizeof(double) * S * C.sx)); FLGP_TRY(Q.alloc(sizeof(double) * S * C.sq));
    FLGP_TRY(part.alloc(sizeof(double) * S * sp)); FLGP_TRY(stat.alloc(12 * S));
    FLGP_TRY(flag.alloc(sizeof(int) * S)); FLGP_TRY(amll.alloc(sizeof(double) * S)); FLGP_TRY(act.alloc(sizeof(int) * 2 * S));
    apair.assign(S, 0);
    double *v = vec.as<double>(), *k = kv.as<double>();
    const size_t vs = S * C.sv, ks = S * C.sk;
    C.f = v; C.fnew = v + vs; C.sW = v + 2 * vs; C.b = v + 3 * vs; C.a = v + 4 * vs; C.D = v + 5 * vs; C.dh = v + 6 * vs;
    C.xs = v + 7 * vs; C.c = v + 8 * vs; C.g = v + 9 * vs; C.Xv = v + 10 * vs;
    C.u = k; C.l = k + ks; C.ls = k + 2 * ks;
    C.X = X.as<double>(); C.Q = Q.as<double>(); C.flag = flag.as<int>(); C.amll = amll.as<double>();
    return FLGP_OK;
  }
  // the pair of act[q] at position q, or nullptr for a chunk on one pair; batch_newton_loop keeps it beside `act`
  const int *act_pair() const { return C.pair ? (const int *)act.p + apair.size() : nullptr; }
  // C (M x 1) = A^T B or A B per listed slot, as gemm_tn / gemm_nn on the slot's operands (a stride of 0: the shared V1;
  // la: the operand's own list, for V1 of the position's pair)
  int tn(hipStream_t st, int A, const double *Am, long lda, long a_bs, const double *x, double *out, const int *la = nullptr) {
    GemmBatch gb{A, act.as<int>(), a_bs, C.sv, C.sk, 0, sp};
    gb.a_slots = la;
    return gemm_launch(st, C.K, 1, C.m, 1.0, Am, lda, 1, x, 1, C.m, 0.0, nullptr, 0, 0, out, 1, C.K, part.as<double>(), pe, 0.0,
                       nullptr, nullptr, nullptr, planU, nullptr, &gb);
  }
  int nn(hipStream_t st, int A, const double *Am, long lda, long a_bs, const double *u, double *out, const int *la = nullptr) {
    GemmBatch gb{A, act.as<int>(), a_bs, C.sk, C.sv, 0, 0};
    gb.a_slots = la;
    return gemm_launch(st, C.m, 1, C.K, 1.0, Am, 1, lda, u, 1, C.K, 0.0, nullptr, 0, 0, out, 1, C.m, nullptr, 0, 0.0, nullptr,
                       nullptr, nullptr, 0, nullptr, &gb);
  }
  // out = C x = V1 (L (V1^T x)) + sigma x   (Xv is the scratch)
  int cmul(hipStream_t st, int A, const double *x, double *out) {
    const int *a = act.as<int>(), *la = act_pair();
    FLGP_TRY(tn(st, A, C.V1, C.ld1, C.s1, x, C.u, la));
    FLGP_TRY(lrb_mul(st, C.K, C.l, C.sk, C.u, C.sk, C.u, C.sk, a, A));
    FLGP_TRY(nn(st, A, C.V1, C.ld1, C.s1, C.u, C.Xv, la));
    return lrb_axpy(st, C.m, C.Xv, C.sv, C.sigma, x, C.sv, out, C.sv, a, A);
  }
  // one Newton iteration of the A listed slots: every launch once, whatever A is
  int iteration(hipStream_t st, int A) {
    ProfScope ps("logit_lr_batch_iter", st, 0.0);
    const int *a = act.as<int>();
    FLGP_TRY(lrb_w(st, C, a, A));                                                             // sW, b
    FLGP_TRY(lrb_d(st, C, a, A));                                                             // D, dh, xs
    FLGP_TRY(lrb_scale2(st, C, a, A));                                                        // X, then Q = I + X^T X = L_Q L_Q^T
    {
      const GemmBatch gb{A, a, C.sx, C.sx, C.sq, 0, sp};
      FLGP_TRY(gemm_launch(st, C.K, C.K, C.m, 1.0, C.X, C.m, 1, C.X, 1, C.m, 0.0, nullptr, 0, 0, C.Q, 1, C.K, part.as<double>(), pe,
                           0.0, nullptr, nullptr, nullptr, planQ, nullptr, &gb));
    }
    FLGP_TRY(lrb_add_diag(st, C, a, A));
    FLGP_TRY(lrb_chol(st, C, a, A));
    FLGP_TRY(cmul(st, A, C.b, C.c));                                                          // c = C b
    FLGP_TRY(lrb_mul(st, C.m, C.xs, C.sv, C.c, C.sv, C.g, C.sv, a, A));                       // g = D^-1/2 sW c
    FLGP_TRY(tn(st, A, C.X, C.m, C.sx, C.g, C.u));                                            // Xv = X Q^-1 X^T g
    FLGP_TRY(lrb_trsv(st, C, a, A));
    FLGP_TRY(nn(st, A, C.X, C.m, C.sx, C.u, C.Xv));
    FLGP_TRY(lrb_a(st, C, a, A));                                                             // a = b - sW dh (g - Xv)
    FLGP_TRY(cmul(st, A, C.a, C.fnew));                                                       // f_new = C a
    return lrb_step(st, C, a, A, stat.as<double>());
  }
};

// bad_of / iter_of (optional, one entry per slot of the chunk): every failing slot's flag and iteration, for a caller that
// reports per problem
struct BatchFailure { int problem = -1, bad = 0, iter = 0; int *bad_of = nullptr, *iter_of = nullptr; };

// The host side of a chunk's Newton loops, the objective's (lr_batch_chunk) and the posterior's (ws_batch_chunk): the chunk
// [p0, p0 + S) from f = 0, `iteration(A)` one Newton iteration of the A listed slots.  After every iteration the host reads
// the A norms and the A flags (12 A bytes), notes the iteration count of every listed problem and takes the converged ones
// (norm < tol) and the failed ones (a pivot flag) off the list: GpcNewton::run's protocol per problem; nothing writes a
// slot that left.  fail: the lowest failing problem; its: the S counts.  d_all (or nullptr): a device list that gets
// 0 .. S-1, for the steps that follow the loop on every slot.  d_values: the pair's eigenvalues, or, for a chunk on several
// pairs (C.pair), every pair's at stride C.sk; such a chunk's list goes up with the pair of every position behind it.
template <class Iteration>
int batch_newton_loop(hipStream_t st, LrBatch &L, const double *d_values, const double *d_ts, int S, double tol, int max_iter,
                      int p0, int *its, BatchFailure &fail, int *d_all, Iteration iteration) {
  LrChunk &C = L.C;
  C.slots = S;
  FLGP_TRY(lrb_weights(st, d_values, C.pair, C.K, d_ts, S, C.sk, C.ls, C.l));
  FLGP_HIP(hipMemsetAsync(C.f, 0, sizeof(double) * (size_t)S * C.sv, st));
  FLGP_HIP(hipMemsetAsync(C.flag, 0, sizeof(int) * (size_t)S, st));
  std::vector<int> act((size_t)S), next;
  for (int s = 0; s < S; ++s) act[(size_t)s] = s;
  if (d_all) {
    FLGP_TRY(h2d(d_all, act.data(), sizeof(int) * (size_t)S, st));
    FLGP_HIP(hipStreamSynchronize(st));          // `act` changes below: the copy has read it
  }
  std::vector<double> stat((size_t)S * 2);       // 12 A bytes are read into it: A doubles, then A ints
  bool changed = true;
  for (int it = 0; it < max_iter && !act.empty(); ++it) {
    const int A = (int)act.size();
    if (changed) FLGP_TRY(h2d(L.act.p, act.data(), sizeof(int) * (size_t)A, st));
    if (changed && C.pair) {                     // read, like `act`, before the wait below, and not written until after it
      for (int q = 0; q < A; ++q) L.apair[(size_t)q] = L.pair_h[act[(size_t)q]];
      FLGP_TRY(h2d((void *)L.act_pair(), L.apair.data(), sizeof(int) * (size_t)A, st));
    }
    FLGP_TRY(iteration(A));
    FLGP_TRY(d2h(stat.data(), L.stat.p, (size_t)12 * A, st));
    FLGP_HIP(hipStreamSynchronize(st));
    const int *bad = (const int *)(stat.data() + A);
    next.clear();
    for (int q = 0; q < A; ++q) {
      const int s = act[(size_t)q];
      its[s] = it + 1;
      if (bad[q]) {
        if (fail.bad_of) { fail.bad_of[s] = bad[q]; fail.iter_of[s] = it + 1; }
        if (fail.problem < 0 || p0 + s < fail.problem) { fail.problem = p0 + s; fail.bad = bad[q]; fail.iter = it + 1; }
      } else if (!(stat[(size_t)q] < tol)) {
        next.push_back(s);
      }
    }
    changed = next.size() != act.size();
    act.swap(next);
  }
  return FLGP_OK;
}

// The objective's chunk: the loops, then the final sums for every slot.  amll_h / its: the S results.
int lr_batch_chunk(hipStream_t st, LrBatch &L, const double *d_values, const double *d_ts, int S, double tol, int max_iter,
                   int p0, double *amll_h, int *its, BatchFailure &fail) {
  FLGP_TRY(batch_newton_loop(st, L, d_values, d_ts, S, tol, max_iter, p0, its, fail, nullptr, [&](int A) { return L.iteration(st, A); }));
  FLGP_TRY(lrb_amll(st, L.C));
  FLGP_TRY(d2h(amll_h, L.C.amll, sizeof(double) * (size_t)S, st));
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// what a worker of the dense route (m <= K) owns: its C, the contraction's workspace and the loop's state
struct DenseObjWorker {
  DevBuf C, work;
  GpcNewton S;
  int alloc(int m, int K) {
    FLGP_TRY(C.alloc(sizeof(double) * (size_t)m * m));
    FLGP_TRY(work.alloc(flgp_dev_hk_workspace(m, m, K, 1)));
    return S.alloc(m);
  }
  static double bytes(int m, int K) { return 8.0 * (2.0 * m * m + 8.0 * m) + (double)flgp_dev_hk_workspace(m, m, K, 1); }
  // one problem: C = HK(r, r) + sigma I at t (src/train.cpp:30-31; a zero sigma launches nothing: the diagonal of HK(r, r)
  // is a sum of squares, never -0), GpcNewton's loop on it and the final sums
  int objective(hipStream_t st, const flgp_eigenpair *ep, int K, double t, const Rows &r, double sigma, const double *dY,
                const double *dN, double tol, int max_iter, const char *who, int *iters, double *amll) {
    FLGP_TRY(hk(st, ep, K, t, r, r, C.as<double>(), work.as<double>()));
    if (sigma != 0.0) FLGP_TRY(gpr_add_diag(st, C.as<double>(), r.m, sigma));
    FLGP_TRY(S.run(st, C.as<double>(), dY, dN, tol, max_iter, who, iters));
    return S.amll(st, dY, dN, amll);
  }
};

// The checks the two entries word alike, under the caller's name; each entry calls them at its own place among its others.
int objective_approach(const char *who, const char *approach, bool *posterior) {
  FLGP_REQUIRE(approach, "%s: null pointer", who);
  *posterior = std::strcmp(approach, "posterior") == 0;
  if (!*posterior && std::strcmp(approach, "marginal") != 0) {
    set_error("This model selection approach is not supported!");
    return FLGP_ERR_UNSUPPORTED;
  }
  return FLGP_OK;
}
// sigma, then pr = the caller's prior (p, q, tau) or PostOFData's defaults (src/train.h:138-140)
int objective_sigma_prior(const char *who, double sigma, const double *prior, double *pr) {
  FLGP_REQUIRE(sigma >= 0.0 && std::isfinite(sigma), "%s: sigma=%g must be finite and >= 0", who, sigma);
  const double dflt[3] = {1e-2, 10.0, 2.0};
  for (int k = 0; k < 3; ++k) pr[k] = prior ? prior[k] : dflt[k];
  FLGP_REQUIRE(all_finite(pr, 3), "%s: prior (p, q, tau) must be finite", who);
  return FLGP_OK;
}

// negative_marginal_likelihood_logit_cpp / negative_log_posterior_logit_cpp (src/train.cpp:14-34) from the loop's amll
double logit_objective_value(bool posterior, const double *pr, double t, double amll) {
  const double p = posterior ? pr[0] * std::log(t + 1e-9) + std::pow(t / pr[2], -pr[1]) : 0.0;
  return posterior ? -amll + p : -amll;
}

// The B checked problems on the checked rows r: problem b is column col[b] of Y (r.m x ncol; col NULL: column b) at ts[b],
// N NULL is one trial per row (the one-vs-rest route, src/MultiClassification.cpp:36).  A problem that fails is reported
// as "problem b (t=..): <text>" (by_problem, the batch entry's form) or with the text alone.  values and iters (may be
// NULL) are written on success only.
int logit_objectives(const char *who, bool by_problem, const flgp_eigenpair *ep, int K, Rows &r, const double *Y, int ncol,
                     const double *N, const int *col, const double *ts, int B, double sigma, bool posterior, const double *pr,
                     double tol, int max_iter, int max_parallel, double *values, int *iters) {
  const int m = r.m;
  std::vector<double> ones;
  if (!N) { ones.assign((size_t)m, 1.0); N = ones.data(); }
  std::vector<int> cols((size_t)B);
  for (int b = 0; b < B; ++b) cols[(size_t)b] = col ? col[b] : b;
  auto name_failure = [&](int b, const std::string &msg) {
    if (by_problem) set_error("problem %d (t=%g): %s", b, ts[b], msg.c_str());
    else set_error("%s", msg.c_str());
  };

  Stream st;
  FLGP_TRY(st.create());
  // up once: the rows, Y, N and, for the batched loop, the problems' columns and values of t
  DevBuf dY, dN;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m * ncol, st.s));
  FLGP_TRY(upload(dN, N, sizeof(double) * (size_t)m, st.s));
  std::vector<double> amll((size_t)B, 0.0);
  std::vector<int> its((size_t)B, 0);
  if (m <= K) {
    // the dense loop per problem, the problems dealt to the pool's workers (worker_pool.h); one worker runs on st
    FLGP_TRY(r.resolve(st.s));
    FLGP_HIP(hipStreamSynchronize(st.s));
    DevicePool pool;
    FLGP_TRY(pool.plan(max_parallel, B, DenseObjWorker::bytes(m, K)));
    const PoolFailure bad = pool.run<DenseObjWorker>(
        st.s, B, [&](DenseObjWorker &W) { return W.alloc(m, K); },
        [&](hipStream_t ws, DenseObjWorker &W, int b) -> int {
          return W.objective(ws, ep, K, ts[b], r, sigma, dY.as<double>() + (size_t)cols[(size_t)b] * m, dN.as<double>(), tol,
                             max_iter, who, &its[(size_t)b], &amll[(size_t)b]);
        });
    if (bad.item >= 0) { name_failure(bad.item, bad.message); return bad.status; }
  } else {
    FLGP_TRY(r.gather(st.s, ep, K));
    DevBuf dcol, dts;
    FLGP_TRY(upload(dcol, cols.data(), sizeof(int) * (size_t)B, st.s));
    FLGP_TRY(upload(dts, ts, sizeof(double) * (size_t)B, st.s));
    // the chunk: max_parallel problems, or (<= 0) all of them; where that is more than one, no more than fit into 90 % of
    // the free memory
    const int want = max_parallel > 0 ? max_parallel : B;
    size_t free_b = 0, total_b = 0;
    if (plan_workers(want, B, 0.0, 0.0) > 1) FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
    const int chunk = std::min(plan_workers(want, B, (double)free_b, LrBatch::bytes(m, K)), GEMM_BATCH_MAX);
    LrBatch L;
    FLGP_TRY(L.alloc(m, K, chunk));
    L.C.Y = dY.as<double>(); L.C.ldy = m; L.C.N = dN.as<double>();
    L.C.V1 = r.V; L.C.ld1 = r.ld; L.C.sigma = sigma;
    for (int p0 = 0; p0 < B; p0 += chunk) {
      const int S = std::min(chunk, B - p0);
      L.C.ycol = dcol.as<int>() + p0;
      BatchFailure fail;
      FLGP_TRY(lr_batch_chunk(st.s, L, (const double *)ep->values.p, dts.as<double>() + p0, S, tol, max_iter, p0, amll.data() + p0,
                              its.data() + p0, fail));
      if (fail.problem >= 0) {
        const int rc = GpcNewton::pivot_error(fail.bad, who, fail.iter);
        name_failure(fail.problem, std::string(flgp_last_error()));
        return rc;
      }
    }
  }
  for (int b = 0; b < B; ++b) {
    values[b] = logit_objective_value(posterior, pr, ts[b], amll[(size_t)b]);
    if (iters) iters[b] = its[(size_t)b];
  }
  return FLGP_OK;
}
}  // namespace

// The single entry is the batch of one: one problem, one chunk of one slot (m > K) or one worker on the entry's stream.
extern "C" int flgp_eigenpair_logit_objective(const flgp_eigenpair *ep, int K, const int *idx, int m, const double *Y,
                                              const double *N, double sigma, const char *approach, const double *prior,
                                              double t, double tol, int max_iter, double *value, int *iters) {
  const char *who = "logit_objective";
  bool posterior = false;
  double pr[3];
  FLGP_TRY(objective_approach(who, approach, &posterior));
  FLGP_REQUIRE(ep && idx && Y && value, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && max_iter >= 1, "%s: bad shape (K=%d of %d, m=%d, max_iter=%d)", who, K, ep->K,
               m, max_iter);
  Rows r;
  FLGP_TRY(r.check(ep, idx, m, who, "idx"));
  FLGP_TRY(check_labels(Y, N, m, who));
  FLGP_REQUIRE(std::isfinite(t), "%s: t=%g must be finite", who, t);
  FLGP_REQUIRE(!posterior || t > 0.0, "%s: t=%g must be positive under \"posterior\"", who, t);
  FLGP_TRY(objective_sigma_prior(who, sigma, prior, pr));
  return logit_objectives(who, false, ep, K, r, Y, 1, N, nullptr, &t, 1, sigma, posterior, pr, tol, max_iter, 1, value, iters);
}

extern "C" int flgp_eigenpair_logit_objective_batch(const flgp_eigenpair *ep, int K, const int *idx, int m, const double *Y,
                                                    int ncol, const double *N, const int *col, const double *ts, int B,
                                                    double sigma, const char *approach, const double *prior, double tol,
                                                    int max_iter, int max_parallel, double *values, int *iters) {
  const char *who = "logit_objective_batch";
  bool posterior = false;
  double pr[3];
  FLGP_TRY(objective_approach(who, approach, &posterior));
  FLGP_REQUIRE(ep && idx && Y && ts && values, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && max_iter >= 1 && B >= 1 && ncol >= 1,
               "%s: bad shape (K=%d of %d, m=%d, max_iter=%d, B=%d, ncol=%d)", who, K, ep->K, m, max_iter, B, ncol);
  FLGP_REQUIRE(col || ncol == B, "%s: col may be NULL only if ncol == B (ncol=%d, B=%d)", who, ncol, B);
  for (int b = 0; b < B; ++b) {
    const int c = col ? col[b] : b;
    FLGP_REQUIRE(c >= 0 && c < ncol, "problem %d (t=%g): %s: col=%d is outside [0, ncol=%d)", b, ts[b], who, c, ncol);
    FLGP_REQUIRE(std::isfinite(ts[b]), "problem %d (t=%g): %s: t must be finite", b, ts[b], who);
    FLGP_REQUIRE(!posterior || ts[b] > 0.0, "problem %d (t=%g): %s: t must be positive under \"posterior\"", b, ts[b], who);
  }
  FLGP_TRY(objective_sigma_prior(who, sigma, prior, pr));
  Rows r;
  FLGP_TRY(r.check(ep, idx, m, who, "idx"));
  for (int c = 0; c < ncol; ++c) FLGP_TRY(check_labels(Y + (size_t)c * m, N, m, who));
  return logit_objectives(who, true, ep, K, r, Y, ncol, N, col, ts, B, sigma, posterior, pr, tol, max_iter, max_parallel, values,
                          iters);
}


// ---- logit posterior: the binary entry, the one-vs-rest entries and the batch entry on one body; for
// m > K the mode in weight space for a chunk of problems in shared launches, the predictive rows in one pass ---------------
namespace {
// mean_i = u^T v2_i, cov_i = sigma22 + |G v2_i|^2 for the rows r1 of the pair (G K x K lower triangular, u K; device
// pointers, as dmean / dcov) where K is too wide for the fused kernel (gpc_predict_rows_applicable): Z = V2 G^T by the
// MFMA GEMM and its row sums of squares, in row blocks that keep Z (and the gathered rows of an index set) at 256 MB each.
int predict_rows_wide(hipStream_t st, const flgp_eigenpair *ep, int K, Rows &r1, const double *G, const double *u, double sigma22,
                      double *dmean, double *dcov) {
  FLGP_TRY(r1.resolve(st));
  const double *dvec = (const double *)ep->vectors.p;
  ProfScope ps("gpc_predict_rows_wide", st, 2.0 * r1.m * K * (K + 1));
  const int rb = (int)std::min<size_t>((size_t)r1.m, std::max<size_t>(64, (((size_t)256 << 20) / (sizeof(double) * K)) / 64 * 64));
  DevBuf Z, Vb;
  FLGP_TRY(Z.alloc(sizeof(double) * (size_t)rb * K));
  if (r1.d) FLGP_TRY(Vb.alloc(sizeof(double) * (size_t)rb * K));
  for (int o = 0; o < r1.m; o += rb) {
    const int rows = std::min(rb, r1.m - o);
    const double *V = dvec + r1.row0 + o;
    long ld = ep->n;
    if (r1.d) {
      FLGP_TRY(flgp_dev_gather_rows(st, dvec, ep->n, r1.d + o, rows, K, Vb.as<double>()));
      V = Vb.as<double>(); ld = rows;
    }
    FLGP_TRY(gemm_launch(st, rows, K, K, 1.0, V, 1, ld, G, K, 1, 0.0, nullptr, 0, 0, Z.as<double>(), 1, rows, nullptr, 0, 0.0,
                         nullptr));                                                                   // Z = V2 G^T
    FLGP_TRY(gpc_rowsumsq_add(st, Z.as<double>(), rows, rows, K, sigma22, dcov + o));
    FLGP_TRY(gemm_nn(st, rows, 1, K, V, ld, u, K, dmean + o, nullptr, 0));
  }
  return FLGP_OK;
}

// The weight-space Newton loop of the posterior for a chunk of problems.  Alg. 3.1's step written as a = (I + W C)^-1 b on
// C = V1 L V1^T + sigma I, which gives Phi^T a = Q^-1 Phi^T D^-1 b exactly (Phi = V1 L^1/2, D = 1 + sigma W,
// X = diag(sqrt(W / D)) Phi, Q = I + X^T X).  Per iteration from f = 0, N = 1:
//   W, b from f; D, xs; Q factored;  beta = Q^-1 L^1/2 V1^T (b / D);  p = V1 L^1/2 beta;  f_new = p + sigma (b - W p) / D.
// Unlike LrBatch's a = b - sW dh (g - X Q^-1 X^T g), whose difference of two nearly equal vectors costs the mean
// m lambda / 4 in relative accuracy (harmless for amll, which is stationary at the mode), the one subtraction here is
// multiplied by sigma.  solve() is also the final step at the mode: beta there gives mean_i = v2_i^T L^1/2 beta.
// It runs on LrBatch's slots, lists and planes: slot s of every buffer belongs to problem p0 + s for the whole chunk and
// every step of an iteration is one launch over the device list of the slots still iterating, so a problem's bits depend
// on nothing that shares its chunk.  Of the chunk's m-vectors c holds b / D and g holds p; u holds beta and then
// L^1/2 beta (a and Xv are not used).  The products take LrBatch's plans.  Beside the loop's state a slot owns L_Q^-1 (Li),
// the 64 x K block and the planes of the triangular inverse, and its predictive operand.
struct WsBatch {
  LrBatch L;
  DevBuf Li, Tb, tpart, Gf, all;
  size_t wi = 0, tpe = 0, ge = 0;
  long stb = 0, stp = 0;

  // device bytes of one problem: LrBatch's (X, Q, the m-vectors, u, l, ls, the loop's planes), L_Q^-1, the 64 x K block,
  // the inverse's planes, the operand and two output columns
  static double bytes(int m, int K, int mnew) {
    const size_t wi = (size_t)32 * 64 * K;
    return LrBatch::bytes(m, K) + 8.0 * ((double)pad32((long)K * K) + pad32((long)64 * K) +
                                         pad32((long)wsb_tri_inverse_planes(K, wi)) + (double)gpc_predict_operand_elems(K) +
                                         2.0 * mnew) + 4.0;
  }
  int alloc(int m, int K, int slots, bool fused) {
    FLGP_TRY(L.alloc(m, K, slots));
    wi = (size_t)32 * 64 * K;                                  // bounds the inverse's splits: its value fixes the bits
    tpe = wsb_tri_inverse_planes(K, wi);
    stb = pad32((long)64 * K); stp = pad32((long)tpe);
    ge = gpc_predict_operand_elems(K);
    const size_t S = (size_t)slots;
    FLGP_TRY(Li.alloc(sizeof(double) * S * L.C.sq)); FLGP_TRY(Tb.alloc(sizeof(double) * S * stb));
    FLGP_TRY(tpart.alloc(sizeof(double) * std::max<size_t>(S * stp, 1)));
    if (fused) FLGP_TRY(Gf.alloc(sizeof(double) * S * ge));
    return all.alloc(sizeof(int) * S);
  }
  // on the A listed slots: W, b, D, X and L_Q at the current f, then u = beta = Q^-1 L^1/2 V1^T (b / D)
  int solve(hipStream_t st, const int *a, int A) {
    LrChunk &C = L.C;
    FLGP_TRY(wsb_w(st, C, a, A));                                                             // sW, b
    FLGP_TRY(lrb_d(st, C, a, A));                                                             // D, dh, xs
    FLGP_TRY(lrb_scale2(st, C, a, A));                                                        // X, then Q = I + X^T X = L_Q L_Q^T
    {
      const GemmBatch gb{A, a, C.sx, C.sx, C.sq, 0, L.sp};
      FLGP_TRY(gemm_launch(st, C.K, C.K, C.m, 1.0, C.X, C.m, 1, C.X, 1, C.m, 0.0, nullptr, 0, 0, C.Q, 1, C.K, L.part.as<double>(),
                           L.pe, 0.0, nullptr, nullptr, nullptr, L.planQ, nullptr, &gb));
    }
    FLGP_TRY(lrb_add_diag(st, C, a, A));
    FLGP_TRY(lrb_chol(st, C, a, A));
    FLGP_TRY(wsb_bd(st, C, a, A));                                                            // c = b / D
    FLGP_TRY(tn(st, a, A, C.c, C.u));                                                         // V1^T (.)
    FLGP_TRY(lrb_mul(st, C.K, C.ls, C.sk, C.u, C.sk, C.u, C.sk, a, A));                       // L^1/2 (.)
    return lrb_trsv(st, C, a, A);                                                             // beta
  }
  // LrBatch::tn / nn against the shared V1 with the list given (the final step runs on every slot, not on the loop's list)
  int tn(hipStream_t st, const int *a, int A, const double *x, double *out) {
    LrChunk &C = L.C;
    const GemmBatch gb{A, a, 0, C.sv, C.sk, 0, L.sp};
    return gemm_launch(st, C.K, 1, C.m, 1.0, C.V1, C.ld1, 1, x, 1, C.m, 0.0, nullptr, 0, 0, out, 1, C.K, L.part.as<double>(), L.pe,
                       0.0, nullptr, nullptr, nullptr, L.planU, nullptr, &gb);
  }
  int nn(hipStream_t st, const int *a, int A, const double *u, double *out) {
    LrChunk &C = L.C;
    const GemmBatch gb{A, a, 0, C.sk, C.sv, 0, 0};
    return gemm_launch(st, C.m, 1, C.K, 1.0, C.V1, 1, C.ld1, u, 1, C.K, 0.0, nullptr, 0, 0, out, 1, C.m, nullptr, 0, 0.0, nullptr,
                       nullptr, nullptr, 0, nullptr, &gb);
  }
  // u <- L^1/2 beta
  int scaled_beta(hipStream_t st, const int *a, int A) {
    LrChunk &C = L.C;
    return lrb_mul(st, C.K, C.ls, C.sk, C.u, C.sk, C.u, C.sk, a, A);
  }
  // one Newton iteration of the A listed slots: every launch once, whatever A is
  int iteration(hipStream_t st, int A) {
    ProfScope ps("logit_ws_batch_iter", st, 0.0);
    LrChunk &C = L.C;
    const int *a = L.act.as<int>();
    FLGP_TRY(solve(st, a, A));
    FLGP_TRY(scaled_beta(st, a, A));
    FLGP_TRY(nn(st, a, A, C.u, C.g));                                                         // p = V1 L^1/2 beta
    FLGP_TRY(wsb_fnew(st, C, a, A));                                                          // f_new = p + sigma (b - W p) / D
    return lrb_step(st, C, a, A, L.stat.as<double>());
  }
  // The final step for every slot 0 .. S-1: the weights once more at the final f (as GpcNewton::weights in the dense
  // route), L_Q, beta,
  // u = L^1/2 beta, Li = L_Q^-1 L^1/2, and (fused) the slot's operand [Li ; u^T]
  int operands(hipStream_t st, int S) {
    LrChunk &C = L.C;
    const int *a = all.as<int>();
    FLGP_TRY(solve(st, a, S));
    FLGP_TRY(scaled_beta(st, a, S));
    FLGP_TRY(wsb_tri_inverse(st, C, a, S, Li.as<double>(), Tb.as<double>(), stb, tpart.as<double>(), tpe, stp, wi));
    FLGP_TRY(wsb_scale_cols(st, C, a, S, Li.as<double>()));
    return Gf.p ? wsb_predict_prep(st, C, a, S, Li.as<double>(), Gf.as<double>()) : FLGP_OK;
  }
};

// The posterior's chunk [p0, p0 + S): the loops, then the final step for every slot and its pivot flags (iter 0: the
// factorisation at the mode).  A chunk with a failure in the loop skips the final step, so fail is the lowest problem that
// failed in the loop or, if none did, the lowest that failed at the mode.  its: the S counts.  r1 (optional), the rows the caller
// predicts for next, are resolved while the device runs the final step: the scan of a long idx1 costs the host alone.
int ws_batch_chunk(hipStream_t st, WsBatch &W, const flgp_eigenpair *ep, const double *d_ts, int S, double tol, int max_iter,
                   int p0, int *its, BatchFailure &fail, Rows *r1) {
  FLGP_TRY(batch_newton_loop(st, W.L, (const double *)ep->values.p, d_ts, S, tol, max_iter, p0, its, fail, W.all.as<int>(),
                             [&](int A) { return W.iteration(st, A); }));
  if (fail.problem >= 0) return FLGP_OK;
  FLGP_TRY(W.operands(st, S));
  if (r1) FLGP_TRY(r1->resolve(st));
  std::vector<int> flags((size_t)S, 0);
  FLGP_TRY(d2h(flags.data(), W.L.C.flag, sizeof(int) * (size_t)S, st));
  FLGP_HIP(hipStreamSynchronize(st));
  for (int s = 0; s < S; ++s)
    if (flags[(size_t)s]) { fail.problem = p0 + s; fail.bad = flags[(size_t)s]; fail.iter = 0; break; }
  return FLGP_OK;
}

// The weight-space route of B problems on the checked rows r0: V1 gathered once, then chunks of max_parallel problems (<= 0:
// all B; where that is more than one, no more than fit into 90 % of the free memory, a problem counted with the rows r1 it
// predicts for), each run to its operands (ws_batch_chunk; `fused`: with the fused kernel's form of them) and handed to
// `each` (p0, S, W) while they are valid.  The posterior entries predict the rows r1 there, the predictor folds the
// operands into its anchor side (r1 == nullptr): one loop, the same launches.  A failing chunk ends the call as logit_posteriors says.
template <class Each>
int ws_chunks(hipStream_t st, const char *who, bool by_class, const flgp_eigenpair *ep, int K, Rows &r0, Rows *r1, const double *dY,
              const int *cols, const double *ts, int B, double sigma11, double tol, int max_iter, int max_parallel, bool fused,
              int *its, BatchFailure &fail, Each each) {
  const int m = r0.m, mnew = r1 ? r1->m : 0;
  FLGP_TRY(r0.gather(st, ep, K));
  DevBuf dcol, dts;
  FLGP_TRY(upload(dcol, cols, sizeof(int) * (size_t)B, st));
  FLGP_TRY(upload(dts, ts, sizeof(double) * (size_t)B, st));
  const int want = max_parallel > 0 ? max_parallel : B;
  size_t free_b = 0, total_b = 0;
  if (plan_workers(want, B, 0.0, 0.0) > 1) FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
  const int chunk = std::min(plan_workers(want, B, (double)free_b, WsBatch::bytes(m, K, mnew)), GEMM_BATCH_MAX);
  WsBatch W;
  FLGP_TRY(W.alloc(m, K, chunk, fused));
  LrChunk &C = W.L.C;
  C.Y = dY; C.ldy = m; C.N = nullptr;
  C.V1 = r0.V; C.ld1 = r0.ld; C.sigma = sigma11;
  for (int p0 = 0; p0 < B; p0 += chunk) {
    const int S = std::min(chunk, B - p0);
    C.ycol = dcol.as<int>() + p0;
    FLGP_TRY(ws_batch_chunk(st, W, ep, dts.as<double>() + p0, S, tol, max_iter, p0, its + p0, fail, r1));
    if (fail.problem >= 0) {
      char name[64];
      std::snprintf(name, sizeof(name), "%s: class %d", who, fail.problem);
      return GpcNewton::pivot_error(fail.bad, by_class ? name : who, fail.iter);
    }
    FLGP_TRY(each(p0, S, W));
  }
  return FLGP_OK;
}

// The B checked problems on the checked rows r0 / r1, on the entry's stream: problem b is column cols[b] of dY (r0.m x ncol
// on the device) at ts[b]; column b of dmean / dcov (r1.m x B on the device) and its[b] (host) are its results.
// m <= K: the dense body per problem, one after another.  m > K: V1 gathered once, then chunks of max_parallel problems
// (<= 0: all B; where that is more than one, no more than fit into 90 % of the free memory), each with one fused pass over
// the rows r1 for all its operands (the wide route: per slot).
// A problem that fails ends the call: fail.problem names it -- the first on the dense route, the lowest of the first
// failing chunk otherwise (ws_batch_chunk) -- and fail.iter is 0 for the factorisation at the mode, which follows a loop
// whose count is in its[], and otherwise the loop's iteration (-1 on the dense route: in its loop).  The status is returned
// and the text is the failure's under the problem's name: `who`, or "<who>: class <b>" (by_class).
int logit_posteriors(hipStream_t st, const char *who, bool by_class, const flgp_eigenpair *ep, int K, Rows &r0, Rows &r1,
                     const double *dY, const int *cols, const double *ts, int B, double sigma11, double sigma22, double tol,
                     int max_iter, int max_parallel, double *dmean, double *dcov, int *its, BatchFailure &fail) {
  const int m = r0.m, mnew = r1.m;
  const size_t colb = (size_t)mnew;
  char name[64];
  auto name_of = [&](int b) -> const char * {
    if (!by_class) return who;
    std::snprintf(name, sizeof(name), "%s: class %d", who, b);
    return name;
  };
  if (m <= K) {
    for (int b = 0; b < B; ++b) {
      its[b] = 0;
      const int rc = posterior_dense_on(st, name_of(b), ep, K, ts[b], sigma11, sigma22, r0, m, dY + (size_t)cols[b] * m, r1, mnew,
                                        tol, max_iter, dmean + b * colb, dcov + b * colb, &its[b]);
      if (rc != FLGP_OK) { fail.problem = b; fail.iter = its[b] > 0 ? 0 : -1; return rc; }
    }
    return FLGP_OK;
  }
  const bool fused = gpc_predict_rows_applicable(K);
  return ws_chunks(st, who, by_class, ep, K, r0, &r1, dY, cols, ts, B, sigma11, tol, max_iter, max_parallel, fused, its, fail,
                   [&](int p0, int S, WsBatch &W) -> int {
                     const LrChunk &C = W.L.C;
                     double *cm = dmean + p0 * colb, *cc = dcov + p0 * colb;
                     if (fused)      // one pass over the rows idx1 of the pair for the chunk's S operands
                       return gpc_predict_rows_multi(st, (const double *)ep->vectors.p, ep->n, r1.d, r1.row0, mnew, K, S,
                                                     W.Gf.as<double>(), sigma22, cm, cc, (long)mnew);
                     for (int s = 0; s < S; ++s)
                       FLGP_TRY(predict_rows_wide(st, ep, K, r1, W.Li.as<double>() + s * C.sq, C.u + s * C.sk, sigma22, cm + s * colb,
                                                  cc + s * colb));
                     return FLGP_OK;
                   });
}
}  // namespace

// The binary entry is the batch of one: one problem, one chunk of one slot (m > K) or one run of the dense body.
extern "C" int flgp_eigenpair_logit_posterior(const flgp_eigenpair *ep, int K, double t, double sigma11, double sigma22,
                                              const int *idx0, int m, const double *Y, const int *idx1, int mnew, double tol,
                                              int max_iter, double *mean, double *cov, int *iters) {
  const char *who = "logit_posterior";
  Rows r0, r1;
  FLGP_TRY(posterior_check(who, ep, K, idx0, m, Y, idx1, mnew, max_iter, mean, cov, r0, r1));
  FLGP_REQUIRE(std::isfinite(t), "%s: t=%g must be finite", who, t);
  FLGP_TRY(posterior_check_sigmas(who, sigma11, sigma22));

  Stream st;
  FLGP_TRY(st.create());
  const size_t nb = sizeof(double) * (size_t)mnew;
  DevBuf dY, dmean, dcov;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m, st.s));
  FLGP_TRY(dmean.alloc(nb)); FLGP_TRY(dcov.alloc(nb));
  const int col = 0;
  int it = 0;
  BatchFailure fail;
  const int rc = logit_posteriors(st.s, who, false, ep, K, r0, r1, dY.as<double>(), &col, &t, 1, sigma11, sigma22, tol, max_iter,
                                  1, dmean.as<double>(), dcov.as<double>(), &it, fail);
  // the count is the loop's: it is there before the factorisation at the mode is looked at
  if (iters && (rc == FLGP_OK || (fail.problem == 0 && fail.iter == 0))) *iters = it;
  if (rc != FLGP_OK) return rc;
  FLGP_TRY(d2h(mean, dmean.p, nb, st.s));
  FLGP_TRY(d2h(cov, dcov.p, nb, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

// ---- one-vs-rest logit posterior: the batch of J on the indicator matrix ---------------------------------
namespace {
// The shared body of the two entries.  nll == nullptr: flgp_eigenpair_logit_posterior_multiclass (mean and cov wanted).
int posterior_multiclass(const flgp_eigenpair *ep, int K, const double *ts, int J, double sigma11, double sigma22, const int *idx0,
                         int m, const double *Y, const int *idx1, int mnew, double tol, int max_iter, int max_parallel,
                         double *mean, double *cov, int *iters, const double *target, int n_samples, unsigned long long seed,
                         double *nll) {
  const char *who = "logit_posterior_multiclass";
  FLGP_REQUIRE(J >= 1, "%s: J=%d must be at least 1", who, J);
  Rows r0, r1;
  const bool outputs = nll ? (target && !mean == !cov) : (mean && cov);
  FLGP_TRY(posterior_check_rows(who, ep, K, idx0, m, idx1, mnew, max_iter, ts && Y && outputs, r0, r1));
  for (int j = 0; j < J; ++j) FLGP_REQUIRE(std::isfinite(ts[j]), "%s: ts[%d]=%g must be finite", who, j, ts[j]);
  FLGP_TRY(posterior_check_sigmas(who, sigma11, sigma22));
  FLGP_TRY(check_class_labels(who, "Y", Y, m, J, false));
  if (nll) {
    FLGP_REQUIRE(n_samples >= 1, "%s: n_samples=%d must be at least 1", who, n_samples);
    FLGP_REQUIRE((long)mnew <= (long)0x7FFFFFFF * 256 / J, "%s: bad shape (m_new=%d, J=%d)", who, mnew, J);
    FLGP_TRY(check_class_labels(who, "target", target, mnew, J, true));
  }

  Stream st;
  FLGP_TRY(st.create());
  const size_t col = (size_t)mnew, nj = sizeof(double) * col * J;
  DevBuf dlab, dY, dmean, dcov;
  FLGP_TRY(upload(dlab, Y, sizeof(double) * (size_t)m, st.s));
  FLGP_TRY(dY.alloc(sizeof(double) * (size_t)m * J));
  FLGP_TRY(dmean.alloc(nj)); FLGP_TRY(dcov.alloc(nj));
  // column j = (Y == j): the indicator matrix of multi_train_split, formed on the device
  std::vector<int> cols((size_t)J), its((size_t)J, 0);
  for (int j = 0; j < J; ++j) {
    cols[(size_t)j] = j;
    FLGP_TRY(gpc_class_indicator(st.s, dlab.as<double>(), m, j, dY.as<double>() + (size_t)j * m));
  }
  BatchFailure fail;      // the body has worded it: "<who>: class <j>: .."
  FLGP_TRY(logit_posteriors(st.s, who, true, ep, K, r0, r1, dY.as<double>(), cols.data(), ts, J, sigma11, sigma22, tol, max_iter,
                            std::max(max_parallel, 1), dmean.as<double>(), dcov.as<double>(), its.data(), fail));
  if (iters) std::copy(its.begin(), its.end(), iters);
  DevBuf dtarget, dnll, work;
  if (nll) {
    FLGP_TRY(upload(dtarget, target, sizeof(double) * col, st.s));
    FLGP_TRY(dnll.alloc(sizeof(double))); FLGP_TRY(work.alloc(flgp_dev_nll_workspace(mnew, J)));
    FLGP_TRY(flgp_dev_nll_classification(st.s, dmean.as<double>(), dcov.as<double>(), dtarget.as<double>(), mnew, J, 1, n_samples,
                                         seed, 0, nullptr, dnll.as<double>(), work.as<double>()));
    FLGP_TRY(d2h(nll, dnll.p, sizeof(double), st.s));
  }
  if (mean) {
    FLGP_TRY(d2h(mean, dmean.p, nj, st.s));
    FLGP_TRY(d2h(cov, dcov.p, nj, st.s));
  }
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}
}  // namespace

extern "C" int flgp_eigenpair_logit_posterior_multiclass(const flgp_eigenpair *ep, int K, const double *ts, int J, double sigma11,
                                                         double sigma22, const int *idx0, int m, const double *Y, const int *idx1,
                                                         int mnew, double tol, int max_iter, int max_parallel, double *mean,
                                                         double *cov, int *iters) {
  return posterior_multiclass(ep, K, ts, J, sigma11, sigma22, idx0, m, Y, idx1, mnew, tol, max_iter, max_parallel, mean, cov,
                              iters, nullptr, 0, 0, nullptr);
}

extern "C" int flgp_eigenpair_logit_posterior_multiclass_nll(const flgp_eigenpair *ep, int K, const double *ts, int J,
                                                             double sigma11, double sigma22, const int *idx0, int m,
                                                             const double *Y, const int *idx1, int mnew, double tol, int max_iter,
                                                             int max_parallel, double *mean, double *cov, int *iters,
                                                             const double *target, int n_samples, unsigned long long seed,
                                                             double *nll) {
  FLGP_REQUIRE(nll, "logit_posterior_multiclass: null pointer");
  return posterior_multiclass(ep, K, ts, J, sigma11, sigma22, idx0, m, Y, idx1, mnew, tol, max_iter, max_parallel, mean, cov,
                              iters, target, n_samples, seed, nll);
}

// ---- logit posterior for a batch of (labels, t) problems -------------------------------------------------
extern "C" int flgp_eigenpair_logit_posterior_batch(const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y,
                                                    int ncol, const int *col, const double *ts, int B, double sigma11,
                                                    double sigma22, const int *idx1, int mnew, double tol, int max_iter,
                                                    int max_parallel, double *mean, double *cov, int *iters) {
  const char *who = "logit_posterior_batch";
  FLGP_REQUIRE(idx0 && Y && ts && idx1 && mean && cov, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && m >= 1 && mnew >= 1 && max_iter >= 1 && B >= 1 && ncol >= 1,
               "%s: bad shape (K=%d, m=%d, m_new=%d, max_iter=%d, B=%d, ncol=%d)", who, K, m, mnew, max_iter, B, ncol);
  FLGP_REQUIRE(col || ncol == B, "%s: col may be NULL only if ncol == B (ncol=%d, B=%d)", who, ncol, B);
  std::vector<int> cols((size_t)B);
  for (int b = 0; b < B; ++b) {
    const int c = cols[(size_t)b] = col ? col[b] : b;
    FLGP_REQUIRE(c >= 0 && c < ncol, "problem %d (t=%g): %s: col=%d is outside [0, ncol=%d)", b, ts[b], who, c, ncol);
    FLGP_REQUIRE(std::isfinite(ts[b]), "problem %d (t=%g): %s: t must be finite", b, ts[b], who);
  }
  FLGP_TRY(posterior_check_sigmas(who, sigma11, sigma22));
  for (int c = 0; c < ncol; ++c) FLGP_TRY(check_labels(Y + (size_t)c * m, nullptr, m, who));
  Rows r0, r1;
  FLGP_TRY(posterior_check_rows(who, ep, K, idx0, m, idx1, mnew, max_iter, true, r0, r1));    // the pair is looked at last

  Stream st;
  FLGP_TRY(st.create());
  const size_t nb = sizeof(double) * (size_t)mnew * B;
  DevBuf dY, dmean, dcov;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m * ncol, st.s));
  FLGP_TRY(dmean.alloc(nb)); FLGP_TRY(dcov.alloc(nb));
  std::vector<int> its((size_t)B, 0);
  BatchFailure fail;
  const int rc = logit_posteriors(st.s, who, false, ep, K, r0, r1, dY.as<double>(), cols.data(), ts, B, sigma11, sigma22, tol,
                                  max_iter, max_parallel, dmean.as<double>(), dcov.as<double>(), its.data(), fail);
  if (rc != FLGP_OK) {
    if (fail.problem >= 0) set_error("problem %d (t=%g): %s", fail.problem, ts[fail.problem], std::string(flgp_last_error()).c_str());
    return rc;
  }
  FLGP_TRY(d2h(mean, dmean.p, nb, st.s));
  FLGP_TRY(d2h(cov, dcov.p, nb, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  if (iters) std::copy(its.begin(), its.end(), iters);
  return FLGP_OK;
}

// ---- regression posterior: the drivers' testing step (src/Fit.cpp:70-79) in one call --------------------
namespace {
// mean(i, 0:q) = U^T v_i (dmean at ld r.m) and, with dcov, cov_i = c + |G v_i|^2 for the rows r of the pair.  Gf: the fused
// kernel's operand (gpr_predict_prep on G and U), the rows read in place.  Gf == nullptr: the GEMM route of predict_rows_wide,
// Z = V G^T and its row sums of squares and a K-wide product for the mean, in row blocks of at most 256 MB.
int regression_rows(hipStream_t st, const flgp_eigenpair *ep, int K, int q, Rows &r, const double *G, const double *U,
                    const double *Gf, double c, double *dmean, double *dcov) {
  FLGP_TRY(r.resolve(st));
  const double *dvec = (const double *)ep->vectors.p;
  if (Gf) return gpr_predict_rows(st, dvec, ep->n, r.d, r.row0, r.m, K, q, Gf, c, dmean, (long)r.m, dcov);
  ProfScope ps("gpr_predict_rows_wide", st, 2.0 * r.m * K * (dcov ? K + q : q));
  const int rb = (int)std::min<size_t>((size_t)r.m, std::max<size_t>(64, (((size_t)256 << 20) / (sizeof(double) * K)) / 64 * 64));
  DevBuf Z, Vb;
  if (dcov) FLGP_TRY(Z.alloc(sizeof(double) * (size_t)rb * K));
  if (r.d) FLGP_TRY(Vb.alloc(sizeof(double) * (size_t)rb * K));
  for (int o = 0; o < r.m; o += rb) {
    const int rows = std::min(rb, r.m - o);
    const double *V = dvec + r.row0 + o;
    long ld = ep->n;
    if (r.d) {
      FLGP_TRY(flgp_dev_gather_rows(st, dvec, ep->n, r.d + o, rows, K, Vb.as<double>()));
      V = Vb.as<double>(); ld = rows;
    }
    if (dcov) {
      FLGP_TRY(gemm_launch(st, rows, K, K, 1.0, V, 1, ld, G, K, 1, 0.0, nullptr, 0, 0, Z.as<double>(), 1, rows, nullptr, 0, 0.0,
                           nullptr));                                                                 // Z = V2 G^T
      FLGP_TRY(gpc_rowsumsq_add(st, Z.as<double>(), rows, rows, K, c, dcov + o));
    }
    FLGP_TRY(gemm_launch(st, rows, q, K, 1.0, V, 1, ld, U, 1, K, 0.0, nullptr, 0, 0, dmean + o, 1, (long)r.m, nullptr, 0, 0.0,
                         nullptr));                                                                   // V2 U into rows o ..
  }
  return FLGP_OK;
}

// The trained state of the regression posterior in weight space (the formulas are above the entry below): U = L^1/2 beta
// (K x q) and, with want_cov, Li = sqrt(c) L_Q^-1 L^1/2 (K x K), from the checked training rows r0.  The entry below and the
// predictor's operands (regression_operands) run it: one body, the same launches.  G.flag holds the pivot verdict.
struct GprOperand {
  GprCtx G;
  DevBuf dY, dnoise, zinv, ZV, ZY, M, S, Qd, Qs, U, work;
  DevBuf Li, Tb, wt, lsc;
  int build(hipStream_t st, const flgp_eigenpair *ep, int K, Rows &r0, const double *Y, int q, double t, const double *noise,
            bool different, double sigma, bool want_cov) {
    const int m = r0.m;
    const double c = noise[0] + sigma;
    FLGP_TRY(G.prepare(st, ep, K, t));                          // ls = L^1/2
    FLGP_TRY(r0.gather(st, ep, K));
    const size_t we = vt_work_elems(K, q);
    FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m * q, st));
    FLGP_TRY(M.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(Qd.alloc(sizeof(double) * (size_t)K * K));
    FLGP_TRY(S.alloc(sizeof(double) * (size_t)K * q)); FLGP_TRY(U.alloc(sizeof(double) * (size_t)K * q));
    FLGP_TRY(work.alloc(sizeof(double) * we));
    const double *ls = G.ls.as<double>();
    int *flag = G.flag.as<int>();
    // the mean's system: M = V1^T Z^-1 V1, S = V1^T Z^-1 Y ("same": Z = I and c on Q's diagonal)
    const double *Vz = r0.V, *Yz = dY.as<double>();
    long ldz = r0.ld;
    if (different) {
      FLGP_TRY(upload(dnoise, noise, sizeof(double) * (size_t)m, st));
      FLGP_TRY(zinv.alloc(sizeof(double) * (size_t)m));
      FLGP_TRY(ZV.alloc(sizeof(double) * (size_t)m * K)); FLGP_TRY(ZY.alloc(sizeof(double) * (size_t)m * q));
      FLGP_TRY(gpr_zinv(st, dnoise.as<double>(), sigma, m, zinv.as<double>()));
      FLGP_TRY(gpr_rowscale_ld(st, r0.V, r0.ld, zinv.as<double>(), m, K, ZV.as<double>()));
      FLGP_TRY(gpr_rowscale_ld(st, dY.as<double>(), m, zinv.as<double>(), m, q, ZY.as<double>()));
      Vz = ZV.as<double>(); ldz = m; Yz = ZY.as<double>();
    }
    FLGP_TRY(gemm_tn(st, K, K, m, r0.V, r0.ld, Vz, ldz, M.as<double>(), work.as<double>(), we));
    FLGP_TRY(gemm_tn(st, K, q, m, r0.V, r0.ld, Yz, m, S.as<double>(), work.as<double>(), we));
    FLGP_TRY(gpr_q(st, M.as<double>(), ls, K, different ? 1.0 : c, Qd.as<double>()));
    FLGP_TRY(chol_blocked(st, Qd.as<double>(), K, K, flag));
    FLGP_TRY(gpr_scale(st, S.as<double>(), ls, nullptr, K, q, U.as<double>()));                          // L^1/2 S
    FLGP_TRY(chol_trsv(st, Qd.as<double>(), K, K, U.as<double>(), K, q, 3, flag));                        // beta
    FLGP_TRY(gpr_scale(st, U.as<double>(), ls, nullptr, K, q, U.as<double>()));                          // U = L^1/2 beta
    // the variance's operand: sqrt(c) L_Q^-1 L^1/2; "different" factors Q_s = L^1/2 V1^T V1 L^1/2 + c I beside Q_d
    if (want_cov) {
      const double *LQ = Qd.as<double>();
      if (different) {
        FLGP_TRY(Qs.alloc(sizeof(double) * (size_t)K * K));
        FLGP_TRY(gemm_tn(st, K, K, m, r0.V, r0.ld, r0.V, r0.ld, M.as<double>(), work.as<double>(), we));
        FLGP_TRY(gpr_q(st, M.as<double>(), ls, K, c, Qs.as<double>()));
        FLGP_TRY(chol_blocked(st, Qs.as<double>(), K, K, flag));
        LQ = Qs.as<double>();
      }
      const size_t wi = (size_t)32 * 64 * K;
      FLGP_TRY(Li.alloc(sizeof(double) * (size_t)K * K)); FLGP_TRY(Tb.alloc(sizeof(double) * (size_t)64 * K));
      FLGP_TRY(wt.alloc(sizeof(double) * wi)); FLGP_TRY(lsc.alloc(sizeof(double) * (size_t)K));
      FLGP_TRY(tri_inverse(st, LQ, K, K, Li.as<double>(), K, Tb.as<double>(), wt.as<double>(), wi, flag));
      FLGP_TRY(gpr_scalar_mul(st, ls, std::sqrt(c), K, lsc.as<double>()));
      FLGP_TRY(gpr_scale(st, Li.as<double>(), nullptr, lsc.as<double>(), K, K, Li.as<double>()));
    }
    return FLGP_OK;
  }
};

// m <= K: the three existing bodies, unchanged, under this entry's name; the score is the host entry on their results
int regression_posterior_dense(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1,
                               int mnew, const double *Y, int q, double t, const double *noise, bool different, double sigma,
                               double *train_pred, double *test_pred, double *cov, const double *target, double *nll) {
  const double *nv = different ? noise : nullptr;
  std::vector<double> tp, cv;
  if (nll && !test_pred) { tp.resize((size_t)mnew * q); test_pred = tp.data(); }
  if (nll && !cov) { cv.resize((size_t)mnew); cov = cv.data(); }
  if (train_pred) FLGP_TRY(predict_regression(who, ep, K, idx0, m, idx0, m, Y, q, t, noise[0], nv, sigma, train_pred));
  if (test_pred) FLGP_TRY(predict_regression(who, ep, K, idx0, m, idx1, mnew, Y, q, t, noise[0], nv, sigma, test_pred));
  if (cov) FLGP_TRY(posterior_variance(who, ep, K, idx0, m, idx1, mnew, t, noise[0], sigma, cov));
  if (nll) FLGP_TRY(flgp_negative_log_likelihood(test_pred, cov, target, mnew, 1, "regression", 1, 0, nll, nullptr));
  return FLGP_OK;
}
}  // namespace

// m > K in weight space.  With Phi = V1 L^1/2 and c = noise[0] + sigma:
//   "same":       Q = Phi^T Phi + c I,                   beta = Q^-1 L^1/2 V1^T Y        (push-through of Phi^T (Phi Phi^T + c I)^-1)
//   "different":  Q_d = I + L^1/2 V1^T Z^-1 V1 L^1/2,    beta = Q_d^-1 L^1/2 V1^T Z^-1 Y,  Z = diag(noise_a + sigma)
//   mean = V2 L^1/2 beta,   var_i = c + |sqrt(c) L_Q^-1 L^1/2 v2_i|^2   with Q = Phi^T Phi + c I = L_Q L_Q^T in both models
// (C22_i - beta_i of src/Utils.cpp:238-246 is c + c u^T Q^-1 u with u = L^1/2 v2_i: no subtraction is left, var_i >= c).
extern "C" int flgp_eigenpair_regression_posterior(const flgp_eigenpair *ep, int K, const int *idx0, int m, const int *idx1,
                                                   int mnew, const double *Y, int q, double t, const double *noise,
                                                   int n_noise, double sigma, double *train_pred, double *test_pred,
                                                   double *cov, const double *target, double *nll) {
  const char *who = "regression_posterior";
  // what needs neither the pair nor the arrays comes first
  FLGP_REQUIRE(K >= 1 && m >= 1 && mnew >= 1 && q >= 1, "%s: bad shape (K=%d, m=%d, m_new=%d, q=%d)", who, K, m, mnew, q);
  FLGP_REQUIRE(n_noise == 1 || n_noise == m, "%s: n_noise=%d must be 1 (\"same\") or m=%d (\"different\")", who, n_noise, m);
  FLGP_REQUIRE(!target == !nll, "%s: target and nll must be given together", who);
  FLGP_REQUIRE(!target || q == 1, "%s: the score takes one column (q=%d)", who, q);
  FLGP_REQUIRE(std::isfinite(t) && std::isfinite(sigma), "%s: t=%g and sigma=%g must be finite", who, t, sigma);
  FLGP_REQUIRE(ep && idx0 && idx1 && Y && noise, "%s: null pointer", who);
  FLGP_REQUIRE(train_pred || test_pred || cov || nll, "%s: null pointer (no output is wanted)", who);
  FLGP_REQUIRE(K <= ep->K, "%s: bad shape (K=%d of %d)", who, K, ep->K);
  for (int a = 0; a < n_noise; ++a)
    FLGP_REQUIRE(noise[a] + sigma > 0.0, "%s: noise[%d] + sigma must be positive", who, a);
  Rows r0, r1;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  FLGP_TRY(r1.check(ep, idx1, mnew, who, "idx1"));
  const bool different = n_noise != 1;
  if (m <= K)
    return regression_posterior_dense(who, ep, K, idx0, m, idx1, mnew, Y, q, t, noise, different, sigma, train_pred, test_pred,
                                      cov, target, nll);

  const bool want_cov = cov || nll, want_test = test_pred || want_cov;
  const double c = noise[0] + sigma;
  Stream st;
  FLGP_TRY(st.create());
  GprOperand O;
  FLGP_TRY(O.build(st.s, ep, K, r0, Y, q, t, noise, different, sigma, want_cov));
  const double *Gm = want_cov ? O.Li.as<double>() : nullptr;
  DevBuf Gf;
  if (gpr_predict_rows_applicable(K, q)) {
    FLGP_TRY(Gf.alloc(sizeof(double) * gpr_predict_operand_elems(K, q)));
    FLGP_TRY(gpr_predict_prep(st.s, K, q, Gm, O.U.as<double>(), Gf.as<double>()));
  }
  const double *gf = Gf.p ? Gf.as<double>() : nullptr;
  DevBuf dtrain, dmean, dcov, dtarget, dnll, nwork;
  if (train_pred) {           // the training rows through the same kernel: the mean rows only
    FLGP_TRY(dtrain.alloc(sizeof(double) * (size_t)m * q));
    FLGP_TRY(regression_rows(st.s, ep, K, q, r0, Gm, O.U.as<double>(), gf, c, dtrain.as<double>(), nullptr));
    FLGP_TRY(d2h(train_pred, dtrain.p, sizeof(double) * (size_t)m * q, st.s));
  }
  if (want_test) {
    FLGP_TRY(dmean.alloc(sizeof(double) * (size_t)mnew * q));
    if (want_cov) FLGP_TRY(dcov.alloc(sizeof(double) * (size_t)mnew));
    FLGP_TRY(regression_rows(st.s, ep, K, q, r1, Gm, O.U.as<double>(), gf, c, dmean.as<double>(), want_cov ? dcov.as<double>() : nullptr));
  }
  if (nll) {                  // scored where it lies, before anything is copied
    FLGP_TRY(upload(dtarget, target, sizeof(double) * (size_t)mnew, st.s));
    FLGP_TRY(dnll.alloc(sizeof(double))); FLGP_TRY(nwork.alloc(flgp_dev_nll_workspace(mnew, 1)));
    FLGP_TRY(flgp_dev_nll_regression(st.s, dmean.as<double>(), dcov.as<double>(), dtarget.as<double>(), mnew, nullptr,
                                     dnll.as<double>(), nwork.as<double>()));
    FLGP_TRY(d2h(nll, dnll.p, sizeof(double), st.s));
  }
  if (test_pred) FLGP_TRY(d2h(test_pred, dmean.p, sizeof(double) * (size_t)mnew * q, st.s));
  if (cov) FLGP_TRY(d2h(cov, dcov.p, sizeof(double) * (size_t)mnew, st.s));
  return O.G.verdict(st.s, who);
}

// ---- the trained operands for the predictor (common.h, predictor.hip) -----------------------------------
// The checks of flgp_eigenpair_regression_posterior that concern the trained state, in its order
int flgp::regression_operands_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int q,
                                    double t, const double *noise, int n_noise, double sigma) {
  FLGP_REQUIRE(K >= 1 && m >= 1 && q >= 1, "%s: bad shape (K=%d, m=%d, q=%d)", who, K, m, q);
  FLGP_REQUIRE(n_noise == 1 || n_noise == m, "%s: n_noise=%d must be 1 (\"same\") or m=%d (\"different\")", who, n_noise, m);
  FLGP_REQUIRE(std::isfinite(t) && std::isfinite(sigma), "%s: t=%g and sigma=%g must be finite", who, t, sigma);
  FLGP_REQUIRE(ep && idx0 && Y && noise, "%s: null pointer", who);
  FLGP_REQUIRE(K <= ep->K, "%s: bad shape (K=%d of %d)", who, K, ep->K);
  for (int a = 0; a < n_noise; ++a)
    FLGP_REQUIRE(noise[a] + sigma > 0.0, "%s: noise[%d] + sigma must be positive", who, a);
  Rows r0;
  return r0.check(ep, idx0, m, who, "idx0");
}

// GprOperand whatever m is: the K x K system exists on both sides of m = K
int flgp::regression_operands(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m,
                              const double *Y, int q, double t, const double *noise, int n_noise, double sigma,
                              const OperandSink &sink) {
  Rows r0;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  GprOperand O;
  FLGP_TRY(O.build(st, ep, K, r0, Y, q, t, noise, n_noise != 1, sigma, true));
  FLGP_TRY(sink(0, 1, O.Li.as<double>(), 0, O.U.as<double>(), 0));
  return O.G.verdict(st, who);
}

int flgp::logit_operands_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol,
                               const int *col, const double *ts, int B, double sigma11, double sigma22, int max_iter) {
  FLGP_REQUIRE(idx0 && Y && ts, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && m >= 1 && max_iter >= 1 && B >= 1 && ncol >= 1, "%s: bad shape (K=%d, m=%d, max_iter=%d, B=%d, ncol=%d)", who,
               K, m, max_iter, B, ncol);
  FLGP_REQUIRE(col || ncol == B, "%s: col may be NULL only if ncol == B (ncol=%d, B=%d)", who, ncol, B);
  for (int b = 0; b < B; ++b) {
    const int c = col ? col[b] : b;
    FLGP_REQUIRE(c >= 0 && c < ncol, "problem %d (t=%g): %s: col=%d is outside [0, ncol=%d)", b, ts[b], who, c, ncol);
    FLGP_REQUIRE(std::isfinite(ts[b]), "problem %d (t=%g): %s: t must be finite", b, ts[b], who);
  }
  FLGP_TRY(posterior_check_sigmas(who, sigma11, sigma22));
  for (int c = 0; c < ncol; ++c) FLGP_TRY(check_labels(Y + (size_t)c * m, nullptr, m, who));
  FLGP_REQUIRE(ep, "%s: null pointer", who);                                                 // the pair is looked at last
  FLGP_REQUIRE(K <= ep->K, "%s: bad shape (K=%d of %d)", who, K, ep->K);
  Rows r0;
  return r0.check(ep, idx0, m, who, "idx0");
}

// ws_chunks whatever m is, the sink in the place of the predictive rows; a failure is worded as the batch entry's
int flgp::logit_operands(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y,
                         int ncol, const int *col, const double *ts, int B, double sigma11, double tol, int max_iter,
                         int max_parallel, int *its, const OperandSink &sink) {
  Rows r0;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  std::vector<int> cols((size_t)B);
  for (int b = 0; b < B; ++b) cols[(size_t)b] = col ? col[b] : b;
  DevBuf dY;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m * ncol, st));
  BatchFailure fail;
  const int rc = ws_chunks(st, who, false, ep, K, r0, nullptr, dY.as<double>(), cols.data(), ts, B, sigma11, tol, max_iter,
                           max_parallel, false, its, fail, [&](int p0, int S, WsBatch &W) {
                             const LrChunk &C = W.L.C;
                             return sink(p0, S, W.Li.as<double>(), C.sq, C.u, C.sk);
                           });
  if (rc != FLGP_OK) {
    if (fail.problem >= 0) set_error("problem %d (t=%g): %s", fail.problem, ts[fail.problem], std::string(flgp_last_error()).c_str());
    return rc;
  }
  FLGP_HIP(hipStreamSynchronize(st));
  return FLGP_OK;
}

// ---- Polya-Gamma Gibbs prediction: test_pgbinary_cpp and predict_logit_mult_gp_cpp (pg.hip) ---------------
namespace {
// One chain of PGLogitModel (src/PGLogitModel.cpp) on an m x m B, with a dense C (DENSE: flgp_pg_logit_predict's host
// matrices) or C = V1 L V1^T + sigma I of the resident pair for m <= K (DIRECT: a pool worker of pg_chains; m > K runs in
// PgBatch).  Each sweep resamples f in Matheron's form, with the law of _resample_f (:25-39) and one solve against
// B = sW C sW + I, factored m x m:
//   f0 = V1 L^1/2 z1 + sqrt(sigma) z2 (dense: L_C z2), r = kappa / sW - sW f0 - z3, f = f0 + C (sW B^-1 r),
// then omega ~ PG(1, f).  C x = V1 (L (V1^T x)) + sigma x in DIRECT, where C is formed only to build B, and a dense product in
// DENSE: the routes differ in f0 and C x alone, so they stay branches, not two solver objects.
enum PgRoute { PG_DENSE, PG_DIRECT };
struct PgChain {
  PgRoute route = PG_DENSE;
  int m = 0, K = 0;
  const double *C = nullptr, *LC = nullptr;                  // C (m x m); DENSE: its factor
  // DIRECT, set by the caller: V1 (m x K at ld1), l = exp(-t (1 - values)), ls = l^1/2 and C's sigma
  const double *V1 = nullptr, *l = nullptr, *ls = nullptr;
  long ld1 = 0;
  double sigma = 0.0;
  int *flag = nullptr;
  DevBuf kappa, omega, f, f0, r, sw, z, x, t1, t2, B, u, work;   // u (K) and work (we) are lvt's
  size_t we = 0;

  int alloc(int m_, int K_) {
    m = m_; K = K_;
    const size_t v = sizeof(double) * (size_t)m;
    FLGP_TRY(kappa.alloc(v)); FLGP_TRY(omega.alloc(v)); FLGP_TRY(f.alloc(v)); FLGP_TRY(f0.alloc(v)); FLGP_TRY(r.alloc(v));
    FLGP_TRY(sw.alloc(v)); FLGP_TRY(x.alloc(v)); FLGP_TRY(t1.alloc(v)); FLGP_TRY(t2.alloc(v));
    FLGP_TRY(z.alloc(sizeof(double) * ((size_t)2 * m + K)));
    we = vt_work_elems(K, 1);
    FLGP_TRY(u.alloc(sizeof(double) * (size_t)std::max(K, 1))); FLGP_TRY(work.alloc(sizeof(double) * we));
    return B.alloc(sizeof(double) * (size_t)m * m);
  }
  // sW from omega, B factored in place
  int factor(hipStream_t st) {
    FLGP_TRY(pg_dvec(st, m, omega.as<double>(), 0.0, sw.as<double>(), t1.as<double>(), t2.as<double>()));
    FLGP_TRY(gpc_bmat(st, C, sw.as<double>(), m, B.as<double>()));
    return chol_blocked(st, B.as<double>(), m, m, flag);
  }
  // out = sW .* B^-1 rin with the factor of the last factor()
  int solve(hipStream_t st, const double *rin, double *out) {
    FLGP_HIP(hipMemcpyAsync(t1.p, rin, sizeof(double) * (size_t)m, hipMemcpyDeviceToDevice, st));
    FLGP_TRY(chol_trsv(st, B.as<double>(), m, m, t1.as<double>(), m, 1, 3, flag));
    return pg_mul(st, m, sw.as<double>(), t1.as<double>(), nullptr, out);
  }
  // u = L (V1^T x): the latent mean of a row with eigenvector entries v is then v . u
  int lvt(hipStream_t st, const double *xin) {
    FLGP_TRY(gemm_tn(st, K, 1, m, V1, ld1, xin, m, u.as<double>(), work.as<double>(), we));
    return pg_mul(st, K, l, u.as<double>(), nullptr, u.as<double>());
  }
  // out = add + C xin (add may be nullptr)
  int cmul(hipStream_t st, const double *xin, const double *add, double *out) {
    if (route == PG_DENSE) {
      FLGP_TRY(gpc_gemv(st, C, m, xin, nullptr, t2.as<double>()));
      return pg_axpy3(st, m, add, t2.as<double>(), 0.0, nullptr, out);
    }
    FLGP_TRY(lvt(st, xin));
    FLGP_TRY(gemm_nn(st, m, 1, K, V1, ld1, u.as<double>(), K, t2.as<double>(), nullptr, 0));
    return pg_axpy3(st, m, add, t2.as<double>(), sigma, xin, out);
  }
  int run(hipStream_t st, const double *dY, int n_sample, unsigned long long seed) {
    FLGP_TRY(pg_init(st, m, dY, kappa.as<double>(), omega.as<double>(), f.as<double>()));
    double *z1 = z.as<double>(), *z2 = z1 + K, *z3 = z2 + m;      // DENSE: K = 0
    for (int s = 0; s < n_sample; ++s) {
      ProfScope ps("pg_sweep", st, 0.0);
      FLGP_TRY(pg_normals(st, seed, s, K, m, z1));
      if (route == PG_DENSE) {
        FLGP_TRY(pg_trmv(st, LC, m, m, z2, t2.as<double>(), flag));                                         // L_C z2
      } else {
        FLGP_TRY(pg_mul(st, K, ls, z1, nullptr, u.as<double>()));
        FLGP_TRY(gemm_nn(st, m, 1, K, V1, ld1, u.as<double>(), K, t2.as<double>(), nullptr, 0));            // V1 L^1/2 z1
      }
      FLGP_TRY(pg_f0r(st, m, t2.as<double>(), z2, route == PG_DENSE ? 0.0 : std::sqrt(sigma), z3, kappa.as<double>(),
                      omega.as<double>(), f0.as<double>(), r.as<double>(), sw.as<double>()));
      FLGP_TRY(factor(st));
      FLGP_TRY(solve(st, r.as<double>(), x.as<double>()));
      FLGP_TRY(cmul(st, x.as<double>(), f0.as<double>(), f.as<double>()));
      FLGP_TRY(pg_draw_launch(st, nullptr, f.as<double>(), m, pg_stream_base(seed, 4ull * (unsigned long long)s + 3),
                              omega.as<double>()));
    }
    return FLGP_OK;
  }
  // _collapsed_predict (src/PGLogitModel.cpp:61-73) at the final omega, first half: w = kappa - sW B^-1 (sW C kappa) in x
  int collapsed_w(hipStream_t st) {
    FLGP_TRY(factor(st));
    FLGP_TRY(cmul(st, kappa.as<double>(), nullptr, r.as<double>()));                       // C kappa
    FLGP_TRY(pg_mul(st, m, sw.as<double>(), r.as<double>(), nullptr, r.as<double>()));
    FLGP_TRY(solve(st, r.as<double>(), f0.as<double>()));
    return pg_axpy3(st, m, kappa.as<double>(), nullptr, -1.0, f0.as<double>(), x.as<double>());
  }
};

// For every new row i the training positions j with idx0_j = idx1_i, as CSR (ptr: m_new + 1, list): where the binary
// drivers' C = [Cvv; Cnv] carries sigma on the diagonal of its top block (src/Fit.cpp:574-576).
struct PgMatch {
  DevBuf ptr, list;
  int build(hipStream_t st, const int *idx0, int m, const int *idx1, int mnew) {
    std::vector<std::pair<int, int>> pos((size_t)m);
    for (int j = 0; j < m; ++j) pos[(size_t)j] = {idx0[j], j};
    std::sort(pos.begin(), pos.end());
    std::vector<long> hp((size_t)mnew + 1, 0);
    std::vector<int> hl;
    for (int i = 0; i < mnew; ++i) {
      auto lo = std::lower_bound(pos.begin(), pos.end(), std::make_pair(idx1[i], -1));
      for (; lo != pos.end() && lo->first == idx1[i]; ++lo) hl.push_back(lo->second);
      hp[(size_t)i + 1] = (long)hl.size();
    }
    FLGP_TRY(upload(ptr, hp.data(), sizeof(long) * hp.size(), st));
    FLGP_TRY(upload(list, hl.data(), sizeof(int) * hl.size(), st));          // an empty list still gets a buffer
    FLGP_HIP(hipStreamSynchronize(st));      // the host vectors go out of scope
    return FLGP_OK;
  }
};

int pg_pivot_error(int bad, const char *who) {
  set_error("%s: a Cholesky factorisation met a pivot <= 0 (pivot %d): the covariance is not positive definite or the "
            "chain diverged", who, bad - 1);
  return FLGP_ERR_NOCONV;
}
int pg_verdict(hipStream_t st, const void *d_flag, const char *who) {   // synchronises
  int bad = 0;
  FLGP_TRY(read_flag(st, d_flag, &bad));
  return bad ? pg_pivot_error(bad, who) : FLGP_OK;
}

int check_pg_common(const double *Y, int m, int mnew, int n_sample, const char *who) {
  FLGP_REQUIRE(m >= 1 && mnew >= 1, "%s: bad shape (m=%d, m_new=%d)", who, m, mnew);
  FLGP_REQUIRE(n_sample >= 1, "%s: N_sample=%d must be at least 1", who, n_sample);
  for (int a = 0; a < m; ++a) FLGP_REQUIRE(Y[a] >= 0.0 && Y[a] <= 1.0, "%s: Y[%d]=%g is outside [0, 1]", who, a, Y[a]);
  return FLGP_OK;
}

// PgChain's sweep for m > K, for a chunk of chains in the same launches: B is never formed.  With LrBatch's
// identities (D = 1 + sigma omega, a = D^-1/2 sW its xs, dh = D^-1/2, X = diag(a) V1 L^1/2, Q = I + X^T X factored K x K):
//   sW B^-1 r = sW D^-1/2 (g - X Q^-1 X^T g),  g = D^-1/2 r,
// and C x = V1 (L (V1^T x)) + sigma x.  Slot s of every buffer belongs to chain p0 + s for the whole chunk; each step of
// run / factor / solve / cmul is one launch over the slots: the pgb_* kernels (pg.hip) for the chain's own elementwise
// steps, LrBatch's kernels (lrb_*, on the LrChunk view C) for X, Q and its factor, and the batched GEMM with V1 / V2 at
// stride 0.  Every chain runs all n_sample sweeps, so the slot list is the identity.  The split products take, per chain,
// the plan of an unbatched product with a workspace of vt_work_elems(K, 1) doubles, on planes of the slot's own:
// LrBatch::plans.
struct PgBatch {
  PgChunk P;
  LrChunk C;
  DevBuf vec, zb, kv, X, Q, part, flag, act;
  int planQ = 1, planU = 1;
  size_t pe = 0;
  long sp = 0;                   // doubles between two slots' planes

  // device bytes of one chain: X, Q, eleven m-vectors, z, u, l, ls, its planes, the mnew doubles of the caller's own for it (the
  // batch entry's mean over the new rows), flag and list entry
  static double bytes(int m, int K, int mnew) {
    int a, b;
    size_t pe;
    LrBatch::plans(m, K, &a, &b, &pe);
    return 8.0 * ((double)pad32((long)m * K) + pad32((long)K * K) + 11.0 * pad32(m) + pad32(2L * m + K) + 3.0 * pad32(K) +
                  pad32((long)pe) + pad32(mnew)) + 8.0;
  }
  int alloc(hipStream_t st, int m, int K, int slots) {
    C = LrChunk{};
    C.m = m; C.K = K; C.slots = slots;
    C.sv = pad32(m); C.sk = pad32(K); C.sx = pad32((long)m * K); C.sq = pad32((long)K * K);
    P = PgChunk{};
    P.m = m; P.K = K; P.slots = slots; P.sv = C.sv; P.sz = pad32(2L * m + K); P.ldy = m;
    LrBatch::plans(m, K, &planQ, &planU, &pe);
    sp = pad32((long)pe);
    const size_t S = (size_t)slots;
    FLGP_TRY(vec.alloc(sizeof(double) * 11 * S * P.sv)); FLGP_TRY(zb.alloc(sizeof(double) * S * P.sz));
    FLGP_TRY(kv.alloc(sizeof(double) * 3 * S * C.sk));
    FLGP_TRY(X.alloc(sizeof(double) * S * C.sx)); FLGP_TRY(Q.alloc(sizeof(double) * S * C.sq));
    FLGP_TRY(part.alloc(sizeof(double) * S * sp));
    FLGP_TRY(flag.alloc(sizeof(int) * S)); FLGP_TRY(act.alloc(sizeof(int) * S));
    double *v = vec.as<double>(), *k = kv.as<double>();
    const size_t vs = S * P.sv, ks = S * C.sk;
    P.kappa = v; P.omega = v + vs; P.f = v + 2 * vs; P.f0 = v + 3 * vs; P.r = v + 4 * vs; P.sw = v + 5 * vs; P.x = v + 6 * vs;
    P.t1 = v + 7 * vs; P.t2 = v + 8 * vs; P.dh = v + 9 * vs; P.a = v + 10 * vs;
    P.z = zb.as<double>();
    C.xs = P.a;
    C.u = k; C.l = k + ks; C.ls = k + 2 * ks;
    C.X = X.as<double>(); C.Q = Q.as<double>(); C.flag = flag.as<int>();
    std::vector<int> ident(S);
    for (int s = 0; s < slots; ++s) ident[(size_t)s] = s;
    FLGP_TRY(h2d(act.p, ident.data(), sizeof(int) * S, st));
    FLGP_HIP(hipStreamSynchronize(st));      // ident goes out of scope
    return FLGP_OK;
  }
  // LrBatch's two K x 1 / m x 1 products per slot, on this chunk's strides
  int tn(hipStream_t st, const double *Am, long lda, long a_bs, const double *x, double *out) {
    const GemmBatch gb{P.slots, act.as<int>(), a_bs, P.sv, C.sk, 0, sp};
    return gemm_launch(st, C.K, 1, C.m, 1.0, Am, lda, 1, x, 1, C.m, 0.0, nullptr, 0, 0, out, 1, C.K, part.as<double>(), pe, 0.0,
                       nullptr, nullptr, nullptr, planU, nullptr, &gb);
  }
  int nn(hipStream_t st, int rows, const double *Am, long lda, long a_bs, const double *u, double *out, long o_bs) {
    const GemmBatch gb{P.slots, act.as<int>(), a_bs, C.sk, o_bs, 0, 0};
    return gemm_launch(st, rows, 1, C.K, 1.0, Am, 1, lda, u, 1, C.K, 0.0, nullptr, 0, 0, out, 1, rows, nullptr, 0, 0.0, nullptr,
                       nullptr, nullptr, 0, nullptr, &gb);
  }
  // u = L (V1^T x) per slot: PgChain::lvt
  int lvt(hipStream_t st, const double *x) {
    FLGP_TRY(tn(st, C.V1, C.ld1, 0, x, C.u));
    return lrb_mul(st, C.K, C.l, C.sk, C.u, C.sk, C.u, C.sk, act.as<int>(), P.slots);
  }
  int factor(hipStream_t st) {
    const int *a = act.as<int>();
    const int S = P.slots;
    FLGP_TRY(pgb_dvec(st, P));
    FLGP_TRY(lrb_scale2(st, C, a, S));
    const GemmBatch gb{S, a, C.sx, C.sx, C.sq, 0, sp};
    FLGP_TRY(gemm_launch(st, C.K, C.K, C.m, 1.0, C.X, C.m, 1, C.X, 1, C.m, 0.0, nullptr, 0, 0, C.Q, 1, C.K, part.as<double>(), pe,
                         0.0, nullptr, nullptr, nullptr, planQ, nullptr, &gb));
    FLGP_TRY(lrb_add_diag(st, C, a, S));
    return lrb_chol(st, C, a, S);
  }
  int solve(hipStream_t st, const double *rin, double *out) {
    const int *a = act.as<int>();
    FLGP_TRY(lrb_mul(st, C.m, P.dh, P.sv, rin, P.sv, P.t1, P.sv, a, P.slots));                  // g
    FLGP_TRY(tn(st, C.X, C.m, C.sx, P.t1, C.u));
    FLGP_TRY(lrb_trsv(st, C, a, P.slots));
    FLGP_TRY(nn(st, C.m, C.X, C.m, C.sx, C.u, P.t2, P.sv));
    return pgb_wb_out(st, P, out);
  }
  int cmul(hipStream_t st, const double *xin, const double *add, double *out) {
    FLGP_TRY(lvt(st, xin));
    FLGP_TRY(nn(st, C.m, C.V1, C.ld1, 0, C.u, P.t2, P.sv));
    return pgb_axpy3(st, P, add, P.t2, P.sigma, xin, out);
  }
  // the chains of the chunk [p0, p0 + S): weights, the n_sample sweeps, the collapsed w (in x) and u = L V1^T w (in C.u): the
  // latent mean of a row with eigenvector entries v is v . u
  int run(hipStream_t st, const flgp_eigenpair *ep, const double *d_ts, int S, int n_sample) {
    P.slots = C.slots = S;
    const int *a = act.as<int>();
    FLGP_TRY(lrb_weights(st, (const double *)ep->values.p, nullptr, C.K, d_ts, S, C.sk, C.ls, C.l));
    FLGP_HIP(hipMemsetAsync(C.flag, 0, sizeof(int) * (size_t)S, st));
    FLGP_TRY(pgb_init(st, P));
    const double ss = std::sqrt(P.sigma);
    for (int s = 0; s < n_sample; ++s) {
      ProfScope ps("pg_batch_sweep", st, 0.0);
      FLGP_TRY(pgb_normals(st, P, s));
      FLGP_TRY(lrb_mul(st, C.K, C.ls, C.sk, P.z, P.sz, C.u, C.sk, a, S));
      FLGP_TRY(nn(st, C.m, C.V1, C.ld1, 0, C.u, P.t2, P.sv));                                  // V1 L^1/2 z1
      FLGP_TRY(pgb_f0r(st, P, ss));
      FLGP_TRY(factor(st));
      FLGP_TRY(solve(st, P.r, P.x));
      FLGP_TRY(cmul(st, P.x, P.f0, P.f));
      FLGP_TRY(pgb_draw(st, P, s));
    }
    FLGP_TRY(factor(st));                                                                      // PgChain::collapsed_w
    FLGP_TRY(cmul(st, P.kappa, nullptr, P.r));
    FLGP_TRY(lrb_mul(st, C.m, P.sw, P.sv, P.r, P.sv, P.r, P.sv, a, S));
    FLGP_TRY(solve(st, P.r, P.f0));
    FLGP_TRY(pgb_axpy3(st, P, P.kappa, nullptr, -1.0, P.f0, P.x));
    return lvt(st, P.x);
  }
};

// what a worker of the m x m route (m <= K) owns and reuses across its chains: C, the contraction's workspace, the
// spectrum weights and the chain's state
struct PgDirectWorker {
  DevBuf C, work, ls, l;
  PgChain P;
  int alloc(int m, int K, const Rows &r0, double sigma) {
    FLGP_TRY(C.alloc(sizeof(double) * (size_t)m * m));
    FLGP_TRY(work.alloc(flgp_dev_hk_workspace(m, m, K, 1)));
    FLGP_TRY(ls.alloc(sizeof(double) * (size_t)K)); FLGP_TRY(l.alloc(sizeof(double) * (size_t)K));
    P.route = PG_DIRECT; P.C = C.as<double>();
    P.sigma = sigma; P.V1 = r0.V; P.ld1 = r0.ld; P.l = l.as<double>(); P.ls = ls.as<double>();
    return P.alloc(m, K);
  }
  static double bytes(int m, int K, int mnew) {
    return 8.0 * (2.0 * m * m + 11.0 * m + 3.0 * K + mnew + (double)vt_work_elems(K, 1)) + (double)flgp_dev_hk_workspace(m, m, K, 1);
  }
};
}  // namespace

extern "C" int flgp_pg_draw(const double *b, const double *c, int n, unsigned long long seed, double *omega) {
  const char *who = "pg_draw";
  FLGP_REQUIRE(c && omega, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1, "%s: bad shape (n=%d)", who, n);
  for (int i = 0; i < n; ++i) {
    FLGP_REQUIRE(std::isfinite(c[i]), "%s: c[%d]=%g must be finite", who, i, c[i]);
    if (b) FLGP_REQUIRE(b[i] >= 1.0 && b[i] <= 1e6 && b[i] == std::floor(b[i]), "%s: b[%d]=%g must be an integer >= 1", who, i, b[i]);
  }
  Stream st;
  FLGP_TRY(st.create());
  DevBuf db, dc, out;
  FLGP_TRY(out.alloc(sizeof(double) * (size_t)n));
  if (b) FLGP_TRY(upload(db, b, sizeof(double) * (size_t)n, st.s));
  FLGP_TRY(upload(dc, c, sizeof(double) * (size_t)n, st.s));
  FLGP_TRY(pg_draw_launch(st.s, b ? db.as<double>() : nullptr, dc.as<double>(), n, pg_stream_base(seed, 3), out.as<double>()));
  FLGP_TRY(d2h(omega, out.p, sizeof(double) * (size_t)n, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

extern "C" int flgp_pg_logit_predict(const double *C, int m, const double *Y, const double *Cnv, int mnew, int n_sample,
                                     unsigned long long seed, double *pi_pred, double *y_pred, double *omega_out, double *f_out) {
  const char *who = "pg_logit_predict";
  FLGP_REQUIRE(C && Y && Cnv && pi_pred && y_pred, "%s: null pointer", who);
  FLGP_TRY(check_pg_common(Y, m, mnew, n_sample, who));
  Stream st;
  FLGP_TRY(st.create());
  DevBuf dC, dLC, dY, dCnv, flag, mean, dpi, dy;
  const size_t mm = sizeof(double) * (size_t)m * m;
  FLGP_TRY(dC.alloc(mm)); FLGP_TRY(dLC.alloc(mm)); FLGP_TRY(dY.alloc(sizeof(double) * (size_t)m));
  FLGP_TRY(dCnv.alloc(sizeof(double) * (size_t)mnew * m)); FLGP_TRY(flag.alloc(sizeof(int)));
  FLGP_TRY(mean.alloc(sizeof(double) * (size_t)mnew)); FLGP_TRY(dpi.alloc(sizeof(double) * (size_t)mnew));
  FLGP_TRY(dy.alloc(sizeof(double) * (size_t)mnew));
  FLGP_HIP(hipMemsetAsync(flag.p, 0, sizeof(int), st.s));
  FLGP_TRY(h2d(dC.p, C, mm, st.s));
  FLGP_TRY(h2d(dY.p, Y, sizeof(double) * (size_t)m, st.s));
  FLGP_TRY(h2d(dCnv.p, Cnv, sizeof(double) * (size_t)mnew * m, st.s));
  FLGP_HIP(hipMemcpyAsync(dLC.p, dC.p, mm, hipMemcpyDeviceToDevice, st.s));
  FLGP_TRY(chol_blocked(st.s, dLC.as<double>(), m, m, flag.as<int>()));          // C = L_C L_C^T, once per call
  PgChain P;
  P.route = PG_DENSE; P.C = dC.as<double>(); P.LC = dLC.as<double>(); P.flag = flag.as<int>();
  FLGP_TRY(P.alloc(m, 0));
  FLGP_TRY(P.run(st.s, dY.as<double>(), n_sample, seed));
  FLGP_TRY(P.collapsed_w(st.s));
  FLGP_TRY(gemm_nn(st.s, mnew, 1, m, dCnv.as<double>(), mnew, P.x.as<double>(), m, mean.as<double>(), nullptr, 0));   // Cnv w
  FLGP_TRY(pg_pi(st.s, mnew, mean.as<double>(), 0.0, nullptr, nullptr, nullptr, dpi.as<double>(), 1, dy.as<double>()));
  FLGP_TRY(d2h(pi_pred, dpi.p, sizeof(double) * (size_t)mnew, st.s));
  FLGP_TRY(d2h(y_pred, dy.p, sizeof(double) * (size_t)mnew, st.s));
  if (omega_out) FLGP_TRY(d2h(omega_out, P.omega.p, sizeof(double) * (size_t)m, st.s));
  if (f_out) FLGP_TRY(d2h(f_out, P.f.p, sizeof(double) * (size_t)m, st.s));
  return pg_verdict(st.s, flag.p, who);
}

// ---- B chains in one call: the three resident-pair entries, and the chains' trained state for the predictor
// (f-22).  The chains up to u = L (V1^T w) at the final omega: m > K in chunks of chains sharing every launch (PgBatch),
// m <= K dealt to pool workers, each with a PgChain of its own on the m x m route.  What follows u is the caller's: the
// entries multiply the new rows' V2 onto it (pg_predict_chains), the predictor folds it into its anchor side.
namespace {
// what a sink sees of the chains [p0, p0 + S) while it is valid: u of chain p0 + a at U + a su and its collapsed w at w + a sw.
// `act` is the slot list of the batched launches (m > K); it is nullptr on the pool route, where S = 1 and `st` is the
// worker's stream
struct PgChunkOut {
  hipStream_t st;
  int p0, S;
  const double *U; long su;
  const double *w; long sw;
  const int *act;
};
using PgChunkSink = std::function<int(const PgChunkOut &)>;

// words the last error as chain b's
void pg_name_chain(int b, const double *ts, const unsigned long long *seeds) {
  const std::string msg(flgp_last_error());
  set_error("chain %d (t=%g, seed=%llu): %s", b, ts[b], seeds[b], msg.c_str());
}

// r0 gathered, dY on the device, cols resolved.  sink_doubles: the doubles per chain of the caller's own buffers, for the
// planning of the chunk / the workers alone.  flags: one pivot flag per chain, valid once `st` is synchronised (the caller's
// verdict: pg_flags_verdict).  name_chains: a failure comes back worded "chain b (t=.., seed=..): .." (a caller whose
// chains are the user's: the batch entry, the predictor); without, as the chain itself words it (the batch of one, of J classes).
int pg_chains(hipStream_t st, const flgp_eigenpair *ep, int K, const Rows &r0, const double *dY, const int *cols, const double *ts,
              const unsigned long long *seeds, int B, double sigma, int n_sample, int max_parallel, int sink_doubles,
              bool name_chains, double *omega_out, double *f_out, int *flags, DevBuf &dflag, const PgChunkSink &sink) {
  const int m = r0.m;
  const size_t vb = sizeof(double) * (size_t)m;
  if (m <= K) {
    FLGP_TRY(dflag.alloc(sizeof(int) * (size_t)B));
    FLGP_HIP(hipMemsetAsync(dflag.p, 0, sizeof(int) * (size_t)B, st));
    FLGP_HIP(hipStreamSynchronize(st));        // the workers' streams start from the gathered rows and the cleared flags
    DevicePool pool;
    FLGP_TRY(pool.plan(max_parallel > 0 ? max_parallel : std::min(B, 4), B, PgDirectWorker::bytes(m, K, sink_doubles)));
    const PoolFailure bad = pool.run<PgDirectWorker>(
        st, B, [&](PgDirectWorker &W) { return W.alloc(m, K, r0, sigma); },
        [&](hipStream_t ws, PgDirectWorker &W, int b) -> int {
          PgChain &P = W.P;
          P.flag = dflag.as<int>() + b;
          FLGP_TRY(gpr_weights(ws, (const double *)ep->values.p, K, ts[b], W.ls.as<double>(), W.l.as<double>()));
          FLGP_TRY(hk(ws, ep, K, ts[b], r0, r0, W.C.as<double>(), W.work.as<double>()));
          if (sigma != 0.0) FLGP_TRY(gpr_add_diag(ws, W.C.as<double>(), m, sigma));
          FLGP_TRY(P.run(ws, dY + (size_t)cols[b] * m, n_sample, seeds[b]));
          FLGP_TRY(P.collapsed_w(ws));
          FLGP_TRY(P.lvt(ws, P.x.as<double>()));
          FLGP_TRY(sink(PgChunkOut{ws, b, 1, P.u.as<double>(), K, P.x.as<double>(), m, nullptr}));
          if (omega_out) FLGP_TRY(d2h(omega_out + (size_t)b * m, P.omega.p, vb, ws));
          if (f_out) FLGP_TRY(d2h(f_out + (size_t)b * m, P.f.p, vb, ws));
          FLGP_HIP(hipStreamSynchronize(ws));    // the worker's buffers take the next chain
          return FLGP_OK;
        });
    if (bad.item >= 0) {
      set_error("%s", bad.message.c_str());
      if (name_chains) pg_name_chain(bad.item, ts, seeds);
      return bad.status;
    }
    return d2h(flags, dflag.p, sizeof(int) * (size_t)B, st);
  }
  DevBuf dcol, dts, dseed;
  FLGP_TRY(upload(dcol, cols, sizeof(int) * (size_t)B, st));
  FLGP_TRY(upload(dts, ts, sizeof(double) * (size_t)B, st));
  FLGP_TRY(upload(dseed, seeds, sizeof(unsigned long long) * (size_t)B, st));
  // the chunk: max_parallel chains, or (<= 0) all of them; where that is more than one, no more than fit into 90 % of the
  // free memory
  const int want = max_parallel > 0 ? max_parallel : B;
  size_t free_b = 0, total_b = 0;
  if (plan_workers(want, B, 0.0, 0.0) > 1) FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
  const int chunk = std::min(plan_workers(want, B, (double)free_b, PgBatch::bytes(m, K, sink_doubles)), GEMM_BATCH_MAX);
  PgBatch L;
  FLGP_TRY(L.alloc(st, m, K, chunk));
  L.P.Y = dY; L.P.sigma = sigma;
  L.C.V1 = r0.V; L.C.ld1 = r0.ld; L.C.sigma = sigma;
  for (int p0 = 0; p0 < B; p0 += chunk) {
    const int S = std::min(chunk, B - p0);
    L.P.ycol = dcol.as<int>() + p0; L.P.seed = dseed.as<unsigned long long>() + p0;
    FLGP_TRY(L.run(st, ep, dts.as<double>() + p0, S, n_sample));
    FLGP_TRY(sink(PgChunkOut{st, p0, S, L.C.u, L.C.sk, L.P.x, L.P.sv, L.act.as<int>()}));
    // the slots' omega and f, packed: m x S from rows sv apart
    if (omega_out)
      FLGP_HIP(hipMemcpy2DAsync(omega_out + (size_t)p0 * m, vb, L.P.omega, sizeof(double) * (size_t)L.P.sv, vb, (size_t)S,
                                hipMemcpyDeviceToHost, st));
    if (f_out)
      FLGP_HIP(hipMemcpy2DAsync(f_out + (size_t)p0 * m, vb, L.P.f, sizeof(double) * (size_t)L.P.sv, vb, (size_t)S,
                                hipMemcpyDeviceToHost, st));
    FLGP_TRY(d2h(flags + p0, L.C.flag, sizeof(int) * (size_t)S, st));
  }
  return FLGP_OK;
}

// the lowest chain that met a pivot <= 0
int pg_flags_verdict(const char *who, bool name_chains, const int *flags, const double *ts, const unsigned long long *seeds, int B) {
  for (int b = 0; b < B; ++b)
    if (flags[b]) {
      const int rc = pg_pivot_error(flags[b], who);
      if (name_chains) pg_name_chain(b, ts, seeds);
      return rc;
    }
  return FLGP_OK;
}

// The three resident-pair entries after their argument checks (r0, r1 checked): chain b is column col[b] (NULL: b) of Y
// (m x ncol) at ts[b] with seeds[b]; its pi over the new rows into column b of pi_pred and, where asked for, its labels
// into y_pred, the first arg-max over the chains into argmax_out and its final omega and f into omega_out, f_out.
int pg_predict_chains(const char *who, bool name_chains, const flgp_eigenpair *ep, int K, Rows &r0, Rows &r1, const double *Y,
                      int ncol, const int *col, const double *ts, const unsigned long long *seeds, int B, double sigma,
                      double sigma_nv, int n_sample, int max_parallel, double *pi_pred, double *y_pred, double *argmax_out,
                      double *omega_out, double *f_out) {
  const int m = r0.m, mnew = r1.m;
  std::vector<int> cols((size_t)B);
  for (int b = 0; b < B; ++b) cols[(size_t)b] = col ? col[b] : b;
  Stream st;
  FLGP_TRY(st.create());
  const size_t vb = sizeof(double) * (size_t)m, nb = sizeof(double) * (size_t)mnew;
  const long sm = pad32(mnew);                 // doubles between two chains' means over the new rows
  DevBuf dY, dpi, dy, dlab, dflag, dmean;
  FLGP_TRY(upload(dY, Y, vb * ncol, st.s));
  FLGP_TRY(dpi.alloc(nb * B));
  if (y_pred) FLGP_TRY(dy.alloc(nb * B));
  FLGP_TRY(dmean.alloc(sizeof(double) * (size_t)sm * B));
  FLGP_TRY(r0.gather(st.s, ep, K));
  FLGP_TRY(r1.gather(st.s, ep, K));
  PgMatch match;
  if (sigma_nv != 0.0) FLGP_TRY(match.build(st.s, r0.idx, m, r1.idx, mnew));
  const long *mptr = sigma_nv != 0.0 ? match.ptr.as<long>() : nullptr;
  const int *mlist = sigma_nv != 0.0 ? match.list.as<int>() : nullptr;
  std::vector<int> flags((size_t)B, 0);       // one pivot flag per chain, read after the chain's sweeps
  // mean = V2 u, then pi = logistic(mean + sigma_nv sum_{idx0_j = idx1_i} w_j) into the chains' columns
  FLGP_TRY(pg_chains(st.s, ep, K, r0, dY.as<double>(), cols.data(), ts, seeds, B, sigma, n_sample, max_parallel, mnew, name_chains,
                     omega_out, f_out, flags.data(), dflag, [&](const PgChunkOut &o) -> int {
                       double *mean = dmean.as<double>() + (size_t)o.p0 * sm;
                       double *pi = dpi.as<double>() + (size_t)o.p0 * mnew;
                       double *y = y_pred ? dy.as<double>() + (size_t)o.p0 * mnew : nullptr;
                       if (!o.act) {
                         FLGP_TRY(gemm_nn(o.st, mnew, 1, K, r1.V, r1.ld, o.U, K, mean, nullptr, 0));
                         return pg_pi(o.st, mnew, mean, sigma_nv, mptr, mlist, o.w, pi, 1, y);
                       }
                       const GemmBatch gb{o.S, o.act, 0, o.su, sm, 0, 0};
                       FLGP_TRY(gemm_launch(o.st, mnew, 1, K, 1.0, r1.V, 1, r1.ld, o.U, 1, K, 0.0, nullptr, 0, 0, mean, 1, mnew,
                                            nullptr, 0, 0.0, nullptr, nullptr, nullptr, 0, nullptr, &gb));
                       return pgb_pi(o.st, mnew, o.S, mean, sm, sigma_nv, mptr, mlist, o.w, o.sw, pi, y, mnew);
                     }));
  if (argmax_out) {
    FLGP_TRY(dlab.alloc(nb));
    FLGP_TRY(pg_argmax(st.s, mnew, B, dpi.as<double>(), dlab.as<double>()));
    FLGP_TRY(d2h(argmax_out, dlab.p, nb, st.s));
  }
  FLGP_TRY(d2h(pi_pred, dpi.p, nb * B, st.s));
  if (y_pred) FLGP_TRY(d2h(y_pred, dy.p, nb * B, st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return pg_flags_verdict(who, name_chains, flags.data(), ts, seeds, B);
}
}  // namespace

// the batch entry's refusals that concern the trained state alone, in its order and wording; `also` is a further variance
// screened with sigma (the batch entry's sigma_nv)
int flgp::pg_operands_check(const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol,
                            const int *col, const double *ts, const unsigned long long *seeds, int B, double sigma, int n_sample,
                            double also) {
  FLGP_REQUIRE(idx0 && Y && ts && seeds, "%s: null pointer", who);
  FLGP_REQUIRE(B >= 1 && m >= 1 && ncol >= 1, "%s: bad shape (B=%d, m=%d, ncol=%d)", who, B, m, ncol);
  FLGP_REQUIRE(n_sample >= 1, "%s: N_sample=%d must be at least 1", who, n_sample);
  FLGP_REQUIRE(col || ncol == B, "%s: col may be NULL only if ncol == B (ncol=%d, B=%d)", who, ncol, B);
  for (int b = 0; b < B; ++b) {
    const int c = col ? col[b] : b;
    FLGP_REQUIRE(c >= 0 && c < ncol, "chain %d (t=%g, seed=%llu): %s: col=%d is outside [0, ncol=%d)", b, ts[b], seeds[b], who, c, ncol);
    FLGP_REQUIRE(std::isfinite(ts[b]), "chain %d (t=%g, seed=%llu): %s: t must be finite", b, ts[b], seeds[b], who);
  }
  for (int c = 0; c < ncol; ++c)
    for (int a = 0; a < m; ++a) {
      const double y = Y[(size_t)c * m + a];
      FLGP_REQUIRE(y >= 0.0 && y <= 1.0, "%s: Y[%d, %d]=%g is outside [0, 1]", who, a, c, y);
    }
  FLGP_REQUIRE(std::isfinite(sigma) && sigma >= 0.0 && std::isfinite(also), "%s: sigma must be finite and >= 0", who);
  FLGP_REQUIRE(ep, "%s: null eigenpair", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K, "%s: need 1 <= K <= %d (K=%d)", who, ep->K, K);
  Rows r0;
  return r0.check(ep, idx0, m, who, "idx0");
}

int flgp::pg_operands(hipStream_t st, const char *who, const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y,
                      int ncol, const int *col, const double *ts, const unsigned long long *seeds, int B, double sigma,
                      int n_sample, int max_parallel, double *omega_out, double *f_out, const PgSink &sink) {
  Rows r0;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  std::vector<int> cols((size_t)B), flags((size_t)B, 0);
  for (int b = 0; b < B; ++b) cols[(size_t)b] = col ? col[b] : b;
  DevBuf dY, dflag;
  FLGP_TRY(upload(dY, Y, sizeof(double) * (size_t)m * ncol, st));
  FLGP_TRY(r0.gather(st, ep, K));
  FLGP_TRY(pg_chains(st, ep, K, r0, dY.as<double>(), cols.data(), ts, seeds, B, sigma, n_sample, max_parallel, 0, true, omega_out,
                     f_out, flags.data(), dflag, [&](const PgChunkOut &o) { return sink(o.st, o.p0, o.S, o.U, o.su); }));
  FLGP_HIP(hipStreamSynchronize(st));
  return pg_flags_verdict(who, true, flags.data(), ts, seeds, B);
}

// Chain b is column col[b] of Y at ts[b] with seeds[b], and its columns of the outputs are the same bits whatever shares
// the call: the two entries below are this one with B = 1 and with B = J.
extern "C" int flgp_eigenpair_pg_predict_batch(const flgp_eigenpair *ep, int K, const int *idx0, int m, const double *Y, int ncol,
                                               const int *col, const double *ts, const unsigned long long *seeds, int B,
                                               double sigma, double sigma_nv, const int *idx1, int mnew, int n_sample,
                                               int max_parallel, double *pi_pred, double *y_pred, double *argmax_out,
                                               double *omega_out, double *f_out) {
  const char *who = "eigenpair_pg_predict_batch";
  // what concerns idx1, m_new and pi_pred stands where it stood among the refusals: the null pointers and the shape come first
  FLGP_REQUIRE(idx0 && Y && ts && seeds && idx1 && pi_pred, "%s: null pointer", who);
  FLGP_REQUIRE(B >= 1 && m >= 1 && mnew >= 1 && ncol >= 1, "%s: bad shape (B=%d, m=%d, m_new=%d, ncol=%d)", who, B, m, mnew, ncol);
  FLGP_TRY(pg_operands_check(who, ep, K, idx0, m, Y, ncol, col, ts, seeds, B, sigma, n_sample, sigma_nv));
  Rows r0, r1;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  FLGP_TRY(r1.check(ep, idx1, mnew, who, "idx1"));
  return pg_predict_chains(who, true, ep, K, r0, r1, Y, ncol, col, ts, seeds, B, sigma, sigma_nv, n_sample, max_parallel, pi_pred,
                           y_pred, argmax_out, omega_out, f_out);
}

// test_pgbinary_cpp on the resident pair: the batch of one
extern "C" int flgp_eigenpair_pg_predict(const flgp_eigenpair *ep, int K, double t, double sigma, double sigma_nv,
                                         const int *idx0, int m, const double *Y, const int *idx1, int mnew, int n_sample,
                                         unsigned long long seed, double *pi_pred, double *y_pred, double *omega_out,
                                         double *f_out) {
  const char *who = "eigenpair_pg_predict";
  FLGP_REQUIRE(idx0 && Y && idx1 && pi_pred && y_pred, "%s: null pointer", who);
  FLGP_REQUIRE(std::isfinite(t), "%s: t must be finite", who);
  FLGP_REQUIRE(std::isfinite(sigma) && sigma >= 0.0 && std::isfinite(sigma_nv), "%s: sigma must be finite and >= 0", who);
  FLGP_TRY(check_pg_common(Y, m, mnew, n_sample, who));
  FLGP_REQUIRE(ep, "%s: null eigenpair", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K, "%s: need 1 <= K <= %d (K=%d)", who, ep->K, K);
  Rows r0, r1;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  FLGP_TRY(r1.check(ep, idx1, mnew, who, "idx1"));
  return pg_predict_chains(who, false, ep, K, r0, r1, Y, 1, nullptr, &t, &seed, 1, sigma, sigma_nv, n_sample, 0, pi_pred, y_pred,
                           nullptr, omega_out, f_out);
}

// predict_logit_mult_gp_cpp (src/MultiClassification.cpp:57-88): one-vs-rest over the J classes of multi_train_split(Y), the
// batch of J on the indicator matrix: class j is flgp_eigenpair_pg_predict with t = ts[j], sigma_nv = 0 and seed + j, bit for
// bit.  The J chains run together: for m > K one chunk of up to J chains sharing every launch, as many as fit
// into 90 % of the free device memory (a chain's state is PgBatch::bytes: X alone 8 m K bytes, 16 MB at m = 1e4, K = 200);
// for m <= K min(J, 4) pool workers.  labels: the first arg-max of each row of probs (m_new x J).
extern "C" int flgp_eigenpair_pg_predict_multiclass(const flgp_eigenpair *ep, int K, const double *ts, int J, double sigma,
                                                    const int *idx0, int m, const double *Y, const int *idx1, int mnew,
                                                    int n_sample, unsigned long long seed, double *probs, double *labels) {
  const char *who = "eigenpair_pg_predict_multiclass";
  FLGP_REQUIRE(ts && idx0 && Y && idx1 && probs && labels, "%s: null pointer", who);
  FLGP_REQUIRE(J >= 1 && m >= 1 && mnew >= 1, "%s: bad shape (J=%d, m=%d, m_new=%d)", who, J, m, mnew);
  FLGP_REQUIRE(n_sample >= 1, "%s: N_sample=%d must be at least 1", who, n_sample);
  FLGP_REQUIRE(std::isfinite(sigma) && sigma >= 0.0, "%s: sigma must be finite and >= 0", who);
  for (int j = 0; j < J; ++j) FLGP_REQUIRE(std::isfinite(ts[j]), "%s: ts[%d] must be finite", who, j);
  for (int a = 0; a < m; ++a)
    FLGP_REQUIRE(Y[a] >= 0.0 && Y[a] < J && Y[a] == std::floor(Y[a]), "%s: Y[%d]=%g is not a class label in 0 .. %d", who, a,
                 Y[a], J - 1);
  FLGP_REQUIRE(ep, "%s: null eigenpair", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K, "%s: need 1 <= K <= %d (K=%d)", who, ep->K, K);
  Rows r0, r1;
  FLGP_TRY(r0.check(ep, idx0, m, who, "idx0"));
  FLGP_TRY(r1.check(ep, idx1, mnew, who, "idx1"));
  std::vector<double> aug((size_t)m * J, 0.0);          // multi_train_split (src/MultiClassification.cpp:14-26)
  for (int a = 0; a < m; ++a) aug[(size_t)Y[a] * m + a] = 1.0;
  std::vector<unsigned long long> seeds((size_t)J);
  for (int j = 0; j < J; ++j) seeds[(size_t)j] = seed + (unsigned long long)j;
  return pg_predict_chains(who, false, ep, K, r0, r1, aug.data(), J, nullptr, ts, seeds.data(), J, sigma, 0.0, n_sample, 0, probs,
                           nullptr, labels, nullptr, nullptr);
}

// ---- regression training objective for B (pair, x) problems in one call -------------------------------
// A training context: made once per grid of pairs, evaluated once per optimiser step.  What depends on (pair, rows, Y) only
// is built at create; an evaluation uploads the x of its problems and brings their values and gradients down.
// flgp_eigenpair_regression_objective is the context of one problem, made on the stack, evaluated once and gone: the library
// holds the Woodbury steps once.
namespace {
struct NoState {};
// The host's side of a buffer that is copied every evaluation: pinned for a context, which lives through many; plain memory
// for the single entry's, which is used once (a pageable copy, as its upload and d2h always were).
struct HostMirror {
  double *p = nullptr;
  bool pinned = false;
  ~HostMirror() { if (pinned) (void)hipHostFree(p); else std::free(p); }
  int alloc(size_t bytes, bool pin) {
    pinned = pin;
    if (pin) FLGP_HIP(hipHostMalloc((void **)&p, bytes, hipHostMallocDefault));
    else p = (double *)std::malloc(bytes);
    if (!p) { set_error("malloc of %zu bytes failed", bytes); return FLGP_ERR_NOMEM; }
    return FLGP_OK;
  }
};
}  // namespace

struct flgp_regression_batch {
  int B = 0, K = 0, m = 0, q = 0, nx = 0, chunk = 1, P = 0, max_parallel = 0, device = 0;
  bool different = false, posterior = false, direct = false;
  bool in_place = false;                          // the rows are a range and are read where the pair keeps them
  double sigma = 0.0, prior[5] = {0, 0, 0, 0, 0};
  std::vector<const flgp_eigenpair *> pairs;      // the P distinct ones, in order of first appearance
  std::vector<int> pair_of, idx;                  // problem -> pair; the rows (the host's copy)
  Stream st;
  DevBuf didx, dY, vals, V, M0, R0;               // per pair: K eigenvalues, the gathered rows, "same": V^T V and V^T Y
  DevBuf work0;                                   // the workspace of M0 and R0: giving it back waits for the device, so the
                                                  // one-shot context keeps it to its end and create returns it after its wait
  // pair p's rows (m x K) and their leading dimension: where the pair keeps them, or the gathered copy
  const double *rows_of(int p) const {
    return in_place ? (const double *)pairs[(size_t)p]->vectors.p + idx[0] : (const double *)V.p + (size_t)p * C.sx;
  }
  long ld_of(int p) const { return in_place ? pairs[(size_t)p]->n : m; }
  // the Woodbury route's chunk
  RgbChunk C{};
  LrChunk L{};                                    // its K x K factor under the lrb_* / wsb_* steps: K, Q, sq, flag
  DevBuf in, ls, alpha, Tq, R, Vta, M, Q, Li, Tb, Qinv, LsM, M1, d, ZV, Pm, logdet, flag, out, part;
  int planM = 1, planR = 1, planQi = 1;           // the splits of the single entry's products on its workspace
  size_t pe = 0, wi = 0;
  long sp = 0, stb = 0, in_elems = 0, off_c = 0, off_ci = 0, off_pair = 0, off_all = 0;
  HostMirror h_in, h_out;                         // of `in` and `out`
  const int *all = nullptr;                       // 0 .. chunk-1, in `in`

  static void plans(int m, int K, int q, int *pM, int *pR, int *pQi, size_t *pe, size_t *wi) {
    const size_t we = vt_work_elems(K, q);
    *pM = gemm_plan_split(K, K, m, we);
    *pR = gemm_plan_split(K, q, m, we);
    *pQi = gemm_plan_split(K, K, K, we);
    *wi = (size_t)32 * 64 * K;
    *pe = std::max(std::max((size_t)*pM * K * K, (size_t)*pR * K * q),
                   std::max((size_t)*pQi * K * K, wsb_tri_inverse_planes(K, *wi)));
  }
  // device bytes of one slot of the Woodbury chunk: x, c, 1 / c and the pair's number; ls; alpha, Tq; R, Vta; Q, Li, Qinv,
  // LsM, M1 and T (64 x K); its planes; logdet, the results and two flags; "different": M, d, ZV and P as well
  static double slot_bytes(int m, int K, int q, int nx, bool different) {
    int a, b, c;
    size_t pe, wi;
    plans(m, K, q, &a, &b, &c, &pe, &wi);
    double e = (double)pad32(nx) + 3.0 + pad32(K) + 2.0 * pad32((long)m * q) + 2.0 * pad32((long)K * q) +
               5.0 * pad32((long)K * K) + pad32((long)64 * K) + pad32((long)pe) + 1.0 + (1.0 + nx);
    if (different) e += (double)pad32((long)K * K) + pad32(m) + 2.0 * pad32((long)m * K);
    return 8.0 * e + 8.0;
  }
  int alloc_chunk(bool pinned) {
    RgbChunk &c = C;
    const size_t S = (size_t)chunk;
    plans(m, K, q, &planM, &planR, &planQi, &pe, &wi);
    sp = pad32((long)pe); stb = pad32((long)64 * K);
    c.sv = pad32(m); c.sk = pad32(K); c.skq = pad32((long)K * q); c.smq = pad32((long)m * q); c.sq = pad32((long)K * K);
    c.sx = pad32((long)m * K); c.sxn = pad32(nx);
    // one upload per chunk: [x of every slot | c | 1 / c | the pairs' numbers (ints) | 0 .. chunk-1 (ints), written once]
    off_c = (long)S * c.sxn; off_ci = off_c + pad32(chunk); off_pair = off_ci + pad32(chunk); off_all = off_pair + pad32(chunk);
    in_elems = off_all + pad32(chunk);
    FLGP_TRY(in.alloc(sizeof(double) * (size_t)in_elems));
    FLGP_TRY(ls.alloc(sizeof(double) * S * c.sk));
    FLGP_TRY(alpha.alloc(sizeof(double) * S * c.smq)); FLGP_TRY(Tq.alloc(sizeof(double) * S * c.smq));
    FLGP_TRY(R.alloc(sizeof(double) * S * c.skq)); FLGP_TRY(Vta.alloc(sizeof(double) * S * c.skq));
    FLGP_TRY(Q.alloc(sizeof(double) * S * c.sq)); FLGP_TRY(Li.alloc(sizeof(double) * S * c.sq));
    FLGP_TRY(Qinv.alloc(sizeof(double) * S * c.sq)); FLGP_TRY(LsM.alloc(sizeof(double) * S * c.sq));
    FLGP_TRY(M1.alloc(sizeof(double) * S * c.sq)); FLGP_TRY(Tb.alloc(sizeof(double) * S * stb));
    FLGP_TRY(part.alloc(sizeof(double) * S * std::max(sp, 32L)));
    FLGP_TRY(logdet.alloc(sizeof(double) * S)); FLGP_TRY(flag.alloc(sizeof(int) * S));
    FLGP_TRY(out.alloc(sizeof(double) * S * (size_t)(1 + nx) + sizeof(int) * S));
    if (different) {
      FLGP_TRY(M.alloc(sizeof(double) * S * c.sq)); FLGP_TRY(d.alloc(sizeof(double) * S * c.sv));
      FLGP_TRY(ZV.alloc(sizeof(double) * S * c.sx)); FLGP_TRY(Pm.alloc(sizeof(double) * S * c.sx));
    }
    FLGP_TRY(h_in.alloc(sizeof(double) * (size_t)in_elems, pinned));
    FLGP_TRY(h_out.alloc(sizeof(double) * S * (size_t)(1 + nx) + sizeof(int) * S, pinned));
    std::memset(h_in.p, 0, sizeof(double) * (size_t)in_elems);
    for (size_t s = 0; s < S; ++s) ((int *)(h_in.p + off_all))[s] = (int)s;
    c.m = m; c.q = q; c.K = K; c.nx = nx; c.different = different; c.posterior = posterior; c.grad = 1;
    c.sigma = sigma;
    for (int a = 0; a < 5; ++a) c.prior[a] = prior[a];
    c.x = in.as<double>(); c.c = c.x + off_c; c.ci = c.x + off_ci; c.pair = (const int *)(c.x + off_pair);
    all = (const int *)(c.x + off_all);
    c.values = vals.as<double>(); c.V = rows_of(0); c.M0 = M0.as<double>(); c.Y = dY.as<double>();
    c.ls = ls.as<double>(); c.alpha = alpha.as<double>(); c.Tq = Tq.as<double>(); c.R = R.as<double>(); c.Vta = Vta.as<double>();
    c.M = M.as<double>(); c.Q = Q.as<double>(); c.Li = Li.as<double>(); c.Qinv = Qinv.as<double>(); c.LsM = LsM.as<double>();
    c.M1 = M1.as<double>(); c.d = d.as<double>(); c.ZV = ZV.as<double>(); c.P = Pm.as<double>();
    c.logdet = logdet.as<double>(); c.flag = flag.as<int>(); c.out = out.as<double>();
    L = LrChunk{};
    L.m = m; L.K = K; L.slots = chunk; L.sv = c.sv; L.sk = c.sk; L.sx = c.sx; L.sq = c.sq;
    L.Q = c.Q; L.flag = c.flag;
    return FLGP_OK;
  }
  // one batched product on the chunk's planes; la / lb: the list of the A / B operand where it is not the slots' own
  int gemm(int S, int Mr, int Nc, int Kd, const double *A, long a_is, long a_ks, long a_bs, const int *la, const double *Bm,
           long b_ks, long b_js, long b_bs, double *Cm, long c_js, long c_bs, int split) {
    GemmBatch gb{S, all, a_bs, b_bs, c_bs, 0, split ? sp : 0};
    gb.a_slots = la;
    return gemm_launch(st.s, Mr, Nc, Kd, 1.0, A, a_is, a_ks, Bm, b_ks, b_js, 0.0, nullptr, 0, 0, Cm, 1, c_js,
                       split ? part.as<double>() : nullptr, split ? pe : 0, 0.0, nullptr, nullptr, nullptr, split, nullptr, &gb);
  }
  // Woodbury (:395-405, :492-502) for the S slots whose x, c and pairs are in h_in, every step one launch: M = V^T V or
  // V^T Z^-1 V, Q = Ls M Ls + (c or 1) I, alpha = Z^-1 (Y - V Ls Q^-1 Ls V^T Z^-1 Y), then value and gradient.  The factor
  // of Q stays for the log-determinant and the gradient, so this is a blocked Cholesky, not woodbury_step's chol_solve.
  int woodbury_chunk(int S, bool grad) {
    RgbChunk &c = C;
    hipStream_t s = st.s;
    c.grad = grad ? 1 : 0;
    const int *pl = c.pair, *a = all;
    const long ldv = ld_of(0);
    FLGP_TRY(h2d(in.p, h_in.p, sizeof(double) * (size_t)in_elems, s));
    FLGP_HIP(hipMemsetAsync(c.flag, 0, sizeof(int) * (size_t)S, s));
    FLGP_TRY(rgb_weights(s, c, S));
    if (different) {
      FLGP_TRY(rgb_zinv(s, c, S));                                                                        // d = z^-1 for now
      FLGP_TRY(rgb_rowscale(s, S, m, K, c.V, ldv, c.sx, pl, c.d, c.sv, c.ZV, c.sx));                      // Z^-1 V
      FLGP_TRY(rgb_rowscale(s, S, m, q, c.Y, m, 0, nullptr, c.d, c.sv, c.alpha, c.smq));                // Z^-1 Y
      FLGP_TRY(gemm(S, K, K, m, c.V, ldv, 1, c.sx, pl, c.ZV, 1, m, c.sx, c.M, K, c.sq, planM));           // M = V^T Z^-1 V
      FLGP_TRY(gemm(S, K, q, m, c.V, ldv, 1, c.sx, pl, c.alpha, 1, m, c.smq, c.R, K, c.skq, planR));      // V^T Z^-1 Y
    }
    FLGP_TRY(rgb_q(s, c, S));
    FLGP_TRY(lrb_chol(s, L, a, S));
    // Ls V^T Z^-1 Y ("same": from the pair's R0), Q^-1 (.), Ls (.)
    if (different) FLGP_TRY(rgb_scale(s, S, K, q, c.R, c.skq, nullptr, c.ls, c.sk, nullptr, 0, c.R, c.skq));
    else FLGP_TRY(rgb_scale(s, S, K, q, R0.as<double>(), c.skq, pl, c.ls, c.sk, nullptr, 0, c.R, c.skq));
    FLGP_TRY(lrb_trsv_cols(s, L, a, S, c.R, c.skq, q));
    FLGP_TRY(rgb_scale(s, S, K, q, c.R, c.skq, nullptr, c.ls, c.sk, nullptr, 0, c.R, c.skq));
    FLGP_TRY(gemm(S, m, q, K, c.V, 1, ldv, c.sx, pl, c.R, 1, K, c.skq, c.Tq, m, c.smq, 0));               // V (.)
    FLGP_TRY(rgb_diff(s, S, (long)m * q, c.Y, 0, c.Tq, c.smq, c.ci, c.alpha, c.smq));
    if (different) FLGP_TRY(rgb_rowscale(s, S, m, q, c.alpha, m, c.smq, nullptr, c.d, c.sv, c.alpha, c.smq));
    if (grad) {
      // Q^-1 = L_Q^-T L_Q^-1, M1 = Q^-1 Ls M, V^T alpha; "different": d_i = |row i of V Ls L_Q^-T|^2
      const double *Mm = different ? c.M : c.M0;
      const int *ml = different ? nullptr : pl;
      FLGP_TRY(wsb_tri_inverse(s, L, a, S, c.Li, Tb.as<double>(), stb, part.as<double>(), pe, sp, wi));
      FLGP_TRY(gemm(S, K, K, K, c.Li, K, 1, c.sq, nullptr, c.Li, 1, K, c.sq, c.Qinv, K, c.sq, planQi));
      FLGP_TRY(rgb_scale(s, S, K, K, Mm, c.sq, ml, c.ls, c.sk, nullptr, 0, c.LsM, c.sq));
      FLGP_TRY(gemm(S, K, K, K, c.Qinv, 1, K, c.sq, nullptr, c.LsM, 1, K, c.sq, c.M1, K, c.sq, 0));
      FLGP_TRY(gemm(S, K, q, m, c.V, ldv, 1, c.sx, pl, c.alpha, 1, m, c.smq, c.Vta, K, c.skq, planR));
      if (different) {
        FLGP_TRY(rgb_scale(s, S, K, K, c.Li, c.sq, nullptr, nullptr, 0, c.ls, c.sk, c.LsM, c.sq));     // reuse: Li Ls
        FLGP_TRY(gemm(S, m, K, K, c.V, 1, ldv, c.sx, pl, c.LsM, K, 1, c.sq, c.P, m, c.sx, 0));            // P = V (Li Ls)^T
        FLGP_TRY(rgb_rowsumsq(s, S, c.P, c.sx, m, m, K, c.d, c.sv));
      }
    }
    FLGP_TRY(rgb_assemble(s, c, S));
    FLGP_TRY(d2h(h_out.p, out.p, sizeof(double) * (size_t)S * (1 + nx) + sizeof(int) * (size_t)S, s));
    FLGP_HIP(hipStreamSynchronize(s));
    return FLGP_OK;
  }
  // one problem of the direct route (m <= K) on the worker's stream: the spectral weights, x up and what the steps fill; Y
  // and the rows are the context's
  int direct_one(hipStream_t ws, const char *who, int b, const double *x, double *value, double *grad) {
    const int p = pair_of[(size_t)b];
    const flgp_eigenpair *ep = pairs[(size_t)p];
    RgDirect E;
    E.st = ws; E.ep = ep; E.x = x;
    Rows &r = E.r;
    r.idx = idx.data(); r.m = m; r.resolved = true; r.gathered_K = K;
    r.V = rows_of(p); r.ld = ld_of(p);
    if (in_place) r.row0 = idx[0];
    else r.d = didx.as<int>();
    RgTerms &T = E.T;
    T.m = m; T.q = q; T.K = K; T.direct = 1; T.different = different; T.posterior = posterior; T.grad = grad != nullptr;
    T.sigma = sigma; T.c = different ? 1.0 : x[1] + sigma;
    for (int a = 0; a < 5; ++a) T.prior[a] = prior[a];
    FLGP_TRY(E.G.prepare(ws, ep, K, x[0]));
    E.dY.borrow(dY.p);
    FLGP_TRY(upload(E.dx, x, sizeof(double) * (size_t)nx, ws));
    FLGP_TRY(E.alpha.alloc(sizeof(double) * (size_t)m * q)); FLGP_TRY(E.out.alloc(sizeof(double) * (size_t)(1 + nx)));
    FLGP_TRY(E.ld.alloc(sizeof(double)));
    if (T.grad) { FLGP_TRY(E.Vta.alloc(sizeof(double) * (size_t)K * q)); FLGP_TRY(E.d.alloc(sizeof(double) * (size_t)m)); }
    FLGP_TRY(E.terms());
    return E.finish(who, nx, value, grad);
  }
};

namespace {
constexpr double RG_DEFAULT_PRIOR[5] = {1.0, 10.0, 2.0, 0.1, 1e-3};         // PostOFDataReg (src/train.h:153-155)

// the two strings of every entry, refused with the reference's texts
int rg_strings(const char *who, const char *noise, const char *approach, bool *different, bool *posterior) {
  FLGP_REQUIRE(noise && approach, "%s: null pointer", who);
  *different = std::strcmp(noise, "different") == 0;
  if (!*different && std::strcmp(noise, "same") != 0) { set_error("The noise setting is illegal!"); return FLGP_ERR_UNSUPPORTED; }
  *posterior = std::strcmp(approach, "posterior") == 0;
  if (!*posterior && std::strcmp(approach, "marginal") != 0) {
    set_error("This model selection approach is not supported!");
    return FLGP_ERR_UNSUPPORTED;
  }
  return FLGP_OK;
}

// what every entry refuses about one x; `at`: "" or "position <a>: "
int rg_check_x(const char *at, const char *who, const double *x, int nx, double sigma, bool posterior) {
  FLGP_REQUIRE(all_finite(x, nx), "%s%s: x must be finite", at, who);
  for (int i = 1; i < nx; ++i) FLGP_REQUIRE(x[i] + sigma > 0.0, "%s%s: x[%d] + sigma must be positive", at, who, i);
  FLGP_REQUIRE(!posterior || x[0] > 0.0, "%s%s: t = x[0] must be positive under \"posterior\"", at, who);
  return FLGP_OK;
}

// The context of the problems eps[0 .. B-1], whose arguments the entry has checked: what depends on (pair, rows, Y) only.
// Nothing here waits for the device, so the one-shot call queues its evaluation behind this.  `pinned`: see HostMirror.
int rg_build(flgp_regression_batch &h, const flgp_eigenpair *const *eps, int B, int K, const int *idx, int m, const double *Y,
             int q, double sigma, bool different, bool posterior, const double *prior, int max_parallel, bool pinned) {
  h.B = B; h.K = K; h.m = m; h.q = q; h.nx = different ? m + 1 : 2; h.max_parallel = max_parallel;
  h.different = different; h.posterior = posterior; h.direct = m <= K; h.sigma = sigma;
  h.device = eps[0]->device;
  for (int a = 0; a < 5; ++a) h.prior[a] = prior ? prior[a] : RG_DEFAULT_PRIOR[a];
  h.pair_of.resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    size_t p = 0;
    while (p < h.pairs.size() && h.pairs[p] != eps[b]) ++p;
    if (p == h.pairs.size()) h.pairs.push_back(eps[b]);
    h.pair_of[(size_t)b] = (int)p;
  }
  h.P = (int)h.pairs.size();
  h.idx.assign(idx, idx + m);
  // A range of rows is read in place, as Rows::gather reads it: by the direct route always, by the Woodbury route -- whose
  // launches take one base and one leading dimension for every pair -- where there is one pair.  Any other rows are
  // gathered, every distinct pair's into one buffer under the slots' strides.
  h.in_place = is_range(idx, m) && (h.direct || h.P == 1);
  FLGP_TRY(h.st.create());
  hipStream_t st = h.st.s;
  FLGP_TRY(upload(h.dY, Y, sizeof(double) * (size_t)m * q, st));
  const long sx = pad32((long)m * K), sk = pad32(K), sq = pad32((long)K * K), skq = pad32((long)K * q);
  h.C.sx = sx;
  if (!h.in_place) {
    FLGP_TRY(upload(h.didx, idx, sizeof(int) * (size_t)m, st));
    FLGP_TRY(h.V.alloc(sizeof(double) * (size_t)h.P * sx));
    for (int p = 0; p < h.P; ++p)
      FLGP_TRY(flgp_dev_gather_rows(st, (const double *)h.pairs[(size_t)p]->vectors.p, h.pairs[(size_t)p]->n, h.didx.as<int>(), m,
                                    K, h.V.as<double>() + (size_t)p * sx));
  }
  if (h.direct) {
    h.chunk = plan_workers(max_parallel, B, 0.0, 0.0);
    return FLGP_OK;
  }
  if (h.P == 1) h.vals.borrow(h.pairs[0]->values.p);      // a lone pair's eigenvalues are read where they are
  else FLGP_TRY(h.vals.alloc(sizeof(double) * (size_t)h.P * sk));
  for (int p = 0; h.P > 1 && p < h.P; ++p)
    FLGP_HIP(hipMemcpyAsync(h.vals.as<double>() + (size_t)p * sk, h.pairs[(size_t)p]->values.p, sizeof(double) * (size_t)K,
                            hipMemcpyDeviceToDevice, st));
  if (!different) {
    // M0 = V^T V and R0 = V^T Y per pair, on the workspace that decides their split
    const size_t we = vt_work_elems(K, q);
    DevBuf &work = h.work0;
    FLGP_TRY(work.alloc(sizeof(double) * we));
    FLGP_TRY(h.M0.alloc(sizeof(double) * (size_t)h.P * sq)); FLGP_TRY(h.R0.alloc(sizeof(double) * (size_t)h.P * skq));
    for (int p = 0; p < h.P; ++p) {
      const double *Vp = h.rows_of(p);
      const long ld = h.ld_of(p);
      FLGP_TRY(gemm_tn(st, K, K, m, Vp, ld, Vp, ld, h.M0.as<double>() + (size_t)p * sq, work.as<double>(), we));
      FLGP_TRY(gemm_tn(st, K, q, m, Vp, ld, h.dY.as<double>(), m, h.R0.as<double>() + (size_t)p * skq, work.as<double>(), we));
    }
  }
  // the chunk: max_parallel problems, or (<= 0) all of them; where that is more than one, no more than fit into 90 % of the
  // free memory
  const int want = max_parallel > 0 ? max_parallel : B;
  size_t free_b = 0, total_b = 0;
  if (plan_workers(want, B, 0.0, 0.0) > 1) FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
  h.chunk = std::min(plan_workers(want, B, (double)free_b, flgp_regression_batch::slot_bytes(m, K, q, h.nx, different)),
                     GEMM_BATCH_MAX);
  return h.alloc_chunk(pinned);
}

// A evaluations on a context, whose arguments the entry has checked.  A failed position is reported under `who`, as
// "position <a>: ..." where by_position.
int rg_eval(flgp_regression_batch &h, const char *who, bool by_position, const int *prob, int A, const double *X, int ldx,
            double *values, double *grads, int ldg, int *status) {
  const int nx = h.nx, m = h.m;
  std::vector<int> stat((size_t)A, FLGP_OK);
  std::vector<std::string> why((size_t)A);
  const int cnt = grads ? nx + 1 : 1;
  auto fail = [&](int a, const std::string &verdict) {
    stat[(size_t)a] = FLGP_ERR_NOCONV;
    why[(size_t)a] = verdict;
    if (!by_position) return;                           // the single entry leaves its outputs as they were, as it always did
    values[a] = std::nan("");
    if (grads) std::fill(grads + (size_t)a * ldg, grads + (size_t)a * ldg + nx, std::nan(""));
  };
  auto report = [&](int a, const std::string &text, int rc) {
    if (by_position) set_error("position %d: %s", a, text.c_str());
    else set_error("%s", text.c_str());
    return rc;
  };
  if (h.direct) {
    // the problems dealt to the pool's workers (worker_pool.h); one worker runs on the calling thread and the context's stream
    DevicePool pool;
    FLGP_TRY(pool.plan(h.max_parallel, A, 8.0 * (4.0 * m * m + 96.0 * m + (double)m * h.K + 2.0 * m * h.q) +
                                              (double)flgp_dev_hk_workspace(m, m, h.K, 1)));
    const PoolFailure bad = pool.run<NoState>(
        h.st.s, A, [](NoState &) { return FLGP_OK; },
        [&](hipStream_t ws, NoState &, int a) -> int {
          const int b = prob ? prob[a] : a;
          const int rc = h.direct_one(ws, who, b, X + (size_t)a * ldx, &values[a], grads ? grads + (size_t)a * ldg : nullptr);
          if (rc == FLGP_ERR_NOCONV) { fail(a, flgp_last_error()); return FLGP_OK; }
          return rc;
        });
    if (bad.item >= 0) return report(bad.item, bad.message, bad.status);
  } else {
    for (int p0 = 0; p0 < A; p0 += h.chunk) {
      const int S = std::min(h.chunk, A - p0);
      int *hpair = (int *)(h.h_in.p + h.off_pair);
      for (int s = 0; s < S; ++s) {
        const int a = p0 + s, b = prob ? prob[a] : a;
        const double *x = X + (size_t)a * ldx;
        std::memcpy(h.h_in.p + (size_t)s * h.C.sxn, x, sizeof(double) * (size_t)nx);
        const double c = h.different ? 1.0 : x[1] + h.sigma;
        h.h_in.p[h.off_c + s] = c;
        h.h_in.p[h.off_ci + s] = h.different ? 1.0 : 1.0 / c;
        hpair[s] = h.pair_of[(size_t)b];
      }
      FLGP_TRY(h.woodbury_chunk(S, grads != nullptr));
      const int *flags = (const int *)(h.h_out.p + (size_t)S * (1 + nx));
      for (int s = 0; s < S; ++s) {                     // the flag is judged before the numbers
        const int a = p0 + s;
        const double *o = h.h_out.p + (size_t)s * (1 + nx);
        if (flags[s]) { fail(a, not_positive_definite(who)); continue; }
        if (!all_finite(o, cnt)) { fail(a, not_finite(who)); continue; }
        values[a] = o[0];
        if (grads) std::memcpy(grads + (size_t)a * ldg, o + 1, sizeof(double) * (size_t)nx);
      }
    }
  }
  if (status) { std::memcpy(status, stat.data(), sizeof(int) * (size_t)A); return FLGP_OK; }
  for (int a = 0; a < A; ++a)
    if (stat[(size_t)a] != FLGP_OK) return report(a, why[(size_t)a], stat[(size_t)a]);
  return FLGP_OK;
}
}  // namespace

// negative_marginal_likelihood{,_diff_noise}_regression_cpp (src/train.cpp:351-436, 459-555) and their posterior forms
// (:333-348, 438-457): the context of one problem.  The m x m matrices of the direct branch (C^-1, U, G) are replaced by L^-1
// (gpr_grad.hip); the Woodbury branch forms alpha (m x q) as the reference does.
extern "C" int flgp_eigenpair_regression_objective(const flgp_eigenpair *ep, int K, const int *idx, int m, const double *Y, int q,
                                                   double sigma, const char *noise, const char *approach, const double *prior,
                                                   const double *x, int nx, double *value, double *grad) {
  const char *who = "regression_objective";
  bool different = false, posterior = false;
  FLGP_TRY(rg_strings(who, noise, approach, &different, &posterior));
  FLGP_REQUIRE(ep && idx && Y && x && value, "%s: null pointer", who);
  FLGP_REQUIRE(K >= 1 && K <= ep->K && m >= 1 && q >= 1, "%s: bad shape (K=%d of %d, m=%d, q=%d)", who, K, ep->K, m, q);
  FLGP_REQUIRE(nx == (different ? m + 1 : 2), "%s: noise \"%s\" takes %d parameters, not %d", who, noise, different ? m + 1 : 2, nx);
  FLGP_TRY(rg_check_x("", who, x, nx, sigma, posterior));
  for (int a = 0; a < m; ++a) FLGP_REQUIRE(idx[a] >= 0 && idx[a] < ep->n, "%s: idx[%d]=%d out of range", who, a, idx[a]);
  flgp_regression_batch h;
  FLGP_TRY(rg_build(h, &ep, 1, K, idx, m, Y, q, sigma, different, posterior, prior, 1, false));
  return rg_eval(h, who, false, nullptr, 1, x, nx, value, grad, nx, nullptr);
}

extern "C" int flgp_regression_batch_create(const flgp_eigenpair *const *eps, int B, int K, const int *idx, int m,
                                            const double *Y, int q, double sigma, const char *noise, const char *approach,
                                            const double *prior, int max_parallel, flgp_regression_batch **out) {
  const char *who = "regression_objective_batch";
  bool different = false, posterior = false;
  FLGP_TRY(rg_strings(who, noise, approach, &different, &posterior));
  FLGP_REQUIRE(eps && idx && Y && out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(B >= 1, "%s: B=%d problems", who, B);
  for (int b = 0; b < B; ++b) {
    FLGP_REQUIRE(eps[b], "problem %d: %s: null pointer", b, who);
    FLGP_REQUIRE(K >= 1 && K <= eps[b]->K && m >= 1 && q >= 1, "problem %d: %s: bad shape (K=%d of %d, m=%d, q=%d)", b, who, K,
                 eps[b]->K, m, q);
    FLGP_REQUIRE(eps[b]->device == eps[0]->device, "problem %d: %s: the pair lives on device %d, problem 0's on device %d", b,
                 who, eps[b]->device, eps[0]->device);
  }
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < m; ++a)
      FLGP_REQUIRE(idx[a] >= 0 && idx[a] < eps[b]->n, "problem %d: %s: idx[%d]=%d out of range", b, who, a, idx[a]);
  int dev = 0;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == eps[0]->device, "%s: the pairs live on device %d, the current device is %d", who, eps[0]->device, dev);
  std::unique_ptr<flgp_regression_batch> H(new flgp_regression_batch);
  FLGP_TRY(rg_build(*H, eps, B, K, idx, m, Y, q, sigma, different, posterior, prior, max_parallel, true));
  FLGP_HIP(hipStreamSynchronize(H->st.s));                // the caller's idx and Y have gone up
  H->work0.release();
  *out = H.release();
  return FLGP_OK;
}

extern "C" int flgp_regression_batch_dims(const flgp_regression_batch *h, int *B, int *K, int *m, int *q, int *nx, int *chunk) {
  FLGP_REQUIRE(h, "regression_objective_batch: null pointer");
  if (B) *B = h->B;
  if (K) *K = h->K;
  if (m) *m = h->m;
  if (q) *q = h->q;
  if (nx) *nx = h->nx;
  if (chunk) *chunk = h->chunk;
  return FLGP_OK;
}

extern "C" void flgp_regression_batch_free(flgp_regression_batch *h) { delete h; }

extern "C" int flgp_regression_batch_eval(flgp_regression_batch *hp, const int *prob, int A, const double *X, int ldx,
                                          double *values, double *grads, int ldg, int *status) {
  const char *who = "regression_objective_batch";
  FLGP_REQUIRE(hp && X && values, "%s: null pointer", who);
  flgp_regression_batch &h = *hp;
  const int nx = h.nx;
  FLGP_REQUIRE(A >= 1, "%s: A=%d problems", who, A);
  FLGP_REQUIRE(prob || A == h.B, "%s: prob may be NULL only if A == B (A=%d, B=%d)", who, A, h.B);
  FLGP_REQUIRE(ldx >= nx, "%s: noise \"%s\" takes %d parameters, not %d", who, h.different ? "different" : "same", nx, ldx);
  FLGP_REQUIRE(!grads || ldg >= nx, "%s: noise \"%s\" takes %d parameters, not %d", who, h.different ? "different" : "same", nx,
               ldg);
  for (int a = 0; a < A; ++a) {
    const int b = prob ? prob[a] : a;
    char at[32];
    std::snprintf(at, sizeof at, "position %d: ", a);
    FLGP_REQUIRE(b >= 0 && b < h.B, "%s%s: prob=%d is outside [0, B=%d)", at, who, b, h.B);
    FLGP_TRY(rg_check_x(at, who, X + (size_t)a * ldx, nx, h.sigma, h.posterior));
  }
  int dev = 0;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == h.device, "%s: the pairs live on device %d, the current device is %d", who, h.device, dev);
  return rg_eval(h, who, true, prob, A, X, ldx, values, grads, ldg, status);
}


// ---- logit training context: B (pair, labels, t) problems per evaluation on state made once ------------
// What create keeps: one stream; idx, Y, N and the problems' columns on the device; for m > K every distinct pair's rows
// (m x K) in one buffer under the slots' stride and the pairs' eigenvalues at stride sk (a lone pair's are read where they
// are, and a range of its rows in place), the chunk's LrBatch and one pinned upload buffer; for m <= K the resolved rows.
struct flgp_logit_batch {
  int B = 0, P = 0, K = 0, m = 0, ncol = 0, chunk = 1, max_parallel = 0, max_iter = 0, device = 0;
  bool posterior = false, dense = false, in_place = false;
  double sigma = 0.0, tol = 0.0, pr[3] = {0, 0, 0};
  std::vector<const flgp_eigenpair *> pairs;      // the P distinct ones, in order of first appearance
  std::vector<int> pair_of, col, idx;             // problem -> pair, problem -> column of Y; the rows (the host's copy)
  Stream st;
  DevBuf didx, dY, dN, V, vals, in;
  LrBatch L;                                      // the low-rank route's chunk
  HostMirror h_in;                                // one upload per chunk: [t of every slot | its column (ints) | its pair (ints)]
  long off_col = 0, off_pair = 0, in_elems = 0;

  // the rows as the dense route's contraction takes them: resolved at create, nothing owned
  void rows(Rows &r) const {
    r.idx = idx.data(); r.m = m; r.resolved = true;
    if (in_place) r.row0 = idx[0];
    else r.d = (const int *)didx.p;
  }
};

namespace {
const char *const LB_WHO = "logit_objective_context";

// The context of the checked problems: what depends on (pairs, rows, Y, N) only.
int lb_build(flgp_logit_batch &h, const flgp_eigenpair *const *eps, const int *col, int B, int K, const int *idx, int m,
             const double *Y, int ncol, const double *N, double sigma, bool posterior, const double *pr, double tol, int max_iter,
             int max_parallel) {
  h.B = B; h.K = K; h.m = m; h.ncol = ncol; h.max_parallel = max_parallel; h.max_iter = max_iter;
  h.posterior = posterior; h.dense = m <= K; h.sigma = sigma; h.tol = tol;
  h.device = eps[0]->device;
  for (int a = 0; a < 3; ++a) h.pr[a] = pr[a];
  h.pair_of.resize((size_t)B); h.col.resize((size_t)B);
  for (int b = 0; b < B; ++b) {
    size_t p = 0;
    while (p < h.pairs.size() && h.pairs[p] != eps[b]) ++p;
    if (p == h.pairs.size()) h.pairs.push_back(eps[b]);
    h.pair_of[(size_t)b] = (int)p;
    h.col[(size_t)b] = col ? col[b] : b;
  }
  h.P = (int)h.pairs.size();
  h.idx.assign(idx, idx + m);
  // A range of rows is read in place, as Rows::gather reads it: by the dense route always (its contraction reads the
  // pair's own rows), by the low-rank route -- whose launches take one base and one leading dimension -- for a lone pair.
  h.in_place = is_range(idx, m) && (h.dense || h.P == 1);
  FLGP_TRY(h.st.create());
  hipStream_t st = h.st.s;
  std::vector<double> ones;
  if (!N) { ones.assign((size_t)m, 1.0); N = ones.data(); }
  FLGP_TRY(upload(h.dY, Y, sizeof(double) * (size_t)m * ncol, st));
  FLGP_TRY(upload(h.dN, N, sizeof(double) * (size_t)m, st));
  if (!h.in_place) FLGP_TRY(upload(h.didx, idx, sizeof(int) * (size_t)m, st));
  if (h.dense) {
    h.chunk = plan_workers(max_parallel, B, 0.0, 0.0);
    FLGP_HIP(hipStreamSynchronize(st));          // `ones` goes with this frame
    return FLGP_OK;
  }
  const long sx = pad32((long)m * K), sk = pad32(K);
  if (!h.in_place) {
    FLGP_TRY(h.V.alloc(sizeof(double) * (size_t)h.P * sx));
    for (int p = 0; p < h.P; ++p)
      FLGP_TRY(flgp_dev_gather_rows(st, (const double *)h.pairs[(size_t)p]->vectors.p, h.pairs[(size_t)p]->n, h.didx.as<int>(), m,
                                    K, h.V.as<double>() + (size_t)p * sx));
  }
  if (h.P == 1) h.vals.borrow(h.pairs[0]->values.p);      // a lone pair's eigenvalues are read where they are
  else FLGP_TRY(h.vals.alloc(sizeof(double) * (size_t)h.P * sk));
  for (int p = 0; h.P > 1 && p < h.P; ++p)
    FLGP_HIP(hipMemcpyAsync(h.vals.as<double>() + (size_t)p * sk, h.pairs[(size_t)p]->values.p, sizeof(double) * (size_t)K,
                            hipMemcpyDeviceToDevice, st));
  // the chunk, as the batch entry plans it: max_parallel problems, or (<= 0) all of them; where that is more than one, no
  // more than fit into 90 % of the free memory
  const int want = max_parallel > 0 ? max_parallel : B;
  size_t free_b = 0, total_b = 0;
  if (plan_workers(want, B, 0.0, 0.0) > 1) FLGP_HIP(hipMemGetInfo(&free_b, &total_b));
  h.chunk = std::min(plan_workers(want, B, (double)free_b, LrBatch::bytes(m, K)), GEMM_BATCH_MAX);
  FLGP_TRY(h.L.alloc(m, K, h.chunk));
  h.off_col = pad32(h.chunk); h.off_pair = 2 * h.off_col; h.in_elems = 3 * h.off_col;
  FLGP_TRY(h.in.alloc(sizeof(double) * (size_t)h.in_elems));
  FLGP_TRY(h.h_in.alloc(sizeof(double) * (size_t)h.in_elems, true));
  std::memset(h.h_in.p, 0, sizeof(double) * (size_t)h.in_elems);
  LrChunk &C = h.L.C;
  C.Y = h.dY.as<double>(); C.ldy = m; C.N = h.dN.as<double>(); C.sigma = sigma;
  C.ycol = (const int *)(h.in.as<double>() + h.off_col);
  C.V1 = h.in_place ? (const double *)h.pairs[0]->vectors.p + idx[0] : h.V.as<double>();
  C.ld1 = h.in_place ? h.pairs[0]->n : m;
  if (h.P > 1) {                                  // a slot finds its pair through the list; one pair is the shared V1
    C.pair = (const int *)(h.in.as<double>() + h.off_pair); C.s1 = sx;
    h.L.pair_h = (const int *)(h.h_in.p + h.off_pair);
  }
  FLGP_HIP(hipStreamSynchronize(st));            // the caller's idx, Y and N have gone up
  return FLGP_OK;
}

// A checked evaluations.  A position whose factorisation meets a pivot <= 0 fails alone (status, NaN).
int lb_eval(flgp_logit_batch &h, const int *prob, int A, const double *ts, double *values, int *iters, int *status) {
  const char *who = LB_WHO;
  const int m = h.m, K = h.K;
  std::vector<int> stat((size_t)A, FLGP_OK), its((size_t)A, 0);
  std::vector<double> amll((size_t)A, 0.0);
  std::vector<std::string> why((size_t)A);
  auto report = [&](int a, const std::string &text, int rc) {
    set_error("position %d (t=%g): %s", a, ts[a], text.c_str());
    return rc;
  };
  if (h.dense) {
    // the dense loop per position, the positions dealt to the pool's workers; one worker runs on the context's stream
    DevicePool pool;
    FLGP_TRY(pool.plan(h.max_parallel, A, DenseObjWorker::bytes(m, K)));
    const PoolFailure bad = pool.run<DenseObjWorker>(
        h.st.s, A, [&](DenseObjWorker &W) { return W.alloc(m, K); },
        [&](hipStream_t ws, DenseObjWorker &W, int a) -> int {
          const int b = prob ? prob[a] : a;
          Rows r;
          h.rows(r);
          const int rc = W.objective(ws, h.pairs[(size_t)h.pair_of[(size_t)b]], K, ts[a], r, h.sigma,
                                     h.dY.as<double>() + (size_t)h.col[(size_t)b] * m, h.dN.as<double>(), h.tol, h.max_iter, who,
                                     &its[(size_t)a], &amll[(size_t)a]);
          if (rc == FLGP_ERR_NOCONV) { stat[(size_t)a] = rc; why[(size_t)a] = flgp_last_error(); return FLGP_OK; }
          return rc;
        });
    if (bad.item >= 0) return report(bad.item, bad.message, bad.status);
  } else {
    std::vector<int> bad_of((size_t)h.chunk), iter_of((size_t)h.chunk);
    int *hcol = (int *)(h.h_in.p + h.off_col), *hpair = (int *)(h.h_in.p + h.off_pair);
    for (int p0 = 0; p0 < A; p0 += h.chunk) {
      const int S = std::min(h.chunk, A - p0);
      for (int s = 0; s < S; ++s) {
        const int a = p0 + s, b = prob ? prob[a] : a;
        h.h_in.p[s] = ts[a];
        hcol[s] = h.col[(size_t)b];
        hpair[s] = h.pair_of[(size_t)b];
      }
      FLGP_TRY(h2d(h.in.p, h.h_in.p, sizeof(double) * (size_t)h.in_elems, h.st.s));
      std::fill(bad_of.begin(), bad_of.end(), 0);
      BatchFailure fail;
      fail.bad_of = bad_of.data(); fail.iter_of = iter_of.data();
      // (the chunk's last wait is behind everything that read h_in: the next chunk may fill it)
      FLGP_TRY(lr_batch_chunk(h.st.s, h.L, h.vals.as<double>(), h.in.as<double>(), S, h.tol, h.max_iter, p0, amll.data() + p0,
                              its.data() + p0, fail));
      for (int s = 0; s < S; ++s)
        if (bad_of[(size_t)s]) {
          stat[(size_t)(p0 + s)] = GpcNewton::pivot_error(bad_of[(size_t)s], who, iter_of[(size_t)s]);
          why[(size_t)(p0 + s)] = flgp_last_error();
        }
    }
  }
  for (int a = 0; a < A; ++a) {
    const bool ok = stat[(size_t)a] == FLGP_OK;
    values[a] = ok ? logit_objective_value(h.posterior, h.pr, ts[a], amll[(size_t)a]) : std::nan("");
    if (iters) iters[a] = its[(size_t)a];
  }
  if (status) { std::memcpy(status, stat.data(), sizeof(int) * (size_t)A); return FLGP_OK; }
  for (int a = 0; a < A; ++a)
    if (stat[(size_t)a] != FLGP_OK) return report(a, why[(size_t)a], stat[(size_t)a]);
  return FLGP_OK;
}
}  // namespace

extern "C" int flgp_logit_batch_create(const flgp_eigenpair *const *eps, const int *col, int B, int K, const int *idx, int m,
                                       const double *Y, int ncol, const double *N, double sigma, const char *approach,
                                       const double *prior, double tol, int max_iter, int max_parallel,
                                       flgp_logit_batch **out) {
  const char *who = LB_WHO;
  bool posterior = false;
  double pr[3];
  FLGP_TRY(objective_approach(who, approach, &posterior));
  FLGP_REQUIRE(eps && idx && Y && out, "%s: null pointer", who);
  *out = nullptr;
  FLGP_REQUIRE(B >= 1 && K >= 1 && m >= 1 && ncol >= 1 && max_iter >= 1, "%s: bad shape (B=%d, K=%d, m=%d, ncol=%d, max_iter=%d)",
               who, B, K, m, ncol, max_iter);
  FLGP_REQUIRE(col || ncol == B, "%s: col may be NULL only if ncol == B (ncol=%d, B=%d)", who, ncol, B);
  for (int b = 0; b < B; ++b) {
    FLGP_REQUIRE(eps[b], "problem %d: %s: null pointer", b, who);
    FLGP_REQUIRE(K <= eps[b]->K, "problem %d: %s: bad shape (K=%d of %d)", b, who, K, eps[b]->K);
    FLGP_REQUIRE(eps[b]->device == eps[0]->device, "problem %d: %s: the pair lives on device %d, problem 0's on device %d", b,
                 who, eps[b]->device, eps[0]->device);
    const int c = col ? col[b] : b;
    FLGP_REQUIRE(c >= 0 && c < ncol, "problem %d: %s: col=%d is outside [0, ncol=%d)", b, who, c, ncol);
  }
  for (int b = 0; b < B; ++b)
    for (int a = 0; a < m; ++a)
      FLGP_REQUIRE(idx[a] >= 0 && idx[a] < eps[b]->n, "problem %d: %s: idx[%d]=%d out of range", b, who, a, idx[a]);
  FLGP_TRY(objective_sigma_prior(who, sigma, prior, pr));
  for (int c = 0; c < ncol; ++c) FLGP_TRY(check_labels(Y + (size_t)c * m, N, m, who));
  int dev = 0;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == eps[0]->device, "%s: the pairs live on device %d, the current device is %d", who, eps[0]->device, dev);
  std::unique_ptr<flgp_logit_batch> H(new flgp_logit_batch);
  FLGP_TRY(lb_build(*H, eps, col, B, K, idx, m, Y, ncol, N, sigma, posterior, pr, tol, max_iter, max_parallel));
  *out = H.release();
  return FLGP_OK;
}

extern "C" int flgp_logit_batch_dims(const flgp_logit_batch *h, int *B, int *P, int *K, int *m, int *ncol, int *chunk) {
  FLGP_REQUIRE(h, "%s: null pointer", LB_WHO);
  if (B) *B = h->B;
  if (P) *P = h->P;
  if (K) *K = h->K;
  if (m) *m = h->m;
  if (ncol) *ncol = h->ncol;
  if (chunk) *chunk = h->chunk;
  return FLGP_OK;
}

extern "C" void flgp_logit_batch_free(flgp_logit_batch *h) { delete h; }

extern "C" int flgp_logit_batch_eval(flgp_logit_batch *hp, const int *prob, int A, const double *ts, double *values, int *iters,
                                     int *status) {
  const char *who = LB_WHO;
  FLGP_REQUIRE(hp && ts && values, "%s: null pointer", who);
  flgp_logit_batch &h = *hp;
  FLGP_REQUIRE(A >= 1, "%s: A=%d problems", who, A);
  FLGP_REQUIRE(prob || A == h.B, "%s: prob may be NULL only if A == B (A=%d, B=%d)", who, A, h.B);
  for (int a = 0; a < A; ++a) {
    const int b = prob ? prob[a] : a;
    FLGP_REQUIRE(b >= 0 && b < h.B, "position %d (t=%g): %s: prob=%d is outside [0, B=%d)", a, ts[a], who, b, h.B);
    FLGP_REQUIRE(std::isfinite(ts[a]), "position %d (t=%g): %s: t must be finite", a, ts[a], who);
    FLGP_REQUIRE(!h.posterior || ts[a] > 0.0, "position %d (t=%g): %s: t must be positive under \"posterior\"", a, ts[a], who);
  }
  int dev = 0;
  FLGP_HIP(hipGetDevice(&dev));
  FLGP_REQUIRE(dev == h.device, "%s: the pairs live on device %d, the current device is %d", who, h.device, dev);
  return lb_eval(h, prob, A, ts, values, iters, status);
}

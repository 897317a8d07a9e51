// The regression consumers of the device-resident EigenPair: prediction, posterior variance and the training objectives
// with their gradients (kernels in gpr.hip and gpr_grad.hip; the drivers' whole testing step
// in one call, in weight space for m > K: DESIGN 8 f-13; the objective for B (pair, x) problems through a training
// context: f-18; the trained operands of the posterior for the fitted predictor of predictor.hip: f-20).  The algebra
// prediction and variance share for m > K is written once: woodbury_step.
#include "eigenpair_internal.h"

using namespace flgp;

// ---- regression consumers of the resident pair: the Woodbury algebra stays on the device --------------
namespace {
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

// ---- regression training objectives: train_regression_gp_cpp's four objectives on the resident pair.  The
// entries and the Woodbury route (m > K) are with the training context at the end of this file -------------
namespace {
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

// ---- regression training objective for B (pair, x) problems in one call -------------------------------
// A training context: made once per grid of pairs, evaluated once per optimiser step.  What depends on (pair, rows, Y) only
// is built at create; an evaluation uploads the x of its problems and brings their values and gradients down.
// flgp_eigenpair_regression_objective is the context of one problem, made on the stack, evaluated once and gone: the library
// holds the Woodbury steps once.
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

// The Laplace approximation of the logit GP on the device-resident EigenPair, its posterior and its training objective
// (kernels in gpc.hip; the posterior's route for m > K, B problems in shared launches: DESIGN 8 f-11; the
// binary entry is its batch of one, the J one-vs-rest posteriors its batch of J: f-12; any response matrix in one call:
// f-17; the training objective for B problems in one call: f-15, and through a training context: f-19; the trained
// operands of the posterior for the fitted predictor of predictor.hip: f-20).  The Newton loops run on LrBatch
// (eigenpair_internal.h).
#include "eigenpair_internal.h"

using namespace flgp;

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

// ---- logit training objective: what train_lae_logit_gp_cpp's COBYLA minimises, on the
// resident pair, for B problems (labels, t) in one call; the single entry is the batch of one ------------------------------
namespace {
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

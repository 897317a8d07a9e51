// Polya-Gamma Gibbs prediction on the device-resident EigenPair (kernels in pg.hip; B chains in one call,
// the binary entry its batch of one and the one-vs-rest entry its batch of J: DESIGN 8 f-16; the chains' trained state
// for the fitted predictor of predictor.hip: f-22).  PgBatch takes its plans and its K x K solve from LrBatch
// (eigenpair_internal.h).
#include "eigenpair_internal.h"

using namespace flgp;

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

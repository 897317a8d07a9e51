// What more than one family of consumers of the device-resident EigenPair uses (the V products of eigenpair.hip, the
// regression consumers of eigenpair_regression.hip, the Laplace logit consumers of eigenpair_logit.hip, Polya-Gamma
// prediction of eigenpair_pg.hip): the row sets and the contractions on the pair, the column-major products, the
// regression context with its verdicts, and the host side of the training contexts.  The algebra the classifiers share is
// written once here: LrBatch (the K x K solve against B = sW C sW + I, for the Newton loop and, through PgBatch, the Gibbs
// sweep).
#pragma once
#include "common.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
#include <vector>

namespace flgp {

// X = the host's `bytes` at `host`, allocated and copied on `st`
inline int upload(DevBuf &X, const void *host, size_t bytes, hipStream_t st) {
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
inline int hk(hipStream_t st, const flgp_eigenpair *ep, int K, double t, const Rows &a, const Rows &b, double *H, double *work) {
  const double *dvec = (const double *)ep->vectors.p;
  return flgp_dev_hk(st, (const double *)ep->values.p, K, t, dvec, ep->n, a.d, a.row0, a.m, dvec, ep->n, b.d, b.row0, b.m, H,
                     a.m, work);
}
// C = C11 = HK(r, r) + sigma I (r.m x r.m), with `work` of work_bytes for it and the caller's later contractions.  A zero
// sigma launches nothing: the diagonal of HK(r, r) is a sum of squares, never -0.
inline int hk_c11(hipStream_t st, const flgp_eigenpair *ep, int K, double t, Rows &r, double sigma, DevBuf &C, DevBuf &work,
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
inline size_t vt_work_elems(int K, int q) { return (size_t)128 * K * K + (size_t)64 * K * q + 1024; }
inline int gemm_tn(hipStream_t st, int M, int N, int k, const double *A, long lda, const double *B, long ldb, double *C, double *work,
            size_t we) {
  return gemm_launch(st, M, N, k, 1.0, A, lda, 1, B, 1, ldb, 0.0, nullptr, 0, 0, C, 1, M, work, we, 0.0, nullptr);
}
inline int gemm_nn(hipStream_t st, int M, int N, int k, const double *A, long lda, const double *B, long ldb, double *C, double *work,
            size_t we) {
  return gemm_launch(st, M, N, k, 1.0, A, 1, lda, B, 1, ldb, 0.0, nullptr, 0, 0, C, 1, M, work, we, 0.0, nullptr);
}

// the two verdicts on a system matrix that did not factor, under the entry's name, and how one is returned
inline std::string not_positive_definite(const char *who) {
  return std::string(who) + ": the system matrix is not positive definite (Cholesky pivot <= 0)";
}
inline std::string not_finite(const char *who) {
  return std::string(who) + ": the objective is not finite (the system matrix is numerically singular)";
}
inline int noconv(const std::string &verdict) { set_error("%s", verdict.c_str()); return FLGP_ERR_NOCONV; }
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

inline bool all_finite(const double *v, int cnt) {
  for (int a = 0; a < cnt; ++a)
    if (!std::isfinite(v[a])) return false;
  return true;
}

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

}  // namespace flgp

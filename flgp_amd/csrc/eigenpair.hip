// Consumers of the device-resident EigenPair (include/flgp_hip.h; the pair itself is made in capi.hip), one file per
// family: the V products here, regression in eigenpair_regression.hip, the Laplace approximation of the
// logit GP in eigenpair_logit.hip, Polya-Gamma Gibbs prediction in eigenpair_pg.hip; what more than one family uses is in
// eigenpair_internal.h.  Each entry checks its arguments on the host, then runs on one stream of its own.
#include "eigenpair_internal.h"

using namespace flgp;

namespace {

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

// The predictive negative log likelihood on the device: negative_log_likelihood and nll_classification
// (reference src/Utils.cpp:302-336), the score computed from the `posterior` list of every fit_* driver.
//
// Classification.  Row i of class j with mean mu, variance v and 0/1 target y:
//   f_k = mu + sqrt(v) z_k, pi_k = 1 / (1 + exp(-f_k)) for k = 0 .. n_samples - 1,
//   like = (sum_k [pi_k y + (1 - pi_k) (1 - y)]) / n_samples,   the class's value = -mean_i log(like_i + 1e-2),
// and the J class values are added in class order from 0.0.  The reference's arithmetic is kept: sqrt of a negative
// variance gives NaN and the NaN reaches the value, exp overflow gives pi = 0, a non-binary y is used linearly.  Equal in
// law to the reference (which draws z from R's rnorm), reproducible from `seed`, not bit-identical with R.
//
// Random numbers.  The counter RNG of flgp_amd/synth.py (rng.h).  Class j uses stream stream0 + j (the host entry:
// stream0 = 0); the sample (i, k) is normal number i * n_samples + k of that stream, i.e. Box-Muller on its uniforms
// 2 (i n_samples + k) and 2 (i n_samples + k) + 1, so that synth.normal(seed, j, n_samples, offset=i * n_samples) is
// row i's sample vector.  All counters are 64-bit: 2 i n_samples passes 2^32 at sizes a user can reach.
//
// Launch shape.  One launch for all n x J (row, class) pairs, a lane per pair looping over the samples; the multinomial
// targets y = (label_i == j) are formed in the kernel.  A row's n_samples terms are added in the order k = 0, 1, .. with
// a compensated (Kahan) sum, whatever the grid, so two calls give the same bits and column j of a multinomial call is
// the binary call on that column's targets with stream0 = j.  The per-row terms -log(like + 1e-2) are reduced per class by
// flgp_dev_mean's fixed tree.
//
// Regression.  ( mean_i[ (y_i - mu_i)^2 / v_i + log(v_i + 1e-9) ] + log(2 * 3.1415926) ) / 2 -- the truncated constant is
// the reference's -- one elementwise kernel for the per-row terms, flgp_dev_mean for their mean.
#include "common.h"
#include "rng.h"
#include <cmath>

using namespace flgp;

extern "C" int flgp_dev_mean(void *stream, const double *d_x, long count, double *d_out, double *d_work);

namespace {

// like[p] (optional) and terms[p] = -log(like + 1e-2) of pair p = j n + i; mean and cov are n x J column-major
__global__ __launch_bounds__(256) void nll_class_kernel(const double *__restrict__ mean, const double *__restrict__ cov,
                                                        const double *__restrict__ target, long n, long pairs, int labels,
                                                        int n_samples, unsigned long long seed, unsigned long long stream0,
                                                        double *__restrict__ like, double *__restrict__ terms) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pairs) return;
  const long j = p / n, i = p - j * n;
  const unsigned long long base = rng_stream_base(seed, stream0 + (unsigned long long)j);
  const double mu = mean[p], sd = sqrt(cov[p]);
  const double t = target[i];
  const double y = labels ? (t == (double)j ? 1.0 : 0.0) : t;
  unsigned long long q = 2ull * (unsigned long long)i * (unsigned long long)n_samples;
  double acc = 0.0, comp = 0.0;
  for (int k = 0; k < n_samples; ++k, q += 2) {
    const double z = rng_box_muller(rng_unif(base, q), rng_unif(base, q + 1));
    const double pi = 1.0 / (1.0 + exp(-(mu + sd * z)));
    const double term = pi * y + (1.0 - pi) * (1.0 - y);
    const double a = term - comp, s = acc + a;
    comp = (s - acc) - a;
    acc = s;
  }
  const double l = acc / (double)n_samples;
  if (like) like[p] = l;
  terms[p] = -log(l + 1e-2);
}

__global__ void nll_reg_kernel(const double *__restrict__ mean, const double *__restrict__ cov,
                               const double *__restrict__ target, long n, double *__restrict__ like,
                               double *__restrict__ terms) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double d = target[i] - mean[i], v = cov[i];
  const double term = d * d / v + log(v + 1e-9);
  if (like) like[i] = term;
  terms[i] = term;
}

// classification: out = the J class values added in class order from 0.0; regression: out = (vals[0] + log(2 * 3.1415926)) / 2
__global__ void nll_finish_kernel(const double *__restrict__ vals, int J, int regression, double *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (regression) { out[0] = (vals[0] + log(2 * 3.1415926)) / 2; return; }
  double acc = 0.0;
  for (int j = 0; j < J; ++j) acc += vals[j];
  out[0] = acc;
}

inline long nll_parts(long n) { return (n + 4095) / 4096; }

// the means of the J columns of terms (d_work) into vals, each by flgp_dev_mean on its own slab partials, then the finish
int nll_reduce(hipStream_t st, long n, int J, int regression, double *d_work, double *d_nll) {
  double *terms = d_work, *parts = d_work + n * J, *vals = parts + nll_parts(n) * J;
  for (int j = 0; j < J; ++j) FLGP_TRY(flgp_dev_mean(st, terms + (long)j * n, n, vals + j, parts + (long)j * nll_parts(n)));
  hipLaunchKernelGGL(nll_finish_kernel, dim3(1), dim3(64), 0, st, vals, J, regression, d_nll);
  return check_launch("nll_finish_kernel");
}

}  // namespace

int flgp::check_class_labels(const char *who, const char *name, const double *v, long n, int J, bool all_named) {
  double top = -1.0;
  for (long i = 0; i < n; ++i) {
    FLGP_REQUIRE(v[i] >= 0.0 && v[i] < J && v[i] == std::floor(v[i]), "%s: %s[%ld]=%g is not a class label in 0 .. %d", who, name, i,
                 v[i], J - 1);
    if (v[i] > top) top = v[i];
  }
  // the reference takes J from the labels: a posterior with another column count would be read out of bounds there
  if (all_named)
    FLGP_REQUIRE((int)top + 1 == J, "%s: the labels name %d classes, mean and cov have J=%d columns", who, (int)top + 1, J);
  return FLGP_OK;
}

extern "C" size_t flgp_dev_nll_workspace(long n, int J) {
  if (n < 1 || J < 1) return 0;
  return sizeof(double) * (size_t)J * ((size_t)n + (size_t)nll_parts(n) + 1);
}

extern "C" int flgp_dev_nll_classification(void *stream, const double *d_mean, const double *d_cov, const double *d_target,
                                           long n, int J, int labels, int n_samples, unsigned long long seed,
                                           unsigned long long stream0, double *d_like, double *d_nll, double *d_work) {
  const char *who = "nll_classification";
  FLGP_REQUIRE(d_mean && d_cov && d_target && d_nll && d_work, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1 && J >= 1 && n <= (long)0x7FFFFFFF * 256 / J, "%s: bad shape (n=%ld, J=%d)", who, n, J);
  FLGP_REQUIRE(n_samples >= 1, "%s: n_samples=%d must be at least 1", who, n_samples);
  hipStream_t st = (hipStream_t)stream;
  const long pairs = n * J;
  // few pairs: wave-sized workgroups, so that they spread over the compute units; the bits do not depend on it
  const int block = pairs <= 65536 ? 64 : 256;
  {
    ProfScope ps("nll_class_kernel", st, (double)pairs * n_samples);
    hipLaunchKernelGGL(nll_class_kernel, dim3(ceil_div(pairs, block)), dim3(block), 0, st, d_mean, d_cov, d_target, n, pairs,
                       labels, n_samples, seed, stream0, d_like, d_work);
    FLGP_TRY(check_launch("nll_class_kernel"));
  }
  return nll_reduce(st, n, J, 0, d_work, d_nll);
}

extern "C" int flgp_dev_nll_regression(void *stream, const double *d_mean, const double *d_cov, const double *d_target, long n,
                                       double *d_like, double *d_nll, double *d_work) {
  const char *who = "nll_regression";
  FLGP_REQUIRE(d_mean && d_cov && d_target && d_nll && d_work, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1 && n <= (long)0x7FFFFFFF * 256, "%s: bad shape (n=%ld)", who, n);
  hipStream_t st = (hipStream_t)stream;
  {
    ProfScope ps("nll_reg_kernel", st, (double)n);
    hipLaunchKernelGGL(nll_reg_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_mean, d_cov, d_target, n, d_like, d_work);
    FLGP_TRY(check_launch("nll_reg_kernel"));
  }
  return nll_reduce(st, n, 1, 1, d_work, d_nll);
}

extern "C" int flgp_negative_log_likelihood(const double *mean, const double *cov, const double *target, long n, int J,
                                            const char *type, int n_samples, unsigned long long seed, double *nll,
                                            double *like) {
  const char *who = "negative_log_likelihood";
  FLGP_REQUIRE(mean && cov && target && nll && type, "%s: null pointer", who);
  const bool reg = !strcmp(type, "regression"), bin = !strcmp(type, "binary"), mul = !strcmp(type, "multinomial");
  FLGP_REQUIRE(reg || bin || mul, "The type of likelihood is not supported!");
  FLGP_REQUIRE(n >= 1 && J >= 1 && n <= (long)0x7FFFFFFF * 256 / J, "%s: bad shape (n=%ld, J=%d)", who, n, J);
  FLGP_REQUIRE(mul || J == 1, "%s: type \"%s\" takes one column (J=%d)", who, type, J);
  if (!reg) FLGP_REQUIRE(n_samples >= 1, "%s: n_samples=%d must be at least 1", who, n_samples);
  if (mul) FLGP_TRY(check_class_labels(who, "target", target, n, J, true));
  Stream st;
  FLGP_TRY(st.create());
  const size_t nj = sizeof(double) * (size_t)n * J;
  DevBuf dmean, dcov, dtarget, dlike, dnll, work;
  FLGP_TRY(dmean.alloc(nj)); FLGP_TRY(dcov.alloc(nj)); FLGP_TRY(dtarget.alloc(sizeof(double) * (size_t)n));
  FLGP_TRY(dnll.alloc(sizeof(double))); FLGP_TRY(work.alloc(flgp_dev_nll_workspace(n, J)));
  if (like) FLGP_TRY(dlike.alloc(nj));
  FLGP_TRY(h2d(dmean.p, mean, nj, st.s));
  FLGP_TRY(h2d(dcov.p, cov, nj, st.s));
  FLGP_TRY(h2d(dtarget.p, target, sizeof(double) * (size_t)n, st.s));
  if (reg)
    FLGP_TRY(flgp_dev_nll_regression(st.s, dmean.as<double>(), dcov.as<double>(), dtarget.as<double>(), n, dlike.as<double>(),
                                     dnll.as<double>(), work.as<double>()));
  else
    FLGP_TRY(flgp_dev_nll_classification(st.s, dmean.as<double>(), dcov.as<double>(), dtarget.as<double>(), n, J, mul ? 1 : 0,
                                         n_samples, seed, 0, dlike.as<double>(), dnll.as<double>(), work.as<double>()));
  if (like) FLGP_TRY(d2h(like, dlike.p, nj, st.s));
  FLGP_TRY(d2h(nll, dnll.p, sizeof(double), st.s));
  FLGP_HIP(hipStreamSynchronize(st.s));
  return FLGP_OK;
}

// The Polya-Gamma Gibbs sampler of the logit GP on the device: test_pgbinary_cpp (reference
// src/Predict.cpp:11-26, src/PGLogitModel.cpp) and predict_logit_mult_gp_cpp (src/MultiClassification.cpp:57-88).
//
// PG(1, c) draws: Devroye's alternating-series method as Polson, Scott & Windle (JASA 2013, section 4) adapt it, one lane
// per entry.  X ~ J*(1, z) with z = |c| / 2 and truncation point t = 0.64, returned as X / 4; PG(b, c) for an integer b is
// the sum of b such draws, in order.
//
// Random numbers.  The construction of flgp_amd/synth.py, unchanged (rng.h, shared with nll.hip), so that numpy can
// regenerate every number the device consumes: stream st under seed has the base splitmix64(seed * 0x100000001B3 + st);
// its counter q gives the uniform ((splitmix64(base + q) >> 11) + 0.5) 2^-53; normal i of a stream is Box-Muller on the
// uniforms 2i, 2i + 1, sqrt(-2 log u_2i) cos(2 pi u_2i+1); an exponential is -log u.  Nothing depends on the launch
// geometry.
//
// Layout of one chain under its own seed (flgp_pg_logit_predict's, and every chain of flgp_eigenpair_pg_predict_batch:
// flgp_eigenpair_pg_predict is its batch of one, flgp_eigenpair_pg_predict_multiclass its batch of J with seed + j),
// sweep s = 0 .. n_sample - 1:
//   stream 4s     normal k (k < K): z1 of f0 = V1 L^1/2 z1 + sqrt(sigma) z2 (unused by the dense entry);
//   stream 4s + 1 normal a (a < m): z2 (the dense entry: f0 = L_C z2);
//   stream 4s + 2 normal a: z3 of r = kappa / sqrt(omega) - sqrt(omega) f0 - z3;
//   stream 4s + 3 counter a 2^32 + q: the q-th uniform of the PG draw of entry a.
// flgp_pg_draw uses stream 3, the layout of a chain's first omega draw.
//
// The uniforms of one PG(1, z) draw, in the order they are consumed (repeated per trial until acceptance):
//   u                       right proposal (X = t + E / K) when u < p / (p + q);
//   right:    u             E = -log u;
//   left, mu = 1/z > t:     repeat (u, u') E1 = -log u, E2 = -log u' until E1^2 <= 2 E2 / t; X = t / (1 + t E1)^2;
//                           then u'' -- accept the proposal when u'' <= exp(-z^2 X / 2), else draw E1, E2 again;
//   left, mu <= t:          repeat (u, u') the normal sqrt(-2 log u) cos(2 pi u'), y = normal^2, a = mu y,
//                           X = mu / (1 + a/2 + sqrt(a^2 + 4a)/2) (the Michael-Schucany-Haas root, in a form without
//                           cancellation), then u'' -- X = mu^2 / X when u'' > mu / (mu + X) -- until X < t;
//   u                       the series: S = a_0(X), Y = u S, then n = 1, 2, ..: odd n S -= a_n, accept if Y <= S;
//                           even n S += a_n, reject (next trial) if Y > S.
// The counter runs on over the b draws of one entry.  A draw that has not finished after 2^16 loop steps (only with a
// non-finite argument) returns NaN, so a diverging chain cannot hang the device; the pivot flag of the next
// factorisation reports it.
#include "common.h"
#include "rng.h"

namespace flgp {

namespace {
constexpr double PG_T = 0.64;

// log Phi(x), without the underflow of Phi for x << 0
__device__ __forceinline__ double pg_log_phi(double x) {
  if (x < 0.0) return log(0.5 * erfcx(-x * M_SQRT1_2)) - 0.5 * x * x;
  return log(0.5 * erfc(-x * M_SQRT1_2));
}

__device__ __forceinline__ double pg_a(int n, double x) {
  const double k = n + 0.5;
  if (x <= PG_T) return M_PI * k * pow(2.0 / (M_PI * x), 1.5) * exp(-2.0 * k * k / x);
  return M_PI * k * exp(-0.5 * k * k * M_PI * M_PI * x);
}

struct PgCtr {
  unsigned long long base, q;
  __device__ double next() { return rng_unif(base, q++); }
};

// X ~ J*(1, z), z >= 0
__device__ double jstar_draw(double z, PgCtr &r) {
  if (!(z < HUGE_VAL)) return __builtin_nan("");
  const double t = PG_T, st = sqrt(t);
  const double K = M_PI * M_PI / 8.0 + 0.5 * z * z;
  const double lp = log(M_PI / (2.0 * K)) - K * t;
  const double l1 = -z + pg_log_phi((t * z - 1.0) / st), l2 = z + pg_log_phi(-(t * z + 1.0) / st);
  const double lq = M_LN2 + fmax(l1, l2) + log1p(exp(-fabs(l1 - l2)));
  const double p_right = 1.0 / (1.0 + exp(lq - lp));
  const double mu = 1.0 / z;             // +inf at z = 0
  int guard = 1 << 16;
  for (;;) {
    double X;
    if (r.next() < p_right) {
      X = t + (-log(r.next())) / K;
    } else if (mu > t) {
      for (;;) {
        double E1, E2;
        do {
          E1 = -log(r.next());
          E2 = -log(r.next());
          if (--guard <= 0) return __builtin_nan("");
        } while (E1 * E1 > 2.0 * E2 / t);
        const double d = 1.0 + t * E1;
        X = t / (d * d);
        if (r.next() <= exp(-0.5 * z * z * X)) break;
      }
    } else {
      do {
        const double u1 = r.next(), u2 = r.next();
        const double nr = rng_box_muller(u1, u2);
        const double a = mu * (nr * nr);
        X = mu / (1.0 + 0.5 * a + 0.5 * sqrt(a * a + 4.0 * a));
        if (r.next() > mu / (mu + X)) X = mu * mu / X;
        if (--guard <= 0) return __builtin_nan("");
      } while (X >= t);
    }
    double S = pg_a(0, X);
    const double Y = r.next() * S;
    for (int n = 1;; ++n) {
      if (--guard <= 0) return __builtin_nan("");
      const double an = pg_a(n, X);
      if (n & 1) {
        S -= an;
        if (Y <= S) return X;
      } else {
        S += an;
        if (Y > S) break;
      }
    }
  }
}
}  // namespace

unsigned long long pg_stream_base(unsigned long long seed, unsigned long long stream) {
  return rng_stream_base(seed, stream);
}

// out[i] = PG(b_i, c_i) (b == nullptr: b_i = 1) on the stream with base `base`, entry i at counter i 2^32
__global__ void pg_draw_kernel(const double *__restrict__ b, const double *__restrict__ c, long n, unsigned long long base,
                               double *__restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PgCtr r{base, (unsigned long long)i << 32};
  const double z = 0.5 * fabs(c[i]);
  const int nb = b ? (int)b[i] : 1;
  double s = 0.0;
  for (int d = 0; d < nb; ++d) s += 0.25 * jstar_draw(z, r);
  out[i] = s;
}

int pg_draw_launch(hipStream_t st, const double *d_b, const double *d_c, long n, unsigned long long base, double *d_out) {
  if (n <= 0) return FLGP_OK;
  hipLaunchKernelGGL(pg_draw_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_b, d_c, n, base, d_out);
  return check_launch("pg_draw_kernel");
}

// the normals of one sweep: out[0:K] from stream 4s, out[K:K+m] from 4s + 1, out[K+m:K+2m] from 4s + 2
__global__ void pg_normals_kernel(unsigned long long b0, unsigned long long b1, unsigned long long b2, int K, int m,
                                  double *__restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= K + 2 * m) return;
  unsigned long long base;
  int i;
  if (e < K) { base = b0; i = e; }
  else if (e < K + m) { base = b1; i = e - K; }
  else { base = b2; i = e - K - m; }
  const unsigned long long q = 2ull * (unsigned long long)i;
  out[e] = rng_box_muller(rng_unif(base, q), rng_unif(base, q + 1));
}

int pg_normals(hipStream_t st, unsigned long long seed, int sweep, int K, int m, double *d_out) {
  const unsigned long long s4 = 4ull * (unsigned long long)sweep;
  hipLaunchKernelGGL(pg_normals_kernel, dim3(ceil_div(K + 2 * m, 256)), dim3(256), 0, st, pg_stream_base(seed, s4),
                     pg_stream_base(seed, s4 + 1), pg_stream_base(seed, s4 + 2), K, m, d_out);
  return check_launch("pg_normals_kernel");
}

// f0 = Vz + ss z2; r = kappa / sqrt(omega) - sqrt(omega) f0 - z3; sw = sqrt(omega)
__global__ void pg_f0r_kernel(int m, const double *__restrict__ Vz, const double *__restrict__ z2, double ss,
                              const double *__restrict__ z3, const double *__restrict__ kappa, const double *__restrict__ omega,
                              double *__restrict__ f0, double *__restrict__ r, double *__restrict__ sw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double f = Vz[i] + ss * z2[i];
  const double s = sqrt(omega[i]);
  f0[i] = f;
  r[i] = kappa[i] / s - s * f - z3[i];
  sw[i] = s;
}

int pg_f0r(hipStream_t st, int m, const double *Vz, const double *z2, double ss, const double *z3, const double *kappa,
           const double *omega, double *f0, double *r, double *sw) {
  hipLaunchKernelGGL(pg_f0r_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, m, Vz, z2, ss, z3, kappa, omega, f0, r, sw);
  return check_launch("pg_f0r_kernel");
}

// sw = sqrt(omega), dh = 1 / sqrt(1 + sigma omega), a = sw dh    (the Woodbury form of B = D + U L U^T)
__global__ void pg_dvec_kernel(int m, const double *__restrict__ omega, double sigma, double *__restrict__ sw,
                               double *__restrict__ dh, double *__restrict__ a) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double w = omega[i];
  const double s = sqrt(w), d = 1.0 / sqrt(1.0 + sigma * w);
  sw[i] = s; dh[i] = d; a[i] = s * d;
}

int pg_dvec(hipStream_t st, int m, const double *omega, double sigma, double *sw, double *dh, double *a) {
  hipLaunchKernelGGL(pg_dvec_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, m, omega, sigma, sw, dh, a);
  return check_launch("pg_dvec_kernel");
}

// out = a .* x (.* b when b is given)
__global__ void pg_mul_kernel(int m, const double *__restrict__ a, const double *__restrict__ x, const double *__restrict__ b,
                              double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double v = a[i] * x[i];
  out[i] = b ? v * b[i] : v;
}

int pg_mul(hipStream_t st, int m, const double *a, const double *x, const double *b, double *out) {
  hipLaunchKernelGGL(pg_mul_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, m, a, x, b, out);
  return check_launch("pg_mul_kernel");
}

// out = x + y + c z   (x, y, z each optional: a missing term is left out, not added as 0)
__global__ void pg_axpy3_kernel(int m, const double *__restrict__ x, const double *__restrict__ y, double c,
                                const double *__restrict__ z, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double v = x ? x[i] : 0.0;
  if (y) v = x ? v + y[i] : y[i];
  if (z) v = (x || y) ? v + c * z[i] : c * z[i];
  out[i] = v;
}

int pg_axpy3(hipStream_t st, int m, const double *x, const double *y, double c, const double *z, double *out) {
  hipLaunchKernelGGL(pg_axpy3_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, m, x, y, c, z, out);
  return check_launch("pg_axpy3_kernel");
}

// y = L z for the lower factor chol_blocked left in L (its upper triangle is not read); a thread per row
__global__ void pg_trmv_kernel(const double *__restrict__ L, long lda, int m, const double *__restrict__ z,
                               double *__restrict__ y, const int *__restrict__ flag) {
  if (flag[0]) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  double acc = 0.0;
  for (int j = 0; j <= i; ++j) acc += L[(size_t)j * lda + i] * z[j];
  y[i] = acc;
}

int pg_trmv(hipStream_t st, const double *dL, long lda, int m, const double *z, double *y, const int *d_flag) {
  hipLaunchKernelGGL(pg_trmv_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, dL, lda, m, z, y, d_flag);
  return check_launch("pg_trmv_kernel");
}

// pi_i = logistic(mean_i + sigma_nv sum_{p in [ptr_i, ptr_i+1)} w[list_p]) (no ptr: mean_i alone), y_i = (pi_i > 0.5);
// either output may be nullptr.  pi is written to pi[i * ld].
__global__ void pg_pi_kernel(long n, const double *__restrict__ mean, double sigma_nv, const long *__restrict__ ptr,
                             const int *__restrict__ list, const double *__restrict__ w, double *__restrict__ pi, long ld,
                             double *__restrict__ y) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double f = mean[i];
  if (ptr) {
    double acc = 0.0;
    for (long p = ptr[i]; p < ptr[i + 1]; ++p) acc += w[list[p]];
    f = f + sigma_nv * acc;
  }
  const double v = 1.0 / (1.0 + exp(-f));
  if (pi) pi[i * ld] = v;
  if (y) y[i] = v > 0.5 ? 1.0 : 0.0;
}

int pg_pi(hipStream_t st, long n, const double *mean, double sigma_nv, const long *ptr, const int *list, const double *w,
          double *pi, long ld, double *y) {
  if (n <= 0) return FLGP_OK;
  hipLaunchKernelGGL(pg_pi_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, n, mean, sigma_nv, ptr, list, w, pi, ld, y);
  return check_launch("pg_pi_kernel");
}

// labels_i = the first j with probs(i, j) maximal (Eigen's maxCoeff), probs n x J column-major
__global__ void pg_argmax_kernel(long n, int J, const double *__restrict__ probs, double *__restrict__ labels) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double best = probs[i];
  int loc = 0;
  for (int j = 1; j < J; ++j) {
    const double v = probs[(size_t)j * n + i];
    if (v > best) { best = v; loc = j; }
  }
  labels[i] = (double)loc;
}

int pg_argmax(hipStream_t st, long n, int J, const double *probs, double *labels) {
  if (n <= 0) return FLGP_OK;
  hipLaunchKernelGGL(pg_argmax_kernel, dim3(ceil_div(n, 256)), dim3(256), 0, st, n, J, probs, labels);
  return check_launch("pg_argmax_kernel");
}

// kappa = Y - 1/2, omega = 1, f = 0
__global__ void pg_init_kernel(int m, const double *__restrict__ Y, double *__restrict__ kappa, double *__restrict__ omega,
                               double *__restrict__ f) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  kappa[i] = Y[i] - 0.5;
  omega[i] = 1.0;
  f[i] = 0.0;
}

int pg_init(hipStream_t st, int m, const double *Y, double *kappa, double *omega, double *f) {
  hipLaunchKernelGGL(pg_init_kernel, dim3(ceil_div(m, 256)), dim3(256), 0, st, m, Y, kappa, omega, f);
  return check_launch("pg_init_kernel");
}

// ---- the Woodbury sweep for a chunk of chains (PgChunk, common.h; the sweep is in eigenpair_pg.hip) -------
// The kernels above with the chain's slot in blockIdx.y.  A thread reads and writes its own slot only, every expression is
// its namesake's and every random number is a function of (seed[slot], sweep, stream, entry, draw), so a chain's bits are
// those of the single entry whatever shares its chunk.

__global__ void pgb_init_kernel(PgChunk c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long s = blockIdx.y, o = s * c.sv + i;
  c.kappa[o] = c.Y[(size_t)c.ycol[s] * c.ldy + i] - 0.5;
  c.omega[o] = 1.0;
  c.f[o] = 0.0;
}

__global__ void pgb_normals_kernel(PgChunk c, unsigned long long s4) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int K = c.K, m = c.m;
  if (e >= K + 2 * m) return;
  const long s = blockIdx.y;
  const unsigned long long seed = c.seed[s];
  unsigned long long base;
  int i;
  if (e < K) { base = rng_stream_base(seed, s4); i = e; }
  else if (e < K + m) { base = rng_stream_base(seed, s4 + 1); i = e - K; }
  else { base = rng_stream_base(seed, s4 + 2); i = e - K - m; }
  const unsigned long long q = 2ull * (unsigned long long)i;
  c.z[s * c.sz + e] = rng_box_muller(rng_unif(base, q), rng_unif(base, q + 1));
}

__global__ void pgb_f0r_kernel(PgChunk c, double ss) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long sl = blockIdx.y, o = sl * c.sv + i;
  const double *z2 = c.z + sl * c.sz + c.K, *z3 = z2 + c.m;
  const double f = c.t2[o] + ss * z2[i];
  const double s = sqrt(c.omega[o]);
  c.f0[o] = f;
  c.r[o] = c.kappa[o] / s - s * f - z3[i];
  c.sw[o] = s;
}

__global__ void pgb_dvec_kernel(PgChunk c) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long o = (long)blockIdx.y * c.sv + i;
  const double w = c.omega[o];
  const double s = sqrt(w), d = 1.0 / sqrt(1.0 + c.sigma * w);
  c.sw[o] = s; c.dh[o] = d; c.a[o] = s * d;
}

__global__ void pgb_wb_out_kernel(PgChunk c, double *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long o = (long)blockIdx.y * c.sv + i;
  out[o] = c.sw[o] * (c.dh[o] * (c.t1[o] - c.t2[o]));
}

// (out may be x: an element is read before it is written, by its own thread)
__global__ void pgb_axpy3_kernel(int m, long sv, const double *x, const double *y, double c, const double *z, double *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const long o = (long)blockIdx.y * sv + i;
  double v = x ? x[o] : 0.0;
  if (y) v = x ? v + y[o] : y[o];
  if (z) v = (x || y) ? v + c * z[o] : c * z[o];
  out[o] = v;
}

__global__ void pgb_draw_kernel(PgChunk c, unsigned long long stream) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c.m) return;
  const long sl = blockIdx.y, o = sl * c.sv + i;
  PgCtr r{rng_stream_base(c.seed[sl], stream), (unsigned long long)i << 32};
  const double z = 0.5 * fabs(c.f[o]);
  double s = 0.0;
  s += 0.25 * jstar_draw(z, r);
  c.omega[o] = s;
}

__global__ void pgb_pi_kernel(long n, const double *__restrict__ mean, long smean, double sigma_nv, const long *__restrict__ ptr,
                              const int *__restrict__ list, const double *__restrict__ w, long sw, double *__restrict__ pi,
                              double *__restrict__ y, long ldo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long s = blockIdx.y;
  double f = mean[s * smean + i];
  if (ptr) {
    const double *ws = w + s * sw;
    double acc = 0.0;
    for (long p = ptr[i]; p < ptr[i + 1]; ++p) acc += ws[list[p]];
    f = f + sigma_nv * acc;
  }
  const double v = 1.0 / (1.0 + exp(-f));
  pi[s * ldo + i] = v;
  if (y) y[s * ldo + i] = v > 0.5 ? 1.0 : 0.0;
}

int pgb_init(hipStream_t st, const PgChunk &c) {
  hipLaunchKernelGGL(pgb_init_kernel, dim3(ceil_div(c.m, 256), c.slots), dim3(256), 0, st, c);
  return check_launch("pgb_init_kernel");
}
int pgb_normals(hipStream_t st, const PgChunk &c, int sweep) {
  hipLaunchKernelGGL(pgb_normals_kernel, dim3(ceil_div(c.K + 2 * c.m, 256), c.slots), dim3(256), 0, st, c,
                     4ull * (unsigned long long)sweep);
  return check_launch("pgb_normals_kernel");
}
int pgb_f0r(hipStream_t st, const PgChunk &c, double ss) {
  hipLaunchKernelGGL(pgb_f0r_kernel, dim3(ceil_div(c.m, 256), c.slots), dim3(256), 0, st, c, ss);
  return check_launch("pgb_f0r_kernel");
}
int pgb_dvec(hipStream_t st, const PgChunk &c) {
  hipLaunchKernelGGL(pgb_dvec_kernel, dim3(ceil_div(c.m, 256), c.slots), dim3(256), 0, st, c);
  return check_launch("pgb_dvec_kernel");
}
int pgb_wb_out(hipStream_t st, const PgChunk &c, double *out) {
  hipLaunchKernelGGL(pgb_wb_out_kernel, dim3(ceil_div(c.m, 256), c.slots), dim3(256), 0, st, c, out);
  return check_launch("pgb_wb_out_kernel");
}
int pgb_axpy3(hipStream_t st, const PgChunk &c, const double *x, const double *y, double cz, const double *z, double *out) {
  hipLaunchKernelGGL(pgb_axpy3_kernel, dim3(ceil_div(c.m, 256), c.slots), dim3(256), 0, st, c.m, c.sv, x, y, cz, z, out);
  return check_launch("pgb_axpy3_kernel");
}
int pgb_draw(hipStream_t st, const PgChunk &c, int sweep) {
  hipLaunchKernelGGL(pgb_draw_kernel, dim3(ceil_div(c.m, 256), c.slots), dim3(256), 0, st, c,
                     4ull * (unsigned long long)sweep + 3);
  return check_launch("pgb_draw_kernel");
}
int pgb_pi(hipStream_t st, long n, int slots, const double *mean, long smean, double sigma_nv, const long *ptr, const int *list,
           const double *w, long sw, double *pi, double *y, long ldo) {
  if (n <= 0 || slots <= 0) return FLGP_OK;
  hipLaunchKernelGGL(pgb_pi_kernel, dim3(ceil_div(n, 256), slots), dim3(256), 0, st, n, mean, smean, sigma_nv, ptr, list, w, sw,
                     pi, y, ldo);
  return check_launch("pgb_pi_kernel");
}

}  // namespace flgp

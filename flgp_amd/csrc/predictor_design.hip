// Greedy maximum-variance design on a regression handle's feature columns (include/flgp_hip.h): which B of n
// candidate rows to label next.  With z_i = a_i P_K the row kernels' chain on a row's r scaled anchor weights and d = noise +
// sigma the observation variance of a new label, step t picks the untaken row j_t of largest score (the latent posterior
// variance given the picks so far; at equal scores the lowest index; a NaN is never larger), and conditions on it:
//   z = z_(j_t),  b_tau = u_tau . z (tau < t),  v = z - sum_tau u_tau b_tau,  u_t = v / sqrt(gain_t + d),
//   p = P_K u_t (s values),  c_i = a_i p = z_i . u_t,  score_i <- score_i - c_i c_i   for every row i.
// No n x K array and no K x K solve exist: a step is one s x K matrix-vector product, r gathers from an s-vector and one
// multiply-subtract per candidate.  All B steps are enqueued without a host wait: three launches per step (pick, project,
// downdate).  Every sum has one order that depends on the shapes alone -- not on the grid, not on the knob
// predictor_design_grid -- and every operation is one rounded IEEE operation (-ffp-contract=off):
//   score0_i  predictor_rows_kernel's `sq` (flgp_dev_predictor_rows with cg = 0.0 and no mean: lane l adds the squares of
//             k = l, l + 64, .. ascending from 0.0, then six butterfly steps o = 32 .. 1);
//   z[k]      a ascending, multiply then add, from 0.0 (predictor_cols_kernel's chain);
//   b_tau     k ascending, multiply then add, from 0.0;
//   v[k]      z[k] - acc, acc = the chain tau ascending of u_tau[k] b_tau, multiply then add, from 0.0;
//   u_t[k]    v[k] / sqrt(gain_t + d): one addition, one square root, one division per element;
//   p[j]      lane l adds P(j, k) u_t[k] for k = l, l + 64, .. ascending from 0.0 (multiply then add), then six butterfly steps
//             S_l <- S_l + S_(l xor o), o = 32, 16, 8, 4, 2, 1 (predictor_rows_kernel's order, with products for squares);
//   c_i       a ascending, multiply then add, from 0.0; score_i - c_i c_i is one multiplication and one subtraction, unclamped.
// The argmax is a reduction under a total order -- the larger score, a NaN below every number, at equal scores (or two NaNs) the
// lower index -- so its result does not depend on how the candidates are split over lanes, waves, workgroups and partials.
// predictor.hip holds the handle entries (flgp_predictor_design / flgp_dev_predictor_design), predictor_rows.hip the
// predictor_rows_kernel named above.
#include "common.h"
#include <algorithm>
#include <cmath>

using namespace flgp;

namespace flgp {

constexpr int PD_ROWS = 256;                    // the rows of one range of the downdate kernel: a lane per row, four waves
constexpr int PD_MAX_GRID = 1024;               // the most workgroups (= partials) of the downdate kernel
constexpr int PD_PICK_THREADS = 1024;
constexpr int PD_LDS_S = 20480;                 // p sits in LDS up to this s: 163840 bytes, U-recovery's rule (sparse.hip)
constexpr int PD_NONE = 0x7fffffff;             // the index of "no candidate"
constexpr int PD_REDUCE_BYTES = (PD_ROWS / 64) * (int)(sizeof(double) + sizeof(int));

// (v, i) is a better candidate than (bv, bi): a total order, so every reduction tree gives the same answer
__device__ __forceinline__ bool pd_better(double v, int i, double bv, int bi) {
  if (i == PD_NONE) return false;
  if (bi == PD_NONE) return true;
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return bn;                      // a NaN is never larger
  if (!vn && v != bv) return v > bv;
  return i < bi;
}

__device__ __forceinline__ void pd_wave_best(double &bv, int &bi) {
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (pd_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
  }
}

// acc = 0.0; acc = acc + x(i) y(i), i ascending: the chain of every sum of the pick kernel, with the loads of NB terms issued
// before the first is used -- a term at a time the chain waited for one L2 round trip after the other (184 us per step at
// t ~ 500, K = 200).  cnt is the same in every lane; a load past the end repeats the last term's and is not added.
template <int NB, class FX, class FY>
__device__ __forceinline__ double pd_chain(int cnt, FX x, FY y) {
  double acc = 0.0;
  for (int i0 = 0; i0 < cnt; i0 += NB) {
    double xv[NB], yv[NB];
#pragma unroll
    for (int e = 0; e < NB; ++e) {
      const int i = i0 + e < cnt ? i0 + e : cnt - 1;
      xv[e] = x(i); yv[e] = y(i);
    }
#pragma unroll
    for (int e = 0; e < NB; ++e)
      if (i0 + e < cnt) acc = acc + xv[e] * yv[e];
  }
  return acc;
}

// the pool's rows a-major: idxT[a n + i], valT[a n + i].  The downdate kernel reads them B times with lane = row: a wave's
// load is 256 (indices) or 512 (values) consecutive bytes, where the row-major arrays give a stride of 4 r and 8 r bytes.
// The values and their order are the rows'.  Entry (i, a) sits at a sa + i si: (n, 1) packed, (1, r) in the caller's row-major
// arrays, which the kernels read in place when the knob predictor_design_pack is 0 (the measurement of DESIGN f-25).
__global__ __launch_bounds__(256) void design_pack_kernel(const int *__restrict__ ell_idx, const double *__restrict__ ell_val, long n,
                                                          int r, int *__restrict__ idxT, double *__restrict__ valT) {
  const long total = n * r;
  for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long)gridDim.x * 256) {
    const long a = e / n, i = e - a * n;
    idxT[e] = ell_idx[i * r + a];
    valT[e] = ell_val[i * r + a];
  }
}

// Step 5 for every row, and the (largest untaken score, lowest index) of the workgroup's rows.  Lane = row; workgroup w walks the
// ranges w, w + grid, .. of PD_ROWS rows.  p == nullptr: no downdate, the partials alone (before the first pick).  LDS: p is
// copied to LDS once per workgroup and gathered from there (8-byte reads at random anchors: conflicts are the data's, there is
// no layout to choose); otherwise it is gathered from global memory.
template <bool LDS>
__global__ __launch_bounds__(PD_ROWS) void design_downdate_kernel(const int *__restrict__ idxT, const double *__restrict__ valT, long n,
                                                                  long sa, long si, int r, int s, const double *__restrict__ p,
                                                                  double *__restrict__ score, const unsigned char *__restrict__ taken,
                                                                  double *__restrict__ part_val, int *__restrict__ part_idx) {
  // dynamic LDS alone: at s = 20480 p takes all 163840 bytes a workgroup may have, and the four (value, index) pairs of the
  // waves reuse its first 48 bytes once the rows are done (PD_REDUCE_BYTES where p is not staged)
  extern __shared__ __attribute__((aligned(16))) double pd_p[];
  const int tid = threadIdx.x;
  if (LDS && p) {
    for (int j = tid; j < s; j += PD_ROWS) pd_p[j] = p[j];
    __syncthreads();
  }
  double bv = 0.0;
  int bi = PD_NONE;
  for (long base = (long)blockIdx.x * PD_ROWS; base < n; base += (long)gridDim.x * PD_ROWS) {
    const long i = base + tid;
    if (i < n) {
      double sc = score[i];
      if (p) {
        double c = 0.0;
        for (int a = 0; a < r; ++a) {
          const int j = idxT[a * sa + i * si];
          const double pj = LDS ? pd_p[j] : p[j];
          c = c + valT[a * sa + i * si] * pj;
        }
        sc = sc - c * c;
        score[i] = sc;
      }
      if (!taken[i] && pd_better(sc, (int)i, bv, bi)) { bv = sc; bi = (int)i; }
    }
  }
  pd_wave_best(bv, bi);
  double *wv = pd_p;
  int *wi = (int *)(pd_p + PD_ROWS / 64);
  __syncthreads();                              // every gather from p is done
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < PD_ROWS / 64; ++w)
      if (pd_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
    part_val[blockIdx.x] = bv;
    part_idx[blockIdx.x] = bi;
  }
}

// One workgroup: steps 1 to 3.  It reduces the partials to j_t, writes picks[t] and gain[t] and marks the row; thread k builds
// z[k] from the row's r rows of P_K; thread tau builds b_tau from the k-major copy Ut (ld B: consecutive tau are consecutive
// doubles); thread k builds v[k] and u_t[k] from the tau-major copy U (ld K) and stores u_t in both copies and in `u` for the
// projection.  z and b live in the workspace: what one thread wrote is read by others after a workgroup barrier.
__global__ __launch_bounds__(PD_PICK_THREADS) void design_pick_kernel(const double *__restrict__ part_val, const int *__restrict__ part_idx,
                                                                      int nparts, const int *__restrict__ idxT,
                                                                      const double *__restrict__ valT, long sa, long si, int r,
                                                                      const double *__restrict__ P, long ldp, int K, double d, int t,
                                                                      int B, int *__restrict__ picks, double *__restrict__ gain,
                                                                      unsigned char *__restrict__ taken, double *__restrict__ z,
                                                                      double *__restrict__ b, double *__restrict__ u,
                                                                      double *__restrict__ U, double *__restrict__ Ut) {
  __shared__ double wv[PD_PICK_THREADS / 64];
  __shared__ int wi[PD_PICK_THREADS / 64];
  const int tid = threadIdx.x;
  double bv = 0.0;
  int bi = PD_NONE;
  for (int q = tid; q < nparts; q += PD_PICK_THREADS) {
    const double v = part_val[q];
    const int i = part_idx[q];
    if (pd_better(v, i, bv, bi)) { bv = v; bi = i; }
  }
  pd_wave_best(bv, bi);
  if ((tid & 63) == 0) { wv[tid >> 6] = bv; wi[tid >> 6] = bi; }
  __syncthreads();
  bv = wv[0]; bi = wi[0];
  for (int w = 1; w < PD_PICK_THREADS / 64; ++w)
    if (pd_better(wv[w], wi[w], bv, bi)) { bv = wv[w]; bi = wi[w]; }
  if (bi == PD_NONE) bi = 0;                    // (B <= n: an untaken row exists; never an index out of range)
  const long j = bi;
  const double g = bv;
  if (tid == 0) {
    picks[t] = bi;
    if (gain) gain[t] = g;
    taken[j] = 1;
  }
  for (int k = tid; k < K; k += PD_PICK_THREADS) {
    z[k] = pd_chain<8>(r, [&](int a) { return valT[a * sa + j * si]; }, [&](int a) { return P[(long)idxT[a * sa + j * si] * ldp + k]; });
  }
  __syncthreads();
  for (int tau = tid; tau < t; tau += PD_PICK_THREADS) {
    b[tau] = pd_chain<16>(K, [&](int k) { return Ut[(size_t)k * B + tau]; }, [&](int k) { return z[k]; });
  }
  __syncthreads();
  const double den = sqrt(g + d);
  for (int k = tid; k < K; k += PD_PICK_THREADS) {
    const double acc = pd_chain<16>(t, [&](int tau) { return U[(size_t)tau * K + k]; }, [&](int tau) { return b[tau]; });
    const double v = z[k] - acc;
    const double uk = v / den;
    u[k] = uk;
    U[(size_t)t * K + k] = uk;
    Ut[(size_t)k * B + t] = uk;
  }
}

// p[j] = sum_k P(j, k) u[k]: one wave per anchor, a row of P_K read coalesced, the order in the head of this file
__global__ __launch_bounds__(256) void design_project_kernel(const double *__restrict__ P, long ldp, int s, int K,
                                                             const double *__restrict__ u, double *__restrict__ p) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= s) return;                           // wave-uniform
  const double *__restrict__ Pj = P + (long)j * ldp;
  double acc = 0.0;
  for (int k = lane; k < K; k += 64) acc = acc + Pj[k] * u[k];
  for (int o = 32; o >= 1; o >>= 1) acc = acc + __shfl_xor(acc, o);
  if (lane == 0) p[j] = acc;
}

// the workspace, in this order; every piece starts on 256 bytes
struct DesignWork {
  size_t idxT, valT, score, taken, part_val, part_idx, zero, z, u, b, p, U, Ut, total;
  DesignWork(long n, int r, int s, int K, int B) {
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += (bytes + 255) / 256 * 256; return o; };
    idxT = take(sizeof(int) * (size_t)n * r);
    valT = take(sizeof(double) * (size_t)n * r);
    score = take(sizeof(double) * (size_t)n);
    taken = take((size_t)n);
    part_val = take(sizeof(double) * PD_MAX_GRID);
    part_idx = take(sizeof(int) * PD_MAX_GRID);
    zero = take(sizeof(double));
    z = take(sizeof(double) * (size_t)K);
    u = take(sizeof(double) * (size_t)K);
    b = take(sizeof(double) * (size_t)B);
    p = take(sizeof(double) * (size_t)s);
    U = take(sizeof(double) * (size_t)K * B);
    Ut = take(sizeof(double) * (size_t)K * B);
    total = at;
  }
};

static bool design_shape_ok(int n, int r, int s, int K, int B) {
  return n >= 1 && r >= 1 && r <= FLGP_RMAX && s >= 1 && s <= 32768 && K >= 1 && B >= 1 && B <= n;
}

size_t predictor_design_bytes(int n, int r, int s, int K, int B) { return DesignWork(n, r, s, K, B).total; }

// the downdate grid: a workgroup per range, at most PD_MAX_GRID, at most the knob predictor_design_grid where it is set
static int design_grid(int n) {
  int g = std::min(ceil_div(n, PD_ROWS), PD_MAX_GRID);
  const int knob = tuning("predictor_design_grid", 0);
  if (knob > 0) g = std::min(g, knob);
  return g;
}

// the loop on the ELL rows of the pool; asynchronous on `st`
int predictor_design_rows(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P, long ldp,
                          int s, int K, double d, int B, int *d_picks, double *d_gain, double *d_score, void *d_work) {
  const DesignWork W(n, r, s, K, B);
  char *w = (char *)d_work;
  int *idxT = (int *)(w + W.idxT);
  double *valT = (double *)(w + W.valT), *score = (double *)(w + W.score);
  unsigned char *taken = (unsigned char *)(w + W.taken);
  double *part_val = (double *)(w + W.part_val);
  int *part_idx = (int *)(w + W.part_idx);
  double *zero = (double *)(w + W.zero), *z = (double *)(w + W.z), *u = (double *)(w + W.u), *b = (double *)(w + W.b);
  double *p = (double *)(w + W.p), *U = (double *)(w + W.U), *Ut = (double *)(w + W.Ut);
  const bool lds = s <= PD_LDS_S;
  const size_t lds_bytes = std::max<size_t>(lds ? sizeof(double) * (size_t)s : 0, PD_REDUCE_BYTES);
  if (lds_bytes > 48 * 1024)
    FLGP_HIP(hipFuncSetAttribute((const void *)design_downdate_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  const int grid = design_grid(n);
  const bool pack = tuning("predictor_design_pack", 1) != 0;
  const int *ri = pack ? idxT : d_ell_idx;
  const double *rv = pack ? valT : d_ell_val;
  const long sa = pack ? n : 1, si = pack ? 1 : r;
  FLGP_HIP(hipMemsetAsync(taken, 0, (size_t)n, st));
  FLGP_HIP(hipMemsetAsync(zero, 0, sizeof(double), st));
  if (pack) {
    hipLaunchKernelGGL(design_pack_kernel, dim3((unsigned)std::min<long>(((long)n * r + 255) / 256, 65536)), dim3(256), 0, st, d_ell_idx,
                       d_ell_val, (long)n, r, idxT, valT);
    FLGP_TRY(check_launch("design_pack_kernel"));
  }
  // score0 = 0.0 + sq: the bits of sq, which is a sum of squares from +0.0
  FLGP_TRY(flgp_dev_predictor_rows(st, d_ell_idx, d_ell_val, n, r, d_P, ldp, s, 1, K, 0, zero, nullptr, 0, score, n));
  ProfScope ps("predictor_design_loop", st, (double)B * (2.0 * s * K + 2.0 * (double)n * r));
  auto downdate = [&](const double *pp) {
    if (lds)
      hipLaunchKernelGGL(design_downdate_kernel<true>, dim3(grid), dim3(PD_ROWS), pp ? lds_bytes : PD_REDUCE_BYTES, st, ri, rv, (long)n,
                         sa, si, r, s, pp, score, taken, part_val, part_idx);
    else
      hipLaunchKernelGGL(design_downdate_kernel<false>, dim3(grid), dim3(PD_ROWS), PD_REDUCE_BYTES, st, ri, rv, (long)n, sa, si, r, s,
                         pp, score, taken, part_val, part_idx);
    return check_launch("design_downdate_kernel");
  };
  FLGP_TRY(downdate(nullptr));
  for (int t = 0; t < B; ++t) {
    hipLaunchKernelGGL(design_pick_kernel, dim3(1), dim3(PD_PICK_THREADS), 0, st, part_val, part_idx, grid, ri, rv, sa, si, r, d_P,
                       ldp, K, d, t, B, d_picks, d_gain, taken, z, b, u, U, Ut);
    FLGP_TRY(check_launch("design_pick_kernel"));
    hipLaunchKernelGGL(design_project_kernel, dim3(ceil_div(s, 4)), dim3(256), 0, st, d_P, ldp, s, K, u, p);
    FLGP_TRY(check_launch("design_project_kernel"));
    FLGP_TRY(downdate(p));
  }
  if (d_score) FLGP_HIP(hipMemcpyAsync(d_score, score, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, st));
  return FLGP_OK;
}

}  // namespace flgp

extern "C" size_t flgp_dev_predictor_design_workspace(int n, int r, int s, int K, int B) {
  if (!design_shape_ok(n, r, s, K, B)) return 0;
  return predictor_design_bytes(n, r, s, K, B);
}

extern "C" int flgp_dev_predictor_design_rows(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P,
                                              long ldp, int s, int K, double d, int B, int *d_picks, double *d_gain, double *d_score,
                                              void *d_work, size_t work_bytes) {
  const char *who = "predictor_design_rows";
  FLGP_REQUIRE(d_ell_idx && d_ell_val && d_P && d_picks && d_work, "%s: null pointer", who);
  FLGP_REQUIRE(design_shape_ok(n, r, s, K, B), "%s: bad shape (n=%d, r=%d, s=%d, K=%d, B=%d)", who, n, r, s, K, B);
  FLGP_REQUIRE(ldp >= K, "%s: ldp=%ld is below K = %d", who, ldp, K);
  FLGP_REQUIRE(std::isfinite(d) && d > 0.0, "%s: the observation variance d = %g must be finite and positive", who, d);
  const size_t need = predictor_design_bytes(n, r, s, K, B);
  FLGP_REQUIRE(work_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed", who, work_bytes, need);
  return predictor_design_rows((hipStream_t)stream, d_ell_idx, d_ell_val, n, r, d_P, ldp, s, K, d, B, d_picks, d_gain, d_score, d_work);
}

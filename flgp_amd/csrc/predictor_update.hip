// The Gram kernel of the predictor's update (include/flgp_hip.h): a regression handle conditioned on newly
// labelled rows.  With e_i = [ z_i ; y_i - mean_i ] (K + q entries; z_i = a_i P_K and mean_i = a_i P_mean the row kernels'
// chains on the row's r scaled anchor weights) and w_i = 1 / (noise_i + sigma),
//   S = sum_i w_i e_i e_i^T   ((K + q) x (K + q)),
// from the ELL rows and P alone: no n x K and no n x (K + q) array exists in global memory.  A workgroup owns one 64 x 64 output
// tile (I, J), I >= J, of one chunk of GC rows; it builds steps of 32 rows of E for its two column tiles in LDS the way
// predictor_cols_kernel builds its tile, the I side scaled by w_i, and feeds them to v_mfma_f64_16x16x4_f64 with the rows as the
// contraction index.  The chunk partials are added in ascending chunk order by a second kernel.  predictor.hip holds the
// entries that use it (flgp_predictor_update / flgp_dev_predictor_update).
#include "common.h"
#include <algorithm>

using namespace flgp;

namespace flgp {

typedef double pg_d4 __attribute__((ext_vector_type(4)));

// PG_CT: the column tile.  PG_STEP: the rows of E in LDS at a time.  PG_GC: the rows of a chunk, counted from row 0 of the call.
// PG_LD: a tile row in doubles; 80 = 16 mod 32, so the MFMA operand read (16 consecutive doubles of four consecutive rows) puts
// the two rows of a half wave on disjoint halves of the 64 banks, and the build's store is 64 consecutive doubles.
constexpr int PG_CT = 64, PG_STEP = 32, PG_GC = 256, PG_WAVES = 4, PG_LD = 80;
constexpr int PG_LAUNCH_CHUNKS = 64;            // the chunks of one launch (knob predictor_gram_launch_chunks)

// grid: x = chunk, y = tile pair p = I (I + 1) / 2 + J.  Wave w builds rows 8 w .. 8 w + 7 of the step, all eight at once: a row's r
// (index, value) pairs sit in lanes 0 .. r-1 and are broadcast, lane l holds column 64 I + l (and 64 J + l), a row of P is one
// coalesced load, and for every a the eight (sixteen) loads of the wave's rows are issued before the first is used -- with a row
// at a time the kernel waited for one load after the other.  The chain is a ascending, multiply then add, from 0.0; a column
// j >= K takes Y(i, j - K) minus the chain, one subtraction.  Rows past the chunk's end and columns past K + q are stored as 0.0;
// no column of P past K + q is loaded (a row past the end repeats the loads of the chunk's last row).  Then wave w owns the 16
// output rows 16 w .. 16 w + 15 of the tile and its block columns bj (bj <= w on a diagonal tile: the blocks above the diagonal
// are not computed): acc[bj] is one chain of MFMAs from 0.0 over the chunk's rows, four at a time, ascending -- the chain of
// flgp_dev_gemm without a workspace on A = (w E)^T, B = E (a zero row adds +0.0 and changes no bit).  D(row = (lane >> 4) + 4 reg,
// col = lane & 15) goes to part[chunk][row (K + q) + col].
__global__ __launch_bounds__(PG_WAVES * 64) void predictor_gram_kernel(const int *__restrict__ ell_idx,
                                                                        const double *__restrict__ ell_val, int n, int r,
                                                                        const double *__restrict__ P, long ldp, int K, int q,
                                                                        const double *__restrict__ w, const double *__restrict__ Y,
                                                                        long ldy, double *__restrict__ part) {
  __shared__ double tA[PG_STEP * PG_LD];      // w_i e_i, columns of tile I
  __shared__ double tB[PG_STEP * PG_LD];      // e_i, columns of tile J
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = K + q;
  int I = 0, J = (int)blockIdx.y;
  while (J > I) { J -= I + 1; ++I; }
  const long i0 = (long)blockIdx.x * PG_GC;
  const long i1 = std::min<long>(i0 + PG_GC, n);
  const int fr = lane & 15, fk = lane >> 4;
  const int nbj = I == J ? wave + 1 : PG_CT / 16;
  pg_d4 acc[PG_CT / 16];
#pragma unroll
  for (int bj = 0; bj < PG_CT / 16; ++bj) acc[bj] = pg_d4{0.0, 0.0, 0.0, 0.0};
  const int jA = I * PG_CT + lane, jB = J * PG_CT + lane;
  const bool onA = jA < W, onB = jB < W;
  constexpr int RW = PG_STEP / PG_WAVES;        // the rows of a step a wave builds, all of them in flight at once
  for (long s0 = i0; s0 < i1; s0 += PG_STEP) {
    const long r0 = s0 + wave * RW;
    double ea[RW], eb[RW];
#pragma unroll
    for (int k = 0; k < RW; ++k) ea[k] = eb[k] = 0.0;
    if (r0 < i1) {                              // wave-uniform; a row past the chunk's end repeats the last one and is zeroed below
      int my_idx[RW];
      double my_val[RW];
#pragma unroll
      for (int k = 0; k < RW; ++k) {
        const long i = std::min<long>(r0 + k, i1 - 1);
        my_idx[k] = 0; my_val[k] = 0.0;
        if (lane < r) { my_idx[k] = ell_idx[i * r + lane]; my_val[k] = ell_val[i * r + lane]; }
      }
      for (int a = 0; a < r; ++a) {
        double va[RW], pa[RW], pb[RW];
#pragma unroll
        for (int k = 0; k < RW; ++k) {           // RW (2 RW off the diagonal) loads before the first use
          const long ja = __builtin_amdgcn_readlane(my_idx[k], a);
          va[k] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_val[k]), a),
                                   __builtin_amdgcn_readlane(__double2loint(my_val[k]), a));
          const double *__restrict__ Pr = P + ja * ldp;
          pa[k] = onA ? Pr[jA] : 0.0;
          pb[k] = (I != J && onB) ? Pr[jB] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < RW; ++k) {
          ea[k] = ea[k] + va[k] * pa[k];
          eb[k] = eb[k] + va[k] * pb[k];
        }
      }
#pragma unroll
      for (int k = 0; k < RW; ++k) {
        const long i = r0 + k;
        if (i < i1) {                           // wave-uniform
          if (I == J) eb[k] = ea[k];
          if (onA && jA >= K) ea[k] = Y[(long)(jA - K) * ldy + i] - ea[k];
          if (onB && jB >= K) eb[k] = Y[(long)(jB - K) * ldy + i] - eb[k];
          ea[k] = w[i] * ea[k];
        }
        if (i >= i1 || !onA) ea[k] = 0.0;
        if (i >= i1 || !onB) eb[k] = 0.0;
      }
    }
#pragma unroll
    for (int k = 0; k < RW; ++k) {
      tA[(wave * RW + k) * PG_LD + lane] = ea[k];
      tB[(wave * RW + k) * PG_LD + lane] = eb[k];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < PG_STEP / 4; ++ks) {
      const double fa = tA[(4 * ks + fk) * PG_LD + 16 * wave + fr];
#pragma unroll
      for (int bj = 0; bj < PG_CT / 16; ++bj) {
        if (bj < nbj) {                         // wave-uniform
          const double fb = tB[(4 * ks + fk) * PG_LD + 16 * bj + fr];
          acc[bj] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa, fb, acc[bj], 0, 0, 0);
        }
      }
    }
    __syncthreads();
  }
  double *__restrict__ pc = part + (size_t)blockIdx.x * (size_t)W * (size_t)W;
#pragma unroll
  for (int bj = 0; bj < PG_CT / 16; ++bj) {
    if (bj >= nbj) continue;
    const int col = J * PG_CT + 16 * bj + fr;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int row = I * PG_CT + 16 * wave + fk + 4 * reg;
      if (row < W && col <= row) pc[(size_t)row * W + col] = acc[bj][reg];
    }
  }
}

// S(k, l), k >= l: from 0.0 (first) or from S(k, l) as it stands, plus the partials of chunks 0, 1, .. in that order; the strict
// upper triangle takes the lower one's bits.  Nothing depends on the grid.
__global__ void predictor_gram_reduce_kernel(const double *__restrict__ part, int nchunk, int W, int first, double *__restrict__ S,
                                             long lds) {
  const int l = blockIdx.x * 64 + (threadIdx.x & 63);
  const int k = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (k >= W || l > k) return;
  const size_t WW = (size_t)W * (size_t)W;
  const double *__restrict__ p = part + (size_t)k * W + l;
  double acc = first ? 0.0 : S[(long)l * lds + k];
  for (int c = 0; c < nchunk; ++c) acc = acc + p[(size_t)c * WW];
  S[(long)l * lds + k] = acc;
  if (l < k) S[(long)k * lds + l] = acc;
}

// M = I + S[:K, :K] (K x K, ld K) and R = S[:K, K:] (K x q, ld K) of S ((K + q) x (K + q), ld K + q)
__global__ void predictor_update_system_kernel(const double *__restrict__ S, int K, int q, double *__restrict__ M,
                                               double *__restrict__ R) {
  const long W = K + q, total = (long)K * W;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long k = e % K, c = e / K;
    const double v = S[c * W + k];
    if (c < K) M[c * K + k] = k == c ? 1.0 + v : v;
    else R[(c - K) * K + k] = v;
  }
}

// the chunks of one launch: the knob, no more than 256 MiB of partials
static int gram_launch_chunks(int K, int q) {
  const size_t one = sizeof(double) * ((size_t)K + q) * ((size_t)K + q);
  const long cap = std::max<long>(1, (long)(((size_t)256 << 20) / one));
  return (int)std::min<long>(std::max(1, tuning("predictor_gram_launch_chunks", PG_LAUNCH_CHUNKS)), cap);
}

size_t predictor_gram_bytes(long n, int K, int q) {
  const size_t W = (size_t)K + (size_t)q;
  return sizeof(double) * (size_t)std::min<long>((n + PG_GC - 1) / PG_GC, gram_launch_chunks(K, q)) * W * W;
}

int predictor_gram_chunk() { return PG_GC; }

// launches of at most gram_launch_chunks chunks, each followed by its reduction into S: one ascending chain whatever the knob
int predictor_gram(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P, long ldp, int K,
                   int q, const double *d_w, const double *d_Y, long ldy, double *d_S, long lds, double *d_part, bool first) {
  const int W = K + q, T = ceil_div(W, PG_CT);
  const long per = (long)gram_launch_chunks(K, q) * PG_GC;
  ProfScope ps("predictor_gram", st, (double)n * ((double)W * W + 2.0 * r * W));
  for (long i0 = 0; i0 < n; i0 += per) {
    const int nl = (int)std::min<long>(per, n - i0), nchunk = ceil_div(nl, PG_GC);
    hipLaunchKernelGGL(predictor_gram_kernel, dim3(nchunk, T * (T + 1) / 2), dim3(PG_WAVES * 64), 0, st, d_ell_idx + i0 * r,
                       d_ell_val + i0 * r, nl, r, d_P, ldp, K, q, d_w + i0, d_Y ? d_Y + i0 : nullptr, ldy, d_part);
    FLGP_TRY(check_launch("predictor_gram_kernel"));
    hipLaunchKernelGGL(predictor_gram_reduce_kernel, dim3(ceil_div(W, 64), ceil_div(W, 4)), dim3(256), 0, st, d_part, nchunk, W,
                       first && i0 == 0 ? 1 : 0, d_S, lds);
    FLGP_TRY(check_launch("predictor_gram_reduce_kernel"));
  }
  return FLGP_OK;
}

int predictor_update_system(hipStream_t st, const double *d_S, int K, int q, double *d_M, double *d_R) {
  const long total = (long)K * (K + q);
  hipLaunchKernelGGL(predictor_update_system_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, st, d_S, K, q,
                     d_M, d_R);
  return check_launch("predictor_update_system_kernel");
}

}  // namespace flgp

extern "C" size_t flgp_dev_predictor_gram_workspace(int n, int K, int q) {
  if (n < 1 || K < 1 || q < 0) return 0;
  return predictor_gram_bytes(n, K, q);
}

extern "C" int flgp_dev_predictor_gram(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P,
                                       long ldp, int s, int K, int q, const double *d_w, const double *d_Y, long ldy, double *d_S,
                                       long lds, void *d_work, size_t work_bytes) {
  const char *who = "predictor_gram";
  FLGP_REQUIRE(d_ell_idx && d_ell_val && d_P && d_w && d_S && d_work, "%s: null pointer", who);
  FLGP_REQUIRE(q == 0 || d_Y, "%s: null pointer (q = %d needs Y)", who, q);
  FLGP_REQUIRE(n >= 1 && r >= 1 && r <= FLGP_RMAX && s >= 1 && K >= 1 && q >= 0, "%s: bad shape (n=%d, r=%d, s=%d, K=%d, q=%d)", who, n, r,
               s, K, q);
  const long W = (long)K + q;
  FLGP_REQUIRE(ceil_div((int)std::min<long>(W, 1 << 30), PG_CT) <= 361, "%s: K + q = %ld is above %d columns", who, W, 361 * PG_CT);
  FLGP_REQUIRE(ldp >= W, "%s: ldp=%ld is below K + q = %ld", who, ldp, W);
  FLGP_REQUIRE(q == 0 || ldy >= n, "%s: ldy=%ld is below n = %d", who, ldy, n);
  FLGP_REQUIRE(lds >= W, "%s: lds=%ld is below K + q = %ld", who, lds, W);
  const size_t need = predictor_gram_bytes(n, K, q);
  FLGP_REQUIRE(work_bytes >= need, "%s: the workspace holds %zu bytes, %zu are needed", who, work_bytes, need);
  return predictor_gram((hipStream_t)stream, d_ell_idx, d_ell_val, n, r, d_P, ldp, K, q, d_w, d_Y, ldy, d_S, lds, (double *)d_work, true);
}

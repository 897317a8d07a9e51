// The wide row kernel of the fitted predictor and the kernels of the draws handle (include/flgp_hip.h).
//   out(i, c) = sum_a A(i, a) P(idx(i, a), c0 + c),   c < nc
// is the chain of predictor_rows_kernel / predictor_pg_rows_kernel (predictor_rows.hip) -- a ascending, multiply then add, from
// 0.0 -- for hundreds of columns: those kernels give lane l column 64 c + l and store it at once, 64 addresses ldo doubles apart.
// Here a workgroup owns 64 rows x 64 columns, passes the tile through LDS and stores column segments of 64 consecutive rows.
// The draws handle: xi(k, col) from the project's counter RNG (rng.h) and P_draw(:, col) = P_mean(:, c) + P_K xi(:, col).
#include "common.h"
#include "rng.h"
#include <algorithm>

using namespace flgp;

namespace flgp {

// A wave per row as in predictor_rows_kernel: the row's r (index, value) pairs sit in lanes 0 .. r-1 and are broadcast, lane l
// holds column 64 ct + l, a row of P is one coalesced load.  Wave w computes rows 16 w .. 16 w + 15 of the tile into
// tile[row][column]; then lane l is row l and wave w stores columns w, w + 4, ..: 512 contiguous bytes per column.  A tile row
// is 65 doubles: the compute phase writes 64 consecutive doubles, the store phase reads doubles 65 apart, which are 32
// distinct bank pairs per half wave.  Rows past n are not computed and not stored, columns past nc load and store nothing.
constexpr int PC_TILE = 64, PC_WAVES = 4, PC_LD = PC_TILE + 1;
constexpr int PC_TILE_MIN = 512;                 // the narrowest call the tile kernel takes (knob predictor_cols_tile_min)
__global__ __launch_bounds__(PC_WAVES * 64) void predictor_cols_kernel(const int *__restrict__ ell_idx,
                                                                        const double *__restrict__ ell_val, int n, int r,
                                                                        const double *__restrict__ P, long ldp, int c0, int nc,
                                                                        double *__restrict__ out, long ldo) {
  __shared__ double tile[PC_TILE * PC_LD];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long i0 = (long)blockIdx.x * PC_TILE;
  const int nct = (nc + PC_TILE - 1) / PC_TILE;
  for (int ct = blockIdx.y; ct < nct; ct += gridDim.y) {
    const int j = ct * PC_TILE + lane;
    const bool on = j < nc;
    const double *__restrict__ Pc = P + c0 + j;
    for (int k = 0; k < PC_TILE / PC_WAVES; ++k) {
      const int rl = wave * (PC_TILE / PC_WAVES) + k;
      const long i = i0 + rl;
      if (i >= n) break;                        // wave-uniform
      int my_idx = 0;
      double my_val = 0.0;
      if (lane < r) { my_idx = ell_idx[i * r + lane]; my_val = ell_val[i * r + lane]; }
      double z = 0.0;
      for (int a = 0; a < r; ++a) {
        const long ja = __builtin_amdgcn_readlane(my_idx, a);
        const double va = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(my_val), a),
                                           __builtin_amdgcn_readlane(__double2loint(my_val), a));
        if (on) z = z + va * Pc[ja * ldp];
      }
      tile[rl * PC_LD + lane] = z;
    }
    __syncthreads();
    const long i = i0 + lane;
    if (i < n) {
      for (int cc = wave; cc < PC_TILE; cc += PC_WAVES) {
        const int c = ct * PC_TILE + cc;
        if (c < nc) out[(long)c * ldo + i] = tile[lane * PC_LD + cc];
      }
    }
    __syncthreads();
  }
}

// xi(k, col) = normal p = k of stream (col / S) 2^32 + col % S under seed (pg_normals_kernel's expression); xi[k ncol + col]
__global__ void draws_normals_kernel(unsigned long long seed, int K, int S, long ncol, double *__restrict__ xi) {
  const long total = (long)K * ncol;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    const long col = e % ncol;
    const unsigned long long k = (unsigned long long)(e / ncol);
    const unsigned long long base = rng_stream_base(seed, ((unsigned long long)(col / S) << 32) + (unsigned long long)(col % S));
    xi[e] = rng_box_muller(rng_unif(base, 2ull * k), rng_unif(base, 2ull * k + 1));
  }
}

// P_draw(j, col) = P(j, g w + K + c) + acc, acc the chain over k ascending from 0.0 of P(j, g w + k) xi(k, col), multiply then
// add; col = (g q + c) S + t.  A lane per column of one group (blockIdx.z), so the entries of P are wave-uniform; DF_J rows
// of P per pass over xi.  A column depends on (P, seed, g, c, t) alone.
constexpr int DF_J = 8;
__global__ __launch_bounds__(256) void draws_fold_kernel(const double *__restrict__ P, long ldp, int s, int groups, int K, int q,
                                                         int S, const double *__restrict__ xi, long ncol,
                                                         double *__restrict__ Pd, long ldd) {
  const long qS = (long)q * S;
  const long cg = (long)blockIdx.x * 256 + threadIdx.x;
  const bool on = cg < qS;
  const int c = on ? (int)(cg / S) : 0;
  for (int g = blockIdx.z; g < groups; g += gridDim.z) {
    const double *__restrict__ Pg = P + (long)g * (K + q);
    const long col = (long)g * qS + cg;
    for (int j0 = blockIdx.y * DF_J; j0 < s; j0 += gridDim.y * DF_J) {
      double acc[DF_J];
#pragma unroll
      for (int jj = 0; jj < DF_J; ++jj) acc[jj] = 0.0;
      for (int k = 0; k < K; ++k) {
        const double x = on ? xi[(long)k * ncol + col] : 0.0;
#pragma unroll
        for (int jj = 0; jj < DF_J; ++jj) {
          const int jr = j0 + jj < s ? j0 + jj : s - 1;
          acc[jj] = acc[jj] + Pg[(long)jr * ldp + k] * x;
        }
      }
      if (on) {
#pragma unroll
        for (int jj = 0; jj < DF_J; ++jj)
          if (j0 + jj < s) Pd[(long)(j0 + jj) * ldd + col] = Pg[(long)(j0 + jj) * ldp + K + c] + acc[jj];
      }
    }
  }
}

// C(i, j) = C(j, i) for i < j: the strict upper triangle takes the lower one's bits (C n x n column-major, ldc)
__global__ void sym_mirror_kernel(double *__restrict__ C, int n, long ldc) {
  const int i = blockIdx.x * 64 + (threadIdx.x & 63);
  if (i >= n) return;
  for (long j = (long)blockIdx.y * 4 + (threadIdx.x >> 6); j < n; j += (long)gridDim.y * 4)
    if (i < j) C[j * ldc + i] = C[(long)i * ldc + j];
}

int draws_normals_fill(hipStream_t st, unsigned long long seed, int K, int S, long ncol, double *d_xi) {
  const long total = (long)K * ncol;
  hipLaunchKernelGGL(draws_normals_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 1 << 20)), dim3(256), 0, st, seed, K, S, ncol,
                     d_xi);
  return check_launch("draws_normals_kernel");
}

int draws_fold(hipStream_t st, const double *d_P, long ldp, int s, int groups, int K, int q, int S, const double *d_xi, double *d_Pd,
               long ldd) {
  const long qS = (long)q * S;
  const dim3 grid((unsigned)((qS + 255) / 256), std::min(ceil_div(s, DF_J), 65535), std::min(groups, 65535));
  hipLaunchKernelGGL(draws_fold_kernel, grid, dim3(256), 0, st, d_P, ldp, s, groups, K, q, S, d_xi, (long)groups * qS, d_Pd, ldd);
  return check_launch("draws_fold_kernel");
}

int sym_mirror(hipStream_t st, double *d_C, int n, long ldc) {
  hipLaunchKernelGGL(sym_mirror_kernel, dim3(ceil_div(n, 64), std::min(ceil_div(n, 4), 65535)), dim3(256), 0, st, d_C, n, ldc);
  return check_launch("sym_mirror_kernel");
}

}  // namespace flgp

extern "C" int flgp_dev_predictor_cols(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *d_P,
                                       long ldp, int s, int c0, int nc, double *d_out, long ldo) {
  const char *who = "predictor_cols";
  FLGP_REQUIRE(d_ell_idx && d_ell_val && d_P && d_out, "%s: null pointer", who);
  FLGP_REQUIRE(n >= 1 && r >= 1 && r <= FLGP_RMAX && s >= 1 && nc >= 1, "%s: bad shape (n=%d, r=%d, s=%d, nc=%d)", who, n, r, s, nc);
  FLGP_REQUIRE(c0 >= 0 && (long)c0 + nc <= ldp, "%s: columns [%d, %ld) are outside ldp = %ld", who, c0, (long)c0 + nc, ldp);
  FLGP_REQUIRE(ldo >= n, "%s: ldo=%ld is below n = %d", who, ldo, n);
  hipStream_t st = (hipStream_t)stream;
  // Below this width the tile kernel was measured no faster than predictor_pg_rows_kernel asked for f alone (DESIGN f-23): those
  // widths go to that kernel, handed P + c0.  The two kernels walk the same chain, so the knob changes no bit.
  if (nc < std::max(1, tuning("predictor_cols_tile_min", PC_TILE_MIN)))
    return flgp_dev_predictor_pg_rows(stream, d_ell_idx, d_ell_val, n, r, d_P + c0, ldp, s, nc, d_out, ldo, nullptr, 0, nullptr, 0, nullptr);
  ProfScope ps("predictor_cols", st, 2.0 * (double)n * r * nc);
  const dim3 grid(ceil_div(n, PC_TILE), std::min(ceil_div(nc, PC_TILE), 65535));
  hipLaunchKernelGGL(predictor_cols_kernel, grid, dim3(PC_WAVES * 64), 0, st, d_ell_idx, d_ell_val, n, r, d_P, ldp, c0, nc, d_out, ldo);
  return check_launch("predictor_cols_kernel");
}

extern "C" int flgp_dev_predictor_draws_fold(void *stream, const double *d_P, long ldp, int s, int groups, int K, int q, int S,
                                             unsigned long long seed, double *d_xi, double *d_Pdraw, long ldd) {
  const char *who = "predictor_draws_fold";
  FLGP_REQUIRE(d_P && d_xi && d_Pdraw, "%s: null pointer", who);
  FLGP_REQUIRE(s >= 1 && groups >= 1 && K >= 1 && q >= 1 && S >= 1, "%s: bad shape (s=%d, groups=%d, K=%d, q=%d, S=%d)", who, s, groups, K,
               q, S);
  const long ncol = (long)groups * q * S;
  FLGP_REQUIRE(ncol <= 0x7fffffffL - 15, "%s: groups q S = %ld columns overflow an int", who, ncol);
  FLGP_REQUIRE(ldp >= (long)groups * ((long)K + q), "%s: ldp=%ld is below groups (K + q) = %ld", who, ldp, (long)groups * ((long)K + q));
  FLGP_REQUIRE(ldd >= ncol, "%s: ldd=%ld is below groups q S = %ld", who, ldd, ncol);
  hipStream_t st = (hipStream_t)stream;
  FLGP_TRY(draws_normals_fill(st, seed, K, S, ncol, d_xi));
  return draws_fold(st, d_P, ldp, s, groups, K, q, S, d_xi, d_Pdraw, ldd);
}

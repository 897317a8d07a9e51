// k5 and the sparse half of k6: everything that touches the n x s similarity matrix Z / A in
// its ELL form (row-major idx[n][r], val[n][r], rows sorted by column).
//
//   - CSC view of the pattern by a stable counting sort (deterministic, rows ascending);
//   - column sums in row-ascending order == `RowVectorXd::Ones(n) * Z` on a row-major sparse
//     matrix (reference src/Utils.cpp:200,203, src/Spectrum.cpp:149), bit-exact vs the oracle;
//   - column / row scalings of graphLaplacian_cpp (src/Utils.cpp:195-212) and of
//     spectrum_from_Z_cpp (src/Spectrum.cpp:150);
//   - Gram matrix G = A^T A in a fixed summation order (the s x s operator RSpectra::svds
//     iterates on, src/TruncatedSVD.cpp:23-28);
//   - u_k = A v_k / sigma_k * sqrt(n) (svds' left vectors + src/Spectrum.cpp:157-158).
//
// All of these are HBM / latency bound integer-and-fp64 streaming work: no MFMA here.
#include "common.h"

namespace flgp {

// ----------------------------------------------------------------------------------------
// CSC build: stable counting sort of the nnz = n*r entries by column.
//   pass 1  per-chunk column histograms (LDS int atomics: counts are order independent)
//   pass 2  per column: exclusive prefix over chunks, column totals
//   pass 3  exclusive scan of the totals -> colptr
//   pass 4  one wave per chunk walks its entries in order, 64 at a time; lanes that hit the
//           same column in one step are ranked by lane id (ballot-built match mask), so the
//           order inside a column is exactly the entry order == ascending row.
// ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void csc_hist_kernel(const int *__restrict__ ell_idx, long nnz, int s,
                                                       int chunk, int *__restrict__ hist) {
  extern __shared__ int lh[];
  for (int j = threadIdx.x; j < s; j += blockDim.x) lh[j] = 0;
  __syncthreads();
  const long e0 = (long)blockIdx.x * chunk;
  long e1 = e0 + chunk;
  if (e1 > nnz) e1 = nnz;
  for (long e = e0 + threadIdx.x; e < e1; e += blockDim.x) atomicAdd(&lh[ell_idx[e]], 1);
  __syncthreads();
  int *out = hist + (size_t)blockIdx.x * s;
  for (int j = threadIdx.x; j < s; j += blockDim.x) out[j] = lh[j];
}

__global__ void csc_colscan_kernel(int *__restrict__ hist, int nchunks, int s, int *__restrict__ tot) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= s) return;
  int run = 0;
  // 16 loads in flight per thread: one load, one store, one add at a time (the compiler cannot move a load above
  // the preceding store to the same array) made each of the ~2000 steps a full memory round trip
  constexpr int CB = 16;
  int c = 0;
  for (; c + CB <= nchunks; c += CB) {
    int h[CB];
#pragma unroll
    for (int u = 0; u < CB; ++u) h[u] = hist[(size_t)(c + u) * s + j];
#pragma unroll
    for (int u = 0; u < CB; ++u) { hist[(size_t)(c + u) * s + j] = run; run += h[u]; }
  }
  for (; c < nchunks; ++c) {
    const int h = hist[(size_t)c * s + j];
    hist[(size_t)c * s + j] = run;
    run += h;
  }
  tot[j] = run;
}

// single-block exclusive scan of tot[0..s) -> colptr[0..s]
__global__ __launch_bounds__(1024) void csc_scan_kernel(const int *__restrict__ tot, int s, int *__restrict__ colptr) {
  __shared__ int part[1024];
  const int t = threadIdx.x;
  const int per = (s + 1023) / 1024;
  const int lo = t * per, hi = (lo + per < s) ? lo + per : s;
  int sum = 0;
  for (int j = lo; j < hi; ++j) sum += tot[j];
  part[t] = sum;
  __syncthreads();
  for (int off = 1; off < 1024; off <<= 1) {
    int v = (t >= off) ? part[t - off] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = (t == 0) ? 0 : part[t - 1];
  for (int j = lo; j < hi; ++j) { colptr[j] = run; run += tot[j]; }
  if (t == 1023) colptr[s] = part[1023];
}

__global__ __launch_bounds__(64) void csc_scatter_kernel(const int *__restrict__ ell_idx, long nnz, int s,
                                                         int chunk, int nbits, const int *__restrict__ hist,
                                                         const int *__restrict__ colptr, int *__restrict__ pos) {
  extern __shared__ int cur[];  // running count per column inside this chunk
  const int lane = threadIdx.x;
  for (int j = lane; j < s; j += 64) cur[j] = 0;
  __syncthreads();
  const int *hoff = hist + (size_t)blockIdx.x * s;
  const long e0 = (long)blockIdx.x * chunk;
  long e1 = e0 + chunk;
  if (e1 > nnz) e1 = nnz;
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  for (long eb = e0; eb < e1; eb += 64) {
    const long e = eb + lane;
    const bool act = e < e1;
    const int col = act ? ell_idx[e] : 0;
    unsigned long long m = __ballot(act);
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (col >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    if (act) {
      const int rank = __popcll(m & lt);
      const int base = cur[col];
      pos[(size_t)colptr[col] + hoff[col] + base + rank] = (int)e;
      if (rank == 0) cur[col] = base + __popcll(m);  // one writer per column group; all read before (same instr)
    }
    __syncthreads();  // single wave: orders the LDS read-modify-write between steps
  }
}

// Column sums in the fixed two-level order of the oracle (oracle/flgp_oracle.c, flgp_oracle_colsum): chunks of
// COLSUM_CHUNK consecutive rows; inside a chunk every column's entries are added in row order, then the chunk totals
// in chunk order.  One wave owns a chunk and a table of s sums in LDS, streams the chunk's entries 64 at a time
// (coalesced: the round-1 kernel walked the CSC lists instead and fetched a 128-byte line for every 8-byte value,
// 1.2 GB for 80 MB) and adds them with ds_add_f64.  Lanes of one step that hit the same column are ranked by lane
// (= entry order) with the ballot match of csc_scatter_kernel and applied in as many passes as the largest rank
// needs; the LDS unit executes a wave's instructions in order, so pass k+1 sees pass k.
constexpr int COLSUM_CHUNK = 1024;     // rows; FLGP_COLSUM_CHUNK of the oracle

// WIN: the table holds the columns [w0, w0 + wn) of window blockIdx.y only (s beyond what LDS holds: the chunk is walked once
// per window, entries of other windows are skipped -- the order inside a column is untouched)
template <bool WIN>
__global__ __launch_bounds__(64) void colsum_chunk_kernel(const int *__restrict__ ell_idx, const double *__restrict__ val,
                                                          int n, int r, int s, int nbits, double *__restrict__ part, int wmax,
                                                          int direct) {
  extern __shared__ double bins[];
  const int lane = threadIdx.x;
  const int w0 = WIN ? (int)blockIdx.y * wmax : 0;
  const int wn = WIN ? ((s - w0 < wmax) ? s - w0 : wmax) : s;
  for (int j = lane; j < wn; j += 64) bins[j] = 0.0;
  __syncthreads();
  const long i0 = (long)blockIdx.x * COLSUM_CHUNK;
  const long i1 = (i0 + COLSUM_CHUNK < n) ? i0 + COLSUM_CHUNK : n;
  const long e0 = i0 * r, e1 = i1 * r;
  if (direct) {
    // ONE ds_add_f64 per step of 64 entries: lanes that hit the same column are applied by the LDS unit in ascending lane
    // order, which is the entries' order -- the rule gram_kernel's row groups rest on (bit-exact there and here on all 1e6
    // rows of configs[2]); the LDS unit executes a wave's instructions in order, so step follows step.  Eight steps' loads
    // are in flight (with one the wave -- alone on its SIMD: 977 chunks on 1024 SIMDs -- waited a memory latency per step).
    constexpr int CU = 8;
    for (long eb = e0; eb < e1; eb += 64 * CU) {
      int cq[CU];
      double vq[CU];
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        const long e = eb + 64 * u + lane;
        const long ec = e < e1 ? e : e1 - 1;             // (unconditional loads: a valid address, masked below)
        cq[u] = ell_idx[ec];
        vq[u] = val[ec];
      }
#pragma unroll
      for (int u = 0; u < CU; ++u) {
        const bool on = eb + 64 * u + lane < e1 && (!WIN || (unsigned)(cq[u] - w0) < (unsigned)wn);
        const int bin = on ? cq[u] - w0 : 0;
        if (on) __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)&bins[bin], vq[u]);
      }
    }
    __syncthreads();
    double *outd = part + (size_t)blockIdx.x * s + w0;
    for (int j = lane; j < wn; j += 64) outd[j] = bins[j];
    return;
  }
  const unsigned long long lt = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  // the next step's entries are loaded while this step's are ranked and added
  long e = e0 + lane;
  int col = (e < e1) ? ell_idx[e] : 0;
  double v = (e < e1) ? val[e] : 0.0;
  for (long eb = e0; eb < e1; eb += 64) {
    const long en = eb + 64 + lane;
    const int coln = (en < e1) ? ell_idx[en] : 0;
    const double vn = (en < e1) ? val[en] : 0.0;
    const bool act = eb + lane < e1 && (!WIN || (unsigned)(col - w0) < (unsigned)wn);
    unsigned long long m = __ballot(act);
    for (int b = 0; b < nbits; ++b) {
      const bool bit = (col >> b) & 1;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const int rank = act ? __popcll(m & lt) : -1;
    // pass k adds the lanes of rank k; the ranks of a column's lanes are 0, 1, 2, ... without gaps, so the first k that
    // nobody holds ends the step (a ballot per pass; the wave-wide maximum by six dependent shuffles that stood here was
    // most of the step: ~700 of its ~1200 cycles)
    for (int k = 0; __ballot(rank == k) != 0ull; ++k)
      if (rank == k)
        __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)&bins[col - w0], v);
    col = coln; v = vn;
  }
  __syncthreads();
  double *out = part + (size_t)blockIdx.x * s + w0;
  for (int j = lane; j < wn; j += 64) out[j] = bins[j];
}

// colsum[j] = chunk totals added in chunk order, from 0.0
__global__ void colsum_reduce_kernel(const double *__restrict__ part, int nchunks, int s, double *__restrict__ colsum) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= s) return;
  double acc = 0.0;
  int c = 0;
  for (; c + 32 <= nchunks; c += 32) {    // 32 loads in flight, added in order (s / 256 workgroups: a few waves on the whole chip,
    double p[32];                         //  every batch a memory latency -- with eight in flight 46 us for 977 chunks)
#pragma unroll
    for (int u = 0; u < 32; ++u) p[u] = part[(size_t)(c + u) * s + j];
#pragma unroll
    for (int u = 0; u < 32; ++u) acc += p[u];
  }
  for (; c + 8 <= nchunks; c += 8) {
    double p[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) p[u] = part[(size_t)(c + u) * s + j];
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += p[u];
  }
  for (; c < nchunks; ++c) acc += part[(size_t)c * s + j];
  colsum[j] = acc;
}

__global__ void col_scale_kernel(const int *__restrict__ ell_idx, double *__restrict__ val, long nnz,
                                 const double *__restrict__ colsum, const double *__restrict__ num_class,
                                 int mode) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  const int j = ell_idx[e];
  const double c = colsum[j];
  double v = val[e];
  if (mode == 0) {
    v = v * (1.0 / (c + 1e-9));                    // src/Utils.cpp:201,204
    if (num_class) v = v * num_class[j];           // src/Utils.cpp:205
  } else {
    v = v * (1.0 / __builtin_sqrt(__builtin_fabs(c) + 1e-9));  // src/Spectrum.cpp:150
  }
  val[e] = v;
}

// 256 rows per workgroup, staged through LDS: the rows are r doubles apart, so a thread walking its own row in
// global memory touched a different cache line than its neighbours on every load (measured: 4x the bytes fetched and
// written); the block's 256 r values are one contiguous run, read and written back coalesced.
// With `idx` the column scaling of col_scale_kernel's mode 0 is applied on the way in (the same two or three rounded
// multiplications per entry, then the same row sums): graphLaplacian_cpp's two passes over the values in one.
__global__ __launch_bounds__(256) void row_normalize_kernel(double *__restrict__ val, int n, int r,
                                                            const int *__restrict__ idx = nullptr,
                                                            const double *__restrict__ colsum = nullptr,
                                                            const double *__restrict__ num_class = nullptr) {
  extern __shared__ double rn_rows[];
  const long i0 = (long)blockIdx.x * 256;
  const int rows = (n - i0 < 256) ? (int)(n - i0) : 256;
  double *g = val + (size_t)i0 * r;
  const int cnt = rows * r;
  if (idx) {
    const int *gi = idx + (size_t)i0 * r;
    for (int e = threadIdx.x; e < cnt; e += 256) {
      const int j = gi[e];
      double v = g[e];
      v = v * (1.0 / (colsum[j] + 1e-9));              // src/Utils.cpp:201,204
      if (num_class) v = v * num_class[j];             // src/Utils.cpp:205
      rn_rows[e] = v;
    }
  } else
  for (int e = threadIdx.x; e < cnt; e += 256) rn_rows[e] = g[e];
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    double *row = rn_rows + (size_t)threadIdx.x * r;
    double rs = 0.0;
    for (int a = 0; a < r; ++a) rs += row[a];        // ascending column order (src/Utils.cpp:210)
    const double inv = 1.0 / (rs + 1e-9);
    for (int a = 0; a < r; ++a) row[a] = inv * row[a];  // src/Utils.cpp:211
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cnt; e += 256) g[e] = rn_rows[e];
}

// A row's values under GIVEN column sums (the fitted spectrum model's extension, model.hip): col_scale_kernel's mode 0,
// the row normalisation above and col_scale_kernel's mode 1 in one pass over the values, in row_normalize_kernel's shape
// (256 rows per workgroup through LDS, coalesced in and out).  Every entry sees the same rounded operations in the same
// order as in the three kernels, so the bits are theirs; c1 == nullptr ("rw"): no scaling on the way in.  The column
// indices are read again on the way out (coalesced, and in cache from the way in) rather than kept in LDS.
__global__ __launch_bounds__(256) void extend_scale_kernel(const int *__restrict__ idx, double *__restrict__ val, int n, int r,
                                                           const double *__restrict__ c1, const double *__restrict__ num_class,
                                                           const double *__restrict__ c2) {
  extern __shared__ double es_rows[];
  const long i0 = (long)blockIdx.x * 256;
  const int rows = (n - i0 < 256) ? (int)(n - i0) : 256;
  double *g = val + (size_t)i0 * r;
  const int *gi = idx + (size_t)i0 * r;
  const int cnt = rows * r;
  if (c1) {
    for (int e = threadIdx.x; e < cnt; e += 256) {
      const int j = gi[e];
      double v = g[e];
      v = v * (1.0 / (c1[j] + 1e-9));                  // src/Utils.cpp:201,204
      if (num_class) v = v * num_class[j];             // src/Utils.cpp:205
      es_rows[e] = v;
    }
  } else
  for (int e = threadIdx.x; e < cnt; e += 256) es_rows[e] = g[e];
  __syncthreads();
  if ((int)threadIdx.x < rows) {
    double *row = es_rows + (size_t)threadIdx.x * r;
    double rs = 0.0;
    for (int a = 0; a < r; ++a) rs += row[a];        // ascending column order (src/Utils.cpp:210)
    const double inv = 1.0 / (rs + 1e-9);
    for (int a = 0; a < r; ++a) row[a] = inv * row[a];  // src/Utils.cpp:211
  }
  __syncthreads();
  for (int e = threadIdx.x; e < cnt; e += 256)
    g[e] = es_rows[e] * (1.0 / __builtin_sqrt(__builtin_fabs(c2[gi[e]]) + 1e-9));  // src/Spectrum.cpp:150
}

// ----------------------------------------------------------------------------------------
// Gram: one wave per column j1.  The wave owns row j1 of G in LDS (s doubles) and walks the column's entries in
// ascending row order: every G(j1, j2) is summed in ascending row order -- deterministic, and identical to the oracle.
// A row's r products go to r distinct bins; consecutive rows of a column share anchors (they all have j1, and usually
// more).  One ds_add_f64 serves a group of rows: lanes that hit the same bin are applied in ascending lane order
// (= ascending row), and the LDS unit executes a wave's instructions in order, so the sums stay sequential without a
// round trip through registers (see the note at `apply` below).
//
// Where the time goes: a ds_add_f64 costs ~60 cycles per instruction per wave whatever the number of active lanes
// (scripts/ubench_ldsatomic.hip), and four waves per CU get four times that throughput: 0.25 ms at the flagship shape.
// The row of G caps a CU at one wave per SIMD, so nothing else hides a wave's memory latency: what counts is how many
// rows a wave has in flight.  Hence
//   * a group is as many rows as 64 lanes hold: LPR lanes per row, 64 / LPR rows per ds_add_f64.  LPR = r where that
//     gains a row over the power-of-two packing (six rows at r = 10 instead of four), else 16 or 32;
//   * the column is walked in steps of GF groups, and the wave keeps GF groups of loads in flight at all times: as soon
//     as a group is applied, the group GF places on (the same place of the next step) is fetched into its registers;
//   * the positions of a step are fetched two steps ahead, so that they are there when its first group is fetched;
//   * every load is issued unconditionally at a valid address (an idle slot reads entry p0 / row 0), so that the number
//     in flight does not depend on the data and the compiler's vmcnt waits are counted, not vmcnt(0);
//   * entry / r is a multiplication;
//   * the waves are dealt their columns longest first (`order`, gram_order_kernel below): a column is one wave's work
//     from end to end, and the longest one at the flagship shape is 278 steps where a fair share is 153 -- started
//     last it runs on alone.  Which wave takes which column changes no sum.
// ----------------------------------------------------------------------------------------
// order[0..s): the columns by descending entry count, ties by ascending column: an exact rank sort.  Thread j counts
// the keys (count, s - 1 - j) above its own -- they are all distinct, so the ranks are a permutation.  A workgroup
// serves 64 columns (lane = column) with sixteen waves that take a sixteenth of the keys each: the key a wave compares
// against is the same in all its lanes, so it comes through the scalar cache and costs the vector unit a compare and
// an add.  (Tiles of keys in LDS, 256 columns per workgroup and one wave per SIMD: 0.10 ms at s = 5000, every read
// waited for.)  Nothing to tune or to fall back from up to FLGP_SMAX.
constexpr int ORDER_WAVES = 16;
__device__ __forceinline__ unsigned long long gram_order_key(const int *__restrict__ colptr, int s, int j) {
  return ((unsigned long long)(unsigned)(colptr[j + 1] - colptr[j]) << 32) | (unsigned)(s - 1 - j);
}
__global__ __launch_bounds__(64 * ORDER_WAVES) void gram_order_kernel(const int *__restrict__ colptr, int s,
                                                                       int *__restrict__ order) {
  __shared__ int part[ORDER_WAVES][64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int j = blockIdx.x * 64 + lane;
  const unsigned long long mine = gram_order_key(colptr, s, j < s ? j : s - 1);
  const int per = (s + ORDER_WAVES - 1) / ORDER_WAVES;
  const int q0 = w * per, q1 = q0 + per < s ? q0 + per : s;
  int rank = 0;
#pragma unroll 8
  for (int q = q0; q < q1; ++q) rank += gram_order_key(colptr, s, q) > mine ? 1 : 0;
  part[w][lane] = rank;
  __syncthreads();
  if (w == 0 && j < s) {
    int total = 0;
#pragma unroll
    for (int k = 0; k < ORDER_WAVES; ++k) total += part[k][lane];
    order[total] = j;
  }
}

// A row's record: its r values, then its r indices, in 128 bytes (r <= 10), 256 (r <= 21) or 384: one cache line per
// visit of gram_kernel at r <= 10 where the two ELL rows (80 bytes at 80 i, 40 at 40 i) straddle 2.93 on average.
static int gram_record_doubles(int r) { return ceil_div(12 * r, 128) * 16; }
__global__ __launch_bounds__(256) void gram_pack_kernel(const int *__restrict__ ell_idx, const double *__restrict__ val, long nnz,
                                                        int r, double inv_r, int recd, double *__restrict__ rec) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= nnz) return;
  const long row = (long)(((double)e + 0.5) * inv_r);
  const int a = (int)(e - row * r);
  double *rp = rec + (size_t)row * recd;
  rp[a] = val[e];
  ((int *)(rp + r))[a] = ell_idx[e];
}

// WIN: the wave owns the columns [w0, w0 + wn) of row j1 only (window blockIdx.y); products for other windows are skipped.
// LPR: lanes per row, 0 for r itself.  order: the column of workgroup blockIdx.x, or nullptr for blockIdx.x itself.
// REC: a visit reads the row's 128-byte-aligned record (gram_pack_kernel) instead of the ELL arrays.
template <int LPR, bool WIN, bool REC>
__global__ __launch_bounds__(64) void gram_kernel(const int *__restrict__ ell_idx, const double *__restrict__ val,
                                                  int s, int r, double inv_r, const int *__restrict__ colptr,
                                                  const int *__restrict__ pos, double *__restrict__ G, int ldg, int wmax,
                                                  const int *__restrict__ order, const double *__restrict__ rec, int recd) {
  extern __shared__ double acc[];
  // groups in flight: 3 loads each + 2 of positions stay below the 63 vector loads a wave can have outstanding.  Eleven
  // groups of six rows are the 64 positions of a step at r = 10 (groups beyond a step's positions load for nothing).
  constexpr int GF = LPR ? 16 : 11;
  const int lane = threadIdx.x;
  const int j1 = order ? order[blockIdx.x] : (int)blockIdx.x;
  const int w0 = WIN ? (int)blockIdx.y * wmax : 0;
  const int wn = WIN ? ((s - w0 < wmax) ? s - w0 : wmax) : s;
  for (int j = lane; j < wn; j += 64) acc[j] = 0.0;
  __syncthreads();
  const int lpr = LPR ? LPR : r;
  const int rpg = 64 / lpr;         // rows per group
  const int sub = lane / lpr;       // which row of a group this lane serves: lane order is row order
  const int a = lane - sub * lpr;   // slot inside the row
  const bool slot_ok = a < r && sub < rpg;
  const int ac = a < r ? a : 0;
  const int p0 = colptr[j1], p1 = colptr[j1 + 1];
  if (p0 < p1) {
    const int ng = (63 + rpg) / rpg;                        // groups that 64 positions make (the last one may be partial)
    const int step = (ng <= GF) ? 64 : GF * rpg;            // positions per step: a step is at most GF groups
    auto positions = [&](int pb) { const int p = pb + lane; return pos[p < p1 ? p : p0]; };
    struct Grp { int j2; double v, vj; bool act; };
    // the group whose lanes were handed the entries `en` (0 where idle)
    auto fetch = [&](int en, bool act) {
      Grp o;
      o.act = act;
      const int ee = act ? en : 0;
      const int row = (int)(((double)ee + 0.5) * inv_r);            // == ee / r exactly for ee < 2^31, r <= 32
      if constexpr (REC) {
        const double *rp = rec + (size_t)row * recd;
        o.j2 = ((const int *)(rp + r))[ac];
        o.v = rp[ac];
        o.vj = rp[ee - row * r];
      } else {
        const size_t rowbase = (size_t)row * r;
        o.j2 = ell_idx[rowbase + ac];
        o.v = val[rowbase + ac];
        o.vj = val[ee];
      }
      return o;
    };
    // ONE ds_add_f64 per group: lanes of different rows that hit the same bin (bin j1 always, usually more) are applied
    // by the LDS unit in ascending lane order = ascending row, which is the oracle's order, and the LDS unit executes a
    // wave's instructions in program order = group order.  (Spelled as one instruction per row, the compiler merges them --
    // and with a window test in the condition it once split them in another order: 1 ulp off in 0.5 % of the entries.)
    auto apply = [&](const Grp &o) {
      const double prod = o.vj * o.v;
      const bool on = o.act && (!WIN || (unsigned)(o.j2 - w0) < (unsigned)wn);
      const int bin = on ? o.j2 - w0 : 0;
      if (on) __builtin_amdgcn_ds_atomic_fadd_f64((__attribute__((address_space(3))) double *)&acc[bin], prod);
    };
    // The loop starts a step early, with nothing to apply: the first groups are then fetched by the loop's own code, in
    // the loop's own order, and the wait counts at its head are those of the steady state.
    Grp q[GF];
#pragma unroll
    for (int u = 0; u < GF; ++u) q[u] = Grp{0, 0.0, 0.0, false};
    int e1 = positions(p0);
    asm volatile("" : "+v"(e1));    // waited for here: a load pending on entry would make the loop's first wait vmcnt(0) for good
    for (int pc = p0 - step; pc < p1; pc += step) {
      const int e2 = positions(pc + 2 * step);
      const int left = p1 - pc - step;                              // entries from the next step on
      const int cnt = left < step ? left : step;                    // (<= 0 after the last step: its fetches are all idle)
      // every group's entries in one go: the shuffles pass through the LDS unit behind the adds of the step before
      int en[GF];
#pragma unroll
      for (int u = 0; u < GF; ++u) en[u] = __shfl(e1, (u * rpg + sub) & 63, 64);
#pragma unroll
      for (int u = 0; u < GF; ++u) {
        apply(q[u]);
        q[u] = fetch(en[u], slot_ok && u * rpg + sub < cnt);
      }
      e1 = e2;
    }
  }
  __syncthreads();
  double *out = G + (size_t)j1 * ldg + w0;
  for (int j = lane; j < wn; j += 64) out[j] = acc[j];
}

// vectors(i,k) = (sum_a A(i,a) V(idx(i,a),k)) / sigma_k * scale ; sigma_k = sqrt(max(eig_k,0))
__global__ __launch_bounds__(256) void u_recover_kernel(const int *__restrict__ ell_idx,
                                                        const double *__restrict__ val, int n, int r,
                                                        const double *__restrict__ V, int ldv,
                                                        const double *__restrict__ eig, int K, double scale,
                                                        double *__restrict__ out, int ldo) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int k0 = blockIdx.y * 8;
  double acc[8];
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) acc[kk] = 0.0;
  for (int a = 0; a < r; ++a) {  // a ascending per (i,k): the oracle's order; mul then add
    const int id = ell_idx[(size_t)i * r + a];
    const double va = val[(size_t)i * r + a];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      if (k0 + kk < K) acc[kk] += va * V[(size_t)(k0 + kk) * ldv + id];
  }
#pragma unroll
  for (int kk = 0; kk < 8; ++kk) {
    const int k = k0 + kk;
    if (k < K) {
      const double ev = eig[k];
      const double sigma = __builtin_sqrt(ev > 0.0 ? ev : 0.0);
      // sigma = 0 (K reaches into the null space of A): a zero column instead of Inf / NaN; the host entry points refuse
      out[(size_t)k * ldo + i] = sigma > 0.0 ? (acc[kk] / sigma) * scale : 0.0;
    }
  }
}

// Vt(j, k) = V(j, k) stored k-contiguous: Vt[j*K + k]  (V: s x K column-major, ld = ldv)
__global__ void transpose_v_kernel(const double *__restrict__ V, int ldv, int s, int K, double *__restrict__ Vt) {
  __shared__ double t[32][33];
  const int j0 = blockIdx.x * 32, k0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 256 threads: ty 0..7
  for (int kk = ty; kk < 32; kk += 8) {
    const int j = j0 + tx, k = k0 + kk;
    t[kk][tx] = (j < s && k < K) ? V[(size_t)k * ldv + j] : 0.0;
  }
  __syncthreads();
  for (int jj = ty; jj < 32; jj += 8) {
    const int j = j0 + jj, k = k0 + tx;
    if (j < s && k < K) Vt[(size_t)j * K + k] = t[tx][jj];
  }
}

// U-recovery, gather form: a workgroup owns 64 rows x 64 eigen-columns.  Lanes run along k, so the
// r rows of Vt a point needs are read as contiguous 512-byte pieces (they come from L2: Vt is
// s*K*8 bytes); the 64 x 64 tile is turned through LDS so that the column-major output is written
// in 512-byte pieces as well.  Arithmetic as u_recover_kernel: acc = 0; acc += A(i,a) V(idx,k)
// (a ascending, mul then add); (acc / sigma_k) * scale.
#ifndef U_RECOVER_UNROLL
#define U_RECOVER_UNROLL 8
#endif
__global__ __launch_bounds__(256) void u_recover_tiled_kernel(const int *__restrict__ ell_idx,
                                                              const double *__restrict__ val, int n, int r,
                                                              const double *__restrict__ Vt,
                                                              const double *__restrict__ eig, int K, double scale,
                                                              double *__restrict__ out, int ldo) {
  __shared__ double tile[64][65];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long i0 = (long)blockIdx.x * 64;
  const int k0 = blockIdx.y * 64;
  const int k = k0 + lane;
  const bool kok = k < K;
  double sigma = 1.0;
  if (kok) { const double ev = eig[k]; sigma = __builtin_sqrt(ev > 0.0 ? ev : 0.0); }
  // UR rows in flight per wave: their UR r gathers are issued before the first one is consumed
  constexpr int UR = U_RECOVER_UNROLL;
  const double inv_guard = kok ? 1.0 : 0.0;
  const int kk = kok ? k : 0;
  for (int il = wave * 16; il < wave * 16 + 16; il += UR) {
    double acc[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u) acc[u] = 0.0;
    for (int a = 0; a < r; ++a) {
      double v[UR], z[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const long i = (i0 + il + u < n) ? i0 + il + u : n - 1;   // wave-uniform: scalar loads
        z[u] = val[(size_t)i * r + a];
        v[u] = Vt[(size_t)ell_idx[(size_t)i * r + a] * K + kk];
      }
#pragma unroll
      for (int u = 0; u < UR; ++u) acc[u] += z[u] * v[u];
    }
#pragma unroll
    for (int u = 0; u < UR; ++u) tile[lane][il + u] = sigma > 0.0 ? ((acc[u] * inv_guard) / sigma) * scale : 0.0;
  }
  __syncthreads();
  const int i = tid & 63;
  if (i0 + i < n)
    for (int kq = tid >> 6; kq < 64; kq += 4)
      if (k0 + kq < K) out[(size_t)(k0 + kq) * ldo + i0 + i] = tile[kq][i];
}

// The same with KPL eigen-columns per lane (64 KPL per workgroup; K a multiple of KPL): a row of Vt is K * 8 contiguous
// bytes, so one 8 KPL-byte load per lane takes 512 KPL bytes of it -- 1 / KPL as many gather instructions as the
// 64-column kernel, and K = 200 is two column tiles at KPL = 2 (128 + 72) or one at KPL = 4 instead of four
// (64 + 64 + 64 + 8, the last one all overhead).  ROWS rows per workgroup (a quarter per wave).
template <int KPL, int ROWS>
__global__ __launch_bounds__(256) void u_recover_wide_kernel(const int *__restrict__ ell_idx,
                                                             const double *__restrict__ val, int n, int r,
                                                             const double *__restrict__ Vt,
                                                             const double *__restrict__ eig, int K, double scale,
                                                             double *__restrict__ out, int ldo) {
  typedef double vec_t __attribute__((ext_vector_type(KPL)));
  constexpr int KT = 64 * KPL, RPW = ROWS / 4;
  constexpr int UR = (RPW < U_RECOVER_UNROLL) ? RPW : U_RECOVER_UNROLL;
  __shared__ double tile[KT][ROWS + 1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long i0 = (long)blockIdx.x * ROWS;
  const int k0 = blockIdx.y * KT;
  const int k = k0 + KPL * lane;
  const bool kok = k < K;                  // K % KPL == 0: a lane's columns are in or out together
  double sg[KPL];
#pragma unroll
  for (int c = 0; c < KPL; ++c) { const double e = kok ? eig[k + c] : 1.0; sg[c] = __builtin_sqrt(e > 0.0 ? e : 0.0); }
  const double inv_guard = kok ? 1.0 : 0.0;
  const int kk = kok ? k : 0;
  for (int il = wave * RPW; il < wave * RPW + RPW; il += UR) {
    vec_t acc[UR];
#pragma unroll
    for (int u = 0; u < UR; ++u)
#pragma unroll
      for (int c = 0; c < KPL; ++c) acc[u][c] = 0.0;
    for (int a = 0; a < r; ++a) {
      vec_t v[UR];
      double z[UR];
#pragma unroll
      for (int u = 0; u < UR; ++u) {
        const long i = (i0 + il + u < n) ? i0 + il + u : n - 1;   // wave-uniform: scalar loads
        z[u] = val[(size_t)i * r + a];
        v[u] = *(const vec_t *)(Vt + (size_t)ell_idx[(size_t)i * r + a] * K + kk);
      }
#pragma unroll
      for (int u = 0; u < UR; ++u)
#pragma unroll
        for (int c = 0; c < KPL; ++c) acc[u][c] += z[u] * v[u][c];
    }
#pragma unroll
    for (int u = 0; u < UR; ++u)
#pragma unroll
      for (int c = 0; c < KPL; ++c)
        tile[KPL * lane + c][il + u] = sg[c] > 0.0 ? ((acc[u][c] * inv_guard) / sg[c]) * scale : 0.0;
  }
  __syncthreads();
  for (int e = tid; e < KT * ROWS; e += 256) {
    const int kq = e / ROWS, i = e % ROWS;
    if (k0 + kq < K && i0 + i < n) out[(size_t)(k0 + kq) * ldo + i0 + i] = tile[kq][i];
  }
}

// ----------------------------------------------------------------------------------------
// U-recovery from an LDS-resident column slice.  The kernels above gather the r rows of Vt a point needs from L2 (and, Vt being
// s K 8 bytes against 4 MB of L2 per XCD, from the Infinity Cache): n r K 8 bytes of 32-byte pieces.  Rows share no anchors
// with their neighbours, so they cannot be staged by rows -- but W eigen-columns of ALL s anchors are s W 8 bytes, and W = 4
// fits the 163840 bytes of LDS a workgroup may declare up to s = 5120.  A workgroup keeps one such slice, walks a range of
// rows with lane = row, gathers from LDS and writes its W output columns in 512-byte pieces; idx / val are streamed once
// per slice instead (K / W times 12 n r bytes, from L2 where the workgroups of an XCD walk the same rows).
// Arithmetic as u_recover_kernel: acc = 0; acc += A(i,a) V(idx,k) (a ascending, mul then add); (acc / sigma_k) * scale.
// ----------------------------------------------------------------------------------------
#ifndef U_RECOVER_LDS_THREADS
#define U_RECOVER_LDS_THREADS 1024
#endif
#ifndef U_RECOVER_LDS_MIN_N           // rows from which the LDS kernel is the faster one (DESIGN.md section 4 has the measurements)
#define U_RECOVER_LDS_MIN_N 10000
#endif
constexpr int U_LDS_BYTES = 163840;
// flgp_dev_hk_rows_route: the K W / r from which the heat-kernel rows take over from the MFMA contraction -- against
// hk_panel2_kernel (m >= 480) and against hk_panel_kernel (100 <= m < 480; no smaller m was measured)
constexpr int HK_ROWS_MIN_KW_PER_R = 60, HK_ROWS_MIN_KW_PER_R_SMALL_M = 40, HK_ROWS_PANEL2_M = 480, HK_ROWS_MIN_M = 100;

// eigen-columns per slice: min(4, floor(163840 / (8 s))); 0 = not even one column fits
static int u_lds_width(int s) {
  const long w = s >= 1 ? (long)U_LDS_BYTES / (8L * s) : 0;
  return w > 4 ? 4 : (int)w;
}

// pairs per step of u_recover_lds_kernel: a row is ceil(r / 2) pairs, walked in the fewest steps of at most U_LDS_MAX_PAIRS,
// all of one size: one step up to r = 12, two steps of 4..6 pairs up to r = 24, three of 5 or 6 up to r = 32.  At most two
// pairs, in the row's last step, are loaded for nothing.  (Seven and eight pairs in two buffers spill at four eigen-columns.)
constexpr int U_LDS_MAX_PAIRS = 6;
static int u_lds_pairs(int r) {
  const int pairs = (r + 1) / 2, steps = ceil_div(pairs, U_LDS_MAX_PAIRS);
  return ceil_div(pairs, steps);
}

// ----------------------------------------------------------------------------------------
// Wave tiles of the ELL rows: what a wave of u_recover_lds_kernel (lane = row) loads in one instruction, stored contiguously.
// Tile T holds rows 64 T .. 64 T + 63: PT x 64 value pairs of 16 bytes, pair p of lane l at (p 64 + l) 16, then PT x 64 index
// pairs of 8 bytes in the same order; pair p of a row is its entries 2 p and 2 p + 1, and PT = steps x u_lds_pairs(r) is the
// number of pair slots the row kernel loads per row (5 at r = 10, 8 at r = 13, 15 at r = 25).  A tile is PT 1536 bytes, so every
// tile starts on a 128-byte edge.  Slots past r and rows past n hold value 0.0 and index 0: they are loaded (every load is
// unconditional and in bounds) and never summed.  A wave's load is then one coalesced 1 KB (values) or 512 B (indices) request:
// 8 + 4 cache lines where the row-major arrays (80-byte and 40-byte stride at r = 10) give 40 + 20.
// ----------------------------------------------------------------------------------------
static int row_tile_pairs(int r) { return ceil_div((r + 1) / 2, U_LDS_MAX_PAIRS) * u_lds_pairs(r); }
constexpr int ROW_TILE_PAIR_BYTES = 64 * (16 + 8);
// one thread per (tile, pair slot, lane): strided reads (it runs once per step), 1 KB / 512 B coalesced writes per wave
__global__ __launch_bounds__(256) void row_tiles_pack_kernel(const int *__restrict__ ell_idx, const double *__restrict__ val, int n,
                                                             int r, int pt, long slots, char *__restrict__ tiles) {
  typedef double d2 __attribute__((ext_vector_type(2)));
  typedef int i2 __attribute__((ext_vector_type(2)));
  const long g = (long)blockIdx.x * 256 + threadIdx.x;       // (tile pt + p) 64 + lane
  if (g >= slots) return;
  const int lane = (int)(g & 63);
  const long tp = g >> 6, tile = tp / pt;
  const int p = (int)(tp - tile * pt);
  const long row = tile * 64 + lane;
  d2 z = {0.0, 0.0};
  i2 j = {0, 0};
  if (row < n) {
    const long b = row * r + 2 * p;
    if (2 * p < r) { z[0] = val[b]; j[0] = ell_idx[b]; }
    if (2 * p + 1 < r) { z[1] = val[b + 1]; j[1] = ell_idx[b + 1]; }
  }
  char *tb = tiles + (size_t)tile * pt * ROW_TILE_PAIR_BYTES;
  ((d2 *)tb)[p * 64 + lane] = z;
  ((i2 *)(tb + (size_t)pt * 1024))[p * 64 + lane] = j;
}

// Vts[slice][j][c] = V(j, slice W + c), columns past K zero: the image a workgroup of u_recover_lds_kernel copies into LDS
template <int W>
__global__ __launch_bounds__(256) void transpose_v_slices_kernel(const double *__restrict__ V, int ldv, int s, int K,
                                                                 double *__restrict__ Vts) {
  const int j = blockIdx.x * 256 + threadIdx.x, sl = blockIdx.y;
  if (j >= s) return;
  double *o = Vts + ((size_t)sl * s + j) * W;
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const int k = sl * W + c;
    o[c] = k < K ? V[(size_t)k * ldv + j] : 0.0;
  }
}

// where double q of a slice sits in LDS.  W = 4: an anchor is two 16-byte halves and a ds_read_b128 of "the first half" of 16
// random anchors would use the even ones of the 16 slots of a bank row only; bit 3 of the anchor swaps its halves.
template <int W> __device__ __forceinline__ int u_lds_slot(int q) { return W == 4 ? q ^ (((q >> 5) & 1) << 1) : q; }

// NP: pairs of entries per step (u_lds_pairs above: the fewest equal steps of at most six pairs that cover a row).
// RAW: the sums are stored as they are, out(i, k) = sum_a val(i, a) M(idx(i, a), k), and eig / scale are not read (the heat-kernel
// rows of flgp_dev_hk_rows, where M is the s x m matrix Wm and the scaling is already inside it).
// TIL: the rows come from their wave tiles (row_tiles_pack_kernel), passed as `val`; ell_idx is not read.  Only the loads
// differ: the same values and indices reach the same sums in the same order.
template <int W, int NP, bool RAW, bool TIL>
__global__ __launch_bounds__(U_RECOVER_LDS_THREADS) void u_recover_lds_kernel(const int *__restrict__ ell_idx,
                                                                              const double *__restrict__ val, int n, int r, int s,
                                                                              const double *__restrict__ Vts,
                                                                              const double *__restrict__ eig, int K, double scale,
                                                                              double *__restrict__ out, int ldo, int rows_per_range) {
  typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));   // a row starts on 8 bytes (values) / 4 (indices)
  typedef int i2u __attribute__((ext_vector_type(2), aligned(4)));
  typedef double d2 __attribute__((ext_vector_type(2)));
  extern __shared__ __attribute__((aligned(16))) double u_slice[];
  const int tid = threadIdx.x, T = blockDim.x, sl = blockIdx.y;
  const double *src = Vts + (size_t)sl * s * W;
  for (int q = tid; q < s * W; q += T) u_slice[u_lds_slot<W>(q)] = src[q];
  double sg[W];
#pragma unroll
  for (int c = 0; c < W; ++c) {
    const int k = sl * W + c;
    const double e = (!RAW && k < K) ? eig[k] : 0.0;
    sg[c] = __builtin_sqrt(e > 0.0 ? e : 0.0);
    if constexpr (TIL && !RAW) {          // the same in every lane: kept in scalar registers, it leaves the loop its 128 VGPRs
      sg[c] = __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(sg[c])),
                               __builtin_amdgcn_readfirstlane(__double2loint(sg[c])));
    }
  }
  __syncthreads();
  const long i_lo = (long)blockIdx.x * rows_per_range;
  const long i_hi = (i_lo + rows_per_range < n) ? i_lo + rows_per_range : n;
  const long last_pair = (long)n * r - 2;       // (n r >= 2: the route rule)
  // A step is CE = 2 NP entries of a row as NP pairs: a 16-byte load of values and an 8-byte load of indices per lane, the
  // pair starting at the even slot a of row i.  NP is cut to the row (five pairs, one step at r = 10): with steps of eight
  // entries whatever r, the second step of a row of ten issued three of its four pairs for nothing and took the ragged path.
  // The pair of an odd r's last slot reaches into the next row, and in the last row of all it is moved back by one (`up` below).  Loads are unconditional, so that the number in flight is the same on every path and
  // the wait counts stay tight; what a lane has no use for (past its row, past its range) is read from ONE address, the
  // range's first entry, which costs the cache a single line look-up.
  constexpr int CE = 2 * NP;
  // gathers issued ahead of their sums: the whole step up to four pairs, half of it beyond (a third at W = 4, NP = 6) --
  // the most for which two buffers and the gathered anchors stay inside the 128 VGPRs of a 1024-thread workgroup
  constexpr int GB = NP <= 4 ? CE : (W == 4 && NP == 6) ? 4 : NP;
  struct Chunk { double z0[NP], z1[NP]; int j0[NP], j1[NP]; };
  // TIL: a wave's 64 rows are one tile (ranges are whole waves of rows), so the base is uniform and a pair is one 16-byte and
  // one 8-byte load at base + lane x size + a constant; a wave whose rows all lie past the range re-reads the range's first
  // tile.  No pair reaches into the next row, so nothing is ever `moved`.
  typedef int i2 __attribute__((ext_vector_type(2)));
  const int pt = (((r + 1) / 2 + U_LDS_MAX_PAIRS - 1) / U_LDS_MAX_PAIRS) * NP;       // row_tile_pairs(r)
  const int lane = tid & 63, wave0 = __builtin_amdgcn_readfirstlane(tid & ~63);
  // row i = i_lo + tid + rd T of chunk ch (rd, the round, only so that the tile's address is built from uniform values alone)
  auto fetch = [&](long i, int ch, int rd) {
    Chunk c;
    if constexpr (TIL) {
      const int w0 = (int)i_lo + wave0 + rd * T;                       // the wave's first row
      const int tile = (w0 < (int)i_hi ? w0 : (int)i_lo) >> 6;
      // scalar bases, set 2 KB into the step's values so that every pair's constant fits the load's signed 13-bit offset
      typedef const __attribute__((address_space(1))) char *gbytes;
      typedef const __attribute__((address_space(1))) d2 *gd2;
      typedef const __attribute__((address_space(1))) i2 *gi2;
      const size_t tb = (size_t)val + (size_t)tile * (size_t)(pt * ROW_TILE_PAIR_BYTES);
      size_t zb = tb + (ch * (NP * 1024) + 2048);
      size_t jb = tb + (pt * 1024 + ch * (NP * 512));
      asm("" : "+s"(zb), "+s"(jb));       // the bases stay scalar: left to itself, the loop carries per-lane 64-bit addresses
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const d2 z = *(gd2)((gbytes)zb + (size_t)(unsigned)(lane * 16) + (u * 1024 - 2048));
        const i2 j = *(gi2)((gbytes)jb + (size_t)(unsigned)(lane * 8) + u * 512);
        c.z0[u] = z[0]; c.z1[u] = z[1];
        c.j0[u] = j[0]; c.j1[u] = j[1];
      }
    } else {
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const int a = CE * ch + 2 * u;
        long b = (i < i_hi && a < r) ? i * r + a : i_lo * r;
        b = b < last_pair ? b : last_pair;
        const d2u z = *(const d2u *)(val + b);
        const i2u j = *(const i2u *)(ell_idx + b);
        c.z0[u] = z[0]; c.z1[u] = z[1];
        c.j0[u] = j[0]; c.j1[u] = j[1];
      }
    }
    return c;
  };
  // one entry of a chunk, slot a = CE ch + 2 u + h of row i: its value and the W doubles of its anchor
  auto gather = [&](const Chunk &cur, int u, int h, bool moved, double &z, double (&v)[W]) {
    const bool up = h || moved;
    const int id = up ? cur.j1[u] : cur.j0[u];
    z = up ? cur.z1[u] : cur.z0[u];
    if constexpr (W == 4) {
      const int x = ((id >> 3) & 1) << 1;
      const d2 lo = *(const d2 *)&u_slice[id * 4 + x], hi = *(const d2 *)&u_slice[id * 4 + (x ^ 2)];
      v[0] = lo[0]; v[1] = lo[1]; v[2] = hi[0]; v[3] = hi[1];
    } else if constexpr (W == 2) {
      const d2 lo = *(const d2 *)&u_slice[id * 2];
      v[0] = lo[0]; v[1] = lo[1];
    } else {
#pragma unroll
      for (int c = 0; c < W; ++c) v[c] = u_slice[id * W + c];
    }
  };
  double acc[W];
#pragma unroll
  for (int c = 0; c < W; ++c) acc[c] = 0.0;
  const int nch = (r + CE - 1) / CE;
  // chunk ch of row i: its entries in ascending order; behind the row's last chunk the W results are stored
  auto apply = [&](const Chunk &cur, long i, int ch) {
    const int left = r - ch * CE;
    if (left >= CE) {                                                  // (uniform) a whole chunk: GB gathers, then their sums
#pragma unroll
      for (int e0 = 0; e0 < CE; e0 += GB) {
        double z[GB], v[GB][W];
#pragma unroll
        for (int e = e0; e < e0 + GB && e < CE; ++e)                     // (an entry follows every pair: none moved)
          gather(cur, e >> 1, e & 1, false, z[e - e0], v[e - e0]);
#pragma unroll
        for (int e = e0; e < e0 + GB && e < CE; ++e)
#pragma unroll
          for (int c = 0; c < W; ++c) acc[c] += z[e - e0] * v[e - e0][c];
      }
    } else {
#pragma unroll
      for (int u = 0; u < NP; ++u) {
        const bool moved = !TIL && i * r + ch * CE + 2 * u > last_pair; // only the last slot of the last row, r odd
#pragma unroll
        for (int h = 0; h < 2; ++h)
          if (2 * u + h < left) {
            double z, v[W];
            gather(cur, u, h, moved, z, v);
#pragma unroll
            for (int c = 0; c < W; ++c) acc[c] += z * v[c];
          }
      }
    }
    if (ch == nch - 1) {
      if (i < i_hi) {
#pragma unroll
        for (int c = 0; c < W; ++c) {
          const int k = sl * W + c;
          if (k < K) out[(size_t)k * ldo + i] = RAW ? acc[c] : sg[c] > 0.0 ? (acc[c] / sg[c]) * scale : 0.0;
        }
      }
#pragma unroll
      for (int c = 0; c < W; ++c) acc[c] = 0.0;
    }
  };
  // The (row, chunk) steps of a lane in order, two buffers: the loads of step t + 1 fly while step t is applied.  (One buffer
  // handed on at the end of the step would wait for them at the hand-over.)
  const long nit = i_hi > i_lo ? (i_hi - i_lo + T - 1) / T : 0;
  const long steps = nit * nch;
  long ia = i_lo + tid; int cha = 0, rda = 0;                          // step t
  auto next = [&](long &i, int &ch, int &rd) { if (++ch == nch) { ch = 0; i += T; ++rd; } };
  Chunk A = fetch(ia, cha, rda), B;
  for (long t = 0; t < steps; t += 2) {
    long ib = ia; int chb = cha, rdb = rda; next(ib, chb, rdb);        // step t + 1 (past the last step: masked loads)
    B = fetch(ib, chb, rdb);
    apply(A, ia, cha);
    ia = ib; cha = chb; rda = rdb; next(ia, cha, rda);
    A = fetch(ia, cha, rda);
    if (t + 1 < steps) apply(B, ib, chb);
  }
}

__global__ void values_out_kernel(const double *__restrict__ eig, int K, int root, double *__restrict__ values) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= K) return;
  const double ev = eig[k] > 0.0 ? eig[k] : 0.0;
  values[k] = root ? __builtin_sqrt(ev) : ev;   // values = d^2 (src/TruncatedSVD.cpp:29), sqrt if root (src/Spectrum.cpp:153-155)
}

// B(j, k) = Vs(j, k) q_k with q_k = scale / sigma_k, sigma_k = sqrt(max(eig_k, 0)), and q_k = 0 where sigma_k = 0 (the zero
// column of U-recovery); B is s x K column-major with leading dimension s
__global__ void hk_rows_b_kernel(const double *__restrict__ Vs, int ldv, int s, const double *__restrict__ eig, int K,
                                 double scale, double *__restrict__ B) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)s * K) return;
  const int j = (int)(e % s), k = (int)(e / s);
  const double ev = eig[k];
  const double sigma = __builtin_sqrt(ev > 0.0 ? ev : 0.0);
  const double q = sigma > 0.0 ? scale / sigma : 0.0;
  B[e] = Vs[(size_t)k * ldv + j] * q;
}

int hk_rows_b(hipStream_t st, const double *dVs, int ldv, int s, const double *d_eig, int K, double scale, double *dB) {
  hipLaunchKernelGGL(hk_rows_b_kernel, dim3(ceil_div((long)s * K, 256)), dim3(256), 0, st, dVs, ldv, s, d_eig, K, scale, dB);
  return check_launch("hk_rows_b_kernel");
}

struct CscPlan {
  int nchunks, chunk, nbits;
  size_t hist_bytes, tot_bytes;
};

static CscPlan csc_plan(long nnz, int s) {
  CscPlan p;
  long nc = (nnz + 2047) / 2048;
  if (nc > 2048) nc = 2048;
  if (nc < 1) nc = 1;
  long chunk = (nnz + nc - 1) / nc;
  chunk = (chunk + 63) / 64 * 64;
  if (chunk < 64) chunk = 64;
  p.chunk = (int)chunk;
  p.nchunks = (int)((nnz + chunk - 1) / chunk);
  if (p.nchunks < 1) p.nchunks = 1;
  p.nbits = 1;
  while ((1 << p.nbits) < s) ++p.nbits;
  p.hist_bytes = sizeof(int) * (size_t)p.nchunks * s;
  p.tot_bytes = sizeof(int) * (size_t)s;
  return p;
}

}  // namespace flgp

using namespace flgp;

extern "C" size_t flgp_dev_csc_workspace(int n, int s, int r) {
  const CscPlan p = csc_plan((long)n * r, s);
  return p.hist_bytes + p.tot_bytes + 256;
}

extern "C" int flgp_dev_csc_build(void *stream, const int *d_ell_idx, int n, int s, int r, int *d_colptr,
                                  int *d_pos, void *d_work, size_t work_bytes) {
  hipStream_t st = (hipStream_t)stream;
  const long nnz = (long)n * r;
  FLGP_REQUIRE(nnz < 2147483647L, "CSC: n*r = %ld does not fit int32 positions", nnz);
  FLGP_REQUIRE(s >= 1 && s <= FLGP_SMAX, "CSC: kernels are built for s <= %d (got %d)", FLGP_SMAX, s);
  FLGP_REQUIRE(work_bytes >= flgp_dev_csc_workspace(n, s, r), "CSC: workspace too small");
  const CscPlan p = csc_plan(nnz, s);
  int *hist = (int *)d_work;
  int *tot = (int *)((char *)d_work + p.hist_bytes);
  const size_t lds = sizeof(int) * (size_t)s;
  if (lds > 48 * 1024) {
    FLGP_HIP(hipFuncSetAttribute((const void *)csc_hist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    FLGP_HIP(hipFuncSetAttribute((const void *)csc_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  ProfScope ps("csc_build", st, 12.0 * (double)nnz);
  hipLaunchKernelGGL(csc_hist_kernel, dim3(p.nchunks), dim3(256), lds, st, d_ell_idx, nnz, s, p.chunk, hist);
  FLGP_TRY(check_launch("csc_hist_kernel"));
  hipLaunchKernelGGL(csc_colscan_kernel, dim3(ceil_div(s, 256)), dim3(256), 0, st, hist, p.nchunks, s, tot);
  FLGP_TRY(check_launch("csc_colscan_kernel"));
  hipLaunchKernelGGL(csc_scan_kernel, dim3(1), dim3(1024), 0, st, tot, s, d_colptr);
  FLGP_TRY(check_launch("csc_scan_kernel"));
  hipLaunchKernelGGL(csc_scatter_kernel, dim3(p.nchunks), dim3(64), lds, st, d_ell_idx, nnz, s, p.chunk, p.nbits,
                     hist, d_colptr, d_pos);
  return check_launch("csc_scatter_kernel");
}

// columns of a per-column table of doubles that one workgroup keeps in LDS: all s of them up to 20000 (what rounds 1-3 were
// built for), windows of 16384 beyond (the kernels then walk their input once per window)
static int lds_window(int s) {
  const int forced = tuning("sparse_window", 0);      // tests: windows on small inputs
  if (forced > 0 && forced < s) return forced;
  return s <= 20000 ? s : 16384;
}

extern "C" size_t flgp_dev_colsum_workspace(int n, int s) {
  return sizeof(double) * (size_t)ceil_div(n > 0 ? n : 1, COLSUM_CHUNK) * (size_t)s + 256;
}

extern "C" int flgp_dev_colsum(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, int s,
                               double *d_colsum, void *d_work, size_t work_bytes) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(n >= 0 && r >= 1 && s >= 1 && s <= FLGP_SMAX, "colsum: need 1 <= s <= %d (got %d)", FLGP_SMAX, s);
  FLGP_REQUIRE(work_bytes >= flgp_dev_colsum_workspace(n, s), "colsum: workspace too small");
  const int nchunks = ceil_div(n > 0 ? n : 1, COLSUM_CHUNK);
  int nbits = 1;
  while ((1 << nbits) < s) ++nbits;
  const int wmax = lds_window(s);                    // s itself while a table of s doubles fits LDS
  const size_t lds = sizeof(double) * (size_t)wmax;
  const void *fn = wmax < s ? (const void *)colsum_chunk_kernel<true> : (const void *)colsum_chunk_kernel<false>;
  if (lds > 48 * 1024) FLGP_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  ProfScope ps("colsum_kernel", st, 12.0 * (double)n * r);
  if (wmax < s)
    hipLaunchKernelGGL(colsum_chunk_kernel<true>, dim3(nchunks, ceil_div(s, wmax)), dim3(64), lds, st, d_ell_idx, d_ell_val, n, r, s,
                       nbits, (double *)d_work, wmax, tuning("colsum_direct", 1));
  else
    hipLaunchKernelGGL(colsum_chunk_kernel<false>, dim3(nchunks), dim3(64), lds, st, d_ell_idx, d_ell_val, n, r, s, nbits,
                       (double *)d_work, wmax, tuning("colsum_direct", 1));
  FLGP_TRY(check_launch("colsum_chunk_kernel"));
  hipLaunchKernelGGL(colsum_reduce_kernel, dim3(ceil_div(s, 64)), dim3(64), 0, st, (const double *)d_work, nchunks, s, d_colsum);
  return check_launch("colsum_reduce_kernel");
}

extern "C" int flgp_dev_col_scale(void *stream, const int *d_ell_idx, double *d_ell_val, int n, int r,
                                  const double *d_colsum, const double *d_num_class, int mode) {
  FLGP_REQUIRE(mode == 0 || mode == 1, "col_scale: mode must be 0 or 1");
  const long nnz = (long)n * r;
  if (nnz == 0) return FLGP_OK;
  hipLaunchKernelGGL(col_scale_kernel, dim3(ceil_div(nnz, 256)), dim3(256), 0, (hipStream_t)stream, d_ell_idx,
                     d_ell_val, nnz, d_colsum, d_num_class, mode);
  return check_launch("col_scale_kernel");
}

extern "C" int flgp_dev_row_normalize(void *stream, double *d_ell_val, int n, int r) {
  if (n == 0) return FLGP_OK;
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX, "row_normalize: r = %d outside 1..%d", r, FLGP_RMAX);
  const size_t lds = sizeof(double) * 256 * (size_t)r;
  if (lds > 48 * 1024)
    FLGP_HIP(hipFuncSetAttribute((const void *)row_normalize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(row_normalize_kernel, dim3(ceil_div(n, 256)), dim3(256), lds, (hipStream_t)stream, d_ell_val,
                     n, r);
  return check_launch("row_normalize_kernel");
}

// graphLaplacian_cpp's column scaling and row normalisation in one pass over the values (reference src/Utils.cpp:199-211):
// the same operations per entry as flgp_dev_col_scale(mode 0) followed by flgp_dev_row_normalize, the same bits
extern "C" int flgp_dev_col_scale_row_normalize(void *stream, const int *d_ell_idx, double *d_ell_val, int n, int r,
                                                const double *d_colsum, const double *d_num_class) {
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && d_ell_idx && d_ell_val && d_colsum, "col_scale_row_normalize: bad arguments");
  if (n == 0) return FLGP_OK;
  const size_t lds = sizeof(double) * 256 * (size_t)r;
  if (lds > 48 * 1024)
    FLGP_HIP(hipFuncSetAttribute((const void *)row_normalize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(row_normalize_kernel, dim3(ceil_div(n, 256)), dim3(256), lds, (hipStream_t)stream, d_ell_val, n, r, d_ell_idx,
                     d_colsum, d_num_class);
  return check_launch("row_normalize_kernel");
}

// the extension's three scalings in one pass (extend_scale_kernel): the bits of flgp_dev_col_scale(mode 0) ->
// flgp_dev_row_normalize -> flgp_dev_col_scale(mode 1) under the given column sums
extern "C" int flgp_dev_extend_scale(void *stream, const int *d_ell_idx, double *d_ell_val, int n, int r,
                                     const double *d_colsum_gl, const double *d_num_class, const double *d_colsum_spectrum) {
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && n >= 0 && d_ell_idx && d_ell_val && d_colsum_spectrum, "extend_scale: bad arguments");
  if (n == 0) return FLGP_OK;
  const size_t lds = sizeof(double) * 256 * (size_t)r;
  if (lds > 48 * 1024)
    FLGP_HIP(hipFuncSetAttribute((const void *)extend_scale_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(extend_scale_kernel, dim3(ceil_div(n, 256)), dim3(256), lds, (hipStream_t)stream, d_ell_idx, d_ell_val, n, r,
                     d_colsum_gl, d_num_class, d_colsum_spectrum);
  return check_launch("extend_scale_kernel");
}

extern "C" int flgp_dev_gram_order(void *stream, const int *d_colptr, int s, int *d_order) {
  FLGP_REQUIRE(s >= 1 && s <= FLGP_SMAX && d_colptr && d_order, "Gram order: need 1 <= s <= %d (got %d) and both arrays", FLGP_SMAX, s);
  hipLaunchKernelGGL(gram_order_kernel, dim3(ceil_div(s, 64)), dim3(64 * ORDER_WAVES), 0, (hipStream_t)stream, d_colptr, s, d_order);
  return check_launch("gram_order_kernel");
}

extern "C" size_t flgp_dev_gram_record_bytes(int n, int r) {
  return sizeof(double) * (size_t)(n > 0 ? n : 0) * (size_t)gram_record_doubles(r > 0 ? r : 1) + 256;
}

// Do the records pay?  Where one workgroup holds the whole row of G (no windows): 0.505 -> 0.288 ms for a pack of 0.041 ms
// at the flagship shape; with two windows of s = 20 500 every row is visited twice as often and the kernel is bound
// elsewhere (3.40 -> 3.44 ms).
extern "C" int flgp_dev_gram_uses_records(int s, int r) {
  return s >= 1 && s <= FLGP_SMAX && r >= 1 && r <= FLGP_RMAX && lds_window(s) >= s;
}

extern "C" int flgp_dev_gram_pack(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, double *d_rec) {
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && n >= 0 && d_rec, "Gram records: bad arguments");
  FLGP_REQUIRE(((size_t)d_rec & 127) == 0, "Gram records: the buffer must be 128-byte aligned");
  const long nnz = (long)n * r;
  if (nnz == 0) return FLGP_OK;
  hipLaunchKernelGGL(gram_pack_kernel, dim3(ceil_div(nnz, 256)), dim3(256), 0, (hipStream_t)stream, d_ell_idx, d_ell_val, nnz, r,
                     1.0 / (double)r, gram_record_doubles(r), d_rec);
  return check_launch("gram_pack_kernel");
}

// d_order: flgp_dev_gram_order's list (any permutation of the columns gives the same G), or NULL.  d_rec: the records of
// flgp_dev_gram_pack for these ELL arrays, or NULL to read the arrays themselves.
extern "C" int flgp_dev_gram_ordered(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int s, int r,
                                     const int *d_colptr, const int *d_pos, const int *d_order, const double *d_rec,
                                     double *dG, int ldg) {
  (void)n;
  FLGP_REQUIRE(s >= 1 && s <= FLGP_SMAX, "Gram: need 1 <= s <= %d (got %d)", FLGP_SMAX, s);
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && ldg >= s, "Gram: bad r / ldg");
  const int wmax = lds_window(s);
  const size_t lds = sizeof(double) * (size_t)wmax;
  const bool win = wmax < s;
  // lanes per row: r itself where that puts more rows into a group than the power-of-two packing does (r <= 12, 17..21)
  const int lpr = (64 / r > (r <= 16 ? 4 : 2)) ? 0 : (r <= 16 ? 16 : 32);
  const bool recs = d_rec != nullptr;
  const int recd = gram_record_doubles(r);
  ProfScope ps("gram_kernel", (hipStream_t)stream, 12.0 * (double)n * r + 8.0 * (double)s * s);
  const dim3 grid(s, win ? ceil_div(s, wmax) : 1);
#define GRAM_LAUNCH3(LPRv, WINv, RECv)                                                                                         \
  do {                                                                                                                         \
    if (lds > 48 * 1024)                                                                                                       \
      FLGP_HIP(hipFuncSetAttribute((const void *)gram_kernel<LPRv, WINv, RECv>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                                   (int)lds));                                                                                 \
    hipLaunchKernelGGL((gram_kernel<LPRv, WINv, RECv>), grid, dim3(64), lds, (hipStream_t)stream, d_ell_idx, d_ell_val, s, r,  \
                       1.0 / (double)r, d_colptr, d_pos, dG, ldg, wmax, d_order, d_rec, recd);                                 \
  } while (0)
#define GRAM_LAUNCH(LPRv, WINv) do { if (recs) GRAM_LAUNCH3(LPRv, WINv, true); else GRAM_LAUNCH3(LPRv, WINv, false); } while (0)
  if (lpr == 0) { if (win) GRAM_LAUNCH(0, true); else GRAM_LAUNCH(0, false); }
  else if (lpr == 16) { if (win) GRAM_LAUNCH(16, true); else GRAM_LAUNCH(16, false); }
  else { if (win) GRAM_LAUNCH(32, true); else GRAM_LAUNCH(32, false); }
#undef GRAM_LAUNCH
#undef GRAM_LAUNCH3
  return check_launch("gram_kernel");
}

extern "C" int flgp_dev_gram(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int s, int r,
                             const int *d_colptr, const int *d_pos, double *dG, int ldg) {
  return flgp_dev_gram_ordered(stream, d_ell_idx, d_ell_val, n, s, r, d_colptr, d_pos, nullptr, nullptr, dG, ldg);
}

// ---- upper triangle of a symmetric matrix as one contiguous run (exchange 3 of the row-sharded path sends s(s+1)/2
// doubles instead of s^2; mirroring after the reduction also makes G symmetric bit for bit, which a ring all-reduce
// of the full square does not: (i,j) and (j,i) travel in different chunks and are added in different rank orders).
// Column j's rows 0..j sit at packed[j(j+1)/2 ..].
__global__ __launch_bounds__(256) void sym_pack_kernel(const double *__restrict__ G, int ldg, int s, double *__restrict__ packed) {
  const int j = blockIdx.y;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i <= j) packed[(size_t)j * (j + 1) / 2 + i] = G[(size_t)j * ldg + i];
}
// 32 x 32 tiles (ti <= tj): the upper tile is copied, its mirror image written through an LDS transpose
__global__ __launch_bounds__(256) void sym_unpack_kernel(const double *__restrict__ packed, int s, double *__restrict__ G, int ldg) {
  __shared__ double tile[32][33];
  const int ti = blockIdx.x, tj = blockIdx.y;
  if (ti > tj) return;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int c = ty; c < 32; c += 8) {
    const int i = ti * 32 + tx, j = tj * 32 + c;
    double v = 0.0;
    if (i < s && j < s) {
      v = (i <= j) ? packed[(size_t)j * (j + 1) / 2 + i] : packed[(size_t)i * (i + 1) / 2 + j];   // i > j only on diagonal tiles
      G[(size_t)j * ldg + i] = v;
    }
    tile[c][tx] = v;
  }
  __syncthreads();
  if (ti == tj) return;
  for (int c = ty; c < 32; c += 8) {
    const int i = tj * 32 + tx, j = ti * 32 + c;     // element (i, j) of the lower tile = (j, i) of the upper one
    if (i < s && j < s) G[(size_t)j * ldg + i] = tile[tx][c];
  }
}

extern "C" int flgp_dev_sym_pack(void *stream, const double *dG, int ldg, int s, double *d_packed) {
  FLGP_REQUIRE(s >= 1 && ldg >= s, "sym_pack: bad shape");
  hipLaunchKernelGGL(sym_pack_kernel, dim3(ceil_div(s, 256), s), dim3(256), 0, (hipStream_t)stream, dG, ldg, s, d_packed);
  return check_launch("sym_pack_kernel");
}
extern "C" int flgp_dev_sym_unpack(void *stream, const double *d_packed, int s, double *dG, int ldg) {
  FLGP_REQUIRE(s >= 1 && ldg >= s, "sym_unpack: bad shape");
  const int nt = ceil_div(s, 32);
  hipLaunchKernelGGL(sym_unpack_kernel, dim3(nt, nt), dim3(256), 0, (hipStream_t)stream, d_packed, s, dG, ldg);
  return check_launch("sym_unpack_kernel");
}

// the transposed V of the gather kernels (s K doubles), or the slices of the LDS kernel with the last one filled up
extern "C" size_t flgp_dev_u_recover_workspace(int s, int K) {
  const int w = u_lds_width(s);
  const size_t cols = w >= 1 && K >= 1 ? (size_t)ceil_div(K, w) * w : (size_t)(K > 0 ? K : 0);
  return sizeof(double) * (size_t)(s > 0 ? s : 0) * cols + 256;
}

// Which kernel flgp_dev_u_recover runs: 0 u_recover_kernel (no workspace), 1 tiled, 2 wide<2,64>, 3 wide<4,32>, 4 LDS slices.
// The LDS kernel needs the workspace, a slice that fits (s <= 20480) and n >= U_RECOVER_LDS_MIN_N, the smallest n at which
// it was measured against the gather kernels (and was faster, as at every larger one).
extern "C" int flgp_dev_u_recover_route(int n, int r, int s, int K, int has_work) {
  if (!has_work) return 0;
  if (u_lds_width(s) >= 1 && n >= U_RECOVER_LDS_MIN_N && (long)n * r >= 2) return 4;      // (two entries: the kernel loads pairs)
  return K % 4 == 0 ? 3 : K % 2 == 0 ? 2 : 1;
}

static int num_cus() {
  static int cus[16] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 256;
  if (!cus[dev]) {
    int c = 0;
    cus[dev] = (hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0) ? c : 256;
  }
  return cus[dev];
}

// d_tiles: the wave tiles of the rows (flgp_dev_row_tiles_pack), or NULL to read the ELL arrays themselves
template <int W, int NP, bool RAW>
static int u_recover_lds_launch(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, const void *d_tiles, int n, int r,
                                const double *dV, int ldv, int s, const double *d_eig, int K, double scale, double *d_vectors,
                                int ldo, double *d_work) {
  const int slices = ceil_div(K, W);
  hipLaunchKernelGGL((transpose_v_slices_kernel<W>), dim3(ceil_div(s, 256), slices), dim3(256), 0, st, dV, ldv, s, K, d_work);
  FLGP_TRY(check_launch("transpose_v_slices_kernel"));
  // about one workgroup per CU, one round; a range is whole waves of rows
  int ranges = num_cus() / slices;
  if (ranges < 1) ranges = 1;
  int rows = ceil_div(ceil_div(n, ranges), 64) * 64;
  ranges = ceil_div(n, rows);
  const size_t lds = sizeof(double) * (size_t)s * W;
#define U_LDS_LAUNCH(TILv, idxv, valv)                                                                                         \
  do {                                                                                                                         \
    if (lds > 48 * 1024)                                                                                                       \
      FLGP_HIP(hipFuncSetAttribute((const void *)u_recover_lds_kernel<W, NP, RAW, TILv>,                                       \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                                     \
    hipLaunchKernelGGL((u_recover_lds_kernel<W, NP, RAW, TILv>), dim3(ranges, slices), dim3(U_RECOVER_LDS_THREADS), lds, st,   \
                       idxv, valv, n, r, s, d_work, d_eig, K, scale, d_vectors, ldo, rows);                                    \
  } while (0)
  if (d_tiles) U_LDS_LAUNCH(true, (const int *)nullptr, (const double *)d_tiles);
  else U_LDS_LAUNCH(false, d_ell_idx, d_ell_val);
#undef U_LDS_LAUNCH
  return FLGP_OK;
}

template <int W, bool RAW>
static int u_recover_lds_pairs(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, const void *d_tiles, int n, int r,
                               const double *dV, int ldv, int s, const double *d_eig, int K, double scale, double *d_vectors,
                               int ldo, double *d_work) {
  switch (u_lds_pairs(r)) {
#define U_LDS_PAIRS(NPv)                                                                                                       \
  case NPv:                                                                                                                    \
    return u_recover_lds_launch<W, NPv, RAW>(st, d_ell_idx, d_ell_val, d_tiles, n, r, dV, ldv, s, d_eig, K, scale, d_vectors,  \
                                             ldo, d_work)
    U_LDS_PAIRS(1); U_LDS_PAIRS(2); U_LDS_PAIRS(3); U_LDS_PAIRS(4); U_LDS_PAIRS(5);
    default: U_LDS_PAIRS(6);
#undef U_LDS_PAIRS
  }
}

// the slice image of dV (s x K, ld = ldv) into d_work, then the LDS row kernel at the slice width of s
template <bool RAW>
static int u_recover_lds_width(hipStream_t st, const int *d_ell_idx, const double *d_ell_val, const void *d_tiles, int n, int r,
                               const double *dV, int ldv, int s, const double *d_eig, int K, double scale, double *d_vectors,
                               int ldo, double *d_work) {
  switch (u_lds_width(s)) {
#define U_LDS_CASE(Wv)                                                                                                         \
  case Wv:                                                                                                                     \
    return u_recover_lds_pairs<Wv, RAW>(st, d_ell_idx, d_ell_val, d_tiles, n, r, dV, ldv, s, d_eig, K, scale, d_vectors, ldo,  \
                                        d_work)
    U_LDS_CASE(1); U_LDS_CASE(2); U_LDS_CASE(3);
    default: U_LDS_CASE(4);
#undef U_LDS_CASE
  }
}

extern "C" size_t flgp_dev_row_tiles_bytes(int n, int r) {
  if (n <= 0 || r < 1 || r > FLGP_RMAX) return 0;
  return (size_t)ceil_div(n, 64) * (size_t)row_tile_pairs(r) * ROW_TILE_PAIR_BYTES;
}

// 1: the drivers pack the tiles and call the tiles entries (the LDS row kernel's conditions and the knob row_tiles, default 1)
extern "C" int flgp_dev_row_tiles_route(int n, int r, int s) {
  return tuning("row_tiles", 1) != 0 && r >= 1 && r <= FLGP_RMAX && flgp_dev_u_recover_route(n, r, s, 1, 1) == 4;
}

extern "C" int flgp_dev_row_tiles_pack(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, void *d_tiles) {
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && n >= 0, "row tiles: bad arguments");
  if (n == 0) return FLGP_OK;
  FLGP_REQUIRE(d_ell_idx && d_ell_val && d_tiles, "row tiles: null pointer");
  FLGP_REQUIRE(((size_t)d_tiles & 127) == 0, "row tiles: the buffer must be 128-byte aligned");
  const int pt = row_tile_pairs(r);
  const long slots = (long)ceil_div(n, 64) * pt * 64;
  hipLaunchKernelGGL(row_tiles_pack_kernel, dim3(ceil_div(slots, 256)), dim3(256), 0, (hipStream_t)stream, d_ell_idx, d_ell_val, n,
                     r, pt, slots, (char *)d_tiles);
  return check_launch("row_tiles_pack_kernel");
}

extern "C" int flgp_dev_u_recover(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r,
                                  const double *dV, int ldv, int s, const double *d_eig, int K, double scale,
                                  int root, double *d_vectors, int ldo, double *d_values_out, double *d_work) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && K >= 1 && ldo >= n, "u_recover: bad shape");
  if (n > 0) {
    ProfScope ps("u_recover_kernel", st, 12.0 * (double)n * r + 8.0 * (double)s * K + 8.0 * (double)n * K);
    const int route = flgp_dev_u_recover_route(n, r, s, K, d_work != nullptr);
    if (route == 4) {
      FLGP_TRY(u_recover_lds_width<false>(st, d_ell_idx, d_ell_val, nullptr, n, r, dV, ldv, s, d_eig, K, scale, d_vectors, ldo,
                                          d_work));
    } else if (d_work) {
      hipLaunchKernelGGL(transpose_v_kernel, dim3(ceil_div(s, 32), ceil_div(K, 32)), dim3(256), 0, st, dV, ldv, s, K,
                         d_work);
      if (K % 4 == 0) {
        hipLaunchKernelGGL((u_recover_wide_kernel<4, 32>), dim3(ceil_div(n, 32), ceil_div(K, 256)), dim3(256), 0, st, d_ell_idx,
                           d_ell_val, n, r, d_work, d_eig, K, scale, d_vectors, ldo);
      } else if (K % 2 == 0) {
        hipLaunchKernelGGL((u_recover_wide_kernel<2, 64>), dim3(ceil_div(n, 64), ceil_div(K, 128)), dim3(256), 0, st, d_ell_idx,
                           d_ell_val, n, r, d_work, d_eig, K, scale, d_vectors, ldo);
      } else {
        hipLaunchKernelGGL(u_recover_tiled_kernel, dim3(ceil_div(n, 64), ceil_div(K, 64)), dim3(256), 0, st, d_ell_idx,
                           d_ell_val, n, r, d_work, d_eig, K, scale, d_vectors, ldo);
      }
    } else {
      hipLaunchKernelGGL(u_recover_kernel, dim3(ceil_div(n, 256), ceil_div(K, 8)), dim3(256), 0, st, d_ell_idx,
                         d_ell_val, n, r, dV, ldv, d_eig, K, scale, d_vectors, ldo);
    }
    FLGP_TRY(check_launch("u_recover_kernel"));
  }
  if (d_values_out) {
    hipLaunchKernelGGL(values_out_kernel, dim3(ceil_div(K, 256)), dim3(256), 0, st, d_eig, K, root, d_values_out);
    FLGP_TRY(check_launch("values_out_kernel"));
  }
  return FLGP_OK;
}

// flgp_dev_u_recover on the wave tiles of the rows: the LDS slice kernel (route 4) and nothing else
extern "C" int flgp_dev_u_recover_tiles(void *stream, const void *d_tiles, int n, int r, const double *dV, int ldv, int s,
                                        const double *d_eig, int K, double scale, int root, double *d_vectors, int ldo,
                                        double *d_values_out, double *d_work) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && K >= 1 && ldo >= n, "u_recover_tiles: bad shape");
  FLGP_REQUIRE(d_tiles && ((size_t)d_tiles & 127) == 0, "u_recover_tiles: the tiles must be there and 128-byte aligned");
  FLGP_REQUIRE(flgp_dev_u_recover_route(n, r, s, K, d_work != nullptr) == 4,
               "u_recover_tiles: no LDS slice route for n=%d r=%d s=%d (ask flgp_dev_u_recover_route)", n, r, s);
  {
    ProfScope ps("u_recover_kernel", st, 12.0 * (double)n * r + 8.0 * (double)s * K + 8.0 * (double)n * K);
    FLGP_TRY(u_recover_lds_width<false>(st, nullptr, nullptr, d_tiles, n, r, dV, ldv, s, d_eig, K, scale, d_vectors, ldo, d_work));
    FLGP_TRY(check_launch("u_recover_kernel"));
  }
  if (d_values_out) {
    hipLaunchKernelGGL(values_out_kernel, dim3(ceil_div(K, 256)), dim3(256), 0, st, d_eig, K, root, d_values_out);
    FLGP_TRY(check_launch("values_out_kernel"));
  }
  return FLGP_OK;
}

// ----------------------------------------------------------------------------------------
// Heat-kernel covariance from the sparse rows.  On the covariance path every row of V is a combination of r anchor rows,
//   V(i, k) = ((sum_a A(i, a) Vs(idx(i, a), k)) / sigma_k) scale,
// so H(i, b) = sum_k V(i, k) e^{-t (1 - lambda_k)} V1(b, k) = sum_a A(i, a) Wm(idx(i, a), b) with the s x m matrix
//   Wm = B Vw^T,  B = Vs diag(scale / sigma_k),  Vw(b, k) = e^{-t (1 - lambda_k)} V1(b, k):
// 2 n r m + 2 s m K flop instead of 2 n m K, and H is the LDS row kernel of U-recovery applied to Wm with K := m (its output
// layout is H's).  Workspace, in doubles: B (s K) | Vw (m K) | Wm (s m) | the slice image of Wm, each part on a 256-byte edge.
// ----------------------------------------------------------------------------------------
namespace {
struct HkRowsLayout { size_t b, vw, wm, image, total; };
HkRowsLayout hk_rows_layout(int s, int m, int K) {
  auto up = [](size_t e) { return (e + 31) / 32 * 32; };
  const int w = u_lds_width(s);
  const size_t S = s > 0 ? s : 0, M = m > 0 ? m : 0, Kk = K > 0 ? K : 0;
  HkRowsLayout L;
  L.b = 0;
  L.vw = L.b + up(S * Kk);
  L.wm = L.vw + up(M * Kk);
  L.image = L.wm + up(S * M);
  L.total = L.image + up(S * (w >= 1 ? (size_t)ceil_div(M, w) * w : M));
  return L;
}
}  // namespace

extern "C" size_t flgp_dev_hk_rows_workspace(int s, int m, int K) { return sizeof(double) * hk_rows_layout(s, m, K).total + 256; }

// 1: flgp_dev_hk_rows computes H; 0: the caller keeps flgp_dev_u_recover + flgp_dev_hk.  The row kernel needs what the LDS
// kernel of U-recovery needs; beyond that the MFMA contraction costs ~ n m K and the rows ~ n r ceil(m / W) (W columns per
// slice), so the rows win from some K W / r on.  Measured at r = 10, n = 1e5 and 1e6 (profiles/r08_hk_rows_crossover.json,
// rows / MFMA at the call alone): m = 1000: 0.71-0.79 at K W / r = 80, 1.26-1.36 at 40, 1.6-3.0 below; m = 100 (the
// contraction is hk_panel_kernel there): 0.45-0.56 at 80, 0.69-0.86 at 40, 0.86-1.26 at 20.
// Tuning knob hk_rows: 0 never, 1 (default) by this rule, 2 wherever the row kernel applies.
extern "C" int flgp_dev_hk_rows_route(int n, int r, int s, int K, int m) {
  const int knob = tuning("hk_rows", 1);
  const int w = u_lds_width(s);
  if (!knob || w < 1 || n < U_RECOVER_LDS_MIN_N || (long)n * r < 2 || r < 1 || r > FLGP_RMAX || K < 1 || m < 1) return 0;
  if (knob == 2) return 1;
  if (m < HK_ROWS_MIN_M) return 0;
  return (long)K * w >= (m >= HK_ROWS_PANEL2_M ? HK_ROWS_MIN_KW_PER_R : HK_ROWS_MIN_KW_PER_R_SMALL_M) * (long)r;
}

// the rows from the ELL arrays, or from their wave tiles where d_tiles is there; `who` names the entry in the messages
static int hk_rows_run(const char *who, void *stream, const int *d_ell_idx, const double *d_ell_val, const void *d_tiles, int n, int r,
                       const double *dVs, int ldv, int s, const double *d_eig, int K, double scale, const double *d_values, double t,
                       const double *dV1, int ld1, int m, double *dH, int ldh, double *d_work) {
  hipStream_t st = (hipStream_t)stream;
  FLGP_REQUIRE((d_tiles || (d_ell_idx && d_ell_val)) && dVs && d_eig && d_values && dV1 && dH && d_work, "%s: null pointer", who);
  FLGP_REQUIRE(((size_t)d_tiles & 127) == 0, "%s: the tiles must be 128-byte aligned", who);
  FLGP_REQUIRE(r >= 1 && r <= FLGP_RMAX && K >= 1 && m >= 1 && s >= 1 && ldv >= s && ld1 >= m && ldh >= n, "%s: bad shape", who);
  FLGP_REQUIRE(u_lds_width(s) >= 1 && n >= U_RECOVER_LDS_MIN_N && (long)n * r >= 2,
               "%s: no LDS slice for n=%d r=%d s=%d (ask flgp_dev_hk_rows_route)", who, n, r, s);
  const HkRowsLayout L = hk_rows_layout(s, m, K);
  double *B = d_work + L.b, *Vw = d_work + L.vw, *Wm = d_work + L.wm, *image = d_work + L.image;
  FLGP_TRY(hk_rows_b(st, dVs, ldv, s, d_eig, K, scale, B));
  FLGP_TRY(hk_scale_launch(st, d_values, K, t, dV1, ld1, nullptr, 0, m, Vw));
  // Wm(j, b) = sum_k B(j, k) Vw(b, k): no workspace, so one k-ascending MFMA chain per element (never split)
  FLGP_TRY(gemm_launch(st, s, m, K, 1.0, B, 1, s, Vw, m, 1, 0.0, nullptr, 0, 0, Wm, 1, s, nullptr, 0, 0.0, nullptr));
  ProfScope ps("hk_rows_kernel", st, 2.0 * (double)n * r * m);     // (with the slice image of Wm: 16 s m bytes)
  return u_recover_lds_width<true>(st, d_ell_idx, d_ell_val, d_tiles, n, r, Wm, s, s, nullptr, m, 1.0, dH, ldh, image);
}

extern "C" int flgp_dev_hk_rows(void *stream, const int *d_ell_idx, const double *d_ell_val, int n, int r, const double *dVs,
                                int ldv, int s, const double *d_eig, int K, double scale, const double *d_values, double t,
                                const double *dV1, int ld1, int m, double *dH, int ldh, double *d_work) {
  FLGP_REQUIRE(d_ell_idx && d_ell_val, "hk_rows: null pointer");
  return hk_rows_run("hk_rows", stream, d_ell_idx, d_ell_val, nullptr, n, r, dVs, ldv, s, d_eig, K, scale, d_values, t, dV1, ld1, m,
                     dH, ldh, d_work);
}

// flgp_dev_hk_rows on the wave tiles of the rows (flgp_dev_row_tiles_pack)
extern "C" int flgp_dev_hk_rows_tiles(void *stream, const void *d_tiles, int n, int r, const double *dVs, int ldv, int s,
                                      const double *d_eig, int K, double scale, const double *d_values, double t,
                                      const double *dV1, int ld1, int m, double *dH, int ldh, double *d_work) {
  FLGP_REQUIRE(d_tiles, "hk_rows_tiles: null pointer");
  return hk_rows_run("hk_rows_tiles", stream, nullptr, nullptr, d_tiles, n, r, dVs, ldv, s, d_eig, K, scale, d_values, t, dV1, ld1,
                     m, dH, ldh, d_work);
}

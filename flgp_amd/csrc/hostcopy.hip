// Device results to the caller's pageable memory through pinned staging buffers, the copies overlapped with the work
// that feeds them: hk_ranges_to_host (H of the single-GPU host entries) and d2h_cols_pipelined (a rank's rows of H).
#include "common.h"
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

using namespace flgp;

namespace {

// ------------------------------------------------------------------------------------------
// H to the caller's (pageable) buffer without serialising GEMM, PCIe and the host copy.
// H is n0 x n1 column-major and the contraction is independent per column, so H goes over in blocks of columns:
// block c is contracted into one of two device buffers while block c-1 crosses PCIe into one of two pinned buffers and
// block c-2 is copied from there into the caller's memory by a few host threads.  (hipMemcpyAsync straight into
// pageable memory stages through the runtime's own bounce buffer on ONE thread and never overlaps the GEMM: 0.44-0.74 s
// for the 8 GB of BASELINE configs[2] in round 1, against 0.16 s of PCIe.)  The pinned buffers are kept for the
// lifetime of the process (pinning 1 GB costs more than the whole call).
// ------------------------------------------------------------------------------------------
struct PinnedRing {
  void *buf[2] = {nullptr, nullptr};
  size_t bytes = 0;
  bool busy = false;
  void drop() {
    for (int q = 0; q < 2; ++q) { if (buf[q]) (void)hipHostFree(buf[q]); buf[q] = nullptr; }
    bytes = 0;
  }
  int ensure(size_t need) {
    if (need <= bytes) return FLGP_OK;
    drop();
    for (int q = 0; q < 2; ++q)
      if (hipHostMalloc(&buf[q], need, hipHostMallocDefault) != hipSuccess) {
        set_error("hipHostMalloc of %zu bytes failed", need);
        drop();
        return FLGP_ERR_NOMEM;
      }
    bytes = need;
    return FLGP_OK;
  }
};
// The rings are handed out one per call in flight (the lock covers the hand-out only, not the multi-GB transfer): a
// second caller gets a ring of its own, up to `hk_rings_max` (2); beyond that callers queue.  flgp_release_pinned()
// gives the idle ones back to the system.
std::mutex g_ring_mu;
std::condition_variable g_ring_cv;
std::vector<PinnedRing *> g_rings;
struct RingLease {
  PinnedRing *r = nullptr;
  explicit RingLease(int at_least) {     // at_least: the ranks of one multi-GPU call each need a ring at the same time
    std::unique_lock<std::mutex> lk(g_ring_mu);
    const size_t cap = (size_t)std::max(std::max(1, tuning("hk_rings_max", 2)), at_least);
    for (;;) {
      for (PinnedRing *c : g_rings) if (!c->busy) { r = c; break; }
      if (!r && g_rings.size() < cap) { r = new PinnedRing(); g_rings.push_back(r); }
      if (r) break;
      g_ring_cv.wait(lk);
    }
    r->busy = true;
  }
  ~RingLease() {
    { std::lock_guard<std::mutex> lk(g_ring_mu); r->busy = false; }
    g_ring_cv.notify_one();
  }
};
// events of one call, destroyed on every way out
struct EventSet {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  int create() {
    for (int q = 0; q < 4; ++q)
      if (hipEventCreateWithFlags(&e[q], hipEventDisableTiming) != hipSuccess) { e[q] = nullptr; set_error("hipEventCreate failed"); return FLGP_ERR_HIP; }
    return FLGP_OK;
  }
  ~EventSet() { for (int q = 0; q < 4; ++q) if (e[q]) (void)hipEventDestroy(e[q]); }
};

// What one pipelined copy holds while it runs: a ring with room for a block in either buffer, the events, and the host
// threads that empty pinned buffer q (join(q) before buffer q is written again)
struct CopyPipe {
  RingLease lease;
  EventSet evs;
  std::vector<std::thread> copiers[2];
  const int nthreads = std::max(1, std::min(tuning("hk_copy_threads", 8), (int)std::thread::hardware_concurrency()));
  explicit CopyPipe(int rings_at_least = 0) : lease(rings_at_least) {}
  int create(size_t blkbytes) { FLGP_TRY(lease.r->ensure(blkbytes)); return evs.create(); }
  void *buf(int q) const { return lease.r->buf[q]; }
  void join(int q) { for (auto &th : copiers[q]) th.join(); copiers[q].clear(); }
};

void parallel_copy(char *dst, const char *src, size_t bytes, int nthreads, std::vector<std::thread> &pool) {
  const size_t per = (bytes / nthreads + 4095) / 4096 * 4096;
  for (int q = 0; q < nthreads; ++q) {
    const size_t a = (size_t)q * per;
    if (a >= bytes) break;
    const size_t len = std::min(per, bytes - a);
    pool.emplace_back([=] { memcpy(dst + a, src + a, len); });
  }
}

}  // namespace

extern "C" void flgp_release_pinned(void) {
  std::lock_guard<std::mutex> lk(g_ring_mu);
  for (PinnedRing *c : g_rings) if (!c->busy) c->drop();
}

namespace flgp {

int hk_ranges_to_host(hipStream_t st, const double *d_values, int K, double t, const double *d_vectors, int ldv,
                      int row0_0, int n0, int row0_1, int n1, double *H) {
  if (n0 == 0 || n1 == 0) return FLGP_OK;
  const size_t colbytes = sizeof(double) * (size_t)n0;
  // block width: ~512 MB per block, a multiple of 64 columns where that is possible (half a GEMM tile)
  int nc = (int)std::max<size_t>(1, ((size_t)std::max(1, tuning("hk_block_mb", 512)) << 20) / colbytes);
  if (nc >= 64) nc = nc / 64 * 64;
  if (nc > n1) nc = n1;
  const int nblk = ceil_div(n1, nc);
  if (nblk <= 1 || tuning("hk_pipelined_d2h", 1) == 0) {   // small: one contraction, one copy
    DevBuf dH, work;
    FLGP_TRY(dH.alloc(colbytes * n1));
    FLGP_TRY(work.alloc(flgp_dev_hk_workspace(n0, n1, K, 0)));
    FLGP_TRY(flgp_dev_hk(st, d_values, K, t, d_vectors, ldv, nullptr, row0_0, n0, d_vectors, ldv, nullptr, row0_1, n1,
                         dH.as<double>(), n0, work.as<double>()));
    FLGP_TRY(d2h(H, dH.p, colbytes * n1, st));
    FLGP_HIP(hipStreamSynchronize(st));
    return FLGP_OK;
  }
  CopyPipe pipe;
  const size_t blkbytes = colbytes * nc;
  FLGP_TRY(pipe.create(blkbytes));
  DevBuf dH[2], work;
  FLGP_TRY(dH[0].alloc(blkbytes)); FLGP_TRY(dH[1].alloc(blkbytes));
  FLGP_TRY(work.alloc(flgp_dev_hk_workspace(n0, nc, K, 0)));
  Stream cp;
  FLGP_TRY(cp.create());
  hipEvent_t *gemm_done = pipe.evs.e, *dma_done = pipe.evs.e + 2;
  int rc = FLGP_OK;
  for (int c = 0; c <= nblk + 1 && rc == FLGP_OK; ++c) {
    const int q = c & 1;
    if (c < nblk) {
      const int b0 = c * nc, w = std::min(nc, n1 - b0);
      // device buffer q was last read by the DMA of block c-2, pinned buffer q by the host copy of block c-2
      if (c >= 2) { if (hipStreamWaitEvent(st, dma_done[q], 0) != hipSuccess) rc = FLGP_ERR_HIP; }
      if (rc == FLGP_OK)
        rc = flgp_dev_hk(st, d_values, K, t, d_vectors, ldv, nullptr, row0_0, n0, d_vectors, ldv, nullptr, row0_1 + b0, w,
                         dH[q].as<double>(), n0, work.as<double>());
      if (rc == FLGP_OK && hipEventRecord(gemm_done[q], st) != hipSuccess) rc = FLGP_ERR_HIP;
      pipe.join(q);                              // host copy of block c-2 out of pinned buffer q
      if (rc == FLGP_OK && (hipStreamWaitEvent(cp.s, gemm_done[q], 0) != hipSuccess ||
                            hipMemcpyAsync(pipe.buf(q), dH[q].p, colbytes * w, hipMemcpyDeviceToHost, cp.s) != hipSuccess ||
                            hipEventRecord(dma_done[q], cp.s) != hipSuccess)) rc = FLGP_ERR_HIP;
    }
    if (c >= 1 && c - 1 < nblk && rc == FLGP_OK) {   // block c-1 has been enqueued: when it has landed, copy it out
      const int p = (c - 1) & 1, b0 = (c - 1) * nc, w = std::min(nc, n1 - b0);
      if (hipEventSynchronize(dma_done[p]) != hipSuccess) rc = FLGP_ERR_HIP;
      else parallel_copy((char *)H + colbytes * b0, (const char *)pipe.buf(p), colbytes * w, pipe.nthreads, pipe.copiers[p]);
    }
  }
  pipe.join(0); pipe.join(1);
  (void)hipStreamSynchronize(cp.s);
  (void)hipStreamSynchronize(st);
  if (rc == FLGP_ERR_HIP) set_error("HIP error in the pipelined copy of H");
  return rc;
}

// Through the pinned ring: the DMA of block c runs while a few host threads copy block c-1 out of its pinned buffer.
// What the multi-GPU host entry uses per rank (round 4; a single hipMemcpy2DAsync into pageable memory staged through
// the runtime's bounce buffer on one thread before).
int d2h_cols_pipelined(hipStream_t st, const double *dM, long rows, int cols, double *H, long ldh, int rings_at_least) {
  if (rows <= 0 || cols <= 0) return FLGP_OK;
  const size_t colbytes = sizeof(double) * (size_t)rows;
  int nc = (int)std::max<size_t>(1, ((size_t)std::max(1, tuning("hk_block_mb", 512)) << 19) / colbytes);   // half of the GEMM path's block: nothing to overlap with but the copies themselves
  if (nc > cols) nc = cols;
  const int nblk = ceil_div(cols, nc);
  CopyPipe pipe(rings_at_least);
  FLGP_TRY(pipe.create(colbytes * nc));
  hipEvent_t *dma_done = pipe.evs.e;
  int rc = FLGP_OK;
  for (int c = 0; c <= nblk && rc == FLGP_OK; ++c) {
    const int q = c & 1;
    if (c < nblk) {
      const int b0 = c * nc, w = std::min(nc, cols - b0);
      pipe.join(q);                              // the host copy of block c-2 has left pinned buffer q
      if (hipMemcpyAsync(pipe.buf(q), dM + (size_t)b0 * rows, colbytes * w, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipEventRecord(dma_done[q], st) != hipSuccess) rc = FLGP_ERR_HIP;
    }
    if (c >= 1 && rc == FLGP_OK) {
      const int p = (c - 1) & 1, b0 = (c - 1) * nc, w = std::min(nc, cols - b0);
      if (hipEventSynchronize(dma_done[p]) != hipSuccess) { rc = FLGP_ERR_HIP; break; }
      const char *src = (const char *)pipe.buf(p);
      const int per = (w + pipe.nthreads - 1) / pipe.nthreads;
      for (int tq = 0; tq < pipe.nthreads; ++tq) {
        const int c0 = tq * per, c1 = std::min(w, c0 + per);
        if (c0 >= c1) break;
        pipe.copiers[p].emplace_back([=] {
          for (int cc = c0; cc < c1; ++cc) memcpy(H + (size_t)(b0 + cc) * (size_t)ldh, src + colbytes * (size_t)cc, colbytes);
        });
      }
    }
  }
  pipe.join(0); pipe.join(1);
  (void)hipStreamSynchronize(st);
  if (rc == FLGP_ERR_HIP) set_error("HIP error in the pipelined copy of a rank's rows of H");
  return rc;
}

}  // namespace flgp

// Independent work items on one device, `workers` at a time: the bandwidths of the Nystrom, GLGP and SE grids, the dense
// logit objectives and the Polya-Gamma chains for m <= K.  Worker w owns one State (on the device: a stream and its buffers, see DevicePool
// in common.h) and takes items w, w + workers, ...; the call reports the lowest failing item.  Generic over the
// operations and free of HIP so that the scheduling is tested on the CPU (tests/c/worker_pool_check.cc).
#pragma once
#include <string>
#include <thread>
#include <vector>

namespace flgp {

// The rule include/flgp_hip.h states for the Nystrom grid: at most max_parallel (below 1: 1), at most `items`, and, where
// more than one is left and bytes_per_worker > 0, no more than fit into 90 % of free_bytes; never fewer than one.
inline int plan_workers(int max_parallel, int items, double free_bytes, double bytes_per_worker) {
  int workers = max_parallel < 1 ? 1 : max_parallel;
  if (workers > items) workers = items;
  if (workers > 1 && bytes_per_worker > 0.0) {
    const double fit = 0.9 * free_bytes / bytes_per_worker;
    if (fit < workers) workers = (int)fit;
  }
  return workers < 1 ? 1 : workers;
}

struct PoolFailure {
  int item = -1;      // -1: every item returned 0
  int status = 0;
  std::string message;
};

// setup(w, State &) -> status: what worker w owns, made in the worker's thread; a failure is pinned on item w.
// item(State &, i) -> status; last_error() -> the calling thread's error text, asked for in the thread that failed.
// A worker stops at its first non-zero status, so every item below the lowest failing one has run.  workers == 1 runs on
// the calling thread; otherwise one std::thread per worker, all joined before the return.
template <class State, class Setup, class Item, class LastError>
PoolFailure run_strided(int items, int workers, Setup setup, Item item, LastError last_error) {
  std::vector<PoolFailure> failed((size_t)workers);
  auto run = [&](int w) {
    State S;
    PoolFailure &f = failed[(size_t)w];
    int at = w;
    f.status = setup(w, S);
    while (f.status == 0 && at < items) {
      f.status = item(S, at);
      if (f.status == 0) at += workers;
    }
    if (f.status != 0) { f.item = at; f.message = last_error(); }
  };
  if (workers == 1) {
    run(0);
  } else {
    std::vector<std::thread> th;
    for (int w = 0; w < workers; ++w) th.emplace_back(run, w);
    for (auto &t : th) t.join();
  }
  PoolFailure first;
  for (auto &f : failed)
    if (f.item >= 0 && (first.item < 0 || f.item < first.item)) first = f;
  return first;
}

}  // namespace flgp

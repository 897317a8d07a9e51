// CPU check of flgp::plan_workers and flgp::run_strided (csrc/worker_pool.h): the worker-count rule, which worker runs
// which item, what a failure stops and what it leaves running, where its message is fetched, and the in-line mode.
#include "../../flgp_amd/csrc/worker_pool.h"
#include <cstdio>
#include <mutex>

static int fails = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); ++fails; } } while (0)

// the "last error" of this thread, as flgp_last_error() is
static thread_local std::string t_text;
static std::string last_text() { return t_text; }

struct State { int w = -1; };

int main() {
  using flgp::plan_workers;
  {  // max_parallel below 1 is 1; never more workers than items
    CHECK(plan_workers(-3, 10, 0, 0) == 1 && plan_workers(0, 10, 0, 0) == 1 && plan_workers(1, 10, 0, 0) == 1, "clip below 1");
    CHECK(plan_workers(8, 3, 0, 0) == 3, "items < max_parallel: %d", plan_workers(8, 3, 0, 0));
    CHECK(plan_workers(4, 10, 0, 0) == 4 && plan_workers(4, 10, 123.0, -1.0) == 4, "no cap");
    // a cap: fit = 0.9 free / per, here 0.9 * (10 fit) / 9 with products and quotients that are exact or far from an integer
    CHECK(plan_workers(4, 10, 4.0, 9.0) == 1, "fit 0.4: %d", plan_workers(4, 10, 4.0, 9.0));
    CHECK(plan_workers(4, 10, 10.0, 9.0) == 1, "fit 1.0: %d", plan_workers(4, 10, 10.0, 9.0));
    CHECK(plan_workers(4, 10, 29.0, 9.0) == 2, "fit 2.9: %d", plan_workers(4, 10, 29.0, 9.0));
    CHECK(plan_workers(4, 10, 40.0, 9.0) == 4, "fit = workers: %d", plan_workers(4, 10, 40.0, 9.0));
    CHECK(plan_workers(4, 10, 400.0, 9.0) == 4, "fit above workers: %d", plan_workers(4, 10, 400.0, 9.0));
    CHECK(plan_workers(1, 10, 0.0, 1.0) == 1, "one worker is never capped");
  }
  const int shapes[5][2] = {{1, 1}, {5, 1}, {5, 2}, {5, 5}, {16, 3}};
  for (auto &sh : shapes) {  // every item exactly once, item i on worker i mod workers
    const int items = sh[0], workers = sh[1];
    std::mutex mu;
    std::vector<int> runs(items, 0), on(items, -1);
    const flgp::PoolFailure f = flgp::run_strided<State>(
        items, workers, [](int w, State &S) { S.w = w; return 0; },
        [&](State &S, int i) {
          std::lock_guard<std::mutex> lk(mu);
          ++runs[i]; on[i] = S.w;
          return 0;
        },
        last_text);
    CHECK(f.item == -1 && f.status == 0 && f.message.empty(), "(%d,%d): reported item %d", items, workers, f.item);
    for (int i = 0; i < items; ++i)
      CHECK(runs[i] == 1 && on[i] == i % workers, "(%d,%d): item %d ran %d times on worker %d", items, workers, i, runs[i], on[i]);
  }
  {  // items 4 and 1 of 6 fail, 3 workers: both are worker 1's, which stops at item 1 and never reaches item 4.  The result
    // is item 1 with its own status and the text of its own thread; the other workers run all of theirs.
    std::vector<int> ran(6, 0);
    const flgp::PoolFailure f = flgp::run_strided<State>(
        6, 3, [](int w, State &S) { S.w = w; t_text = "idle text of worker " + std::to_string(w); return 0; },
        [&](State &S, int i) {
          ran[i] = 1;
          if (i == 4 || i == 1) { t_text = "item " + std::to_string(i) + " failed on worker " + std::to_string(S.w); return 100 + i; }
          return 0;
        },
        last_text);
    CHECK(f.item == 1 && f.status == 101, "lowest failing item: item %d status %d", f.item, f.status);
    CHECK(f.message == "item 1 failed on worker 1", "message: '%s'", f.message.c_str());
    CHECK(ran[0] && ran[3] && ran[2] && ran[5], "other workers' items were run: %d %d %d %d", ran[0], ran[3], ran[2], ran[5]);
    CHECK(ran[1] && !ran[4], "worker 1 stops at item 1: ran[1]=%d ran[4]=%d", ran[1], ran[4]);
    CHECK(t_text.empty(), "the calling thread's text was touched: '%s'", t_text.c_str());
  }
  {  // the same two items on different workers (2 workers: item 4 is worker 0's, item 1 worker 1's): the lowest is reported,
    // each worker stops at its own failure
    std::vector<int> ran(6, 0);
    const flgp::PoolFailure f = flgp::run_strided<State>(
        6, 2, [](int w, State &S) { S.w = w; return 0; },
        [&](State &S, int i) {
          ran[i] = 1;
          if (i == 4 || i == 1) { t_text = "item " + std::to_string(i) + " on worker " + std::to_string(S.w); return 100 + i; }
          return 0;
        },
        last_text);
    CHECK(f.item == 1 && f.status == 101 && f.message == "item 1 on worker 1", "two workers fail: item %d status %d '%s'", f.item,
          f.status, f.message.c_str());
    CHECK(ran[0] && ran[2] && ran[4] && ran[1] && !ran[3] && !ran[5], "who ran: %d %d %d %d %d %d", ran[0], ran[1], ran[2], ran[3],
          ran[4], ran[5]);
  }
  {  // a set-up failure of worker 2 is item 2's, with the set-up's status and text; none of its items run
    std::vector<int> ran(7, 0);
    const flgp::PoolFailure f = flgp::run_strided<State>(
        7, 3, [](int w, State &) { if (w == 2) { t_text = "no memory for worker 2"; return 7; } return 0; },
        [&](State &, int i) { ran[i] = 1; return 0; }, last_text);
    CHECK(f.item == 2 && f.status == 7 && f.message == "no memory for worker 2", "set-up failure: item %d status %d '%s'", f.item,
          f.status, f.message.c_str());
    CHECK(!ran[2] && !ran[5] && ran[0] && ran[1] && ran[3] && ran[4] && ran[6], "set-up failure: who ran");
  }
  {  // one worker runs on the calling thread, set-up and items, and stops at its first failure too
    const std::thread::id me = std::this_thread::get_id();
    bool same = true;
    std::vector<int> ran(4, 0);
    const flgp::PoolFailure f = flgp::run_strided<State>(
        4, 1, [&](int, State &) { same = same && std::this_thread::get_id() == me; return 0; },
        [&](State &, int i) {
          same = same && std::this_thread::get_id() == me;
          ran[i] = 1;
          if (i == 2) { t_text = "in line"; return 9; }
          return 0;
        },
        last_text);
    CHECK(same, "workers == 1 left the calling thread");
    CHECK(f.item == 2 && f.status == 9 && f.message == "in line" && ran[0] && ran[1] && ran[2] && !ran[3], "in line: item %d", f.item);
    // ... and several workers do not
    bool other = true;
    flgp::run_strided<State>(2, 2, [&](int, State &) { return 0; },
                             [&](State &, int) { if (std::this_thread::get_id() == me) other = false; return 0; }, last_text);
    CHECK(other, "workers == 2 ran an item on the calling thread");
  }
  if (!fails) printf("worker_pool ok\n");
  return fails;
}

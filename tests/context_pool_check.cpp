// context_pool_check.cpp — host checks of csrc/context_pool.hpp (compiled and run by test_context_pool_cpu.py): a pool
// of at most 4 fake contexts under 8 threads of 200 acquire / release rounds each, and a make() that fails once.  Prints
// one line per failed check and exits non-zero if there was one.
#include <atomic>
#include <cstdio>
#include <memory>
#include <thread>
#include <vector>

#include "context_pool.hpp"

using namespace vi;

static std::atomic<int> failures{0};

#define CHECK(cond, ...)               \
  do {                                 \
    if (!(cond)) {                     \
      ++failures;                      \
      std::printf("FAIL %s: ", #cond); \
      std::printf(__VA_ARGS__);        \
      std::printf("\n");               \
    }                                  \
  } while (0)

constexpr int kContexts = 4, kThreads = 8, kRounds = 200;

struct FakeContext {
  std::atomic<int> holders{0};
  int uses = 0;  // written by the holder only: a second holder is a data race the thread sanitizer sees
};
using Pool = ContextPool<FakeContext, kContexts>;

static std::atomic<int> created{0}, held{0}, high_water{0};

static std::unique_ptr<FakeContext> make_fake() {
  ++created;
  return std::make_unique<FakeContext>();
}

static void enter(FakeContext &c) {
  CHECK(c.holders.fetch_add(1) == 0, "a context is held twice");
  const int now = ++held;
  for (int hw = high_water.load(); hw < now && !high_water.compare_exchange_weak(hw, now);) {}
  ++c.uses;
  std::this_thread::yield();
}
static void leave(FakeContext &c) {
  --held;
  CHECK(c.holders.fetch_sub(1) == 1, "a context is held twice");
}

// the bounds under contention: half of the threads use the pool directly, half through leases
static void check_contention() {
  Pool pool;
  int published = 0;  // by every release, under the pool's lock alone
  std::vector<std::thread> threads;
  for (int t = 0; t < kThreads; ++t)
    threads.emplace_back([&pool, &published, t] {
      for (int r = 0; r < kRounds; ++r) {
        if (t % 2) {
          FakeContext *c = pool.acquire(make_fake);
          CHECK(c != nullptr, "thread %d round %d: no context", t, r);
          if (!c) return;
          enter(*c);
          leave(*c);
          pool.release(c, [&] { ++published; });
        } else {
          ContextLease lease(pool, make_fake, [&] { ++published; });
          CHECK(lease.ctx != nullptr, "thread %d round %d: no context", t, r);
          if (!lease.ctx) return;
          enter(*lease.ctx);
          leave(*lease.ctx);
        }
      }
    });
  for (auto &th : threads) th.join();
  int seen = 0;
  pool.locked([&] { seen = published; });
  CHECK(seen == kThreads * kRounds, "%d releases ran their callable, of %d", seen, kThreads * kRounds);
  CHECK(created.load() >= 1 && created.load() <= kContexts, "%d contexts created", created.load());
  CHECK(high_water.load() >= 1 && high_water.load() <= kContexts, "%d contexts held at once", high_water.load());
  CHECK(held.load() == 0, "%d contexts still held", held.load());
  // every context is free again, and no further one is made
  std::vector<FakeContext *> all;
  int uses = 0;
  for (int i = 0; i < created.load(); ++i) {
    all.push_back(pool.acquire([]() -> std::unique_ptr<FakeContext> {
      CHECK(false, "a context was made while one was free");
      return nullptr;
    }));
    if (all.back()) uses += all.back()->uses;
  }
  CHECK(uses == kThreads * kRounds, "the contexts were used %d times, of %d", uses, kThreads * kRounds);
  for (FakeContext *c : all)
    if (c) pool.release(c, [] {});
}

// a make() that fails leaves the pool as it was: nothing to release, the next acquire makes its context, and the failed
// attempt does not count against the four
static void check_failed_make() {
  Pool pool;
  int made = 0, released = 0;
  auto failing = []() -> std::unique_ptr<FakeContext> { return nullptr; };
  auto counting = [&] {
    ++made;
    return std::make_unique<FakeContext>();
  };
  {
    ContextLease lease(pool, failing, [&] { ++released; });
    CHECK(lease.ctx == nullptr, "a failed make gave a context");
  }
  CHECK(released == 0, "a lease without a context ran its callable %d times", released);
  std::vector<FakeContext *> got;
  for (int i = 0; i < kContexts; ++i) {
    got.push_back(pool.acquire(counting));
    CHECK(got.back() != nullptr, "acquire %d after the failed make gave no context", i);
  }
  CHECK(made == kContexts, "%d contexts made after the failed make, of %d", made, kContexts);
  for (size_t i = 0; i < got.size(); ++i)
    for (size_t j = 0; j < i; ++j) CHECK(got[i] != got[j], "acquires %zu and %zu gave the same context", j, i);
  // all four are held: a fifth caller waits until one comes back, and gets that one
  std::atomic<FakeContext *> fifth{nullptr};
  std::thread waiter([&] { fifth = pool.acquire(failing); });
  pool.release(got[0], [&] { ++released; });
  waiter.join();
  CHECK(fifth.load() == got[0], "the waiting caller did not get the released context");
  CHECK(released == 1, "release ran its callable %d times", released);
  for (FakeContext *c : got)
    if (c) pool.release(c, [] {});
}

int main() {
  check_contention();
  check_failed_make();
  if (failures) std::printf("%d checks failed\n", failures.load());
  return failures ? 1 : 0;
}

// context_pool.hpp — the contexts that concurrent calls on one handle hold, one per call: at most N, made on demand
// (standard library only: tests/test_context_pool_cpu.py).
#pragma once
#include <condition_variable>
#include <memory>
#include <mutex>
#include <vector>

namespace vi {

template <class Ctx, int N>
class ContextPool {
 public:
  using context = Ctx;
  // a free context, or make() — a std::unique_ptr<Ctx>, null: failure, returned as it is — while fewer than N exist, or
  // the wait for one
  template <class Make>
  Ctx *acquire(Make make) {
    std::unique_lock<std::mutex> lock(mu_);
    for (;;) {
      if (!free_.empty()) { Ctx *c = free_.back(); free_.pop_back(); return c; }
      if ((int)owned_.size() < N) {
        std::unique_ptr<Ctx> c = make();
        Ctx *made = c.get();
        if (made) owned_.push_back(std::move(c));
        return made;
      }
      cv_.wait(lock);
    }
  }
  // under_lock() — what the call publishes on the handle — runs under the pool's lock, then the context is free again
  template <class F>
  void release(Ctx *c, F under_lock) {
    std::unique_lock<std::mutex> lock(mu_);
    under_lock();
    free_.push_back(c);
    lock.unlock();
    cv_.notify_one();
  }
  template <class F>
  void locked(F f) const {  // (the readers of what the releases publish)
    std::lock_guard<std::mutex> lock(mu_);
    f();
  }

 private:
  mutable std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::unique_ptr<Ctx>> owned_;
  std::vector<Ctx *> free_;
};

// one context of `pool` until the end of the scope, null if make() failed; on_release runs under the pool's lock
template <class Pool, class F>
struct ContextLease {
  Pool &pool;
  F on_release;
  typename Pool::context *const ctx;
  template <class Make>
  ContextLease(Pool &p, Make make, F f) : pool(p), on_release(f), ctx(p.acquire(make)) {}
  ContextLease(const ContextLease &) = delete;
  ~ContextLease() { if (ctx) pool.release(ctx, on_release); }
};

}  // namespace vi

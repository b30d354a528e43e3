// The engine's host threads (host-only, no HIP: the sanitizer tests build
// this header with a plain C++ compiler).  Worker: one thread per device
// context, running submitted tasks in order.  CopyPool: large host copies
// spread over a few persistent threads.
#pragma once

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "coa_env.h"
#include "coa_stage.h"  // Seg

namespace coa_rt __attribute__((visibility("hidden"))) {

// Result of a task run on another thread: return code + that thread's error.
using TaskResult = std::pair<int, std::string>;

// One host thread running submitted tasks in order.  on_start runs first on
// the thread (the engine marks its thread-locals there); a task answers its
// TaskResult itself, so what "that thread's error" is stays the caller's.
class Worker {
 public:
  explicit Worker(std::function<void()> on_start = nullptr)
      : th_([this, on_start = std::move(on_start)] {
          if (on_start) on_start();
          loop();
        }) {}
  ~Worker() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    cv_.notify_all();
    th_.join();
  }
  std::future<TaskResult> submit(std::function<TaskResult()> f) {
    // wrapped in a lambda: its type is this namespace's, so the library exports
    // no std::packaged_task instantiation
    auto task = std::make_shared<std::packaged_task<TaskResult()>>([f = std::move(f)] { return f(); });
    std::future<TaskResult> fut = task->get_future();
    {
      std::lock_guard<std::mutex> l(m_);
      q_.emplace_back([task] { (*task)(); });
    }
    cv_.notify_one();
    return fut;
  }

 private:
  void loop() {
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || !q_.empty(); });
        if (q_.empty()) return;
        job = std::move(q_.front());
        q_.pop_front();
      }
      job();
    }
  }
  std::mutex m_;
  std::condition_variable cv_;
  std::deque<std::function<void()>> q_;
  bool stop_ = false;
  std::thread th_;  // last: starts after the members above exist
};

// Host copies split over a few persistent threads: packing a round of
// certificates (68 MB at C3) into page-locked staging runs at one core's
// memcpy rate (~8 GB/s) on one thread -- slower than PCIe.  COA_PACK_THREADS
// (default 8, at most 16) threads including the caller.
class CopyPool {
 public:
  static CopyPool& get() {
    static CopyPool pool;
    return pool;
  }
  // Copies every segment, pieces of at most kPiece bytes spread over the pool.
  void copy(const std::vector<Seg>& segs) { copy(segs.data(), segs.size()); }
  void copy(const Seg* segs, size_t n) {
    // Below kInline bytes the caller copies alone: waking the pool
    // (notify_all of 7 threads + a done_cv wait) cost one C3 certificate
    // (~10 KB in 7 segments) ~27 us of its 0.12 ms p50 in round 4.
    size_t total = 0;
    for (const Seg* g = segs; g != segs + n; g++) total += g->bytes;
    if (total < kInline) {
      for (const Seg* g = segs; g != segs + n; g++) std::memcpy(g->dst, g->src, g->bytes);
      return;
    }
    std::vector<Seg> pieces;
    for (const Seg* g = segs; g != segs + n; g++)
      for (size_t o = 0; o < g->bytes; o += kPiece)
        pieces.push_back({static_cast<uint8_t*>(g->dst) + o, static_cast<const uint8_t*>(g->src) + o,
                          std::min(kPiece, g->bytes - o)});
    // chunks of consecutive pieces of >= kChunk bytes, claimed with one atomic
    // add each: a queue window of C3 certificates is ~2,000 segments of a few
    // KB, and a mutex per segment made eight threads copy at 3 GB/s
    std::vector<size_t> cuts{0};
    size_t acc = 0;
    for (size_t k = 0; k < pieces.size(); k++) {
      acc += pieces[k].bytes;
      if (acc >= kChunk) {
        cuts.push_back(k + 1);
        acc = 0;
      }
    }
    if (cuts.back() != pieces.size()) cuts.push_back(pieces.size());
    const size_t nchunks = cuts.size() - 1;
    if (nchunks <= 1 || th_.empty()) {
      for (const Seg& g : pieces) std::memcpy(g.dst, g.src, g.bytes);
      return;
    }
    // Several jobs may be in progress at once (two collectors' windows, a
    // host call): each has its own counters, the workers take chunks of the
    // oldest job that has some left, and every caller works on its own job
    // until it is claimed, then waits for the rest of it.  (Round 5 ran one
    // job at a time and a second caller copied alone, at one core's rate.)
    auto job = std::make_shared<Job>();
    job->pieces = pieces.data();
    job->cuts = cuts.data();
    job->n = nchunks;
    {
      std::lock_guard<std::mutex> l(m_);
      jobs_.push_back(job);
    }
    cv_.notify_all();
    work(*job);
    std::unique_lock<std::mutex> l(m_);
    done_cv_.wait(l, [&] { return job->done.load(std::memory_order_acquire) == nchunks; });
    jobs_.erase(std::find(jobs_.begin(), jobs_.end(), job));
  }
  ~CopyPool() {
    {
      std::lock_guard<std::mutex> l(m_);
      stop_ = true;
    }
    cv_.notify_all();
    for (auto& t : th_) t.join();
  }

 private:
  struct Job {
    const Seg* pieces = nullptr;
    const size_t* cuts = nullptr;  // chunk k = pieces [cuts[k], cuts[k + 1])
    size_t n = 0;                  // chunks
    std::atomic<size_t> next{0}, done{0};
  };
  static constexpr size_t kPiece = 1 << 20;
  static constexpr size_t kChunk = 256 << 10;
  static constexpr size_t kInline = 512 << 10;  // ~50 us of one core's memcpy
  CopyPool() {
    const long n = env_int("COA_PACK_THREADS", 8, 1, 16);  // read once, at the first copy
    for (long i = 1; i < n; i++) th_.emplace_back([this] { loop(); });
  }
  void work(Job& j) {
    for (;;) {
      const size_t k = j.next.fetch_add(1, std::memory_order_relaxed);
      if (k >= j.n) return;
      for (size_t i = j.cuts[k]; i < j.cuts[k + 1]; i++) std::memcpy(j.pieces[i].dst, j.pieces[i].src, j.pieces[i].bytes);
      if (j.done.fetch_add(1, std::memory_order_acq_rel) + 1 == j.n) {
        std::lock_guard<std::mutex> l(m_);
        done_cv_.notify_all();
      }
    }
  }
  // the oldest job with unclaimed chunks (under m_), or null
  std::shared_ptr<Job> open_job() const {
    for (const auto& j : jobs_)
      if (j->next.load(std::memory_order_relaxed) < j->n) return j;
    return nullptr;
  }
  void loop() {
    for (;;) {
      std::shared_ptr<Job> j;
      {
        // the job is taken by the predicate itself: chunks are claimed without
        // the lock, so a second open_job() here could find none left
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return stop_ || (j = open_job()) != nullptr; });
        if (stop_) return;
      }
      work(*j);
    }
  }
  std::mutex m_;
  std::condition_variable cv_, done_cv_;
  std::vector<std::shared_ptr<Job>> jobs_;  // in progress, oldest first
  bool stop_ = false;
  std::vector<std::thread> th_;
};

}  // namespace coa_rt


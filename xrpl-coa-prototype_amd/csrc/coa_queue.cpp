// Aggregation queue: the pre-verification stage between
// PrimaryReceiverHandler::dispatch (primary/src/primary.rs:223-244) and
// Core (primary/src/core.rs:349-389).  Core verifies one message at a time;
// this stage collects pending header/vote signatures, whole headers and
// votes (Header::verify / Vote::verify with their digests), vote batches, whole
// certificates and worker batch digests from any number of producer threads
// and launches them as a few large GPU calls.  Modelled on the reference's
// SignatureService (crypto/src/lib.rs:222-250): a request channel in, a
// per-request reply (here a C callback, which the Rust side maps onto a
// oneshot channel: rust/crypto/src/service.rs).
//
// Pipeline:
//   producers   copy each request into an intake shard under that shard's
//               lock only.  A queue has a fixed pool of kShards shards; a
//               thread always uses shard (thread ordinal mod kShards), so
//               memory is bounded whatever the number of threads or queues.
//               The queue-wide pending count is told in steps (a shard's
//               first item, then every kReport items), so producers do not
//               share a written cache line per request
//   collector   closes the window when `max_batch` items are pending, when
//               the oldest request is `max_delay_us` old, on flush, or --
//               with COA_QUEUE_IDLE_LAUNCH=k -- as soon as fewer than k
//               windows are in flight (a lone request on an idle device
//               launches at once; under load the arrivals still coalesce
//               behind the windows in flight), takes
//               every non-empty shard's window (a swap per shard -- the
//               parts are never merged on the host: the backend packs them
//               straight into its pinned staging) and hands the parts to the
//               backend, which enqueues their copies and kernels on a free
//               device slot's stream WITHOUT waiting; it then collects the
//               next window, which is packed and launched while the previous
//               one is still on the GPU
//   completer   waits for the launches in order and answers every request
//               through its callback.  A failed launch is retried on the
//               backend's recovery context of each device in turn (its slot
//               rebuilt meanwhile); only when every attempt failed do the
//               callbacks get the engine error -- the reference's verify
//               never fails for a reason other than the signature, and
//               Core::run logs every error and continues
//               (primary/src/core.rs:390-398).
// Lanes: all of the above exists twice -- one lane for signatures, vote
// batches and certificates, one for worker-batch digests -- each with its own
// shards, collector, backend slots and completer.  A digest window is a 14 ms
// serial SHA-512 chain per batch; in a shared window, slot or completion
// order it would hold every verdict behind it for that long.
// The backend (coa_queue.h) is the HIP one (coa_queue_hip.cpp) or, in the
// sanitizer and CPU tests, a stub.
//
// Verdict requests (coa_queue_submit_*_verdict): a certificate, header or
// vote whose callback gets the reference's whole DagResult as one COA_DAG_*
// word (n = 4) instead of crypto bits.  They are items of the same arrays as
// the crypto requests of their kind, marked in the window (Window::c_vreq,
// hd_vreq, vt_vreq, with the payload counts), so they share shards, windows,
// slots, retries and ordering; the backend decides their words in the window
// and leaves open only certificates whose votes need the exact check.  A
// window whose key-cache generation has no protocol table answers them with
// COA_EINVAL (Launch::verdict_rc) and the failed word -- no engine failure.
//
// Metrics (coa_queue_metrics): per-kind request counts, window sizes,
// windows in flight, pending depth, retried / recovered / failed windows, the
// submit -> callback wait time of every request (mean, max, p50/p99 from a
// log-spaced histogram), and where a tail comes from: the slowest window's
// launch -> completion time with its size and kinds, the longest wait for a
// free slot, staging reallocations -- the numbers needed to tune max_batch /
// max_delay_us against the serial Core::run.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "coa_env.h"
#include "coa_qmetrics.h"
#include "coa_queue.h"

using namespace coa_rt;  // the switch readers of coa_env.h

namespace {

using coa_q::LaneMetrics;
using coa_q::Launch;
using coa_q::WaitTally;
using coa_q::Window;

// The *_V kinds are the verdict requests: items of the same arrays as K_CERT,
// K_HEADER and K_VOTE (idx counts both), answered with a COA_DAG_* word.
enum Kind : uint8_t { K_VERIFY, K_BATCH, K_CERT, K_DIGEST, K_HEADER, K_VOTE, K_CERT_V, K_HEADER_V, K_VOTE_V };

inline void cpu_relax() {
#if defined(__x86_64__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}

inline int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

struct Req {
  coa_verdict_cb cb;
  void* user;
  int64_t t0;      // submission time, ns
  uint32_t idx;    // index among the part's requests of this kind
  uint32_t n;      // K_VERIFY: consecutive signatures of the request
  Kind kind;
};

// Where each kind's answer is -- the only per-kind tables of the outputs, for
// the completer and the resolver alike.  True for a request the backend left
// open in its window (Window::c_defer, m_defer, g_defer): the resolver's.
inline bool is_deferred(const Req& r, const Window& w) {
  switch (r.kind) {
    case K_CERT:
    case K_CERT_V: return w.is_deferred_cert(r.idx);
    case K_BATCH: return w.g_defer;
    case K_HEADER: return w.is_deferred_msg(r.idx);
    case K_VOTE: return w.is_deferred_msg((uint32_t)w.nhd + r.idx);
    case K_VERIFY:
    case K_DIGEST:
    case K_HEADER_V:  // answered by the protocol word alone, in their window
    case K_VOTE_V: break;
  }
  return false;
}
// A verdict request's callback: one COA_DAG_* word (n = 4), with the window's
// status or, when that is fine, the verdict requests' own (COA_EINVAL: no
// protocol table).  The word is the failed one whenever the status is negative.
inline void answer_word(const Req& r, const std::vector<uint32_t>& words, int rc, int verdict_rc) {
  r.cb(r.user, rc != COA_OK ? rc : verdict_rc, reinterpret_cast<const uint8_t*>(words.data() + r.idx), 4);
}
// The request's callback with the launch's (or the resolver pass's) status
// and its output in the window.
inline void answer_req(const Req& r, const Window& w, int rc, int verdict_rc) {
  switch (r.kind) {
    case K_CERT_V: answer_word(r, w.c_words, rc, verdict_rc); break;
    case K_HEADER_V: answer_word(r, w.hd_words, rc, verdict_rc); break;
    case K_VOTE_V: answer_word(r, w.vt_words, rc, verdict_rc); break;
    case K_VERIFY: r.cb(r.user, rc, w.v_out.data() + r.idx, r.n); break;
    case K_BATCH: r.cb(r.user, rc, w.g_out.data() + r.idx, 1); break;
    case K_CERT: r.cb(r.user, rc, w.c_out.data() + r.idx, 1); break;
    case K_DIGEST: r.cb(r.user, rc, w.d_out.data() + (size_t)r.idx * 32, 32); break;
    case K_HEADER: r.cb(r.user, rc, w.hd_out.data() + r.idx, 1); break;
    case K_VOTE: r.cb(r.user, rc, w.vt_out.data() + r.idx, 1); break;
  }
}

constexpr size_t kShards = 64;  // intake shards per queue
// bounded spins around a shard's lock: the collector's pause-spin on try_lock
// before it yields between tries (~tens of microseconds), and a producer's
// yields to a `taking` collector before it queues on the lock anyway
constexpr int kGatherSpins = 4096;
constexpr int kTakingYields = 2000;
constexpr size_t kReport = 64;  // a shard tells the pending count every kReport items
constexpr size_t kSpares = 4;   // recycled windows kept per shard

// One intake shard.  `reported` is the part of `items` already added to the
// queue's pending count.
struct alignas(64) Shard {
  std::mutex mu;
  // set while the collector waits to take the shard: a producer submitting
  // in a tight loop re-takes the (unfair) mutex within nanoseconds of
  // releasing it, and a round-4 take waited 60-310 us per window for a gap;
  // producers hold off while it is set, so a take waits for one copy at most
  std::atomic<bool> taking{false};
  std::unique_ptr<Window> w;
  std::vector<Req> reqs;
  size_t items = 0, reported = 0;
  // recycled windows and request vectors for the next takes (capacity kept):
  // up to kSpares each, because with several windows in flight a shard's
  // windows come back later than it needs the next one -- a fresh Window
  // grows its vectors from nothing, on new pages (round 4's streamed C3:
  // producers copied at ~3 GB/s, the collector's take cost 60-190 us)
  std::vector<std::unique_ptr<Window>> spares;
  std::vector<std::vector<Req>> spare_reqs;

  Shard() { w = fresh(); }  // in the body: fresh() reads spares, declared after w
  // An empty window: a spare, or a new one (mu held, or nobody else yet).
  std::unique_ptr<Window> fresh() {
    std::unique_ptr<Window> f;
    if (!spares.empty()) {
      f = std::move(spares.back());
      spares.pop_back();
    } else {
      f.reset(new Window());
      f->reset();
    }
    return f;
  }
  // The collector's take (mu held): the filled window and its requests out
  // (`out` comes in empty), a fresh window and a spare request vector in.
  std::unique_ptr<Window> take(std::vector<Req>& out) {
    std::unique_ptr<Window> full = std::move(w);
    out.swap(reqs);
    w = fresh();
    if (!spare_reqs.empty()) {
      reqs.swap(spare_reqs.back());
      spare_reqs.pop_back();
    }
    items = reported = 0;
    return full;
  }
  // An answered window and/or request vector (either may be null) back into
  // the pool: emptied without the lock, kept under mu while fewer than
  // kSpares are (otherwise left with the caller).
  void recycle(std::unique_ptr<Window>& win, std::vector<Req>* rq) {
    if (win) win->reset();
    if (rq) rq->clear();
    std::lock_guard<std::mutex> g(mu);
    if (win && spares.size() < kSpares) spares.push_back(std::move(win));
    if (rq && spare_reqs.size() < kSpares) spare_reqs.push_back(std::move(*rq));
  }
};

// One shard's requests inside a launch.  Also the requests of a part that
// the backend left open (Window::c_defer, m_defer, g_defer), with the part's
// window (moved out of the flight, not recycled): the resolver thread decides
// them, answers their callbacks and returns the window to the shard's pool.
struct Part {
  std::unique_ptr<Window> w;
  std::vector<Req> reqs;
  uint32_t shard;
};

struct Flight {
  std::vector<Part> parts;
  Launch L;
  int64_t t_launch = 0;  // ns, when the collector handed the window to the backend
};

std::atomic<uint64_t> g_queue_ids{1};
std::atomic<uint32_t> g_thread_ord{0};

uint32_t thread_ordinal() {
  static thread_local const uint32_t ord = g_thread_ord.fetch_add(1, std::memory_order_relaxed);
  return ord;
}

// Callback helpers: the completion thread answers a large launch together
// with kHelpers threads, each taking contiguous runs of requests (a launch
// of 10^5 single signatures is 10^5 callbacks: on one thread they, not the
// GPU, set the queue's rate).  Launches still complete in order: the next
// one starts only when every run of this one has been answered.
constexpr int kHelpersDefault = 3;         // COA_QUEUE_HELPERS overrides (0..15; read at queue creation)
constexpr size_t kParallelAnswer = 8192;  // requests per launch from which the helpers join
constexpr size_t kRun = 4096;             // requests per run

// True on the queue's own completion, helper and resolver threads: a
// callback that submits must not launch from there (a launch can wait for a
// free slot, and only those threads free slots).
thread_local bool t_queue_thread = false;

struct AnswerPool {
  std::mutex m;
  std::condition_variable cv, done_cv;
  std::function<void(size_t)> job;
  size_t runs = 0, next = 0, done = 0;
  uint64_t gen = 0;
  bool stop = false;
  std::vector<std::thread> th;

  void start(int n) {
    for (int i = 0; i < n; i++)
      th.emplace_back([this] {
        t_queue_thread = true;
        loop();
      });
  }
  ~AnswerPool() {
    {
      std::lock_guard<std::mutex> l(m);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
  // Runs f(0..n-1) on the helpers and the calling thread; returns when all ran.
  void run(size_t n, std::function<void(size_t)> f) {
    {
      std::lock_guard<std::mutex> l(m);
      job = std::move(f);
      runs = n;
      next = 0;
      done = 0;
      gen++;
    }
    cv.notify_all();
    work();
    std::unique_lock<std::mutex> l(m);
    done_cv.wait(l, [&] { return done == runs; });
    job = nullptr;
  }

 private:
  // takes runs until none is left (caller or helper)
  void work() {
    for (;;) {
      size_t i;
      std::function<void(size_t)>* f;
      {
        std::lock_guard<std::mutex> l(m);
        if (next >= runs) return;
        i = next++;
        f = &job;
      }
      (*f)(i);
      std::lock_guard<std::mutex> l(m);
      if (++done == runs) done_cv.notify_all();
    }
  }
  void loop() {
    uint64_t seen = 0;
    for (;;) {
      {
        std::unique_lock<std::mutex> l(m);
        cv.wait(l, [&] { return stop || (gen != seen && next < runs); });
        if (stop) return;
        seen = gen;
      }
      work();
    }
  }
};

// One lane of a queue: intake shards, collector, backend slots, completer.
struct Lane {
  size_t max_batch = 65536;
  // A window closed while every slot is busy waits for a slot first; if a
  // backlog of at least backlog_min windows (of max_batch items) built up
  // meanwhile, the window takes up to backlog_batch items of it instead of
  // max_batch.  Round 6's paced C3 stream (max_batch 16,384: windows of ~240
  // certificates) was slot-bound at ~2.4 M certificates/s, so 3 M/s offered
  // built a backlog (p99 7.4-8.7 ms); with backlog windows of 32,768 items
  // it keeps up (2.93 M/s achieved, p99 1.5-1.7 ms, profiles/
  // r06_backlog_ab.txt).  Windows grown further (65,536) serialise the
  // backlog on one slot's quarter of the CUs and fell behind again (2.2-2.7
  // M/s); grown at a backlog of one window they raised the 2 M/s p99 from
  // 0.86 to 1.5-5.9 ms.  COA_QUEUE_BACKLOG_BATCH (read at creation; 0 = off)
  // and COA_QUEUE_BACKLOG_MIN override; default min(2 x max_batch, 65,536)
  // (never below max_batch) on the verify lane, off on the digest lane.
  size_t backlog_batch = 65536;
  double backlog_min = 2.0;
  size_t reserve_items = 131072;  // Window::reserve_for's items (coa_queue_create)
  bool digest_lane = false;
  std::atomic<bool> prepared{false};  // slots' streams and staging set up (coa_queue_create or the first window)
  std::chrono::microseconds max_delay{500};
  std::unique_ptr<coa_q::Backend> be;
  std::unique_ptr<Shard[]> shards{new Shard[kShards]};

  std::mutex mu;
  std::condition_variable cv;         // collector: requests arrived / flush / stop
  std::condition_variable flight_cv;  // completer: a window was launched / stop
  std::condition_variable idle_cv;    // flush: everything answered
  std::condition_variable resolve_cv; // resolver: open requests deferred / stop
  std::atomic<int64_t> pend{0};  // reported items not yet taken (briefly < 0 while a take races a report)
  std::atomic<bool> stop{false};
  std::chrono::steady_clock::time_point oldest;
  std::deque<Flight> flight;  // launched, not yet answered (launch order)
  size_t busy = 0;            // windows taken by the collector and not yet answered
  bool flush = false, collector_done = false;
  int collectors_live = 0;  // collector threads not yet exited
  std::deque<Part> open;  // deferred parts waiting for the resolver
  size_t resolving = 0;   // deferred parts not yet answered (queued or in a pass)
  bool resolver_stop = false;
  bool idle() const { return pend.load() <= 0 && busy == 0 && resolving == 0; }

  // metrics: under mu, except m_max_pending (producers raise it without mu)
  LaneMetrics m{now_ns()};  // epoch_ns; the rest zero
  std::atomic<int64_t> m_max_pending{0};

  // COA_QUEUE_COLLECTORS (1..4, default 2; read at creation): collector
  // threads.  A window's pack (its requests' bytes into the slot's
  // page-locked staging, ~13 MB for a streamed C3 window) runs on the thread
  // that closed the window, so with one collector the next window could not
  // be gathered until that pack was done: the streamed C3 path's bound
  // (gather + pack + enqueue ~300 us per window of ~1,300 certificates, one
  // thread).  A second collector closes and packs the next window meanwhile.
  std::vector<std::thread> collectors;
  std::thread completer, resolver;
  std::mutex prep_mu;  // one prepare() (cold lane) at a time
  AnswerPool helpers;  // started lazily by the first large launch
  int n_helpers = kHelpersDefault;
  bool helpers_on = false;
  // COA_QUEUE_IDLE_LAUNCH (read at creation; 0 = off, the default): a window
  // closes at once while fewer than this many windows are in flight
  size_t idle_launch = 0;
  // With idle launch, a request that finds the engine idle is launched by
  // the submitting thread itself (COA_QUEUE_DIRECT=0: by the collector, as
  // before): no wake-up of the collector thread on a lone request's path
  bool direct_ok = true;
  std::mutex gather_mu;  // one gather at a time (the collector, or a submitter launching directly)
  double trace_slow_us = 0;  // COA_QUEUE_TRACE_SLOW_US (read at creation): report slower windows on stderr

  void start() {
    const int n = (int)env_int("COA_QUEUE_COLLECTORS", 2, 1, 4);
    collectors_live = n;
    for (int i = 0; i < n; i++) collectors.emplace_back([this] { collect(); });
    completer = std::thread([this] { answer(); });
    resolver = std::thread([this] { resolve_loop(); });
  }

  // The calling thread's shard, locked into `sl`; a shard whose window already
  // holds max_batch items sends the request on to the next one (the
  // collector takes whole shards, so one busy producer thread would otherwise
  // build a window of any size behind a backlog: 254,184 items of streamed
  // certificates, 920 worker batches at 4,000 batches/s).  The last shard
  // tried takes the overflow.
  Shard& intake(std::unique_lock<std::mutex>& sl) {
    const size_t home = thread_ordinal() % kShards;
    for (size_t k = 0;; k++) {
      Shard& sh = shards[(home + k) % kShards];
      // the collector is taking this shard: let it have the lock first (a
      // producer that takes it back at once starves the collector: a bounded
      // pause-spin here cut the 1-producer C3 stream from 3.7 to 1.2 M/s), by
      // yielding -- bounded, so a descheduled collector cannot park the
      // shard's producers for long
      for (int y = 0; y < kTakingYields && sh.taking.load(std::memory_order_acquire); y++) std::this_thread::yield();
      sl = std::unique_lock<std::mutex>(sh.mu);
      if (sh.items < max_batch || k + 1 == kShards) return sh;
    }
  }

  // `items` more items were reported by a shard (its lock released).  Wakes
  // the collector only on the two edges it waits for: the first pending item
  // (arms the deadline) and max_batch reached.
  void arrived(size_t items) {
    const int64_t old = pend.fetch_add((int64_t)items), now_pend = old + (int64_t)items;
    int64_t mx = m_max_pending.load(std::memory_order_relaxed);
    while (now_pend > mx && !m_max_pending.compare_exchange_weak(mx, now_pend, std::memory_order_relaxed)) {
    }
    const bool first = old <= 0 && now_pend > 0;
    const bool crossed = old < (int64_t)max_batch && now_pend >= (int64_t)max_batch;
    if (first || crossed) {
      std::unique_lock<std::mutex> l(mu);
      if (first) oldest = std::chrono::steady_clock::now();
      // idle launch on an idle engine: this thread takes the window and
      // launches it at once (the collector's wake-up was most of a lone
      // request's queueing at low rates, where its thread has gone to sleep)
      if (first && direct_ok && !t_queue_thread && busy < idle_launch && busy < (size_t)be->slots() && !stop.load() &&
          !flush && prepared.load() && pend.load() > 0) {
        busy++;
        launch_window(l);
        return;
      }
      cv.notify_one();
    }
  }

  // Non-empty shards' windows into f (the collector, no queue lock): whole
  // shards, starting one shard further each window, until f holds `cap`
  // items (max_batch, or backlog_batch after a wait for a slot); the rest waits for the next window (which the collector then
  // closes at once: pend is still >= max_batch).
  size_t rr = 0;
  void gather(Flight& f, size_t cap) {
    const size_t start = rr++ % kShards;
    size_t taken = 0;
    for (size_t k = 0; k < kShards && taken < cap; k++) {
      const uint32_t si = (uint32_t)((start + k) % kShards);
      Shard& sh = shards[si];
      Part p;
      size_t items, rep;
      {
        // spin, not sleep: the holder is inside one copy and will not re-take
        // the lock while `taking` is set (a futex sleep here cost a scheduling
        // round trip per shard under load) -- for a bounded number of tries,
        // then yield between tries: gather may run on a submitting thread
        // (direct launch), which must not burn a core while the holder is
        // descheduled.  Never a blocking lock(): a producer that got the
        // mutex back first would starve the collector
        sh.taking.store(true, std::memory_order_release);
        for (int spin = 0; !sh.mu.try_lock(); spin++) {
          if (spin < kGatherSpins)
            cpu_relax();
          else
            std::this_thread::yield();
        }
        std::lock_guard<std::mutex> l(sh.mu, std::adopt_lock);
        sh.taking.store(false, std::memory_order_release);
        if (sh.items == 0) continue;
        items = sh.items;
        rep = sh.reported;
        p.w = sh.take(p.reqs);
      }
      pend.fetch_sub((int64_t)rep);
      taken += items;
      p.shard = si;
      f.parts.push_back(std::move(p));
    }
    f.L.parts.clear();
    for (Part& p : f.parts) {
      p.w->bind();
      f.L.parts.push_back(p.w.get());
      f.L.stage_ns[COA_QSTAGE_INTAKE] += p.w->intake_ns;
    }
    f.L.tally();
  }

  void collect() {
    std::unique_lock<std::mutex> l(mu);
    for (;;) {
      cv.wait(l, [&] { return stop.load() || pend.load() > 0; });
      if (stop.load() && pend.load() <= 0) break;  // stop with nothing pending
      // window is open: close it when full, at the deadline, on flush or
      // stop, or (idle launch) while fewer than idle_launch windows are in
      // flight -- the completer wakes the collector when one is answered
      while (!stop.load() && !flush && pend.load() < (int64_t)max_batch && busy >= idle_launch) {
        if (cv.wait_until(l, oldest + max_delay) == std::cv_status::timeout) break;
      }
      flush = false;
      busy++;  // before the take: flush must not see pend == 0 and busy == 0 meanwhile
      launch_window(l);
    }
    if (--collectors_live == 0) {  // the last collector out (under mu)
      collector_done = true;
      flight_cv.notify_one();
    }
  }

  // Takes the pending requests as one window and launches it: the collector,
  // or (idle launch) a submitting thread that found the engine idle.  Called
  // with `l` holding mu and busy already counting the window; returns with
  // `l` held.
  void launch_window(std::unique_lock<std::mutex>& l) {
    Flight f;
    l.unlock();
    take_window(f);
    l.lock();
    if (f.parts.empty()) {  // every pending item was taken by an earlier window
      busy--;
      if (idle()) idle_cv.notify_all();
      return;
    }
    m.max_window = std::max<uint64_t>(m.max_window, f.L.items());
    l.unlock();
    launch(f);
    l.lock();
    m.windows++;
    flight.push_back(std::move(f));
    m.max_in_flight = std::max<uint64_t>(m.max_in_flight, flight.size());
    flight_cv.notify_one();
  }

  // The pending requests into f (no queue lock).  Every slot busy: waits for
  // one before taking the window, which grows to backlog_batch items if a
  // backlog built up meanwhile (see backlog_batch).
  void take_window(Flight& f) {
    size_t cap = max_batch;
    const int64_t tw = now_ns();
    if (be->wait_free_slot()) {
      if ((double)pend.load() >= backlog_min * (double)max_batch) cap = backlog_batch;
      f.L.stage_ns[COA_QSTAGE_SLOT_WAIT] += now_ns() - tw;
    }
    const int64_t tg = now_ns();
    {
      std::lock_guard<std::mutex> g(gather_mu);
      gather(f, cap);
    }
    f.L.stage_ns[COA_QSTAGE_GATHER] += now_ns() - tg;
  }

  // Hands the taken window to the backend (no queue lock).
  void launch(Flight& f) {
    f.L.reset_outputs();
    f.L.attempts = 1;
    f.t_launch = now_ns();
    if (!prepared.load()) {  // a lane COA_QUEUE_LANES left cold: set up by its first window (the collector's)
      std::lock_guard<std::mutex> p(prep_mu);
      if (!prepared.load()) {
        be->prepare(backlog_batch);
        prepared.store(true);
      }
    }
    be->launch(f.L);  // stages and enqueues; blocks only while every slot is busy
    f.L.stage_ns[COA_QSTAGE_SLOT_WAIT] += f.L.slot_wait_ns;
  }

  // The completer: per window, in launch order, the steps below.  Callbacks,
  // then the windows back to their shards, then busy-- / idle_cv: what
  // coa_queue_flush relies on.
  void answer() {
    t_queue_thread = true;
    std::unique_lock<std::mutex> l(mu);
    for (;;) {
      flight_cv.wait(l, [&] { return !flight.empty() || collector_done; });
      if (flight.empty()) return;
      Flight f = std::move(flight.front());
      flight.pop_front();
      l.unlock();
      be->complete(f.L);
      const double window_us = (double)(now_ns() - f.t_launch) * 1e-3;
      trace_slow(f, window_us);
      const bool retried = recover(f.L);
      const bool any_open = mark_open(f);
      const WaitTally waits = run_callbacks(f, any_open);
      std::vector<Part> jobs;
      if (any_open) jobs = split_open(f);
      for (Part& p : f.parts) shards[p.shard].recycle(p.w, &p.reqs);
      l.lock();
      m.record(f.L, f.t_launch, window_us, retried, waits);
      if (!jobs.empty()) {
        resolving += jobs.size();
        for (Part& d : jobs) open.push_back(std::move(d));
        resolve_cv.notify_one();
      }
      busy--;
      if (idle()) idle_cv.notify_all();
      if (idle_launch && busy < idle_launch && pend.load() > 0) cv.notify_one();
    }
  }

  // COA_QUEUE_TRACE_SLOW_US (diagnostics): a window slower than that, with
  // its stages, on stderr.
  void trace_slow(const Flight& f, double window_us) const {
    if (!(trace_slow_us > 0 && window_us > trace_slow_us)) return;
    const Launch& L = f.L;
    fprintf(stderr,
            "[coa queue] slow window %.0f us at t=%.6f s: %zu items kinds %u slot %d; slot_wait %.0f pack %.0f "
            "enqueue %.0f (pin %.0f h2d %.0f launch %.0f d2h %.0f event %.0f) device_wait %.0f scatter %.0f us\n",
            window_us, (double)f.t_launch * 1e-9, L.items(), L.kinds(), L.slot, L.stage_ns[COA_QSTAGE_SLOT_WAIT] * 1e-3,
            L.stage_ns[COA_QSTAGE_PACK] * 1e-3, L.stage_ns[COA_QSTAGE_ENQUEUE] * 1e-3, L.enq_ns[Launch::ENQ_PIN] * 1e-3,
            L.enq_ns[Launch::ENQ_H2D] * 1e-3, L.enq_ns[Launch::ENQ_LAUNCH] * 1e-3, L.enq_ns[Launch::ENQ_D2H] * 1e-3,
            L.enq_ns[Launch::ENQ_EVENT] * 1e-3, L.stage_ns[COA_QSTAGE_DEVICE_WAIT] * 1e-3,
            L.stage_ns[COA_QSTAGE_SCATTER] * 1e-3);
  }

  // A launch that failed on the device (a HIP error or an allocation
  // failure; not "no device" or bad arguments): retried on the recovery
  // context of each device in turn (the first retry on the next device),
  // until one succeeds.  True if the launch had failed.
  static bool recoverable(int rc) { return rc == COA_EHIP || rc == COA_ENOMEM; }
  bool recover(Launch& L) {
    if (!recoverable(L.rc)) return false;
    const int n = std::max(1, be->devices());
    for (int a = 1; a <= n && recoverable(L.rc); a++) {
      L.reset_outputs();
      L.attempts++;
      be->retry(L, a);
    }
    return true;
  }

  // True if the backend left requests of the window open: those go to the
  // resolver, the rest are answered now.  A failed window leaves nothing
  // open: every request gets the error.
  static bool mark_open(Flight& f) {
    bool any = false;
    for (Part& p : f.parts) {
      if (f.L.rc != COA_OK) p.w->close_open();
      any = any || p.w->deferred();
    }
    return any;
  }

  // The callbacks of the window's requests (not the open ones), in runs of
  // contiguous requests -- the helpers join for large launches -- with the
  // wait times from a clock read every 32 requests.
  WaitTally run_callbacks(Flight& f, bool any_open) {
    const int64_t tcb = now_ns();
    const int rc = f.L.rc;
    struct Run {
      const Part* p;
      size_t lo, hi;
    };
    std::vector<Run> runs;
    size_t nreq = 0;
    for (const Part& p : f.parts) {
      for (size_t lo = 0; lo < p.reqs.size(); lo += kRun) runs.push_back({&p, lo, std::min(p.reqs.size(), lo + kRun)});
      nreq += p.reqs.size();
    }
    std::vector<WaitTally> tallies(runs.size());
    auto answer_run = [&](size_t ri) {
      const Run& g = runs[ri];
      const Window& w = *g.p->w;
      WaitTally& t = tallies[ri];
      int64_t tnow = now_ns();
      for (size_t k = g.lo; k < g.hi; k++) {
        const Req& r = g.p->reqs[k];
        if (any_open && is_deferred(r, w)) continue;  // the resolver answers it
        if (((k - g.lo) & 31) == 31) tnow = now_ns();
        t.add((double)(tnow - r.t0) * 1e-3);
        answer_req(r, w, rc, f.L.verdict_rc);
      }
    };
    if (n_helpers > 0 && nreq >= kParallelAnswer && runs.size() > 1) {
      if (!helpers_on) {
        helpers.start(n_helpers);
        helpers_on = true;
      }
      helpers.run(runs.size(), answer_run);
    } else {
      for (size_t ri = 0; ri < runs.size(); ri++) answer_run(ri);
    }
    f.L.stage_ns[COA_QSTAGE_CALLBACKS] += now_ns() - tcb;
    WaitTally all;
    for (const WaitTally& t : tallies) all.merge(t);
    return all;
  }

  // The open requests, with their windows (moved out of the flight), for the
  // resolver.
  static std::vector<Part> split_open(Flight& f) {
    std::vector<Part> jobs;
    for (Part& p : f.parts) {
      if (!p.w->deferred()) continue;
      Part d;
      for (const Req& r : p.reqs)
        if (is_deferred(r, *p.w)) d.reqs.push_back(r);
      d.w = std::move(p.w);
      d.shard = p.shard;
      jobs.push_back(std::move(d));
    }
    return jobs;
  }

  // The resolver: takes every deferred part queued so far, has the backend
  // decide them in one pass (one engine call per kind for all of them), and
  // answers their callbacks -- off the completion thread, so the windows
  // behind an open certificate are answered while it is being decided.  A
  // pass that failed answers them with the engine error and "failed" values.
  // The windows go back to their shards' pools (their request vectors were
  // the completer's to recycle).
  void resolve_loop() {
    t_queue_thread = true;
    std::unique_lock<std::mutex> l(mu);
    for (;;) {
      resolve_cv.wait(l, [&] { return !open.empty() || resolver_stop; });
      if (open.empty()) return;
      std::vector<Part> jobs;
      while (!open.empty()) {
        jobs.push_back(std::move(open.front()));
        open.pop_front();
      }
      l.unlock();
      const int64_t t0 = now_ns();
      std::vector<Window*> ws;
      for (Part& d : jobs) ws.push_back(d.w.get());
      const int rc = be->resolve(ws);
      if (rc != COA_OK)
        for (Window* w : ws) w->fail_open();
      const int64_t t1 = now_ns();
      WaitTally waits;
      for (const Part& d : jobs)
        for (const Req& r : d.reqs) {
          waits.add((double)(now_ns() - r.t0) * 1e-3);
          answer_req(r, *d.w, rc, COA_OK);
        }
      const int64_t t2 = now_ns();
      for (Part& d : jobs) shards[d.shard].recycle(d.w, nullptr);
      l.lock();
      m.record_pass(waits, (double)(t1 - t0) * 1e-3, (double)(t2 - t1) * 1e-3);
      resolving -= jobs.size();
      if (idle()) idle_cv.notify_all();
    }
  }

  void reset_metrics() {
    std::lock_guard<std::mutex> l(mu);
    m = LaneMetrics{now_ns()};
    m_max_pending.store(0);
    be->reset_grows();
  }

  void shutdown() {
    {
      std::lock_guard<std::mutex> l(mu);
      stop = true;
      cv.notify_all();
    }
    for (std::thread& c : collectors) c.join();
    completer.join();
    {
      std::lock_guard<std::mutex> l(mu);
      resolver_stop = true;
      resolve_cv.notify_one();
    }
    resolver.join();
  }

  int flush_all() {
    std::unique_lock<std::mutex> l(mu);
    if (idle()) return COA_OK;
    if (pend.load() > 0) {
      flush = true;
      cv.notify_one();
    }
    idle_cv.wait(l, [&] { return idle(); });
    return COA_OK;
  }
};

}  // namespace

struct coa_queue {
  const uint64_t id = g_queue_ids.fetch_add(1);
  Lane lanes[coa_q::LANES];
  Lane& lane_of(Kind k) { return lanes[k == K_DIGEST ? coa_q::LANE_DIGEST : coa_q::LANE_VERIFY]; }
};

namespace {
// A submission's intake: the request goes into the calling thread's shard of
// the kind's lane under that shard's lock (held from the constructor to
// done(), or to the destructor if the lane is stopping); then the lane's
// pending count (and, on an edge, its collector) learns of it.
struct Intake {
  const int64_t t_in = now_ns();
  Lane& ln;
  std::unique_lock<std::mutex> sl;
  Shard& sh;
  Window& w;  // the shard's open window, its capacity reserved
  Intake(coa_queue* q, Kind kind) : ln(q->lane_of(kind)), sh(ln.intake(sl)), w(*sh.w) {
    if (ok() && !w.reserved) w.reserve_for(ln.reserve_items, ln.digest_lane);
  }
  bool ok() const { return !ln.stop.load(); }
  // The request is in the window as the kind's idx-th (n: a K_VERIFY
  // request's signatures), `items` items more for the collector.
  void done(Kind kind, uint32_t idx, uint32_t n, size_t items, coa_verdict_cb cb, void* user) {
    sh.reqs.push_back(Req{cb, user, t_in, idx, n, kind});
    w.intake_ns += now_ns() - t_in;
    sh.items += items;
    size_t delta = 0;
    if (sh.reported == 0 || sh.items - sh.reported >= kReport) {
      delta = sh.items - sh.reported;
      sh.reported = sh.items;
    }
    sl.unlock();
    if (delta) ln.arrived(delta);
  }
};

template <size_t N>
inline void put(std::vector<uint8_t>& v, const uint8_t* src) {
  v.insert(v.end(), src, src + N);  // one copy (resize would zero the bytes first)
}

// A certificate request: `r` holds the caller's pointers; a copy (r.owned)
// appends their bytes to the window's own buffer, one append per
// field, and keeps the offsets (bind() turns them into pointers at the take).
// `pcount`: a verdict request's payload count (null: a crypto request).
inline bool count_fits(uint32_t payload_count, size_t header_len) {
  return payload_count == 0 || 40 + 36 * (uint64_t)payload_count <= header_len;
}
// Item idx of a kind becomes a verdict request: its flag and, for the kinds
// that have one, its payload count (the vectors reach as far as idx).
inline void mark_verdict(std::vector<uint8_t>& vreq, std::vector<uint32_t>* pcounts, size_t idx, uint32_t pcount) {
  vreq.resize(idx + 1, 0);
  vreq[idx] = 1;
  if (pcounts) {
    pcounts->resize(idx + 1, 0);
    (*pcounts)[idx] = pcount;
  }
}
inline int submit_cert(coa_queue* q, Window::CertRef r, coa_verdict_cb cb, void* user,
                       const uint32_t* pcount = nullptr) {
  if (!q || (r.hlen && !r.hdr) || !r.id || !r.origin || !r.hsig || (r.nv && (!r.vpks || !r.vsigs)) || !cb)
    return COA_EINVAL;
  if (pcount && !count_fits(*pcount, r.hlen)) return COA_EINVAL;
  Intake in(q, K_CERT);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  if (r.owned) {
    std::vector<uint8_t>& o = w.c_own;
    auto own = [&o](const uint8_t*& field, size_t len) {
      const uint8_t* src = field;
      field = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(o.size()));
      if (len) o.insert(o.end(), src, src + len);
    };
    own(r.hdr, r.hlen);
    own(r.id, 32);
    own(r.origin, 32);
    own(r.hsig, 64);
    own(r.vpks, r.nv * 32);
    own(r.vsigs, r.nv * 64);
  }
  w.c_refs.push_back(r);
  w.c_votes += r.nv;
  w.c_hbytes += r.hlen;
  if (pcount) {
    mark_verdict(w.c_vreq, &w.c_pcounts, w.nc, *pcount);
    w.n_vc++;
  }
  in.done(pcount ? K_CERT_V : K_CERT, (uint32_t)w.nc++, 1, 1 + r.nv, cb, user);
  return COA_OK;
}

inline int submit_header(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t* id,
                         const uint8_t* author, const uint8_t* sig, coa_verdict_cb cb, void* user,
                         const uint32_t* pcount = nullptr) {
  if (!q || (header_len && !header_data) || !id || !author || !sig || !cb) return COA_EINVAL;
  if (pcount && !count_fits(*pcount, header_len)) return COA_EINVAL;
  Intake in(q, K_HEADER);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  if (header_len) w.hd_data.insert(w.hd_data.end(), header_data, header_data + header_len);
  w.hd_offs.push_back(w.hd_data.size());
  put<32>(w.hd_ids, id);
  put<32>(w.hd_authors, author);
  put<64>(w.hd_sigs, sig);
  if (pcount) {
    mark_verdict(w.hd_vreq, &w.hd_pcounts, w.nhd, *pcount);
    w.n_vh++;
  }
  in.done(pcount ? K_HEADER_V : K_HEADER, (uint32_t)w.nhd++, 1, 1, cb, user);
  return COA_OK;
}

inline int submit_vote(coa_queue* q, const uint8_t* id, uint64_t round, const uint8_t* origin, const uint8_t* author,
                       const uint8_t* sig, coa_verdict_cb cb, void* user, bool verdict) {
  if (!q || !id || !origin || !author || !sig || !cb) return COA_EINVAL;
  Intake in(q, K_VOTE);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  put<32>(w.vt_ids, id);
  w.vt_rounds.push_back(round);
  put<32>(w.vt_origins, origin);
  put<32>(w.vt_authors, author);
  put<64>(w.vt_sigs, sig);
  if (verdict) {
    mark_verdict(w.vt_vreq, nullptr, w.nvt, 0);
    w.n_vvt++;
  }
  in.done(verdict ? K_VOTE_V : K_VOTE, (uint32_t)w.nvt++, 1, 1, cb, user);
  return COA_OK;
}
}  // namespace

extern "C" {

coa_queue* coa_queue_create(size_t max_batch, uint32_t max_delay_us) {
  coa_queue* q = new coa_queue();
  for (int k = 0; k < coa_q::LANES; k++) {
    Lane& L = q->lanes[k];
    L.max_batch = max_batch ? max_batch : 65536;
    if (k == coa_q::LANE_DIGEST) {
      // Digest windows hold whole ~500 KB worker batches: at most
      // COA_QUEUE_DIGEST_MAX (default 96, ~49 MB) per window, so a backlog
      // is split over the lane's slots and the staging warmed at creation
      // (2 x 32 MB per slot) is never regrown on the launch path.  Unbounded,
      // a backlog at 4,000 batches/s became windows of up to 920 batches
      // (467 MB) whose page-locked regrowth held a window 218-234 ms.
      const size_t cap = (size_t)env_int("COA_QUEUE_DIGEST_MAX", 96, 1, 0x7fffffff);
      L.max_batch = std::min(L.max_batch, cap);
    }
    L.max_delay = std::chrono::microseconds(max_delay_us);
    L.digest_lane = k == coa_q::LANE_DIGEST;
    // windows reserve their capacity on first use (a shard no producer
    // thread maps to never does): twice max_batch items, capped at 2 x 65,536
    // -- a larger max_batch's windows grow past it on demand
    L.reserve_items = 2 * std::min<size_t>(L.max_batch, 65536);
    L.backlog_batch = k == coa_q::LANE_DIGEST ? L.max_batch
                                              : std::max<size_t>(L.max_batch, std::min<size_t>(2 * L.max_batch, 65536));
    // each switch, where set, replaces the default above
    const long bb = env_int("COA_QUEUE_BACKLOG_BATCH", (long)L.backlog_batch);
    L.backlog_batch = bb <= 0 ? L.max_batch : std::max<size_t>(L.max_batch, (size_t)bb);
    L.backlog_min = std::max(0.0, env_double("COA_QUEUE_BACKLOG_MIN", L.backlog_min));
    L.n_helpers = (int)env_int("COA_QUEUE_HELPERS", L.n_helpers, 0, 15);
    L.idle_launch = (size_t)env_int("COA_QUEUE_IDLE_LAUNCH", (long)L.idle_launch, 0, 64);
    L.direct_ok = env_on("COA_QUEUE_DIRECT", L.direct_ok);
    L.trace_slow_us = env_double("COA_QUEUE_TRACE_SLOW_US", L.trace_slow_us);
    L.be.reset(coa_q::make_backend(k));
    // COA_QUEUE_LANES=verify|digest|verify,digest (read at creation; default
    // both): the lanes set up now -- streams, their first dispatch, staging
    // (a verify slot ~23 MB page-locked + ~320 MB of HBM at max_batch 65,536,
    // a digest slot 64 + 64 MB; four verify and eight digest slots per GPU).  A primary that never
    // hashes worker batches, or a worker that never verifies, names its lane;
    // the other is set up by its first window (which then waits ~25-75 ms).
    const char* lanes = env_str("COA_QUEUE_LANES");
    const bool warm = !lanes || std::strstr(lanes, k == coa_q::LANE_DIGEST ? "digest" : "verify") != nullptr;
    if (warm) {
      L.be->prepare(L.backlog_batch);
      L.prepared.store(true);
    }
    L.start();
  }
  return q;
}

// The submissions (Intake above): arguments checked, the request's bytes
// appended to the shard's window, done().
int coa_queue_submit_verify(coa_queue* q, const uint8_t msg[32], const uint8_t pk[32], const uint8_t sig[64],
                            coa_verdict_cb cb, void* user) {
  if (!q || !msg || !pk || !sig || !cb) return COA_EINVAL;
  Intake in(q, K_VERIFY);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  put<32>(w.v_msgs, msg);
  put<32>(w.v_pks, pk);
  put<64>(w.v_sigs, sig);
  in.done(K_VERIFY, (uint32_t)w.nv++, 1, 1, cb, user);
  return COA_OK;
}

int coa_queue_submit_verify_many(coa_queue* q, const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, size_t n,
                                 coa_verdict_cb cb, void* user) {
  if (!q || !cb || n == 0 || n > UINT32_MAX || !msgs || !pks || !sigs) return COA_EINVAL;
  Intake in(q, K_VERIFY);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  w.v_msgs.insert(w.v_msgs.end(), msgs, msgs + n * 32);
  w.v_pks.insert(w.v_pks.end(), pks, pks + n * 32);
  w.v_sigs.insert(w.v_sigs.end(), sigs, sigs + n * 64);
  const uint32_t idx = (uint32_t)w.nv;
  w.nv += n;
  in.done(K_VERIFY, idx, (uint32_t)n, n, cb, user);
  return COA_OK;
}

int coa_queue_submit_batch(coa_queue* q, const uint8_t msg[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                           coa_verdict_cb cb, void* user) {
  if (!q || !msg || (n && (!pks || !sigs)) || !cb) return COA_EINVAL;
  Intake in(q, K_BATCH);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  put<32>(w.g_msgs, msg);
  if (n) {
    w.g_pks.insert(w.g_pks.end(), pks, pks + n * 32);
    w.g_sigs.insert(w.g_sigs.end(), sigs, sigs + n * 64);
  }
  w.g_offs.push_back(w.g_offs.back() + n);
  in.done(K_BATCH, (uint32_t)w.ng++, 1, n ? n : 1, cb, user);
  return COA_OK;
}

int coa_queue_submit_certificate(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                                 const uint8_t origin[32], const uint8_t header_sig[64], uint64_t round,
                                 const uint8_t* vote_pks, const uint8_t* vote_sigs, size_t n_votes, coa_verdict_cb cb,
                                 void* user) {
  return submit_cert(q, {header_data, id, origin, header_sig, vote_pks, vote_sigs, header_len, round, n_votes, true},
                     cb, user);
}

int coa_queue_submit_certificate_borrowed(coa_queue* q, const uint8_t* header_data, size_t header_len,
                                          const uint8_t id[32], const uint8_t origin[32], const uint8_t header_sig[64],
                                          uint64_t round, const uint8_t* vote_pks, const uint8_t* vote_sigs,
                                          size_t n_votes, coa_verdict_cb cb, void* user) {
  return submit_cert(q, {header_data, id, origin, header_sig, vote_pks, vote_sigs, header_len, round, n_votes, false},
                     cb, user);
}

int coa_queue_submit_digest(coa_queue* q, const uint8_t* data, size_t len, coa_verdict_cb cb, void* user) {
  if (!q || (len && !data) || !cb) return COA_EINVAL;
  Intake in(q, K_DIGEST);
  if (!in.ok()) return COA_EINVAL;
  Window& w = in.w;
  if (len) w.d_data.insert(w.d_data.end(), data, data + len);
  w.d_offs.push_back(w.d_data.size());
  in.done(K_DIGEST, (uint32_t)w.nd++, 1, 1, cb, user);
  return COA_OK;
}

int coa_queue_submit_header(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                            const uint8_t author[32], const uint8_t sig[64], coa_verdict_cb cb, void* user) {
  return submit_header(q, header_data, header_len, id, author, sig, cb, user);
}

int coa_queue_submit_vote(coa_queue* q, const uint8_t id[32], uint64_t round, const uint8_t origin[32],
                          const uint8_t author[32], const uint8_t sig[64], coa_verdict_cb cb, void* user) {
  return submit_vote(q, id, round, origin, author, sig, cb, user, false);
}

// The verdict requests: the same intake with the item marked (and its payload
// count kept); a count that overruns its header is refused here.
int coa_queue_submit_certificate_verdict(coa_queue* q, const uint8_t* header_data, size_t header_len,
                                         const uint8_t id[32], const uint8_t origin[32], const uint8_t header_sig[64],
                                         uint64_t round, const uint8_t* vote_pks, const uint8_t* vote_sigs,
                                         size_t n_votes, uint32_t payload_count, coa_verdict_cb cb, void* user) {
  return submit_cert(q, {header_data, id, origin, header_sig, vote_pks, vote_sigs, header_len, round, n_votes, true},
                     cb, user, &payload_count);
}

int coa_queue_submit_certificate_verdict_borrowed(coa_queue* q, const uint8_t* header_data, size_t header_len,
                                                  const uint8_t id[32], const uint8_t origin[32],
                                                  const uint8_t header_sig[64], uint64_t round,
                                                  const uint8_t* vote_pks, const uint8_t* vote_sigs, size_t n_votes,
                                                  uint32_t payload_count, coa_verdict_cb cb, void* user) {
  return submit_cert(q, {header_data, id, origin, header_sig, vote_pks, vote_sigs, header_len, round, n_votes, false},
                     cb, user, &payload_count);
}

int coa_queue_submit_header_verdict(coa_queue* q, const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                                    const uint8_t author[32], const uint8_t sig[64], uint32_t payload_count,
                                    coa_verdict_cb cb, void* user) {
  return submit_header(q, header_data, header_len, id, author, sig, cb, user, &payload_count);
}

int coa_queue_submit_vote_verdict(coa_queue* q, const uint8_t id[32], uint64_t round, const uint8_t origin[32],
                                  const uint8_t author[32], const uint8_t sig[64], coa_verdict_cb cb, void* user) {
  return submit_vote(q, id, round, origin, author, sig, cb, user, true);
}

int coa_queue_verdict_stats(coa_queue* q, uint64_t* certificates, uint64_t* headers, uint64_t* votes,
                            uint64_t* verdict_windows) {
  if (!q) return COA_EINVAL;
  Lane& L = q->lanes[coa_q::LANE_VERIFY];
  std::lock_guard<std::mutex> l(L.mu);
  if (certificates) *certificates = L.m.v_cert;
  if (headers) *headers = L.m.v_hdr;
  if (votes) *votes = L.m.v_vote;
  if (verdict_windows) *verdict_windows = L.m.v_windows;
  return COA_OK;
}

int coa_queue_message_stats(coa_queue* q, uint64_t* headers, uint64_t* votes, uint64_t* latency_windows,
                            uint64_t* throughput_windows) {
  if (!q) return COA_EINVAL;
  Lane& L = q->lanes[coa_q::LANE_VERIFY];
  std::lock_guard<std::mutex> l(L.mu);
  if (headers) *headers = L.m.hdr;
  if (votes) *votes = L.m.vote;
  if (latency_windows) *latency_windows = L.m.msg_lat;
  if (throughput_windows) *throughput_windows = L.m.msg_tp;
  return COA_OK;
}

int coa_queue_flush(coa_queue* q) {
  if (!q) return COA_EINVAL;
  for (Lane& L : q->lanes) L.flush_all();
  return COA_OK;
}

int coa_queue_set_idle_launch(coa_queue* q, uint32_t windows_in_flight) {
  if (!q || windows_in_flight > 64) return COA_EINVAL;
  for (Lane& L : q->lanes) {
    std::lock_guard<std::mutex> l(L.mu);
    L.idle_launch = windows_in_flight;
    L.cv.notify_one();  // an open window may close now
  }
  return COA_OK;
}

int coa_queue_stats(coa_queue* q, uint64_t* launches, uint64_t* items, uint64_t* groups) {
  if (!q) return COA_EINVAL;
  uint64_t w = 0, it = 0, g = 0;
  for (Lane& L : q->lanes) {
    std::lock_guard<std::mutex> l(L.mu);
    w += L.m.windows;
    it += L.m.sig;
    g += L.m.batch + L.m.cert;
  }
  if (launches) *launches = w;
  if (items) *items = it;
  if (groups) *groups = g;
  return COA_OK;
}

int coa_queue_digest_count(coa_queue* q, uint64_t* digests) {
  if (!q || !digests) return COA_EINVAL;
  Lane& L = q->lanes[coa_q::LANE_DIGEST];
  std::lock_guard<std::mutex> l(L.mu);
  *digests = L.m.dig;
  return COA_OK;
}

int coa_queue_metrics(coa_queue* q, coa_queue_metrics_t* out) {
  if (!q || !out) return COA_EINVAL;
  std::memset(out, 0, sizeof(*out));
  WaitTally waits;  // over all lanes
  for (int k = 0; k < coa_q::LANES; k++) {
    Lane& L = q->lanes[k];
    std::lock_guard<std::mutex> l(L.mu);
    L.m.add_to(*out, waits);
    out->max_pending = std::max<uint64_t>(out->max_pending, (uint64_t)std::max<int64_t>(0, L.m_max_pending.load()));
    out->staging_grows += L.be->grows();
    out->stream_kind = std::max(out->stream_kind, (int32_t)L.be->stream_kind());
    (k == coa_q::LANE_DIGEST ? out->slots_digest : out->slots_verify) = (uint32_t)L.be->slots();
  }
  out->wait_us_mean = out->requests ? waits.sum / (double)out->requests : 0.0;
  out->wait_us_max = waits.max;
  out->wait_us_p50 = coa_q::hist_percentile(waits.hist, 0.50);
  out->wait_us_p99 = coa_q::hist_percentile(waits.hist, 0.99);
  return COA_OK;
}

int coa_queue_metrics_reset(coa_queue* q) {
  if (!q) return COA_EINVAL;
  for (Lane& L : q->lanes) L.reset_metrics();
  return COA_OK;
}

int coa_queue_destroy(coa_queue* q) {
  if (!q) return COA_EINVAL;
  coa_queue_flush(q);
  for (Lane& L : q->lanes) L.shutdown();
  delete q;
  return COA_OK;
}

}  // extern "C"

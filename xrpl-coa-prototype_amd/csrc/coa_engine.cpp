// The engine core behind include/coa_verify.h (see coa_engine.h): init and
// shutdown, the device contexts, the key-cache generations and their
// trailing, sharding and recovery, the latency path's result words.
#include "coa_engine.h"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <random>
#include <thread>

#include "coa_halved.h"
#include "coa_kernels.h"

namespace coa_rt __attribute__((visibility("hidden"))) {

// file-local: see coa_engine.h on why other files go through the functions
static thread_local std::string g_err;
static thread_local bool t_in_worker = false;
static thread_local const KeySetP* t_keys_pinned = nullptr;

std::string& last_error() { return g_err; }
bool in_worker() { return t_in_worker; }

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

KeyScope::KeyScope(const KeySetP& ks) : prev(t_keys_pinned) {
  if (!(prev && *prev)) t_keys_pinned = &ks;
}
KeyScope::~KeyScope() { t_keys_pinned = prev; }

// Bytes of HBM the committee's wide key combs may take (COA_KEY_WCOMB_MB,
// default 16 GiB: committees up to 341 keys; 0 disables them).
double key_wcomb_budget() { return env_mb("COA_KEY_WCOMB_MB", 16384.0); }
// Bytes of HBM the radix-2^20 key combs (654 MB per key) of one key-cache
// generation may take on one device (COA_KEY_WCOMB20_MB, default 128 GiB of
// the MI355X's 288 GB: committees up to ~210 keys; 0 disables them).  The
// generation is shared by the device's contexts; while a registration
// builds the next one both are resident for a moment (the new one falls
// back to the radix-2^16 combs, or to none, when that does not fit).
double key_wcomb20_budget() { return env_mb("COA_KEY_WCOMB20_MB", 131072.0); }
// Bytes of HBM the wide key combs of ALL key-cache generations resident on
// one device at once may take (COA_KEY_RESIDENT_MB, default 224 GiB of the
// MI355X's 288 GB, beside B's 11.8 GB comb and the contexts' workspaces): the
// current generation, the one a registration builds beside it, and the
// spare kept for the next registration.  A new generation takes wide combs
// only when they fit beside the current one; a spare is kept only when it
// fits beside the current generation (the per-generation budget
// alone let two 65 GB generations plus a spare approach the HBM size).
double key_resident_budget() { return env_mb("COA_KEY_RESIDENT_MB", 229376.0); }

// The contexts and the per-device shared state live until coa_shutdown.  A
// process that exits without it never runs their destructors (the vectors
// are not destroyed at exit): those call into the HIP runtime, which may be
// gone by then, and the process's device memory goes with it anyway.
std::mutex g_init_mu;
std::vector<std::unique_ptr<Dev>>& g_devs = *new std::vector<std::unique_ptr<Dev>>();
bool g_inited = false;

// Engine-failure recovery counters (coa_engine_recoveries).
std::atomic<uint64_t> g_ctx_rebuilt{0}, g_shards_rerun{0};

// one per opened HIP device id
std::vector<std::unique_ptr<DevShared>>& g_shared = *new std::vector<std::unique_ptr<DevShared>>();

DevShared* shared_of(int id) {
  for (auto& p : g_shared)
    if (p->id == id) return p.get();
  return nullptr;
}

KeySetP keys_now(const Dev& d) {
  if (t_keys_pinned && *t_keys_pinned && (*t_keys_pinned)->dev == d.id) return *t_keys_pinned;
  std::lock_guard<std::mutex> l(d.sh->mu);
  return d.sh->keys;
}

// Drops the trailing generations whose kernels have completed (an event in
// error counts as complete: nothing more will read through it).
void reap_trailing(DevShared& sh) {
  std::lock_guard<std::mutex> l(sh.trail_mu);
  for (size_t i = 0; i < sh.trailing.size();) {
    if (hipEventQuery(sh.trailing[i].first) != hipErrorNotReady) {
      sh.trail_events.push_back(sh.trailing[i].first);
      sh.trailing[i] = std::move(sh.trailing.back());
      sh.trailing.pop_back();
    } else {
      i++;
    }
  }
  (void)hipGetLastError();
}

// A device-pointer call that read generation `ks` in kernels it enqueued on
// `s` and returns before they complete: `ks` stays held until they have (an
// event on `s`).  Windows of the aggregation queue pin their generation until
// complete() and need none: a call that read the pinned generation itself
// returns at once.  A pin for another device does not cover `ks` (keys_now
// then handed out this device's current generation), so that call trails.
// If no event can be recorded, the call waits for its stream instead.
int trail_keys(Dev& d, const KeySetP& ks, hipStream_t s) {
  if (t_keys_pinned && ks == *t_keys_pinned) return COA_OK;
  DevShared& sh = *d.sh;
  reap_trailing(sh);
  hipEvent_t ev = nullptr;
  {
    std::lock_guard<std::mutex> l(sh.trail_mu);
    if (!sh.trail_events.empty()) {
      ev = sh.trail_events.back();
      sh.trail_events.pop_back();
    }
  }
  if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) ev = nullptr;
  if (!ev || hipEventRecord(ev, s) != hipSuccess) {
    if (ev) (void)hipEventDestroy(ev);
    (void)hipGetLastError();
    HIP_TRY(hipStreamSynchronize(s));
    return COA_OK;
  }
  std::lock_guard<std::mutex> l(sh.trail_mu);
  sh.trailing.emplace_back(ev, ks);
  return COA_OK;
}

// Context d's streams, each once its work has drained (d's device current after).
void drop_streams(Dev& d) {
  (void)hipSetDevice(d.id);
  for (hipStream_t* st : {&d.stream, &d.cstreams[0], &d.cstreams[1], &d.cstreams[2]})
    if (*st) {
      (void)hipStreamSynchronize(*st);
      (void)hipStreamDestroy(*st);
      *st = nullptr;
    }
}

// A context goes once no call uses it (coa_shutdown holds its lock first; a
// failed open never handed it out): its worker, its streams once drained,
// then what it allocated by hand.  The buffers free themselves after this,
// with the device still current.
Dev::~Dev() {
  worker.reset();
  drop_streams(*this);
  if (lat_res) (void)hipHostFree(lat_res);
  if (lat_ctr) (void)hipFree(lat_ctr);
  if (btab) (void)hipFree(btab);
  if (comb) (void)hipFree(comb);
}

DevShared::~DevShared() {
  (void)hipSetDevice(id);
  for (auto& e : trailing) {
    (void)hipEventSynchronize(e.first);
    (void)hipEventDestroy(e.first);
  }
  for (hipEvent_t e : trail_events) (void)hipEventDestroy(e);
  if (wcomb) (void)hipFree(wcomb);
  if (build) (void)hipStreamDestroy(build);
  if (kstage) (void)hipHostFree(kstage);
}

// A failure leaves nothing behind: `dev` frees what it had got so far, and
// init_locked drops the contexts and shared tables opened before it.
int open_device(int d) {
  auto dev = std::make_unique<Dev>();
  dev->id = d;
  HIP_TRY(hipSetDevice(d));
  HIP_TRY(hipStreamCreateWithFlags(&dev->stream, hipStreamNonBlocking));
  HIP_TRY(hipMalloc(&dev->btab, COA_BTAB_DWORDS * sizeof(uint32_t)));
  HIP_TRY(coa_launch_build_btable(dev->btab, dev->stream));
  HIP_TRY(hipMalloc(&dev->comb, COA_COMB_DWORDS * sizeof(uint32_t)));
  HIP_TRY(coa_launch_build_comb(dev->comb, dev->btab, dev->stream));
  DevShared* sh = shared_of(d);
  if (!sh) {  // first context on this device: its shared tables
    g_shared.push_back(std::make_unique<DevShared>());
    sh = g_shared.back().get();
    sh->id = d;
    auto empty = std::make_shared<KeySet>();
    empty->dev = d;
    sh->keys = std::move(empty);
    // the wide comb only speeds things up: without the memory for it the
    // radix-256 comb serves every call
    if (!env_is("COA_WCOMB", "0")) {
      if (hipMalloc(&sh->wcomb, COA_WCOMB_DWORDS * sizeof(uint32_t)) == hipSuccess) {
        HIP_TRY(coa_launch_build_wcomb(sh->wcomb, dev->comb, dev->stream));
      } else {
        sh->wcomb = nullptr;
        (void)hipGetLastError();
      }
    }
  }
  dev->sh = sh;
  HIP_TRY(hipStreamSynchronize(dev->stream));
  dev->worker = std::make_unique<Worker>([] { t_in_worker = true; });
  g_devs.push_back(std::move(dev));
  return COA_OK;
}

// Opens the listed devices (ids == nullptr: the first n, n <= 0: all).
int init_locked(const int* ids, int n) {
  if (g_inited) return COA_OK;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(COA_ENODEVICE, "no HIP device available (this engine has no CPU fallback)");
  std::vector<int> want;
  if (ids) {
    // a device listed k times gets k contexts (k index-range shards on one
    // GPU: rehearses an N-GPU split, e.g. tests/test_gpu_c5.py)
    for (int i = 0; i < n; i++) {
      if (ids[i] < 0 || ids[i] >= count) return fail(COA_EINVAL, "device id out of range");
      want.push_back(ids[i]);
    }
    if (want.empty()) return fail(COA_EINVAL, "empty device list");
  } else {
    if (n <= 0 || n > count) n = count;
    for (int d = 0; d < n; d++) want.push_back(d);
  }
  for (int d : want) {
    const int rc = open_device(d);
    if (rc != COA_OK) {
      g_devs.clear();
      g_shared.clear();
      return rc;
    }
  }
  g_inited = true;
  return COA_OK;
}
int init_locked(int n_gpus) { return init_locked(nullptr, n_gpus); }

int ensure_init() {
  std::lock_guard<std::mutex> g(g_init_mu);
  return init_locked(0);
}

Dev* dev_by_id(int device) {
  for (auto& d : g_devs)
    if (d->id == device) return d.get();
  return nullptr;
}

int enter_device(int device, void* stream, Dev*& d, hipStream_t& s) {
  d = dev_by_id(device);
  if (!d) return fail(COA_EINVAL, "device not opened by coa_init");
  HIP_TRY(hipSetDevice(device));
  s = stream ? (hipStream_t)stream : d->stream;
  return COA_OK;
}

uint32_t verify_lanes(size_t n) {
  const size_t lanes = align_up(std::max<size_t>(n, 1), COA_VERIFY_BLOCK);
  return (uint32_t)std::min<size_t>(lanes, COA_VERIFY_MAX_LANES);
}

struct Range {
  Dev* dev;
  size_t lo, hi;
};

// Items per shard below which a call uses fewer contexts (COA_MIN_SHARD,
// default 65,536 = one lane per item, one wave per SIMD on an MI355X: a
// smaller shard leaves SIMDs idle in the one-wave main kernel, and a call
// spread over every context cannot overlap with another caller's).
size_t min_shard() {
  return (size_t)env_u64("COA_MIN_SHARD", 65536);  // read per call
}
std::atomic<uint32_t> g_shard_rr{0};

// Contiguous index ranges [g*n/G', (g+1)*n/G') over G' of the opened
// contexts: all of them when every shard keeps min_shard() items (a C5 set
// over the 8 GPUs of a node), else n / min_shard() of them (at least one),
// idle ones first, starting one further each call -- so host threads calling
// at once land on different contexts and their calls run side by side.
// `work`: the call's size in the min_shard() unit (signatures; a
// certificate counts its votes too).
std::vector<Range> shard(size_t n, size_t work) {
  std::vector<Range> r;
  const size_t G = g_devs.size();
  const size_t ms = min_shard();
  const size_t want = ms ? std::max<size_t>(1, std::min(G, work / ms)) : G;
  std::vector<Dev*> pick;
  if (want == G) {
    for (auto& d : g_devs) pick.push_back(d.get());
  } else {
    const size_t start = g_shard_rr.fetch_add(1, std::memory_order_relaxed) % G;
    std::vector<bool> taken(G, false);
    for (size_t k = 0; k < G && pick.size() < want; k++) {
      const size_t i = (start + k) % G;
      if (g_devs[i]->mu.try_lock()) {  // idle now
        g_devs[i]->mu.unlock();
        pick.push_back(g_devs[i].get());
        taken[i] = true;
      }
    }
    for (size_t k = 0; k < G && pick.size() < want; k++)
      if (!taken[(start + k) % G]) pick.push_back(g_devs[(start + k) % G].get());
  }
  const size_t P = pick.size();
  for (size_t g = 0; g < P; g++) {
    const size_t lo = n * g / P, hi = n * (g + 1) / P;
    if (hi > lo) r.push_back({pick[g], lo, hi});
  }
  return r;
}

// Calls of at most lat_max() signatures with 32-byte messages take the
// single-signature latency kernel (coa_latency.hip, one workgroup per
// signature: faster than the split kernels up to ~2k signatures,
// tools/lat_probe.py); COA_LAT_MAX overrides (0 = never).
size_t lat_max() {
  return (size_t)env_u64("COA_LAT_MAX", 2048);  // read per call
}

// n <= lat_max() triples with 32-byte messages through k_verify_lat on device
// d (its lock held, device set).  Up to COA_LAT_INLINE signatures travel in
// the kernel arguments (no H2D copy); the kernel writes tagged verdict words
// into page-locked host memory and this thread polls for the tag (no D2H copy,
// no stream synchronisation on the latency path).
// Page-locked result words for n items and the call's tag (device d, its
// lock held).
int lat_res_prepare(Dev& d, size_t n, uint32_t& tag) {
  if (n > d.lat_res_cap) {
    if (d.lat_res) (void)hipHostFree(d.lat_res);
    d.lat_res = nullptr;
    d.lat_res_cap = 0;
    const size_t cap = std::max<size_t>(n, 64);
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&d.lat_res), cap * 4, hipHostMallocCoherent));
    d.lat_res_cap = cap;
  }
  // the words this call waits for start at 0, which no tag matches: a word
  // left over from an earlier call can never pass for this call's result,
  // however the 24-bit tag wraps
  std::memset(d.lat_res, 0, n * 4);
  d.lat_tag = (d.lat_tag + 1) & 0xffffffu;
  if (d.lat_tag == 0) d.lat_tag = 1;
  tag = d.lat_tag;
  return COA_OK;
}

// The context a latency call runs on: the first idle one (its lock free),
// starting one further on each call; when every context is busy, the next
// one in turn (the call then waits for its lock).  Concurrent one-message
// calls (Core and the two Processors) thus spread over every opened context
// instead of queueing on the first.
std::atomic<uint32_t> g_lat_rr{0};
Dev& lat_dev(std::unique_lock<std::mutex>& lk) {
  const size_t n = g_devs.size();
  const size_t start = g_lat_rr.fetch_add(1, std::memory_order_relaxed) % n;
  for (size_t k = 0; k < n; k++) {
    Dev& d = *g_devs[(start + k) % n];
    std::unique_lock<std::mutex> l(d.mu, std::try_to_lock);
    if (l.owns_lock()) {
      lk = std::move(l);
      return d;
    }
  }
  Dev& d = *g_devs[start];
  lk = std::unique_lock<std::mutex>(d.mu);
  return d;
}

// Waits until the n result words carry `tag` (written by the kernel just
// launched on s); the low byte of each goes to out[i] (out may be null).  A
// kernel that ends without publishing (a fault) ends the wait through the
// stream's status; a bound stops a hang.
int lat_res_wait(Dev& d, hipStream_t s, size_t n, uint32_t tag, uint32_t* out) {
  const auto t0 = std::chrono::steady_clock::now();
  for (size_t i = 0; i < n; i++) {
    const volatile uint32_t* w = d.lat_res + i;
    for (uint64_t spin = 0; (*w >> 8) != tag; spin++) {
      if ((spin & 1023) == 1023) {
        const hipError_t q = hipStreamQuery(s);
        if (q != hipSuccess && q != hipErrorNotReady)
          return fail(COA_EHIP, std::string("latency kernel: ") + hipGetErrorString(q));
        if (q == hipSuccess && (*w >> 8) != tag)
          return fail(COA_EHIP, "latency kernel finished without publishing a result");
        if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10))
          return fail(COA_EHIP, "latency kernel timed out");
      }
    }
    if (out) out[i] = *w & 0xffu;
  }
  return COA_OK;
}

// msg_of: item i's message is msgs + msg_of[i] * 32 (null: item i's own).
// batch_n: items [0, batch_n) take the verify_batch prefilter (LatArgs::batch_n).
// cd_in / n_cd: Certificate::digest inputs (72 bytes each, LatArgs::cd_in);
// a prefilter item's message is then its certificate's index (first dword).
int lat_verify(Dev& d, const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, size_t n, uint8_t* out,
               const uint32_t* msg_of, size_t batch_n, const uint8_t* cd_in, size_t n_cd) {
  uint32_t tag = 0;
  int rc = lat_res_prepare(d, n, tag);
  if (rc != COA_OK) return rc;
  LatArgs a;
  std::memset(&a, 0, sizeof(a));
  hipStream_t s = d.stream;
  a.n = (uint32_t)n;
  a.batch_n = (uint32_t)batch_n;
  a.n_inline = (uint32_t)std::min<size_t>(n, COA_LAT_INLINE);
  auto msg = [&](size_t i) { return msgs + (msg_of ? (size_t)msg_of[i] : i) * 32; };
  for (size_t i = 0; i < a.n_inline; i++) {
    std::memcpy(&a.inl[i][0], msg(i), 32);
    std::memcpy(&a.inl[i][8], pks + i * 32, 32);
    std::memcpy(&a.inl[i][16], sigs + i * 64, 64);
  }
  // the records past the inline ones, then the certificate digest inputs,
  // through one pinned staging buffer and one H2D
  const size_t rec_end = n > COA_LAT_INLINE ? n * 128 : 0;
  const size_t cd_off = align_up(std::max<size_t>(rec_end, COA_LAT_INLINE * 128), 256);
  const size_t in_bytes = n_cd ? cd_off + n_cd * 72 : rec_end;
  if (in_bytes) {
    HIP_TRY(d.pin.ensure(in_bytes));
    HIP_TRY(d.lat.ensure(in_bytes));
    uint8_t* h = static_cast<uint8_t*>(d.pin.p);
    for (size_t i = COA_LAT_INLINE; i < n; i++) {
      std::memcpy(h + i * 128, msg(i), 32);
      std::memcpy(h + i * 128 + 32, pks + i * 32, 32);
      std::memcpy(h + i * 128 + 64, sigs + i * 64, 64);
    }
    if (n_cd) std::memcpy(h + cd_off, cd_in, n_cd * 72);
    const size_t from = rec_end ? (size_t)COA_LAT_INLINE * 128 : cd_off;
    HIP_TRY(hipMemcpyAsync(d.lat.as<uint8_t>() + from, h + from, in_bytes - from, hipMemcpyHostToDevice, s));
    a.in = d.lat.as<uint32_t>();
    if (n_cd) a.cd_in = reinterpret_cast<const uint32_t*>(d.lat.as<uint8_t>() + cd_off);
  }
  a.tag = tag;
  a.res = d.lat_res;
  const KeySetP ks = keys_now(d);  // held until the verdicts are in
  key_args(a, d, *ks);
  HIP_TRY(coa_launch_verify_lat(a, s));
  std::vector<uint32_t> words(n);
  rc = lat_res_wait(d, s, n, tag, words.data());
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < n; i++) out[i] = (uint8_t)words[i];
  return COA_OK;
}

int check_n(size_t n) {
  if (n > 0xffffffffull / 2) return fail(COA_EINVAL, "n too large for one call");
  return COA_OK;
}

// f on context d's worker thread; the result carries that thread's error text.
std::future<TaskResult> submit_task(Dev& d, std::function<int()> f) {
  return d.worker->submit([f = std::move(f)] {
    g_err.clear();
    const int rc = f();
    return TaskResult(rc, rc == COA_OK ? std::string() : g_err);
  });
}

// Runs tasks that each own one context: concurrently on the contexts' worker
// threads, or inline on this thread when they all use one context (no thread
// hop on the latency path) or when this is already a worker.  Returns the
// first failure (its message in this thread's coa_last_error).
int run_tasks(TaskList& tasks) {
  bool one_ctx = true;
  for (auto& t : tasks) one_ctx = one_ctx && t.first == tasks[0].first;
  if (one_ctx || t_in_worker) {
    for (auto& t : tasks) {
      const int rc = t.second();
      if (rc != COA_OK) return rc;
    }
    return COA_OK;
  }
  std::vector<std::future<TaskResult>> futs;
  futs.reserve(tasks.size());
  for (auto& t : tasks) futs.push_back(submit_task(*t.first, t.second));
  int rc = COA_OK;
  std::string msg;
  for (auto& f : futs) {
    TaskResult r = f.get();  // wait for every task: they reference the caller's buffers
    if (r.first != COA_OK && rc == COA_OK) {
      rc = r.first;
      msg = r.second;
    }
  }
  if (rc != COA_OK) g_err = msg;
  return rc;
}

// COA_FAULT_SHARD=<k>: every k-th shard of a sharded call fails with
// COA_EHIP after its work has run (fault injection for the recovery tests;
// never set in production).  COA_FAULT_SHARD=all: every attempt fails,
// re-runs on the other contexts included, so the call itself fails (the
// caller's failure policy is then what answers: tests/test_gpu_recovery.py).
// Read per call.
bool fault_every_attempt() { return env_is("COA_FAULT_SHARD", "all"); }
bool inject_shard_fault() {
  static std::atomic<unsigned long long> count{0};
  if (fault_every_attempt()) return true;
  const unsigned long long every = env_u64("COA_FAULT_SHARD", 0);
  return every && (count.fetch_add(1) + 1) % every == 0;
}

// Rebuilds a context after a HIP failure (its lock held): drains and
// replaces its stream and releases its per-call buffers (they regrow on
// demand).  The fixed-base and committee tables are kept: they were built
// and checked before and no call writes them.  Same process, no exec.
int rebuild_context(Dev& d) {
  drop_streams(d);
  for (DevBuf* b : d.all()) b->release();  // per-call buffers (the tables live in DevShared)
  (void)hipGetLastError();
  HIP_TRY(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
  g_ctx_rebuilt++;
  return COA_OK;
}

// Run `body` for every shard with its context's lock held, then drain the
// context's stream.  body(Dev&, lo, hi) enqueues work and returns COA_OK or an
// error.  The shards run concurrently, one per context worker.
// Engine-failure recovery: a shard that fails with a device error
// (COA_EHIP / COA_ENOMEM) has its context rebuilt and is re-run on the next
// contexts in turn (the rebuilt one last); the call fails only when every
// context failed it.  body must therefore be re-runnable for its range: it
// writes only its own slice of the caller's outputs.
int for_shards(size_t n, const std::function<int(Dev&, size_t, size_t)>& body, size_t work) {
  TaskList tasks;
  const std::vector<Range> ranges = shard(n, work ? work : n);
  std::vector<int> rcs(ranges.size(), COA_OK);
  std::vector<std::string> msgs(ranges.size());
  auto run_on = [&body](Dev& d, size_t lo, size_t hi, bool inject) -> int {
    std::lock_guard<std::mutex> l(d.mu);
    if (hipSetDevice(d.id) != hipSuccess) return fail(COA_EHIP, "hipSetDevice failed");
    int rc = body(d, lo, hi);
    const hipError_t e = hipStreamSynchronize(d.stream);
    if (e != hipSuccess && rc == COA_OK) rc = fail(COA_EHIP, std::string("stream sync: ") + hipGetErrorString(e));
    if (rc == COA_OK && inject) rc = fail(COA_EHIP, "injected shard fault (COA_FAULT_SHARD)");
    if (rc == COA_EHIP || rc == COA_ENOMEM) (void)rebuild_context(d);
    return rc;
  };
  for (size_t i = 0; i < ranges.size(); i++) {
    const Range r = ranges[i];
    const bool inject = inject_shard_fault();
    tasks.emplace_back(r.dev, [r, inject, i, &rcs, &msgs, &run_on]() -> int {
      rcs[i] = run_on(*r.dev, r.lo, r.hi, inject);
      if (rcs[i] != COA_OK) msgs[i] = g_err;
      // recoverable failures are re-run below, so the other shards finish
      return (rcs[i] == COA_EHIP || rcs[i] == COA_ENOMEM) ? COA_OK : rcs[i];
    });
  }
  int rc = run_tasks(tasks);
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < ranges.size(); i++) {
    if (rcs[i] == COA_OK) continue;
    size_t at = 0;
    for (size_t g = 0; g < g_devs.size(); g++)
      if (g_devs[g].get() == ranges[i].dev) at = g;
    int r = rcs[i];
    const std::string first = msgs[i];
    for (size_t k = 1; k <= g_devs.size() && (r == COA_EHIP || r == COA_ENOMEM); k++) {
      r = run_on(*g_devs[(at + k) % g_devs.size()], ranges[i].lo, ranges[i].hi, fault_every_attempt());
      g_shards_rerun++;
    }
    if (r != COA_OK) return fail(r, "shard failed on every context: " + first + " / " + g_err);
  }
  return COA_OK;
}

uint64_t os_entropy_seed() {
  std::random_device rd;
  uint64_t s = 0;
  while (s == 0) s = ((uint64_t)rd() << 32) ^ rd();
  return s;
}

// Builds the next key-cache generation of device sh on its build stream
// while every call and queue window keeps the current one, swaps it in, then
// frees the old generation once nothing holds it: no call or window waits
// for a registration, and none is held back (the round-3 write gate stalled
// the queue's certificate windows for the whole 0.6-2.7 s build).
int build_keyset(DevShared& sh, const std::vector<std::array<uint32_t, 8>>& keys, const CoaProtTable* pt) {
  std::lock_guard<std::mutex> r(sh.reg_mu);
  HIP_TRY(hipSetDevice(sh.id));
  if (!sh.build) {
    // the build runs beside live windows (a committee-100 build is 65 GB of
    // comb entries, ~0.6 s on the whole GPU): on a plain stream at the least
    // priority, so the hardware queue scheduler dispatches the windows'
    // workgroups first.  tools/regab.sh, a C3 certificate stream at 5,000/s
    // with two re-registrations (profiles/r04_register_ab.txt): request
    // latency p99 during the build 0.89 ms (max 1.3 ms), registration 0.61 s;
    // a CU-masked stream over half the CUs (COA_REGISTER_CUS=128) left the
    // windows 17 ms (bounded resident grid) to 1.4 s (one workgroup per 256
    // entries) behind.
    int cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sh.id));
    const int want = (int)env_int("COA_REGISTER_CUS", 0);
    if (want <= 0) {
      int least = 0, greatest = 0;
      HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
      HIP_TRY(hipStreamCreateWithPriority(&sh.build, hipStreamNonBlocking, least));
    } else {
      const int use = std::min(cus, want);
      std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
      for (int c = cus - use; c < cus; c++) mask[(size_t)c / 32] |= 1u << (c % 32);
      HIP_TRY(hipExtStreamCreateWithCUMask(&sh.build, (uint32_t)mask.size(), mask.data()));
    }
  }
  const size_t nk = keys.size();
  // the buffers of the generation before the current one, when kept
  // (COA_KEY_SPARE=0: none kept, every registration allocates)
  const bool keep_spare = !env_is("COA_KEY_SPARE", "0");
  std::shared_ptr<KeySet> ks = keep_spare && sh.spare ? std::move(sh.spare) : std::make_shared<KeySet>();
  sh.spare.reset();
  // wide-comb bytes the current generation keeps resident while this one is
  // built (charged against COA_KEY_RESIDENT_MB)
  double cur_wide = 0.0;
  {
    std::lock_guard<std::mutex> l(sh.mu);
    if (sh.keys) cur_wide = (double)sh.keys->kwtabs.cap;
  }
  const double resident_room = key_resident_budget() - cur_wide;
  ks->dev = sh.id;
  ks->nkeys = 0;
  ks->kwide = ks->kw20 = false;
  ks->has_prot = false;
  hipStream_t s = sh.build;
  // COA_REGISTER_TRACE=1: phase times of this registration on stderr
  using clk = std::chrono::steady_clock;
  const auto t0 = clk::now();
  auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  clk::time_point t_alloc = t0, t_built = t0;
  if (nk) {
    HIP_TRY(ks->ckeys.ensure(nk * 32));
    HIP_TRY(ks->kflags.ensure(nk * 4));
    HIP_TRY(ks->ktabs.ensure(nk * (size_t)COA_KEY_TAB_DWORDS * 4));
    if (env_is("COA_REGISTER_PAGEABLE", "1")) {  // A/B: the keys straight from the caller's (pageable) vector
      HIP_TRY(hipMemcpyAsync(ks->ckeys.p, keys.data(), nk * 32, hipMemcpyHostToDevice, s));
    } else {
      if (sh.kstage_cap < nk * 32) {
        if (sh.kstage) HIP_TRY(hipHostFree(sh.kstage));
        sh.kstage = nullptr;
        sh.kstage_cap = 0;
        HIP_TRY(hipHostMalloc(&sh.kstage, nk * 32, hipHostMallocDefault));
        sh.kstage_cap = nk * 32;
      }
      std::memcpy(sh.kstage, keys.data(), nk * 32);
      HIP_TRY(hipMemcpyAsync(ks->ckeys.p, sh.kstage, nk * 32, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(coa_launch_key_flags(ks->ckeys.as<uint32_t>(), (uint32_t)nk, ks->kflags.as<uint32_t>(), s));
    HIP_TRY(coa_launch_key_tables(ks->ckeys.as<uint32_t>(), (uint32_t)nk, ks->ktabs.as<uint32_t>(), s));
    // wide combs when the committee fits the budget: radix 2^20 (654 MB per
    // key, 13 additions per [k](-A)) within COA_KEY_WCOMB20_MB, else radix
    // 2^16 (48 MiB per key, 16 additions) within COA_KEY_WCOMB_MB (speed
    // only: without the memory the radix-256 key combs serve)
    KeySet& k = *ks;
    // an exact fit is reused as it is; a different size is reallocated
    auto fit = [](DevBuf& b, size_t bytes) {
      if (b.cap != bytes) b.release();
      return b.ensure(bytes, true);
    };
    const double w20 = (double)nk * COA_KWCOMB20_DWORDS * 4, w16 = (double)nk * COA_KWCOMB_DWORDS * 4;
    if (w20 <= key_wcomb20_budget() && w20 <= resident_room) {
      if (fit(k.kwtabs, nk * (size_t)COA_KWCOMB20_DWORDS * 4) == hipSuccess) {
        t_alloc = clk::now();
        HIP_TRY(coa_launch_key_wcombs20(k.ktabs.as<uint32_t>(), (uint32_t)nk, k.kwtabs.as<uint32_t>(), s));
        k.kwide = k.kw20 = true;
      } else {
        k.kwtabs.release();
        (void)hipGetLastError();
      }
    }
    if (!k.kw20 && w16 <= key_wcomb_budget() && w16 <= resident_room) {
      if (fit(k.kwtabs, nk * (size_t)COA_KWCOMB_DWORDS * 4) == hipSuccess) {
        HIP_TRY(coa_launch_key_wcombs(k.ktabs.as<uint32_t>(), (uint32_t)nk, k.kwtabs.as<uint32_t>(), s));
        k.kwide = true;
      } else {
        k.kwtabs.release();
        (void)hipGetLastError();
      }
    }
    if (!k.kwide) k.kwtabs.release();  // a reused spare's wide combs no budget admits
    HIP_TRY(hipStreamSynchronize(s));
    k.nkeys = (uint32_t)nk;
    t_built = clk::now();
  }
  if (pt) {  // the protocol table of this generation, in the same key order
    std::vector<uint32_t> w(pt->stake);
    w.insert(w.end(), pt->woff.begin(), pt->woff.end());
    w.insert(w.end(), pt->wids.begin(), pt->wids.end());
    HIP_TRY(ks->prot.ensure(w.size() * 4));
    HIP_TRY(hipMemcpyAsync(ks->prot.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    ks->quorum = pt->quorum;
    ks->has_prot = true;
  }
  KeySetP old;
  {
    std::lock_guard<std::mutex> l(sh.mu);
    old = std::move(sh.keys);
    sh.keys = std::move(ks);
  }
  // the old generation: calls and windows that took it still hold it (their
  // kernels read it until they complete), and a device-pointer call on a
  // caller's stream left it in `trailing` with an event after its kernels
  // (trail_keys).  Only this thread waits -- no hipDeviceSynchronize, which
  // held every other thread's launches for its whole wait.
  const auto t_swap = clk::now();
  while (old.use_count() > 1) {
    reap_trailing(sh);
    if (old.use_count() > 1) std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
  const auto t_unpinned = clk::now();
  const auto t_synced = t_unpinned;
  // the replaced generation's buffers become the spare of the next
  // registration; after the first registration of a device (nothing to
  // replace yet) a spare of the same size is allocated now, while the
  // committee is being set up rather than under load later
  if (keep_spare && nk) {
    const KeySet& cur = *sh.keys;
    // the next registration of a committee this size finds its buffers ready
    auto fits = [&](const KeySet& k) {
      return k.ckeys.cap >= nk * 32 && k.kflags.cap >= nk * 4 && k.ktabs.cap >= nk * (size_t)COA_KEY_TAB_DWORDS * 4 &&
             k.kwtabs.cap == cur.kwtabs.cap;
    };
    // a spare only beside the current generation within COA_KEY_RESIDENT_MB
    // (without one, the next registration allocates its wide combs while
    // windows run: 2.4-7.6 ms held back, profiles/r04_register_ab.txt)
    const bool room = 2.0 * (double)cur.kwtabs.cap <= key_resident_budget();
    if (!room) {
      old.reset();
    } else if (old && fits(*old)) {
      sh.spare = std::const_pointer_cast<KeySet>(old);
    } else {
      old.reset();  // another size: freed now, and a spare of this size made
      auto sp = std::make_shared<KeySet>();
      sp->dev = sh.id;
      if (sp->ckeys.ensure(cur.ckeys.cap, true) == hipSuccess && sp->kflags.ensure(cur.kflags.cap, true) == hipSuccess &&
          sp->ktabs.ensure(cur.ktabs.cap, true) == hipSuccess &&
          (!cur.kwtabs.cap || sp->kwtabs.ensure(cur.kwtabs.cap, true) == hipSuccess))
        sh.spare = std::move(sp);
      else
        (void)hipGetLastError();  // no spare: the next registration allocates
    }
  } else if (keep_spare && !nk && old && old->nkeys && !sh.spare) {
    // a committee cleared: its generation's buffers stay as the spare instead
    // of being freed.  Freeing a 65 GB generation here, and allocating one
    // again at the next registration, each held the HIP runtime while other
    // threads enqueued: a signature window of the queue spent 7.9 ms in
    // `enqueue` (profiles/r05_register_gc.txt:19) while
    // test_register_while_queue_saturated_with_certificates cleared and
    // re-registered the committee in a loop
    sh.spare = std::const_pointer_cast<KeySet>(old);
  }
  old.reset();
  if (env_is("COA_REGISTER_TRACE", "1"))
    fprintf(stderr,
            "coa_committee_register dev %d keys %zu at t=%.6f s: alloc %.1f build %.1f swap %.1f unpinned %.1f sync "
            "%.1f free %.1f ms\n",
            sh.id, nk, std::chrono::duration<double>(t0.time_since_epoch()).count(), ms(t0, t_alloc),
            ms(t_alloc, t_built), ms(t_built, t_swap), ms(t_swap, t_unpinned),
            ms(t_unpinned, t_synced), ms(t_synced, clk::now()));
  return COA_OK;
}

int on_each_device(const std::function<int(DevShared&)>& build) {
  TaskList tasks;
  for (auto& shp : g_shared) {
    DevShared* sh = shp.get();
    Dev* first = nullptr;
    for (auto& dp : g_devs)
      if (dp->id == sh->id && !first) first = dp.get();
    if (!first) continue;
    tasks.emplace_back(first, [sh, &build]() -> int { return build(*sh); });
  }
  return run_tasks(tasks);
}

}  // namespace coa_rt

using namespace coa_rt;

extern "C" {

const char* coa_last_error(void) { return g_err.c_str(); }
const char* coa_version(void) { return "coa_verify 0.1.0 gfx950"; }

int coa_init(int n_gpus) {
  std::lock_guard<std::mutex> g(g_init_mu);
  return init_locked(n_gpus);
}

int coa_init_devices(const int* device_ids, int n) {
  if (!device_ids || n <= 0) return fail(COA_EINVAL, "empty device list");
  std::lock_guard<std::mutex> g(g_init_mu);
  return init_locked(device_ids, n);
}

// Lock, drain, clear: a context's lock is free once the call that held it has
// drained its stream; the destructors (coa_engine.h) release the rest.
int coa_shutdown(void) {
  std::lock_guard<std::mutex> g(g_init_mu);
  for (auto& d : g_devs) std::lock_guard<std::mutex> l(d->mu);
  g_devs.clear();
  g_shared.clear();
  g_inited = false;
  return COA_OK;
}

int coa_device_count(void) {
  const int r = ensure_init();
  if (r != COA_OK) return r;
  return (int)g_devs.size();
}

int coa_device_ids(int* ids_out, int cap) {
  const int r = ensure_init();
  if (r != COA_OK) return r;
  if (cap > 0 && !ids_out) return fail(COA_EINVAL, "null argument");
  for (int i = 0; i < (int)g_devs.size() && i < cap; i++) ids_out[i] = g_devs[i]->id;
  return (int)g_devs.size();
}

int coa_self_test(int device, uint64_t* bad_entries) {
  if (!bad_entries) return fail(COA_EINVAL, "null output");
  *bad_entries = 0;
  const int r = ensure_init();
  if (r != COA_OK) return r;
  Dev* d;
  hipStream_t s;
  if (const int rc = enter_device(device, nullptr, d, s)) return rc;
  std::lock_guard<std::mutex> l(d->mu);
  if (!d->sh->wcomb) return COA_OK;
  uint32_t* dbad = nullptr;
  HIP_TRY(hipMalloc(&dbad, sizeof(uint32_t)));
  uint32_t hbad = 0;
  hipError_t e = hipMemsetAsync(dbad, 0, sizeof(uint32_t), s);
  if (e == hipSuccess) e = coa_launch_check_wcomb(d->sh->wcomb, dbad, s);
  if (e == hipSuccess) e = hipMemcpyAsync(&hbad, dbad, sizeof(uint32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(dbad);
  HIP_TRY(e);
  *bad_entries = hbad;
  return COA_OK;
}

int coa_fe_rows_check_device(int device, const uint8_t* d_in, size_t n, uint32_t* d_out, void* stream) {
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n && (!d_in || !d_out)) return fail(COA_EINVAL, "null argument");
  if (n > (1u << 24)) return fail(COA_EINVAL, "n too large");
  Dev* d;
  hipStream_t s;
  if (const int r = enter_device(device, stream, d, s)) return r;
  HIP_TRY(coa_launch_fe_rows_check(d_in, (uint32_t)n, d_out, s));
  if (!stream) HIP_TRY(hipStreamSynchronize(s));
  return COA_OK;
}

void* coa_keycache_pin(int device) {
  DevShared* sh = shared_of(device);
  if (!sh) return nullptr;
  std::lock_guard<std::mutex> l(sh->mu);
  return new KeySetP(sh->keys);
}

void coa_keycache_unpin(void* pin) { delete static_cast<KeySetP*>(pin); }

void coa_keycache_use(void* pin) { t_keys_pinned = static_cast<const KeySetP*>(pin); }

void coa_copy_segments(const Seg* segs, size_t n) { CopyPool::get().copy(segs, n); }

size_t coa_lat_max(void) { return lat_max(); }

int coa_engine_recoveries(uint64_t* contexts_rebuilt, uint64_t* shards_rerun) {
  if (contexts_rebuilt) *contexts_rebuilt = g_ctx_rebuilt.load();
  if (shards_rerun) *shards_rerun = g_shards_rerun.load();
  return COA_OK;
}

}  // extern "C"

// HIP launch backend of the aggregation queue (coa_queue.h), one per lane:
// device slots (four per opened GPU and lane by default:
// COA_QUEUE_SLOTS for the verify lane, COA_QUEUE_DIGEST_SLOTS for the digest
// lane), each with its own stream, event, page-locked staging and device
// buffers.
//
// Hardware queues.  HIP gives a process GPU_MAX_HW_QUEUES hardware queues
// per priority (4 by default, and a node cannot rely on exporting more
// before its first HIP call) and maps every stream onto them; streams that
// share a hardware queue run one after another.  With the engine's context
// streams, a host's own streams and eight slots on four queues, a 14 ms
// digest window would sit in front of a certificate window (round 3:
// queue_round_mix p99 7.2-7.7 ms and c4_stream 4,000/s p50 94 ms on a box
// with the default 4).  So a slot's stream is made to get a hardware queue
// of its own (COA_QUEUE_STREAMS, tools/hwq_probe.hip measures which kind
// does): "cumask" (the default) -- hipExtStreamCreateWithCUMask with every
// CU enabled: HIP never shares a CU-masked stream's queue, whatever
// GPU_MAX_HW_QUEUES says; "priority" -- the high-priority pool (its own 4
// queues) for the verify lane; "plain" -- shared queues (the round-3 form).
//
// What a window's blocks hold is coa_qstage.h's (host code only, tested on
// the CPU): the layout of the input and output blocks, the packer, the
// scatter and the resolver's gather / write-back.  This file holds the HIP
// around it.  enqueue() lays the launch out, packs its parts (one per intake
// shard) straight into the slot's pinned input block -- the parts are never
// merged first -- and picks a route (coa_q::Route), each a member function:
// staged -- ONE host-to-device copy, the engine's device-resident entry points
// (asynchronous with an explicit workspace, no engine lock) and ONE
// device-to-host copy on the slot's stream, then an event that complete()
// waits for -- or, for a small window of one kind, one of the publish routes.
// complete() then scatters the outputs back to the parts.  So while window N
// runs on slot A, window N + 1 is packed and enqueued on slot B, and the
// copies of one window overlap the kernels of the other.
//
// Per kind:
//   signatures    coa_ed25519_verify_strict_many_device (Signature::verify);
//                 windows of at most COA_LAT_MAX (2,048) signatures take the
//                 latency kernel instead (one workgroup per signature)
//   certificates  coa_certificate_verify_many_device (the fused
//                 Certificate::verify crypto); the certificates whose raw
//                 status words need the exact random-linear-combination check
//                 or carry a key outside the registered committee are left
//                 open by complete() (Window::c_defer) and decided by
//                 resolve() on the lane's resolver thread with
//                 coa_certificate_resolve_raw -- the exact path alone, not a
//                 second fused launch -- while the rest of the window is
//                 answered at once.  A window with certificates pins its
//                 device's key-cache generation from launch to completion
//   headers, votes  the committee-comb message kernels, Header::digest checked
//                 and Vote::digest hashed on the device: alone in a window of
//                 at most 64 messages, the latency kernel in publish mode
//                 (ROUTE_MSG_PUBLISH); a window of at most COA_QUEUE_MSG_LAT_MAX
//                 messages, the latency kernel with its status words staged
//                 (coa_msg_lat_verify_device); a larger one,
//                 coa_header_verify_many_device / coa_vote_verify_many_device.
//                 Messages by authors outside the registered committee
//                 (COA_CST_UNCACHED) are left open (Window::m_defer) and
//                 decided by resolve() with coa_message_resolve_raw
//   verdicts      a window that holds a verdict request (coa_queue_submit_*_verdict)
//                 takes the staged route; after the crypto entries of its
//                 certificates, headers and votes, ONE k_window_verdict launch
//                 (coa_window_verdict_device) decides the protocol checks of
//                 all of them over the same staged arrays -- plus the two
//                 payload-count sections -- and merges them with the raw status
//                 words into the verdict-word section of the output block,
//                 which the one D2H copy carries.  The scatter gives every
//                 verdict request its word; only a certificate left
//                 COA_DAG_VOTES_OPEN goes to resolve().  A pinned generation
//                 without protocol table: Launch::verdict_rc = COA_EINVAL,
//                 nothing launched for the verdicts, the rest as usual.
//                 Except a window whose messages are all verdict requests,
//                 at most COA_QUEUE_MSG_LAT_MAX of them, with no certificate
//                 verdict (Launch::msg_words): k_msg_verdict_lat decides the
//                 protocol code in each signature job and writes the merged
//                 words where the crypto messages' status words go -- on
//                 ROUTE_MSG_PUBLISH when alone and at most 64
//                 (coa_msg_lat_verdict_publish), else staged
//                 (coa_msg_lat_verdict_device) -- with no further launch
//   digests       coa_sha512_many_device (worker/src/processor.rs:38)
//   vote batches  coa_ed25519_verify_batch_groups in resolve() (host
//                 pointers; bare batches are rare next to whole certificates)
//
// Engine-failure recovery: a failed launch drains its stream (the error code
// kept), its slot is rebuilt (new stream and event, device buffers freed and
// regrown on demand) and freed; the queue then re-runs the window through
// retry() on the recovery context of another device (one per device, used
// only by retries).  COA_QUEUE_FAULT=<k> makes every k-th window's launch
// fail once its input copy is enqueued -- before anything is, on the routes
// without a copy of their own (fault injection for the recovery tests; never
// set in production).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "coa_committee.h"
#include "coa_env.h"
#include "coa_latency.h"
#include "coa_protocol_dev.h"
#include "coa_qstage.h"
#include "coa_queue.h"

#define COA_QUEUE_SLOTS_DEFAULT 4
// The digest lane's windows are one ~14 ms SHA-512 chain each on a few
// waves (L = 64 lanes per batch), so more of them in flight cost the GPU
// nothing and shorten the wait for a slot: at C4's 1,000 batches/s, 8 slots
// give p50 16.0 ms against 19.6 with 4 (profiles/r05_digest_slots_ab.jsonl)
#define COA_QUEUE_DIGEST_SLOTS_DEFAULT 8
// Largest message window (headers + votes) the latency kernel takes
// (COA_QUEUE_MSG_LAT_MAX, read at queue creation): the largest window size of
// tools/queue_message_ab.py's device-side sweep at which k_msg_verify_lat was
// not slower than k_msg_verify, for headers and for votes
// (profiles/queue_message_ab.json)
#define COA_QUEUE_MSG_LAT_MAX_DEFAULT 512

using namespace coa_rt;  // the switch readers of coa_env.h

namespace {

inline int64_t ns_between(std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count();
}

struct Grave {  // an outgrown staging buffer (see grow_pinned)
  void* p;
  bool pinned;
};

struct Slot {
  int dev = -1;
  int kind = COA_QUEUE_STREAM_PLAIN;  // how its stream is made
  int lane = 0;
  hipStream_t s = nullptr;
  hipEvent_t ev = nullptr;
  void* hin = nullptr;   // pinned input block
  void* hout = nullptr;  // pinned output block
  void* din = nullptr;   // device input block
  void* dout = nullptr;  // device output block
  void* ws = nullptr;    // device workspace (verify + certificates)
  size_t cap_hin = 0, cap_hout = 0, cap_din = 0, cap_dout = 0, cap_ws = 0;
  std::vector<Grave> grave;  // outgrown staging, freed with the slot
  bool busy = false;
  bool launched = false;  // device work was enqueued (complete() must drain it)
  void* keys = nullptr;   // the key-cache generation the launch pinned (coa_keycache_pin)
  bool lat = false;       // the launch's signatures took the latency kernel (result words)
  coa_q::WindowPack pack;  // the launch's staging layout
  // How the launch's results come back (coa_qstage.h).  On a publish route the
  // kernel writes npub result words tagged ltag straight into lres (page-locked,
  // coherent), which complete() polls -- no D2H copy, no event wait.
  coa_q::Route route = coa_q::ROUTE_STAGED;
  uint32_t* lres = nullptr;  // COA_PUBLISH_WORDS words
  uint32_t ltag = 0;
  size_t npub = 0;           // result words the launch publishes (new_tag)
  uint32_t* dctr = nullptr;  // the publishing kernels' 65 device counter words, zero between launches
};

// A slot's staging grows geometrically (twice what a window needs) and an
// outgrown buffer is not freed on the launch path: hipFree / hipHostFree wait
// for the whole device, i.e. for every other slot's window in flight (round
// 4: a 3-batch digest window took 136 ms behind its lane's regrowths at
// 4,000 batches/s).  Outgrown buffers go to the slot's graveyard, freed with
// the slot; the geometric growth bounds them to the final size.
hipError_t grow_pinned(void*& p, size_t& cap, size_t want, std::vector<Grave>& grave) {
  if (want <= cap) return hipSuccess;
  if (p) grave.push_back({p, true});
  p = nullptr;
  cap = 0;
  want = 2 * want + 4096;
  hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
  if (e == hipSuccess) cap = want;
  return e;
}
hipError_t grow_dev(void*& p, size_t& cap, size_t want, std::vector<Grave>& grave) {
  if (want <= cap) return hipSuccess;
  if (p) grave.push_back({p, false});
  p = nullptr;
  cap = 0;
  want = 2 * want + 4096;
  hipError_t e = hipMalloc(&p, want);
  if (e == hipSuccess) cap = want;
  return e;
}
void bury(std::vector<Grave>& grave) {
  for (const Grave& g : grave) (void)(g.pinned ? hipHostFree(g.p) : hipFree(g.p));
  grave.clear();
}

// Process-wide pool of the slots' streams.  Every queue used to create its
// slots' streams and destroy them with the queue: a CU-masked stream is a
// hardware queue of its own, so a process that makes many queues (bench.py
// makes ~40) created and tore down ~500 hardware queues.  Under
// `rocprofv3 --kernel-trace` that ended in a SIGSEGV at address 0x34 inside
// hipExtStreamCreateWithCUMask (round 5, gpurun_out/fullprof.err: stack
// make_stream <- HipBackend::ready <- coa_queue_create <-
// latc_stream_certificates, late in the run; the same section alone
// profiled clean).  A healthy slot's stream now returns here when its queue
// is destroyed and the next queue takes it, so a process holds at most the
// streams of the queues alive at once, and a later queue also skips the
// first-dispatch cost of a new hardware queue (~25-75 ms for a CU-masked
// one).  A stream whose window failed is destroyed, never pooled.
struct PooledStream {
  int dev, kind, prio;
  hipStream_t s;
};
std::mutex g_pool_mu;
std::vector<PooledStream>& stream_pool() {
  static auto* pool = new std::vector<PooledStream>();  // never destroyed: streams outlive static teardown
  return *pool;
}
int slot_prio(const Slot& sl) { return sl.kind == COA_QUEUE_STREAM_PRIORITY && sl.lane == coa_q::LANE_VERIFY; }
hipStream_t pool_take(const Slot& sl) {
  std::lock_guard<std::mutex> l(g_pool_mu);
  auto& pool = stream_pool();
  for (size_t i = 0; i < pool.size(); i++)
    if (pool[i].dev == sl.dev && pool[i].kind == sl.kind && pool[i].prio == slot_prio(sl)) {
      const hipStream_t s = pool[i].s;
      pool[i] = pool.back();
      pool.pop_back();
      return s;
    }
  return nullptr;
}
// Hands a slot's stream to the pool (drained first); a stream that does not
// drain cleanly is destroyed instead.
void pool_give(Slot& sl) {
  if (!sl.s) return;
  if (hipStreamSynchronize(sl.s) == hipSuccess && hipStreamQuery(sl.s) == hipSuccess) {
    std::lock_guard<std::mutex> l(g_pool_mu);
    stream_pool().push_back({sl.dev, sl.kind, slot_prio(sl), sl.s});
  } else {
    (void)hipStreamDestroy(sl.s);
    (void)hipGetLastError();
  }
  sl.s = nullptr;
}

// New stream and event for a slot; its device buffers are freed (regrown by
// the next launch).  The pinned host blocks are kept.  A slot without a
// stream takes one from the pool when one of its kind is there; a slot being
// rebuilt after a failed window gets a fresh one.
int make_stream(Slot& sl) {
  if (hipSetDevice(sl.dev) != hipSuccess) return COA_EHIP;
  const bool rebuild = sl.s != nullptr;
  if (sl.s) {
    (void)hipStreamSynchronize(sl.s);
    (void)hipStreamDestroy(sl.s);
    sl.s = nullptr;
  }
  if (sl.ev) {
    (void)hipEventDestroy(sl.ev);
    sl.ev = nullptr;
  }
  for (void** p : {&sl.din, &sl.dout, &sl.ws, reinterpret_cast<void**>(&sl.dctr)})
    if (*p) {
      (void)hipFree(*p);
      *p = nullptr;
    }
  sl.cap_din = sl.cap_dout = sl.cap_ws = 0;
  bury(sl.grave);
  (void)hipGetLastError();  // a failed launch's error is not sticky for the new stream
  hipError_t e = hipSuccess;
  if (!rebuild) sl.s = pool_take(sl);
  if (sl.s) {
    // pooled
  } else if (sl.kind == COA_QUEUE_STREAM_CUMASK) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sl.dev) != hipSuccess || cus <= 0)
      return COA_EHIP;
    std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
    for (int c = 0; c < cus; c++) mask[(size_t)c / 32] |= 1u << (c % 32);
    e = hipExtStreamCreateWithCUMask(&sl.s, (uint32_t)mask.size(), mask.data());
  } else if (sl.kind == COA_QUEUE_STREAM_PRIORITY) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) return COA_EHIP;
    e = hipStreamCreateWithPriority(&sl.s, hipStreamNonBlocking, sl.lane == coa_q::LANE_VERIFY ? greatest : least);
  } else {
    e = hipStreamCreateWithFlags(&sl.s, hipStreamNonBlocking);
  }
  if (e != hipSuccess || hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming) != hipSuccess) return COA_EHIP;
  return COA_OK;
}

// True when rocprofv3's tool library is loaded into this process (the
// environment rocprofv3 gives the program it runs).  The slots then use plain
// streams: CU-masked stream creation under its tracer is what faulted in
// round 5 (see stream_pool), and the kernels -- what a profile measures --
// are the same on either kind.
bool under_rocprofiler() { return env_str("ROCP_TOOL_LIBRARIES") || env_str("ROCPROFILER_LIBRARY_CTOR"); }

int stream_kind_env() {
  if (!env_str("COA_QUEUE_STREAMS")) return under_rocprofiler() ? COA_QUEUE_STREAM_PLAIN : COA_QUEUE_STREAM_CUMASK;
  if (env_is("COA_QUEUE_STREAMS", "plain")) return COA_QUEUE_STREAM_PLAIN;
  if (env_is("COA_QUEUE_STREAMS", "priority")) return COA_QUEUE_STREAM_PRIORITY;
  return COA_QUEUE_STREAM_CUMASK;
}

void free_slot(Slot& sl) {
  if (sl.dev < 0) return;
  (void)hipSetDevice(sl.dev);
  if (sl.s) (void)hipStreamSynchronize(sl.s);
  if (sl.hin) (void)hipHostFree(sl.hin);
  if (sl.hout) (void)hipHostFree(sl.hout);
  if (sl.din) (void)hipFree(sl.din);
  if (sl.dout) (void)hipFree(sl.dout);
  if (sl.ws) (void)hipFree(sl.ws);
  if (sl.lres) (void)hipHostFree(sl.lres);
  if (sl.dctr) (void)hipFree(sl.dctr);
  if (sl.ev) (void)hipEventDestroy(sl.ev);
  pool_give(sl);
  bury(sl.grave);
}

class HipBackend : public coa_q::Backend {
 public:
  explicit HipBackend(int lane) : lane_(lane) {
    msg_lat_max_ = (size_t)env_u64("COA_QUEUE_MSG_LAT_MAX", msg_lat_max_);
  }
  ~HipBackend() override {
    for (Slot& sl : slots_) free_slot(sl);
    for (Slot& sl : rescue_) free_slot(sl);
  }

  int slots() const override { return (int)slots_.size(); }
  int devices() const override { return std::max<int>(1, (int)devs_.size()); }
  // windows of this queue lane that had to enlarge a slot's staging or
  // workspace (the warm-up at creation not counted)
  uint64_t grows() const override { return grows_.load(); }
  void reset_grows() override { grows_.store(0); }

  // Everything a first window would otherwise pay for, done at queue
  // creation: the slots' streams, their page-locked and device staging, and
  // one small copy through each stream, which makes HIP create the stream's
  // hardware queue (a CU-masked stream's first dispatch took ~25-75 ms:
  // round-4 paced runs, one queue per rate, p99 20-75 ms from that alone).
  //
  // The verify lane is sized for the largest window the collector can close:
  // whole shards are taken until max_batch items are in, and a shard holds up
  // to max_batch items, so a window holds < 2 x max_batch items.  Certificate
  // items (a certificate and its votes: 9,920 B per committee-100 certificate
  // of 68 items) take <= 160 B each in the input block, signatures 128 B.
  // Sized for half of that (grow_* double it), staging never regrows on the
  // launch path (round 4's streamed C3 regrew 2-4 times per run, windows of
  // up to 107 K items, p99 wait 8-12 ms).
  void prepare(size_t max_batch) override {
    if (!ready()) return;
    // capped at 65,536 (a larger max_batch's windows regrow on demand): a
    // queue made with max_batch 2^20 would otherwise stage ~20 GB of HBM
    const size_t items = std::min<size_t>(std::max<size_t>(max_batch, 1024), 65536);
    const size_t pre_in = lane_ == coa_q::LANE_DIGEST ? (32u << 20) : items * 160 + (1u << 20);
    const size_t pre_out = lane_ == coa_q::LANE_DIGEST ? (256u << 10) : items * 4 + (64u << 10);
    // workspace for the widest window of each kind (each regrowth is a
    // hipMalloc on the launch path: the round mix showed 6-9 per queue, with
    // windows held 3-12 ms)
    const size_t pre_ws = lane_ == coa_q::LANE_DIGEST
                              ? 256
                              : std::max(coa_verify_workspace_bytes(items),
                                         coa_cert_scratch_bytes(items / 68 + 1 + items, keysort_)) + 256;
    for (Slot& sl : slots_) {
      if (lane_ == coa_q::LANE_VERIFY && hipSetDevice(sl.dev) == hipSuccess) {
        (void)lat_words(sl);
        (void)ctr_words(sl);
      }
      if (hipSetDevice(sl.dev) != hipSuccess || grow_pinned(sl.hin, sl.cap_hin, pre_in, sl.grave) != hipSuccess ||
          grow_pinned(sl.hout, sl.cap_hout, pre_out, sl.grave) != hipSuccess ||
          grow_dev(sl.din, sl.cap_din, pre_in, sl.grave) != hipSuccess ||
          grow_dev(sl.dout, sl.cap_dout, pre_out, sl.grave) != hipSuccess ||
          grow_dev(sl.ws, sl.cap_ws, pre_ws, sl.grave) != hipSuccess)
        continue;  // the first launch regrows and reports any failure
      (void)hipMemcpyAsync(sl.din, sl.hin, 4096, hipMemcpyHostToDevice, sl.s);
      (void)hipMemsetAsync(sl.dout, 0, 4096, sl.s);
      (void)hipStreamSynchronize(sl.s);
    }
    (void)hipGetLastError();
  }
  int stream_kind() const override { return kind_; }

  // The slot's page-locked result words for inline latency windows
  // (allocated once; null when the allocation failed: such windows then take
  // the staged path)
  static uint32_t* lat_words(Slot& sl) {
    if (!sl.lres && hipHostMalloc(reinterpret_cast<void**>(&sl.lres), COA_PUBLISH_WORDS * sizeof(uint32_t),
                                  hipHostMallocCoherent) != hipSuccess) {
      sl.lres = nullptr;
      (void)hipGetLastError();
    }
    return sl.lres;
  }
  // ... and its device counter block for published certificate windows
  // (zeroed once; the kernel re-zeroes it after each window)
  static uint32_t* ctr_words(Slot& sl) {
    if (!sl.dctr) {
      if (hipMalloc(reinterpret_cast<void**>(&sl.dctr), 65 * sizeof(uint32_t)) != hipSuccess ||
          hipMemset(sl.dctr, 0, 65 * sizeof(uint32_t)) != hipSuccess) {
        if (sl.dctr) (void)hipFree(sl.dctr);
        sl.dctr = nullptr;
        (void)hipGetLastError();
      }
    }
    return sl.dctr;
  }

  void launch(coa_q::Launch& L) override {
    if (!ready()) {
      L.rc = init_rc_;
      return;
    }
    Slot* sl;
    bool inject = false;
    {
      // the next free slot in turn (a busy slot is passed over, not waited for)
      std::unique_lock<std::mutex> l(m_);
      auto free_slot = [&]() -> long {
        for (size_t k = 0; k < slots_.size(); k++) {
          const size_t i = (next_ + k) % slots_.size();
          if (!slots_[i].busy) return (long)i;
        }
        return -1;
      };
      long k = free_slot();
      if (k < 0) {
        const auto t0 = std::chrono::steady_clock::now();
        cv_.wait(l, [&] { return (k = free_slot()) >= 0; });
        L.slot_wait_ns = std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0)
                             .count();
      }
      next_ = (size_t)k + 1;
      slots_[k].busy = true;
      L.slot = (int)k;
      sl = &slots_[k];
      inject = fault_every_ && ++launches_ % fault_every_ == 0;
    }
    sl->launched = false;
    L.rc = enqueue(*sl, L, inject);
  }

  bool wait_free_slot() override {
    if (!ready()) return false;
    std::unique_lock<std::mutex> l(m_);
    auto any_free = [&] {
      for (const Slot& s : slots_)
        if (!s.busy) return true;
      return false;
    };
    if (any_free()) return false;
    cv_.wait(l, any_free);
    return true;
  }

  void complete(coa_q::Launch& L) override {
    if (L.slot < 0) return;  // never staged (no device)
    Slot& sl = slots_[L.slot];
    finish(sl, L);
    if (L.rc != COA_OK) (void)make_stream(sl);  // rebuilt before reuse
    std::lock_guard<std::mutex> l(m_);
    sl.busy = false;
    cv_.notify_all();
  }

  void retry(coa_q::Launch& L, int attempt) override {
    if (!ready() || devs_.empty()) {
      L.rc = init_rc_ != COA_OK ? init_rc_ : COA_ENODEVICE;
      return;
    }
    size_t pos = 0;
    if (L.slot >= 0)
      for (size_t i = 0; i < devs_.size(); i++)
        if (devs_[i] == slots_[L.slot].dev) pos = i;
    Slot& sl = rescue_[(pos + (size_t)attempt) % devs_.size()];
    if (!sl.s && make_stream(sl) != COA_OK) {
      L.rc = COA_EHIP;
      return;
    }
    sl.launched = false;
    L.rc = enqueue(sl, L, false);
    finish(sl, L);
    if (L.rc != COA_OK) (void)make_stream(sl);
  }

 private:
  bool ready() {
    std::lock_guard<std::mutex> l(m_);
    if (inited_) return init_rc_ == COA_OK;
    inited_ = true;
    int ids[64];
    const int n = coa_device_ids(ids, 64);
    if (n <= 0) {
      init_rc_ = n < 0 ? n : COA_ENODEVICE;
      return false;
    }
    const int nctx = std::min(n, 64);
    for (int i = 0; i < nctx; i++)
      if (std::find(devs_.begin(), devs_.end(), ids[i]) == devs_.end()) devs_.push_back(ids[i]);
    // device slots per GPU (not per engine context: eight contexts open on
    // one GPU made 32 slots per lane there, 64 CU-masked streams and so 64
    // hardware queues on one device, more than its scheduler maps at once --
    // the suspected cause of round 4's 84-149 ms window on a re-opened
    // 8-context engine): windows in flight at once (1..8; COA_QUEUE_SLOTS for
    // the verify lane, COA_QUEUE_DIGEST_SLOTS for the digest lane;
    // tools/queue_probe.c measures the choice)
    size_t per = lane_ == coa_q::LANE_DIGEST ? COA_QUEUE_DIGEST_SLOTS_DEFAULT : COA_QUEUE_SLOTS_DEFAULT;
    const long v = env_int(lane_ == coa_q::LANE_DIGEST ? "COA_QUEUE_DIGEST_SLOTS" : "COA_QUEUE_SLOTS", 0);
    if (v >= 1 && v <= 8) per = (size_t)v;  // anything else: the default
    fault_every_ = env_u64("COA_QUEUE_FAULT", fault_every_);
    // COA_QUEUE_INLINE=0: small signature windows take the staged path too (A/B)
    inline_ok_ = env_on("COA_QUEUE_INLINE", inline_ok_);
    // COA_QUEUE_KEYSORT=0|1: certificate windows of >= 16,384 jobs take their
    // jobs in committee-key order (coa_certificate_verify_many_device_order).
    // Default on: round 6's same-box A/B of the streamed C3 lines was within
    // noise either way (profiles/r06_keysort_ab.txt), and the fused kernel's
    // translation misses fall from ~50 % to ~1.5 % of requests in key order
    // (round 5); coa_committee.hip's note that queue windows do not sort
    // predates this switch
    keysort_ = env_on("COA_QUEUE_KEYSORT", keysort_);
    kind_ = stream_kind_env();
    slots_.resize(per * devs_.size());
    // (page-locked staging is sized by prepare(): a reallocation on the
    // launch path is a hipHostFree/hipHostMalloc pair, milliseconds)
    for (size_t k = 0; k < slots_.size(); k++) {
      Slot& sl = slots_[k];
      sl.dev = devs_[k % devs_.size()];
      sl.kind = kind_;
      sl.lane = lane_;
      if (make_stream(sl) != COA_OK) {
        init_rc_ = COA_EHIP;
        return false;
      }
    }
    rescue_.resize(devs_.size());
    for (size_t i = 0; i < devs_.size(); i++) {
      rescue_[i].dev = devs_[i];
      rescue_[i].kind = kind_;
      rescue_[i].lane = lane_;
    }
    return true;
  }

  // The next tag of the slot's result words, the launch's n of them cleared
  // (no tag matches 0).
  static void new_tag(Slot& sl, size_t n) {
    std::memset(sl.lres, 0, n * sizeof(uint32_t));
    sl.ltag = (sl.ltag + 1) & 0xffffffu;
    if (sl.ltag == 0) sl.ltag = 1;
    sl.npub = n;
  }

  // Layout, pack, route (coa_qstage.h): the launch's parts packed into the
  // slot's page-locked input block, then one of the publish routes
  // (Slot::route) when the window is small and of one kind, else the staged
  // route.
  int enqueue(Slot& sl, coa_q::Launch& L, bool inject) {
    if (hipSetDevice(sl.dev) != hipSuccess) return COA_EHIP;
    const auto t_pack = std::chrono::steady_clock::now();
    // a window of few signatures takes the latency kernel (one four-wave
    // workgroup per signature: ~0.1 ms however few, against ~0.8 ms for the
    // one-lane throughput kernels); its inputs are interleaved 128-byte
    // records and its results 32-bit words
    sl.lat = L.nv > 0 && L.nv <= coa_lat_max();
    sl.pack = coa_q::window_layout(L, sl.lat);
    sl.route = coa_q::ROUTE_STAGED;
    const coa_q::WindowPack& p = sl.pack;
    const size_t msgs = L.nhd + L.nvt;
    const bool msg_lat = msgs > 0 && msgs <= msg_lat_max_;
    const size_t ws_m = (msgs && !msg_lat) ? coa_message_workspace_bytes(std::max(L.nhd, L.nvt)) : 0;
    const size_t ws_v = L.nv ? coa_verify_workspace_bytes(L.nv) : 0;
    const size_t ws_c = L.nc ? coa_cert_scratch_bytes(L.nc + L.nvotes, keysort_) : 0;
    const size_t caps0 = sl.cap_hin + sl.cap_hout + sl.cap_din + sl.cap_dout + sl.cap_ws;
    if (grow_pinned(sl.hin, sl.cap_hin, p.in_total, sl.grave) != hipSuccess ||
        grow_pinned(sl.hout, sl.cap_hout, p.out_total, sl.grave) != hipSuccess ||
        grow_dev(sl.din, sl.cap_din, p.in_total, sl.grave) != hipSuccess ||
        grow_dev(sl.dout, sl.cap_dout, p.out_total, sl.grave) != hipSuccess ||
        grow_dev(sl.ws, sl.cap_ws, std::max(std::max(ws_v, ws_c), ws_m) + 256, sl.grave) != hipSuccess)
      return COA_ENOMEM;
    if (sl.cap_hin + sl.cap_hout + sl.cap_din + sl.cap_dout + sl.cap_ws != caps0) grows_++;
    // the bulk copies of a large window go to the runtime's copy threads (a
    // C3 round is ~68 MB: one thread's memcpy would be slower than PCIe)
    std::vector<Seg> bulk;
    coa_q::window_pack(static_cast<uint8_t*>(sl.hin), p, L, bulk);
    size_t bulk_bytes = 0;
    for (const Seg& g : bulk) bulk_bytes += g.bytes;
    if (bulk_bytes >= (1u << 20)) {
      coa_copy_segments(bulk.data(), bulk.size());
    } else {
      for (const Seg& g : bulk) std::memcpy(g.dst, g.src, g.bytes);
    }
    const auto t_enq = std::chrono::steady_clock::now();
    L.stage_ns[COA_QSTAGE_PACK] += ns_between(t_pack, t_enq);
    if (L.nv + L.nc + L.nd + msgs == 0) return COA_OK;  // bare vote batches only: left to resolve()
    EnqClock clk{L, t_enq, t_enq};
    const bool alone_v = L.nc == 0 && L.nd == 0 && msgs == 0, alone_c = L.nv == 0 && L.nd == 0 && msgs == 0,
               alone_m = L.nv == 0 && L.nc == 0 && L.nd == 0;
    if (inline_ok_ && sl.lat && L.nv <= COA_LAT_INLINE && alone_v && lat_words(sl) != nullptr) {
      sl.route = coa_q::ROUTE_SIG_INLINE;
      return enqueue_sig_inline(sl, L, inject, clk);
    }
    // a window with a verdict request takes the staged route: its words are a
    // section of the output block (a certificate's published word has 8 status
    // bits, no room for a vote index).  Except message windows of verdict
    // requests alone, small enough for the latency kernel: k_msg_verdict_lat
    // answers their words itself, on the routes of the crypto messages
    const bool verd = L.verdicts();
    L.msg_words = msg_lat && L.all_message_verdicts();
    if (inline_ok_ && !verd && L.nc > 0 && L.nc <= COA_PUBLISH_WORDS && alone_c && lat_words(sl) != nullptr &&
        ctr_words(sl) != nullptr) {
      sl.route = coa_q::ROUTE_CERT_PUBLISH;
      const int rc = enqueue_cert_publish(sl, L, inject, clk);
      if (rc != 1) return rc;
      sl.route = coa_q::ROUTE_STAGED;  // too many jobs for the latency kernel
    }
    if (msgs) L.msg_route = msg_lat ? coa_q::Launch::MSG_LATENCY : coa_q::Launch::MSG_THROUGHPUT;
    if (inline_ok_ && (!verd || L.msg_words) && msg_lat && msgs <= COA_PUBLISH_WORDS && alone_m &&
        lat_words(sl) != nullptr && ctr_words(sl) != nullptr) {
      sl.route = coa_q::ROUTE_MSG_PUBLISH;
      const int rc = enqueue_msg_publish(sl, L, inject, clk);
      if (rc != 1) return rc;
      // no protocol table: no kernel ran and nothing is published; the input
      // copy in flight is waited for as on the staged route
      sl.route = coa_q::ROUTE_STAGED;
      L.verdict_rc = COA_EINVAL;
      return record(sl, clk);
    }
    return enqueue_staged(sl, L, msg_lat, inject, clk);
  }

  // The ENQUEUE stage of a launch: all of enqueue() after the pack, whichever
  // way it returns, and its parts (Launch::enq_ns) -- each mark() charges the
  // time since the previous one to part k.
  struct EnqClock {
    coa_q::Launch& L;
    const std::chrono::steady_clock::time_point t0;
    std::chrono::steady_clock::time_point t_mark;
    ~EnqClock() { L.stage_ns[COA_QSTAGE_ENQUEUE] += ns_between(t0, std::chrono::steady_clock::now()); }
    void mark(int k) {
      const auto t = std::chrono::steady_clock::now();
      L.enq_ns[k] += ns_between(t_mark, t);
      t_mark = t;
    }
  };

  // The committee key-cache generation a route's launches read, for its
  // scope: the one the slot has pinned, the current one pinned first when it
  // holds none (finish() un-pins it -- a registration meanwhile builds the
  // next generation beside it).
  struct KeyUse {
    explicit KeyUse(Slot& sl, bool pin = true) {
      if (pin && !sl.keys) sl.keys = coa_keycache_pin(sl.dev);
      coa_keycache_use(sl.keys);
    }
    ~KeyUse() { coa_keycache_use(nullptr); }
  };

  // One H2D copy of the whole input block.
  static int copy_in(Slot& sl, EnqClock& clk) {
    if (hipMemcpyAsync(sl.din, sl.hin, sl.pack.in_total, hipMemcpyHostToDevice, sl.s) != hipSuccess) return COA_EHIP;
    clk.mark(coa_q::Launch::ENQ_H2D);
    sl.launched = true;
    return COA_OK;
  }
  // The event finish() waits for, or queries while it polls.
  static int record(Slot& sl, EnqClock& clk) {
    const hipError_t e = hipEventRecord(sl.ev, sl.s);
    clk.mark(coa_q::Launch::ENQ_EVENT);
    return e == hipSuccess ? COA_OK : COA_EHIP;
  }

  // The window's headers and votes in block d, as the latency entries take them.
  static CoaMsgLatIn msg_lat_in(const uint8_t* d, const coa_q::WindowPack& p, const coa_q::Launch& L) {
    const MsgIn h = msg_view(d, p.hdr, false), v = msg_view(d, p.vote, true);
    CoaMsgLatIn in{};
    if (L.nhd) {
      in.hdr_data = h.hdr_data, in.hdr_off = h.hdr_off;
      in.hids = h.ids, in.hauthors = h.authors, in.hsigs = h.sigs, in.nh = L.nhd;
    }
    if (L.nvt) {
      in.vids = v.ids, in.vrounds = v.rounds, in.vorigins = v.origins;
      in.vauthors = v.authors, in.vsigs = v.sigs, in.nv = L.nvt;
    }
    return in;
  }

  // The headers' payload counts in block d (a window with verdict requests).
  static const uint32_t* h_pcounts(const void* d, const coa_q::WindowPack& p) {
    return reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(d) + p.hdr.pcounts.at);
  }

  // A few signatures alone (Header::verify / Vote::verify at low load): the
  // packed records go in the kernel arguments and the verdict words come back
  // by the kernel's own stores, as coa_ed25519_verify_strict does -- the
  // staged route's two copies (and the event wait) were most of such a
  // window's time besides the kernel.
  static int enqueue_sig_inline(Slot& sl, coa_q::Launch& L, bool inject, EnqClock& clk) {
    new_tag(sl, L.nv);
    sl.launched = true;
    if (inject) return COA_EHIP;  // fault injection: nothing launched
    int rc;
    {
      KeyUse keys(sl);
      clk.mark(coa_q::Launch::ENQ_PIN);
      rc = coa_lat_verify_inline(sl.dev, static_cast<const uint8_t*>(sl.hin) + sl.pack.v_recs.at, L.nv, sl.lres,
                                 sl.ltag, sl.s);
    }
    clk.mark(coa_q::Launch::ENQ_LAUNCH);
    return rc == COA_OK ? record(sl, clk) : rc;
  }

  // Certificates alone, few (Certificate::verify at low load).  Returns 1,
  // with nothing enqueued, when their jobs exceed the latency kernel's: the
  // window then takes the staged route.
  static int enqueue_cert_publish(Slot& sl, coa_q::Launch& L, bool inject, EnqClock& clk) {
    if (inject) {
      sl.launched = true;
      return COA_EHIP;  // fault injection: nothing launched
    }
    new_tag(sl, L.nc);
    int rc;
    {
      KeyUse keys(sl);
      clk.mark(coa_q::Launch::ENQ_PIN);
      rc = coa_certificate_verify_publish(sl.dev, static_cast<const uint8_t*>(sl.hin), static_cast<uint8_t*>(sl.din),
                                          sl.pack.in_total, &sl.pack.cert, L.nc, L.nvotes, sl.dctr, sl.lres, sl.ltag,
                                          sl.s);
    }
    clk.mark(coa_q::Launch::ENQ_LAUNCH);  // (its H2D copy, when the window does not fit the arguments, included)
    if (rc == 1) return 1;
    sl.launched = true;  // on a failure something may be enqueued: finish() drains the stream
    return rc == COA_OK ? record(sl, clk) : rc;
  }

  // Headers and votes alone, few (Header::verify / Vote::verify at low load).
  // No status memset, no D2H copy, no event wait.
  static int enqueue_msg_publish(Slot& sl, coa_q::Launch& L, bool inject, EnqClock& clk) {
    new_tag(sl, L.nhd + L.nvt);
    if (copy_in(sl, clk) != COA_OK) return COA_EHIP;
    if (inject) return COA_EHIP;  // fault injection: the copy is in flight, the kernel never runs
    const CoaMsgLatIn in = msg_lat_in(static_cast<const uint8_t*>(sl.din), sl.pack, L);
    int rc;
    {
      KeyUse keys(sl);
      clk.mark(coa_q::Launch::ENQ_PIN);
      if (L.msg_words)
        rc = coa_msg_lat_verdict_publish(sl.dev, &in, h_pcounts(sl.din, sl.pack), sl.dctr, sl.lres, sl.ltag, sl.s);
      else
        rc = coa_msg_lat_verify_publish(sl.dev, &in, sl.dctr, sl.lres, sl.ltag, sl.s);
    }
    clk.mark(coa_q::Launch::ENQ_LAUNCH);
    return rc == COA_OK ? record(sl, clk) : rc;  // 1: see enqueue()
  }

  // Everything else: ONE H2D copy, the device-resident entry of each kind the
  // window holds, ONE D2H copy of the output block.
  int enqueue_staged(Slot& sl, coa_q::Launch& L, bool msg_lat, bool inject, EnqClock& clk) {
    if (copy_in(sl, clk) != COA_OK) return COA_EHIP;
    if (inject) return COA_EHIP;  // fault injection: the copy is in flight, the kernels never run
    const coa_q::WindowPack& p = sl.pack;
    const uint8_t* d = static_cast<const uint8_t*>(sl.din);
    uint8_t* dout = static_cast<uint8_t*>(sl.dout);
    auto out_words = [dout](const Sec& s) { return reinterpret_cast<uint32_t*>(dout + s.at); };
    const size_t msgs = L.nhd + L.nvt;
    int rc = COA_OK;
    {
      // the latency, certificate and message kernels read the key cache
      KeyUse keys(sl, sl.lat || L.nc || msgs);
      clk.mark(coa_q::Launch::ENQ_PIN);
      if (L.nv && sl.lat)
        rc = coa_lat_verify_device(sl.dev, d + p.v_recs.at, L.nv, out_words(p.o_sigs), sl.s);
      else if (L.nv)
        rc = coa_ed25519_verify_strict_many_device(sl.dev, d + p.v_msgs.at, 32, d + p.v_pks.at, d + p.v_sigs.at, L.nv,
                                                   dout + p.o_sigs.at, sl.ws, sl.s);
      if (rc == COA_OK && L.nc) {
        // key order for a large window (COA_QUEUE_KEYSORT): see
        // coa_certificate_verify_many_device_order
        const CertIn c = cert_view(d, p.cert);
        rc = coa_certificate_verify_many_device_order(sl.dev, c.hdr_data, c.hdr_off, c.ids, c.origins, c.hsigs,
                                                      c.rounds, c.vpks, c.vsigs, c.voff, L.nc, L.nvotes,
                                                      out_words(p.o_certs), sl.ws, sl.s, keysort_ ? 1 : 0);
      }
      uint32_t* d_mst = out_words(p.o_msgs);  // the headers' status words, then the votes'
      if (rc == COA_OK && L.msg_words) {  // the messages' verdict words, in the status words' place
        const CoaMsgLatIn in = msg_lat_in(d, p, L);
        rc = coa_msg_lat_verdict_device(sl.dev, &in, h_pcounts(d, p), d_mst, sl.s);
        if (rc == 1) {  // no protocol table in the pinned generation: the verdict requests' own status
          L.verdict_rc = COA_EINVAL;
          rc = COA_OK;
        }
      } else if (rc == COA_OK && msg_lat) {
        const CoaMsgLatIn in = msg_lat_in(d, p, L);
        rc = coa_msg_lat_verify_device(sl.dev, &in, d_mst, sl.s);
      } else if (rc == COA_OK && msgs) {
        const MsgIn h = msg_view(d, p.hdr, false), v = msg_view(d, p.vote, true);
        if (L.nhd)
          rc = coa_header_verify_many_device(sl.dev, h.hdr_data, h.hdr_off, h.ids, h.authors, h.sigs, L.nhd, d_mst,
                                             sl.ws, sl.s);
        if (rc == COA_OK && L.nvt)
          rc = coa_vote_verify_many_device(sl.dev, v.ids, v.rounds, v.origins, v.authors, v.sigs, L.nvt,
                                           d_mst + L.nhd, sl.ws, sl.s);
      }
      // the verdict words of every certificate, header and vote of a window
      // with verdict requests: one launch behind the crypto entries, over the
      // same staged arrays and their raw words
      if (rc == COA_OK && L.verdicts() && !L.msg_words) {
        const CertIn c = cert_view(d, p.cert);
        const MsgIn h = msg_view(d, p.hdr, false), v = msg_view(d, p.vote, true);
        CoaWindowVerdictIn in{};
        in.c_hdr_data = c.hdr_data, in.c_hdr_off = c.hdr_off, in.c_ids = c.ids, in.c_origins = c.origins;
        in.c_rounds = c.rounds, in.c_vpks = c.vpks, in.c_voff = c.voff;
        in.c_pcounts = reinterpret_cast<const uint32_t*>(d + p.cert.pcounts.at);
        in.nc = L.nc, in.n_votes = L.nvotes;
        in.h_hdr_data = h.hdr_data, in.h_hdr_off = h.hdr_off, in.h_authors = h.authors;
        in.h_pcounts = reinterpret_cast<const uint32_t*>(d + p.hdr.pcounts.at);
        in.nh = L.nhd;
        in.v_authors = v.authors, in.nv = L.nvt;
        in.cert_raw = out_words(p.o_certs), in.msg_raw = d_mst, in.words = out_words(p.o_words);
        rc = coa_window_verdict_device(sl.dev, &in, sl.s);
        if (rc == 1) {  // no protocol table in the pinned generation: the verdict requests' own status
          L.verdict_rc = COA_EINVAL;
          rc = COA_OK;
        }
      }
      if (rc == COA_OK && L.nd)
        rc = coa_sha512_many_device(sl.dev, d + p.d_data.at, reinterpret_cast<const uint64_t*>(d + p.d_off.at), L.nd,
                                    dout + p.o_digs.at, sl.s);
    }
    clk.mark(coa_q::Launch::ENQ_LAUNCH);
    if (rc != COA_OK) return rc;
    if (hipMemcpyAsync(sl.hout, dout, p.out_total, hipMemcpyDeviceToHost, sl.s) != hipSuccess) return COA_EHIP;
    clk.mark(coa_q::Launch::ENQ_D2H);
    return record(sl, clk);
  }

  // Waits for the slot's work (a failed enqueue drains its stream, keeping
  // the error), then scatters the outputs to the parts; what the kernels left
  // open (and every bare vote batch) is marked for resolve().
  void finish(Slot& sl, coa_q::Launch& L) {
    const auto t_wait = std::chrono::steady_clock::now();
    if (sl.launched) {
      (void)hipSetDevice(sl.dev);
      if (L.rc == COA_OK && sl.route != coa_q::ROUTE_STAGED) {
        L.rc = poll_words(sl);
      } else if (L.rc == COA_OK) {
        if (hipEventSynchronize(sl.ev) != hipSuccess) L.rc = COA_EHIP;
      } else {
        (void)hipStreamSynchronize(sl.s);  // nothing may still read the staging when the slot is reused
      }
      sl.launched = false;
    }
    const auto t_scatter = std::chrono::steady_clock::now();
    L.stage_ns[COA_QSTAGE_DEVICE_WAIT] += ns_between(t_wait, t_scatter);
    if (L.rc == COA_OK) coa_q::window_scatter(L, sl.pack, static_cast<const uint8_t*>(sl.hout), sl.route, sl.lres);
    if (sl.keys) {
      coa_keycache_unpin(sl.keys);
      sl.keys = nullptr;
    }
    L.stage_ns[COA_QSTAGE_SCATTER] += ns_between(t_scatter, std::chrono::steady_clock::now());
  }

  // A publish route's result words (Slot::npub of them), polled for the
  // slot's tag.  A kernel that ended without publishing (a fault) ends the
  // wait through the slot's event; a bound stops a hang.  On failure the
  // stream is drained before the slot is reused.
  static int poll_words(Slot& sl) {
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t i = 0; i < sl.npub; i++) {
      const volatile uint32_t* w = sl.lres + i;
      for (uint64_t spin = 0; (*w >> 8) != sl.ltag; spin++) {
        if ((spin & 1023) != 1023) continue;
        const hipError_t q = hipEventQuery(sl.ev);
        const bool stuck = std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10);
        if ((q != hipSuccess && q != hipErrorNotReady) || (q == hipSuccess && (*w >> 8) != sl.ltag) || stuck) {
          (void)hipStreamSynchronize(sl.s);
          return COA_EHIP;
        }
      }
    }
    return COA_OK;
  }

 public:
  // The open certificates of every window in `ws` in one exact pass
  // (coa_certificate_resolve_raw: header signature by verify_strict and votes
  // by the RLC kernels for a key outside the committee, the RLC kernels alone
  // for inconclusive votes -- never the fused kernel again), and every bare
  // vote batch in one coa_ed25519_verify_batch_groups call.
  int resolve(const std::vector<coa_q::Window*>& ws) override {
    coa_q::Deferred d = coa_q::gather_deferred(ws);
    // the open messages: verify_strict through the uncached path, the votes
    // over Vote::digest
    for (int vote = 0; vote < 2; vote++) {
      if (d.m_raw[vote].empty()) continue;
      const int rc = coa_message_resolve_raw(d.m_ids[vote].data(), vote ? d.m_rounds.data() : nullptr,
                                             vote ? d.m_origins.data() : nullptr, d.m_authors[vote].data(),
                                             d.m_sigs[vote].data(), d.m_raw[vote].size(), d.m_raw[vote].data());
      if (rc != COA_OK) return rc;
    }
    coa_q::put_messages(ws, d);
    if (!d.c_raw.empty()) {
      std::vector<uint8_t> out(d.c_raw.size(), 7);
      const int rc = coa_certificate_resolve_raw(d.c_ids.data(), d.c_origins.data(), d.c_hsigs.data(),
                                                 d.c_rounds.data(), d.c_vpks.data(), d.c_vsigs.data(),
                                                 d.c_voff.data(), d.c_raw.size(), d.c_raw.data(), out.data());
      if (rc != COA_OK) return rc;
      coa_q::put_certs(ws, out.data());
    }
    if (d.g_off.size() > 1) {
      std::vector<uint8_t> out(d.g_off.size() - 1, 1);
      const int rc = coa_ed25519_verify_batch_groups(d.g_msgs.data(), d.g_pks.data(), d.g_sigs.data(),
                                                     d.g_off.data(), d.g_off.size() - 1, out.data(), 0);
      if (rc != COA_OK) return rc;
      coa_q::put_groups(ws, out.data());
    }
    return COA_OK;
  }

 private:
  std::vector<Slot> slots_;
  std::vector<Slot> rescue_;  // one recovery context per device, used only by retry()
  std::vector<int> devs_;     // distinct device ids
  const int lane_;
  int kind_ = COA_QUEUE_STREAM_PLAIN;
  std::atomic<uint64_t> grows_{0};
  size_t next_ = 0;
  std::mutex m_;
  std::condition_variable cv_;
  bool inited_ = false;
  int init_rc_ = COA_OK;
  unsigned long long fault_every_ = 0, launches_ = 0;
  bool inline_ok_ = true;  // COA_QUEUE_INLINE
  bool keysort_ = true;     // COA_QUEUE_KEYSORT
  size_t msg_lat_max_ = COA_QUEUE_MSG_LAT_MAX_DEFAULT;
};

}  // namespace

coa_q::Backend* coa_q::make_backend(int lane) { return new HipBackend(lane); }

// The host runtime behind include/coa_verify.h, shared by its translation
// units (internal; nothing here is exported):
//   coa_engine.cpp  the core: init and shutdown, the device contexts, the
//                   key-cache generations and their trailing, sharding and
//                   recovery, the latency path's result words
//   coa_sig.cpp     entries: signatures, batches, SHA-512, signing
//   coa_dag.cpp     entries: certificates, messages, verdicts, registrations
//   coa_hostpool.h  Worker and CopyPool          (host-only, no HIP)
//   coa_env.h       the COA_* switch readers     (host-only)
//   coa_offsets.h   offset checks, digest input  (host-only)
//
// * One context per GPU: a non-blocking HIP stream, the fixed-base B table
//   (built on the device by k_build_btable at coa_init), growable device
//   buffers and its own host worker thread ("each GPU has its
//   own host thread, context and streams").  Each context has its own mutex; a
//   shard holds its context's mutex until the context's stream drains.
// * Host-pointer "many" calls shard items by contiguous index range over the
//   opened contexts: every shard runs on its context's worker
//   thread, so the shards' copies, launches and waits proceed concurrently; no
//   cross-GPU exchange, verdict bytes land in place in the caller's output
//   slice.  A call with one shard runs on the caller's thread (no hop).
// * Device-pointer calls enqueue on the caller's stream and return.
// * No CPU fallback anywhere: without a usable GPU, calls fail with
//   COA_ENODEVICE.
#pragma once

#include "../../include/coa_verify.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "coa_committee.h"
#include "coa_env.h"
#include "coa_hostpool.h"
#include "coa_latency.h"
#include "coa_offsets.h"
#include "coa_protocol.h"

namespace coa_rt __attribute__((visibility("hidden"))) {

// The engine's thread-locals live in coa_engine.cpp alone and are reached
// through these functions: an `extern thread_local` read from another file
// goes through a wrapper that calls the variable's init function by a weak
// reference, and for a variable that needs none that reference is undefined
// -- with this namespace's hidden visibility it does not even compare equal
// to null in position-independent code.
// This thread's coa_last_error text; fail() sets it and returns `code`.
std::string& last_error();
int fail(int code, const std::string& msg);
// True on a context worker thread: nested sharded calls then run inline
// (a worker never waits for its own queue).
bool in_worker();

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) return fail(COA_EHIP, std::string(#expr ": ") + hipGetErrorString(e_)); \
  } while (0)

// Growable device memory; freed with its owner (whose destructor makes the
// device current first).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  // exact: no 25 % growth headroom (multi-GB tables)
  hipError_t ensure(size_t bytes, bool exact = false) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = exact ? bytes : std::max<size_t>(bytes + bytes / 4, 4096);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Page-locked host staging (hipHostMalloc), growable: one H2D copy per call
// on the certificate path.
struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 4, 1 << 16);
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

// One committee's key tables on one device (f2): sorted keys, flags, a
// radix-256 comb of -A per key and (within the HBM budget) the wide combs.
// Immutable once built and shared by every context open on the device; a
// registration builds the next generation beside it (DevShared).
struct KeySet {
  int dev = -1;
  DevBuf ckeys, kflags, ktabs, kwtabs;
  uint32_t nkeys = 0;
  bool kwide = false;  // kwtabs holds the committee's wide combs
  bool kw20 = false;   // ... in the radix-2^20 layout (COA_KWCOMB20_*)
  // protocol table (coa_committee_register_authorities): stake [nkeys] |
  // worker offsets [nkeys + 1] | worker ids, in the sorted key order
  DevBuf prot;
  bool has_prot = false;
  uint32_t quorum = 0;
  KeySet() = default;
  KeySet(const KeySet&) = delete;
  KeySet& operator=(const KeySet&) = delete;
  ~KeySet() {  // the buffers free themselves next
    if (dev >= 0) (void)hipSetDevice(dev);
  }
};
using KeySetP = std::shared_ptr<const KeySet>;

// What the contexts open on one HIP device share: B's wide comb (11 GiB,
// built once per device, not once per context) and the current key-cache
// generation.  coa_committee_register builds a new generation on `build`
// (no context's lock, stream or buffers), swaps it in under `mu`, and frees
// the old one once no call or queue window holds it.
struct DevShared {
  int id = -1;
  // wide B comb: COA_WCOMB_ENTRIES = 11 x 2^23 entries of COA_WC_STRIDE = 32
  // dwords (128 B) at W = 24: 11 GiB = 11.8 GB
  uint32_t* wcomb = nullptr;
  hipStream_t build = nullptr;
  std::mutex mu;  // guards `keys`
  KeySetP keys;   // never null while the device is open
  std::mutex reg_mu;  // one registration at a time per device
  // (under reg_mu) a generation's buffers no call holds any more, kept for
  // the next registration: a 65 GB allocation clears its memory on the
  // device, which held live windows back 2.4-7.6 ms (profiles/r04_register_ab.txt)
  std::shared_ptr<KeySet> spare;
  // Generations read by kernels a device-pointer call enqueued on a caller's
  // stream and returned from (the call's own pin is gone): each held until
  // its event completes.  The registrar waits for these instead of a
  // hipDeviceSynchronize, which blocked every other thread's kernel launches
  // for its whole wait (a queue window's launch 13.2 ms, exactly the
  // registrar's sync: profiles/r06_regtrace.txt).
  std::mutex trail_mu;
  std::vector<std::pair<hipEvent_t, KeySetP>> trailing;
  std::vector<hipEvent_t> trail_events;  // completed ones, for reuse
  // (under reg_mu) page-locked staging of the committee's keys: a copy from
  // pageable memory is staged by HIP itself, synchronously
  void* kstage = nullptr;
  size_t kstage_cap = 0;
  DevShared() = default;
  DevShared(const DevShared&) = delete;
  ~DevShared();  // waits for the trailing kernels, then frees all of the above
};

// The per-call device buffers of a context: they grow on demand, and
// rebuild_context drops them all after a HIP failure.
struct CallBufs {
  DevBuf msgs, pks, sigs, kbuf, rec, verdicts, scratch, aux, rbuf, seeds, offs, data, out, idx, zs, terms, flags;
  DevBuf cert, cscr;
  DevBuf vws;  // engine-owned workspace of the device-resident verdict calls (under mu)
  DevBuf certc[4], cscrc[4];  // pipelined certificate path: up to four chunks in flight
  DevBuf msm;  // Pippenger workspace (one large verify_batch group)
  DevBuf lat;  // single-signature latency path: inputs beyond the inline ones
  std::array<DevBuf*, 30> all() {
    return {&msgs, &pks,  &sigs,  &kbuf, &rec, &verdicts, &scratch,  &aux,     &rbuf,     &seeds,   &offs, &data,
            &out,  &idx,  &zs,    &terms, &flags, &cert,   &cscr,   &certc[0], &certc[1], &certc[2], &certc[3],
            &cscrc[0], &cscrc[1], &cscrc[2], &cscrc[3], &msm, &lat, &vws};
  }
};
static_assert(sizeof(CallBufs) == 30 * sizeof(DevBuf), "CallBufs::all() lists every member, and every member is a DevBuf");

// One device context.  Its destructor drains and destroys the streams and
// frees everything the context owns (coa_shutdown, and an open that failed).
struct Dev : CallBufs {
  int id = 0;
  DevShared* sh = nullptr;
  std::unique_ptr<Worker> worker;
  hipStream_t stream = nullptr;
  hipStream_t cstreams[3] = {};  // further streams of the pipelined certificate path (created on first use)
  uint32_t* btab = nullptr;  // 128 x (j+1)B, radix-256 fixed-base table (12 KiB)
  uint32_t* comb = nullptr;  // 32 x 128 x (v+1)256^j B comb for k_verify_halved (384 KiB)
  PinBuf pinc[4];  // the staging of certc
  uint32_t* lat_res = nullptr;  // page-locked result words the latency kernels write
  size_t lat_res_cap = 0;
  uint32_t lat_tag = 0;
  uint32_t* lat_ctr = nullptr;  // device block counter of k_cert_verify_lat (0 between calls)
  PinBuf pin;
  std::mutex mu;
  Dev() = default;
  ~Dev();
};

// The wide comb is built at device open unless COA_WCOMB=0 then; COA_WCOMB=0
// at call time selects the radix-256 comb (A/B runs; read per call).
inline const uint32_t* wcomb_of(const Dev& d) { return env_is("COA_WCOMB", "0") ? nullptr : d.sh->wcomb; }

// The key tables of generation ks and context d's fixed-base combs into the
// arguments of any committee kernel; the wide combs too, except for the
// latency kernels (LatArgs and MsgLatArgs have no fields for them).
template <class A>
void key_args(A& a, const Dev& d, const KeySet& ks) {
  a.keys = ks.ckeys.as<uint32_t>();
  a.kflags = ks.kflags.as<uint32_t>();
  a.ktabs = ks.ktabs.as<uint32_t>();
  a.nk = ks.nkeys;
  a.comb = d.comb;
  if constexpr (!std::is_same_v<A, LatArgs> && !std::is_same_v<A, MsgLatArgs>) {
    a.wcomb = wcomb_of(d);
    a.kwtabs = (ks.kwide && !env_is("COA_KEY_WCOMB", "0")) ? ks.kwtabs.as<uint32_t>() : nullptr;
    a.kw20 = ks.kw20 ? 1u : 0u;
  }
}

// ---- coa_engine.cpp
// The opened contexts, in coa_init's order (fixed between init and shutdown).
extern std::vector<std::unique_ptr<Dev>>& g_devs;
int ensure_init();
int check_n(size_t n);  // "n too large for one call"
uint64_t os_entropy_seed();
uint32_t verify_lanes(size_t n);

// What a device-pointer entry does once its arguments have passed: the
// context coa_init opened on HIP device `device` (COA_EINVAL when there is
// none), that device made current, and the stream the entry enqueues on --
// the caller's, or the context's own.
int enter_device(int device, void* stream, Dev*& d, hipStream_t& s);

// The key-cache generation a call or launch on context d reads: the one this
// thread pinned (coa_keycache_use, the aggregation queue's windows) or the
// device's current one.  Holding the returned pointer keeps it alive.
KeySetP keys_now(const Dev& d);
// This thread's launches read generation `ks` for the scope's lifetime, so
// the crypto launch and the protocol launch of one device-resident verdict
// call see the same committee (a pin the aggregation queue set stays as it
// is).
struct KeyScope {
  const KeySetP* prev;
  explicit KeyScope(const KeySetP& ks);
  ~KeyScope();
};
int trail_keys(Dev& d, const KeySetP& ks, hipStream_t s);
int build_keyset(DevShared& sh, const std::vector<std::array<uint32_t, 8>>& keys, const CoaProtTable* pt = nullptr);
// build(sh) for every opened device, concurrently, each on the worker of the
// device's first context (a registration: one generation per device).
int on_each_device(const std::function<int(DevShared&)>& build);

using TaskList = std::vector<std::pair<Dev*, std::function<int()>>>;
int run_tasks(TaskList& tasks);
std::future<TaskResult> submit_task(Dev& d, std::function<int()> f);
int for_shards(size_t n, const std::function<int(Dev&, size_t, size_t)>& body, size_t work = 0);

size_t lat_max();
Dev& lat_dev(std::unique_lock<std::mutex>& lk);
int lat_res_prepare(Dev& d, size_t n, uint32_t& tag);
int lat_res_wait(Dev& d, hipStream_t s, size_t n, uint32_t tag, uint32_t* out);
int lat_verify(Dev& d, const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, size_t n, uint8_t* out,
               const uint32_t* msg_of = nullptr, size_t batch_n = 0, const uint8_t* cd_in = nullptr,
               size_t n_cd = 0);

// The workspace of a device-pointer call.  The caller's: enqueue(workspace)
// and return with the kernels still running (`trail`: the key-cache
// generation they read, held until they complete; null when they read none).
// None: the context's buffer `own` grown to `bytes` under the context's lock,
// and the call waits for its stream before the lock lets the buffer go.
template <class F>
int with_workspace(Dev& d, hipStream_t s, void* workspace, DevBuf& own, size_t bytes, const KeySetP* trail, F enqueue) {
  if (workspace) {
    const int rc = enqueue(workspace);
    return rc != COA_OK || !trail ? rc : trail_keys(d, *trail, s);
  }
  std::lock_guard<std::mutex> l(d.mu);
  HIP_TRY(own.ensure(bytes));
  const int rc = enqueue(own.p);
  if (rc != COA_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s));  // engine-owned workspace: drain before release
  return COA_OK;
}

// ---- coa_sig.cpp
// gbase: the global index of the call's first group (the z_i hash binds it).
int batch_groups_impl(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, const uint64_t* group_offsets,
                      size_t n_groups, const uint8_t* zs_in, uint64_t seed, uint8_t* verdicts_out,
                      uint32_t gbase = 0, bool prefilter = true);

}  // namespace coa_rt


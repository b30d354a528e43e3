// Entries of include/coa_verify.h over the engine core (coa_engine.h):
// Signature::verify and verify_batch, SHA-512, key generation and signing.
#include "coa_engine.h"

#include <cstring>
#include <future>

#include "coa_batch.h"
#include "coa_halved.h"
#include "coa_kernels.h"
#include "coa_msm.h"

namespace coa_rt __attribute__((visibility("hidden"))) {

// COA_VERIFY_IMPL=full selects the full-length k_verify_strict kernel (A/B
// and parity runs; read per call); the default is the halved-scalar path.
bool full_impl() { return env_is("COA_VERIFY_IMPL", "full"); }
// COA_VERIFY_WAVES=3 selects the 168-VGPR instance of k_verify_halved.
int verify_waves() { return env_is("COA_VERIFY_WAVES", "3") ? 3 : 2; }

// Workspace layout for n items: k [n][32] | rec [n][128] | scratch [lanes][2 KiB]
struct Workspace {
  uint32_t* k;
  uint32_t* rec;
  uint8_t* flags;  // split path: pre-check verdicts, two bytes (A, R) per item
  uint32_t* ebp;   // split path: [e]B per item (cached form, 128 B)
  uint32_t* scratch;
};
size_t ws_bytes(size_t n) {
  n = std::max<size_t>(n, 1);
  // scratch: per-lane slabs (single-kernel path) or per-item slabs of one
  // split chunk, whichever is larger (the path is chosen per call)
  const size_t slabs = std::max<size_t>(verify_lanes(n), std::min<size_t>(n, COA_SPLIT_CHUNK));
  return align_up(n * 32, 256) + align_up(n * COA_HALVE_REC_BYTES, 256) + align_up(2 * n, 256) + n * 128 +
         slabs * COA_HALVED_SCRATCH_PER_LANE;
}
Workspace ws_carve(void* base, size_t n) {
  n = std::max<size_t>(n, 1);
  uint8_t* p = static_cast<uint8_t*>(base);
  Workspace w;
  w.k = reinterpret_cast<uint32_t*>(p);
  p += align_up(n * 32, 256);
  w.rec = reinterpret_cast<uint32_t*>(p);
  p += align_up(n * COA_HALVE_REC_BYTES, 256);
  w.flags = p;
  p += align_up(2 * n, 256);
  w.ebp = reinterpret_cast<uint32_t*>(p);
  p += n * 128;
  w.scratch = reinterpret_cast<uint32_t*>(p);
  return w;
}

// COA_VERIFY_SPLIT=0 selects the single-kernel k_halve + k_verify_halved path
// (A/B runs; read per call); the default is the split path.
bool split_impl() { return !env_is("COA_VERIFY_SPLIT", "0"); }

// Split path in chunks of at most COA_SPLIT_CHUNK items (one slab each).
// k from d_k, or hashed in k_pre_halve from d_msgs (msg_len bytes per item)
// when d_k is null.  [e]B is summed by k_pre_halve's hash/halving role after
// the halving (that role ends early beside the two decompression roles:
// the 13 comb additions fill its idle tail instead of k_verify_main's lone
// wave); COA_SPLIT_EB=0 leaves it to k_verify_main (A/B, parity tests).
int enqueue_split(Dev& d, const uint8_t* d_msgs, size_t msg_len, const uint32_t* d_k, const uint8_t* d_pks,
                  const uint8_t* d_sigs, size_t n, uint8_t* d_verdicts, const Workspace& w, hipStream_t s) {
  for (size_t lo = 0; lo < n; lo += COA_SPLIT_CHUNK) {
    const uint32_t cnt = (uint32_t)std::min<size_t>(COA_SPLIT_CHUNK, n - lo);
    HIP_TRY(coa_launch_verify_split(d_pks + lo * 32, d_sigs + lo * 64, d_k ? nullptr : d_msgs + lo * msg_len,
                                    (uint32_t)msg_len, d_k ? d_k + lo * 8 : nullptr, cnt, w.rec + lo * 32,
                                    w.flags + 2 * lo, d_verdicts + lo, w.scratch,
                                    env_is("COA_SPLIT_EB", "0") ? nullptr : w.ebp, d.comb, wcomb_of(d), s));
  }
  return COA_OK;
}

// Verify with k already in w.k: halved path (k_halve + k_verify_halved) or
// the full-length k_verify_strict.
int enqueue_verify_prehashed(Dev& d, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n, uint8_t* d_verdicts,
                             const uint32_t* d_k, const Workspace& w, hipStream_t s) {
  const uint32_t lanes = verify_lanes(n);
  if (full_impl()) {
    HIP_TRY(coa_launch_verify_strict(d_pks, d_sigs, d_k, (uint32_t)n, d_verdicts, w.scratch, lanes, d.btab, s));
    return COA_OK;
  }
  if (split_impl()) return enqueue_split(d, nullptr, 0, d_k, d_pks, d_sigs, n, d_verdicts, w, s);
  HIP_TRY(coa_launch_halve(d_k, d_sigs, (uint32_t)n, w.rec, s));
  HIP_TRY(coa_launch_verify_halved(d_pks, d_sigs, w.rec, (uint32_t)n, d_verdicts, w.scratch, lanes, d.comb,
                                   wcomb_of(d), verify_waves(), s));
  return COA_OK;
}

// Enqueue k = H(R||A||M) then the verification for device-resident inputs.
int enqueue_verify(Dev& d, const uint8_t* d_msgs, size_t msg_len, const uint8_t* d_pks, const uint8_t* d_sigs,
                   size_t n, uint8_t* d_verdicts, const Workspace& w, hipStream_t s) {
  if (split_impl() && !full_impl() && !env_is("COA_SPLIT_HRAM", "kernel") && (d_msgs || msg_len == 0))
    return enqueue_split(d, d_msgs ? d_msgs : d_pks, msg_len, nullptr, d_pks, d_sigs, n, d_verdicts, w, s);
  HIP_TRY(coa_launch_hram(d_msgs, (uint32_t)msg_len, msg_len, nullptr, d_pks, d_sigs, (uint32_t)n, w.k, s));
  return enqueue_verify_prehashed(d, d_pks, d_sigs, n, d_verdicts, w.k, w, s);
}

// Groups of at least msm_min() signatures take the Pippenger path
// (coa_msm.hip), and so do the groups of a call with at most two; COA_MSM_MIN
// overrides (0 = never).
size_t msm_min() {
  return (size_t)env_u64("COA_MSM_MIN", 16384);  // read per call
}

// One group through the Pippenger kernels, device buffers resident.
// d_zs: caller weights (16 B per signature) or NULL = derive from seed.
int enqueue_msm(Dev& d, const uint8_t* d_msg, const uint8_t* d_pks, const uint8_t* d_sigs, size_t n,
                const uint8_t* d_zs, uint64_t seed, uint32_t group, uint8_t* d_verdict, void* ws_base,
                hipStream_t s) {
  const MsmWs ws = coa_msm_ws_carve(ws_base, n);
  HIP_TRY(coa_launch_hram(d_msg, 32, 0, nullptr, d_pks, d_sigs, (uint32_t)n, ws.k, s));
  if (d_zs) HIP_TRY(hipMemcpyAsync(ws.z, d_zs, n * 16, hipMemcpyDeviceToDevice, s));
  else HIP_TRY(coa_launch_batch_z(ws.k, d_sigs, nullptr, group, (uint32_t)n, seed, ws.z, s));
  HIP_TRY(coa_launch_msm(d_pks, d_sigs, (uint32_t)n, ws, d_verdict, s));
  return COA_OK;
}

// Host-pointer form for one group on device d (lock held by the caller).
int msm_group(Dev& d, const uint8_t* msg, const uint8_t* pks, const uint8_t* sigs, size_t n, const uint8_t* zs_in,
              uint64_t seed, uint32_t group, uint8_t* verdict_out) {
  hipStream_t s = d.stream;
  HIP_TRY(d.msgs.ensure(32));
  HIP_TRY(d.pks.ensure(n * 32 + 32));
  HIP_TRY(d.sigs.ensure(n * 64 + 64));
  HIP_TRY(d.verdicts.ensure(16));
  HIP_TRY(d.msm.ensure(coa_msm_ws_bytes(n)));
  if (zs_in) HIP_TRY(d.zs.ensure(n * 16 + 16));
  HIP_TRY(hipMemcpyAsync(d.msgs.p, msg, 32, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d.pks.p, pks, n * 32, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d.sigs.p, sigs, n * 64, hipMemcpyHostToDevice, s));
  if (zs_in) HIP_TRY(hipMemcpyAsync(d.zs.p, zs_in, n * 16, hipMemcpyHostToDevice, s));
  const int rc = enqueue_msm(d, d.msgs.as<uint8_t>(), d.pks.as<uint8_t>(), d.sigs.as<uint8_t>(), n,
                             zs_in ? d.zs.as<uint8_t>() : nullptr, seed, group, d.verdicts.as<uint8_t>(), d.msm.p, s);
  if (rc != COA_OK) return rc;
  HIP_TRY(hipMemcpyAsync(verdict_out, d.verdicts.p, 1, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return COA_OK;
}


// Large groups through the Pippenger path, dealt round-robin to the contexts
// and run concurrently on their workers; runs of small groups through the
// per-vote path (sharded over the contexts) meanwhile.
// gbase: the global index of this call's first group (the z_i hash binds it).
int batch_groups_split(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, const uint64_t* group_offsets,
                       size_t n_groups, const uint8_t* zs_in, uint64_t seed, uint8_t* verdicts_out, size_t mmin,
                       uint32_t gbase) {
  std::vector<std::vector<size_t>> large(g_devs.size());
  std::vector<std::pair<size_t, size_t>> small_runs;
  size_t nlarge = 0;
  for (size_t g = 0; g < n_groups;) {
    size_t e = g;
    while (e < n_groups && group_offsets[e + 1] - group_offsets[e] < mmin) e++;
    if (e > g) {
      small_runs.emplace_back(g, e);
      g = e;
    } else {
      large[nlarge++ % g_devs.size()].push_back(g++);
    }
  }
  TaskList tasks;
  for (size_t di = 0; di < g_devs.size(); di++) {
    if (large[di].empty()) continue;
    Dev* d = g_devs[di].get();
    const std::vector<size_t>* mine = &large[di];
    tasks.emplace_back(d, [=]() -> int {
      std::lock_guard<std::mutex> l(d->mu);
      HIP_TRY(hipSetDevice(d->id));
      for (size_t g : *mine) {
        const uint64_t v0 = group_offsets[g], nv = group_offsets[g + 1] - v0;
        const int rc = msm_group(*d, msgs + g * 32, pks + v0 * 32, sigs + v0 * 64, nv,
                                 zs_in ? zs_in + v0 * 16 : nullptr, seed, gbase + (uint32_t)g, verdicts_out + g);
        if (rc != COA_OK) return rc;
      }
      return COA_OK;
    });
  }
  // the large groups go to the workers first when there are several
  // contexts; with one context (or inside a worker) everything runs here
  bool one_ctx = g_devs.size() == 1 || in_worker();
  std::vector<std::future<TaskResult>> futs;
  if (!one_ctx)
    for (auto& t : tasks) futs.push_back(submit_task(*t.first, t.second));
  int rc = COA_OK;
  for (auto& r : small_runs) {
    const size_t g = r.first, e = r.second;
    const uint64_t v0 = group_offsets[g];
    const std::vector<uint64_t> offs = rebased_offsets(group_offsets, g, e);
    rc = batch_groups_impl(msgs + g * 32, pks + v0 * 32, sigs + v0 * 64, offs.data(), e - g,
                           zs_in ? zs_in + v0 * 16 : nullptr, seed, verdicts_out + g, gbase + (uint32_t)g, false);
    if (rc != COA_OK) break;
  }
  std::string msg = rc != COA_OK ? last_error() : std::string();
  if (one_ctx) {
    if (rc == COA_OK) rc = run_tasks(tasks);
    return rc;
  }
  for (auto& f : futs) {
    TaskResult t = f.get();
    if (t.first != COA_OK && rc == COA_OK) {
      rc = t.first;
      msg = t.second;
    }
  }
  if (rc != COA_OK) last_error() = msg;
  return rc;
}

// Calls of at most lat_max() signatures first go through the latency kernel
// as a prefilter (LatArgs::batch): a group whose votes all pass it (verify_strict
// and [l]A == O) is accepted by dalek's batch equation for every z, so its
// verdict is Ok without the batch kernels; the other groups -- some vote
// failing its own equation, a key with torsion, an encoding error -- are
// resolved exactly below, each with its own global group index (the z_i
// derivation binds it).  One launch of one workgroup per vote, the groups'
// votes side by side: ~0.2 ms for one certificate's 67 votes against ~0.4 ms
// through the Pippenger kernels.  COA_BATCH_LAT=0 disables it.
int batch_prefilter(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, const uint64_t* group_offsets,
                    size_t n_groups, uint8_t* verdicts_out, std::vector<uint8_t>& pass) {
  const size_t total = group_offsets[n_groups];
  std::vector<uint32_t> msg_of(total);
  for (size_t g = 0; g < n_groups; g++)
    for (uint64_t i = group_offsets[g]; i < group_offsets[g + 1]; i++) msg_of[i] = (uint32_t)g;
  std::vector<uint8_t> v(total);
  {
    std::unique_lock<std::mutex> l;
    Dev& d = lat_dev(l);
    HIP_TRY(hipSetDevice(d.id));
    const int rc = lat_verify(d, msgs, pks, sigs, total, v.data(), msg_of.data(), total);
    if (rc != COA_OK) return rc;
  }
  pass.assign(n_groups, 1);
  for (size_t g = 0; g < n_groups; g++) {
    for (uint64_t i = group_offsets[g]; i < group_offsets[g + 1]; i++) pass[g] &= v[i] == 0 ? 1 : 0;
    if (pass[g]) verdicts_out[g] = 0;
  }
  return COA_OK;
}

int batch_groups_impl(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs, const uint64_t* group_offsets,
                      size_t n_groups, const uint8_t* zs_in, uint64_t seed, uint8_t* verdicts_out, uint32_t gbase,
                      bool prefilter) {
  if (n_groups == 0) return COA_OK;
  if (!msgs || !group_offsets || !verdicts_out) return fail(COA_EINVAL, "null argument");
  if (group_offsets[0] != 0) return fail(COA_EINVAL, "group_offsets[0] must be 0");
  if (!offsets_monotone(group_offsets, n_groups)) return fail(COA_EINVAL, "group_offsets not monotone");
  const size_t total = group_offsets[n_groups];
  if (total && (!pks || !sigs)) return fail(COA_EINVAL, "null pks/sigs");
  if (check_n(total) != COA_OK) return COA_EINVAL;
  const uint64_t eff_seed = zs_in ? 0 : (seed ? seed : os_entropy_seed());
  if (prefilter && total > 0 && total <= lat_max() && !env_is("COA_BATCH_LAT", "0")) {
    std::vector<uint8_t> pass;
    int rc = batch_prefilter(msgs, pks, sigs, group_offsets, n_groups, verdicts_out, pass);
    if (rc != COA_OK) return rc;
    // runs of groups the prefilter did not accept, through the exact path
    for (size_t g = 0; g < n_groups;) {
      if (pass[g]) {
        g++;
        continue;
      }
      size_t e = g;
      while (e < n_groups && !pass[e]) e++;
      const uint64_t v0 = group_offsets[g];
      const std::vector<uint64_t> offs = rebased_offsets(group_offsets, g, e);
      rc = batch_groups_impl(msgs + g * 32, pks + v0 * 32, sigs + v0 * 64, offs.data(), e - g,
                             zs_in ? zs_in + v0 * 16 : nullptr, eff_seed, verdicts_out + g, gbase + (uint32_t)g, false);
      if (rc != COA_OK) return rc;
      g = e;
    }
    return COA_OK;
  }
  // One or two groups take the Pippenger path at any size: the per-vote path
  // waits for one lane's whole joint scalar multiplication (~1.4 ms however
  // few groups), the Pippenger kernels spread a group over the chip (~0.5 ms
  // at 67 votes, tools/batch_route_probe.py); from three groups one per-vote
  // launch is faster than the groups one after another.
  size_t mmin = msm_min();
  if (mmin && n_groups <= 2) mmin = 1;
  if (mmin) {
    for (size_t g = 0; g < n_groups; g++)
      if (group_offsets[g + 1] - group_offsets[g] >= mmin)
        return batch_groups_split(msgs, pks, sigs, group_offsets, n_groups, zs_in, eff_seed, verdicts_out, mmin,
                                  gbase);
  }
  // shard by group index (sized by the votes)
  return for_shards(n_groups, [&](Dev& d, size_t glo, size_t ghi) -> int {
    const size_t vlo = group_offsets[glo], vhi = group_offsets[ghi];
    const size_t nv = vhi - vlo, ng = ghi - glo;
    const std::vector<uint64_t> offs = rebased_offsets(group_offsets, glo, ghi);
    std::vector<uint32_t> group_of(std::max<size_t>(nv, 1));
    for (size_t g = 0; g < ng; g++)
      for (uint64_t i = offs[g]; i < offs[g + 1]; i++) group_of[i] = (uint32_t)(glo + g);
    const uint32_t lanes = verify_lanes(nv);
    hipStream_t s = d.stream;
    HIP_TRY(d.msgs.ensure(ng * 32));
    HIP_TRY(d.pks.ensure(nv * 32 + 32));
    HIP_TRY(d.sigs.ensure(nv * 64 + 64));
    HIP_TRY(d.kbuf.ensure(nv * 32 + 32));
    HIP_TRY(d.zs.ensure(nv * 16 + 16));
    HIP_TRY(d.idx.ensure(group_of.size() * 4));
    HIP_TRY(d.offs.ensure((ng + 1) * 8));
    HIP_TRY(d.terms.ensure(nv * 128 + 128));
    HIP_TRY(d.flags.ensure(nv + 16));
    HIP_TRY(d.scratch.ensure((size_t)lanes * COA_BATCH_SCRATCH_PER_LANE));
    HIP_TRY(d.verdicts.ensure(ng + 16));
    HIP_TRY(hipMemcpyAsync(d.msgs.p, msgs + glo * 32, ng * 32, hipMemcpyHostToDevice, s));
    if (nv) {
      HIP_TRY(hipMemcpyAsync(d.pks.p, pks + vlo * 32, nv * 32, hipMemcpyHostToDevice, s));
      HIP_TRY(hipMemcpyAsync(d.sigs.p, sigs + vlo * 64, nv * 64, hipMemcpyHostToDevice, s));
    }
    // group ids are relative to this shard's message slice
    for (auto& gid : group_of) gid -= (uint32_t)glo;
    HIP_TRY(hipMemcpyAsync(d.idx.p, group_of.data(), group_of.size() * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.offs.p, offs.data(), (ng + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(coa_launch_hram(d.msgs.as<uint8_t>(), 32, 32, d.idx.as<uint32_t>(), d.pks.as<uint8_t>(),
                            d.sigs.as<uint8_t>(), (uint32_t)nv, d.kbuf.as<uint32_t>(), s));
    if (zs_in) {
      if (nv) HIP_TRY(hipMemcpyAsync(d.zs.p, zs_in + vlo * 16, nv * 16, hipMemcpyHostToDevice, s));
    } else {
      // z derivation binds the global group index: restore it for the hash
      std::vector<uint32_t> gabs(group_of.size());
      for (size_t i = 0; i < group_of.size(); i++) gabs[i] = group_of[i] + (uint32_t)glo + gbase;
      HIP_TRY(hipMemcpyAsync(d.idx.p, gabs.data(), gabs.size() * 4, hipMemcpyHostToDevice, s));
      HIP_TRY(coa_launch_batch_z(d.kbuf.as<uint32_t>(), d.sigs.as<uint8_t>(), d.idx.as<uint32_t>(), 0, (uint32_t)nv,
                                 eff_seed, d.zs.as<uint32_t>(), s));
      HIP_TRY(hipStreamSynchronize(s));  // gabs lifetime
    }
    HIP_TRY(coa_launch_batch_terms(d.pks.as<uint8_t>(), d.sigs.as<uint8_t>(), d.kbuf.as<uint32_t>(),
                                   d.zs.as<uint32_t>(), (uint32_t)nv, d.terms.as<uint32_t>(), d.flags.as<uint8_t>(),
                                   d.scratch.as<uint32_t>(), lanes, d.btab, s));
    HIP_TRY(coa_launch_batch_reduce(d.offs.as<uint64_t>(), (uint32_t)ng, d.terms.as<uint32_t>(),
                                    d.flags.as<uint8_t>(), d.verdicts.as<uint8_t>(), s));
    HIP_TRY(hipMemcpyAsync(verdicts_out + glo, d.verdicts.p, ng, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // offs / group_of host vectors die here
    return COA_OK;
  }, group_offsets[n_groups]);
}

int sign_enqueue(Dev& d, const uint8_t* d_seeds, const uint8_t* d_msgs, size_t msg_len, size_t n, uint8_t* d_pks,
                 uint8_t* d_sigs, hipStream_t s) {
  HIP_TRY(d.aux.ensure(n * 64 + 64));
  HIP_TRY(d.rbuf.ensure(n * 32 + 32));
  HIP_TRY(d.kbuf.ensure(n * 32 + 32));
  HIP_TRY(coa_launch_keygen(d_seeds, (uint32_t)n, d_pks, d.aux.as<uint32_t>(), d.btab, s));
  HIP_TRY(coa_launch_sign_r(d.aux.as<uint32_t>(), d_msgs, (uint32_t)msg_len, (uint32_t)n, d_sigs,
                            d.rbuf.as<uint32_t>(), d.btab, s));
  HIP_TRY(coa_launch_hram(d_msgs, (uint32_t)msg_len, msg_len, nullptr, d_pks, d_sigs, (uint32_t)n,
                          d.kbuf.as<uint32_t>(), s));
  HIP_TRY(coa_launch_sign_s(d.aux.as<uint32_t>(), d.rbuf.as<uint32_t>(), d.kbuf.as<uint32_t>(), (uint32_t)n, d_sigs,
                            s));
  return COA_OK;
}

}  // namespace coa_rt

using namespace coa_rt;

extern "C" {

size_t coa_verify_workspace_bytes(size_t n) { return ws_bytes(n); }

int coa_ed25519_verify_strict_many(const uint8_t* msgs, size_t msg_len, const uint8_t* pks, const uint8_t* sigs,
                                   size_t n, uint8_t* verdicts_out) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if ((!msgs && msg_len) || !pks || !sigs || !verdicts_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  if (msg_len == 32 && n <= lat_max()) {  // few signatures: the latency kernel on an idle context
    std::unique_lock<std::mutex> l;
    Dev& d = lat_dev(l);
    HIP_TRY(hipSetDevice(d.id));
    return lat_verify(d, msgs, pks, sigs, n, verdicts_out);
  }
  return for_shards(n, [&](Dev& d, size_t lo, size_t hi) -> int {
    const size_t cnt = hi - lo;
    hipStream_t s = d.stream;
    HIP_TRY(d.msgs.ensure(cnt * msg_len + 4));
    HIP_TRY(d.pks.ensure(cnt * 32));
    HIP_TRY(d.sigs.ensure(cnt * 64));
    HIP_TRY(d.scratch.ensure(ws_bytes(cnt)));
    HIP_TRY(d.verdicts.ensure(cnt));
    if (msg_len) HIP_TRY(hipMemcpyAsync(d.msgs.p, msgs + lo * msg_len, cnt * msg_len, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.pks.p, pks + lo * 32, cnt * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.sigs.p, sigs + lo * 64, cnt * 64, hipMemcpyHostToDevice, s));
    int r = enqueue_verify(d, d.msgs.as<uint8_t>(), msg_len, d.pks.as<uint8_t>(), d.sigs.as<uint8_t>(), cnt,
                           d.verdicts.as<uint8_t>(), ws_carve(d.scratch.p, cnt), s);
    if (r != COA_OK) return r;
    HIP_TRY(hipMemcpyAsync(verdicts_out + lo, d.verdicts.p, cnt, hipMemcpyDeviceToHost, s));
    return COA_OK;
  });
}

int coa_ed25519_verify_strict(const uint8_t msg[32], const uint8_t pk[32], const uint8_t sig[64]) {
  uint8_t v = 1;
  const int rc = coa_ed25519_verify_strict_many(msg, 32, pk, sig, 1, &v);
  if (rc != COA_OK) return rc;
  return v ? COA_REJECT : COA_OK;
}

int coa_ed25519_verify_strict_many_device(int device, const uint8_t* d_msgs, size_t msg_len, const uint8_t* d_pks,
                                          const uint8_t* d_sigs, size_t n, uint8_t* d_verdicts, void* workspace,
                                          void* stream) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if ((!d_msgs && msg_len) || !d_pks || !d_sigs || !d_verdicts) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  return with_workspace(*d, s, workspace, d->scratch, ws_bytes(n), nullptr, [&](void* ws) {
    return enqueue_verify(*d, d_msgs, msg_len, d_pks, d_sigs, n, d_verdicts, ws_carve(ws, n), s);
  });
}

int coa_ed25519_challenge_many_device(int device, const uint8_t* d_msgs, size_t msg_len, const uint8_t* d_pks,
                                      const uint8_t* d_sigs, size_t n, uint8_t* d_k_out, void* stream) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if ((!d_msgs && msg_len) || !d_pks || !d_sigs || !d_k_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  HIP_TRY(coa_launch_hram(d_msgs, (uint32_t)msg_len, msg_len, nullptr, d_pks, d_sigs, (uint32_t)n,
                          reinterpret_cast<uint32_t*>(d_k_out), s));
  return COA_OK;
}

int coa_ed25519_verify_prehashed_many_device(int device, const uint8_t* d_k, const uint8_t* d_pks,
                                             const uint8_t* d_sigs, size_t n, uint8_t* d_verdicts, void* workspace,
                                             void* stream) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!d_k || !d_pks || !d_sigs || !d_verdicts) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  const uint32_t* k = reinterpret_cast<const uint32_t*>(d_k);
  return with_workspace(*d, s, workspace, d->scratch, ws_bytes(n), nullptr, [&](void* ws) {
    return enqueue_verify_prehashed(*d, d_pks, d_sigs, n, d_verdicts, k, ws_carve(ws, n), s);
  });
}

int coa_ed25519_verify_batch_groups(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs,
                                    const uint64_t* group_offsets, size_t n_groups, uint8_t* group_verdicts_out,
                                    uint64_t rng_seed) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  return batch_groups_impl(msgs, pks, sigs, group_offsets, n_groups, nullptr, rng_seed, group_verdicts_out);
}

int coa_ed25519_verify_batch_groups_z(const uint8_t* msgs, const uint8_t* pks, const uint8_t* sigs,
                                      const uint64_t* group_offsets, size_t n_groups, const uint8_t* zs,
                                      uint8_t* group_verdicts_out) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!zs && n_groups && group_offsets && group_offsets[n_groups]) return fail(COA_EINVAL, "null zs");
  static const uint8_t zero16[16] = {0};
  return batch_groups_impl(msgs, pks, sigs, group_offsets, n_groups, zs ? zs : zero16, 0, group_verdicts_out);
}

size_t coa_verify_batch_workspace_bytes(size_t n) { return coa_msm_ws_bytes(n); }

int coa_ed25519_verify_batch_device(int device, const uint8_t* d_msg, const uint8_t* d_pks, const uint8_t* d_sigs,
                                    size_t n, const uint8_t* d_zs, uint64_t rng_seed, uint8_t* d_verdict,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!d_msg || !d_verdict || (n && (!d_pks || !d_sigs))) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  if (n == 0) {  // empty batch: the equation is [0]B = O, Ok (as dalek)
    HIP_TRY(hipMemsetAsync(d_verdict, 0, 1, s));
    return COA_OK;
  }
  const uint64_t seed = d_zs ? 0 : (rng_seed ? rng_seed : os_entropy_seed());
  // the chunk count (and so the layout) depends on the bucket run length of
  // this call: refuse a buffer sized for another one
  if (workspace && workspace_bytes < coa_msm_ws_bytes(n))
    return fail(COA_EINVAL, "workspace smaller than coa_verify_batch_workspace_bytes(n)");
  return with_workspace(*d, s, workspace, d->msm, coa_msm_ws_bytes(n), nullptr, [&](void* ws) {
    return enqueue_msm(*d, d_msg, d_pks, d_sigs, n, d_zs, seed, 0, d_verdict, ws, s);
  });
}

int coa_ed25519_verify_batch(const uint8_t msg[32], const uint8_t* pks, const uint8_t* sigs, size_t n,
                             uint64_t rng_seed) {
  const uint64_t offs[2] = {0, (uint64_t)n};
  uint8_t v = 1;
  const int rc = coa_ed25519_verify_batch_groups(msg, pks, sigs, offs, 1, &v, rng_seed);
  if (rc != COA_OK) return rc;
  return v ? COA_REJECT : COA_OK;
}

int coa_sha512_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out64) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!offsets || !out64) return fail(COA_EINVAL, "null argument");
  if (!offsets_monotone(offsets, n)) return fail(COA_EINVAL, "offsets not monotone");
  if (offsets[n] > offsets[0] && !data) return fail(COA_EINVAL, "null data");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return for_shards(n, [&](Dev& d, size_t lo, size_t hi) -> int {
    const size_t cnt = hi - lo;
    const uint64_t base = offsets[lo], bytes = offsets[hi] - base;
    const std::vector<uint64_t> rel = rebased_offsets(offsets, lo, hi);
    hipStream_t s = d.stream;
    HIP_TRY(d.data.ensure(bytes + 16));
    HIP_TRY(d.offs.ensure((cnt + 1) * 8));
    HIP_TRY(d.out.ensure(cnt * 64));
    if (bytes) HIP_TRY(hipMemcpyAsync(d.data.p, data + base, bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d.offs.p, rel.data(), (cnt + 1) * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(coa_launch_sha512_many(d.data.as<uint8_t>(), d.offs.as<uint64_t>(), (uint32_t)cnt,
                                   d.out.as<uint32_t>(), s));
    HIP_TRY(hipMemcpyAsync(out64 + lo * 64, d.out.p, cnt * 64, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // rel dies here
    return COA_OK;
  });
}

int coa_sha512_trunc32_many(const uint8_t* data, const uint64_t* offsets, size_t n, uint8_t* out32) {
  if (n == 0) return ensure_init();
  if (!out32) return fail(COA_EINVAL, "null argument");
  std::vector<uint8_t> full(n * 64);
  const int rc = coa_sha512_many(data, offsets, n, full.data());
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < n; i++) std::memcpy(out32 + i * 32, full.data() + i * 64, 32);
  return COA_OK;
}

int coa_sha512_many_device(int device, const uint8_t* d_data, const uint64_t* d_offsets, size_t n, uint8_t* d_out64,
                           void* stream) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!d_data || !d_offsets || !d_out64) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  HIP_TRY(coa_launch_sha512_many(d_data, d_offsets, (uint32_t)n, reinterpret_cast<uint32_t*>(d_out64), s));
  return COA_OK;
}

int coa_ed25519_sign_many(const uint8_t* seeds, const uint8_t* msgs, size_t msg_len, size_t n, uint8_t* pks_out,
                          uint8_t* sigs_out) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!seeds || (!msgs && msg_len) || !pks_out || !sigs_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return for_shards(n, [&](Dev& d, size_t lo, size_t hi) -> int {
    const size_t cnt = hi - lo;
    hipStream_t s = d.stream;
    HIP_TRY(d.seeds.ensure(cnt * 32));
    HIP_TRY(d.msgs.ensure(cnt * msg_len + 4));
    HIP_TRY(d.pks.ensure(cnt * 32));
    HIP_TRY(d.sigs.ensure(cnt * 64));
    HIP_TRY(hipMemcpyAsync(d.seeds.p, seeds + lo * 32, cnt * 32, hipMemcpyHostToDevice, s));
    if (msg_len) HIP_TRY(hipMemcpyAsync(d.msgs.p, msgs + lo * msg_len, cnt * msg_len, hipMemcpyHostToDevice, s));
    int r = sign_enqueue(d, d.seeds.as<uint8_t>(), d.msgs.as<uint8_t>(), msg_len, cnt, d.pks.as<uint8_t>(),
                         d.sigs.as<uint8_t>(), s);
    if (r != COA_OK) return r;
    HIP_TRY(hipMemcpyAsync(pks_out + lo * 32, d.pks.p, cnt * 32, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(sigs_out + lo * 64, d.sigs.p, cnt * 64, hipMemcpyDeviceToHost, s));
    return COA_OK;
  });
}

int coa_ed25519_public_keys(const uint8_t* seeds, size_t n, uint8_t* pks_out) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!seeds || !pks_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return for_shards(n, [&](Dev& d, size_t lo, size_t hi) -> int {
    const size_t cnt = hi - lo;
    hipStream_t s = d.stream;
    HIP_TRY(d.seeds.ensure(cnt * 32));
    HIP_TRY(d.pks.ensure(cnt * 32));
    HIP_TRY(d.aux.ensure(cnt * 64));
    HIP_TRY(hipMemcpyAsync(d.seeds.p, seeds + lo * 32, cnt * 32, hipMemcpyHostToDevice, s));
    HIP_TRY(coa_launch_keygen(d.seeds.as<uint8_t>(), (uint32_t)cnt, d.pks.as<uint8_t>(), d.aux.as<uint32_t>(),
                              d.btab, s));
    HIP_TRY(hipMemcpyAsync(pks_out + lo * 32, d.pks.p, cnt * 32, hipMemcpyDeviceToHost, s));
    return COA_OK;
  });
}

int coa_ed25519_sign_many_device(int device, const uint8_t* d_seeds, const uint8_t* d_msgs, size_t msg_len, size_t n,
                                 uint8_t* d_pks_out, uint8_t* d_sigs_out, void* stream) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!d_seeds || (!d_msgs && msg_len) || !d_pks_out || !d_sigs_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  std::lock_guard<std::mutex> l(d->mu);
  rc = sign_enqueue(*d, d_seeds, d_msgs, msg_len, n, d_pks_out, d_sigs_out, s);
  if (rc != COA_OK) return rc;
  HIP_TRY(hipStreamSynchronize(s));
  return COA_OK;
}

int coa_lat_verify_device(int device, const uint8_t* d_in, size_t n, uint32_t* d_res, void* stream) {
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!d_in || !d_res) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  LatArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = (uint32_t)n;
  a.n_inline = 0;
  a.in = reinterpret_cast<const uint32_t*>(d_in);
  a.res = d_res;
  a.tag = 1;
  // the pinned generation (the queue) or the current one: a registration
  // frees a replaced generation only after the device has drained
  const KeySetP ks = keys_now(*d);
  key_args(a, *d, *ks);
  HIP_TRY(coa_launch_verify_lat(a, s));
  return trail_keys(*d, ks, s);
}

int coa_lat_verify_inline(int device, const uint8_t* h_records, size_t n, uint32_t* res, uint32_t tag, void* stream) {
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!h_records || !res || tag == 0) return fail(COA_EINVAL, "null argument or zero tag");
  if (n > COA_LAT_INLINE) return fail(COA_EINVAL, "more records than the kernel arguments hold");
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  LatArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = a.n_inline = (uint32_t)n;
  std::memcpy(a.inl, h_records, n * 128);  // msg | pk | R | s, as the device records
  a.res = res;
  a.tag = tag;
  const KeySetP ks = keys_now(*d);  // pinned (the queue) or current; see coa_lat_verify_device
  key_args(a, *d, *ks);
  HIP_TRY(coa_launch_verify_lat(a, s));
  return trail_keys(*d, ks, s);
}

}  // extern "C"

// Protocol checks of Certificate::verify / Header::verify / Vote::verify on
// the device (primary/src/messages.rs:48-67,131-142,189-215): everything the
// reference checks beside the crypto -- genesis, the author's stake, the
// header's worker ids, voter reuse, voter stake and the quorum -- from the
// committee's protocol table (stakes and worker ids in the key cache's sorted
// key order, coa_committee_register_authorities), and the merge of that
// answer with the crypto kernels' status word into one COA_DAG_* verdict.
//
//   k_cert_protocol   one certificate per wavefront, 64-lane strides over
//                     its votes
//   k_msg_protocol    one header or vote per lane
//   k_verdict_merge   one item per lane
//   k_window_verdict  a queue window's certificates, headers and votes in one
//                     launch: the two bodies above, each followed by the merge
//
// The kernels read the same arrays as k_cert_verify / k_msg_verify and are
// independent of them; only the merge needs both answers.
#include "coa_protocol_dev.h"

#include "coa_keycache.h"
#include "coa_prot_scan.h"
#include "coa_protocol.h"

namespace {

using coa_kc::key_lookup;
using coa_kc::load8;
using coa_prot::has_worker;
using coa_prot::worker_id_at;

constexpr int kWaves = 4;  // certificates per 256-thread block

COA_DEV uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, 64));
  return v;
}

COA_DEV uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

// One certificate per wavefront.  Reuse (messages.rs:202) is found through
// first[slot], the lowest vote index that named committee slot `slot`, kept
// in the wave's own slice of LDS: the strides run in vote order, every lane of
// a stride enters its index with atomicMin before any lane reads, so vote j is
// a reuse iff first[slot] < j.  A key outside the committee has no slot and
// fails the stake test at its first occurrence, so slots suffice.  Called by
// a whole wavefront with its slice `first` of LDS; every lane returns the
// certificate's protocol word.
COA_DEV uint32_t cert_proto_word(const CertProtArgs& a, const ProtTab& t, uint32_t c, uint32_t lane, uint32_t* first) {
  const uint32_t nk = min(t.nk, (uint32_t)COA_MAX_AUTHORITIES);
  for (uint32_t s = lane; s < nk; s += 64) first[s] = 0xffffffffu;

  // header part, the same on every lane: author slot, genesis, stake
  uint32_t id[8], origin[8];
  load8(id, a.ids + (uint64_t)c * 8);
  load8(origin, a.origins + (uint64_t)c * 8);
  const int aslot = key_lookup<coa_kc::kLane>(t.keys, nk, origin);
  uint32_t id_or = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) id_or |= id[i];
  const bool genesis = id_or == 0 && a.rounds[c] == 0 && aslot >= 0;
  const uint32_t astake = aslot >= 0 ? t.stake[aslot] : 0u;
  // worker ids of the payload, spread over the lanes
  bool malformed = false;
  if (astake) {
    const uint64_t h0 = a.hdr_off[c], hlen = a.hdr_off[c + 1] - h0;
    const uint32_t pc = a.pcounts[c];
    if (pc && 40 + 36 * (uint64_t)pc > hlen) {
      malformed = true;  // the count overruns the header: nothing is read
    } else {
      const uint32_t wlo = t.woff[aslot], whi = t.woff[aslot + 1];
      for (uint32_t k = lane; k < pc; k += 64)
        malformed = malformed || !has_worker(t.wids, wlo, whi, worker_id_at(a.hdr_data + h0, k));
    }
  }
  malformed = __any(malformed);

  // the vote loop (:201-207)
  const uint64_t v0 = a.voff[c], nv = a.voff[c + 1] - v0;
  uint32_t fail = 0xffffffffu;  // (vote index << 8) | code of this lane's first failing vote
  uint64_t weight = 0;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // the reset before the first atomicMin
  for (uint64_t base = 0; base < nv; base += 64) {
    const uint64_t j = base + lane;
    const bool live = j < nv && v0 + j < a.nv;
    int slot = -1;
    if (live) {
      uint32_t pk[8];
      load8(pk, a.vpks + (v0 + j) * 8);
      slot = key_lookup<coa_kc::kLane>(t.keys, nk, pk);
      if (slot >= 0) atomicMin(&first[slot], (uint32_t)min(j, (uint64_t)0xfffffffeu));
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    if (live) {
      const uint32_t idx = (uint32_t)min(j, (uint64_t)COA_PROTO_MAX_INDEX) << 8;
      const uint32_t st = slot >= 0 ? t.stake[slot] : 0u;
      uint32_t f = 0xffffffffu;
      if (slot >= 0 && first[slot] < j) f = idx | COA_DAG_AUTHORITY_REUSE;
      else if (st == 0) f = idx | COA_DAG_UNKNOWN_VOTER;
      fail = min(fail, f);
      weight += st;
    }
  }
  fail = wave_min(fail);
  weight = wave_sum(weight);
  uint32_t w = 0;
  if (genesis) w = COA_PROTO_GENESIS;                           // :190-193
  else if (astake == 0) w = COA_DAG_UNKNOWN_AUTHOR;             // :53-54
  else if (malformed) w = COA_DAG_MALFORMED_HEADER;             // :57-61
  else if (fail != 0xffffffffu) w = fail;                       // :202-204
  else if (weight < t.quorum) w = COA_DAG_REQUIRES_QUORUM;      // :208-211
  return w;
}

__global__ void __launch_bounds__(64 * kWaves) k_cert_protocol(const CertProtArgs a, const ProtTab t) {
  __shared__ uint32_t first_all[kWaves][COA_MAX_AUTHORITIES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t c = blockIdx.x * kWaves + wave;
  if (c >= a.nc) return;  // whole waves leave; no block-wide barrier below
  const uint32_t w = cert_proto_word(a, t, c, lane, first_all[wave]);
  if (lane == 0) a.proto[c] = w;
}

// One header (hdr_data set) or vote per lane: the author's stake (:53-54,
// :133-136) and, for headers, the worker ids (:57-61).
COA_DEV uint32_t msg_proto_word(const MsgProtArgs& a, const ProtTab& t, uint32_t i) {
  uint32_t author[8];
  load8(author, a.authors + (uint64_t)i * 8);
  const int slot = key_lookup<coa_kc::kLane>(t.keys, t.nk, author);
  uint32_t w = 0;
  if (slot < 0 || t.stake[slot] == 0) {
    w = COA_DAG_UNKNOWN_AUTHOR;
  } else if (a.hdr_data) {
    const uint64_t h0 = a.hdr_off[i], hlen = a.hdr_off[i + 1] - h0;
    const uint32_t pc = a.pcounts[i];
    if (pc && 40 + 36 * (uint64_t)pc > hlen) {
      w = COA_DAG_MALFORMED_HEADER;
    } else {
      const uint32_t wlo = t.woff[slot], whi = t.woff[slot + 1];
      for (uint32_t k = 0; k < pc && !w; k++)
        if (!has_worker(t.wids, wlo, whi, worker_id_at(a.hdr_data + h0, k))) w = COA_DAG_MALFORMED_HEADER;
    }
  }
  return w;
}

__global__ void __launch_bounds__(256) k_msg_protocol(const MsgProtArgs a, const ProtTab t) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  a.proto[i] = msg_proto_word(a, t, i);
}

__global__ void __launch_bounds__(256) k_verdict_merge(const uint32_t* __restrict__ raw,
                                                       const uint32_t* __restrict__ proto,
                                                       uint32_t* __restrict__ verdicts, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) verdicts[i] = coa_verdict_merge(raw[i], proto[i]);
}

// The whole verdict of an aggregation-queue window in one launch, over the
// window's staged arrays and the raw status words its crypto launches wrote
// earlier on the stream.  The leading cert_blocks blocks take one certificate
// per wavefront (cert_proto_word); the blocks after them one header or vote
// per lane (msg_proto_word), the headers first.  Each item's protocol word is
// merged with its raw word at once: word c of a.words belongs to certificate
// c, word nc + i to header i, word nc + nh + j to vote j.
// The message-role blocks carry the certificate role's 16 KB of LDS unused:
// a CU runs at most 32 waves, eight such blocks, whose 128 KB fit its 160 KB,
// so the table does not bound their occupancy.
__global__ void __launch_bounds__(64 * kWaves) k_window_verdict(const WindowVerdictArgs a, const ProtTab t) {
  __shared__ uint32_t first_all[kWaves][COA_MAX_AUTHORITIES];
  if (blockIdx.x < a.cert_blocks) {
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t c = blockIdx.x * kWaves + wave;
    if (c >= a.cert.nc) return;  // whole waves leave; no block-wide barrier below
    const uint32_t w = cert_proto_word(a.cert, t, c, lane, first_all[wave]);
    if (lane == 0) a.words[c] = coa_verdict_merge(a.cert_raw[c], w);
    return;
  }
  const uint32_t i = (blockIdx.x - a.cert_blocks) * blockDim.x + threadIdx.x;
  const uint32_t nh = a.hdr.n, nv = a.vote.n;
  if (i >= nh + nv) return;
  const uint32_t w = i < nh ? msg_proto_word(a.hdr, t, i) : msg_proto_word(a.vote, t, i - nh);
  a.words[a.cert.nc + i] = coa_verdict_merge(a.msg_raw[i], w);
}

}  // namespace

hipError_t coa_launch_cert_protocol(const CertProtArgs& a, const ProtTab& t, hipStream_t s) {
  if (a.nc == 0) return hipSuccess;
  hipLaunchKernelGGL(k_cert_protocol, dim3((a.nc + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a, t);
  return hipGetLastError();
}

hipError_t coa_launch_msg_protocol(const MsgProtArgs& a, const ProtTab& t, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_msg_protocol, dim3((a.n + 255) / 256), dim3(256), 0, s, a, t);
  return hipGetLastError();
}

hipError_t coa_launch_verdict_merge(const uint32_t* raw, const uint32_t* proto, uint32_t* verdicts, uint32_t n,
                                    hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_verdict_merge, dim3((n + 255) / 256), dim3(256), 0, s, raw, proto, verdicts, n);
  return hipGetLastError();
}

hipError_t coa_launch_window_verdict(WindowVerdictArgs a, const ProtTab& t, hipStream_t s) {
  const uint32_t msgs = a.hdr.n + a.vote.n;
  a.cert_blocks = (a.cert.nc + kWaves - 1) / kWaves;
  const uint32_t blocks = a.cert_blocks + (msgs + 64 * kWaves - 1) / (64 * kWaves);
  if (blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(k_window_verdict, dim3(blocks), dim3(64 * kWaves), 0, s, a, t);
  return hipGetLastError();
}

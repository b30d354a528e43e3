// The device-resident wire decoder (include/coa_verify.h, "wire decode on the
// device"): bincode PrimaryMessage frames in device memory into the arrays of
// the *_many_device calls, bit-identical to csrc/coa_wire.cpp.  Every rule of
// the format -- which bytes are read, in which order errors count, how keys
// compare -- is coa_wire_parse.h; this file holds the work split only.
//
//   k_wire_scan     one wavefront per frame: kind or error, digest-input
//                   length, votes
//   k_wire_block_totals / k_wire_scan_totals / k_wire_add
//                   exclusive prefix sums of header bytes and votes over the
//                   frames of the call's kind, as three launches: no kernel
//                   waits for another workgroup
//   k_wire_decode   one wavefront per frame: the fields into the output arrays
//   k_wire_decode_mixed / k_wire_scatter
//                   the mixed mode: the sums run over six quantities (every
//                   kind's frames, header bytes and votes), a frame's fields
//                   go to its slot in its kind's arrays, and the verdict
//                   words come back to frame order
//
// A frame of up to kStage bytes is copied into LDS first (dword loads between
// the unaligned ends) and every rule then reads LDS; a longer frame is read
// where it lies.  The field walk up to a certificate's vote list is short and
// sequential, so every lane runs it on the same addresses; the lanes split
// the votes (speculating on the canonical stride, coa_wp_vote_canonical) and
// the set entries (coa_wp_is_last, coa_wp_rank).
#include <hip/hip_runtime.h>

#include "coa_wire_dev.h"
#include "coa_wire_parse.h"

namespace {

constexpr uint32_t kWaves = 4;       // frames per block
constexpr uint32_t kMixedWaves = 1;  // frames per block of k_wire_decode_mixed: neighbours differ in kind and length, and a block's LDS is held for its longest frame
constexpr uint32_t kStage = 12288;   // LDS bytes per frame: a 67-vote, 67-parent, 32-payload certificate is 11.3 KB

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    const uint64_t t = __shfl_xor((unsigned long long)v, o);
    v = t < v ? t : v;
  }
  return v;
}

// The frame g[0, len), len <= kStage, copied into LDS at `stage` (kStage + 4
// bytes): the copy starts at the frame's own alignment, so the middle moves as
// dwords.  Returns the copy.
__device__ __forceinline__ const uint8_t* stage_frame(const uint8_t* g, uint32_t len, uint32_t lane, uint8_t* stage) {
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 3);
  uint8_t* l = stage + mis;
  const uint32_t head = min(len, (4 - mis) & 3);
  const uint32_t words = (len - head) / 4;
  const uint32_t tail = head + words * 4;
  if (lane < head) l[lane] = g[lane];
  const uint32_t* gw = reinterpret_cast<const uint32_t*>(g + head);
  uint32_t* lw = reinterpret_cast<uint32_t*>(l + head);
  for (uint32_t w = lane; w < words; w += 64) lw[w] = gw[w];
  if (tail + lane < len) l[tail + lane] = g[tail + lane];  // at most 3 bytes
  wave_sync();
  return l;
}

// A certificate's vote list: COA_OK or the first error in wire order; the
// decoded keys and signatures go to pks / sigs when those are not null.
__device__ __forceinline__ int votes_do(const uint8_t* p, size_t n, const CoaWpFrame& f, uint32_t lane, uint8_t* pks, uint8_t* sigs) {
  bool canon = true;
  for (uint64_t b = 0; b < f.nv; b += 64)
    if (b + lane < f.nv && !coa_wp_vote_canonical(p, n, f.votes, b + lane)) canon = false;
  if (!__all(canon))  // some key string is not 44 long: the walk, the same on every lane; lane 0 writes
    return coa_wp_votes(p, n, f.votes, f.nv, lane == 0 ? pks : nullptr, lane == 0 ? sigs : nullptr);
  uint64_t first = COA_WP_NO_ERROR;
  for (uint64_t b = 0; b < f.nv; b += 64) {
    const uint64_t k = b + lane;
    if (k < f.nv) {
      size_t pos = f.votes + (size_t)k * COA_WP_VOTE_STRIDE;
      const int rc = coa_wp_vote(p, n, &pos, pks ? pks + k * 32 : nullptr, nullptr);
      const uint64_t w = coa_wp_error_word(k, rc);
      first = w < first ? w : first;
    }
  }
  const int rc = coa_wp_error_code(wave_min(first));
  if (sigs && rc == COA_OK)  // every vote is whole: the signatures as consecutive dwords over the lanes
    for (uint64_t w = lane; w < f.nv * 16; w += 64)
      coa_wp_put32(sigs + w * 4, coa_wp_u32(p + coa_wp_canonical_sig_word(f.votes, w)));
  return rc;
}

// last[i] for the n entries of a set, split over the lanes; the number of
// survivors.
__device__ __forceinline__ uint32_t set_last(const uint8_t* base, size_t stride, uint32_t n, uint32_t lane, uint8_t* last) {
  uint32_t c = 0;
  for (uint32_t i = lane; i < n; i += 64) {
    const bool l = coa_wp_is_last(base, stride, n, i);
    last[i] = l;
    c += l;
  }
  wave_sync();
  return wave_sum(c);
}

// The survivors of a set into key order at out (stride bytes each).
__device__ __forceinline__ void set_emit(const uint8_t* base, size_t stride, uint32_t n, uint32_t lane, const uint8_t* last,
                         uint8_t* out) {
  for (uint32_t i = lane; i < n; i += 64)
    if (last[i]) coa_wp_copy(out + (size_t)coa_wp_rank(base, stride, n, i, last) * stride, base + (size_t)i * stride, stride);
  wave_sync();  // `last` is reused for the next set
}

// One frame's kind, digest-input length and votes.  p is the frame in LDS or in
// place: the body is compiled once for each (an LDS read does not queue behind
// the global stores the decode issues, a flat one would).
__device__ __forceinline__ void scan_frame(const uint8_t* p, size_t len, uint32_t lane, uint8_t* last, int32_t& kind,
                                           uint64_t& hb, uint64_t& nv) {
  CoaWpFrame f;
  kind = coa_wp_walk(p, len, &f);
  if (kind == COA_MSG_CERTIFICATE) {
    const int rc = votes_do(p, len, f, lane, nullptr, nullptr);
    if (rc != COA_OK) kind = rc;
  }
  kind = coa_wp_capacity(kind, f.np, f.nq);
  if (kind == COA_MSG_HEADER || kind == COA_MSG_CERTIFICATE) {
    const uint32_t P = set_last(p + f.payload, 36, (uint32_t)f.np, lane, last);
    const uint32_t Q = set_last(p + f.parents, 32, (uint32_t)f.nq, lane, last);
    hb = coa_wp_digest_len(P, Q);
    nv = f.nv;
  }
}

__global__ void __launch_bounds__(64 * kWaves) k_wire_scan(const WireHead a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][kStage + 16];
  __shared__ uint8_t last[kWaves][COA_WIRE_DEV_MAX_ENTRIES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * kWaves + wave;
  if (i >= a.n) return;  // whole waves leave; no block-wide barrier below
  int32_t kind = COA_WIRE_ETRUNC;
  uint64_t hb = 0, nv = 0;
  const uint64_t o0 = a.offs[i], o1 = a.offs[i + 1];
  if (coa_wp_frame_range(o0, o1, a.frame_bytes)) {  // else nothing of the frame is read
    const size_t len = (size_t)(o1 - o0);
    if (len <= kStage)
      scan_frame(stage_frame(a.frames + o0, (uint32_t)len, lane, stage[wave]), len, lane, last[wave], kind, hb, nv);
    else
      scan_frame(a.frames + o0, len, lane, last[wave], kind, hb, nv);
  }
  if (lane == 0) {
    a.kinds[i] = kind;
    a.hb[i] = hb;
    a.nv[i] = nv;
  }
}

// What the prefix sums run over.  One kind (the index-aligned decoders): three
// quantities of the frames of a.want.
struct SumsOne {
  static constexpr int Q = 3;
  using Args = WireArgs;
  // What frame i adds to the call's sums: header bytes, votes, one frame.
  static __device__ __forceinline__ void contribution(const WireArgs& a, uint32_t i, uint64_t v[3]) {
    const bool mine = i < a.n && a.kinds[i] == a.want;
    v[0] = mine && a.want != COA_MSG_VOTE ? a.hb[i] : 0;
    v[1] = mine && a.want == COA_MSG_CERTIFICATE ? a.nv[i] : 0;
    v[2] = mine ? 1 : 0;
  }
  static __device__ __forceinline__ void totals(const WireArgs& a, const uint64_t total[3]) {
    if (!a.totals) return;
    a.totals[0] = total[0];
    a.totals[1] = total[1];
    a.totals[2] = total[2];
    a.totals[3] = a.n - total[2];
  }
  // Frame i's place: its exclusive sums `at`, its own contribution v.
  static __device__ __forceinline__ void place(const WireArgs& a, uint32_t i, const uint64_t at[3], const uint64_t v[3]) {
    if (a.out.hoff) {
      a.out.hoff[i] = at[0];
      if (i == a.n - 1) a.out.hoff[a.n] = at[0] + v[0];
    }
    if (a.out.voff) {
      a.out.voff[i] = at[1];
      if (i == a.n - 1) a.out.voff[a.n] = at[1] + v[1];
    }
  }
};

// Every kind at once (the mixed mode): headers and their bytes | votes |
// certificates, their bytes and their votes -- the first six words of the
// call's totals.
struct SumsMixed {
  static constexpr int Q = COA_WIRE_MIXED_SUMS;
  using Args = WireMixedArgs;
  static __device__ __forceinline__ void contribution(const WireMixedArgs& a, uint32_t i, uint64_t v[6]) {
    const int32_t kind = i < a.n ? a.kinds[i] : -1;
    const bool h = kind == COA_MSG_HEADER, c = kind == COA_MSG_CERTIFICATE;
    v[0] = h;
    v[1] = h ? a.hb[i] : 0;
    v[2] = kind == COA_MSG_VOTE;
    v[3] = c;
    v[4] = c ? a.hb[i] : 0;
    v[5] = c ? a.nv[i] : 0;
  }
  // The totals, and each kind's offsets at its count: the offsets are defined
  // on [0, count], also where the count is 0.
  static __device__ __forceinline__ void totals(const WireMixedArgs& a, const uint64_t total[6]) {
    for (int q = 0; q < 6; q++) a.totals[q] = total[q];
    a.totals[6] = a.n - (total[0] + total[2] + total[3]);
    a.totals[7] = 0;
    a.set[COA_MSG_HEADER].hoff[total[0]] = total[1];
    a.set[COA_MSG_CERTIFICATE].hoff[total[3]] = total[4];
    a.set[COA_MSG_CERTIFICATE].voff[total[3]] = total[5];
  }
  // The slot: the frame's rank among the frames of its kind (the partition
  // is stable); a header's and a certificate's offsets at their slot.
  static __device__ __forceinline__ void place(const WireMixedArgs& a, uint32_t i, const uint64_t at[6], const uint64_t v[6]) {
    uint32_t slot = COA_WIRE_NO_SLOT;
    if (v[0]) {
      slot = (uint32_t)at[0];
      a.set[COA_MSG_HEADER].hoff[slot] = at[1];
    } else if (v[2]) {
      slot = (uint32_t)at[2];
    } else if (v[3]) {
      slot = (uint32_t)at[3];
      a.set[COA_MSG_CERTIFICATE].hoff[slot] = at[4];
      a.set[COA_MSG_CERTIFICATE].voff[slot] = at[5];
    }
    a.slots[i] = slot;
  }
};

// Exclusive scan of v over the block's COA_WIRE_SCAN_BLOCK threads.
template <int Q>
__device__ void block_scan(const uint64_t v[Q], uint64_t (*sh)[COA_WIRE_SCAN_BLOCK], uint64_t excl[Q], uint64_t total[Q]) {
  const uint32_t t = threadIdx.x;
  for (int q = 0; q < Q; q++) sh[q][t] = v[q];
  __syncthreads();
  for (uint32_t o = 1; o < COA_WIRE_SCAN_BLOCK; o <<= 1) {
    uint64_t x[Q];
    for (int q = 0; q < Q; q++) x[q] = t >= o ? sh[q][t - o] : 0;
    __syncthreads();
    for (int q = 0; q < Q; q++) sh[q][t] += x[q];
    __syncthreads();
  }
  for (int q = 0; q < Q; q++) {
    excl[q] = sh[q][t] - v[q];
    total[q] = sh[q][COA_WIRE_SCAN_BLOCK - 1];
  }
}

template <class M>
__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_block_totals(const typename M::Args a) {
  constexpr int Q = M::Q;
  __shared__ uint64_t sh[Q][COA_WIRE_SCAN_BLOCK];
  uint64_t v[Q], excl[Q], total[Q];
  M::contribution(a, blockIdx.x * COA_WIRE_SCAN_BLOCK + threadIdx.x, v);
  block_scan<Q>(v, sh, excl, total);
  if (threadIdx.x < Q) a.bt[(size_t)blockIdx.x * Q + threadIdx.x] = total[threadIdx.x];
}

// One block: the block totals become their exclusive prefixes in place, and
// the call's totals are written.
template <class M>
__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_scan_totals(const typename M::Args a, uint32_t blocks) {
  constexpr int Q = M::Q;
  __shared__ uint64_t sh[Q][COA_WIRE_SCAN_BLOCK];
  const uint32_t per = (blocks + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK;
  const uint32_t lo = min(blocks, threadIdx.x * per), hi = min(blocks, lo + per);
  uint64_t v[Q] = {}, excl[Q], total[Q];
  for (uint32_t b = lo; b < hi; b++)
    for (int q = 0; q < Q; q++) v[q] += a.bt[(size_t)b * Q + q];
  block_scan<Q>(v, sh, excl, total);
  for (uint32_t b = lo; b < hi; b++)
    for (int q = 0; q < Q; q++) {
      const uint64_t t = a.bt[(size_t)b * Q + q];
      a.bt[(size_t)b * Q + q] = excl[q];
      excl[q] += t;
    }
  if (threadIdx.x == 0) M::totals(a, total);
}

template <class M>
__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_add(const typename M::Args a) {
  constexpr int Q = M::Q;
  __shared__ uint64_t sh[Q][COA_WIRE_SCAN_BLOCK];
  const uint32_t i = blockIdx.x * COA_WIRE_SCAN_BLOCK + threadIdx.x;
  uint64_t v[Q], excl[Q], total[Q];
  M::contribution(a, i, v);
  block_scan<Q>(v, sh, excl, total);
  if (i >= a.n) return;
  for (int q = 0; q < Q; q++) excl[q] += a.bt[(size_t)blockIdx.x * Q + q];
  M::place(a, i, excl, v);
}

// A frame known to be a well-formed message of kind `want` into item `item` of
// the arrays o (the index-aligned decode: item i is frame i; the mixed mode:
// the frame's slot).
__device__ __forceinline__ void decode_frame(const WireSet& o, int32_t want, uint32_t item, const uint8_t* p, size_t len,
                                             uint32_t lane, uint8_t* last) {
  CoaWpFrame f;
  (void)coa_wp_walk(p, len, &f);
  const size_t i = item;
  if (want == COA_MSG_VOTE) {
    if (lane < 32) o.ids[i * 32 + lane] = p[f.v_id + lane];
    o.sigs[i * 64 + lane] = p[f.v_sig + lane];
    if (lane == 0) o.rounds[i] = f.v_round;
    if (lane < 2) {
      size_t pos = lane ? f.v_author : f.v_origin;
      (void)coa_wp_key(p, len, &pos, (lane ? o.authors : o.vorigins) + i * 32);
    }
    return;
  }
  uint8_t* out = o.hdata + o.hoff[i];
  if (lane < 32) o.ids[i * 32 + lane] = p[f.id + lane];
  o.sigs[i * 64 + lane] = p[f.sig + lane];
  if (lane < 2) {
    size_t pos = f.author;
    (void)coa_wp_key(p, len, &pos, lane ? o.authors + i * 32 : out);
  }
  if (lane == 2) o.rounds[i] = f.round;
  if (lane >= 8 && lane < 16) out[32 + (lane - 8)] = (uint8_t)(f.round >> (8 * (lane - 8)));
  const uint32_t P = set_last(p + f.payload, 36, (uint32_t)f.np, lane, last);
  set_emit(p + f.payload, 36, (uint32_t)f.np, lane, last, out + 40);
  (void)set_last(p + f.parents, 32, (uint32_t)f.nq, lane, last);
  set_emit(p + f.parents, 32, (uint32_t)f.nq, lane, last, out + 40 + 36 * (size_t)P);
  if (lane == 0) o.pcounts[i] = P;
  if (want == COA_MSG_CERTIFICATE) {
    const uint64_t v0 = o.voff[i];
    (void)votes_do(p, len, f, lane, o.vpks + v0 * 32, o.vsigs + v0 * 64);
  }
}

__global__ void __launch_bounds__(64 * kWaves) k_wire_decode(const WireArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[kWaves][kStage + 16];
  __shared__ uint8_t last[kWaves][COA_WIRE_DEV_MAX_ENTRIES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * kWaves + wave;
  if (i >= a.n) return;
  if (a.kinds[i] != a.want) {
    // the placeholder: item i stays aligned with frame i and holds nothing
    if (lane < 32) a.out.ids[(size_t)i * 32 + lane] = 0;
    if (lane < 32) a.out.authors[(size_t)i * 32 + lane] = 0;
    if (lane < 32 && a.out.vorigins) a.out.vorigins[(size_t)i * 32 + lane] = 0;
    a.out.sigs[(size_t)i * 64 + lane] = 0;
    if (lane == 0) a.out.rounds[i] = 0;
    if (lane == 0 && a.out.pcounts) a.out.pcounts[i] = 0;
    return;
  }
  // the scan found the frame inside the buffer and well formed
  const uint64_t o0 = a.offs[i];
  const size_t len = (size_t)(a.offs[i + 1] - o0);
  if (len <= kStage)
    decode_frame(a.out, a.want, i, stage_frame(a.frames + o0, (uint32_t)len, lane, stage[wave]), len, lane, last[wave]);
  else
    decode_frame(a.out, a.want, i, a.frames + o0, len, lane, last[wave]);
}

// The mixed mode: frame i of kind k into item slots[i] of kind k's arrays.  A
// frame without a slot writes nothing: no placeholders, and nothing at or
// above a kind's count.
template <uint32_t W>
__global__ void __launch_bounds__(64 * W) k_wire_decode_mixed(const WireMixedArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[W][kStage + 16];
  __shared__ uint8_t last[W][COA_WIRE_DEV_MAX_ENTRIES];
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t i = blockIdx.x * W + wave;
  if (i >= a.n) return;
  const uint32_t slot = a.slots[i];
  if (slot == COA_WIRE_NO_SLOT) return;
  // the scan found the frame inside the buffer and well formed, of kind 0, 1 or 2
  const int32_t kind = __builtin_amdgcn_readfirstlane(a.kinds[i]);
  const WireSet& o = a.set[kind];
  const uint64_t o0 = a.offs[i];
  const size_t len = (size_t)(a.offs[i + 1] - o0);
  if (len <= kStage)
    decode_frame(o, kind, slot, stage_frame(a.frames + o0, (uint32_t)len, lane, stage[wave]), len, lane, last[wave]);
  else
    decode_frame(o, kind, slot, a.frames + o0, len, lane, last[wave]);
}

// One thread per frame: its item's word, or COA_DAG_NO_MESSAGE.
__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_scatter(const int32_t* kinds, const uint32_t* slots,
                                                                       const uint32_t* w0, const uint32_t* w1,
                                                                       const uint32_t* w2, uint32_t* out, uint32_t n) {
  const uint32_t i = blockIdx.x * COA_WIRE_SCAN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = slots[i];
  uint32_t w = COA_DAG_NO_MESSAGE;
  if (slot != COA_WIRE_NO_SLOT) {
    const int32_t kind = kinds[i];
    w = (kind == COA_MSG_HEADER ? w0 : kind == COA_MSG_VOTE ? w1 : w2)[slot];
  }
  out[i] = w;
}

}  // namespace

hipError_t coa_launch_wire_scan(const WireHead& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wire_scan, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  return hipGetLastError();
}

hipError_t coa_launch_wire_decode(const WireArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = (a.n + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK;
  hipLaunchKernelGGL(k_wire_scan, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  hipLaunchKernelGGL(k_wire_block_totals<SumsOne>, dim3(blocks), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_wire_scan_totals<SumsOne>, dim3(1), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a, blocks);
  hipLaunchKernelGGL(k_wire_add<SumsOne>, dim3(blocks), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_wire_decode, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  return hipGetLastError();
}

hipError_t coa_launch_wire_decode_mixed(const WireMixedArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = (a.n + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK;
  hipLaunchKernelGGL(k_wire_scan, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  hipLaunchKernelGGL(k_wire_block_totals<SumsMixed>, dim3(blocks), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_wire_scan_totals<SumsMixed>, dim3(1), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a, blocks);
  hipLaunchKernelGGL(k_wire_add<SumsMixed>, dim3(blocks), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_wire_decode_mixed<kMixedWaves>, dim3((a.n + kMixedWaves - 1) / kMixedWaves), dim3(64 * kMixedWaves), 0,
                     s, a);
  return hipGetLastError();
}

hipError_t coa_launch_wire_scatter(const int32_t* kinds, const uint32_t* slots, const uint32_t* header_words,
                                   const uint32_t* vote_words, const uint32_t* certificate_words, uint32_t* out,
                                   uint32_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wire_scatter, dim3((n + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK), dim3(COA_WIRE_SCAN_BLOCK), 0,
                     s, kinds, slots, header_words, vote_words, certificate_words, out, n);
  return hipGetLastError();
}

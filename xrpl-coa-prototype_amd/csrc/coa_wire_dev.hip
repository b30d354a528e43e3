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

__global__ void __launch_bounds__(64 * kWaves) k_wire_scan(const WireArgs a) {
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

// What frame i adds to the call's sums: header bytes, votes, one frame.
__device__ __forceinline__ void contribution(const WireArgs& a, uint32_t i, uint64_t v[3]) {
  const bool mine = i < a.n && a.kinds[i] == a.want;
  v[0] = mine && a.want != COA_MSG_VOTE ? a.hb[i] : 0;
  v[1] = mine && a.want == COA_MSG_CERTIFICATE ? a.nv[i] : 0;
  v[2] = mine ? 1 : 0;
}

// Exclusive scan of v over the block's COA_WIRE_SCAN_BLOCK threads.
__device__ void block_scan(const uint64_t v[3], uint64_t (*sh)[COA_WIRE_SCAN_BLOCK], uint64_t excl[3], uint64_t total[3]) {
  const uint32_t t = threadIdx.x;
  for (int q = 0; q < 3; q++) sh[q][t] = v[q];
  __syncthreads();
  for (uint32_t o = 1; o < COA_WIRE_SCAN_BLOCK; o <<= 1) {
    uint64_t x[3];
    for (int q = 0; q < 3; q++) x[q] = t >= o ? sh[q][t - o] : 0;
    __syncthreads();
    for (int q = 0; q < 3; q++) sh[q][t] += x[q];
    __syncthreads();
  }
  for (int q = 0; q < 3; q++) {
    excl[q] = sh[q][t] - v[q];
    total[q] = sh[q][COA_WIRE_SCAN_BLOCK - 1];
  }
}

__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_block_totals(const WireArgs a) {
  __shared__ uint64_t sh[3][COA_WIRE_SCAN_BLOCK];
  uint64_t v[3], excl[3], total[3];
  contribution(a, blockIdx.x * COA_WIRE_SCAN_BLOCK + threadIdx.x, v);
  block_scan(v, sh, excl, total);
  if (threadIdx.x < 3) a.bt[(size_t)blockIdx.x * 3 + threadIdx.x] = total[threadIdx.x];
}

// One block: the block totals become their exclusive prefixes in place, and
// the call's totals are written.
__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_scan_totals(const WireArgs a, uint32_t blocks) {
  __shared__ uint64_t sh[3][COA_WIRE_SCAN_BLOCK];
  const uint32_t per = (blocks + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK;
  const uint32_t lo = min(blocks, threadIdx.x * per), hi = min(blocks, lo + per);
  uint64_t v[3] = {0, 0, 0}, excl[3], total[3];
  for (uint32_t b = lo; b < hi; b++)
    for (int q = 0; q < 3; q++) v[q] += a.bt[(size_t)b * 3 + q];
  block_scan(v, sh, excl, total);
  for (uint32_t b = lo; b < hi; b++)
    for (int q = 0; q < 3; q++) {
      const uint64_t t = a.bt[(size_t)b * 3 + q];
      a.bt[(size_t)b * 3 + q] = excl[q];
      excl[q] += t;
    }
  if (threadIdx.x == 0 && a.totals) {
    a.totals[0] = total[0];
    a.totals[1] = total[1];
    a.totals[2] = total[2];
    a.totals[3] = a.n - total[2];
  }
}

__global__ void __launch_bounds__(COA_WIRE_SCAN_BLOCK) k_wire_add(const WireArgs a) {
  __shared__ uint64_t sh[3][COA_WIRE_SCAN_BLOCK];
  const uint32_t i = blockIdx.x * COA_WIRE_SCAN_BLOCK + threadIdx.x;
  uint64_t v[3], excl[3], total[3];
  contribution(a, i, v);
  block_scan(v, sh, excl, total);
  if (i >= a.n) return;
  const uint64_t h = a.bt[(size_t)blockIdx.x * 3] + excl[0], w = a.bt[(size_t)blockIdx.x * 3 + 1] + excl[1];
  if (a.hoff) {
    a.hoff[i] = h;
    if (i == a.n - 1) a.hoff[a.n] = h + v[0];
  }
  if (a.voff) {
    a.voff[i] = w;
    if (i == a.n - 1) a.voff[a.n] = w + v[1];
  }
}

// Frame i, known to be a well-formed message of kind a.want, into the arrays.
__device__ __forceinline__ void decode_frame(const WireArgs& a, uint32_t i, const uint8_t* p, size_t len, uint32_t lane,
                                             uint8_t* last) {
  CoaWpFrame f;
  (void)coa_wp_walk(p, len, &f);
  if (a.want == COA_MSG_VOTE) {
    if (lane < 32) a.ids[(size_t)i * 32 + lane] = p[f.v_id + lane];
    a.sigs[(size_t)i * 64 + lane] = p[f.v_sig + lane];
    if (lane == 0) a.rounds[i] = f.v_round;
    if (lane < 2) {
      size_t pos = lane ? f.v_author : f.v_origin;
      (void)coa_wp_key(p, len, &pos, (lane ? a.authors : a.vorigins) + (size_t)i * 32);
    }
    return;
  }
  uint8_t* out = a.hdata + a.hoff[i];
  if (lane < 32) a.ids[(size_t)i * 32 + lane] = p[f.id + lane];
  a.sigs[(size_t)i * 64 + lane] = p[f.sig + lane];
  if (lane < 2) {
    size_t pos = f.author;
    (void)coa_wp_key(p, len, &pos, lane ? a.authors + (size_t)i * 32 : out);
  }
  if (lane == 2) a.rounds[i] = f.round;
  if (lane >= 8 && lane < 16) out[32 + (lane - 8)] = (uint8_t)(f.round >> (8 * (lane - 8)));
  const uint32_t P = set_last(p + f.payload, 36, (uint32_t)f.np, lane, last);
  set_emit(p + f.payload, 36, (uint32_t)f.np, lane, last, out + 40);
  (void)set_last(p + f.parents, 32, (uint32_t)f.nq, lane, last);
  set_emit(p + f.parents, 32, (uint32_t)f.nq, lane, last, out + 40 + 36 * (size_t)P);
  if (lane == 0) a.pcounts[i] = P;
  if (a.want == COA_MSG_CERTIFICATE) {
    const uint64_t v0 = a.voff[i];
    (void)votes_do(p, len, f, lane, a.vpks + v0 * 32, a.vsigs + v0 * 64);
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
    if (lane < 32) a.ids[(size_t)i * 32 + lane] = 0;
    if (lane < 32) a.authors[(size_t)i * 32 + lane] = 0;
    if (lane < 32 && a.vorigins) a.vorigins[(size_t)i * 32 + lane] = 0;
    a.sigs[(size_t)i * 64 + lane] = 0;
    if (lane == 0) a.rounds[i] = 0;
    if (lane == 0 && a.pcounts) a.pcounts[i] = 0;
    return;
  }
  // the scan found the frame inside the buffer and well formed
  const uint64_t o0 = a.offs[i];
  const size_t len = (size_t)(a.offs[i + 1] - o0);
  if (len <= kStage)
    decode_frame(a, i, stage_frame(a.frames + o0, (uint32_t)len, lane, stage[wave]), len, lane, last[wave]);
  else
    decode_frame(a, i, a.frames + o0, len, lane, last[wave]);
}

}  // namespace

hipError_t coa_launch_wire_scan(const WireArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_wire_scan, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  return hipGetLastError();
}

hipError_t coa_launch_wire_decode(const WireArgs& a, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  const uint32_t blocks = (a.n + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK;
  hipLaunchKernelGGL(k_wire_scan, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  hipLaunchKernelGGL(k_wire_block_totals, dim3(blocks), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_wire_scan_totals, dim3(1), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a, blocks);
  hipLaunchKernelGGL(k_wire_add, dim3(blocks), dim3(COA_WIRE_SCAN_BLOCK), 0, s, a);
  hipLaunchKernelGGL(k_wire_decode, dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, s, a);
  return hipGetLastError();
}

// Latency variants of the committee kernels for gfx950: one 192-thread
// workgroup per signature job (the registered-key latency job, coa_lat_job.h)
// and one per header digest: its lanes expand every block's message schedule
// into LDS, then one wave runs the rounds (coa_sha512.h, compress_kw).
//   k_cert_verify_lat      Certificate::verify's crypto, one certificate at a
//                          time (the checks of coa_committee.hip's k_cert_verify)
//   k_cert_verify_lat_inl  the same, the arrays in the kernel arguments
//   k_msg_verify_lat       a window's headers and votes, every job strict
//   k_msg_verdict_lat      the same answering whole verdicts (wave 0 also
//                          decides the protocol code of its message,
//                          coa_prot_scan.h)
// Also here: k_fe_rows_check, which checks the row arithmetic only these
// kernels and coa_latency.hip use.
// kernels here exceed the +-128 KiB reach of an out-of-line fold (coa_fe.h)
#define COA_RARE_INLINE
#include "coa_committee.h"

#include <cstddef>
#include <type_traits>

#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_halved.h"
#include "coa_sc.h"
#include "coa_keycache.h"
#include "coa_lat_job.h"
#include "coa_prot_scan.h"
#include "coa_sha512.h"
#include "coa_smul.h"

using namespace coa_kc;

// Blocks [0, nc): header digests (wave 0 of each).  Blocks [nc, 2nc + nv):
// one signature job each.
#define KW_CHUNK 64  // blocks of schedule per LDS pass (40 KiB)
#ifdef COA_LAT_TRACE  // phase timestamps of the first signature job (tools/lat_trace.py)
__device__ unsigned long long g_lat_trace[3][8];
#define LAT_MARK(w, i) \
  if (job == 0 && lane == 0) g_lat_trace[w][i] = clock64();
extern "C" int coa_lat_trace(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_lat_trace), sizeof(g_lat_trace)) == hipSuccess ? 0 : -1;
}
// header-digest block of certificate 0 and the kernel's end, in the
// GPU-wide 100 MHz real-time clock (comparable across CUs): 0 start, 1
// schedule expanded, 2 rounds done, 3 compared, 5 signature job 0's verdict,
// 6 the last block's publish, 7 signature job 0's start
__device__ unsigned long long g_hdr_trace[12];
#define HDR_MARK(i) g_hdr_trace[i] = __builtin_amdgcn_s_memrealtime();
extern "C" int coa_lat_trace_hdr(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_hdr_trace), sizeof(g_hdr_trace)) == hipSuccess ? 0 : -1;
}
#else
#define LAT_MARK(w, i)
#define HDR_MARK(i)
#endif
// What differs between the latency kernels (A: CertArgs, k_cert_verify_lat,
// or MsgLatArgs, k_msg_verify_lat): lat_digests header-digest blocks lead the
// grid, lat_words status words are published, and lat_job names signature job
// `job`: its status word, its signature, its key, the 32-byte id it signs
// (strict: dalek's verify_strict rule; digest: the message is SHA-512(id ||
// round LE || origin)[..32] of *round and origin, hashed on wave 0).
namespace {
struct LatJob {
  bool strict, digest;
  uint32_t c;
  const uint32_t *sig, *pk, *id, *origin;
  const uint64_t* round;
};
COA_DEV uint32_t lat_digests(const CertArgs& a) { return a.nc; }
COA_DEV uint32_t lat_words(const CertArgs& a) { return a.nc; }
COA_DEV LatJob lat_job(const CertArgs& a, uint32_t job) {
  const bool hdr = job < a.nc;
  const uint32_t vi = job - a.nc;
  const uint32_t c = hdr ? job : vote_cert<kUniform>(a.voff, a.nc, vi);
  LatJob j;
  j.strict = hdr;
  j.digest = !hdr;
  j.c = c;
  j.sig = sel_ptr(hdr, a.hsigs + (uint64_t)c * 16, a.vsigs + (uint64_t)vi * 16);
  j.pk = sel_ptr(hdr, a.origins + (uint64_t)c * 8, a.vpks + (uint64_t)vi * 8);
  j.id = a.ids + (uint64_t)c * 8;
  j.origin = a.origins + (uint64_t)c * 8;
  j.round = a.rounds + c;
  return j;
}
COA_DEV uint32_t lat_digests(const MsgLatArgs& a) { return a.nh; }
COA_DEV uint32_t lat_words(const MsgLatArgs& a) { return a.nh + a.nv; }
COA_DEV LatJob lat_job(const MsgLatArgs& a, uint32_t job) {
  const bool hdr = job < a.nh;
  const uint32_t vi = job - a.nh;
  LatJob j;
  j.strict = true;
  j.digest = !hdr;
  j.c = job;
  j.sig = sel_ptr(hdr, a.hsigs + (uint64_t)job * 16, a.vsigs + (uint64_t)vi * 16);
  j.pk = sel_ptr(hdr, a.hauthors + (uint64_t)job * 8, a.vauthors + (uint64_t)vi * 8);
  j.id = sel_ptr(hdr, a.ids + (uint64_t)job * 8, a.vids + (uint64_t)vi * 8);
  j.origin = a.vorigins + (uint64_t)vi * 8;  // read only when digest
  j.round = a.vrounds + vi;
  return j;
}

// k_msg_verdict_lat (A: MsgVerdictLatArgs) answers verdict words instead: a
// signature block's bits carry its message's protocol code in bits 8-15
// (with_code), and the word that leaves is coa_verdict_merge(status bits,
// code).  Publishing, the last block merges as it stores.  In status mode the
// block of a word that ends last stores the merged word over it: a vote's only
// block at once, a header's two blocks (digest and signature) told apart by
// bit 31, which each sets with its OR -- the one that finds it set is the
// second.
template <class A>
constexpr bool kLatVerdict = std::is_same_v<A, MsgVerdictLatArgs>;
constexpr uint32_t kLatFirstDone = 1u << 31;
COA_DEV uint32_t with_code(uint32_t status, uint32_t code) { return status | (code << 8); }
COA_DEV uint32_t merged(uint32_t st) { return coa_verdict_merge(st & 0xffu, (st >> 8) & 0xffu); }

// One block's end of the latency kernel (one thread): OR its status bits
// into certificate c's word and, with a.host_res set, count itself done; the
// block that finishes last publishes every certificate's status word into
// page-locked host memory, tagged with the call (the host polls for the tag:
// no device-to-host copy, no stream synchronisation), and resets the status
// words and the block counter for the next call.
// Every value that crosses blocks is an atomic on its own word, so no fence
// orders other memory: the OR is a returning atomic whose completion the
// block waits for (s_waitcnt) before its count, so the last block's exchange
// (issued after its count saw every other block's) finds every OR.  The
// acq_rel fences this replaced cost an L2 write-back and an L1 invalidate
// each (buffer_wbl2 / buffer_inv sc1), four and three of them on the
// critical block's tail.
template <class A>
COA_DEV void lat_block_done(const A& a, uint32_t c, uint32_t bits) {
  if constexpr (kLatVerdict<A>) {
    if (!a.host_res) {
      if (c >= a.nh) {
        a.status[c] = merged(bits);
        return;
      }
      const uint32_t old =
          __hip_atomic_fetch_or(a.status + c, bits | kLatFirstDone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old & kLatFirstDone)
        __hip_atomic_store(a.status + c, merged(old | bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
  if (bits) (void)__hip_atomic_fetch_or(a.status + c, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!a.host_res) return;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const uint32_t old = __hip_atomic_fetch_add(a.done_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (old + 1 != a.total_blocks) return;
  HDR_MARK(6)
  __hip_atomic_store(a.done_ctr, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (uint32_t k = 0; k < lat_words(a); k++) {
    const uint32_t st = __hip_atomic_exchange(a.status + k, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if constexpr (kLatVerdict<A>)
      __hip_atomic_store(a.host_res + k, (a.tag << 8) | merged(st), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else
      __hip_atomic_store(a.host_res + k, (a.tag << 8) | (st & 0xffu), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

template <class A>
COA_DEV void cert_lat_body(const A& a) {
  const uint32_t wave = coa_sha::uni(threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (blockIdx.x < lat_digests(a)) {  // header digest: schedule in parallel, rounds on wave 0
    __shared__ uint64_t kw_lds[KW_CHUNK * 80];
    const uint32_t c = blockIdx.x;
    if (c == 0 && threadIdx.x == 0) { HDR_MARK(0) }
    const uint64_t o0 = uni64(a.hdr_off[c]), len = uni64(a.hdr_off[c + 1]) - o0;
    if (c == 0 && threadIdx.x == 0 && len != ~0ull) { HDR_MARK(4) }
    const uint8_t* p = a.hdr_data + o0;
    const uint64_t nblk = (len + 17 + 127) / 128;
    // the rounds on wave 0, each lane pair running one round's two halves
    // (coa_sha512.h, compress_kw2); lane 0 ends with the whole state
    const coa_sha::Lane2 L2 = coa_sha::lane2(lane);
    uint64_t hs[4];
    coa_sha::init2(hs, L2);
#pragma unroll 1
    for (uint64_t b0 = 0; b0 < nblk; b0 += KW_CHUNK) {
      const uint32_t nb = (uint32_t)min<uint64_t>(KW_CHUNK, nblk - b0);
      if (threadIdx.x < nb) {
        uint64_t W[16];
        coa_sha::padded_block(W, p, len, b0 + threadIdx.x, nblk);
        if (c == 0 && threadIdx.x == 0 && b0 == 0 && W[0] != 0x0123456789abcdefull) { HDR_MARK(8) }
        coa_sha::expand_kw(kw_lds + threadIdx.x * 80, W);
#ifdef COA_LAT_TRACE
        if (c == 0 && threadIdx.x == 0 && b0 == 0) {
          __builtin_amdgcn_s_waitcnt(0);  // the schedule's LDS writes done
          HDR_MARK(9)
        }
#endif
      }
      __syncthreads();
      if (c == 0 && threadIdx.x == 0 && b0 == 0) { HDR_MARK(1) }
      if (wave == 0) {
#pragma unroll 1
        for (uint32_t b = 0; b < nb; b++) coa_sha::compress_kw2(hs, kw_lds + b * 80, L2);
      }
      __syncthreads();
    }
    if (c == 0 && threadIdx.x == 0) { HDR_MARK(2) }
    if (wave) return;
    uint64_t st[8];
    coa_sha::gather2(st, hs);
    const bool same = id_matches<kUniform>(st, a.ids + (uint64_t)c * 8);
    if (c == 0 && lane == 0) { HDR_MARK(3) }
    if (lane == 0) lat_block_done(a, c, same ? 0u : (uint32_t)COA_CST_BAD_HEADER_ID);
    return;
  }
  __shared__ uint32_t s_lds[32];  // [s]B from wave 2
  __shared__ uint32_t s_ready;    // wave 2 published [s]B
  __shared__ rcmp::Shared cmp;    // wave 0's half of the compare, for wave 1
  latjob::init(&s_ready, cmp);
  const uint32_t job = blockIdx.x - lat_digests(a);
  const LatJob J = lat_job(a, job);
  const uint32_t* sig = J.sig;
  uint32_t rw[8];
  load8u(rw, sig);
  LAT_MARK(wave, 0)
  if (job == 0 && threadIdx.x == 0) { HDR_MARK(7) }
  if (wave == 1) {  // R's decompression on the wave's DPP rows, the compare, the verdict
    uint32_t word;
    uint32_t bits = latjob::decide(cmp, rw, word, [&] { LAT_MARK(1, 1) }, [&] { LAT_MARK(1, 2) });
    if constexpr (kLatVerdict<A>) bits = with_code(bits, coa_job_code(word));  // the protocol code wave 0 handed over
    LAT_MARK(1, 5)
    if (job == 0 && lane == 0) { HDR_MARK(5) }
    if (lane == 0) lat_block_done(a, J.c, bits);
    return;
  }
  // one comb term per lane (lanes 0..31; the upper half sums a copy),
  // [s]B on wave 2 from B's comb, [k](-A) on wave 0 from the key's comb
  uint32_t dg[8];
  const uint32_t* tab = a.comb;
  uint32_t pre = 0, code = 0;
  if (wave == 2) {
    load8u(dg, sig + 8);
  } else {
    uint32_t pk[8], sw[8], msg[8];
    load8u(pk, J.pk);
    load8u(sw, sig + 8);
    load8u(msg, J.id);
    const int slot = key_lookup<kUniform>(a.keys, a.nk, pk);
    if (slot < 0) {
      // outside the committee: the verdict needs no crypto
      if constexpr (kLatVerdict<A>) code = COA_DAG_UNKNOWN_AUTHOR;
      LAT_MARK(wave, 1)
      latjob::skip(cmp, code, lane);
      return;
    }
    // the message's protocol code, beside wave 1's chain: the stake of the
    // slot just found and a header's worker ids over the lanes
    if constexpr (kLatVerdict<A>) {
      const uint8_t* hp = nullptr;
      uint64_t hlen = 0;
      uint32_t pc = 0;
      if (job < a.nh) {  // a header's job (J.strict is set for votes too)
        const uint64_t o0 = uni64(a.hdr_off[job]);
        hlen = uni64(a.hdr_off[job + 1]) - o0;
        hp = a.hdr_data + o0;
        pc = coa_sha::uni(a.hpcounts[job]);
      }
      code = coa_prot::msg_code_wave(a.t, (uint32_t)slot, hp, hlen, pc, lane);
    }
    if (J.digest) {  // Certificate::digest / Vote::digest on the scalar unit
      uint32_t origin[8];
      load8u(origin, J.origin);
      round_origin_digest(msg, uni64(*J.round), origin);
    }
    pre = latjob::challenge_bits(dg, rw, pk, sw, msg, coa_sha::uni(a.kflags[slot]), J.strict ? COA_JOB_STRICT : 0u);
    tab = a.ktabs + (uint64_t)slot * COA_KEY_TAB_DWORDS;
  }
  LAT_MARK(wave, 1)
  rp::P1 P;  // row form (coa_ge_rows.h)
  rcmp::comb_sum_rows(P, dg, tab, lane);
  LAT_MARK(wave, 3)
  if (wave == 2) {
    latjob::publish_sB(s_lds, &s_ready, P, lane);
    return;
  }
  latjob::finish_P(cmp, s_lds, &s_ready, P, rw, pre, code, lane);
  LAT_MARK(0, 4)
}
}  // namespace

__global__ void __launch_bounds__(192) k_cert_verify_lat(CertArgs a) { cert_lat_body(a); }

// Header::verify / Vote::verify crypto of one window's messages, latency
// shape (MsgLatArgs, coa_committee.h): the body above with every signature
// job strict.  A header's signature job signs ids[i] as given, so it runs
// beside that header's digest block, not after it.
__global__ void __launch_bounds__(192) k_msg_verify_lat(MsgLatArgs a) { cert_lat_body(a); }

// The same answering whole Header::verify / Vote::verify verdicts
// (MsgVerdictLatArgs): no further launch, no lookup on the publishing tail.
__global__ void __launch_bounds__(192) k_msg_verdict_lat(MsgVerdictLatArgs a) { cert_lat_body(a); }

// The same with the certificate's arrays read from the kernel arguments.  The
// buffer is addressed through the kernarg segment pointer (ci is the only
// argument, at offset 0): a pointer taken from the by-value parameter itself
// would make hipcc copy the whole 3 KB argument into scratch per thread.
__global__ void __launch_bounds__(192) k_cert_verify_lat_inl(CertInl ci) {
  CertArgs a = ci.a;
  const uint8_t* b = reinterpret_cast<const uint8_t*>(
                         reinterpret_cast<uintptr_t>(__builtin_amdgcn_kernarg_segment_ptr())) +
                     offsetof(CertInl, buf);
  a.hdr_data = b + ci.off_hdr;
  a.hdr_off = reinterpret_cast<const uint64_t*>(b + ci.off_hoff);
  a.ids = reinterpret_cast<const uint32_t*>(b + ci.off_ids);
  a.origins = reinterpret_cast<const uint32_t*>(b + ci.off_origins);
  a.hsigs = reinterpret_cast<const uint32_t*>(b + ci.off_hsigs);
  a.rounds = reinterpret_cast<const uint64_t*>(b + ci.off_rounds);
  a.voff = reinterpret_cast<const uint64_t*>(b + ci.off_voff);
  a.vpks = reinterpret_cast<const uint32_t*>(b + ci.off_vpks);
  a.vsigs = reinterpret_cast<const uint32_t*>(b + ci.off_vsigs);
  cert_lat_body(a);
}

// one workgroup per header digest and per signature
hipError_t coa_launch_cert_verify_lat(CertArgs a, hipStream_t s) {
  if (a.nc == 0) return hipSuccess;
  a.hdr_blocks = (a.nc + 255) / 256;
  a.total_blocks = 2 * a.nc + a.nv;
  hipLaunchKernelGGL(k_cert_verify_lat, dim3(a.total_blocks), dim3(192), 0, s, a);
  return hipGetLastError();
}

hipError_t coa_launch_cert_verify_inl(const CertInl& ci, hipStream_t s) {
  if (ci.a.nc == 0) return hipSuccess;
  CertInl c = ci;
  c.a.hdr_blocks = (c.a.nc + 255) / 256;
  c.a.total_blocks = 2 * c.a.nc + c.a.nv;
  hipLaunchKernelGGL(k_cert_verify_lat_inl, dim3(c.a.total_blocks), dim3(192), 0, s, c);
  return hipGetLastError();
}

hipError_t coa_launch_msg_verify_lat(MsgLatArgs a, hipStream_t s) {
  if (a.nh + a.nv == 0) return hipSuccess;
  a.total_blocks = 2 * a.nh + a.nv;
  hipLaunchKernelGGL(k_msg_verify_lat, dim3(a.total_blocks), dim3(192), 0, s, a);
  return hipGetLastError();
}

hipError_t coa_launch_msg_verdict_lat(MsgVerdictLatArgs a, hipStream_t s) {
  if (a.nh + a.nv == 0) return hipSuccess;
  a.total_blocks = 2 * a.nh + a.nv;
  hipLaunchKernelGGL(k_msg_verdict_lat, dim3(a.total_blocks), dim3(192), 0, s, a);
  return hipGetLastError();
}

// coa_fe_rows_check: the row-parallel chains against the one-lane ones.
__global__ void __launch_bounds__(64) k_fe_rows_check(const uint8_t* __restrict__ in, uint32_t n,
                                                      uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x;
  uint32_t w[8], w2[8];
  load8u(w, reinterpret_cast<const uint32_t*>(in + (uint64_t)i * 32));
  load8u(w2, reinterpret_cast<const uint32_t*>(in + (uint64_t)((i + 1) % n) * 32));
  fe x, y;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    x.v[k] = w[k];
    y.v[k] = w2[k];
  }
  uint32_t bad = 0;
  fe a, b;
  fe_pow_p58_rows(a, x);
  fe_pow_p58(b, x);
  bad |= fe_eq(a, b) ? 0u : 1u;
  fe_invert_rows(a, x);
  fe_invert(b, x);
  bad |= fe_eq(a, b) ? 0u : 2u;
  fw::to_fe(a, fw::mul(fw::from_fe(x), fw::from_fe(y)));
  fe_mul(b, x, y);
  bad |= fe_eq(a, b) ? 0u : 4u;
  fw::to_fe(a, fw::add(fw::from_fe(x), fw::from_fe(y)));
  fe_add(b, x, y);
  bad |= fe_eq(a, b) ? 0u : 16u;
  fw::to_fe(a, fw::sub(fw::from_fe(x), fw::from_fe(y)));
  fe_sub(b, x, y);
  bad |= fe_eq(a, b) ? 0u : 32u;
  ge_p3 P, Q;
  const bool ok_r = ge_decompress<true>(P, w);
  const bool ok_s = ge_decompress(Q, w);
  if (ok_r != ok_s || (ok_s && !(fe_eq(P.X, Q.X) && fe_eq(P.Y, Q.Y) && fe_eq(P.T, Q.T)))) bad |= 8u;
  if (threadIdx.x == 0) out[i] = bad;
}

hipError_t coa_launch_fe_rows_check(const uint8_t* in, uint32_t n, uint32_t* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_fe_rows_check, dim3(n), dim3(64), 0, s, in, n, out);
  return hipGetLastError();
}

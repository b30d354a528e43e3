// The fused Certificate::verify kernel and its message
// counterpart for gfx950, throughput variant.
//
// With the committee key cache (coa_keybuild.hip), a signature's equation
// P = [s]B + [k](-A) needs no doubling: 13 to 32 comb additions per scalar.
//
// k_cert_verify runs the whole crypto of Certificate::verify
// (primary/src/messages.rs:189-215) in one launch, every check independent:
//   * header digest role (leading blocks, one lane per certificate):
//     SHA-512(Header::digest bytes)[..32] == header.id   (messages.rs:49-51)
//   * signature role, one job per header signature and per vote:
//     header: verify_strict(header.id, author)            (messages.rs:64-66)
//             -- s < l, A and R decompress, neither small order, P == R
//     vote:   the message is Certificate::digest =
//             SHA-512(id || round || origin)[..32]         (messages.rs:226-234)
//             computed in-kernel; per vote s < l, A and R decompress and
//             P == R (cofactorless, projective).
// verify_batch exactness (crypto/src/lib.rs:206-219 -> dalek verify_batch):
// dalek accepts iff sum z_i (R_i + h_i A_i - s_i B) == O for its random z_i,
// when every A_i is torsion free (then (z_i h_i mod l) A_i == z_i h_i A_i).
// So if every vote satisfies its own equation and every key is torsion free
// the batch verdict is Ok for EVERY z -- exactly dalek's.  Any other outcome
// with well-formed inputs is flagged COA_CST_VOTES_INCONCLUSIVE and the host
// re-runs that certificate through the exact RLC kernels (coa_batch.hip) with
// real weights; malformed inputs (s >= l, R or A not decompressing) are a
// definitive Err, as in dalek.  The rule is coa_rule_throughput
// (coa_job_bits.h).
//
// Throughput variant (the latency one: coa_cert_lat.hip): two waves per SIMD,
// each lane a strided set of signatures, P compared with R's encoding after
// one inversion shared by the lane's signatures; one lane per header digest.
// k_msg_verify is the same grid over Header::verify / Vote::verify messages.
// kernels here exceed the +-128 KiB reach of an out-of-line fold (coa_fe.h)
#define COA_RARE_INLINE
#include "coa_committee.h"

#include <cstdlib>

#include "coa_cert_scratch.h"
#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_halved.h"
#include "coa_job_bits.h"
#include "coa_sc.h"
#include "coa_keycache.h"
#include "coa_sha512.h"
#include "coa_smul.h"

namespace {
using namespace coa_kc;

// What differs between the kernels' jobs: job_load fetches a job's key, R, s
// and 32-byte message id and looks the key up (its slot, < 0: not
// registered); `strict` selects dalek's verify_strict rule (a header
// signature, every message job), `cert` is the status word the job reports
// to.  job_message then turns the id into the signed message.
COA_DEV int job_load(const CertArgs& a, uint32_t job, bool& strict, uint32_t& cert, uint32_t* pk, uint32_t* rw,
                     uint32_t* sw, uint32_t* msg) {
  const bool hdr = job < a.nc;
  const uint32_t vi = job - a.nc;
  const uint32_t c = hdr ? job : vote_cert<kLane>(a.voff, a.nc, vi);
  cert = c;
  strict = hdr;
  const uint32_t* sig = sel_ptr(hdr, a.hsigs + (uint64_t)c * 16, a.vsigs + (uint64_t)vi * 16);
  load8(pk, sel_ptr(hdr, a.origins + (uint64_t)c * 8, a.vpks + (uint64_t)vi * 8));
  load8(rw, sig);
  load8(sw, sig + 8);
  load8(msg, a.ids + (uint64_t)c * 8);
  return key_lookup<kLane>(a.keys, a.nk, pk);
}
COA_DEV void job_message(const CertArgs& a, bool hdr, uint32_t c, uint32_t* msg) {
  if (!hdr && a.cdig) {  // Certificate::digest from the prologue kernel
    load8(msg, a.cdig + (uint64_t)c * 8);
  } else if (!hdr) {  // Certificate::digest = SHA-512(id || round u64 LE || origin)[..32]
    uint32_t origin[8];
    load8(origin, a.origins + (uint64_t)c * 8);
    round_origin_digest(msg, a.rounds[c], origin);
  }
}
// A message job (k_msg_verify): always strict; the message is the id
// (headers) or Vote::digest hashed here (votes).
COA_DEV int job_load(const MsgArgs& a, uint32_t job, bool& strict, uint32_t& cert, uint32_t* pk, uint32_t* rw,
                     uint32_t* sw, uint32_t* msg) {
  cert = job;
  strict = true;
  const uint32_t* sig = a.sigs + (uint64_t)job * 16;
  load8(pk, a.authors + (uint64_t)job * 8);
  load8(rw, sig);
  load8(sw, sig + 8);
  load8(msg, a.ids + (uint64_t)job * 8);
  return key_lookup<kLane>(a.keys, a.nk, pk);
}
COA_DEV void job_message(const MsgArgs& a, bool, uint32_t job, uint32_t* msg) {
  if (!a.rounds) return;
  uint32_t origin[8];
  load8(origin, a.origins + (uint64_t)job * 8);
  round_origin_digest(msg, a.rounds[job], origin);
}

// Phase A of one signature job, shared by the certificate and the message
// kernels (A: CertArgs or MsgArgs, which name the key tables alike).
template <class A>
COA_DEV void job_comb(const A& a, uint32_t job, ge_p3& P, uint32_t& pre, uint32_t& cert) {
  bool strict;
  uint32_t pk[8], rw[8], sw[8], msg[8];
  const int slot = job_load(a, job, strict, cert, pk, rw, sw, msg);
  ge_p3_identity(P);
  if (slot < 0) {
    pre = COA_JOB_UNCACHED;
    return;
  }
  job_message(a, strict, cert, msg);
  sc k;
  challenge(k, rw, pk, msg);
  const uint32_t kf = a.kflags[slot];
  pre = (sc_is_canonical(sw) ? 0u : COA_JOB_S) | ((kf & COA_KEY_DECOMPRESSES) ? 0u : COA_JOB_A) |
        ((kf & COA_KEY_SMALL_ORDER) ? COA_JOB_SMALL_A : 0u) | ((kf & COA_KEY_TORSION_FREE) ? 0u : COA_JOB_TORSION) |
        (strict ? COA_JOB_STRICT : 0u);
  // terms t < 32: B-comb bytes of s; t >= 32: key-comb bytes of k (signed
  // radix-256 digits = bytes of x + 0x80..80)
  uint32_t sd[8], kd[8];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    sd[i] = sw[i];
    kd[i] = k.v[i];
  }
  add_const_word(sd, 0x80808080u);
  add_const_word(kd, 0x80808080u);
  const uint32_t* ktab = a.ktabs + (uint64_t)slot * COA_KEY_TAB_DWORDS;
  ge_p1p1 t;
  // [s]B: 13 additions from the wide HBM comb when it is built, else the 32
  // byte terms of the radix-256 comb (an s >= l only reaches Err verdicts);
  // [k](-A): 13 or 16 additions from the key's wide comb (radix 2^20 or
  // 2^16) when the committee has them, else its 32 radix-256 terms
  if (a.wcomb) {
    wcomb_accumulate(P, sw, a.wcomb);
  } else {
#pragma unroll 1
    for (int j = 0; j < 32; j++) {
      ge_niels q;
      comb_select(q, a.comb, j, (int)byte_of(sd, j) - 128);
      ge_madd(t, P, q);
      ge_p1p1_to_p3(P, t);
    }
  }
  if (a.kwtabs && a.kw20) {
    wc_accumulate<COA_KWCOMB20_W, COA_KWCOMB20_POS, COA_KWC_STRIDE>(P, k.v, a.kwtabs + (uint64_t)slot * COA_KWCOMB20_DWORDS);
  } else if (a.kwtabs) {
    wc_accumulate<COA_KWCOMB_W, COA_KWCOMB_POS, COA_KWC_STRIDE>(P, k.v, a.kwtabs + (uint64_t)slot * COA_KWCOMB_DWORDS);
  } else {
#pragma unroll 1
    for (int j = 0; j < 32; j++) {
      ge_niels q;
      comb_select(q, ktab, j, (int)byte_of(kd, j) - 128);
      ge_madd(t, P, q);
      ge_p1p1_to_p3(P, t);
    }
  }
}

// Phase C: the verdict bits of a job from P's affine coordinates.  dalek's
// `P == decompress(R)` holds iff y_P == y_R (mod p; R's y is read as 255 bits,
// y >= p meaning y - p) and, unless x_P == 0, x_P's sign equals R's sign bit:
// when y_P == y_R the point P itself proves that R decompresses (to +-x_P).
COA_DEV uint32_t sig_verdict(uint32_t pre, const uint32_t* rw, const fe& x, const fe& y) {
  fe yr, xc, yc;
  fe_from_words(yr, rw);
  fe_canon(yr, yr);
  fe_canon(xc, x);
  fe_canon(yc, y);
  bool same_y = true, x_zero = true;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    same_y = same_y && yc.v[i] == yr.v[i];
    x_zero = x_zero && xc.v[i] == 0;
  }
  const bool eq = same_y && (x_zero || (xc.v[0] & 1u) == (rw[7] >> 31));
  if (pre & COA_JOB_STRICT) {
    // verify_strict: R == P, neither A nor R (== P) small order
    fe xx, yy, ss;
    fe_sq(xx, xc);
    fe_sq(yy, yc);
    fe_add(ss, xx, yy);
    bool y_zero = true;
#pragma unroll
    for (int i = 0; i < 8; i++) y_zero = y_zero && yc.v[i] == 0;
    const bool small_p = x_zero || y_zero || fe_iszero(ss);
    // the bit is this phase's alone (phase A leaves it clear)
    return coa_rule_throughput((pre & ~(uint32_t)COA_JOB_SMALL_P) | (small_p ? COA_JOB_SMALL_P : 0u), eq);
  }
  return coa_rule_throughput(pre, eq);
}

COA_DEV uint32_t job_verdict(const CertArgs& a, uint32_t job, uint32_t pre, const fe& x, const fe& y) {
  if (pre & (COA_JOB_NONE | COA_JOB_UNCACHED)) return coa_rule_throughput(pre, false);  // nothing to load
  const bool hdr = (pre & COA_JOB_STRICT) != 0;
  const uint32_t* sig = sel_ptr(hdr, a.hsigs + (uint64_t)job * 16, a.vsigs + (uint64_t)(job - a.nc) * 16);
  uint32_t rw[8];
  load8(rw, sig);
  return sig_verdict(pre, rw, x, y);
}

COA_DEV uint32_t job_verdict(const MsgArgs& a, uint32_t job, uint32_t pre, const fe& x, const fe& y) {
  if (pre & (COA_JOB_NONE | COA_JOB_UNCACHED)) return coa_rule_throughput(pre, false);  // nothing to load
  uint32_t rw[8];
  load8(rw, a.sigs + (uint64_t)job * 16);
  return sig_verdict(pre, rw, x, y);  // every job strict: COA_CST_BAD_HEADER_SIG or 0
}

// the job a chunk position stands for (certificates: key order when sorted)
COA_DEV uint64_t job_at(const CertArgs& a, uint64_t pos, uint64_t jobs) {
  return (a.perm && pos < jobs) ? a.perm[pos] : pos;
}
COA_DEV uint64_t job_at(const MsgArgs&, uint64_t pos, uint64_t) { return pos; }

// Scratch slab of the throughput kernel: per job slot 9 uint4 rows, each row
// lane-major (row r of slot q at uint4 index (q * 9 + r) * lanes + lane):
// X, Y, Z, prefix product of the Z's (2 rows each), then (pre, cert, -, -).
COA_DEV void pscr_put(uint32_t* pscr, uint64_t lanes, uint64_t lane, int j, int row, const fe& f) {
#pragma unroll
  for (int h = 0; h < 2; h++)
    reinterpret_cast<uint4*>(pscr)[((uint64_t)j * PSCR_ROWS + row + h) * lanes + lane] =
        make_uint4(f.v[4 * h], f.v[4 * h + 1], f.v[4 * h + 2], f.v[4 * h + 3]);
}
COA_DEV void pscr_get(fe& f, const uint32_t* pscr, uint64_t lanes, uint64_t lane, int j, int row) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint4 v = reinterpret_cast<const uint4*>(pscr)[((uint64_t)j * PSCR_ROWS + row + h) * lanes + lane];
    f.v[4 * h] = v.x;
    f.v[4 * h + 1] = v.y;
    f.v[4 * h + 2] = v.z;
    f.v[4 * h + 3] = v.w;
  }
}

}  // namespace

// Prologue of the throughput variant: Certificate::digest = SHA-512(id ||
// round u64 LE || origin)[..32] once per certificate (primary/src/
// messages.rs:226-234), instead of once per vote in the signature jobs (a
// C3 certificate has 67 votes: one SHA-512 block each saved).
__global__ void __launch_bounds__(256) k_cert_digests(CertArgs a, uint32_t* __restrict__ out) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= a.nc) return;
  uint32_t h[8], origin[8];
  load8(h, a.ids + (uint64_t)c * 8);
  load8(origin, a.origins + (uint64_t)c * 8);
  round_origin_digest(h, a.rounds[c], origin);
  uint4* o = reinterpret_cast<uint4*>(out + (uint64_t)c * 8);
  o[0] = make_uint4(h[0], h[1], h[2], h[3]);
  o[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

// Throughput variant.  The leading blocks hash the header digests, one lane
// per certificate (SHA-512 of the Header::digest bytes, ~27 blocks at C3),
// beside the signature waves.  The signature waves are a persistent grid of
// two waves per SIMD that take chunks of 64 consecutive jobs (one per lane)
// from a global counter until none is left, so every SIMD stays busy to
// within one chunk of the end: a static split leaves some SIMDs with one
// chunk more than others (5 vs 6 at C3, ~15 %), and the signature waves the
// header waves displace start late and simply take fewer chunks.
// Phase A computes each job's P and parks it with the running product of the
// Z's in a lane-major scratch slab; ONE field inversion serves all of a
// lane's jobs (Montgomery's trick), then phase C compares each affine P with
// its R encoding.  Per vote: ~265/jobs field operations of inversion instead
// of R's ~277-operation decompression.  pscr[0] is the chunk counter (zeroed
// by the launcher); the slab holds jcap jobs per lane.
// The header digest role of a leading block: lane c checks
// SHA-512(Header::digest bytes of c)[..32] == ids[c].
COA_DEV void header_digest_lane(const uint8_t* hdr_data, const uint64_t* hdr_off, const uint32_t* ids,
                                uint32_t* status, uint32_t c) {
  const uint64_t o0 = hdr_off[c], o1 = hdr_off[c + 1];
  uint64_t st[8];
  coa_sha::hash_mem(st, hdr_data + o0, o1 - o0);
  if (!id_matches<kLane>(st, ids + (uint64_t)c * 8)) atomicOr(status + c, COA_CST_BAD_HEADER_ID);
}

// The signature waves of a throughput grid (blocks from a.hdr_blocks on)
// over `jobs` jobs of A (CertArgs or MsgArgs: job_at, job_comb, job_verdict).
template <class A>
COA_DEV void tp_signature_waves(const A& a, uint32_t* __restrict__ pscr, uint32_t jcap, uint64_t jobs) {
  const uint64_t lanes = (uint64_t)(gridDim.x - a.hdr_blocks) * blockDim.x;
  const uint64_t lane = (uint64_t)(blockIdx.x - a.hdr_blocks) * blockDim.x + threadIdx.x;
  const uint32_t sub = threadIdx.x & 63;
  uint32_t* ctr = pscr + CertScratch::ctr;
  uint32_t* slab = pscr + CertScratch::slab;
  const uint32_t chunks = (uint32_t)((jobs + 63) / 64);
  int nj = 0;  // this wave's chunks (the same for all its lanes)
  fe zp;       // running prefix product of the Z's
#pragma unroll 1
  for (;;) {
    if (nj >= (int)jcap) break;  // slab full: the other waves take the rest
    uint32_t chunk = 0;
    if (sub == 0) chunk = atomicAdd(ctr, 1u);
    chunk = __builtin_amdgcn_readfirstlane(__shfl(chunk, 0));
    if (chunk >= chunks) break;
    const uint64_t job = job_at(a, (uint64_t)chunk * 64 + sub, jobs);  // key order (k_job_count, k_job_place)
    ge_p3 P;
    uint32_t pre = COA_JOB_NONE, cert = 0;
    if (job < jobs) job_comb(a, (uint32_t)job, P, pre, cert);
    else ge_p3_identity(P);
    if (nj == 0) zp = P.Z;
    else fe_mul(zp, zp, P.Z);
    pscr_put(slab, lanes, lane, nj, 0, P.X);
    pscr_put(slab, lanes, lane, nj, 2, P.Y);
    pscr_put(slab, lanes, lane, nj, 4, P.Z);
    pscr_put(slab, lanes, lane, nj, 6, zp);
    reinterpret_cast<uint4*>(slab)[((uint64_t)nj * PSCR_ROWS + 8) * lanes + lane] =
        make_uint4(pre, cert, (uint32_t)job, 0);
    nj++;
  }
  if (nj == 0) return;
  fe inv;
  fe_invert(inv, zp);
#pragma unroll 1
  for (int j = nj - 1; j >= 0; j--) {
    fe zinv, x, y, X, Y;
    if (j > 0) {
      fe Z, zprev;
      pscr_get(zprev, slab, lanes, lane, j - 1, 6);
      pscr_get(Z, slab, lanes, lane, j, 4);
      fe_mul(zinv, inv, zprev);
      fe_mul(inv, inv, Z);
    } else {
      zinv = inv;
    }
    pscr_get(X, slab, lanes, lane, j, 0);
    pscr_get(Y, slab, lanes, lane, j, 2);
    const uint4 m = reinterpret_cast<const uint4*>(slab)[((uint64_t)j * PSCR_ROWS + 8) * lanes + lane];
    fe_mul(x, X, zinv);
    fe_mul(y, Y, zinv);
    const uint32_t bits = job_verdict(a, m.z, m.x, x, y);
    if (bits) atomicOr(a.status + m.y, bits);
  }
}

__global__ void __launch_bounds__(256, 2) k_cert_verify(CertArgs a, uint32_t* __restrict__ pscr, uint32_t jcap) {
  if (blockIdx.x < a.hdr_blocks) {  // header digest role, one lane per certificate
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.nc) return;
    header_digest_lane(a.hdr_data, a.hdr_off, a.ids, a.status, c);
    return;
  }
  tp_signature_waves(a, pscr, jcap, (uint64_t)a.nc + a.nv);
}

// Header::verify / Vote::verify crypto of many messages: the throughput
// design above with one strict job per message (MsgArgs, coa_committee.h).
// Headers: the leading blocks check the Header::digest bytes against ids[i]
// (bit 1) beside the signature waves (bit 2).  Votes: no leading blocks; each
// job hashes Vote::digest itself.  A strict verdict depends on no weights,
// so nothing is ever inconclusive: an unregistered author sets
// COA_CST_UNCACHED and nothing else is decided for that job.
__global__ void __launch_bounds__(256, 2) k_msg_verify(MsgArgs a, uint32_t* __restrict__ pscr, uint32_t jcap) {
  if (blockIdx.x < a.hdr_blocks) {  // header digest role, one lane per header
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < a.n) header_digest_lane(a.hdr_data, a.hdr_off, a.ids, a.status, c);
    return;
  }
  tp_signature_waves(a, pscr, jcap, (uint64_t)a.n);
}

// ---------------------------------------------------------------------------
// Grid of the throughput kernel: two waves per SIMD (256 CUs x 4 SIMDs x 2
// x 64 lanes), or one lane per job when there are fewer jobs.
// COA_CERT_LANES_TOTAL overrides (A/B runs).
uint64_t cert_tp_lanes(uint64_t jobs) {
  uint64_t target = 256ull * 4 * 2 * 64;
  if (const char* e = getenv("COA_CERT_LANES_TOTAL")) target = strtoull(e, nullptr, 10);
  if (target < 256) target = 256;
  const uint64_t lanes = jobs < target ? jobs : target;
  return (lanes + 255) / 256 * 256;
}

// Jobs in key order for the throughput kernel.  A chunk of 64 consecutive
// jobs in certificate order holds 64 different keys (a certificate's votes
// come from distinct members), so each of the 13 key-comb additions reads 64
// random entries of 64 different 654 MB combs: half the kernel's requests
// missed the per-CU translation cache (profiles/r05_cert_tlb_pmc.txt).  Sorted
// by key slot, a chunk's lanes read one key's comb.  A counting sort with
// few contended atomics (one global counter per key took 680k of them,
// 0.4 ms): COA_SORT_WGS workgroups each count a contiguous range of jobs
// per slot in LDS (unregistered keys in the last bin), keep the counts
// (counts[wg][bin]) and add them to the bin totals (one atomic per
// workgroup and bin); one block turns the totals into start cursors; each
// workgroup then reserves its range in every bin it uses (one atomic each)
// and places its jobs with LDS counters.  The order inside a bin is
// arbitrary: every job's verdict depends on its own inputs only.
__global__ void __launch_bounds__(256) k_job_count(CertArgs a, uint32_t bins, uint32_t per,
                                                   uint32_t* __restrict__ total, uint32_t* __restrict__ counts,
                                                   uint32_t* __restrict__ bin) {
  __shared__ uint32_t h[COA_SORT_BINS];
  for (uint32_t k = threadIdx.x; k < bins; k += blockDim.x) h[k] = 0;
  __syncthreads();
  const uint64_t jobs = (uint64_t)a.nc + a.nv;
  const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < jobs ? lo + per : jobs;
  for (uint64_t j = lo + threadIdx.x; j < hi; j += blockDim.x) {
    uint32_t pk[8];
    load8(pk, j < a.nc ? a.origins + j * 8 : a.vpks + (j - a.nc) * 8);
    const int slot = key_lookup<kLane>(a.keys, a.nk, pk);
    const uint32_t b = slot < 0 ? a.nk : (uint32_t)slot;
    bin[j] = b;
    atomicAdd(h + b, 1u);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < bins; k += blockDim.x) {
    const uint32_t c = h[k];
    counts[(uint64_t)blockIdx.x * COA_SORT_BINS + k] = c;
    if (c) atomicAdd(total + k, c);
  }
}
// Bin totals -> exclusive start cursors, in place, one block.
__global__ void __launch_bounds__(1024) k_job_scan(uint32_t* __restrict__ v, uint32_t n) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x, per = (n + 1023) / 1024;
  uint32_t mine[COA_SORT_BINS / 1024], sum = 0;
#pragma unroll
  for (uint32_t i = 0; i < COA_SORT_BINS / 1024; i++) {
    const uint32_t k = t * per + i;
    mine[i] = (i < per && k < n) ? v[k] : 0u;
    sum += mine[i];
  }
  part[t] = sum;
  __syncthreads();
  for (uint32_t o = 1; o < 1024; o <<= 1) {  // inclusive scan of the per-thread sums
    const uint32_t x = t >= o ? part[t - o] : 0u;
    __syncthreads();
    part[t] += x;
    __syncthreads();
  }
  uint32_t run = part[t] - sum;  // exclusive start of this thread's bins
#pragma unroll
  for (uint32_t i = 0; i < COA_SORT_BINS / 1024; i++) {
    const uint32_t k = t * per + i;
    if (i < per && k < n) v[k] = run;
    run += mine[i];
  }
}
__global__ void __launch_bounds__(256) k_job_place(uint64_t jobs, uint32_t bins, uint32_t per,
                                                   uint32_t* __restrict__ cursor, const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ bin, uint32_t* __restrict__ perm) {
  __shared__ uint32_t cur[COA_SORT_BINS];
  for (uint32_t k = threadIdx.x; k < bins; k += blockDim.x) {
    const uint32_t c = counts[(uint64_t)blockIdx.x * COA_SORT_BINS + k];
    cur[k] = c ? atomicAdd(cursor + k, c) : 0u;  // this workgroup's range in bin k
  }
  __syncthreads();
  const uint64_t lo = (uint64_t)blockIdx.x * per, hi = lo + per < jobs ? lo + per : jobs;
  for (uint64_t j = lo + threadIdx.x; j < hi; j += blockDim.x) perm[atomicAdd(cur + bin[j], 1u)] = (uint32_t)j;
}

size_t coa_cert_scratch_bytes(uint64_t jobs, bool key_order) {
  return CertScratch(jobs, cert_tp_lanes(jobs ? jobs : 1), true, key_order).bytes;
}

static uint32_t tp_blocks(uint32_t hdr_blocks, uint64_t lanes) { return (uint32_t)(hdr_blocks + lanes / 256); }

hipError_t coa_launch_cert_verify(CertArgs a, int lanes_per_sig, uint32_t* pscr, hipStream_t s) {
  if (lanes_per_sig == 64) return coa_launch_cert_verify_lat(a, s);
  if (a.nc == 0) return hipSuccess;
  a.hdr_blocks = (a.nc + 255) / 256;
  const uint64_t jobs = (uint64_t)a.nc + a.nv;
  const uint64_t lanes = cert_tp_lanes(jobs);
  const CertScratch L(jobs, lanes, true, a.key_order != 0);
  hipError_t e = hipMemsetAsync(pscr + L.ctr, 0, 4, s);  // the chunk counter starts at zero
  if (e != hipSuccess) return e;
  // the prologue pays for its launch when certificates carry many votes (C3:
  // 67 votes, +2-5 %); with few (C1: 3 votes) the digest stays per vote.
  // COA_CERT_DIGEST_PER_VOTE=1 forces per vote (A/B).
  if (a.nv >= 8ull * a.nc && !getenv("COA_CERT_DIGEST_PER_VOTE")) {
    hipLaunchKernelGGL(k_cert_digests, dim3((a.nc + 255) / 256), dim3(256), 0, s, a, pscr + L.cdig);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.cdig = pscr + L.cdig;
  }
  // jobs in key order when the caller asks for it, the committee fits the
  // bins and the call is large enough to pay for the sort
  // (COA_CERT_KEYSORT=0: certificate order everywhere, A/B).  The callers
  // that ask: the device-resident round (+16-18 %) and, since round 6, the
  // queue's windows (COA_QUEUE_KEYSORT, within noise either way:
  // profiles/r06_keysort_ab.txt); not the pipelined host chunks, whose
  // concurrent launches lost more to the sort's own launches than the order
  // gained (profiles/r05_cert_keysort_ab.txt)
  const char* ks = getenv("COA_CERT_KEYSORT");
  if (L.sorts && a.nk > 0 && a.nk + 1 <= COA_SORT_BINS && !(ks && ks[0] == '0' && ks[1] == 0)) {
    uint32_t *total = pscr + L.total, *counts = pscr + L.counts, *bin = pscr + L.bin, *perm = pscr + L.perm;
    const uint32_t bins = a.nk + 1, per = (uint32_t)((jobs + COA_SORT_WGS - 1) / COA_SORT_WGS);
    e = hipMemsetAsync(total, 0, bins * 4, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_job_count, dim3(COA_SORT_WGS), dim3(256), 0, s, a, bins, per, total, counts, bin);
    hipLaunchKernelGGL(k_job_scan, dim3(1), dim3(1024), 0, s, total, bins);
    hipLaunchKernelGGL(k_job_place, dim3(COA_SORT_WGS), dim3(256), 0, s, jobs, bins, per, total, counts, bin, perm);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    a.perm = perm;
  }
  hipLaunchKernelGGL(k_cert_verify, dim3(tp_blocks(a.hdr_blocks, lanes)), dim3(256), 0, s, a, pscr, L.jcap);
  return hipGetLastError();
}

size_t coa_msg_scratch_bytes(uint64_t n) {
  const uint64_t jobs = n ? n : 1;
  return CertScratch(jobs, cert_tp_lanes(jobs), false, false).bytes;
}

// The same grid as the certificates' (cert_tp_lanes); no key-order sort.
hipError_t coa_launch_msg_verify(MsgArgs a, uint32_t* pscr, hipStream_t s) {
  if (a.n == 0) return hipSuccess;
  a.hdr_blocks = a.hdr_data ? (a.n + 255) / 256 : 0;
  const uint64_t lanes = cert_tp_lanes(a.n);
  const CertScratch L(a.n, lanes, false, false);
  hipError_t e = hipMemsetAsync(pscr + L.ctr, 0, 4, s);  // the chunk counter
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_msg_verify, dim3(tp_blocks(a.hdr_blocks, lanes)), dim3(256), 0, s, a, pscr, L.jcap);
  return hipGetLastError();
}

// The registered-key latency job: one signature on three waves of one
// workgroup, each wave's steps written once for k_verify_lat's cached branch
// (coa_latency.hip) and the body of the latency kernels (coa_cert_lat.hip).
//   wave 2  [s]B from B's comb on the rows (rcmp::comb_sum_rows), then
//           publish_sB: into an LDS point and a ready flag
//   wave 0  challenge_bits: k = SHA-512(R || A || M) mod l and the prefix bits
//           from the key's flags; [k](-A) from the key's comb; finish_P: once
//           wave 2 has published, P = [s]B + [k](-A) and the half of the
//           compare that needs only P (coa_rcmp.h), small-order test included.
//           skip instead of all that when the key is not registered
//   wave 1  decide: R's decompression, the compare and the latency rule
//           (coa_job_bits.h); the caller publishes the answer
// The callers keep what differs: where a job's arrays are, its message
// (Certificate::digest, Vote::digest or as given), a window message's protocol
// code, the batch prefilter's torsion term, trace marks, how the answer
// leaves -- and the comb sum between the steps: coa_cert_lat.hip's waves 0 and
// 2 share one inlined copy, k_verify_lat has one per wave (7,000 instructions).
#pragma once
#include "coa_committee.h"
#include "coa_job_bits.h"
#include "coa_rcmp.h"

namespace latjob {

// the LDS the three waves meet in; pt is [s]B in row-limb layout (X, Y, Z, T)
COA_DEV void init(uint32_t* ready, rcmp::Shared& cmp) {
  if (threadIdx.x == 0) {
    *ready = 0;
    cmp.ready = 0;
  }
  __syncthreads();
}

// wave 2: S = [s]B for wave 0
COA_DEV void publish_sB(uint32_t* pt, uint32_t* ready, const rp::P1& S, uint32_t lane) {
  if (lane < 8) {
    pt[lane] = S.X;
    pt[8 + lane] = S.Y;
    pt[16 + lane] = S.Z;
    pt[24 + lane] = S.T;
  }
  if (lane == 0) __hip_atomic_store(ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// wave 0, once msg is what was signed: k into dg, and the job's prefix bits
// from s, the key's flags kf and the job's own bits (COA_JOB_STRICT)
COA_DEV uint32_t challenge_bits(uint32_t* dg, const uint32_t* rw, const uint32_t* pk, const uint32_t* sw,
                                const uint32_t* msg, uint32_t kf, uint32_t extra) {
  sc k;
  coa_kc::challenge(k, rw, pk, msg);
#pragma unroll
  for (int i = 0; i < 8; i++) dg[i] = k.v[i];
  return (sc_is_canonical(sw) ? 0u : COA_JOB_S) | ((kf & COA_KEY_DECOMPRESSES) ? 0u : COA_JOB_A) |
         ((kf & COA_KEY_SMALL_ORDER) ? COA_JOB_SMALL_A : 0u) | ((kf & COA_KEY_TORSION_FREE) ? 0u : COA_JOB_TORSION) |
         extra;
}

// wave 0 with P = [k](-A): everything that needs only P while wave 1 still
// decompresses R (the critical chain): P = [s]B + [k](-A) once wave 2 has
// published [s]B, verify_strict's small-order test of R taken on P (an
// accepting verdict needs R == P, every other strict verdict is Err already),
// the compare's P half.  code: see coa_job_word.
COA_DEV void finish_P(rcmp::Shared& cmp, const uint32_t* pt, uint32_t* ready, rp::P1& P, const uint32_t* rw,
                      uint32_t pre, uint32_t code, uint32_t lane) {
#pragma unroll 1
  while (__hip_atomic_load(ready, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) __builtin_amdgcn_s_sleep(1);
  rp::P1 S;
  S.X = rp::ld(pt);
  S.Y = rp::ld(pt + 8);
  S.Z = rp::ld(pt + 16);
  S.T = rp::ld(pt + 24);
  rcmp::add_rows(P, P, S);
  rcmp::prepare_rows(cmp, P, rw, coa_job_word(0, pre, code), (pre & COA_JOB_STRICT) ? COA_JOB_WORD_SMALL_P : 0u,
                     lane == 0);
}

// wave 0, key not registered: nothing to compare, only the code travels
COA_DEV void skip(rcmp::Shared& cmp, uint32_t code, uint32_t lane) {
  rcmp::skip(cmp, coa_job_word(COA_CST_UNCACHED, 0, code), lane == 0);
}

// wave 1: the job's COA_CST_* bits; `word` is what wave 0 handed over.
// chain_done() and compared() run after the power chain and after the compare
// (trace marks).
template <class ChainDone, class Compared>
COA_DEV uint32_t decide(const rcmp::Shared& cmp, const uint32_t* rw, uint32_t& word, ChainDone chain_done,
                        Compared compared) {
  const uint32_t res = rcmp::decompress_eq(cmp, rw, word, chain_done);
  compared();
  if (coa_job_status(word) & COA_CST_UNCACHED) return COA_CST_UNCACHED;
  return coa_rule_latency(coa_job_pre(word), (res & rcmp::R_DECOMPRESSES) != 0, (res & rcmp::R_EQUALS_P) != 0);
}

}  // namespace latjob

// One signature job of the committee kernels (a header signature, a vote, a
// message, a single verify on a registered key): its prefix bits, the word
// that carries them between the waves of a latency job, and the two accept
// rules.  Plain C++ and also compiled for the device (COA_HD, as
// coa_protocol.h), so tests/test_job_rules_host.py builds it with plain g++.
#pragma once
#include <stdint.h>

#include "coa_stage.h"  // COA_CST_*

#ifndef COA_HD
#if defined(__HIPCC__)
#define COA_HD __host__ __device__ inline
#else
#define COA_HD inline
#endif
#endif

// What is known of a job before P = [s]B + [k](-A) is compared with R.
enum CoaJobBit : uint32_t {
  COA_JOB_S = 1u,          // s >= l (not canonical)
  COA_JOB_A = 2u,          // A does not decompress
  COA_JOB_SMALL_A = 4u,    // [8]A == O
  COA_JOB_TORSION = 8u,    // [l]A != O
  COA_JOB_STRICT = 16u,    // dalek's verify_strict decides (a header signature, a message, a single verify)
  COA_JOB_UNCACHED = 32u,  // the key is not registered: nothing was computed
  COA_JOB_NONE = 64u,      // no job (the tail of the last chunk)
  COA_JOB_SMALL_P = 128u   // P has small order; read only beside P == R, where it is R's small order
};

// The word wave 0 of a latency job hands to wave 1 (rcmp::Shared::bits):
// status bits (COA_CST_*; only COA_CST_UNCACHED travels) in 0-7, prefix bits
// in 8-15, the message's protocol code (k_msg_verdict_lat, else 0) in 16-23.
COA_HD uint32_t coa_job_word(uint32_t status, uint32_t pre, uint32_t code) {
  return (status & 0xffu) | ((pre & 0xffu) << 8) | ((code & 0xffu) << 16);
}
COA_HD uint32_t coa_job_status(uint32_t word) { return word & 0xffu; }
COA_HD uint32_t coa_job_pre(uint32_t word) { return (word >> 8) & 0xffu; }
COA_HD uint32_t coa_job_code(uint32_t word) { return (word >> 16) & 0xffu; }
// P's half of the compare found P of small order (rcmp::prepare_rows ORs it in)
#define COA_JOB_WORD_SMALL_P ((uint32_t)COA_JOB_SMALL_P << 8)

// Both rules answer COA_CST_* bits; 0 accepts.  `eq`: decompress(R) == P.
//
// Latency rule (one workgroup per job; wave 1 decompresses R itself, so
// `r_ok`, decompress(R) is Some, is known).  strict: s < l, A and R
// decompress, neither of small order, P == R.  vote: s >= l, A or R not
// decompressing is dalek's definitive Err; else the vote passes for every
// batch weight iff P == R and A is torsion free, and anything else is left to
// the exact batch kernels.  The throughput rule below has no r_ok: it leaves a
// malformed R open where this one says Err at once; the host resolves every
// open certificate exactly, so both end in the same COA_CERT_* answer.
COA_HD uint32_t coa_rule_latency(uint32_t pre, bool r_ok, bool eq) {
  if (pre & (COA_JOB_NONE | COA_JOB_UNCACHED)) return (pre & COA_JOB_UNCACHED) ? COA_CST_UNCACHED : 0u;
  if (pre & COA_JOB_STRICT)
    return (!(pre & (COA_JOB_S | COA_JOB_A | COA_JOB_SMALL_A | COA_JOB_SMALL_P)) && r_ok && eq) ? 0u
                                                                                                 : COA_CST_BAD_HEADER_SIG;
  if ((pre & (COA_JOB_S | COA_JOB_A)) || !r_ok) return COA_CST_BAD_VOTES;
  return (eq && !(pre & COA_JOB_TORSION)) ? 0u : COA_CST_VOTES_INCONCLUSIVE;
}

// Throughput rule (one lane per job; R is never decompressed: P's affine
// coordinates are compared with R's encoding, and P == R proves that R
// decompresses).  With P != R nothing says whether R decompresses (Err) or
// differs from P by a torsion point (a weight-dependent verdict), so a vote is
// COA_CST_VOTES_INCONCLUSIVE and the host's exact batch path decides: the one
// difference from the latency rule, gone after the host's resolution.  A
// strict job needs no such care: P != R is Err whatever R is.
COA_HD uint32_t coa_rule_throughput(uint32_t pre, bool eq) {
  if (pre & (COA_JOB_NONE | COA_JOB_UNCACHED)) return (pre & COA_JOB_UNCACHED) ? COA_CST_UNCACHED : 0u;
  if (pre & COA_JOB_STRICT)
    return (!(pre & (COA_JOB_S | COA_JOB_A | COA_JOB_SMALL_A | COA_JOB_SMALL_P)) && eq) ? 0u : COA_CST_BAD_HEADER_SIG;
  if (pre & (COA_JOB_S | COA_JOB_A)) return COA_CST_BAD_VOTES;
  return (eq && !(pre & COA_JOB_TORSION)) ? 0u : COA_CST_VOTES_INCONCLUSIVE;
}

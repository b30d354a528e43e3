// The workspace of coa_certificate_votes_resolve_device as one layout: what
// coa_certificate_votes_resolve_workspace_bytes sizes and what the launcher
// carves (coa_resolve.hip).  Host code only (no HIP), so
// tests/test_votes_resolve_host.py builds it with plain g++.
#pragma once
#include <cstddef>
#include <cstdint>

// most lanes of the term grid: two 256-lane blocks on each of 256 CUs
// (k_resolve_terms' launch bounds); each owns 2 KiB of term scratch
#define COA_RESOLVE_MAX_LANES (256u * 2u * 256u)
#define COA_RESOLVE_SCRATCH_PER_LANE 2048  // COA_BATCH_SCRATCH_PER_LANE (coa_batch.h)
#define COA_RESOLVE_COUNT_WORDS 4          // found, resolved, votes, unused

// count words | open certificate indices [n] | exclusive vote prefix of the
// open certificates [n + 1] | per open vote, `cap` of them: challenge k (32 B),
// weight z (16 B), term (128 B), flag (1 B) | term scratch (2 KiB per lane).
// Byte offsets from the workspace pointer; every section starts on 256 bytes
// (its widest access is a uint4; the scratch is read by 128-byte lines).
// Certificate::digest needs no section: the prepare kernel hands it from the
// lane that hashes it to the certificate's other votes through LDS.
struct ResolveWs {
  uint32_t cap;    // open votes one call resolves at most
  uint32_t lanes;  // lanes of the term grid
  size_t counts = 0, idx = 0, pre = 0, k = 0, z = 0, terms = 0, flags = 0, scr = 0;
  size_t bytes = 0;

  static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }

  // open_votes_cap 0 (or more than the call has votes): every vote
  ResolveWs(uint64_t n, uint64_t n_votes, uint64_t open_votes_cap) {
    cap = (uint32_t)((open_votes_cap == 0 || open_votes_cap > n_votes) ? n_votes : open_votes_cap);
    const uint64_t want = ((uint64_t)(cap ? cap : 1) + 255) / 256 * 256;
    lanes = (uint32_t)(want < COA_RESOLVE_MAX_LANES ? want : COA_RESOLVE_MAX_LANES);
    size_t end = 0;
    auto take = [&end](size_t bytes_) {
      const size_t at = end;
      end = up(at + bytes_);
      return at;
    };
    counts = take(COA_RESOLVE_COUNT_WORDS * 4);
    idx = take((size_t)n * 4);
    pre = take(((size_t)n + 1) * 4);
    k = take((size_t)cap * 32);
    z = take((size_t)cap * 16);
    terms = take((size_t)cap * 128);
    flags = take((size_t)cap);
    scr = take((size_t)lanes * COA_RESOLVE_SCRATCH_PER_LANE);
    bytes = end;
  }
};

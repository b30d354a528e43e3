// Internal launch wrapper of the device-side resolution of open certificates
// (coa_resolve.hip); the workspace layout is coa_resolve_ws.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct ResolveArgs {
  const uint32_t* ids;      // n * 8 words
  const uint32_t* origins;  // n * 8 words
  const uint64_t* rounds;   // n
  const uint8_t* vpks;      // n_votes * 32
  const uint8_t* vsigs;     // n_votes * 64
  const uint64_t* voff;     // n + 1
  const uint32_t* zs;       // n_votes * 4 words, or null: derived from seed
  uint64_t seed;
  uint32_t n, n_votes, cap;  // cap: the call's open_votes_cap (0 = n_votes)
  uint32_t* verdicts;        // n words, updated in place
  uint32_t* counts_out;      // 3 words or null
};

// k_open_scan, k_resolve_prepare, k_resolve_terms and k_resolve_sum on s, over
// workspace ws laid out as ResolveWs(a.n, a.n_votes, a.cap); btab is the
// context's fixed-base table of B.
hipError_t coa_launch_votes_resolve(const ResolveArgs& a, uint8_t* ws, const uint32_t* btab, hipStream_t s);

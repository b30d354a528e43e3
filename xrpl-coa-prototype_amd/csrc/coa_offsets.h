// Small host-only pieces the entries share (no HIP): the checks and copies of
// the caller's offset arrays, and the 72-byte Certificate::digest /
// Vote::digest input.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace coa_rt __attribute__((visibility("hidden"))) {

// off[0] <= off[1] <= ... <= off[n] (n + 1 entries).
inline bool offsets_monotone(const uint64_t* off, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}

// off[lo..hi] rebased so that the first is 0: the offsets of items [lo, hi)
// within their own slice of the data.
inline std::vector<uint64_t> rebased_offsets(const uint64_t* off, size_t lo, size_t hi) {
  std::vector<uint64_t> rel(hi - lo + 1);
  for (size_t k = 0; k <= hi - lo; k++) rel[k] = off[lo + k] - off[lo];
  return rel;
}

// id || round LE || origin: what Certificate::digest and Vote::digest hash.
constexpr size_t kDigestInput = 72;
inline void digest_input(uint8_t* out, const uint8_t* id, uint64_t round, const uint8_t* origin) {
  std::memcpy(out, id, 32);
  for (int b = 0; b < 8; b++) out[32 + b] = (uint8_t)(round >> (8 * b));
  std::memcpy(out + 40, origin, 32);
}

}  // namespace coa_rt

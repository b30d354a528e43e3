// Host check of the workspace layout of coa_certificate_votes_resolve_device
// (xrpl-coa-prototype_amd/csrc/coa_resolve_ws.h), built with
// -fsanitize=address,undefined by tests/test_votes_resolve_host.py: over
// n in {1, 2, 255, 256, 257, 10,000}, votes in {0, 1, 67 n} and caps in
// {0, 1, votes} the sections are disjoint, each is aligned for its widest
// access and holds what the kernels put there, and all lie within `bytes`.
// A buffer of `bytes` bytes is then written at each section's first and last
// byte, so an overrun is the sanitizer's to report.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "coa_resolve_ws.h"

struct Sec {
  const char* name;
  size_t at, bytes, align;
};

static int check(uint64_t n, uint64_t votes, uint64_t cap_in) {
  const ResolveWs w(n, votes, cap_in);
  const uint64_t cap = (cap_in == 0 || cap_in > votes) ? votes : cap_in;
  int bad = 0;
  auto fail = [&](const char* what, const char* sec) {
    std::printf("FAIL n=%llu votes=%llu cap=%llu: %s (%s)\n", (unsigned long long)n, (unsigned long long)votes,
                (unsigned long long)cap_in, what, sec);
    bad++;
  };
  if (w.cap != cap) fail("cap", "-");
  if (w.lanes % 256 || w.lanes < 256 || w.lanes > COA_RESOLVE_MAX_LANES) fail("lanes", "-");
  if (w.lanes < std::min<uint64_t>((cap + 255) / 256 * 256, COA_RESOLVE_MAX_LANES)) fail("lanes below the cap", "-");
  // name, offset, bytes the kernels touch, alignment of the widest access
  // (uint4 = 16; the scratch is read by 128-byte lines; count words as dwords)
  const Sec secs[] = {
      {"counts", w.counts, 4 * 4, 4},          {"idx", w.idx, (size_t)n * 4, 4},
      {"pre", w.pre, ((size_t)n + 1) * 4, 4},  {"k", w.k, (size_t)cap * 32, 16},
      {"z", w.z, (size_t)cap * 16, 16},        {"terms", w.terms, (size_t)cap * 128, 16},
      {"flags", w.flags, (size_t)cap, 1},      {"scr", w.scr, (size_t)w.lanes * 2048, 128},
  };
  const size_t ns = sizeof(secs) / sizeof(secs[0]);
  for (size_t i = 0; i < ns; i++) {
    if (secs[i].at % secs[i].align) fail("alignment", secs[i].name);
    if (secs[i].at + secs[i].bytes > w.bytes) fail("past the reported size", secs[i].name);
    for (size_t j = i + 1; j < ns; j++) {
      const bool apart = secs[i].at + secs[i].bytes <= secs[j].at || secs[j].at + secs[j].bytes <= secs[i].at;
      if (!apart) fail("overlap", secs[j].name);
    }
  }
  if (bad) return bad;
  // untouched pages cost nothing: only the sections' ends are written
  uint8_t* buf = static_cast<uint8_t*>(std::malloc(w.bytes));
  if (!buf) return bad + 1;
  for (size_t i = 0; i < ns; i++) {
    if (!secs[i].bytes) continue;
    buf[secs[i].at] = 1;
    buf[secs[i].at + secs[i].bytes - 1] = 1;
  }
  std::free(buf);
  return bad;
}

int main() {
  const uint64_t ns[] = {1, 2, 255, 256, 257, 10000};
  int bad = 0, cases = 0;
  for (uint64_t n : ns) {
    const uint64_t vs[] = {0, 1, 67 * n};
    for (uint64_t v : vs) {
      const uint64_t caps[] = {0, 1, v};
      for (uint64_t c : caps) {
        bad += check(n, v, c);
        cases++;
      }
    }
  }
  std::printf("%s %d cases\n", bad ? "BAD" : "ok", cases);
  return bad ? 1 : 0;
}

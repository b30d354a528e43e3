// The host-only part of the wire decoder's mixed mode
// (xrpl-coa-prototype_amd/csrc/coa_wire_mixed.h) under ASan + UBSan: the
// workspace layout and the partition / scatter pair that
// coa_cpu_wire_verdict_many runs and the device's six prefix sums restate.
// Built and run by tests/test_wire_mixed_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "coa_wire_mixed.h"

static int fails = 0, cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);                  \
      fails++;                                                             \
    }                                                                      \
  } while (0)

static void layout(uint64_t n) {
  cases++;
  const WireMixedWs L(n);
  const size_t blocks = (size_t)((n + 255) / 256);
  CHECK(L.blocks == blocks);
  // sections in order, each on 256 bytes, each as long as what it holds
  CHECK(L.hb == 0);
  CHECK(L.hb % 256 == 0 && L.nv % 256 == 0 && L.bt % 256 == 0 && L.bytes % 256 == 0);
  CHECK(L.hb + n * 8 <= L.nv);
  CHECK(L.nv + n * 8 <= L.bt);
  CHECK(L.bt + blocks * COA_WIRE_MIXED_SUMS * 8 <= L.bytes);
  CHECK(L.bytes > 0);  // never a zero-byte allocation
  // no slack beyond the alignment
  CHECK(L.nv - L.hb < n * 8 + 256 && L.bt - L.nv < n * 8 + 256);
  CHECK(L.bytes - L.bt < (blocks ? blocks : 1) * COA_WIRE_MIXED_SUMS * 8 + 256);
  // touch every byte a kernel may: the sections are inside the allocation and disjoint
  std::vector<uint8_t> ws(L.bytes, 0);
  for (size_t i = 0; i < n * 8; i++) ws[L.hb + i]++;
  for (size_t i = 0; i < n * 8; i++) ws[L.nv + i]++;
  for (size_t i = 0; i < blocks * COA_WIRE_MIXED_SUMS * 8; i++) ws[L.bt + i]++;
  bool once = true;
  for (uint8_t b : ws) once = once && b <= 1;
  CHECK(once);
}

// The partition of `kinds` against its definition, and scatter o partition.
static void partition(const std::vector<int32_t>& kinds) {
  cases++;
  const size_t n = kinds.size();
  std::vector<uint32_t> slots(n + 1, 0x5a5a5a5au);
  size_t count[COA_WIRE_MIXED_KINDS];
  const size_t none = coa_wire_mixed_partition(kinds.data(), n, slots.data(), count);
  CHECK(slots[n] == 0x5a5a5a5au);
  size_t seen[COA_WIRE_MIXED_KINDS] = {0, 0, 0}, without = 0;
  for (size_t i = 0; i < n; i++) {
    const int32_t k = kinds[i];
    if (k == 0 || k == 1 || k == 2) {
      CHECK(slots[i] == seen[k]);  // the rank among the frames of its kind, in frame order: stable
      seen[k]++;
    } else {
      CHECK(slots[i] == COA_WIRE_NO_SLOT);
      without++;
    }
  }
  for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) CHECK(count[k] == seen[k]);
  CHECK(none == without && none + count[0] + count[1] + count[2] == n);
  // each kind's words name the frame they belong to; the scatter brings every frame its own
  std::vector<uint32_t> words[COA_WIRE_MIXED_KINDS];
  for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) words[k].assign(count[k], 0);
  for (size_t i = 0; i < n; i++)
    if (slots[i] != COA_WIRE_NO_SLOT) words[kinds[i]][slots[i]] = (uint32_t)(i + 1000);
  const uint32_t* by_kind[COA_WIRE_MIXED_KINDS] = {count[0] ? words[0].data() : nullptr, count[1] ? words[1].data() : nullptr,
                                                   count[2] ? words[2].data() : nullptr};
  std::vector<uint32_t> out(n + 1, 0x5a5a5a5au);
  coa_wire_mixed_scatter(kinds.data(), slots.data(), n, by_kind, 255u, out.data());
  CHECK(out[n] == 0x5a5a5a5au);
  for (size_t i = 0; i < n; i++) CHECK(out[i] == (slots[i] == COA_WIRE_NO_SLOT ? 255u : (uint32_t)(i + 1000)));
}

int main() {
  for (uint64_t n : {0ull, 1ull, 255ull, 256ull, 257ull, 65536ull, 65537ull}) layout(n);
  // monotone in n
  size_t prev = 0;
  for (uint64_t n = 0; n < 2000; n++) {
    const size_t b = WireMixedWs(n).bytes;
    CHECK(b >= prev);
    prev = b;
  }
  cases++;

  const int32_t all[] = {0, 1, 2, 3, -10, -11, -12, -13};
  partition({});
  for (int32_t k : all) partition(std::vector<int32_t>(300, k));  // one kind; no kind at all for the last five
  for (int a = 0; a < 8; a++)
    for (int b = 0; b < 8; b++) {
      std::vector<int32_t> v(513);
      for (size_t i = 0; i < v.size(); i++) v[i] = i % 2 ? all[a] : all[b];  // alternating
      partition(v);
    }
  std::mt19937 rng(7);
  for (int round = 0; round < 40; round++) {
    std::vector<int32_t> v(rng() % 3000);
    const unsigned span = 1 + rng() % 8;
    for (auto& k : v) k = all[rng() % span];
    partition(v);
  }
  if (fails) {
    std::printf("%d failures\n", fails);
    return 1;
  }
  std::printf("ok %d cases\n", cases);
  return 0;
}

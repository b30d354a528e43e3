// The host-only part of the device wire decoder
// (xrpl-coa-prototype_amd/csrc/coa_wire_layout.h) under ASan + UBSan: the
// workspace layout of both modes, the device block of the frames-to-verdicts
// calls, and the partition / scatter pair that coa_cpu_wire_verdict_many runs
// and the device's six prefix sums restate.
// Built and run by tests/test_wire_mixed_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "coa_wire_layout.h"

static int fails = 0, cases = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAIL line %d: %s\n", __LINE__, #cond);                  \
      fails++;                                                             \
    }                                                                      \
  } while (0)

static void layout(uint64_t n, int sums) {
  cases++;
  const WireWs L(n, sums);
  const size_t blocks = (size_t)((n + 255) / 256);
  CHECK(L.blocks == blocks);
  // sections in order, each on 256 bytes, each as long as what it holds
  CHECK(L.hb == 0);
  CHECK(L.hb % 256 == 0 && L.nv % 256 == 0 && L.bt % 256 == 0 && L.bytes % 256 == 0);
  CHECK(L.hb + n * 8 <= L.nv);
  CHECK(L.nv + n * 8 <= L.bt);
  CHECK(L.bt + blocks * sums * 8 <= L.bytes);
  CHECK(L.bytes > 0);  // never a zero-byte allocation
  // no slack beyond the alignment
  CHECK(L.nv - L.hb < n * 8 + 256 && L.bt - L.nv < n * 8 + 256);
  CHECK(L.bytes - L.bt < (blocks ? blocks : 1) * sums * 8 + 256);
  // touch every byte a kernel may: the sections are inside the allocation and disjoint
  std::vector<uint8_t> ws(L.bytes, 0);
  for (size_t i = 0; i < n * 8; i++) ws[L.hb + i]++;
  for (size_t i = 0; i < n * 8; i++) ws[L.nv + i]++;
  for (size_t i = 0; i < blocks * sums * 8; i++) ws[L.bt + i]++;
  bool once = true;
  for (uint8_t b : ws) once = once && b <= 1;
  CHECK(once);
}

// What a set of each kind holds, stated apart from coa_wire_set_has: a vote has
// no header data, offsets or payload counts and alone has origins; only a
// certificate has vote arrays.  Columns in the order of the section enum.
static const bool kHas[COA_WIRE_MIXED_KINDS][wWords] = {
    {1, 1, 1, 1, 0, 1, 1, 1, 0, 0, 0},   // header
    {0, 0, 1, 1, 1, 1, 1, 0, 0, 0, 0},   // vote
    {1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1}};  // certificate

struct Section {
  size_t at, cap;  // the bytes a copy or a kernel may write at the stated capacities
};

// The device block of a fused call over n frames of fb bytes for the kinds of mask.
static size_t block(size_t n, size_t fb, unsigned mask) {
  cases++;
  const WireBlock L(n, fb, mask);
  const bool mixed = mask == 7;
  CHECK(L.mixed == mixed);
  const size_t votes = fb / 115;
  const size_t cap[wWords] = {fb + 16, (n + 1) * 8, n * 32,          n * 32,          n * 32,     n * 64,
                              n * 8,   n * 4,       votes * 32 + 16, votes * 64 + 16, (n + 1) * 8};
  // the sections in their stated order
  std::vector<Section> sec = {{L.offs, (n + 1) * 8}, {L.frames, fb}};
  for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) {
    for (int j = 0; j < wWords; j++) {
      const bool has = (mask >> k & 1) && kHas[k][j];
      CHECK((L.set[k][j] != WireBlock::kNone) == has);  // exactly what the rule gives
      if (has) sec.push_back({L.set[k][j], cap[j]});
    }
    // per-kind words only where the items are not the frames; else the frame-order words
    if (mixed) sec.push_back({L.set[k][wWords], n * 4});
    else CHECK(L.set[k][wWords] == (mask >> k & 1 ? L.words : WireBlock::kNone));
  }
  CHECK(L.ntotals == (mixed ? (size_t)COA_WIRE_MIXED_TOTALS : 4u));
  sec.push_back({L.totals, L.ntotals * 8});
  CHECK((L.slots != WireBlock::kNone) == mixed);
  if (mixed) sec.push_back({L.slots, n * 4});
  sec.push_back({L.kinds, n * 4});
  sec.push_back({L.words, n * 4});
  sec.push_back({L.ws, WireWs(n, mixed ? COA_WIRE_MIXED_SUMS : 3).bytes});
  // every section on 256 bytes, inside the block, after the one before it
  CHECK(L.offs == 0 && L.bytes % 256 == 0);
  for (size_t i = 0; i < sec.size(); i++) {
    CHECK(sec[i].at % 256 == 0 && sec[i].at + sec[i].cap <= L.bytes);
    if (i) CHECK(sec[i].at >= sec[i - 1].at + sec[i - 1].cap && sec[i].at < sec[i - 1].at + sec[i - 1].cap + 256 + 4);
  }
  CHECK(L.bytes - (L.ws + sec.back().cap) < 256);
  // touch every byte once: the sections are pairwise disjoint
  std::vector<uint8_t> blk(L.bytes, 0);
  for (const Section& x : sec)
    for (size_t i = 0; i < x.cap; i++) blk[x.at + i]++;
  bool once = true;
  for (uint8_t b : blk) once = once && b <= 1;
  CHECK(once);
  // the upload: the offsets and fb frame bytes, and nothing else
  CHECK(L.upload == L.frames + fb && L.offs + (n + 1) * 8 <= L.frames);
  for (size_t i = 2; i < sec.size(); i++) CHECK(sec[i].at >= L.upload);
  // the download: kinds and words side by side, and nothing else
  CHECK(L.words == L.kinds + ((n * 4 + 255) & ~(size_t)255));
  CHECK(L.download == L.words + n * 4 - L.kinds);
  for (size_t i = 0; i < sec.size(); i++)
    CHECK(sec[i].at == L.kinds || sec[i].at == L.words || sec[i].at + sec[i].cap <= L.kinds ||
          sec[i].at >= L.kinds + L.download);
  return L.bytes;
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
  for (int sums : {3, COA_WIRE_MIXED_SUMS}) {
    for (uint64_t n : {0ull, 1ull, 255ull, 256ull, 257ull, 65536ull, 65537ull}) layout(n, sums);
    // monotone in n
    size_t prev = 0;
    for (uint64_t n = 0; n < 2000; n++) {
      const size_t b = WireWs(n, sums).bytes;
      CHECK(b >= prev);
      prev = b;
    }
    cases++;
  }
  CHECK(WireWs(65536, 3).bytes == 2 * 65536 * 8 + 256 * 3 * 8 && WireWs(65536, 6).bytes == 2 * 65536 * 8 + 256 * 6 * 8);

  const size_t ns[] = {1, 255, 256, 257, 65537}, fbs[] = {0, 1, 115, 12288, 1 << 20};
  const unsigned masks[] = {1u << COA_MSG_HEADER, 1u << COA_MSG_VOTE, 1u << COA_MSG_CERTIFICATE, 7u};
  for (size_t n : ns)
    for (size_t fb : fbs) {
      size_t bytes[4];
      for (int m = 0; m < 4; m++) bytes[m] = block(n, fb, masks[m]);
      for (int m = 0; m < 3; m++) CHECK(bytes[3] >= bytes[m]);  // all three need no less than any one
    }
  // monotone in n and in the frames' bytes
  for (unsigned mask : masks) {
    cases++;
    for (size_t fb : fbs) {
      size_t prev = 0;
      for (size_t n = 1; n < 70000; n = n < 600 ? n + 1 : n + 997) {
        const size_t b = WireBlock(n, fb, mask).bytes;
        CHECK(b >= prev);
        prev = b;
      }
    }
    for (size_t n : ns) {
      size_t prev = 0;
      for (size_t fb = 0; fb < (1 << 20) + 600; fb = fb < 600 ? fb + 1 : fb + 4099) {
        const size_t b = WireBlock(n, fb, mask).bytes;
        CHECK(b >= prev);
        prev = b;
      }
    }
  }

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

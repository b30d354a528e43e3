// Where the device wire decoder's host side (coa_wire_dev.cpp) puts things,
// for the single-kind and the mixed mode alike (include/coa_verify.h, "wire
// decode on the device", "mixed frame batches"): the decoder's workspace, the
// device block of a frames-to-verdicts call, and the partition of a batch by
// kind as the host does it, which coa_cpu_wire_verdict_many runs and which
// states what the device's six prefix sums (coa_wire_dev.hip) must produce.
// Host code only (no HIP), so tests/sanitize/wire_mixed_driver.cpp builds it
// with plain g++.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/coa_verify.h"

#define COA_WIRE_SCAN_BLOCK 256u  // frames per block of the prefix-sum kernels
#define COA_WIRE_MIXED_SUMS 6        // headers, their bytes | votes | certificates, their bytes, their votes
#define COA_WIRE_MIXED_TOTALS 8      // the six sums, frames without a slot, 0
#define COA_WIRE_NO_SLOT 0xFFFFFFFFu
#define COA_WIRE_MIXED_KINDS 3       // COA_MSG_HEADER, COA_MSG_VOTE, COA_MSG_CERTIFICATE: 0, 1, 2

inline size_t coa_wire_up(size_t x) { return (x + 255) & ~(size_t)255; }

// per-frame header bytes [n] | per-frame votes [n] | `sums` block totals per
// COA_WIRE_SCAN_BLOCK frames: 3 for one kind (header bytes, votes, frames of
// the kind), COA_WIRE_MIXED_SUMS for the mixed mode.  Byte offsets from the
// workspace pointer, every section on 256 bytes.  The frames' size does not
// enter: nothing per byte is kept between the passes.
struct WireWs {
  size_t hb = 0, nv = 0, bt = 0, bytes = 0;
  uint32_t blocks = 0;
  WireWs(uint64_t n, int sums) {
    blocks = (uint32_t)((n + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK);
    nv = hb + coa_wire_up((size_t)n * 8);
    bt = nv + coa_wire_up((size_t)n * 8);
    bytes = bt + coa_wire_up((size_t)(blocks ? blocks : 1) * sums * 8);
  }
};

// One kind's arrays in the device block; wWords only in a mixed block, whose
// verdict words are per item until the scatter.
enum { wHdata, wHoff, wIds, wAuthors, wOrigins, wSigs, wRounds, wPcounts, wVpks, wVsigs, wVoff, wWords, wSetSections };

// A vote has no header data, offsets or payload counts (and alone has
// origins); only a certificate has vote arrays.
inline bool coa_wire_set_has(int kind, int sec) {
  switch (sec) {
    case wHdata: case wHoff: case wPcounts: return kind != COA_MSG_VOTE;
    case wOrigins: return kind == COA_MSG_VOTE;
    case wVpks: case wVsigs: case wVoff: return kind == COA_MSG_CERTIFICATE;
    default: return true;
  }
}

// The layout of the fused device block for n frames of frame_bytes bytes and
// the kinds of `mask` (bit k: kind k): offsets | frames | one array set per
// requested kind at the capacities coa_verify.h states | totals | slots and
// per-kind words (more than one kind only) | kinds | words in frame order |
// the decoder's workspace.  Byte offsets, every section on 256 bytes, kNone
// for a section the block lacks.  One H2D brings [0, upload), one D2H returns
// [kinds, kinds + download).
struct WireBlock {
  static constexpr size_t kNone = ~(size_t)0;
  bool mixed = false;
  size_t offs = 0, frames = 0, set[COA_WIRE_MIXED_KINDS][wSetSections], totals = 0, ntotals = 0, slots = kNone, kinds = 0,
         words = 0, ws = 0, bytes = 0, upload = 0, download = 0;
  WireBlock(size_t n, size_t fb, unsigned mask) : mixed((mask & (mask - 1)) != 0) {
    size_t end = 0;
    auto take = [&end](size_t b) {
      const size_t at = end;
      end = coa_wire_up(at + b);
      return at;
    };
    offs = take((n + 1) * 8);
    frames = take(fb + 4);
    upload = frames + fb;
    const size_t votes = COA_WIRE_VOTES_BOUND(fb);
    const size_t cap[wSetSections] = {fb + 16, (n + 1) * 8, n * 32,          n * 32,          n * 32,      n * 64,
                                      n * 8,   n * 4,       votes * 32 + 16, votes * 64 + 16, (n + 1) * 8, n * 4};
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++)
      for (int sec = 0; sec < wSetSections; sec++)
        set[k][sec] = ((mask >> k) & 1) && coa_wire_set_has(k, sec) && (mixed || sec != wWords) ? take(cap[sec]) : kNone;
    ntotals = mixed ? COA_WIRE_MIXED_TOTALS : 4;
    totals = take(ntotals * 8);
    if (mixed) slots = take(n * 4);
    kinds = take(n * 4);
    words = take(n * 4);
    download = words - kinds + n * 4;
    ws = take(WireWs(n, mixed ? COA_WIRE_MIXED_SUMS : 3).bytes);
    bytes = end;
    // one kind: item i is frame i, so its verdict call writes the frame-order words
    if (!mixed)
      for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++)
        if ((mask >> k) & 1) set[k][wWords] = words;
  }
};

// A frame's kind has a slot when it is one of the three message kinds the
// verdict calls take; a certificate request, a negative COA_WIRE_E* and
// COA_WIRE_ECAPACITY have none.
inline bool coa_wire_mixed_has_slot(int32_t kind) { return kind >= 0 && kind < COA_WIRE_MIXED_KINDS; }

// The stable partition: slots[i] = the rank of frame i among the frames of its
// kind, in frame order, or COA_WIRE_NO_SLOT; counts[k] = frames of kind k.
// Returns the number of frames without a slot.
inline size_t coa_wire_mixed_partition(const int32_t* kinds, size_t n, uint32_t* slots,
                                       size_t counts[COA_WIRE_MIXED_KINDS]) {
  size_t none = 0;
  for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) counts[k] = 0;
  for (size_t i = 0; i < n; i++) {
    if (coa_wire_mixed_has_slot(kinds[i])) {
      slots[i] = (uint32_t)counts[kinds[i]]++;
    } else {
      slots[i] = COA_WIRE_NO_SLOT;
      none++;
    }
  }
  return none;
}

// out[i] = the word of item slots[i] in the words of frame i's kind; `none`
// where the frame has no slot.  words[k] may be null when no frame is of kind k.
inline void coa_wire_mixed_scatter(const int32_t* kinds, const uint32_t* slots, size_t n,
                                   const uint32_t* const words[COA_WIRE_MIXED_KINDS], uint32_t none, uint32_t* out) {
  for (size_t i = 0; i < n; i++) out[i] = slots[i] == COA_WIRE_NO_SLOT ? none : words[kinds[i]][slots[i]];
}

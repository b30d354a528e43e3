// The mixed mode of the wire decoder (include/coa_verify.h, "mixed frame
// batches"): the workspace of coa_wire_decode_mixed_device as one layout --
// what coa_wire_mixed_workspace_bytes sizes and what the launcher carves
// (coa_wire_dev.cpp) -- and the partition of a batch by kind as the host does
// it, which coa_cpu_wire_verdict_many runs and which states what the device's
// six prefix sums (coa_wire_dev.hip) must produce.  Host code only (no HIP), so
// tests/sanitize/wire_mixed_driver.cpp builds it with plain g++.
#pragma once
#include <cstddef>
#include <cstdint>

#define COA_WIRE_MIXED_BLOCK 256u    // frames per block of the prefix-sum kernels (COA_WIRE_SCAN_BLOCK)
#define COA_WIRE_MIXED_SUMS 6        // headers, their bytes | votes | certificates, their bytes, their votes
#define COA_WIRE_MIXED_TOTALS 8      // the six sums, frames without a slot, 0
#define COA_WIRE_NO_SLOT 0xFFFFFFFFu
#define COA_WIRE_MIXED_KINDS 3       // COA_MSG_HEADER, COA_MSG_VOTE, COA_MSG_CERTIFICATE: 0, 1, 2

// per-frame header bytes [n] | per-frame votes [n] | six block totals per
// COA_WIRE_MIXED_BLOCK frames.  Byte offsets from the workspace pointer, every
// section on 256 bytes.  The frames' size does not enter.
struct WireMixedWs {
  size_t hb = 0, nv = 0, bt = 0, bytes = 0;
  uint32_t blocks = 0;
  static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }
  explicit WireMixedWs(uint64_t n) {
    blocks = (uint32_t)((n + COA_WIRE_MIXED_BLOCK - 1) / COA_WIRE_MIXED_BLOCK);
    hb = 0;
    nv = hb + up((size_t)n * 8);
    bt = nv + up((size_t)n * 8);
    bytes = bt + up((size_t)(blocks ? blocks : 1) * COA_WIRE_MIXED_SUMS * 8);
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

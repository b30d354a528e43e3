// Internal launch wrapper of the device-resident wire decoder
// (coa_wire_dev.hip) and its workspace layout; the frame grammar is
// coa_wire_parse.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "coa_wire_mixed.h"  // WireMixedWs: the mixed mode's workspace, host-only

#define COA_WIRE_SCAN_BLOCK 256u  // frames per block of the prefix-sum kernels

// per-frame header bytes [n] | per-frame votes [n] | three block totals per
// COA_WIRE_SCAN_BLOCK frames (header bytes, votes, frames of the kind).  Byte
// offsets from the workspace pointer, every section on 256 bytes.  The frames'
// size does not enter: nothing per byte is kept between the passes.
struct WireWs {
  size_t hb = 0, nv = 0, bt = 0, bytes = 0;
  uint32_t blocks = 0;
  static size_t up(size_t x) { return (x + 255) & ~(size_t)255; }
  explicit WireWs(uint64_t n) {
    blocks = (uint32_t)((n + COA_WIRE_SCAN_BLOCK - 1) / COA_WIRE_SCAN_BLOCK);
    hb = 0;
    nv = hb + up((size_t)n * 8);
    bt = nv + up((size_t)n * 8);
    bytes = bt + up((size_t)(blocks ? blocks : 1) * 3 * 8);
  }
};

struct WireArgs {
  const uint8_t* frames;
  const uint64_t* offs;  // n + 1
  uint64_t frame_bytes;
  uint32_t n;
  // the scan's answers, per frame
  int32_t* kinds;
  uint64_t* hb;
  uint64_t* nv;
  // the decode: frames of kind `want`, everything else a placeholder
  int32_t want;
  uint8_t* hdata;     // Header / Certificate
  uint64_t* hoff;     // n + 1
  uint8_t* ids;       // n * 32
  uint8_t* authors;   // n * 32: the header's author (a certificate's origin), a vote's author
  uint8_t* sigs;      // n * 64
  uint64_t* rounds;   // n
  uint32_t* pcounts;  // n
  uint8_t* vpks;      // Certificate: the votes
  uint8_t* vsigs;
  uint64_t* voff;     // n + 1
  uint8_t* vorigins;  // Vote: n * 32
  uint64_t* bt;       // 3 * blocks
  uint64_t* totals;   // 4
};

// The mixed mode: one array set per kind (the fields of WireArgs' decode part,
// item k of kind's set is the k-th frame of the kind), a slot per frame.
struct WireSet {
  uint8_t* hdata;
  uint64_t* hoff;  // count + 1 used, n + 1 provided
  uint8_t* ids;
  uint8_t* authors;
  uint8_t* sigs;
  uint64_t* rounds;
  uint32_t* pcounts;
  uint8_t* vpks;
  uint8_t* vsigs;
  uint64_t* voff;
  uint8_t* vorigins;
};

struct WireMixedArgs {
  const uint8_t* frames;
  const uint64_t* offs;  // n + 1
  uint64_t frame_bytes;
  uint32_t n;
  int32_t* kinds;
  uint64_t* hb;
  uint64_t* nv;
  WireSet set[COA_WIRE_MIXED_KINDS];  // by COA_MSG_HEADER, COA_MSG_VOTE, COA_MSG_CERTIFICATE
  uint32_t* slots;   // n
  uint64_t* bt;      // COA_WIRE_MIXED_SUMS * blocks
  uint64_t* totals;  // COA_WIRE_MIXED_TOTALS
};
static_assert(COA_WIRE_MIXED_BLOCK == COA_WIRE_SCAN_BLOCK, "one block size for both modes' prefix sums");

// k_wire_scan on s: kinds, hb and nv of every frame.
hipError_t coa_launch_wire_scan(const WireArgs& a, hipStream_t s);
// The scan, the three prefix-sum launches and k_wire_decode on s.
hipError_t coa_launch_wire_decode(const WireArgs& a, hipStream_t s);
// The scan, the three prefix-sum launches over six quantities and
// k_wire_decode_mixed on s.
hipError_t coa_launch_wire_decode_mixed(const WireMixedArgs& a, hipStream_t s);
// out[i] = words[kinds[i]][slots[i]], COA_DAG_NO_MESSAGE where frame i has no slot.
hipError_t coa_launch_wire_scatter(const int32_t* kinds, const uint32_t* slots, const uint32_t* header_words,
                                   const uint32_t* vote_words, const uint32_t* certificate_words, uint32_t* out,
                                   uint32_t n, hipStream_t s);

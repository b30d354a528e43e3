// Internal launch wrappers of the device-resident wire decoder
// (coa_wire_dev.hip) and their argument structs; the frame grammar is
// coa_wire_parse.h, the workspace and block layouts coa_wire_layout.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "coa_wire_layout.h"

// What both modes start with: the frames, and the scan's answers per frame.
struct WireHead {
  const uint8_t* frames;
  const uint64_t* offs;  // n + 1
  uint64_t frame_bytes;
  uint32_t n;
  int32_t* kinds;
  uint64_t* hb;
  uint64_t* nv;
};

// The decoded arrays of one kind, at the capacities coa_verify.h states for n
// frames.  Index-aligned decode: item i is frame i; mixed mode: the frame's slot.
struct WireSet {
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
};

// The index-aligned decode: frames of kind `want`, everything else a placeholder.
struct WireArgs : WireHead {
  int32_t want;
  WireSet out;
  uint64_t* bt;      // 3 * blocks
  uint64_t* totals;  // 4
};

// The mixed mode: one array set per kind, a slot per frame.
struct WireMixedArgs : WireHead {
  WireSet set[COA_WIRE_MIXED_KINDS];  // by COA_MSG_HEADER, COA_MSG_VOTE, COA_MSG_CERTIFICATE
  uint32_t* slots;   // n
  uint64_t* bt;      // COA_WIRE_MIXED_SUMS * blocks
  uint64_t* totals;  // COA_WIRE_MIXED_TOTALS
};

// k_wire_scan on s: kinds, hb and nv of every frame.
hipError_t coa_launch_wire_scan(const WireHead& a, hipStream_t s);
// The scan, the three prefix-sum launches and k_wire_decode on s.
hipError_t coa_launch_wire_decode(const WireArgs& a, hipStream_t s);
// The scan, the three prefix-sum launches over six quantities and
// k_wire_decode_mixed on s.
hipError_t coa_launch_wire_decode_mixed(const WireMixedArgs& a, hipStream_t s);
// out[i] = words[kinds[i]][slots[i]], COA_DAG_NO_MESSAGE where frame i has no slot.
hipError_t coa_launch_wire_scatter(const int32_t* kinds, const uint32_t* slots, const uint32_t* header_words,
                                   const uint32_t* vote_words, const uint32_t* certificate_words, uint32_t* out,
                                   uint32_t n, hipStream_t s);

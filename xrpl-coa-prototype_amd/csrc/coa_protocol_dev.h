// Internal launch wrappers of the protocol kernels -- coa_protocol.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The protocol table of one key-cache generation (KeySet, coa_engine.h),
// in the engine's sorted key order.
struct ProtTab {
  const uint32_t* keys;   // [nk][8]
  const uint32_t* stake;  // [nk]
  const uint32_t* woff;   // [nk + 1] into wids
  const uint32_t* wids;   // each key's worker ids, sorted
  uint32_t nk;
  uint32_t quorum;
};

struct CertProtArgs {
  const uint8_t* hdr_data;
  const uint64_t* hdr_off;  // [nc + 1]
  const uint32_t* ids;      // [nc][8]
  const uint32_t* origins;  // [nc][8]
  const uint64_t* rounds;   // [nc]
  const uint32_t* vpks;     // [nv][8]
  const uint64_t* voff;     // [nc + 1]
  const uint32_t* pcounts;  // [nc] payload entries of each header
  uint32_t nc, nv;
  uint32_t* proto;          // [nc] protocol words out
};

struct MsgProtArgs {
  const uint8_t* hdr_data;  // headers only (null: votes)
  const uint64_t* hdr_off;
  const uint32_t* pcounts;
  const uint32_t* authors;  // [n][8]
  uint32_t n;
  uint32_t* proto;
};

hipError_t coa_launch_cert_protocol(const CertProtArgs& a, const ProtTab& t, hipStream_t s);
hipError_t coa_launch_msg_protocol(const MsgProtArgs& a, const ProtTab& t, hipStream_t s);
// verdicts[i] = coa_verdict_merge(raw[i], proto[i])
hipError_t coa_launch_verdict_merge(const uint32_t* raw, const uint32_t* proto, uint32_t* verdicts, uint32_t n,
                                    hipStream_t s);

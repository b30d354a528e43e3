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

// One aggregation-queue window (k_window_verdict): its certificates, headers
// and votes as the two kernels above take them (proto unused), the raw status
// words of the window's crypto launches, and the verdict words out.
struct WindowVerdictArgs {
  CertProtArgs cert;
  MsgProtArgs hdr, vote;     // vote.hdr_data null
  const uint32_t* cert_raw;  // [cert.nc]
  const uint32_t* msg_raw;   // [hdr.n + vote.n], the headers' first
  uint32_t* words;           // [cert.nc + hdr.n + vote.n]
  uint32_t cert_blocks;      // set by the launcher
};

hipError_t coa_launch_cert_protocol(const CertProtArgs& a, const ProtTab& t, hipStream_t s);
hipError_t coa_launch_msg_protocol(const MsgProtArgs& a, const ProtTab& t, hipStream_t s);
// verdicts[i] = coa_verdict_merge(raw[i], proto[i])
hipError_t coa_launch_verdict_merge(const uint32_t* raw, const uint32_t* proto, uint32_t* verdicts, uint32_t n,
                                    hipStream_t s);
hipError_t coa_launch_window_verdict(WindowVerdictArgs a, const ProtTab& t, hipStream_t s);

// The verdict words of one aggregation-queue window (k_window_verdict;
// coa_queue_hip.cpp calls it after the window's crypto entries, on the same
// stream): device pointers into the window's staged input block -- the arrays
// the crypto entries read, plus the certificates' and the headers' payload
// counts -- and into its output block, the raw status words in and the verdict
// words out (certificates, then headers, then votes).  Reads the protocol
// table of the generation the calling thread pinned (coa_keycache_use).
// Returns 1, with nothing enqueued, when that generation has none (a plain
// coa_committee_register); else COA_OK or a negative COA_E*.
struct CoaWindowVerdictIn {
  const uint8_t* c_hdr_data;
  const uint64_t* c_hdr_off;
  const uint8_t *c_ids, *c_origins;
  const uint64_t* c_rounds;
  const uint8_t* c_vpks;
  const uint64_t* c_voff;
  const uint32_t* c_pcounts;
  uint64_t nc, n_votes;
  const uint8_t* h_hdr_data;
  const uint64_t* h_hdr_off;
  const uint32_t* h_pcounts;
  const uint8_t* h_authors;
  uint64_t nh;
  const uint8_t* v_authors;
  uint64_t nv;
  const uint32_t* cert_raw;  // [nc]
  const uint32_t* msg_raw;   // [nh + nv]
  uint32_t* words;           // [nc + nh + nv]
};
extern "C" int coa_window_verdict_device(int device, const CoaWindowVerdictIn* in, void* stream);

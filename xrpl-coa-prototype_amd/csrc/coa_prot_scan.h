// Header::verify's worker-id check (primary/src/messages.rs:57-61) on the
// device: the pieces k_cert_protocol / k_msg_protocol / k_window_verdict
// (coa_protocol.hip) and k_msg_verdict_lat (coa_cert_lat.hip) share.
#pragma once
#include "coa_fe.h"
#include "coa_protocol.h"
#include "coa_protocol_dev.h"

namespace coa_prot {

// worker id k of a header: the u32 LE at byte 40 + 36 k + 32 of its digest
// input (author | round | (digest | worker id)* | parents*), any alignment
COA_DEV uint32_t worker_id_at(const uint8_t* hdr, uint32_t k) {
  const uint8_t* p = hdr + 40 + 36 * (uint64_t)k + 32;
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// committee.worker(author, id) (config/src/lib.rs:201-212) over the author's
// sorted ids [lo, hi)
COA_DEV bool has_worker(const uint32_t* __restrict__ wids, uint32_t lo, uint32_t hi, uint32_t id) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    const uint32_t w = wids[mid];
    if (w == id) return true;
    if (w < id) lo = mid + 1;
    else hi = mid;
  }
  return false;
}

// (one whole wave, every argument wave-uniform) the protocol code of a header
// or vote whose author holds committee slot `slot`: its stake and, for a
// header (hdr set: its digest input of hlen bytes and pc payload entries), the
// worker ids spread over the 64 lanes.  What msg_proto_word answers for a
// registered author.
COA_DEV uint32_t msg_code_wave(const ProtTab& t, uint32_t slot, const uint8_t* hdr, uint64_t hlen, uint32_t pc,
                               uint32_t lane) {
  if (t.stake[slot] == 0) return COA_DAG_UNKNOWN_AUTHOR;
  if (!hdr || pc == 0) return 0;
  if (40 + 36 * (uint64_t)pc > hlen) return COA_DAG_MALFORMED_HEADER;  // the count overruns the header: nothing is read
  const uint32_t wlo = t.woff[slot], whi = t.woff[slot + 1];
  bool bad = false;
  for (uint32_t k = lane; k < pc; k += 64) bad = bad || !has_worker(t.wids, wlo, whi, worker_id_at(hdr, k));
  return __any(bad) ? COA_DAG_MALFORMED_HEADER : 0u;
}

}  // namespace coa_prot

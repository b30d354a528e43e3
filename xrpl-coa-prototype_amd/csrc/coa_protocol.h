// Protocol checks of Certificate::verify / Header::verify / Vote::verify
// (primary/src/messages.rs:48-67,131-142,189-215) beside the crypto: the
// committee's protocol table, the protocol word of one item, and the merge
// of that word with the crypto status word into the COA_DAG_* verdict.
//
// Plain C++ (the CPU path and its sanitizer driver build without HIP); the
// merge is also compiled for the device, where k_verdict_merge calls it.
// The device kernels are in coa_protocol.hip.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/coa_verify.h"

#if defined(__HIPCC__)
#define COA_HD __host__ __device__ inline
#else
#define COA_HD inline
#endif

// Protocol word of one item: bits 0-7 the first failing protocol check (a
// COA_DAG_* code; 0 = none) or COA_PROTO_GENESIS, bits 8-31 the vote index of
// codes 5 and 6.
#define COA_PROTO_GENESIS 0xffu
#define COA_PROTO_MAX_INDEX 0xffffffu

// Crypto status bits as the kernels write them (coa_committee.h COA_CST_*).
#define COA_PST_BAD_HEADER_ID 1u
#define COA_PST_BAD_SIG 2u
#define COA_PST_BAD_VOTES 4u
#define COA_PST_VOTES_INCONCLUSIVE 8u

// The verdict of one item, in the reference's order.  `raw`: the status word
// of k_cert_verify / k_msg_verify (a vote's signature bit is COA_PST_BAD_SIG).
// The header signature bit is read only when the author has stake, i.e. is
// registered and was decided on the combs; the vote bits only when every
// voter has stake, so an uncached job cannot matter in either place.
COA_HD uint32_t coa_verdict_merge(uint32_t raw, uint32_t proto) {
  const uint32_t code = proto & 0xffu;
  if (code == COA_PROTO_GENESIS) return COA_DAG_OK;                                      // :190-193
  if (raw & COA_PST_BAD_HEADER_ID) return COA_DAG_INVALID_HEADER_ID;                     // :50
  if (code == COA_DAG_UNKNOWN_AUTHOR || code == COA_DAG_MALFORMED_HEADER) return code;   // :53-61, :133-136
  if (raw & COA_PST_BAD_SIG) return COA_DAG_INVALID_SIGNATURE;                           // :64-66, :139-141
  if (code) return proto;                                                                // :201-211
  if (raw & COA_PST_BAD_VOTES) return COA_DAG_INVALID_VOTES;                             // :214
  if (raw & COA_PST_VOTES_INCONCLUSIVE) return COA_DAG_VOTES_OPEN;
  return COA_DAG_OK;
}

// config::Committee in the engine's sorted key order.
struct CoaProtTable {
  std::vector<std::array<uint32_t, 8>> keys;  // sorted as coa_committee_register sorts them
  std::vector<uint32_t> stake;                // [nk]
  std::vector<uint32_t> woff;                 // [nk + 1] into wids
  std::vector<uint32_t> wids;                 // each key's worker ids, sorted
  uint32_t quorum = 0;                        // 2 * total / 3 + 1

  int slot(const uint8_t* pk) const {
    std::array<uint32_t, 8> k;
    std::memcpy(k.data(), pk, 32);
    const auto it = std::lower_bound(keys.begin(), keys.end(), k);
    return it != keys.end() && *it == k ? (int)(it - keys.begin()) : -1;
  }
  bool has_worker(int s, uint32_t wid) const {
    return std::binary_search(wids.begin() + woff[(size_t)s], wids.begin() + woff[(size_t)s + 1], wid);
  }
};

// Validates the arrays of coa_committee_register_authorities and builds the
// table.  Returns false with a text in `err` for what the entry point rejects.
inline bool coa_prot_build(const uint8_t* pks, const uint32_t* stakes, const uint32_t* worker_ids,
                           const uint64_t* worker_offsets, size_t n, CoaProtTable& t, std::string& err) {
  if (n && (!pks || !stakes || !worker_offsets)) return err = "null argument", false;
  if (n > COA_MAX_AUTHORITIES) return err = "more than COA_MAX_AUTHORITIES authorities", false;
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) {
    total += stakes[i];
    if (worker_offsets[i + 1] < worker_offsets[i]) return err = "worker offsets not monotone", false;
  }
  if (total >= (1ull << 31)) return err = "total stake of 2^31 or more", false;
  const uint64_t nw = n ? worker_offsets[n] - worker_offsets[0] : 0;
  if (nw >> 31) return err = "too many worker ids", false;
  if (nw && !worker_ids) return err = "null argument", false;
  std::vector<uint32_t> order(n);
  std::vector<std::array<uint32_t, 8>> k(n);
  for (size_t i = 0; i < n; i++) {
    order[i] = (uint32_t)i;
    std::memcpy(k[i].data(), pks + 32 * i, 32);
  }
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
  for (size_t i = 1; i < n; i++)
    if (k[order[i]] == k[order[i - 1]]) return err = "duplicate authority key", false;
  t = CoaProtTable();
  t.woff.push_back(0);
  for (size_t i = 0; i < n; i++) {
    const uint32_t a = order[i];
    t.keys.push_back(k[a]);
    t.stake.push_back(stakes[a]);
    const size_t at = t.wids.size();
    t.wids.insert(t.wids.end(), worker_ids + worker_offsets[a], worker_ids + worker_offsets[a + 1]);
    std::sort(t.wids.begin() + (long)at, t.wids.end());
    t.woff.push_back((uint32_t)t.wids.size());
  }
  t.quorum = (uint32_t)(2 * total / 3 + 1);
  return true;
}

inline uint32_t coa_prot_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// Header::verify's protocol checks (:53-61) for an author and its header
// bytes: 0, COA_DAG_UNKNOWN_AUTHOR or COA_DAG_MALFORMED_HEADER.  The caller
// has checked that `count` entries fit `len`.
inline uint32_t coa_prot_header_word(const CoaProtTable& t, int slot, const uint8_t* hdr, uint32_t count) {
  if (slot < 0 || t.stake[(size_t)slot] == 0) return COA_DAG_UNKNOWN_AUTHOR;
  for (uint32_t k = 0; k < count; k++)
    if (!t.has_worker(slot, coa_prot_le32(hdr + 40 + 36 * (size_t)k + 32))) return COA_DAG_MALFORMED_HEADER;
  return 0;
}

// Certificate::verify's protocol checks for one certificate.
inline uint32_t coa_prot_cert_word(const CoaProtTable& t, const uint8_t* id, uint64_t round, const uint8_t* origin,
                                   const uint8_t* hdr, uint32_t count, const uint8_t* vote_pks, size_t n_votes,
                                   std::vector<uint32_t>& first) {
  const int aslot = t.slot(origin);
  bool zero_id = true;
  for (int b = 0; b < 32; b++) zero_id = zero_id && id[b] == 0;
  if (zero_id && round == 0 && aslot >= 0) return COA_PROTO_GENESIS;
  const uint32_t h = coa_prot_header_word(t, aslot, hdr, count);
  if (h) return h;
  first.assign(t.keys.size(), 0xffffffffu);
  uint64_t weight = 0;
  for (size_t j = 0; j < n_votes; j++) {
    const int s = t.slot(vote_pks + 32 * j);
    const uint32_t idx = (uint32_t)std::min<size_t>(j, COA_PROTO_MAX_INDEX) << 8;
    if (s >= 0 && first[(size_t)s] != 0xffffffffu) return COA_DAG_AUTHORITY_REUSE | idx;
    if (s < 0 || t.stake[(size_t)s] == 0) return COA_DAG_UNKNOWN_VOTER | idx;
    first[(size_t)s] = (uint32_t)j;
    weight += t.stake[(size_t)s];
  }
  return weight >= t.quorum ? 0u : (uint32_t)COA_DAG_REQUIRES_QUORUM;
}

// true when every payload count fits its header (40 + 36 k <= length)
inline bool coa_prot_counts_fit(const uint64_t* header_offsets, const uint32_t* payload_counts, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (40 + 36 * (uint64_t)payload_counts[i] > header_offsets[i + 1] - header_offsets[i] && payload_counts[i])
      return false;
  return true;
}

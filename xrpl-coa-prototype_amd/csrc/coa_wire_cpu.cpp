// coa_cpu_wire_verdict_many: coa_wire_verdict_many on the engine's CPU path.
// The host scan (coa_wire.cpp), the partition of coa_wire_mixed.h, the host
// decoders over each kind's frames gathered in order, the coa_cpu_*_verdict_many
// calls (coa_cpu.cpp) and the scatter.  Stateless and host-only: no HIP, no
// coa_init, never called implicitly.
#include <cstring>
#include <vector>

#include "../../include/coa_verify.h"
#include "coa_wire_layout.h"

extern "C" int coa_cpu_wire_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n,
                                         uint64_t rng_seed, const uint8_t* committee_pks, const uint32_t* stakes,
                                         const uint32_t* worker_ids, const uint64_t* worker_offsets,
                                         size_t n_authorities, int32_t* kinds_out, uint32_t* verdicts_out,
                                         int nthreads) {
  if (n == 0) return COA_OK;
  if (!frame_offsets || !kinds_out || !verdicts_out) return COA_EINVAL;
  std::vector<uint64_t> hb(n), nv(n);
  int rc = coa_wire_scan(frames, frame_offsets, n, kinds_out, hb.data(), nv.data());  // checks the offsets
  if (rc != COA_OK) return rc;
  std::vector<uint32_t> slots(n);
  size_t count[COA_WIRE_MIXED_KINDS];
  (void)coa_wire_mixed_partition(kinds_out, n, slots.data(), count);

  // each kind's frames back to back, in frame order
  std::vector<uint8_t> bytes[COA_WIRE_MIXED_KINDS];
  std::vector<uint64_t> offs[COA_WIRE_MIXED_KINDS];
  size_t hbytes[COA_WIRE_MIXED_KINDS] = {}, votes = 0;
  {
    size_t total[COA_WIRE_MIXED_KINDS] = {};
    for (size_t i = 0; i < n; i++)
      if (slots[i] != COA_WIRE_NO_SLOT) total[kinds_out[i]] += (size_t)(frame_offsets[i + 1] - frame_offsets[i]);
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) {
      bytes[k].resize(total[k] + 1);
      offs[k].assign(count[k] + 1, 0);
    }
  }
  for (size_t i = 0; i < n; i++) {
    if (slots[i] == COA_WIRE_NO_SLOT) continue;
    const int k = kinds_out[i];
    const size_t len = (size_t)(frame_offsets[i + 1] - frame_offsets[i]), at = (size_t)offs[k][slots[i]];
    if (len) std::memcpy(bytes[k].data() + at, frames + frame_offsets[i], len);
    offs[k][slots[i] + 1] = at + len;
    if (k != COA_MSG_VOTE) hbytes[k] += (size_t)hb[i];
    if (k == COA_MSG_CERTIFICATE) votes += (size_t)nv[i];
  }

  std::vector<uint32_t> words[COA_WIRE_MIXED_KINDS];
  for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) words[k].assign(count[k] + 1, COA_DAG_NO_MESSAGE);
  if (const size_t m = count[COA_MSG_HEADER]) {
    std::vector<uint8_t> hdata(hbytes[COA_MSG_HEADER] + 1), ids(m * 32), authors(m * 32), sigs(m * 64);
    std::vector<uint64_t> hoff(m + 1), rounds(m);
    std::vector<uint32_t> pc(m);
    rc = coa_wire_decode_headers(bytes[COA_MSG_HEADER].data(), offs[COA_MSG_HEADER].data(), m, hdata.data(), hoff.data(),
                                 ids.data(), authors.data(), sigs.data(), rounds.data(), pc.data());
    if (rc == COA_OK)
      rc = coa_cpu_header_verdict_many(hdata.data(), hoff.data(), ids.data(), authors.data(), sigs.data(), m, pc.data(),
                                       committee_pks, stakes, worker_ids, worker_offsets, n_authorities,
                                       words[COA_MSG_HEADER].data(), nthreads);
    if (rc != COA_OK) return rc;
  }
  if (const size_t m = count[COA_MSG_VOTE]) {
    std::vector<uint8_t> ids(m * 32), origins(m * 32), authors(m * 32), sigs(m * 64);
    std::vector<uint64_t> rounds(m);
    rc = coa_wire_decode_votes(bytes[COA_MSG_VOTE].data(), offs[COA_MSG_VOTE].data(), m, ids.data(), rounds.data(),
                               origins.data(), authors.data(), sigs.data());
    if (rc == COA_OK)
      rc = coa_cpu_vote_verdict_many(ids.data(), rounds.data(), origins.data(), authors.data(), sigs.data(), m,
                                     committee_pks, stakes, worker_ids, worker_offsets, n_authorities,
                                     words[COA_MSG_VOTE].data(), nthreads);
    if (rc != COA_OK) return rc;
  }
  if (const size_t m = count[COA_MSG_CERTIFICATE]) {
    std::vector<uint8_t> hdata(hbytes[COA_MSG_CERTIFICATE] + 1), ids(m * 32), origins(m * 32), sigs(m * 64);
    std::vector<uint8_t> vpks(votes * 32 + 1), vsigs(votes * 64 + 1);
    std::vector<uint64_t> hoff(m + 1), rounds(m), voff(m + 1);
    std::vector<uint32_t> pc(m);
    rc = coa_wire_decode_certificates(bytes[COA_MSG_CERTIFICATE].data(), offs[COA_MSG_CERTIFICATE].data(), m,
                                      hdata.data(), hoff.data(), ids.data(), origins.data(), sigs.data(), rounds.data(),
                                      vpks.data(), vsigs.data(), voff.data(), pc.data());
    if (rc == COA_OK)
      rc = coa_cpu_certificate_verdict_many(hdata.data(), hoff.data(), ids.data(), origins.data(), sigs.data(),
                                            rounds.data(), vpks.data(), vsigs.data(), voff.data(), m, rng_seed, pc.data(),
                                            committee_pks, stakes, worker_ids, worker_offsets, n_authorities,
                                            words[COA_MSG_CERTIFICATE].data(), nthreads);
    if (rc != COA_OK) return rc;
  }
  const uint32_t* const by_kind[COA_WIRE_MIXED_KINDS] = {words[0].data(), words[1].data(), words[2].data()};
  coa_wire_mixed_scatter(kinds_out, slots.data(), n, by_kind, COA_DAG_NO_MESSAGE, verdicts_out);
  return COA_OK;
}

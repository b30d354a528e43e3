// Wire decode of the primary's messages, host side.
//
// PrimaryReceiverHandler::dispatch (primary/src/primary.rs:223-244) runs
// `bincode::deserialize::<PrimaryMessage>` on every frame; Core then
// verifies one message at a time.  This decoder turns a window of frames into
// the struct-of-arrays the engine's batched entry points take (one
// coa_certificate_verify_many launch for all certificates of the window),
// without building per-message objects.
//
// The format and every rule of it are in coa_wire_parse.h; this file drives
// those functions over one frame after the other.  Only a set's order is taken
// its own way, by a sort: frames here are untrusted and of any size, so the
// capped device decoder's quadratic coa_wp_is_last / coa_wp_rank are not used.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "coa_offsets.h"
#include "coa_wire_parse.h"

namespace {

// Frame i of a call, walked: its kind is the walk's, then that of a
// certificate's votes; the first error in wire order decides.  Keys are kept as
// they are checked, so each is read once.  votes: null, or where the vote list
// goes meanwhile (nv * 32 key bytes, then nv * 64 of signatures) -- not the
// caller's arrays, which are sized for well formed frames only.
struct Walked {
  const uint8_t* p;
  size_t n;
  CoaWpFrame f;
  int32_t kind;
  uint8_t key0[32], key1[32];  // a header's author; a vote's origin and author
  Walked(const uint8_t* frames, const uint64_t* offs, size_t i, std::vector<uint8_t>* votes = nullptr)
      : p(frames + offs[i]), n(offs[i + 1] - offs[i]) {
    kind = coa_wp_walk(p, n, &f, key0, key1);
    if (kind != COA_MSG_CERTIFICATE) return;
    if (votes) votes->resize((size_t)f.nv * 96);  // nv <= n / 72
    uint8_t* v = votes && f.nv ? votes->data() : nullptr;
    const int rc = coa_wp_votes(p, n, f.votes, f.nv, v, v ? v + (size_t)f.nv * 32 : nullptr);
    if (rc != COA_OK) kind = rc;
  }
};

// BTreeMap / BTreeSet over n wire entries of `stride` bytes keyed by their
// first 32: the wire indices sorted by (key, wire index), of which the last of
// each run of equal keys survives.  ord: the survivors in key order; returns
// their number.
using Order = std::vector<size_t>;
size_t set_order(const uint8_t* base, size_t stride, size_t n, Order& ord) {
  ord.resize(n);
  std::iota(ord.begin(), ord.end(), (size_t)0);
  std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) {
    const int c = coa_wp_key_cmp(base + a * stride, base + b * stride);
    return c ? c < 0 : a < b;
  });
  size_t kept = 0;
  for (size_t k = 0; k < n; k++)
    if (k + 1 == n || coa_wp_key_cmp(base + ord[k] * stride, base + ord[k + 1] * stride) != 0) ord[kept++] = ord[k];
  ord.resize(kept);
  return kept;
}

bool frames_ok(const uint8_t* frames, const uint64_t* offs, size_t n) {
  return offs && coa_rt::offsets_monotone(offs, n) && !(offs[n] > offs[0] && !frames);
}

// coa_wire_decode_headers (want COA_MSG_HEADER, no vote arrays) and
// coa_wire_decode_certificates: a certificate is a header and its votes.
int decode_headers(int32_t want, const uint8_t* frames, const uint64_t* offs, size_t n, uint8_t* data, uint64_t* hoff,
                   uint8_t* ids, uint8_t* authors, uint8_t* sigs, uint64_t* rounds, uint32_t* payload_counts,
                   uint8_t* vpks, uint8_t* vsigs, uint64_t* voff) {
  if (!frames_ok(frames, offs, n) || !hoff || !ids || !authors || !sigs || !rounds) return COA_EINVAL;
  if (want == COA_MSG_HEADER ? !data : !voff) return COA_EINVAL;
  hoff[0] = 0;
  if (voff) voff[0] = 0;
  Order payload, parents;  // reused from frame to frame
  std::vector<uint8_t> votes;
  for (size_t i = 0; i < n; i++) {
    const Walked w(frames, offs, i, &votes);
    if (w.kind != want) return COA_EINVAL;  // coa_wire_scan first: only frames of one kind here
    if (!data || (w.f.nv && (!vpks || !vsigs))) return COA_EINVAL;
    uint8_t* o = data + hoff[i];  // the Header::digest input
    std::memcpy(o, w.key0, 32);
    std::memcpy(authors + i * 32, w.key0, 32);
    for (int b = 0; b < 8; b++) o[32 + b] = (uint8_t)(w.f.round >> (8 * b));
    o += 40;
    set_order(w.p + w.f.payload, 36, (size_t)w.f.np, payload);
    for (size_t k : payload) std::memcpy(o, w.p + w.f.payload + k * 36, 36), o += 36;
    set_order(w.p + w.f.parents, 32, (size_t)w.f.nq, parents);
    for (size_t k : parents) std::memcpy(o, w.p + w.f.parents + k * 32, 32), o += 32;
    hoff[i + 1] = (uint64_t)(o - data);
    std::memcpy(ids + i * 32, w.p + w.f.id, 32);
    std::memcpy(sigs + i * 64, w.p + w.f.sig, 64);
    rounds[i] = w.f.round;
    if (payload_counts) payload_counts[i] = (uint32_t)payload.size();
    if (!voff) continue;
    if (w.f.nv) {
      std::memcpy(vpks + voff[i] * 32, votes.data(), (size_t)w.f.nv * 32);
      std::memcpy(vsigs + voff[i] * 64, votes.data() + (size_t)w.f.nv * 32, (size_t)w.f.nv * 64);
    }
    voff[i + 1] = voff[i] + w.f.nv;
  }
  return COA_OK;
}

}  // namespace

extern "C" {

int coa_wire_scan(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kind_out,
                  uint64_t* header_bytes_out, uint64_t* votes_out) {
  if (!kind_out || !frames_ok(frames, frame_offsets, n)) return COA_EINVAL;
  Order ord;
  for (size_t i = 0; i < n; i++) {
    const Walked w(frames, frame_offsets, i);
    kind_out[i] = w.kind;
    const bool hdr = w.kind == COA_MSG_HEADER || w.kind == COA_MSG_CERTIFICATE;
    if (header_bytes_out) {  // only the survivor counts are needed
      const size_t P = hdr ? set_order(w.p + w.f.payload, 36, (size_t)w.f.np, ord) : 0;
      header_bytes_out[i] = hdr ? 40 + 36 * P + 32 * set_order(w.p + w.f.parents, 32, (size_t)w.f.nq, ord) : 0;
    }
    if (votes_out) votes_out[i] = w.kind == COA_MSG_CERTIFICATE ? w.f.nv : 0;
  }
  return COA_OK;
}

int coa_wire_decode_certificates(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint8_t* header_data,
                                 uint64_t* header_offsets, uint8_t* ids, uint8_t* origins, uint8_t* header_sigs,
                                 uint64_t* rounds, uint8_t* vote_pks, uint8_t* vote_sigs, uint64_t* vote_offsets,
                                 uint32_t* payload_counts) {
  return decode_headers(COA_MSG_CERTIFICATE, frames, frame_offsets, n, header_data, header_offsets, ids, origins,
                        header_sigs, rounds, payload_counts, vote_pks, vote_sigs, vote_offsets);
}

int coa_wire_decode_headers(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint8_t* header_data,
                            uint64_t* header_offsets, uint8_t* ids, uint8_t* authors, uint8_t* sigs,
                            uint64_t* rounds, uint32_t* payload_counts) {
  return decode_headers(COA_MSG_HEADER, frames, frame_offsets, n, header_data, header_offsets, ids, authors, sigs, rounds,
                        payload_counts, nullptr, nullptr, nullptr);
}

int coa_wire_decode_votes(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint8_t* ids,
                          uint64_t* rounds, uint8_t* origins, uint8_t* authors, uint8_t* sigs) {
  if (!frames_ok(frames, frame_offsets, n) || !ids || !rounds || !origins || !authors || !sigs) return COA_EINVAL;
  for (size_t i = 0; i < n; i++) {
    const Walked w(frames, frame_offsets, i);
    if (w.kind != COA_MSG_VOTE) return COA_EINVAL;
    std::memcpy(ids + i * 32, w.p + w.f.v_id, 32);
    rounds[i] = w.f.v_round;
    std::memcpy(origins + i * 32, w.key0, 32);
    std::memcpy(authors + i * 32, w.key1, 32);
    std::memcpy(sigs + i * 64, w.p + w.f.v_sig, 64);
  }
  return COA_OK;
}

}  // extern "C"

// Entries of include/coa_verify.h over the engine core (coa_engine.h): the
// device-resident wire decoder (kernels: coa_wire_dev.hip, grammar:
// coa_wire_parse.h, layouts: coa_wire_layout.h) and the fused
// frames-to-verdicts calls on top of it.
#include "coa_engine.h"

#include <cstring>

#include "coa_resolve_ws.h"
#include "coa_wire_dev.h"

namespace coa_rt __attribute__((visibility("hidden"))) {

// Checks shared by the device entries; COA_OK with d and s set, else the
// call's answer.
int wire_enter(int device, const void* d_frames, const uint64_t* d_offs, size_t n, size_t frame_bytes, bool arrays_ok,
               void* stream, Dev*& d, hipStream_t& s) {
  if (!d_frames || !d_offs || !arrays_ok) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK || check_n(frame_bytes) != COA_OK) return COA_EINVAL;
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  return enter_device(device, stream, d, s);
}

WireHead wire_head(const uint8_t* d_frames, const uint64_t* d_offs, size_t n, size_t frame_bytes, int32_t* d_kinds) {
  return {d_frames, d_offs, frame_bytes, (uint32_t)n, d_kinds, nullptr, nullptr};
}

// To carve a wire workspace: the scan's per-frame sums, where the caller gave
// none, and the `sums` block totals per block.
void wire_carve(WireHead& a, uint64_t*& bt, int sums, void* ws) {
  const WireWs L(a.n, sums);
  uint8_t* base = static_cast<uint8_t*>(ws);
  if (!a.hb) a.hb = reinterpret_cast<uint64_t*>(base + L.hb);
  if (!a.nv) a.nv = reinterpret_cast<uint64_t*>(base + L.nv);
  bt = reinterpret_cast<uint64_t*>(base + L.bt);
}

// The three kinds' sets from an entry's pointers, in the entry's order.
WireSet header_set(uint8_t* hdata, uint64_t* hoff, uint8_t* ids, uint8_t* authors, uint8_t* sigs, uint32_t* pcounts,
                   uint64_t* rounds) {
  return {hdata, hoff, ids, authors, sigs, rounds, pcounts, nullptr, nullptr, nullptr, nullptr};
}

WireSet vote_set(uint8_t* ids, uint64_t* rounds, uint8_t* origins, uint8_t* authors, uint8_t* sigs) {
  return {nullptr, nullptr, ids, authors, sigs, rounds, nullptr, nullptr, nullptr, nullptr, origins};
}

WireSet certificate_set(uint8_t* hdata, uint64_t* hoff, uint8_t* ids, uint8_t* origins, uint8_t* sigs, uint64_t* rounds,
                        uint8_t* vpks, uint8_t* vsigs, uint64_t* voff, uint32_t* pcounts) {
  return {hdata, hoff, ids, origins, sigs, rounds, pcounts, vpks, vsigs, voff, nullptr};
}

// Every array a set of this kind has (coa_wire_set_has) is given.
bool set_complete(int kind, const WireSet& o) {
  const void* const at[wWords] = {o.hdata, o.hoff,    o.ids,  o.authors, o.vorigins, o.sigs,
                                  o.rounds, o.pcounts, o.vpks, o.vsigs,   o.voff};
  for (int sec = 0; sec < wWords; sec++)
    if (coa_wire_set_has(kind, sec) && !at[sec]) return false;
  return true;
}

// The index-aligned decode entries.
int wire_decode(int device, const uint8_t* d_frames, const uint64_t* d_offs, size_t n, size_t frame_bytes, int32_t want,
                const WireSet& out, int32_t* d_kinds, uint64_t* d_totals, void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  const bool ok = set_complete(want, out) && d_kinds && d_totals;
  if (const int e = wire_enter(device, d_frames, d_offs, n, frame_bytes, ok, stream, d, s)) return e;
  WireArgs a{wire_head(d_frames, d_offs, n, frame_bytes, d_kinds), want, out, nullptr, d_totals};
  // no key-cache generation to trail: the decode reads no committee table
  return with_workspace(*d, s, workspace, d->vws, WireWs(n, 3).bytes, nullptr, [&](void* ws) -> int {
    wire_carve(a, a.bt, 3, ws);
    HIP_TRY(coa_launch_wire_decode(a, s));
    return COA_OK;
  });
}

// ---- frames to verdicts
// To bind a set: kind k's arrays in the block at b, null where the kind has none.
void bind(WireSet& o, uint8_t* b, const WireBlock& L, int k) {
  auto at = [&](int sec) { return L.set[k][sec] == WireBlock::kNone ? nullptr : b + L.set[k][sec]; };
  auto at64 = [&](int sec) { return reinterpret_cast<uint64_t*>(at(sec)); };
  o = {at(wHdata), at64(wHoff), at(wIds),   at(wAuthors), at(wSigs),   at64(wRounds), reinterpret_cast<uint32_t*>(at(wPcounts)),
       at(wVpks),  at(wVsigs),  at64(wVoff), at(wOrigins)};
}

// Workspace bytes of kind k's verdict call with `count` items and `votes` votes.
size_t verdict_ws_bytes(int k, size_t count, size_t votes) {
  if (k != COA_MSG_CERTIFICATE) return coa_message_verdict_workspace_bytes(count);
  return std::max(coa_certificate_verdict_workspace_bytes(count, votes), ResolveWs(count, votes, 0).bytes);
}

// To run kind k's verdict call over the first `count` items of o on s; a
// certificate's open votes are resolved after it.
int verdict_many(Dev& d, hipStream_t s, int k, const WireSet& o, size_t count, size_t votes, uint64_t rng_seed,
                 uint32_t* words) {
  if (k == COA_MSG_HEADER)
    return coa_header_verdict_many_device(d.id, o.hdata, o.hoff, o.ids, o.authors, o.sigs, count, o.pcounts, words,
                                          d.vws.p, s);
  if (k == COA_MSG_VOTE)
    return coa_vote_verdict_many_device(d.id, o.ids, o.rounds, o.vorigins, o.authors, o.sigs, count, words, d.vws.p, s);
  const int rc = coa_certificate_verdict_many_device(d.id, o.hdata, o.hoff, o.ids, o.authors, o.sigs, o.rounds, o.vpks,
                                                     o.vsigs, o.voff, count, votes, o.pcounts, words, d.vws.p, s);
  if (rc != COA_OK) return rc;
  return coa_certificate_votes_resolve_device(d.id, o.ids, o.authors, o.rounds, o.vpks, o.vsigs, o.voff, count, votes, 0,
                                              nullptr, rng_seed, words, nullptr, d.vws.p, s);
}

// Raw host frames to kinds and verdict words for the kinds of `mask` (bit k:
// kind k): one kind index-aligned, all three partitioned by kind on the device.
int wire_fused(unsigned mask, const uint8_t* frames, const uint64_t* offs, size_t n, uint64_t rng_seed,
               int32_t* kinds_out, uint32_t* verdicts_out) {
  if (n == 0) return COA_OK;
  if (!offs || !kinds_out || !verdicts_out) return fail(COA_EINVAL, "null argument");
  if (!offsets_monotone(offs, n)) return fail(COA_EINVAL, "offsets not monotone");
  const size_t fb = offs[n];
  if (fb && !frames) return fail(COA_EINVAL, "null frames");
  if (check_n(n) != COA_OK || check_n(fb) != COA_OK) return COA_EINVAL;
  const int rc0 = ensure_init();
  if (rc0 != COA_OK) return rc0;
  // one context per call: a single shard, under its context's lock
  return for_shards(1, [&](Dev& d, size_t, size_t) -> int {
    hipStream_t s = d.stream;
    const WireBlock L(n, fb, mask);
    const int32_t want = L.mixed ? -1 : (int32_t)(mask >> 1);  // the one bit's index: 1, 2, 4 to 0, 1, 2
    // what each verdict call below answers itself; here also for a mixed batch that holds no message
    if (L.mixed && !keys_now(d)->has_prot) return fail(COA_EINVAL, "committee registered without stakes");
    HIP_TRY(d.pin.ensure(std::max(L.upload, L.download)));
    HIP_TRY(d.out.ensure(L.bytes));
    uint8_t* h = static_cast<uint8_t*>(d.pin.p);
    uint8_t* b = d.out.as<uint8_t>();
    const Seg segs[2] = {{h + L.offs, offs, (n + 1) * 8}, {h + L.frames, frames, fb}};
    CopyPool::get().copy(segs, fb ? 2 : 1);  // a round's frames are ~100 MB: the pool's threads share the copy
    HIP_TRY(hipMemcpyAsync(b, h, L.upload, hipMemcpyHostToDevice, s));
    int32_t* d_kinds = reinterpret_cast<int32_t*>(b + L.kinds);
    uint32_t* d_slots = L.mixed ? reinterpret_cast<uint32_t*>(b + L.slots) : nullptr;
    uint64_t* d_totals = reinterpret_cast<uint64_t*>(b + L.totals);
    const WireHead head = wire_head(b + L.frames, reinterpret_cast<const uint64_t*>(b + L.offs), n, fb, d_kinds);
    WireSet set[COA_WIRE_MIXED_KINDS] = {};
    uint32_t* words[COA_WIRE_MIXED_KINDS] = {};
    size_t count[COA_WIRE_MIXED_KINDS] = {}, votes = 0;
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) {
      if (!((mask >> k) & 1)) continue;
      bind(set[k], b, L, k);
      words[k] = reinterpret_cast<uint32_t*>(b + L.set[k][wWords]);
      count[k] = n;  // one kind: every frame is an item
    }
    if (L.mixed) {
      WireMixedArgs a{head, {set[0], set[1], set[2]}, d_slots, nullptr, d_totals};
      wire_carve(a, a.bt, COA_WIRE_MIXED_SUMS, b + L.ws);
      HIP_TRY(coa_launch_wire_decode_mixed(a, s));
    } else {
      WireArgs a{head, want, set[want], nullptr, d_totals};
      wire_carve(a, a.bt, 3, b + L.ws);
      HIP_TRY(coa_launch_wire_decode(a, s));
    }
    if ((mask >> COA_MSG_CERTIFICATE) & 1) {
      // the verdict calls take their counts, the certificate call its votes, as host arguments
      const uint64_t* totals = reinterpret_cast<const uint64_t*>(h);
      HIP_TRY(hipMemcpyAsync(h, d_totals, L.ntotals * 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      votes = (size_t)totals[L.mixed ? 5 : 1];
      const int count_at[COA_WIRE_MIXED_KINDS] = {0, 2, 3};  // headers, votes, certificates among the six sums
      if (L.mixed)
        for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) count[k] = (size_t)totals[count_at[k]];
    }
    size_t need = 0;
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++)
      if (count[k]) need = std::max(need, verdict_ws_bytes(k, count[k], votes));
    if (need) HIP_TRY(d.vws.ensure(need));  // one workspace: the calls follow each other on s
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) {  // header, vote, certificate; a kind without a frame launches nothing
      if (!count[k]) continue;
      const int rc = verdict_many(d, s, k, set[k], count[k], votes, rng_seed, words[k]);
      if (rc != COA_OK) return rc;
    }
    uint32_t* d_words = reinterpret_cast<uint32_t*>(b + L.words);
    if (L.mixed)
      HIP_TRY(coa_launch_wire_scatter(d_kinds, d_slots, words[0], words[1], words[2], d_words, (uint32_t)n, s));
    HIP_TRY(hipMemcpyAsync(h, d_kinds, L.download, hipMemcpyDeviceToHost, s));  // kinds and words lie side by side: one D2H
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(kinds_out, h, n * 4);
    std::memcpy(verdicts_out, h + (L.words - L.kinds), n * 4);
    if (!L.mixed)
      for (size_t i = 0; i < n; i++)
        if (kinds_out[i] != want) verdicts_out[i] = COA_DAG_NO_MESSAGE;
    return COA_OK;
  });
}

}  // namespace coa_rt

using namespace coa_rt;

extern "C" {

size_t coa_wire_workspace_bytes(size_t n, size_t frame_bytes) {
  (void)frame_bytes;  // nothing per byte is kept between the passes
  return WireWs(n, 3).bytes;
}

int coa_wire_scan_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                         size_t frame_bytes, int32_t* d_kinds, uint64_t* d_header_bytes, uint64_t* d_votes,
                         void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, d_kinds != nullptr, stream, d, s))
    return e;
  WireHead a = wire_head(d_frames, d_frame_offsets, n, frame_bytes, d_kinds);
  a.hb = d_header_bytes;
  a.nv = d_votes;
  if (d_header_bytes && d_votes) {  // nothing of the workspace is touched
    HIP_TRY(coa_launch_wire_scan(a, s));
    if (!workspace) HIP_TRY(hipStreamSynchronize(s));
    return COA_OK;
  }
  return with_workspace(*d, s, workspace, d->vws, WireWs(n, 3).bytes, nullptr, [&](void* ws) -> int {
    uint64_t* bt;  // the scan alone has no block totals
    wire_carve(a, bt, 3, ws);
    HIP_TRY(coa_launch_wire_scan(a, s));
    return COA_OK;
  });
}

int coa_wire_decode_certificates_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                        size_t frame_bytes, uint8_t* d_header_data, uint64_t* d_header_offsets,
                                        uint8_t* d_ids, uint8_t* d_origins, uint8_t* d_header_sigs, uint64_t* d_rounds,
                                        uint8_t* d_vote_pks, uint8_t* d_vote_sigs, uint64_t* d_vote_offsets,
                                        uint32_t* d_payload_counts, int32_t* d_kinds, uint64_t* d_totals,
                                        void* workspace, void* stream) {
  return wire_decode(device, d_frames, d_frame_offsets, n, frame_bytes, COA_MSG_CERTIFICATE,
                     certificate_set(d_header_data, d_header_offsets, d_ids, d_origins, d_header_sigs, d_rounds, d_vote_pks,
                                     d_vote_sigs, d_vote_offsets, d_payload_counts),
                     d_kinds, d_totals, workspace, stream);
}

int coa_wire_decode_headers_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                   size_t frame_bytes, uint8_t* d_header_data, uint64_t* d_header_offsets,
                                   uint8_t* d_ids, uint8_t* d_authors, uint8_t* d_sigs, uint32_t* d_payload_counts,
                                   uint64_t* d_rounds, int32_t* d_kinds, uint64_t* d_totals, void* workspace,
                                   void* stream) {
  return wire_decode(device, d_frames, d_frame_offsets, n, frame_bytes, COA_MSG_HEADER,
                     header_set(d_header_data, d_header_offsets, d_ids, d_authors, d_sigs, d_payload_counts, d_rounds),
                     d_kinds, d_totals, workspace, stream);
}

int coa_wire_decode_votes_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                 size_t frame_bytes, uint8_t* d_ids, uint64_t* d_rounds, uint8_t* d_origins,
                                 uint8_t* d_authors, uint8_t* d_sigs, int32_t* d_kinds, uint64_t* d_totals,
                                 void* workspace, void* stream) {
  return wire_decode(device, d_frames, d_frame_offsets, n, frame_bytes, COA_MSG_VOTE,
                     vote_set(d_ids, d_rounds, d_origins, d_authors, d_sigs), d_kinds, d_totals, workspace, stream);
}

size_t coa_wire_mixed_workspace_bytes(size_t n, size_t frame_bytes) {
  (void)frame_bytes;  // as coa_wire_workspace_bytes
  return WireWs(n, COA_WIRE_MIXED_SUMS).bytes;
}

int coa_wire_decode_mixed_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                 size_t frame_bytes, uint8_t* d_h_header_data, uint64_t* d_h_header_offsets,
                                 uint8_t* d_h_ids, uint8_t* d_h_authors, uint8_t* d_h_sigs,
                                 uint32_t* d_h_payload_counts, uint64_t* d_h_rounds, uint8_t* d_v_ids,
                                 uint64_t* d_v_rounds, uint8_t* d_v_origins, uint8_t* d_v_authors, uint8_t* d_v_sigs,
                                 uint8_t* d_c_header_data, uint64_t* d_c_header_offsets, uint8_t* d_c_ids,
                                 uint8_t* d_c_origins, uint8_t* d_c_header_sigs, uint64_t* d_c_rounds,
                                 uint8_t* d_c_vote_pks, uint8_t* d_c_vote_sigs, uint64_t* d_c_vote_offsets,
                                 uint32_t* d_c_payload_counts, int32_t* d_kinds, uint32_t* d_slots,
                                 uint64_t* d_totals, void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  WireMixedArgs a{wire_head(d_frames, d_frame_offsets, n, frame_bytes, d_kinds),
                  {header_set(d_h_header_data, d_h_header_offsets, d_h_ids, d_h_authors, d_h_sigs, d_h_payload_counts,
                              d_h_rounds),
                   vote_set(d_v_ids, d_v_rounds, d_v_origins, d_v_authors, d_v_sigs),
                   certificate_set(d_c_header_data, d_c_header_offsets, d_c_ids, d_c_origins, d_c_header_sigs, d_c_rounds,
                                   d_c_vote_pks, d_c_vote_sigs, d_c_vote_offsets, d_c_payload_counts)},
                  d_slots, nullptr, d_totals};
  bool ok = d_kinds && d_slots && d_totals;
  for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) ok = ok && set_complete(k, a.set[k]);
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, ok, stream, d, s)) return e;
  // no key-cache generation to trail: the decode reads no committee table
  return with_workspace(*d, s, workspace, d->vws, WireWs(n, COA_WIRE_MIXED_SUMS).bytes, nullptr, [&](void* ws) -> int {
    wire_carve(a, a.bt, COA_WIRE_MIXED_SUMS, ws);
    HIP_TRY(coa_launch_wire_decode_mixed(a, s));
    return COA_OK;
  });
}

int coa_wire_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint64_t rng_seed,
                          int32_t* kinds_out, uint32_t* verdicts_out) {
  return wire_fused(7u, frames, frame_offsets, n, rng_seed, kinds_out, verdicts_out);
}

int coa_wire_certificate_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n,
                                      uint64_t rng_seed, int32_t* kinds_out, uint32_t* verdicts_out) {
  return wire_fused(1u << COA_MSG_CERTIFICATE, frames, frame_offsets, n, rng_seed, kinds_out, verdicts_out);
}

int coa_wire_header_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kinds_out,
                                 uint32_t* verdicts_out) {
  return wire_fused(1u << COA_MSG_HEADER, frames, frame_offsets, n, 0, kinds_out, verdicts_out);
}

int coa_wire_vote_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kinds_out,
                               uint32_t* verdicts_out) {
  return wire_fused(1u << COA_MSG_VOTE, frames, frame_offsets, n, 0, kinds_out, verdicts_out);
}

}  // extern "C"

// Entries of include/coa_verify.h over the engine core (coa_engine.h): the
// device-resident wire decoder (kernels: coa_wire_dev.hip, grammar:
// coa_wire_parse.h) and the fused frames-to-verdicts calls on top of it.
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

WireArgs wire_args(const uint8_t* d_frames, const uint64_t* d_offs, size_t n, size_t frame_bytes, int32_t* d_kinds) {
  WireArgs a{};
  a.frames = d_frames;
  a.offs = d_offs;
  a.frame_bytes = frame_bytes;
  a.n = (uint32_t)n;
  a.kinds = d_kinds;
  return a;
}

// The scan's per-frame sums and the block totals live in the workspace.
void wire_carve(WireArgs& a, void* ws) {
  const WireWs L(a.n);
  uint8_t* base = static_cast<uint8_t*>(ws);
  if (!a.hb) a.hb = reinterpret_cast<uint64_t*>(base + L.hb);
  if (!a.nv) a.nv = reinterpret_cast<uint64_t*>(base + L.nv);
  a.bt = reinterpret_cast<uint64_t*>(base + L.bt);
}

int wire_decode(Dev& d, hipStream_t s, WireArgs a, void* workspace) {
  // no key-cache generation to trail: the decode reads no committee table
  return with_workspace(d, s, workspace, d.vws, WireWs(a.n).bytes, nullptr, [&](void* ws) -> int {
    wire_carve(a, ws);
    HIP_TRY(coa_launch_wire_decode(a, s));
    return COA_OK;
  });
}

// ---- frames to verdicts
enum { kHdata, kHoff, kIds, kAuthors, kOrigins, kSigs, kRounds, kPcounts, kVpks, kVsigs, kVoff, kTotals, kKinds, kWords,
       kWireWs, kSections };

// The device block of one fused call: frame offsets and frames (one H2D), the
// decoded arrays at their stated capacities, kinds and words side by side
// (one D2H), the decoder's workspace.
struct FusedLayout {
  size_t offs = 0, frames = 0, at[kSections] = {}, bytes = 0;
  FusedLayout(size_t n, size_t fb) {
    size_t end = 0;
    auto take = [&end](size_t b) {
      const size_t at_ = end;
      end = align_up(at_ + b, 256);
      return at_;
    };
    offs = take((n + 1) * 8);
    frames = take(fb + 4);
    const size_t votes = COA_WIRE_VOTES_BOUND(fb);
    at[kHdata] = take(fb + 16);
    at[kHoff] = take((n + 1) * 8);
    at[kIds] = take(n * 32);
    at[kAuthors] = take(n * 32);
    at[kOrigins] = take(n * 32);
    at[kSigs] = take(n * 64);
    at[kRounds] = take(n * 8);
    at[kPcounts] = take(n * 4);
    at[kVpks] = take(votes * 32 + 16);
    at[kVsigs] = take(votes * 64 + 16);
    at[kVoff] = take((n + 1) * 8);
    at[kTotals] = take(32);
    at[kKinds] = take(n * 4);
    at[kWords] = take(n * 4);
    at[kWireWs] = take(WireWs(n).bytes);
    bytes = end;
  }
};

int wire_fused(int32_t want, const uint8_t* frames, const uint64_t* offs, size_t n, uint64_t rng_seed, int32_t* kinds_out,
               uint32_t* verdicts_out) {
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
    const FusedLayout L(n, fb);
    HIP_TRY(d.pin.ensure(std::max(L.at[kHdata], L.at[kWords] - L.at[kKinds] + n * 4)));  // the H2D block; kinds | words
    HIP_TRY(d.out.ensure(L.bytes));
    uint8_t* h = static_cast<uint8_t*>(d.pin.p);
    uint8_t* b = d.out.as<uint8_t>();
    const Seg segs[2] = {{h + L.offs, offs, (n + 1) * 8}, {h + L.frames, frames, fb}};
    CopyPool::get().copy(segs, fb ? 2 : 1);  // a round's frames are ~100 MB: the pool's threads share the copy
    HIP_TRY(hipMemcpyAsync(b, h, L.frames + fb, hipMemcpyHostToDevice, s));
    auto u8 = [&](int k) { return b + L.at[k]; };
    auto u64 = [&](int k) { return reinterpret_cast<uint64_t*>(b + L.at[k]); };
    auto u32 = [&](int k) { return reinterpret_cast<uint32_t*>(b + L.at[k]); };
    int32_t* d_kinds = reinterpret_cast<int32_t*>(b + L.at[kKinds]);
    WireArgs a = wire_args(b + L.frames, reinterpret_cast<const uint64_t*>(b + L.offs), n, fb, d_kinds);
    a.want = want;
    a.ids = u8(kIds);
    a.authors = u8(kAuthors);
    a.sigs = u8(kSigs);
    a.rounds = u64(kRounds);
    a.totals = u64(kTotals);
    if (want == COA_MSG_VOTE) {
      a.vorigins = u8(kOrigins);
    } else {
      a.hdata = u8(kHdata);
      a.hoff = u64(kHoff);
      a.pcounts = u32(kPcounts);
    }
    if (want == COA_MSG_CERTIFICATE) {
      a.vpks = u8(kVpks);
      a.vsigs = u8(kVsigs);
      a.voff = u64(kVoff);
    }
    wire_carve(a, u8(kWireWs));
    HIP_TRY(coa_launch_wire_decode(a, s));
    int rc = COA_OK;
    if (want == COA_MSG_CERTIFICATE) {
      // the verdict call takes its vote count as a host argument
      uint64_t* totals = reinterpret_cast<uint64_t*>(h);
      HIP_TRY(hipMemcpyAsync(totals, u64(kTotals), 32, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      const size_t nvotes = (size_t)totals[1];
      HIP_TRY(d.vws.ensure(std::max(coa_certificate_verdict_workspace_bytes(n, nvotes), ResolveWs(n, nvotes, 0).bytes)));
      rc = coa_certificate_verdict_many_device(d.id, u8(kHdata), u64(kHoff), u8(kIds), u8(kAuthors), u8(kSigs),
                                               u64(kRounds), u8(kVpks), u8(kVsigs), u64(kVoff), n, nvotes,
                                               u32(kPcounts), u32(kWords), d.vws.p, s);
      if (rc == COA_OK)
        rc = coa_certificate_votes_resolve_device(d.id, u8(kIds), u8(kAuthors), u64(kRounds), u8(kVpks), u8(kVsigs),
                                                  u64(kVoff), n, nvotes, 0, nullptr, rng_seed, u32(kWords), nullptr,
                                                  d.vws.p, s);
    } else {
      HIP_TRY(d.vws.ensure(coa_message_verdict_workspace_bytes(n)));
      rc = want == COA_MSG_HEADER
               ? coa_header_verdict_many_device(d.id, u8(kHdata), u64(kHoff), u8(kIds), u8(kAuthors), u8(kSigs), n,
                                                u32(kPcounts), u32(kWords), d.vws.p, s)
               : coa_vote_verdict_many_device(d.id, u8(kIds), u64(kRounds), u8(kOrigins), u8(kAuthors), u8(kSigs), n,
                                              u32(kWords), d.vws.p, s);
    }
    if (rc != COA_OK) return rc;
    // kinds and words lie side by side: one D2H
    HIP_TRY(hipMemcpyAsync(h, d_kinds, L.at[kWords] - L.at[kKinds] + n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(kinds_out, h, n * 4);
    std::memcpy(verdicts_out, h + (L.at[kWords] - L.at[kKinds]), n * 4);
    for (size_t i = 0; i < n; i++)
      if (kinds_out[i] != want) verdicts_out[i] = COA_DAG_NO_MESSAGE;
    return COA_OK;
  });
}

// ---- mixed batches
void mixed_carve(WireMixedArgs& a, void* ws) {
  const WireMixedWs L(a.n);
  uint8_t* base = static_cast<uint8_t*>(ws);
  a.hb = reinterpret_cast<uint64_t*>(base + L.hb);
  a.nv = reinterpret_cast<uint64_t*>(base + L.nv);
  a.bt = reinterpret_cast<uint64_t*>(base + L.bt);
}

// One kind's arrays in the device block of a mixed fused call; a vote has no
// header data, a header no votes.
enum { mHdata, mHoff, mIds, mAuthors, mOrigins, mSigs, mRounds, mPcounts, mVpks, mVsigs, mVoff, mWords, mSetSections };

// offsets | frames (one H2D) | the three array sets at their stated capacities
// | totals | slots | kinds | words in frame order (kinds and words: one D2H) |
// the decoder's workspace.
struct MixedLayout {
  size_t offs = 0, frames = 0, set[COA_WIRE_MIXED_KINDS][mSetSections] = {}, totals = 0, slots = 0, kinds = 0, words = 0,
         ws = 0, bytes = 0;
  MixedLayout(size_t n, size_t fb) {
    size_t end = 0;
    auto take = [&end](size_t b) {
      const size_t at_ = end;
      end = align_up(at_ + b, 256);
      return at_;
    };
    offs = take((n + 1) * 8);
    frames = take(fb + 4);
    const size_t votes = COA_WIRE_VOTES_BOUND(fb);
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) {
      size_t* at = set[k];
      const bool hdr = k != COA_MSG_VOTE, cert = k == COA_MSG_CERTIFICATE;
      at[mHdata] = take(hdr ? fb + 16 : 0);
      at[mHoff] = take(hdr ? (n + 1) * 8 : 0);
      at[mIds] = take(n * 32);
      at[mAuthors] = take(n * 32);
      at[mOrigins] = take(hdr ? 0 : n * 32);
      at[mSigs] = take(n * 64);
      at[mRounds] = take(n * 8);
      at[mPcounts] = take(hdr ? n * 4 : 0);
      at[mVpks] = take(cert ? votes * 32 + 16 : 0);
      at[mVsigs] = take(cert ? votes * 64 + 16 : 0);
      at[mVoff] = take(cert ? (n + 1) * 8 : 0);
      at[mWords] = take(n * 4);
    }
    totals = take(COA_WIRE_MIXED_TOTALS * 8);
    slots = take(n * 4);
    kinds = take(n * 4);
    words = take(n * 4);
    ws = take(WireMixedWs(n).bytes);
    bytes = end;
  }
};

int wire_fused_mixed(const uint8_t* frames, const uint64_t* offs, size_t n, uint64_t rng_seed, int32_t* kinds_out,
                     uint32_t* verdicts_out) {
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
    // what each verdict call below answers itself; here also for a batch that holds no message
    if (!keys_now(d)->has_prot) return fail(COA_EINVAL, "committee registered without stakes");
    const MixedLayout L(n, fb);
    const size_t back = L.words - L.kinds + n * 4;  // kinds | words
    HIP_TRY(d.pin.ensure(std::max(L.frames + fb + 4, back)));
    HIP_TRY(d.out.ensure(L.bytes));
    uint8_t* h = static_cast<uint8_t*>(d.pin.p);
    uint8_t* b = d.out.as<uint8_t>();
    const Seg segs[2] = {{h + L.offs, offs, (n + 1) * 8}, {h + L.frames, frames, fb}};
    CopyPool::get().copy(segs, fb ? 2 : 1);
    HIP_TRY(hipMemcpyAsync(b, h, L.frames + fb, hipMemcpyHostToDevice, s));
    int32_t* d_kinds = reinterpret_cast<int32_t*>(b + L.kinds);
    uint32_t* d_slots = reinterpret_cast<uint32_t*>(b + L.slots);
    WireMixedArgs a{};
    a.frames = b + L.frames;
    a.offs = reinterpret_cast<const uint64_t*>(b + L.offs);
    a.frame_bytes = fb;
    a.n = (uint32_t)n;
    a.kinds = d_kinds;
    a.slots = d_slots;
    a.totals = reinterpret_cast<uint64_t*>(b + L.totals);
    auto u8 = [&](int k, int sec) { return b + L.set[k][sec]; };
    auto u64 = [&](int k, int sec) { return reinterpret_cast<uint64_t*>(b + L.set[k][sec]); };
    auto u32 = [&](int k, int sec) { return reinterpret_cast<uint32_t*>(b + L.set[k][sec]); };
    for (int k = 0; k < COA_WIRE_MIXED_KINDS; k++) {
      WireSet& o = a.set[k];
      o.ids = u8(k, mIds);
      o.authors = u8(k, mAuthors);
      o.sigs = u8(k, mSigs);
      o.rounds = u64(k, mRounds);
      if (k == COA_MSG_VOTE) {
        o.vorigins = u8(k, mOrigins);
        continue;
      }
      o.hdata = u8(k, mHdata);
      o.hoff = u64(k, mHoff);
      o.pcounts = u32(k, mPcounts);
      if (k == COA_MSG_CERTIFICATE) {
        o.vpks = u8(k, mVpks);
        o.vsigs = u8(k, mVsigs);
        o.voff = u64(k, mVoff);
      }
    }
    mixed_carve(a, b + L.ws);
    HIP_TRY(coa_launch_wire_decode_mixed(a, s));
    // the verdict calls take their counts, the certificate call its votes, as host arguments
    uint64_t* totals = reinterpret_cast<uint64_t*>(h);
    HIP_TRY(hipMemcpyAsync(totals, a.totals, COA_WIRE_MIXED_TOTALS * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const size_t nh = (size_t)totals[0], nvt = (size_t)totals[2], nc = (size_t)totals[3], cvotes = (size_t)totals[5];
    size_t need = 0;
    if (nh) need = std::max(need, coa_message_verdict_workspace_bytes(nh));
    if (nvt) need = std::max(need, coa_message_verdict_workspace_bytes(nvt));
    if (nc) need = std::max({need, coa_certificate_verdict_workspace_bytes(nc, cvotes), ResolveWs(nc, cvotes, 0).bytes});
    if (need) HIP_TRY(d.vws.ensure(need));  // one workspace: the calls follow each other on s
    int rc = COA_OK;
    const int H = COA_MSG_HEADER, V = COA_MSG_VOTE, C = COA_MSG_CERTIFICATE;
    if (nh)
      rc = coa_header_verdict_many_device(d.id, u8(H, mHdata), u64(H, mHoff), u8(H, mIds), u8(H, mAuthors), u8(H, mSigs),
                                          nh, u32(H, mPcounts), u32(H, mWords), d.vws.p, s);
    if (rc == COA_OK && nvt)
      rc = coa_vote_verdict_many_device(d.id, u8(V, mIds), u64(V, mRounds), u8(V, mOrigins), u8(V, mAuthors),
                                        u8(V, mSigs), nvt, u32(V, mWords), d.vws.p, s);
    if (rc == COA_OK && nc) {
      rc = coa_certificate_verdict_many_device(d.id, u8(C, mHdata), u64(C, mHoff), u8(C, mIds), u8(C, mAuthors),
                                               u8(C, mSigs), u64(C, mRounds), u8(C, mVpks), u8(C, mVsigs), u64(C, mVoff),
                                               nc, cvotes, u32(C, mPcounts), u32(C, mWords), d.vws.p, s);
      if (rc == COA_OK)
        rc = coa_certificate_votes_resolve_device(d.id, u8(C, mIds), u8(C, mAuthors), u64(C, mRounds), u8(C, mVpks),
                                                  u8(C, mVsigs), u64(C, mVoff), nc, cvotes, 0, nullptr, rng_seed,
                                                  u32(C, mWords), nullptr, d.vws.p, s);
    }
    if (rc != COA_OK) return rc;
    uint32_t* d_words = reinterpret_cast<uint32_t*>(b + L.words);
    HIP_TRY(coa_launch_wire_scatter(d_kinds, d_slots, u32(H, mWords), u32(V, mWords), u32(C, mWords), d_words,
                                    (uint32_t)n, s));
    HIP_TRY(hipMemcpyAsync(h, d_kinds, back, hipMemcpyDeviceToHost, s));  // kinds and words lie side by side: one D2H
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(kinds_out, h, n * 4);
    std::memcpy(verdicts_out, h + (L.words - L.kinds), n * 4);
    return COA_OK;
  });
}

}  // namespace coa_rt

using namespace coa_rt;

extern "C" {

size_t coa_wire_workspace_bytes(size_t n, size_t frame_bytes) {
  (void)frame_bytes;  // nothing per byte is kept between the passes
  return WireWs(n).bytes;
}

int coa_wire_scan_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                         size_t frame_bytes, int32_t* d_kinds, uint64_t* d_header_bytes, uint64_t* d_votes,
                         void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, d_kinds != nullptr, stream, d, s))
    return e;
  WireArgs a = wire_args(d_frames, d_frame_offsets, n, frame_bytes, d_kinds);
  a.hb = d_header_bytes;
  a.nv = d_votes;
  if (d_header_bytes && d_votes) {  // nothing of the workspace is touched
    HIP_TRY(coa_launch_wire_scan(a, s));
    if (!workspace) HIP_TRY(hipStreamSynchronize(s));
    return COA_OK;
  }
  return with_workspace(*d, s, workspace, d->vws, WireWs(n).bytes, nullptr, [&](void* ws) -> int {
    wire_carve(a, ws);
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
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  const bool ok = d_header_data && d_header_offsets && d_ids && d_origins && d_header_sigs && d_rounds && d_vote_pks &&
                  d_vote_sigs && d_vote_offsets && d_payload_counts && d_kinds && d_totals;
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, ok, stream, d, s)) return e;
  WireArgs a = wire_args(d_frames, d_frame_offsets, n, frame_bytes, d_kinds);
  a.want = COA_MSG_CERTIFICATE;
  a.hdata = d_header_data;
  a.hoff = d_header_offsets;
  a.ids = d_ids;
  a.authors = d_origins;
  a.sigs = d_header_sigs;
  a.rounds = d_rounds;
  a.vpks = d_vote_pks;
  a.vsigs = d_vote_sigs;
  a.voff = d_vote_offsets;
  a.pcounts = d_payload_counts;
  a.totals = d_totals;
  return wire_decode(*d, s, a, workspace);
}

int coa_wire_decode_headers_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                   size_t frame_bytes, uint8_t* d_header_data, uint64_t* d_header_offsets,
                                   uint8_t* d_ids, uint8_t* d_authors, uint8_t* d_sigs, uint32_t* d_payload_counts,
                                   uint64_t* d_rounds, int32_t* d_kinds, uint64_t* d_totals, void* workspace,
                                   void* stream) {
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  const bool ok = d_header_data && d_header_offsets && d_ids && d_authors && d_sigs && d_payload_counts && d_rounds &&
                  d_kinds && d_totals;
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, ok, stream, d, s)) return e;
  WireArgs a = wire_args(d_frames, d_frame_offsets, n, frame_bytes, d_kinds);
  a.want = COA_MSG_HEADER;
  a.hdata = d_header_data;
  a.hoff = d_header_offsets;
  a.ids = d_ids;
  a.authors = d_authors;
  a.sigs = d_sigs;
  a.rounds = d_rounds;
  a.pcounts = d_payload_counts;
  a.totals = d_totals;
  return wire_decode(*d, s, a, workspace);
}

int coa_wire_decode_votes_device(int device, const uint8_t* d_frames, const uint64_t* d_frame_offsets, size_t n,
                                 size_t frame_bytes, uint8_t* d_ids, uint64_t* d_rounds, uint8_t* d_origins,
                                 uint8_t* d_authors, uint8_t* d_sigs, int32_t* d_kinds, uint64_t* d_totals,
                                 void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  Dev* d;
  hipStream_t s;
  const bool ok = d_ids && d_rounds && d_origins && d_authors && d_sigs && d_kinds && d_totals;
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, ok, stream, d, s)) return e;
  WireArgs a = wire_args(d_frames, d_frame_offsets, n, frame_bytes, d_kinds);
  a.want = COA_MSG_VOTE;
  a.ids = d_ids;
  a.rounds = d_rounds;
  a.vorigins = d_origins;
  a.authors = d_authors;
  a.sigs = d_sigs;
  a.totals = d_totals;
  return wire_decode(*d, s, a, workspace);
}

size_t coa_wire_mixed_workspace_bytes(size_t n, size_t frame_bytes) {
  (void)frame_bytes;  // as coa_wire_workspace_bytes
  return WireMixedWs(n).bytes;
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
  const bool ok = d_h_header_data && d_h_header_offsets && d_h_ids && d_h_authors && d_h_sigs && d_h_payload_counts &&
                  d_h_rounds && d_v_ids && d_v_rounds && d_v_origins && d_v_authors && d_v_sigs && d_c_header_data &&
                  d_c_header_offsets && d_c_ids && d_c_origins && d_c_header_sigs && d_c_rounds && d_c_vote_pks &&
                  d_c_vote_sigs && d_c_vote_offsets && d_c_payload_counts && d_kinds && d_slots && d_totals;
  if (const int e = wire_enter(device, d_frames, d_frame_offsets, n, frame_bytes, ok, stream, d, s)) return e;
  WireMixedArgs a{};
  a.frames = d_frames;
  a.offs = d_frame_offsets;
  a.frame_bytes = frame_bytes;
  a.n = (uint32_t)n;
  a.kinds = d_kinds;
  a.slots = d_slots;
  a.totals = d_totals;
  WireSet& h = a.set[COA_MSG_HEADER];
  h.hdata = d_h_header_data;
  h.hoff = d_h_header_offsets;
  h.ids = d_h_ids;
  h.authors = d_h_authors;
  h.sigs = d_h_sigs;
  h.pcounts = d_h_payload_counts;
  h.rounds = d_h_rounds;
  WireSet& v = a.set[COA_MSG_VOTE];
  v.ids = d_v_ids;
  v.rounds = d_v_rounds;
  v.vorigins = d_v_origins;
  v.authors = d_v_authors;
  v.sigs = d_v_sigs;
  WireSet& c = a.set[COA_MSG_CERTIFICATE];
  c.hdata = d_c_header_data;
  c.hoff = d_c_header_offsets;
  c.ids = d_c_ids;
  c.authors = d_c_origins;
  c.sigs = d_c_header_sigs;
  c.rounds = d_c_rounds;
  c.vpks = d_c_vote_pks;
  c.vsigs = d_c_vote_sigs;
  c.voff = d_c_vote_offsets;
  c.pcounts = d_c_payload_counts;
  // no key-cache generation to trail: the decode reads no committee table
  return with_workspace(*d, s, workspace, d->vws, WireMixedWs(n).bytes, nullptr, [&](void* ws) -> int {
    mixed_carve(a, ws);
    HIP_TRY(coa_launch_wire_decode_mixed(a, s));
    return COA_OK;
  });
}

int coa_wire_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, uint64_t rng_seed,
                          int32_t* kinds_out, uint32_t* verdicts_out) {
  return wire_fused_mixed(frames, frame_offsets, n, rng_seed, kinds_out, verdicts_out);
}

int coa_wire_certificate_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n,
                                      uint64_t rng_seed, int32_t* kinds_out, uint32_t* verdicts_out) {
  return wire_fused(COA_MSG_CERTIFICATE, frames, frame_offsets, n, rng_seed, kinds_out, verdicts_out);
}

int coa_wire_header_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kinds_out,
                                 uint32_t* verdicts_out) {
  return wire_fused(COA_MSG_HEADER, frames, frame_offsets, n, 0, kinds_out, verdicts_out);
}

int coa_wire_vote_verdict_many(const uint8_t* frames, const uint64_t* frame_offsets, size_t n, int32_t* kinds_out,
                               uint32_t* verdicts_out) {
  return wire_fused(COA_MSG_VOTE, frames, frame_offsets, n, 0, kinds_out, verdicts_out);
}

}  // extern "C"

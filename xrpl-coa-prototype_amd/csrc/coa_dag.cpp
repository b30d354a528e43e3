// Entries of include/coa_verify.h over the engine core (coa_engine.h): the
// DAG messages -- Certificate / Header / Vote::verify's crypto, their verdicts
// with the protocol checks, and the committee registrations they read.
#include "coa_engine.h"

#include <chrono>
#include <cstdio>
#include <cstring>

#include "coa_protocol_dev.h"
#include "coa_resolve.h"
#include "coa_resolve_ws.h"

namespace coa_rt __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------------
// Certificate::verify crypto (f2 + f3).  Inputs of a shard [lo, hi) are
// packed into the device's pinned staging buffer (coa_stage.h) and copied
// with ONE H2D; the status words come back with one D2H.
// COA_CERT_LANES=1|64 forces the lanes-per-signature variant.
int cert_lanes(size_t jobs) {
  if (env_is("COA_CERT_LANES", "1")) return 1;
  if (env_is("COA_CERT_LANES", "64")) return 64;
  return jobs <= 2048 ? 64 : 1;
}

// The arrays of a certificate launch, device pointers (status and the key
// tables are the caller's to set).
CertArgs cert_args(const uint8_t* hdr_data, const uint64_t* hdr_off, const uint8_t* ids, const uint8_t* origins,
                   const uint8_t* hsigs, const uint64_t* rounds, const uint8_t* vpks, const uint8_t* vsigs,
                   const uint64_t* voff, size_t nc, size_t nv) {
  CertArgs a;
  a.hdr_data = hdr_data;
  a.hdr_off = hdr_off;
  a.ids = reinterpret_cast<const uint32_t*>(ids);
  a.origins = reinterpret_cast<const uint32_t*>(origins);
  a.hsigs = reinterpret_cast<const uint32_t*>(hsigs);
  a.rounds = rounds;
  a.vpks = reinterpret_cast<const uint32_t*>(vpks);
  a.vsigs = reinterpret_cast<const uint32_t*>(vsigs);
  a.voff = voff;
  a.nc = (uint32_t)nc;
  a.nv = (uint32_t)nv;
  a.hdr_blocks = 0;
  return a;
}

// The protocol kernel's view of the arrays of crypto launch a: payload counts
// in, protocol words out.
CertProtArgs cert_prot_args(const CertArgs& a, const uint32_t* pcounts, uint32_t* proto) {
  CertProtArgs q{};
  q.hdr_data = a.hdr_data;
  q.hdr_off = a.hdr_off;
  q.ids = a.ids;
  q.origins = a.origins;
  q.rounds = a.rounds;
  q.vpks = a.vpks;
  q.voff = a.voff;
  q.pcounts = pcounts;
  q.nc = a.nc;
  q.nv = a.nv;
  q.proto = proto;
  return q;
}

// The launch over a block laid out as p at device address base, on
// generation ks.
CertArgs cert_args_packed(const Dev& d, const KeySet& ks, uint8_t* base, const CertPack& p, size_t nc, size_t nv) {
  CertArgs a = cert_args(base + p.hdata.at, reinterpret_cast<const uint64_t*>(base + p.hoff.at), base + p.ids.at,
                         base + p.origins.at, base + p.hsigs.at, reinterpret_cast<const uint64_t*>(base + p.rounds.at),
                         base + p.vpks.at, base + p.vsigs.at, reinterpret_cast<const uint64_t*>(base + p.voff.at), nc,
                         nv);
  key_args(a, d, ks);
  a.status = reinterpret_cast<uint32_t*>(base + p.status.at);
  return a;
}

// Certificates [lo, hi) of `in` inline in ci's buffer (no pinned staging
// copy, no H2D transfer); false when they do not fit (ci untouched).
bool cert_inl_build(CertInl& ci, const CertIn& in, size_t lo, size_t hi) {
  CertPack p;
  if (!cert_inline_pack(ci.buf, COA_CERT_INLINE_BYTES, p, in, lo, hi)) return false;
  ci.off_hoff = (uint32_t)p.hoff.at;
  ci.off_voff = (uint32_t)p.voff.at;
  ci.off_ids = (uint32_t)p.ids.at;
  ci.off_origins = (uint32_t)p.origins.at;
  ci.off_hsigs = (uint32_t)p.hsigs.at;
  ci.off_rounds = (uint32_t)p.rounds.at;
  ci.off_vpks = (uint32_t)p.vpks.at;
  ci.off_vsigs = (uint32_t)p.vsigs.at;
  ci.off_hdr = (uint32_t)p.hdata.at;
  return true;
}

// a's last block publishes nc status words into d.lat_res under a fresh tag.
// d.lat_ctr is allocated on first use: [0] the latency kernels' block
// counter, [1..64] status words; the kernel re-zeroes both.
int cert_publish_prepare(Dev& d, hipStream_t s, size_t nc, CertArgs& a) {
  if (!d.lat_ctr) {
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d.lat_ctr), 65 * 4));
    HIP_TRY(hipMemsetAsync(d.lat_ctr, 0, 65 * 4, s));
  }
  const int rc = lat_res_prepare(d, nc, a.tag);  // may move d.lat_res
  a.host_res = d.lat_res;
  a.done_ctr = d.lat_ctr;
  return rc;
}

// The latency launch with the certificates inline in the kernel arguments:
// for calls whose arrays fit COA_CERT_INLINE_BYTES.  Returns 1 when they do
// not fit (nothing launched).
int cert_inline(Dev& d, const CertIn& in, size_t lo, size_t hi, uint32_t* status_out) {
  const size_t nc = hi - lo;
  const uint64_t nv = in.voff[hi] - in.voff[lo];
  static thread_local CertInl ci;  // ~3 KB, staged on the host; copied into the launch
  if (!cert_inl_build(ci, in, lo, hi)) return 1;
  hipStream_t s = d.stream;
  CertArgs& a = ci.a;
  const KeySetP ks = keys_now(d);  // held until the status words are in
  a = cert_args_packed(d, *ks, nullptr, CertPack{}, nc, nv);
  const int rc = cert_publish_prepare(d, s, nc, a);
  if (rc != COA_OK) return rc;
  a.status = d.lat_ctr + 1;
  HIP_TRY(coa_launch_cert_verify_inl(ci, s));
  return lat_res_wait(d, s, nc, a.tag, status_out + lo);
}

// What a verdict call adds to a shard: the payload counts (null for votes,
// which have none).  The shard then decides the protocol checks of
// coa_protocol.hip on its own stream, over the arrays its crypto launch
// reads, and answers verdict words (include/coa_verify.h, COA_DAG_*) instead
// of raw status words.
struct ProtoIn {
  const uint32_t* pcounts;
};

// The protocol table of generation ks (wanted false: a crypto-only shard
// needs none).
int prot_tab(bool wanted, const KeySet& ks, ProtTab& t) {
  if (!wanted) return COA_OK;
  if (!ks.has_prot) return fail(COA_EINVAL, "committee registered without stakes");
  const uint32_t* w = ks.prot.as<uint32_t>();
  t.keys = ks.ckeys.as<uint32_t>();
  t.stake = w;
  t.woff = w + ks.nkeys;
  t.wids = w + 2 * (size_t)ks.nkeys + 1;
  t.nk = ks.nkeys;
  t.quorum = ks.quorum;
  return COA_OK;
}

// Jobs (header + votes) per chunk of the pipelined certificate path
// (COA_CERT_CHUNK_JOBS, read per call; default 2^17: ~1,900 C3
// certificates, ~19 MB of staging, enough jobs for the persistent
// certificate grid to fill the chip) and chunks in flight
// (COA_CERT_BUFFERS, 2..4, default 3).
size_t cert_chunk_jobs() {
  const long v = env_int("COA_CERT_CHUNK_JOBS", 0);
  return v >= (1 << 12) ? (size_t)v : ((size_t)1 << 17);
}
// The first chunks of a pipelined call are smaller (COA_CERT_RAMP = r, read
// per call, default 1: chunk k < r takes chunk_jobs >> (r - k) jobs), so the
// GPU starts after a half chunk's pack and copy instead of a full one's.
// Host C3 round, same box, 8 alternating pairs: r = 1 +1.4 to +6.7 % over
// r = 0; r = 2 and 3 slower (more chunks); profiles/r05_c3_host_ramp_ab.txt.
int cert_ramp() { return (int)env_int("COA_CERT_RAMP", 1, 0, 4); }
// COA_CERT_PIPE_KEYSORT=1: the pipelined host path's chunks also take
// their jobs in key order (A/B; see coa_committee.hip k_job_count)
bool pipe_keysort() { return env_is("COA_CERT_PIPE_KEYSORT", "1"); }
int cert_buffers() { return (int)env_int("COA_CERT_BUFFERS", 3, 2, 4); }

// One packed block of certificates: page-locked staging h, device copy base.
struct CertBlock {
  CertPack p;
  size_t nc, nv;
  uint8_t* h;
  uint8_t* base;
};

// Packs certificates [lo, hi) into pin (the copies spread over the
// CopyPool) for its device copy dev; pr: with the payload counts.
int cert_pack(CertBlock& b, const CertIn& in, const ProtoIn* pr, size_t lo, size_t hi, PinBuf& pin, DevBuf& dev) {
  b.nc = hi - lo;
  b.nv = in.voff[hi] - in.voff[lo];
  b.p = cert_layout(b.nc, b.nv, in.hdr_off[hi] - in.hdr_off[lo], pr != nullptr);
  HIP_TRY(pin.ensure(b.p.total));
  HIP_TRY(dev.ensure(b.p.total));
  b.h = static_cast<uint8_t*>(pin.p);
  b.base = dev.as<uint8_t>();
  const SegList segs = cert_segments(b.h, b.p, in, pr ? pr->pcounts : nullptr, lo, hi);
  CopyPool::get().copy(segs.s, segs.n);
  return COA_OK;
}

// Block b's H2D copy, the crypto launch and, with a protocol table, the
// protocol kernel and the merge, all on s; `words` is the section that then
// holds the block's answer (status words, or verdict words with t).
int cert_launch(const Dev& d, const KeySet& ks, const ProtTab* t, const CertBlock& b, int lanes, bool key_order,
                uint32_t* scratch, hipStream_t s, Sec& words) {
  const CertPack& p = b.p;
  HIP_TRY(hipMemcpyAsync(b.base, b.h, p.total, hipMemcpyHostToDevice, s));
  CertArgs a = cert_args_packed(d, ks, b.base, p, b.nc, b.nv);
  a.key_order = key_order ? 1u : 0u;
  HIP_TRY(coa_launch_cert_verify(a, lanes, scratch, s));
  words = p.status;
  if (!t) return COA_OK;
  const CertProtArgs q = cert_prot_args(a, reinterpret_cast<const uint32_t*>(b.base + p.pcounts.at),
                                        reinterpret_cast<uint32_t*>(b.base + p.proto.at));
  HIP_TRY(coa_launch_cert_protocol(q, *t, s));
  HIP_TRY(coa_launch_verdict_merge(a.status, q.proto, reinterpret_cast<uint32_t*>(b.base + p.verd.at), a.nc, s));
  words = p.verd;
  return COA_OK;
}

// A shard's answer: section `words` of device block base through its
// staging h to out (one D2H), once the stream has drained.
int read_back(uint8_t* h, const uint8_t* base, const Sec& words, uint32_t* out, hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(h + words.at, base + words.at, words.bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  std::memcpy(out, h + words.at, words.bytes);
  return COA_OK;
}

// Certificates [lo, hi) on one device in chunks, up to cert_buffers() in
// flight on as many streams, each with its own page-locked staging and
// device buffers: while the GPU runs chunk k's kernel, chunk k + 1's copy
// crosses PCIe and the host packs chunk k + 2 (CopyPool).  With two buffer
// sets the host could only pack chunk k + 2 once chunk k had finished, so a
// round took about (pack + copy + kernel) / 2 per chunk.  Answer words as
// cert_shard's (a chunk ends between certificates, and a verdict word's vote
// index is relative to its certificate, so chunking does not change them).
// COA_CERT_TRACE=1 prints the host's pack and wait time per call.
int cert_shard_pipelined(Dev& d, const CertIn& in, const ProtoIn* pr, size_t lo, size_t hi, uint32_t* out) {
  const int nb = cert_buffers();
  const std::vector<size_t> cuts = cert_chunk_cuts(in.voff, lo, hi, cert_chunk_jobs(), cert_ramp());
  hipStream_t st[4] = {d.stream, nullptr, nullptr, nullptr};
  for (int b = 1; b < nb; b++) {
    if (!d.cstreams[b - 1]) HIP_TRY(hipStreamCreateWithFlags(&d.cstreams[b - 1], hipStreamNonBlocking));
    st[b] = d.cstreams[b - 1];
  }
  const KeySetP ks = keys_now(d);  // held until every chunk is done
  ProtTab t;
  int rc = prot_tab(pr != nullptr, *ks, t);
  if (rc != COA_OK) return rc;
  struct Pending {
    bool busy = false;
    size_t lo = 0;
    Sec words;
  } pend[4];
  const bool trace = env_is("COA_CERT_TRACE", "1");
  double t_pack = 0, t_wait = 0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  auto drain = [&](int b) -> int {
    if (!pend[b].busy) return COA_OK;
    const double t0 = trace ? now() : 0;
    HIP_TRY(hipStreamSynchronize(st[b]));
    if (trace) t_wait += now() - t0;
    std::memcpy(out + pend[b].lo, static_cast<uint8_t*>(d.pinc[b].p) + pend[b].words.at, pend[b].words.bytes);
    pend[b].busy = false;
    return COA_OK;
  };
  for (size_t k = 0; k + 1 < cuts.size(); k++) {
    const int b = (int)(k % nb);
    rc = drain(b);  // this buffer set's previous chunk
    if (rc != COA_OK) return rc;
    const size_t clo = cuts[k], chi = cuts[k + 1];
    const double t0 = trace ? now() : 0;
    CertBlock blk;
    rc = cert_pack(blk, in, pr, clo, chi, d.pinc[b], d.certc[b]);
    if (rc != COA_OK) return rc;
    if (trace) t_pack += now() - t0;
    HIP_TRY(d.cscrc[b].ensure(coa_cert_scratch_bytes(blk.nc + blk.nv, pipe_keysort())));
    Sec words;
    rc = cert_launch(d, *ks, pr ? &t : nullptr, blk, 1, pipe_keysort(), d.cscrc[b].as<uint32_t>(), st[b], words);
    if (rc != COA_OK) return rc;
    HIP_TRY(hipMemcpyAsync(blk.h + words.at, blk.base + words.at, words.bytes, hipMemcpyDeviceToHost, st[b]));
    pend[b] = {true, clo, words};
  }
  for (size_t k = 0; k < (size_t)nb; k++) {
    rc = drain((int)((cuts.size() - 1 + k) % nb));  // oldest first
    if (rc != COA_OK) return rc;
  }
  if (trace)
    fprintf(stderr, "[coa] cert pipeline: %zu chunks x %d buffers, pack %.3f ms, wait %.3f ms\n", cuts.size() - 1, nb,
            t_pack * 1e3, t_wait * 1e3);
  return COA_OK;
}

// Fast path for certificates [lo, hi) on one device (its lock held): raw
// status words out, or with pr their verdict words.  publish: the latency
// variant writes its status words straight into page-locked host memory (no
// D2H copy, no stream synchronisation).
int cert_shard(Dev& d, const CertIn& in, const ProtoIn* pr, size_t lo, size_t hi, uint32_t* out,
               bool publish = false) {
  const size_t nc = hi - lo;
  const uint64_t nv = in.voff[hi] - in.voff[lo];
  const int lanes = cert_lanes(nc + nv);
  publish = publish && lanes == 64;
  if (publish && !env_is("COA_CERT_INLINE", "0")) {
    const int rc = cert_inline(d, in, lo, hi, out);
    if (rc != 1) return rc;
  }
  if (!publish && nc + nv >= 2 * cert_chunk_jobs() && !env_is("COA_CERT_PIPELINE", "0"))
    return cert_shard_pipelined(d, in, pr, lo, hi, out);
  const KeySetP ks = keys_now(d);  // held until the answer words are in
  ProtTab t;
  int rc = prot_tab(pr != nullptr, *ks, t);
  if (rc != COA_OK) return rc;
  CertBlock b;
  rc = cert_pack(b, in, pr, lo, hi, d.pin, d.cert);
  if (rc != COA_OK) return rc;
  hipStream_t s = d.stream;
  if (publish) {  // the last block writes the status words to host memory
    HIP_TRY(hipMemcpyAsync(b.base, b.h, b.p.total, hipMemcpyHostToDevice, s));
    CertArgs a = cert_args_packed(d, *ks, b.base, b.p, nc, nv);
    rc = cert_publish_prepare(d, s, nc, a);
    if (rc != COA_OK) return rc;
    HIP_TRY(coa_launch_cert_verify(a, lanes, nullptr, s));
    return lat_res_wait(d, s, nc, a.tag, out + lo);
  }
  if (lanes == 1) HIP_TRY(d.cscr.ensure(coa_cert_scratch_bytes(nc + nv, false)));
  Sec words;
  rc = cert_launch(d, *ks, pr ? &t : nullptr, b, lanes, false, d.cscr.as<uint32_t>(), s, words);
  if (rc != COA_OK) return rc;
  return read_back(b.h, b.base, words, out + lo, s);
}

// Exact (non-cached) resolution of certificates `idx`: header signatures by
// verify_strict (only when `hdr_too`), votes by the RLC kernels over
// Certificate::digest.  ORs COA_CST_BAD_* into status.
int cert_resolve(const CertIn& in, const std::vector<size_t>& idx, bool hdr_too, uint64_t seed, uint32_t* status) {
  if (idx.empty()) return COA_OK;
  const size_t m = idx.size();
  // Certificate::digest inputs
  std::vector<uint8_t> cin(m * 72);
  for (size_t j = 0; j < m; j++) {
    const size_t c = idx[j];
    digest_input(&cin[j * 72], in.ids + c * 32, in.rounds[c], in.origins + c * 32);
  }
  // the digests of certificates `sel` (indices into idx) into gm
  std::vector<uint8_t> gm(m * 32), gv(m), vp, vs;
  auto digests = [&](const std::vector<size_t>& sel) -> int {
    if (sel.empty()) return COA_OK;
    std::vector<uint8_t> sin(sel.size() * 72), dig(sel.size() * 64);
    std::vector<uint64_t> soff(sel.size() + 1);
    for (size_t k = 0; k < sel.size(); k++) {
      std::memcpy(&sin[k * 72], &cin[sel[k] * 72], 72);
      soff[k] = k * 72;
    }
    soff[sel.size()] = sel.size() * 72;
    const int r = coa_sha512_many(sin.data(), soff.data(), sel.size(), dig.data());
    for (size_t k = 0; r == COA_OK && k < sel.size(); k++) std::memcpy(&gm[sel[k] * 32], &dig[k * 64], 32);
    return r;
  };
  std::vector<uint64_t> goff(m + 1, 0);
  for (size_t j = 0; j < m; j++) {
    const size_t c = idx[j];
    const uint64_t a = in.voff[c], b = in.voff[c + 1];
    vp.insert(vp.end(), in.vpks + a * 32, in.vpks + b * 32);
    vs.insert(vs.end(), in.vsigs + a * 64, in.vsigs + b * 64);
    goff[j + 1] = goff[j] + (b - a);
  }
  std::vector<uint8_t> hv(m, 0);
  const size_t nvotes = goff[m];
  int rc;
  if (hdr_too && nvotes + m <= lat_max() && !env_is("COA_BATCH_LAT", "0") && !env_is("COA_RESOLVE_ONE_LAUNCH", "0")) {
    // ONE latency launch for the votes (the verify_batch prefilter: items
    // [0, nvotes), each message Certificate::digest hashed in the kernel from
    // cin, LatArgs::cd_in) and the header signatures (plain verify_strict:
    // items [nvotes, nvotes + m)): a certificate with keys outside the
    // committee took a digest launch, a prefilter launch and a header launch,
    // one after the other
    std::vector<uint8_t> msgs(m * 32, 0), pks(vp), sigs(vs);
    std::vector<uint32_t> msg_of(nvotes + m);
    for (size_t j = 0; j < m; j++) {
      const uint32_t jj = (uint32_t)j;
      std::memcpy(&msgs[j * 32], &jj, 4);  // the certificate's index: its digest input in cin
      for (uint64_t i = goff[j]; i < goff[j + 1]; i++) msg_of[i] = (uint32_t)j;
      msg_of[nvotes + j] = (uint32_t)(m + j);
      const size_t c = idx[j];
      msgs.insert(msgs.end(), in.ids + c * 32, in.ids + c * 32 + 32);
      pks.insert(pks.end(), in.origins + c * 32, in.origins + c * 32 + 32);
      sigs.insert(sigs.end(), in.hsigs + c * 64, in.hsigs + c * 64 + 64);
    }
    std::vector<uint8_t> v(nvotes + m);
    {
      std::unique_lock<std::mutex> l;
      Dev& d = lat_dev(l);
      HIP_TRY(hipSetDevice(d.id));
      rc = lat_verify(d, msgs.data(), pks.data(), sigs.data(), nvotes + m, v.data(), msg_of.data(), nvotes,
                      cin.data(), m);
      if (rc != COA_OK) return rc;
    }
    // a group every vote of which passed is Ok for every z; the others take
    // the exact path with their own weights (as batch_groups_impl's prefilter)
    std::vector<size_t> open;
    for (size_t j = 0; j < m; j++) {
      bool pass = true;
      for (uint64_t i = goff[j]; i < goff[j + 1]; i++) pass = pass && v[i] == 0;
      gv[j] = pass ? 0 : 1;
      if (!pass) open.push_back(j);
      hv[j] = v[nvotes + j] ? 1 : 0;
    }
    rc = digests(open);  // only the groups the prefilter did not accept need their digest on the host
    if (rc != COA_OK) return rc;
    for (size_t j : open) {
      const uint64_t a = goff[j], n = goff[j + 1] - a;
      const uint64_t offs[2] = {0, n};
      rc = batch_groups_impl(&gm[j * 32], vp.data() + a * 32, vs.data() + a * 64, offs, 1, nullptr, seed, &gv[j], 0,
                             false);
      if (rc != COA_OK) return rc;
    }
    for (size_t j = 0; j < m; j++)
      status[idx[j]] |= (gv[j] ? COA_CST_BAD_VOTES : 0u) | (hv[j] ? COA_CST_BAD_HEADER_SIG : 0u);
    return COA_OK;
  }
  std::vector<size_t> all(m);
  for (size_t j = 0; j < m; j++) all[j] = j;
  rc = digests(all);
  if (rc != COA_OK) return rc;
  rc = batch_groups_impl(gm.data(), vp.data(), vs.data(), goff.data(), m, nullptr, seed, gv.data());
  if (rc != COA_OK) return rc;
  if (hdr_too) {
    std::vector<uint8_t> hm(m * 32), hp(m * 32), hs(m * 64);
    for (size_t j = 0; j < m; j++) {
      const size_t c = idx[j];
      std::memcpy(&hm[j * 32], in.ids + c * 32, 32);
      std::memcpy(&hp[j * 32], in.origins + c * 32, 32);
      std::memcpy(&hs[j * 64], in.hsigs + c * 64, 64);
    }
    rc = coa_ed25519_verify_strict_many(hm.data(), 32, hp.data(), hs.data(), m, hv.data());
    if (rc != COA_OK) return rc;
  }
  for (size_t j = 0; j < m; j++) {
    status[idx[j]] |= (gv[j] ? COA_CST_BAD_VOTES : 0u) | (hv[j] ? COA_CST_BAD_HEADER_SIG : 0u);
  }
  return COA_OK;
}

// Raw status words of the fused kernel -> exact verdicts: a certificate with
// a key outside the registered committee is re-decided entirely (header
// signature by verify_strict, votes by the RLC kernels; its digest check does
// not use the cache and stands), one whose votes were inconclusive (a vote
// failed its own equation, or a key has torsion) by the RLC kernels alone.
// Shared by certificates_impl and the queue's resolver
// (coa_certificate_resolve_raw), which hands over the words of the
// certificates its window could not answer at once.
int resolve_raw(const CertIn& in, size_t n, uint32_t* st, uint64_t rng_seed) {
  std::vector<size_t> uncached, rlc;
  for (size_t i = 0; i < n; i++) {
    if (st[i] & COA_CST_UNCACHED) {
      st[i] &= COA_CST_BAD_HEADER_ID;  // the digest check does not use the cache
      uncached.push_back(i);
    } else if ((st[i] & COA_CST_VOTES_INCONCLUSIVE) && !(st[i] & COA_CST_BAD_VOTES)) {
      rlc.push_back(i);
    }
  }
  // weights for the exact re-decision only: OS entropy is a syscall, and the
  // common call (every certificate decided by the cached kernel) needs none
  const uint64_t seed = rng_seed || (uncached.empty() && rlc.empty()) ? rng_seed : os_entropy_seed();
  int rc = cert_resolve(in, uncached, true, seed, st);
  if (rc != COA_OK) return rc;
  return cert_resolve(in, rlc, false, seed, st);
}

// The argument checks of the host-pointer certificate calls (out: the call's
// output array).
int cert_in_check(const CertIn& in, size_t n, const void* out) {
  if (!in.hdr_off || !in.ids || !in.origins || !in.hsigs || !in.rounds || !in.voff || !out)
    return fail(COA_EINVAL, "null argument");
  if (!offsets_monotone(in.hdr_off, n) || !offsets_monotone(in.voff, n))
    return fail(COA_EINVAL, "offsets not monotone");
  if (in.voff[0] != 0) return fail(COA_EINVAL, "vote_offsets[0] must be 0");
  if (in.hdr_off[n] > in.hdr_off[0] && !in.hdr_data) return fail(COA_EINVAL, "null header data");
  if (in.voff[n] && (!in.vpks || !in.vsigs)) return fail(COA_EINVAL, "null vote arrays");
  return check_n(n + in.voff[n]);
}

int certificates_impl(const CertIn& in, size_t n, uint64_t rng_seed, uint8_t* status_out) {
  if (n == 0) return COA_OK;
  int rc = cert_in_check(in, n, status_out);
  if (rc != COA_OK) return rc;
  std::vector<uint32_t> st(n, 0);
  if (cert_lanes(n + in.voff[n]) == 64) {  // latency path: one idle context, no stream sync
    std::unique_lock<std::mutex> l;
    Dev& d = lat_dev(l);
    HIP_TRY(hipSetDevice(d.id));
    rc = cert_shard(d, in, nullptr, 0, n, st.data(), true);
  } else {
    rc = for_shards(
        n, [&](Dev& d, size_t lo, size_t hi) -> int { return cert_shard(d, in, nullptr, lo, hi, st.data()); },
        n + in.voff[n]);
  }
  if (rc != COA_OK) return rc;
  rc = resolve_raw(in, n, st.data(), rng_seed);
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < n; i++) status_out[i] = (uint8_t)(st[i] & 7u);
  return COA_OK;
}

// ------------------------------------------------------------------------
// Header::verify / Vote::verify crypto for many messages (k_msg_verify).  A
// shard [lo, hi) is packed into the context's pinned staging and copied with
// ONE H2D; the raw status words come back with one D2H.
// The arrays of a message launch, device pointers (hdr_* null: votes; rounds
// and origins null: headers); the key tables are the caller's to set.
MsgArgs msg_args(const uint8_t* hdr_data, const uint64_t* hdr_off, const uint8_t* ids, const uint64_t* rounds,
                 const uint8_t* origins, const uint8_t* authors, const uint8_t* sigs, size_t n, uint32_t* status) {
  MsgArgs a{};
  a.hdr_data = hdr_data;
  a.hdr_off = hdr_off;
  a.ids = reinterpret_cast<const uint32_t*>(ids);
  a.rounds = rounds;
  a.origins = reinterpret_cast<const uint32_t*>(origins);
  a.authors = reinterpret_cast<const uint32_t*>(authors);
  a.sigs = reinterpret_cast<const uint32_t*>(sigs);
  a.n = (uint32_t)n;
  a.status = status;
  return a;
}

// The protocol kernel's view of the arrays of crypto launch a (pcounts null:
// votes, which have no payload).
MsgProtArgs msg_prot_args(const MsgArgs& a, const uint32_t* pcounts, uint32_t* proto) {
  MsgProtArgs q{};
  q.hdr_data = a.hdr_data;
  q.hdr_off = a.hdr_off;
  q.pcounts = pcounts;
  q.authors = a.authors;
  q.n = a.n;
  q.proto = proto;
  return q;
}

// Messages [lo, hi) on one context (its lock held): raw status words out, or
// with pr their verdict words (cert_shard's protocol tail, for messages).
int msg_shard(Dev& d, const MsgIn& in, const ProtoIn* pr, size_t lo, size_t hi, uint32_t* out) {
  const size_t n = hi - lo;
  const KeySetP ks = keys_now(d);  // held until the answer words are in
  ProtTab t;
  const int rc = prot_tab(pr != nullptr, *ks, t);
  if (rc != COA_OK) return rc;
  const MsgPack p = msg_layout(n, in.votes, in.votes ? 0 : in.hdr_off[hi] - in.hdr_off[lo], pr != nullptr);
  HIP_TRY(d.pin.ensure(p.total));
  HIP_TRY(d.cert.ensure(p.total));
  HIP_TRY(d.cscr.ensure(coa_msg_scratch_bytes(n)));
  uint8_t* h = static_cast<uint8_t*>(d.pin.p);
  const SegList segs = msg_segments(h, p, in, pr ? pr->pcounts : nullptr, lo, hi);
  CopyPool::get().copy(segs.s, segs.n);
  hipStream_t s = d.stream;
  uint8_t* base = d.cert.as<uint8_t>();
  HIP_TRY(hipMemcpyAsync(base, h, p.total, hipMemcpyHostToDevice, s));
  const uint8_t* none = nullptr;  // the other shape's arrays
  MsgArgs a = msg_args(in.votes ? none : base + p.hdata.at,
                       reinterpret_cast<const uint64_t*>(in.votes ? none : base + p.hoff.at), base + p.ids.at,
                       reinterpret_cast<const uint64_t*>(in.votes ? base + p.rounds.at : none),
                       in.votes ? base + p.origins.at : none, base + p.authors.at, base + p.sigs.at, n,
                       reinterpret_cast<uint32_t*>(base + p.status.at));
  key_args(a, d, *ks);
  HIP_TRY(coa_launch_msg_verify(a, d.cscr.as<uint32_t>(), s));
  if (!pr) return read_back(h, base, p.status, out + lo, s);
  const MsgProtArgs q = msg_prot_args(a, in.votes ? nullptr : reinterpret_cast<const uint32_t*>(base + p.pcounts.at),
                                      reinterpret_cast<uint32_t*>(base + p.proto.at));
  HIP_TRY(coa_launch_msg_protocol(q, t, s));
  HIP_TRY(coa_launch_verdict_merge(a.status, q.proto, reinterpret_cast<uint32_t*>(base + p.verd.at), a.n, s));
  return read_back(h, base, p.verd, out + lo, s);
}

// Raw words of all n messages, then the exact re-decision of the items whose
// author is not registered through the uncached path: verify_strict over the
// id (headers) or Vote::digest (votes).  A header's digest bit does not use
// the cache and stands.
int messages_resolve(const MsgIn& in, size_t n, uint32_t* st);
int messages_impl(const MsgIn& in, size_t n, std::vector<uint32_t>& st) {
  st.assign(n, 0);
  int rc = for_shards(n, [&](Dev& d, size_t lo, size_t hi) -> int { return msg_shard(d, in, nullptr, lo, hi, st.data()); });
  if (rc != COA_OK) return rc;
  return messages_resolve(in, n, st.data());
}

// The re-decision alone (coa_message_resolve_raw: the aggregation queue's
// resolver has the raw words already).
int messages_resolve(const MsgIn& in, size_t n, uint32_t* st) {
  int rc = COA_OK;
  std::vector<size_t> open;
  for (size_t i = 0; i < n; i++)
    if (st[i] & COA_CST_UNCACHED) open.push_back(i);
  if (open.empty()) return COA_OK;
  const size_t m = open.size();
  std::vector<uint8_t> msgs(m * 32), pks(m * 32), sigs(m * 64), v(m);
  for (size_t j = 0; j < m; j++) {
    std::memcpy(&pks[j * 32], in.authors + open[j] * 32, 32);
    std::memcpy(&sigs[j * 64], in.sigs + open[j] * 64, 64);
  }
  if (in.votes) {  // Vote::digest inputs
    std::vector<uint8_t> vin(m * 72);
    std::vector<uint64_t> off(m + 1);
    for (size_t j = 0; j < m; j++) {
      const size_t i = open[j];
      digest_input(&vin[j * 72], in.ids + i * 32, in.rounds[i], in.origins + i * 32);
      off[j] = j * 72;
    }
    off[m] = m * 72;
    rc = coa_sha512_trunc32_many(vin.data(), off.data(), m, msgs.data());
    if (rc != COA_OK) return rc;
  } else {
    for (size_t j = 0; j < m; j++) std::memcpy(&msgs[j * 32], in.ids + open[j] * 32, 32);
  }
  rc = coa_ed25519_verify_strict_many(msgs.data(), 32, pks.data(), sigs.data(), m, v.data());
  if (rc != COA_OK) return rc;
  for (size_t j = 0; j < m; j++)
    st[open[j]] = (st[open[j]] & COA_CST_BAD_HEADER_ID) | (v[j] ? COA_CST_BAD_HEADER_SIG : 0u);
  return COA_OK;
}

// Device-resident form of either shape (a.status zeroed here).
int messages_device(int device, MsgArgs a, void* workspace, void* stream) {
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  const KeySetP ks = keys_now(*d);  // pinned (the queue) or current
  key_args(a, *d, *ks);
  HIP_TRY(hipMemsetAsync(a.status, 0, (size_t)a.n * 4, s));
  return with_workspace(*d, s, workspace, d->cscr, coa_msg_scratch_bytes(a.n), &ks, [&](void* ws) -> int {
    HIP_TRY(coa_launch_msg_verify(a, static_cast<uint32_t*>(ws), s));
    return COA_OK;
  });
}

// ------------------------------------------------------------------------
// Verdicts: the crypto status words above merged on the device with the
// protocol checks of coa_protocol.hip (include/coa_verify.h, COA_DAG_*).
// The host-pointer forms are the crypto shards with their protocol tail.
int message_verdicts(const MsgIn& in, const uint32_t* pcounts, size_t n, uint32_t* out) {
  const ProtoIn pr{pcounts};
  return for_shards(n, [&](Dev& d, size_t lo, size_t hi) -> int { return msg_shard(d, in, &pr, lo, hi, out); });
}

// Device-resident verdict calls: `crypto` enqueues the *_verify_many_device
// launch with its raw words at `raw` and its workspace at `ws`; the protocol
// kernel and the merge follow on the same stream.  workspace NULL: the
// context's own, and the call waits for its stream.
size_t verdict_ws_bytes(size_t crypto_bytes, size_t n) { return align_up(crypto_bytes, 256) + 2 * align_up(n * 4, 256); }

template <class Crypto, class Proto>
int verdicts_device(int device, size_t n, size_t crypto_bytes, uint32_t* d_verdicts, void* workspace, void* stream,
                    Crypto crypto, Proto proto) {
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  const KeySetP ks = keys_now(*d);
  ProtTab t;
  int rc = prot_tab(true, *ks, t);
  if (rc != COA_OK) return rc;
  // the crypto call inside always gets a workspace: it takes no lock itself
  return with_workspace(*d, s, workspace, d->vws, verdict_ws_bytes(crypto_bytes, n), &ks, [&](void* base) -> int {
    uint8_t* ws = static_cast<uint8_t*>(base);
    uint32_t* raw = reinterpret_cast<uint32_t*>(ws + align_up(crypto_bytes, 256));
    uint32_t* pw = reinterpret_cast<uint32_t*>(ws + align_up(crypto_bytes, 256) + align_up(n * 4, 256));
    {
      const KeyScope scope(ks);
      const int r = crypto(raw, ws, s);
      if (r != COA_OK) return r;
    }
    HIP_TRY(proto(pw, t, s));
    HIP_TRY(coa_launch_verdict_merge(raw, pw, d_verdicts, (uint32_t)n, s));
    return COA_OK;
  });
}

}  // namespace coa_rt

using namespace coa_rt;

extern "C" {

int coa_committee_register(const uint8_t* pks, size_t n) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n && !pks) return fail(COA_EINVAL, "null argument");
  if (n > (1u << 20)) return fail(COA_EINVAL, "committee too large");
  std::vector<std::array<uint32_t, 8>> keys(n);
  for (size_t i = 0; i < n; i++) std::memcpy(keys[i].data(), pks + i * 32, 32);
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  // one generation per device (shared by its contexts)
  rc = on_each_device([&](DevShared& sh) { return build_keyset(sh, keys); });
  if (rc != COA_OK) return rc;
  return (int)keys.size();
}

int coa_certificate_verify_publish(int device, const uint8_t* h_base, uint8_t* d_base, size_t in_bytes,
                                   const CertPack* p, size_t n, size_t n_votes, uint32_t* d_ctr, uint32_t* host_res,
                                   uint32_t tag, void* stream) {
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (n > 64 || cert_lanes(n + n_votes) != 64) return 1;  // not the latency kernel's size: nothing enqueued
  if (!h_base || !d_base || !p || !d_ctr || !host_res || tag == 0) return fail(COA_EINVAL, "null argument");
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  const KeySetP ks = keys_now(*d);  // pinned (the queue) or current; see coa_lat_verify_device
  static thread_local CertInl ci;
  if (!env_is("COA_CERT_INLINE", "0") && cert_inl_build(ci, cert_view(h_base, *p), 0, n)) {
    CertArgs& a = ci.a;
    a = cert_args_packed(*d, *ks, nullptr, CertPack{}, n, n_votes);
    a.status = d_ctr + 1;
    a.host_res = host_res;
    a.done_ctr = d_ctr;
    a.tag = tag;
    HIP_TRY(coa_launch_cert_verify_inl(ci, s));
    return trail_keys(*d, ks, s);
  }
  HIP_TRY(hipMemcpyAsync(d_base, h_base, in_bytes, hipMemcpyHostToDevice, s));
  CertArgs a = cert_args_packed(*d, *ks, d_base, *p, n, n_votes);
  a.status = d_ctr + 1;
  a.host_res = host_res;
  a.done_ctr = d_ctr;
  a.tag = tag;
  HIP_TRY(coa_launch_cert_verify(a, 64, nullptr, s));
  return trail_keys(*d, ks, s);
}

int coa_committee_key_flags(uint32_t* flags_out, size_t cap) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  Dev& d = *g_devs[0];
  std::lock_guard<std::mutex> l(d.mu);
  const KeySetP ks = keys_now(d);
  const size_t nk = std::min<size_t>(ks->nkeys, cap);
  if (nk == 0) return (int)ks->nkeys;
  if (!flags_out) return fail(COA_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(d.id));
  HIP_TRY(hipMemcpyAsync(flags_out, ks->kflags.p, nk * 4, hipMemcpyDeviceToHost, d.stream));
  HIP_TRY(hipStreamSynchronize(d.stream));
  return (int)ks->nkeys;
}

int coa_certificate_verify_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                size_t n, uint64_t rng_seed, uint8_t* status_out) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  const CertIn in{header_data, header_offsets, ids, origins, header_sigs, rounds, vote_pks, vote_sigs, vote_offsets};
  return certificates_impl(in, n, rng_seed, status_out);
}

int coa_certificate_verify(const uint8_t* header_data, size_t header_len, const uint8_t id[32],
                           const uint8_t origin[32], const uint8_t header_sig[64], uint64_t round,
                           const uint8_t* vote_pks, const uint8_t* vote_sigs, size_t n_votes, uint64_t rng_seed) {
  const uint64_t hoff[2] = {0, (uint64_t)header_len};
  const uint64_t voff[2] = {0, (uint64_t)n_votes};
  uint8_t st = 0;
  const int rc = coa_certificate_verify_many(header_data, hoff, id, origin, header_sig, &round, vote_pks, vote_sigs,
                                             voff, 1, rng_seed, &st);
  return rc != COA_OK ? rc : (int)st;
}

int coa_certificate_resolve_raw(const uint8_t* ids, const uint8_t* origins, const uint8_t* header_sigs,
                                const uint64_t* rounds, const uint8_t* vote_pks, const uint8_t* vote_sigs,
                                const uint64_t* vote_offsets, size_t n, uint32_t* raw, uint8_t* status_out) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!ids || !origins || !header_sigs || !rounds || !vote_offsets || !raw || !status_out ||
      (vote_offsets[n] && (!vote_pks || !vote_sigs)))
    return fail(COA_EINVAL, "null argument");
  // the exact path never reads the header bytes (Header::digest was checked
  // by the fused kernel and its bit stands)
  const CertIn in{nullptr, nullptr, ids, origins, header_sigs, rounds, vote_pks, vote_sigs, vote_offsets};
  rc = resolve_raw(in, n, raw, 0);
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < n; i++) status_out[i] = (uint8_t)(raw[i] & 7u);
  return COA_OK;
}

size_t coa_certificate_workspace_bytes(size_t n, size_t n_votes) {
  return coa_cert_scratch_bytes(n + n_votes, true);  // the public device call sorts by key
}

int coa_certificate_verify_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                       const uint8_t* d_ids, const uint8_t* d_origins, const uint8_t* d_header_sigs,
                                       const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                       const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                       size_t n_votes, uint32_t* d_status, void* workspace, void* stream) {
  // one device-resident round: jobs in key order
  return coa_certificate_verify_many_device_order(device, d_header_data, d_header_offsets, d_ids, d_origins,
                                                  d_header_sigs, d_rounds, d_vote_pks, d_vote_sigs, d_vote_offsets, n,
                                                  n_votes, d_status, workspace, stream, 1);
}

int coa_certificate_verify_many_device_order(int device, const uint8_t* d_header_data,
                                             const uint64_t* d_header_offsets, const uint8_t* d_ids,
                                             const uint8_t* d_origins, const uint8_t* d_header_sigs,
                                             const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                             const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                             size_t n_votes, uint32_t* d_status, void* workspace, void* stream,
                                             int key_order) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (n == 0) return COA_OK;
  if (!d_header_offsets || !d_ids || !d_origins || !d_header_sigs || !d_rounds || !d_vote_offsets || !d_status ||
      (n_votes && (!d_vote_pks || !d_vote_sigs)))
    return fail(COA_EINVAL, "null argument");
  if (check_n(n + n_votes) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  CertArgs a = cert_args(d_header_data, d_header_offsets, d_ids, d_origins, d_header_sigs, d_rounds, d_vote_pks,
                         d_vote_sigs, d_vote_offsets, n, n_votes);
  const KeySetP ks = keys_now(*d);  // pinned (the queue) or current; see coa_lat_verify_device
  key_args(a, *d, *ks);
  a.status = d_status;
  a.key_order = key_order ? 1u : 0u;
  const int lanes = cert_lanes(n + n_votes);
  HIP_TRY(hipMemsetAsync(d_status, 0, n * 4, s));
  // not with_workspace: the latency variant needs no workspace at all, so a
  // call without one still returns with its kernel running
  if (workspace || lanes == 64) {
    HIP_TRY(coa_launch_cert_verify(a, lanes, static_cast<uint32_t*>(workspace), s));
    return trail_keys(*d, ks, s);
  }
  std::lock_guard<std::mutex> l(d->mu);
  HIP_TRY(d->cscr.ensure(coa_cert_scratch_bytes(n + n_votes, a.key_order != 0)));
  HIP_TRY(coa_launch_cert_verify(a, lanes, d->cscr.as<uint32_t>(), s));
  HIP_TRY(hipStreamSynchronize(s));  // engine-owned workspace: drain before release
  return COA_OK;
}

int coa_header_verify_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                           const uint8_t* authors, const uint8_t* sigs, size_t n, uint8_t* status_out) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!header_offsets || !ids || !authors || !sigs || !status_out) return fail(COA_EINVAL, "null argument");
  if (!offsets_monotone(header_offsets, n)) return fail(COA_EINVAL, "offsets not monotone");
  if (header_offsets[n] > header_offsets[0] && !header_data) return fail(COA_EINVAL, "null header data");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  const MsgIn in{header_data, header_offsets, ids, nullptr, nullptr, authors, sigs, false};
  std::vector<uint32_t> st;
  rc = messages_impl(in, n, st);
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < n; i++) status_out[i] = (uint8_t)(st[i] & 3u);
  return COA_OK;
}

int coa_vote_verify_many(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins, const uint8_t* authors,
                         const uint8_t* sigs, size_t n, uint8_t* verdicts_out) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!ids || !rounds || !origins || !authors || !sigs || !verdicts_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  const MsgIn in{nullptr, nullptr, ids, rounds, origins, authors, sigs, true};
  std::vector<uint32_t> st;
  rc = messages_impl(in, n, st);
  if (rc != COA_OK) return rc;
  for (size_t i = 0; i < n; i++) verdicts_out[i] = (st[i] & COA_CST_BAD_HEADER_SIG) ? 1 : 0;
  return COA_OK;
}

int coa_message_resolve_raw(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins,
                            const uint8_t* authors, const uint8_t* sigs, size_t n, uint32_t* raw) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!ids || !authors || !sigs || !raw || (rounds && !origins)) return fail(COA_EINVAL, "null argument");
  const MsgIn in{nullptr, nullptr, ids, rounds, origins, authors, sigs, rounds != nullptr};
  return messages_resolve(in, n, raw);
}

// k_msg_verify_lat over device arrays, on the pinned (the queue) or current
// key-cache generation; with `verdict`, k_msg_verdict_lat against that
// generation's protocol table and the headers' payload counts (returns 1,
// nothing enqueued, when it has none).
static int msg_lat_launch(int device, const CoaMsgLatIn* in, uint32_t* d_status, uint32_t* d_ctr, uint32_t* host_res,
                          uint32_t tag, void* stream, bool verdict = false, const uint32_t* h_pcounts = nullptr) {
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!in) return fail(COA_EINVAL, "null argument");
  const size_t n = in->nh + in->nv;
  if (n == 0) return COA_OK;
  if ((in->nh && (!in->hdr_data || !in->hdr_off || !in->hids || !in->hauthors || !in->hsigs)) ||
      (in->nv && (!in->vids || !in->vrounds || !in->vorigins || !in->vauthors || !in->vsigs)) || !d_status ||
      (verdict && in->nh && !h_pcounts))
    return fail(COA_EINVAL, "null argument");
  if (check_n(2 * n) != COA_OK) return COA_EINVAL;  // 2 nh + nv blocks
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  MsgVerdictLatArgs a{};
  a.hdr_data = in->hdr_data;
  a.hdr_off = in->hdr_off;
  a.ids = reinterpret_cast<const uint32_t*>(in->hids);
  a.hauthors = reinterpret_cast<const uint32_t*>(in->hauthors);
  a.hsigs = reinterpret_cast<const uint32_t*>(in->hsigs);
  a.vids = reinterpret_cast<const uint32_t*>(in->vids);
  a.vrounds = in->vrounds;
  a.vorigins = reinterpret_cast<const uint32_t*>(in->vorigins);
  a.vauthors = reinterpret_cast<const uint32_t*>(in->vauthors);
  a.vsigs = reinterpret_cast<const uint32_t*>(in->vsigs);
  a.nh = (uint32_t)in->nh;
  a.nv = (uint32_t)in->nv;
  const KeySetP ks = keys_now(*d);  // see coa_lat_verify_device
  if (verdict && !ks->has_prot) return 1;
  key_args(static_cast<MsgLatArgs&>(a), *d, *ks);
  a.status = d_status;
  if (host_res) {
    a.host_res = host_res;
    a.done_ctr = d_ctr;
    a.tag = tag;
  } else {
    HIP_TRY(hipMemsetAsync(d_status, 0, n * 4, s));
  }
  if (verdict) {
    (void)prot_tab(true, *ks, a.t);
    a.hpcounts = h_pcounts;
    HIP_TRY(coa_launch_msg_verdict_lat(a, s));
  } else {
    HIP_TRY(coa_launch_msg_verify_lat(a, s));
  }
  return trail_keys(*d, ks, s);
}

int coa_msg_lat_verify_device(int device, const CoaMsgLatIn* in, uint32_t* d_status, void* stream) {
  return msg_lat_launch(device, in, d_status, nullptr, nullptr, 0, stream);
}

int coa_msg_lat_verify_publish(int device, const CoaMsgLatIn* in, uint32_t* d_ctr, uint32_t* host_res, uint32_t tag,
                               void* stream) {
  if (!in || !d_ctr || !host_res || tag == 0) return fail(COA_EINVAL, "null argument or zero tag");
  if (in->nh + in->nv > 64) return fail(COA_EINVAL, "more messages than the result words hold");
  return msg_lat_launch(device, in, d_ctr + 1, d_ctr, host_res, tag, stream);
}

int coa_msg_lat_verdict_device(int device, const CoaMsgLatIn* in, const uint32_t* h_pcounts, uint32_t* d_words,
                               void* stream) {
  return msg_lat_launch(device, in, d_words, nullptr, nullptr, 0, stream, true, h_pcounts);
}

int coa_msg_lat_verdict_publish(int device, const CoaMsgLatIn* in, const uint32_t* h_pcounts, uint32_t* d_ctr,
                                uint32_t* host_res, uint32_t tag, void* stream) {
  if (!in || !d_ctr || !host_res || tag == 0) return fail(COA_EINVAL, "null argument or zero tag");
  if (in->nh + in->nv > 64) return fail(COA_EINVAL, "more messages than the result words hold");
  return msg_lat_launch(device, in, d_ctr + 1, d_ctr, host_res, tag, stream, true, h_pcounts);
}

int coa_window_verdict_device(int device, const CoaWindowVerdictIn* in, void* stream) {
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!in) return fail(COA_EINVAL, "null argument");
  const size_t n = in->nc + in->nh + in->nv;
  if (n == 0) return COA_OK;
  if ((in->nc && (!in->c_hdr_data || !in->c_hdr_off || !in->c_ids || !in->c_origins || !in->c_rounds || !in->c_voff ||
                  !in->c_pcounts || !in->cert_raw || (in->n_votes && !in->c_vpks))) ||
      (in->nh && (!in->h_hdr_data || !in->h_hdr_off || !in->h_pcounts || !in->h_authors)) ||
      (in->nv && !in->v_authors) || ((in->nh || in->nv) && !in->msg_raw) || !in->words)
    return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK || check_n(in->n_votes) != COA_OK) return COA_EINVAL;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  const KeySetP ks = keys_now(*d);  // pinned (the queue) or current
  if (!ks->has_prot) return 1;      // the window's verdict requests get COA_EINVAL; nothing to run
  ProtTab t;
  (void)prot_tab(true, *ks, t);
  WindowVerdictArgs a{};
  a.cert.hdr_data = in->c_hdr_data;
  a.cert.hdr_off = in->c_hdr_off;
  a.cert.ids = reinterpret_cast<const uint32_t*>(in->c_ids);
  a.cert.origins = reinterpret_cast<const uint32_t*>(in->c_origins);
  a.cert.rounds = in->c_rounds;
  a.cert.vpks = reinterpret_cast<const uint32_t*>(in->c_vpks);
  a.cert.voff = in->c_voff;
  a.cert.pcounts = in->c_pcounts;
  a.cert.nc = (uint32_t)in->nc;
  a.cert.nv = (uint32_t)in->n_votes;
  if (in->nh) {
    a.hdr.hdr_data = in->h_hdr_data;
    a.hdr.hdr_off = in->h_hdr_off;
    a.hdr.pcounts = in->h_pcounts;
    a.hdr.authors = reinterpret_cast<const uint32_t*>(in->h_authors);
    a.hdr.n = (uint32_t)in->nh;
  }
  a.vote.authors = reinterpret_cast<const uint32_t*>(in->v_authors);
  a.vote.n = (uint32_t)in->nv;
  a.cert_raw = in->cert_raw;
  a.msg_raw = in->msg_raw;
  a.words = in->words;
  HIP_TRY(coa_launch_window_verdict(a, t, s));
  return trail_keys(*d, ks, s);
}

size_t coa_message_workspace_bytes(size_t n) { return coa_msg_scratch_bytes(n); }

int coa_header_verify_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                  const uint8_t* d_ids, const uint8_t* d_authors, const uint8_t* d_sigs, size_t n,
                                  uint32_t* d_status, void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!d_header_data || !d_header_offsets || !d_ids || !d_authors || !d_sigs || !d_status)
    return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return messages_device(device, msg_args(d_header_data, d_header_offsets, d_ids, nullptr, nullptr, d_authors, d_sigs, n,
                                          d_status), workspace, stream);
}

int coa_vote_verify_many_device(int device, const uint8_t* d_ids, const uint64_t* d_rounds, const uint8_t* d_origins,
                                const uint8_t* d_authors, const uint8_t* d_sigs, size_t n, uint32_t* d_status,
                                void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!d_ids || !d_rounds || !d_origins || !d_authors || !d_sigs || !d_status)
    return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return messages_device(device, msg_args(nullptr, nullptr, d_ids, d_rounds, d_origins, d_authors, d_sigs, n, d_status),
                         workspace, stream);
}

// ------------------------------------------------------------- verdicts
int coa_committee_register_authorities(const uint8_t* pks, const uint32_t* stakes, const uint32_t* worker_ids,
                                       const uint64_t* worker_offsets, size_t n) {
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  CoaProtTable pt;
  std::string err;
  if (!coa_prot_build(pks, stakes, worker_ids, worker_offsets, n, pt, err)) return fail(COA_EINVAL, err);
  rc = on_each_device([&](DevShared& sh) { return build_keyset(sh, pt.keys, &pt); });
  if (rc != COA_OK) return rc;
  return (int)pt.keys.size();
}

int coa_certificate_verdict_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                                 const uint8_t* origins, const uint8_t* header_sigs, const uint64_t* rounds,
                                 const uint8_t* vote_pks, const uint8_t* vote_sigs, const uint64_t* vote_offsets,
                                 size_t n, uint64_t rng_seed, const uint32_t* payload_counts,
                                 uint32_t* verdicts_out) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  const CertIn in{header_data, header_offsets, ids, origins, header_sigs, rounds, vote_pks, vote_sigs, vote_offsets};
  rc = cert_in_check(in, n, payload_counts ? verdicts_out : nullptr);
  if (rc != COA_OK) return rc;
  if (!coa_prot_counts_fit(in.hdr_off, payload_counts, n))
    return fail(COA_EINVAL, "a payload count overruns its header");
  const ProtoIn pr{payload_counts};
  rc = for_shards(
      n, [&](Dev& d, size_t lo, size_t hi) -> int { return cert_shard(d, in, &pr, lo, hi, verdicts_out); },
      n + in.voff[n]);
  if (rc != COA_OK) return rc;
  // what stays open: every earlier check passed and the votes need the exact
  // random-linear-combination check
  std::vector<size_t> open;
  for (size_t i = 0; i < n; i++)
    if (verdicts_out[i] == COA_DAG_VOTES_OPEN) open.push_back(i);
  if (open.empty()) return COA_OK;
  std::vector<uint32_t> st(n, 0);
  rc = cert_resolve(in, open, false, rng_seed ? rng_seed : os_entropy_seed(), st.data());
  if (rc != COA_OK) return rc;
  for (size_t i : open) verdicts_out[i] = (st[i] & COA_CST_BAD_VOTES) ? COA_DAG_INVALID_VOTES : COA_DAG_OK;
  return COA_OK;
}

int coa_header_verdict_many(const uint8_t* header_data, const uint64_t* header_offsets, const uint8_t* ids,
                            const uint8_t* authors, const uint8_t* sigs, size_t n, const uint32_t* payload_counts,
                            uint32_t* verdicts_out) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!header_offsets || !ids || !authors || !sigs || !payload_counts || !verdicts_out)
    return fail(COA_EINVAL, "null argument");
  if (!offsets_monotone(header_offsets, n)) return fail(COA_EINVAL, "offsets not monotone");
  if (header_offsets[n] > header_offsets[0] && !header_data) return fail(COA_EINVAL, "null header data");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  if (!coa_prot_counts_fit(header_offsets, payload_counts, n))
    return fail(COA_EINVAL, "a payload count overruns its header");
  const MsgIn in{header_data, header_offsets, ids, nullptr, nullptr, authors, sigs, false};
  return message_verdicts(in, payload_counts, n, verdicts_out);
}

int coa_vote_verdict_many(const uint8_t* ids, const uint64_t* rounds, const uint8_t* origins, const uint8_t* authors,
                          const uint8_t* sigs, size_t n, uint32_t* verdicts_out) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!ids || !rounds || !origins || !authors || !sigs || !verdicts_out) return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  const MsgIn in{nullptr, nullptr, ids, rounds, origins, authors, sigs, true};
  return message_verdicts(in, nullptr, n, verdicts_out);
}

size_t coa_certificate_verdict_workspace_bytes(size_t n, size_t n_votes) {
  return verdict_ws_bytes(coa_certificate_workspace_bytes(n, n_votes), n);
}

int coa_certificate_verdict_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                        const uint8_t* d_ids, const uint8_t* d_origins, const uint8_t* d_header_sigs,
                                        const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                        const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                        size_t n_votes, const uint32_t* d_payload_counts, uint32_t* d_verdicts,
                                        void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!d_header_offsets || !d_ids || !d_origins || !d_header_sigs || !d_rounds || !d_vote_offsets ||
      !d_payload_counts || !d_verdicts || (n_votes && (!d_vote_pks || !d_vote_sigs)))
    return fail(COA_EINVAL, "null argument");
  if (check_n(n + n_votes) != COA_OK) return COA_EINVAL;
  return verdicts_device(
      device, n, coa_certificate_workspace_bytes(n, n_votes), d_verdicts, workspace, stream,
      [&](uint32_t* raw, void* ws, hipStream_t s) {
        return coa_certificate_verify_many_device(device, d_header_data, d_header_offsets, d_ids, d_origins,
                                                  d_header_sigs, d_rounds, d_vote_pks, d_vote_sigs, d_vote_offsets, n,
                                                  n_votes, raw, ws, s);
      },
      [&](uint32_t* pw, const ProtTab& t, hipStream_t s) {
        const CertArgs a = cert_args(d_header_data, d_header_offsets, d_ids, d_origins, d_header_sigs, d_rounds,
                                     d_vote_pks, d_vote_sigs, d_vote_offsets, n, n_votes);
        return coa_launch_cert_protocol(cert_prot_args(a, d_payload_counts, pw), t, s);
      });
}

size_t coa_certificate_votes_resolve_workspace_bytes(size_t n, size_t n_votes, size_t open_votes_cap) {
  return ResolveWs(n, n_votes, open_votes_cap).bytes;
}

int coa_certificate_votes_resolve_device(int device, const uint8_t* d_ids, const uint8_t* d_origins,
                                         const uint64_t* d_rounds, const uint8_t* d_vote_pks,
                                         const uint8_t* d_vote_sigs, const uint64_t* d_vote_offsets, size_t n,
                                         size_t n_votes, size_t open_votes_cap, const uint8_t* d_zs, uint64_t rng_seed,
                                         uint32_t* d_verdicts, uint32_t* d_counts, void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  if (!d_ids || !d_origins || !d_rounds || !d_vote_offsets || !d_verdicts || (n_votes && (!d_vote_pks || !d_vote_sigs)))
    return fail(COA_EINVAL, "null argument");
  if (check_n(n + n_votes) != COA_OK) return COA_EINVAL;
  const int rc = ensure_init();
  if (rc != COA_OK) return rc;
  Dev* d;
  hipStream_t s;
  if (const int e = enter_device(device, stream, d, s)) return e;
  ResolveArgs a{};
  a.ids = reinterpret_cast<const uint32_t*>(d_ids);
  a.origins = reinterpret_cast<const uint32_t*>(d_origins);
  a.rounds = d_rounds;
  a.vpks = d_vote_pks;
  a.vsigs = d_vote_sigs;
  a.voff = d_vote_offsets;
  a.zs = reinterpret_cast<const uint32_t*>(d_zs);
  // derived weights: OS entropy is drawn here, on the host, and only passed on
  a.seed = d_zs ? 0 : (rng_seed ? rng_seed : os_entropy_seed());
  a.n = (uint32_t)n;
  a.n_votes = (uint32_t)n_votes;
  a.cap = (uint32_t)std::min(open_votes_cap, n_votes);  // 0 and n_votes both mean every vote
  a.verdicts = d_verdicts;
  a.counts_out = d_counts;
  // no key-cache generation to trail: the call reads no committee table
  return with_workspace(*d, s, workspace, d->vws, ResolveWs(n, n_votes, a.cap).bytes, nullptr, [&](void* ws) -> int {
    HIP_TRY(coa_launch_votes_resolve(a, static_cast<uint8_t*>(ws), d->btab, s));
    return COA_OK;
  });
}

size_t coa_message_verdict_workspace_bytes(size_t n) { return verdict_ws_bytes(coa_message_workspace_bytes(n), n); }

int coa_header_verdict_many_device(int device, const uint8_t* d_header_data, const uint64_t* d_header_offsets,
                                   const uint8_t* d_ids, const uint8_t* d_authors, const uint8_t* d_sigs, size_t n,
                                   const uint32_t* d_payload_counts, uint32_t* d_verdicts, void* workspace,
                                   void* stream) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!d_header_data || !d_header_offsets || !d_ids || !d_authors || !d_sigs || !d_payload_counts || !d_verdicts)
    return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return verdicts_device(
      device, n, coa_message_workspace_bytes(n), d_verdicts, workspace, stream,
      [&](uint32_t* raw, void* ws, hipStream_t s) {
        return coa_header_verify_many_device(device, d_header_data, d_header_offsets, d_ids, d_authors, d_sigs, n, raw,
                                             ws, s);
      },
      [&](uint32_t* pw, const ProtTab& t, hipStream_t s) {
        const MsgArgs a = msg_args(d_header_data, d_header_offsets, d_ids, nullptr, nullptr, d_authors, d_sigs, n, nullptr);
        return coa_launch_msg_protocol(msg_prot_args(a, d_payload_counts, pw), t, s);
      });
}

int coa_vote_verdict_many_device(int device, const uint8_t* d_ids, const uint64_t* d_rounds, const uint8_t* d_origins,
                                 const uint8_t* d_authors, const uint8_t* d_sigs, size_t n, uint32_t* d_verdicts,
                                 void* workspace, void* stream) {
  if (n == 0) return COA_OK;
  int rc = ensure_init();
  if (rc != COA_OK) return rc;
  if (!d_ids || !d_rounds || !d_origins || !d_authors || !d_sigs || !d_verdicts)
    return fail(COA_EINVAL, "null argument");
  if (check_n(n) != COA_OK) return COA_EINVAL;
  return verdicts_device(
      device, n, coa_message_workspace_bytes(n), d_verdicts, workspace, stream,
      [&](uint32_t* raw, void* ws, hipStream_t s) {
        return coa_vote_verify_many_device(device, d_ids, d_rounds, d_origins, d_authors, d_sigs, n, raw, ws, s);
      },
      [&](uint32_t* pw, const ProtTab& t, hipStream_t s) {
        const MsgArgs a = msg_args(nullptr, nullptr, d_ids, d_rounds, d_origins, d_authors, d_sigs, n, nullptr);
        return coa_launch_msg_protocol(msg_prot_args(a, nullptr, pw), t, s);
      });
}

}  // extern "C"

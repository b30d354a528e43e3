// What an aggregation-queue window's staging blocks hold (coa_queue_hip.cpp):
// the layout of the input and output blocks of one launch, the packer of the
// launch's parts, the scatter of the outputs back to the parts, and the
// gather / write-back halves of the resolver.  Host code only (no HIP), so
// tests/sanitize/qstage_driver.cpp builds it with plain g++.  The sections of
// a block are read through coa_stage.h's cert_view / msg_view, over the
// page-locked block and the device block alike.
#pragma once
#include "coa_queue.h"
#include "coa_stage.h"

namespace coa_q {

// Input block: every section the parts' arrays one after another in part
// order, offsets rebased to the section.  Output block: what the device
// writes.  Sections start at multiples of 256.
struct WindowPack {
  // signatures: 128-byte records msg | pk | R | s (the latency kernel), or
  // msgs | pks | sigs
  Sec v_recs, v_msgs, v_pks, v_sigs;
  // the nine certificate arrays (hdata with 16 bytes of slack); pcounts, the
  // certificates' u32 payload counts, only in a window with verdict requests
  CertPack cert;
  Sec d_data, d_off;  // digest inputs (16 bytes of slack) and their nd + 1 offsets
  MsgPack hdr;     // ids, authors, sigs, hoff, hdata (slack as above), pcounts as cert's; empty without headers
  MsgPack vote;    // ids, rounds, origins, authors, sigs
  size_t in_total = 0;
  Sec o_sigs;   // nv verdict bytes, or nv words for the latency kernel
  Sec o_certs;  // nc raw status words
  Sec o_digs;   // nd x 64
  Sec o_msgs;   // the headers' raw status words, then the votes'
  // verdict words (k_window_verdict) of the certificates, then the headers,
  // then the votes: only in a window with verdict requests
  Sec o_words;
  size_t out_total = 0;
};

inline WindowPack window_layout(const Launch& L, bool sig_lat) {
  WindowPack p;
  Carve c{256};
  p.v_recs = c.take(sig_lat ? L.nv * 128 : 0);
  p.v_msgs = c.take(sig_lat ? 0 : L.nv * 32), p.v_pks = c.take(sig_lat ? 0 : L.nv * 32);
  p.v_sigs = c.take(sig_lat ? 0 : L.nv * 64);
  p.cert.hdata = c.take(L.hbytes + 16), p.cert.hoff = c.take((L.nc + 1) * 8);
  p.cert.ids = c.take(L.nc * 32), p.cert.origins = c.take(L.nc * 32), p.cert.hsigs = c.take(L.nc * 64);
  p.cert.rounds = c.take(L.nc * 8);
  p.cert.vpks = c.take(L.nvotes * 32), p.cert.vsigs = c.take(L.nvotes * 64), p.cert.voff = c.take((L.nc + 1) * 8);
  p.cert.pcounts = c.take(L.verdicts() ? L.nc * 4 : 0);
  p.d_data = c.take(L.dbytes + 16), p.d_off = c.take((L.nd + 1) * 8);
  p.hdr.hdata = c.take(L.nhd ? L.hdbytes + 16 : 0), p.hdr.hoff = c.take(L.nhd ? (L.nhd + 1) * 8 : 0);
  p.hdr.ids = c.take(L.nhd * 32), p.hdr.authors = c.take(L.nhd * 32), p.hdr.sigs = c.take(L.nhd * 64);
  p.hdr.pcounts = c.take(L.verdicts() ? L.nhd * 4 : 0);
  p.vote.ids = c.take(L.nvt * 32), p.vote.rounds = c.take(L.nvt * 8), p.vote.origins = c.take(L.nvt * 32);
  p.vote.authors = c.take(L.nvt * 32), p.vote.sigs = c.take(L.nvt * 64);
  p.in_total = c.end;
  Carve o{256};
  p.o_sigs = o.take(sig_lat ? L.nv * 4 : L.nv);
  p.o_certs = o.take(L.nc * 4);
  p.o_digs = o.take(L.nd * 64);
  p.o_msgs = o.take((L.nhd + L.nvt) * 4);
  p.o_words = o.take(L.verdicts() ? (L.nc + L.nhd + L.nvt) * 4 : 0);
  p.out_total = o.end;
  return p;
}

// The launch's parts into input block h laid out as p = window_layout(L,
// sig_lat): the latency records, the certificates' small fixed fields and the
// rebased offset arrays are written here; every other array (a C3
// certificate's header input and votes are ~9.7 KB of its 9.9) is appended to
// `bulk` for the caller to copy.
inline void window_pack(uint8_t* h, const WindowPack& p, const Launch& L, std::vector<Seg>& bulk) {
  auto copy = [&bulk](void* dst, const void* src, size_t bytes) {
    if (bytes) bulk.push_back({dst, src, bytes});
  };
  auto u64 = [h](const Sec& s) { return reinterpret_cast<uint64_t*>(h + s.at); };
  uint64_t *cho = u64(p.cert.hoff), *cvo = u64(p.cert.voff), *dof = u64(p.d_off), *hdo = u64(p.hdr.hoff);
  cho[0] = cvo[0] = dof[0] = 0;
  if (L.nhd) hdo[0] = 0;
  size_t v = 0, c = 0, cv = 0, hb = 0, dn = 0, db = 0, mh = 0, mhb = 0, mt = 0;
  // payload counts: zero for every crypto request, a verdict request's own
  // (a part's vectors reach as far as its last verdict request)
  auto counts = [h](const Sec& s, size_t at, const std::vector<uint32_t>& pc, size_t n) {
    if (!s.bytes) return;
    uint32_t* to = reinterpret_cast<uint32_t*>(h + s.at) + at;
    std::memset(to, 0, n * 4);
    if (!pc.empty()) std::memcpy(to, pc.data(), std::min(pc.size(), n) * 4);
  };
  for (const Window* w : L.parts) {
    counts(p.cert.pcounts, c, w->c_pcounts, w->nc);
    counts(p.hdr.pcounts, mh, w->hd_pcounts, w->nhd);
    if (p.v_recs.bytes) {
      for (size_t i = 0; i < w->nv; i++) {
        uint8_t* r = h + p.v_recs.at + (v + i) * 128;
        std::memcpy(r, w->v_msgs.data() + i * 32, 32);
        std::memcpy(r + 32, w->v_pks.data() + i * 32, 32);
        std::memcpy(r + 64, w->v_sigs.data() + i * 64, 64);
      }
    } else if (w->nv) {
      copy(h + p.v_msgs.at + v * 32, w->v_msgs.data(), w->nv * 32);
      copy(h + p.v_pks.at + v * 32, w->v_pks.data(), w->nv * 32);
      copy(h + p.v_sigs.at + v * 64, w->v_sigs.data(), w->nv * 64);
    }
    v += w->nv;
    // certificates from their refs (the window's own bytes, or a borrowed
    // request's arrays)
    for (size_t i = 0; i < w->nc; i++, c++) {
      const Window::CertRef& r = w->c_refs[i];
      copy(h + p.cert.hdata.at + hb, r.hdr, r.hlen);
      hb += r.hlen;
      cho[c + 1] = hb;
      std::memcpy(h + p.cert.ids.at + c * 32, r.id, 32);
      std::memcpy(h + p.cert.origins.at + c * 32, r.origin, 32);
      std::memcpy(h + p.cert.hsigs.at + c * 64, r.hsig, 64);
      std::memcpy(h + p.cert.rounds.at + c * 8, &r.round, 8);
      copy(h + p.cert.vpks.at + cv * 32, r.vpks, r.nv * 32);
      copy(h + p.cert.vsigs.at + cv * 64, r.vsigs, r.nv * 64);
      cv += r.nv;
      cvo[c + 1] = cv;
    }
    if (w->nd) {
      copy(h + p.d_data.at + db, w->d_data.data(), w->d_data.size());
      for (size_t i = 1; i <= w->nd; i++) dof[dn + i] = db + w->d_offs[i];
      dn += w->nd;
      db += w->d_data.size();
    }
    if (w->nhd) {
      copy(h + p.hdr.hdata.at + mhb, w->hd_data.data(), w->hd_data.size());
      for (size_t i = 1; i <= w->nhd; i++) hdo[mh + i] = mhb + w->hd_offs[i];
      copy(h + p.hdr.ids.at + mh * 32, w->hd_ids.data(), w->nhd * 32);
      copy(h + p.hdr.authors.at + mh * 32, w->hd_authors.data(), w->nhd * 32);
      copy(h + p.hdr.sigs.at + mh * 64, w->hd_sigs.data(), w->nhd * 64);
      mh += w->nhd;
      mhb += w->hd_data.size();
    }
    if (w->nvt) {
      copy(h + p.vote.ids.at + mt * 32, w->vt_ids.data(), w->nvt * 32);
      copy(h + p.vote.rounds.at + mt * 8, w->vt_rounds.data(), w->nvt * 8);
      copy(h + p.vote.origins.at + mt * 32, w->vt_origins.data(), w->nvt * 32);
      copy(h + p.vote.authors.at + mt * 32, w->vt_authors.data(), w->nvt * 32);
      copy(h + p.vote.sigs.at + mt * 64, w->vt_sigs.data(), w->nvt * 64);
      mt += w->nvt;
    }
  }
}

// How a window's results come back.  The three publish routes are windows of
// one kind and at most COA_PUBLISH_WORDS items whose kernel writes
// (tag << 8) | word per item into the slot's page-locked result words; the
// staged route copies the output block back.
#define COA_PUBLISH_WORDS 64
enum Route { ROUTE_STAGED, ROUTE_SIG_INLINE, ROUTE_CERT_PUBLISH, ROUTE_MSG_PUBLISH };

// Raw message status words (a published word's tag ignored) -> the
// headers' COA_CERT_BAD_HEADER_* bits and the votes' verdicts; a message by an
// author outside the committee is left open for the resolver, a header's
// digest bit kept.  A verdict request is never left open: its word of `hw` /
// `vw` (the window's verdict words; null when none were computed, the words
// then stay "failed") answers it.  hw == hst / vw == vst: the status words are
// k_msg_verdict_lat's verdict words themselves, message codes in 8 bits under
// a published word's tag.
inline void scatter_messages(Window& w, const uint32_t* hst, const uint32_t* vst, const uint32_t* hw = nullptr,
                             const uint32_t* vw = nullptr) {
  w.m_defer.clear();
  for (size_t i = 0; i < w.nhd; i++) {
    if (w.verdict_header(i)) {
      if (hw) w.hd_words[i] = hw == hst ? hw[i] & 0xffu : hw[i];
      continue;
    }
    const bool open = (hst[i] & COA_CST_UNCACHED) != 0;
    if (open) w.m_defer.push_back((uint32_t)i);
    w.hd_out[i] = (uint8_t)(hst[i] & (open ? 1u : 3u));
  }
  for (size_t i = 0; i < w.nvt; i++) {
    if (w.verdict_vote(i)) {
      if (vw) w.vt_words[i] = vw == vst ? vw[i] & 0xffu : vw[i];
      continue;
    }
    if (vst[i] & COA_CST_UNCACHED) w.m_defer.push_back((uint32_t)(w.nhd + i));
    w.vt_out[i] = (vst[i] & COA_CST_BAD_HEADER_SIG) ? 1 : 0;
  }
}

// Raw certificate status words -> COA_CERT_* bits; the certificates the
// fused kernel could not decide alone keep their raw words and are left
// open for the resolver.  A verdict request gets its word of `cw` (as in
// scatter_messages) and is left open only when that is COA_DAG_VOTES_OPEN:
// every earlier check passed and the votes need the exact check.
inline void scatter_certs(Window& w, const uint32_t* st, const uint32_t* cw = nullptr) {
  w.c_raw.assign(st, st + w.nc);
  w.c_defer.clear();
  for (size_t c = 0; c < w.nc; c++) {
    if (w.verdict_cert(c)) {
      if (cw) w.c_words[c] = cw[c];
      if (cw && cw[c] == COA_DAG_VOTES_OPEN) w.c_defer.push_back((uint32_t)c);
      continue;
    }
    // exactly the words coa_certificate_resolve_raw re-decides: a key
    // outside the committee, or inconclusive votes not already bad
    const bool open = (st[c] & COA_CST_UNCACHED) ||
                      ((st[c] & COA_CST_VOTES_INCONCLUSIVE) && !(st[c] & COA_CST_BAD_VOTES));
    if (open) w.c_defer.push_back((uint32_t)c);
    w.c_out[c] = (uint8_t)(st[c] & 7u);
  }
}

// Output block `out` (laid out as p) back to the launch's parts; on a publish
// route that kind's words are read from `pub` instead.  What the kernels left
// open, and every bare vote batch, is marked for the resolver.
inline void window_scatter(const Launch& L, const WindowPack& p, const uint8_t* out, Route route,
                           const uint32_t* pub) {
  auto words = [&](const Sec& s, Route published) {
    return route == published ? pub : reinterpret_cast<const uint32_t*>(out + s.at);
  };
  const uint32_t* sst = words(p.o_sigs, ROUTE_SIG_INLINE);
  const uint32_t* cst = words(p.o_certs, ROUTE_CERT_PUBLISH);
  const uint32_t* mst = words(p.o_msgs, ROUTE_MSG_PUBLISH);
  // the verdict words, when the window has the section and the kernel ran
  const uint32_t* vw = p.o_words.bytes && L.verdict_rc == COA_OK && route == ROUTE_STAGED && !L.msg_words
                           ? reinterpret_cast<const uint32_t*>(out + p.o_words.at)
                           : nullptr;
  auto at = [vw](size_t i) { return vw ? vw + i : nullptr; };
  // ... or, from k_msg_verdict_lat, the messages' own words (a published
  // word's tag is taken off as the word is read)
  const bool mw = L.msg_words && L.verdict_rc == COA_OK;
  const bool sig_lat = p.v_recs.bytes != 0;
  size_t v = 0, c = 0, dn = 0, mh = 0, mt = 0;
  for (Window* w : L.parts) {
    if (mw)
      scatter_messages(*w, mst + mh, mst + L.nhd + mt, mst + mh, mst + L.nhd + mt);
    else
      scatter_messages(*w, mst + mh, mst + L.nhd + mt, at(L.nc + mh), at(L.nc + L.nhd + mt));
    if (w->nv && sig_lat) {
      for (size_t i = 0; i < w->nv; i++) w->v_out[i] = (uint8_t)(sst[v + i] & 0xffu);
    } else if (w->nv) {
      std::memcpy(w->v_out.data(), out + p.o_sigs.at + v, w->nv);
    }
    for (size_t i = 0; i < w->nd; i++) std::memcpy(&w->d_out[i * 32], out + p.o_digs.at + (dn + i) * 64, 32);
    if (w->nc && route == ROUTE_CERT_PUBLISH) {
      uint32_t st[COA_PUBLISH_WORDS];
      for (size_t i = 0; i < w->nc; i++) st[i] = cst[c + i] & 0xffu;  // the tag off
      scatter_certs(*w, st);
    } else if (w->nc) {
      scatter_certs(*w, cst + c, at(c));
    }
    w->g_defer = w->ng > 0;
    v += w->nv;
    c += w->nc;
    dn += w->nd;
    mh += w->nhd;
    mt += w->nvt;
  }
}

// What the windows of one resolver pass left open, gathered into the
// contiguous host arrays the exact engine calls take: window order, then
// index order.
struct Deferred {
  // certificates (coa_certificate_resolve_raw), vote offsets rebased
  std::vector<uint8_t> c_ids, c_origins, c_hsigs, c_vpks, c_vsigs;
  std::vector<uint64_t> c_rounds, c_voff{0};
  std::vector<uint32_t> c_raw;
  // messages (coa_message_resolve_raw): [0] headers, [1] votes; a header's raw
  // word carries its digest bit
  std::vector<uint8_t> m_ids[2], m_authors[2], m_sigs[2], m_origins;
  std::vector<uint64_t> m_rounds;
  std::vector<uint32_t> m_raw[2];
  // bare vote batches (coa_ed25519_verify_batch_groups)
  std::vector<uint8_t> g_msgs, g_pks, g_sigs;
  std::vector<uint64_t> g_off{0};
};

inline Deferred gather_deferred(const std::vector<Window*>& ws) {
  Deferred d;
  auto put = [](std::vector<uint8_t>& to, const uint8_t* p, size_t n) { to.insert(to.end(), p, p + n); };
  for (const Window* w : ws) {
    for (uint32_t c : w->c_defer) {
      const Window::CertRef& r = w->c_refs[c];
      put(d.c_ids, r.id, 32);
      put(d.c_origins, r.origin, 32);
      put(d.c_hsigs, r.hsig, 64);
      d.c_rounds.push_back(r.round);
      put(d.c_vpks, r.vpks, r.nv * 32);
      put(d.c_vsigs, r.vsigs, r.nv * 64);
      d.c_voff.push_back(d.c_vpks.size() / 32);
      d.c_raw.push_back(w->c_raw[c]);
    }
    for (uint32_t m : w->m_defer) {
      const bool vote = m >= w->nhd;
      const size_t i = vote ? m - w->nhd : m;
      put(d.m_ids[vote], (vote ? w->vt_ids : w->hd_ids).data() + i * 32, 32);
      put(d.m_authors[vote], (vote ? w->vt_authors : w->hd_authors).data() + i * 32, 32);
      put(d.m_sigs[vote], (vote ? w->vt_sigs : w->hd_sigs).data() + i * 64, 64);
      if (vote) {
        put(d.m_origins, w->vt_origins.data() + i * 32, 32);
        d.m_rounds.push_back(w->vt_rounds[i]);
      }
      d.m_raw[vote].push_back(COA_CST_UNCACHED | (vote ? 0u : (uint32_t)(w->hd_out[i] & 1u)));
    }
    if (w->g_defer) {
      d.g_msgs.insert(d.g_msgs.end(), w->g_msgs.begin(), w->g_msgs.end());
      d.g_pks.insert(d.g_pks.end(), w->g_pks.begin(), w->g_pks.end());
      d.g_sigs.insert(d.g_sigs.end(), w->g_sigs.begin(), w->g_sigs.end());
      for (size_t g = 1; g <= w->ng; g++) d.g_off.push_back(d.g_off.back() + (w->g_offs[g] - w->g_offs[g - 1]));
    }
  }
  return d;
}

// The answers back to the items gather_deferred took, in its order: the
// messages' re-decided raw words (d.m_raw), the certificates' COA_CERT_* bytes
// and the bare batches' verdicts.  An open verdict certificate passed every
// earlier check (COA_DAG_VOTES_OPEN), so its exact answer is the vote bit.
inline void put_messages(const std::vector<Window*>& ws, const Deferred& d) {
  size_t j[2] = {0, 0};
  for (Window* w : ws)
    for (uint32_t m : w->m_defer) {
      const bool vote = m >= w->nhd;
      const uint32_t st = d.m_raw[vote][j[vote]++];
      if (vote)
        w->vt_out[m - w->nhd] = (st & COA_CST_BAD_HEADER_SIG) ? 1 : 0;
      else
        w->hd_out[m] = (uint8_t)(st & 3u);
    }
}
inline void put_certs(const std::vector<Window*>& ws, const uint8_t* status) {
  for (Window* w : ws)
    for (uint32_t c : w->c_defer) {
      if (w->verdict_cert(c)) w->c_words[c] = (*status & COA_CERT_BAD_VOTES) ? COA_DAG_INVALID_VOTES : COA_DAG_OK;
      w->c_out[c] = *status++;
    }
}
inline void put_groups(const std::vector<Window*>& ws, const uint8_t* verdicts) {
  for (Window* w : ws)
    if (w->g_defer)
      for (size_t g = 0; g < w->ng; g++) w->g_out[g] = *verdicts++;
}

}  // namespace coa_q

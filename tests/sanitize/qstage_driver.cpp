// The staging of an aggregation-queue window (csrc/coa_qstage.h: layout,
// packer, scatter, the resolver's gather and write-back) under ASan + UBSan,
// host code only.  Windows are built by hand and launched over 1, 3 and 5
// parts; every block is allocated at exactly the layout's total.  A fake
// device fills the output block from the packed input block -- read through
// the views, never through the Windows -- with pure functions of the bytes,
// and what the scatter hands each part is compared with the same functions
// applied to the Windows directly.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <memory>
#include <vector>

#include "coa_qstage.h"

using coa_q::Launch;
using coa_q::Window;
using coa_q::WindowPack;

static int g_bad = 0;
#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      if (g_bad++ < 20) printf("FAIL line %d (%s): %s\n", __LINE__, g_case, #cond); \
    }                                                                   \
  } while (0)
static const char* g_case = "";
static const uint8_t kFill = 0xEE;  // what a block holds where nothing was written
static uint32_t g_seen_cert = 0, g_seen_msg = 0;  // raw status words the fake device produced (bit per word value)
static int g_resolved = 0;  // what the resolver runs had open: 1 certificates, 2 headers, 4 votes, 8 bare batches

typedef std::vector<uint8_t> Bytes;

static Bytes bytes_of(size_t n, uint32_t tag) {
  Bytes v(n);
  for (size_t i = 0; i < n; i++) v[i] = (uint8_t)((((uint32_t)i + tag * 7919u) * 2654435761u) >> 13);
  return v;
}
static void append(Bytes& to, const void* p, size_t n) {
  const uint8_t* b = static_cast<const uint8_t*>(p);
  if (n) to.insert(to.end(), b, b + n);
}

// ---- the fake device's pure functions ---------------------------------
static const uint32_t kU = COA_CST_UNCACHED, kI = COA_CST_VOTES_INCONCLUSIVE, kB = COA_CST_BAD_VOTES;
static const uint32_t kCertWords[] = {0, 1, 2, kB, 7, kU, kU | 1, kI, kI | kB, kI | 2, kU | kI | kB, kI | kB | 3};
static const uint32_t kHdrWords[] = {0, 1, 2, 3, kU, kU | 1, kU | 2, kU | 3};
static const uint32_t kVoteWords[] = {0, 2, kU, kU | 2};

static uint8_t sig_verdict(const uint8_t* msg, const uint8_t* pk, const uint8_t* sig) {
  return (uint8_t)((msg[0] ^ msg[31] ^ pk[1] ^ pk[30] ^ sig[2] ^ sig[63]) & 1);
}
static uint32_t cert_word(const uint8_t* hdr, uint64_t hlen, const uint8_t* id, const uint8_t* origin,
                          const uint8_t* hsig, uint64_t round, const uint8_t* vpks, const uint8_t* vsigs, uint64_t nv) {
  uint64_t h = id[0] + 3 * id[31] + 5 * origin[0] + 7 * origin[31] + 11 * hsig[0] + 13 * hsig[63] + 17 * round +
               19 * hlen + 23 * nv;
  if (hlen) h += hdr[0] + 29 * hdr[hlen - 1];
  if (nv) h += vpks[0] + 31 * vpks[nv * 32 - 1] + vsigs[0] + 37 * vsigs[nv * 64 - 1];
  return kCertWords[h % (sizeof(kCertWords) / 4)];
}
static void digest64(const uint8_t* data, uint64_t len, uint8_t* out) {
  for (size_t j = 0; j < 64; j++) out[j] = (uint8_t)(j * 3 + len + (len ? data[j % len] + data[len - 1] : 0));
}
static uint32_t hdr_word(const uint8_t* data, uint64_t len, const uint8_t* id, const uint8_t* author,
                         const uint8_t* sig) {
  uint64_t h = id[0] + 3 * id[31] + 5 * author[0] + 7 * author[31] + 11 * sig[0] + 13 * sig[63] + 17 * len;
  if (len) h += data[0] + 19 * data[len - 1];
  return kHdrWords[h % (sizeof(kHdrWords) / 4)];
}
static uint32_t vote_word(const uint8_t* id, uint64_t round, const uint8_t* origin, const uint8_t* author,
                          const uint8_t* sig) {
  const uint64_t h = id[0] + 3 * id[31] + 5 * origin[0] + 7 * origin[31] + 11 * author[0] + 13 * author[31] +
                     17 * sig[0] + 19 * sig[63] + 23 * round;
  return kVoteWords[h % (sizeof(kVoteWords) / 4)];
}

// Reads the packed input block `in` through the views and fills the output
// block.  sig_hi is or-ed into bits 8.. of a latency verdict word (not
// defined when staged), word_hi into those of a certificate or message status
// word (a published word's tag; a staged word has none).
static void fake_device(const uint8_t* in, const WindowPack& p, const Launch& L, uint8_t* out, uint32_t sig_hi,
                        uint32_t word_hi) {
  auto words = [out](const Sec& s) { return reinterpret_cast<uint32_t*>(out + s.at); };
  for (size_t i = 0; i < L.nv; i++) {
    if (p.v_recs.bytes) {
      const uint8_t* r = in + p.v_recs.at + i * 128;
      words(p.o_sigs)[i] = sig_verdict(r, r + 32, r + 64) | sig_hi;
    } else {
      out[p.o_sigs.at + i] = sig_verdict(in + p.v_msgs.at + i * 32, in + p.v_pks.at + i * 32, in + p.v_sigs.at + i * 64);
    }
  }
  const CertIn c = cert_view(in, p.cert);
  for (size_t i = 0; i < L.nc; i++) {
    const uint64_t h0 = c.hdr_off[i], v0 = c.voff[i];
    const uint32_t w = cert_word(c.hdr_data + h0, c.hdr_off[i + 1] - h0, c.ids + i * 32, c.origins + i * 32,
                                 c.hsigs + i * 64, c.rounds[i], c.vpks + v0 * 32, c.vsigs + v0 * 64, c.voff[i + 1] - v0);
    g_seen_cert |= 1u << w;
    words(p.o_certs)[i] = w | word_hi;
  }
  const uint64_t* doff = reinterpret_cast<const uint64_t*>(in + p.d_off.at);
  for (size_t i = 0; i < L.nd; i++)
    digest64(in + p.d_data.at + doff[i], doff[i + 1] - doff[i], out + p.o_digs.at + i * 64);
  const MsgIn h = msg_view(in, p.hdr, false), v = msg_view(in, p.vote, true);
  for (size_t i = 0; i < L.nhd; i++) {
    const uint32_t w = hdr_word(h.hdr_data + h.hdr_off[i], h.hdr_off[i + 1] - h.hdr_off[i], h.ids + i * 32,
                                h.authors + i * 32, h.sigs + i * 64);
    g_seen_msg |= 1u << w;
    words(p.o_msgs)[i] = w | word_hi;
  }
  for (size_t i = 0; i < L.nvt; i++)
    words(p.o_msgs)[L.nhd + i] =
        vote_word(v.ids + i * 32, v.rounds[i], v.origins + i * 32, v.authors + i * 32, v.sigs + i * 64) | word_hi;
}

// ---- windows built by hand ---------------------------------------------
struct CertSpec {
  size_t hlen, votes;
  bool owned;  // copied into Window::c_own (offsets until bind()); else borrowed
};
struct Spec {
  size_t nv = 0;
  std::vector<CertSpec> certs;
  std::vector<size_t> digs, hdrs;  // byte lengths
  size_t nvt = 0;
  std::vector<size_t> groups;  // votes per bare batch
};

static std::deque<Bytes> g_borrowed;  // the callers' arrays of borrowed certificates
static uint32_t g_tag = 1;

static std::unique_ptr<Window> make_window(const Spec& s) {
  std::unique_ptr<Window> wp(new Window);
  Window& w = *wp;
  w.reset();
  w.nv = s.nv;
  w.v_msgs = bytes_of(s.nv * 32, g_tag++), w.v_pks = bytes_of(s.nv * 32, g_tag++), w.v_sigs = bytes_of(s.nv * 64, g_tag++);
  for (const CertSpec& c : s.certs) {
    const size_t sizes[6] = {c.hlen, 32, 32, 64, c.votes * 32, c.votes * 64};
    Window::CertRef r{};
    const uint8_t** f[6] = {&r.hdr, &r.id, &r.origin, &r.hsig, &r.vpks, &r.vsigs};
    for (int k = 0; k < 6; k++) {
      const Bytes b = bytes_of(sizes[k], g_tag++);
      if (c.owned) {
        *f[k] = reinterpret_cast<const uint8_t*>((uintptr_t)w.c_own.size());
        append(w.c_own, b.data(), b.size());
      } else {
        g_borrowed.push_back(b);
        *f[k] = g_borrowed.back().data();
      }
    }
    r.hlen = c.hlen, r.round = 1000 + g_tag, r.nv = c.votes, r.owned = c.owned;
    w.c_refs.push_back(r);
    w.nc++, w.c_votes += c.votes, w.c_hbytes += c.hlen;
  }
  for (size_t len : s.digs) {
    append(w.d_data, bytes_of(len, g_tag++).data(), len);
    w.d_offs.push_back(w.d_data.size());
    w.nd++;
  }
  for (size_t len : s.hdrs) {
    append(w.hd_data, bytes_of(len, g_tag++).data(), len);
    w.hd_offs.push_back(w.hd_data.size());
    w.nhd++;
  }
  w.hd_ids = bytes_of(w.nhd * 32, g_tag++), w.hd_authors = bytes_of(w.nhd * 32, g_tag++);
  w.hd_sigs = bytes_of(w.nhd * 64, g_tag++);
  w.nvt = s.nvt;
  w.vt_ids = bytes_of(s.nvt * 32, g_tag++), w.vt_origins = bytes_of(s.nvt * 32, g_tag++);
  w.vt_authors = bytes_of(s.nvt * 32, g_tag++), w.vt_sigs = bytes_of(s.nvt * 64, g_tag++);
  for (size_t i = 0; i < s.nvt; i++) w.vt_rounds.push_back(77 + 3 * i + g_tag);
  for (size_t votes : s.groups) {
    append(w.g_msgs, bytes_of(votes * 32, g_tag++).data(), votes * 32);
    append(w.g_pks, bytes_of(votes * 32, g_tag++).data(), votes * 32);
    append(w.g_sigs, bytes_of(votes * 64, g_tag++).data(), votes * 64);
    w.g_offs.push_back(w.g_offs.back() + votes);
    w.ng++;
  }
  w.bind();  // the collector's take
  return wp;
}

// ---- layout --------------------------------------------------------------
struct Named {
  Sec sec;
  Bytes want;    // the bytes the host packs there (an input section)
  size_t slack;  // bytes of the section after `want` that nothing writes
};

static size_t up256(size_t x) { return (x + 255) / 256 * 256; }

static void check_secs(const std::vector<Sec>& secs, size_t total) {
  std::vector<Sec> s = secs;
  std::sort(s.begin(), s.end(), [](const Sec& a, const Sec& b) { return a.at < b.at || (a.at == b.at && a.bytes < b.bytes); });
  size_t end = 0;
  for (const Sec& x : s) {
    CHECK(x.at % 256 == 0);
    CHECK(x.at >= end);  // disjoint
    end = x.at + x.bytes;
    CHECK(end <= total);
  }
}

// The input sections with what belongs in each, computed from the Windows.
static std::vector<Named> expect_input(const Launch& L, const WindowPack& p, bool sig_lat) {
  Bytes recs, vm, vp, vs, ch, cid, cor, chs, cvp, cvs, dd, hd, hid, hau, hsg, tid, tor, tau, tsg;
  std::vector<uint64_t> cho{0}, crd, cvo{0}, dof{0}, hdo{0}, trd;
  for (const Window* w : L.parts) {
    for (size_t i = 0; i < w->nv; i++) {
      append(recs, &w->v_msgs[i * 32], 32), append(recs, &w->v_pks[i * 32], 32), append(recs, &w->v_sigs[i * 64], 64);
    }
    append(vm, w->v_msgs.data(), w->nv * 32), append(vp, w->v_pks.data(), w->nv * 32);
    append(vs, w->v_sigs.data(), w->nv * 64);
    for (const Window::CertRef& r : w->c_refs) {
      append(ch, r.hdr, r.hlen), append(cid, r.id, 32), append(cor, r.origin, 32), append(chs, r.hsig, 64);
      append(cvp, r.vpks, r.nv * 32), append(cvs, r.vsigs, r.nv * 64);
      cho.push_back(ch.size()), crd.push_back(r.round), cvo.push_back(cvp.size() / 32);
    }
    for (size_t i = 0; i < w->nd; i++) dof.push_back(dd.size() + w->d_offs[i + 1]);
    append(dd, w->d_data.data(), w->d_data.size());
    for (size_t i = 0; i < w->nhd; i++) hdo.push_back(hd.size() + w->hd_offs[i + 1]);
    append(hd, w->hd_data.data(), w->hd_data.size());
    append(hid, w->hd_ids.data(), w->nhd * 32), append(hau, w->hd_authors.data(), w->nhd * 32);
    append(hsg, w->hd_sigs.data(), w->nhd * 64);
    append(tid, w->vt_ids.data(), w->nvt * 32), append(tor, w->vt_origins.data(), w->nvt * 32);
    append(tau, w->vt_authors.data(), w->nvt * 32), append(tsg, w->vt_sigs.data(), w->nvt * 64);
    trd.insert(trd.end(), w->vt_rounds.begin(), w->vt_rounds.end());
  }
  // the three offset arrays start at 0 and end at the section's byte or vote count
  CHECK(cho.back() == L.hbytes && cvo.back() == L.nvotes && dof.back() == L.dbytes && hdo.back() == L.hdbytes);
  auto u64 = [](const std::vector<uint64_t>& v) {
    Bytes b;
    append(b, v.data(), v.size() * 8);
    return b;
  };
  if (!sig_lat) recs.clear();
  if (sig_lat) vm.clear(), vp.clear(), vs.clear();
  const bool hdrs = L.nhd != 0;
  return {{p.v_recs, recs, 0},         {p.v_msgs, vm, 0},          {p.v_pks, vp, 0},         {p.v_sigs, vs, 0},
          {p.cert.hdata, ch, 16},      {p.cert.hoff, u64(cho), 0}, {p.cert.ids, cid, 0},     {p.cert.origins, cor, 0},
          {p.cert.hsigs, chs, 0},      {p.cert.rounds, u64(crd), 0}, {p.cert.vpks, cvp, 0},  {p.cert.vsigs, cvs, 0},
          {p.cert.voff, u64(cvo), 0},  {p.d_data, dd, 16},         {p.d_off, u64(dof), 0},
          {p.hdr.hdata, hd, hdrs ? 16u : 0u}, {p.hdr.hoff, hdrs ? u64(hdo) : Bytes(), 0}, {p.hdr.ids, hid, 0},
          {p.hdr.authors, hau, 0},     {p.hdr.sigs, hsg, 0},       {p.vote.ids, tid, 0},     {p.vote.rounds, u64(trd), 0},
          {p.vote.origins, tor, 0},    {p.vote.authors, tau, 0},   {p.vote.sigs, tsg, 0}};
}

struct Block {  // exactly n bytes on the heap: one byte past it is an ASan report
  std::unique_ptr<uint8_t[]> p;
  explicit Block(size_t n) : p(new uint8_t[n]) { std::memset(p.get(), kFill, n); }
  uint8_t* get() { return p.get(); }
};

// Lays the launch out, checks the layout, packs it and checks every byte of
// the input block.
static WindowPack pack_checked(const Launch& L, bool sig_lat, Block& in) {
  const WindowPack p = coa_q::window_layout(L, sig_lat);
  // the totals from the counts alone
  const size_t msgs = L.nhd + L.nvt;
  size_t want_in = (sig_lat ? up256(L.nv * 128) : 2 * up256(L.nv * 32) + up256(L.nv * 64)) + up256(L.hbytes + 16) +
                   2 * up256((L.nc + 1) * 8) + 2 * up256(L.nc * 32) + up256(L.nc * 64) + up256(L.nc * 8) +
                   up256(L.nvotes * 32) + up256(L.nvotes * 64) + up256(L.dbytes + 16) + up256((L.nd + 1) * 8) +
                   2 * up256(L.nhd * 32) + up256(L.nhd * 64) + 3 * up256(L.nvt * 32) + up256(L.nvt * 8) +
                   up256(L.nvt * 64);
  if (L.nhd) want_in += up256(L.hdbytes + 16) + up256((L.nhd + 1) * 8);
  CHECK(p.in_total == want_in);
  CHECK(p.out_total == up256(sig_lat ? L.nv * 4 : L.nv) + up256(L.nc * 4) + up256(L.nd * 64) + up256(msgs * 4));
  CHECK(p.o_sigs.bytes == (sig_lat ? L.nv * 4 : L.nv) && p.o_certs.bytes == L.nc * 4 && p.o_digs.bytes == L.nd * 64 &&
        p.o_msgs.bytes == msgs * 4);
  check_secs({p.o_sigs, p.o_certs, p.o_digs, p.o_msgs}, p.out_total);
  const std::vector<Named> secs = expect_input(L, p, sig_lat);
  std::vector<Sec> all;
  for (const Named& s : secs) {
    all.push_back(s.sec);
    CHECK(s.sec.bytes == s.want.size() + s.slack);
  }
  check_secs(all, p.in_total);
  if (g_bad) return p;  // a wrong layout: packing into it could run off the block

  in = Block(p.in_total);
  std::vector<Seg> bulk;
  coa_q::window_pack(in.get(), p, L, bulk);
  for (const Seg& g : bulk) {
    CHECK(g.bytes > 0);
    std::memcpy(g.dst, g.src, g.bytes);
  }
  std::vector<uint8_t> written(p.in_total, 0);
  for (const Named& s : secs) {
    CHECK(s.want.empty() || std::memcmp(in.get() + s.sec.at, s.want.data(), s.want.size()) == 0);
    std::fill(written.begin() + s.sec.at, written.begin() + s.sec.at + s.want.size(), 1);
  }
  for (size_t i = 0; i < p.in_total; i++)
    if (!written[i]) CHECK(in.get()[i] == kFill);
  return p;
}

// ---- scatter ---------------------------------------------------------------
// What the scatter must hand part w, from the Window's own arrays.
struct PartOut {
  Bytes v_out, c_out, d_out, hd_out, vt_out;
  std::vector<uint32_t> c_raw, c_defer, m_defer;
  bool g_defer;
};
static PartOut expect_part(const Window& w) {
  PartOut e;
  for (size_t i = 0; i < w.nv; i++) e.v_out.push_back(sig_verdict(&w.v_msgs[i * 32], &w.v_pks[i * 32], &w.v_sigs[i * 64]));
  for (size_t i = 0; i < w.nc; i++) {
    const Window::CertRef& r = w.c_refs[i];
    const uint32_t s = cert_word(r.hdr, r.hlen, r.id, r.origin, r.hsig, r.round, r.vpks, r.vsigs, r.nv);
    e.c_raw.push_back(s);
    e.c_out.push_back((uint8_t)(s & 7));
    if ((s & kU) || ((s & kI) && !(s & kB))) e.c_defer.push_back((uint32_t)i);
  }
  for (size_t i = 0; i < w.nd; i++) {
    uint8_t d[64];
    digest64(w.d_data.data() + w.d_offs[i], w.d_offs[i + 1] - w.d_offs[i], d);
    append(e.d_out, d, 32);
  }
  for (size_t i = 0; i < w.nhd; i++) {
    const uint32_t s = hdr_word(w.hd_data.data() + w.hd_offs[i], w.hd_offs[i + 1] - w.hd_offs[i], &w.hd_ids[i * 32],
                                &w.hd_authors[i * 32], &w.hd_sigs[i * 64]);
    if (s & kU) e.m_defer.push_back((uint32_t)i);
    e.hd_out.push_back((uint8_t)(s & ((s & kU) ? 1 : 3)));
  }
  for (size_t i = 0; i < w.nvt; i++) {
    const uint32_t s = vote_word(&w.vt_ids[i * 32], w.vt_rounds[i], &w.vt_origins[i * 32], &w.vt_authors[i * 32],
                                 &w.vt_sigs[i * 64]);
    if (s & kU) e.m_defer.push_back((uint32_t)(w.nhd + i));
    e.vt_out.push_back((s & 2) ? 1 : 0);
  }
  e.g_defer = w.ng > 0;
  return e;
}
static void check_parts(const Launch& L) {
  for (const Window* w : L.parts) {
    const PartOut e = expect_part(*w);
    CHECK(w->v_out == e.v_out);
    CHECK(w->c_out == e.c_out);
    CHECK(w->d_out == e.d_out);
    CHECK(w->hd_out == e.hd_out);
    CHECK(w->vt_out == e.vt_out);
    CHECK(w->c_raw == e.c_raw);
    CHECK(w->c_defer == e.c_defer);
    CHECK(w->m_defer == e.m_defer);
    CHECK(w->g_defer == e.g_defer);
    CHECK(w->g_out == Bytes(w->ng, 1));  // left to the resolver
  }
}

// Pack, fake device, scatter: staged, and -- for a window of one kind and at
// most 64 items -- published, with the tag in bits 8..31 of the words and the
// staged words of that kind left as fill.
static void run_launch(Launch& L, bool sig_lat) {
  L.tally();
  Block in(0);
  const WindowPack p = pack_checked(L, sig_lat, in);
  if (g_bad) return;
  L.reset_outputs();
  Block out(p.out_total);
  fake_device(in.get(), p, L, out.get(), 0x5a5a5a00u, 0);
  coa_q::window_scatter(L, p, out.get(), coa_q::ROUTE_STAGED, nullptr);
  check_parts(L);

  const size_t msgs = L.nhd + L.nvt, kinds = (L.nv != 0) + (L.nc != 0) + (L.nd != 0) + (msgs != 0);
  if (kinds != 1 || L.nd || L.nv + L.nc + msgs > 64 || (L.nv && !sig_lat)) return;
  const coa_q::Route route = L.nv ? coa_q::ROUTE_SIG_INLINE : L.nc ? coa_q::ROUTE_CERT_PUBLISH : coa_q::ROUTE_MSG_PUBLISH;
  const Sec& sec = L.nv ? p.o_sigs : L.nc ? p.o_certs : p.o_msgs;
  const uint32_t tag = 0xABCDEFu;
  Block staged(p.out_total);
  fake_device(in.get(), p, L, staged.get(), tag << 8, tag << 8);
  Block pub(sec.bytes);  // exactly the window's words
  std::memcpy(pub.get(), staged.get() + sec.at, sec.bytes);
  out = Block(p.out_total);  // all fill: the published kind must not be read from here
  L.reset_outputs();
  coa_q::window_scatter(L, p, out.get(), route, reinterpret_cast<const uint32_t*>(pub.get()));
  check_parts(L);
}

// ---- the resolver's halves -------------------------------------------------
static void run_resolver(const std::vector<Window*>& ws) {
  // what is open, from the Windows' own arrays
  Bytes ids, org, hs, vp, vs, gm, gp, gs, mi[2], ma[2], ms[2], mo;
  std::vector<uint64_t> rd, vo{0}, go{0}, mr;
  std::vector<uint32_t> raw, mraw[2];
  for (const Window* w : ws) {
    const PartOut e = expect_part(*w);
    for (uint32_t c : e.c_defer) {
      const Window::CertRef& r = w->c_refs[c];
      append(ids, r.id, 32), append(org, r.origin, 32), append(hs, r.hsig, 64), rd.push_back(r.round);
      append(vp, r.vpks, r.nv * 32), append(vs, r.vsigs, r.nv * 64);
      vo.push_back(vo.back() + r.nv);
      raw.push_back(e.c_raw[c]);
    }
    for (uint32_t m : e.m_defer) {
      if (m < w->nhd) {
        append(mi[0], &w->hd_ids[m * 32], 32), append(ma[0], &w->hd_authors[m * 32], 32);
        append(ms[0], &w->hd_sigs[m * 64], 64);
        mraw[0].push_back(kU | (e.hd_out[m] & 1u));
      } else {
        const size_t i = m - w->nhd;
        append(mi[1], &w->vt_ids[i * 32], 32), append(ma[1], &w->vt_authors[i * 32], 32);
        append(ms[1], &w->vt_sigs[i * 64], 64), append(mo, &w->vt_origins[i * 32], 32);
        mr.push_back(w->vt_rounds[i]);
        mraw[1].push_back(kU);
      }
    }
    if (w->ng) {
      append(gm, w->g_msgs.data(), w->g_msgs.size()), append(gp, w->g_pks.data(), w->g_pks.size());
      append(gs, w->g_sigs.data(), w->g_sigs.size());
      for (size_t g = 0; g < w->ng; g++) go.push_back(go.back() + w->g_offs[g + 1] - w->g_offs[g]);
    }
  }
  coa_q::Deferred d = coa_q::gather_deferred(ws);
  CHECK(d.c_ids == ids && d.c_origins == org && d.c_hsigs == hs && d.c_rounds == rd && d.c_vpks == vp && d.c_vsigs == vs);
  CHECK(d.c_voff == vo && d.c_raw == raw);
  for (int k = 0; k < 2; k++) CHECK(d.m_ids[k] == mi[k] && d.m_authors[k] == ma[k] && d.m_sigs[k] == ms[k] && d.m_raw[k] == mraw[k]);
  CHECK(d.m_origins == mo && d.m_rounds == mr);
  CHECK(d.g_msgs == gm && d.g_pks == gp && d.g_sigs == gs && d.g_off == go);
  g_resolved |= (raw.empty() ? 0 : 1) | (mraw[0].empty() ? 0 : 2) | (mraw[1].empty() ? 0 : 4) | (go.size() > 1 ? 8 : 0);

  // answers: values the scatter never leaves behind (bit 3 of a status byte,
  // verdict 2 + j % 2), so one landing on a wrong item shows
  struct Before {
    Bytes c_out, hd_out, vt_out, g_out;
  };
  std::vector<Before> before;
  for (const Window* w : ws) before.push_back({w->c_out, w->hd_out, w->vt_out, w->g_out});
  Bytes c_ans(raw.size()), g_ans(go.size() - 1);
  for (size_t j = 0; j < c_ans.size(); j++) c_ans[j] = (uint8_t)(8 + j % 8);
  for (size_t j = 0; j < g_ans.size(); j++) g_ans[j] = (uint8_t)(2 + j % 2);
  for (int k = 0; k < 2; k++)
    for (size_t j = 0; j < d.m_raw[k].size(); j++) d.m_raw[k][j] = (uint32_t)((j + k) % 4);  // re-decided: bits 0, 1
  coa_q::put_messages(ws, d);
  coa_q::put_certs(ws, c_ans.data());
  coa_q::put_groups(ws, g_ans.data());
  size_t jc = 0, jg = 0, jm[2] = {0, 0};
  for (size_t k = 0; k < ws.size(); k++) {
    const Window& w = *ws[k];
    const PartOut e = expect_part(w);
    Before want = before[k];
    for (uint32_t c : e.c_defer) want.c_out[c] = c_ans[jc++];
    for (uint32_t m : e.m_defer) {
      if (m < w.nhd)
        want.hd_out[m] = (uint8_t)(d.m_raw[0][jm[0]++] & 3);
      else
        want.vt_out[m - w.nhd] = (d.m_raw[1][jm[1]++] & 2) ? 1 : 0;
    }
    for (size_t g = 0; g < w.ng; g++) want.g_out[g] = g_ans[jg++];
    CHECK(w.c_out == want.c_out && w.hd_out == want.hd_out && w.vt_out == want.vt_out && w.g_out == want.g_out);
  }
  CHECK(jc == c_ans.size() && jg == g_ans.size());
}

// ---- cases -------------------------------------------------------------------
static Spec all_kinds(size_t k) {  // a part holding every kind, sized by k
  Spec s;
  s.nv = 3 + k;
  // a copied certificate beside borrowed ones; one with 0 votes; header
  // inputs of length 0 and of lengths that are no multiple of 4
  s.certs = {{101 + k, 3 + k, true}, {0, 5, false}, {64, 0, k % 2 == 0}, {37, 7 + 2 * k, false}};
  s.digs = {17 + k, 0, 300};
  s.hdrs = {0, 45 + k, 128, 7};
  s.nvt = 6 + k;
  s.groups = {2 + k, 1};
  return s;
}

static void launch_of(const char* name, const std::vector<Spec>& specs, bool resolver = false) {
  g_case = name;
  std::vector<std::unique_ptr<Window>> own;
  Launch L;
  for (const Spec& s : specs) {
    own.push_back(make_window(s));
    L.parts.push_back(own.back().get());
  }
  for (int sig_lat = 0; sig_lat < 2; sig_lat++) run_launch(L, sig_lat != 0);
  if (resolver && !g_bad) run_resolver(L.parts);  // the parts as the last (staged-form) scatter left them
}

int main() {
  Spec sigs, certs, digs, hdrs, votes, groups, empty;
  sigs.nv = 9;
  certs.certs = {{33, 4, true}, {96, 0, false}, {0, 2, false}, {50, 9, true}};
  digs.digs = {5, 0, 1000, 64};
  hdrs.hdrs = {13, 0, 90, 256, 3};
  votes.nvt = 11;
  groups.groups = {3, 1, 4};
  // each kind alone, over 1, 3 and 5 parts
  const std::pair<const char*, Spec> alone[] = {{"signatures", sigs}, {"certificates", certs}, {"digests", digs},
                                                {"headers", hdrs},    {"votes", votes},        {"bare batches", groups}};
  for (const auto& a : alone)
    for (size_t parts : {1, 3, 5}) launch_of(a.first, std::vector<Spec>(parts, a.second));
  Spec msgs = hdrs;
  msgs.nvt = 4;
  launch_of("headers and votes", {msgs, msgs, msgs});
  // all six kinds together
  launch_of("all kinds, 1 part", {all_kinds(0)}, true);
  launch_of("all kinds, 3 parts", {all_kinds(0), all_kinds(1), all_kinds(2)}, true);
  launch_of("all kinds, 5 parts", {all_kinds(3), all_kinds(0), sigs, all_kinds(5), certs}, true);
  // an empty part between two full ones
  launch_of("empty part between", {all_kinds(1), empty, all_kinds(2)}, true);
  launch_of("empty parts around", {empty, all_kinds(4), empty, empty, all_kinds(0)}, true);
  g_case = "coverage";
  // every raw word the scatter tells apart was produced: UNCACHED, and
  // VOTES_INCONCLUSIVE with and without BAD_VOTES, among the certificates';
  // open and decided headers among the messages'
  for (uint32_t w : kCertWords) CHECK((g_seen_cert >> w) & 1);
  for (uint32_t w : kHdrWords) CHECK((g_seen_msg >> w) & 1);
  CHECK(g_resolved == 15);
  printf("qstage ok: %d bad\n", g_bad);
  return g_bad ? 1 : 0;
}

// Stand-alone driver of the verdict sections of an aggregation-queue window's
// staging (xrpl-coa-prototype_amd/csrc/coa_qstage.h, host code only): the two
// u32 payload-count sections of the input block and the verdict-word section
// of the output block -- layout, pack and scatter of a window that mixes
// crypto and verdict requests over several parts, parts with zero items of a
// kind included -- and the resolver's write-back of an open verdict
// certificate.  Blocks are heap buffers of exactly the laid-out size, so ASan
// sees any write or read past a section's block.
//
// Build (tests/test_queue_verdicts.py): g++ -fsanitize=address,undefined.
// Exit status 0 when every check held; each failed check is printed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "coa_qstage.h"

using coa_q::Launch;
using coa_q::Window;

static int g_failed = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("line %d: check failed: %s\n", __LINE__, #cond); \
      g_failed++;                                                    \
    }                                                                \
  } while (0)

namespace {

// Backing bytes of the certificates' borrowed arrays (stable addresses).
struct Pool {
  std::vector<std::unique_ptr<std::vector<uint8_t>>> bufs;
  const uint8_t* bytes(size_t n, uint8_t fill) {
    bufs.emplace_back(new std::vector<uint8_t>(n ? n : 1, fill));
    return bufs.back()->data();
  }
};

void mark(std::vector<uint8_t>& vreq, std::vector<uint32_t>* pc, size_t idx, uint32_t count) {
  vreq.resize(idx + 1, 0);
  vreq[idx] = 1;
  if (pc) {
    pc->resize(idx + 1, 0);
    (*pc)[idx] = count;
  }
}

// count < 0: a crypto request
void add_cert(Window& w, Pool& pool, size_t hlen, size_t nv, long count, uint8_t tag) {
  Window::CertRef r{pool.bytes(hlen, tag),    pool.bytes(32, tag),      pool.bytes(32, (uint8_t)(tag + 1)),
                    pool.bytes(64, (uint8_t)(tag + 2)), pool.bytes(nv * 32, (uint8_t)(tag + 3)),
                    pool.bytes(nv * 64, (uint8_t)(tag + 4)), hlen, 9, nv, false};
  w.c_refs.push_back(r);
  w.c_votes += nv;
  w.c_hbytes += hlen;
  if (count >= 0) {
    mark(w.c_vreq, &w.c_pcounts, w.nc, (uint32_t)count);
    w.n_vc++;
  }
  w.nc++;
}

void add_header(Window& w, size_t hlen, long count, uint8_t tag) {
  w.hd_data.insert(w.hd_data.end(), hlen, tag);
  w.hd_offs.push_back(w.hd_data.size());
  w.hd_ids.insert(w.hd_ids.end(), 32, tag);
  w.hd_authors.insert(w.hd_authors.end(), 32, (uint8_t)(tag + 1));
  w.hd_sigs.insert(w.hd_sigs.end(), 64, (uint8_t)(tag + 2));
  if (count >= 0) {
    mark(w.hd_vreq, &w.hd_pcounts, w.nhd, (uint32_t)count);
    w.n_vh++;
  }
  w.nhd++;
}

void add_vote(Window& w, bool verdict, uint8_t tag) {
  w.vt_ids.insert(w.vt_ids.end(), 32, tag);
  w.vt_rounds.push_back(tag);
  w.vt_origins.insert(w.vt_origins.end(), 32, (uint8_t)(tag + 1));
  w.vt_authors.insert(w.vt_authors.end(), 32, (uint8_t)(tag + 2));
  w.vt_sigs.insert(w.vt_sigs.end(), 64, (uint8_t)(tag + 3));
  if (verdict) {
    mark(w.vt_vreq, nullptr, w.nvt, 0);
    w.n_vvt++;
  }
  w.nvt++;
}

void add_sig(Window& w, uint8_t tag) {
  w.v_msgs.insert(w.v_msgs.end(), 32, tag);
  w.v_pks.insert(w.v_pks.end(), 32, tag);
  w.v_sigs.insert(w.v_sigs.end(), 64, tag);
  w.nv++;
}

bool inside(const Sec& s, size_t total) { return s.at % 256 == 0 && s.at + s.bytes <= total; }
bool apart(const Sec& a, const Sec& b) { return a.bytes == 0 || b.bytes == 0 || a.at + a.bytes <= b.at || b.at + b.bytes <= a.at; }

void pack(std::vector<uint8_t>& in, const coa_q::WindowPack& p, const Launch& L) {
  in.assign(p.in_total, 0xEE);
  in.shrink_to_fit();
  std::vector<Seg> bulk;
  coa_q::window_pack(in.data(), p, L, bulk);
  for (const Seg& g : bulk) std::memcpy(g.dst, g.src, g.bytes);
}

const uint32_t* words_at(const std::vector<uint8_t>& block, const Sec& s) {
  return reinterpret_cast<const uint32_t*>(block.data() + s.at);
}

}  // namespace

int main() {
  Pool pool;
  // part 0: a verdict and a crypto certificate, three headers (the middle one
  // a verdict request), two votes (the first a verdict request), a signature
  // part 1: no certificate, no header; three votes, the last a verdict request
  // part 2: one verdict certificate and nothing else
  // part 3: crypto requests only -- one certificate, one header, one vote
  // part 4: a crypto then a verdict certificate; a verdict header of count 0
  Window w[5];
  for (Window& x : w) x.reset();
  add_cert(w[0], pool, 112, 3, 2, 10), add_cert(w[0], pool, 50, 0, -1, 20);
  add_header(w[0], 60, -1, 30), add_header(w[0], 76, 1, 31), add_header(w[0], 0, -1, 32);
  add_vote(w[0], true, 40), add_vote(w[0], false, 41);
  add_sig(w[0], 50);
  add_vote(w[1], false, 42), add_vote(w[1], false, 43), add_vote(w[1], true, 44);
  add_cert(w[2], pool, 40, 70, 0, 60);
  add_cert(w[3], pool, 45, 2, -1, 70), add_header(w[3], 41, -1, 33), add_vote(w[3], false, 45);
  add_cert(w[4], pool, 44, 1, -1, 80), add_cert(w[4], pool, 148, 1, 3, 90), add_header(w[4], 40, 0, 34);

  Launch L;
  for (Window& x : w) L.parts.push_back(&x);
  L.tally();
  L.reset_outputs();
  CHECK(L.nc == 6 && L.nhd == 5 && L.nvt == 6 && L.n_vc == 3 && L.n_vh == 2 && L.n_vvt == 2 && L.verdicts());

  // ---- layout: the three sections exist, aligned, inside their blocks, and
  // overlap none of their neighbours
  const coa_q::WindowPack p = coa_q::window_layout(L, false);
  CHECK(p.cert.pcounts.bytes == L.nc * 4 && p.hdr.pcounts.bytes == L.nhd * 4);
  CHECK(p.o_words.bytes == (L.nc + L.nhd + L.nvt) * 4);
  CHECK(inside(p.cert.pcounts, p.in_total) && inside(p.hdr.pcounts, p.in_total) && inside(p.o_words, p.out_total));
  for (const Sec* s : {&p.v_msgs, &p.v_pks, &p.v_sigs, &p.cert.hdata, &p.cert.hoff, &p.cert.ids, &p.cert.origins,
                       &p.cert.hsigs, &p.cert.rounds, &p.cert.vpks, &p.cert.vsigs, &p.cert.voff, &p.d_data, &p.d_off,
                       &p.hdr.hdata, &p.hdr.hoff, &p.hdr.ids, &p.hdr.authors, &p.hdr.sigs, &p.vote.ids, &p.vote.rounds,
                       &p.vote.origins, &p.vote.authors, &p.vote.sigs}) {
    CHECK(apart(*s, p.cert.pcounts) && apart(*s, p.hdr.pcounts));
  }
  CHECK(apart(p.cert.pcounts, p.hdr.pcounts));
  for (const Sec* s : {&p.o_sigs, &p.o_certs, &p.o_digs, &p.o_msgs}) CHECK(apart(*s, p.o_words));
  {
    // a window without verdict requests has none of the three, and is laid
    // out as before
    Launch Lc;
    Lc.parts.push_back(&w[3]);
    Lc.tally();
    const coa_q::WindowPack pc = coa_q::window_layout(Lc, false);
    CHECK(!Lc.verdicts() && pc.cert.pcounts.bytes == 0 && pc.hdr.pcounts.bytes == 0 && pc.o_words.bytes == 0);
    std::vector<uint8_t> in;
    pack(in, pc, Lc);
  }

  // ---- pack: a verdict request's own count, zero for every crypto request
  std::vector<uint8_t> in;
  pack(in, p, L);
  const uint32_t want_c[6] = {2, 0, 0, 0, 0, 3}, want_h[5] = {0, 1, 0, 0, 0};
  CHECK(std::memcmp(words_at(in, p.cert.pcounts), want_c, sizeof(want_c)) == 0);
  CHECK(std::memcmp(words_at(in, p.hdr.pcounts), want_h, sizeof(want_h)) == 0);
  // the arrays beside them are the ones cert_view / msg_view hand the kernels
  const CertIn cv = cert_view(in.data(), p.cert);
  CHECK(cv.hdr_off[6] == 112 + 50 + 40 + 45 + 44 + 148 && cv.voff[6] == 3 + 0 + 70 + 2 + 1 + 1);
  CHECK(cv.ids[5 * 32] == 90 && cv.ids[2 * 32] == 60);
  const MsgIn hv = msg_view(in.data(), p.hdr, false), vv = msg_view(in.data(), p.vote, true);
  CHECK(hv.hdr_off[5] == 60 + 76 + 0 + 41 + 40 && hv.authors[4 * 32] == 35 && vv.authors[5 * 32] == 47);

  // ---- scatter: raw words and verdict words of the output block
  std::vector<uint8_t> out(p.out_total, 0xEE);
  out.shrink_to_fit();
  auto mut = [&out](const Sec& s) { return reinterpret_cast<uint32_t*>(out.data() + s.at); };
  // certificates 0 (verdict, an outsider voter: raw uncached, word UNKNOWN_VOTER
  // at vote 2), 1 (crypto, uncached: the resolver's), 2 (verdict, VOTES_OPEN),
  // 3 (crypto, bad votes), 4 (crypto, fine), 5 (verdict, fine)
  const uint32_t craw[6] = {COA_CST_UNCACHED, COA_CST_UNCACHED, COA_CST_VOTES_INCONCLUSIVE, COA_CST_BAD_VOTES, 0, 0};
  // headers 0 (crypto, bad id), 1 (verdict, outsider author), 2 (crypto,
  // outsider: the resolver's), 3 (crypto, fine), 4 (verdict, fine); votes 0
  // (verdict, outsider), 1 (crypto, bad), 2 (crypto), 3 (crypto, outsider), 4
  // (verdict, bad signature), 5 (crypto)
  const uint32_t mraw[11] = {1, COA_CST_UNCACHED, COA_CST_UNCACHED | 1, 0, 0,
                             COA_CST_UNCACHED, 2, 0, COA_CST_UNCACHED, 2, 0};
  const uint32_t words[17] = {COA_DAG_UNKNOWN_VOTER | (2u << 8), 0x55, COA_DAG_VOTES_OPEN, 0x55, 0x55, COA_DAG_OK,
                              0x55, COA_DAG_UNKNOWN_AUTHOR, 0x55, 0x55, COA_DAG_OK,
                              COA_DAG_UNKNOWN_AUTHOR, 0x55, 0x55, 0x55, COA_DAG_INVALID_SIGNATURE, 0x55};
  std::memcpy(mut(p.o_certs), craw, sizeof(craw));
  std::memcpy(mut(p.o_msgs), mraw, sizeof(mraw));
  std::memcpy(mut(p.o_words), words, sizeof(words));
  out[p.o_sigs.at] = 0;
  coa_q::window_scatter(L, p, out.data(), coa_q::ROUTE_STAGED, nullptr);
  CHECK(w[0].c_words[0] == (COA_DAG_UNKNOWN_VOTER | (2u << 8)) && w[2].c_words[0] == COA_DAG_VOTES_OPEN &&
        w[4].c_words[1] == COA_DAG_OK);
  CHECK(w[0].hd_words[1] == COA_DAG_UNKNOWN_AUTHOR && w[4].hd_words[0] == COA_DAG_OK);
  CHECK(w[0].vt_words[0] == COA_DAG_UNKNOWN_AUTHOR && w[1].vt_words[2] == COA_DAG_INVALID_SIGNATURE);
  // who is left open: the uncached crypto certificate and the VOTES_OPEN
  // verdict certificate; the uncached crypto messages; no verdict message,
  // and not the verdict certificate with the outsider voter
  CHECK(w[0].c_defer == std::vector<uint32_t>{1} && w[2].c_defer == std::vector<uint32_t>{0});
  CHECK(w[3].c_defer.empty() && w[4].c_defer.empty() && w[3].c_out[0] == COA_CERT_BAD_VOTES && w[4].c_out[0] == 0);
  CHECK(w[0].m_defer == std::vector<uint32_t>{2} && w[1].m_defer == std::vector<uint32_t>{1});
  CHECK(w[3].m_defer.empty() && w[4].m_defer.empty());
  CHECK(w[0].hd_out[0] == 1 && w[0].hd_out[2] == 1 && w[3].hd_out[0] == 0 && w[0].vt_out[1] == 1 && w[1].vt_out[1] == 0);
  // parts without verdict requests of a kind hold no words of it
  CHECK(w[1].c_words.empty() && w[1].hd_words.empty() && w[3].vt_words.empty() && w[2].hd_words.empty());

  // ---- the resolver's halves: the open verdict certificate's exact answer
  {
    std::vector<Window*> ws{&w[0], &w[2]};
    const coa_q::Deferred d = coa_q::gather_deferred(ws);
    CHECK(d.c_raw.size() == 2 && d.c_raw[0] == COA_CST_UNCACHED && d.c_raw[1] == COA_CST_VOTES_INCONCLUSIVE);
    CHECK(d.c_voff.size() == 3 && d.c_voff[2] == 70);
    const uint8_t bad[2] = {COA_CERT_BAD_HEADER_SIG, COA_CERT_BAD_VOTES};
    coa_q::put_certs(ws, bad);
    CHECK(w[0].c_out[1] == COA_CERT_BAD_HEADER_SIG && w[2].c_words[0] == COA_DAG_INVALID_VOTES);
    const uint8_t good[2] = {0, 0};
    coa_q::put_certs(ws, good);
    CHECK(w[0].c_out[1] == 0 && w[2].c_words[0] == COA_DAG_OK);
    // a failed pass: the failed word, and only for what was open
    w[2].fail_open();
    w[0].fail_open();
    CHECK(w[2].c_words[0] == coa_q::kWordFailed && w[0].c_out[1] == coa_q::kCertFailed);
    CHECK(w[0].c_words[0] == (COA_DAG_UNKNOWN_VOTER | (2u << 8)));
  }

  // ---- a generation without protocol table: the words stay "failed", no
  // verdict request is left open, the crypto requests are scattered as before
  L.reset_outputs();
  L.verdict_rc = COA_EINVAL;
  coa_q::window_scatter(L, p, out.data(), coa_q::ROUTE_STAGED, nullptr);
  CHECK(w[0].c_words[0] == coa_q::kWordFailed && w[2].c_words[0] == coa_q::kWordFailed);
  CHECK(w[0].hd_words[1] == coa_q::kWordFailed && w[1].vt_words[2] == coa_q::kWordFailed);
  CHECK(w[2].c_defer.empty() && w[0].c_defer == std::vector<uint32_t>{1} && w[0].m_defer == std::vector<uint32_t>{2});
  CHECK(w[3].c_out[0] == COA_CERT_BAD_VOTES && w[0].vt_out[1] == 1);

  // ---- a recycled window forgets its verdict requests
  w[0].reset();
  CHECK(!w[0].verdicts() && w[0].c_vreq.empty() && w[0].hd_pcounts.empty() && !w[0].verdict_cert(0));

  std::printf("qstage verdict sections: %d failed checks\n", g_failed);
  return g_failed ? 1 : 0;
}

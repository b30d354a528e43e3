// The staging layouts and packers of csrc/coa_stage.h (what a shard of a
// host-pointer certificate / header / vote call copies to the device) under
// ASan + UBSan, host code only.  Synthetic caller arrays whose bytes encode
// their own index; every sub-range [lo, hi) of a small call is packed into a
// heap buffer of exactly `total` bytes and compared with its source slices.
// argv: the vote counts of a certificate set (tests/verdict_cases.py); the
// chunk cuts of the pipelined path are checked over six tiles of it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "coa_stage.h"

static int g_bad = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      if (g_bad++ < 20) printf("FAIL line %d: %s\n", __LINE__, #cond); \
    }                                                          \
  } while (0)

static const uint8_t kFill = 0xEE;  // what the buffer holds where nothing was packed
static const size_t kInlineCap = 2816;  // COA_CERT_INLINE_BYTES (csrc/coa_committee.h)

static std::vector<uint8_t> bytes_of(size_t n, uint32_t tag) {
  std::vector<uint8_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (uint8_t)((((uint32_t)i + tag * 7919u) * 2654435761u) >> 13);
  return v;
}

static std::vector<uint64_t> prefix(const std::vector<size_t>& sizes, uint64_t first) {
  std::vector<uint64_t> off(sizes.size() + 1, first);
  for (size_t i = 0; i < sizes.size(); i++) off[i + 1] = off[i] + sizes[i];
  return off;
}

struct Named {
  const char* name;
  Sec sec;
  const void* src;  // what the host packs there (null: zeroes, or written on the device)
  bool host;        // packed by the host
};

// Alignment, order, coverage of [0, total) up to padding, and the contents
// of every section; bytes outside the host's sections must be untouched.
static void check_block(const std::vector<uint8_t>& buf, const std::vector<Named>& secs, size_t total, size_t align) {
  CHECK(buf.size() == total);
  std::vector<uint8_t> packed(total, 0);
  size_t end = 0;
  for (const Named& s : secs) {
    CHECK(s.sec.at % align == 0);
    CHECK(s.sec.at >= end);          // disjoint, in layout order
    CHECK(s.sec.at - end < align);   // nothing but padding between sections
    end = s.sec.at + s.sec.bytes;
    CHECK(end <= total);
    if (end > total) return;
    if (!s.host) continue;
    for (size_t i = 0; i < s.sec.bytes; i++) packed[s.sec.at + i] = 1;
    if (s.src) CHECK(std::memcmp(buf.data() + s.sec.at, s.src, s.sec.bytes) == 0);
  }
  CHECK(total - end < align);
  for (size_t i = 0; i < total; i++)
    if (!packed[i]) CHECK(buf[i] == kFill);
}

struct CertCall {
  std::vector<uint64_t> hoff, voff, rounds;
  std::vector<uint8_t> hdata, ids, origins, hsigs, vpks, vsigs;
  std::vector<uint32_t> pcounts;
  CertIn in() const {
    return {hdata.data(), hoff.data(), ids.data(), origins.data(), hsigs.data(), rounds.data(), vpks.data(),
            vsigs.data(), voff.data()};
  }
};

// hdr_first: the caller's header offsets need not start at 0
static CertCall cert_call(const std::vector<size_t>& hbytes, const std::vector<size_t>& votes, uint64_t hdr_first) {
  CertCall c;
  const size_t nc = hbytes.size();
  c.hoff = prefix(hbytes, hdr_first);
  c.voff = prefix(votes, 0);
  c.hdata = bytes_of(c.hoff[nc], 1);
  c.ids = bytes_of(nc * 32, 2);
  c.origins = bytes_of(nc * 32, 3);
  c.hsigs = bytes_of(nc * 64, 4);
  c.vpks = bytes_of(c.voff[nc] * 32, 5);
  c.vsigs = bytes_of(c.voff[nc] * 64, 6);
  for (size_t i = 0; i < nc; i++) {
    c.rounds.push_back(0x0102030405060708ull * (i + 1));
    c.pcounts.push_back(0xC0000000u + (uint32_t)i);
  }
  return c;
}

static void check_cert_range(const CertCall& c, size_t lo, size_t hi, bool verdicts, bool inl) {
  const CertIn in = c.in();
  const size_t nc = hi - lo, nv = c.voff[hi] - c.voff[lo], hb = c.hoff[hi] - c.hoff[lo];
  CertPack p;
  std::vector<uint8_t> buf;
  if (inl) {
    buf.assign(kInlineCap, kFill);
    CHECK(cert_inline_pack(buf.data(), kInlineCap, p, in, lo, hi));
    for (size_t i = p.total; i < kInlineCap; i++) CHECK(buf[i] == kFill);
    buf.resize(p.total);
    CHECK(p.status.bytes == 0);
  } else {
    p = cert_layout(nc, nv, hb, verdicts);
    buf.assign(p.total, kFill);
    for (const Seg& g : cert_segments(buf.data(), p, in, verdicts ? c.pcounts.data() : nullptr, lo, hi))
      std::memcpy(g.dst, g.src, g.bytes);
    CHECK(p.status.bytes == nc * 4);
  }
  CHECK((p.pcounts.bytes == (verdicts ? nc * 4 : 0)) && p.proto.bytes == p.pcounts.bytes &&
        p.verd.bytes == p.pcounts.bytes);
  std::vector<uint64_t> ho(nc + 1), vo(nc + 1);
  for (size_t i = 0; i <= nc; i++) {
    ho[i] = c.hoff[lo + i] - c.hoff[lo];
    vo[i] = c.voff[lo + i] - c.voff[lo];
  }
  CHECK(ho[0] == 0 && vo[0] == 0);
  std::vector<uint8_t> hd(c.hdata.begin() + c.hoff[lo], c.hdata.begin() + c.hoff[hi]);
  hd.resize(hb + 16, 0);  // the zeroed slack
  const std::vector<uint8_t> zero(nc * 4, 0);
  check_block(buf,
              {{"status", p.status, zero.data(), true},
               {"hoff", p.hoff, ho.data(), true},
               {"voff", p.voff, vo.data(), true},
               {"ids", p.ids, c.ids.data() + lo * 32, true},
               {"origins", p.origins, c.origins.data() + lo * 32, true},
               {"hsigs", p.hsigs, c.hsigs.data() + lo * 64, true},
               {"rounds", p.rounds, c.rounds.data() + lo, true},
               {"vpks", p.vpks, c.vpks.data() + c.voff[lo] * 32, true},
               {"vsigs", p.vsigs, c.vsigs.data() + c.voff[lo] * 64, true},
               {"hdata", p.hdata, hd.data(), true},
               {"pcounts", p.pcounts, c.pcounts.data() + lo, true},
               {"proto", p.proto, nullptr, false},
               {"verd", p.verd, nullptr, false}},
              p.total, inl ? 16 : 256);
}

static void certificates() {
  // one certificate, no votes, no header bytes
  const CertCall one = cert_call({0}, {0}, 0);
  for (int v = 0; v < 2; v++) check_cert_range(one, 0, 1, v != 0, false);
  check_cert_range(one, 0, 1, false, true);
  // certificates without votes in the middle and at the end; an empty header;
  // the caller's header offsets start past 0
  const CertCall c = cert_call({200, 1, 0, 133, 64, 7, 180}, {3, 0, 5, 0, 0, 2, 0}, 40);
  for (size_t lo = 0; lo < 7; lo++)
    for (size_t hi = lo + 1; hi <= 7; hi++) {
      check_cert_range(c, lo, hi, false, false);
      check_cert_range(c, lo, hi, true, false);
      check_cert_range(c, lo, hi, false, true);  // all of them fit the inline record
    }
}

static void inline_limit() {
  // 1 certificate of 20 votes: 176 + 20 * 96 bytes before the header section,
  // so 704 header bytes (+ 16 of slack) fill the record exactly
  CertCall fits = cert_call({704}, {20}, 0);
  CertPack p;
  CHECK(cert_layout(1, 20, 704, false, true).total == kInlineCap);
  check_cert_range(fits, 0, 1, false, true);
  const CertCall over = cert_call({705}, {20}, 0);
  std::vector<uint8_t> buf(kInlineCap, kFill);  // heap, exactly the record: a write past it is ASan's
  CHECK(!cert_inline_pack(buf.data(), kInlineCap, p, over.in(), 0, 1));
  CHECK(p.total > kInlineCap);
  CHECK(buf == std::vector<uint8_t>(kInlineCap, kFill));
  // more certificates than the latency kernel's 64 status words
  const CertCall many = cert_call(std::vector<size_t>(65, 0), std::vector<size_t>(65, 0), 0);
  CHECK(!cert_inline_pack(buf.data(), kInlineCap, p, many.in(), 0, 65));
  CHECK(buf == std::vector<uint8_t>(kInlineCap, kFill));
}

static void messages(bool votes) {
  const std::vector<size_t> hbytes = {90, 0, 41, 256, 5};
  const size_t n = hbytes.size();
  const std::vector<uint64_t> hoff = prefix(hbytes, 24);
  const std::vector<uint8_t> hdata = bytes_of(hoff[n], 11), ids = bytes_of(n * 32, 12), origins = bytes_of(n * 32, 13),
                             authors = bytes_of(n * 32, 14), sigs = bytes_of(n * 64, 15);
  std::vector<uint64_t> rounds;
  std::vector<uint32_t> pcounts;
  for (size_t i = 0; i < n; i++) {
    rounds.push_back(0x1112131415161718ull * (i + 1));
    pcounts.push_back(0xD0000000u + (uint32_t)i);
  }
  const MsgIn in = votes ? MsgIn{nullptr, nullptr, ids.data(), rounds.data(), origins.data(), authors.data(),
                                 sigs.data(), true}
                         : MsgIn{hdata.data(), hoff.data(), ids.data(), nullptr, nullptr, authors.data(), sigs.data(),
                                 false};
  for (size_t lo = 0; lo < n; lo++)
    for (size_t hi = lo + 1; hi <= n; hi++)
      for (int verdicts = 0; verdicts < 2; verdicts++) {
        const size_t m = hi - lo, hb = votes ? 0 : hoff[hi] - hoff[lo];
        const MsgPack p = msg_layout(m, votes, hb, verdicts != 0);
        std::vector<uint8_t> buf(p.total, kFill);
        // votes have no payload counts: the pointer is null in both forms
        for (const Seg& g : msg_segments(buf.data(), p, in, verdicts && !votes ? pcounts.data() : nullptr, lo, hi))
          std::memcpy(g.dst, g.src, g.bytes);
        CHECK(p.pcounts.bytes == (verdicts && !votes ? m * 4 : 0));
        CHECK(p.proto.bytes == (verdicts ? m * 4 : 0) && p.verd.bytes == p.proto.bytes);
        const std::vector<uint8_t> zero(m * 4, 0);
        std::vector<Named> secs = {{"status", p.status, zero.data(), true},
                                   {"ids", p.ids, ids.data() + lo * 32, true},
                                   {"authors", p.authors, authors.data() + lo * 32, true},
                                   {"sigs", p.sigs, sigs.data() + lo * 64, true}};
        std::vector<uint64_t> ho(m + 1);
        std::vector<uint8_t> hd;
        if (votes) {
          CHECK(p.hoff.bytes == 0 && p.hdata.bytes == 0);
          secs.push_back({"rounds", p.rounds, rounds.data() + lo, true});
          secs.push_back({"origins", p.origins, origins.data() + lo * 32, true});
        } else {
          CHECK(p.rounds.bytes == 0 && p.origins.bytes == 0);
          for (size_t i = 0; i <= m; i++) ho[i] = hoff[lo + i] - hoff[lo];
          hd.assign(hdata.begin() + hoff[lo], hdata.begin() + hoff[hi]);
          hd.resize(hb + 16, 0);
          secs.push_back({"hoff", p.hoff, ho.data(), true});
          secs.push_back({"hdata", p.hdata, hd.data(), true});
          secs.push_back({"pcounts", p.pcounts, pcounts.data() + lo, true});
        }
        secs.push_back({"proto", p.proto, nullptr, false});
        secs.push_back({"verd", p.verd, nullptr, false});
        check_block(buf, secs, p.total, 256);
      }
}

static void chunk_cuts(const std::vector<size_t>& set_votes) {
  std::vector<size_t> votes;
  for (int t = 0; t < 6; t++) votes.insert(votes.end(), set_votes.begin(), set_votes.end());
  const std::vector<uint64_t> voff = prefix(votes, 0);
  const size_t n = votes.size();
  const size_t ranges[][2] = {{0, n}, {5, n}, {0, n - 3}, {n / 3, n / 3 + 1}, {n / 4, 3 * n / 4}};
  for (const auto& r : ranges)
    for (size_t chunk_jobs : {(size_t)4096, (size_t)1 << 17})
      for (int ramp = 0; ramp <= 4; ramp++) {
        const std::vector<size_t> cuts = cert_chunk_cuts(voff.data(), r[0], r[1], chunk_jobs, ramp);
        CHECK(cuts.size() >= 2 && cuts.front() == r[0] && cuts.back() == r[1]);  // contiguous, cover [lo, hi)
        for (size_t k = 0; k + 1 < cuts.size(); k++) {
          CHECK(cuts[k] < cuts[k + 1]);  // non-empty
          const size_t jobs = (cuts[k + 1] - cuts[k]) + (voff[cuts[k + 1]] - voff[cuts[k]]);
          if (k + 2 < cuts.size()) CHECK(jobs >= (chunk_jobs >> std::max(0, ramp - (int)k)));
        }
        if (r[0] == 0 && r[1] == n && chunk_jobs == 4096 && ramp == 1) CHECK(cuts.size() - 1 >= 4);
      }
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: %s <vote count of each certificate of the set>\n", argv[0]);
    return 2;
  }
  std::vector<size_t> set_votes;
  for (int i = 1; i < argc; i++) set_votes.push_back((size_t)strtoull(argv[i], nullptr, 10));
  certificates();
  inline_limit();
  messages(false);
  messages(true);
  chunk_cuts(set_votes);
  printf("stage ok: %d bad\n", g_bad);
  return g_bad != 0;
}

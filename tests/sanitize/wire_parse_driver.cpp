// Stand-alone driver of tests/test_wire_parse_host.py: the library's one frame
// grammar, xrpl-coa-prototype_amd/csrc/coa_wire_parse.h, against the
// independent container-based model tests/sanitize/wire_model.h, frame by
// frame, under -fsanitize=address,undefined.  Every frame is copied into an
// exactly sized heap block (an over-read is caught) and decoded three ways:
// by the model; through the shared header the way the kernels do it (the
// sequential walk, and the 64-lane split of the votes and of the set entries);
// and by coa_wire_scan / coa_wire_decode_* of csrc/coa_wire.cpp, the host's
// sequential driver of the same header.  Both are compared with the model:
// kind, lengths and every output byte.  The only allowed difference is the
// lanes' COA_WIRE_ECAPACITY for a frame the model accepts whose sets are over
// COA_WIRE_DEV_MAX_ENTRIES; the host entries have no cap and are compared in
// full on those frames too.
//
// usage: wire_parse_driver <corpus dir> <case file> <mutations>
//   corpus dir  tests/fuzz/wire_corpus (every *.bin is one frame)
//   case file   u64 LE length | frame, repeated: the constructed cases
// Inputs: the corpus, every strict prefix of each corpus frame under 1 KiB,
// `mutations` seeded mutations of the corpus (byte flips, length-prefix edits,
// splices), the case file, and one oversized header frame made here (300,000
// payload entries, about 11 MB: an order of the host's sets that is quadratic
// does not finish it).  Prints "ok <frames> frames".
#include <dirent.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "coa_wire_parse.h"
#include "wire_model.h"

namespace {

using Bytes = std::vector<uint8_t>;
size_t g_frames = 0, g_capacity = 0, g_fallback = 0, g_by_kind[4] = {}, g_errors = 0;

[[noreturn]] void die(const char* what, const Bytes& f) {
  std::fprintf(stderr, "FAIL: %s (frame of %zu bytes, frame #%zu)\n", what, f.size(), g_frames);
  for (size_t i = 0; i < f.size() && i < 64; i++) std::fprintf(stderr, "%02x", f[i]);
  std::fprintf(stderr, "\n");
  std::exit(1);
}

struct Rng {
  uint64_t s;
  uint64_t next() {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
  }
  size_t below(size_t n) { return n ? (size_t)(next() % n) : 0; }
};

// The vote list as the kernel's 64 lanes take it (votes_do of
// coa_wire_dev.hip): speculation, then one coa_wp_vote per lane and the
// reduction to the earliest error; the walk when the speculation fails.
int votes_lanes(const uint8_t* p, size_t n, const CoaWpFrame& f, uint8_t* pks, uint8_t* sigs, bool& walked) {
  bool canon = true;
  for (uint64_t k = 0; k < f.nv; k++) canon = canon && coa_wp_vote_canonical(p, n, f.votes, k);
  walked = !canon;
  if (!canon) return coa_wp_votes(p, n, f.votes, f.nv, pks, sigs);
  uint64_t first = COA_WP_NO_ERROR;
  for (uint64_t k = f.nv; k-- > 0;) {  // any lane order reduces to the same word
    size_t pos = f.votes + (size_t)k * COA_WP_VOTE_STRIDE;
    const int rc = coa_wp_vote(p, n, &pos, pks ? pks + k * 32 : nullptr, nullptr);
    first = std::min(first, coa_wp_error_word(k, rc));
  }
  const int rc = coa_wp_error_code(first);
  if (sigs && rc == COA_OK)
    for (uint64_t w = 0; w < f.nv * 16; w++)
      coa_wp_put32(sigs + w * 4, coa_wp_u32(p + coa_wp_canonical_sig_word(f.votes, w)));
  return rc;
}

struct Scan {
  int32_t kind;
  uint64_t hb, nv;
  uint32_t P, Q;
  CoaWpFrame f;
};

uint32_t set_last(const uint8_t* base, size_t stride, uint32_t n, uint8_t* last) {
  uint32_t c = 0;
  for (uint32_t i = 0; i < n; i++) c += (last[i] = coa_wp_is_last(base, stride, n, i));
  return c;
}

void set_emit(const uint8_t* base, size_t stride, uint32_t n, const uint8_t* last, uint8_t* out) {
  for (uint32_t i = 0; i < n; i++)
    if (last[i]) coa_wp_copy(out + (size_t)coa_wp_rank(base, stride, n, i, last) * stride, base + (size_t)i * stride, stride);
}

// k_wire_scan for one frame
Scan scan_frame(const uint8_t* p, size_t n) {
  Scan s{};
  s.kind = coa_wp_walk(p, n, &s.f);
  if (s.kind == COA_MSG_CERTIFICATE) {
    bool walked = false;
    const int rc = votes_lanes(p, n, s.f, nullptr, nullptr, walked);
    const int rc_walk = coa_wp_votes(p, n, s.f.votes, s.f.nv, nullptr, nullptr);
    if (rc != rc_walk) die("the lanes and the walk disagree on the vote list", Bytes(p, p + n));
    g_fallback += walked;
    if (rc != COA_OK) s.kind = rc;
  }
  s.kind = coa_wp_capacity(s.kind, s.f.np, s.f.nq);
  if (s.kind == COA_MSG_HEADER || s.kind == COA_MSG_CERTIFICATE) {
    uint8_t last[COA_WIRE_DEV_MAX_ENTRIES];
    s.P = set_last(p + s.f.payload, 36, (uint32_t)s.f.np, last);
    s.Q = set_last(p + s.f.parents, 32, (uint32_t)s.f.nq, last);
    s.hb = coa_wp_digest_len(s.P, s.Q);
    s.nv = s.f.nv;
  }
  return s;
}

// An output array of exactly `bytes` bytes, pre-filled so that a byte the
// decode leaves out shows.
std::unique_ptr<uint8_t[]> out_block(size_t bytes, uint8_t fill) {
  std::unique_ptr<uint8_t[]> b(new uint8_t[bytes]);
  std::memset(b.get(), fill, bytes);
  return b;
}

// One frame's decoded outputs, each array exactly sized.  A Header or
// Certificate fills hd, id, author, sig (and vp, vs); a Vote id, origin,
// author, sig.
struct Out {
  size_t hb, nv;
  std::unique_ptr<uint8_t[]> hd, id, origin, author, sig, vp, vs;
  uint64_t round = ~0ull;
  uint32_t P = 99;
  Out(size_t hb_, size_t nv_, uint8_t fill)
      : hb(hb_), nv(nv_), hd(out_block(hb, fill)), id(out_block(32, fill)), origin(out_block(32, fill)),
        author(out_block(32, fill)), sig(out_block(64, fill)), vp(out_block(nv * 32, fill)), vs(out_block(nv * 64, fill)) {}
};

// What the model says of a frame.
struct Model {
  wire_model::Frame m;
  int32_t kind;
  Bytes hd;  // the Header::digest input
  size_t nv = 0;
  Model(const uint8_t* p, size_t n) : kind(wire_model::parse(p, n, m)) {
    if (kind == COA_MSG_HEADER || kind == COA_MSG_CERTIFICATE) {
      hd.resize(wire_model::digest_input_len(m.h));
      wire_model::digest_input(m.h, hd.data());
    }
    if (kind == COA_MSG_CERTIFICATE) nv = m.vote_pks.size() / 32;
  }
};

// Every output byte of a decoded frame against the model's.
void compare(const Out& o, const Model& w, const char* who, const Bytes& frame) {
  const auto fail = [&](const char* what) { die((std::string(who) + ": " + what).c_str(), frame); };
  const wire_model::Frame& m = w.m;
  if (w.kind == COA_MSG_VOTE) {
    if (std::memcmp(o.id.get(), m.vid, 32) || std::memcmp(o.origin.get(), m.vorigin, 32) ||
        std::memcmp(o.author.get(), m.vauthor, 32) || std::memcmp(o.sig.get(), m.vsig, 64) || o.round != m.vround)
      fail("vote fields differ");
    return;
  }
  if (o.hb != w.hd.size() || o.P != m.h.payload.size() || o.round != m.h.round)
    fail("header length, payload count or round differs");
  if (std::memcmp(o.hd.get(), w.hd.data(), o.hb)) fail("digest input differs");
  if (std::memcmp(o.id.get(), m.h.id, 32) || std::memcmp(o.author.get(), m.h.author, 32) ||
      std::memcmp(o.sig.get(), m.h.sig, 64))
    fail("header fields differ");
  if (o.nv != w.nv) fail("vote count differs");
  if (o.nv && (std::memcmp(o.vp.get(), m.vote_pks.data(), o.nv * 32) || std::memcmp(o.vs.get(), m.vote_sigs.data(), o.nv * 64)))
    fail("votes differ");
}

// The lane emulation (k_wire_scan, then k_wire_decode, for one frame) against
// the model.  The only allowed difference is COA_WIRE_ECAPACITY; true then.
bool check_lanes(const uint8_t* p, size_t n, const Model& w, const Bytes& frame) {
  const Scan s = scan_frame(p, n);
  if (s.kind == COA_WIRE_ECAPACITY) {
    if (w.kind != COA_MSG_HEADER && w.kind != COA_MSG_CERTIFICATE) die("ECAPACITY for a frame the model rejects", frame);
    if (s.f.np <= COA_WIRE_DEV_MAX_ENTRIES && s.f.nq <= COA_WIRE_DEV_MAX_ENTRIES) die("ECAPACITY under the cap", frame);
    if (s.hb || s.nv) die("ECAPACITY with lengths", frame);
    return true;
  }
  if (s.kind != w.kind) {
    std::fprintf(stderr, "kind %d, model %d\n", s.kind, w.kind);
    die("lanes: kind differs", frame);
  }
  if (s.hb != w.hd.size() || s.nv != w.nv) die("lanes: lengths differ", frame);
  if (s.kind < 0 || s.kind == COA_MSG_CERT_REQUEST) return false;

  Out o((size_t)s.hb, (size_t)s.nv, 0xa5);
  if (s.kind == COA_MSG_VOTE) {
    coa_wp_copy(o.id.get(), p + s.f.v_id, 32);
    coa_wp_copy(o.sig.get(), p + s.f.v_sig, 64);
    o.round = s.f.v_round;
    size_t pos = s.f.v_origin;
    if (coa_wp_key(p, n, &pos, o.origin.get()) != COA_OK) die("vote origin", frame);
    pos = s.f.v_author;
    if (coa_wp_key(p, n, &pos, o.author.get()) != COA_OK) die("vote author", frame);
  } else {
    size_t pos = s.f.author;
    if (coa_wp_key(p, n, &pos, o.hd.get()) != COA_OK) die("author", frame);
    pos = s.f.author;
    (void)coa_wp_key(p, n, &pos, o.author.get());
    for (int b = 0; b < 8; b++) o.hd[32 + b] = (uint8_t)(s.f.round >> (8 * b));
    o.round = s.f.round;
    uint8_t last[COA_WIRE_DEV_MAX_ENTRIES];
    o.P = set_last(p + s.f.payload, 36, (uint32_t)s.f.np, last);
    set_emit(p + s.f.payload, 36, (uint32_t)s.f.np, last, o.hd.get() + 40);
    (void)set_last(p + s.f.parents, 32, (uint32_t)s.f.nq, last);
    set_emit(p + s.f.parents, 32, (uint32_t)s.f.nq, last, o.hd.get() + 40 + 36 * (size_t)o.P);
    coa_wp_copy(o.id.get(), p + s.f.id, 32);
    coa_wp_copy(o.sig.get(), p + s.f.sig, 64);
    bool walked = false;
    if (s.kind == COA_MSG_CERTIFICATE && votes_lanes(p, n, s.f, o.vp.get(), o.vs.get(), walked) != COA_OK)
      die("votes", frame);
  }
  compare(o, w, "lanes", frame);
  return false;
}

// The library's host entries (coa_wire.cpp, the sequential driver of the same
// header) against the model: every frame, those over the device's cap too.
void check_host(const uint8_t* p, size_t n, const Model& w, const Bytes& frame) {
  const uint64_t offs[2] = {0, n};
  int32_t hk = 0;
  uint64_t hhb = 0, hnv = 0;
  const uint8_t dummy = 0;
  if (coa_wire_scan(n ? p : &dummy, offs, 1, &hk, &hhb, &hnv) != COA_OK) die("coa_wire_scan failed", frame);
  if (hk != w.kind) {
    std::fprintf(stderr, "kind %d, model %d\n", hk, w.kind);
    die("host: kind differs", frame);
  }
  if (hhb != w.hd.size() || hnv != w.nv) die("host: lengths differ", frame);
  if (hk < 0 || hk == COA_MSG_CERT_REQUEST) return;

  Out o((size_t)hhb, (size_t)hnv, 0x5a);
  uint64_t hoff[2] = {9, 9}, voff[2] = {9, 0};
  int rc;
  if (hk == COA_MSG_VOTE)
    rc = coa_wire_decode_votes(p, offs, 1, o.id.get(), &o.round, o.origin.get(), o.author.get(), o.sig.get());
  else if (hk == COA_MSG_CERTIFICATE)
    rc = coa_wire_decode_certificates(p, offs, 1, o.hd.get(), hoff, o.id.get(), o.author.get(), o.sig.get(), &o.round,
                                      o.vp.get(), o.vs.get(), voff, &o.P);
  else
    rc = coa_wire_decode_headers(p, offs, 1, o.hd.get(), hoff, o.id.get(), o.author.get(), o.sig.get(), &o.round, &o.P);
  if (rc != COA_OK) die("host decode failed", frame);
  if (hk != COA_MSG_VOTE && (hoff[0] != 0 || hoff[1] != hhb)) die("host: header offsets differ", frame);
  if (hk == COA_MSG_CERTIFICATE && (voff[0] != 0 || voff[1] != hnv)) die("host: vote offsets differ", frame);
  compare(o, w, "host", frame);
}

void check_frame(const Bytes& frame) {
  g_frames++;
  const size_t n = frame.size();
  std::unique_ptr<uint8_t[]> block(new uint8_t[n]);  // exactly sized: ASan sees one byte too many
  if (n) std::memcpy(block.get(), frame.data(), n);
  const uint8_t* p = block.get();

  const Model w(p, n);
  check_host(p, n, w, frame);
  if (check_lanes(p, n, w, frame))
    g_capacity++;
  else if (w.kind < 0)
    g_errors++;
  else
    g_by_kind[w.kind]++;
}

std::vector<Bytes> read_corpus(const std::string& dir) {
  std::vector<std::string> names;
  DIR* d = opendir(dir.c_str());
  if (!d) {
    std::fprintf(stderr, "cannot open %s\n", dir.c_str());
    std::exit(2);
  }
  while (dirent* e = readdir(d)) {
    const std::string nm = e->d_name;
    if (nm.size() > 4 && nm.substr(nm.size() - 4) == ".bin") names.push_back(nm);
  }
  closedir(d);
  std::sort(names.begin(), names.end());
  std::vector<Bytes> out;
  for (auto& nm : names) {
    FILE* f = std::fopen((dir + "/" + nm).c_str(), "rb");
    if (!f) std::exit(2);
    Bytes b;
    uint8_t buf[4096];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + k);
    std::fclose(f);
    out.push_back(std::move(b));
  }
  return out;
}

std::vector<Bytes> read_cases(const char* path) {
  std::vector<Bytes> out;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  uint8_t lenb[8];
  while (std::fread(lenb, 1, 8, f) == 8) {
    Bytes b((size_t)coa_wp_u64(lenb));
    if (!b.empty() && std::fread(b.data(), 1, b.size(), f) != b.size()) std::exit(2);
    out.push_back(std::move(b));
  }
  std::fclose(f);
  return out;
}

Bytes mutate(const std::vector<Bytes>& corpus, Rng& r) {
  Bytes f = corpus[r.below(corpus.size())];
  switch (r.below(4)) {
    case 0:  // byte flips
      for (size_t k = 1 + r.below(4); k-- > 0 && !f.empty();) f[r.below(f.size())] ^= (uint8_t)(1u << r.below(8));
      break;
    case 1: {  // a length prefix (or anything else 8 bytes wide) edited
      if (f.size() < 12) break;
      const size_t at = 4 + r.below(f.size() - 11);
      const uint64_t pick[] = {0, 1, 43, 44, 45, 64, (uint64_t)f.size(), (uint64_t)f.size() / 32, 1025, 1ull << 32,
                               ~0ull, coa_wp_u64(&f[at]) + 1, coa_wp_u64(&f[at]) - 1};
      const uint64_t v = pick[r.below(sizeof pick / sizeof *pick)];
      for (int b = 0; b < 8; b++) f[at + b] = (uint8_t)(v >> (8 * b));
      break;
    }
    case 2: {  // splice: the head of one frame, the tail of another
      const Bytes& g = corpus[r.below(corpus.size())];
      f.resize(r.below(f.size() + 1));
      const size_t from = r.below(g.size() + 1);
      f.insert(f.end(), g.begin() + from, g.end());
      break;
    }
    default:  // a key string's characters: random bytes in a short window
      if (f.size() > 16) {
        const size_t at = r.below(f.size() - 8);
        for (size_t k = 0; k < 1 + r.below(3); k++) f[at + r.below(8)] = (uint8_t)r.next();
      }
      break;
  }
  if (r.below(8) == 0) f.resize(r.below(f.size() + 1));
  return f;
}

void put_u64(Bytes& f, uint64_t v) {
  for (int b = 0; b < 8; b++) f.push_back((uint8_t)(v >> (8 * b)));
}

// Key j of the oversized frame: bytes of every value, the high ones among them
// (the order is of unsigned bytes), and distinct for distinct j.
void put_key(Bytes& f, uint32_t j) {
  Rng r{0x2545f4914f6cdd1dull * (j + 1)};
  for (int b = 0; b < 28; b++) f.push_back((uint8_t)(r.next() >> 32));
  for (int b = 0; b < 4; b++) f.push_back((uint8_t)(j >> (8 * b)));
}

// A Header far over the device's cap, for the host entries alone: 300,000
// payload entries drawn from 100,000 keys (each repeated entry with another
// worker id, so the last one shows) and 5,000 parents drawn from 1,500.
Bytes oversized_frame() {
  static const char kB64[] = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/";
  Rng r{0x6a09e667f3bcc909ull};
  Bytes f = {0, 0, 0, 0};  // Header
  put_u64(f, 44);
  for (int k = 0; k < 42; k++) f.push_back((uint8_t)kB64[r.below(64)]);
  f.push_back((uint8_t)kB64[4 * r.below(16)]);  // 43 symbols are 32 bytes and two trailing bits, which are zero
  f.push_back('=');
  put_u64(f, 77);  // round
  const uint32_t np = 300000, nq = 5000;
  put_u64(f, np);
  for (uint32_t k = 0; k < np; k++) {
    put_key(f, (uint32_t)r.below(100000));
    for (int b = 0; b < 4; b++) f.push_back((uint8_t)(k >> (8 * b)));
  }
  put_u64(f, nq);
  for (uint32_t k = 0; k < nq; k++) put_key(f, 1000000 + (uint32_t)r.below(1500));
  for (int b = 0; b < 96; b++) f.push_back((uint8_t)r.next());  // id | signature
  return f;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s <corpus dir> <case file> <mutations>\n", argv[0]);
    return 2;
  }
  // the offsets rule, before any byte is read
  if (!coa_wp_frame_range(0, 0, 0) || !coa_wp_frame_range(3, 10, 10) || coa_wp_frame_range(3, 11, 10) ||
      coa_wp_frame_range(7, 3, 10) || coa_wp_frame_range(~0ull, 5, 10) || coa_wp_frame_range(11, 11, 10)) {
    std::fprintf(stderr, "FAIL: coa_wp_frame_range\n");
    return 1;
  }
  // the dword stores, at every alignment of source and destination
  for (size_t so = 0; so < 4; so++)
    for (size_t dd = 0; dd < 4; dd++)
      for (size_t k = 0; k <= 36; k++) {
        std::unique_ptr<uint8_t[]> src(new uint8_t[so + k]), dst(new uint8_t[dd + k]);
        for (size_t i = 0; i < so + k; i++) src[i] = (uint8_t)(7 * i + 3);
        coa_wp_copy(dst.get() + dd, src.get() + so, k);
        if (k && std::memcmp(dst.get() + dd, src.get() + so, k)) {
          std::fprintf(stderr, "FAIL: coa_wp_copy\n");
          return 1;
        }
      }
  const std::vector<Bytes> corpus = read_corpus(argv[1]);
  if (corpus.empty()) return 2;
  for (auto& f : corpus) check_frame(f);
  for (auto& f : corpus)
    if (f.size() < 1024)
      for (size_t k = 0; k < f.size(); k++) check_frame(Bytes(f.begin(), f.begin() + k));
  Rng r{0x9e3779b97f4a7c15ull};
  for (long k = std::atol(argv[3]); k-- > 0;) check_frame(mutate(corpus, r));
  for (auto& f : read_cases(argv[2])) check_frame(f);
  {
    const Bytes big = oversized_frame();
    const uint64_t offs[2] = {0, big.size()};
    int32_t kind = 0;
    uint64_t hb = 0;
    auto t0 = std::chrono::steady_clock::now();
    if (coa_wire_scan(big.data(), offs, 1, &kind, &hb, nullptr) != COA_OK || kind != COA_MSG_HEADER)
      die("the oversized frame is not a header", big);
    const double scan_s = seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    check_frame(big);
    std::printf("oversized frame: %zu bytes, digest input %llu bytes; coa_wire_scan %.3f s, model + scan + decode + compare %.3f s\n",
                big.size(), (unsigned long long)hb, scan_s, seconds_since(t0));
  }
  std::printf("headers %zu votes %zu certificates %zu requests %zu errors %zu capacity %zu walked %zu\n", g_by_kind[0],
              g_by_kind[1], g_by_kind[2], g_by_kind[3], g_errors, g_capacity, g_fallback);
  std::printf("ok %zu frames\n", g_frames);
  return 0;
}

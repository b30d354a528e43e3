// Stand-alone driver of tests/test_wire_parse_host.py: the frame grammar of
// xrpl-coa-prototype_amd/csrc/coa_wire_parse.h -- what the device decoder's
// lanes run -- against the host decoder csrc/coa_wire.cpp, frame by frame,
// under -fsanitize=address,undefined.  Every frame is copied into an exactly
// sized heap block (an over-read is caught), scanned and decoded through the
// shared header the way the kernels do it (the sequential walk, and the 64-lane
// split of the votes and of the set entries), and compared with
// coa_wire_scan / coa_wire_decode_*: kind, lengths and every output byte.  The
// only allowed difference is COA_WIRE_ECAPACITY for a frame the host accepts
// whose sets are over COA_WIRE_DEV_MAX_ENTRIES.
//
// usage: wire_parse_driver <corpus dir> <case file> <mutations>
//   corpus dir  tests/fuzz/wire_corpus (every *.bin is one frame)
//   case file   u64 LE length | frame, repeated: the constructed cases
// Inputs: the corpus, every strict prefix of each corpus frame under 1 KiB,
// `mutations` seeded mutations of the corpus (byte flips, length-prefix edits,
// splices), the case file.  Prints "ok <frames> frames".
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "coa_wire_parse.h"

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

void check_frame(const Bytes& frame) {
  g_frames++;
  const size_t n = frame.size();
  std::unique_ptr<uint8_t[]> block(new uint8_t[n]);  // exactly sized: ASan sees one byte too many
  if (n) std::memcpy(block.get(), frame.data(), n);
  const uint8_t* p = block.get();

  const Scan s = scan_frame(p, n);

  const uint64_t offs[2] = {0, n};
  int32_t hk = 0;
  uint64_t hhb = 0, hnv = 0;
  const uint8_t dummy = 0;
  if (coa_wire_scan(n ? p : &dummy, offs, 1, &hk, &hhb, &hnv) != COA_OK) die("coa_wire_scan failed", frame);

  if (s.kind == COA_WIRE_ECAPACITY) {
    if (hk != COA_MSG_HEADER && hk != COA_MSG_CERTIFICATE) die("ECAPACITY for a frame the host rejects", frame);
    if (s.f.np <= COA_WIRE_DEV_MAX_ENTRIES && s.f.nq <= COA_WIRE_DEV_MAX_ENTRIES) die("ECAPACITY under the cap", frame);
    if (s.hb || s.nv) die("ECAPACITY with lengths", frame);
    g_capacity++;
    return;
  }
  if (s.kind != hk) {
    std::fprintf(stderr, "kind %d, host %d\n", s.kind, hk);
    die("kind differs", frame);
  }
  if (s.hb != hhb || s.nv != hnv) die("lengths differ", frame);
  if (hk < 0) {
    g_errors++;
    return;
  }
  g_by_kind[hk]++;

  if (hk == COA_MSG_VOTE) {
    auto ids = out_block(32, 0xa5), orig = out_block(32, 0xa5), auth = out_block(32, 0xa5), sig = out_block(64, 0xa5);
    auto hids = out_block(32, 0x5a), horig = out_block(32, 0x5a), hauth = out_block(32, 0x5a), hsig = out_block(64, 0x5a);
    uint64_t hround = 0;
    if (coa_wire_decode_votes(p, offs, 1, hids.get(), &hround, horig.get(), hauth.get(), hsig.get()) != COA_OK)
      die("coa_wire_decode_votes failed", frame);
    coa_wp_copy(ids.get(), p + s.f.v_id, 32);
    coa_wp_copy(sig.get(), p + s.f.v_sig, 64);
    size_t pos = s.f.v_origin;
    if (coa_wp_key(p, n, &pos, orig.get()) != COA_OK) die("vote origin", frame);
    pos = s.f.v_author;
    if (coa_wp_key(p, n, &pos, auth.get()) != COA_OK) die("vote author", frame);
    if (std::memcmp(ids.get(), hids.get(), 32) || std::memcmp(orig.get(), horig.get(), 32) ||
        std::memcmp(auth.get(), hauth.get(), 32) || std::memcmp(sig.get(), hsig.get(), 64) || s.f.v_round != hround)
      die("vote fields differ", frame);
    return;
  }
  if (hk == COA_MSG_CERT_REQUEST) return;

  // Header / Certificate: k_wire_decode for one frame
  const size_t hb = (size_t)s.hb, nv = (size_t)s.nv;
  auto hd = out_block(hb, 0xa5), id = out_block(32, 0xa5), author = out_block(32, 0xa5), sig = out_block(64, 0xa5);
  auto vp = out_block(nv * 32, 0xa5), vs = out_block(nv * 64, 0xa5);
  size_t pos = s.f.author;
  if (coa_wp_key(p, n, &pos, hd.get()) != COA_OK) die("author", frame);
  pos = s.f.author;
  (void)coa_wp_key(p, n, &pos, author.get());
  for (int b = 0; b < 8; b++) hd[32 + b] = (uint8_t)(s.f.round >> (8 * b));
  uint8_t last[COA_WIRE_DEV_MAX_ENTRIES];
  const uint32_t P = set_last(p + s.f.payload, 36, (uint32_t)s.f.np, last);
  set_emit(p + s.f.payload, 36, (uint32_t)s.f.np, last, hd.get() + 40);
  (void)set_last(p + s.f.parents, 32, (uint32_t)s.f.nq, last);
  set_emit(p + s.f.parents, 32, (uint32_t)s.f.nq, last, hd.get() + 40 + 36 * (size_t)P);
  coa_wp_copy(id.get(), p + s.f.id, 32);
  coa_wp_copy(sig.get(), p + s.f.sig, 64);
  if (hk == COA_MSG_CERTIFICATE) {
    bool walked = false;
    if (votes_lanes(p, n, s.f, vp.get(), vs.get(), walked) != COA_OK) die("votes", frame);
  }

  auto hhd = out_block(hb, 0x5a), hid = out_block(32, 0x5a), hauthor = out_block(32, 0x5a), hsig = out_block(64, 0x5a);
  auto hvp = out_block(nv * 32, 0x5a), hvs = out_block(nv * 64, 0x5a);
  uint64_t hoff[2] = {9, 9}, hvoff[2] = {9, 9}, hround = 0;
  uint32_t hpc = 99;
  int rc;
  if (hk == COA_MSG_CERTIFICATE)
    rc = coa_wire_decode_certificates(p, offs, 1, hhd.get(), hoff, hid.get(), hauthor.get(), hsig.get(), &hround,
                                      hvp.get(), hvs.get(), hvoff, &hpc);
  else
    rc = coa_wire_decode_headers(p, offs, 1, hhd.get(), hoff, hid.get(), hauthor.get(), hsig.get(), &hround, &hpc);
  if (rc != COA_OK) die("host decode failed", frame);
  if (hoff[1] != hb || hpc != P || hround != s.f.round) die("header length, payload count or round differs", frame);
  if (std::memcmp(hd.get(), hhd.get(), hb)) die("digest input differs", frame);
  if (std::memcmp(id.get(), hid.get(), 32) || std::memcmp(author.get(), hauthor.get(), 32) ||
      std::memcmp(sig.get(), hsig.get(), 64))
    die("header fields differ", frame);
  if (hk == COA_MSG_CERTIFICATE) {
    if (hvoff[1] != nv) die("vote count differs", frame);
    if (std::memcmp(vp.get(), hvp.get(), nv * 32) || std::memcmp(vs.get(), hvs.get(), nv * 64)) die("votes differ", frame);
  }
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
  std::printf("headers %zu votes %zu certificates %zu requests %zu errors %zu capacity %zu walked %zu\n", g_by_kind[0],
              g_by_kind[1], g_by_kind[2], g_by_kind[3], g_errors, g_capacity, g_fallback);
  std::printf("ok %zu frames\n", g_frames);
  return 0;
}

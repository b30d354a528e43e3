// What a shard's staging block holds and how it is packed (coa_dag.cpp):
// the arrays of certificates or messages [lo, hi) of a host-pointer call,
// carved into one block that crosses to the device with ONE copy.  Host code
// only (no HIP), so tests/sanitize/stage_driver.cpp builds it with plain g++.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Raw status bits of the certificate and message kernels (the low three are
// the public COA_CERT_BAD_* bits of include/coa_verify.h).
#define COA_CST_BAD_HEADER_ID 1u
#define COA_CST_BAD_HEADER_SIG 2u
#define COA_CST_BAD_VOTES 4u
#define COA_CST_VOTES_INCONCLUSIVE 8u  // some vote failed its own equation, or a key has torsion
#define COA_CST_UNCACHED 16u           // author or a voter is not in the registered committee

// One section of a block: `bytes` at offset `at` (bytes 0: not in this block).
struct Sec {
  size_t at = 0, bytes = 0;
};

// Carves sections off a block, each starting at a multiple of `align`.
struct Carve {
  size_t align, end = 0;
  Sec take(size_t bytes) {
    const Sec s{end, bytes};
    end = align_up(end + bytes, align);
    return s;
  }
};

// One host copy (CopyPool, coa_hostpool.h).
struct Seg {
  void* dst;
  const void* src;
  size_t bytes;
};

// The copies that fill one block: a fixed array, so the one-certificate
// latency path allocates nothing for it.
struct SegList {
  Seg s[8];
  size_t n = 0;
  void add(void* dst, const void* src, size_t bytes) { s[n++] = {dst, src, bytes}; }
  const Seg* begin() const { return s; }
  const Seg* end() const { return s + n; }
};

// ------------------------------------------------------------------------
// Certificates: the caller's arrays, as coa_certificate_verify_many takes them.
struct CertIn {
  const uint8_t* hdr_data;
  const uint64_t* hdr_off;
  const uint8_t* ids;
  const uint8_t* origins;
  const uint8_t* hsigs;
  const uint64_t* rounds;
  const uint8_t* vpks;
  const uint8_t* vsigs;
  const uint64_t* voff;
};

// hdata carries 16 bytes of slack (zeroed) after the header bytes for the
// kernels' aligned-dword reads.  pcounts (payload counts in), proto and verd
// (protocol and verdict words, written on the device) have size 0 unless the
// call wants verdicts.
struct CertPack {
  Sec status, hoff, voff, ids, origins, hsigs, rounds, vpks, vsigs, hdata, pcounts, proto, verd;
  size_t total = 0;
};

// The arrays of a block laid out as p at address base (host or device).
inline CertIn cert_view(const uint8_t* base, const CertPack& p) {
  auto u64 = [base](const Sec& s) { return reinterpret_cast<const uint64_t*>(base + s.at); };
  return {base + p.hdata.at, u64(p.hoff), base + p.ids.at, base + p.origins.at, base + p.hsigs.at,
          u64(p.rounds),     base + p.vpks.at, base + p.vsigs.at, u64(p.voff)};
}

// inl: the record inline in the latency kernel's arguments -- 16-byte
// sections and no status words (they live in the context's counter block);
// otherwise the shard form, 256-byte sections.
inline CertPack cert_layout(size_t nc, size_t nv, size_t hbytes, bool verdicts, bool inl = false) {
  CertPack p;
  Carve c{inl ? (size_t)16 : (size_t)256};
  p.status = c.take(inl ? 0 : nc * 4);
  p.hoff = c.take((nc + 1) * 8);
  p.voff = c.take((nc + 1) * 8);
  p.ids = c.take(nc * 32);
  p.origins = c.take(nc * 32);
  p.hsigs = c.take(nc * 64);
  p.rounds = c.take(nc * 8);
  p.vpks = c.take(nv * 32);
  p.vsigs = c.take(nv * 64);
  p.hdata = c.take(hbytes + 16);
  p.pcounts = c.take(verdicts ? nc * 4 : 0);
  p.proto = c.take(verdicts ? nc * 4 : 0);
  p.verd = c.take(verdicts ? nc * 4 : 0);
  p.total = c.end;
  return p;
}

// Certificates [lo, hi) of `in` into block h laid out as p =
// cert_layout(hi - lo, their votes, their header bytes, ...): writes the
// offset arrays rebased to 0, zeroes the status words and the header slack,
// and returns the copies of everything else.  pcounts is read only when p
// has the section.
inline SegList cert_segments(uint8_t* h, const CertPack& p, const CertIn& in, const uint32_t* pcounts, size_t lo,
                             size_t hi) {
  const size_t nc = hi - lo;
  const uint64_t h0 = in.hdr_off[lo], hb = in.hdr_off[hi] - h0;
  const uint64_t v0 = in.voff[lo], nv = in.voff[hi] - v0;
  std::memset(h + p.status.at, 0, p.status.bytes);
  uint64_t* ho = reinterpret_cast<uint64_t*>(h + p.hoff.at);
  uint64_t* vo = reinterpret_cast<uint64_t*>(h + p.voff.at);
  for (size_t i = 0; i <= nc; i++) {
    ho[i] = in.hdr_off[lo + i] - h0;
    vo[i] = in.voff[lo + i] - v0;
  }
  std::memset(h + p.hdata.at + hb, 0, 16);
  SegList segs;
  segs.add(h + p.ids.at, in.ids + lo * 32, nc * 32);
  segs.add(h + p.origins.at, in.origins + lo * 32, nc * 32);
  segs.add(h + p.hsigs.at, in.hsigs + lo * 64, nc * 64);
  segs.add(h + p.rounds.at, in.rounds + lo, nc * 8);
  if (nv) {
    segs.add(h + p.vpks.at, in.vpks + v0 * 32, nv * 32);
    segs.add(h + p.vsigs.at, in.vsigs + v0 * 64, nv * 64);
  }
  if (hb) segs.add(h + p.hdata.at, in.hdr_data + h0, hb);
  if (p.pcounts.bytes) segs.add(h + p.pcounts.at, pcounts + lo, nc * 4);
  return segs;
}

// The inline form of certificates [lo, hi): packed into buf (cap bytes) on
// the calling thread; false, with nothing written, when there are more than
// 64 of them or they do not fit.
inline bool cert_inline_pack(uint8_t* buf, size_t cap, CertPack& p, const CertIn& in, size_t lo, size_t hi) {
  p = cert_layout(hi - lo, in.voff[hi] - in.voff[lo], in.hdr_off[hi] - in.hdr_off[lo], false, true);
  if (p.total > cap || hi - lo > 64) return false;
  for (const Seg& g : cert_segments(buf, p, in, nullptr, lo, hi)) std::memcpy(g.dst, g.src, g.bytes);
  return true;
}

// The chunks of the pipelined certificate path: cuts[k] .. cuts[k + 1] is
// chunk k of [lo, hi).  A chunk closes once it holds chunk_jobs jobs (a
// certificate is 1 + its votes); the first `ramp` chunks are smaller (chunk
// k < ramp closes at chunk_jobs >> (ramp - k)), so the GPU starts after a
// fraction of a chunk's pack and copy.
inline std::vector<size_t> cert_chunk_cuts(const uint64_t* voff, size_t lo, size_t hi, size_t chunk_jobs, int ramp) {
  std::vector<size_t> cuts{lo};
  size_t jobs = 0;
  for (size_t c = lo; c < hi; c++) {
    jobs += 1 + (voff[c + 1] - voff[c]);
    const int k = (int)cuts.size() - 1;  // the chunk being cut
    if (jobs >= (chunk_jobs >> std::max(0, ramp - k)) && c + 1 < hi) {
      cuts.push_back(c + 1);
      jobs = 0;
    }
  }
  cuts.push_back(hi);
  return cuts;
}

// ------------------------------------------------------------------------
// Headers or votes: the caller's arrays, as coa_header_verify_many /
// coa_vote_verify_many take them.
struct MsgIn {
  const uint8_t* hdr_data;  // headers only
  const uint64_t* hdr_off;  // headers only
  const uint8_t* ids;
  const uint64_t* rounds;   // votes only
  const uint8_t* origins;   // votes only
  const uint8_t* authors;
  const uint8_t* sigs;
  bool votes;
};

// Votes carry rounds and origins, headers hoff and hdata (with CertPack's
// slack).  pcounts is headers' only; proto and verd as in CertPack.
struct MsgPack {
  Sec status, ids, authors, sigs, rounds, origins, hoff, hdata, pcounts, proto, verd;
  size_t total = 0;
};

// As cert_view.  The arrays the shape does not have point at the block's
// start and are not read.
inline MsgIn msg_view(const uint8_t* base, const MsgPack& p, bool votes) {
  auto u64 = [base](const Sec& s) { return reinterpret_cast<const uint64_t*>(base + s.at); };
  return {base + p.hdata.at, u64(p.hoff),       base + p.ids.at,  u64(p.rounds),
          base + p.origins.at, base + p.authors.at, base + p.sigs.at, votes};
}

inline MsgPack msg_layout(size_t n, bool votes, size_t hbytes, bool verdicts) {
  MsgPack p;
  Carve c{256};
  p.status = c.take(n * 4);
  p.ids = c.take(n * 32);
  p.authors = c.take(n * 32);
  p.sigs = c.take(n * 64);
  if (votes) {
    p.rounds = c.take(n * 8);
    p.origins = c.take(n * 32);
  } else {
    p.hoff = c.take((n + 1) * 8);
    p.hdata = c.take(hbytes + 16);
    p.pcounts = c.take(verdicts ? n * 4 : 0);
  }
  p.proto = c.take(verdicts ? n * 4 : 0);
  p.verd = c.take(verdicts ? n * 4 : 0);
  p.total = c.end;
  return p;
}

// Messages [lo, hi) of `in` into block h laid out as p = msg_layout(hi - lo,
// in.votes, their header bytes, ...); as cert_segments.
inline SegList msg_segments(uint8_t* h, const MsgPack& p, const MsgIn& in, const uint32_t* pcounts, size_t lo,
                            size_t hi) {
  const size_t n = hi - lo;
  std::memset(h + p.status.at, 0, p.status.bytes);
  SegList segs;
  segs.add(h + p.ids.at, in.ids + lo * 32, n * 32);
  segs.add(h + p.authors.at, in.authors + lo * 32, n * 32);
  segs.add(h + p.sigs.at, in.sigs + lo * 64, n * 64);
  if (in.votes) {
    segs.add(h + p.rounds.at, in.rounds + lo, n * 8);
    segs.add(h + p.origins.at, in.origins + lo * 32, n * 32);
    return segs;
  }
  const uint64_t h0 = in.hdr_off[lo], hb = in.hdr_off[hi] - h0;
  uint64_t* ho = reinterpret_cast<uint64_t*>(h + p.hoff.at);
  for (size_t i = 0; i <= n; i++) ho[i] = in.hdr_off[lo + i] - h0;
  std::memset(h + p.hdata.at + hb, 0, 16);
  if (hb) segs.add(h + p.hdata.at, in.hdr_data + h0, hb);
  if (p.pcounts.bytes) segs.add(h + p.pcounts.at, pcounts + lo, n * 4);
  return segs;
}

// An independent model of the bincode PrimaryMessage decode, for the tests
// only: the container-based decoder the library had before its host decoder
// became a driver of xrpl-coa-prototype_amd/csrc/coa_wire_parse.h.  It is
// deliberately naive and deliberately separate: its own reader, its own base64
// and UTF-8, and std::map / std::set for the BTreeMap / BTreeSet rule (the last
// value of a repeated key, iteration in key order).  It must not include
// coa_wire_parse.h or share a line with it -- tests/sanitize/
// wire_parse_driver.cpp compares the library's one grammar against this second
// statement of the format, and that comparison is worth what their
// independence is worth.  The format itself is described at the top of
// coa_wire_parse.h.
//
// wire_model::parse(p, n, f) is the entry: the frame's kind (COA_MSG_* or the
// first error in wire order) and, for a well-formed frame, its fields in f;
// digest_input_len / digest_input give the Header::digest input of f.h.
#pragma once
#include <array>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "coa_verify.h"

namespace wire_model {

using D32 = std::array<uint8_t, 32>;

struct Rd {
  const uint8_t* p;
  size_t n, i = 0;
  bool ok = true;
  bool take(void* dst, size_t k) {
    if (!ok || n - i < k) return ok = false;
    if (dst) std::memcpy(dst, p + i, k);
    i += k;
    return true;
  }
  uint32_t u32() {
    uint32_t v = 0;
    take(&v, 4);
    return v;
  }
  uint64_t u64() {
    uint64_t v = 0;
    take(&v, 8);
    return v;
  }
};

inline int b64_val(uint8_t c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

// base64 STANDARD decode; false on any malformed input.
inline bool b64_decode(const uint8_t* s, size_t len, std::vector<uint8_t>& out) {
  size_t body = len;
  while (body > 0 && s[body - 1] == '=') body--;
  const size_t pads = len - body;
  if (pads > 2) return false;
  if (body % 4 == 1) return false;
  if (pads && (body + pads) % 4 != 0) return false;
  out.clear();
  uint32_t acc = 0;
  int bits = 0;
  for (size_t i = 0; i < body; i++) {
    const int v = b64_val(s[i]);
    if (v < 0) return false;
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      out.push_back((uint8_t)(acc >> bits));
      acc &= (1u << bits) - 1;
    }
  }
  return acc == 0;  // trailing bits of the last symbol must be zero
}

// serde String: the bytes must be UTF-8 (structure check; a key is ASCII
// base64 anyway, so any non-ASCII byte fails one way or the other)
inline bool utf8_valid(const uint8_t* s, size_t n) {
  size_t i = 0;
  while (i < n) {
    const uint8_t c = s[i];
    size_t k;
    if (c < 0x80) k = 0;
    else if ((c >> 5) == 6) k = 1;
    else if ((c >> 4) == 14) k = 2;
    else if ((c >> 3) == 30) k = 3;
    else return false;
    if (n - i - 1 < k) return false;
    for (size_t j = 1; j <= k; j++)
      if ((s[i + j] & 0xC0) != 0x80) return false;
    i += k + 1;
  }
  return true;
}

inline int read_key(Rd& r, uint8_t out[32]) {
  const uint64_t len = r.u64();
  if (!r.ok || len > r.n - r.i) return COA_WIRE_ETRUNC;
  const uint8_t* s = r.p + r.i;
  r.i += len;
  if (!utf8_valid(s, len)) return COA_WIRE_EFORMAT;
  std::vector<uint8_t> bytes;
  if (!b64_decode(s, len, bytes)) return COA_WIRE_EKEY;
  if (bytes.size() < 32) return COA_WIRE_EKEY;  // the reference panics here
  std::memcpy(out, bytes.data(), 32);
  return COA_OK;
}

struct HeaderV {
  uint8_t author[32];
  uint64_t round;
  std::map<D32, uint32_t> payload;
  std::set<D32> parents;
  uint8_t id[32], sig[64];
};

inline int read_header(Rd& r, HeaderV& h) {
  int rc = read_key(r, h.author);
  if (rc != COA_OK) return rc;
  h.round = r.u64();
  const uint64_t np = r.u64();
  if (!r.ok || np > (r.n - r.i) / 36) return COA_WIRE_ETRUNC;
  for (uint64_t k = 0; k < np; k++) {
    D32 d;
    r.take(d.data(), 32);
    h.payload[d] = r.u32();  // BTreeMap: the last value of a repeated key wins
  }
  const uint64_t nq = r.u64();
  if (!r.ok || nq > (r.n - r.i) / 32) return COA_WIRE_ETRUNC;
  for (uint64_t k = 0; k < nq; k++) {
    D32 d;
    r.take(d.data(), 32);
    h.parents.insert(d);
  }
  r.take(h.id, 32);
  r.take(h.sig, 64);
  return r.ok ? COA_OK : COA_WIRE_ETRUNC;
}

inline size_t digest_input_len(const HeaderV& h) { return 40 + 36 * h.payload.size() + 32 * h.parents.size(); }

inline void digest_input(const HeaderV& h, uint8_t* out) {
  std::memcpy(out, h.author, 32);
  std::memcpy(out + 32, &h.round, 8);
  size_t o = 40;
  for (auto& kv : h.payload) {
    std::memcpy(out + o, kv.first.data(), 32);
    std::memcpy(out + o + 32, &kv.second, 4);
    o += 36;
  }
  for (auto& d : h.parents) {
    std::memcpy(out + o, d.data(), 32);
    o += 32;
  }
}

struct Frame {
  int kind = COA_WIRE_EFORMAT;
  HeaderV h;
  uint8_t vid[32], vorigin[32], vauthor[32], vsig[64];
  uint64_t vround = 0;
  std::vector<uint8_t> vote_pks, vote_sigs;
};

inline int parse(const uint8_t* p, size_t n, Frame& f) {
  Rd r{p, n};
  const uint32_t variant = r.u32();
  if (!r.ok) return f.kind = COA_WIRE_ETRUNC;
  int rc = COA_OK;
  switch (variant) {
    case 0:
      rc = read_header(r, f.h);
      break;
    case 1:
      r.take(f.vid, 32);
      f.vround = r.u64();
      if (!r.ok) return f.kind = COA_WIRE_ETRUNC;
      if ((rc = read_key(r, f.vorigin)) != COA_OK) break;
      if ((rc = read_key(r, f.vauthor)) != COA_OK) break;
      if (!r.take(f.vsig, 64)) rc = COA_WIRE_ETRUNC;
      break;
    case 2: {
      if ((rc = read_header(r, f.h)) != COA_OK) break;
      const uint64_t nv = r.u64();
      if (!r.ok || nv > (r.n - r.i) / (8 + 64)) {
        rc = COA_WIRE_ETRUNC;
        break;
      }
      f.vote_pks.resize(nv * 32);
      f.vote_sigs.resize(nv * 64);
      for (uint64_t k = 0; k < nv && rc == COA_OK; k++) {
        rc = read_key(r, &f.vote_pks[k * 32]);
        if (rc == COA_OK && !r.take(&f.vote_sigs[k * 64], 64)) rc = COA_WIRE_ETRUNC;
      }
      break;
    }
    case 3: {  // CertificatesRequest(Vec<Digest>, PublicKey): no crypto to do
      const uint64_t nd = r.u64();
      if (!r.ok || nd > (r.n - r.i) / 32) return f.kind = COA_WIRE_ETRUNC;
      r.take(nullptr, nd * 32);
      uint8_t k[32];
      rc = read_key(r, k);
      break;
    }
    default:
      return f.kind = COA_WIRE_EFORMAT;
  }
  return f.kind = (rc == COA_OK ? (int)variant : rc);
}

}  // namespace wire_model

// The grammar of a bincode PrimaryMessage frame, written once: the field walk,
// the bounds rules, the UTF-8 and base64 rules of a PublicKey string, the error
// codes' precedence (the first error in wire order decides) and the order of
// 32-byte keys.  The library holds no second copy: csrc/coa_wire.cpp drives
// these functions one frame after the other on the host, csrc/coa_wire_dev.hip
// runs them across a wave's lanes on the device.  What they are pinned against
// is outside the library: the container-based model tests/sanitize/
// wire_model.h, which tests/sanitize/wire_parse_driver.cpp compares with both
// frame by frame.  Plain C++ and also compiled for the device (COA_WP_FN, in
// the way of coa_job_bits.h): no containers, no allocation, no HIP types.
//
// Format: bincode 1.3 `deserialize` (legacy options: little-endian, fixed-
// width integers, u64 length prefixes, trailing bytes allowed) of
//   PrimaryMessage = u32 variant: 0 Header, 1 Vote, 2 Certificate,
//                    3 CertificatesRequest(Vec<Digest>, PublicKey)
//   Header      author PublicKey | round u64 | payload BTreeMap<Digest, u32>
//               | parents BTreeSet<Digest> | id Digest | signature
//   Vote        id | round u64 | origin PublicKey | author PublicKey | signature
//   Certificate header | votes Vec<(PublicKey, Signature)>
//   Digest      32 raw bytes;  Signature  part1 32 | part2 32
//   PublicKey   serde string (u64 length | UTF-8) holding base64 of the key
//               (crypto/src/lib.rs:94-112); decode_base64 keeps the first 32
//               decoded bytes (:72-78)
// (primary/src/messages.rs:13-21,105-112,168-172).  BTreeMap/BTreeSet
// deserialisation keeps the last value of a repeated key and iterates in key
// order, and Header::digest hashes that iteration (messages.rs:70-84), so the
// digest input a decoder emits is author | round LE | (digest | wid LE)* sorted
// | parents* sorted -- the bytes the reference hashes, not the wire bytes.
//
// Errors are per frame (the reference drops a frame whose decode fails).
// Where the reference would PANIC rather than error -- a base64 key that
// decodes to fewer than 32 bytes hits `bytes[..32]` at crypto/src/lib.rs:74
// -- these rules report COA_WIRE_EKEY instead.  base64 0.13 itself is not
// available here: canonical padded keys (what every node emits) are decoded
// exactly; for non-canonical forms this follows base64 0.13's documented
// STANDARD rules (padding optional, no bytes after padding, zero trailing
// bits) -- parity unpinned there.
//
// Every function reads the frame p[0, n) through byte loads only (fields sit
// at arbitrary offsets: key strings are 43, 44, 64 ... characters long) and
// reads no byte before its position has been checked against n.  Positions
// (`pos`) are byte offsets into the frame with pos <= n.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/coa_verify.h"

// Always inlined on the device: a kernel that has staged its frame in LDS
// hands these functions an LDS pointer, and only inlined code lets the compiler
// keep the address space (LDS reads that do not queue behind global stores).
// Spelled out (it is what __forceinline__ expands to) so that a host-only
// translation unit compiled as HIP needs no hip_runtime.h before this header.
#if defined(__HIPCC__)
#define COA_WP_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define COA_WP_FN inline
#endif

#define COA_WP_VOTE_STRIDE 116u  // 8 (length) + 44 (canonical base64 of 32 bytes) + 64 (signature)

COA_WP_FN uint32_t coa_wp_u32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
COA_WP_FN uint64_t coa_wp_u64(const uint8_t* p) { return (uint64_t)coa_wp_u32(p) | ((uint64_t)coa_wp_u32(p + 4) << 32); }

// Outputs are written a dword at a time where the destination allows it (the
// call's arrays are aligned; nothing requires it): the bytes are the same.
COA_WP_FN void coa_wp_put32(uint8_t* dst, uint32_t w) {
  if ((reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
    const uint8_t b[4] = {(uint8_t)w, (uint8_t)(w >> 8), (uint8_t)(w >> 16), (uint8_t)(w >> 24)};
    __builtin_memcpy(__builtin_assume_aligned(dst, 4), b, 4);
  } else {
    for (int i = 0; i < 4; i++) dst[i] = (uint8_t)(w >> (8 * i));
  }
}
COA_WP_FN void coa_wp_copy(uint8_t* dst, const uint8_t* src, size_t k) {
  size_t i = 0;
  for (; i + 4 <= k; i += 4) coa_wp_put32(dst + i, coa_wp_u32(src + i));
  for (; i < k; i++) dst[i] = src[i];
}

// Frame i of a call is bytes [o0, o1) of a buffer of frame_bytes bytes.  False:
// the offsets decrease or leave the buffer -- the frame is COA_WIRE_ETRUNC and
// none of its bytes are read.
COA_WP_FN bool coa_wp_frame_range(uint64_t o0, uint64_t o1, uint64_t frame_bytes) { return o0 <= o1 && o1 <= frame_bytes; }

// Rust's Ord on [u8; 32]: unsigned bytes, lexicographic from byte 0.
COA_WP_FN int coa_wp_key_cmp(const uint8_t* a, const uint8_t* b) {
  for (int i = 0; i < 32; i++)
    if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
  return 0;
}

COA_WP_FN int coa_wp_b64_val(uint8_t c) {
  if (c >= 'A' && c <= 'Z') return c - 'A';
  if (c >= 'a' && c <= 'z') return c - 'a' + 26;
  if (c >= '0' && c <= '9') return c - '0' + 52;
  if (c == '+') return 62;
  if (c == '/') return 63;
  return -1;
}

// serde String: the bytes must be UTF-8 (structure check; a key is ASCII
// base64 anyway, so any non-ASCII byte fails one way or the other)
COA_WP_FN bool coa_wp_utf8_valid(const uint8_t* s, size_t n) {
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

// A PublicKey at *pos: u64 length | string.  The checks in this order:
// the length against the frame's end (COA_WIRE_ETRUNC), UTF-8
// (COA_WIRE_EFORMAT), base64 STANDARD with optional padding, nothing after
// the padding and zero trailing bits, of at least 32 bytes (COA_WIRE_EKEY).
// COA_OK: *pos is behind the string and out (if not null) holds the first 32
// decoded bytes; on an error out's content is unspecified.
COA_WP_FN int coa_wp_key(const uint8_t* p, size_t n, size_t* pos, uint8_t* out) {
  size_t i = *pos;
  if (n - i < 8) return COA_WIRE_ETRUNC;
  const uint64_t len = coa_wp_u64(p + i);
  i += 8;
  if (len > n - i) return COA_WIRE_ETRUNC;
  const uint8_t* s = p + i;
  *pos = i + (size_t)len;
  if (!coa_wp_utf8_valid(s, (size_t)len)) return COA_WIRE_EFORMAT;
  size_t body = (size_t)len;
  while (body > 0 && s[body - 1] == '=') body--;
  const size_t pads = (size_t)len - body;
  if (pads > 2 || body % 4 == 1 || (pads && (body + pads) % 4 != 0)) return COA_WIRE_EKEY;
  uint32_t acc = 0, bits = 0, word = 0;
  size_t nout = 0;
  for (size_t k = 0; k < body; k++) {
    const int v = coa_wp_b64_val(s[k]);
    if (v < 0) return COA_WIRE_EKEY;
    acc = (acc << 6) | (uint32_t)v;
    bits += 6;
    if (bits >= 8) {
      bits -= 8;
      if (out && nout < 32) {  // the first 32 bytes are kept, four at a time
        word |= ((acc >> bits) & 0xffu) << (8 * (nout & 3));
        if ((nout & 3) == 3) {
          coa_wp_put32(out + nout - 3, word);
          word = 0;
        }
      }
      nout++;
      acc &= (1u << bits) - 1;
    }
  }
  if (acc != 0 || nout < 32) return COA_WIRE_EKEY;
  return COA_OK;
}

// What the walk finds: positions of the fields, none of them decoded (the
// walk can hand out the keys it has to check anyway: coa_wp_walk).
struct CoaWpFrame {
  int32_t kind;                      // COA_MSG_* so far, or the first error
  // Header (and Certificate.header)
  size_t author;                     // the author's key string (its length prefix)
  uint64_t round, np, nq;            // wire counts of payload entries and parents
  size_t payload, parents, id, sig;  // np * 36 | nq * 32 | 32 | 64 bytes
  // Certificate
  uint64_t nv;
  size_t votes;  // the first vote: (key string | 64) * nv, of variable stride
  // Vote
  size_t v_id, v_origin, v_author, v_sig;
  uint64_t v_round;
};

// Header at *pos; each count is checked against the bytes left before its
// entries are stepped over.  COA_OK or the first error.  author: null, or 32
// bytes for the decoded key.
COA_WP_FN int coa_wp_header(const uint8_t* p, size_t n, size_t* pos, CoaWpFrame* f, uint8_t* author = nullptr) {
  size_t i = *pos;
  f->author = i;
  const int rc = coa_wp_key(p, n, &i, author);
  if (rc != COA_OK) return rc;
  if (n - i < 16) return COA_WIRE_ETRUNC;
  f->round = coa_wp_u64(p + i);
  f->np = coa_wp_u64(p + i + 8);
  i += 16;
  if (f->np > (n - i) / 36) return COA_WIRE_ETRUNC;
  f->payload = i;
  i += (size_t)f->np * 36;
  if (n - i < 8) return COA_WIRE_ETRUNC;
  f->nq = coa_wp_u64(p + i);
  i += 8;
  if (f->nq > (n - i) / 32) return COA_WIRE_ETRUNC;
  f->parents = i;
  i += (size_t)f->nq * 32;
  if (n - i < 96) return COA_WIRE_ETRUNC;
  f->id = i;
  f->sig = i + 32;
  *pos = i + 96;
  return COA_OK;
}

// The frame up to, and without, a certificate's vote list: f->kind is the
// variant when everything walked is well formed (a Certificate's votes are
// still to be checked: coa_wp_votes or coa_wp_vote per vote), else the error.
// key0, key1: null, or 32 bytes each for the keys the walk checks on its way,
// so that a sequential caller need not read them twice -- a Header's or
// Certificate's author in key0, a Vote's origin in key0 and author in key1;
// their content is unspecified unless the walk returns the variant.
COA_WP_FN int coa_wp_walk(const uint8_t* p, size_t n, CoaWpFrame* f, uint8_t* key0 = nullptr, uint8_t* key1 = nullptr) {
  f->np = f->nq = f->nv = 0;
  if (n < 4) return f->kind = COA_WIRE_ETRUNC;
  const uint32_t variant = coa_wp_u32(p);
  size_t i = 4;
  int rc = COA_OK;
  switch (variant) {
    case COA_MSG_HEADER:
      rc = coa_wp_header(p, n, &i, f, key0);
      break;
    case COA_MSG_VOTE:
      if (n - i < 40) return f->kind = COA_WIRE_ETRUNC;
      f->v_id = i;
      f->v_round = coa_wp_u64(p + i + 32);
      i += 40;
      f->v_origin = i;
      if ((rc = coa_wp_key(p, n, &i, key0)) != COA_OK) break;
      f->v_author = i;
      if ((rc = coa_wp_key(p, n, &i, key1)) != COA_OK) break;
      f->v_sig = i;
      if (n - i < 64) rc = COA_WIRE_ETRUNC;
      break;
    case COA_MSG_CERTIFICATE:
      if ((rc = coa_wp_header(p, n, &i, f, key0)) != COA_OK) break;
      if (n - i < 8) {
        rc = COA_WIRE_ETRUNC;
        break;
      }
      f->nv = coa_wp_u64(p + i);
      i += 8;
      if (f->nv > (n - i) / (8 + 64)) rc = COA_WIRE_ETRUNC;
      f->votes = i;
      break;
    case COA_MSG_CERT_REQUEST: {
      if (n - i < 8) return f->kind = COA_WIRE_ETRUNC;
      const uint64_t nd = coa_wp_u64(p + i);
      i += 8;
      if (nd > (n - i) / 32) return f->kind = COA_WIRE_ETRUNC;
      i += (size_t)nd * 32;
      rc = coa_wp_key(p, n, &i, nullptr);
      break;
    }
    default:
      return f->kind = COA_WIRE_EFORMAT;
  }
  return f->kind = (rc == COA_OK ? (int32_t)variant : rc);
}

// One vote at *pos: key string | signature.  pk (32) and sig (64) may be null.
COA_WP_FN int coa_wp_vote(const uint8_t* p, size_t n, size_t* pos, uint8_t* pk, uint8_t* sig) {
  const int rc = coa_wp_key(p, n, pos, pk);
  if (rc != COA_OK) return rc;
  if (n - *pos < 64) return COA_WIRE_ETRUNC;
  if (sig) coa_wp_copy(sig, p + *pos, 64);
  *pos += 64;
  return COA_OK;
}

// The vote list in wire order (the walk that is always right); pks / sigs
// null or nv * 32 / nv * 64 bytes.
COA_WP_FN int coa_wp_votes(const uint8_t* p, size_t n, size_t pos, uint64_t nv, uint8_t* pks, uint8_t* sigs) {
  for (uint64_t k = 0; k < nv; k++) {
    const int rc = coa_wp_vote(p, n, &pos, pks ? pks + k * 32 : nullptr, sigs ? sigs + k * 64 : nullptr);
    if (rc != COA_OK) return rc;
  }
  return COA_OK;
}

// Speculation on the canonical stride: vote k sits at votes + k *
// COA_WP_VOTE_STRIDE if every earlier vote's key string is 44 long.  True when
// the length prefix at that position is inside the frame and says 44; when it
// holds for every k < nv the positions are exact (induction from vote 0) and
// each vote may be checked on its own with coa_wp_vote.  Anything else: walk.
COA_WP_FN bool coa_wp_vote_canonical(const uint8_t* p, size_t n, size_t votes, uint64_t k) {
  const uint64_t at = (uint64_t)votes + k * COA_WP_VOTE_STRIDE;  // k <= n / 72: no overflow
  return at <= n && n - at >= 8 && coa_wp_u64(p + at) == 44;
}

// With every key string 44 long the signatures are nv * 64 bytes at a fixed
// stride: dword w of them (w < nv * 16) lies here.
COA_WP_FN size_t coa_wp_canonical_sig_word(size_t votes, uint64_t w) {
  return votes + (size_t)(w / 16) * COA_WP_VOTE_STRIDE + 8 + 44 + (size_t)(w % 16) * 4;
}

// Errors found in parallel reduce to the earliest in wire order: the smallest
// of these words (vote index above the code); COA_WP_NO_ERROR when none.
#define COA_WP_NO_ERROR 0xffffffffffffffffull
COA_WP_FN uint64_t coa_wp_error_word(uint64_t index, int rc) {
  return rc == COA_OK ? COA_WP_NO_ERROR : (index << 8) | (uint64_t)(uint8_t)(-rc);
}
COA_WP_FN int coa_wp_error_code(uint64_t word) { return word == COA_WP_NO_ERROR ? COA_OK : -(int)(word & 0xff); }

// A well-formed frame whose sets are beyond what the device sorts:
// COA_WIRE_ECAPACITY (the caller decodes it on the host, which has no cap).
// Every error of the grammar has been decided before this is asked.
COA_WP_FN int32_t coa_wp_capacity(int32_t kind, uint64_t np, uint64_t nq) {
  if ((kind == COA_MSG_HEADER || kind == COA_MSG_CERTIFICATE) &&
      (np > COA_WIRE_DEV_MAX_ENTRIES || nq > COA_WIRE_DEV_MAX_ENTRIES))
    return COA_WIRE_ECAPACITY;
  return kind;
}

// BTreeMap / BTreeSet over n wire entries of `stride` bytes whose first 32 are
// the key.  Entry i survives iff no later entry has its key (BTreeMap::insert:
// the last value of a repeated key wins; for a set any occurrence will do), and
// a survivor's place in key order is the number of survivors with a smaller
// key.  The wire index breaks ties, so the order is total and needs no stable
// network.  `last`: n flags filled from coa_wp_is_last.
COA_WP_FN bool coa_wp_is_last(const uint8_t* base, size_t stride, uint32_t n, uint32_t i) {
  for (uint32_t j = i + 1; j < n; j++)
    if (coa_wp_key_cmp(base + (size_t)j * stride, base + (size_t)i * stride) == 0) return false;
  return true;
}
COA_WP_FN uint32_t coa_wp_rank(const uint8_t* base, size_t stride, uint32_t n, uint32_t i, const uint8_t* last) {
  uint32_t r = 0;
  for (uint32_t j = 0; j < n; j++)
    if (last[j] && coa_wp_key_cmp(base + (size_t)j * stride, base + (size_t)i * stride) < 0) r++;
  return r;
}

// Length of the Header::digest input with P distinct payload keys and Q
// distinct parents.
COA_WP_FN uint64_t coa_wp_digest_len(uint32_t P, uint32_t Q) { return 40 + 36 * (uint64_t)P + 32 * (uint64_t)Q; }


// Committee key cache helpers shared by the committee kernels (coa_committee.hip,
// coa_cert_lat.hip, coa_keybuild.hip) and the single-signature latency kernel
// (coa_latency.hip): word/byte access to 8-dword scalars, per-lane and
// wave-uniform loads, the binary searches (a key among the registered, sorted
// keys; the certificate owning a vote), the hashes every signature job takes
// (the challenge k, Certificate::digest / Vote::digest, the header-id
// compare), and field element exchange between lanes.
#pragma once
#include "coa_fe.h"
#include "coa_sc.h"
#include "coa_sha512.h"

namespace coa_kc {

COA_DEV uint32_t word_sel(const uint32_t* x, int i) {
  // masks, not selects: a select chain over a register array is turned back
  // into dynamic indexing, i.e. a scratch round trip
  uint32_t w = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) w |= x[k] & (0u - (uint32_t)(i == k));
  return w;
}

COA_DEV uint32_t byte_of(const uint32_t* x, int j) { return (word_sel(x, j >> 2) >> (8 * (j & 3))) & 0xffu; }

COA_DEV void load8(uint32_t* d, const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

// wave-uniform copies (SGPRs) of values every lane loaded alike
COA_DEV void load8u(uint32_t* d, const uint32_t* p) {
  load8(d, p);
#pragma unroll
  for (int i = 0; i < 8; i++) d[i] = coa_sha::uni(d[i]);
}
COA_DEV uint64_t uni64(uint64_t v) {
  return ((uint64_t)coa_sha::uni((uint32_t)(v >> 32)) << 32) | coa_sha::uni((uint32_t)v);
}

// The load kind of a helper below: per lane, or wave-uniform (every lane reads
// the same address and the values land in SGPRs, which keeps the latency
// kernels' control flow on the scalar unit).
constexpr bool kLane = false, kUniform = true;
template <bool UNI>
COA_DEV void load8k(uint32_t* d, const uint32_t* p) {
  if constexpr (UNI) load8u(d, p);
  else load8(d, p);
}

// p or q as a plain integer select (a ternary over two kernel-argument
// pointers is lowered through a private two-entry array, i.e. scratch)
COA_DEV const uint32_t* sel_ptr(bool c, const uint32_t* p, const uint32_t* q) {
  return reinterpret_cast<const uint32_t*>(c ? reinterpret_cast<uintptr_t>(p) : reinterpret_cast<uintptr_t>(q));
}

// Lexicographic compare of two 8-dword tuples (the registration sort order).
COA_DEV int cmp8(const uint32_t* a, const uint32_t* b) {
  int r = 0;
#pragma unroll
  for (int i = 7; i >= 0; i--) r = a[i] != b[i] ? (a[i] < b[i] ? -1 : 1) : r;
  return r;
}

// slot of pk among the nk registered keys, < 0: not registered
template <bool UNI>
COA_DEV int key_lookup(const uint32_t* __restrict__ keys, uint32_t nk, const uint32_t* pk) {
  int lo = 0, hi = (int)nk - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    uint32_t k[8];
    load8k<UNI>(k, keys + (uint64_t)mid * 8);
    const int c = cmp8(k, pk);
    if (c == 0) return mid;
    if (c < 0) lo = mid + 1;
    else hi = mid - 1;
  }
  return -1;
}

// certificate owning vote vi: the last c with voff[c] <= vi
template <bool UNI>
COA_DEV uint32_t vote_cert(const uint64_t* __restrict__ voff, uint32_t nc, uint32_t vi) {
  uint32_t lo = 0, hi = nc;  // voff[lo] <= vi < voff[hi]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if ((UNI ? uni64(voff[mid]) : voff[mid]) <= vi) lo = mid;
    else hi = mid;
  }
  return lo;
}

// k = SHA-512(R || A || M) mod l
COA_DEV void challenge(sc& k, const uint32_t* rw, const uint32_t* pk, const uint32_t* msg) {
  uint64_t st[8];
  uint32_t h[16];
  {
    uint32_t in[24];
#pragma unroll
    for (int i = 0; i < 8; i++) {
      in[i] = rw[i];
      in[8 + i] = pk[i];
      in[16 + i] = msg[i];
    }
    coa_sha::hash_words<24>(st, in);
    coa_sha::state_to_le_words(h, st);
  }
  sc_reduce512(k, h);
}

// msg <- SHA-512(msg || round u64 LE || origin)[..32]: Certificate::digest
// (messages.rs:226-234) and Vote::digest (messages.rs:145-153); origin as 8
// loaded words
COA_DEV void round_origin_digest(uint32_t* msg, uint64_t rd, const uint32_t* origin) {
  uint64_t st[8];
  uint32_t h[16], in[18];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    in[i] = msg[i];
    in[10 + i] = origin[i];
  }
  in[8] = (uint32_t)rd;
  in[9] = (uint32_t)(rd >> 32);
  coa_sha::hash_words<18>(st, in);
  coa_sha::state_to_le_words(h, st);
#pragma unroll
  for (int i = 0; i < 8; i++) msg[i] = h[i];
}

// SHA-512 state st: its first 32 bytes are the header id at `id`
template <bool UNI>
COA_DEV bool id_matches(const uint64_t* st, const uint32_t* id) {
  uint32_t h[16], w[8];
  coa_sha::state_to_le_words(h, st);
  load8k<UNI>(w, id);
  bool same = true;
#pragma unroll
  for (int i = 0; i < 8; i++) same = same && h[i] == w[i];
  return same;
}

template <int L>
COA_DEV void shfl_fe(fe& r, const fe& a, int off) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = (uint32_t)__shfl_xor((int)a.v[i], off, 64);
}

}  // namespace coa_kc

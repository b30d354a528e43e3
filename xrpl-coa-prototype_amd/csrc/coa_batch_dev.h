// Device bodies of the batch (random-linear-combination) check, shared by the
// kernels of coa_batch.hip (host-sized launches over a call's votes) and
// coa_resolve.hip (the same check over the open certificates' votes, found and
// counted on the device): the weight block of k_batch_z, the per-vote term of
// k_batch_terms and the per-group sum of k_batch_reduce.  One definition each;
// the kernels differ only in where a vote's bytes and its slot come from.
//
// The term (256 VGPRs, the budget of its launch bounds, no spills) spilled 7
// dwords with the trimmed first and last comba columns of coa_fe.h: every file
// that includes this header keeps the uniform columns, so it must come before
// any other include of coa_fe.h.
#pragma once
#define COA_COMBA_ALL_CARRIES
#include "coa_batch.h"
#include "coa_kernels.h"
#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_sc.h"
#include "coa_sha512.h"

#define BATCH_BLOCK 256

namespace coa_batch {

static_assert(!COA_COMBA_TRIM, "coa_batch_dev.h must be included before coa_fe.h");

// per-lane tables j·P (j = 1..8) for two bases, cached form, lane-major
// (2 KiB per lane; one 128-byte line per lookup, as in coa_kernels.hip):
//   uint4 index = ((lane * 16 + tab * 8 + entry) * 8 + quad)
COA_DEV void tab_store(uint32_t* scr, uint32_t lanes, uint32_t lane, int tab, int entry, const ge_cached& q) {
  const fe* f[4] = {&q.YplusX, &q.YminusX, &q.Z, &q.T2d};
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      uint4* dst = reinterpret_cast<uint4*>(scr) + (((uint64_t)lane * 16 + tab * 8 + entry) * 8 + c * 2 + h);
      *dst = make_uint4(f[c]->v[4 * h], f[c]->v[4 * h + 1], f[c]->v[4 * h + 2], f[c]->v[4 * h + 3]);
    }
}

COA_DEV void tab_select(ge_cached& q, const uint32_t* scr, uint32_t lanes, uint32_t lane, int tab, int d) {
  const int m = d < 0 ? -d : d;
  const int entry = m == 0 ? 0 : m - 1;
  fe* f[4] = {&q.YplusX, &q.YminusX, &q.Z, &q.T2d};
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint4 v =
          reinterpret_cast<const uint4*>(scr)[((uint64_t)lane * 16 + tab * 8 + entry) * 8 + c * 2 + h];
      f[c]->v[4 * h] = v.x;
      f[c]->v[4 * h + 1] = v.y;
      f[c]->v[4 * h + 2] = v.z;
      f[c]->v[4 * h + 3] = v.w;
    }
  if (m == 0) ge_cached_identity(q);
  ge_cached_cneg(q, d < 0);
}

COA_DEV void build_tab(uint32_t* scr, uint32_t lanes, uint32_t lane, int tab, const ge_p3& P) {
  ge_cached c1;
  ge_p3_to_cached(c1, P);
  tab_store(scr, lanes, lane, tab, 0, c1);
  ge_p3 cur = P;
#pragma unroll 1
  for (int j = 1; j < 8; j++) {
    ge_p1p1 t;
    ge_add(t, cur, c1);
    ge_p1p1_to_p3(cur, t);
    ge_cached cj;
    ge_p3_to_cached(cj, cur);
    tab_store(scr, lanes, lane, tab, j, cj);
  }
}

COA_DEV void add_const8(uint32_t* x, uint32_t c) {
  uint32_t cy = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) x[i] = addc32(x[i], c, cy, cy);
}
COA_DEV uint32_t top_byte(uint32_t* x) {
  const uint32_t top = x[7] >> 24;
#pragma unroll
  for (int i = 7; i > 0; i--) x[i] = (x[i] << 8) | (x[i - 1] >> 24);
  x[0] <<= 8;
  return top;
}

// Signed radix-256 digit e -> ±|e|·B from the LDS table (identity for 0).
COA_DEV void btab_niels(ge_niels& q, const uint32_t* lds, int e) {
  const int m = e < 0 ? -e : e;
  const int idx = m == 0 ? 0 : m - 1;
  const uint4* src = reinterpret_cast<const uint4*>(lds + idx * 24);
  uint32_t w[24];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const uint4 v = src[i];
    w[4 * i] = v.x;
    w[4 * i + 1] = v.y;
    w[4 * i + 2] = v.z;
    w[4 * i + 3] = v.w;
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    q.yplusx.v[i] = w[i];
    q.yminusx.v[i] = w[8 + i];
    q.xy2d.v[i] = w[16 + i];
  }
  if (m == 0) ge_niels_identity(q);
  ge_niels_cneg(q, e < 0);
}

COA_DEV uint32_t top_nibble(uint32_t* x) {
  const uint32_t top = x[7] >> 28;
#pragma unroll
  for (int i = 7; i > 0; i--) x[i] = (x[i] << 4) | (x[i - 1] >> 28);
  x[0] <<= 4;
  return top;
}

// The fixed-base table of B into a block's LDS (COA_BTAB_DWORDS words).
COA_DEV void btab_load(uint32_t* btab, const uint32_t* __restrict__ btab_g) {
  for (int t = threadIdx.x; t < COA_BTAB_DWORDS / 4; t += blockDim.x)
    reinterpret_cast<uint4*>(btab)[t] = reinterpret_cast<const uint4*>(btab_g)[t];
  __syncthreads();
}

// z = SHA-512("coa-batch-z" || seed || group || i || h || s)[0..16): the weight
// of vote i of group `group`; h its challenge (8 words), s the second half of
// its signature (8 words).
COA_DEV void z_derive(uint32_t* z4, uint64_t seed, uint32_t group, uint32_t i, const uint32_t* hw,
                      const uint32_t* sw) {
  // one block: "coa-batch-z"(11) pad to 16 | seed 8 | group 4 | i 4 | h 32 | s 32 = 96 bytes
  uint32_t m[24];
  m[0] = 0x2d616f63u;  // "coa-"
  m[1] = 0x63746162u;  // "batc"
  m[2] = 0x007a2d68u;  // "h-z\0"
  m[3] = 0;
  m[4] = (uint32_t)seed;
  m[5] = (uint32_t)(seed >> 32);
  m[6] = group;
  m[7] = i;
#pragma unroll
  for (int j = 0; j < 8; j++) m[8 + j] = hw[j];
#pragma unroll
  for (int j = 0; j < 8; j++) m[16 + j] = sw[j];
  uint64_t W[16];
#pragma unroll
  for (int w = 0; w < 12; w++) W[w] = coa_sha::be64(m[2 * w], m[2 * w + 1]);
  W[12] = 0x8000000000000000ull;
  W[13] = 0;
  W[14] = 0;
  W[15] = 96 * 8;
  uint64_t st[8];
  coa_sha::init(st);
  coa_sha::compress(st, W);
  uint32_t h[16];
  coa_sha::state_to_le_words(h, st);
#pragma unroll
  for (int j = 0; j < 4; j++) z4[j] = h[j];
}

// One vote: flag (1 = valid encoding) and P = [z]R + [z·h mod l]A +
// [-(z·s) mod l]B.  The vote's key and signature are entry `src` of pks and
// sigs; its challenge, weight, term (X, Y, Z, T: 32 words) and flag are entry
// `slot` of kbuf, zs, terms and flags.
// `lane` of `lanes` owns 2 KiB of scr; btab is the block's LDS table of B.
COA_DEV void term(const uint8_t* pks, const uint8_t* sigs, uint32_t src, const uint32_t* kbuf, const uint32_t* zs,
                  uint32_t slot, uint32_t* terms, uint8_t* flags, uint32_t* scr, uint32_t lanes, uint32_t lane,
                  const uint32_t* btab) {
  uint32_t aw[8], rw[8], sw[8], hw[8], z[8];
  const uint32_t* pk = reinterpret_cast<const uint32_t*>(pks + (uint64_t)src * 32);
  const uint32_t* sg = reinterpret_cast<const uint32_t*>(sigs + (uint64_t)src * 64);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    aw[j] = pk[j];
    rw[j] = sg[j];
    sw[j] = sg[8 + j];
    hw[j] = kbuf[(uint64_t)slot * 8 + j];
    z[j] = j < 4 ? zs[(uint64_t)slot * 4 + j] : 0;
  }
  bool ok = ((sw[7] & 0xe0000000u) == 0) && sc_is_canonical(sw);
  ge_p3 A, R;
#pragma unroll 1
  for (int which = 0; which < 2; which++) {
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = which ? rw[j] : aw[j];
    ge_p3 P;
    ok = ge_decompress(P, w) && ok;
    if (which == 0) A = P;
    else R = P;
  }
  sc c, wz, nw;
  sc_mul(c, z, hw);   // z·h mod l
  sc_mul(wz, z, sw);  // z·s mod l
  sc_neg(nw, wz.v);   // -(z·s) mod l
  ge_p3 acc3;
  ge_p3_identity(acc3);
  if (ok) {
    build_tab(scr, lanes, lane, 0, R);
    build_tab(scr, lanes, lane, 1, A);
    uint32_t zp[8], cp[8], bp[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
      zp[j] = z[j];
      cp[j] = c.v[j];
      bp[j] = nw.v[j];
    }
    add_const8(zp, 0x88888888u);
    add_const8(cp, 0x88888888u);
    add_const8(bp, 0x80808080u);
    ge_p2 acc2;
    ge_p1p1 t;
#pragma unroll 1
    for (int d = 63; d >= 0; d--) {
      if (d != 63) {
#pragma unroll 1
        for (int dd = 0; dd < 3; dd++) {
          ge_p2_dbl(t, acc2);
          ge_p1p1_to_p2(acc2, t);
        }
        ge_p2_dbl(t, acc2);
        ge_p1p1_to_p3(acc3, t);
      }
      ge_cached q;
      tab_select(q, scr, lanes, lane, 0, (int)top_nibble(zp) - 8);
      ge_add(t, acc3, q);
      ge_p1p1_to_p3(acc3, t);
      tab_select(q, scr, lanes, lane, 1, (int)top_nibble(cp) - 8);
      ge_add(t, acc3, q);
      if ((d & 1) == 0) {
        const int e = (int)top_byte(bp) - 128;
        ge_niels qb;
        btab_niels(qb, btab, e);
        ge_p1p1_to_p3(acc3, t);
        ge_madd(t, acc3, qb);
      }
      if (d == 0) ge_p1p1_to_p3(acc3, t);
      else ge_p1p1_to_p2(acc2, t);
    }
  }
  // terms: X,Y,Z,T (32 dwords) per vote
  uint4* o = reinterpret_cast<uint4*>(terms + (uint64_t)slot * 32);
  const fe* f[4] = {&acc3.X, &acc3.Y, &acc3.Z, &acc3.T};
#pragma unroll
  for (int q = 0; q < 4; q++) {
    o[2 * q] = make_uint4(f[q]->v[0], f[q]->v[1], f[q]->v[2], f[q]->v[3]);
    o[2 * q + 1] = make_uint4(f[q]->v[4], f[q]->v[5], f[q]->v[6], f[q]->v[7]);
  }
  flags[slot] = ok ? 1 : 0;
}

COA_DEV void load_p3(ge_p3& p, const uint32_t* src) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    p.X.v[j] = src[j];
    p.Y.v[j] = src[8 + j];
    p.Z.v[j] = src[16 + j];
    p.T.v[j] = src[24 + j];
  }
}
COA_DEV void store_p3(uint32_t* dst, const ge_p3& p) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    dst[j] = p.X.v[j];
    dst[8 + j] = p.Y.v[j];
    dst[16 + j] = p.Z.v[j];
    dst[24 + j] = p.T.v[j];
  }
}

// One workgroup of BATCH_BLOCK lanes: the sum of terms [lo, hi), its identity
// test and the AND of their flags.  pts (BATCH_BLOCK * 32 words) and *bad are
// the block's LDS; the answer (true = Ok) is thread 0's.
COA_DEV bool group_ok(uint64_t lo, uint64_t hi, const uint32_t* __restrict__ terms,
                      const uint8_t* __restrict__ flags, uint32_t* pts, int* bad) {
  const int tid = threadIdx.x;
  if (tid == 0) *bad = 0;
  __syncthreads();
  ge_p3 acc;
  ge_p3_identity(acc);
  int mybad = 0;
  for (uint64_t i = lo + tid; i < hi; i += BATCH_BLOCK) {
    if (!flags[i]) mybad = 1;
    ge_p3 p;
    load_p3(p, terms + i * 32);
    ge_cached c;
    ge_p3_to_cached(c, p);
    ge_p1p1 t;
    ge_add(t, acc, c);
    ge_p1p1_to_p3(acc, t);
  }
  if (mybad) atomicOr(bad, 1);
  store_p3(pts + tid * 32, acc);
  __syncthreads();
  for (int half = BATCH_BLOCK / 2; half > 0; half >>= 1) {
    if (tid < half) {
      ge_p3 a, b;
      load_p3(a, pts + tid * 32);
      load_p3(b, pts + (tid + half) * 32);
      ge_cached c;
      ge_p3_to_cached(c, b);
      ge_p1p1 t;
      ge_add(t, a, c);
      ge_p1p1_to_p3(a, t);
      store_p3(pts + tid * 32, a);
    }
    __syncthreads();
  }
  if (tid != 0) return false;
  ge_p2 r;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    r.X.v[j] = pts[j];
    r.Y.v[j] = pts[8 + j];
    r.Z.v[j] = pts[16 + j];
  }
  return ge_p2_is_identity(r) && !*bad;
}

}  // namespace coa_batch

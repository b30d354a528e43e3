// Device helpers of the halved verification kernels (coa_halved.hip), each
// written once: 8-word vector moves, a cached point as 32 dwords (global
// memory, registers, LDS columns), the plain / interleaved point formulas
// behind one template parameter, the Horner digit step, the [e]B comb sums,
// the verdict, and the comb builders' two ends.  k_verify_main, the
// k_verify_halved instances and the comb builders are written in terms of
// them.  k_pre_halve, k_verify_main2 and k_verify_main_sums use only the
// 8-word moves: with any of the other helpers the compiler assigns their
// registers differently, and those two-wave kernels then run measurably
// slower ("One copy of each shared step").
#pragma once
#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_sc.h"
#include "coa_smul.h"

COA_DEV int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
  return v;
}

// ------------------------------------------------ 8 words as two uint4 moves
COA_DEV void load8_u4(uint32_t* dst, const void* src) {
  const uint4* q = reinterpret_cast<const uint4*>(src);
  const uint4 a = q[0], b = q[1];
  dst[0] = a.x; dst[1] = a.y; dst[2] = a.z; dst[3] = a.w;
  dst[4] = b.x; dst[5] = b.y; dst[6] = b.z; dst[7] = b.w;
}
COA_DEV void store8_u4(void* dst, const uint32_t* w) {
  uint4* q = reinterpret_cast<uint4*>(dst);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// ------------------------------------------- a cached point as 32 dwords
// Dword k of (Y+X, Y-X, Z, 2dT), eight words each; C is ge_cached or const
// ge_cached.  k is a constant after unrolling, so this is a register name.
template <class C>
COA_DEV auto& cached_word(C& c, int k) {
  decltype(&c.Z) f[4] = {&c.YplusX, &c.YminusX, &c.Z, &c.T2d};
  return f[k >> 3]->v[k & 7];
}
// global memory (16-byte aligned)
COA_DEV void cached_load(ge_cached& c, const uint32_t* src) {
#pragma unroll
  for (int q = 0; q < 4; q++) load8_u4(&cached_word(c, 8 * q), src + 8 * q);
}
COA_DEV void cached_store(uint32_t* dst, const ge_cached& c) {
#pragma unroll
  for (int q = 0; q < 4; q++) store8_u4(dst + 8 * q, &cached_word(c, 8 * q));
}
// a register array
COA_DEV void cached_from_words(ge_cached& c, const uint32_t* w) {
#pragma unroll
  for (int k = 0; k < 32; k++) cached_word(c, k) = w[k];
}
// an LDS column lds[dword][item] of N items
template <int N>
COA_DEV void cached_put_lds(uint32_t (*lds)[N], uint32_t item, const ge_cached& c) {
#pragma unroll
  for (int k = 0; k < 32; k++) lds[k][item] = cached_word(c, k);
}
template <int N>
COA_DEV void cached_get_lds(ge_cached& c, const uint32_t (*lds)[N], uint32_t item) {
#pragma unroll
  for (int k = 0; k < 32; k++) cached_word(c, k) = lds[k][item];
}

// ------------- the point formulas of coa_ge.h, plain or interleaved (*_il)
template <bool IL>
COA_DEV void p2_dbl(ge_p1p1& r, const ge_p2& p) {
  if constexpr (IL) ge_p2_dbl_il(r, p);
  else ge_p2_dbl(r, p);
}
template <bool IL>
COA_DEV void to_p2(ge_p2& r, const ge_p1p1& p) {
  if constexpr (IL) ge_p1p1_to_p2_il(r, p);
  else ge_p1p1_to_p2(r, p);
}
template <bool IL>
COA_DEV void to_p3(ge_p3& r, const ge_p1p1& p) {
  if constexpr (IL) ge_p1p1_to_p3_il(r, p);
  else ge_p1p1_to_p3(r, p);
}
template <bool IL>
COA_DEV void add(ge_p1p1& r, const ge_p3& p, const ge_cached& q, bool t2d_neg = false) {
  if constexpr (IL) ge_add_il(r, p, q, t2d_neg);
  else ge_add(r, p, q, t2d_neg);
}

// ----------------------------------------------------- the Horner digit step
// acc3 = 16 * acc2: the four doublings of one radix-16 digit, three to p2
// and the last to p3 (t is left holding the last doubling).  go: false for
// the first digit, whose accumulator is still the identity; the test is in
// here and not around the call because the call site's form decides how the
// compiler lays the loop out (tools/digit_count.py shows the difference).
template <bool IL>
COA_DEV void horner_x16(ge_p3& acc3, ge_p2& acc2, ge_p1p1& t, bool go) {
  if (!go) return;
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    p2_dbl<IL>(t, acc2);
    to_p2<IL>(acc2, t);
  }
  p2_dbl<IL>(t, acc2);
  to_p3<IL>(acc3, t);
}
// Signed radix-16 digit pos of a record word (the word that holds nibble pos
// of c' or d', halve_rec): the nibble minus 8.
COA_DEV int digit_of(uint32_t w, int pos) { return (int)((w >> (4 * (pos & 7))) & 15u) - 8; }

// ----------------------------------------------------------------- acc += [e]B
// By the doubling-free radix-256 comb: 32 mixed additions (e is consumed; t
// is the caller's scratch point, as in horner_x16).
COA_DEV void comb_accumulate(ge_p3& acc, ge_p1p1& t, uint32_t* e, const uint32_t* comb) {
  add_const_word(e, 0x80808080u);
#pragma unroll 1
  for (int j = 0; j < 32; j++) {
    const int ej = (int)take_low_byte(e) - 128;
    ge_niels qb;
    comb_select(qb, comb, j, ej);
    ge_madd(t, acc, qb);
    ge_p1p1_to_p3(acc, t);
  }
}
// From the wide HBM comb if there is one (COA_WCOMB_POS mixed additions,
// interleaved for IL), else from the narrow one.
template <bool IL>
COA_DEV void eb_accumulate(ge_p3& acc, ge_p1p1& t, uint32_t* e, const uint32_t* comb, const uint32_t* wcomb) {
  if (wcomb) wcomb_accumulate<IL>(acc, e, wcomb);
  else comb_accumulate(acc, t, e, comb);
}

// -------------------------------------------------------------------- verdict
// 0 (accept) iff the check sum Q is the identity.
COA_DEV uint8_t verdict_of(const ge_p3& acc3) {
  ge_p2 q2;
  ge_p3_to_p2(q2, acc3);
  return ge_p2_is_identity(q2) ? 0 : 1;
}

// ------------------------------------------------------- the comb builders
// x = (m << bitpos) mod l for a small multiple m (the shifted value has up to
// 512 bits).
COA_DEV void sc_small_shifted(sc& x, uint32_t m, int bitpos) {
  uint32_t wide[16];
#pragma unroll
  for (int i = 0; i < 16; i++) wide[i] = 0;
  const uint64_t mm = (uint64_t)m << (bitpos & 31);
  for (int i = 0; i < 16; i++) {
    if (i == (bitpos >> 5)) wide[i] = (uint32_t)mm;
    if (i == (bitpos >> 5) + 1) wide[i] = (uint32_t)(mm >> 32);
  }
  sc_reduce512(x, wide);
}
// Projective (X, Y, Z) -> affine Niels (y + x, y - x, 2d x y), canonical.
COA_DEV void affine_niels_canon(fe& n0, fe& n1, fe& n2, const fe& X, const fe& Y, const fe& Z) {
  fe zi, xx, yy, xy, d2;
  fe_invert(zi, Z);
  fe_mul(xx, X, zi);
  fe_mul(yy, Y, zi);
  fe_mul(xy, xx, yy);
  fe_const_d2(d2);
  fe_add(n0, yy, xx);
  fe_sub(n1, yy, xx);
  fe_mul(n2, xy, d2);
  fe_canon(n0, n0);
  fe_canon(n1, n1);
  fe_canon(n2, n2);
}

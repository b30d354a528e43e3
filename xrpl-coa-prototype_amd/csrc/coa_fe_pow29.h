// z^((p-5)/8) on nine carry-free 29-bit limbs, for the decompression roles of
// k_pre_halve (coa_ge_dec29.h).  The chain is 251 dependent squarings and 11
// multiplications with no addition between them, so the one drawback of an
// unsaturated radix (additions that have to renormalise) never comes up,
// while every product term is a bare v_mad_u64_u32: a column of at most nine
// 58-bit products cannot overflow its 64-bit accumulator, and the
// v_addc_co_u32 that coa_fe.h pays per term is gone.
//
// Representation (fe29): value = sum v[i] 2^(29 i), i = 0..8 (261 bits),
// congruent to the element mod p.  Limb bounds, in and out of sq29 / mul29:
//     v[1] <= 2^29 + 2^17,   every other v[i] <= 2^29 - 1.
// (from_fe gives v[i] < 2^29 and v[8] < 2^24.)
//
// Product scanning with ONE live accumulator.  The high columns 9..16 run
// first and are carried into limbs h[0..7]; what is left of the accumulator
// after column 16 is h[8] (column 17).  Since 2^261 = 2^6 2^255 == 64 * 19 =
// 1216 (mod p), h[j] then enters low column j as one more term h[j] * 1216,
// and the carry out of low column 8 (again of weight 2^261) goes to limb 0
// the same way.  A squaring doubles its operand once and takes the 36 cross
// terms from the doubled limbs: 45 + 9 mads; a product takes 81 + 9.
//
// Bounds (tests/test_pow29_host.py asserts them by interval arithmetic on
// exactly these steps).  With B = 2^29 + 2^17 for limb 1 and 2^29 - 1 for
// the others:
//  * doubled limbs 2 v[i] < 2^31 fit a dword;
//  * a column holds at most nine products, each < 2^58.001: < 2^61.2;
//  * the carry into a column is the column before it shifted down by 29 bits,
//    < 2^32.2, and the fold term h[j] * 1216 is < 2^39.3 (h[8] < 2^29.01 is
//    the carry out of column 16, which holds one product): every column sum
//    stays below 2^61.2 < 2^64;
//  * the carry out of low column 8 is c < 2^32.2, which needs 33 bits:
//    c * 1216 is formed from its two dwords and added to limb 0, < 2^42.5;
//    limb 0 keeps the low 29 bits and limb 1 takes the rest, < 2^13.5, which
//    keeps it well inside its 2^29 + 2^17 bound.
//
// coa_fe.h, coa_ge.h and coa_smul.h are untouched: every other kernel keeps
// the radix-2^32 field.
#pragma once
#include "coa_fe.h"

struct fe29 {
  uint32_t v[9];
};

constexpr uint32_t COA_M29 = 0x1fffffffu;
constexpr uint32_t COA_W261 = 1216u;  // 2^261 mod p

COA_DEV uint64_t mad29(uint32_t a, uint32_t b, uint64_t c) { return (uint64_t)a * b + c; }

// Low 29 bits of the accumulator as a limb; the accumulator moves down by 29
// bits.  hipcc emits one v_lshrrev_b64 for the shift (and folds the pair
// v_alignbit_b32 + v_lshrrev_b32 back into it when written out): one issue
// slot instead of two, and at 4.2 cycles against 2 x 2.5 no dearer in
// throughput (issue costs).
COA_DEV uint32_t take29(uint64_t& acc) {
  const uint32_t limb = (uint32_t)acc & COA_M29;
  acc >>= 29;
  return limb;
}

// acc += sum_p x[p] * y[p], one asm statement per column.  Written in C++
// the sums are reassociated: hipcc starts every column from zero and joins
// it to the shifted accumulator with 64-bit adds, two more slow-rate
// instructions per column.  The carry-out that v_mad_u64_u32 must name goes
// to VCC and is never read.
#define COA_MAD29(X, Y) "v_mad_u64_u32 %0, vcc, %" #X ", %" #Y ", %0\n\t"
#define COA_XY(p) "v"(x[p]), "v"(y[p])
template <int P>
COA_DEV void madcol29(uint64_t& acc, const uint32_t* x, const uint32_t* y) {
  static_assert(P >= 1 && P <= 10, "column width");
  if constexpr (P == 1) {
    asm(COA_MAD29(1, 2) : "+v"(acc) : COA_XY(0) : "vcc");
  } else if constexpr (P == 2) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) : "+v"(acc) : COA_XY(0), COA_XY(1) : "vcc");
  } else if constexpr (P == 3) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) : "+v"(acc) : COA_XY(0), COA_XY(1), COA_XY(2) : "vcc");
  } else if constexpr (P == 4) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8)
        : "+v"(acc) : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3) : "vcc");
  } else if constexpr (P == 5) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8) COA_MAD29(9, 10)
        : "+v"(acc) : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3), COA_XY(4) : "vcc");
  } else if constexpr (P == 6) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8) COA_MAD29(9, 10) COA_MAD29(11, 12)
        : "+v"(acc) : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3), COA_XY(4), COA_XY(5) : "vcc");
  } else if constexpr (P == 7) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8) COA_MAD29(9, 10) COA_MAD29(11, 12)
            COA_MAD29(13, 14)
        : "+v"(acc) : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3), COA_XY(4), COA_XY(5), COA_XY(6) : "vcc");
  } else if constexpr (P == 8) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8) COA_MAD29(9, 10) COA_MAD29(11, 12)
            COA_MAD29(13, 14) COA_MAD29(15, 16)
        : "+v"(acc)
        : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3), COA_XY(4), COA_XY(5), COA_XY(6), COA_XY(7) : "vcc");
  } else if constexpr (P == 9) {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8) COA_MAD29(9, 10) COA_MAD29(11, 12)
            COA_MAD29(13, 14) COA_MAD29(15, 16) COA_MAD29(17, 18)
        : "+v"(acc)
        : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3), COA_XY(4), COA_XY(5), COA_XY(6), COA_XY(7), COA_XY(8) : "vcc");
  } else {
    asm(COA_MAD29(1, 2) COA_MAD29(3, 4) COA_MAD29(5, 6) COA_MAD29(7, 8) COA_MAD29(9, 10) COA_MAD29(11, 12)
            COA_MAD29(13, 14) COA_MAD29(15, 16) COA_MAD29(17, 18) COA_MAD29(19, 20)
        : "+v"(acc)
        : COA_XY(0), COA_XY(1), COA_XY(2), COA_XY(3), COA_XY(4), COA_XY(5), COA_XY(6), COA_XY(7), COA_XY(8),
          COA_XY(9) : "vcc");
  }
}
#undef COA_XY

// Terms of column K: all pairs i + j = K of a * b, or for a squaring the
// cross pairs i < j once (from the doubled limbs a2) and the square on even
// columns; a low column also takes its fold term h * 1216.
template <bool SQ>
constexpr int col29_terms(int k) {
  const int lo = k < 9 ? 0 : k - 8, hi = k < 9 ? k : 8;
  return (SQ ? (hi - lo + 2) / 2 : hi - lo + 1) + (k < 9 ? 1 : 0);
}

template <bool SQ, int K>
COA_DEV void col29(uint64_t& acc, const uint32_t* a, const uint32_t* a2, const uint32_t* b, uint32_t h) {
  constexpr int P = col29_terms<SQ>(K);
  uint32_t x[P], y[P];
  int p = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int j = K - i;
    if (j < 0 || j > 8 || (SQ && i > j)) continue;
    x[p] = SQ && i < j ? a2[i] : a[i];
    y[p++] = SQ ? a[j] : b[j];
  }
  if (K < 9) {
    x[p] = h;
    y[p++] = COA_W261;
  }
  if constexpr (K == 0 || K == 9) {  // first column of its half: the accumulator starts as a bare product
    acc = mad29(x[0], y[0], 0);
    if constexpr (P > 1) madcol29<P - 1>(acc, x + 1, y + 1);
  } else {
    madcol29<P>(acc, x, y);
  }
}

template <bool SQ, int K = 9>
COA_DEV void cols29_high(uint32_t* h, uint64_t& acc, const uint32_t* a, const uint32_t* a2, const uint32_t* b) {
  if constexpr (K < 17) {
    col29<SQ, K>(acc, a, a2, b, 0);
    h[K - 9] = take29(acc);
    cols29_high<SQ, K + 1>(h, acc, a, a2, b);
  }
}
template <bool SQ, int K = 0>
COA_DEV void cols29_low(uint32_t* o, uint64_t& acc, const uint32_t* a, const uint32_t* a2, const uint32_t* b,
                        const uint32_t* h) {
  if constexpr (K < 9) {
    col29<SQ, K>(acc, a, a2, b, h[K]);
    o[K] = take29(acc);
    cols29_low<SQ, K + 1>(o, acc, a, a2, b, h);
  }
}

template <bool SQ>
COA_DEV void prod29(fe29& r, const fe29& a, const fe29& b) {
  uint32_t a2[9], h[9], o[9];
#pragma unroll
  for (int i = 0; i < 9; i++) a2[i] = SQ ? a.v[i] << 1 : 0;
  uint64_t acc;
  cols29_high<SQ>(h, acc, a.v, a2, b.v);
  h[8] = (uint32_t)acc;  // column 17: < 2^32
  cols29_low<SQ>(o, acc, a.v, a2, b.v, h);
  // acc (33 bits) has weight 2^261: limb 0 takes acc * 1216, formed from the two dwords of acc
  const uint64_t t = mad29((uint32_t)acc, COA_W261, o[0]);
  const uint32_t thi = (uint32_t)(t >> 32) + (uint32_t)(acc >> 32) * COA_W261;
  o[0] = (uint32_t)t & COA_M29;
  o[1] += __builtin_amdgcn_alignbit(thi, (uint32_t)t, 29);
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = o[i];
}

COA_DEV void fe29_sq(fe29& r, const fe29& a) { prod29<true>(r, a, a); }
COA_DEV void fe29_mul(fe29& r, const fe29& a, const fe29& b) { prod29<false>(r, a, b); }

// r = a^(2^n), n >= 1.  Two squarings per trip, so the loop-carried element
// stays in its registers and no trip ends with a nine-dword copy.
COA_DEV void fe29_sqn(fe29& r, const fe29& a, int n) {
  fe29 t;
  if (n & 1) {
    fe29_sq(r, a);
  } else {
    fe29_sq(t, a);
    fe29_sq(r, t);
  }
#pragma unroll 1
  for (int i = (n - 1) >> 1; i > 0; i--) {
    fe29_sq(t, r);
    fe29_sq(r, t);
  }
}

// Eight dwords (a value < 2^256) to limbs: shifts and masks.
COA_DEV void fe29_from_fe(fe29& r, const fe& a) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const int w = (29 * i) / 32, s = (29 * i) % 32;
    const uint32_t x = s == 0  ? a.v[w]
                       : w < 7 ? __builtin_amdgcn_alignbit(a.v[w + 1], a.v[w], s)
                               : a.v[w] >> s;
    r.v[i] = x & COA_M29;
  }
}

// Limbs to the usual element in [0, 2^256): the limbs are summed at their
// offsets (limb 1 may hold 30 bits, so this is an addition, not a bit
// packing), and the five bits above 2^256 are folded as 38.
COA_DEV void fe29_to_fe(fe& r, const fe29& a) {
  uint64_t acc = 0;
  int bits = 0, j = 0;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    acc += (uint64_t)a.v[i] << bits;
    bits += 29;
    if (bits >= 32) {
      r.v[j++] = (uint32_t)acc;
      acc >>= 32;
      bits -= 32;
    }
  }
  fe_fold_word(r, (uint32_t)acc * 38u);  // acc < 2^6
}

// curve25519-dalek FieldElement::pow_p58's addition chain (fe_pow_p58 of
// coa_fe.h) on fe29: the same field element, as a weakly reduced fe.
COA_DEV void fe_pow_p58_29(fe& r, const fe& z8) {
  fe29 z, z2, t, z9, z11, z_5_0, z_10_0, z_20_0, z_40_0, z_50_0, z_100_0;
  fe29_from_fe(z, z8);
  fe29_sq(z2, z);                 // z^2
  fe29_sqn(t, z2, 2);             // z^8
  fe29_mul(z9, t, z);             // z^9
  fe29_mul(z11, z9, z2);          // z^11
  fe29_sq(t, z11);                // z^22
  fe29_mul(z_5_0, t, z9);         // z^(2^5-1)
  fe29_sqn(t, z_5_0, 5);
  fe29_mul(z_10_0, t, z_5_0);     // 2^10-1
  fe29_sqn(t, z_10_0, 10);
  fe29_mul(z_20_0, t, z_10_0);    // 2^20-1
  fe29_sqn(t, z_20_0, 20);
  fe29_mul(z_40_0, t, z_20_0);    // 2^40-1
  fe29_sqn(t, z_40_0, 10);
  fe29_mul(z_50_0, t, z_10_0);    // 2^50-1
  fe29_sqn(t, z_50_0, 50);
  fe29_mul(z_100_0, t, z_50_0);   // 2^100-1
  fe29_sqn(t, z_100_0, 100);
  fe29_mul(t, t, z_100_0);        // 2^200-1
  fe29_sqn(t, t, 50);
  fe29_mul(t, t, z_50_0);         // 2^250-1
  fe29_sqn(t, t, 2);              // 2^252-4
  fe29_mul(t, t, z);              // 2^252-3
  fe29_to_fe(r, t);
}

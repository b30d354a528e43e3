// The Horner accumulator of k_verify_main_sums (coa_halved.hip) on nine
// carry-free 29-bit limbs: coa_fe_pow29.h's prod29 for every product, and
// additions and subtractions that are nine independent dword operations each
// with no carry chain.  The price of the unsaturated radix, renormalising
// after additions, is one parallel carry pass on two of a formula's four
// outputs; a doubling with its conversion then issues 985 instructions, 493
// of them mads and none a v_addc_co_u32, against 1,102 with 392 mads and 416
// v_addc_co_u32 on coa_fe.h's radix-2^32 field (tools/digit_count.py).
//
// coa_fe_pow29.h, coa_fe.h, coa_ge.h, coa_smul.h and coa_ge_sums.h are
// untouched: only the consumer role of k_verify_main_sums uses this file.
//
// Limb bounds.  A limb vector is in class k N when v[i] <= k * N[i], with
//     N = (2^29 + 2^14, 2^29 + 2^17, 2^29 + 2^3, ..., 2^29 + 2^3).
// N holds what a product leaves (limb 1 <= 2^29 + 2^17, the others below
// 2^29: coa_fe_pow29.h), what fe29_from_fe leaves (every limb below 2^29) and
// what fe29_carry leaves for any dwords (limb 0 <= 2^29 - 1 + 7 * 1216, the
// others <= 2^29 - 1 + 7).  tests/test_ge29_bounds_host.py proves by interval
// arithmetic over exactly the steps below that
//  * a product of a class-ka and a class-kb vector with ka * kb <= 6 keeps
//    every column below 2^64 and column 17 inside a dword, and leaves N
//    (nine terms of at most 6 * 2^58.01 are below 2^63.8; the carry out of low
//    column 8 is below 2^35, its fold 2^45.3, so limb 1 gains less than
//    2^17);
//  * a squaring of a class-2 vector does the same, and its doubled limbs,
//    at most 2^31 + 2^19, fit a dword;
//  * every limb-wise sum stays below 2^32: the largest is class 6.
// Subtraction is a + BIAS_K - b limb by limb with BIAS_K = K * 64 p =
// K * (2^261 - 1216), whose limbs are K (2^29 - 1216), K (2^29 - 1), ...:
// BIAS_2 covers a class-1 subtrahend, BIAS_3 class 2, BIAS_4 class 3, and the
// difference is in class (k_a + K).
//
// The budget of the formulas (classes; `c` marks a carry pass):
//   ge29_p2_dbl     X, Y, Z in 1.  X+Y in 2, squared.  r.Y = yy + xx in 2,
//                   r.Z = yy - xx in 3, r.X = a - r.Y in 4 -> c -> 1,
//                   r.T = 2 zz - r.Z in 6 -> c -> 1.
//   ge29_p1p1_to_*  X T = 1 * 1, Y Z <= 2 * 3, Z T <= 3 * 1, X Y <= 3 * 2.
//   ge29_add        p in 1, q in 1.  Y+X in 2, Y-X in 3, times class 1.
//                   r.Y = o0 + o1 in 2, r.X = o0 - o1 in 3, zs = 2 zz + c in 3
//                   -> c -> 1, zd = 2 zz - c in 4 -> c -> 1.
// Every output of a p1p1 -> p2 / p3 conversion is a product, class 1 and
// inside fe29_to_fe's stated input bounds.
#pragma once
#include "coa_fe_pow29.h"
#include "coa_ge.h"

COA_DEV void fe29_set(fe29& r, uint32_t x) {
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = i == 0 ? x : 0u;
}

COA_DEV void fe29_add(fe29& r, const fe29& a, const fe29& b) {
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = a.v[i] + b.v[i];
}

// Limb i of K * 64 p.
template <int K>
constexpr uint32_t fe29_bias(int i) {
  return (uint32_t)K * (i == 0 ? COA_M29 + 1u - COA_W261 : COA_M29);
}

// r = a - b (mod p) as a + BIAS_K - b; b in class K - 1 (header).
template <int K>
COA_DEV void fe29_sub(fe29& r, const fe29& a, const fe29& b) {
  static_assert(K >= 2 && K <= 4, "bias");
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = a.v[i] + fe29_bias<K>(i) - b.v[i];
}

// One parallel carry pass over any nine dwords: each limb keeps its low 29
// bits and takes what the limb below it held above them; what limb 8 held
// above them has weight 2^261 and enters limb 0 times 1216.  Leaves class 1.
COA_DEV void fe29_carry(fe29& r, const fe29& a) {
  uint32_t o[9];
  o[0] = (a.v[0] & COA_M29) + (a.v[8] >> 29) * COA_W261;
#pragma unroll
  for (int i = 1; i < 9; i++) o[i] = (a.v[i] & COA_M29) + (a.v[i - 1] >> 29);
#pragma unroll
  for (int i = 0; i < 9; i++) r.v[i] = o[i];
}

// r = c ? b : a and s = c ? a : b, limb by limb (fe_cswap_to of coa_ge.h).
COA_DEV void fe29_cswap_to(fe29& r, fe29& s, const fe29& a, const fe29& b, bool c) {
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const uint32_t x = a.v[i], y = b.v[i];
    r.v[i] = c ? y : x;
    s.v[i] = c ? x : y;
  }
}

struct ge29_p2 {
  fe29 X, Y, Z;
};
struct ge29_p3 {
  fe29 X, Y, Z, T;
};
struct ge29_p1p1 {
  fe29 X, Y, Z, T;
};
struct ge29_cached {
  fe29 YplusX, YminusX, Z, T2d;
};

COA_DEV void ge29_p3_from(ge29_p3& r, const ge_p3& p) {
  fe29_from_fe(r.X, p.X);
  fe29_from_fe(r.Y, p.Y);
  fe29_from_fe(r.Z, p.Z);
  fe29_from_fe(r.T, p.T);
}
// p's coordinates are products (class 1, inside fe29_to_fe's bounds).
COA_DEV void ge29_p3_to(ge_p3& r, const ge29_p3& p) {
  fe29_to_fe(r.X, p.X);
  fe29_to_fe(r.Y, p.Y);
  fe29_to_fe(r.Z, p.Z);
  fe29_to_fe(r.T, p.T);
}
// p1p1 form of the identity, (0, 1, 1, 1).
COA_DEV void ge29_p1p1_identity(ge29_p1p1& r) {
  fe29_set(r.X, 0);
  fe29_set(r.Y, 1);
  fe29_set(r.Z, 1);
  fe29_set(r.T, 1);
}

COA_DEV void ge29_p1p1_to_p2(ge29_p2& r, const ge29_p1p1& p) {
  fe29_mul(r.X, p.X, p.T);
  fe29_mul(r.Y, p.Y, p.Z);
  fe29_mul(r.Z, p.Z, p.T);
}
COA_DEV void ge29_p1p1_to_p3(ge29_p3& r, const ge29_p1p1& p) {
  fe29_mul(r.X, p.X, p.T);
  fe29_mul(r.Y, p.Y, p.Z);
  fe29_mul(r.Z, p.Z, p.T);
  fe29_mul(r.T, p.X, p.Y);
}

// ge_p2_dbl of coa_ge.h.
COA_DEV void ge29_p2_dbl(ge29_p1p1& r, const ge29_p2& p) {
  fe29 xx, yy, zz, a, b;
  fe29_sq(xx, p.X);
  fe29_sq(yy, p.Y);
  fe29_sq(zz, p.Z);
  fe29_add(a, p.X, p.Y);
  fe29_sq(a, a);
  fe29_add(r.Y, yy, xx);
  fe29_sub<2>(r.Z, yy, xx);
  fe29_sub<3>(a, a, r.Y);
  fe29_carry(r.X, a);
  fe29_add(b, zz, zz);
  fe29_sub<4>(b, b, r.Z);
  fe29_carry(r.T, b);
}

// ge_add of coa_ge.h: p + q, q in cached form with every field in class 1;
// t2d_neg as there.
COA_DEV void ge29_add(ge29_p1p1& r, const ge29_p3& p, const ge29_cached& q, bool t2d_neg = false) {
  fe29 s, d, o0, o1, o2, o3, zs, zd;
  fe29_add(s, p.Y, p.X);
  fe29_sub<2>(d, p.Y, p.X);
  fe29_mul(o0, s, q.YplusX);
  fe29_mul(o1, d, q.YminusX);
  fe29_mul(o2, q.T2d, p.T);
  fe29_mul(o3, p.Z, q.Z);
  fe29_add(o3, o3, o3);
  fe29_add(r.Y, o0, o1);
  fe29_sub<2>(r.X, o0, o1);
  fe29_add(zs, o3, o2);
  fe29_sub<2>(zd, o3, o2);
  fe29_carry(zs, zs);
  fe29_carry(zd, zd);
  fe29_cswap_to(r.Z, r.T, zs, zd, t2d_neg);
}

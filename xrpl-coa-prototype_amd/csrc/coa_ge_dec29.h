// Point decompression for the pre roles of k_pre_halve (pre_one in
// coa_halved.hip): ge_decompress / ge_is_small_order of coa_ge.h with the
// (p-5)/8 chain on carry-free 29-bit limbs (coa_fe_pow29.h) and three
// savings that a private copy is free to take.  Every other kernel keeps
// coa_ge.h's functions.  Accepts and rejects exactly what ge_decompress and
// ge_is_small_order do; of a rejected encoding only the verdict is defined.
#pragma once
#include "coa_fe_pow29.h"
#include "coa_ge.h"

// x^2 and y^2 of the decompressed point, for ge_is_small_order_29.
struct ge_dec29_squares {
  fe xx, yy;
};

// curve25519-dalek sqrt_ratio_i(u, v) as the decompression uses it: returns
// was_nonzero_square and, when that holds, r = the non-negative root of u/v
// and rr = r^2.
//  * u v^3 and u v^7 come from w = u v as w v^2 and (w v^2) (v^2)^2: 2S + 3M
//    where v^3 = v^2 v, v^7 = (v^3)^2 v, u v^3, u v^7 take 2S + 4M.
//  * dalek also tests check == -u i and then returns r i: that root belongs
//    to i u/v, the result is "not a square", and the decompression rejects
//    the encoding whatever r holds.  The product nu i and that test are
//    dropped; r is then unspecified for a rejected encoding.
COA_DEV bool fe_sqrt_ratio_29(fe& r, fe& rr, const fe& u, const fe& v) {
  fe i, nu, w, v2, uv3, t, check, ri;
  fe_const_sqrtm1(i);
  fe_neg(nu, u);
  fe_mul(w, u, v);
  fe_sq(v2, v);
  fe_mul(uv3, w, v2);  // u v^3
  fe_sq(t, v2);        // v^4
  fe_mul(t, uv3, t);   // u v^7
  fe_pow_p58_29(t, t);  // (u v^7)^((p-5)/8)
  fe_mul(r, uv3, t);
  fe_sq(rr, r);
  fe_mul(check, rr, v);
  fe_mul(ri, r, i);
  const bool correct = fe_eq(check, u);
  const bool flipped = fe_eq(check, nu);
  fe_cmov(r, ri, flipped);  // (r i)^2 = -r^2
  fe_cneg(rr, flipped);
  fe_cneg(r, fe_isneg(r) != 0);
  return correct || flipped;
}

// ge_decompress's contract (dalek 3.x CompressedEdwardsY::decompress: y in
// [p, 2^255) and "negative zero" accepted); q receives x^2 and y^2.
COA_DEV bool ge_decompress_29(ge_p3& r, ge_dec29_squares& q, const uint32_t* w) {
  fe y, u, v, x, one, d;
  fe_from_words(y, w);
  fe_set(one, 1);
  fe_const_d(d);
  fe_sq(q.yy, y);
  fe_sub(u, q.yy, one);  // u = y^2 - 1
  fe_mul(v, q.yy, d);
  fe_add(v, v, one);     // v = d y^2 + 1
  const bool ok = fe_sqrt_ratio_29(x, q.xx, u, v);
  fe_cneg(x, (w[7] >> 31) != 0);
  r.X = x;
  r.Y = y;
  fe_set(r.Z, 1);
  fe_mul(r.T, x, y);
  return ok;
}

// ge_is_small_order for a point that ge_decompress_29 accepted (Z = 1): the
// same coordinate test, X = 0, Y = 0 or X^2 + Y^2 = 0, with the two squares
// taken from the decompression, which has computed both, instead of squared
// again.
COA_DEV bool ge_is_small_order_29(const ge_p3& p, const ge_dec29_squares& q) {
  fe s;
  fe_add(s, q.xx, q.yy);
  return fe_iszero(p.X) || fe_iszero(p.Y) || fe_iszero(s);
}

// The sum of two table entries, for k_verify_main_sums (coa_halved.hip): the
// addition of two addend-form points and the slab table in the form its second
// operand needs.  These are additions to coa_ge.h and coa_smul.h kept in a
// file of their own: the committed counter profile of the committee kernels
// (profiles/r06_c3_pmc.json) is tied to those two files by sha256, and the
// committee kernels use nothing of this.
#pragma once
#include "coa_ge.h"
#include "coa_smul.h"

// P + Q of two addend-form points: p cached (Y+X, Y-X, Z, 2dT), q the same
// with plain T in its fourth field (tab2_form's plain-T form), so that the T
// product carries 2d once (ge_add of two cached points would carry it twice).
// The four products (Y+X)(Y+X), (Y-X)(Y-X), 2dT*T, Z*Z are interleaved as in
// ge_add_il, with no leading fe_addsub: both sides already hold their Y+X /
// Y-X.  t_neg: the T product is to be taken negated -- for two table entries
// whose Y+X / Y-X halves tab2_load swapped for a negative digit, the product
// of the two digits' signs; as in ge_add that trades Z and T, no field
// negation.  tab2_identity, (1, 1, 1, 0), is the identity in both forms.
COA_DEV void ge_add_cc_il(ge_p1p1& r, const ge_cached& p, const ge_cached& q, bool t_neg = false) {
  const fe a[4] = {p.YplusX, p.YminusX, p.T2d, p.Z}, b[4] = {q.YplusX, q.YminusX, q.T2d, q.Z};
  fe o[4], zs, zd;
  fe_mul_n<4>(o, a, b);
  fe_add(o[3], o[3], o[3]);
  fe_addsub(r.Y, r.X, o[0], o[1]);
  fe_addsub(zs, zd, o[3], o[2]);
  fe_cswap_to(r.Z, r.T, zs, zd, t_neg);
}

// A table entry's stored form: cached, or (plain_t) with plain T in the fourth
// field instead of 2dT -- ge_add_cc_il's second operand.
COA_DEV void tab2_form(ge_cached& c, const ge_p3& p, bool plain_t) {
  fe_add(c.YplusX, p.Y, p.X);
  fe_sub(c.YminusX, p.Y, p.X);
  c.Z = p.Z;
  c.T2d = p.T;
  if (!plain_t) {
    fe d2;
    fe_const_d2(d2);
    fe_mul(c.T2d, p.T, d2);
  }
}

// tab2_build (coa_smul.h: the table j*P, j = 1..8, of a decompressed point P,
// by doublings and mixed additions) with the entries in tab2_form's form.
// plain_t must be uniform over the workgroup.  In the plain-T form seven of the
// eight 2d*T products go (P's own is still needed for the mixed additions).
COA_DEV void tab2_build_form(uint32_t* scr, uint32_t lane, int tab, const ge_p3& P, bool plain_t) {
  ge_cached c;
  ge_p3_to_cached(c, P);
  ge_niels n1;
  n1.yplusx = c.YplusX;
  n1.yminusx = c.YminusX;
  n1.xy2d = c.T2d;
  if (plain_t) c.T2d = P.T;
  tab2_store(scr, lane, tab, 0, c);
  ge_p2 q0, q1;
  ge_p3_to_p2(q0, P);
  q1 = q0;
#pragma unroll 1
  for (int k = 1; k <= 4; k++) {
    ge_p1p1 t;
    ge_p3 e;
    ge_p2_dbl(t, q0);
    ge_p1p1_to_p3(e, t);
    tab2_form(c, e, plain_t);
    tab2_store(scr, lane, tab, 2 * k - 1, c);
    if (k == 1) {
      ge_p3_to_p2(q0, e);
    } else {
      q0 = q1;
      if (k == 2) ge_p3_to_p2(q1, e);
    }
    if (k < 4) {
      ge_madd(t, e, n1);
      ge_p1p1_to_p3(e, t);
      tab2_form(c, e, plain_t);
      tab2_store(scr, lane, tab, 2 * k, c);
      if (k == 1) ge_p3_to_p2(q1, e);
    }
  }
}

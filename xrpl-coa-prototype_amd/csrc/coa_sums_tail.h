// The excess top digits of k_verify_main_sums (coa_halved.hip) on the DPP
// rows.  That kernel loops max(H) times over a 256-item workgroup, and H =
// (max(bits c, bits d) + 5) / 4 has a tail the halving cannot avoid (d must be
// odd): 98.8 % of the items need at most 33 digits, 1.2 % need 34 and a few
// more (profiles/halve_width_hist.json), so nearly every workgroup used to
// loop 34 times and the longest of a C2 call 36 times, every lane of it paying
// four doublings and an addition per extra digit.  The loop is now capped at
// COA_SUMS_CAP digits, and a consumer wave first computes, for each of its
// lanes above the cap (a tail lane),
//     acc0 = 16 * sum_{pos >= cap} 16^(pos - cap) (A_tab[dc_pos] + R_tab[dr_pos])
// with the whole wave on that one item: the point in rp::'s row form
// (coa_ge_rows.h: a step's four products on the four rows at once, ~1 product
// time per step instead of four on one lane), the digits and the table entries
// loaded from the item's record and slab straight into row form.  The lane
// then enters the digit loop with acc0 instead of the identity; the loop's
// first iteration does not double, hence the factor 16.  The wave takes its
// tail lanes one after another (their table loads two lanes at a time); this
// runs beside the producer wave's first sum, before the consumer's first
// barrier.  One row per tail lane (four lanes per pass, each row doing a
// step's four products in turn) has the same throughput and four times the
// latency for the one or two tail lanes a wave usually has.
//
// Kept out of coa_ge.h / coa_smul.h / coa_fe.h: committed counter profiles are
// tied to those files by sha256.
#pragma once
#include "coa_ge_rows.h"

// Digits the loop of k_verify_main_sums runs at most.
#ifndef COA_SUMS_CAP
#define COA_SUMS_CAP 33
#endif
// The most tail lanes a wave may have for its workgroup to cap the loop; above
// it the workgroup loops max(H) times as before (k can be ground offline, so a
// call may consist of tail items only, and 64 row passes per wave cost more
// than the extra digit).  Measured: with k
// one-excess-digit tail lanes in every wave of a C2 call one more loop
// iteration costs 11.6 us and one tail lane 4.6 us, the first ~4 us hidden
// behind the producer's first sum (tools/sums_tail_breakeven.py: capped
// against uncapped 0.594 / 0.604 ms at k = 1, 0.607 / 0.604 at 4, 0.627 / 0.604
// at 8), a break-even of 3 lanes when every wave has them.  With natural k few
// waves do, and a workgroup that falls back pays for its deepest lane too: the
// bench's call runs in 0.611 ms at a threshold of 3 or 4, 0.607 at 5, 6, 8 and
// 64, 0.623 uncapped (profiles/sums_tail_ab.json).  6 keeps the natural gain;
// a call ground to six tail lanes in every wave runs ~2 % longer than
// uncapped.  COA_SUMS_TAIL_MAX (environment, read per call) overrides it for
// A/B runs and tests.
#ifndef COA_SUMS_TAIL_MAX
#define COA_SUMS_TAIL_MAX 6
#endif

namespace sums_tail {

// Entry |d| of table `tab` of item's slab (coa_smul.h tab2_store: Y+X, Y-X, Z
// and the T field, 8 dwords each) for the signed digit d in row form, as a
// cached point: negated for d < 0, the identity for d == 0.  plain_t: the T
// field holds plain T (tab2_form), so 2d*T takes a row product here.  item,
// tab and d are wave-uniform.
COA_DEV void entry(rp::Ca& c, const uint32_t* __restrict__ scr, uint32_t item, int tab, int d, bool plain_t) {
  const int m = d < 0 ? -d : d;
  const uint32_t l = __lane_id() & 15u;
  if (m == 0) {
    const uint32_t one = l == 0 ? 1u : 0u;
    c.ypx = one;
    c.ymx = one;
    c.Z = one;
    c.t2d = 0;
    return;
  }
  const uint32_t* e = scr + ((uint64_t)item * 16 + (uint32_t)(tab * 8 + m - 1)) * 32;
  const uint32_t k = l & 7u;  // lanes 8..15 load in bounds and drop the word
  const uint32_t w0 = e[k], w1 = e[8 + k], w2 = e[16 + k], w3 = e[24 + k];
  const bool lo = l < 8;
  const uint32_t ypx = lo ? w0 : 0u, ymx = lo ? w1 : 0u;
  c.Z = lo ? w2 : 0u;
  uint32_t t = lo ? w3 : 0u;
  if (plain_t) {
    fe d2;
    fe_const_d2(d2);
    t = fw::mul(t, fw::from_fe(d2));
  }
  if (d < 0) {  // -(x, y) = (-x, y): swap Y+X and Y-X, negate 2dT
    c.ypx = ymx;
    c.ymx = ypx;
    c.t2d = fw::sub(0u, t);
  } else {
    c.ypx = ypx;
    c.ymx = ymx;
    c.t2d = t;
  }
}

// A tail lane's top digit pair: both table entries as loaded (this lane's limb
// of each field; lanes 8..15 of a row hold a limb they drop in top_sum) and the
// two signed digits.  Nearly every tail lane has this one excess digit only.
struct Top {
  uint32_t a[4], r[4];  // Y+X, Y-X, Z, T field of the A / R entry
  int dc, dr;
};

// The loads of a Top for the wave-uniform digits dc, dr of item (a zero digit
// loads entry 1 in bounds and takes the identity in top_sum).
COA_DEV void top_load(Top& w, const uint32_t* __restrict__ scr, uint32_t item, int dc, int dr) {
  const int ma = dc < 0 ? -dc : dc, mr = dr < 0 ? -dr : dr;
  const uint32_t k = __lane_id() & 7u;
  const uint32_t* ea = scr + ((uint64_t)item * 16 + (uint32_t)(ma == 0 ? 0 : ma - 1)) * 32 + k;
  const uint32_t* er = scr + ((uint64_t)item * 16 + 8u + (uint32_t)(mr == 0 ? 0 : mr - 1)) * 32 + k;
#pragma unroll
  for (int f = 0; f < 4; f++) {
    w.a[f] = ea[8 * f];
    w.r[f] = er[8 * f];
  }
  w.dc = dc;
  w.dr = dr;
}

// A_tab[dc] + R_tab[dr] (p1p1, lazy) straight from the two addend forms, as
// ge_add_cc_il (coa_ge_sums.h): the four products (Y+X)(Y+X), (Y-X)(Y-X),
// 2dT * T, Z * Z on the four rows at once, so the sum costs one row product
// and R's plain T needs no 2d.  A negative digit swaps its entry's Y+X / Y-X;
// the product of the two signs swaps Z and T of the result.
COA_DEV void top_sum(rp::L1& t, const Top& w) {
  const uint32_t l = __lane_id() & 15u;
  const bool lo = l < 8;
  const uint32_t one = l == 0 ? 1u : 0u;
  uint32_t a[4], r[4];
#pragma unroll
  for (int f = 0; f < 4; f++) {
    a[f] = w.dc == 0 ? (f < 3 ? one : 0u) : (lo ? w.a[f] : 0u);
    r[f] = w.dr == 0 ? (f < 3 ? one : 0u) : (lo ? w.r[f] : 0u);
  }
  const uint32_t x = rp::pick(w.dc < 0 ? a[1] : a[0], w.dc < 0 ? a[0] : a[1], a[3], a[2]);
  const uint32_t y = rp::pick(w.dr < 0 ? r[1] : r[0], w.dr < 0 ? r[0] : r[1], r[3], r[2]);
  uint32_t b, aa, cc, zz;
  rp::rows4(fw::mul(x, y), b, aa, cc, zz);
  const uint64_t p4 = fw::four_p();
  const uint64_t zs = 2 * (uint64_t)zz + cc, zd = 2 * (uint64_t)zz + p4 - cc;
  const bool t_neg = (w.dc < 0) != (w.dr < 0);
  t.X = (uint64_t)b + p4 - aa;
  t.Y = (uint64_t)b + aa;
  t.Z = t_neg ? zd : zs;
  t.T = t_neg ? zs : zd;
}

// out = 16 * sum_{pos = lo}^{hi - 1} 16^(pos - lo) (A_tab[dc_pos] + R_tab[dr_pos])
// of one item, replicated on every lane: dc / dd are nibble pos of words 0..7 /
// 8..15 of the item's record minus 8, dr = dneg ? -dd : dd; table 0 is cached,
// table 1 in the plain-T form.  top holds position hi - 1, already loaded;
// lower excess positions (rare) load as they go.  lo < hi <= 64.  All 64 lanes
// of the wave execute this together, with wave-uniform arguments.
COA_DEV void excess(ge_p3& out, const uint32_t* __restrict__ rec, const uint32_t* __restrict__ scr, uint32_t item,
                    int lo, int hi, bool dneg, const Top& top) {
  const uint32_t* r = rec + (uint64_t)item * 32;
  rp::P1 acc3;
  rp::P2 acc2;
  rp::L1 t;
  top_sum(t, top);
  rp::to_p2(acc2, t);
#pragma unroll 1
  for (int pos = hi - 2; pos >= lo; pos--) {
    const int sh = 4 * (pos & 7);
    const int dc = (int)((r[pos >> 3] >> sh) & 15u) - 8;
    const int dd = (int)((r[8 + (pos >> 3)] >> sh) & 15u) - 8;
    rp::Ca qa, qr;
    entry(qa, scr, item, 0, dc, false);
    entry(qr, scr, item, 1, dneg ? -dd : dd, true);
#pragma unroll 1
    for (int k = 0; k < 3; k++) {
      rp::dbl(t, acc2);
      rp::to_p2(acc2, t);
    }
    rp::dbl(t, acc2);
    rp::to_p3(acc3, t);
    rp::add(t, acc3, qa);
    rp::to_p3(acc3, t);
    rp::add(t, acc3, qr);
    rp::to_p2(acc2, t);
  }
#pragma unroll 1
  for (int k = 0; k < 3; k++) {
    rp::dbl(t, acc2);
    rp::to_p2(acc2, t);
  }
  rp::dbl(t, acc2);
  rp::to_p3(acc3, t);
  rp::to_ge_p3(out, acc3);
}

// For every lane of the wave with `tail` set: acc = excess(item, lo, H of meta,
// sign of meta), item and meta (record word 24, lo < H <= 64) being that
// lane's.  The other lanes keep their acc.  The tail lanes first load their own
// top digit words, all at once; a wave-uniform loop then takes the tail lanes
// two at a time, both lanes' table entries loaded before either is computed,
// so a pair waits for memory once.  Nothing in the loop runs under a per-lane
// condition but the final select; all 64 lanes call this.
COA_DEV void prologue(ge_p3& acc, bool tail, uint32_t item, uint32_t meta, const uint32_t* __restrict__ rec,
                      const uint32_t* __restrict__ scr, int lo) {
  // this lane's top digits (0, 0 on the other lanes)
  const int top = min((int)(meta & 0xffu), 64) - 1;
  const uint32_t* mine = rec + (uint64_t)(tail ? item : 0u) * 32 + (tail ? top >> 3 : 0);
  const uint32_t cw = mine[0], dw = mine[8];
  const int sh = 4 * (top & 7);
  const int dc = tail ? (int)((cw >> sh) & 15u) - 8 : 0;
  const int dd = tail ? (int)((dw >> sh) & 15u) - 8 : 0;
  const int dr = (meta >> 31) != 0 ? -dd : dd;
  uint64_t todo = __builtin_amdgcn_ballot_w64(tail);
#pragma unroll 1
  while (todo) {
    int owner[2];
    owner[0] = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int cnt = todo ? 2 : 1;
    owner[1] = todo ? __builtin_ctzll(todo) : owner[0];
    todo &= todo - 1;  // 0 stays 0
    Top w[2];
#pragma unroll
    for (int j = 0; j < 2; j++)
      top_load(w[j], scr, (uint32_t)__builtin_amdgcn_readlane((int)item, owner[j]),
               __builtin_amdgcn_readlane(dc, owner[j]), __builtin_amdgcn_readlane(dr, owner[j]));
#pragma unroll 1
    for (int j = 0; j < cnt; j++) {
      const int own = j ? owner[1] : owner[0];
      Top cur;
#pragma unroll
      for (int f = 0; f < 4; f++) {
        cur.a[f] = j ? w[1].a[f] : w[0].a[f];
        cur.r[f] = j ? w[1].r[f] : w[0].r[f];
      }
      cur.dc = j ? w[1].dc : w[0].dc;
      cur.dr = j ? w[1].dr : w[0].dr;
      const uint32_t it = (uint32_t)__builtin_amdgcn_readlane((int)item, own);
      const uint32_t mt = (uint32_t)__builtin_amdgcn_readlane((int)meta, own);
      ge_p3 s;
      excess(s, rec, scr, it, lo, min((int)(mt & 0xffu), 64), (mt >> 31) != 0, cur);
      const bool me = (int)__lane_id() == own;
      const fe* from[4] = {&s.X, &s.Y, &s.Z, &s.T};
      fe* to[4] = {&acc.X, &acc.Y, &acc.Z, &acc.T};
#pragma unroll
      for (int q = 0; q < 4; q++)
#pragma unroll
        for (int k = 0; k < 8; k++) to[q]->v[k] = me ? from[q]->v[k] : to[q]->v[k];
    }
  }
}

}  // namespace sums_tail


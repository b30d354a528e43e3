// Committee key cache build for gfx950.
//
// The reference re-decompresses every voter key on every call
// (crypto/src/lib.rs:202,216) although keys are fixed per Committee
// (config/src/lib.rs:140-143).  coa_committee_register() precomputes, once
// per committee and per device:
//   k_key_flags    decompression verdict, small order ([8]A == O) and
//                  torsion freedom ([l]A == O) of every key
//   k_key_tables   a comb of -A per key: entry (j, v) = (v+1)*256^j*(-A) as
//                  affine Niels, built by exact double-and-add, so torsion
//                  components are kept (the comb is an integer multiple, never
//                  reduced mod l)
//   k_key_wcomb, k_key_wcomb20   the wide combs of -A, summed from that comb
// kernels here exceed the +-128 KiB reach of an out-of-line fold (coa_fe.h)
#define COA_RARE_INLINE
#include "coa_committee.h"

#include <cstdlib>

#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_halved.h"
#include "coa_sc.h"
#include "coa_keycache.h"
#include "coa_smul.h"

namespace {
using namespace coa_kc;

COA_DEV void ge_neg(ge_p3& r, const ge_p3& p) {
  r = p;
  fe_neg(r.X, p.X);
  fe_neg(r.T, p.T);
}

// [m]P by MSB-first double-and-add over bits top..0 of m: an exact integer
// multiple (registration only; latency is irrelevant there).
COA_DEV void ge_mul_bits(ge_p3& out, const ge_p3& P, const uint32_t* m, int top) {
  ge_cached Pc;
  ge_p3_to_cached(Pc, P);
  ge_p3 acc;
  ge_p3_identity(acc);
  ge_p1p1 t;
#pragma unroll 1
  for (int b = top; b >= 0; b--) {
    ge_p3_dbl(t, acc);
    ge_p1p1_to_p3(acc, t);
    if ((word_sel(m, b >> 5) >> (b & 31)) & 1u) {
      ge_add(t, acc, Pc);
      ge_p1p1_to_p3(acc, t);
    }
  }
  out = acc;
}

COA_DEV void store_niels(uint32_t* e, const ge_p3& P) {
  fe zi, x, y, xy, d2, n0, n1, n2;
  fe_invert(zi, P.Z);
  fe_mul(x, P.X, zi);
  fe_mul(y, P.Y, zi);
  fe_mul(xy, x, y);
  fe_const_d2(d2);
  fe_add(n0, y, x);
  fe_sub(n1, y, x);
  fe_mul(n2, xy, d2);
  fe_canon(n0, n0);
  fe_canon(n1, n1);
  fe_canon(n2, n2);
  uint4* o = reinterpret_cast<uint4*>(e);
  o[0] = make_uint4(n0.v[0], n0.v[1], n0.v[2], n0.v[3]);
  o[1] = make_uint4(n0.v[4], n0.v[5], n0.v[6], n0.v[7]);
  o[2] = make_uint4(n1.v[0], n1.v[1], n1.v[2], n1.v[3]);
  o[3] = make_uint4(n1.v[4], n1.v[5], n1.v[6], n1.v[7]);
  o[4] = make_uint4(n2.v[0], n2.v[1], n2.v[2], n2.v[3]);
  o[5] = make_uint4(n2.v[4], n2.v[5], n2.v[6], n2.v[7]);
}

}  // namespace

// ---------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_key_flags(const uint32_t* __restrict__ keys, uint32_t nk,
                                                   uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nk) return;
  uint32_t w[8];
  load8(w, keys + (uint64_t)i * 8);
  ge_p3 A;
  uint32_t f = 0;
  if (ge_decompress(A, w)) {
    f |= COA_KEY_DECOMPRESSES;
    if (ge_is_small_order(A)) f |= COA_KEY_SMALL_ORDER;
    uint32_t l[8];
    sc_const_l(l);
    ge_p3 LA;
    ge_mul_bits(LA, A, l, 252);
    ge_p2 q;
    ge_p3_to_p2(q, LA);
    if (ge_p2_is_identity(q)) f |= COA_KEY_TORSION_FREE;
  }
  flags[i] = f;
}

// one lane per table entry: (key, j, v) -> (v+1)*256^j*(-A)
__global__ void __launch_bounds__(256) k_key_tables(const uint32_t* __restrict__ keys, uint32_t nk,
                                                    uint32_t* __restrict__ tabs) {
  const uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t key = (uint32_t)(id / COA_KEY_TAB_ENTRIES);
  if (key >= nk) return;
  const uint32_t e = (uint32_t)(id % COA_KEY_TAB_ENTRIES), j = e >> 7, v = e & 127;
  uint32_t w[8];
  load8(w, keys + (uint64_t)key * 8);
  uint32_t* out = tabs + (uint64_t)key * COA_KEY_TAB_DWORDS + (uint64_t)e * 24;
  ge_p3 A;
  if (!ge_decompress(A, w)) {  // never selected by an accepting path; keep it a valid point
    ge_p3_identity(A);
  }
  ge_p3 nA, M;
  ge_neg(nA, A);
  uint32_t m[8];
#pragma unroll
  for (int i = 0; i < 8; i++) m[i] = 0;
  // (v+1) << 8j with v+1 <= 128: at most two dwords are nonzero
  const uint64_t sh = (uint64_t)(v + 1) << ((8 * j) & 31);
#pragma unroll
  for (int i = 0; i < 8; i++) {
    if (i == (int)((8 * j) >> 5)) m[i] = (uint32_t)sh;
    if (i == (int)((8 * j) >> 5) + 1) m[i] = (uint32_t)(sh >> 32);
  }
  ge_mul_bits(M, nA, m, 8 * j + 7);
  store_niels(out, M);
}

hipError_t coa_launch_key_flags(const uint32_t* keys, uint32_t nk, uint32_t* flags, hipStream_t s) {
  if (nk == 0) return hipSuccess;
  hipLaunchKernelGGL(k_key_flags, dim3((nk + 255) / 256), dim3(256), 0, s, keys, nk, flags);
  return hipGetLastError();
}

// Wide comb entry (key, j, m-1) = m * 2^(16 j) * (-A): with m = lo + 256 hi,
// lo a signed byte, it is the sum of the exact radix-256 comb entries
// (2j, lo) and (2j+1, hi) -- an integer multiple, torsion kept -- made affine.
__global__ void __launch_bounds__(256) k_key_wcomb(const uint32_t* __restrict__ tabs, uint32_t nk,
                                                   uint32_t* __restrict__ wtabs) {
  // grid-stride (a bounded, resident grid: see coa_launch_key_wcombs20)
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < (uint64_t)nk * COA_KWCOMB_ENTRIES;
       id += (uint64_t)gridDim.x * blockDim.x) {
  const uint32_t key = (uint32_t)(id / COA_KWCOMB_ENTRIES);
  const uint32_t e = (uint32_t)(id % COA_KWCOMB_ENTRIES);
  const int j = (int)(e >> (COA_KWCOMB_W - 1));
  const int m = (int)(e & ((1u << (COA_KWCOMB_W - 1)) - 1)) + 1;
  int lo = m & 255, hi = m >> 8;
  if (lo >= 128) {
    lo -= 256;
    hi += 1;
  }
  const uint32_t* ktab = tabs + (uint64_t)key * COA_KEY_TAB_DWORDS;
  ge_p3 P;
  ge_p3_identity(P);
  ge_p1p1 t;
  ge_niels q;
  comb_select(q, ktab, 2 * j, lo);
  ge_madd(t, P, q);
  ge_p1p1_to_p3(P, t);
  comb_select(q, ktab, 2 * j + 1, hi);
  ge_madd(t, P, q);
  ge_p1p1_to_p3(P, t);
  store_niels(wtabs + (uint64_t)key * COA_KWCOMB_DWORDS + (uint64_t)e * COA_KWC_STRIDE, P);
  }
}

// Widest comb entry (key, j, m-1) = m * 2^(20 j) * (-A): 20 j = 8 q + r, and
// m 2^r < 2^24 is recoded into signed bytes b0, b1, b2, so the entry is the
// sum of the exact radix-256 comb entries (q, b0), (q+1, b1), (q+2, b2) -- an
// integer multiple, torsion kept -- made affine.  At j = 12 (q = 30) a byte
// at position 32 would be needed only for m > 2^16, which no scalar below l
// produces (its top digit is at most 2^13, wc_recode): those entries are
// never read and hold the sum of the first two bytes.
__global__ void __launch_bounds__(256) k_key_wcomb20(const uint32_t* __restrict__ tabs, uint32_t nk,
                                                     uint32_t* __restrict__ wtabs) {
  // grid-stride (a bounded, resident grid: see coa_launch_key_wcombs20)
  for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < (uint64_t)nk * COA_KWCOMB20_ENTRIES;
       id += (uint64_t)gridDim.x * blockDim.x) {
  const uint32_t key = (uint32_t)(id / COA_KWCOMB20_ENTRIES);
  const uint64_t e = id % COA_KWCOMB20_ENTRIES;
  const int j = (int)(e >> (COA_KWCOMB20_W - 1));
  const uint32_t m = (uint32_t)(e & ((1u << (COA_KWCOMB20_W - 1)) - 1)) + 1;
  const int bit = COA_KWCOMB20_W * j, q = bit >> 3;
  uint32_t v = m << (bit & 7);
  int b[3];
  int carry = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    int x = (int)(v & 255u) + carry;
    v >>= 8;
    carry = 0;
    if (i < 2 && x >= 128) {
      x -= 256;
      carry = 1;
    }
    b[i] = x;
  }
  const uint32_t* ktab = tabs + (uint64_t)key * COA_KEY_TAB_DWORDS;
  ge_p3 P;
  ge_p3_identity(P);
  ge_p1p1 t;
  ge_niels qn;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    if (q + i > 31) break;
    comb_select(qn, ktab, q + i, b[i]);
    ge_madd(t, P, qn);
    ge_p1p1_to_p3(P, t);
  }
  store_niels(wtabs + (uint64_t)key * COA_KWCOMB20_DWORDS + e * COA_KWC_STRIDE, P);
  }
}

// The wide key combs are built while the device serves live windows (a
// registration builds the next key-cache generation beside the current one,
// on a least-priority stream: coa_runtime.cpp build_keyset).  One workgroup
// per 256 entries by default -- short workgroups, so the scheduler hands the
// CUs to the windows' workgroups between them; COA_BUILD_BLOCKS=<n> bounds
// the grid to n resident workgroups striding over the entries (A/B:
// slower build, p99 0.65 vs 0.89 ms under a 5,000/s certificate stream).
static uint32_t build_blocks(uint64_t total) {
  const char* e = getenv("COA_BUILD_BLOCKS");
  const uint64_t cap = e ? strtoull(e, nullptr, 10) : 0;
  const uint64_t want = (total + 255) / 256;
  return (uint32_t)(want < cap ? want : (cap ? cap : want));
}

hipError_t coa_launch_key_wcombs20(const uint32_t* tabs, uint32_t nk, uint32_t* wtabs, hipStream_t s) {
  if (nk == 0) return hipSuccess;
  const uint64_t total = (uint64_t)nk * COA_KWCOMB20_ENTRIES;
  hipLaunchKernelGGL(k_key_wcomb20, dim3(build_blocks(total)), dim3(256), 0, s, tabs, nk, wtabs);
  return hipGetLastError();
}

hipError_t coa_launch_key_wcombs(const uint32_t* tabs, uint32_t nk, uint32_t* wtabs, hipStream_t s) {
  if (nk == 0) return hipSuccess;
  const uint64_t total = (uint64_t)nk * COA_KWCOMB_ENTRIES;
  hipLaunchKernelGGL(k_key_wcomb, dim3(build_blocks(total)), dim3(256), 0, s, tabs, nk, wtabs);
  return hipGetLastError();
}

hipError_t coa_launch_key_tables(const uint32_t* keys, uint32_t nk, uint32_t* tabs, hipStream_t s) {
  if (nk == 0) return hipSuccess;
  const uint64_t lanes = (uint64_t)nk * COA_KEY_TAB_ENTRIES;
  hipLaunchKernelGGL(k_key_tables, dim3((uint32_t)((lanes + 255) / 256)), dim3(256), 0, s, keys, nk, tabs);
  return hipGetLastError();
}

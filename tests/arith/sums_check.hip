// Test-only device library, beside arith_check.hip and alias_check.hip: the
// sum of two addend-form points, ge_add_cc_il (csrc/coa_ge_sums.h), as
// k_verify_main_sums' producer waves use it -- one item per lane, operands in,
// RAW output limbs of the p1p1 -> p3 result out, for
// tests/test_gpu_arith_sums.py.
//
//   OP_ADD_CC   p and q extended with any Z; p goes to cached form, q to the
//               plain-T form.  Control word: bit 0 / 1 negate p / q the way
//               tab2_load does (Y+X and Y-X swapped, the T field as stored),
//               bit 2 / 3 replace p / q by the literal identity entry
//               tab2_identity.  The T product's sign goes in as bit 0 != bit 1.
//   OP_TAB_SUM  p and q affine; table 0 of the item's slab is built from p in
//               cached form (tab2_build), table 1 from q in plain-T form
//               (tab2_build_form), both entries come back through tab2_load for
//               the digits c[0] - 8 and c[1] - 8: the producer's path for one
//               digit.
//
// build.py compiles this file twice into lib/libcoa_sumscheck.so, as is and
// with -DCOA_RARE_INLINE; coa_sums_run picks one.  Blocks are 64 threads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_ge_sums.h"
#include "coa_smul.h"

#ifdef COA_RARE_INLINE
#define COA_SM_NS sm_inl
#define COA_SM_RUN coa_sums_run_inl
#else
#define COA_SM_NS sm_out
#define COA_SM_RUN coa_sums_run_out
#endif

// words of table slab per item (two tables of 8 entries)
#define COA_SM_SLAB_WORDS (COA_HALVED_SCRATCH_PER_LANE / 4)

namespace COA_SM_NS {

// Keep in step with OPS of tests/test_gpu_arith_sums.py.
enum Op : int { OP_ADD_CC = 0, OP_TAB_SUM, OP_COUNT };

COA_DEV void ld_fe(fe& r, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
}
COA_DEV void st_fe(uint32_t* w, const fe& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
COA_DEV void ld_p3(ge_p3& p, const uint32_t* w) {
  ld_fe(p.X, w);
  ld_fe(p.Y, w + 8);
  ld_fe(p.Z, w + 16);
  ld_fe(p.T, w + 24);
}
COA_DEV void ld_affine(ge_p3& p, const uint32_t* w) {
  ld_fe(p.X, w);
  ld_fe(p.Y, w + 8);
  fe_set(p.Z, 1);
  fe_mul(p.T, p.X, p.Y);
}
// what tab2_load hands out for a negative digit / for digit zero
COA_DEV void as_loaded(ge_cached& c, bool neg, bool ident) {
  if (ident) {
    ld_fe(c.YplusX, tab2_identity);
    ld_fe(c.YminusX, tab2_identity + 8);
    ld_fe(c.Z, tab2_identity + 16);
    ld_fe(c.T2d, tab2_identity + 24);
  }
  if (neg) {
    const fe s = c.YplusX;
    c.YplusX = c.YminusX;
    c.YminusX = s;
  }
}

// A: p (32 words, or 16 affine), B: q likewise, C: two control words
template <int OP>
__global__ void __launch_bounds__(64) k_sums(const uint32_t* __restrict__ d_a, const uint32_t* __restrict__ d_b,
                                             const uint32_t* __restrict__ d_c, uint32_t n,
                                             uint32_t* __restrict__ d_scr, uint32_t* __restrict__ d_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  constexpr int NW = OP == OP_ADD_CC ? 32 : 16;
  uint32_t A[NW], B[NW];
#pragma unroll
  for (int k = 0; k < NW; k++) {
    A[k] = d_a[(uint64_t)i * NW + k];
    B[k] = d_b[(uint64_t)i * NW + k];
  }
  const uint32_t c0 = d_c[2 * (uint64_t)i], c1 = d_c[2 * (uint64_t)i + 1];
  ge_p3 p, q, r;
  ge_cached pc, qc;
  ge_p1p1 t;
  if constexpr (OP == OP_ADD_CC) {
    ld_p3(p, A);
    ld_p3(q, B);
    tab2_form(pc, p, false);
    tab2_form(qc, q, true);
    const bool np = (c0 & 1u) != 0, nq = (c0 & 2u) != 0;
    as_loaded(pc, np, (c0 & 4u) != 0);
    as_loaded(qc, nq, (c0 & 8u) != 0);
    ge_add_cc_il(t, pc, qc, np != nq);
  } else {
    ld_affine(p, A);
    ld_affine(q, B);
    tab2_build(d_scr, i, 0, p);
    tab2_build_form(d_scr, i, 1, q, true);
    const int dp = (int)c0 - 8, dq = (int)c1 - 8;
    tab2_load(pc, d_scr, i, 0, dp);
    tab2_load(qc, d_scr, i, 1, dq);
    ge_add_cc_il(t, pc, qc, (dp < 0) != (dq < 0));
  }
  ge_p1p1_to_p3_il(r, t);
  uint32_t* dst = d_out + (uint64_t)i * 32;
  st_fe(dst, r.X);
  st_fe(dst + 8, r.Y);
  st_fe(dst + 16, r.Z);
  st_fe(dst + 24, r.T);
}

}  // namespace COA_SM_NS

extern "C" {

__attribute__((visibility("default"))) int COA_SM_RUN(int op, const uint32_t* d_a, const uint32_t* d_b,
                                                      const uint32_t* d_c, uint32_t n, uint32_t* d_scr,
                                                      uint32_t* d_out, void* stream) {
  using namespace COA_SM_NS;
  if (!d_a || !d_b || !d_c || !d_out) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  const dim3 grid((n + 63u) / 64u), block(64);
  if (op == OP_ADD_CC) {
    hipLaunchKernelGGL(k_sums<OP_ADD_CC>, grid, block, 0, (hipStream_t)stream, d_a, d_b, d_c, n, d_scr, d_out);
  } else if (op == OP_TAB_SUM) {
    if (!d_scr) return (int)hipErrorInvalidValue;  // n slabs of COA_SM_SLAB_WORDS words
    hipLaunchKernelGGL(k_sums<OP_TAB_SUM>, grid, block, 0, (hipStream_t)stream, d_a, d_b, d_c, n, d_scr, d_out);
  } else {
    return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}

#ifndef COA_RARE_INLINE
int coa_sums_run_inl(int op, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, uint32_t n,
                     uint32_t* d_scr, uint32_t* d_out, void* stream);

// Runs op on n items (device pointers; the current device, the given stream)
// and returns the HIP error code.  rare_inline picks the COA_RARE_INLINE copy.
__attribute__((visibility("default"))) int coa_sums_run(int op, int rare_inline, const uint32_t* d_a,
                                                        const uint32_t* d_b, const uint32_t* d_c, uint32_t n,
                                                        uint32_t* d_scr, uint32_t* d_out, void* stream) {
  return rare_inline ? coa_sums_run_inl(op, d_a, d_b, d_c, n, d_scr, d_out, stream)
                     : coa_sums_run_out(op, d_a, d_b, d_c, n, d_scr, d_out, stream);
}

__attribute__((visibility("default"))) int coa_sums_op_count(void) { return COA_SM_NS::OP_COUNT; }
__attribute__((visibility("default"))) int coa_sums_slab_words(void) { return COA_SM_SLAB_WORDS; }
#endif

}  // extern "C"

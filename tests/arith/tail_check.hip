// Test-only device library, beside sums_check.hip: the row prologue of
// k_verify_main_sums, sums_tail::prologue (csrc/coa_sums_tail.h), on synthetic
// records and tables -- RAW output limbs of each lane's accumulator out, for
// tests/test_gpu_arith_tail.py.
//
// Per lane: p and q affine, a 32-word halving record (words 0..7 / 8..15 the
// digits of c / |d| as nibbles + 8, word 24 = H | (d < 0) << 31) and a control
// word (bit 0: the lane is a tail lane).  Table 0 of the lane's slab is built
// from p in cached form (tab2_build), table 1 from q in plain-T form
// (tab2_build_form), as k_pre_halve<3, true> leaves them; every lane starts
// from the identity and the wave runs the prologue from digit position lo.
//
// build.py compiles this file twice into lib/libcoa_tailcheck.so, as is and
// with -DCOA_RARE_INLINE; coa_tail_run picks one.  Blocks are 64 threads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_ge_sums.h"
#include "coa_smul.h"
#include "coa_sums_tail.h"

#ifdef COA_RARE_INLINE
#define COA_TL_NS tl_inl
#define COA_TL_RUN coa_tail_run_inl
#else
#define COA_TL_NS tl_out
#define COA_TL_RUN coa_tail_run_out
#endif

#define COA_TL_SLAB_WORDS (COA_HALVED_SCRATCH_PER_LANE / 4)

namespace COA_TL_NS {

COA_DEV void ld_affine(ge_p3& p, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    p.X.v[i] = w[i];
    p.Y.v[i] = w[8 + i];
  }
  fe_set(p.Z, 1);
  fe_mul(p.T, p.X, p.Y);
}

// n must be a multiple of 64: every lane of a wave runs the prologue
__global__ void __launch_bounds__(64) k_tail(const uint32_t* __restrict__ d_p, const uint32_t* __restrict__ d_q,
                                             const uint32_t* __restrict__ d_rec, const uint32_t* __restrict__ d_ctl,
                                             int lo, uint32_t* d_scr, uint32_t* __restrict__ d_out) {
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  ge_p3 p, q;
  ld_affine(p, d_p + (uint64_t)i * 16);
  ld_affine(q, d_q + (uint64_t)i * 16);
  tab2_build(d_scr, i, 0, p);
  tab2_build_form(d_scr, i, 1, q, true);
  __threadfence();  // the prologue's lanes read other lanes' slabs
  __syncthreads();
  const uint32_t meta = d_rec[(uint64_t)i * 32 + 24];
  ge_p3 acc;
  ge_p3_identity(acc);
  sums_tail::prologue(acc, (d_ctl[i] & 1u) != 0, i, meta, d_rec, d_scr, lo);
  uint32_t* dst = d_out + (uint64_t)i * 32;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    dst[k] = acc.X.v[k];
    dst[8 + k] = acc.Y.v[k];
    dst[16 + k] = acc.Z.v[k];
    dst[24 + k] = acc.T.v[k];
  }
}

}  // namespace COA_TL_NS

extern "C" {

__attribute__((visibility("default"))) int COA_TL_RUN(const uint32_t* d_p, const uint32_t* d_q, const uint32_t* d_rec,
                                                      const uint32_t* d_ctl, int lo, uint32_t n, uint32_t* d_scr,
                                                      uint32_t* d_out, void* stream) {
  if (!d_p || !d_q || !d_rec || !d_ctl || !d_scr || !d_out) return (int)hipErrorInvalidValue;
  if (n == 0 || n % 64u != 0 || lo < 0 || lo > 63) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(COA_TL_NS::k_tail, dim3(n / 64u), dim3(64), 0, (hipStream_t)stream, d_p, d_q, d_rec, d_ctl, lo,
                     d_scr, d_out);
  return (int)hipGetLastError();
}

#ifndef COA_RARE_INLINE
int coa_tail_run_inl(const uint32_t* d_p, const uint32_t* d_q, const uint32_t* d_rec, const uint32_t* d_ctl, int lo,
                     uint32_t n, uint32_t* d_scr, uint32_t* d_out, void* stream);

// Runs the prologue on n lanes (a multiple of 64; device pointers, d_scr n
// slabs of coa_tail_slab_words words; the current device, the given stream)
// and returns the HIP error code.  rare_inline picks the COA_RARE_INLINE copy.
__attribute__((visibility("default"))) int coa_tail_run(int rare_inline, const uint32_t* d_p, const uint32_t* d_q,
                                                        const uint32_t* d_rec, const uint32_t* d_ctl, int lo,
                                                        uint32_t n, uint32_t* d_scr, uint32_t* d_out, void* stream) {
  return rare_inline ? coa_tail_run_inl(d_p, d_q, d_rec, d_ctl, lo, n, d_scr, d_out, stream)
                     : coa_tail_run_out(d_p, d_q, d_rec, d_ctl, lo, n, d_scr, d_out, stream);
}

__attribute__((visibility("default"))) int coa_tail_slab_words(void) { return COA_TL_SLAB_WORDS; }
#endif

}  // extern "C"

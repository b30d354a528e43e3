// Test-only kernels around csrc/coa_fe_pow29.h: the 29-bit-limb squaring,
// multiplication, the two conversions and the whole (p-5)/8 chain, one item
// per lane, operands in, RAW output limbs out, for
// tests/test_gpu_arith_pow29.py to compare with the integer model of
// tests/pow29_ref.py.  The header is included unchanged.
//
// build.py compiles this file twice into lib/libcoa_arithcheck.so, beside
// arith_check.hip: as is and with -DCOA_RARE_INLINE (fe29_to_fe ends in
// fe_fold_word; the chain itself has no rare block).  coa_pow29_run picks
// the copy.  Workgroups are 256 lanes; lanes at or above n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coa_fe_pow29.h"

#ifdef COA_RARE_INLINE
#define COA_P29_NS p29_inl
#define COA_P29_RUN coa_pow29_run_inl
#else
#define COA_P29_NS p29_out
#define COA_P29_RUN coa_pow29_run_out
#endif

namespace COA_P29_NS {

// Keep in step with OPS of tests/test_gpu_arith_pow29.py.
enum Op : int { OP_SQ = 0, OP_MUL, OP_FROM_FE, OP_TO_FE, OP_POW_P58, OP_COUNT };

__host__ __device__ constexpr int words_in(int op) { return op == OP_FROM_FE || op == OP_POW_P58 ? 8 : 9; }
__host__ __device__ constexpr int words_out(int op) { return op == OP_TO_FE || op == OP_POW_P58 ? 8 : 9; }

template <int OP>
__global__ void __launch_bounds__(256) k(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n,
                                         uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NI = words_in(OP), NO = words_out(OP);
  uint32_t x[9] = {}, y[9] = {}, r[9] = {};
#pragma unroll
  for (int j = 0; j < NI; j++) x[j] = a[(uint64_t)i * NI + j];
  if constexpr (OP == OP_MUL) {
#pragma unroll
    for (int j = 0; j < 9; j++) y[j] = b[(uint64_t)i * 9 + j];
  }
  fe29 p, q, s;
  fe f, g;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    p.v[j] = x[j];
    q.v[j] = y[j];
  }
#pragma unroll
  for (int j = 0; j < 8; j++) f.v[j] = x[j];
  if constexpr (OP == OP_SQ) {
    fe29_sq(s, p);
  } else if constexpr (OP == OP_MUL) {
    fe29_mul(s, p, q);
  } else if constexpr (OP == OP_FROM_FE) {
    fe29_from_fe(s, f);
  } else if constexpr (OP == OP_TO_FE) {
    fe29_to_fe(g, p);
  } else {
    fe_pow_p58_29(g, f);
  }
#pragma unroll
  for (int j = 0; j < 9; j++) r[j] = s.v[j];
  if constexpr (NO == 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) r[j] = g.v[j];
  }
#pragma unroll
  for (int j = 0; j < NO; j++) out[(uint64_t)i * NO + j] = r[j];
}

template <int OP = 0>
hipError_t dispatch(int op, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out, hipStream_t s) {
  if constexpr (OP < OP_COUNT) {
    if (op == OP) {
      hipLaunchKernelGGL(k<OP>, dim3((n + 255) / 256), dim3(256), 0, s, a, b, n, out);
      return hipGetLastError();
    }
    return dispatch<OP + 1>(op, a, b, n, out, s);
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace COA_P29_NS

extern "C" {

__attribute__((visibility("default"))) int COA_P29_RUN(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t n,
                                                       uint32_t* d_out, void* stream) {
  if (op < 0 || op >= COA_P29_NS::OP_COUNT) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  return (int)COA_P29_NS::dispatch<>(op, d_a, d_b, n, d_out, (hipStream_t)stream);
}

#ifndef COA_RARE_INLINE
int coa_pow29_run_inl(int op, const uint32_t* d_a, const uint32_t* d_b, uint32_t n, uint32_t* d_out, void* stream);

// Runs op on n items (device pointers: a and b hold words_in(op) dwords per
// item, b only for OP_MUL; out words_out(op) per item) on the current device
// and the given stream; returns the HIP error code.
__attribute__((visibility("default"))) int coa_pow29_run(int op, int rare_inline, const uint32_t* d_a,
                                                         const uint32_t* d_b, uint32_t n, uint32_t* d_out,
                                                         void* stream) {
  return rare_inline ? coa_pow29_run_inl(op, d_a, d_b, n, d_out, stream)
                     : coa_pow29_run_out(op, d_a, d_b, n, d_out, stream);
}
#endif

}  // extern "C"

// Test-only kernels around csrc/coa_ge29.h: every field helper and point
// formula of the limb-form accumulator, one item per lane, operands in, RAW
// output limbs out, for tests/test_gpu_arith_ge29.py to compare with the
// integer model of tests/ge29_ref.py.  The header is included unchanged.
//
// build.py compiles this file twice into lib/libcoa_ge29check.so: as is and
// with -DCOA_RARE_INLINE (ge29_p3_to ends in fe_fold_word; nothing else here
// has a rare block).  coa_ge29_run picks the copy.  Workgroups are 256 lanes;
// lanes at or above n do nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coa_ge29.h"

#ifdef COA_RARE_INLINE
#define COA_G29_NS g29_inl
#define COA_G29_RUN coa_ge29_run_inl
#else
#define COA_G29_NS g29_out
#define COA_G29_RUN coa_ge29_run_out
#endif

namespace COA_G29_NS {

// Keep in step with OPS of tests/test_gpu_arith_ge29.py.
enum Op : int {
  OP_ADD = 0, OP_SUB2, OP_SUB3, OP_SUB4, OP_CARRY, OP_CSWAP, OP_DBL, OP_TO_P2, OP_TO_P3, OP_ADD_PT, OP_P3_FROM,
  OP_P3_TO, OP_DIGIT, OP_COUNT
};

// dwords per item of a, b and out
__host__ __device__ constexpr int words_a(int op) {
  return op <= OP_CSWAP ? 9 : op == OP_DBL || op == OP_DIGIT ? 27 : op == OP_P3_FROM ? 32 : 36;
}
__host__ __device__ constexpr int words_b(int op) {
  return op <= OP_SUB4 || op == OP_CSWAP ? 9 : op == OP_ADD_PT || op == OP_DIGIT ? 36 : 0;
}
__host__ __device__ constexpr int words_out(int op) {
  return op <= OP_CARRY ? 9 : op == OP_CSWAP ? 18 : op == OP_TO_P2 || op == OP_DIGIT ? 27 : op == OP_P3_TO ? 32 : 36;
}

COA_DEV void put(uint32_t* r, const fe29& a, int at) {
#pragma unroll
  for (int j = 0; j < 9; j++) r[9 * at + j] = a.v[j];
}

template <int OP>
__global__ void __launch_bounds__(256) k(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                         const uint32_t* __restrict__ flag, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int NA = words_a(OP), NB = words_b(OP), NO = words_out(OP);
  uint32_t x[36] = {}, y[36] = {}, r[36] = {};
#pragma unroll
  for (int j = 0; j < NA; j++) x[j] = a[(uint64_t)i * NA + j];
#pragma unroll
  for (int j = 0; j < NB; j++) y[j] = b[(uint64_t)i * NB + j];
  const bool c = flag[i] != 0;
  fe29 p[4], q[4], s[4];
#pragma unroll
  for (int f = 0; f < 4; f++)
#pragma unroll
    for (int j = 0; j < 9; j++) {
      p[f].v[j] = x[9 * f + j];
      q[f].v[j] = y[9 * f + j];
      s[f].v[j] = 0;
    }
  if constexpr (OP == OP_ADD) {
    fe29_add(s[0], p[0], q[0]);
  } else if constexpr (OP == OP_SUB2) {
    fe29_sub<2>(s[0], p[0], q[0]);
  } else if constexpr (OP == OP_SUB3) {
    fe29_sub<3>(s[0], p[0], q[0]);
  } else if constexpr (OP == OP_SUB4) {
    fe29_sub<4>(s[0], p[0], q[0]);
  } else if constexpr (OP == OP_CARRY) {
    fe29_carry(s[0], p[0]);
  } else if constexpr (OP == OP_CSWAP) {
    fe29_cswap_to(s[0], s[1], p[0], q[0], c);
  } else if constexpr (OP == OP_DBL) {
    const ge29_p2 in = {p[0], p[1], p[2]};
    ge29_p1p1 o;
    ge29_p2_dbl(o, in);
    s[0] = o.X, s[1] = o.Y, s[2] = o.Z, s[3] = o.T;
  } else if constexpr (OP == OP_TO_P2) {
    const ge29_p1p1 in = {p[0], p[1], p[2], p[3]};
    ge29_p2 o;
    ge29_p1p1_to_p2(o, in);
    s[0] = o.X, s[1] = o.Y, s[2] = o.Z;
  } else if constexpr (OP == OP_TO_P3) {
    const ge29_p1p1 in = {p[0], p[1], p[2], p[3]};
    ge29_p3 o;
    ge29_p1p1_to_p3(o, in);
    s[0] = o.X, s[1] = o.Y, s[2] = o.Z, s[3] = o.T;
  } else if constexpr (OP == OP_ADD_PT) {
    const ge29_p3 in = {p[0], p[1], p[2], p[3]};
    const ge29_cached ad = {q[0], q[1], q[2], q[3]};
    ge29_p1p1 o;
    ge29_add(o, in, ad, c);
    s[0] = o.X, s[1] = o.Y, s[2] = o.Z, s[3] = o.T;
  } else if constexpr (OP == OP_P3_FROM) {
    ge_p3 in;
    fe* f[4] = {&in.X, &in.Y, &in.Z, &in.T};
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int j = 0; j < 8; j++) f[t]->v[j] = x[8 * t + j];
    ge29_p3 o;
    ge29_p3_from(o, in);
    s[0] = o.X, s[1] = o.Y, s[2] = o.Z, s[3] = o.T;
  } else if constexpr (OP == OP_P3_TO) {
    const ge29_p3 in = {p[0], p[1], p[2], p[3]};
    ge_p3 o;
    ge29_p3_to(o, in);
    const fe* f[4] = {&o.X, &o.Y, &o.Z, &o.T};
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int j = 0; j < 8; j++) r[8 * t + j] = f[t]->v[j];
  } else {  // OP_DIGIT: the consumer's whole digit, p2 in, the next digit's p2 out
    ge29_p2 acc2 = {p[0], p[1], p[2]};
    ge29_p3 acc3;
    ge29_p1p1 t;
    const ge29_cached ad = {q[0], q[1], q[2], q[3]};
#pragma unroll 1
    for (int d = 0; d < 3; d++) {
      ge29_p2_dbl(t, acc2);
      ge29_p1p1_to_p2(acc2, t);
    }
    ge29_p2_dbl(t, acc2);
    ge29_p1p1_to_p3(acc3, t);
    ge29_add(t, acc3, ad, c);
    ge29_p1p1_to_p2(acc2, t);
    s[0] = acc2.X, s[1] = acc2.Y, s[2] = acc2.Z;
  }
  if constexpr (OP != OP_P3_TO) {
#pragma unroll
    for (int f = 0; f < 4; f++) put(r, s[f], f);
  }
#pragma unroll
  for (int j = 0; j < NO; j++) out[(uint64_t)i * NO + j] = r[j];
}

template <int OP = 0>
hipError_t dispatch(int op, const uint32_t* a, const uint32_t* b, const uint32_t* flag, uint32_t n, uint32_t* out,
                    hipStream_t s) {
  if constexpr (OP < OP_COUNT) {
    if (op == OP) {
      hipLaunchKernelGGL(k<OP>, dim3((n + 255) / 256), dim3(256), 0, s, a, b, flag, n, out);
      return hipGetLastError();
    }
    return dispatch<OP + 1>(op, a, b, flag, n, out, s);
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace COA_G29_NS

extern "C" {

__attribute__((visibility("default"))) int COA_G29_RUN(int op, const uint32_t* d_a, const uint32_t* d_b,
                                                       const uint32_t* d_flag, uint32_t n, uint32_t* d_out,
                                                       void* stream) {
  if (op < 0 || op >= COA_G29_NS::OP_COUNT) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  return (int)COA_G29_NS::dispatch<>(op, d_a, d_b, d_flag, n, d_out, (hipStream_t)stream);
}

#ifndef COA_RARE_INLINE
int coa_ge29_run_inl(int op, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_flag, uint32_t n,
                     uint32_t* d_out, void* stream);

// Runs op on n items (device pointers: a, b and out hold words_a(op),
// words_b(op) and words_out(op) dwords per item, flag one dword per item: the
// swap / t2d_neg flag) on the current device and the given stream; returns the
// HIP error code.
__attribute__((visibility("default"))) int coa_ge29_run(int op, int rare_inline, const uint32_t* d_a,
                                                        const uint32_t* d_b, const uint32_t* d_flag, uint32_t n,
                                                        uint32_t* d_out, void* stream) {
  return rare_inline ? coa_ge29_run_inl(op, d_a, d_b, d_flag, n, d_out, stream)
                     : coa_ge29_run_out(op, d_a, d_b, d_flag, n, d_out, stream);
}
#endif

}  // extern "C"

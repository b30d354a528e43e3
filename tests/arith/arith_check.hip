// Test-only device library: every arithmetic primitive of csrc/coa_fe.h,
// coa_fe_wave.h, coa_sc.h, coa_halve.h and coa_ge.h behind a trivial kernel --
// one item per lane (one item per 16-lane row for the row forms), operands
// in, RAW output limbs out -- so that tests/test_gpu_arith.py can compare them
// with Python big integers.  The product headers are included unchanged.
//
// build.py compiles this file twice into lib/libcoa_arithcheck.so: as is (the
// rare carry blocks out of line, as in coa_kernels.hip / coa_halved.hip) and
// with -DCOA_RARE_INLINE (as in coa_latency.hip, coa_committee.hip, coa_cert_lat.hip
// and coa_keybuild.hip).  The
// two copies live in different namespaces and export coa_arith_run_out /
// coa_arith_run_inl; coa_arith_run picks one.  Not part of the C ABI of
// include/coa_verify.h.
//
// Blocks are 64 threads: one block is one wave, so the position of an item in
// the operand arrays is its position in the wave.  With a mask, an item whose
// mask byte is 0 skips the primitive inside a divergent `if` and gets the
// sentinel in every output word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coa_fe.h"
#include "coa_fe_wave.h"
#include "coa_ge.h"
#include "coa_halve.h"
#include "coa_sc.h"

#ifdef COA_RARE_INLINE
#define COA_AC_NS ac_inl
#define COA_AC_RUN coa_arith_run_inl
#else
#define COA_AC_NS ac_out
#define COA_AC_RUN coa_arith_run_out
#endif

#define COA_AC_SENTINEL 0xA5A5A5A5u

namespace COA_AC_NS {

// Keep in step with OPS of tests/arith_ref.py (coa_arith_dims is compared
// with it by the tests).
enum Op : int {
  OP_FE_ADD = 0, OP_FE_SUB, OP_FE_ADDSUB, OP_FE_NEG, OP_FE_MUL, OP_FE_SQ, OP_FE_MUL_N4, OP_FE_SQ_N4,
  OP_FE_REDUCE512, OP_FE_MUL_SMALL, OP_FE_FOLD_WORD, OP_FE_CANON, OP_FE_TO_WORDS, OP_FE_ISZERO, OP_FE_ISNEG,
  OP_FE_EQ, OP_FE_FROM_WORDS, OP_FE_POW_P58, OP_FE_INVERT, OP_FE_SQRT_RATIO,
  OP_FW_ADD, OP_FW_SUB, OP_FW_MUL, OP_FW_SQ, OP_FW_POW_P58, OP_FW_INVERT, OP_FW_SQRT_RATIO,
  OP_SC_IS_CANONICAL, OP_SC_REDUCE512, OP_SC_MULADD, OP_SC_MUL, OP_SC_ADD, OP_SC_NEG,
  OP_HALVE,
  OP_GE_ADD, OP_GE_SUB, OP_GE_MADD, OP_GE_P2_DBL, OP_GE_P3_DBL, OP_GE_ADD_IL, OP_GE_MADD_IL, OP_GE_P2_DBL_IL,
  OP_GE_P3_TO_CACHED, OP_GE_IS_SMALL_ORDER, OP_GE_P2_IS_IDENTITY, OP_GE_P2_EQ_P3, OP_GE_P2_COMPRESS,
  OP_GE_DECOMPRESS,
  OP_COUNT
};

struct Dims {
  int na, nb, nc, nout, rows;  // words per item of a, b, c and out; rows: one item per 16-lane row
};

__host__ __device__ constexpr Dims dims(int op) {
  switch (op) {
    case OP_FE_ADD: case OP_FE_SUB: case OP_FE_MUL: return {8, 8, 0, 8, 0};
    case OP_FE_ADDSUB: return {8, 8, 0, 16, 0};
    case OP_FE_NEG: case OP_FE_SQ: case OP_FE_CANON: case OP_FE_TO_WORDS: case OP_FE_FROM_WORDS:
    case OP_FE_POW_P58: case OP_FE_INVERT: return {8, 0, 0, 8, 0};
    case OP_FE_MUL_N4: case OP_FE_SQ_N4: return {8, 8, 8, 32, 0};
    case OP_FE_REDUCE512: return {16, 0, 0, 8, 0};
    case OP_FE_MUL_SMALL: case OP_FE_FOLD_WORD: return {8, 1, 0, 8, 0};
    case OP_FE_ISZERO: case OP_FE_ISNEG: return {8, 0, 0, 1, 0};
    case OP_FE_EQ: return {8, 8, 0, 1, 0};
    case OP_FE_SQRT_RATIO: return {8, 8, 0, 9, 0};
    case OP_FW_ADD: case OP_FW_SUB: case OP_FW_MUL: return {8, 8, 0, 8, 1};
    case OP_FW_SQ: case OP_FW_POW_P58: case OP_FW_INVERT: return {8, 0, 0, 8, 1};
    case OP_FW_SQRT_RATIO: return {8, 8, 0, 9, 1};
    case OP_SC_IS_CANONICAL: return {8, 0, 0, 1, 0};
    case OP_SC_REDUCE512: return {16, 0, 0, 8, 0};
    case OP_SC_MULADD: return {8, 8, 8, 8, 0};
    case OP_SC_MUL: case OP_SC_ADD: return {8, 8, 0, 8, 0};
    case OP_SC_NEG: return {8, 0, 0, 8, 0};
    case OP_HALVE: return {8, 0, 0, 18, 0};
    case OP_GE_ADD: case OP_GE_SUB: case OP_GE_ADD_IL: return {32, 32, 0, 32, 0};
    case OP_GE_MADD: case OP_GE_MADD_IL: return {32, 24, 0, 32, 0};
    case OP_GE_P2_DBL: case OP_GE_P3_DBL: case OP_GE_P2_DBL_IL: case OP_GE_P3_TO_CACHED: return {32, 0, 0, 32, 0};
    case OP_GE_IS_SMALL_ORDER: case OP_GE_P2_IS_IDENTITY: return {32, 0, 0, 1, 0};
    case OP_GE_P2_EQ_P3: return {32, 32, 0, 1, 0};
    case OP_GE_P2_COMPRESS: return {32, 0, 0, 8, 0};
    case OP_GE_DECOMPRESS: return {8, 0, 0, 25, 0};
    default: return {0, 0, 0, 0, 0};
  }
}

COA_DEV void ld_fe(fe& r, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
}
COA_DEV void st_fe(uint32_t* w, const fe& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = a.v[i];
}
COA_DEV void ld_p3(ge_p3& r, const uint32_t* w) {
  ld_fe(r.X, w);
  ld_fe(r.Y, w + 8);
  ld_fe(r.Z, w + 16);
  ld_fe(r.T, w + 24);
}
COA_DEV void st_p3(uint32_t* w, const ge_p3& p) {
  st_fe(w, p.X);
  st_fe(w + 8, p.Y);
  st_fe(w + 16, p.Z);
  st_fe(w + 24, p.T);
}
COA_DEV void ld_niels(ge_niels& r, const uint32_t* w) {
  ld_fe(r.yplusx, w);
  ld_fe(r.yminusx, w + 8);
  ld_fe(r.xy2d, w + 16);
}

// One item of op OP: A, B, C are the item's operand words, o its output.
template <int OP>
COA_DEV void run(const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t* o) {
  if constexpr (OP == OP_FE_ADD || OP == OP_FE_SUB || OP == OP_FE_MUL) {
    fe a, b, r;
    ld_fe(a, A);
    ld_fe(b, B);
    if constexpr (OP == OP_FE_ADD) fe_add(r, a, b);
    if constexpr (OP == OP_FE_SUB) fe_sub(r, a, b);
    if constexpr (OP == OP_FE_MUL) fe_mul(r, a, b);
    st_fe(o, r);
  } else if constexpr (OP == OP_FE_ADDSUB) {
    fe a, b, s, d;
    ld_fe(a, A);
    ld_fe(b, B);
    fe_addsub(s, d, a, b);
    st_fe(o, s);
    st_fe(o + 8, d);
  } else if constexpr (OP == OP_FE_NEG || OP == OP_FE_SQ || OP == OP_FE_CANON || OP == OP_FE_POW_P58 ||
                       OP == OP_FE_INVERT) {
    fe a, r;
    ld_fe(a, A);
    if constexpr (OP == OP_FE_NEG) fe_neg(r, a);
    if constexpr (OP == OP_FE_SQ) fe_sq(r, a);
    if constexpr (OP == OP_FE_CANON) fe_canon(r, a);
    if constexpr (OP == OP_FE_POW_P58) fe_pow_p58(r, a);
    if constexpr (OP == OP_FE_INVERT) fe_invert(r, a);
    st_fe(o, r);
  } else if constexpr (OP == OP_FE_MUL_N4) {  // a*b, b*c, c*a, b*b
    fe x[4], y[4], r[4];
    ld_fe(x[0], A); ld_fe(y[0], B);
    ld_fe(x[1], B); ld_fe(y[1], C);
    ld_fe(x[2], C); ld_fe(y[2], A);
    ld_fe(x[3], B); ld_fe(y[3], B);
    fe_mul_n<4>(r, x, y);
#pragma unroll
    for (int q = 0; q < 4; q++) st_fe(o + 8 * q, r[q]);
  } else if constexpr (OP == OP_FE_SQ_N4) {  // a^2, b^2, c^2, (a xor b)^2
    fe x[4], r[4];
    ld_fe(x[0], A);
    ld_fe(x[1], B);
    ld_fe(x[2], C);
#pragma unroll
    for (int i = 0; i < 8; i++) x[3].v[i] = A[i] ^ B[i];
    fe_sq_n<4>(r, x);
#pragma unroll
    for (int q = 0; q < 4; q++) st_fe(o + 8 * q, r[q]);
  } else if constexpr (OP == OP_FE_REDUCE512) {
    uint32_t t[16];
#pragma unroll
    for (int i = 0; i < 16; i++) t[i] = A[i];
    fe r;
    fe_reduce512(r, t);
    st_fe(o, r);
  } else if constexpr (OP == OP_FE_MUL_SMALL) {
    fe a, r;
    ld_fe(a, A);
    fe_mul_small(r, a, B[0]);
    st_fe(o, r);
  } else if constexpr (OP == OP_FE_FOLD_WORD) {
    fe r;
    ld_fe(r, A);
    fe_fold_word(r, B[0]);
    st_fe(o, r);
  } else if constexpr (OP == OP_FE_TO_WORDS) {
    fe a;
    ld_fe(a, A);
    fe_to_words(o, a);
  } else if constexpr (OP == OP_FE_ISZERO) {
    fe a;
    ld_fe(a, A);
    o[0] = fe_iszero(a) ? 1u : 0u;
  } else if constexpr (OP == OP_FE_ISNEG) {
    fe a;
    ld_fe(a, A);
    o[0] = fe_isneg(a);
  } else if constexpr (OP == OP_FE_EQ) {
    fe a, b;
    ld_fe(a, A);
    ld_fe(b, B);
    o[0] = fe_eq(a, b) ? 1u : 0u;
  } else if constexpr (OP == OP_FE_FROM_WORDS) {
    fe r;
    fe_from_words(r, A);
    st_fe(o, r);
  } else if constexpr (OP == OP_FE_SQRT_RATIO || OP == OP_FW_SQRT_RATIO) {
    fe u, v, r;
    ld_fe(u, A);
    ld_fe(v, B);
    const bool ok = fe_sqrt_ratio_i<OP == OP_FW_SQRT_RATIO>(r, u, v);
    o[0] = ok ? 1u : 0u;
    st_fe(o + 1, r);
  } else if constexpr (OP == OP_FW_ADD || OP == OP_FW_SUB || OP == OP_FW_MUL) {
    fe a, b, r;
    ld_fe(a, A);
    ld_fe(b, B);
    const uint32_t x = fw::from_fe(a), y = fw::from_fe(b);
    uint32_t z;
    if constexpr (OP == OP_FW_ADD) z = fw::add(x, y);
    if constexpr (OP == OP_FW_SUB) z = fw::sub(x, y);
    if constexpr (OP == OP_FW_MUL) z = fw::mul(x, y);
    fw::to_fe(r, z);
    st_fe(o, r);
  } else if constexpr (OP == OP_FW_SQ || OP == OP_FW_POW_P58 || OP == OP_FW_INVERT) {
    fe a, r;
    ld_fe(a, A);
    const uint32_t x = fw::from_fe(a);
    uint32_t z;
    if constexpr (OP == OP_FW_SQ) z = fw::sq(x);
    if constexpr (OP == OP_FW_POW_P58) z = fw::pow_p58(x);
    if constexpr (OP == OP_FW_INVERT) z = fw::invert(x);
    fw::to_fe(r, z);
    st_fe(o, r);
  } else if constexpr (OP == OP_SC_IS_CANONICAL) {
    o[0] = sc_is_canonical(A) ? 1u : 0u;
  } else if constexpr (OP == OP_SC_REDUCE512) {
    sc r;
    sc_reduce512(r, A);
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = r.v[i];
  } else if constexpr (OP == OP_SC_MULADD || OP == OP_SC_MUL || OP == OP_SC_ADD || OP == OP_SC_NEG) {
    sc r;
    if constexpr (OP == OP_SC_MULADD) sc_muladd(r, A, B, C);
    if constexpr (OP == OP_SC_MUL) sc_mul(r, A, B);
    if constexpr (OP == OP_SC_ADD) sc_add(r, A, B);
    if constexpr (OP == OP_SC_NEG) sc_neg(r, A);
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = r.v[i];
  } else if constexpr (OP == OP_HALVE) {
    uint32_t c[8], d[8];
    int cost;
    bool neg;
    coa_halve::halve(c, d, cost, neg, A);
#pragma unroll
    for (int i = 0; i < 8; i++) {
      o[i] = c[i];
      o[8 + i] = d[i];
    }
    o[16] = neg ? 1u : 0u;
    o[17] = (uint32_t)cost;
  } else if constexpr (OP == OP_GE_ADD || OP == OP_GE_SUB || OP == OP_GE_ADD_IL) {
    ge_p3 p, q, r;
    ge_cached c;
    ge_p1p1 t;
    ld_p3(p, A);
    ld_p3(q, B);
    ge_p3_to_cached(c, q);
    if constexpr (OP == OP_GE_ADD) ge_add(t, p, c);
    if constexpr (OP == OP_GE_SUB) ge_sub(t, p, c);
    if constexpr (OP == OP_GE_ADD_IL) {
      ge_add_il(t, p, c);
      ge_p1p1_to_p3_il(r, t);
    } else {
      ge_p1p1_to_p3(r, t);
    }
    st_p3(o, r);
  } else if constexpr (OP == OP_GE_MADD || OP == OP_GE_MADD_IL) {
    ge_p3 p, r;
    ge_niels q;
    ge_p1p1 t;
    ld_p3(p, A);
    ld_niels(q, B);
    if constexpr (OP == OP_GE_MADD) {
      ge_madd(t, p, q);
      ge_p1p1_to_p3(r, t);
    } else {
      ge_madd_il(t, p, q);
      ge_p1p1_to_p3_il(r, t);
    }
    st_p3(o, r);
  } else if constexpr (OP == OP_GE_P2_DBL || OP == OP_GE_P3_DBL || OP == OP_GE_P2_DBL_IL) {
    ge_p3 p, r;
    ge_p2 p2;
    ge_p1p1 t;
    ld_p3(p, A);
    ge_p3_to_p2(p2, p);
    if constexpr (OP == OP_GE_P2_DBL) ge_p2_dbl(t, p2);
    if constexpr (OP == OP_GE_P3_DBL) ge_p3_dbl(t, p);
    if constexpr (OP == OP_GE_P2_DBL_IL) {
      ge_p2_dbl_il(t, p2);
      ge_p1p1_to_p3_il(r, t);
    } else {
      ge_p1p1_to_p3(r, t);
    }
    st_p3(o, r);
  } else if constexpr (OP == OP_GE_P3_TO_CACHED) {
    ge_p3 p;
    ge_cached c;
    ld_p3(p, A);
    ge_p3_to_cached(c, p);
    st_fe(o, c.YplusX);
    st_fe(o + 8, c.YminusX);
    st_fe(o + 16, c.Z);
    st_fe(o + 24, c.T2d);
  } else if constexpr (OP == OP_GE_IS_SMALL_ORDER) {
    ge_p3 p;
    ld_p3(p, A);
    o[0] = ge_is_small_order(p) ? 1u : 0u;
  } else if constexpr (OP == OP_GE_P2_IS_IDENTITY) {
    ge_p3 p;
    ge_p2 p2;
    ld_p3(p, A);
    ge_p3_to_p2(p2, p);
    o[0] = ge_p2_is_identity(p2) ? 1u : 0u;
  } else if constexpr (OP == OP_GE_P2_EQ_P3) {
    ge_p3 p, q;
    ge_p2 p2;
    ld_p3(p, A);
    ld_p3(q, B);
    ge_p3_to_p2(p2, p);
    o[0] = ge_p2_eq_p3(p2, q) ? 1u : 0u;
  } else if constexpr (OP == OP_GE_P2_COMPRESS) {
    ge_p3 p;
    ge_p2 p2;
    ld_p3(p, A);
    ge_p3_to_p2(p2, p);
    ge_p2_compress(o, p2);
  } else if constexpr (OP == OP_GE_DECOMPRESS) {
    ge_p3 r;
    const bool ok = ge_decompress<false>(r, A);
    o[0] = ok ? 1u : 0u;
    st_fe(o + 1, r.X);
    st_fe(o + 9, r.Y);
    st_fe(o + 17, r.T);
  }
}

// One item per lane, or (rows ops) one item per 16-lane row: every lane of
// the row loads the row's operands and runs the primitive, lane 0 of the row
// stores.  Items past n and rows past n leave together (a whole row sits out).
template <int OP>
__global__ void __launch_bounds__(64) k_arith(const uint32_t* __restrict__ d_a, const uint32_t* __restrict__ d_b,
                                              const uint32_t* __restrict__ d_c, const uint8_t* __restrict__ d_mask,
                                              uint32_t n, uint32_t* __restrict__ d_out) {
  constexpr Dims D = dims(OP);
  const uint32_t gid = blockIdx.x * 64u + threadIdx.x;
  const uint32_t i = D.rows ? gid >> 4 : gid;
  if (i >= n) return;
  uint32_t A[D.na > 0 ? D.na : 1], B[D.nb > 0 ? D.nb : 1], C[D.nc > 0 ? D.nc : 1], o[D.nout];
#pragma unroll
  for (int k = 0; k < D.na; k++) A[k] = d_a[(uint64_t)i * D.na + k];
#pragma unroll
  for (int k = 0; k < D.nb; k++) B[k] = d_b[(uint64_t)i * D.nb + k];
#pragma unroll
  for (int k = 0; k < D.nc; k++) C[k] = d_c[(uint64_t)i * D.nc + k];
  const bool on = d_mask ? d_mask[i] != 0 : true;
  const bool writer = !D.rows || (gid & 15u) == 0u;
  uint32_t* dst = d_out + (uint64_t)i * D.nout;
  // Each side of the branch stores its own words.  (With one store after the
  // join, hipcc's merge of the loaded words with the sentinel constant lost
  // word 6 of the pure copy fe_from_words: the mask byte and the constant were
  // put in the register that still held the operand word.)
  if (on) {
    run<OP>(A, B, C, o);
    if (writer) {
#pragma unroll
      for (int k = 0; k < D.nout; k++) dst[k] = o[k];
    }
  } else if (writer) {
#pragma unroll
    for (int k = 0; k < D.nout; k++) dst[k] = COA_AC_SENTINEL;
  }
}

template <int OP>
hipError_t launch(const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint8_t* m, uint32_t n, uint32_t* out,
                  hipStream_t s) {
  constexpr Dims D = dims(OP);
  const uint64_t threads = (uint64_t)n * (D.rows ? 16u : 1u);
  const uint32_t blocks = (uint32_t)((threads + 63u) / 64u);
  hipLaunchKernelGGL(k_arith<OP>, dim3(blocks), dim3(64), 0, s, a, b, c, m, n, out);
  return hipGetLastError();
}

template <int OP = 0>
hipError_t dispatch(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint8_t* m, uint32_t n,
                    uint32_t* out, hipStream_t s) {
  if constexpr (OP < OP_COUNT) {
    if (op == OP) return launch<OP>(a, b, c, m, n, out, s);
    return dispatch<OP + 1>(op, a, b, c, m, n, out, s);
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace COA_AC_NS

extern "C" {

__attribute__((visibility("default"))) int COA_AC_RUN(int op, const uint32_t* d_a, const uint32_t* d_b,
                                                      const uint32_t* d_c, const uint8_t* d_mask, uint32_t n,
                                                      uint32_t* d_out, void* stream) {
  if (op < 0 || op >= COA_AC_NS::OP_COUNT) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  return (int)COA_AC_NS::dispatch<>(op, d_a, d_b, d_c, d_mask, n, d_out, (hipStream_t)stream);
}

#ifndef COA_RARE_INLINE
int coa_arith_run_inl(int op, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, const uint8_t* d_mask,
                      uint32_t n, uint32_t* d_out, void* stream);

// Runs op on n items (device pointers; the current device, the given stream)
// and returns the HIP error code.  rare_inline picks the COA_RARE_INLINE copy.
__attribute__((visibility("default"))) int coa_arith_run(int op, int rare_inline, const uint32_t* d_a,
                                                         const uint32_t* d_b, const uint32_t* d_c,
                                                         const uint8_t* d_mask, uint32_t n, uint32_t* d_out,
                                                         void* stream) {
  return rare_inline ? coa_arith_run_inl(op, d_a, d_b, d_c, d_mask, n, d_out, stream)
                     : coa_arith_run_out(op, d_a, d_b, d_c, d_mask, n, d_out, stream);
}

// {na, nb, nc, nout, rows} of op into out5; 0 on success.
__attribute__((visibility("default"))) int coa_arith_dims(int op, int* out5) {
  if (op < 0 || op >= COA_AC_NS::OP_COUNT) return 1;
  const COA_AC_NS::Dims d = COA_AC_NS::dims(op);
  out5[0] = d.na;
  out5[1] = d.nb;
  out5[2] = d.nc;
  out5[3] = d.nout;
  out5[4] = d.rows;
  return 0;
}

__attribute__((visibility("default"))) int coa_arith_op_count(void) { return COA_AC_NS::OP_COUNT; }
#endif

}  // extern "C"

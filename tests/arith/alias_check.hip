// Test-only device library, beside arith_check.hip: the call forms of
// csrc/coa_fe.h's out-of-place fe_add / fe_sub / fe_addsub in which a result
// aliases an operand, and the signed table lookups of csrc/coa_smul.h
// (tab2_build / tab2_load) feeding ge_add / ge_add_il -- one item
// per lane, operands in, RAW output limbs out, for tests/test_gpu_alias.py.
//
// Each field op runs `reps` times in a loop the compiler may not unroll, so
// the aliased result really is the next pass's operand (a register carried
// round the loop), as fe_add(b, b, b) is in the doubling loop of
// k_verify_main.
//
// build.py compiles this file twice into lib/libcoa_aliascheck.so, as is and
// with -DCOA_RARE_INLINE (both assembled forms of the rare carry blocks);
// coa_alias_run picks one.  Blocks are 64 threads (one wave); an item whose
// mask byte is 0 skips the primitive inside a divergent `if` and gets the
// sentinel in every output word.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "coa_fe.h"
#include "coa_ge.h"
#include "coa_smul.h"

#ifdef COA_RARE_INLINE
#define COA_AL_NS al_inl
#define COA_AL_RUN coa_alias_run_inl
#else
#define COA_AL_NS al_out
#define COA_AL_RUN coa_alias_run_out
#endif

#define COA_AL_SENTINEL 0xA5A5A5A5u
// words of table slab per item (two tables of 8 cached entries)
#define COA_AL_SLAB_WORDS (COA_HALVED_SCRATCH_PER_LANE / 4)

namespace COA_AL_NS {

// Keep in step with OPS of tests/test_gpu_alias.py.
enum Op : int {
  OP_ADD_RA = 0,     // r = a;        r = r + b
  OP_ADD_RB,         // r = b;        r = a + r
  OP_ADD_AAA,        // r = a;        r = r + r
  OP_SUB_RA,         // r = a;        r = r - b
  OP_SUB_RB,         // r = b;        r = a - r
  OP_SUB_AAA,        // r = a;        r = r - r
  OP_ADDSUB_SA,      // s = a;        (s, d) = (s + b, s - b)
  OP_ADDSUB_SB,      // s = b;        (s, d) = (a + s, a - s)
  OP_ADDSUB_DA,      // d = a;        (s, d) = (d + b, d - b)
  OP_ADDSUB_DB,      // d = b;        (s, d) = (a + d, a - d)
  OP_ADDSUB_SADB,    // s = a, d = b; (s, d) = (s + d, s - d)
  OP_TAB_ADD,        // p + digit * q through the slab table of q, ge_add
  OP_TAB_ADD_IL,     // the same through ge_add_il
  OP_COUNT
};

struct Dims {
  int na, nb, nc, nout;
};

__host__ __device__ constexpr Dims dims(int op) {
  if (op <= OP_SUB_AAA) return {8, 8, 0, 8};
  if (op <= OP_ADDSUB_SADB) return {8, 8, 0, 16};
  if (op <= OP_TAB_ADD_IL) return {32, 16, 1, 32};  // p (X, Y, Z, T), affine q (x, y), digit + 8
  return {0, 0, 0, 0};
}

COA_DEV void ld_fe(fe& r, const uint32_t* w) {
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = w[i];
}
COA_DEV void st_fe(uint32_t* w, const fe& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = a.v[i];
}

template <int OP>
COA_DEV void run(const uint32_t* A, const uint32_t* B, const uint32_t* C, uint32_t* o, int reps, uint32_t* scr,
                 uint32_t item) {
  if constexpr (OP <= OP_SUB_AAA) {
    fe a, b, r;
    ld_fe(a, A);
    ld_fe(b, B);
    r = (OP == OP_ADD_RB || OP == OP_SUB_RB) ? b : a;
#pragma unroll 1
    for (int k = 0; k < reps; k++) {
      if constexpr (OP == OP_ADD_RA) fe_add(r, r, b);
      if constexpr (OP == OP_ADD_RB) fe_add(r, a, r);
      if constexpr (OP == OP_ADD_AAA) fe_add(r, r, r);
      if constexpr (OP == OP_SUB_RA) fe_sub(r, r, b);
      if constexpr (OP == OP_SUB_RB) fe_sub(r, a, r);
      if constexpr (OP == OP_SUB_AAA) fe_sub(r, r, r);
    }
    st_fe(o, r);
  } else if constexpr (OP <= OP_ADDSUB_SADB) {
    fe a, b, s, d;
    ld_fe(a, A);
    ld_fe(b, B);
    s = OP == OP_ADDSUB_SB ? b : a;
    d = OP == OP_ADDSUB_DA ? a : b;
#pragma unroll 1
    for (int k = 0; k < reps; k++) {
      if constexpr (OP == OP_ADDSUB_SA) fe_addsub(s, d, s, b);
      if constexpr (OP == OP_ADDSUB_SB) fe_addsub(s, d, a, s);
      if constexpr (OP == OP_ADDSUB_DA) fe_addsub(s, d, d, b);
      if constexpr (OP == OP_ADDSUB_DB) fe_addsub(s, d, a, d);
      if constexpr (OP == OP_ADDSUB_SADB) fe_addsub(s, d, s, d);
    }
    st_fe(o, s);
    st_fe(o + 8, d);
  } else {
    ge_p3 p, q, r;
    ld_fe(p.X, A);
    ld_fe(p.Y, A + 8);
    ld_fe(p.Z, A + 16);
    ld_fe(p.T, A + 24);
    ld_fe(q.X, B);
    ld_fe(q.Y, B + 8);
    fe_set(q.Z, 1);
    fe_mul(q.T, q.X, q.Y);
    const int tab = (int)(item & 1u);  // both tables of the slab, by item
    tab2_build(scr, item, tab, q);
    const int d = (int)C[0] - 8;
    ge_cached c;
    ge_p1p1 t;
    tab2_load(c, scr, item, tab, d);
    if constexpr (OP == OP_TAB_ADD) {
      ge_add(t, p, c, d < 0);
      ge_p1p1_to_p3(r, t);
    } else {
      ge_add_il(t, p, c, d < 0);
      ge_p1p1_to_p3_il(r, t);
    }
    st_fe(o, r.X);
    st_fe(o + 8, r.Y);
    st_fe(o + 16, r.Z);
    st_fe(o + 24, r.T);
  }
}

template <int OP>
__global__ void __launch_bounds__(64) k_alias(const uint32_t* __restrict__ d_a, const uint32_t* __restrict__ d_b,
                                              const uint32_t* __restrict__ d_c, const uint8_t* __restrict__ d_mask,
                                              uint32_t n, int reps, uint32_t* __restrict__ d_scr,
                                              uint32_t* __restrict__ d_out) {
  constexpr Dims D = dims(OP);
  const uint32_t i = blockIdx.x * 64u + threadIdx.x;
  if (i >= n) return;
  uint32_t A[D.na], B[D.nb], C[D.nc > 0 ? D.nc : 1], o[D.nout];
#pragma unroll
  for (int k = 0; k < D.na; k++) A[k] = d_a[(uint64_t)i * D.na + k];
#pragma unroll
  for (int k = 0; k < D.nb; k++) B[k] = d_b[(uint64_t)i * D.nb + k];
#pragma unroll
  for (int k = 0; k < D.nc; k++) C[k] = d_c[(uint64_t)i * D.nc + k];
  const bool on = d_mask ? d_mask[i] != 0 : true;
  uint32_t* dst = d_out + (uint64_t)i * D.nout;
  // each side of the branch stores its own words (see arith_check.hip)
  if (on) {
    run<OP>(A, B, C, o, reps, d_scr, i);
#pragma unroll
    for (int k = 0; k < D.nout; k++) dst[k] = o[k];
  } else {
#pragma unroll
    for (int k = 0; k < D.nout; k++) dst[k] = COA_AL_SENTINEL;
  }
}

template <int OP = 0>
hipError_t dispatch(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint8_t* m, uint32_t n,
                    int reps, uint32_t* scr, uint32_t* out, hipStream_t s) {
  if constexpr (OP < OP_COUNT) {
    if (op == OP) {
      hipLaunchKernelGGL(k_alias<OP>, dim3((n + 63u) / 64u), dim3(64), 0, s, a, b, c, m, n, reps, scr, out);
      return hipGetLastError();
    }
    return dispatch<OP + 1>(op, a, b, c, m, n, reps, scr, out, s);
  } else {
    return hipErrorInvalidValue;
  }
}

}  // namespace COA_AL_NS

extern "C" {

__attribute__((visibility("default"))) int COA_AL_RUN(int op, const uint32_t* d_a, const uint32_t* d_b,
                                                      const uint32_t* d_c, const uint8_t* d_mask, uint32_t n,
                                                      int reps, uint32_t* d_scr, uint32_t* d_out, void* stream) {
  if (op < 0 || op >= COA_AL_NS::OP_COUNT || reps < 1) return (int)hipErrorInvalidValue;
  // the table ops write n slabs of COA_AL_SLAB_WORDS words at d_scr
  if (op >= COA_AL_NS::OP_TAB_ADD && (!d_scr || !d_c)) return (int)hipErrorInvalidValue;
  if (n == 0) return (int)hipSuccess;
  return (int)COA_AL_NS::dispatch<>(op, d_a, d_b, d_c, d_mask, n, reps, d_scr, d_out, (hipStream_t)stream);
}

#ifndef COA_RARE_INLINE
int coa_alias_run_inl(int op, const uint32_t* d_a, const uint32_t* d_b, const uint32_t* d_c, const uint8_t* d_mask,
                      uint32_t n, int reps, uint32_t* d_scr, uint32_t* d_out, void* stream);

// Runs op on n items (device pointers; the current device, the given stream)
// and returns the HIP error code.  rare_inline picks the COA_RARE_INLINE copy.
__attribute__((visibility("default"))) int coa_alias_run(int op, int rare_inline, const uint32_t* d_a,
                                                         const uint32_t* d_b, const uint32_t* d_c,
                                                         const uint8_t* d_mask, uint32_t n, int reps,
                                                         uint32_t* d_scr, uint32_t* d_out, void* stream) {
  return rare_inline ? coa_alias_run_inl(op, d_a, d_b, d_c, d_mask, n, reps, d_scr, d_out, stream)
                     : coa_alias_run_out(op, d_a, d_b, d_c, d_mask, n, reps, d_scr, d_out, stream);
}

__attribute__((visibility("default"))) int coa_alias_op_count(void) { return COA_AL_NS::OP_COUNT; }
__attribute__((visibility("default"))) int coa_alias_slab_words(void) { return COA_AL_SLAB_WORDS; }
#endif

}  // extern "C"

// Batch (random-linear-combination) verification for gfx950:
// crypto::Signature::verify_batch (crypto/src/lib.rs:206-219) ->
// ed25519-dalek 1.0.1 verify_batch.  One group = one certificate
// (Certificate::verify, primary/src/messages.rs:214).
//
// For a group with votes (A_i, R_i, s_i) over message M and weights z_i:
//   Ok  iff  every s_i < l, every A_i and R_i decompresses, and
//            [-(sum z_i s_i mod l)]B + sum [z_i]R_i + sum [z_i h_i mod l]A_i == O
//   with h_i = H(R_i || A_i || M) mod l.  No small-order rejection, no
//   cofactor -- exactly dalek.  The sum is computed exactly over the group,
//   so with the same z_i the verdict equals dalek's bit for bit, torsion
//   components included.
//
// Kernels:
//   k_batch_z       z_i = SHA-512("coa-batch-z" || seed || group || i || h_i || s_i)[0..16)
//   k_batch_terms   one lane per vote: validity flag and
//                   P_i = [z_i]R_i + [z_i h_i mod l]A_i + [-(z_i s_i) mod l]B
//                   by one joint Horner pass (signed radix-16 digits over two
//                   per-lane tables, signed radix-256 digits of the B scalar
//                   from the LDS B table); summing P_i over the group gives
//                   dalek's multiscalar sum term for term
//   k_batch_reduce  one workgroup per group: sum P_i (LDS tree), identity
//                   test, AND of the validity flags
#include "coa_batch_dev.h"

__global__ void __launch_bounds__(256) k_batch_z(const uint32_t* __restrict__ kbuf, const uint8_t* __restrict__ sigs,
                                                 const uint32_t* __restrict__ group_of, uint32_t group_const,
                                                 uint32_t n, uint64_t seed, uint32_t* __restrict__ zs) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    uint32_t z[4];
    coa_batch::z_derive(z, seed, group_of ? group_of[i] : group_const, i, kbuf + (uint64_t)i * 8,
                        reinterpret_cast<const uint32_t*>(sigs + (uint64_t)i * 64 + 32));
#pragma unroll
    for (int j = 0; j < 4; j++) zs[(uint64_t)i * 4 + j] = z[j];
  }
}

// Per vote: flag (1 = valid encoding), P = [z]R + [z·h mod l]A + [-(z·s) mod l]B
// (coa_batch::term); vote i's bytes and slot are at index i of every array.
__global__ void __launch_bounds__(BATCH_BLOCK, 2) k_batch_terms(const uint8_t* __restrict__ pks,
                                                             const uint8_t* __restrict__ sigs,
                                                             const uint32_t* __restrict__ kbuf,
                                                             const uint32_t* __restrict__ zs, uint32_t n,
                                                             uint32_t* __restrict__ terms, uint8_t* __restrict__ flags,
                                                             uint32_t* __restrict__ scr,
                                                             const uint32_t* __restrict__ btab_g) {
  __shared__ __attribute__((aligned(16))) uint32_t btab[COA_BTAB_DWORDS];
  coa_batch::btab_load(btab, btab_g);
  const uint32_t lanes = gridDim.x * blockDim.x;
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x;
  for (uint32_t i = lane; i < n; i += lanes)
    coa_batch::term(pks, sigs, i, kbuf, zs, i, terms, flags, scr, lanes, lane, btab);
}

// One workgroup per group: sum of the P_i, identity test, AND of the flags.
__global__ void __launch_bounds__(BATCH_BLOCK) k_batch_reduce(const uint64_t* __restrict__ offs,
                                                              const uint32_t* __restrict__ terms,
                                                              const uint8_t* __restrict__ flags,
                                                              uint8_t* __restrict__ verdicts) {
  __shared__ __attribute__((aligned(16))) uint32_t pts[BATCH_BLOCK * 32];
  __shared__ int bad;
  const uint32_t g = blockIdx.x;
  const bool ok = coa_batch::group_ok(offs[g], offs[g + 1], terms, flags, pts, &bad);
  if (threadIdx.x == 0) verdicts[g] = ok ? 0 : 1;
}

hipError_t coa_launch_batch_z(const uint32_t* kbuf, const uint8_t* sigs, const uint32_t* group_of,
                              uint32_t group_const, uint32_t n, uint64_t seed, uint32_t* zs, hipStream_t s) {
  if (n == 0) return hipSuccess;
  uint32_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_batch_z, dim3(blocks), dim3(256), 0, s, kbuf, sigs, group_of, group_const, n, seed, zs);
  return hipGetLastError();
}

hipError_t coa_launch_batch_terms(const uint8_t* pks, const uint8_t* sigs, const uint32_t* kbuf, const uint32_t* zs,
                                  uint32_t n, uint32_t* terms, uint8_t* flags, uint32_t* scratch,
                                  uint32_t scratch_lanes, const uint32_t* btab, hipStream_t s) {
  if (n == 0) return hipSuccess;
  uint64_t blocks = (n + BATCH_BLOCK - 1) / BATCH_BLOCK;
  const uint64_t maxb = scratch_lanes / BATCH_BLOCK;
  if (blocks > maxb) blocks = maxb;
  hipLaunchKernelGGL(k_batch_terms, dim3((uint32_t)blocks), dim3(BATCH_BLOCK), 0, s, pks, sigs, kbuf, zs, n, terms,
                     flags, scratch, btab);
  return hipGetLastError();
}

hipError_t coa_launch_batch_reduce(const uint64_t* offs, uint32_t n_groups, const uint32_t* terms,
                                   const uint8_t* flags, uint8_t* verdicts, hipStream_t s) {
  if (n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(k_batch_reduce, dim3(n_groups), dim3(BATCH_BLOCK), 0, s, offs, terms, flags, verdicts);
  return hipGetLastError();
}

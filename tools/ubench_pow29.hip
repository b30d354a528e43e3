// The whole x -> x^((p-5)/8) chain (251 squarings + 11 multiplications) as
// fe_pow_p58 (radix 2^32 comba, coa_fe.h) and as fe_pow_p58_29 (nine
// carry-free 29-bit limbs, coa_fe_pow29.h), at 1, 2 and 3 waves per SIMD:
// SIMD cycles per chain, i.e. time * clock / (waves per SIMD * chains per
// lane).  Every lane of both forms is checked against a host big-integer
// square-and-multiply on edge operands and random ones, and every timed
// launch against that checked result.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffunction-sections -I xrpl-coa-prototype_amd/csrc \
//       tools/ubench_pow29.hip -o tools/ubench_pow29
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "coa_fe_pow29.h"

// V = 0: fe_pow_p58, V = 1: fe_pow_p58_29; reps chains per lane, each fed the
// one before.  Lane i reads operand i mod m and stores its canonical result.
template <int V>
__global__ void __launch_bounds__(256, 3) k(const fe* __restrict__ x, fe* __restrict__ y, int m, int reps) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  fe a = x[id % m];
#pragma unroll 1
  for (int r = 0; r < reps; r++) {
    if (V == 0) fe_pow_p58(a, a);
    else fe_pow_p58_29(a, a);
  }
  fe_canon(a, a);
  y[id] = a;
}

// ------------------------------------------------------------ host model
typedef unsigned __int128 u128;
struct H {
  uint64_t w[4];
};
static const uint64_t P[4] = {0xffffffffffffffedull, ~0ull, ~0ull, 0x7fffffffffffffffull};
static void modp(uint64_t x[5]) {  // x < 2^320 -> x mod p
  for (int rep = 0; rep < 4; rep++) {
    uint64_t hi[3] = {(x[3] >> 63) | (x[4] << 1), x[4] >> 63, 0};
    x[3] &= 0x7fffffffffffffffull;
    x[4] = 0;
    u128 c = 0;
    for (int k = 0; k < 5; k++) {
      c += (u128)x[k] + (k < 3 ? (u128)hi[k] * 19 : 0);
      x[k] = (uint64_t)c;
      c >>= 64;
    }
  }
  bool ge = true;
  for (int k = 3; k >= 0; k--)
    if (x[k] != P[k]) {
      ge = x[k] > P[k];
      break;
    }
  if (ge) {
    uint64_t b = 0;
    for (int k = 0; k < 4; k++) {
      u128 d = (u128)x[k] - P[k] - b;
      x[k] = (uint64_t)d;
      b = (d >> 64) ? 1 : 0;
    }
  }
}
static H mulmod(const H& a, const H& b) {
  uint64_t prod[9] = {0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)a.w[i] * b.w[j] + prod[i + j];
      prod[i + j] = (uint64_t)c;
      c >>= 64;
    }
    prod[i + 4] += (uint64_t)c;
  }
  uint64_t x[5] = {0};
  u128 c = 0;
  for (int k = 0; k < 4; k++) {
    c += (u128)prod[k] + (u128)prod[k + 4] * 38;
    x[k] = (uint64_t)c;
    c >>= 64;
  }
  x[4] = (uint64_t)c;
  modp(x);
  H r;
  memcpy(r.w, x, 32);
  return r;
}
static H pow_p58_host(const fe& z) {  // z^(2^252 - 3) by plain square-and-multiply, canonical
  uint64_t x[5] = {0};
  for (int i = 0; i < 4; i++) x[i] = (uint64_t)z.v[2 * i] | ((uint64_t)z.v[2 * i + 1] << 32);
  modp(x);
  H b;
  memcpy(b.w, x, 32);
  // 2^252 - 3 = 0b111...101 (252 bits: 249 ones, then 1 0 1)
  H r = b;
  for (int bit = 250; bit >= 0; bit--) {
    r = mulmod(r, r);
    if (bit != 1) r = mulmod(r, b);
  }
  return r;
}

int main() {
  const int M = 16384;  // distinct operands
  fe* h0 = (fe*)malloc(sizeof(fe) * M);
  uint64_t s = 88172645463325252ull;
  for (int i = 0; i < M; i++)
    for (int j = 0; j < 8; j++) {
      s ^= s << 13;
      s ^= s >> 7;
      s ^= s << 17;
      h0[i].v[j] = (uint32_t)s;
    }
  // edge operands: 0, 1, 2, p-1, p, p+1, 2^255-1, 2^256-1, every 29-bit limb
  // full (2^256-1 again), one set bit at each position
  const uint32_t edge[8][2] = {{0, 0}, {1, 0}, {2, 0}, {0xffffffecu, 1}, {0xffffffedu, 1}, {0xffffffeeu, 1},
                               {0xffffffffu, 1}, {0xffffffffu, 2}};
  for (int e = 0; e < 8; e++)
    for (int j = 0; j < 8; j++)
      h0[e].v[j] = j == 0 ? edge[e][0] : edge[e][1] == 0 ? 0 : (j == 7 && edge[e][1] == 1 ? 0x7fffffffu : 0xffffffffu);
  for (int b = 0; b < 256; b++)
    for (int j = 0; j < 8; j++) h0[8 + b].v[j] = j == b / 32 ? 1u << (b % 32) : 0;
  H* want = (H*)malloc(sizeof(H) * M);
  for (int i = 0; i < M; i++) want[i] = pow_p58_host(h0[i]);

  fe *dx, *dy;
  const int maxthreads = 256 * 3 * 256;
  hipMalloc(&dx, sizeof(fe) * M);
  hipMalloc(&dy, sizeof(fe) * maxthreads);
  fe* got = (fe*)malloc(sizeof(fe) * maxthreads);
  hipMemcpy(dx, h0, sizeof(fe) * M, hipMemcpyHostToDevice);
  void (*ks[2])(const fe*, fe*, int, int) = {k<0>, k<1>};
  const char* names[2] = {"fe_pow_p58    (radix 2^32)", "fe_pow_p58_29 (9 x 29 bits)"};
  int bad = 0;
  for (int v = 0; v < 2; v++) {
    hipLaunchKernelGGL(ks[v], dim3(M / 256), dim3(256), 0, 0, dx, dy, M, 1);
    if (hipMemcpy(got, dy, sizeof(fe) * M, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    int b = 0;
    for (int i = 0; i < M; i++) b += memcmp(&got[i], &want[i], 32) != 0;
    printf("%s one chain vs host big integers: %d of %d lanes differ\n", names[v], b, M);
    bad += b;
  }
  if (bad) return 1;
  // expected result of REPS chains, from the checked one-chain kernel
  const int REPS = 8;
  fe* ref = (fe*)malloc(sizeof(fe) * M);
  hipLaunchKernelGGL(ks[0], dim3(M / 256), dim3(256), 0, 0, dx, dy, M, REPS);
  hipMemcpy(ref, dy, sizeof(fe) * M, hipMemcpyDeviceToHost);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  double cyc[2][4];
  for (int waves = 1; waves <= 3; waves++)
    for (int v = 0; v < 2; v++) {
      const int blocks = 256 * waves;
      hipLaunchKernelGGL(ks[v], dim3(blocks), dim3(256), 0, 0, dx, dy, M, 1);
      hipDeviceSynchronize();
      float best = 1e30f;
      for (int r = 0; r < 5; r++) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(ks[v], dim3(blocks), dim3(256), 0, 0, dx, dy, M, REPS);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < best) best = ms;
      }
      hipMemcpy(got, dy, sizeof(fe) * blocks * 256, hipMemcpyDeviceToHost);
      int b = 0;
      for (int i = 0; i < blocks * 256; i++) b += memcmp(&got[i], &ref[i % M], 32) != 0;
      cyc[v][waves] = (best * 1e-3) * 2.4e9 / (waves * REPS);
      printf("%d wave/SIMD %s %9.0f SIMD cycles per chain @2.4GHz (%.1f per field op), %d lanes differ\n", waves,
             names[v], cyc[v][waves], cyc[v][waves] / 262.0, b);
      bad += b;
    }
  for (int waves = 1; waves <= 3; waves++)
    printf("%d wave/SIMD: 29-bit chain %+.1f %% SIMD cycles against fe_pow_p58\n", waves,
           100.0 * (cyc[1][waves] / cyc[0][waves] - 1.0));
  return bad ? 1 : 0;
}

// One Horner digit of k_verify_main_sums' consumer -- four doublings, the last
// into p3, one addition of a cached operand, the conversion back to p2 -- on
// the radix-2^32 field as the kernel runs it today (the *_il forms of
// coa_ge.h) and on nine carry-free 29-bit limbs (coa_ge29.h), at 1 and 2
// waves per SIMD: SIMD cycles per digit, i.e. time * clock / (waves per SIMD *
// digits per lane).  The cached operand is read from memory at every digit,
// as the kernel reads it from LDS.  Every lane of every launch, timed ones
// included, is checked against the same formulas on host big integers before
// any time is printed.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffunction-sections -I xrpl-coa-prototype_amd/csrc \
//       tools/ubench_ge29.hip -o tools/ubench_ge29
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "coa_ge29.h"

struct In {  // per operand: the accumulator (X, Y, Z) and two cached addends (Y+X, Y-X, Z, 2dT)
  fe acc[3];
  fe q[2][4];
};
struct Out {
  fe c[3];  // canonical X, Y, Z
};

// V = 0: radix 2^32, V = 1: 29-bit limbs; digits Horner digits per lane, each
// on the result of the one before.  Digit r adds addend r & 1, taken negated
// (t2d_neg) when r & 2.
template <int V>
__global__ void __launch_bounds__(256, 2) k(const In* __restrict__ x, Out* __restrict__ y, int m, int digits) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  const In* in = x + id % m;
  Out o;
  if constexpr (V == 0) {
    ge_p2 acc2 = {in->acc[0], in->acc[1], in->acc[2]};
    ge_p3 acc3;
    ge_p1p1 t;
#pragma unroll 1
    for (int r = 0; r < digits; r++) {
      const fe* f = in->q[r & 1];
      const ge_cached q = {f[0], f[1], f[2], f[3]};
#pragma unroll 1
      for (int j = 0; j < 3; j++) {
        ge_p2_dbl_il(t, acc2);
        ge_p1p1_to_p2_il(acc2, t);
      }
      ge_p2_dbl_il(t, acc2);
      ge_p1p1_to_p3_il(acc3, t);
      ge_add_il(t, acc3, q, (r & 2) != 0);
      ge_p1p1_to_p2_il(acc2, t);
    }
    fe_canon(o.c[0], acc2.X);
    fe_canon(o.c[1], acc2.Y);
    fe_canon(o.c[2], acc2.Z);
  } else {
    ge29_p2 acc2;
    ge29_p3 acc3;
    ge29_p1p1 t;
    fe29_from_fe(acc2.X, in->acc[0]);
    fe29_from_fe(acc2.Y, in->acc[1]);
    fe29_from_fe(acc2.Z, in->acc[2]);
#pragma unroll 1
    for (int r = 0; r < digits; r++) {
      const fe29* f = reinterpret_cast<const fe29*>(y + (size_t)gridDim.x * blockDim.x) + (size_t)(id % m) * 8 + 4 * (r & 1);
      const ge29_cached q = {f[0], f[1], f[2], f[3]};
#pragma unroll 1
      for (int j = 0; j < 3; j++) {
        ge29_p2_dbl(t, acc2);
        ge29_p1p1_to_p2(acc2, t);
      }
      ge29_p2_dbl(t, acc2);
      ge29_p1p1_to_p3(acc3, t);
      ge29_add(t, acc3, q, (r & 2) != 0);
      ge29_p1p1_to_p2(acc2, t);
    }
    fe a;
    fe29_to_fe(a, acc2.X);
    fe_canon(o.c[0], a);
    fe29_to_fe(a, acc2.Y);
    fe_canon(o.c[1], a);
    fe29_to_fe(a, acc2.Z);
    fe_canon(o.c[2], a);
  }
  y[id] = o;
}

// The addends in limb form (36 dwords each, what the kernel's producer leaves
// in LDS), behind the outputs.
__global__ void k_limbs(const In* __restrict__ x, fe29* __restrict__ q29, int m) {
  const int id = blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= m) return;
#pragma unroll
  for (int j = 0; j < 8; j++) fe29_from_fe(q29[(size_t)id * 8 + j], x[id].q[j >> 2][j & 3]);
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
static H addmod(const H& a, const H& b) {  // a, b canonical
  uint64_t x[5];
  u128 c = 0;
  for (int k = 0; k < 4; k++) {
    c += (u128)a.w[k] + b.w[k];
    x[k] = (uint64_t)c;
    c >>= 64;
  }
  x[4] = (uint64_t)c;
  modp(x);
  H r;
  memcpy(r.w, x, 32);
  return r;
}
static H submod(const H& a, const H& b) {  // a + (p - b)
  H nb;
  uint64_t br = 0;
  for (int k = 0; k < 4; k++) {
    u128 d = (u128)P[k] - b.w[k] - br;
    nb.w[k] = (uint64_t)d;
    br = (d >> 64) ? 1 : 0;
  }
  return addmod(a, nb);
}
static H of_fe(const fe& z) {
  uint64_t x[5] = {0};
  for (int i = 0; i < 4; i++) x[i] = (uint64_t)z.v[2 * i] | ((uint64_t)z.v[2 * i + 1] << 32);
  modp(x);
  H r;
  memcpy(r.w, x, 32);
  return r;
}
struct HP {
  H X, Y, Z, T;
};
static HP dbl_host(const H& X, const H& Y, const H& Z) {  // ge_p2_dbl: p1p1
  const H xx = mulmod(X, X), yy = mulmod(Y, Y), zz = mulmod(Z, Z), s = addmod(X, Y), a = mulmod(s, s);
  HP r;
  r.Y = addmod(yy, xx);
  r.Z = submod(yy, xx);
  r.X = submod(a, r.Y);
  r.T = submod(addmod(zz, zz), r.Z);
  return r;
}
static void digit_host(H acc[3], const H q[4], bool neg) {
  HP t;
  for (int j = 0; j < 4; j++) {
    t = dbl_host(acc[0], acc[1], acc[2]);
    acc[0] = mulmod(t.X, t.T);
    acc[1] = mulmod(t.Y, t.Z);
    acc[2] = mulmod(t.Z, t.T);
  }
  const H T3 = mulmod(t.X, t.Y);
  const H o0 = mulmod(addmod(acc[1], acc[0]), q[0]), o1 = mulmod(submod(acc[1], acc[0]), q[1]);
  const H o2 = mulmod(q[3], T3), zz = mulmod(acc[2], q[2]), z2 = addmod(zz, zz);
  HP u;
  u.Y = addmod(o0, o1);
  u.X = submod(o0, o1);
  const H zs = addmod(z2, o2), zd = submod(z2, o2);
  u.Z = neg ? zd : zs;
  u.T = neg ? zs : zd;
  acc[0] = mulmod(u.X, u.T);
  acc[1] = mulmod(u.Y, u.Z);
  acc[2] = mulmod(u.Z, u.T);
}

int main() {
  const int M = 4096;  // distinct operands
  const int DIGITS = 16;
  In* h0 = (In*)malloc(sizeof(In) * M);
  uint64_t s = 88172645463325252ull;
  for (int i = 0; i < M; i++) {
    uint32_t* w = reinterpret_cast<uint32_t*>(&h0[i]);
    for (size_t j = 0; j < sizeof(In) / 4; j++) {
      s ^= s << 13;
      s ^= s >> 7;
      s ^= s << 17;
      w[j] = (uint32_t)s;
    }
  }
  // edge operands: every coordinate 0, 1, p - 1, p, 2^255 - 1, 2^256 - 1; the identity with identity addends
  const uint32_t lo[6] = {0, 1, 0xffffffecu, 0xffffffedu, 0xffffffffu, 0xffffffffu};
  for (int e = 0; e < 6; e++) {
    fe* f = reinterpret_cast<fe*>(&h0[e]);
    for (size_t c = 0; c < sizeof(In) / sizeof(fe); c++)
      for (int j = 0; j < 8; j++)
        f[c].v[j] = j == 0 ? lo[e] : e < 2 ? 0 : (j == 7 && e < 5 ? 0x7fffffffu : 0xffffffffu);
  }
  memset(&h0[6], 0, sizeof(In));
  h0[6].acc[1].v[0] = h0[6].acc[2].v[0] = 1;
  for (int a = 0; a < 2; a++) h0[6].q[a][0].v[0] = h0[6].q[a][1].v[0] = h0[6].q[a][2].v[0] = 1;

  H(*want)[2][3] = (H(*)[2][3])malloc(sizeof(H) * 6 * M);  // after 1 digit and after DIGITS
  for (int i = 0; i < M; i++) {
    H acc[3], q[2][4];
    for (int c = 0; c < 3; c++) acc[c] = of_fe(h0[i].acc[c]);
    for (int a = 0; a < 2; a++)
      for (int c = 0; c < 4; c++) q[a][c] = of_fe(h0[i].q[a][c]);
    for (int r = 0; r < DIGITS; r++) {
      digit_host(acc, q[r & 1], (r & 2) != 0);
      if (r == 0) memcpy(want[i][0], acc, sizeof(acc));
    }
    memcpy(want[i][1], acc, sizeof(acc));
  }

  In* dx;
  Out* dy;
  const int maxthreads = 256 * 2 * 256;
  if (hipMalloc(&dx, sizeof(In) * M) != hipSuccess) return 2;
  if (hipMalloc(&dy, sizeof(Out) * maxthreads + sizeof(fe29) * 8 * M) != hipSuccess) return 2;
  Out* got = (Out*)malloc(sizeof(Out) * maxthreads);
  hipMemcpy(dx, h0, sizeof(In) * M, hipMemcpyHostToDevice);
  void (*ks[2])(const In*, Out*, int, int) = {k<0>, k<1>};
  const char* names[2] = {"radix 2^32 (*_il) ", "9 x 29 bits       "};
  auto launch = [&](int v, int blocks, int digits) {
    // the limb-form addends sit behind this launch's outputs
    hipLaunchKernelGGL(k_limbs, dim3(M / 256), dim3(256), 0, 0, dx,
                       reinterpret_cast<fe29*>(dy + (size_t)blocks * 256), M);
    hipLaunchKernelGGL(ks[v], dim3(blocks), dim3(256), 0, 0, dx, dy, M, digits);
  };
  auto differ = [&](int lanes, int which) {
    if (hipMemcpy(got, dy, sizeof(Out) * lanes, hipMemcpyDeviceToHost) != hipSuccess) exit(2);
    int b = 0;
    for (int i = 0; i < lanes; i++) b += memcmp(&got[i], want[i % M][which], 96) != 0;
    return b;
  };
  int bad = 0;
  for (int v = 0; v < 2; v++) {
    launch(v, M / 256, 1);
    const int b1 = differ(M, 0);
    launch(v, M / 256, DIGITS);
    const int b2 = differ(M, 1);
    printf("%s vs host big integers: %d (one digit), %d (%d digits) of %d lanes differ\n", names[v], b1, b2, DIGITS, M);
    bad += b1 + b2;
  }
  if (bad) return 1;
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  const int RUNS = 7;
  double best[2][3], worst[2][3];
  for (int waves = 1; waves <= 2; waves++)
    for (int v = 0; v < 2; v++) {
      const int blocks = 256 * waves;
      launch(v, blocks, DIGITS);
      hipDeviceSynchronize();
      float lo_ms = 1e30f, hi_ms = 0;
      for (int r = 0; r < RUNS; r++) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(ks[v], dim3(blocks), dim3(256), 0, 0, dx, dy, M, DIGITS);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (ms < lo_ms) lo_ms = ms;
        if (ms > hi_ms) hi_ms = ms;
      }
      const int b = differ(blocks * 256, 1);
      best[v][waves] = (lo_ms * 1e-3) * 2.4e9 / (waves * DIGITS);
      worst[v][waves] = (hi_ms * 1e-3) * 2.4e9 / (waves * DIGITS);
      printf("%d wave/SIMD %s %7.0f SIMD cycles per digit @2.4GHz (best of %d; worst %7.0f, spread %.2f %%), %d lanes differ\n",
             waves, names[v], best[v][waves], RUNS, worst[v][waves], 100.0 * (worst[v][waves] / best[v][waves] - 1.0), b);
      bad += b;
    }
  for (int waves = 1; waves <= 2; waves++)
    printf("%d wave/SIMD: limb digit %+.1f %% SIMD cycles against radix 2^32 (radix 2^32's own spread %.2f %%)\n", waves,
           100.0 * (best[1][waves] / best[0][waves] - 1.0), 100.0 * (worst[0][waves] / best[0][waves] - 1.0));
  return bad ? 1 : 0;
}

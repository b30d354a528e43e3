// Which phase-2 kernel a split verification call launches
// (coa_launch_verify_split, coa_halved.hip), and k_pre_halve's priority bits.
// Host code only (no HIP), so tests/sanitize/main_pick_driver.cpp builds it
// with plain g++.  The table form phase 1 writes follows from the same value:
// k_pre_halve<3, kernel == COA_MAIN_SUMS>.
#pragma once
#include <cstdint>
#include <cstdlib>

enum CoaMainKernel {
  COA_MAIN_PLAIN,  // k_verify_main<3, false>
  COA_MAIN_IL,     // k_verify_main<1, true>
  COA_MAIN_TWO,    // k_verify_main2
  COA_MAIN_SUMS    // k_verify_main_sums
};

// A switch as the picker takes it: -1 unset, else atoi(value) != 0.  Any
// non-zero number is "on", a negative one included (the launch code used to
// take a negative COA_MAIN_TWO / COA_MAIN_SUMS as unset; only 0 and 1 are
// documented values).
inline int coa_env_switch(const char* v) { return v ? (atoi(v) != 0 ? 1 : 0) : -1; }

// n items; simd_items fill every SIMD with one wave (65,536 on the 256 CUs of
// an MI355X, the C2 size); has_ebp: phase 1 computes [e]B (COA_SPLIT_EB), which
// k_verify_main2 and k_verify_main_sums need.  il_env / two_env / sums_env:
// COA_MAIN_IL / COA_MAIN_TWO / COA_MAIN_SUMS as coa_env_switch gives them (A/B).
inline CoaMainKernel coa_pick_main(uint64_t n, uint64_t simd_items, bool has_ebp, int il_env, int two_env,
                                   int sums_env) {
  // at most one wave per SIMD: the interleaved formulas; COA_MAIN_IL=0/1
  // forces either
  const bool il = il_env >= 0 ? il_env != 0 : n <= simd_items;
  // an item's two chains in two waves (k_verify_main2) when the call has at
  // most a quarter wave per SIMD of items: its waves then run on SIMDs the
  // one-wave kernel leaves idle (4,096 / 16,384 items: 0.507 / 0.511 vs
  // 0.594 / 0.602 ms per call).  At 32,768 some SIMDs already get two of its
  // waves (0.82 vs 0.65 ms), and at C2's size the doubled doublings cost
  // more than the second wave per SIMD wins back (0.90 vs 0.72 ms).
  // COA_MAIN_TWO=0/1 forces either.  An explicit COA_MAIN_IL (without
  // COA_MAIN_TWO) selects the one-lane kernel it names at every size, so an
  // A/B of COA_MAIN_IL alone never measures k_verify_main2 instead.
  const int two_e = two_env >= 0 ? two_env : (il_env >= 0 ? 0 : -1);
  // each digit's table sum in a second wave (k_verify_main_sums): above
  // k_verify_main2's sizes and up to one wave per SIMD, where the one-lane
  // kernel leaves half of every SIMD's issue slots idle.  COA_MAIN_SUMS=0/1
  // forces either at every size (1 goes before COA_MAIN_TWO); an explicit
  // COA_MAIN_IL or COA_MAIN_TWO without it keeps selecting the kernels those
  // name.
  const int sums_e = sums_env >= 0 ? sums_env : ((il_env >= 0 || two_env >= 0) ? 0 : -1);
  if (has_ebp && (sums_e >= 0 ? sums_e != 0 : 4 * n > simd_items && n <= simd_items)) return COA_MAIN_SUMS;
  if (has_ebp && (two_e >= 0 ? two_e != 0 : 4 * n <= simd_items)) return COA_MAIN_TWO;
  return il ? COA_MAIN_IL : COA_MAIN_PLAIN;
}

// k_pre_halve's `prio` argument.  COA_PRE_PRIO: unset or anything else 1 (the
// hash/halving role at a raised wave priority), "0" 0 (default priority),
// "3" 1 | 8 (raised also through the [e]B additions); all A/B.  pre_diag
// (COA_PRE_DIAG, passed only by a library compiled with -DCOA_PRE_DIAG_BUILD):
// bits 2 / 4 skip the decompression / hash roles (role timing only,
// tools/pre_roles.sh; verdicts are then meaningless, so release builds cannot
// reach it).
inline int coa_pre_prio_bits(const char* pre_prio, const char* pre_diag) {
  const int p = pre_prio ? atoi(pre_prio) : 1;
  return (p == 0 ? 0 : p == 3 ? (1 | 8) : 1) | (pre_diag ? atoi(pre_diag) & 6 : 0);
}

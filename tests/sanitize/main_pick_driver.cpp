// The launch choice of the split verification (csrc/coa_main_pick.h) under
// ASan + UBSan, host code only: every row of the rule table, at the edge
// sizes n = 1, S/4, S/4 + 1, S, S + 1, for S = 65,536 (an MI355X) and
// S = 1,024, and k_pre_halve's priority bits.
#include <cstdio>
#include <cstring>

#include "coa_main_pick.h"

static int g_bad = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    if (!(cond)) {                                                               \
      if (g_bad++ < 20) printf("FAIL line %d (%s): %s\n", __LINE__, g_case, #cond); \
    }                                                                            \
  } while (0)
static char g_case[96] = "";

static const CoaMainKernel P = COA_MAIN_PLAIN, I = COA_MAIN_IL, T = COA_MAIN_TWO, U = COA_MAIN_SUMS;

// What a row of the table names at the five edge sizes, in the order
// n = 1, S/4, S/4 + 1, S, S + 1.
struct Row {
  int il, two, sums;  // -1 unset
  bool ebp;
  CoaMainKernel want[5];
};

static const Row kRows[] = {
    // nothing set
    {-1, -1, -1, true, {T, T, U, U, P}},
    {-1, -1, -1, false, {I, I, I, I, P}},
    // COA_MAIN_IL alone: the one-lane kernel it names at every size
    {0, -1, -1, true, {P, P, P, P, P}},
    {0, -1, -1, false, {P, P, P, P, P}},
    {1, -1, -1, true, {I, I, I, I, I}},
    {1, -1, -1, false, {I, I, I, I, I}},
    // COA_MAIN_TWO alone
    {-1, 1, -1, true, {T, T, T, T, T}},
    {-1, 0, -1, true, {I, I, I, I, P}},
    // COA_MAIN_SUMS=1 goes before everything, where phase 1 computes [e]B
    {-1, -1, 1, true, {U, U, U, U, U}},
    {0, -1, 1, true, {U, U, U, U, U}},
    {1, 0, 1, true, {U, U, U, U, U}},
    {-1, 1, 1, true, {U, U, U, U, U}},
    // ... and is ignored where it does not
    {-1, -1, 1, false, {I, I, I, I, P}},
    {0, -1, 1, false, {P, P, P, P, P}},
    {1, -1, 1, false, {I, I, I, I, I}},
    {-1, 1, 1, false, {I, I, I, I, P}},
    // COA_MAIN_SUMS=0 alone
    {-1, -1, 0, true, {T, T, I, I, P}},
    {-1, -1, 0, false, {I, I, I, I, P}},
    // COA_MAIN_IL with COA_MAIN_TWO=1
    {0, 1, -1, true, {T, T, T, T, T}},
    {1, 1, -1, true, {T, T, T, T, T}},
    {0, 0, -1, true, {P, P, P, P, P}},
    {1, 0, -1, true, {I, I, I, I, I}},
    // without [e]B from phase 1, TWO and SUMS are never chosen
    {-1, 1, -1, false, {I, I, I, I, P}},
    {-1, 0, -1, false, {I, I, I, I, P}},
    {0, 1, -1, false, {P, P, P, P, P}},
    {1, 1, 0, false, {I, I, I, I, I}},
    {-1, 1, 0, true, {T, T, T, T, T}},
    {-1, 0, 0, true, {I, I, I, I, P}},
};

static void walk(uint64_t S) {
  const uint64_t ns[5] = {1, S / 4, S / 4 + 1, S, S + 1};
  for (const Row& r : kRows)
    for (int k = 0; k < 5; k++) {
      snprintf(g_case, sizeof g_case, "S=%llu n=%llu il=%d two=%d sums=%d ebp=%d", (unsigned long long)S,
               (unsigned long long)ns[k], r.il, r.two, r.sums, (int)r.ebp);
      const CoaMainKernel got = coa_pick_main(ns[k], S, r.ebp, r.il, r.two, r.sums);
      CHECK(got == r.want[k]);
      if (!r.ebp) CHECK(got != COA_MAIN_TWO && got != COA_MAIN_SUMS);
    }
}

int main() {
  walk(65536);
  walk(1024);

  strcpy(g_case, "env switch");
  CHECK(coa_env_switch(nullptr) == -1);
  CHECK(coa_env_switch("0") == 0);
  CHECK(coa_env_switch("1") == 1);
  CHECK(coa_env_switch("2") == 1);
  CHECK(coa_env_switch("") == 0);

  strcpy(g_case, "pre prio");
  CHECK(coa_pre_prio_bits(nullptr, nullptr) == 1);
  CHECK(coa_pre_prio_bits("0", nullptr) == 0);
  CHECK(coa_pre_prio_bits("1", nullptr) == 1);
  CHECK(coa_pre_prio_bits("3", nullptr) == (1 | 8));
  CHECK(coa_pre_prio_bits("7", nullptr) == 1);
  const char* diag[5] = {"0", "2", "4", "6", "7"};
  const int bits[5] = {0, 2, 4, 6, 6};
  for (int k = 0; k < 5; k++) {
    CHECK(coa_pre_prio_bits(nullptr, diag[k]) == (1 | bits[k]));
    CHECK(coa_pre_prio_bits("0", diag[k]) == bits[k]);
    CHECK(coa_pre_prio_bits("3", diag[k]) == (1 | 8 | bits[k]));
  }

  printf("main pick %s: %d bad\n", g_bad ? "FAILED" : "ok", g_bad);
  return g_bad ? 1 : 0;
}

// The point predicates and the curve value of the engine's CPU path, under
// ASan + UBSan.  This file includes coa_cpu.cpp, one translation unit, to
// reach its anonymous namespace.
//   * the accept decisions rest on pt_same / pt_is_identity / pt_small_order,
//     so for a point with Z == 0 (no point of the curve; (0,0,0,0) is what a
//     zeroed table makes of an accumulator) each answers in the rejecting
//     direction, and for real points they answer as before
//   * curve(): B's table holds [1..8]B, and every thread gets the same value
#include <cstdio>
#include <thread>

#include "coa_cpu.cpp"  // csrc/ is on the include path

static int bad = 0;
#define CHECK(x)                                      \
  do {                                                \
    if (!(x)) {                                       \
      printf("FAILED line %d: %s\n", __LINE__, #x);   \
      bad++;                                          \
    }                                                 \
  } while (0)

int main() {
  const Curve& k = curve();
  const Fe zero = fe_small(0);
  const Pt O0{zero, zero, zero, zero};
  const Pt B = k.base;
  CHECK(!pt_is_identity(O0));
  CHECK(!pt_same(O0, O0));
  CHECK(!pt_same(B, O0));
  CHECK(!pt_same(O0, B));
  CHECK(pt_small_order(O0));
  CHECK(pt_is_identity(pt_identity()));
  CHECK(pt_same(B, B));
  CHECK(!pt_small_order(B));
  // Z == 0 with X, Y not zero: [8]P has Z != 0 again, P itself decides
  CHECK(pt_small_order(Pt{B.X, B.Y, zero, B.T}));
  // the same point in other projective coordinates
  const Fe two = fe_small(2);
  const Pt B2{fe_mul(B.X, two), fe_mul(B.Y, two), fe_mul(B.Z, two), fe_mul(B.T, two)};
  CHECK(pt_same(B, B2) && pt_same(B2, B));
  // base_tab[i-1] is [i]B
  const Cached cb = pt_cache(B, k.d2);
  Pt m = pt_identity();
  for (int i = 1; i <= 8; i++) {
    m = pt_add(m, cb, false);
    CHECK(pt_same(pt_add(pt_identity(), k.base_tab[i - 1], false), m));
    CHECK(!pt_same(m, B) || i == 1);
  }
  CHECK(pt_same(m, pt_double(pt_double(pt_double(B)))));
  // one value, whichever thread asks first or later
  const Curve *a = nullptr, *b = nullptr;
  std::thread ta([&] { a = &curve(); }), tb([&] { b = &curve(); });
  ta.join();
  tb.join();
  CHECK(a == &k && b == &k);
  printf("cpu points: %d bad\n", bad);
  return bad != 0;
}

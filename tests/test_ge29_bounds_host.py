"""csrc/coa_ge29.h on the CPU: the header's limb-bound budget by interval
arithmetic over exactly its steps, the bias constants, and every formula
against the curve, all on the exact-integer model of tests/ge29_ref.py."""
import random

import pytest

import ge29_ref as g
import pow29_ref as p29
from ge29_ref import Exact, Worst, M29, N, P, cls, value


def _within(v, bound):
    return all(x <= m for x, m in zip(v, bound))


# ------------------------------------------------------------------ classes
def test_class_n_holds_what_its_sources_leave():
    # a product's output bounds, a conversion's, and a carry pass over any dwords
    assert _within(p29.LIMB_MAX, N)
    assert _within(p29.from_fe(2**256 - 1), N)
    assert _within(g.carry([2**32 - 1] * 9, Worst), N)
    assert g.carry([2**32 - 1] * 9, Worst)[0] == M29 + 7 * 1216


@pytest.mark.parametrize("k", [2, 3, 4])
def test_bias_is_a_multiple_of_p_and_covers_its_subtrahend(k):
    b = g.bias(k)
    assert value(b) == k * 64 * P and value(b) % P == 0
    assert all(x < 2**32 for x in b)
    assert _within(cls(k - 1), b)  # class k - 1 is what fe29_sub<k> is used on
    assert not _within(cls(k), b)  # and the next bias down would not do
    if k > 2:
        assert not _within(cls(k - 1), g.bias(k - 1))


@pytest.mark.parametrize("ka,kb", [(1, 1), (2, 1), (3, 1), (2, 3), (3, 2), (6, 1)])
def test_product_budget(ka, kb):
    """ka * kb <= 6: every column below 2^64, column 17 a dword (asserted
    inside prod29), and the result back in class 1 -- in fact inside the
    bounds coa_fe_pow29.h states for its own outputs."""
    trace = []
    out = p29.prod29(cls(ka), cls(kb), False, mode=Worst, trace=trace)
    assert max(acc for kind, _, acc in trace if kind == "col") < 2**63.8
    assert [acc for kind, _, acc in trace if kind == "wrap"][0] < 2**35
    assert _within(out, p29.LIMB_MAX)


def test_product_budget_is_tight():
    # 3 x 3 already overflows a column: the budget is not slack by much
    with pytest.raises(AssertionError):
        p29.prod29(cls(3), cls(3), False, mode=Worst)
    with pytest.raises(AssertionError):
        p29.prod29(cls(8), cls(1), False, mode=Worst)


def test_squaring_budget():
    trace = []
    out = p29.prod29(cls(2), cls(2), True, mode=Worst, trace=trace)  # doubled limbs asserted inside
    assert max(2 * v for v in cls(2)) < 2**32
    assert max(acc for kind, _, acc in trace if kind == "col") < 2**63.3
    assert _within(out, p29.LIMB_MAX)
    with pytest.raises(AssertionError):
        p29.prod29(cls(4), cls(4), True, mode=Worst)


def test_prod29_beyond_its_documented_inputs():
    """coa_fe_pow29.h documents inputs of 2^29 - 1 (limb 1: 2^29 + 2^17); a
    parallel carry leaves limb 0 up to 2^29 - 1 + 7 * 1216 and the others up
    to 2^29 + 6.  prod29 is still exact there."""
    rng = random.Random(5)
    top = g.carry([2**32 - 1] * 9, Worst)
    assert not _within(top, p29.LIMB_MAX)
    ops = [top] + [[m - rng.randrange(3) for m in top] for _ in range(20)] + [cls(1)]
    for a in ops:
        for b in (a, ops[0], ops[-1]):
            assert value(g.mul(a, b)) % P == value(a) * value(b) % P
        assert value(g.sq(a)) % P == value(a) ** 2 % P


# ------------------------------------------------- the formulas, by intervals
def test_dbl_budget():
    """ge29_p2_dbl from class-1 coordinates: the classes the header states,
    and every product of both conversions legal (asserted inside prod29)."""
    one = cls(1)
    rX, rY, rZ, rT = g.p2_dbl((one, one, one), Worst)
    assert _within(rY, cls(2)) and _within(rZ, cls(3))
    assert _within(rX, N) and _within(rT, N)
    # before their carries r.X is in class 4 and r.T in class 6, dwords both
    assert max(cls(6)) < 2**32
    for conv in (g.p1p1_to_p2, g.p1p1_to_p3):
        for c in conv((rX, rY, rZ, rT), Worst):
            assert _within(c, p29.LIMB_MAX)


def test_add_budget():
    one = cls(1)
    rX, rY, rZ, rT = g.ge_add((one, one, one, one), (one, one, one, one), mode=Worst)
    assert _within(rX, cls(3)) and _within(rY, cls(2))
    assert _within(rZ, N) and _within(rT, N)
    for conv in (g.p1p1_to_p2, g.p1p1_to_p3):
        for c in conv((rX, rY, rZ, rT), Worst):
            assert _within(c, p29.LIMB_MAX)


def test_whole_digit_is_closed():
    """A Horner digit maps class-1 accumulators to outputs inside prod29's own
    output bounds: the loop can run any number of digits."""
    one = cls(1)
    t, acc2 = g.horner_digit((one, one, one), (one, one, one, one), mode=Worst)
    assert all(_within(c, p29.LIMB_MAX) for c in acc2)
    # what the tail hands to fe29_to_fe (g.to_fe asserts that function's stated bounds)
    for c in g.p1p1_to_p3(t, Worst):
        g.to_fe(c)


# --------------------------------------------------------- results, exactly
def test_helpers_on_values():
    rng = random.Random(3)
    for k in (1, 2, 3):
        for a in g.limb_operands(k, 20):
            b = [rng.randint(0, m) for m in cls(k)]
            assert value(g.add(a, b)) == value(a) + value(b)
            assert value(g.sub(a, b, k + 1)) % P == (value(a) - value(b)) % P
    for a in g.limb_operands(6, 30) + [[2**32 - 1] * 9]:
        c = g.carry(a)
        assert value(c) % P == value(a) % P and _within(c, N)


def test_formulas_against_the_curve():
    pts = g.curve_points(12)
    rng = random.Random(9)
    for i, pt in enumerate(pts):
        z = rng.randrange(1, P)
        acc3 = g.p3_of(pt, z)
        dbl = g.p1p1_to_p2(g.p2_dbl(acc3[:3]))
        assert g.affine(dbl) == g.ed_add(pt, pt)
        other = pts[(i + 5) % len(pts)]
        for neg in (False, True):
            q = g.cached_of(other, rng.randrange(1, P))
            if neg:  # the caller's half of a negation: Y+X / Y-X swapped; t2d_neg does the rest
                q = [q[1], q[0], q[2], q[3]]
            t = g.ge_add(acc3, q, neg)
            want = g.ed_add(pt, ((P - other[0]) % P, other[1]) if neg else other)
            assert g.affine(g.p1p1_to_p2(t)) == want
            X, Y, Z, T = g.point_values(g.p1p1_to_p3(t))
            assert X * Y % P == T * Z % P  # extended coordinates are consistent
            assert g.affine(g.p1p1_to_p3(t)[:3]) == want


def test_digit_against_the_curve():
    pts = g.curve_points(6, seed=77)
    for a, b in zip(pts, pts[1:]):
        acc2 = g.p3_of(a, 12345)[:3]
        _, out = g.horner_digit(acc2, g.cached_of(b, 6789))
        want = a
        for _ in range(4):
            want = g.ed_add(want, want)
        assert g.affine(out) == g.ed_add(want, b)


def test_identity_runs_through():
    """Dead and rejected lanes run the loop on the identity."""
    ident2 = [p29.from_fe(0), p29.from_fe(1), p29.from_fe(1)]
    ident_c = [p29.from_fe(1), p29.from_fe(1), p29.from_fe(1), p29.from_fe(0)]
    acc2 = ident2
    for _ in range(3):
        _, acc2 = g.horner_digit(acc2, ident_c)
        assert g.affine(acc2) == (0, 1)

"""csrc/coa_fe_pow29.h on the CPU: the header's limb bounds by interval
arithmetic and the whole (p-5)/8 chain against pow(), both on the exact-integer
restatement of the algorithm in tests/pow29_ref.py."""
import random

import pytest

from pow29_ref import (LIMB_MAX, M29, P, Worst, from_fe, mul29, operands, pow_p58_29, prod29, sq29, terms, to_fe,
                       value)


# ------------------------------------------------------------------ bounds
@pytest.mark.parametrize("sq", [True, False])
def test_bounds_closed_and_below_2_64(sq):
    trace = []
    out = prod29(LIMB_MAX, LIMB_MAX, sq, mode=Worst, trace=trace)
    # every assertion inside prod29 held for the maxima; the figures the
    # header quotes:
    cols = [acc for kind, _, acc in trace if kind == "col"]
    assert max(cols) < 2**61.4
    wrap = [acc for kind, _, acc in trace if kind == "wrap"][0]
    assert wrap < 2**32.4
    assert all(o <= m for o, m in zip(out, LIMB_MAX)), out
    assert out[1] - M29 < 2**14


def test_conversion_bounds():
    # from_fe stays inside the bounds, limb 8 within 24 bits
    l = from_fe(2**256 - 1)
    assert all(v <= m for v, m in zip(l, LIMB_MAX)) and l[8] < 2**24
    # to_fe accepts every limb at its maximum (asserts inside)
    assert to_fe(LIMB_MAX) % P == value(LIMB_MAX) % P


def test_terms_counts():
    assert sum(len(terms(k, True)) for k in range(17)) == 45
    assert sum(len(terms(k, False)) for k in range(17)) == 81


# ----------------------------------------------------------------- results
def test_single_products_on_worst_limbs():
    rng = random.Random(7)
    cases = [LIMB_MAX, [0] * 9, [1] + [0] * 8]
    cases += [[rng.randint(0, m) for m in LIMB_MAX] for _ in range(300)]
    for a in cases:
        for b in (a, cases[0], cases[-1]):
            r = mul29(a, b)
            assert value(r) % P == value(a) * value(b) % P
            assert all(v <= m for v, m in zip(r, LIMB_MAX))
        r = sq29(a)
        assert value(r) % P == value(a) ** 2 % P
        assert r == mul29(a, a)


def test_round_trip():
    for x in operands():
        assert to_fe(from_fe(x)) % P == x % P


def test_chain_against_pow():
    e = (P - 5) // 8
    assert e == 2**252 - 3
    for z in operands():
        r = pow_p58_29(z)
        assert 0 <= r < 2**256
        assert r % P == pow(z, e, P), hex(z)


def test_vectorised_model_is_the_scalar_one():
    """pow29_ref's numpy form (the device test's reference) against the scalar one."""
    from pow29_ref import pow_p58_29_many, prod29_many

    rng = random.Random(11)
    a = [list(LIMB_MAX)] + [[rng.randint(0, m) for m in LIMB_MAX] for _ in range(64)]
    b = a[::-1]
    assert prod29_many(a, a, True).tolist() == [sq29(x) for x in a]
    assert prod29_many(a, b, False).tolist() == [mul29(x, y) for x, y in zip(a, b)]
    ops = operands()
    got = pow_p58_29_many(ops)
    assert got[:300:7] == [pow_p58_29(z) for z in ops[:300:7]]
    assert all(r % P == pow(z, (P - 5) // 8, P) for r, z in zip(got, ops))

"""csrc/coa_ge29.h restated with exact integers: the reference of
tests/test_ge29_bounds_host.py (CPU) and tests/test_gpu_arith_ge29.py (device).

Every helper and point formula of the header is written out step for step on
lists of nine limbs, over pow29_ref's model of prod29 / fe29_from_fe /
fe29_to_fe.  Each function takes a mode:

  * Exact: plain evaluation, the device's raw limbs;
  * Worst: every value is an upper bound.  Sums and products are monotone; a
    subtraction a + BIAS_K - b is bounded by a + BIAS_K, and the model asserts
    that BIAS_K covers b limb by limb (so the device's dword never wraps); a
    masked limb is bounded by min(v, 2^29 - 1).

In both modes every dword quantity is asserted below 2^32, and pow29_ref's
prod29 asserts every column sum below 2^64 and column 17 inside a dword.
"""
import random

import pow29_ref as p29
from pow29_ref import M29, P, W261, Exact, Worst, from_fe, prod29, value

# class N of the header (inclusive limb maxima); k N is k * N[i]
N = [2**29 + 2**14, 2**29 + 2**17] + [2**29 + 2**3] * 7


def cls(k):
    return [k * v for v in N]


def bias(k):
    """Limbs of k * 64 p = k * (2^261 - 1216)."""
    return [k * (2**29 - W261)] + [k * M29] * 8


def _dwords(v):
    assert all(0 <= x < 2**32 for x in v), v
    return v


def add(a, b):
    return _dwords([x + y for x, y in zip(a, b)])


def sub(a, b, k, mode=Exact):
    bk = bias(k)
    if mode is Worst:
        assert all(y <= z for y, z in zip(b, bk)), ("BIAS_%d does not cover its subtrahend" % k, b)
        return _dwords([x + z for x, z in zip(a, bk)])
    assert all(x + z >= y for x, y, z in zip(a, b, bk))
    return _dwords([x + z - y for x, y, z in zip(a, b, bk)])


def carry(a, mode=Exact):
    _dwords(a)
    lo = [min(x, M29) for x in a] if mode is Worst else [x & M29 for x in a]
    hi = [x >> 29 for x in a]
    assert hi[8] * W261 < 2**32
    return _dwords([lo[0] + hi[8] * W261] + [lo[i] + hi[i - 1] for i in range(1, 9)])


def cswap_to(a, b, c):
    return (list(b), list(a)) if c else (list(a), list(b))


def mul(a, b, mode=Exact):
    return prod29(a, b, False, mode=mode)


def sq(a, mode=Exact):
    return prod29(a, a, True, mode=mode)


def to_fe(a):
    """fe29_to_fe, only ever on limbs inside the bounds coa_fe_pow29.h states for it."""
    assert all(x <= m for x, m in zip(a, p29.LIMB_MAX)), ("outside fe29_to_fe's stated bounds", a)
    return p29.to_fe(a)


# ------------------------------------------------------------ point formulas
# points are tuples of limb lists in the header's field order
def p2_dbl(p, mode=Exact):
    X, Y, Z = p
    xx, yy, zz = sq(X, mode), sq(Y, mode), sq(Z, mode)
    a = sq(add(X, Y), mode)
    rY = add(yy, xx)
    rZ = sub(yy, xx, 2, mode)
    rX = carry(sub(a, rY, 3, mode), mode)
    rT = carry(sub(add(zz, zz), rZ, 4, mode), mode)
    return rX, rY, rZ, rT


def p1p1_to_p2(p, mode=Exact):
    X, Y, Z, T = p
    return mul(X, T, mode), mul(Y, Z, mode), mul(Z, T, mode)


def p1p1_to_p3(p, mode=Exact):
    X, Y, Z, T = p
    return mul(X, T, mode), mul(Y, Z, mode), mul(Z, T, mode), mul(X, Y, mode)


def ge_add(p, q, t2d_neg=False, mode=Exact):
    X, Y, Z, T = p
    qYpX, qYmX, qZ, qT2d = q
    s = add(Y, X)
    d = sub(Y, X, 2, mode)
    o0, o1 = mul(s, qYpX, mode), mul(d, qYmX, mode)
    o2, o3 = mul(qT2d, T, mode), mul(Z, qZ, mode)
    o3 = add(o3, o3)
    rY = add(o0, o1)
    rX = sub(o0, o1, 2, mode)
    zs = carry(add(o3, o2), mode)
    zd = carry(sub(o3, o2, 2, mode), mode)
    if mode is Worst:  # either may land in either place
        zs = zd = [max(x, y) for x, y in zip(zs, zd)]
    rZ, rT = cswap_to(zs, zd, t2d_neg)
    return rX, rY, rZ, rT


def horner_digit(acc2, q, t2d_neg=False, mode=Exact):
    """One digit of the consumer's loop: four doublings, the last into p3, one
    addition, and the conversion the next digit starts from."""
    for _ in range(3):
        acc2 = p1p1_to_p2(p2_dbl(acc2, mode), mode)
    acc3 = p1p1_to_p3(p2_dbl(acc2, mode), mode)
    t = ge_add(acc3, q, t2d_neg, mode)
    return t, p1p1_to_p2(t, mode)


# ------------------------------------------------------- the curve, on values
D = -121665 * pow(121666, P - 2, P) % P


def point_values(p):
    return [value(c) % P for c in p]


def affine(p):
    """(x, y) of a p2 / p3 / p1p1 point given as limb lists."""
    v = point_values(p)
    if len(v) == 3:
        X, Y, Z = v
        return X * pow(Z, P - 2, P) % P, Y * pow(Z, P - 2, P) % P
    return None


def ed_add(a, b):
    (x1, y1), (x2, y2) = a, b
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + x2 * y1) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def curve_points(n, seed=0x6529):
    """n affine points: multiples of the base point."""
    by = 4 * pow(5, P - 2, P) % P
    bx2 = (by * by - 1) * pow(D * by * by + 1, P - 2, P) % P
    bx = pow(bx2, (P + 3) // 8, P)
    if bx * bx % P != bx2:
        bx = bx * pow(2, (P - 1) // 4, P) % P
    if bx & 1:
        bx = P - bx
    base = (bx, by)
    rng = random.Random(seed)
    out, cur = [], base
    for _ in range(n):
        for _ in range(rng.randrange(1, 4)):
            cur = ed_add(cur, base)
        out.append(cur)
    return out


def p3_of(pt, z=1):
    x, y = pt
    return [from_fe(x * z % P), from_fe(y * z % P), from_fe(z % P), from_fe(x * y * z % P)]


def cached_of(pt, z=1):
    x, y = pt
    return [from_fe((y + x) * z % P), from_fe((y - x) * z % P), from_fe(z % P), from_fe(2 * D * x * y * z % P)]


# ---------------------------------------------------------------- operands
def limb_operands(k=1, count=40, seed="coa-ge29"):
    """Limb vectors of class k: the maxima, maxima less a little, random ones, zero."""
    rng = random.Random(seed + str(k))
    top = cls(k)
    out = [list(top), [0] * 9]
    out += [[m - rng.randrange(4) for m in top] for _ in range(8)]
    out += [[rng.randint(0, m) for m in top] for _ in range(count)]
    return out

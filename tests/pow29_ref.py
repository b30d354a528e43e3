"""csrc/coa_fe_pow29.h restated with exact integers: the reference of
tests/test_pow29_host.py (CPU) and tests/test_gpu_arith_pow29.py (device).

The limb algorithm of the header -- nine 29-bit limbs, product scanning with
one accumulator, high columns first, every fold as a term times 2^261 mod p =
1216 -- is written out step for step, so that

  * the limb bounds stated at the top of the header can be asserted by
    interval arithmetic: with every limb at its stated maximum no column sum
    reaches 2^64, no dword quantity reaches 2^32, and the output limbs are
    inside the same bounds (the bounds are closed under sq29 / mul29);
  * the whole chain can be compared with pow(z, (p - 5) // 8, p).

tests/test_gpu_arith_pow29.py checks the device code's raw limbs against this
model.
"""
import random

P = 2**255 - 19
M29 = 2**29 - 1
W261 = 1216
assert pow(2, 261, P) == W261

# the header's stated limb bounds (inclusive)
LIMB_MAX = [M29, 2**29 + 2**17] + [M29] * 7


def from_fe(x):
    """fe29_from_fe: a value < 2^256 cut into 29-bit limbs (limb 8 has 24 bits)."""
    assert 0 <= x < 2**256
    return [(x >> (29 * i)) & M29 for i in range(9)]


def value(l):
    return sum(v << (29 * i) for i, v in enumerate(l))


def to_fe(l):
    """fe29_to_fe: limbs summed at their offsets into eight dwords, the bits
    above 2^256 folded as 38 by fe_fold_word (one fold, result < 2^256)."""
    acc, bits, words = 0, 0, []
    for i in range(9):
        acc += l[i] << bits
        assert acc < 2**64
        bits += 29
        if bits >= 32:
            words.append(acc & 0xFFFFFFFF)
            acc >>= 32
            bits -= 32
    assert len(words) == 8 and acc < 2**6
    w = acc * 38
    assert w < 2**32 - 2**10  # fe_fold_word's precondition
    r = sum(v << (32 * i) for i, v in enumerate(words)) + w
    if r >> 256:
        r = (r & (2**256 - 1)) + 38
    assert r < 2**256
    return r


class Exact:
    """Plain evaluation: limbs are masked, carries shifted."""

    @staticmethod
    def take(acc):
        return acc & M29, acc >> 29


class Worst:
    """Interval evaluation: every operand is an upper bound.  Sums and
    products are monotone; a masked limb is bounded by min(acc, 2^29 - 1)."""

    @staticmethod
    def take(acc):
        return min(acc, M29), acc >> 29


def terms(k, sq):
    """(i, j, doubled) for column k, as col29 of the header enumerates them."""
    out = []
    for i in range(9):
        j = k - i
        if j < 0 or j > 8 or (sq and i > j):
            continue
        out.append((i, j, sq and i < j))
    return out


def prod29(a, b, sq, mode=Exact, trace=None):
    a2 = [2 * v for v in a]
    if sq:
        assert all(v < 2**32 for v in a2[:8])
    h = []
    acc = 0
    for k in range(9, 17):
        for i, j, dbl in terms(k, sq):
            acc += (a2[i] if dbl else a[i]) * (a[j] if sq else b[j])
        assert acc < 2**64, ("high column", k)
        if trace is not None:
            trace.append(("col", k, acc))
        limb, acc = mode.take(acc)
        h.append(limb)
    assert acc < 2**32, "column 17 must fit a dword"
    h.append(acc)
    acc = 0
    o = []
    for k in range(9):
        for i, j, dbl in terms(k, sq):
            acc += (a2[i] if dbl else a[i]) * (a[j] if sq else b[j])
        acc += h[k] * W261
        assert acc < 2**64, ("low column", k)
        if trace is not None:
            trace.append(("col", k, acc))
        limb, acc = mode.take(acc)
        o.append(limb)
    # the wrap of the carry out of column 8 (weight 2^261)
    if trace is not None:
        trace.append(("wrap", 8, acc))
    # device: t = mad(lo32(acc), 1216, o[0]), then hi32(t) += hi32(acc) * 1216 in
    # a dword: the same number as acc * 1216 + o[0] while that dword holds
    assert acc < 2**64
    t = acc * W261 + o[0]
    assert (t >> 32) < 2**32 and (acc >> 32) * W261 < 2**32
    limb, carry = mode.take(t)
    assert carry < 2**32
    o[0] = limb
    o[1] += carry
    assert o[1] < 2**32
    return o


def sq29(a, **kw):
    return prod29(a, a, True, **kw)


def mul29(a, b, **kw):
    return prod29(a, b, False, **kw)


def sqn29(a, n):
    for _ in range(n):
        a = sq29(a)
    return a


def pow_p58_29(z):
    """fe_pow_p58_29: dalek's addition chain on the limb form."""
    z = from_fe(z)
    z2 = sq29(z)
    t = sqn29(z2, 2)
    z9 = mul29(t, z)
    z11 = mul29(z9, z2)
    t = sq29(z11)
    z_5_0 = mul29(t, z9)
    z_10_0 = mul29(sqn29(z_5_0, 5), z_5_0)
    z_20_0 = mul29(sqn29(z_10_0, 10), z_10_0)
    z_40_0 = mul29(sqn29(z_20_0, 20), z_20_0)
    z_50_0 = mul29(sqn29(z_40_0, 10), z_10_0)
    z_100_0 = mul29(sqn29(z_50_0, 50), z_50_0)
    t = mul29(sqn29(z_100_0, 100), z_100_0)
    t = mul29(sqn29(t, 50), z_50_0)
    t = mul29(sqn29(t, 2), z)
    return to_fe(t)


def operands():
    """The operand list shared with the device test."""
    ops = [0, 1, 2, P - 1, P, P + 1, 2**255 - 1, 2**256 - 1]
    ops.append(value([M29] * 8 + [2**24 - 1]))  # every limb full (as far as 256 bits go)
    ops += [1 << b for b in range(256)]
    rng = random.Random(0x29)
    ops += [rng.getrandbits(256) for _ in range(2000)]
    return ops


# ------------------------------------------------------------ many at once
# The same steps on numpy uint64 columns, one row per operand: exact because
# no column sum reaches 2^64 (asserted above for the limb maxima).  For the
# device test, whose expected limbs would otherwise take the scalar model
# several seconds; tests/test_pow29_host.py holds the two models together.
def prod29_many(a, b, sq):
    import numpy as np

    a = np.asarray(a, np.uint64)
    b = np.asarray(b, np.uint64)
    a2 = a * np.uint64(2)
    m29, s29, w = np.uint64(M29), np.uint64(29), np.uint64(W261)

    def column(k, acc):
        for i, j, dbl in terms(k, sq):
            acc = acc + (a2[:, i] if dbl else a[:, i]) * (a[:, j] if sq else b[:, j])
        return acc

    acc = np.zeros(a.shape[0], np.uint64)
    h = []
    for k in range(9, 17):
        acc = column(k, acc)
        h.append(acc & m29)
        acc = acc >> s29
    h.append(acc)
    acc = np.zeros(a.shape[0], np.uint64)
    o = []
    for k in range(9):
        acc = column(k, acc) + h[k] * w
        o.append(acc & m29)
        acc = acc >> s29
    t = acc * w + o[0]
    o[0] = t & m29
    o[1] = o[1] + (t >> s29)
    return np.stack(o, axis=1)


def pow_p58_29_many(zs):
    """[pow_p58_29(z) for z in zs]."""
    import numpy as np

    def sq(a, n=1):
        for _ in range(n):
            a = prod29_many(a, a, True)
        return a

    def mul(a, b):
        return prod29_many(a, b, False)

    z = np.array([from_fe(x) for x in zs], np.uint64)
    z2 = sq(z)
    z9 = mul(sq(z2, 2), z)
    z11 = mul(z9, z2)
    z_5_0 = mul(sq(z11), z9)
    z_10_0 = mul(sq(z_5_0, 5), z_5_0)
    z_20_0 = mul(sq(z_10_0, 10), z_10_0)
    z_40_0 = mul(sq(z_20_0, 20), z_20_0)
    z_50_0 = mul(sq(z_40_0, 10), z_10_0)
    z_100_0 = mul(sq(z_50_0, 50), z_50_0)
    t = mul(sq(z_100_0, 100), z_100_0)
    t = mul(sq(t, 50), z_50_0)
    t = mul(sq(t, 2), z)
    return [to_fe([int(v) for v in row]) for row in t]

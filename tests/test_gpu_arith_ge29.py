"""GPU: csrc/coa_ge29.h on its RAW output limbs against the exact-integer
model of tests/ge29_ref.py, through tests/arith/ge29_check.hip
(lib/libcoa_ge29check.so) in both assembled forms of the rare carry blocks.

Every field helper (add, the three subtractions, the carry pass, the swap) and
every point formula (doubling, p1p1 -> p2 / p3, the addition with its t2d_neg
swap, the two conversions, a whole Horner digit).  Operands:
pow29_ref.operands() cut into limbs, limbs at every maximum the header states
for that operand, random limbs up to those maxima, and both values of the swap
flag.  Every op runs as 256-lane workgroups (the last one partly filled) and as
a 1-lane call, with a guard region behind the output."""
import ctypes
import os
import random

import numpy as np
import pytest

import ge29_ref as g
import pow29_ref as p29

pytestmark = pytest.mark.gpu

FORMS = {"out_of_line": 0, "rare_inline": 1}
# enum Op of ge29_check.hip
OPS = {"add": 0, "sub2": 1, "sub3": 2, "sub4": 3, "carry": 4, "cswap": 5, "dbl": 6, "to_p2": 7, "to_p3": 8,
       "add_pt": 9, "p3_from": 10, "p3_to": 11, "digit": 12}
FILL = 0x5A5A5A5A
GUARD = 64


def _words(x, n=8):
    return [(x >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


def _flat(fields):
    return [v for f in fields for v in f]


@pytest.fixture(scope="module")
def ge29_lib(engine):
    import torch

    path = os.path.join(os.path.dirname(engine.LIB_PATH), "libcoa_ge29check.so")
    assert os.path.exists(path), f"{path} not built"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.coa_ge29_run.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_uint32, vp, vp]
    lib.coa_ge29_run.restype = ctypes.c_int
    torch.cuda.set_device(0)
    return lib


def _vectors(k, rng, values):
    """Limb vectors of class k: the shared operand list (class 1 by itself),
    the maxima, maxima less a little, random limbs up to the maxima."""
    top = g.cls(k)
    out = [list(top), [0] * 9] + [[m - rng.randrange(4) for m in top] for _ in range(6)]
    out += [[rng.randint(0, m) for m in top] for _ in range(120)]
    return out + [p29.from_fe(x) for x in values]


@pytest.fixture(scope="module")
def cases():
    """{op: (a rows, b rows or None, flags, expected rows)}, computed once."""
    rng = random.Random("coa-ge29-limbs")
    values = p29.operands()[:400]  # the edge values, the single bits, 135 random ones
    c = {}

    def pairs(ka, kb):
        a, b = _vectors(ka, rng, values), _vectors(kb, rng, values)
        b = b[:2] + b[3:] + b[2:3]  # maxima meet maxima, the rest is shifted by one
        return a, b

    a, b = pairs(3, 3)
    c["add"] = (a, b, None, [g.add(x, y) for x, y in zip(a, b)])
    for k in (2, 3, 4):  # fe29_sub<k>: a subtrahend of class k - 1, a minuend of the class the formulas give it
        a, b = pairs({2: 2, 3: 1, 4: 2}[k], k - 1)
        c[f"sub{k}"] = (a, b, None, [g.sub(x, y, k) for x, y in zip(a, b)])
    a = _vectors(6, rng, values) + [[2**32 - 1] * 9, [2**29] * 9, [2**29 - 1] * 9]
    c["carry"] = (a, None, None, [g.carry(x) for x in a])
    a, b = pairs(6, 6)
    fl = [i & 1 for i in range(len(a))]
    c["cswap"] = (a, b, fl, [_flat(g.cswap_to(x, y, f)) for x, y, f in zip(a, b, fl)])

    def points(classes):
        cols = [_vectors(k, rng, values) for k in classes]
        n = min(len(col) for col in cols)
        # the same row of every column but rotated, except row 0: all maxima together
        return [[cols[f][0 if i == 0 else 1 + (i + 17 * f) % (n - 1)] for f in range(len(classes))] for i in range(n)]

    p2 = points((1, 1, 1))
    c["dbl"] = ([_flat(p) for p in p2], None, None, [_flat(g.p2_dbl(p)) for p in p2])
    # p1p1 as a doubling (1, 2, 3, 1) and as an addition (3, 2, 1, 1) leave it
    pp = points((1, 2, 3, 1)) + points((3, 2, 1, 1))
    c["to_p2"] = ([_flat(p) for p in pp], None, None, [_flat(g.p1p1_to_p2(p)) for p in pp])
    c["to_p3"] = ([_flat(p) for p in pp], None, None, [_flat(g.p1p1_to_p3(p)) for p in pp])
    p3, q = points((1, 1, 1, 1)), points((1, 1, 1, 1))
    q = q[:1] + q[2:] + q[1:2]
    fl = [(i >> 1) & 1 for i in range(len(p3))]
    c["add_pt"] = ([_flat(p) for p in p3], [_flat(x) for x in q], fl,
                   [_flat(g.ge_add(p, x, bool(f))) for p, x, f in zip(p3, q, fl)])
    vals = [[values[(i + 31 * f) % len(values)] for f in range(4)] for i in range(len(values))]
    c["p3_from"] = ([_flat(_words(v) for v in row) for row in vals], None, None,
                    [_flat(p29.from_fe(v) for v in row) for row in vals])
    # fe29_to_fe only ever sees products: limbs inside coa_fe_pow29.h's own bounds
    lm = p29.LIMB_MAX
    prod = [[list(lm)] * 4] + [[[rng.randint(0, m) for m in lm] for _ in range(4)] for _ in range(200)]
    prod += [[p29.from_fe(v) for v in row] for row in vals[:200]]
    c["p3_to"] = ([_flat(p) for p in prod], None, None, [_flat(_words(g.to_fe(f)) for f in p) for p in prod])
    d2, dq = p2[:300], q[:300]
    fl = [i & 1 for i in range(len(d2))]
    c["digit"] = ([_flat(p) for p in d2], [_flat(x) for x in dq], fl,
                  [_flat(g.horner_digit(p, x, bool(f))[1]) for p, x, f in zip(d2, dq, fl)])
    return c


def _run(lib, form, op, a, b, fl, nout):
    """op on the rows of a (and b, fl): raw output rows."""
    import torch

    dev = torch.device("cuda", 0)
    n = len(a)

    def up(rows):
        return torch.from_numpy(np.ascontiguousarray(rows, np.uint32).view(np.int32)).to(dev)

    d_a = up(a)
    d_b = up(b) if b is not None else None
    d_f = up(fl if fl is not None else [0] * n)
    fill = int(np.array([FILL], np.uint32).view(np.int32)[0])
    d_out = torch.full((n * nout + GUARD,), fill, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = lib.coa_ge29_run(OPS[op], FORMS[form], d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None,
                          d_f.data_ptr(), n, d_out.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, f"[{form}] {op}: coa_ge29_run returned HIP error {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[n * nout:] == FILL).all(), f"[{form}] {op}: wrote past its output"
    return out[:n * nout].reshape(n, nout)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("op", list(OPS))
def test_raw_limbs(ge29_lib, cases, op, form):
    a, b, fl, want = cases[op]
    want = np.array(want, np.uint32)
    nout = want.shape[1]
    assert len(a) % 256 != 0 and len(a) > 256  # several workgroups, the last one partly filled
    got = _run(ge29_lib, form, op, a, b, fl, nout)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"[{form}] {op}: {bad.size} of {len(a)} items differ, first {bad[:4]}: " \
                          f"{[hex(int(v)) for v in got[bad[0]]]} != {[hex(int(v)) for v in want[bad[0]]]}"
    # a 1-lane call: the last operand alone
    one = _run(ge29_lib, form, op, a[-1:], b[-1:] if b else None, fl[-1:] if fl else None, nout)
    assert (one[0] == want[-1]).all(), f"[{form}] {op}: the 1-lane call differs"


def test_model_is_the_field(cases):
    """The expected rows are right as field elements, not only as limbs."""
    a, b, fl, want = cases["add"]
    for x, y, w in zip(a[::41], b[::41], want[::41]):
        assert g.value(w) % g.P == (g.value(x) + g.value(y)) % g.P
    a, b, fl, want = cases["sub4"]
    for x, y, w in zip(a[::41], b[::41], want[::41]):
        assert g.value(w) % g.P == (g.value(x) - g.value(y)) % g.P
    a, _, _, want = cases["carry"]
    for x, w in zip(a, want):
        assert g.value(w) % g.P == g.value(x) % g.P

"""GPU: csrc/coa_fe_pow29.h on its RAW output limbs against the exact-integer
model of tests/pow29_ref.py, through tests/arith/pow29_check.hip (in
lib/libcoa_arithcheck.so) in both assembled forms of the rare carry blocks.

The squaring, the multiplication, the two conversions and the whole (p-5)/8
chain, each on the operand list of pow29_ref.operands() (0, 1, 2, p-1, p, p+1,
2^255-1, 2^256-1, every limb full, one set bit at each of the 256 positions,
2,000 seeded random values); the products also on limbs at their stated
maxima and on random limbs up to them.  Every op runs as 256-lane workgroups
(the last one partly filled) and as a 1-lane call."""
import ctypes
import os
import random

import numpy as np
import pytest

import pow29_ref as ref

pytestmark = pytest.mark.gpu

FORMS = {"out_of_line": 0, "rare_inline": 1}
OPS = {"sq": 0, "mul": 1, "from_fe": 2, "to_fe": 3, "pow_p58": 4}  # enum Op of pow29_check.hip
FILL = 0x5A5A5A5A
GUARD = 64


def _words(x, n):
    return [(x >> (32 * k)) & 0xFFFFFFFF for k in range(n)]


@pytest.fixture(scope="module")
def pow29_lib(engine):
    import torch

    path = os.path.join(os.path.dirname(engine.LIB_PATH), "libcoa_arithcheck.so")
    assert os.path.exists(path), f"{path} not built"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.coa_pow29_run.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, ctypes.c_uint32, vp, vp]
    lib.coa_pow29_run.restype = ctypes.c_int
    torch.cuda.set_device(0)
    return lib


@pytest.fixture(scope="module")
def cases():
    """{op: (a rows, b rows or None, expected rows)}, computed once."""
    ops = ref.operands()
    rng = random.Random("coa-pow29-limbs")
    limbs = [ref.from_fe(x) for x in ops]
    limbs += [list(ref.LIMB_MAX), [0] * 9, [ref.LIMB_MAX[0]] + [0] * 8, [0] * 8 + [ref.LIMB_MAX[8]]]
    limbs += [[rng.randint(0, m) for m in ref.LIMB_MAX] for _ in range(200)]
    limbs += [[m - rng.randrange(4) for m in ref.LIMB_MAX] for _ in range(50)]
    other = limbs[1:] + limbs[:1]
    other[len(ops)] = list(ref.LIMB_MAX)  # maxima times maxima
    return {
        "sq": (limbs, None, ref.prod29_many(limbs, limbs, True).tolist()),
        "mul": (limbs, other, ref.prod29_many(limbs, other, False).tolist()),
        "from_fe": ([_words(x, 8) for x in ops], None, [ref.from_fe(x) for x in ops]),
        "to_fe": (limbs, None, [_words(ref.to_fe(a), 8) for a in limbs]),
        "pow_p58": ([_words(x, 8) for x in ops], None, [_words(r, 8) for r in ref.pow_p58_29_many(ops)]),
    }


def _run(lib, form, op, a, b, n):
    """op on the first n rows of a (and b): raw output rows."""
    import torch

    dev = torch.device("cuda", 0)

    def up(rows):
        return torch.from_numpy(np.ascontiguousarray(rows[:n], np.uint32).view(np.int32)).to(dev)

    d_a = up(a)
    d_b = up(b) if b is not None else None
    nout = 8 if op in ("to_fe", "pow_p58") else 9
    fill = int(np.array([FILL], np.uint32).view(np.int32)[0])
    d_out = torch.full((n * nout + GUARD,), fill, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = lib.coa_pow29_run(OPS[op], FORMS[form], d_a.data_ptr(), d_b.data_ptr() if d_b is not None else None, n,
                           d_out.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, f"[{form}] {op}: coa_pow29_run returned HIP error {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[n * nout:] == FILL).all(), f"[{form}] {op}: wrote past its output"
    return out[:n * nout].reshape(n, nout)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("op", list(OPS))
def test_raw_limbs(pow29_lib, cases, op, form):
    a, b, want = cases[op]
    want = np.array(want, np.uint32)
    # 256-lane workgroups over the whole list, the last one partly filled
    got = np.concatenate([_run(pow29_lib, form, op, a[lo:lo + 256], b[lo:lo + 256] if b else None,
                               min(256, len(a) - lo)) for lo in range(0, len(a), 256)])
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"[{form}] {op}: {bad.size} of {len(a)} items differ, first {bad[:4]}: " \
                          f"{[hex(int(v)) for v in got[bad[0]]]} != {[hex(int(v)) for v in want[bad[0]]]}"
    # a 1-lane call: the last operand alone
    one = _run(pow29_lib, form, op, a[-1:], b[-1:] if b else None, 1)
    assert (one[0] == want[-1]).all(), f"[{form}] {op}: the 1-lane call differs"


def test_model_is_the_field(cases):
    """The expected rows are right as field elements, not only as limbs."""
    a, b, want = cases["mul"]
    for x, y, w in zip(a[::37], b[::37], want[::37]):
        assert ref.value(w) % ref.P == ref.value(x) * ref.value(y) % ref.P
    a, _, want = cases["pow_p58"]
    for x, w in zip(a[::97], want[::97]):
        z = sum(v << (32 * k) for k, v in enumerate(x))
        assert sum(v << (32 * k) for k, v in enumerate(w)) % ref.P == pow(z, (ref.P - 5) // 8, ref.P)

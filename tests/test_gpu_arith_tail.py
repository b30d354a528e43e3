"""GPU: sums_tail::prologue (csrc/coa_sums_tail.h), the row prologue that gives a
tail lane of k_verify_main_sums its digits above the loop's cap, on its RAW
output limbs against Python big integers (tests/arith_ref.py), through
tests/arith/tail_check.hip in both assembled forms of the rare carry blocks.
For excess lengths no signature pool reaches.

256 lanes (four waves) of synthetic records and tables, the prologue from digit
position 33:
* excess lengths 1, 2, 3, 8 and 31 (H = 64, the (k, 1) fallback of the halving),
  several in one wave, so different lengths share a wave's loop;
* both signs of d; A digits -8, 0, 7 and R digits -8, 0, 7 and (negated) 8 at the
  top position, random digits below it, random digits below position 33 that
  the prologue must not read;
* p and q from arith_ref.point_pool(), mixed-order ones and q = p, q = -p included;
* lanes that are not tail lanes keep the identity they came with.

A tail lane's result is 16 (C p + D q), C / D the excess digits of c / sign(d) |d|
as numbers; compared as a projective class (affine x, y and T Z == X Y)."""
import ctypes
import os
import random

import numpy as np
import pytest

import arith_ref as ar
import ed25519_ref as o

pytestmark = pytest.mark.gpu

FORMS = {"out_of_line": 0, "rare_inline": 1}
FILL = 0x5A5A5A5A
GUARD = 64
N = 256
LO = 33
TOP = [(-8, -8), (0, 7), (7, 0), (-8, 0), (0, -8), (7, 7), (0, 0), (7, -8)]  # (A digit, |d| digit) at position H - 1


@pytest.fixture(scope="module")
def tail_lib(engine):
    import torch

    path = os.path.join(os.path.dirname(engine.LIB_PATH), "libcoa_tailcheck.so")
    assert os.path.exists(path), f"{path} not built"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.coa_tail_run.argtypes = [ctypes.c_int, vp, vp, vp, vp, ctypes.c_int, ctypes.c_uint32, vp, vp, vp]
    lib.coa_tail_run.restype = ctypes.c_int
    torch.cuda.set_device(0)
    return lib


def _items():
    """256 x (p, q, tail, H, neg, c digits[64], d digits[64])."""
    rng = random.Random("coa-sums-tail")
    pts, mixed, _ = ar.point_pool()
    allp = pts + mixed
    items = []
    for i in range(N):
        if i % 32 == 5:
            e = 31
        elif i % 8 == 2:
            e = 8
        else:
            e = 1 + i % 3
        tail = i % 4 != 3
        H = LO + e if tail or i % 8 == 3 else rng.choice([0, 31, 33])  # some non-tail lanes with digits up there
        neg = (i >> 1) & 1
        dc = [rng.randrange(-8, 8) for _ in range(64)]
        dd = [rng.randrange(-8, 8) for _ in range(64)]
        for pos in range(H, 64):
            dc[pos] = dd[pos] = 0
        if H > LO:
            dc[H - 1], dd[H - 1] = TOP[(i // 3) % 8]
        p = allp[rng.randrange(len(allp))]
        q = allp[rng.randrange(len(allp))]
        if i % 31 == 0:
            q = p
        if i % 37 == 1:
            q = o.pneg(p)
        items.append((p, q, tail, H, neg, dc, dd))
    return items


def _words(digits):
    v = sum((d + 8) << (4 * pos) for pos, d in enumerate(digits))
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


def _i32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def expected():
    items = _items()
    want = []
    for p, q, tail, H, neg, dc, dd in items:
        if not tail:
            want.append(o.IDENT)
            continue
        C = sum(dc[pos] << (4 * (pos - LO)) for pos in range(LO, H))
        D = sum((-dd[pos] if neg else dd[pos]) << (4 * (pos - LO)) for pos in range(LO, H))
        want.append(o.padd(o.pmul(16 * abs(C), p if C >= 0 else o.pneg(p)),
                           o.pmul(16 * abs(D), q if D >= 0 else o.pneg(q))))
    return items, want


def test_cases_cover(expected):
    items, _ = expected
    tails = [it for it in items if it[2]]
    assert {it[3] - LO for it in tails} == {1, 2, 3, 8, 31}
    assert {it[4] for it in tails} == {0, 1}
    assert {it[5][it[3] - 1] for it in tails} == {-8, 0, 7} == {it[6][it[3] - 1] for it in tails}
    assert any(it[4] and it[6][it[3] - 1] == -8 for it in tails), "an R digit of +8"
    for w in range(4):  # different excess lengths in every wave
        assert len({it[3] for it in items[64 * w:64 * w + 64] if it[2]}) >= 4
    assert any(not it[2] and it[3] > LO for it in items)


@pytest.mark.parametrize("form", list(FORMS))
def test_prologue(tail_lib, expected, form):
    import torch

    items, want = expected
    rng = random.Random("coa-sums-tail-repr")

    def affine_words(pt):
        x, y = ar._affine(pt)
        v = (x + ar.P * rng.getrandbits(1)) | ((y + ar.P * rng.getrandbits(1)) << 256)
        return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(16)]

    rec = np.zeros((N, 32), np.uint32)
    for i, (_, _, _, H, neg, dc, dd) in enumerate(items):
        rec[i, 0:8] = _words(dc)
        rec[i, 8:16] = _words(dd)
        rec[i, 16:24] = [rng.getrandbits(32) for _ in range(8)]
        rec[i, 24] = H | (neg << 31)
    d_p = _i32([affine_words(it[0]) for it in items])
    d_q = _i32([affine_words(it[1]) for it in items])
    d_rec = _i32(rec)
    d_ctl = _i32([1 if it[2] else 0 for it in items])
    dev = torch.device("cuda", 0)
    d_scr = torch.zeros(N * tail_lib.coa_tail_slab_words(), dtype=torch.int32, device=dev)
    fill = np.array([FILL], np.uint32).view(np.int32)[0]
    d_out = torch.full((N * 32 + GUARD,), int(fill), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = tail_lib.coa_tail_run(FORMS[form], d_p.data_ptr(), d_q.data_ptr(), d_rec.data_ptr(), d_ctl.data_ptr(), LO, N,
                               d_scr.data_ptr(), d_out.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, f"[{form}]: coa_tail_run returned HIP error {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[N * 32:] == FILL).all(), f"[{form}]: wrote past its output"
    out = out[:N * 32].reshape(N, 32)
    bad = []
    for i, (it, w) in enumerate(zip(items, want)):
        err = ar._point([int(x) for x in out[i]], w, f"tail {it[2]} H {it[3]} neg {it[4]}")
        if err:
            bad.append(f"[{form}] lane {i}: {err}")
    assert not bad, f"{len(bad)} of {N} wrong:\n" + "\n".join(bad[:6])

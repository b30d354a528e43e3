"""GPU: ge_add_cc_il (csrc/coa_ge_sums.h), the sum of two addend-form points that
k_verify_main_sums' producer waves compute, on its RAW output limbs against
Python big integers (tests/arith_ref.py), through tests/arith/sums_check.hip in
both assembled forms of the rare carry blocks.

* add_cc: 256 lanes of point pairs in random projective representations --
  P + P, P + (-P), P + O, O + P, O + O, P + each torsion point, every pair of
  the eight small-order points, random and mixed-order pairs -- with the four
  combinations of negated operands in turn (negated as tab2_load negates: the
  Y+X / Y-X halves swapped, the T product's sign handed to the addition), and
  lanes whose p or q is the literal identity entry a zero digit reads.
* tab_sum: 256 lanes of dp * p + dq * q for digits -8 .. 8 through tab2_build
  (table 0, cached), tab2_build_form (table 1, plain T), tab2_load and ge_add_cc_il:
  the producer's path for one digit.

The result is compared as a projective class (affine x, y and T Z == X Y)."""
import ctypes
import os
import random

import numpy as np
import pytest

import arith_ref as ar
import ed25519_ref as o

pytestmark = pytest.mark.gpu

FORMS = {"out_of_line": 0, "rare_inline": 1}
OPS = {"add_cc": 0, "tab_sum": 1}  # the enum of tests/arith/sums_check.hip
FILL = 0x5A5A5A5A
GUARD = 64
N = 256


@pytest.fixture(scope="module")
def sums_lib(engine):
    import torch

    path = os.path.join(os.path.dirname(engine.LIB_PATH), "libcoa_sumscheck.so")
    assert os.path.exists(path), f"{path} not built"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.coa_sums_run.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, ctypes.c_uint32, vp, vp, vp]
    lib.coa_sums_run.restype = ctypes.c_int
    assert lib.coa_sums_op_count() == len(OPS)
    torch.cuda.set_device(0)
    return lib


def _dev(vals, nwords):
    import torch

    raw = b"".join(v.to_bytes(4 * nwords, "little") for v in vals)
    arr = np.frombuffer(raw, np.uint32).reshape(len(vals), nwords)
    return torch.from_numpy(arr.view(np.int32).copy()).to(torch.device("cuda", 0))


def _run(lib, name, form, a, b, c, nwords):
    import torch

    n = len(a)
    dev = torch.device("cuda", 0)
    d_a, d_b = _dev(a, nwords), _dev(b, nwords)
    d_c = torch.tensor(c, dtype=torch.int32, device=dev).reshape(n, 2).contiguous()
    d_scr = torch.zeros(n * lib.coa_sums_slab_words(), dtype=torch.int32, device=dev)
    fill = np.array([FILL], np.uint32).view(np.int32)[0]
    d_out = torch.full((n * 32 + GUARD,), int(fill), dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev)
    rc = lib.coa_sums_run(OPS[name], FORMS[form], d_a.data_ptr(), d_b.data_ptr(), d_c.data_ptr(), n,
                          d_scr.data_ptr(), d_out.data_ptr(), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, f"{name} [{form}]: coa_sums_run returned HIP error {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[n * 32:] == FILL).all(), f"{name} [{form}]: wrote past its output"
    return out[:n * 32].reshape(n, 32)


def _add_cc_items():
    """256 (p, q, control word)."""
    rng = random.Random("coa-sums-add-cc")
    special, rand = ar.point_pairs(rng, N)
    pairs = (special + rand)[:N]
    assert len(special) < N and len(pairs) == N
    O = o.IDENT
    assert (O, O) in special and any(p == q != O for p, q in special) and any(q == o.pneg(p) != p for p, q in special)
    tors = o.torsion_points()
    assert all((s, t) in special for s in tors for t in tors)
    items = []
    for i, (p, q) in enumerate(pairs):
        ctl = i % 4                      # bit 0 / 1: p / q negated
        if i % 16 == 5:
            ctl |= 4                     # p is the literal identity entry
        if i % 16 == 11 or i % 64 == 21:
            ctl |= 8                     # q is
        items.append((p, q, ctl))
    return items


@pytest.mark.parametrize("form", list(FORMS))
def test_add_cc(sums_lib, form):
    rng = random.Random("coa-sums-add-cc-repr")
    items = _add_cc_items()
    assert {c & 3 for _, _, c in items} == {0, 1, 2, 3}
    assert {c >> 2 for _, _, c in items} == {0, 1, 2, 3}
    a = [ar.pack_p3(ar.scale(p, rng)) for p, _, _ in items]
    b = [ar.pack_p3(ar.scale(q, rng)) for _, q, _ in items]
    c = [[ctl, 0] for _, _, ctl in items]
    out = _run(sums_lib, "add_cc", form, a, b, c, 32)
    bad = []
    for i, (p, q, ctl) in enumerate(items):
        pp = o.IDENT if ctl & 4 else (o.pneg(p) if ctl & 1 else p)
        qq = o.IDENT if ctl & 8 else (o.pneg(q) if ctl & 2 else q)
        err = ar._point([int(w) for w in out[i]], o.padd(pp, qq), f"(+-p) + (+-q), control {ctl:#x}")
        if err:
            bad.append(f"add_cc [{form}] index {i}: {err}")
    assert not bad, f"{len(bad)} of {len(items)} wrong:\n" + "\n".join(bad[:6])


def _tab_sum_items():
    """256 (p, q, dp, dq): every digit -8 .. 8 on either side, zero digits
    included, all sign pairs; p and q random, mixed order or torsion."""
    rng = random.Random("coa-sums-tab")
    pts, mixed, tors = ar.point_pool()
    allp = pts + mixed
    items = []
    for i in range(N):
        dp, dq = i % 17 - 8, (i // 17 * 5 + i) % 17 - 8
        p = tors[i % 8] if i % 23 == 7 else allp[rng.randrange(len(allp))]
        q = tors[(i // 8) % 8] if i % 29 == 3 else allp[rng.randrange(len(allp))]
        if i % 31 == 0:
            q = p
        if i % 37 == 1:
            q = o.pneg(p)
        items.append((p, q, dp, dq))
    return items


@pytest.mark.parametrize("form", list(FORMS))
def test_tab_sum(sums_lib, form):
    rng = random.Random("coa-sums-tab-repr")
    items = _tab_sum_items()
    assert {d for _, _, d, _ in items} == set(range(-8, 9)) == {d for _, _, _, d in items}
    assert {(dp < 0, dq < 0) for _, _, dp, dq in items if dp and dq} == {(False, False), (False, True), (True, False),
                                                                        (True, True)}
    assert any(dp == 0 and dq == 0 for _, _, dp, dq in items)

    def affine_words(pt):
        x, y = ar._affine(pt)
        return (x + ar.P * rng.getrandbits(1)) | ((y + ar.P * rng.getrandbits(1)) << 256)

    a = [affine_words(p) for p, _, _, _ in items]
    b = [affine_words(q) for _, q, _, _ in items]
    c = [[dp + 8, dq + 8] for _, _, dp, dq in items]
    out = _run(sums_lib, "tab_sum", form, a, b, c, 16)
    bad = []
    for i, (p, q, dp, dq) in enumerate(items):
        want = o.padd(o.pmul(abs(dp), p if dp >= 0 else o.pneg(p)), o.pmul(abs(dq), q if dq >= 0 else o.pneg(q)))
        err = ar._point([int(w) for w in out[i]], want, f"({dp}) p + ({dq}) q")
        if err:
            bad.append(f"tab_sum [{form}] index {i}: {err}")
    assert not bad, f"{len(bad)} of {len(items)} wrong:\n" + "\n".join(bad[:6])

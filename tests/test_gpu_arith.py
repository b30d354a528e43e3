"""GPU: every device arithmetic primitive of csrc/coa_fe.h, coa_fe_wave.h,
coa_sc.h, coa_halve.h and coa_ge.h against Python big integers, on its RAW
output limbs (tests/arith/arith_check.hip wraps each primitive in a trivial
kernel; tests/arith_ref.py has the references and builds the operands).

Exact integer comparisons only.  Each op runs in both assembled forms of the
rare carry blocks (out of line, and COA_RARE_INLINE as coa_latency.hip,
coa_committee.hip, coa_cert_lat.hip and coa_keybuild.hip build them), on operands constructed to take every path --
the second carry pass and its carry out, 0 / 1 final subtractions of l, a
rippling row normalisation -- placed so that a wave holds only rare lanes, one
rare lane (first, last), alternating ones and none; with a partial last wave
(n = 64 m + 37) and n = 1; and from divergent callers (a mask: alternating
lanes, lane 5 alone, the first 32), where masked lanes must keep the sentinel.
Row ops: each 16-lane row has its own operand, exactly one row of a wave
ripples (each of the four in turn), and whole rows sit out.

tests/test_arith_operands.py (CPU) asserts that the operand sets really hold
>= 64 operands on every path."""
import ctypes
import os

import numpy as np
import pytest

import arith_ref as ar

pytestmark = pytest.mark.gpu

FORMS = {"out_of_line": 0, "rare_inline": 1}
FILL = 0x5A5A5A5A  # what the output buffer holds before a run
GUARD = 64         # words past the output that must stay FILL


@pytest.fixture(scope="module")
def arith(engine):
    """libcoa_arithcheck.so beside the engine library, loaded after the engine
    fixture (which imported torch first and built everything)."""
    import torch

    path = os.path.join(os.path.dirname(engine.LIB_PATH), "libcoa_arithcheck.so")
    assert os.path.exists(path), f"{path} not built"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.coa_arith_run.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_uint32, vp, vp]
    lib.coa_arith_run.restype = ctypes.c_int
    torch.cuda.set_device(0)
    return lib


def _pack(vals, nwords):
    if nwords == 0:
        return None
    raw = b"".join(v.to_bytes(4 * nwords, "little") for v in vals)
    return np.frombuffer(raw, np.uint32).reshape(len(vals), nwords)


def _run(lib, name, form, items, mask=None):
    """Raw output words, shape (n, nout), of op `name` on `items`."""
    import torch

    op = ar.OPS[name]
    n = len(items)
    dev = torch.device("cuda", 0)
    bufs = []
    for vals, nw in (([it.a for it in items], op.na), ([it.b for it in items], op.nb), ([it.c for it in items], op.nc)):
        arr = _pack(vals, nw)
        bufs.append(None if arr is None else torch.from_numpy(arr.view(np.int32).copy()).to(dev))
    d_mask = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=dev)
    fill = np.array([FILL], np.uint32).view(np.int32)[0]
    d_out = torch.full((n * op.nout + GUARD,), int(fill), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    stream = torch.cuda.current_stream(dev)
    rc = lib.coa_arith_run(op.id, FORMS[form], ptr(bufs[0]), ptr(bufs[1]), ptr(bufs[2]), ptr(d_mask), n,
                           ptr(d_out), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, f"{name} [{form}]: coa_arith_run returned HIP error {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[n * op.nout:] == FILL).all(), f"{name} [{form}]: wrote past its {n} x {op.nout} output words"
    return out[:n * op.nout].reshape(n, op.nout)


_checked = {}


def _check(name, it, row):
    """ar.check, computed once per (operand, output): the two forms and the
    repeated placements of an operand share the reference work."""
    key = (name, it, row.tobytes())
    if key not in _checked:
        _checked[key] = ar.check(name, it, row)
    return _checked[key]


def _verify(name, form, tag, items, out, mask=None):
    g = 16 if ar.OPS[name].rows else 1
    bad = []
    for i, it in enumerate(items):
        if mask is not None and not mask[i]:
            err = None if (out[i] == ar.SENTINEL).all() else \
                "masked item lost the sentinel: " + " ".join(f"{int(w):08x}" for w in out[i])
        else:
            err = _check(name, it, out[i])
            if err is None and mask is not None and (out[i] == ar.SENTINEL).all():
                err = "active item holds the sentinel"
        if err:
            bad.append(f"{name} [{form}] {tag}: index {i} (wave {i * g // 64}, lane {i * g % 64}) "
                       f"{ar.describe(name, it)}\n    {err}")
    assert not bad, f"{len(bad)} of {len(items)} wrong:\n" + "\n".join(bad[:6])


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", list(ar.OPS))
def test_primitive(arith, name, form):
    # lane mixes and the partial last wave
    items = ar.lane_mix_layout(name)
    assert len(items) % ar.group_size(name) == (37 if ar.group_size(name) == 64 else 3)
    _verify(name, form, "lane mix", items, _run(arith, name, form, items))
    # n == 1: a single lane (row) of a single wave, on a rare operand
    one = [next(it for it in items if it.rare)]
    _verify(name, form, "n=1", one, _run(arith, name, form, one))
    # divergent callers
    for tag, mitems, mask in ar.masked_layouts(name):
        _verify(name, form, "mask " + tag, mitems, _run(arith, name, form, mitems, mask), mask)


def test_entry_point_contract(arith):
    """n == 0 succeeds without a launch (null pointers are never touched) and
    an unknown op is an error, not a launch."""
    for form in FORMS.values():
        assert arith.coa_arith_run(0, form, None, None, None, None, 0, None, None) == 0
        assert arith.coa_arith_run(len(ar.OPS), form, None, None, None, None, 0, None, None) != 0
        assert arith.coa_arith_run(-1, form, None, None, None, None, 1, None, None) != 0

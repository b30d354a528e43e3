"""GPU: what the out-of-place carry chains, the signed table lookups and the
doubling table build must keep exact.

* fe_add / fe_sub / fe_addsub (csrc/coa_fe.h) write fresh early-clobber
  outputs; the forms in which a result aliases an operand -- r = a, r = b,
  (a, a, a), s or d of fe_addsub on either input -- run through
  tests/arith/alias_check.hip in both assembled forms of the rare carry
  blocks, once and three times round a loop (the aliased register is then
  really carried), on the operand sets of tests/arith_ref.py: second carry
  pass not taken, taken, and with its own carry out.  Results are compared
  with arith_ref's integers mod p and, word for word, with the chains' stated
  algorithm (a + b with 2^256 folded as 38, twice).  n = 1 and n = 2 * 64 + 37;
  masked lanes keep the sentinel.
* signed lookups: p + d * q for d = -8 .. 8 through tab2_build / tab2_load
  (csrc/coa_smul.h) and ge_add / ge_add_il, against arith_ref's point
  addition, n = 64 + 37.
* table build: the slab k_pre_halve wrote for 101 items (random valid points,
  the eight torsion points, mixed-order points, y >= p and non-decompressible
  encodings): all 16 entries per item equal j * (-P), and the flag bytes
  equal the oracle's decompression / small-order / canonical-s answers.
* end to end: verify_strict_many_device against the C oracle at n = 1, 63, 64,
  65, 257 (k_verify_main2), 16,385 (k_verify_main<1, true>) and 65,536 with
  COA_MAIN_IL=0 (k_verify_main<3, false>), the eight adversarial classes
  present."""
import ctypes
import os
import random

import numpy as np
import pytest

import arith_ref as ar
import coa_oracle as co
import ed25519_ref as o
from conftest import load_golden

gpu = pytest.mark.gpu

FORMS = {"out_of_line": 0, "rare_inline": 1}
FILL = 0x5A5A5A5A
GUARD = 64
B256, M32, P = ar.B256, ar.M32, ar.P

# the ops of tests/arith/alias_check.hip, in the order of its enum: (na, nb, nc, nout)
OPS = {name: (i,) + dims for i, (name, dims) in enumerate(
    [(n, (8, 8, 0, 8)) for n in ("add_ra", "add_rb", "add_aaa", "sub_ra", "sub_rb", "sub_aaa")] +
    [(n, (8, 8, 0, 16)) for n in ("addsub_sa", "addsub_sb", "addsub_da", "addsub_db", "addsub_sadb")] +
    [(n, (32, 16, 1, 32)) for n in ("tab_add", "tab_add_il")])}


@pytest.fixture(scope="module")
def alias(engine):
    import torch

    path = os.path.join(os.path.dirname(engine.LIB_PATH), "libcoa_aliascheck.so")
    assert os.path.exists(path), f"{path} not built"
    lib = ctypes.CDLL(path)
    vp = ctypes.c_void_p
    lib.coa_alias_run.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_int, vp, vp, vp]
    lib.coa_alias_run.restype = ctypes.c_int
    assert lib.coa_alias_op_count() == len(OPS)
    torch.cuda.set_device(0)
    return lib


def _dev(vals, nwords):
    import torch

    raw = b"".join(v.to_bytes(4 * nwords, "little") for v in vals)
    arr = np.frombuffer(raw, np.uint32).reshape(len(vals), nwords)
    return torch.from_numpy(arr.view(np.int32).copy()).to(torch.device("cuda", 0))


def _run(lib, name, form, a, b, c=None, mask=None, reps=1):
    """Raw output words, shape (n, nout), of op `name` on the operand lists."""
    import torch

    op, na, nb, nc, nout = OPS[name]
    n = len(a)
    dev = torch.device("cuda", 0)
    d_a, d_b = _dev(a, na), _dev(b, nb)
    d_c = _dev(c, nc) if nc else None
    d_mask = None if mask is None else torch.tensor(mask, dtype=torch.uint8, device=dev)
    d_scr = torch.zeros(n * lib.coa_alias_slab_words(), dtype=torch.int32, device=dev) if nc else None
    fill = np.array([FILL], np.uint32).view(np.int32)[0]
    d_out = torch.full((n * nout + GUARD,), int(fill), dtype=torch.int32, device=dev)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    stream = torch.cuda.current_stream(dev)
    rc = lib.coa_alias_run(op, FORMS[form], ptr(d_a), ptr(d_b), ptr(d_c), ptr(d_mask), n, reps, ptr(d_scr),
                           ptr(d_out), ctypes.c_void_p(stream.cuda_stream))
    assert rc == 0, f"{name} [{form}]: coa_alias_run returned HIP error {rc}"
    stream.synchronize()
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[n * nout:] == FILL).all(), f"{name} [{form}]: wrote past its {n} x {nout} output words"
    return out[:n * nout].reshape(n, nout)


# ---------------------------------------------------------------------------
# aliasing forms of the carry chains
# ---------------------------------------------------------------------------
def add_words(a, b):
    """fe_add as coa_fe.h states it: a + b mod 2^256, the carry folded as 38,
    and the carry of that fold folded once more."""
    s = a + b
    for _ in range(2):
        s = (s & (B256 - 1)) + 38 * (s >> 256)
    assert s < B256
    return s


def sub_words(a, b):
    """fe_sub: a - b + 2^256 per borrow, 38 subtracted per borrow, twice."""
    d = a - b
    for _ in range(2):
        if d < 0:
            d += B256 - 38
    assert 0 <= d < B256
    return d


def model(name, a, b, reps):
    """(exact result words as integers, (x, y) operands of the LAST pass)."""
    if name.startswith(("add_", "sub_")):
        f = add_words if name.startswith("add_") else sub_words
        r = b if name.endswith("_rb") else a
        for _ in range(reps):
            x, y = {"ra": (r, b), "rb": (a, r), "aaa": (r, r)}[name.split("_")[1]]
            r = f(x, y)
        return [r], (x, y)
    s, d = (b if name == "addsub_sb" else a), (a if name == "addsub_da" else b)
    for _ in range(reps):
        x, y = {"addsub_sa": (s, b), "addsub_sb": (a, s), "addsub_da": (d, b), "addsub_db": (a, d),
                "addsub_sadb": (s, d)}[name]
        s, d = add_words(x, y), sub_words(x, y)
    return [s, d], (x, y)


def _aaa_pairs(rng):
    """a + a on each path: 2a wraps to all ones above word 0 (path 2), or to a
    low word within 38 of 2^32 (path 1)."""
    p2 = [B256 - 1 - i for i in range(19)]
    p1 = []
    while len(p1) < 48:
        s = B256 + ((rng.getrandbits(223) << 32) | (M32 - (2 * rng.randrange(19) + 1)))
        p1.append(s // 2)
    return p2, p1


def _operands(name):
    """165 (a, b) pairs for op `name`: wave 0 all on the rare paths, wave 1
    alternating rare / common, the 37 lanes of wave 2 common but the first and
    the last."""
    rng = random.Random("coa-alias-" + name)
    kind = "fe_add" if name.startswith("add_") else "fe_sub" if name.startswith("sub_") else "fe_addsub"
    its = ar.operands(kind)
    if name == "add_aaa":
        p2, p1 = _aaa_pairs(rng)
        c2, c1 = [(a, a) for a in p2], [(a, a) for a in p1]
    else:
        c2 = [(it.a, it.b) for it in its if it.cls == 2]
        c1 = [(it.a, it.b) for it in its if it.cls == 1]
    c0 = [(it.a, it.b) for it in its if it.cls == 0 and it.rand]
    rng.shuffle(c2)
    rng.shuffle(c1)
    assert len(c2) >= 19 and len(c1) >= 48 and len(c0) >= 32 + 35
    rare = [(c2, c1)[k % 2][(k // 2) % len((c2, c1)[k % 2])] for k in range(64 + 32 + 2)]  # both paths in turn
    out = rare[:64]
    k = 64
    for pos in range(64):
        out.append(rare[k + pos // 2] if pos % 2 else c0[pos // 2])
    k += 32
    out += [rare[k]] + c0[32:32 + 35] + [rare[k + 1]]
    assert len(out) == 2 * 64 + 37
    return out


def _check_alias(name, form, tag, ops, out, reps, mask=None):
    bad = []
    for i, (a, b) in enumerate(ops):
        row = [int(w) for w in out[i]]
        if mask is not None and not mask[i]:
            err = None if all(w == ar.SENTINEL for w in row) else "masked item lost the sentinel"
        else:
            want, (x, y) = model(name, a, b, reps)
            got = [ar.from_words(row[8 * k:8 * k + 8]) for k in range(len(want))]
            # arith_ref's integers for the last pass, mod p
            kind = "fe_add" if name.startswith("add_") else "fe_sub" if name.startswith("sub_") else "fe_addsub"
            err = ar.check(kind, ar.Item(x, y, None, 0, False, False), row)
            if err is None and got != want:
                err = "limbs: got " + " ".join(f"{g:#x}" for g in got) + ", want " + " ".join(f"{w:#x}" for w in want)
        if err:
            bad.append(f"{name} [{form}] {tag} reps={reps}: index {i} (wave {i // 64}, lane {i % 64}) "
                       f"a={a:#x} b={b:#x}\n    {err}")
    assert not bad, f"{len(bad)} of {len(ops)} wrong:\n" + "\n".join(bad[:6])


FE_OPS = [n for n, v in OPS.items() if v[3] == 0]


def test_operand_sets_take_every_path():
    """CPU part: the operands of each aliasing form hold the common path, the
    second pass and its carry out (by arith_ref's path predicates on the
    operands of the first pass)."""
    for name in FE_OPS:
        if name in ("sub_aaa", "addsub_sadb"):
            continue  # a - a never borrows; (s, d) = (a, b) is covered as the pair (a, b) below
        classes = set()
        for a, b in _operands(name):
            _, (x, y) = model(name, a, b, 1)
            pred = ar.fe_add_path if name.startswith("add_") else ar.fe_sub_path if name.startswith("sub_") \
                else ar.fe_addsub_path
            classes.add(pred(x, y))
        assert classes == {0, 1, 2}, (name, classes)


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", FE_OPS)
def test_aliasing_forms(alias, name, form):
    ops = _operands(name)
    a, b = [x for x, _ in ops], [y for _, y in ops]
    for reps in (1, 3):
        _check_alias(name, form, "n=165", ops, _run(alias, name, form, a, b, reps=reps), reps)
    # n == 1, on a rare operand
    _check_alias(name, form, "n=1", ops[:1], _run(alias, name, form, a[:1], b[:1]), 1)
    # a divergent caller: odd lanes only
    mask = [i % 2 for i in range(len(ops))]
    _check_alias(name, form, "mask", ops, _run(alias, name, form, a, b, mask=mask, reps=3), 3, mask)


# ---------------------------------------------------------------------------
# signed lookups
# ---------------------------------------------------------------------------
def _lookup_items():
    """101 (p, q, digit): digits -8 .. 8 in turn; q affine (random, mixed
    order, torsion), p random or one of the special relations to digit * q."""
    rng = random.Random("coa-alias-lookup")
    pts, mixed, tors = ar.point_pool()
    items = []
    for i in range(64 + 37):
        d = i % 17 - 8
        q = (pts + mixed + tors)[rng.randrange(len(pts) + len(mixed) + len(tors))] if i % 5 else tors[i % 8]
        dq = o.pmul(abs(d), q if d >= 0 else o.pneg(q))
        kind = i % 7
        p = {0: o.IDENT, 1: o.pneg(dq), 2: dq, 3: q}.get(kind, pts[rng.randrange(len(pts))])
        items.append((p, q, d))
    return items


@gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", ["tab_add", "tab_add_il"])
def test_signed_lookups(alias, name, form):
    rng = random.Random("coa-alias-lookup-repr")
    items = _lookup_items()
    assert {d for _, _, d in items} == set(range(-8, 9))
    a, b, c = [], [], []
    for p, q, d in items:
        a.append(ar.pack_p3(ar.scale(p, rng)))
        x, y = ar._affine(q)
        b.append((x + P * rng.getrandbits(1)) | ((y + P * rng.getrandbits(1)) << 256))
        c.append(d + 8)
    out = _run(alias, name, form, a, b, c)
    bad = []
    for i, (p, q, d) in enumerate(items):
        want = o.padd(p, o.pmul(abs(d), q if d >= 0 else o.pneg(q)))
        err = ar._point([int(w) for w in out[i]], want, f"p + ({d}) q")
        if err:
            bad.append(f"{name} [{form}] index {i} digit {d}: {err}")
    assert not bad, f"{len(bad)} of {len(items)} wrong:\n" + "\n".join(bad[:6])


# ---------------------------------------------------------------------------
# the table k_pre_halve builds
# ---------------------------------------------------------------------------
def _align(x, a=256):
    return (x + a - 1) // a * a


def _workspace_offsets(n):
    """Byte offsets of (flags, slabs) in a caller's workspace of n items
    (csrc/coa_sig.cpp ws_carve: k [n][32] | rec [n][128] | flags [2n] |
    [e]B [n][128] | slabs [n][2048], the first three rounded up to 256)."""
    flags = _align(n * 32) + _align(n * 128)
    return flags, flags + _align(2 * n) + n * 128


def _table_inputs(engine):
    from workloads import NONCANONICAL, OFF_CURVE, key_seeds, messages

    n = 101
    msgs = messages(n, 5000)
    pks, sigs = engine.sign_many(key_seeds(n, 5000), msgs)
    pool = load_golden("mixed_order_pool.json")
    tors = o.small_order_encodings()
    for i in range(n):
        k = i % 10
        enc = None
        if k == 1:
            enc = tors[(i // 10) % len(tors)]
        elif k == 2:
            enc = NONCANONICAL[(i // 10) % len(NONCANONICAL)]
        elif k == 3:
            enc = OFF_CURVE[(i // 10) % len(OFF_CURVE)]
        if enc is not None:  # A and R in turn, sometimes both
            if (i // 10) % 3 != 1:
                pks[i] = np.frombuffer(enc, np.uint8)
            if (i // 10) % 3 != 0:
                sigs[i, :32] = np.frombuffer(enc, np.uint8)
        elif k == 4:
            v = pool[(i // 10) % len(pool)]
            msgs[i] = np.frombuffer(bytes.fromhex(v["msg"]), np.uint8)
            pks[i] = np.frombuffer(bytes.fromhex(v["pk"]), np.uint8)
            sigs[i] = np.frombuffer(bytes.fromhex(v["sig"]), np.uint8)
        elif k == 5:  # s >= l: the A role's flag only
            s = int.from_bytes(bytes(sigs[i, 32:]), "little") + o.L
            sigs[i, 32:] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)
    return msgs, pks, sigs


@gpu
def test_table_build_and_flags(engine):
    import torch

    msgs, pks, sigs = _table_inputs(engine)
    n = len(pks)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (msgs, pks, sigs)]
    out = torch.ones(n, dtype=torch.uint8, device=dev)
    nbytes = engine.verify_workspace_bytes(n)
    f_off, s_off = _workspace_offsets(n)
    assert nbytes >= s_off + n * 2048
    ws = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    engine.verify_strict_many_device(0, t[0], t[1], t[2], out, ws)
    torch.cuda.synchronize()
    raw = ws.cpu().numpy()
    flags = raw[f_off:f_off + 2 * n].reshape(n, 2)
    slabs = raw[s_off:s_off + n * 2048].view(np.uint32).reshape(n, 2, 8, 4, 8)  # item, table, entry, coordinate, word
    i2 = pow(2, P - 2, P)
    bad, built = [], 0
    kinds = set()
    for i in range(n):
        s_ok = o.scalar_is_canonical(bytes(sigs[i, 32:]))
        for which, enc in ((0, bytes(pks[i])), (1, bytes(sigs[i, :32]))):
            pt = o.decompress(enc)
            want = pt is not None and not o.is_small_order(pt) and (which == 1 or s_ok)
            kinds.add((pt is None, pt is not None and o.is_small_order(pt), int.from_bytes(enc, "little") & ~(1 << 255) >= P))
            if int(flags[i, which]) != int(want):
                bad.append(f"item {i} role {which}: flag {flags[i, which]}, oracle {int(want)}")
                continue
            if not want:
                continue
            built += 1
            base = o.pneg(pt)
            for j in range(1, 9):
                ypx, ymx, Z, t2d = (ar.from_words(slabs[i, which, j - 1, c]) for c in range(4))
                x, y = ar._affine(o.pmul(j, base))
                zi = pow(Z, P - 2, P) if Z % P else 0
                got = ((ypx - ymx) * i2 * zi % P, (ypx + ymx) * i2 * zi % P, t2d * zi % P)
                if Z % P == 0 or got != (x, y, o.D2 * x * y % P):
                    bad.append(f"item {i} role {which} entry {j}: ({got[0]:#x}, {got[1]:#x}, 2dxy {got[2]:#x}), "
                               f"want ({x:#x}, {y:#x})")
    assert not bad, f"{len(bad)} wrong:\n" + "\n".join(bad[:6])
    # every kind of encoding was there: plain, non-decompressible, small order, y >= p
    assert {k[0] for k in kinds} == {False, True} and any(k[1] for k in kinds) and any(k[2] for k in kinds)
    assert built > n  # most tables of both roles were checked
    exp = co.verify_strict_many(msgs, pks, sigs, 1)
    assert (out.cpu().numpy() == exp).all()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def _pool():
    return [(bytes.fromhex(v["msg"]), bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]))
            for v in load_golden("mixed_order_pool.json")]


@gpu
@pytest.mark.parametrize("n,frac,env", [(1, 1.0, {}), (63, 0.5, {}), (64, 0.5, {}), (65, 0.5, {}), (257, 0.5, {}),
                                        (16_385, 0.02, {}), (65_536, 0.01, {"COA_MAIN_IL": "0"})])
def test_end_to_end_vs_c_oracle(engine, n, frac, env, monkeypatch):
    import torch

    from workloads import adversarial_mix, key_seeds, messages

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m0 = messages(n, 7000)
    pks, sigs = engine.sign_many(key_seeds(n, 7000), m0)
    msgs, pks, sigs, cls = adversarial_mix(m0, pks, sigs, frac=frac, seed=n, mixed_pool=_pool())
    if n >= 63:
        assert set(np.unique(cls[cls >= 0])) == set(range(8))
    exp = co.verify_strict_many(msgs, pks, sigs, min(16, os.cpu_count() or 1))
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (msgs, pks, sigs)]
    out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    engine.verify_strict_many_device(0, t[0], t[1], t[2], out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    mism = np.nonzero(got != exp)[0]
    assert mism.size == 0, [(int(i), int(cls[i]), int(got[i])) for i in mism[:20]]
    assert (got[cls == -1] == 0).all()

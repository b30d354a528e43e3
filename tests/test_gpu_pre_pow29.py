"""GPU: k_pre_halve's decompressions (csrc/coa_ge_dec29.h: the (p-5)/8 chain
on 29-bit limbs, no nu*i product, squares shared with the small-order test)
through the public verify call, k_pre_halve plus the main kernel, at n = 1,
256 and 257.

Every call mixes valid triples, the decompression classes of
tests/golden/verify_vectors.json (encodings with y >= p, "negative zero",
points off the curve, small-order points), all small-order encodings of the
oracle -- the eight points, both signs, y and y + p -- as A and as R, and a
non-canonical s.  Verdicts must equal the oracle's, item for item.

With a COA_PRE_POW29=0 library at build/pre_pow29_0/ (tools/build_variant.py
pre_pow29_0 -DCOA_PRE_POW29=0) the same sets go through it in a fresh process
and its verdict bytes must be identical."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":  # the variant-library child: the paths conftest.py sets up
    for p in (os.path.join(ROOT, "xrpl-coa-prototype_amd"), os.path.join(ROOT, "oracle"), ROOT,
              os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)

import ed25519_ref as o  # noqa: E402
from conftest import load_golden  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = (1, 256, 257)
VARIANT = os.path.join(ROOT, "build", "pre_pow29_0", "libcoa_verify.so")
CLASSES = ("noncanonical_R", "noncanonical_A", "small_order_R", "small_order_A", "small_order_A_eq", "off_curve",
           "s_plus_l", "s_high_bit", "mixed_order_A", "valid")


def _signed(i):
    sd = o.sha512(b"coa-pre-pow29" + struct.pack("<Q", i))[:32]
    m = o.sha512(b"coa-pre-pow29-msg" + struct.pack("<Q", i))[:32]
    return m, o.public_key(sd), o.sign(sd, m)


def _pool():
    """(msg, pk, sig, what) items, 32-byte messages, most interesting first."""
    items = []
    gold = [v for v in load_golden("verify_vectors.json") if len(v["msg"]) == 64 and v["class"] in CLASSES]
    so = o.small_order_encodings()
    m, pk, sg = _signed(0)
    items.append((m, pk, sg, "valid"))  # n = 1 is a valid triple; the next sizes start the same way
    for k, enc in enumerate(so):
        m, pk, sg = _signed(1 + k)
        items.append((m, enc, sg, f"small-order A #{k}"))
        items.append((m, pk, enc + sg[32:], f"small-order R #{k}"))
    m, pk, sg = _signed(100)
    items.append((m, pk, sg[:32] + (int.from_bytes(sg[32:], "little") + o.L).to_bytes(32, "little"), "s + l"))
    for v in gold:
        items.append((bytes.fromhex(v["msg"]), bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]),
                      f"golden {v['class']}: {v['note']}"))
    k = 0
    while len(items) < max(SIZES):
        m, pk, sg = _signed(200 + k)
        if k % 5 == 4:  # a tampered R that still decompresses or not, as it falls
            sg = bytes([sg[0] ^ 1]) + sg[1:]
        items.append((m, pk, sg, "valid" if k % 5 != 4 else "R bit flipped"))
        k += 1
    return items


def _sets():
    """{n: (msgs, pks, sigs, notes)}: n = 1 the valid triple, 256 and 257 the mixed pool; 257 rotated by one
    workgroup position so every class also meets the second workgroup's first lane."""
    pool = _pool()
    assert len(pool) >= max(SIZES)
    out = {}
    for n in SIZES:
        items = pool[:n] if n != 257 else pool[1:257] + pool[:1]
        arr = lambda k, w: np.frombuffer(b"".join(it[k] for it in items), np.uint8).reshape(n, w).copy()
        out[n] = (arr(0, 32), arr(1, 32), arr(2, 64), [it[3] for it in items])
    return out


@pytest.fixture(scope="module")
def sets():
    return _sets()


@pytest.fixture(scope="module")
def oracle_verdicts(sets):
    return {n: np.array([o.verify_strict(bytes(m), bytes(p), bytes(s)) for m, p, s in zip(ms, ps, ss)])
            for n, (ms, ps, ss, _) in sets.items()}


def test_sets_cover(sets, oracle_verdicts):
    _, pks, sigs, notes = sets[256]
    so = set(o.small_order_encodings())
    assert len({bytes(p) for p in pks} & so) == len(so) == len({bytes(s[:32]) for s in sigs} & so)
    assert len(so) >= 8
    for cls in ("noncanonical_R", "noncanonical_A", "off_curve", "small_order_A", "small_order_R", "s_plus_l"):
        assert any(f"golden {cls}" in t for t in notes), cls
    assert any("s + l" in t for t in notes)
    ok = oracle_verdicts[256]
    assert ok.any() and (~ok).any()
    assert oracle_verdicts[1].all()
    assert sets[257][3][:255] == notes[1:] and sets[257][3][-1] == notes[0]


@pytest.mark.parametrize("n", SIZES)
def test_verdicts_equal_the_oracle(engine, sets, oracle_verdicts, n):
    msgs, pks, sigs, notes = sets[n]
    got = engine.verify_strict_many(msgs, pks, sigs) == 0
    bad = np.nonzero(got != oracle_verdicts[n])[0]
    assert bad.size == 0, [(int(i), notes[i], bool(got[i])) for i in bad[:8]]


def test_variant_library_gives_identical_bytes(engine, sets, tmp_path):
    if not os.path.exists(VARIANT):
        pytest.skip("no COA_PRE_POW29=0 library at build/pre_pow29_0/ (tools/build_variant.py)")
    out = str(tmp_path / "variant.npz")
    env = dict(os.environ, COA_VERIFY_LIB=VARIANT)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    theirs = np.load(out)
    for n, (msgs, pks, sigs, _) in sets.items():
        ours = engine.verify_strict_many(msgs, pks, sigs)
        assert ours.tobytes() == theirs[str(n)].tobytes(), n


if __name__ == "__main__":
    import torch  # noqa: F401  (first: one HIP runtime in the process)

    import coa_crypto

    assert coa_crypto.LIB_PATH == os.environ["COA_VERIFY_LIB"]
    np.savez(sys.argv[1], **{str(n): coa_crypto.verify_strict_many(ms, ps, ss) for n, (ms, ps, ss, _) in _sets().items()})

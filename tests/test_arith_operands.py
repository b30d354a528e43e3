"""CPU side of the device arithmetic checks (tests/test_gpu_arith.py): the
side library builds for gfx950, the big-integer references of
tests/arith_ref.py agree with the oracle, and -- the condition that keeps the
GPU tests from silently degrading to random data -- the operand set of every
op with rare paths holds at least 64 operands on each path, by the limb-level
path predicates."""
import collections
import ctypes
import os
import subprocess

import pytest

import arith_ref as ar
import ed25519_ref as o

P, L = ar.P, ar.L


@pytest.fixture(scope="module")
def arith_lib():
    import build  # xrpl-coa-prototype_amd/build.py

    build.build()
    assert os.path.exists(build.ARITH_LIB), "libcoa_arithcheck.so not built"
    return build.ARITH_LIB


def test_side_library_builds_and_exports(arith_lib):
    """lib/libcoa_arithcheck.so, beside the engine: a gfx950 code object from
    each of the two compilations, and the entry points."""
    import build

    assert os.path.dirname(arith_lib) == os.path.dirname(build.LIB)
    lib = ctypes.CDLL(arith_lib)
    for sym in ("coa_arith_run", "coa_arith_run_out", "coa_arith_run_inl", "coa_arith_dims", "coa_arith_op_count"):
        assert hasattr(lib, sym), sym
    blob = open(arith_lib, "rb").read()
    assert blob.count(b"amdgcn-amd-amdhsa--gfx950") >= 2
    needed = subprocess.run(["readelf", "-d", arith_lib], capture_output=True, text=True).stdout
    assert "libamdhip64.so" in needed  # by soname: the process's one HIP runtime (torch's) serves it
    # the kernels of both forms, out of line and COA_RARE_INLINE
    assert b"ac_out" in blob and b"ac_inl" in blob


def test_op_table_matches_library(arith_lib):
    lib = ctypes.CDLL(arith_lib)
    assert lib.coa_arith_op_count() == len(ar.OPS)
    d = (ctypes.c_int * 5)()
    for op in ar.OPS.values():
        assert lib.coa_arith_dims(op.id, d) == 0
        assert tuple(d) == (op.na, op.nb, op.nc, op.nout, op.rows), op.name
    assert lib.coa_arith_dims(len(ar.OPS), d) != 0
    # n == 0 returns success without touching the device (no GPU here)
    lib.coa_arith_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32] + \
        [ctypes.c_void_p] * 2
    assert lib.coa_arith_run(0, 0, None, None, None, None, 0, None, None) == 0
    assert lib.coa_arith_run(0, 1, None, None, None, None, 0, None, None) == 0
    assert lib.coa_arith_run(len(ar.OPS), 0, None, None, None, None, 0, None, None) != 0


def test_references_agree_with_oracle():
    """check() accepts what the oracle computes and rejects a neighbour."""
    W = ar.words
    It = lambda a, b=None, c=None: ar.Item(a, b, c, 0, False, False)  # noqa: E731
    assert ar.MU == ar.from_words([0x0a2c131b, 0xed9ce5a3, 0x086329a7, 0x2106215d, 0xffffffeb, 0xffffffff,
                                   0xffffffff, 0xffffffff, 0x0000000f])  # HAC 14.42's mu for l
    a, b = 3 ** 150 % P, 5 ** 100 % P
    assert ar.check("fe_mul", It(a + P, b), W(a * b % P + P)) is None
    assert ar.check("fe_mul", It(a, b), W(a * b % P + 1)) is not None
    assert ar.check("fe_canon", It(a + P), W(a)) is None
    assert ar.check("fe_canon", It(a + P), W(a + P)) is not None  # congruent but not canonical
    assert ar.check("fe_invert", It(a), W(pow(a, P - 2, P))) is None
    ok, r = o.sqrt_ratio_i(a, b)
    assert ar.check("fe_sqrt_ratio", It(a, b), [int(ok)] + W(r)) is None
    assert ar.check("fe_sqrt_ratio", It(a, b), [1 - int(ok)] + W(r)) is not None
    assert ar.check("sc_muladd", It(L - 1, L - 1, 5), W(6)) is None
    assert ar.check("sc_reduce512", It((1 << 512) - 1), W(((1 << 512) - 1) % L)) is None
    # points: 2B and B + 2B from the oracle, in another representation
    rng = ar._rng("spot")
    B2 = o.pdbl(o.B)
    B3 = o.pmul(3, o.B)
    pk = lambda p: W(ar.pack_p3(ar.scale(p, rng)), 32)  # noqa: E731
    assert ar.check("ge_p2_dbl", It(ar.pack_p3(ar.scale(o.B, rng))), pk(B2)) is None
    assert ar.check("ge_add", It(ar.pack_p3(ar.scale(o.B, rng)), ar.pack_p3(ar.scale(B2, rng))), pk(B3)) is None
    assert ar.check("ge_add", It(ar.pack_p3(o.B), ar.pack_p3(B2)), pk(B2)) is not None
    assert ar.check("ge_sub", It(ar.pack_p3(B3), ar.pack_p3(ar.scale(o.B, rng))), pk(B2)) is None
    assert ar.check("ge_madd", It(ar.pack_p3(B2), ar.pack_niels(o.B, rng)), pk(B3)) is None
    bad = list(pk(B3))
    bad[24] ^= 1  # T no longer X*Y/Z
    assert ar.check("ge_add", It(ar.pack_p3(o.B), ar.pack_p3(B2)), bad) is not None
    enc = int.from_bytes(o.compress(B3), "little")
    X, Y, _, T = o.decompress(o.compress(B3))
    assert ar.check("ge_decompress", It(enc), [1] + W(X) + W(Y + P) + W(T)) is None
    assert ar.check("ge_p2_compress", It(ar.pack_p3(ar.scale(B3, rng))), W(enc)) is None
    for t in o.torsion_points():
        assert ar.check("ge_is_small_order", It(ar.pack_p3(ar.scale(t, rng))), [1]) is None
    assert ar.check("ge_is_small_order", It(ar.pack_p3(B3)), [0]) is None
    # halve: (k, 1) is a valid vector; an even d, a wrong sign or a wrong cost are not
    k = 0x123456789abcdef % L
    assert ar.check_halve(k, W(k) + W(1) + [0, k.bit_length()]) is None
    assert ar.check_halve(k, W(k) + W(1) + [1, k.bit_length()]) is not None
    assert ar.check_halve(k, W(k) + W(1) + [0, k.bit_length() + 1]) is not None
    assert ar.check_halve(k, W(2 * k) + W(2) + [0, (2 * k).bit_length()]) is not None
    assert ar.check_halve(8 * L - 0x1234567, W(0x1234567) + W(1) + [1, 25]) is None  # c = -d k (mod 8l)
    assert ar.check_halve(8 * L - 0x1234567, W(0x1234567) + W(1) + [0, 25]) is not None


def test_path_predicates_on_known_operands():
    """The constructions quoted in the issue, counted by the predicates."""
    B = ar.B256
    assert sum(ar.fe_add_path(B - 1 - i, B - 1 - j) == 2 for i in range(40) for j in range(40)) == 703
    assert sum(ar.fe_sub_path(i, B - 1 - j) == 2 for i in range(40) for j in range(40)) == 703
    assert sum(ar.fe_reduce512_path((B - 1 - i) * (B - 1 - j)) == 2 for j in range(64) for i in range(j + 1)) == 917
    assert ar.fe_reduce512_path((1 << 512) - 1) == 2
    assert ar.fe_add_path(1, 2) == 0 and ar.fe_sub_path(2, 1) == 0 and ar.fe_reduce512_path(6) == 0
    assert ar.fe_add_path(B - 1, (1 << 32) - 38) == 0
    assert ar.fe_add_path(B - 1, (1 << 32) - 37) == 1  # carry, then word 0 + 38 carries on into a zero word
    assert ar.fe_sub_path(0, B - (1 << 64) - 1) == 1
    assert ar.fw_add_passes(B - 1, 1) >= 1 and ar.fw_add_passes(1, 2) == 0
    assert ar.fw_sub_passes(1 << 32, 0) >= 1 and ar.fw_sub_passes(5, 3) == 0
    assert ar.sc_reduce512_subs(5) == 0 and ar.sc_reduce512_subs(L) == 1 and ar.sc_reduce512_subs(L - 1) == 0


@pytest.mark.parametrize("name", sorted(ar.PATH_CLASSES))
def test_coverage_floor(name):
    """At least 64 operands on every path of every op that has paths."""
    its = ar.operands(name)
    counts = collections.Counter(ar.path_class(name, it) for it in its)
    assert all(it.cls == ar.path_class(name, it) for it in its)
    for cls in ar.PATH_CLASSES[name]:
        assert counts[cls] >= ar.FLOOR, (name, cls, dict(counts))
    # and the layouts put them where the issue wants them: a wave whose every
    # position is rare, and waves with exactly one rare position
    lay = ar.lane_mix_layout(name)
    g = ar.group_size(name)
    # (one subtraction of l is sc_reduce512's everyday path: there the structured operands are the rare ones)
    hot = (lambda it: it.rare) if name == "sc_reduce512" else (lambda it: it.cls > 0)
    waves = [[hot(it) for it in lay[k:k + g]] for k in range(0, len(lay) - g + 1, g)]
    assert any(all(w) for w in waves) and any(not any(w) for w in waves)
    singles = {w.index(True) for w in waves if sum(w) == 1}
    assert singles >= ({0, 1, 2, 3} if g == 4 else {0, 63}), singles
    assert len(lay) % g == (37 if g == 64 else 3)


def test_every_op_has_operands():
    for name, op in ar.OPS.items():
        its = ar.operands(name)
        assert len(its) >= 1024, name
        assert sum(it.rand for it in its) >= (1024 if len(its) > 1024 else 512), name
        for it in its[:: max(1, len(its) // 64)]:
            for v, n in ((it.a, op.na), (it.b, op.nb), (it.c, op.nc)):
                assert (v is None) == (n == 0), name
                assert v is None or 0 <= v < 1 << (32 * n), name
        for tag, items, mask in ar.masked_layouts(name):
            assert len(items) == len(mask) and 0 < sum(mask) < len(mask)
            assert any(m and it.rare for it, m in zip(items, mask)), (name, tag)


def test_sc_reduce512_two_subtractions_search():
    """Does any input make sc_reduce512 subtract l twice (Barrett estimate two
    short)?  Outcome of the structured search, j*l + delta with delta in
    {-1, 0, 1} and 1,280 random j of every bit length up to
    floor((2^512-1)/l) -- 998,400 candidates: NONE found.  delta = 0 and +1
    always took exactly one subtraction and delta = -1 none (the estimate was
    one short on every multiple of l tried, never two).  So
    SC_REDUCE_TWO_SUBS is empty and the coverage floor for that path is
    waived, for that path only; paths 0 and 1 keep their floors
    (test_coverage_floor).  This test re-runs a 1/80 sample of the search so
    that a change of mu or of the predicate that opens the path is noticed,
    and checks that anything pinned really is on it."""
    tried, hist, found = ar.sc_two_subs_search(16)
    assert tried > 12000 and hist[0] > 0 and hist[1] > 0
    assert found == [] and hist[2] == 0, [hex(x) for x in found[:4]]
    assert all(ar.sc_reduce512_subs(x) == 2 for x in ar.SC_REDUCE_TWO_SUBS)

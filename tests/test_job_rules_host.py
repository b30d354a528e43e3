"""CPU: the prefix bits, the hand-over word and the two accept rules of a
committee signature job (xrpl-coa-prototype_amd/csrc/coa_job_bits.h), compiled
for the host and checked over every input against a restatement of dalek's
conditions written from oracle/ed25519_ref.py's verify_strict and the file
comment of coa_committee.hip.

`P == R` means decompress(R) == Some(P), so it implies that R decompresses:
the latency rule gets both facts, the throughput rule only their conjunction
(it never decompresses R).  The small-order bit is taken on P and read only
beside P == R, where it is R's."""
import ctypes
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "job_rules", "job_rules_host.cpp")
INC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")

# COA_CST_* (coa_stage.h)
BAD_SIG, BAD_VOTES, INCONCLUSIVE, UNCACHED = 2, 4, 8, 16


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("job_rules") / "libjobrules.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", INC, SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    for f in (lib.rule_latency, lib.rule_throughput, lib.job_word, lib.job_status, lib.job_pre, lib.job_code):
        f.restype = ctypes.c_uint32
    return lib


def _bits(lib):
    out = (ctypes.c_uint32 * 8)()
    lib.job_bits(out)
    return dict(zip(("s", "a", "small_a", "torsion", "strict", "uncached", "none", "small_p"), out))


def _expected(f, r_ok, p_eq_r, latency):
    """f: the facts named as the prefix bits name them (True = the bit is set)."""
    if f["none"] or f["uncached"]:
        return UNCACHED if f["uncached"] else 0
    s_ok, a_ok = not f["s"], not f["a"]
    if f["strict"]:  # verify_strict: every check of ed25519_ref.verify_strict
        ok = s_ok and a_ok and not f["small_a"] and r_ok and not f["small_p"] and p_eq_r
        return 0 if ok else BAD_SIG
    # a vote: malformed inputs are dalek's definitive Err; the latency rule
    # knows whether R decompresses, the throughput rule does not
    if not (s_ok and a_ok and (r_ok or not latency)):
        return BAD_VOTES
    return 0 if (p_eq_r and not f["torsion"]) else INCONCLUSIVE


def test_bits_are_eight_distinct_bits_of_one_byte(lib):
    b = _bits(lib)
    assert sorted(b.values()) == [1 << i for i in range(8)]


def test_hand_over_word_round_trips(lib):
    for status, pre, code in itertools.product((0, 1, 16, 0xFF), (0, 1, 0x80, 0xA5, 0xFF), (0, 1, 6, 0xFF)):
        w = lib.job_word(status, pre, code)
        assert w < 1 << 24
        assert (lib.job_status(w), lib.job_pre(w), lib.job_code(w)) == (status, pre, code)
        assert (w & 0xFF, (w >> 8) & 0xFF, (w >> 16) & 0xFF) == (status, pre, code)


def test_rules_over_every_input(lib):
    b = _bits(lib)
    names = list(b)
    differ = 0
    for flags in itertools.product((False, True), repeat=8):
        f = dict(zip(names, flags))
        pre = sum(b[n] for n in names if f[n])
        for r_ok, eq in itertools.product((False, True), repeat=2):
            p_eq_r = r_ok and eq
            lat = lib.rule_latency(pre, int(r_ok), int(eq))
            thr = lib.rule_throughput(pre, int(p_eq_r))
            assert lat == _expected(f, r_ok, p_eq_r, True), (f, r_ok, eq)
            assert thr == _expected(f, r_ok, p_eq_r, False), (f, r_ok, eq)
            if lat != thr:
                # the documented difference and nothing else: a well-formed
                # vote whose R does not decompress is left to the host
                differ += 1
                assert thr == INCONCLUSIVE and lat == BAD_VOTES, (f, r_ok, eq)
                assert not f["strict"] and not r_ok
    assert differ > 0

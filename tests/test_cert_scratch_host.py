"""CPU: the scratch layout of the throughput kernels (xrpl-coa-prototype_amd/
csrc/coa_cert_scratch.h, CertScratch) compiled for the host: the sections are
in order, aligned and disjoint, the last one ends at `bytes`, `bytes` is the
closed formula callers have always allocated from (restated here), and the
sort sections exist exactly when key order is asked for a call of at least
16,384 jobs.

Alignment: every section starts on 16 bytes except the permutation.  It
follows the jobs' bins (4 bytes per job) without a gap and ends at `bytes`,
whose formula has 8 bytes per job for the two, so with a job count that is no
multiple of 4 it can start on 4 bytes only; it is read and written as dwords."""
import ctypes
import itertools
import os
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "job_rules", "job_rules_host.cpp")
INC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")

JOBS = (1, 63, 64, 65, 16383, 16384, 16385, 680000)
LANES = (256, 512, 131072)
BINS, WGS, MIN_JOBS, ROWS = 4096, 256, 16384, 9


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("cert_scratch") / "libjobrules.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", INC, SRC, "-o", so], check=True)
    lib = ctypes.CDLL(so)
    lib.cert_scratch.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_uint64)]

    def call(jobs, lanes, digests, key_order):
        out = (ctypes.c_uint64 * 10)()
        lib.cert_scratch(jobs, lanes, int(digests), int(key_order), out)
        return dict(zip(("ctr", "slab", "cdig", "total", "counts", "bin", "perm", "bytes", "jcap", "sorts"), out))

    return call


def _jcap(jobs, lanes):
    waves, chunks = lanes // 64, (jobs + 63) // 64
    return (chunks + waves - 1) // waves + 2


def _slab_bytes(jobs, lanes):
    return lanes * _jcap(jobs, lanes) * ROWS * 16


def _cert_bytes(jobs, lanes, key_order):
    base = 256 + _slab_bytes(jobs, lanes) + max(jobs, 1) * 32
    if not key_order or jobs < MIN_JOBS:
        return base
    return base + 256 + BINS * (WGS + 1) * 4 + jobs * 8


def _sections(s, jobs, lanes, digests):
    """(name, first byte, byte length, alignment) of the sections that are there, in layout order."""
    secs = [("ctr", s["ctr"] * 4, 4, 16), ("slab", s["slab"] * 4, _slab_bytes(jobs, lanes), 16)]
    if digests:
        secs.append(("cdig", s["cdig"] * 4, max(jobs, 1) * 32, 16))
    if s["sorts"]:
        secs += [("total", s["total"] * 4, BINS * 4, 16), ("counts", s["counts"] * 4, BINS * WGS * 4, 16),
                 ("bin", s["bin"] * 4, jobs * 4, 16), ("perm", s["perm"] * 4, jobs * 4, 4)]
    return secs


@pytest.mark.parametrize("key_order", (False, True))
def test_certificate_layout(scratch, key_order):
    for jobs, lanes in itertools.product(JOBS, LANES):
        s = scratch(jobs, lanes, True, key_order)
        assert s["jcap"] == _jcap(jobs, lanes)
        assert bool(s["sorts"]) == (key_order and jobs >= MIN_JOBS), (jobs, lanes)
        secs = _sections(s, jobs, lanes, True)
        end = 0
        for name, at, size, align in secs:
            assert at % align == 0, (name, jobs, lanes)
            assert at >= end, (name, jobs, lanes)  # in order and disjoint
            end = at + size
        assert end == s["bytes"], (jobs, lanes)
        assert s["bytes"] == _cert_bytes(jobs, lanes, key_order), (jobs, lanes)
        if not s["sorts"]:
            assert (s["total"], s["counts"], s["bin"], s["perm"]) == (0, 0, 0, 0)


def test_message_layout(scratch):
    for jobs, lanes in itertools.product(JOBS, LANES):
        s = scratch(jobs, lanes, False, True)  # key order is not for messages: no sort sections either way
        assert not s["sorts"] and s["cdig"] == 0
        secs = _sections(s, jobs, lanes, False)
        assert secs[-1][1] + secs[-1][2] == s["bytes"] == 256 + _slab_bytes(jobs, lanes), (jobs, lanes)


def test_empty_call_sizes_as_before(scratch):
    # coa_cert_scratch_bytes(0, .): the slab of zero chunks on 256 lanes, one digest
    assert scratch(0, 256, True, True)["bytes"] == 256 + 256 * 2 * ROWS * 16 + 32

"""CPU: coa_certificate_votes_resolve_device's host side -- its return codes
before any device work (n = 0, null arrays, no GPU), the workspace size
(monotone in n, n_votes and the cap; cap 0 is cap n_votes) -- and the workspace
layout of xrpl-coa-prototype_amd/csrc/coa_resolve_ws.h, checked by a
stand-alone program (tests/sanitize/resolve_ws_driver.cpp) built with
-fsanitize=address,undefined and run as a child process."""
import ctypes
import os
import subprocess

import pytest

from conftest import ROOT

COA_OK, COA_EINVAL, COA_ENODEVICE = 0, -1, -2
SRC = os.path.join(ROOT, "tests", "sanitize", "resolve_ws_driver.cpp")
INC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")


@pytest.fixture(scope="module")
def L():
    import build

    build.build()
    import coa_crypto

    return coa_crypto.lib()


def _call(L, n, n_votes, null=None, cap=0):
    """The entry with distinct host addresses for its arrays (never
    dereferenced: every path taken here returns before device work);
    `null`: the index of the array passed as NULL."""
    buf = (ctypes.c_uint8 * 64)()
    base = ctypes.addressof(buf)
    # ids, origins, rounds, vote_pks, vote_sigs, vote_offsets | zs | verdicts, counts, workspace, stream
    arrays = [base + 8 * i for i in range(6)]
    verdicts = base + 56
    if null is not None and null < 6:
        arrays[null] = None
    if null == 6:
        verdicts = None
    return L.coa_certificate_votes_resolve_device(0, *arrays, n, n_votes, cap, None, 1, verdicts, None, None, None)


def test_empty_call_is_ok(L):
    assert _call(L, 0, 0) == COA_OK
    assert _call(L, 0, 5, null=0) == COA_OK  # n = 0 is decided first, as in the other device forms


@pytest.mark.parametrize("null", range(7), ids=["ids", "origins", "rounds", "vote_pks", "vote_sigs", "vote_offsets",
                                                "verdicts"])
def test_null_arrays_are_refused(L, null):
    assert _call(L, 3, 9, null=null) == COA_EINVAL
    assert b"null" in L.coa_last_error()


def test_vote_arrays_may_be_null_without_votes(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the call would run; covered by tests/test_gpu_votes_resolve.py")
    assert _call(L, 3, 0, null=3) == COA_ENODEVICE


def test_no_gpu_no_answer(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_votes_resolve.py")
    assert _call(L, 3, 9) == COA_ENODEVICE


def test_workspace_size_is_monotone(L):
    f = L.coa_certificate_votes_resolve_workspace_bytes
    ns = (1, 2, 255, 256, 257, 10_000, 100_000)
    for votes in (0, 1, 300, 670_000):
        sizes = [f(n, votes, 0) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0, (votes, sizes)
    vs = (0, 1, 255, 256, 257, 20_100, 670_000, 6_700_000)
    for n in (1, 300, 10_000):
        sizes = [f(n, v, 0) for v in vs]
        assert sizes == sorted(sizes), (n, sizes)
        assert sizes[-1] > sizes[0]
    caps = (1, 2, 255, 256, 257, 6_700, 67_000, 131_072, 131_073, 669_999, 670_000)
    sizes = [f(10_000, 670_000, c) for c in caps]
    assert sizes == sorted(sizes) and sizes[0] < sizes[-1], sizes
    # a 1 % budget does not pay for the worst case: the per-vote sections and the 2 KiB of term scratch per lane
    assert f(10_000, 670_000, 6_700) * 20 < f(10_000, 670_000, 0)


@pytest.mark.parametrize("n,votes", [(1, 0), (1, 1), (256, 17_152), (10_000, 670_000)])
def test_cap_zero_is_every_vote(L, n, votes):
    f = L.coa_certificate_votes_resolve_workspace_bytes
    assert f(n, votes, 0) == f(n, votes, votes)
    assert f(n, votes, votes + 1) == f(n, votes, votes)  # a cap above the call's votes is the call's votes


def test_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "resolve_ws_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok 54 cases")

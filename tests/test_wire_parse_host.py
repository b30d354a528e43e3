"""CPU: the device wire decoder's host side.

The library's one frame grammar (xrpl-coa-prototype_amd/csrc/coa_wire_parse.h)
against the independent container-based model tests/sanitize/wire_model.h, by a
stand-alone program (tests/sanitize/wire_parse_driver.cpp) built with
-fsanitize=address,undefined and run as a child process.  Compared with the
model, each way: the header's functions taken the way the kernels' lanes take
them, and the host entries of coa_wire.cpp, the sequential driver of the same
header.  Over the committed fuzz corpus, every strict prefix of its frames
under 1 KiB, 20,000 seeded mutations, the constructed cases of
tests/wire_dev_cases.py and one oversized header frame the program makes
itself (300,000 payload entries: the host's set order is not quadratic) --
kind, lengths and every output byte equal, each frame in an exactly sized heap
block.

And the new entries' return codes before any device work (n = 0, null arrays,
no GPU) and the workspace size."""
import ctypes
import os
import struct
import subprocess

import pytest

from conftest import ROOT

import wire_dev_cases as cases

COA_OK, COA_EINVAL, COA_ENODEVICE = 0, -1, -2
SRC = os.path.join(ROOT, "tests", "sanitize", "wire_parse_driver.cpp")
CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")
CORPUS = os.path.join(ROOT, "tests", "fuzz", "wire_corpus")
MUTATIONS = 20_000


def test_grammar_header_matches_host_decoder_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wire_parse_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"), SRC, os.path.join(CSRC, "coa_wire.cpp"), "-o", exe],
                   check=True)
    constructed = cases.all_constructed()
    case_file = tmp_path / "cases.bin"
    with open(case_file, "wb") as f:
        for c in constructed:
            f.write(struct.pack("<Q", len(c["frame"])) + c["frame"])
    r = subprocess.run([exe, CORPUS, str(case_file), str(MUTATIONS)], capture_output=True, text=True, timeout=600)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    corpus = [open(os.path.join(CORPUS, n), "rb").read() for n in sorted(os.listdir(CORPUS)) if n.endswith(".bin")]
    frames = len(corpus) + sum(len(f) for f in corpus if len(f) < 1024) + MUTATIONS + len(constructed) + 1  # + the oversized frame
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"ok {frames} frames"
    counts = dict(zip(lines[-2].split()[0::2], map(int, lines[-2].split()[1::2])))
    # the inputs reach every branch: each kind decodes, errors are met, the cap and the walk are taken
    assert min(counts[k] for k in ("headers", "votes", "certificates", "requests", "errors", "walked")) > 0, counts
    assert counts["capacity"] >= 2, counts


@pytest.fixture(scope="module")
def L():
    import build

    build.build()
    import coa_crypto

    return coa_crypto.lib()


def _device_calls(L, n, null=None):
    """Every device entry with distinct host addresses for its arrays (never
    dereferenced: every path taken here returns before device work); `null`:
    the index of the array passed as NULL."""
    buf = (ctypes.c_uint8 * 256)()
    base = ctypes.addressof(buf)

    def arrays(k):
        a = [base + 8 * i for i in range(k)]
        if null is not None and null < k:
            a[null] = None
        return a

    fb = 4096
    out = []
    # frames, offsets | kinds (header bytes and votes are optional)
    a = arrays(3)
    out.append(L.coa_wire_scan_device(0, a[0], a[1], n, fb, a[2], None, None, None, None))
    a = arrays(14)
    out.append(L.coa_wire_decode_certificates_device(0, a[0], a[1], n, fb, *a[2:], None, None))
    a = arrays(11)
    out.append(L.coa_wire_decode_headers_device(0, a[0], a[1], n, fb, *a[2:], None, None))
    a = arrays(9)
    out.append(L.coa_wire_decode_votes_device(0, a[0], a[1], n, fb, *a[2:], None, None))
    return out


def _fused_calls(L, frames, offs, n, kinds=True, words=True):
    k = (ctypes.c_int32 * max(n, 1))()
    w = (ctypes.c_uint32 * max(n, 1))()
    kp, wp = (ctypes.addressof(k) if kinds else None), (ctypes.addressof(w) if words else None)
    fp = ctypes.addressof(frames) if frames is not None else None
    op = ctypes.addressof(offs) if offs is not None else None
    return [L.coa_wire_certificate_verdict_many(fp, op, n, 1, kp, wp), L.coa_wire_header_verdict_many(fp, op, n, kp, wp),
            L.coa_wire_vote_verdict_many(fp, op, n, kp, wp)]


def test_empty_calls_are_ok(L):
    assert _device_calls(L, 0) == [COA_OK] * 4
    assert _device_calls(L, 0, null=0) == [COA_OK] * 4  # n = 0 is decided first, as in the other device forms
    assert _fused_calls(L, None, None, 0) == [COA_OK] * 3


def test_null_arrays_are_refused(L):
    takes = [3, 14, 11, 9]  # arrays of each call, in the order of _device_calls
    for null in range(14):
        got = _device_calls(L, 3, null=null)
        for rc, k in zip(got, takes):
            if null < k:
                assert rc == COA_EINVAL, (null, got)
    assert _device_calls(L, 3, null=2)[0] == COA_EINVAL  # ends with the votes call, which has array 2
    assert b"null" in L.coa_last_error()
    frames = (ctypes.c_uint8 * 16)()
    offs = (ctypes.c_uint64 * 3)(0, 8, 16)
    assert _fused_calls(L, frames, None, 2) == [COA_EINVAL] * 3
    assert _fused_calls(L, frames, offs, 2, kinds=False) == [COA_EINVAL] * 3
    assert _fused_calls(L, frames, offs, 2, words=False) == [COA_EINVAL] * 3
    assert _fused_calls(L, None, offs, 2) == [COA_EINVAL] * 3
    bad = (ctypes.c_uint64 * 3)(0, 9, 8)
    assert _fused_calls(L, frames, bad, 2) == [COA_EINVAL] * 3  # host offsets must not decrease


def test_sizes_beyond_one_call_are_refused(L):
    buf = (ctypes.c_uint8 * 64)()
    a = [ctypes.addressof(buf) + 8 * i for i in range(3)]
    assert L.coa_wire_scan_device(0, a[0], a[1], 3, 1 << 32, a[2], None, None, None, None) == COA_EINVAL
    assert L.coa_wire_scan_device(0, a[0], a[1], 1 << 32, 64, a[2], None, None, None, None) == COA_EINVAL


def test_no_gpu_no_answer(L):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_wire_device.py")
    assert _device_calls(L, 3) == [COA_ENODEVICE] * 4
    frames = (ctypes.c_uint8 * 16)()
    offs = (ctypes.c_uint64 * 3)(0, 8, 16)
    assert _fused_calls(L, frames, offs, 2) == [COA_ENODEVICE] * 3


def test_workspace_size_is_monotone(L):
    f = L.coa_wire_workspace_bytes
    ns = (1, 2, 255, 256, 257, 10_000, 65_536, 1_000_000)
    for fb in (0, 1, 10_388, 103_880_000):
        sizes = [f(n, fb) for n in ns]
        assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0], (fb, sizes)
    for n in (1, 300, 10_000):
        sizes = [f(n, fb) for fb in (0, 1, 4096, 10_388 * n, 1 << 30)]
        assert sizes == sorted(sizes), (n, sizes)


def test_constants_match_the_header():
    import coa_crypto

    text = open(os.path.join(ROOT, "include", "coa_verify.h")).read()
    assert f"#define COA_WIRE_DEV_MAX_ENTRIES {coa_crypto.WIRE_DEV_MAX_ENTRIES}" in text
    assert coa_crypto.WIRE_DEV_MAX_ENTRIES >= 1024 and cases.MAX_ENTRIES == coa_crypto.WIRE_DEV_MAX_ENTRIES
    assert coa_crypto.WIRE_ECAPACITY == -13 and coa_crypto.DAG_NO_MESSAGE == 255
    assert coa_crypto.wire_votes_bound(115 * 7 + 114) == 7

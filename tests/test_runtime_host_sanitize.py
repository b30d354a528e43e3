"""CPU: the runtime's host-only headers -- csrc/coa_env.h (the COA_* switch
readers), csrc/coa_offsets.h (monotone check, rebased offsets, digest input)
and csrc/coa_hostpool.h (Worker) -- built into a stand-alone program
(tests/sanitize/runtime_host_driver.cpp) with ASan + UBSan, and with
ThreadSanitizer where ROCm's clang is present, and run directly.  Nothing is
preloaded; no device code."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


def _build_and_run(name, cxx, san):
    d = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-I", CSRC,
           "-fsanitize=" + san, "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sanitize", "runtime_host_driver.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("COA_")}  # the driver sets its own
    env.update(ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               TSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    assert "runtime host ok: 0 bad" in r.stdout


def test_runtime_host_pieces_asan_ubsan():
    _build_and_run("runtime_host_asan", "g++", "address,undefined")


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang (TSan runtime) not present")
def test_runtime_host_pieces_tsan():
    _build_and_run("runtime_host_tsan", CLANG, "thread")

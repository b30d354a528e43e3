"""CPU: csrc/coa_qstage.h -- the staging of an aggregation-queue window: the
layout of its input and output blocks, the packer of a launch's parts, the
scatter of the outputs back to the parts and the resolver's gather and
write-back -- built with ASan + UBSan into a stand-alone program
(tests/sanitize/qstage_driver.cpp) and run directly.  Nothing is preloaded; no
device code: a fake device in the driver fills the output block from the
packed input block."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")


def test_queue_window_staging_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, "qstage_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sanitize", "qstage_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "qstage ok: 0 bad" in r.stdout

"""CPU: csrc/coa_main_pick.h -- which phase-2 kernel a split verification call
launches for a size and the COA_MAIN_* switches, and k_pre_halve's priority
bits -- built with ASan + UBSan into a stand-alone program
(tests/sanitize/main_pick_driver.cpp) and run directly.  Nothing is preloaded;
no device code."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")


def test_main_kernel_choice_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, "main_pick_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sanitize", "main_pick_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "main pick ok: 0 bad" in r.stdout

"""CPU: the verdict calls of the engine's CPU path (coa_cpu.cpp with
coa_protocol.h, which coa_committee_register_authorities shares for the
validation of the committee arrays) built with ASan + UBSan into a
stand-alone program (tests/sanitize/verdict_driver.cpp) and run over every
case of tests/verdict_cases.py.  Nothing is preloaded; no device code."""
import os
import subprocess

from conftest import ROOT

import verdict_cases as vc

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")


def test_cpu_verdict_path_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, "verdict_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", os.path.join(CSRC, "coa_cpu.cpp"),
           os.path.join(ROOT, "tests", "sanitize", "verdict_driver.cpp"), "-o", exe, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    path = os.path.join(d, "verdict_cases.bin")
    nc, nh, nv = vc.write_case_file(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert f"verdict path ok: {nc} certificates, {nh} headers, {nv} votes, 0 bad" in r.stdout

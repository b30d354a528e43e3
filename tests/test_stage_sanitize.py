"""CPU: csrc/coa_stage.h -- the staging layouts, the packers and the chunk
cuts of the host-pointer certificate, header and vote shards -- built with
ASan + UBSan into a stand-alone program (tests/sanitize/stage_driver.cpp) and
run directly.  Nothing is preloaded; no device code.  The chunk cuts are
checked over six tiles of the certificate cases of tests/verdict_cases.py,
the set test_gpu_verdicts.py sends through the pipelined path."""
import os
import subprocess

from conftest import ROOT

import verdict_cases as vc

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")


def test_stage_layouts_and_packers_asan_ubsan():
    d = os.path.join(ROOT, "tests", "sanitize", "_build")
    os.makedirs(d, exist_ok=True)
    exe = os.path.join(d, "stage_asan")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fno-omit-frame-pointer", "-I", CSRC,
           "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           os.path.join(ROOT, "tests", "sanitize", "stage_driver.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    votes = [len(c["votes"]) for c in vc.certificate_cases()]
    assert (len(votes), sum(votes)) == (72, 1985)  # 2,057 jobs a tile
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe] + [str(v) for v in votes], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "stage ok: 0 bad" in r.stdout

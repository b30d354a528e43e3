"""CPU: the aggregation queue's verdict requests
(coa_queue_submit_certificate_verdict[_borrowed] / coa_queue_submit_header_verdict
/ coa_queue_submit_vote_verdict / coa_queue_verdict_stats).

* tests/sanitize/queue_verdicts_tsan.cpp -- a stand-alone program with its own
  stub backend -- built with coa_queue.cpp under ThreadSanitizer (ROCm clang)
  and under ASan + UBSan: 16 producers submit all ten request kinds; the stub
  derives each verdict word from the request's bytes, leaves some verdict
  certificates open as COA_DAG_VOTES_OPEN for the resolver and gives every
  fifth verdict window a generation without protocol table.  Every callback is
  checked (the exact word and n = 4; the crypto requests of shared windows as
  without verdict requests), with injected launch failures, failing retries
  and failing resolver passes (each the failed word), and the COA_EINVAL
  windows must leave failed_windows and retried_windows alone.  Nothing is
  loaded into Python and nothing is preloaded.
* tests/sanitize/qstage_verdict_driver.cpp -- the payload-count and
  verdict-word sections of coa_qstage.h (layout, pack, scatter of mixed
  windows over several parts) under ASan + UBSan.
* With no GPU the new Python futures raise EngineError and verdict_stats()
  counts the requests.
* tests/c_abi/queue_verdict_harness.c -- a C caller of the new prototypes
  (-std=c11 -Wall -Wextra -Werror) over verdict_cases.write_case_file's case
  file: compiled here and run in its cpu mode (every request answered
  COA_ENODEVICE with the failed word); tests/test_gpu_queue_verdicts.py runs
  its gpu mode."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")
INC = os.path.join(ROOT, "include")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SAN = os.path.join(ROOT, "tests", "sanitize")
QUEUE_SRCS = [os.path.join(CSRC, "coa_queue.cpp"), os.path.join(SAN, "queue_verdicts_tsan.cpp")]
TIMEOUT = 60  # seconds a future may take: a lost callback fails instead of hanging


def _build(name, flags, cxx, srcs):
    out = os.path.join(SAN, "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I", INC, "-I", CSRC] + flags + srcs + \
          ["-o", out, "-pthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(cmd, env_extra):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env_extra))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "WARNING: ThreadSanitizer" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def _check_runs(exe, env):
    # no injected failure: the COA_EINVAL windows alone -- nothing retried, nothing failed
    out = _run([exe, "16", "400"], env)
    assert "6400/6400 answered, 0 wrong" in out and "einval 0 " not in out and "refused 0," not in out, out
    assert "injected 0, retried 0, recovered 0, failed 0, engine errors 0," in out and "deferred 0 " not in out, out
    # every 7th launch fails: each is re-run, every answer exact, no engine error
    out = _run([exe, "16", "400", "7"], env)
    assert "6400/6400 answered, 0 wrong" in out and "injected 0," not in out and "engine errors 0," in out, out
    # ... and with every retry failing too, those callbacks get the engine error and the failed word
    out = _run([exe, "8", "300", "7", "1"], env)
    assert "2400/2400 answered, 0 wrong" in out and "recovered 0," in out and "engine errors 0," not in out, out
    # every resolver pass fails: each request left to it gets the engine error
    # with its kind's "failed" value (an open verdict certificate: the failed word)
    out = _run([exe, "16", "300", "7", "0", "1"], env)
    assert "4800/4800 answered, 0 wrong" in out and "resolver errors 0\n" not in out, out
    assert "engine errors 0," in out and "deferred 0 " not in out, out
    # idle launch: windows also launched by the submitting threads
    out = _run([exe, "16", "300", "7"], dict(env, COA_QUEUE_IDLE_LAUNCH="1"))
    assert "4800/4800 answered, 0 wrong" in out and "injected 0," not in out, out


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang (TSan runtime) not present")
def test_ten_kinds_many_producers_tsan():
    exe = _build("queue_verdicts_tsan", ["-fsanitize=thread"], CLANG, QUEUE_SRCS)
    _check_runs(exe, {"TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"})


def test_ten_kinds_many_producers_asan_ubsan():
    exe = _build("queue_verdicts_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "g++", QUEUE_SRCS)
    _check_runs(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"})


def test_staging_sections_asan_ubsan():
    exe = _build("qstage_verdict_driver", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "g++",
                 [os.path.join(SAN, "qstage_verdict_driver.cpp")])
    out = _run([exe], {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"})
    assert "qstage verdict sections: 0 failed checks" in out, out


HARNESS_SRC = os.path.join(ROOT, "tests", "c_abi", "queue_verdict_harness.c")
HARNESS = os.path.join(ROOT, "tests", "c_abi", "queue_verdict_harness")


def run_queue_verdict_harness(mode, tmp_path):
    """Builds tests/c_abi/queue_verdict_harness.c against the header and the
    library and runs it over the case file."""
    import build
    import verdict_cases as vc

    libdir = os.path.dirname(build.build())
    tmp = f"{HARNESS}.{os.getpid()}"
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", "-pthread", "-I", INC, HARNESS_SRC, "-o", tmp,
           "-L", libdir, "-lcoa_verify", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    os.replace(tmp, HARNESS)
    path = str(tmp_path / "verdict_cases.bin")
    nc, nh, nv = vc.write_case_file(path)
    r = subprocess.run([HARNESS, path, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"queue verdict harness ({mode}): {nc} certificates, {nh} headers, {nv} votes, " in r.stdout
    assert ", 0 bad" in r.stdout and " 0 verdict windows" not in r.stdout, r.stdout


def test_c_harness_compiles_and_refuses_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_queue_verdicts.py runs the harness in its gpu mode")
    run_queue_verdict_harness("cpu", tmp_path)


def test_futures_raise_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    import build

    build.build()
    import coa_crypto

    with coa_crypto.AggregationQueue(max_batch=8, max_delay_us=100) as q:
        futs = [q.submit_header_verdict(b"h" * (76 + i), bytes(32), bytes([i]) * 32, bytes(64), 1) for i in range(5)]
        futs += [q.submit_vote_verdict(bytes(32), 7 + i, bytes([1]) * 32, bytes([i]) * 32, bytes(64)) for i in range(3)]
        votes = [(coa_crypto.PublicKey(bytes([9]) * 32), coa_crypto.Signature.from_bytes(bytes(64)))] * 2
        for borrow in (False, True):
            futs.append(q.submit_certificate_verdict(b"c" * 112, bytes(32), bytes([2]) * 32, bytes(64), 3, votes, 2,
                                                     borrow=borrow))
        futs.append(q.submit_header_verdict(b"", bytes(32), bytes(32), bytes(64), 0))  # count 0 fits an empty header
        # a count that overruns its header is refused at submission
        with pytest.raises(coa_crypto.EngineError):
            q.submit_header_verdict(b"h" * 75, bytes(32), bytes(32), bytes(64), 1)
        with pytest.raises(coa_crypto.EngineError):
            q.submit_certificate_verdict(b"c" * 111, bytes(32), bytes(32), bytes(64), 3, votes, 2)
        for f in futs:
            with pytest.raises(coa_crypto.EngineError):
                f.result(timeout=TIMEOUT)
        q.flush()
        vs = q.verdict_stats()
        assert (vs["certificates"], vs["headers"], vs["votes"]) == (2, 6, 3) and vs["verdict_windows"] >= 1
        ms = q.message_stats()
        assert (ms["headers"], ms["votes"]) == (6, 3)
        m = q.metrics()
        assert m["requests"] == 11 and m["signatures"] == 9 and m["certificates"] == 2 and m["failed_windows"] >= 1

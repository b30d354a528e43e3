"""CPU: header and vote requests of the aggregation queue
(coa_queue_submit_header / coa_queue_submit_vote / coa_queue_message_stats).

* tests/sanitize/queue_messages_tsan.cpp -- a stand-alone program with its own
  stub backend -- built with coa_queue.cpp under ThreadSanitizer (ROCm clang)
  and under ASan + UBSan: 16 producers submit all six request kinds, the stub
  defers messages by a byte of the author so the resolver answers them, and
  launch failures are injected (every 7th launch re-run and exact; every retry
  failing too: the engine error reaches those callbacks; every resolver pass
  failing: its requests get the error with their kinds' "failed" values).
  Nothing is loaded
  into Python and nothing is preloaded.
* With no GPU the futures of submit_header / submit_vote raise EngineError and
  the queue's counters count the requests."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")
INC = os.path.join(ROOT, "include")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SRCS = [os.path.join(CSRC, "coa_queue.cpp"), os.path.join(ROOT, "tests", "sanitize", "queue_messages_tsan.cpp")]
TIMEOUT = 60  # seconds a future may take: a lost callback fails instead of hanging


def _build(name, flags, cxx):
    out = os.path.join(ROOT, "tests", "sanitize", "_build", name)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-I", INC, "-I", CSRC] + flags + SRCS + \
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
    out = _run([exe, "16", "400"], env)
    assert "6400/6400 answered, 0 wrong" in out and " 0 headers" not in out and " 0 votes" not in out, out
    assert "deferred 0 " not in out, out
    # every 7th launch fails: each is re-run, every answer exact, no engine error
    out = _run([exe, "16", "400", "7"], env)
    assert "6400/6400 answered, 0 wrong" in out and "injected 0," not in out and "engine errors 0," in out, out
    # ... and with every retry failing too, those callbacks get the engine error
    out = _run([exe, "8", "300", "7", "1"], env)
    assert "2400/2400 answered, 0 wrong" in out and "recovered 0," in out and "engine errors 0," not in out, out
    # every resolver pass fails: each request left to it gets the engine error
    # with its kind's "failed" value (7 certificate, 3 header, 1 vote or bare
    # batch; the binary checks each callback), every other request is exact
    out = _run([exe, "16", "300", "7", "0", "1"], env)
    assert "4800/4800 answered, 0 wrong" in out and "resolver errors 0\n" not in out, out
    assert "engine errors 0," in out and "deferred 0 " not in out, out
    # idle launch: windows also launched by the submitting threads
    out = _run([exe, "16", "300", "7"], dict(env, COA_QUEUE_IDLE_LAUNCH="1"))
    assert "4800/4800 answered, 0 wrong" in out and "injected 0," not in out, out


@pytest.mark.skipif(not os.path.exists(CLANG), reason="ROCm clang (TSan runtime) not present")
def test_six_kinds_many_producers_tsan():
    exe = _build("queue_messages_tsan", ["-fsanitize=thread"], CLANG)
    _check_runs(exe, {"TSAN_OPTIONS": "halt_on_error=1:second_deadlock_stack=1"})


def test_six_kinds_many_producers_asan_ubsan():
    exe = _build("queue_messages_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "g++")
    _check_runs(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1"})


def test_futures_raise_without_gpu():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by the gpu tests")
    import build

    build.build()
    import coa_crypto

    with coa_crypto.AggregationQueue(max_batch=8, max_delay_us=100) as q:
        futs = [q.submit_header(b"h" * (40 + i), bytes(32), bytes([i]) * 32, bytes(64)) for i in range(5)]
        futs += [q.submit_vote(bytes(32), 7 + i, bytes([1]) * 32, bytes([i]) * 32, bytes(64)) for i in range(3)]
        futs.append(q.submit_header(b"", bytes(32), bytes(32), bytes(64)))  # an empty header input is a request too
        for f in futs:
            with pytest.raises(coa_crypto.EngineError):
                f.result(timeout=TIMEOUT)
        q.flush()
        ms = q.message_stats()
        assert (ms["headers"], ms["votes"]) == (6, 3)
        assert ms["latency_windows"] == 0 and ms["throughput_windows"] == 0  # nothing ran
        m = q.metrics()
        assert m["requests"] == 9 and m["signatures"] == 9 and m["failed_windows"] >= 1
        assert q.stats()["signatures"] == 9

"""GPU: verdict requests through engine-failure recovery.  With
COA_QUEUE_FAULT=3 (the queue's fault injection: every third window's launch
fails and is re-run on the recovery context) every verdict word is still
exact.

The windows of twelve mix message and certificate verdicts (k_window_verdict
behind the crypto kernels); the windows of messages alone are
k_msg_verdict_lat's, publishing.

A file of its own that sorts after tests/test_gpu_recovery.py, as that file
keeps its own fault-injection tests behind
test_registration_never_holds_a_window_back (launch failures
injected into message windows earlier in the same process, "the cause is
open")."""
import pytest

import verdict_cases as vc  # noqa: F401
from test_gpu_queue_verdicts import _cert_reqs, _msg_reqs, _queue_env, _window, registered  # noqa: F401

pytestmark = pytest.mark.gpu


def test_words_exact_through_recovery(registered, monkeypatch):
    """COA_QUEUE_FAULT=3: every third window's launch fails and is re-run on
    the recovery context; every word is still exact."""
    monkeypatch.setenv("COA_QUEUE_FAULT", "3")
    e = registered
    reqs = _msg_reqs()[::4] + _cert_reqs("c")[::5]
    with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
        for lo in range(0, len(reqs), 12):
            _window(e, q, reqs[lo:lo + 12])
        m = q.metrics()
    windows = (len(reqs) + 11) // 12
    assert m["windows"] == windows and m["retried_windows"] == windows // 3
    assert m["recovered_windows"] == m["retried_windows"] and m["failed_windows"] == 0


def test_message_words_exact_through_recovery(registered, monkeypatch):
    """The same for windows of message verdicts alone, five at a time: every
    third publishing launch fails and its window is re-run."""
    monkeypatch.setenv("COA_QUEUE_FAULT", "3")
    e = registered
    reqs = _msg_reqs()[:45]
    with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
        for lo in range(0, len(reqs), 5):
            _window(e, q, reqs[lo:lo + 5])
        m = q.metrics()
    assert m["windows"] == 9 and m["retried_windows"] == 3
    assert m["recovered_windows"] == 3 and m["failed_windows"] == 0

"""GPU: the aggregation queue's verdict requests -- Certificate::verify /
Header::verify / Vote::verify's whole DagResult decided in the window that
carries the request (k_window_verdict behind the window's crypto launches, or
k_msg_verdict_lat alone for a small window of message verdicts).

Cases, committee and expected words come from tests/verdict_cases.py (a
restatement of primary/src/messages.rs over hashlib and the C restatement of
dalek), never from the engine.  Every answer is compared with its expected
word; the crypto requests that share a window with verdict requests are
compared with the same requests submitted alone.  (Fault injection into
verdict windows: tests/test_gpu_verdict_recovery.py.)"""
import hashlib
import re
import threading

import numpy as np
import pytest

import message_cases as M
import verdict_cases as vc
from conftest import load_golden

pytestmark = pytest.mark.gpu

TIMEOUT = 60  # seconds a future may take: a lost callback fails instead of hanging
EINVAL_TEXT = "COA_EINVAL"


@pytest.fixture(scope="module")
def registered(engine):
    engine.committee_register_authorities(*vc.committee().arrays())
    yield engine
    engine.committee_register(np.zeros((0, 32), np.uint8))


@pytest.fixture(autouse=True)
def _queue_env(monkeypatch):
    for k in ("COA_QUEUE_IDLE_LAUNCH", "COA_QUEUE_FAULT", "COA_QUEUE_INLINE", "COA_QUEUE_MSG_LAT_MAX",
              "COA_QUEUE_TRACE_SLOW_US"):
        monkeypatch.delenv(k, raising=False)


def _votes(engine, case):
    return [(engine.PublicKey(pk), engine.Signature.from_bytes(sg)) for pk, sg in case["votes"]]


def _submit(engine, q, req):
    """req: (kind, case, expected word); kinds c (copied certificate), b
    (borrowed certificate), h, v."""
    kind, c = req[0], req[1]
    if kind in "cb":
        return q.submit_certificate_verdict(c["hdr"], c["id"], c["origin"], c["hsig"], c["round"], _votes(engine, c),
                                            c["count"], borrow=kind == "b")
    if kind == "h":
        return q.submit_header_verdict(c["hdr"], c["id"], c["author"], c["sig"], c["count"])
    return q.submit_vote_verdict(c["id"], c["round"], c["origin"], c["author"], c["sig"])


def _window(engine, q, reqs):
    """Submits reqs from 4 threads, closes the window (flush) and checks every
    word."""
    futs = [None] * len(reqs)

    def producer(t):
        for i in range(t, len(reqs), 4):
            futs[i] = _submit(engine, q, reqs[i])

    th = [threading.Thread(target=producer, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    q.flush()
    got = [f.result(timeout=TIMEOUT) for f in futs]
    wrong = [(i, r[0], r[1]["name"], hex(g), hex(int(r[2]))) for i, (r, g) in enumerate(zip(reqs, got)) if g != int(r[2])]
    assert not wrong, wrong[:10]
    assert vc.OPEN not in [g & 0xff for g in got]


def _cert_reqs(kind):
    want, _ = vc.expected_certificates()
    return [(kind, c, w) for c, w in zip(vc.certificate_cases(), want)]


def _msg_reqs():
    """Every header and vote case, interleaved."""
    reqs = [("h", c, w) for c, w in zip(vc.header_cases(), vc.expected_headers())]
    reqs += [("v", c, w) for c, w in zip(vc.vote_cases(), vc.expected_votes())]
    step = next(s for s in (101, 103, 107, 109) if np.gcd(s, len(reqs)) == 1)
    return [reqs[(i * step) % len(reqs)] for i in range(len(reqs))]


# ------------------------------------------------------------- certificates
@pytest.mark.parametrize("kind", ["c", "b"], ids=["copied", "borrowed"])
def test_every_certificate_case(registered, kind):
    e = registered
    reqs = _cert_reqs(kind)
    _, open_ok = vc.expected_certificates()
    counts = sorted({len(c["votes"]) for c in vc.certificate_cases()})
    assert {0, 1, 63, 64, 65, 68, 70} <= set(counts)
    with e.AggregationQueue(max_batch=1 << 16, max_delay_us=5_000_000) as q:
        _window(e, q, reqs)
        m, vs = q.metrics(), q.verdict_stats()
    assert vs == {"certificates": len(reqs), "headers": 0, "votes": 0, "verdict_windows": 1}
    assert m["certificates"] == len(reqs) and m["failed_windows"] == 0 and m["retried_windows"] == 0
    # only a certificate whose votes need the exact check goes to the resolver:
    # outsiders are answered by the protocol word in the window
    assert m["deferred_requests"] <= int(open_ok.sum())
    assert open_ok.any()


# --------------------------------------------------------- headers and votes
SHAPES = ["publish", "latency", "throughput"]
_TRACE = re.compile(r"\[coa queue\] slow window .* launch (\d+) d2h (\d+) event")


def _run_shape(e, monkeypatch, capfd, shape, reqs, sizes=None):
    """publish: a lone request per window (or windows of `sizes`, each at most
    64), answered by k_msg_verdict_lat's published words; latency: all in one
    window of that kernel, staged (status mode, whatever the window's size); throughput: all in one window of the
    throughput kernels plus k_window_verdict.  The queue's window trace tells
    the publish route from the staged one: it enqueues no device-to-host copy."""
    if shape == "throughput":
        monkeypatch.setenv("COA_QUEUE_MSG_LAT_MAX", "0")
    elif shape == "latency":
        monkeypatch.setenv("COA_QUEUE_MSG_LAT_MAX", "100000")
        monkeypatch.setenv("COA_QUEUE_INLINE", "0")  # no publish route: a window of at most 64 is staged too
    monkeypatch.setenv("COA_QUEUE_TRACE_SLOW_US", "0.001")  # every window traced
    if sizes is None:
        sizes = [1] * len(reqs) if shape == "publish" else [len(reqs)]
    assert sum(sizes) == len(reqs)
    capfd.readouterr()
    with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
        lo = 0
        for n in sizes:
            _window(e, q, reqs[lo:lo + n])
            lo += n
        ms, vs, m = q.message_stats(), q.verdict_stats(), q.metrics()
        signatures = q.stats()["signatures"]
    d2h = [int(x.group(2)) for x in _TRACE.finditer(capfd.readouterr().err)]
    assert len(d2h) == len(sizes)
    if shape == "publish":
        assert max(sizes) <= 64 and d2h == [0] * len(sizes)
    else:
        assert all(d2h)  # staged: the words come back with the output block's copy
    nh = sum(1 for r in reqs if r[0] == "h")
    nv = sum(1 for r in reqs if r[0] == "v")
    assert (ms["headers"], ms["votes"]) == (nh, nv) and signatures == nh + nv
    assert vs == {"certificates": 0, "headers": nh, "votes": nv, "verdict_windows": len(sizes)}
    assert m["requests"] == len(reqs) and m["failed_windows"] == 0 and m["retried_windows"] == 0
    assert m["windows"] == len(sizes)
    if shape == "throughput":
        assert (ms["latency_windows"], ms["throughput_windows"]) == (0, len(sizes))
    else:
        assert (ms["latency_windows"], ms["throughput_windows"]) == (len(sizes), 0)
    assert m["deferred_requests"] == 0  # a message verdict never goes to the resolver, outsiders included
    return m


@pytest.mark.parametrize("shape", SHAPES)
def test_every_header_and_vote_case(registered, monkeypatch, capfd, shape):
    """publish: one request per window, slots, tags and the device counter
    re-used window after window."""
    reqs = _msg_reqs()
    assert any(r[1]["author"] == vc.committee().w.out_pk for r in reqs)
    assert {int(r[2]) for r in reqs} == {vc.OK, vc.BAD_ID, vc.UNKNOWN_AUTHOR, vc.MALFORMED, vc.BAD_SIG}
    _run_shape(registered, monkeypatch, capfd, shape, reqs)


def test_published_windows_of_several_messages(registered, monkeypatch, capfd):
    """Publishing windows of 64, 33, 2 and the rest (at most 64 each): the
    last block's merge over every word of the window."""
    reqs = _msg_reqs()
    sizes = [64, 33, 2, 64]
    while sum(sizes) + 64 < len(reqs):
        sizes.append(64)
    sizes.append(len(reqs) - sum(sizes))
    assert 0 < sizes[-1] <= 64
    _run_shape(registered, monkeypatch, capfd, "publish", reqs, sizes)


def test_message_verdicts_beside_a_crypto_message_take_the_window_kernel(registered, monkeypatch, capfd):
    """One crypto header among the verdict requests: the window is not
    k_msg_verdict_lat's (the crypto request's status word must stay raw), and
    every word is still exact."""
    e = registered
    reqs = _msg_reqs()[:20]
    c = vc.header_cases()[0]
    want = int(M.expected_headers([c])[0])
    with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
        plain = q.submit_header(c["hdr"], c["id"], c["author"], c["sig"])
        _window(e, q, reqs)
        assert plain.result(timeout=TIMEOUT) == want
        assert q.message_stats()["latency_windows"] == 1 and q.verdict_stats()["verdict_windows"] == 1


# ------------------------------------------- lane strides and block boundaries
def _stride_headers():
    """Payload counts 63, 64 and 65 (one lane stride of the certificate role,
    and the per-lane loop of the message role): clean, a foreign worker id at
    the last index, one at index 0."""
    c = vc.committee()
    b = vc.Builder()
    author = c.honest[2]
    own = c.workers_of[author]
    out = []
    for n in (63, 64, 65):
        for name, wids in (("clean", [own[k % 3] for k in range(n)]),
                           ("foreign_last", [own[0]] * (n - 1) + [4242]),
                           ("foreign_first", [4242] + [own[1]] * (n - 1))):
            h = b.header(author, wids, tag=b"s%d" % n + name.encode())
            case = {"name": f"{name}_{n}", "hdr": h["hdr"], "id": h["id"], "author": author, "sig": h["hsig"],
                    "count": n}
            want = vc._header_word(c, case["hdr"], n, author, 0, 0)
            assert want == (vc.OK if name == "clean" else vc.MALFORMED)
            out.append(("h", case, want))
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_payload_counts_around_a_lane_stride(registered, monkeypatch, capfd, shape):
    _run_shape(registered, monkeypatch, capfd, shape, _stride_headers())


@pytest.mark.parametrize("n_certs", [5, 0])
def test_block_boundaries_of_both_roles(registered, monkeypatch, n_certs):
    """5 certificates (two blocks of the certificate role, kWaves = 4, the
    second with one live wave) + 1 header + 257 votes (two blocks of 256
    lanes of the message role, the second with two live lanes); and the same
    with no certificate-role block at all."""
    monkeypatch.setenv("COA_QUEUE_MSG_LAT_MAX", "0")
    e = registered
    certs = [r for r in _cert_reqs("c") if len(r[1]["votes"]) in (64, 65, 70)][:n_certs]
    assert len(certs) == n_certs
    hdr = _stride_headers()[1]
    votes = M.take([("v", c, w) for c, w in zip(vc.vote_cases(), vc.expected_votes())], 257)
    reqs = certs + [hdr] + votes
    with e.AggregationQueue(max_batch=1 << 16, max_delay_us=5_000_000) as q:
        _window(e, q, reqs)
        vs, ms = q.verdict_stats(), q.message_stats()
    assert vs == {"certificates": n_certs, "headers": 1, "votes": 257, "verdict_windows": 1}
    assert (ms["latency_windows"], ms["throughput_windows"]) == (0, 1)


# ------------------------------------------------------------ a mixed window
def _crypto_requests(e):
    """Requests of all six existing kinds: (submit(q) -> future, expected)."""
    hc, vt = vc.header_cases(), vc.vote_cases()
    hbits, vbad = M.expected_headers(list(hc)), M.expected_votes(list(vt))
    out = []
    for c, b in list(zip(hc, hbits))[::5]:
        out.append((lambda q, c=c: q.submit_header(c["hdr"], c["id"], c["author"], c["sig"]), int(b)))
    for c, b in list(zip(vt, vbad))[::3]:
        out.append((lambda q, c=c: q.submit_vote(c["id"], c["round"], c["origin"], c["author"], c["sig"]), int(b) == 0))
    for c, b in list(zip(vt, vbad))[1::7]:
        out.append((lambda q, c=c: q.submit_verify(M.vote_digest(c["id"], c["round"], c["origin"]), c["author"],
                                                   c["sig"]), int(b) == 0))
    # crypto certificates: the verdict cases themselves, answered with their COA_CERT_* bits
    for c in vc.certificate_cases()[:12:2]:
        out.append((lambda q, c=c: q.submit_certificate(c["hdr"], c["id"], c["origin"], c["hsig"], c["round"],
                                                        _votes(e, c)), None))
    g = next(g for g in load_golden("batch_vectors.json") if g["expect"] and len(g["pks"]) >= 2)
    out.append((lambda q: q.submit_batch(bytes.fromhex(g["msg"]),
                                         [(e.PublicKey(bytes.fromhex(p)), e.Signature.from_bytes(bytes.fromhex(s)))
                                          for p, s in zip(g["pks"], g["sigs"])]), True))
    return out


def test_mixed_window_leaves_the_crypto_requests_alone(registered):
    """All six existing kinds and the three verdict kinds interleaved in one
    window: the crypto answers are those of the same requests without the
    verdict requests, the words the expected ones."""
    e = registered
    crypto = _crypto_requests(e)
    blob = b"worker batch" * 50
    with e.AggregationQueue(max_batch=1 << 16, max_delay_us=5_000_000) as q:
        base = [s(q) for s, _ in crypto]
        q.flush()
        base = [f.result(timeout=TIMEOUT) for f in base]
        assert q.verdict_stats()["verdict_windows"] == 0
    for (_, want), got in zip(crypto, base):
        assert want is None or got == want
    verdicts = _cert_reqs("c")[::4] + _cert_reqs("b")[1::9] + _msg_reqs()[::3]
    with e.AggregationQueue(max_batch=1 << 16, max_delay_us=5_000_000) as q:
        mixed, words = [], []
        for i in range(max(len(crypto), len(verdicts))):
            if i < len(crypto):
                mixed.append(crypto[i][0](q))
            if i < len(verdicts):
                words.append(_submit(e, q, verdicts[i]))
        dig = q.submit_digest(blob)
        q.flush()
        assert [f.result(timeout=TIMEOUT) for f in mixed] == base
        got = [f.result(timeout=TIMEOUT) for f in words]
        wrong = [(r[0], r[1]["name"], hex(g), hex(int(r[2]))) for r, g in zip(verdicts, got) if g != int(r[2])]
        assert not wrong, wrong[:10]
        assert bytes(dig.result(timeout=TIMEOUT)) == hashlib.sha512(blob).digest()[:32]
        m, vs = q.metrics(), q.verdict_stats()
    assert m["failed_windows"] == 0 and vs["verdict_windows"] == 1
    assert vs["certificates"] + vs["headers"] + vs["votes"] == len(verdicts)


# --------------------------------------------------------------- generations
def test_generation_without_protocol_table_answers_einval(registered):
    """After plain coa_committee_register of the same keys the window's
    verdict requests come back COA_EINVAL; the crypto requests beside them
    stay correct, nothing is retried and no failure is counted."""
    e = registered
    pks, stakes, workers = vc.committee().arrays()
    e.committee_register(pks)
    try:
        hc, vt = vc.header_cases(), vc.vote_cases()
        hbits, vbad = M.expected_headers(list(hc)), M.expected_votes(list(vt))
        with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
            words = [_submit(e, q, r) for r in _msg_reqs()[::6] + _cert_reqs("c")[:6]]
            plain = [(q.submit_header(c["hdr"], c["id"], c["author"], c["sig"]), int(b))
                     for c, b in list(zip(hc, hbits))[::9]]
            plain += [(q.submit_vote(c["id"], c["round"], c["origin"], c["author"], c["sig"]), int(b) == 0)
                      for c, b in list(zip(vt, vbad))[::5]]
            q.flush()
            for f in words:
                with pytest.raises(e.EngineError, match=EINVAL_TEXT):
                    f.result(timeout=TIMEOUT)
            assert all(f.result(timeout=TIMEOUT) == want for f, want in plain)
            m = q.metrics()
        assert m["failed_windows"] == 0 and m["retried_windows"] == 0
    finally:
        e.committee_register_authorities(pks, stakes, workers)


def test_message_windows_without_protocol_table_answer_einval(registered, monkeypatch):
    """The windows k_msg_verdict_lat would answer (a lone request, publishing;
    several, staged): without a protocol table nothing runs for them, every
    request comes back COA_EINVAL and no failure is counted."""
    e = registered
    pks, stakes, workers = vc.committee().arrays()
    e.committee_register(pks)
    try:
        reqs = _msg_reqs()[:9]
        with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
            for lo, hi in ((0, 1), (1, 2), (2, 9)):
                futs = [_submit(e, q, r) for r in reqs[lo:hi]]
                q.flush()
                for f in futs:
                    with pytest.raises(e.EngineError, match=EINVAL_TEXT):
                        f.result(timeout=TIMEOUT)
            m, ms = q.metrics(), q.message_stats()
        assert m["windows"] == 3 and m["failed_windows"] == 0 and m["retried_windows"] == 0
        assert (ms["latency_windows"], ms["throughput_windows"]) == (3, 0)
    finally:
        e.committee_register_authorities(pks, stakes, workers)


def test_words_follow_the_generation_of_the_window(registered):
    """Re-registered with other stakes (the voters that reached the quorum no
    longer do), the same requests get the new table's words."""
    e = registered
    c = vc.committee()
    pks, stakes, workers = c.arrays()
    case = next(x for x in vc.certificate_cases() if x["name"] == "weight_at_quorum")
    voters = [pk for pk, _ in case["votes"]]
    hdr = next(r for r in _msg_reqs() if r[0] == "h" and r[1]["name"] == "payload_1")
    assert int(hdr[2]) == vc.OK
    # the non-voters fifty times heavier, and the header's author without stake
    heavy = [s if k in voters else 50 * s for k, s in zip(c.members, stakes)]
    heavy[c.members.index(hdr[1]["author"])] = 0
    stake_of = dict(zip(c.members, heavy))
    assert stake_of[case["origin"]] > 0 and sum(heavy) < 1 << 31
    # messages.rs:201-211 under the new stakes (the case has no reuse)
    zero = [j for j, pk in enumerate(voters) if stake_of[pk] == 0]
    want = vc.word(vc.UNKNOWN_VOTER, zero[0]) if zero else vc.QUORUM
    assert zero or sum(stake_of[pk] for pk in voters) < 2 * sum(heavy) // 3 + 1
    try:
        e.committee_register_authorities(pks, stakes, workers)
        with e.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
            _window(e, q, [("c", case, vc.OK), hdr])
            e.committee_register_authorities(pks, heavy, workers)
            _window(e, q, [("c", case, want), (hdr[0], hdr[1], vc.UNKNOWN_AUTHOR)])
    finally:
        e.committee_register_authorities(pks, stakes, workers)


# ----------------------------------------------------------------- C callers
def test_c_harness_gpu_mode(engine, tmp_path):
    """tests/c_abi/queue_verdict_harness.c: a C caller registers the committee,
    submits every case of the case file from 4 producer threads and compares
    the words (its own process; the committee it clears is that process's)."""
    from test_queue_verdicts import run_queue_verdict_harness

    run_queue_verdict_harness("gpu", tmp_path)

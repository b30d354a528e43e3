"""GPU: the message latency kernel (k_msg_verify_lat) and the aggregation
queue's header and vote requests on its three routes.

Cases, committee and expected values come from tests/message_cases.py:
hashlib.sha512 and the C restatement of dalek's verify_strict, never the
engine.  The latency kernel's raw words are compared with the throughput
entries' on the same device arrays; through the queue every answer is
compared with the expected one -- authors outside the committee (decided by
the resolver) included, with the committee registered and with none."""
import hashlib
import threading

import numpy as np
import pytest

import message_cases as M
from conftest import load_golden

pytestmark = pytest.mark.gpu

UNCACHED = 16
TIMEOUT = 60  # seconds a future may take: a lost callback fails instead of hanging


@pytest.fixture(scope="module")
def world():
    return M.World()


@pytest.fixture(scope="module")
def votes(world):
    cases = M.vote_cases(world, rounds=2)
    return cases, M.expected_votes(cases)


@pytest.fixture(scope="module")
def headers(world):
    """Every header case (9 lengths x 18) and one header of 8,300 bytes: 65
    SHA-512 blocks, one more than the schedule's LDS pass holds (KW_CHUNK =
    64), valid and with its last byte flipped."""
    cases = M.header_cases(world)
    hdr = bytes((7 * i + 3) & 0xFF for i in range(8300))
    id_ = hashlib.sha512(hdr).digest()[:32]
    import ed25519_ref as o

    sig = o.sign(world.seeds[2], id_)
    cases.append({"name": "long_valid", "hdr": hdr, "id": id_, "author": world.pks[2], "sig": sig})
    cases.append({"name": "long_flip_last", "hdr": M._flip(hdr, 8299), "id": id_, "author": world.pks[2], "sig": sig})
    cases.append({"name": "long_flip_second_pass", "hdr": M._flip(hdr, 8200), "id": id_, "author": world.out_pk,
                  "sig": o.sign(world.out_seed, id_)})
    return cases, M.expected_headers(cases)


@pytest.fixture
def registered(engine, world):
    assert engine.committee_register(world.registered_array()) == len(world.registered)


def _dev(x):
    import torch

    x = np.array(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _header_tensors(cases):
    a = M.header_arrays(cases)
    hdata = np.frombuffer(b"".join(a["header_inputs"]) + bytes(16), np.uint8)  # slack for the aligned dword reads
    hoff = np.zeros(len(cases) + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in a["header_inputs"]])
    return tuple(_dev(t) for t in (hdata, hoff, a["ids"], a["authors"], a["sigs"]))


def _vote_tensors(cases):
    a = M.vote_arrays(cases)
    return tuple(_dev(a[k]) for k in ("ids", "rounds", "origins", "authors", "sigs"))


def _status(n):
    import torch

    return torch.full((n,), -1, dtype=torch.int32, device=torch.device("cuda", 0))  # the calls zero it


def _words(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _raw_both(engine, hc, vc):
    """(latency words, throughput words) of hc headers then vc votes."""
    import torch

    ht = _header_tensors(hc) if hc else None
    vt = _vote_tensors(vc) if vc else None
    lat = _status(len(hc) + len(vc))
    engine.message_lat_verify_device(0, ht, vt, lat)
    tp = _status(len(hc) + len(vc))
    if hc:
        ws = torch.empty(engine.message_workspace_bytes(len(hc)), dtype=torch.uint8, device=lat.device)
        engine.header_verify_many_device(0, *ht, tp[:len(hc)], workspace=ws)
    if vc:
        ws = torch.empty(engine.message_workspace_bytes(len(vc)), dtype=torch.uint8, device=lat.device)
        engine.vote_verify_many_device(0, *vt, tp[len(hc):], workspace=ws)
    return _words(lat), _words(tp)


def _expected_raw(world, hc, hexp, vc, vexp):
    """The raw words where decided: 16 (and a header's digest bit) for an
    author outside the committee, else the expected bits."""
    out = []
    for c, e in zip(hc, hexp):
        out.append(UNCACHED | (int(e) & 1) if c["author"] == world.out_pk else int(e))
    for c, e in zip(vc, vexp):
        out.append(UNCACHED if c["author"] == world.out_pk else 2 * int(e))
    return out


def _check_raw(engine, world, hc, hexp, vc, vexp):
    lat, tp = _raw_both(engine, hc, vc)
    assert lat.tolist() == tp.tolist()
    assert lat.tolist() == _expected_raw(world, hc, hexp, vc, vexp)


def test_latency_words_every_header_case(engine, world, registered, headers):
    hc, hexp = headers
    assert len(hc) == 9 * 18 + 3 and set(hexp.tolist()) == {0, 1, 2, 3}
    assert hexp[-3:].tolist() == [0, 1, 1]  # the 65-block header: valid, flipped in its second LDS pass
    _check_raw(engine, world, hc, hexp, [], [])


def test_latency_words_every_vote_case(engine, world, registered, votes):
    vc, vexp = votes
    assert len(vc) == 102 and set(vexp.tolist()) == {0, 1}
    _check_raw(engine, world, [], [], vc, vexp)


def test_latency_words_single_and_mixed(engine, world, registered, headers, votes):
    hc, hexp = headers
    vc, vexp = votes
    for i in (0, 1, 12, len(hc) - 1):  # n = 1: valid, invalid, an outsider, the long header
        _check_raw(engine, world, [hc[i]], hexp[i:i + 1], [], [])
    for i in (0, 1, 12):
        _check_raw(engine, world, [], [], [vc[i]], vexp[i:i + 1])
    # both kinds in one launch, the counts no multiple of anything
    hs, vs = list(range(3, 3 + 37)), list(range(5, 5 + 29))
    _check_raw(engine, world, [hc[i] for i in hs] + [hc[-1]], np.append(hexp[hs], hexp[-1]), [vc[i] for i in vs],
               vexp[vs])


def test_latency_words_without_committee(engine, world, headers, votes):
    hc, hexp = headers
    vc, vexp = votes
    assert engine.committee_register(np.zeros((0, 32), np.uint8)) == 0
    try:
        lat, tp = _raw_both(engine, hc[:40], vc[:40])
        assert lat.tolist() == tp.tolist()
        assert lat.tolist() == [UNCACHED | (int(e) & 1) for e in hexp[:40]] + [UNCACHED] * 40
    finally:
        engine.committee_register(world.registered_array())


# ---------------------------------------------------------------------------
def _requests(hc, hexp, vc, vexp):
    """One request per message, headers and votes interleaved: (kind, case,
    expected future result)."""
    reqs = [("h", c, int(e)) for c, e in zip(hc, hexp)] + [("v", c, int(e) == 0) for c, e in zip(vc, vexp)]
    return [reqs[(i * 101) % len(reqs)] for i in range(len(reqs))]  # 101 is coprime to 267


def _submit(q, req):
    kind, c, _ = req
    if kind == "h":
        return q.submit_header(c["hdr"], c["id"], c["author"], c["sig"])
    return q.submit_vote(c["id"], c["round"], c["origin"], c["author"], c["sig"])


def _window(q, reqs):
    """Submits reqs from 4 threads, closes the window (flush) and checks every
    answer."""
    futs = [None] * len(reqs)

    def producer(t):
        for i in range(t, len(reqs), 4):
            futs[i] = _submit(q, reqs[i])

    th = [threading.Thread(target=producer, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    q.flush()
    wrong = [(i, r[0], r[1]["name"], f.result(timeout=TIMEOUT), r[2])
             for i, (r, f) in enumerate(zip(reqs, futs)) if f.result(timeout=TIMEOUT) != r[2]]
    assert not wrong, wrong[:10]


ROUTES = ["publish", "staged", "throughput"]


def _run_route(engine, monkeypatch, route, reqs):
    monkeypatch.delenv("COA_QUEUE_IDLE_LAUNCH", raising=False)
    monkeypatch.delenv("COA_QUEUE_FAULT", raising=False)
    monkeypatch.delenv("COA_QUEUE_INLINE", raising=False)
    if route == "publish":
        monkeypatch.delenv("COA_QUEUE_MSG_LAT_MAX", raising=False)
        sizes = [1, 64, 33, 64, 2, 64]  # consecutive windows, so slots, tags and the device counter are re-used
        sizes.append(len(reqs) - sum(sizes))
        assert 0 < sizes[-1] <= 64
        max_batch = 64
    else:
        monkeypatch.setenv("COA_QUEUE_MSG_LAT_MAX", "100000" if route == "staged" else "0")
        sizes = [len(reqs)]
        max_batch = 4096
    with engine.AggregationQueue(max_batch=max_batch, max_delay_us=5_000_000) as q:
        lo = 0
        for n in sizes:
            _window(q, reqs[lo:lo + n])
            lo += n
        ms, m = q.message_stats(), q.metrics()
        signatures = q.stats()["signatures"]
    nh = sum(1 for r in reqs if r[0] == "h")
    assert (ms["headers"], ms["votes"]) == (nh, len(reqs) - nh) and signatures == len(reqs)
    assert m["requests"] == len(reqs) and m["failed_windows"] == 0 and m["retried_windows"] == 0
    assert m["windows"] == len(sizes) and m["max_window"] == max(sizes)
    if route == "throughput":
        assert (ms["latency_windows"], ms["throughput_windows"]) == (0, len(sizes))
    else:
        assert (ms["latency_windows"], ms["throughput_windows"]) == (len(sizes), 0)
    assert m["window_max_kinds"] & (16 | 32) and not m["window_max_kinds"] & 15
    return m


@pytest.mark.parametrize("route", ROUTES)
def test_queue_routes_with_committee(engine, world, registered, headers, votes, monkeypatch, route):
    reqs = _requests(*headers, *votes)
    assert len(reqs) == 267
    m = _run_route(engine, monkeypatch, route, reqs)
    outsiders = sum(1 for r in reqs if r[1]["author"] == world.out_pk)
    assert outsiders > 0 and m["deferred_requests"] == outsiders


@pytest.mark.parametrize("route", ROUTES)
def test_queue_routes_without_committee(engine, world, headers, votes, monkeypatch, route):
    reqs = _requests(*headers, *votes)
    assert engine.committee_register(np.zeros((0, 32), np.uint8)) == 0
    try:
        m = _run_route(engine, monkeypatch, route, reqs)
        assert m["deferred_requests"] == len(reqs)  # everything through the resolver
    finally:
        engine.committee_register(world.registered_array())


def test_queue_all_kinds_at_once(engine, world, headers, votes, monkeypatch):
    """Headers, votes, bare signatures, certificates, a vote batch and a digest
    in one queue (the certificates' committee registered, so the World's
    honest authors are outsiders here): every kind exact."""
    import certificates as C

    monkeypatch.delenv("COA_QUEUE_MSG_LAT_MAX", raising=False)
    hc, hexp = headers
    vc, vexp = votes
    committee, batch = C.synth_certificates(6, committee_size=7, n_payload=3, seed=33)
    batch.vote_sigs[int(batch.offsets[2]) + 1, 40] ^= 1  # certificate 2: a bad vote
    batch.header_sigs[4, 33] ^= 1                        # certificate 4: a bad header signature
    want_cert = [0, 0, engine.CERT_BAD_VOTES, 0, engine.CERT_BAD_HEADER_SIG, 0]
    committee.register()
    try:
        with engine.AggregationQueue(max_batch=4096, max_delay_us=5_000_000) as q:
            out = []
            for c, e in list(zip(hc, hexp))[::3]:
                out.append((q.submit_header(c["hdr"], c["id"], c["author"], c["sig"]), int(e)))
            for c, e in list(zip(vc, vexp))[::2]:
                out.append((q.submit_vote(c["id"], c["round"], c["origin"], c["author"], c["sig"]), int(e) == 0))
            for c, e in list(zip(vc, vexp))[1::2]:  # the parent route: the producer hashes Vote::digest
                out.append((q.submit_verify(M.vote_digest(c["id"], c["round"], c["origin"]), c["author"], c["sig"]),
                            int(e) == 0))
            for i in range(len(batch)):
                vts = [(engine.PublicKey(bytes(batch.vote_pks[j])), engine.Signature.from_bytes(bytes(batch.vote_sigs[j])))
                       for j in range(int(batch.offsets[i]), int(batch.offsets[i + 1]))]
                out.append((q.submit_certificate(batch.header_inputs[i], bytes(batch.ids[i]), bytes(batch.authors[i]),
                                                 bytes(batch.header_sigs[i]), batch.round, vts), want_cert[i]))
            g = next(g for g in load_golden("batch_vectors.json") if g["expect"] and len(g["pks"]) >= 2)
            out.append((q.submit_batch(bytes.fromhex(g["msg"]),
                                       [(engine.PublicKey(bytes.fromhex(p)), engine.Signature.from_bytes(bytes.fromhex(s)))
                                        for p, s in zip(g["pks"], g["sigs"])]), True))
            blob = b"worker batch" * 50
            dig = q.submit_digest(blob)
            q.flush()
            wrong = [(i, f.result(timeout=TIMEOUT), e) for i, (f, e) in enumerate(out) if f.result(timeout=TIMEOUT) != e]
            assert not wrong, wrong[:10]
            assert bytes(dig.result(timeout=TIMEOUT)) == hashlib.sha512(blob).digest()[:32]
            m = q.metrics()
            assert m["failed_windows"] == 0 and m["deferred_requests"] > 0
            assert m["certificates"] == len(batch) and m["batches"] == 1 and m["digests"] == 1
    finally:
        engine.committee_register(world.registered_array())

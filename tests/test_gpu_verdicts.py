"""GPU: the verdict calls -- Certificate::verify / Header::verify /
Vote::verify decided on the device, protocol checks included -- in their
host-pointer and device-resident forms, against tests/verdict_cases.py's
restatement of primary/src/messages.rs (never the engine's own answers).

One call holds every certificate case (about 80, overlapping voter sets,
0 to 70 votes), so several waves of one block run certificates that use the
same committee slots."""
import numpy as np
import pytest

import verdict_cases as vc

pytestmark = pytest.mark.gpu


def _dev(x):
    import torch

    x = np.array(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    elif x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _hdr_dev(header_inputs):
    hdata = np.frombuffer(b"".join(header_inputs) + bytes(16), np.uint8)
    hoff = np.zeros(len(header_inputs) + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in header_inputs])
    return _dev(hdata), _dev(hoff)


def _out(n):
    import torch

    return torch.full((n,), -1, dtype=torch.int32, device=torch.device("cuda", 0))


def _ws(nbytes, own):
    import torch

    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=torch.device("cuda", 0)) if own else None


def _words(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _diff(cases, got, want):
    return [(c["name"], hex(int(g)), hex(int(w))) for c, g, w in zip(cases, got, want) if g != w]


@pytest.fixture(scope="module")
def registered(engine):
    engine.committee_register_authorities(*vc.committee().arrays())
    yield engine
    engine.committee_register(np.zeros((0, 32), np.uint8))


def _device_certificates(engine, cases, own):
    h, ids, origins, hsigs, rounds, vp, vs, off, counts = vc.certificate_arrays(cases)
    hdata, hoff = _hdr_dev(h)
    out = _out(len(cases))
    ws = _ws(engine.certificate_verdict_workspace_bytes(len(cases), vp.shape[0]), own)
    engine.certificate_verdict_many_device(0, hdata, hoff, _dev(ids), _dev(origins), _dev(hsigs), _dev(rounds),
                                           _dev(vp), _dev(vs), _dev(off), _dev(np.array(counts, np.uint32)), out,
                                           workspace=ws)
    return _words(out)


def test_host_forms_match_the_restatement(registered):
    e = registered
    cases = vc.certificate_cases()
    want, _ = vc.expected_certificates()
    got = e.certificate_verdict_many(*vc.certificate_arrays(cases), rng_seed=7)
    print("certificate words:", [hex(int(g)) for g in got])
    assert not _diff(cases, got, want)
    got = e.header_verdict_many(*vc.header_arrays(vc.header_cases()))
    assert not _diff(vc.header_cases(), got, vc.expected_headers())
    got = e.vote_verdict_many(*vc.vote_arrays(vc.vote_cases()))
    assert not _diff(vc.vote_cases(), got, vc.expected_votes())


@pytest.mark.parametrize("own", [False, True], ids=["engine_workspace", "caller_workspace"])
def test_device_forms_match_and_open_only_where_allowed(registered, own):
    e = registered
    cases = vc.certificate_cases()
    want, open_ok = vc.expected_certificates()
    got = _device_certificates(e, cases, own)
    is_open = got == vc.OPEN
    assert not (is_open & ~open_ok).any(), [c["name"] for c, o, a in zip(cases, is_open, open_ok) if o and not a]
    assert (is_open <= np.isin(want, (vc.OK, vc.BAD_VOTES))).all()
    assert not _diff(cases, np.where(is_open, want, got), want)
    assert is_open.any()  # a failed vote equation is left to the exact path
    host = e.certificate_verdict_many(*vc.certificate_arrays(cases), rng_seed=3)
    assert (host[~is_open] == got[~is_open]).all()

    hc = vc.header_cases()
    h, ids, authors, sigs, counts = vc.header_arrays(hc)
    hdata, hoff = _hdr_dev(h)
    out = _out(len(hc))
    e.header_verdict_many_device(0, hdata, hoff, _dev(ids), _dev(authors), _dev(sigs),
                                 _dev(np.array(counts, np.uint32)), out,
                                 workspace=_ws(e.message_verdict_workspace_bytes(len(hc)), own))
    assert not _diff(hc, _words(out), vc.expected_headers())
    vt = vc.vote_cases()
    ids, rounds, origins, authors, sigs = vc.vote_arrays(vt)
    out = _out(len(vt))
    e.vote_verdict_many_device(0, _dev(ids), _dev(rounds), _dev(origins), _dev(authors), _dev(sigs), out,
                               workspace=_ws(e.message_verdict_workspace_bytes(len(vt)), own))
    assert not _diff(vt, _words(out), vc.expected_votes())


def _tiled_certificates(k):
    """k tiles of the certificate cases: the call's arguments, its expected
    words and the oracle's crypto bits (co.certificate_verify_many over one
    tile, as expected_certificates calls it) with the certificates whose
    vote bit depends on the weights."""
    import coa_oracle as co

    h, ids, origins, hsigs, rounds, vp, vs, off, counts = vc.certificate_arrays(vc.certificate_cases())
    bits = co.certificate_verify_many(h, ids, origins, hsigs, rounds, vp, vs, off,
                                      np.random.default_rng(3).integers(0, 256, (vp.shape[0], 16), dtype=np.uint8))
    toff = np.concatenate([[0]] + [off[1:] + t * off[-1] for t in range(k)]).astype(np.uint64)
    args = (list(h) * k, np.tile(ids, (k, 1)), np.tile(origins, (k, 1)), np.tile(hsigs, (k, 1)), np.tile(rounds, k),
            np.tile(vp, (k, 1)), np.tile(vs, (k, 1)), toff, list(counts) * k)
    # verify_batch over a vote by a key with a torsion component answers by
    # its random weights (test_gpu_committee.py, weight-dependent classes), and
    # the engine draws its own: that certificate's vote bit has no one answer
    torsion = {vc.committee().w.mx_pk, vc.committee().w.small_pk, vc.committee().w.off_pk}
    by_weights = np.array([any(pk in torsion for pk, _ in c["votes"]) for c in vc.certificate_cases()])
    return (args, np.tile(vc.expected_certificates()[0], k), np.tile(np.asarray(bits, np.uint8), k),
            np.tile(by_weights, k))


def test_verdicts_through_the_pipelined_certificate_path(registered, monkeypatch):
    """6 tiles of the cases are 432 certificates and 12,342 jobs: with
    COA_CERT_CHUNK_JOBS=4096 (the least the runtime accepts) the call is at
    least twice a chunk, so it takes the pipelined path, in at least 4 chunks
    (the first closes at 2,048 jobs; tests/sanitize/stage_driver.cpp checks
    the cuts of this very set) over 2 buffer sets: a set is reused, chunks
    start at lo > 0, and each chunk's protocol tail runs on its own stream.
    The crypto-only call goes the same way with no tail."""
    e = registered
    args, want, bits, by_weights = _tiled_certificates(6)
    assert len(args[0]) + int(args[7][-1]) == 12_342
    monkeypatch.setenv("COA_CERT_CHUNK_JOBS", "4096")
    monkeypatch.setenv("COA_CERT_BUFFERS", "2")
    piped = e.certificate_verdict_many(*args, rng_seed=7)
    crypto = e.certificate_verify_many(*args[:8], rng_seed=7)
    monkeypatch.setenv("COA_CERT_PIPELINE", "0")
    whole = e.certificate_verdict_many(*args, rng_seed=7)
    crypto_whole = e.certificate_verify_many(*args[:8], rng_seed=7)
    names = [{"name": f"{c['name']}#{t}"} for t in range(6) for c in vc.certificate_cases()]
    assert not _diff(names, piped, want)
    assert not _diff(names, whole, want)
    print("vote bit by the weights:", [n["name"] for n, w in zip(names, by_weights) if w][:12])
    assert by_weights.sum() <= 6 * 4  # a few cases of the 72
    mask = np.where(by_weights, 3, 7).astype(np.uint8)  # BAD_VOTES is bit 2
    assert not _diff(names, crypto & mask, bits & mask)
    assert not _diff(names, crypto, crypto_whole)  # same seed, same weights: every bit


def test_device_form_answers_an_overrunning_count_malformed(registered):
    cases = [dict(c) for c in vc.certificate_cases() if c["name"] in ("payload_1", "clean_a")]
    for c in cases:
        c["count"] = (len(c["hdr"]) - 40) // 36 + 1
    got = _device_certificates(registered, cases, True)
    assert list(got) == [vc.MALFORMED, vc.MALFORMED]
    with pytest.raises(registered.EngineError, match="overruns"):
        registered.certificate_verdict_many(*vc.certificate_arrays(cases))


def test_c_harness_gpu_mode(engine, tmp_path):
    """tests/c_abi/verdict_harness.c: a C caller registers the committee and
    gets the restatement's words from the host-pointer forms (its own
    process; the committee it leaves cleared is that process's)."""
    from test_cpu_verdicts import run_verdict_harness

    run_verdict_harness("gpu", tmp_path)


def _same(a, b):
    return type(a) is type(b) and (a is None or [bytes(x) for x in a.args] == [bytes(x) for x in b.args])


def test_certificates_py_verdicts_equal_the_host_side_checks(registered):
    import certificates as cz
    from coa_crypto import Digest, PublicKey, Signature

    cases = vc.certificate_cases()
    com, certs = vc.as_objects(cases)
    got = cz.verdict_certificates(certs, rng_seed=5)
    want = cz.verify_certificates(certs, com, rng_seed=5)
    bad = [(c["name"], g, w) for c, g, w in zip(cases, got, want) if not _same(g, w)]
    assert not bad, bad
    headers = [c.header for c in certs]
    got, want = cz.verdict_headers(headers), cz.verify_headers(headers, com)
    assert all(_same(g, w) for g, w in zip(got, want))
    votes = [cz.Vote(Digest(v["id"]), v["round"], PublicKey(v["origin"]), PublicKey(v["author"]),
                     Signature.from_bytes(v["sig"])) for v in vc.vote_cases()]
    got, want = cz.verdict_votes(votes), cz.verify_votes(votes, com)
    assert all(_same(g, w) for g, w in zip(got, want))


def test_reregistration_changes_the_quorum_then_plain_registration_refuses(registered):
    e = registered
    c = vc.committee()
    cases = [x for x in vc.certificate_cases() if x["name"] in ("weight_one_below", "weight_at_quorum")]
    args = vc.certificate_arrays(cases)
    assert list(e.certificate_verdict_many(*args)) == [vc.OK, vc.QUORUM]
    pks, stakes, workers = c.arrays()
    try:
        # the small-order member (no voter here) loses its stake of 3: the
        # quorum 2 * total / 3 + 1 drops by 2, below the lighter certificate
        lighter = list(stakes)
        lighter[c.members.index(c.w.small_pk)] = 0
        assert 2 * sum(lighter) // 3 + 1 <= c.quorum - 1
        e.committee_register_authorities(pks, lighter, workers)
        assert list(e.certificate_verdict_many(*args)) == [vc.OK, vc.OK]
        # plain registration: no protocol table; the crypto calls still answer
        e.committee_register(pks)
        for call, a in ((e.certificate_verdict_many, args), (e.vote_verdict_many, vc.vote_arrays(vc.vote_cases()[:3])),
                        (e.header_verdict_many, vc.header_arrays(vc.header_cases()[:3]))):
            with pytest.raises(e.EngineError, match="without stakes"):
                call(*a)
        got = _out(3)
        ids, rounds, origins, authors, sigs = vc.vote_arrays(vc.vote_cases()[:3])
        with pytest.raises(e.EngineError, match="without stakes"):
            e.vote_verdict_many_device(0, _dev(ids), _dev(rounds), _dev(origins), _dev(authors), _dev(sigs), got)
        import message_cases as mc

        vt = vc.vote_cases()
        a = mc.vote_arrays(vt)
        assert (e.vote_verify_many(a["ids"], a["rounds"], a["origins"], a["authors"], a["sigs"])
                == mc.expected_votes(vt)).all()
    finally:
        e.committee_register_authorities(pks, stakes, workers)
    assert list(e.certificate_verdict_many(*args)) == [vc.OK, vc.QUORUM]


def test_host_forms_over_two_contexts(registered, monkeypatch):
    """Two contexts on device 0 and a small COA_MIN_SHARD: every host form
    runs as two index-range shards, the second with lo > 0 -- for a header
    shard the only way to a rebased header-offset array.  COA_MIN_SHARD=64
    gives 186 headers 2 shards and the certificates (2,057 jobs) 2; the 102
    votes need 32 (102 / 64 is one shard).  Last in the file: it re-opens the
    engine."""
    e = registered
    auth = vc.committee().arrays()
    try:
        e.shutdown()
        e.init_devices([0, 0])
        e.committee_register_authorities(*auth)
        monkeypatch.setenv("COA_MIN_SHARD", "64")
        hc, cc = vc.header_cases(), vc.certificate_cases()
        assert len(hc) // 64 >= 2 and (len(cc) + sum(len(c["votes"]) for c in cc)) // 64 >= 2
        got = e.header_verdict_many(*vc.header_arrays(hc))
        assert not _diff(hc, got, vc.expected_headers())
        got = e.certificate_verdict_many(*vc.certificate_arrays(cc), rng_seed=7)
        assert not _diff(cc, got, vc.expected_certificates()[0])
        monkeypatch.setenv("COA_MIN_SHARD", "32")
        vt = vc.vote_cases()
        assert len(vt) // 32 >= 2
        got = e.vote_verdict_many(*vc.vote_arrays(vt))
        assert not _diff(vt, got, vc.expected_votes())
    finally:
        e.shutdown()
        e.init(0)
        e.committee_register_authorities(*auth)

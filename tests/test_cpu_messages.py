"""CPU: the Header::verify / Vote::verify crypto entry points of
include/coa_verify.h without a GPU.

  * coa_cpu_header_verify_many / coa_cpu_vote_verify_many (csrc/coa_cpu.cpp)
    over every case of tests/message_cases.py -- honest, adversarial R / s,
    wrong signer, mutated message, mixed-order / small-order / off-curve
    author, unregistered author -- against hashlib.sha512 and the C
    restatement of dalek's verify_strict, on 1, 3 and the default number of
    threads;
  * the GPU forms refuse with COA_ENODEVICE when there is no device (no CPU
    fallback), and n = 0 is COA_OK everywhere;
  * certificates.verify_headers / verify_votes make ONE engine call each and
    raise in the reference's order (primary/src/messages.rs:48-67,131-142),
    with counting stand-ins for the engine calls.
"""
import hashlib

import numpy as np
import pytest

import coa_oracle as co
import message_cases as M


@pytest.fixture(scope="module")
def cc():
    import build

    build.build()
    import coa_crypto

    return coa_crypto


@pytest.fixture(scope="module")
def world():
    return M.World()


@pytest.fixture(scope="module")
def votes(world):
    cases = M.vote_cases(world, rounds=4)
    return cases, M.vote_arrays(cases), M.expected_votes(cases)


@pytest.fixture(scope="module")
def headers(world):
    cases = M.header_cases(world)
    return cases, M.header_arrays(cases), M.expected_headers(cases)


def _both_verdicts(cases, exp, accept_only=()):
    """Every case class has the verdict it was built for, and both occur."""
    by = {}
    for c, e in zip(cases, exp):
        by.setdefault(c["name"], set()).add(int(e))
    for name, seen in by.items():
        assert len(seen) == 1, (name, seen)
    ok = {n for n, s in by.items() if s == {0}}
    assert ok == set(accept_only), ok
    assert len(by) > len(ok)


def test_case_list_is_not_vacuous(votes, headers):
    vc, _, vexp = votes
    assert len(vc) >= 200
    _both_verdicts(vc, vexp, accept_only=("valid", "mixed_author", "outsider_valid"))
    hc, _, hexp = headers
    assert len(hc) >= 100
    assert {len(c["hdr"]) for c in hc} == set(M.HEADER_LENGTHS)
    _both_verdicts(hc, hexp, accept_only=("valid", "mixed_author", "outsider_valid"))
    assert set(int(x) for x in hexp) == {0, 1, 2, 3}
    assert {int(e) for c, e in zip(hc, hexp) if c["name"].startswith("hdr_flip")} == {1}
    assert {int(e) for c, e in zip(hc, hexp) if c["name"].startswith("both")} == {3}


@pytest.mark.parametrize("nthreads", [1, 3, 0])
def test_cpu_vote_verify_many(cc, votes, nthreads):
    _, a, exp = votes
    got = cc.cpu_vote_verify_many(a["ids"], a["rounds"], a["origins"], a["authors"], a["sigs"], nthreads=nthreads)
    assert got.tolist() == exp.tolist()


@pytest.mark.parametrize("nthreads", [1, 3, 0])
def test_cpu_header_verify_many(cc, headers, nthreads):
    _, a, exp = headers
    got = cc.cpu_header_verify_many(a["header_inputs"], a["ids"], a["authors"], a["sigs"], nthreads=nthreads)
    assert got.tolist() == exp.tolist()


def test_n_zero_is_ok(cc):
    L = cc.lib()
    assert L.coa_cpu_header_verify_many(None, None, None, None, None, 0, None, 1) == 0
    assert L.coa_cpu_vote_verify_many(None, None, None, None, None, 0, None, 1) == 0
    assert L.coa_header_verify_many(None, None, None, None, None, 0, None) == 0
    assert L.coa_vote_verify_many(None, None, None, None, None, 0, None) == 0
    assert L.coa_header_verify_many_device(0, None, None, None, None, None, 0, None, None, None) == 0
    assert L.coa_vote_verify_many_device(0, None, None, None, None, None, 0, None, None, None) == 0
    assert cc.cpu_vote_verify_many(np.zeros((0, 32), np.uint8), np.zeros(0, np.uint64), np.zeros((0, 32), np.uint8),
                                   np.zeros((0, 32), np.uint8), np.zeros((0, 64), np.uint8)).size == 0
    assert cc.cpu_header_verify_many([], np.zeros((0, 32), np.uint8), np.zeros((0, 32), np.uint8),
                                     np.zeros((0, 64), np.uint8)).size == 0


def test_cpu_forms_reject_null_arguments(cc):
    L = cc.lib()
    assert L.coa_cpu_header_verify_many(None, None, None, None, None, 1, None, 1) == -1
    assert L.coa_cpu_vote_verify_many(None, None, None, None, None, 1, None, 1) == -1


def test_gpu_forms_refuse_without_a_device(cc, votes, headers):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_messages.py")
    _, v, _ = votes
    _, h, _ = headers
    with pytest.raises(cc.EngineError, match="ENODEVICE|-2"):
        cc.vote_verify_many(v["ids"], v["rounds"], v["origins"], v["authors"], v["sigs"])
    with pytest.raises(cc.EngineError, match="ENODEVICE|-2"):
        cc.header_verify_many(h["header_inputs"], h["ids"], h["authors"], h["sigs"])
    L = cc.lib()
    buf = np.zeros(4096, np.uint8)
    p = buf.ctypes.data
    assert L.coa_header_verify_many(p, p, p, p, p, 1, p) == -2
    assert L.coa_vote_verify_many(p, p, p, p, p, 1, p) == -2
    assert L.coa_header_verify_many_device(0, p, p, p, p, p, 1, p, None, None) == -2
    assert L.coa_vote_verify_many_device(0, p, p, p, p, p, 1, p, None, None) == -2
    assert L.coa_message_workspace_bytes(1) > 0  # host arithmetic only


# ---------------------------------------------------------------------------
class Engine:
    """Counting stand-ins for the two engine calls of the mirrors, answering
    through hashlib and the C restatement of dalek."""

    def __init__(self, monkeypatch, cc):
        self.header_calls = self.header_items = self.vote_calls = self.vote_items = 0
        monkeypatch.setattr(cc, "header_verify_many", self.header_verify_many)
        monkeypatch.setattr(cc, "vote_verify_many", self.vote_verify_many)
        for name in ("engine_verify_strict", "verify_strict_many", "digest_many", "sha512_many"):
            monkeypatch.setattr(cc, name, self.forbidden)

    def forbidden(self, *a, **k):
        raise AssertionError("the mirrors make one engine call per window, not per-primitive calls")

    def header_verify_many(self, his, ids, authors, sigs):
        self.header_calls += 1
        self.header_items += len(his)
        out = []
        for hi, i, a, s in zip(his, ids, authors, sigs):
            out.append((hashlib.sha512(bytes(hi)).digest()[:32] != bytes(i)) |
                       2 * (not co.verify_strict(bytes(i), bytes(a), bytes(s))))
        return np.array(out, np.uint8)

    def vote_verify_many(self, ids, rounds, origins, authors, sigs):
        self.vote_calls += 1
        self.vote_items += len(ids)
        return np.array([not co.verify_strict(M.vote_digest(bytes(i), int(r), bytes(o)), bytes(a), bytes(s))
                         for i, r, o, a, s in zip(ids, rounds, origins, authors, sigs)], np.uint8)


def _kinds(res):
    return [None if e is None else type(e).__name__ for e in res]


def test_verify_headers_raises_in_the_reference_order(cc, world, monkeypatch):
    import certificates as C
    import ed25519_ref as o

    eng = Engine(monkeypatch, cc)
    pk = [cc.PublicKey(p) for p in world.pks]
    committee = C.Committee({p: 1 for p in world.pks[:6]}, {p: {0, 1} for p in world.pks[:6]})

    def header(author, seed, workers=(0,), bad_id=False, bad_sig=False):
        h = C.Header(pk[author], 4, {cc.Digest(hashlib.sha512(bytes([author, w])).digest()[:32]): w for w in workers},
                     {cc.Digest(bytes([author]) * 32)})
        h.id = cc.Digest(hashlib.sha512(h.digest_input()).digest()[:32])
        sig = o.sign(seed, bytes(h.id))
        if bad_sig:
            sig = M._flip(sig, 9)
        h.signature = cc.Signature.from_bytes(sig)
        if bad_id:
            h.id = cc.Digest(M._flip(bytes(h.id), 0))
        return h

    s = world.seeds
    hs = [header(0, s[0]),
          header(1, s[1], bad_sig=True),
          header(2, s[2], workers=(0, 7)),                      # worker 7 is not the author's
          header(8, s[8]),                                      # stake 0
          header(3, s[3], bad_id=True),
          header(8, s[8], workers=(9,), bad_id=True, bad_sig=True),   # every check fails: the id comes first
          header(8, s[8], workers=(9,), bad_sig=True),                # ... then the stake
          header(4, s[4], workers=(9,), bad_sig=True),                # ... then the worker ids
          header(5, s[5], workers=(1,))]
    got = C.verify_headers(hs, committee)
    assert _kinds(got) == [None, "InvalidSignature", "MalformedHeader", "UnknownAuthority", "InvalidHeaderId",
                           "InvalidHeaderId", "UnknownAuthority", "MalformedHeader", None]
    assert (eng.header_calls, eng.header_items) == (1, len(hs))
    assert C.verify_headers([], committee) == [] and eng.header_calls == 1


def test_verify_votes_raises_in_the_reference_order(cc, world, monkeypatch):
    import certificates as C
    import ed25519_ref as o

    eng = Engine(monkeypatch, cc)
    committee = C.Committee({p: 1 for p in world.pks[:6]})
    id_ = hashlib.sha512(b"current header").digest()[:32]

    def vote(author, seed, bad_sig=False, round_=9):
        sig = o.sign(seed, M.vote_digest(id_, 9, world.pks[0]))
        if bad_sig:
            sig = M._flip(sig, 50)
        return C.Vote(cc.Digest(id_), round_, cc.PublicKey(world.pks[0]), cc.PublicKey(world.pks[author]),
                      cc.Signature.from_bytes(sig))

    s = world.seeds
    vs = [vote(1, s[1]), vote(2, s[2], bad_sig=True), vote(7, s[7]), vote(7, s[7], bad_sig=True),
          vote(3, s[4]), vote(5, s[5], round_=10), vote(0, s[0])]
    got = C.verify_votes(vs, committee)
    assert _kinds(got) == [None, "InvalidSignature", "UnknownAuthority", "UnknownAuthority", "InvalidSignature",
                           "InvalidSignature", None]
    assert (eng.vote_calls, eng.vote_items) == (1, len(vs))
    assert C.verify_votes([], committee) == [] and eng.vote_calls == 1

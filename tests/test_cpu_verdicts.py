"""CPU: the verdict calls (Certificate::verify / Header::verify / Vote::verify
decided by the engine, protocol checks included) on the engine's CPU path.

The expected words are tests/verdict_cases.py's restatement of
primary/src/messages.rs over the oracle's crypto facts, never the engine's.
Also: certificates.py's verdict_* functions against the objects' own
verify_stepwise order, the rejections of the committee arrays, and the GPU
forms' refusal without a GPU."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import verdict_cases as vc


@pytest.fixture(scope="module")
def cc():
    import build

    build.build()
    import coa_crypto

    return coa_crypto


def _names(cases, got, want):
    return [(c["name"], hex(int(g)), hex(int(w))) for c, g, w in zip(cases, got, want) if g != w]


def test_certificate_words_match_the_restatement(cc):
    cases = vc.certificate_cases()
    want, _ = vc.expected_certificates()
    got = cc.cpu_certificate_verdict_many(*vc.certificate_arrays(cases), vc.committee().arrays(), rng_seed=7,
                                          nthreads=4)
    assert not _names(cases, got, want)
    # every code of the table is exercised, and both index-carrying codes beyond the first stride
    assert set(int(w) & 0xff for w in want) == set(range(9))
    assert vc.word(vc.REUSE, 67) in want and vc.word(vc.UNKNOWN_VOTER, 68) in want


def test_certificate_words_from_status_bits(cc):
    """The protocol checks and the merge alone, the crypto bits supplied."""
    import coa_oracle as co

    cases = vc.certificate_cases()
    want, _ = vc.expected_certificates()
    a = vc.certificate_arrays(cases)
    zs = np.random.default_rng(9).integers(0, 256, (int(a[7][-1]), 16), dtype=np.uint8)
    bits = co.certificate_verify_many(*a[:8], zs)
    got = cc.cpu_certificate_verdict_many(*a, vc.committee().arrays(), status=bits, nthreads=1)
    assert not _names(cases, got, want)


def test_header_and_vote_words_match_the_restatement(cc):
    com = vc.committee().arrays()
    hc, vt = vc.header_cases(), vc.vote_cases()
    got = cc.cpu_header_verdict_many(*vc.header_arrays(hc), com, nthreads=3)
    assert not _names(hc, got, vc.expected_headers())
    got = cc.cpu_vote_verdict_many(*vc.vote_arrays(vt), com, nthreads=3)
    assert not _names(vt, got, vc.expected_votes())
    # outsider and stake-0 authors: UNKNOWN_AUTHOR, after INVALID_HEADER_ID only
    c = vc.committee()
    for case, w in zip(hc, vc.expected_headers()):
        if case["author"] in (c.w.out_pk, c.honest[vc.Z]):
            assert w in (vc.UNKNOWN_AUTHOR, vc.BAD_ID), case["name"]
    for case, w in zip(vt, vc.expected_votes()):
        if case["author"] in (c.w.out_pk, c.honest[vc.Z]):
            assert w == vc.UNKNOWN_AUTHOR, case["name"]
    assert vc.UNKNOWN_AUTHOR in vc.expected_votes() and vc.MALFORMED in vc.expected_headers()


def _cpu_stepwise(monkeypatch, cc):
    """The objects' verify_stepwise with its three primitives on the CPU path."""
    monkeypatch.setattr(cc, "digest_many", lambda ms: [cc.Digest(hashlib.sha512(bytes(m)).digest()[:32]) for m in ms])
    monkeypatch.setattr(cc, "engine_verify_strict",
                        lambda d, pk, sg: cc.lib().coa_cpu_ed25519_verify_strict(bytes(d), 32, bytes(pk), bytes(sg)))

    def verify_batch(digest, votes, rng_seed=0):
        votes = list(votes)
        pks = b"".join(bytes(pk) for pk, _ in votes) or None
        sgs = b"".join(s.flatten() for _, s in votes) or None
        if cc.lib().coa_cpu_ed25519_verify_batch(bytes(digest), pks, sgs, len(votes), rng_seed or 1) != 0:
            raise cc.CryptoError("batch verification failed")

    monkeypatch.setattr(cc.Signature, "verify_batch", staticmethod(verify_batch))


def _same(a, b):
    return type(a) is type(b) and (a is None or [bytes(x) for x in a.args] == [bytes(x) for x in b.args])


def test_certificates_py_verdicts_equal_verify_stepwise(cc, monkeypatch):
    import certificates as cz

    _cpu_stepwise(monkeypatch, cc)
    cases = vc.certificate_cases()
    com, certs = vc.as_objects(cases)
    got = cz.verdict_certificates(certs, com, rng_seed=5, cpu=True)
    for case, cert, g in zip(cases, certs, got):
        try:
            cert.verify_stepwise(com, rng_seed=5)
            want = None
        except cz.DagError as e:
            want = e
        assert _same(g, want), (case["name"], g, want)


def test_headers_and_votes_py_verdicts(cc, monkeypatch):
    import certificates as cz
    from coa_crypto import Digest, PublicKey, Signature

    _cpu_stepwise(monkeypatch, cc)
    com, _ = vc.as_objects(())
    votes = [cz.Vote(Digest(v["id"]), v["round"], PublicKey(v["origin"]), PublicKey(v["author"]),
                     Signature.from_bytes(v["sig"])) for v in vc.vote_cases()]
    got = cz.verdict_votes(votes, com, cpu=True)
    for v, g in zip(votes, got):
        try:
            v.verify(com)
            want = None
        except cz.DagError as e:
            want = e
        assert _same(g, want), (g, want)
    _, certs = vc.as_objects(vc.certificate_cases())
    headers = [c.header for c in certs]
    got = cz.verdict_headers(headers, com, cpu=True)
    for h, g in zip(headers, got):
        try:
            h.verify(com)
            want = None
        except cz.DagError as e:
            want = e
        assert _same(g, want), (g, want)


def test_committee_arrays_are_validated(cc):
    c = vc.committee()
    pks, stakes, workers = c.arrays()
    one = vc.vote_arrays(vc.vote_cases()[:1])

    def rc(p, s, w):
        cp, cs, cw, co, cn = cc._committee_arrays(p, s, w)
        out = np.zeros(1, np.uint32)
        return cc.lib().coa_cpu_vote_verdict_many(*(x.ctypes.data for x in one), 1, cp.ctypes.data, cs.ctypes.data,
                                                  cw.ctypes.data, co.ctypes.data, cn, out.ctypes.data, 1)

    assert rc(pks, stakes, workers) == 0
    dup = pks.copy()
    dup[40] = dup[3]
    assert rc(dup, stakes, workers) == -1                                  # duplicate keys
    assert rc(pks, [2 ** 31 - 1] + stakes[1:], workers) == -1              # total stake >= 2^31
    assert rc(pks[:2], [2 ** 30, 2 ** 30 - 1], workers[:2]) == 0           # ... 2^31 - 1 is legal
    n = cc.MAX_AUTHORITIES + 1
    keys = np.zeros((n, 32), np.uint8)
    keys[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
    assert rc(keys, [1] * n, [[0]] * n) == -1                              # more than COA_MAX_AUTHORITIES
    assert rc(keys[:-1], [1] * (n - 1), [[0]] * (n - 1)) == 0
    assert rc(pks, [0] * len(stakes), workers) == 0                        # stake 0 is legal


def test_overrunning_payload_count_is_einval(cc):
    hc = vc.header_cases()[:3]
    a = list(vc.header_arrays(hc))
    a[4] = [0, 0, (len(hc[2]["hdr"]) - 40) // 36 + 1]
    with pytest.raises(cc.EngineError):
        cc.cpu_header_verdict_many(*a, vc.committee().arrays())
    cases = vc.certificate_cases()[:2]
    a = list(vc.certificate_arrays(cases))
    a[8] = [a[8][0], (len(cases[1]["hdr"]) - 40) // 36 + 1]
    with pytest.raises(cc.EngineError):
        cc.cpu_certificate_verdict_many(*a, vc.committee().arrays())


def test_n0_and_null_arguments(cc):
    L = cc.lib()
    assert L.coa_cpu_vote_verdict_many(None, None, None, None, None, 0, None, None, None, None, 0, None, 1) == 0
    assert L.coa_cpu_header_verdict_many(None, None, None, None, None, 0, None, None, None, None, None, 0, None, 1) == 0
    assert L.coa_cpu_vote_verdict_many(None, None, None, None, None, 1, None, None, None, None, 0, None, 1) == -1
    assert L.coa_certificate_verdict_many(None, None, None, None, None, None, None, None, None, 0, 0, None, None) == 0
    assert L.coa_header_verdict_many(None, None, None, None, None, 0, None, None) == 0
    assert L.coa_vote_verdict_many(None, None, None, None, None, 0, None) == 0


HARNESS_SRC = os.path.join(ROOT, "tests", "c_abi", "verdict_harness.c")
HARNESS = os.path.join(ROOT, "tests", "c_abi", "verdict_harness")


def run_verdict_harness(mode, tmp_path):
    """Builds tests/c_abi/verdict_harness.c (-std=c11 -Wall -Wextra -Werror)
    against the header and the library and runs it over the case file."""
    import build

    libdir = os.path.dirname(build.build())
    tmp = f"{HARNESS}.{os.getpid()}"
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"), HARNESS_SRC,
           "-o", tmp, "-L", libdir, "-lcoa_verify", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
           "-Wl,-rpath,/opt/rocm/lib"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    os.replace(tmp, HARNESS)
    path = str(tmp_path / "verdict_cases.bin")
    nc, nh, nv = vc.write_case_file(path)
    r = subprocess.run([HARNESS, path, mode], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"verdict harness ({mode}): {nc} certificates, {nh} headers, {nv} votes, 0 bad" in r.stdout


def test_c_harness_cpu_forms_and_refusal(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gpu_verdicts.py runs the harness in its gpu mode")
    run_verdict_harness("cpu", tmp_path)


def test_gpu_forms_refuse_without_a_gpu(cc):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: covered by tests/test_gpu_verdicts.py")
    pks, stakes, workers = vc.committee().arrays()
    with pytest.raises(cc.EngineError, match="COA_ENODEVICE|-2"):
        cc.committee_register_authorities(pks, stakes, workers)
    with pytest.raises(cc.EngineError, match="COA_ENODEVICE|-2"):
        cc.vote_verdict_many(*vc.vote_arrays(vc.vote_cases()[:2]))
    with pytest.raises(cc.EngineError, match="COA_ENODEVICE|-2"):
        cc.header_verdict_many(*vc.header_arrays(vc.header_cases()[:2]))
    with pytest.raises(cc.EngineError, match="COA_ENODEVICE|-2"):
        cc.certificate_verdict_many(*vc.certificate_arrays(vc.certificate_cases()[:2]))
    L = cc.lib()
    buf = np.zeros(64, np.uint64)
    p = buf.ctypes.data
    assert L.coa_certificate_verdict_many_device(0, p, p, p, p, p, p, p, p, p, 1, 1, p, p, None, None) == -2
    assert L.coa_header_verdict_many_device(0, p, p, p, p, p, 1, p, p, None, None) == -2
    assert L.coa_vote_verdict_many_device(0, p, p, p, p, p, 1, p, None, None) == -2

"""GPU: the fused Header::verify / Vote::verify crypto (k_msg_verify behind
coa_header_verify_many / coa_vote_verify_many and their device forms)
against hashlib.sha512 and the C restatement of dalek's verify_strict.

Cases, committee and expected values come from tests/message_cases.py (never
from the engine).  Covered: the chunk edges of the persistent grid (n = 1,
63, 64, 65, 257), three jobs per lane (n = 600 on a 256-lane grid: the
shared inversion's j > 0 leg, with unregistered authors' identity points in
the chain), the three comb variants, an empty committee (verdict
neutrality), the raw words of the device forms with a caller-owned and an
engine-owned workspace, the Python mirrors against Core.sanitize_frames on
bincode frames, and the host forms called from C through the header alone."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import message_cases as M
import wire_codec as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

UNCACHED = 16


@pytest.fixture(scope="module")
def world():
    return M.World()


@pytest.fixture(scope="module")
def votes(world):
    cases = M.vote_cases(world, rounds=2)
    return cases, M.expected_votes(cases)


@pytest.fixture(scope="module")
def headers(world):
    cases = M.header_cases(world)
    return cases, M.expected_headers(cases)


@pytest.fixture
def registered(engine, world):
    assert engine.committee_register(world.registered_array()) == len(world.registered)


def _host_votes(engine, cases):
    a = M.vote_arrays(cases)
    return engine.vote_verify_many(a["ids"], a["rounds"], a["origins"], a["authors"], a["sigs"])


def _host_headers(engine, cases):
    a = M.header_arrays(cases)
    return engine.header_verify_many(a["header_inputs"], a["ids"], a["authors"], a["sigs"])


def _dev(x):
    import torch

    x = np.array(x)  # a writable, contiguous copy
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _workspace(engine, n, own):
    import torch

    if not own:
        return None
    return torch.empty(engine.message_workspace_bytes(n), dtype=torch.uint8, device=torch.device("cuda", 0))


def _device_votes(engine, cases, own_workspace):
    import torch

    a = M.vote_arrays(cases)
    n = len(cases)
    status = torch.full((n,), -1, dtype=torch.int32, device=torch.device("cuda", 0))  # the call zeroes it
    ws = _workspace(engine, n, own_workspace)
    engine.vote_verify_many_device(0, _dev(a["ids"]), _dev(a["rounds"]), _dev(a["origins"]), _dev(a["authors"]),
                                   _dev(a["sigs"]), status, workspace=ws)
    torch.cuda.synchronize()
    return status.cpu().numpy().view(np.uint32)


def _device_headers(engine, cases, own_workspace):
    import torch

    a = M.header_arrays(cases)
    n = len(cases)
    hdata = np.frombuffer(b"".join(a["header_inputs"]), np.uint8)
    hoff = np.zeros(n + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in a["header_inputs"]])
    status = torch.full((n,), -1, dtype=torch.int32, device=torch.device("cuda", 0))
    ws = _workspace(engine, n, own_workspace)
    engine.header_verify_many_device(0, _dev(hdata), _dev(hoff), _dev(a["ids"]), _dev(a["authors"]), _dev(a["sigs"]),
                                     status, workspace=ws)
    torch.cuda.synchronize()
    return status.cpu().numpy().view(np.uint32)


def _outsiders(world, cases):
    return np.array([c["author"] == world.out_pk for c in cases])


def _check_raw(world, cases, raw, exp, sig_bit_only):
    """Raw device words: 16 exactly for the unregistered authors, for whom
    the signature is left undecided (a header's digest bit stands); every
    other word is the expected one."""
    out = _outsiders(world, cases)
    assert ((raw & UNCACHED) != 0).tolist() == out.tolist()
    want = np.where(out, exp & (0 if sig_bit_only else 1), exp).astype(np.uint32)
    assert (raw & ~np.uint32(UNCACHED)).tolist() == want.tolist()


def _mismatches(cases, got, exp):
    return [(i, c["name"], int(g), int(e)) for i, (c, g, e) in enumerate(zip(cases, got, exp)) if int(g) != int(e)]


def _run_all_forms(engine, world, vc, vexp, hc, hexp):
    assert not _mismatches(vc, _host_votes(engine, vc), vexp)
    assert not _mismatches(hc, _host_headers(engine, hc), hexp)
    for own in (True, False):
        _check_raw(world, vc, _device_votes(engine, vc, own), 2 * vexp.astype(np.uint32), True)
        _check_raw(world, hc, _device_headers(engine, hc, own), hexp.astype(np.uint32), False)


def test_every_case_default_combs(engine, world, registered, votes, headers):
    vc, vexp = votes
    hc, hexp = headers
    # non-vacuity: both verdicts, every status value, registered and not
    assert set(vexp.tolist()) == {0, 1} and set(hexp.tolist()) == {0, 1, 2, 3}
    assert _outsiders(world, vc).any() and _outsiders(world, hc).any()
    by = {}
    for c, e in zip(vc, vexp):
        by.setdefault(c["name"], set()).add(int(e))
    assert {n for n, s in by.items() if s == {0}} == {"valid", "mixed_author", "outsider_valid"}
    assert all(len(s) == 1 for s in by.values()) and len(by) == 17
    _run_all_forms(engine, world, vc, vexp, hc, hexp)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_chunk_edges(engine, world, registered, votes, headers, n):
    vc, vexp = votes
    hc, hexp = headers
    # start at a different case for every size, so n = 1 is not always "valid"
    vsel = [(i + n) % len(vc) for i in range(n)]
    hsel = [(i + n) % len(hc) for i in range(n)]
    _run_all_forms(engine, world, [vc[i] for i in vsel], vexp[vsel], [hc[i] for i in hsel], hexp[hsel])


def test_three_jobs_per_lane(engine, world, registered, votes, headers, monkeypatch):
    """600 jobs on a 256-lane grid: every lane parks two or three points and
    shares one inversion among them, outsiders' identity points and
    s >= l / bad-key jobs included."""
    monkeypatch.setenv("COA_CERT_LANES_TOTAL", "256")
    vc, vexp = votes
    hc, hexp = headers
    n = 600
    vsel, hsel = [i % len(vc) for i in range(n)], [i % len(hc) for i in range(n)]
    v, h = [vc[i] for i in vsel], [hc[i] for i in hsel]
    assert _outsiders(world, v).sum() >= 30 and {"s_plus_l", "off_curve_author"} <= {c["name"] for c in v}
    _run_all_forms(engine, world, v, vexp[vsel], h, hexp[hsel])


@pytest.mark.parametrize("variant", ["narrow", "kw16"])
def test_comb_variants(engine, world, votes, headers, monkeypatch, variant):
    """narrow: [s]B and [k](-A) from the radix-256 combs; kw16: the keys'
    radix-2^16 combs (chosen at registration)."""
    if variant == "narrow":
        monkeypatch.setenv("COA_WCOMB", "0")
        monkeypatch.setenv("COA_KEY_WCOMB", "0")
    else:
        monkeypatch.setenv("COA_KEY_WCOMB20_MB", "0")
    assert engine.committee_register(world.registered_array()) == len(world.registered)
    vc, vexp = votes
    hc, hexp = headers
    _run_all_forms(engine, world, vc, vexp, hc, hexp)


def test_empty_committee_gives_the_same_outputs(engine, world, votes, headers):
    vc, vexp = votes
    hc, hexp = headers
    assert engine.committee_register(np.zeros((0, 32), np.uint8)) == 0
    assert not _mismatches(vc, _host_votes(engine, vc), vexp)
    assert not _mismatches(hc, _host_headers(engine, hc), hexp)
    raw = _device_votes(engine, vc, True)
    assert (raw == UNCACHED).all()  # nothing is decided without a committee
    raw = _device_headers(engine, hc, False)
    assert (raw == (UNCACHED | (hexp & 1))).all()
    assert engine.committee_register(world.registered_array()) == len(world.registered)
    assert not _mismatches(vc, _host_votes(engine, vc), vexp)
    assert not _mismatches(hc, _host_headers(engine, hc), hexp)


# ---------------------------------------------------------------------------
def _kind(e):
    return None if e is None else type(e).__name__


def test_mirrors_agree_with_sanitize_frames(engine, world, registered):
    """verify_headers / verify_votes over a window decoded by the native wire
    decoder give, item for item, what Core.sanitize_frames gives for the same
    frames (its round and expected-vote checks pass for every frame here)."""
    import certificates as C
    import ed25519_ref as o
    import sanitize as S

    members = world.pks[:6] + [world.mx_pk]
    committee = C.Committee({p: 1 for p in members}, {p: {0, 1} for p in members})
    frames = []
    for i, variant in enumerate(["ok", "bad_sig", "bad_worker", "stake0", "outsider", "bad_id", "ok", "bad_id_sig"]):
        a = i % 6
        author, seed = world.pks[a], world.seeds[a]
        if variant == "stake0":
            author, seed = world.pks[8], world.seeds[8]  # registered key without stake
        if variant == "outsider":
            author, seed = world.out_pk, world.out_seed
        pay = [(hashlib.sha512(b"batch%d%d" % (i, k)).digest()[:32], 9 if variant == "bad_worker" else k % 2)
               for k in range(i % 3 + 1)]
        par = [hashlib.sha512(b"parent%d%d" % (i, k)).digest()[:32] for k in range(i % 4)]
        id_ = hashlib.sha512(W.header_digest_input(author, 5, pay, par)).digest()[:32]
        sig = o.sign(seed, id_)
        if variant in ("bad_sig", "bad_id_sig"):
            sig = M._flip(sig, 44)
        if variant in ("bad_id", "bad_id_sig"):
            id_ = M._flip(id_, 3)
        frames.append(W.primary_message(0, W.header(author, 5, pay, par, id_, sig)))
    cur = C.Header(engine.PublicKey(world.pks[0]), 5, {}, set())
    cur.id = engine.Digest(hashlib.sha512(cur.digest_input()).digest()[:32])
    vd = M.vote_digest(bytes(cur.id), 5, world.pks[0])
    for i, variant in enumerate(["ok", "bad_sig", "stake0", "outsider", "mixed", "ok", "outsider_bad"]):
        a = (i + 1) % 6
        author, sig = world.pks[a], o.sign(world.seeds[a], vd)
        if variant == "bad_sig":
            sig = o.sign(world.seeds[a + 1], vd)
        if variant == "stake0":
            author, sig = world.pks[9], o.sign(world.seeds[9], vd)
        if variant.startswith("outsider"):
            author, sig = world.out_pk, o.sign(world.out_seed, vd)
        if variant == "outsider_bad":
            sig = M._flip(sig, 2)
        if variant == "mixed":
            import random

            author, sig = world.mx_pk, world.mixed_sign(vd, random.Random(3))
        frames.append(W.primary_message(1, W.vote(bytes(cur.id), 5, world.pks[0], author, sig)))
    want = [_kind(e) for _, e in S.Core(committee, gc_round=0, current_header=cur).sanitize_frames(frames)]
    assert want == [None, "InvalidSignature", "MalformedHeader", "UnknownAuthority", "UnknownAuthority",
                    "InvalidHeaderId", None, "InvalidHeaderId",
                    None, "InvalidSignature", "UnknownAuthority", "UnknownAuthority", None, None, "UnknownAuthority"]
    dh = engine.wire_decode_headers(frames[:8])
    got_h = C.verify_headers([S._header_from(dh, j) for j in range(8)], committee)
    dv = engine.wire_decode_votes(frames[8:])
    vs = [C.Vote(engine.Digest(bytes(dv["ids"][j])), int(dv["rounds"][j]), engine.PublicKey(bytes(dv["origins"][j])),
                 engine.PublicKey(bytes(dv["authors"][j])), engine.Signature.from_bytes(bytes(dv["sigs"][j])))
          for j in range(len(frames) - 8)]
    got_v = C.verify_votes(vs, committee)
    assert [_kind(e) for e in got_h + got_v] == want
    # the engine's bits for the window, straight from the decoded arrays
    st = engine.header_verify_many(dh["header_inputs"], dh["ids"], dh["authors"], dh["sigs"])
    assert st.tolist() == [0, 2, 0, 0, 0, 3, 0, 3]
    vv = engine.vote_verify_many(dv["ids"], dv["rounds"], dv["origins"], dv["authors"], dv["sigs"])
    assert vv.tolist() == [0, 1, 0, 0, 0, 0, 1]


# ---------------------------------------------------------------------------
HSRC = os.path.join(ROOT, "tests", "c_abi", "message_harness.c")
HOUT = os.path.join(ROOT, "tests", "c_abi", "message_harness")


def build_message_harness():
    import build

    libdir = os.path.dirname(build.build())
    tmp = f"{HOUT}.{os.getpid()}"
    cmd = ["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-pedantic", "-O1", "-I", os.path.join(ROOT, "include"),
           HSRC, "-o", tmp, "-L", libdir, "-lcoa_verify", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib",
           "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    os.replace(tmp, HOUT)
    return HOUT


def write_message_vectors(path, world, vc, vexp, hc, hexp):
    """The harness's input: committee keys, headers and votes with the
    expected outputs (little-endian; see message_harness.c)."""
    hdata = b"".join(c["hdr"] for c in hc)
    hoff = np.zeros(len(hc) + 1, np.uint64)
    hoff[1:] = np.cumsum([len(c["hdr"]) for c in hc])
    out = [struct.pack("<5I", 0x4D414F43, len(world.registered), len(hc), len(vc), len(hdata)),
           b"".join(world.registered), hoff.tobytes(), hdata]
    for key in ("id", "author", "sig"):
        out.append(b"".join(c[key] for c in hc))
    out.append(bytes(int(e) for e in hexp))
    out.append(b"".join(c["id"] for c in vc))
    out.append(np.array([c["round"] for c in vc], np.uint64).tobytes())
    for key in ("origin", "author", "sig"):
        out.append(b"".join(c[key] for c in vc))
    out.append(bytes(int(e) for e in vexp))
    with open(path, "wb") as f:
        f.write(b"".join(out))


def test_c_harness_host_forms(world, votes, headers, tmp_path):
    vc, vexp = votes
    hc, hexp = headers
    exe = build_message_harness()
    vec = tmp_path / "message_vectors.bin"
    write_message_vectors(vec, world, vc, vexp, hc, hexp)
    r = subprocess.run([exe, str(vec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert f"message harness ok ({len(hc)} headers, {len(vc)} votes)" in r.stdout

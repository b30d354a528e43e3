"""GPU: the device-resident wire decoder (coa_wire_*_device) and the fused
frames-to-verdicts calls (coa_wire_*_verdict_many).

Expected fields come from the independent encoder tests/wire_codec.py (the
fields a frame was built from, header_digest_input) and from the host decoder
coa_wire.cpp -- the sequential driver of the rules the kernels split over
lanes (coa_wire_parse.h), which tests/test_wire.py pins against that encoder
and tests/test_wire_parse_host.py against an independent model; expected
verdict words from tests/verdict_cases.py and the oracle.  Nothing expected
comes from the kernels under test.

The frames sit in a device buffer with 4 KiB of slack behind them and
frame_bytes is the true size, so a wrong bound reads allocated memory and
shows as a wrong answer.  The kernels' work split at its own boundaries
(alignment, the staging switch, the prefix sums, output extents, the offsets
rule) is tests/test_gpu_wire_device_edges.py.

Header cases of verdict_cases.py whose digest input no frame can carry (random
bytes: it does not start with the author, or its sets are not in key order) go
through as the frame built from their fields; the expected word is then
verdict_cases' rule and the oracle over the digest input that frame decodes to
(wire_dev_cases.verdict_frame), never the engine's answer."""
import functools
import hashlib

import numpy as np
import pytest

import verdict_cases as vc
import wire_codec as W
import wire_dev_cases as cases

pytestmark = pytest.mark.gpu

HEADER, VOTE, CERTIFICATE = 0, 1, 2
SLACK = 4096


def _dev(x):
    import torch

    x = np.array(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    elif x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _np(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


GUARD = 256
BYTE_ARRAYS = ("hdata", "ids", "authors", "origins", "sigs", "vpks", "vsigs")


def device_decode(e, kind, frames, own=False, guard=False, shift=0, frames_shift=0, offsets=None, slack=None):
    """One coa_wire_decode_*_device call over `frames`; every output as numpy.
    own: a caller workspace, on a stream that is not the default one.
    guard: every output and a caller workspace of exactly
    wire_workspace_bytes lie inside larger allocations, GUARD pattern bytes
    before and after each, and are of exactly the capacities the call states
    (hdata frame_bytes + 16, vpks / vsigs wire_votes_bound rows);
    out["bands"] names every array whose bands the call changed.
    shift: the byte arrays start this many bytes into their allocation.
    frames_shift: the frames tensor is a view this many bytes into its allocation.
    offsets: the frame offsets (default: the frames back to back); `frames` is
    then the buffer's content in order, n = len(offsets) - 1.
    slack: what lies behind frame_bytes (default SLACK bytes of 0xee)."""
    import torch

    blob = b"".join(frames)
    fb = len(blob)
    if offsets is None:
        offs = np.zeros(len(frames) + 1, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in frames])
    else:
        offs = np.array(offsets, np.uint64)
        assert int(offs.max()) <= fb + SLACK  # inside the allocation
    n = len(offs) - 1
    tail = (slack or b"") + b"\xee" * (SLACK - len(slack or b""))
    assert len(tail) == SLACK
    d_frames = _dev(np.frombuffer(b"\xdd" * frames_shift + blob + tail, np.uint8))[frames_shift:]
    d_offs = _dev(offs)
    dev = torch.device("cuda", 0)
    raw = {}

    def fill(name, shape, dt, exact=None):
        if not guard and not (shift and name in BYTE_ARRAYS):
            return torch.full(shape, 0x5a, dtype=dt, device=dev)
        if guard and exact is not None:
            shape = exact
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        lo = (GUARD if guard else 0) + (shift if name in BYTE_ARRAYS else 0)
        buf = torch.full((lo + nbytes + GUARD,), 0x5a, dtype=torch.uint8, device=dev)
        raw[name] = (buf, lo, nbytes)
        return buf[lo:lo + nbytes].view(dt).view(shape)

    nvb = e.wire_votes_bound(fb)
    o = dict(hdata=fill("hdata", (fb + 16 + SLACK,), torch.uint8, (fb + 16,)), hoff=fill("hoff", (n + 1,), torch.int64),
             ids=fill("ids", (n, 32), torch.uint8), authors=fill("authors", (n, 32), torch.uint8),
             origins=fill("origins", (n, 32), torch.uint8), sigs=fill("sigs", (n, 64), torch.uint8),
             rounds=fill("rounds", (n,), torch.int64), pcounts=fill("pcounts", (n,), torch.int32),
             vpks=fill("vpks", (max(nvb, 1), 32), torch.uint8, (nvb, 32)),
             vsigs=fill("vsigs", (max(nvb, 1), 64), torch.uint8, (nvb, 64)), voff=fill("voff", (n + 1,), torch.int64),
             kinds=fill("kinds", (n,), torch.int32), totals=fill("totals", (4,), torch.int64))
    kw = {}
    side = None
    if own or guard:
        if guard:
            ws = fill("workspace", (e.wire_workspace_bytes(n, fb),), torch.uint8)
            assert ws.data_ptr() % 256 == 0
        else:
            ws = torch.empty(max(e.wire_workspace_bytes(n, fb), 16), dtype=torch.uint8, device=dev)
        side = torch.cuda.Stream(device=0)
        side.wait_stream(torch.cuda.current_stream(0))
        kw = dict(stream=side, workspace=ws)
    kw["frame_bytes"] = fb
    if kind == CERTIFICATE:
        e.wire_decode_certificates_device(0, d_frames, d_offs, o["hdata"], o["hoff"], o["ids"], o["authors"], o["sigs"],
                                          o["rounds"], o["vpks"], o["vsigs"], o["voff"], o["pcounts"], o["kinds"],
                                          o["totals"], **kw)
    elif kind == HEADER:
        e.wire_decode_headers_device(0, d_frames, d_offs, o["hdata"], o["hoff"], o["ids"], o["authors"], o["sigs"],
                                     o["pcounts"], o["rounds"], o["kinds"], o["totals"], **kw)
    else:
        e.wire_decode_votes_device(0, d_frames, d_offs, o["ids"], o["rounds"], o["origins"], o["authors"], o["sigs"],
                                   o["kinds"], o["totals"], **kw)
    if side is not None:
        side.synchronize()
    torch.cuda.synchronize()
    out = {k: _np(v) for k, v in o.items()}
    for k in ("hoff", "voff", "rounds", "totals"):
        out[k] = out[k].view(np.uint64)
    out["pcounts"] = out["pcounts"].view(np.uint32)
    out["tensors"] = o
    out["frame_bytes"] = fb
    out["bands"] = [k for k, (buf, lo, nbytes) in raw.items()
                    if not (bool((buf[:lo] == 0x5a).all()) and bool((buf[lo + nbytes:] == 0x5a).all()))]
    return out


def expected_kinds(e, items):
    """The host scan's kinds; COA_WIRE_ECAPACITY where the case says so (and
    the host accepts the frame)."""
    hk, _, _ = e.wire_scan([c["frame"] for c in items])
    hk = hk.copy()
    for i, c in enumerate(items):
        if c.get("kind") == e.WIRE_ECAPACITY:
            assert hk[i] in (HEADER, CERTIFICATE)
            hk[i] = e.WIRE_ECAPACITY
        elif c.get("kind") is not None:
            assert hk[i] == c["kind"], (i, hk[i], c["kind"])
    return hk


def check_decode(e, kind, items, got):
    """Every array of one decode call against the host decoder and, where the
    case carries its fields, against wire_codec."""
    frames = [c["frame"] for c in items]
    n = len(frames)
    want_kinds = expected_kinds(e, items)
    assert got["kinds"].tolist() == want_kinds.tolist()
    mine = [i for i in range(n) if want_kinds[i] == kind]
    sub = [frames[i] for i in mine]
    if kind == CERTIFICATE:
        h = e.wire_decode_certificates(sub)
        h_auth, h_sigs = h["origins"], h["header_sigs"]
    elif kind == HEADER:
        h = e.wire_decode_headers(sub)
        h_auth, h_sigs = h["authors"], h["sigs"]
    else:
        h = e.wire_decode_votes(sub)
        h_auth, h_sigs = h["authors"], h["sigs"]
    hb = nv = 0
    if kind != VOTE:
        assert int(got["hoff"][0]) == 0
    if kind == CERTIFICATE:
        assert int(got["voff"][0]) == 0
    k = 0
    for i in range(n):
        if i in mine and k < len(mine) and mine[k] == i:
            c = items[i]
            assert bytes(got["ids"][i]) == bytes(h["ids"][k]), i
            assert bytes(got["authors"][i]) == bytes(h_auth[k]), i
            assert bytes(got["sigs"][i]) == bytes(h_sigs[k]), i
            assert int(got["rounds"][i]) == int(h["rounds"][k]), i
            if kind == VOTE:
                assert bytes(got["origins"][i]) == bytes(h["origins"][k]), i
                if "origin" in c:
                    assert (bytes(got["ids"][i]), int(got["rounds"][i]), bytes(got["origins"][i]), bytes(got["authors"][i]),
                            bytes(got["sigs"][i])) == (c["id"], c["round"], c["origin"], c["author"], c["sig"]), i
            else:
                lo, hi = int(got["hoff"][i]), int(got["hoff"][i + 1])
                assert lo == hb, i
                assert bytes(got["hdata"][lo:hi]) == h["header_inputs"][k], i
                assert int(got["pcounts"][i]) == int(h["payload_counts"][k]), i
                hb = hi
                if "payload" in c:
                    assert bytes(got["hdata"][lo:hi]) == W.header_digest_input(c["author"], c["round"], c["payload"],
                                                                               c["parents"]), i
                    assert (bytes(got["ids"][i]), bytes(got["authors"][i]), bytes(got["sigs"][i]),
                            int(got["rounds"][i])) == (c["id"], c["author"], c["sig"], c["round"]), i
                    assert int(got["pcounts"][i]) == len({bytes(d) for d, _ in c["payload"]}), i
            if kind == CERTIFICATE:
                lo, hi = int(got["voff"][i]), int(got["voff"][i + 1])
                hlo, hhi = int(h["vote_offsets"][k]), int(h["vote_offsets"][k + 1])
                assert lo == nv and hi - lo == hhi - hlo, i
                assert got["vpks"][lo:hi].tobytes() == h["vote_pks"][hlo:hhi].tobytes(), i
                assert got["vsigs"][lo:hi].tobytes() == h["vote_sigs"][hlo:hhi].tobytes(), i
                nv = hi
                if "votes" in c:
                    assert [(bytes(a), bytes(b)) for a, b in zip(got["vpks"][lo:hi], got["vsigs"][lo:hi])] == \
                        [(bytes(a), bytes(b)) for a, b in c["votes"]], i
            k += 1
        else:
            # the placeholder: zeroed fields, no header bytes, no votes
            assert not got["ids"][i].any() and not got["authors"][i].any() and not got["sigs"][i].any(), i
            assert int(got["rounds"][i]) == 0, i
            if kind == VOTE:
                assert not got["origins"][i].any(), i
            else:
                assert int(got["pcounts"][i]) == 0 and int(got["hoff"][i + 1]) == int(got["hoff"][i]) == hb, i
            if kind == CERTIFICATE:
                assert int(got["voff"][i + 1]) == int(got["voff"][i]) == nv, i
    assert k == len(mine)
    assert got["totals"].tolist() == [hb, nv, len(mine), n - len(mine)]
    # nothing written past what the call's capacities promise
    if kind != VOTE:
        assert (got["hdata"][got["frame_bytes"] + 16:] == 0x5a).all()


# ---------------------------------------------------------------- test 1
@pytest.mark.parametrize("own", [False, True], ids=["engine_workspace", "caller_workspace_side_stream"])
@pytest.mark.parametrize("n", [1, 40])
def test_small_certificates_field_for_field(engine, n, own):
    items = cases.small_certificates()[:n]
    check_decode(engine, CERTIFICATE, items, device_decode(engine, CERTIFICATE, [c["frame"] for c in items], own=own))


# ---------------------------------------------------------------- test 2
def test_sort_and_dedupe_boundaries(engine):
    items = cases.boundary_frames()
    frames = [c["frame"] for c in items]
    assert {c["kind"] for c in items} == {HEADER, CERTIFICATE}
    check_decode(engine, HEADER, items, device_decode(engine, HEADER, frames))
    got = device_decode(engine, CERTIFICATE, frames, own=True)
    check_decode(engine, CERTIFICATE, items, got)
    # all parents equal collapse to one; of a key repeated three times the last worker id wins
    same = [c for c in items if len(c["parents"]) > 1 and len(set(c["parents"])) == 1]
    assert len(same) == 4
    three = [(i, c) for i, c in enumerate(items) if len(c["payload"]) == 9 and len({d for d, _ in c["payload"]}) == 7]
    assert len(three) == 2
    for i, c in three:
        d = c["payload"][0][0] if c["kind"] == HEADER else c["payload"][-1][0]
        last = [w for k, w in c["payload"] if k == d][-1]
        g = got if c["kind"] == CERTIFICATE else device_decode(engine, HEADER, [c["frame"]])
        j = i if c["kind"] == CERTIFICATE else 0
        entries = bytes(g["hdata"][int(g["hoff"][j]) + 40:int(g["hoff"][j]) + 40 + 36 * 7])
        assert entries.count(d) == 1 and entries[entries.index(d) + 32:][:4] == last.to_bytes(4, "little")


# ---------------------------------------------------------------- test 3
def test_key_strings(engine):
    items = cases.key_string_frames()
    frames = [c["frame"] for c in items]
    kinds = expected_kinds(engine, items)
    assert {-10, -11, -12} <= set(kinds.tolist())  # the malformed set gives each of the host's codes
    for kind in (HEADER, VOTE, CERTIFICATE):
        check_decode(engine, kind, items, device_decode(engine, kind, frames))


# ---------------------------------------------------------------- test 4
def test_error_precedence_and_truncation(engine):
    items = cases.error_frames()
    frames = [c["frame"] for c in items]
    kinds = expected_kinds(engine, items)
    assert (kinds < 0).sum() > 500 and {-10, -11, -12} <= set(kinds.tolist())
    for kind in (CERTIFICATE, HEADER, VOTE):
        check_decode(engine, kind, items, device_decode(engine, kind, frames, own=kind == HEADER))


# ---------------------------------------------------------------- test 5
def test_mixed_kinds_and_capacity(engine):
    import torch

    items = cases.mixed_frames()
    frames = [c["frame"] for c in items]
    want = expected_kinds(engine, items)
    assert {0, 1, 2, 3, engine.WIRE_ECAPACITY} <= set(want.tolist()) and (want < -13).sum() == 0
    assert want.tolist().count(engine.WIRE_ECAPACITY) == 2
    # the scan alone: kinds, digest-input lengths and vote counts as the host's
    blob = b"".join(frames)
    offs = np.zeros(len(frames) + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    kinds = torch.full((len(frames),), 0x5a, dtype=torch.int32, device="cuda:0")
    hb = torch.full((len(frames),), 0x5a, dtype=torch.int64, device="cuda:0")
    nv = torch.full((len(frames),), 0x5a, dtype=torch.int64, device="cuda:0")
    engine.wire_scan_device(0, _dev(np.frombuffer(blob + b"\xee" * SLACK, np.uint8)), _dev(offs), kinds, hb, nv,
                            frame_bytes=len(blob))
    torch.cuda.synchronize()
    _, hhb, hnv = engine.wire_scan(frames)
    over = want == engine.WIRE_ECAPACITY
    assert _np(kinds).tolist() == want.tolist()
    assert _np(hb).tolist() == np.where(over, 0, hhb).tolist() and _np(nv).tolist() == np.where(over, 0, hnv).tolist()
    kinds2 = torch.full((len(frames),), 0x5a, dtype=torch.int32, device="cuda:0")  # without the optional arrays
    engine.wire_scan_device(0, _dev(np.frombuffer(blob + b"\xee" * SLACK, np.uint8)), _dev(offs), kinds2,
                            frame_bytes=len(blob))
    torch.cuda.synchronize()
    assert _np(kinds2).tolist() == want.tolist()
    for kind in (HEADER, VOTE, CERTIFICATE):
        check_decode(engine, kind, items, device_decode(engine, kind, frames))


# ---------------------------------------------------------------- test 6
@pytest.fixture(scope="module")
def registered(engine):
    engine.committee_register_authorities(*vc.committee().arrays())
    yield engine
    engine.committee_register(np.zeros((0, 32), np.uint8))


def _splice(frames):
    """Two undecodable frames and one frame of another kind among `frames`:
    (batch, index of each original frame in it)."""
    other = cases.make_vote(__import__("random").Random(4))["frame"]
    if frames and frames[0][:4] == b"\x01\x00\x00\x00":
        other = cases.small_certificates(1)[0]["frame"]
    extra = {3: frames[0][:len(frames[0]) // 2], 10: other, len(frames) + 2: b"\x09\x00\x00\x00rubbish"}
    batch, at = [], []
    it = iter(frames)
    for i in range(len(frames) + 3):
        if i in extra:
            batch.append(extra[i])
        else:
            at.append(i)
            batch.append(next(it))
    return batch, at, sorted(extra)


def _diff(names, got, want):
    return [(n, hex(int(g)), hex(int(w))) for n, g, w in zip(names, got, want) if g != w]


def test_certificate_frames_to_verdicts(registered):
    e = registered
    cs = vc.certificate_cases()
    frames = []
    for c in cs:
        f, hdr, count = cases.verdict_frame(2, c["hdr"], c["count"], c["origin"], c["id"], c["hsig"], c["votes"])
        assert hdr == c["hdr"] and count == c["count"]  # the case table's expectation holds for the frame
        frames.append(f)
    batch, at, extra = _splice(frames)
    want, _ = vc.expected_certificates()
    for seed in (11, 0):  # these cases are weight-independent by construction
        kinds, words = e.wire_certificate_verdict_many(batch, rng_seed=seed)
        assert not _diff([c["name"] for c in cs], words[at], want)
        assert (kinds[at] == CERTIFICATE).all()
        assert (words[extra] == e.DAG_NO_MESSAGE).all() and (kinds[extra] != CERTIFICATE).all()
        assert kinds[extra].tolist() == e.wire_scan([batch[i] for i in extra])[0].tolist()
        assert not ((words & 0xff) == e.DAG_VOTES_OPEN).any()


def test_weight_dependent_certificates_follow_the_oracle(registered):
    """Where a word rests on the weights: the device decode, the verdict call
    and the resolution with explicit weights, against the oracle under the
    same weights (the cases of tests/test_gpu_votes_resolve.py)."""
    import torch

    import coa_oracle as co
    from test_gpu_votes_resolve import weight_cases

    e = registered
    cs = weight_cases()
    frames = [cases.verdict_frame(2, c["hdr"], c["count"], c["origin"], c["id"], c["hsig"], c["votes"])[0] for c in cs]
    got = device_decode(e, CERTIFICATE, frames)
    assert (got["kinds"] == CERTIFICATE).all()
    t = got["tensors"]
    nv = int(got["totals"][1])
    assert nv == sum(len(c["votes"]) for c in cs)
    words = torch.full((len(cs),), -1, dtype=torch.int32, device="cuda:0")
    e.certificate_verdict_many_device(0, t["hdata"], t["hoff"], t["ids"], t["authors"], t["sigs"], t["rounds"],
                                      t["vpks"][:nv], t["vsigs"][:nv], t["voff"], t["pcounts"], words)
    torch.cuda.synchronize()
    before = _np(words).view(np.uint32).copy()
    assert (before[:4] == vc.OPEN).all()
    host = vc.certificate_arrays(cs)
    gen = np.random.default_rng(5)
    seen = set()
    for _ in range(6):
        zs = gen.integers(0, 256, (nv, 16), dtype=np.uint8)
        bits = np.asarray(co.certificate_verify_many(*host[:8], zs))
        want = np.where(bits & 4, vc.BAD_VOTES, vc.OK).astype(np.uint32)
        out = words.clone()
        e.certificate_votes_resolve_device(0, t["ids"], t["authors"], t["rounds"], t["vpks"][:nv], t["vsigs"][:nv],
                                           t["voff"], out, zs=_dev(zs))
        torch.cuda.synchronize()
        after = _np(out).view(np.uint32)
        assert not _diff([c["name"] for c in cs], after, want)
        seen |= set(want[:4].tolist())
    assert seen == {vc.OK, vc.BAD_VOTES}  # the weights decided both ways


@functools.lru_cache(maxsize=None)
def wire_header_cases():
    """(frames, names, expected words) for vc.header_cases() as frames."""
    import message_cases as mc

    c = vc.committee()
    frames, carried = [], []
    for h in vc.header_cases():
        f, hdr, count = cases.verdict_frame(0, h["hdr"], h["count"], h["author"], h["id"], h["sig"])
        frames.append(f)
        carried.append(dict(h, hdr=hdr, count=count))
    bits = mc.expected_headers(carried)
    want = np.array([vc._header_word(c, h["hdr"], h["count"], h["author"], bits[i] & 1, bits[i] & 2)
                     for i, h in enumerate(carried)], np.uint32)
    same = [i for i, (h, g) in enumerate(zip(vc.header_cases(), carried)) if h["hdr"] == g["hdr"]]
    assert len(same) >= 16 and (want[same] == vc.expected_headers()[same]).all()
    assert {vc.OK, vc.BAD_ID, vc.UNKNOWN_AUTHOR, vc.MALFORMED, vc.BAD_SIG} <= set(want.tolist())
    return frames, [h["name"] for h in carried], want


def test_header_and_vote_frames_to_verdicts(registered):
    e = registered
    frames, names, want = wire_header_cases()
    batch, at, extra = _splice(frames)
    kinds, words = e.wire_header_verdict_many(batch)
    assert not _diff(names, words[at], want)
    assert (kinds[at] == HEADER).all() and (words[extra] == e.DAG_NO_MESSAGE).all()
    assert kinds[extra].tolist() == e.wire_scan([batch[i] for i in extra])[0].tolist()

    vs = vc.vote_cases()
    frames = [W.primary_message(1, W.vote(v["id"], v["round"], v["origin"], v["author"], v["sig"])) for v in vs]
    batch, at, extra = _splice(frames)
    kinds, words = e.wire_vote_verdict_many(batch)
    assert not _diff([v["name"] for v in vs], words[at], vc.expected_votes())
    assert (kinds[at] == VOTE).all() and (words[extra] == e.DAG_NO_MESSAGE).all()
    assert kinds[extra].tolist() == e.wire_scan([batch[i] for i in extra])[0].tolist()


def test_fused_calls_need_a_protocol_table(engine):
    engine.committee_register(np.zeros((0, 32), np.uint8))
    f = cases.small_certificates(2)
    with pytest.raises(engine.EngineError, match="COA_EINVAL"):
        engine.wire_certificate_verdict_many([c["frame"] for c in f])


# ---------------------------------------------------------------- test 7
def test_c3_shape(engine):
    import certificates as C

    committee, batch = C.synth_certificates(16, committee_size=100, n_payload=32, seed=8)
    committee.register_authorities()
    try:
        frames = []
        for i in range(len(batch)):
            hi_ = batch.header_inputs[i]
            _, pay, par = cases.digest_input_fields(hi_, 32)
            assert len(par) == 67
            lo, hi = int(batch.offsets[i]), int(batch.offsets[i + 1])
            votes = [(bytes(batch.vote_pks[j]), bytes(batch.vote_sigs[j])) for j in range(lo, hi)]
            hb = W.header(bytes(batch.authors[i]), batch.round, pay[::-1], par[::-1], bytes(batch.ids[i]),
                          bytes(batch.header_sigs[i]))  # wire order reversed: the decoder re-sorts
            frames.append(W.primary_message(2, W.certificate(hb, votes)))
        frames[3] = frames[3][:-40] + bytes([frames[3][-40] ^ 1]) + frames[3][-39:]  # corrupt the last vote's R
        items = [dict(frame=f, kind=2) for f in frames]
        got = device_decode(engine, CERTIFICATE, frames)
        check_decode(engine, CERTIFICATE, items, got)  # the host decoder, byte for byte
        assert [bytes(got["hdata"][int(got["hoff"][i]):int(got["hoff"][i + 1])]) for i in range(16)] == batch.header_inputs
        d = engine.wire_decode_certificates(frames)
        want = engine.certificate_verdict_many(d["header_inputs"], d["ids"], d["origins"], d["header_sigs"], d["rounds"],
                                               d["vote_pks"], d["vote_sigs"], d["vote_offsets"], d["payload_counts"],
                                               rng_seed=2)
        kinds, words = engine.wire_certificate_verdict_many(frames, rng_seed=2)
        assert (kinds == CERTIFICATE).all() and words.tolist() == want.tolist()
        assert np.flatnonzero(words).tolist() == [3] and words[3] == engine.DAG_INVALID_VOTES
        assert hashlib.sha512(batch.header_inputs[0]).digest()[:32] == bytes(batch.ids[0])
    finally:
        engine.committee_register(np.zeros((0, 32), np.uint8))

"""GPU: the mixed mode of the device wire decoder -- one batch of interleaved
frames partitioned by kind on the device (coa_wire_decode_mixed_device) and
carried to one verdict word per frame (coa_wire_verdict_many).

The contract under test: for each kind, the compacted arrays and the words are
exactly what the single-kind entry gives on the batch's frames of that kind
alone, in order.  Expected kinds, sums and fields come from the host scanner
and the host decoders (coa_wire.cpp) over each kind's frames, expected slots
and offsets from NumPy cumulative sums of the host scan, expected words from
tests/verdict_cases.py, the existing single-kind fused calls and the engine's
CPU path.  Nothing expected comes from the kernels under test.  What the
batches must hold for these tests to mean anything is asserted without a GPU
in tests/test_wire_mixed_host.py.

Every output is prefilled with 0xA5, so an entry the call must not touch is
told from one it wrote."""
import numpy as np
import pytest

import verdict_cases as vc
import wire_codec as W
import wire_dev_cases as cases
import wire_mixed_cases as mixed
from wire_mixed_cases import CERT_REQUEST, CERTIFICATE, ECAPACITY, ETRUNC, HEADER, NO_SLOT, VOTE

pytestmark = pytest.mark.gpu

SLACK = 4096
GUARD = 256
FILL = 0xa5
KINDS = (HEADER, VOTE, CERTIFICATE)


def _dev(x):
    import torch

    x = np.array(x)
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def mixed_decode(e, frames, own=False, guard=False):
    """One coa_wire_decode_mixed_device call over `frames`; every output as
    numpy.  The frames lie in a buffer with SLACK bytes of 0xee behind them and
    frame_bytes is their true size.  own: a caller workspace on a side stream.
    guard: every output at exactly its stated capacity (n per-item entries,
    n + 1 offsets, frame_bytes + 16 header bytes, wire_votes_bound rows) and a
    caller workspace of exactly wire_mixed_workspace_bytes, each between GUARD
    pattern bytes; out["bands"] names every array whose bands changed."""
    import torch

    dev = torch.device("cuda", 0)
    blob = b"".join(frames)
    fb, n = len(blob), len(frames)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum([len(f) for f in frames])
    d_frames = _dev(np.frombuffer(blob + b"\xee" * SLACK, np.uint8))
    d_offs = _dev(offs)
    raw = {}

    def fill(name, count, dt, exact=None):
        if guard and exact is not None:
            count = exact
        size = torch.empty((), dtype=dt).element_size()
        lo = GUARD if guard else 0
        buf = torch.full((lo + count * size + lo,), FILL, dtype=torch.uint8, device=dev)
        raw[name] = (buf, lo, count * size)
        return buf[lo:lo + count * size].view(dt)

    nvb = e.wire_votes_bound(fb)
    shapes = dict(hdata=(fb + 16 + SLACK, torch.uint8, fb + 16), hoff=(n + 1, torch.int64, None), ids=(n * 32, torch.uint8, None),
                  authors=(n * 32, torch.uint8, None), origins=(n * 32, torch.uint8, None), sigs=(n * 64, torch.uint8, None),
                  hsigs=(n * 64, torch.uint8, None), pcounts=(n, torch.int32, None), rounds=(n, torch.int64, None),
                  vpks=((nvb + 8) * 32, torch.uint8, nvb * 32), vsigs=((nvb + 8) * 64, torch.uint8, nvb * 64),
                  voff=(n + 1, torch.int64, None))
    sets = {k: {name: fill(f"{k}.{name}", *shapes[name]) for name in e.WIRE_MIXED_SET_NAMES[k]} for k in KINDS}
    kinds = fill("kinds", n, torch.int32)
    slots = fill("slots", n, torch.int32)
    totals = fill("totals", 8, torch.int64)
    kw = {}
    side = None
    if own or guard:
        ws = fill("workspace", e.wire_mixed_workspace_bytes(n, fb), torch.uint8)
        if guard:
            assert ws.data_ptr() % 256 == 0
        side = torch.cuda.Stream(device=0)
        side.wait_stream(torch.cuda.current_stream(0))
        kw = dict(stream=side, workspace=ws)
    e.wire_decode_mixed_device(0, d_frames, d_offs, sets[HEADER], sets[VOTE], sets[CERTIFICATE], kinds, slots, totals,
                               frame_bytes=fb, **kw)
    if side is not None:
        side.synchronize()
    torch.cuda.synchronize()
    out = dict(kinds=kinds.cpu().numpy(), slots=slots.cpu().numpy().view(np.uint32),
               totals=totals.cpu().numpy().tolist(), frame_bytes=fb, n=n,
               sets={k: {name: t.cpu().numpy() for name, t in s.items()} for k, s in sets.items()})
    out["bands"] = [k for k, (buf, lo, nbytes) in raw.items()
                    if not (bool((buf[:lo] == FILL).all()) and bool((buf[lo + nbytes:] == FILL).all()))]
    return out


def _untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


def check_sums(e, frames, got):
    """Kinds, slots, totals and each kind's offsets on [0, n_k] against the
    host scan and NumPy cumulative sums; nothing written above."""
    dk, hb, nv = mixed.device_kinds(e, frames)
    assert (got["kinds"] == dk).all()
    assert (got["slots"] == mixed.expected_slots(dk)).all()
    assert got["totals"] == mixed.expected_totals(dk, hb, nv)
    for kind, name, q in ((HEADER, "hoff", hb), (CERTIFICATE, "hoff", hb), (CERTIFICATE, "voff", nv)):
        want = np.concatenate([[0], np.cumsum(q[dk == kind].astype(np.int64))])
        off = got["sets"][kind][name]
        assert (off[:len(want)] == want).all(), (kind, name)
        assert _untouched(off[len(want):]), (kind, name)
    return dk, hb, nv


def check_mixed(e, frames, got):
    """The whole contract: check_sums, then per kind items [0, n_k) against
    the host decoder over that kind's frames in order, byte for byte, and the
    fill pattern at and above n_k and beyond the summed bytes and rows."""
    dk, hb, nv = check_sums(e, frames, got)
    for kind in KINDS:
        sub = [f for f, k in zip(frames, dk) if k == kind]
        m = len(sub)
        s = got["sets"][kind]
        if kind == VOTE:
            h = e.wire_decode_votes(sub)
            pairs = [("ids", h["ids"], 32), ("origins", h["origins"], 32), ("authors", h["authors"], 32), ("sigs", h["sigs"], 64)]
        elif kind == HEADER:
            h = e.wire_decode_headers(sub)
            pairs = [("ids", h["ids"], 32), ("authors", h["authors"], 32), ("sigs", h["sigs"], 64)]
        else:
            h = e.wire_decode_certificates(sub)
            pairs = [("ids", h["ids"], 32), ("origins", h["origins"], 32), ("hsigs", h["header_sigs"], 64)]
        for name, want, width in pairs:
            assert s[name][:m * width].tobytes() == np.asarray(want)[:m].tobytes(), (kind, name)
            assert _untouched(s[name][m * width:]), (kind, name)
        assert (s["rounds"][:m].view(np.uint64) == h["rounds"][:m]).all() and _untouched(s["rounds"][m:]), kind
        if kind == VOTE:
            continue
        assert (s["pcounts"][:m].view(np.uint32) == h["payload_counts"][:m]).all() and _untouched(s["pcounts"][m:]), kind
        data = b"".join(h["header_inputs"])
        assert len(data) == int(s["hoff"][m]) and s["hdata"][:len(data)].tobytes() == data, kind
        assert _untouched(s["hdata"][len(data):]), kind
        if kind == CERTIFICATE:
            rows = int(s["voff"][m])
            assert (s["voff"][:m + 1].view(np.uint64) == h["vote_offsets"][:m + 1]).all()
            assert rows == len(h["vote_pks"]) or m == 0
            assert s["vpks"][:rows * 32].tobytes() == h["vote_pks"][:rows].tobytes()
            assert s["vsigs"][:rows * 64].tobytes() == h["vote_sigs"][:rows].tobytes()
            assert _untouched(s["vpks"][rows * 32:]) and _untouched(s["vsigs"][rows * 64:])
    return dk


# ---------------------------------------------------------------- test 1
@pytest.mark.parametrize("own", [False, True], ids=["engine_workspace", "caller_workspace_side_stream"])
def test_equals_the_single_kind_decoders_compacted(engine, own):
    items = cases.mixed_frames()
    frames = [c["frame"] for c in items]
    dk = check_mixed(engine, frames, mixed_decode(engine, frames, own=own))
    assert {HEADER, VOTE, CERTIFICATE, CERT_REQUEST, ETRUNC, ECAPACITY} <= set(dk.tolist())
    assert [c["kind"] for c in items if c.get("kind") is not None] == [int(k) for c, k in zip(items, dk) if c.get("kind") is not None]


# ---------------------------------------------------------------- test 2
@pytest.mark.parametrize("last", mixed.LASTS, ids=["last_header", "last_vote", "last_certificate", "last_error"])
@pytest.mark.parametrize("n", mixed.SUM_SIZES)
def test_sum_boundaries(engine, n, last):
    """One block, one frame more and less; three blocks; 256 and 257 blocks,
    where a thread of the totals kernel sums two block totals.  Frames 255 /
    256 / 257 of three kinds, a block wholly of certificates, a block without
    a vote, the last frame each kind and an error (tests/test_wire_mixed_host.py
    asserts the arrangement)."""
    pool = [c["frame"] for c in cases.prefix_pool()]
    idx = mixed.sum_indices(n, last)
    frames = [pool[i] for i in idx]
    got = mixed_decode(engine, frames, own=n == 513)
    dk, _, _ = check_sums(engine, frames, got)
    # each item's id is its frame's: the decode followed the slots
    pk = engine.wire_scan(pool)[0]
    for kind in KINDS:
        ids = np.zeros((16, 32), np.uint8)
        for i in np.flatnonzero(pk == kind):
            one = [pool[i]]
            ids[i] = (engine.wire_decode_votes(one) if kind == VOTE else engine.wire_decode_headers(one) if kind == HEADER
                      else engine.wire_decode_certificates(one))["ids"][0]
        mine = idx[dk == kind]
        assert (got["sets"][kind]["ids"][:len(mine) * 32].reshape(-1, 32) == ids[mine]).all(), kind
        assert _untouched(got["sets"][kind]["ids"][len(mine) * 32:]), kind


# ---------------------------------------------------------------- test 3
def test_work_split_and_extents(engine):
    """LDS-staged and flat frames of different kinds beside each other; every
    output at exactly its stated capacity and the workspace at exactly
    wire_mixed_workspace_bytes between guard bands; nothing at or above n_k,
    beyond the summed header bytes or beyond the summed vote rows."""
    frames = [c["frame"] for c in mixed.work_split_items()]
    got = mixed_decode(engine, frames, guard=True)
    assert got["bands"] == []
    fb = got["frame_bytes"]
    for kind in (HEADER, CERTIFICATE):
        assert len(got["sets"][kind]["hdata"]) == fb + 16
    c = got["sets"][CERTIFICATE]
    assert len(c["vpks"]) == 32 * engine.wire_votes_bound(fb) and len(c["vsigs"]) == 64 * engine.wire_votes_bound(fb)
    check_mixed(engine, frames, got)
    # the same batch with the engine's workspace gives the same bytes
    again = mixed_decode(engine, frames)
    for kind in KINDS:
        for name, a in got["sets"][kind].items():
            b = again["sets"][kind][name]
            m = min(len(a), len(b))
            assert (a[:m] == b[:m]).all(), (kind, name)


# ---------------------------------------------------------------- test 4
def test_differential(engine):
    """4,000 seeded mutations of the fuzz corpus and the constructed frames,
    with every kind and every code among them, in one batch."""
    frames = [c["frame"] for c in mixed.differential_items()]
    dk = check_mixed(engine, frames, mixed_decode(engine, frames, own=True))
    assert {HEADER, VOTE, CERTIFICATE, CERT_REQUEST, -10, -11, -12, -13} <= set(dk.tolist())


# ---------------------------------------------------------------- test 5
@pytest.fixture(scope="module")
def registered(engine):
    engine.committee_register_authorities(*vc.committee().arrays())
    yield engine
    engine.committee_register(np.zeros((0, 32), np.uint8))


def _diff(names, got, want):
    return [(n, hex(int(g)), hex(int(w))) for n, g, w in zip(names, got, want) if g != w]


def single_kind_route(e, frames, seed):
    """(kinds, words) by the three existing fused calls, merged by kind."""
    words = np.full(len(frames), e.DAG_NO_MESSAGE, np.uint32)
    kinds = None
    for kind, call in ((HEADER, lambda: e.wire_header_verdict_many(frames)), (VOTE, lambda: e.wire_vote_verdict_many(frames)),
                       (CERTIFICATE, lambda: e.wire_certificate_verdict_many(frames, rng_seed=seed))):
        k, w = call()
        assert kinds is None or (k == kinds).all()
        kinds = k
        words[k == kind] = w[k == kind]
    return kinds, words


@pytest.mark.parametrize("seed", [0, 11])
def test_frames_to_verdicts(registered, seed):
    e = registered
    frames, names, _, want = mixed.verdict_batch()
    kinds, words = e.wire_verdict_many(frames, rng_seed=seed)
    assert not _diff(names, words, want)
    assert kinds.tolist() == e.wire_scan(frames)[0].tolist()
    k3, w3 = single_kind_route(e, frames, seed)
    assert kinds.tolist() == k3.tolist() and not _diff(names, words, w3)  # the compaction changed no verdict
    assert not ((words & 0xff) == e.DAG_VOTES_OPEN).any()
    pks, stakes, workers = vc.committee().arrays()
    ck, cw = e.cpu_wire_verdict_many(frames, (pks, stakes, workers), rng_seed=seed)
    assert kinds.tolist() == ck.tolist() and not _diff(names, words, cw)
    # and the reversed batch gives the reversed answer
    rk, rw = e.wire_verdict_many(frames[::-1], rng_seed=seed)
    assert rk.tolist() == kinds.tolist()[::-1] and rw.tolist() == words.tolist()[::-1]


# ---------------------------------------------------------------- test 6
def test_degenerate_batches(registered):
    e = registered
    frames, names, kinds_of, want = mixed.verdict_batch()
    by_kind = {k: [i for i, x in enumerate(kinds_of) if x == k] for k in (HEADER, VOTE, CERTIFICATE, CERT_REQUEST)}
    request = frames[by_kind[CERT_REQUEST][0]]

    def run(idx_or_frames):
        fs = [frames[i] if isinstance(i, int) else i for i in idx_or_frames]
        w = np.array([want[i] if isinstance(i, int) else e.DAG_NO_MESSAGE for i in idx_or_frames], np.uint32)
        kinds, words = e.wire_verdict_many(fs, rng_seed=11)
        assert kinds.tolist() == e.wire_scan(fs)[0].tolist()
        assert words.tolist() == w.tolist()
        return kinds, words

    # only votes
    kinds, words = run(by_kind[VOTE])
    assert (kinds == VOTE).all() and len(set(words.tolist())) >= 2
    # only certificate requests and rubbish: no message, every word DAG_NO_MESSAGE
    kinds, words = run([request, b"\x09\x00\x00\x00rubbish", request, b"\x04\x00\x00\x00", request])
    assert kinds.tolist() == [3, -11, 3, -11, 3] and (words == e.DAG_NO_MESSAGE).all()
    # exactly one frame of each kind
    kinds, _ = run([by_kind[CERTIFICATE][1], request, by_kind[VOTE][1], by_kind[HEADER][1]])
    assert kinds.tolist() == [CERTIFICATE, CERT_REQUEST, VOTE, HEADER]
    # five empty frames: n > 0 with no frame bytes at all
    kinds, words = run([b""] * 5)
    assert kinds.tolist() == [ETRUNC] * 5
    # the only certificate is the last frame
    bad = next(i for i in by_kind[CERTIFICATE] if want[i] != 0)
    kinds, words = run(by_kind[VOTE][:7] + by_kind[HEADER][:7] + [request, bad])
    assert (kinds == CERTIFICATE).sum() == 1 and kinds[-1] == CERTIFICATE and words[-1] == want[bad]


def test_fused_call_needs_a_protocol_table(engine):
    engine.committee_register(np.zeros((0, 32), np.uint8))
    frames = mixed.verdict_batch()[0]
    with pytest.raises(engine.EngineError, match="COA_EINVAL"):
        engine.wire_verdict_many(frames[:12])
    with pytest.raises(engine.EngineError, match="COA_EINVAL"):
        engine.wire_verdict_many([b"\x09\x00\x00\x00rubbish"])  # as the single-kind fused calls: also without a message


# ---------------------------------------------------------------- test 7
def test_c3_shape_small(engine):
    """16 committee-100 certificates (67 votes, 67 parents, 32 payload
    entries), one with a corrupted vote, interleaved with their headers and
    with votes for them."""
    import certificates as C

    committee, batch = C.synth_certificates(16, committee_size=100, n_payload=32, seed=8)
    committee.register_authorities()
    try:
        certs, headers, votes = [], [], []
        for i in range(len(batch)):
            hi_ = batch.header_inputs[i]
            _, pay, par = cases.digest_input_fields(hi_, 32)
            assert len(par) == 67
            lo, hi = int(batch.offsets[i]), int(batch.offsets[i + 1])
            vs = [(bytes(batch.vote_pks[j]), bytes(batch.vote_sigs[j])) for j in range(lo, hi)]
            hb = W.header(bytes(batch.authors[i]), batch.round, pay[::-1], par[::-1], bytes(batch.ids[i]),
                          bytes(batch.header_sigs[i]))
            certs.append(W.primary_message(2, W.certificate(hb, vs)))
            headers.append(W.primary_message(0, hb))
            votes.append(W.primary_message(1, W.vote(bytes(batch.ids[i]), batch.round, bytes(batch.authors[i]), vs[0][0],
                                                     vs[0][1])))
        certs[3] = certs[3][:-40] + bytes([certs[3][-40] ^ 1]) + certs[3][-39:]  # corrupt the last vote's R
        frames = [f for trio in zip(headers, certs, votes) for f in trio]
        kinds, words = engine.wire_verdict_many(frames, rng_seed=2)
        assert kinds.tolist() == [HEADER, CERTIFICATE, VOTE] * 16
        _, cw = engine.wire_certificate_verdict_many(certs, rng_seed=2)
        assert words[1::3].tolist() == cw.tolist()
        assert np.flatnonzero(words[1::3]).tolist() == [3] and words[1 + 3 * 3] == engine.DAG_INVALID_VOTES
        assert words[0::3].tolist() == engine.wire_header_verdict_many(headers)[1].tolist() and not words[0::3].any()
        assert words[2::3].tolist() == engine.wire_vote_verdict_many(votes)[1].tolist()
    finally:
        engine.committee_register(np.zeros((0, 32), np.uint8))

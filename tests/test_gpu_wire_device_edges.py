"""GPU: the device wire decoder's work split at its own boundaries.

tests/test_gpu_wire_device.py reaches the kernels of coa_wire_dev.hip through
frames built to exercise the grammar.  These tests aim at what the kernels add
to the grammar: the LDS staging copy at every alignment and at the staging
switch (A), the three prefix-sum launches with several block totals per
thread (B), the wave-wide error reduction over more than one round of lanes
(C), the lane-strided sort on the payload stride and at the cap (D), the
extents of every output (E), the offsets rule (F), a seeded batch of mutated
frames (G) and the fused calls' reused buffers (H).

Everything is compared bit for bit.  Expected fields come from the host decoder
coa_wire.cpp (the same rules of coa_wire_parse.h run one after the other, so a
difference is one of the work split; the rules themselves are pinned against
an independent model in tests/test_wire_parse_host.py) and the independent
encoder tests/wire_codec.py (check_decode of
tests/test_gpu_wire_device.py); expected verdict words from the host route
wire_scan + wire_decode_* + *_verdict_many.  Nothing expected comes from the
kernels under test.  What these inputs must be for the tests to mean anything
is asserted without a GPU in tests/test_wire_dev_cases_host.py."""
import functools
import glob
import os

import numpy as np
import pytest

from conftest import ROOT

import verdict_cases as vc
import wire_codec as W
import wire_dev_cases as cases
from test_gpu_wire_device import (CERTIFICATE, HEADER, VOTE, check_decode, device_decode, expected_kinds,
                                  registered, wire_header_cases)  # noqa: F401  (registered: a fixture)

pytestmark = pytest.mark.gpu

KINDS = (HEADER, VOTE, CERTIFICATE)
PATTERN = 0x5a  # device_decode's fill


def _frames(items):
    return [c["frame"] for c in items]


def check_extents(kind, got):
    """Beyond what the call's sums say it used, every output still holds the
    fill pattern; arrays the call does not take are untouched."""
    n = len(got["kinds"])
    if kind == VOTE:
        untouched = ("hdata", "hoff", "voff", "pcounts", "vpks", "vsigs")
    else:
        untouched = ("origins",) + (() if kind == CERTIFICATE else ("vpks", "vsigs", "voff"))
        assert (got["hdata"][int(got["hoff"][n]):] == PATTERN).all()
    if kind == CERTIFICATE:
        assert (got["vpks"][int(got["voff"][n]):] == PATTERN).all() and (got["vsigs"][int(got["voff"][n]):] == PATTERN).all()
    for name in untouched:
        a = got[name]  # typed arrays are filled by value, or by byte when carved out of a guarded allocation
        assert (a == PATTERN).all() or (a.view(np.uint8) == PATTERN).all(), name


# ---------------------------------------------------------------- group A
@functools.lru_cache(maxsize=None)
def alignment_batch():
    return cases.at_every_alignment(cases.alignment_frames() + cases.stage_switch_frames())


@pytest.mark.parametrize("frames_shift", [0, 1, 2, 3])
def test_every_alignment_and_the_staging_switch(engine, frames_shift):
    """Every frame under test 0-3 bytes past a dword boundary, the buffer
    itself 0-3 bytes into its allocation: the head, dword and tail parts of
    stage_frame at every split, frames shorter than the head, frames whose
    staged copy ends at the end of the stage, and the same frames one to four
    bytes longer, read in place."""
    batch, at, mis = alignment_batch()
    frames = _frames(batch)
    want = expected_kinds(engine, batch)
    assert (want[at] >= 0).sum() >= 4 * (4 + 16)
    for kind in KINDS:
        check_decode(engine, kind, batch, device_decode(engine, kind, frames, frames_shift=frames_shift, own=kind == VOTE))


def unaligned_outputs_batch():
    return (cases.mixed_frames() + cases.alignment_frames()[:4] + cases.stage_switch_frames()[-6:] +
            cases.vote_reduction_frames()[-4:])


@pytest.mark.parametrize("kind", KINDS)
def test_unaligned_byte_outputs(engine, kind):
    """include/coa_verify.h states no alignment for the byte arrays: passed 1,
    2 and 3 bytes into their allocations they hold the aligned run's bytes
    (coa_wp_put32's byte path; the dword signature copy to an odd address)."""
    items = unaligned_outputs_batch()
    frames = _frames(items)
    aligned = device_decode(engine, kind, frames)
    check_decode(engine, kind, items, aligned)
    for shift in (1, 2, 3):
        got = device_decode(engine, kind, frames, shift=shift)
        assert got["tensors"]["ids"].data_ptr() % 4 == shift and got["tensors"]["rounds"].data_ptr() % 8 == 0
        assert got["bands"] == []
        for name in ("kinds", "totals", "rounds", "ids", "authors", "sigs") + \
                (("origins",) if kind == VOTE else ("hoff", "pcounts")) + (("voff",) if kind == CERTIFICATE else ()):
            assert (got[name] == aligned[name]).all(), (shift, name)
        if kind != VOTE:
            used = int(aligned["hoff"][-1])
            assert used > 0 and got["hdata"][:used].tobytes() == aligned["hdata"][:used].tobytes(), shift
        if kind == CERTIFICATE:
            used = int(aligned["voff"][-1])
            assert used > 130 and got["vpks"][:used].tobytes() == aligned["vpks"][:used].tobytes(), shift
            assert got["vsigs"][:used].tobytes() == aligned["vsigs"][:used].tobytes(), shift
        check_decode(engine, kind, items, got)
        check_extents(kind, got)


# ---------------------------------------------------------------- group B
@functools.lru_cache(maxsize=None)
def pool_reference(e, kind):
    """The host decoder's answer for each pool frame as arrays indexed by pool
    position (zero where the frame is not of `kind`, as the placeholder)."""
    pool = cases.prefix_pool()
    frames = _frames(pool)
    hk = expected_kinds(e, pool)
    r = dict(kinds=hk, mine=hk == kind, ids=np.zeros((16, 32), np.uint8), authors=np.zeros((16, 32), np.uint8),
             origins=np.zeros((16, 32), np.uint8), sigs=np.zeros((16, 64), np.uint8), rounds=np.zeros(16, np.uint64),
             pcounts=np.zeros(16, np.uint32), hlen=np.zeros(16, np.int64), hmat=np.zeros((16, 512), np.uint8),
             nv=np.zeros(16, np.int64), vp=np.zeros((16, 5, 32), np.uint8), vs=np.zeros((16, 5, 64), np.uint8))
    for i in np.flatnonzero(r["mine"]):
        one = [frames[i]]
        if kind == VOTE:
            h = e.wire_decode_votes(one)
            r["origins"][i] = h["origins"][0]
            auth, sigs = h["authors"], h["sigs"]
        else:
            h = e.wire_decode_headers(one) if kind == HEADER else e.wire_decode_certificates(one)
            auth, sigs = (h["authors"], h["sigs"]) if kind == HEADER else (h["origins"], h["header_sigs"])
            hi = h["header_inputs"][0]
            assert hi == W.header_digest_input(pool[i]["author"], pool[i]["round"], pool[i]["payload"], pool[i]["parents"])
            r["hlen"][i] = len(hi)
            r["hmat"][i, :len(hi)] = np.frombuffer(hi, np.uint8)
            r["pcounts"][i] = h["payload_counts"][0]
        if kind == CERTIFICATE:
            nv = len(h["vote_pks"])
            r["nv"][i] = nv
            r["vp"][i, :nv], r["vs"][i, :nv] = h["vote_pks"], h["vote_sigs"]
        r["ids"][i], r["authors"][i], r["sigs"][i], r["rounds"][i] = h["ids"][0], auth[0], sigs[0], h["rounds"][0]
    return r


def check_gathered(e, kind, idx, got):
    """One decode of the pool frames idx[0..n) against the host's per-frame
    answers gathered by index: no Python loop over the frames."""
    r = pool_reference(e, kind)
    n = len(idx)
    mine = r["mine"][idx]
    assert (got["kinds"] == r["kinds"][idx]).all()
    for name in ("ids", "authors", "sigs", "rounds") + (("origins",) if kind == VOTE else ("pcounts",)):
        assert (got[name] == r[name][idx]).all(), name
    hb = nv = 0
    if kind != VOTE:
        hoff = np.concatenate([[0], np.cumsum(r["hlen"][idx])]).astype(np.uint64)
        assert (got["hoff"] == hoff).all()
        hb = int(hoff[n])
        want = r["hmat"][idx][np.arange(512)[None, :] < r["hlen"][idx][:, None]]
        assert len(want) == hb and (got["hdata"][:hb] == want).all()
    if kind == CERTIFICATE:
        voff = np.concatenate([[0], np.cumsum(r["nv"][idx])]).astype(np.uint64)
        assert (got["voff"] == voff).all()
        nv = int(voff[n])
        rows = np.arange(5)[None, :] < r["nv"][idx][:, None]
        assert (got["vpks"][:nv] == r["vp"][idx][rows]).all() and (got["vsigs"][:nv] == r["vs"][idx][rows]).all()
    assert got["totals"].tolist() == [hb, nv, int(mine.sum()), n - int(mine.sum())]
    check_extents(kind, got)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", cases.PREFIX_SIZES[:3])
def test_prefix_sums_around_one_block(engine, n, kind):
    pool = _frames(cases.prefix_pool())
    idx = cases.prefix_indices(n, kind)
    check_gathered(engine, kind, idx, device_decode(engine, kind, [pool[i] for i in idx]))


@pytest.mark.parametrize("kind", [CERTIFICATE, HEADER])
@pytest.mark.parametrize("n", cases.PREFIX_SIZES[3:])
def test_prefix_sums_with_several_block_totals_per_thread(engine, n, kind):
    """65,537 frames: two block totals per thread of k_wire_scan_totals;
    131,329: three, the last thread's share ragged and idle threads behind it.
    In the largest batch the first three blocks hold no frame of the kind, one
    middle block nothing else, and the last frame is of the kind (hoff[n] and
    voff[n] come from the i == n - 1 store)."""
    pool = _frames(cases.prefix_pool())
    idx = cases.prefix_indices(n, kind)
    got = device_decode(engine, kind, [pool[i] for i in idx], own=kind == HEADER)
    check_gathered(engine, kind, idx, got)
    if n == cases.PREFIX_SIZES[-1]:
        assert int(got["hoff"][3 * cases.SCAN_BLOCK]) == 0 and int(got["hoff"][n]) > int(got["hoff"][n - 1])


# ---------------------------------------------------------------- group C
def test_vote_errors_across_rounds_of_lanes(engine):
    """130 votes: a lane checks votes k, k + 64 and k + 128.  Two defects of
    different codes in different rounds and in neighbouring lanes, in both
    orders; a cut in the last vote against an earlier key error; a
    43-character key first in a round (the walk); a vote count beyond what
    fits at the canonical stride.  The first defect in wire order decides."""
    items = cases.vote_reduction_frames()
    want = expected_kinds(engine, items)
    assert want.tolist() == [CERTIFICATE if c["code"] is None else c["code"] for c in items]
    assert {-10, -11, -12} <= set(want.tolist())
    for kind in (CERTIFICATE, HEADER):
        got = device_decode(engine, kind, _frames(items))
        assert got["kinds"].tolist() == want.tolist(), [c["note"] for c, g, w in zip(items, got["kinds"], want) if g != w]
        check_decode(engine, kind, items, got)
        check_extents(kind, got)


# ---------------------------------------------------------------- group D
def test_payload_sets_across_rounds_of_lanes_and_at_the_cap(engine):
    """The payload stride (36) at 63-129 entries and at the cap of 1,024, in
    three wire orders; a key repeated 1, 63, 64, 65 and 128 entries on; one key
    at entries 0, 64 and 128 (the last worker id wins); 1,024 wire entries
    with 512 and with 3 survivors; both sets at the cap."""
    items = cases.set_frames()
    assert (expected_kinds(engine, items) >= 0).all()  # at the cap: decodes, no COA_WIRE_ECAPACITY
    for kind in (HEADER, CERTIFICATE):
        got = device_decode(engine, kind, _frames(items), own=kind == CERTIFICATE)
        check_decode(engine, kind, items, got)  # header_digest_input of the fields each frame was built from
        check_extents(kind, got)
        for i, c in enumerate(items):
            if c["kind"] != kind:
                continue
            lo = int(got["hoff"][i])
            P = int(got["pcounts"][i])
            entries = bytes(got["hdata"][lo + 40:lo + 40 + 36 * P])
            if c.get("note") == "duplicates":
                d = c["payload"][0][0]
                assert P == 192 - 7 and entries.count(d) == 1
                assert entries[entries.index(d) + 32:][:4] == (7003).to_bytes(4, "little")
            elif c.get("note") == "512 of 1024":
                assert P == 512
            elif c.get("note") == "3 of 1024":
                assert int(got["hoff"][i + 1]) - lo == 40 + 36 * P + 32 * 3
            elif c.get("note") == "both at the cap":
                assert int(got["hoff"][i + 1]) - lo == 40 + (36 + 32) * cases.MAX_ENTRIES


# ---------------------------------------------------------------- group E
@pytest.mark.parametrize("batch", ["mixed", "alignment"])
def test_guard_bands_and_extents(engine, batch):
    """Every output at exactly its stated capacity and a caller workspace of
    exactly wire_workspace_bytes, each between 256 pattern bytes: the bands are
    unchanged and, inside the arrays, nothing beyond the sums is written."""
    items = cases.mixed_frames() if batch == "mixed" else alignment_batch()[0]
    for kind in KINDS:
        got = device_decode(engine, kind, _frames(items), guard=True)
        assert got["bands"] == []
        assert len(got["hdata"]) == got["frame_bytes"] + 16
        assert len(got["vpks"]) == len(got["vsigs"]) == engine.wire_votes_bound(got["frame_bytes"])
        check_decode(engine, kind, items, got)
        check_extents(kind, got)


def test_vote_arrays_at_the_bound(engine):
    """The certificate with the fewest bytes per vote, alone in its call: 200
    of the bound's 201 rows are used, the last keeps the pattern."""
    c = cases.tightest_certificate()
    got = device_decode(engine, CERTIFICATE, [c["frame"]], guard=True)
    assert got["bands"] == [] and len(got["vpks"]) == len(got["vsigs"]) == 201 and int(got["voff"][1]) == 200
    check_decode(engine, CERTIFICATE, [c], got)
    check_extents(CERTIFICATE, got)


# ---------------------------------------------------------------- group F
@pytest.mark.parametrize("kind", KINDS)
def test_offsets_rule_on_the_device(engine, kind):
    """coa_wp_frame_range: frames whose offsets decrease, end one byte behind
    frame_bytes or lie wholly behind it are COA_WIRE_ETRUNC placeholders that
    add nothing to the sums; the frames around them decode.  Every offset is
    inside the allocation and the bytes out of range would decode, so a kernel
    that ignored the rule gives a wrong answer, not a fault."""
    blob, slack, offsets, items = cases.offsets_case()
    got = device_decode(engine, kind, [blob], offsets=offsets, slack=slack, guard=kind == CERTIFICATE)
    assert got["frame_bytes"] == len(blob) and got["bands"] == []
    assert [k == cases.ETRUNC for k in got["kinds"].tolist()] == [c["frame"] == b"" for c in items]
    check_decode(engine, kind, items, got)
    check_extents(kind, got)


# ---------------------------------------------------------------- group G
def test_mutated_frames_differential(engine):
    """4,000 seeded mutations of the fuzz corpus and the constructed frames in
    one batch: the kernels choose the staged or in-place body, speculation or
    walk, and reduce errors over the wave on frames nobody constructed."""
    corpus = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "fuzz", "wire_corpus", "*.bin")))]
    assert len(corpus) >= 15
    items = cases.differential_frames(corpus)
    frames = _frames(items)
    hk = engine.wire_scan(frames)[0]
    # mutants of the frames over the cap: COA_WIRE_ECAPACITY where the host accepts them (by the cases' own parse)
    items = [dict(c, kind=engine.WIRE_ECAPACITY) if k in (HEADER, CERTIFICATE) and cases.over_the_cap(c["frame"]) else c
             for c, k in zip(items, hk)]
    assert 0 < sum(c["kind"] is not None for c in items) < 400
    for kind in KINDS:
        got = device_decode(engine, kind, frames, own=kind == HEADER)
        check_decode(engine, kind, items, got)
        check_extents(kind, got)


# ---------------------------------------------------------------- group H
def host_route(e, kind, items, seed=0):
    """(kinds, words) of a fused call by the host route: the host scan, the
    host decode of the frames of the kind, their *_verdict_many words;
    DAG_NO_MESSAGE elsewhere."""
    kinds = expected_kinds(e, items)
    words = np.full(len(items), e.DAG_NO_MESSAGE, np.uint32)
    mine = np.flatnonzero(kinds == kind)
    sub = [items[i]["frame"] for i in mine]
    if not sub:
        return kinds, words
    if kind == CERTIFICATE:
        d = e.wire_decode_certificates(sub)
        words[mine] = e.certificate_verdict_many(d["header_inputs"], d["ids"], d["origins"], d["header_sigs"], d["rounds"],
                                                 d["vote_pks"], d["vote_sigs"], d["vote_offsets"], d["payload_counts"],
                                                 rng_seed=seed)
    elif kind == HEADER:
        d = e.wire_decode_headers(sub)
        words[mine] = e.header_verdict_many(d["header_inputs"], d["ids"], d["authors"], d["sigs"], d["payload_counts"])
    else:
        d = e.wire_decode_votes(sub)
        words[mine] = e.vote_verdict_many(d["ids"], d["rounds"], d["origins"], d["authors"], d["sigs"])
    return kinds, words


def fused(e, kind, items, seed=0):
    frames = _frames(items)
    if kind == CERTIFICATE:
        return e.wire_certificate_verdict_many(frames, rng_seed=seed)
    return e.wire_header_verdict_many(frames) if kind == HEADER else e.wire_vote_verdict_many(frames)


@functools.lru_cache(maxsize=None)
def verdict_frames():
    """Frames of tests/verdict_cases.py per kind, as cases."""
    certs = [cases.verdict_frame(2, c["hdr"], c["count"], c["origin"], c["id"], c["hsig"], c["votes"])[0]
             for c in vc.certificate_cases()]
    votes = [W.primary_message(1, W.vote(v["id"], v["round"], v["origin"], v["author"], v["sig"])) for v in vc.vote_cases()]
    return {CERTIFICATE: [dict(frame=f, kind=2) for f in certs], HEADER: [dict(frame=f, kind=0) for f in wire_header_cases()[0]],
            VOTE: [dict(frame=f, kind=1) for f in votes]}


def interleaved(n):
    """n frames: certificate, header and vote cases and errors in turn, so
    every fused call meets placeholders throughout its batch."""
    v = verdict_frames()
    errors = [c for c in cases.error_frames()[::37]] + [dict(frame=b"", kind=None), cases.prefix_pool()[13]]
    out = []
    for i in range(n):
        src = (v[CERTIFICATE], v[HEADER], v[VOTE], errors)[i % 4]
        out.append(src[(i // 4 * 7) % len(src)])  # a stride through each table: every word of the case tables occurs
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_fused_calls_small_large_small(registered, kind):
    """d.pin and d.out grow on demand and are reused: 3 frames, 600, 3 again."""
    e = registered
    small, large = interleaved(3), interleaved(600)
    answers = []
    for items in (small, large, small):
        kinds, words = fused(e, kind, items, seed=11)
        want_kinds, want_words = host_route(e, kind, items, seed=11)
        assert kinds.tolist() == want_kinds.tolist()
        assert words.tolist() == want_words.tolist()
        answers.append((kinds.tolist(), words.tolist()))
    assert answers[2] == answers[0]
    kinds, words = np.array(answers[1][0]), np.array(answers[1][1])
    assert (kinds == kind).sum() == 150 and (kinds < 0).sum() > 100
    assert len(set(words[kinds == kind].tolist())) >= 3 and (words[kinds != kind] == e.DAG_NO_MESSAGE).all()


@pytest.mark.parametrize("kind", KINDS)
def test_fused_calls_without_a_frame_of_their_kind(registered, kind):
    e = registered
    v = verdict_frames()
    others = [c for k in KINDS if k != kind for c in v[k][:5]] + cases.error_frames()[5:200:45]
    kinds, words = fused(e, kind, others)
    assert kinds.tolist() == e.wire_scan(_frames(others))[0].tolist() and not (kinds == kind).any()
    assert (words == e.DAG_NO_MESSAGE).all()
    # five empty frames: n > 0 with no frame bytes at all
    kinds, words = fused(e, kind, [dict(frame=b"", kind=None)] * 5)
    assert kinds.tolist() == [cases.ETRUNC] * 5 and (words == e.DAG_NO_MESSAGE).all()


@pytest.mark.parametrize("kind", [HEADER, CERTIFICATE])
def test_fused_calls_with_frames_over_the_cap(registered, kind):
    """COA_WIRE_ECAPACITY through a fused call: kind -13 and DAG_NO_MESSAGE
    for the frame, its neighbours' words as the host route's."""
    e = registered
    v = verdict_frames()
    over = [c for c in cases.mixed_frames() if c.get("kind") == e.WIRE_ECAPACITY]
    assert len(over) == 2
    items = [v[HEADER][0], over[0], v[CERTIFICATE][0], v[kind][1], over[1], v[VOTE][0], v[kind][2]]
    kinds, words = fused(e, kind, items, seed=3)
    want_kinds, want_words = host_route(e, kind, items, seed=3)
    assert kinds.tolist() == want_kinds.tolist() and kinds[[1, 4]].tolist() == [e.WIRE_ECAPACITY] * 2
    assert words.tolist() == want_words.tolist() and (words[[1, 4]] == e.DAG_NO_MESSAGE).all()
    assert (kinds == kind).sum() == 3 and (words[kinds == kind] != e.DAG_NO_MESSAGE).all()

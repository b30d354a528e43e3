"""CPU: the premises of tests/test_gpu_wire_device_edges.py, asserted with the
host decoder coa_wire.cpp alone (the sequential driver of coa_wire_parse.h, the
grammar the kernels share).

Those GPU tests pin the device wire decoder's work split (LDS staging, the two
compiled bodies, the speculation on the vote stride, the lane-strided sort,
the prefix sums) at its own boundaries; each rests on its inputs having a
property -- a frame of a given length decodes, a batch holds every alignment,
the first defect in wire order has a given code, a mutated batch still reaches
every path.  Here those properties are checked where no GPU is needed, so a
change to tests/wire_dev_cases.py that empties a GPU test of its meaning fails
on any machine."""
import glob
import os
import struct

import numpy as np
import pytest

from conftest import ROOT

import wire_codec as W
import wire_dev_cases as cases

HEADER, VOTE, CERTIFICATE = 0, 1, 2
SLACK = 4096  # behind the frames in the GPU tests' buffers


@pytest.fixture(scope="module")
def e():
    import build

    build.build()
    import coa_crypto

    coa_crypto.lib()
    return coa_crypto


def _kinds(e, items):
    return e.wire_scan([c["frame"] for c in items])[0]


def _as_built(e, items):
    """Every case that names a kind decodes as it on the host."""
    hk = _kinds(e, items)
    for i, c in enumerate(items):
        if c.get("kind") is not None and c["kind"] != e.WIRE_ECAPACITY:
            assert hk[i] == c["kind"], (i, hk[i], c["kind"])
    return hk


def corpus():
    names = sorted(glob.glob(os.path.join(ROOT, "tests", "fuzz", "wire_corpus", "*.bin")))
    return [open(n, "rb").read() for n in names]


# ---------------------------------------------------------------- group A
def test_alignment_and_stage_switch_inputs(e):
    under_test = cases.alignment_frames()
    hk = _as_built(e, under_test)
    assert hk[:4].tolist() == [VOTE, HEADER, CERTIFICATE, CERTIFICATE]
    assert not cases.takes_the_walk(under_test[2]["frame"]) and cases.takes_the_walk(under_test[3]["frame"])
    assert len(set(under_test[1]["parents"])) < len(under_test[1]["parents"])
    assert len({d for d, _ in under_test[1]["payload"]}) < len(under_test[1]["payload"])
    assert [len(c["frame"]) for c in under_test[4:]] == [0, 1, 2, 3, 4, 5] and (hk[4:] < 0).all()

    switch = cases.stage_switch_frames()
    hk = _as_built(e, switch)
    assert set(hk.tolist()) == {HEADER, CERTIFICATE}
    by_len = {}
    for c, k in zip(switch, hk):
        by_len.setdefault(len(c["frame"]), set()).add(int(k))
    assert sorted(by_len) == list(range(cases.STAGE - 4, cases.STAGE + 5))  # every length, each by a decoding frame
    below = set().union(*(v for n, v in by_len.items() if n <= cases.STAGE))
    above = set().union(*(v for n, v in by_len.items() if n > cases.STAGE))
    assert below == above == {HEADER, CERTIFICATE} and by_len[cases.STAGE] == {HEADER, CERTIFICATE}
    # decoded in place with the dword signature copy: canonical votes just above the switch, at an even and an odd length
    canon = {len(c["frame"]) for c in switch if c["kind"] == CERTIFICATE and not cases.takes_the_walk(c["frame"])}
    assert {cases.STAGE, cases.STAGE + 3, cases.STAGE + 4} <= canon
    d = e.wire_decode_certificates([c["frame"] for c in switch if c["kind"] == CERTIFICATE])
    assert (np.diff(d["vote_offsets"].astype(np.int64)) == 7).all()

    batch, at, mis = cases.at_every_alignment(under_test + switch)
    hk = _kinds(e, batch)
    offs = np.concatenate([[0], np.cumsum([len(c["frame"]) for c in batch])])
    assert [int(offs[i]) % 4 for i in at] == mis == [0, 1, 2, 3] * (len(under_test) + len(switch))
    assert all(len(batch[i - 1]["frame"]) < 4 for i in at)  # the fillers
    for j, i in enumerate(at):
        assert batch[i] is (under_test + switch)[j // 4]
    pairs = {(int(offs[i]) % 4, len(batch[i]["frame"]) % 4) for i in range(len(batch)) if hk[i] >= 0}
    assert len(pairs) == 16
    # ... and the frames shorter than what the staging copy moves before its first dword
    assert {(int(offs[i]) % 4, len(batch[i]["frame"])) for i in at if len(batch[i]["frame"]) < 4} == \
        {(m, n) for m in range(4) for n in range(4)}


# ---------------------------------------------------------------- group B
def test_prefix_sum_batches(e):
    pool = cases.prefix_pool()
    hk = _as_built(e, pool)
    assert len(pool) == 16 and max(len(c["frame"]) for c in pool) < 1024
    assert {0, 1, 2, 3} <= set(hk.tolist()) and (hk < 0).sum() == 2 and min(len(c["frame"]) for c in pool) == 0
    d = e.wire_decode_certificates([c["frame"] for c in pool if c["kind"] == CERTIFICATE])
    assert set(np.diff(d["vote_offsets"].astype(np.int64)).tolist()) == {0, 1, 2, 3, 4, 5}
    B = cases.SCAN_BLOCK
    assert cases.PREFIX_SIZES == (255, 256, 257, 65537, 2 * 65536 + 257)
    per = [-(-(-(-n // B)) // B) for n in cases.PREFIX_SIZES]  # block totals per thread of k_wire_scan_totals
    assert per == [1, 1, 1, 2, 3]
    blocks = -(-cases.PREFIX_SIZES[-1] // B)
    assert -(-blocks // 3) < B and blocks % 3 != 0  # idle threads behind a ragged last one
    assert sum(len(c["frame"]) for c in pool) / 16 * cases.PREFIX_SIZES[-1] < 41e6  # the largest batch: about 40 MB
    for n in cases.PREFIX_SIZES:
        for kind in (HEADER, VOTE, CERTIFICATE):
            idx = cases.prefix_indices(n, kind)
            assert len(idx) == n and idx.min() == 0 and idx.max() == 15
            mine = hk[idx] == kind
            forced = n == cases.PREFIX_SIZES[-1]
            lo = 3 * B if forced else 0
            full = (n - lo) // B
            m = mine[lo:lo + full * B].reshape(full, B)
            if forced:
                assert not mine[:lo].any() and mine[-1]
                f = cases.PREFIX_FORCED_BLOCK - 3
                assert m[f].all() and 3 < cases.PREFIX_FORCED_BLOCK < blocks - 1
                m = np.delete(m, f, axis=0)
            if full:
                assert (m.any(axis=1) & ~m.all(axis=1)).all()  # every block: frames of the kind and others
            assert mine.any() and not mine.all()


# ---------------------------------------------------------------- group C
def test_vote_reduction_inputs(e):
    items = cases.vote_reduction_frames()
    hk = _kinds(e, items)
    for c, k in zip(items, hk):
        assert k == (CERTIFICATE if c["code"] is None else c["code"]), (c["note"], k)
    assert {c["code"] for c in items} == {None, cases.ETRUNC, cases.EFORMAT, cases.EKEY}
    pairs = [c for c in items if c.get("pair")]
    assert len(pairs) == 12
    for c in pairs:  # the canonical length throughout: the speculation holds and the wave-wide minimum decides
        assert not cases.takes_the_walk(c["frame"]) and len(cases.vote_key_fields(c["frame"])) == 130
        (a, ca), (b, cb) = c["pair"]
        assert {ca, cb} == {cases.EKEY, cases.EFORMAT} and c["code"] == (ca if a < b else cb)
    for places in ((3, 70), (70, 3), (63, 64), (64, 63), (127, 128), (128, 127)):  # each code in each place
        there = [c["pair"] for c in pairs if (c["pair"][0][0], c["pair"][1][0]) == places]
        assert {p[0][1] for p in there} == {cases.EKEY, cases.EFORMAT}
    cuts = [c for c in items if "cut" in c["note"]]
    assert [c["code"] for c in cuts] == [cases.ETRUNC, cases.EKEY] * 2
    for c in cuts:
        at = cases.vote_key_fields(c["frame"])
        assert len(at) in (129, 130)  # the cut is inside vote 129
        assert len(c["frame"]) - at[128] - cases.VOTE_STRIDE in (4, 52 + 34)
    walk = [c for c in items if "characters" in c["note"]]
    assert len(walk) == 2 and all(cases.takes_the_walk(c["frame"]) and c["code"] is None for c in walk)
    d = e.wire_decode_certificates([c["frame"] for c in items if c["code"] is None])
    assert np.diff(d["vote_offsets"].astype(np.int64)).tolist() == [130, 130, 130]
    over = [c for c in items if "claimed" in c["note"]]
    assert len(over) == 1 and items[-1] is not over[0]
    f = over[0]["frame"]
    at = cases.vote_key_fields(f)
    nv = struct.unpack_from("<Q", f, at[0] - 8)[0]
    rest = len(f) - at[0]
    assert rest // cases.VOTE_STRIDE < nv <= rest // 72 and len(at) == 62 and not cases.takes_the_walk(f)


# ---------------------------------------------------------------- group D
def test_set_inputs(e):
    items = cases.set_frames()
    hk = _as_built(e, items)
    assert set(hk.tolist()) == {HEADER, CERTIFICATE}
    sizes = {}
    for c in items[:21]:
        sizes.setdefault(len(c["payload"]), []).append(c)
    assert sorted(sizes) == [63, 64, 65, 127, 128, 129, cases.MAX_ENTRIES]
    for cs in sizes.values():
        keys = [[d for d, _ in c["payload"]] for c in cs]
        assert keys[0] == sorted(keys[0]) and keys[1] == sorted(keys[1], reverse=True)
        assert keys[2] not in (sorted(keys[2]), sorted(keys[2], reverse=True))
    for c, k in zip(items, hk):
        one = [c["frame"]]
        d = e.wire_decode_headers(one) if k == HEADER else e.wire_decode_certificates(one)
        assert d["header_inputs"][0] == W.header_digest_input(c["author"], c["round"], c["payload"], c["parents"])
        assert int(d["payload_counts"][0]) == len({d_ for d_, _ in c["payload"]})
    dup = [c for c in items if c.get("note") == "duplicates"]
    assert sorted(c["kind"] for c in dup) == [HEADER, CERTIFICATE]
    for c in dup:
        keys = [d for d, _ in c["payload"]]
        assert len(keys) == 192
        dist = sorted(j - i for i in range(192) for j in range(i + 1, 192) if keys[i] == keys[j])
        assert dist == [1, 63, 64, 64, 64, 65, 128, 128]
        assert keys[0] == keys[64] == keys[128] and [c["payload"][i][1] for i in (0, 64, 128)] == [7001, 7002, 7003]
        got = e.wire_decode_headers([c["frame"]]) if c["kind"] == HEADER else e.wire_decode_certificates([c["frame"]])
        entries = got["header_inputs"][0][40:40 + 36 * int(got["payload_counts"][0])]
        assert entries.count(keys[0]) == 1 and entries[entries.index(keys[0]) + 32:][:4] == struct.pack("<I", 7003)
    few = {c["note"]: c for c in items if c.get("note") in ("512 of 1024", "3 of 1024")}
    c = few["512 of 1024"]
    assert len(c["payload"]) == cases.MAX_ENTRIES and len({d for d, _ in c["payload"]}) == 512
    c = few["3 of 1024"]
    assert len(c["parents"]) == cases.MAX_ENTRIES and len(set(c["parents"])) == 3
    both = [c for c in items if c.get("note") == "both at the cap"]
    assert sorted(c["kind"] for c in both) == [HEADER, CERTIFICATE]
    assert all(len(c["payload"]) == len(c["parents"]) == cases.MAX_ENTRIES for c in both)


# ---------------------------------------------------------------- group E
def test_tightest_certificate_uses_the_bound_less_one(e):
    c = cases.tightest_certificate()
    f = c["frame"]
    assert len(f) == 183 + 115 * 200
    kinds, _, nv = e.wire_scan([f])
    assert kinds[0] == CERTIFICATE and int(nv[0]) == 200 == e.wire_votes_bound(len(f)) - 1
    d = e.wire_decode_certificates([f])
    assert d["header_inputs"][0] == W.header_digest_input(c["author"], c["round"], [], [])
    assert [bytes(p) for p in d["vote_pks"]] == [pk for pk, _ in c["votes"]]


# ---------------------------------------------------------------- group F
def test_offsets_case(e):
    blob, slack, offsets, items = cases.offsets_case()
    fb = len(blob)
    n = len(offsets) - 1
    assert len(items) == n and max(offsets) <= fb + SLACK and len(slack) <= SLACK
    whole = blob + slack + b"\xee" * (SLACK - len(slack))
    ranges = list(zip(offsets[:-1], offsets[1:]))
    ok = [o0 <= o1 <= fb for o0, o1 in ranges]
    assert sum(o0 > o1 for o0, o1 in ranges) == 2  # decreasing pairs
    assert any(o0 < fb and o1 == fb + 1 for o0, o1 in ranges)  # ends one byte behind the buffer
    assert any(fb < o0 < o1 for o0, o1 in ranges)  # wholly in the slack
    hk = _as_built(e, items)
    for (o0, o1), good, c, k in zip(ranges, ok, items, hk):
        if good:
            assert whole[o0:o1] == c["frame"] and k == c["kind"] and k >= 0
        else:
            assert c["frame"] == b"" and k == cases.ETRUNC
    assert ok[0] and ok[1] and ok[-1] and not all(ok[2:-1]) and sum(ok) == 5
    assert {int(k) for k, good in zip(hk, ok) if good} == {HEADER, VOTE, CERTIFICATE}
    # a decoder that ignored the rule would answer differently: those bytes decode
    ignored = [whole[o0:o1] for (o0, o1), good in zip(ranges, ok) if not good and o0 <= o1]
    assert (e.wire_scan(ignored)[0] >= 0).sum() >= 2


# ---------------------------------------------------------------- group G
def test_differential_batch_reaches_every_path(e):
    items = cases.differential_frames(corpus())
    assert items == cases.differential_frames(corpus())  # seeded
    n = len(items)
    assert n == 4000
    hk = _kinds(e, items).copy()
    over = np.array([cases.over_the_cap(c["frame"]) for c in items]) & ((hk == HEADER) | (hk == CERTIFICATE))
    assert 0 < over.sum() < n // 10
    hk[over] = e.WIRE_ECAPACITY  # not decoded on the device
    assert (hk >= 0).sum() >= n // 4
    for kind in (HEADER, VOTE, CERTIFICATE):
        assert (hk == kind).sum() >= n // 20, kind
    for code in (-10, -11, -12):
        assert (hk == code).sum() >= 50, code
    assert sum(1 for c, k in zip(items, hk) if k == CERTIFICATE and cases.takes_the_walk(c["frame"])) >= 100
    assert sum(len(c["frame"]) > cases.STAGE for c in items) >= 100
    assert sum(1 for c, k in zip(items, hk) if k >= 0 and len(c["frame"]) > cases.STAGE) >= 50


def test_constants_match_the_sources():
    csrc = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")
    hip = open(os.path.join(csrc, "coa_wire_dev.hip")).read()
    assert f"constexpr uint32_t kStage = {cases.STAGE};" in hip
    assert f"#define COA_WIRE_SCAN_BLOCK {cases.SCAN_BLOCK}u" in open(os.path.join(csrc, "coa_wire_layout.h")).read()
    assert f"#define COA_WP_VOTE_STRIDE {cases.VOTE_STRIDE}u" in open(os.path.join(csrc, "coa_wire_parse.h")).read()

"""Batches of interleaved PrimaryMessage frames for the mixed mode of the wire
decoder (coa_wire_decode_mixed_device, coa_wire_verdict_many,
coa_cpu_wire_verdict_many), built from tests/wire_dev_cases.py and
tests/verdict_cases.py.  tests/test_wire_mixed_host.py asserts without a GPU
what these batches must hold for tests/test_gpu_wire_mixed.py to mean
anything."""
import functools
import glob
import os

import numpy as np

import verdict_cases as vc
import wire_codec as W
import wire_dev_cases as cases

HEADER, VOTE, CERTIFICATE, CERT_REQUEST = 0, 1, 2, 3
ETRUNC, EFORMAT, EKEY, ECAPACITY = -10, -11, -12, -13
NO_MESSAGE = 255
NO_SLOT = 0xffffffff
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_kinds(e, frames):
    """What the device scan answers: the host scan's kinds, COA_WIRE_ECAPACITY
    where the host accepts a Header / Certificate one of whose sets is over the
    cap (by wire_dev_cases' own parse of the frame)."""
    hk, hb, nv = e.wire_scan(frames)
    hk = hk.copy()
    for i, f in enumerate(frames):
        if hk[i] in (HEADER, CERTIFICATE) and cases.over_the_cap(f):
            hk[i] = ECAPACITY
    slot = (hk >= 0) & (hk <= 2)
    return hk, np.where(slot, hb, 0), np.where(hk == CERTIFICATE, nv, 0)


def expected_slots(kinds):
    """The stable partition by NumPy: each frame's rank among the frames of
    its kind, NO_SLOT for the frames without one."""
    kinds = np.asarray(kinds)
    slots = np.full(len(kinds), NO_SLOT, np.uint32)
    for k in (HEADER, VOTE, CERTIFICATE):
        m = kinds == k
        slots[m] = np.arange(int(m.sum()), dtype=np.uint32)
    return slots


def expected_totals(kinds, hb, nv):
    kinds, hb, nv = np.asarray(kinds), np.asarray(hb).astype(np.int64), np.asarray(nv).astype(np.int64)
    h, v, c = kinds == HEADER, kinds == VOTE, kinds == CERTIFICATE
    return [int(h.sum()), int(hb[h].sum()), int(v.sum()), int(c.sum()), int(hb[c].sum()), int(nv[c].sum()),
            int(len(kinds) - h.sum() - v.sum() - c.sum()), 0]


# ------------------------------------------------------------ verdict cases
@functools.lru_cache(maxsize=None)
def verdict_batch():
    """The verdict cases of tests/verdict_cases.py as frames, certificates,
    headers and votes dealt round-robin into one batch, plus a truncated, a
    rubbish and an empty frame and a certificate request.  Returns (frames,
    names, kind of each frame or None where it must not decode, expected
    words)."""
    from test_gpu_wire_device import wire_header_cases

    certs = []
    for c in vc.certificate_cases():
        f, hdr, count = cases.verdict_frame(2, c["hdr"], c["count"], c["origin"], c["id"], c["hsig"], c["votes"])
        assert hdr == c["hdr"] and count == c["count"]
        certs.append(f)
    hframes, hnames, hwant = wire_header_cases()
    votes = [W.primary_message(1, W.vote(v["id"], v["round"], v["origin"], v["author"], v["sig"])) for v in vc.vote_cases()]
    tables = [(CERTIFICATE, certs, [c["name"] for c in vc.certificate_cases()], vc.expected_certificates()[0]),
              (HEADER, hframes, hnames, hwant),
              (VOTE, votes, [v["name"] for v in vc.vote_cases()], vc.expected_votes())]
    frames, names, kinds, want = [], [], [], []
    for j in range(max(len(t[1]) for t in tables)):
        for kind, fs, ns, ws in tables:
            if j < len(fs):
                frames.append(fs[j])
                names.append(ns[j])
                kinds.append(kind)
                want.append(int(ws[j]))
    request = W.primary_message(3, W.cert_request([bytes(range(32)), bytes(range(1, 33))], bytes(range(2, 34))))
    extras = [(7, certs[0][:len(certs[0]) // 2], "truncated", None), (20, b"\x09\x00\x00\x00rubbish", "rubbish", None),
              (33, b"", "empty", None), (len(frames) + 3, request, "certificate request", CERT_REQUEST)]
    for at, f, name, kind in extras:
        frames.insert(at, f)
        names.insert(at, name)
        kinds.insert(at, kind)
        want.insert(at, NO_MESSAGE)
    return frames, names, kinds, np.array(want, np.uint32)


# ------------------------------------------------------------- prefix sums
SUM_SIZES = (255, 256, 257, 513, 65536, 65537)
LASTS = (HEADER, VOTE, CERTIFICATE, None)  # None: an error
# of prefix_pool(): by kind; the short ones for the two large sizes (votes, a header and certificates with one entry
# or none, a certificate request, a truncated and an empty frame)
POOL = {HEADER: [2, 3, 4, 5], VOTE: [0, 1], CERTIFICATE: [6, 7, 8, 9, 10, 11, 12], CERT_REQUEST: [13], None: [14, 15]}
SHORT = {HEADER: [3], VOTE: [0, 1], CERTIFICATE: [6, 7], CERT_REQUEST: [13], None: [14, 15]}
BLOCK = cases.SCAN_BLOCK
ALL_CERTIFICATES_BLOCK, NO_VOTE_BLOCK = 5, 7  # of the two large batches


def sum_indices(n, last, seed=91):
    """Pool indices of an n-frame batch with the kinds interleaved at random
    and: frames 255 / 256 / 257 a vote, a header and a certificate; at 513 no
    vote in block 1; at the two large sizes block 5 wholly certificates and no
    vote in block 7; the last frame of kind `last` (None: an error)."""
    pool = SHORT if n >= 65536 else POOL
    every = [i for v in pool.values() for i in v]
    g = np.random.default_rng(seed + n)
    idx = g.choice(every, n)
    no_vote = [i for k, v in pool.items() if k != VOTE for i in v]

    def block(b, choice):
        lo, hi = b * BLOCK, min(n, (b + 1) * BLOCK)
        if lo < hi:
            idx[lo:hi] = g.choice(choice, hi - lo)

    if n == 513:
        block(1, no_vote)
    if n >= 65536:
        block(ALL_CERTIFICATES_BLOCK, pool[CERTIFICATE])
        block(NO_VOTE_BLOCK, no_vote)
    for at, kind in ((255, VOTE), (256, HEADER), (257, CERTIFICATE)):
        if at < n:
            idx[at] = pool[kind][at % len(pool[kind])]
    idx[n - 1] = pool[last][0]
    return idx


# ---------------------------------------------------- work split and extents
@functools.lru_cache(maxsize=None)
def work_split_items():
    """alignment_frames() and stage_switch_frames() dealt into one batch with
    votes between them, so LDS-staged and flat frames of different kinds sit
    beside each other; then every kind and code the pools lack (premise of
    tests/test_wire_mixed_host.py)."""
    import random

    rng = random.Random(93)
    out = []
    for a in cases.alignment_frames() + cases.stage_switch_frames():
        out.append(a)
        out.append(cases.make_vote(rng))
    return out + coverage_items()


@functools.lru_cache(maxsize=None)
def coverage_items():
    """Constructed frames that give a pool every kind and every code: the
    batch of mixed_frames() (four kinds, the cap on both sides, a truncation)
    and, from error_frames(), truncations and the constructed defects at its
    end: an unknown variant, malformed keys of both codes in both orders, the
    count checks (tests/test_wire_mixed_host.py checks against the host scan
    that every code is there)."""
    errs = cases.error_frames()
    return cases.mixed_frames() + errs[::29] + errs[-18:]


@functools.lru_cache(maxsize=None)
def differential_items():
    corpus = [open(p, "rb").read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "fuzz", "wire_corpus", "*.bin")))]
    assert len(corpus) >= 15
    return cases.differential_frames(corpus, 4000) + coverage_items()

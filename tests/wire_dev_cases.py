"""Test infrastructure: the constructed frames of the device wire decoder's
tests, built with the independent encoder tests/wire_codec.py.  Shared by
tests/test_gpu_wire_device.py (the kernels) and tests/test_wire_parse_host.py
(the same grammar header on the CPU, through tests/sanitize/wire_parse_driver.cpp).

Every case is a dict: frame (bytes), kind (0 Header, 1 Vote, 2 Certificate,
3 CertificatesRequest, None: whatever the host decoder says) and, for a frame
that decodes, the fields it was built from (author, round, payload, parents,
id, sig, votes | origin), from which wire_codec.header_digest_input gives the
expected digest input."""
import base64
import random
import struct

import wire_codec as W

MAX_ENTRIES = 1024  # COA_WIRE_DEV_MAX_ENTRIES


def _rand(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def make_header(rng, payload, parents, variant=0, votes=(), author_field=None, vote_fields=None):
    """A Header (variant 0) or Certificate (2) frame and its fields.
    vote_fields: per vote, the raw key field to use instead of W.key(pk)."""
    author, id_, sig, rnd = _rand(rng, 32), _rand(rng, 32), _rand(rng, 64), rng.getrandbits(64)
    hb = W.header(author, rnd, payload, parents, id_, sig, author_field=author_field)
    if variant == 0:
        body = hb
    else:
        body = hb + struct.pack("<Q", len(votes))
        for k, (pk, sg) in enumerate(votes):
            body += (vote_fields[k] if vote_fields and vote_fields[k] is not None else W.key(pk)) + bytes(sg)
    return dict(frame=W.primary_message(variant, body), kind=variant, author=author, round=rnd, payload=list(payload),
                parents=list(parents), id=id_, sig=sig, votes=list(votes))


def make_vote(rng, origin_field=None, author_field=None):
    id_, rnd, origin, author, sig = _rand(rng, 32), rng.getrandbits(64), _rand(rng, 32), _rand(rng, 32), _rand(rng, 64)
    body = bytes(id_) + struct.pack("<Q", rnd) + (origin_field or W.key(origin)) + (author_field or W.key(author)) + sig
    return dict(frame=W.primary_message(1, body), kind=1, id=id_, round=rnd, origin=origin, author=author, sig=sig)


def small_certificates(n=40, seed=1):
    """The frames of test_wire.py::test_certificate_frames_roundtrip: payload
    0-6, parents 0-4, votes 0-8, every third with a repeated payload key and a
    repeated parent."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        payload = [(_rand(rng, 32), rng.getrandbits(32)) for _ in range(i % 7)]
        parents = [_rand(rng, 32) for _ in range((3 * i) % 5)]
        if i % 3 == 0 and payload:
            payload.append((payload[0][0], 77))
        if i % 3 == 0 and parents:
            parents.append(parents[-1])
        votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(i % 9)]
        out.append(make_header(rng, payload, parents, 2, votes))
    return out


def _ordered(rng, items, order):
    items = sorted(items)
    if order == "descending":
        items.reverse()
    elif order == "shuffled":
        rng.shuffle(items)
    return items


def boundary_frames(seed=5):
    """Set sizes around the wave width and its multiples, in three wire
    orders; key sets that tell a wrong comparison; duplicates."""
    rng = random.Random(seed)
    out = []
    k = 0
    for npay in (0, 1, 2, 31, 32, 33):
        for npar in (0, 1, 2, 63, 64, 65, 67, 127, 128, 129):
            for order in ("ascending", "descending", "shuffled"):
                pay = _ordered(rng, [(_rand(rng, 32), rng.getrandbits(32)) for _ in range(npay)], order)
                par = _ordered(rng, [_rand(rng, 32) for _ in range(npar)], order)
                votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(k % 3)]
                out.append(make_header(rng, pay, par, 2 if k % 2 else 0, votes if k % 2 else ()))
                k += 1
    base = _rand(rng, 32)
    sets = {
        "byte 31 only": [base[:31] + bytes([v]) for v in (0x00, 0x01, 0x7f, 0x80, 0x81, 0xff, 0x10, 0xf0)],
        "byte 0 only, both sides of 0x80": [bytes([v]) + base[1:] for v in (0x00, 0x7f, 0x80, 0xff, 0x01, 0x81, 0x40, 0xc0)],
        "first 8 bytes shared": [base[:8] + _rand(rng, 24) for _ in range(9)],
        "first 16 bytes shared": [base[:16] + _rand(rng, 16) for _ in range(9)],
        # little-endian words: byte 3 is a word's top byte, byte 4 the next word's low byte
        "bytes 3 and 4": [base[:3] + bytes([a, b]) + base[5:] for a, b in ((1, 2), (2, 1), (0x80, 0), (0, 0x80), (0xff, 1))],
    }
    for keys in sets.values():
        for order in ("ascending", "descending", "shuffled"):
            ks = _ordered(rng, keys, order)
            out.append(make_header(rng, [(d, i + 1) for i, d in enumerate(ks)], ks, 0))
            out.append(make_header(rng, [(d, i + 1) for i, d in enumerate(ks)], ks[::-1], 2,
                                   [(_rand(rng, 32), _rand(rng, 64))]))
    same = _rand(rng, 32)
    for npar in (2, 64, 67, 130):
        out.append(make_header(rng, [], [same] * npar, 0))  # all parents equal: one
    d = _rand(rng, 32)
    others = [(_rand(rng, 32), 10 + i) for i in range(6)]
    pay = [(d, 1), others[0], others[1], (d, 2), others[2], others[3], others[4], (d, 3), others[5]]
    out.append(make_header(rng, pay, [_rand(rng, 32)], 0))  # three occurrences, not adjacent: worker id 3 wins
    out.append(make_header(rng, pay[::-1], [_rand(rng, 32)], 2, [(_rand(rng, 32), _rand(rng, 64))]))  # ... id 1 wins
    return out


def _key_forms(k32, rng):
    """The accepted string forms of a 32-byte key."""
    canonical = base64.b64encode(k32)
    return {"canonical 44": W.raw_key(canonical), "unpadded 43": W.raw_key(canonical.rstrip(b"=")),
            "64 characters": W.raw_key(base64.b64encode(k32 + _rand(rng, 16)))}


def malformed_keys():
    """name -> raw key field, the malformed set of test_truncation_and_malformed_keys."""
    k32 = bytes(range(32))
    return {
        "short key": W.raw_key(base64.b64encode(k32[:16])),
        "invalid character": W.raw_key(base64.b64encode(k32)[:-3] + b"*A="),
        "non-zero trailing bits": W.raw_key(base64.b64encode(k32)[:-2] + b"B="),
        "too much padding": W.raw_key(base64.b64encode(k32) + b"=="),
        "not UTF-8": W.raw_key(b"\xff" * 44),
        "length prefix beyond the frame": b"\xff" * 8 + b"AAAA",
        "one byte short": W.raw_key(base64.b64encode(k32[:31])),  # 44 characters, as a canonical key has
    }


def key_string_frames(seed=6):
    rng = random.Random(seed)
    out = []
    # the author in each accepted form; the votes of one certificate in mixed forms (the stride varies inside the frame)
    for name in ("canonical 44", "unpadded 43", "64 characters"):
        c = make_header(rng, [(_rand(rng, 32), 1)], [_rand(rng, 32)], 0)
        out.append(make_header(rng, c["payload"], c["parents"], 0, author_field=None))
        a = _rand(rng, 32)
        h = make_header(rng, c["payload"], c["parents"], 0, author_field=_key_forms(a, rng)[name])
        h["author"] = a
        out.append(h)
        for pos in (0, 3, 6):  # the odd form first, in the middle, last of 7 votes
            votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(7)]
            fields = [None] * 7
            fields[pos] = _key_forms(votes[pos][0], rng)[name]
            out.append(make_header(rng, c["payload"], c["parents"], 2, votes, vote_fields=fields))
    votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(70)]  # more than one wave of votes, three forms mixed
    fields = [_key_forms(pk, rng)[("canonical 44", "unpadded 43", "64 characters")[k % 3]] for k, (pk, _) in enumerate(votes)]
    out.append(make_header(rng, [], [], 2, votes, vote_fields=fields))
    votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(130)]
    out.append(make_header(rng, [], [], 2, votes))  # canonical throughout: three rounds of lanes
    fields = [None] * 130
    fields[129] = _key_forms(votes[129][0], rng)["unpadded 43"]
    out.append(make_header(rng, [], [], 2, votes, vote_fields=fields))
    v = make_vote(rng)
    for name in ("unpadded 43", "64 characters"):
        o, a = _rand(rng, 32), _rand(rng, 32)
        w = make_vote(rng, origin_field=_key_forms(o, rng)[name], author_field=_key_forms(a, rng)[name])
        w["origin"], w["author"] = o, a
        out.append(w)
    out.append(v)
    # malformed: on the author, and on a vote in the middle of a certificate
    for name, field in malformed_keys().items():
        bad = make_header(rng, [], [], 0, author_field=field)
        out.append(dict(frame=bad["frame"], kind=None))
        for pos in (0, 2, 4):
            votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(5)]
            fields = [None] * 5
            fields[pos] = field
            out.append(dict(frame=make_header(rng, [], [_rand(rng, 32)], 2, votes, vote_fields=fields)["frame"], kind=None))
        out.append(dict(frame=make_vote(rng, author_field=field)["frame"], kind=None))
    return out


def error_frames(seed=7):
    """Truncation at every byte, trailing bytes, an unknown variant, and two
    defects of different codes in both orders."""
    rng = random.Random(seed)
    out = []
    cert = make_header(rng, [(_rand(rng, 32), 1), (_rand(rng, 32), 2)], [_rand(rng, 32), _rand(rng, 32)], 2,
                       [(_rand(rng, 32), _rand(rng, 64)) for _ in range(2)])
    hdr = make_header(rng, [(_rand(rng, 32), 1)], [_rand(rng, 32)], 0)
    vote = make_vote(rng)
    for whole in (cert, hdr, vote):
        f = whole["frame"]
        out += [dict(frame=f[:k], kind=None) for k in range(len(f))]
        t = dict(whole)
        t["frame"] = f + b"trailing"
        out.append(t)
    out.append(dict(frame=b"\x07\x00\x00\x00" + cert["frame"][4:], kind=None))
    out.append(dict(frame=b"\x04\x00\x00\x00", kind=None))
    bad = malformed_keys()
    ekey, eformat = bad["short key"], bad["not UTF-8"]
    votes = [(_rand(rng, 32), _rand(rng, 64)) for _ in range(6)]
    for first, second in ((ekey, eformat), (eformat, ekey)):
        fields = [None, first, None, None, second, None]
        out.append(dict(frame=make_header(rng, [], [], 2, votes, vote_fields=fields)["frame"], kind=None))
        # a bad author and a bad vote; a bad vote and a truncated tail
        out.append(dict(frame=make_header(rng, [], [], 2, votes, author_field=first, vote_fields=fields)["frame"], kind=None))
        f = make_header(rng, [], [], 2, votes, vote_fields=[None, None, None, None, first, None])["frame"]
        out.append(dict(frame=f[:-30], kind=None))  # the error at vote 4 comes before the cut in vote 5
        out.append(dict(frame=f[:-(116 + 30)], kind=None))  # ... and here the cut is in vote 4's signature, after its key
        out.append(dict(frame=make_vote(rng, origin_field=first, author_field=second)["frame"], kind=None))
    # the up-front count checks: a count that cannot fit, before later defects
    h = make_header(rng, [(_rand(rng, 32), 1)], [_rand(rng, 32)], 0)["frame"]
    at_np = 4 + 8 + 44 + 8
    for v in (1 << 40, len(h), (len(h) - at_np - 8) // 36 + 1):
        out.append(dict(frame=h[:at_np] + struct.pack("<Q", v) + h[at_np + 8:], kind=None))
    out.append(dict(frame=b"", kind=None))
    return out


def mixed_frames(seed=9):
    """One batch of every kind, with the capacity boundary."""
    rng = random.Random(seed)
    out = []
    for k in range(24):
        if k % 4 == 0:
            out.append(make_header(rng, [(_rand(rng, 32), k)], [_rand(rng, 32) for _ in range(k % 5)], 0))
        elif k % 4 == 1:
            out.append(make_vote(rng))
        elif k % 4 == 2:
            out.append(make_header(rng, [(_rand(rng, 32), k), (_rand(rng, 32), k + 1)], [_rand(rng, 32) for _ in range(k % 3)], 2,
                                   [(_rand(rng, 32), _rand(rng, 64)) for _ in range(k % 5)]))
        else:
            out.append(dict(frame=W.primary_message(3, W.cert_request([_rand(rng, 32) for _ in range(k % 4)], _rand(rng, 32))),
                            kind=3))
    out.insert(5, dict(frame=out[0]["frame"][:50], kind=None))
    out.append(make_header(rng, [], [_rand(rng, 32) for _ in range(MAX_ENTRIES)], 0))  # at the cap: decodes
    over = make_header(rng, [], [_rand(rng, 32) for _ in range(MAX_ENTRIES + 1)], 0)
    out.append(dict(frame=over["frame"], kind=-13))  # COA_WIRE_ECAPACITY: the host decoder accepts it
    over = make_header(rng, [(_rand(rng, 32), 1)] * (MAX_ENTRIES + 1), [], 2, [(_rand(rng, 32), _rand(rng, 64))])
    out.append(dict(frame=over["frame"], kind=-13))
    # over the cap and malformed further on: the host's error wins
    out.append(dict(frame=make_header(rng, [], [_rand(rng, 32) for _ in range(MAX_ENTRIES + 1)], 2,
                                      [(_rand(rng, 32), _rand(rng, 64))],
                                      vote_fields=[malformed_keys()["short key"]])["frame"], kind=None))
    return out


def digest_input_fields(hdr, count):
    """(round, payload, parents) of a Header::digest input with `count`
    payload entries; bytes after the last whole parent are dropped."""
    rnd = struct.unpack("<Q", hdr[32:40])[0]
    pay = [(hdr[40 + 36 * k:72 + 36 * k], struct.unpack("<I", hdr[72 + 36 * k:76 + 36 * k])[0]) for k in range(count)]
    rest = hdr[40 + 36 * count:]
    return rnd, pay, [rest[32 * k:32 * k + 32] for k in range(len(rest) // 32)]


def verdict_frame(variant, hdr, count, author, id_, sig, votes=()):
    """A Header or Certificate of tests/verdict_cases.py as a frame, payload
    and parents in wire order reversed.  Returns (frame, the digest input the
    frame decodes to, its payload count): equal to (hdr, count) when hdr is a
    digest input a frame can carry -- starts with the author, whole entries,
    sets in key order."""
    rnd, pay, par = digest_input_fields(hdr, count)
    body = W.header(author, rnd, pay[::-1], par[::-1], id_, sig)
    if variant == 2:
        body = W.certificate(body, votes)
    return (W.primary_message(variant, body), W.header_digest_input(author, rnd, pay, par),
            len({bytes(d) for d, _ in pay}))


# ------------------------------------------------------------------------
# The kernels' work split at its own boundaries (tests/test_gpu_wire_device_edges.py;
# the premises these inputs rest on are asserted with the host decoder alone
# in tests/test_wire_dev_cases_host.py).
LANES = 64
STAGE = 12288      # kStage of coa_wire_dev.hip: frames up to this long are staged in LDS
SCAN_BLOCK = 256   # COA_WIRE_SCAN_BLOCK
VOTE_STRIDE = 116  # COA_WP_VOTE_STRIDE
ETRUNC, EFORMAT, EKEY = -10, -11, -12


def _votes(rng, n):
    return [(_rand(rng, 32), _rand(rng, 64)) for _ in range(n)]


def _short_key(pk):
    return W.raw_key(base64.b64encode(pk).rstrip(b"="))


def alignment_frames(seed=21):
    """The frames placed at every dword misalignment: a vote, a header whose
    sets hold duplicates, a canonical certificate, one with a 43-character
    vote key, and frames shorter than a dword and just above it."""
    rng = random.Random(seed)
    pay = [(_rand(rng, 32), 1 + i) for i in range(2)]
    pay.append((pay[0][0], 9))
    par = [_rand(rng, 32) for _ in range(3)]
    par = [par[0], par[1], par[0], par[2], par[1]]
    votes = _votes(rng, 7)
    fields = [None] * 7
    fields[4] = _short_key(votes[4][0])
    out = [make_vote(rng), make_header(rng, pay, par, 0), make_header(rng, pay[::-1], par[::-1], 2, votes),
           make_header(rng, pay, par, 2, votes, vote_fields=fields)]
    whole = make_vote(rng)["frame"]
    out += [dict(frame=whole[:k], kind=None) for k in range(6)]
    return out


def _sized_sets(rng, total):
    """(payload, parents) with 36 * np + 32 * nq == total, 1 <= np <= 8."""
    for np_ in range(1, 9):
        if total >= 36 * np_ and (total - 36 * np_) % 32 == 0:
            nq = (total - 36 * np_) // 32
            return [(_rand(rng, 32), rng.getrandbits(32)) for _ in range(np_)], [_rand(rng, 32) for _ in range(nq)]
    raise ValueError(total)


def stage_switch_frames(seed=22):
    """Decoding frames of every length in STAGE - 4 .. STAGE + 4: a header
    (176 + 36 np + 32 nq; a 43-character author takes one byte off, a
    64-character one adds 20) where the length's residue allows one, and a
    7-vote certificate (a header, 8, 116 a vote; each 43-character vote key
    takes one byte off) at every length.  The certificates at STAGE and STAGE
    + 4 have canonical votes throughout, and so has one of STAGE + 3 with a
    43-character author: decoded in place, its signatures sit at odd
    addresses."""
    rng = random.Random(seed)
    out = []
    for length in range(STAGE - 4, STAGE + 5):
        if length % 4 in (0, 3):
            short = length % 4 == 3
            author = _rand(rng, 32)
            pay, par = _sized_sets(rng, length + short - 176)
            h = make_header(rng, pay, par, 0, author_field=_short_key(author) if short else None)
            if short:
                h["author"] = author
            out.append(h)
        k = -length % 4  # 43-character vote keys
        votes = _votes(rng, 7)
        fields = [None] * 7
        for j in range(k):
            fields[(2 * j + 1) % 7] = _short_key(votes[(2 * j + 1) % 7][0])
        pay, par = _sized_sets(rng, length + k - 8 - 7 * VOTE_STRIDE - 176)
        out.append(make_header(rng, pay, par, 2, votes, vote_fields=fields))
    author = _rand(rng, 32)
    pay, par = _sized_sets(rng, STAGE + 3 + 1 - 8 - 7 * VOTE_STRIDE - 176)
    c = make_header(rng, pay, par, 2, _votes(rng, 7), author_field=_short_key(author))
    c["author"] = author
    out.append(c)
    author = _rand(rng, 32)  # a 64-character author: 20 bytes more, staged at exactly STAGE
    pay, par = _sized_sets(rng, STAGE - 20 - 176)
    h = make_header(rng, pay, par, 0, author_field=W.raw_key(base64.b64encode(author + _rand(rng, 16))))
    h["author"] = author
    out.append(h)
    return out


def at_every_alignment(items, seed=23):
    """Each of `items` four times, after a filler frame of 0-3 rubbish bytes
    chosen so that the item starts 0, 1, 2 and 3 bytes past a dword boundary
    of the batch.  Returns (batch, index of each placed item, its offset mod 4)."""
    rng = random.Random(seed)
    batch, at, mis = [], [], []
    off = 0
    for c in items:
        for m in range(4):
            pad = (m - off) % 4
            batch.append(dict(frame=_rand(rng, pad), kind=None))
            off += pad
            at.append(len(batch))
            mis.append(off % 4)
            batch.append(c)
            off += len(c["frame"])
    return batch, at, mis


def prefix_pool(seed=31):
    """16 short frames the prefix-sum batches are drawn from: every kind, small
    sets, 0-5 votes, a truncated and an empty frame."""
    rng = random.Random(seed)
    key = lambda: _rand(rng, 32)  # noqa: E731
    pool = [make_vote(rng), make_vote(rng),
            make_header(rng, [], [], 0), make_header(rng, [(key(), 1)], [key()], 0),
            make_header(rng, [(key(), 1), (key(), 2)], [key()], 0),
            make_header(rng, [(key(), 3)] * 2, [key()] * 2, 0)]
    for nv in range(6):
        pool.append(make_header(rng, [(key(), 7)] * (2 * (nv == 1)), [key()] * (nv == 4), 2, _votes(rng, nv)))
    pk = key()
    pool.append(make_header(rng, [], [key()], 2, [(pk, _rand(rng, 64))], vote_fields=[_short_key(pk)]))  # the walk
    pool.append(dict(frame=W.primary_message(3, W.cert_request([key(), key()], key())), kind=3))
    pool.append(dict(frame=pool[4]["frame"][:40], kind=None))
    pool.append(dict(frame=b"", kind=None))
    assert len(pool) == 16
    return pool


PREFIX_SIZES = (255, 256, 257, 65537, 2 * 65536 + 257)
PREFIX_FORCED_BLOCK = 301  # of the largest batch: every frame of the kind


def prefix_indices(n, kind, seed=32):
    """Pool indices of an n-frame batch decoded as `kind`.  Random; the largest
    batch (three block totals per thread of k_wire_scan_totals, idle threads
    behind them) is forced: its first three blocks hold no frame of the kind,
    every frame of one middle block is of the kind, and so is the last frame."""
    import numpy as np

    idx = np.random.default_rng(seed + n).integers(0, 16, n)
    if n == PREFIX_SIZES[-1]:
        pool = prefix_pool()
        mine = [i for i, c in enumerate(pool) if c["kind"] == kind]
        others = [i for i, c in enumerate(pool) if c["kind"] != kind]
        pick = np.random.default_rng(seed)
        idx[:3 * SCAN_BLOCK] = pick.choice(others, 3 * SCAN_BLOCK)
        b = PREFIX_FORCED_BLOCK * SCAN_BLOCK
        idx[b:b + SCAN_BLOCK] = pick.choice(mine, SCAN_BLOCK)
        idx[-1] = mine[-1]
    return idx


def vote_reduction_frames(seed=41):
    """Certificates of 130 votes (three rounds of lanes) whose defects meet in
    the wave-wide minimum of votes_do.  Each case carries `code`, the error the
    first defect in wire order gives (None: the frame decodes); the cases of two
    defective keys also `pair`: ((vote, code), (vote, code))."""
    rng = random.Random(seed)
    bad = malformed_keys()
    defect = {EKEY: bad["invalid character"], EFORMAT: bad["not UTF-8"]}
    assert all(len(f) == 8 + 44 for f in defect.values())  # the canonical length: the speculation holds
    votes = _votes(rng, 130)
    out = []

    def cert(fields, nv=None, cut=None, code=None, note="", pair=None):
        c = make_header(rng, [], [_rand(rng, 32)], 2, votes, vote_fields=fields)
        f = c["frame"]
        if nv is not None or cut is not None:
            at = len(f) - 130 * VOTE_STRIDE  # the first vote
            if nv is not None:
                f = f[:at - 8] + struct.pack("<Q", nv[0]) + f[at:at + nv[1] * VOTE_STRIDE]
            else:
                f = f[:at + cut]
        if code is None:
            out.append(dict(c, frame=f, code=None, note=note))
        else:
            out.append(dict(frame=f, kind=None, code=code, note=note, pair=pair))

    for a, b in ((3, 70), (70, 3), (63, 64), (64, 63), (127, 128), (128, 127)):
        for ca, cb in ((EKEY, EFORMAT), (EFORMAT, EKEY)):
            fields = [None] * 130
            fields[a], fields[b] = defect[ca], defect[cb]
            cert(fields, code=ca if a < b else cb, note=f"{ca} at {a}, {cb} at {b}", pair=((a, ca), (b, cb)))
    for cut, what in ((129 * VOTE_STRIDE + 52 + 34, "in vote 129's signature"), (129 * VOTE_STRIDE + 4, "in vote 129's length")):
        cert([None] * 130, cut=cut, code=ETRUNC, note="cut " + what)
        fields = [None] * 130
        fields[65] = defect[EKEY]
        cert(fields, cut=cut, code=EKEY, note="EKEY at 65, cut " + what)
    for pos in (0, 64):  # a 43-character key: the walk
        fields = [None] * 130
        fields[pos] = _short_key(votes[pos][0])
        cert(fields, note=f"43 characters at {pos}")
    # a count that passes nv <= rest / 72 and exceeds rest / 116: lanes ask for votes beyond the frame
    cert([None] * 130, nv=(99, 62), code=ETRUNC, note="99 votes claimed, 62 present")
    cert([None] * 130, note="canonical")
    return out


def set_frames(seed=51):
    """Payload sets (stride 36) around the wave width, its multiples and at the
    cap, in three wire orders; duplicates a whole number of lane rounds and one
    lane more or less apart; sets at the cap with few survivors."""
    rng = random.Random(seed)
    key = lambda: _rand(rng, 32)  # noqa: E731
    out = []
    k = 0
    for npay in (63, 64, 65, 127, 128, 129, MAX_ENTRIES):
        for order in ("ascending", "descending", "shuffled"):
            pay = _ordered(rng, [(key(), rng.getrandbits(32)) for _ in range(npay)], order)
            par = _ordered(rng, [key() for _ in range(k % 4)], order)
            out.append(make_header(rng, pay, par, 2 if k % 2 else 0, _votes(rng, 1 + k % 3) if k % 2 else ()))
            k += 1
    pay = [(key(), i) for i in range(192)]
    for i, dist in ((10, 1), (20, 63), (30, 64), (40, 65), (50, 128)):
        pay[i + dist] = (pay[i][0], 5000 + dist)
    for n, i in enumerate((0, 64, 128)):
        pay[i] = (pay[0][0], 7001 + n)
    out.append(dict(make_header(rng, pay, [key()], 0), note="duplicates"))
    out.append(dict(make_header(rng, pay, [key(), key()], 2, _votes(rng, 2)), note="duplicates"))
    half = [key() for _ in range(MAX_ENTRIES // 2)]
    pay = [(half[rng.randrange(len(half))] if i >= len(half) else half[i], i) for i in range(MAX_ENTRIES)]
    rng.shuffle(pay)
    out.append(dict(make_header(rng, pay, [key()], 0), note="512 of 1024"))
    three = [key() for _ in range(3)]
    par = three + [three[rng.randrange(3)] for _ in range(MAX_ENTRIES - 3)]
    rng.shuffle(par)
    out.append(dict(make_header(rng, [(key(), 1)], par, 2, _votes(rng, 3)), note="3 of 1024"))
    for variant in (0, 2):
        out.append(dict(make_header(rng, [(key(), i) for i in range(MAX_ENTRIES)], [key() for _ in range(MAX_ENTRIES)], variant,
                                    _votes(rng, 2) if variant else ()), note="both at the cap"))
    return out


def tightest_certificate(seed=61, nv=200):
    """The certificate with the fewest bytes per vote the format allows: a
    43-character author, empty sets, 43-character vote keys: 183 + 115 nv
    bytes, so a single-frame call uses all but one row of COA_WIRE_VOTES_BOUND."""
    rng = random.Random(seed)
    author = _rand(rng, 32)
    votes = _votes(rng, nv)
    c = make_header(rng, [], [], 2, votes, author_field=_short_key(author), vote_fields=[_short_key(pk) for pk, _ in votes])
    c["author"] = author
    return c


def offsets_case(seed=71):
    """Group F: (blob, slack, offsets, items).  Four valid frames A B C D lie
    back to back in `blob`; `slack` is what lies behind frame_bytes in the
    allocation: one byte, then a copy of A.  The offsets name A, B, a
    decreasing pair, B again, C, D with one slack byte (ends at frame_bytes +
    1; trailing bytes would decode), the copy of A (wholly in the slack), more
    slack, a second decreasing pair, D.  items: what each frame must decode as
    -- the frames out of range as empty frames."""
    rng = random.Random(seed)
    A = make_header(rng, [(_rand(rng, 32), 4)], [_rand(rng, 32)], 0)
    B = make_header(rng, [(_rand(rng, 32), 5)], [_rand(rng, 32)] * 2, 2, _votes(rng, 3))
    C = make_vote(rng)
    D = make_header(rng, [], [_rand(rng, 32)], 2, _votes(rng, 2))
    blob = b"".join(c["frame"] for c in (A, B, C, D))
    a = len(A["frame"])
    b = a + len(B["frame"])
    c = b + len(C["frame"])
    fb = len(blob)
    slack = b"\x00" + A["frame"]
    offsets = [0, a, b, a, b, c, fb + 1, fb + 1 + a, fb + 300, c, fb]
    empty = dict(frame=b"", kind=None)
    items = [A, B, empty, B, C, empty, empty, empty, empty, D]
    return blob, slack, offsets, items


def _layout(f):
    """Positions in a Header / Certificate frame with a well-formed front, by
    a parse of this file's own: dict(author, np_at, payload, np, nq_at,
    parents, nq, id, nv_at) or None."""
    if len(f) < 12 or f[:4] not in (b"\x00\x00\x00\x00", b"\x02\x00\x00\x00"):
        return None
    klen = struct.unpack_from("<Q", f, 4)[0]
    i = 12 + klen + 8
    if klen > 100 or i + 8 > len(f):
        return None
    np_ = struct.unpack_from("<Q", f, i)[0]
    L = dict(author=4, np_at=i, payload=i + 8, np=np_)
    i += 8 + 36 * np_
    if np_ > 5000 or i + 8 > len(f):
        return None
    nq = struct.unpack_from("<Q", f, i)[0]
    L.update(nq_at=i, parents=i + 8, nq=nq)
    i += 8 + 32 * nq
    if nq > 5000 or i + 96 > len(f):
        return None
    L.update(id=i, nv_at=i + 96 if f[0] == 2 and i + 104 <= len(f) else None)
    return L


def vote_key_fields(f):
    """Offsets of the vote key strings' length prefixes in a Certificate frame
    with a well-formed header (as far as they lie inside the frame)."""
    L = _layout(f)
    if L is None or L["nv_at"] is None:
        return []
    nv = struct.unpack_from("<Q", f, L["nv_at"])[0]
    at, pos = [], L["nv_at"] + 8
    for _ in range(min(nv, 2000)):
        if pos + 8 > len(f):
            break
        at.append(pos)
        pos += 8 + struct.unpack_from("<Q", f, pos)[0] + 64
    return at


def over_the_cap(f):
    """A Header / Certificate frame one of whose sets has more wire entries
    than the device sorts: COA_WIRE_ECAPACITY if the host decoder accepts it."""
    L = _layout(f)
    return L is not None and (L["np"] > MAX_ENTRIES or L["nq"] > MAX_ENTRIES)


def takes_the_walk(f):
    """A Certificate frame some vote key string of which is not 44 long."""
    return any(struct.unpack_from("<Q", f, p)[0] != 44 for p in vote_key_fields(f))


def differential_frames(corpus, n=4000, seed=81):
    """Group G: n frames mutated from `corpus` (the committed fuzz corpus as a
    list of bytes) and the constructed frames above.  A third stay as built or
    change only bytes that no rule reads (ids, signatures, rounds); the rest
    take one to three of: bit and byte flips, edits of a length or count prefix
    (+-1, +-64, 44, 43, 64, large), truncation, appended bytes, a splice of two
    frames, a swap of two set entries, a repeated entry."""
    rng = random.Random(seed)
    built = [c["frame"] for c in small_certificates() + key_string_frames() + mixed_frames() + alignment_frames() +
             vote_reduction_frames() + set_frames()[:21:4] + [tightest_certificate(nv=70)]]
    big = [c["frame"] for c in stage_switch_frames()]
    walkers = [c["frame"] for c in key_string_frames() + vote_reduction_frames() + [tightest_certificate(nv=9)]
               if c.get("kind") == 2 and takes_the_walk(c["frame"])]
    voters = [f for f in list(corpus) + built if f[:4] == b"\x01\x00\x00\x00" and len(f) >= 200]
    seeds = list(corpus) + built

    def prefixes(f):
        """Offsets of the u64 length and count prefixes of f."""
        L = _layout(f)
        if L is None:
            return [4] if len(f) >= 12 else []
        at = [L["author"], L["np_at"], L["nq_at"]]
        if L["nv_at"] is not None:
            at += [L["nv_at"]] + vote_key_fields(f)
        return at

    def mutate(f):
        f = bytearray(f)
        what = rng.randrange(9)
        L = _layout(bytes(f))
        if what == 0 and f:  # bit flip
            f[rng.randrange(len(f))] ^= 1 << rng.randrange(8)
        elif what == 1 and f:  # byte flip
            f[rng.randrange(len(f))] = rng.getrandbits(8)
        elif what == 2:  # a length or count prefix
            at = prefixes(bytes(f))
            if at:
                p = rng.choice(at)
                v = struct.unpack_from("<Q", f, p)[0]
                v = rng.choice([v + 1, v - 1, v + 64, v - 64, 44, 43, 64, 1 << 40, (1 << 64) - 1, len(f)]) % (1 << 64)
                struct.pack_into("<Q", f, p, v)
        elif what == 3 and f:  # truncation
            del f[rng.randrange(len(f)):]
        elif what == 4:  # appended bytes
            f += _rand(rng, rng.randrange(1, 9))
        elif what == 5:  # the front of this frame, the back of another
            g = rng.choice(seeds)
            f = bytearray(bytes(f[:rng.randrange(len(f) + 1)]) + g[rng.randrange(len(g) + 1):])
        elif what in (6, 7) and L is not None:
            base, stride, cnt = (L["payload"], 36, L["np"]) if rng.random() < 0.5 and L["np"] > 1 else (L["parents"], 32, L["nq"])
            if cnt > 1:
                i, j = rng.sample(range(cnt), 2)
                a, b = bytes(f[base + i * stride:base + (i + 1) * stride]), bytes(f[base + j * stride:base + (j + 1) * stride])
                f[base + i * stride:base + (i + 1) * stride] = b  # a repeated entry ...
                if what == 6:
                    f[base + j * stride:base + (j + 1) * stride] = a  # ... or a swap
        elif L is not None:  # bytes that no rule reads: the id and the header's signature
            f[L["id"] + rng.randrange(96)] ^= 0xff
        return bytes(f)

    out = []
    for k in range(n):
        r = k % 20
        f = rng.choice(big) if r < 1 else rng.choice(walkers) if r == 2 else rng.choice(voters) if r in (3, 4) else \
            rng.choice(seeds)
        style = rng.random()
        if r < 1 and style < 0.7:
            L = _layout(f)  # large frames mostly keep decoding: sets reordered, entries repeated
            f = bytearray(f)
            for _ in range(3):
                i, j = rng.sample(range(L["nq"]), 2)
                f[L["parents"] + 32 * i:L["parents"] + 32 * i + 32] = f[L["parents"] + 32 * j:L["parents"] + 32 * j + 32]
            f = bytes(f)
        elif style < 0.35:
            L = _layout(f)
            if L is not None:
                f = bytearray(f)
                f[L["id"] + rng.randrange(96)] ^= 1 << rng.randrange(8)
                f = bytes(f)
        else:
            for _ in range(rng.randrange(1, 4)):
                f = mutate(f)
        out.append(dict(frame=f, kind=None))
    return out


def all_constructed():
    return (small_certificates() + boundary_frames() + key_string_frames() + error_frames() + mixed_frames() +
            alignment_frames() + stage_switch_frames() + prefix_pool() + vote_reduction_frames() + set_frames() +
            [tightest_certificate()] + offsets_case()[3])

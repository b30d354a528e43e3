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


def all_constructed():
    return small_certificates() + boundary_frames() + key_string_frames() + error_frames() + mixed_frames()

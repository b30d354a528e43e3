"""Test infrastructure: certificates, headers and votes for the verdict calls
(coa_*_verdict_many: Certificate::verify / Header::verify / Vote::verify
decided by the engine, protocol checks included) with the word each must get.

Nothing here comes from the engine.  The cases are built with the Python
reference (oracle/ed25519_ref.py) around tests/message_cases.World; the
expected word is a plain restatement of primary/src/messages.rs:48-67,
131-142, 189-215 whose crypto facts are hashlib's SHA-512 and the C
restatement of dalek (oracle/coa_oracle.py: certificate_verify_many with
explicit weights, verify_strict_many).  A certificate whose answer reaches
verify_batch (:214) is only used when the oracle's bits agree under two
different weight vectors (asserted below).

Committee: 72 keys -- 69 honest (World's 10 first), the mixed-order,
small-order and off-curve members -- with stakes 1, 2, 3, ... (honest member
Z = 4 has stake 0) and worker sets that differ per authority; one outsider.
"""
import functools
import hashlib
import random
import struct

import numpy as np

import coa_oracle as co
import ed25519_ref as o
import message_cases as mc

N_HONEST = 69
Z = 4  # the honest member with stake 0
OK, BAD_ID, UNKNOWN_AUTHOR, MALFORMED, BAD_SIG, REUSE, UNKNOWN_VOTER, QUORUM, BAD_VOTES, OPEN = range(10)
ROUND = 5


def word(code, index=0):
    return code | (index << 8)


class Committee72:
    def __init__(self):
        self.w = mc.World()
        self.seeds = list(self.w.seeds) + [o.sha512(b"coa-key" + struct.pack("<Q", 7100 + i))[:32]
                                           for i in range(N_HONEST - len(self.w.seeds))]
        self.honest = [o.public_key(s) for s in self.seeds]
        assert self.honest[:10] == self.w.pks
        self.members = self.honest + [self.w.mx_pk, self.w.small_pk, self.w.off_pk]
        self.stakes = [0 if i == Z else i + 1 for i in range(N_HONEST)] + [2, 3, 1]
        self.workers = [[i, 1000 + i, 7] for i in range(N_HONEST)] + [[500], [501, 7], [502]]
        self.stake_of = dict(zip(self.members, self.stakes))
        self.workers_of = dict(zip(self.members, self.workers))
        self.total = sum(self.stakes)
        self.quorum = 2 * self.total // 3 + 1
        self.seed_of = dict(zip(self.honest, self.seeds))
        self.seed_of[self.w.out_pk] = self.w.out_seed
        # honest members with stake, heaviest first
        self.plain = sorted((i for i in range(N_HONEST) if i != Z), key=lambda i: -self.stakes[i])

    def arrays(self):
        """(pks [72, 32], stakes, workers) in member order (not sorted)."""
        return np.array([list(k) for k in self.members], np.uint8), list(self.stakes), [list(x) for x in self.workers]

    @functools.lru_cache(maxsize=None)
    def sign(self, pk, msg):
        return o.sign(self.seed_of[pk], msg)

    def subset_with_weight(self, target):
        """Plain voters whose stakes sum to exactly `target`."""
        out, left = [], target
        for i in self.plain:
            if self.stakes[i] <= left:
                out.append(i)
                left -= self.stakes[i]
        assert left == 0, (target, left)
        return out


@functools.lru_cache(maxsize=None)
def committee():
    return Committee72()


def header_bytes(author, payload, parents, round_=ROUND):
    """Header::digest input: author | round LE | (digest | worker id LE)* | parents*."""
    out = bytearray(author) + struct.pack("<Q", round_)
    for d, wid in payload:
        out += d + struct.pack("<I", wid)
    for p in parents:
        out += p
    return bytes(out)


def cert_digest(id_, round_, origin):
    return hashlib.sha512(bytes(id_) + struct.pack("<Q", round_) + bytes(origin)).digest()[:32]


def _flip(b, i, bit=1):
    x = bytearray(b)
    x[i] ^= bit
    return bytes(x)


def _digests(tag, n):
    return sorted(o.sha512(tag + bytes([k]))[:32] for k in range(n))


class Builder:
    """Certificates around a few headers; vote signatures cached per digest."""

    def __init__(self):
        self.c = committee()
        self.cases = []

    def header(self, author, wids, tag=b"h", round_=ROUND):
        payload = list(zip(_digests(b"batch" + tag, len(wids)), wids))
        hdr = header_bytes(author, payload, _digests(b"parent" + tag, 3), round_)
        id_ = hashlib.sha512(hdr).digest()[:32]
        sig = self.c.sign(author, id_) if author in self.c.seed_of else bytes(64)
        return {"hdr": hdr, "id": id_, "origin": author, "hsig": sig, "round": round_, "count": len(wids),
                "payload": payload}

    def votes(self, h, voters):
        d = cert_digest(h["id"], h["round"], h["origin"])
        return [(pk, self.c.sign(pk, d)) for pk in voters]

    def add(self, name, h, votes, **over):
        case = dict(h, name=name, votes=list(votes))
        case.update(over)
        self.cases.append(case)
        return case


@functools.lru_cache(maxsize=None)
def certificate_cases():
    b = Builder()
    c, w = b.c, b.c.w
    H = c.honest
    a0 = H[0]
    rng = random.Random(11)
    quorum_voters = [H[i] for i in c.plain[:30]]
    assert sum(c.stake_of[k] for k in quorum_voters) >= c.quorum
    h0 = b.header(a0, [0, 1000])
    all_plain = [H[i] for i in c.plain]                      # 68 voters
    d0 = cert_digest(h0["id"], ROUND, a0)
    garbage = [(H[1], bytes(range(64))), (w.out_pk, bytes(64)), (H[1], bytes(range(64)))]

    # vote counts over two lane strides
    for n in (0, 1, 63, 64, 65, 68):
        b.add(f"votes_{n}", h0, b.votes(h0, all_plain[:n]))
    v70 = b.votes(h0, all_plain + [H[Z], w.out_pk])
    b.add("votes_70_stake0_then_outsider", h0, v70)          # UNKNOWN_VOTER at 68
    # the same certificate clean, with a reuse, clean again (one block's waves share slots)
    v65 = b.votes(h0, all_plain[:65])
    b.add("clean_a", h0, v65)
    b.add("reuse_stride0_3_9", h0, v65[:9] + [v65[3]] + v65[10:])
    b.add("clean_b", h0, v65)
    v70p = b.votes(h0, all_plain) + [v65[0], v65[1]]
    b.add("reuse_across_strides_3_67", h0, v70p[:67] + [v70p[3]] + v70p[68:])
    b.add("reuse_stride1_64_66", h0, v70p[:66] + [v70p[64]] + v70p[67:68])
    A, X = b.votes(h0, [H[1]])[0], b.votes(h0, [w.out_pk])[0]
    b.add("order_AA", h0, [A, A])
    b.add("order_XX", h0, [X, X])
    b.add("order_AXA", h0, [A, X, A])
    b.add("order_AAX", h0, [A, A, X])
    zv = b.votes(h0, [H[Z]])[0]
    b.add("stake0_voter", h0, v65[:40] + [zv] + v65[41:])
    b.add("stake0_voter_twice", h0, [zv, zv])
    b.add("weight_at_quorum", h0, b.votes(h0, [H[i] for i in c.subset_with_weight(c.quorum)]))
    b.add("weight_one_below", h0, b.votes(h0, [H[i] for i in c.subset_with_weight(c.quorum - 1)]))
    # invalid votes that dalek rejects under any weights
    qv = b.votes(h0, quorum_voters)
    b.add("one_vote_s_flip", h0, [qv[0], (qv[1][0], _flip(qv[1][1], 40))] + qv[2:])
    b.add("one_vote_s_plus_l", h0, qv[:7] + [(qv[7][0], mc._bump_s(qv[7][1], o.L))] + qv[8:])
    # a torsion voter, behind an earlier failure
    mx = (w.mx_pk, w.mixed_sign(d0, rng))
    b.add("mixed_voter_and_reuse", h0, [qv[0], mx, qv[0]] + qv[1:])

    # header checks: payload counts 0, 1, 32; foreign worker ids
    for n, wids in ((0, []), (1, [7]), (32, [0, 1000, 7] * 10 + [0, 7])):
        h = b.header(a0, wids, tag=b"p%d" % n)
        b.add(f"payload_{n}", h, b.votes(h, quorum_voters))
    b.add("foreign_worker_first", b.header(a0, [9999] + [0] * 31, tag=b"f"), garbage)
    b.add("foreign_worker_last", b.header(a0, [0] * 31 + [9999], tag=b"l"), garbage)
    b.add("worker_of_another_authority", b.header(a0, [0, 1], tag=b"o"), garbage)
    b.add("stake0_author", b.header(H[Z], [Z], tag=b"z"), garbage)
    hx = b.header(w.out_pk, [0], tag=b"x")
    b.add("outsider_author", hx, b.votes(hx, quorum_voters))

    # genesis
    gen = {"hdr": header_bytes(a0, [], [], 0), "id": bytes(32), "origin": a0, "hsig": bytes(range(64)), "round": 0,
           "count": 0, "payload": []}
    b.add("genesis_garbage", gen, garbage)
    b.add("genesis_stake0_origin", dict(gen, hdr=header_bytes(H[Z], [], [], 0), origin=H[Z]), garbage)
    b.add("genesis_outsider_origin", dict(gen, hdr=header_bytes(w.out_pk, [], [], 0), origin=w.out_pk), garbage)
    b.add("zero_id_round_1", dict(gen, hdr=header_bytes(a0, [], [], 1), round=1), garbage)

    # order: every set of one, two or all of the eight checks failing at once
    flags = ("bad_id", "unknown_author", "malformed", "bad_hsig", "reuse", "unknown_voter", "low_weight",
             "bad_votes")
    combos = [(f,) for f in flags] + [(f, g) for i, f in enumerate(flags) for g in flags[i + 1:]] + [flags]
    for combo in combos:
        author = w.out_pk if "unknown_author" in combo else a0
        h = b.header(author, [0, 4242] if "malformed" in combo else [0, 1000],
                     tag=b"c" + bytes([int("unknown_author" in combo), int("malformed" in combo)]))
        v = b.votes(h, quorum_voters)
        if "low_weight" in combo:
            v = v[:12]
        if "bad_votes" in combo:
            v[1] = (v[1][0], _flip(v[1][1], 40))
        if "unknown_voter" in combo:
            v[5] = b.votes(h, [w.out_pk])[0]
        if "reuse" in combo:
            v[9] = v[3]
        over = {}
        if "bad_id" in combo:
            over["hdr"] = _flip(h["hdr"], len(h["hdr"]) - 1)  # in the parents: worker ids and author stay
        if "bad_hsig" in combo:
            over["hsig"] = _flip(h["hsig"], 40)
        b.add("fail_" + "+".join(combo), h, v, **over)
    return tuple(b.cases)


def certificate_arrays(cases):
    """The arguments of coa_crypto.certificate_verdict_many (without rng_seed)."""
    vp = np.array([list(pk) for c in cases for pk, _ in c["votes"]], np.uint8).reshape(-1, 32)
    vs = np.array([list(sg) for c in cases for _, sg in c["votes"]], np.uint8).reshape(-1, 64)
    off = np.zeros(len(cases) + 1, np.uint64)
    off[1:] = np.cumsum([len(c["votes"]) for c in cases])
    return ([c["hdr"] for c in cases], mc._rows(cases, "id", 32), mc._rows(cases, "origin", 32),
            mc._rows(cases, "hsig", 64), np.array([c["round"] for c in cases], np.uint64), vp, vs, off,
            [c["count"] for c in cases])


def _header_word(c, hdr, count, author, bad_id, bad_sig):
    if bad_id:                                               # messages.rs:50
        return BAD_ID
    if c.stake_of.get(author, 0) <= 0:                       # :53-54
        return UNKNOWN_AUTHOR
    for k in range(count):                                   # :57-61
        at = 40 + 36 * k + 32
        if struct.unpack("<I", hdr[at:at + 4])[0] not in c.workers_of[author]:
            return MALFORMED
    if bad_sig:                                              # :64-66
        return BAD_SIG
    return OK


def _certificate_word(c, case, bits):
    """(word, reaches verify_batch)."""
    if case["id"] == bytes(32) and case["round"] == 0 and case["origin"] in c.stake_of:  # :190-193
        return OK, False
    h = _header_word(c, case["hdr"], case["count"], case["origin"], bits & 1, bits & 2)
    if h:
        return h, False
    weight, used = 0, set()
    for j, (name, _) in enumerate(case["votes"]):            # :201-207
        if name in used:
            return word(REUSE, j), False
        if c.stake_of.get(name, 0) <= 0:
            return word(UNKNOWN_VOTER, j), False
        used.add(name)
        weight += c.stake_of[name]
    if weight < c.quorum:                                    # :208-211
        return QUORUM, False
    return (BAD_VOTES if bits & 4 else OK), True             # :214


@functools.lru_cache(maxsize=None)
def expected_certificates():
    """(words uint32 [n], open_allowed bool [n]) for certificate_cases().
    open_allowed: the device-resident form may answer VOTES_OPEN -- the
    answer is verify_batch's and some vote does not hold its own equation or
    is by a key with torsion."""
    cases = certificate_cases()
    c = committee()
    a = certificate_arrays(cases)
    nv = int(a[7][-1])
    rng = np.random.default_rng(3)
    bits = [co.certificate_verify_many(*a[:8], rng.integers(0, 256, (max(nv, 1), 16), dtype=np.uint8))
            for _ in range(2)]
    words, open_ok = [], []
    torsion = {c.w.mx_pk, c.w.small_pk, c.w.off_pk}
    for i, case in enumerate(cases):
        w0, reaches = _certificate_word(c, case, int(bits[0][i]))
        w1, _ = _certificate_word(c, case, int(bits[1][i]))
        assert w0 == w1, f"{case['name']}: weight-dependent answer, not a usable case"
        d = cert_digest(case["id"], case["round"], case["origin"])
        inexact = any(pk in torsion or not o.verify_equation_cofactorless(d, pk, sg) for pk, sg in case["votes"]) \
            if reaches else False
        words.append(w0)
        open_ok.append(bool(reaches and inexact))
    return np.array(words, np.uint32), np.array(open_ok, bool)


# ------------------------------------------------------- headers and votes
@functools.lru_cache(maxsize=None)
def header_cases():
    """message_cases.header_cases with a payload count attached (the bytes
    are random, so a counted worker id is almost surely foreign), and headers
    with well-formed payloads by a member, a stake-0 member and an outsider."""
    c = committee()
    out = []
    for i, h in enumerate(mc.header_cases(c.w)):
        fit = (len(h["hdr"]) - 40) // 36
        out.append(dict(h, count=min(fit, (0, 1, 3)[i % 3])))
    b = Builder()
    for name, author, wids in (("payload_0", c.honest[2], []), ("payload_1", c.honest[2], [1002]),
                               ("payload_32", c.honest[2], [2, 7] * 16), ("foreign_first", c.honest[2], [3] + [2] * 31),
                               ("foreign_last", c.honest[2], [2] * 31 + [1003]), ("stake0", c.honest[Z], [Z]),
                               ("outsider", c.w.out_pk, [0]), ("mixed_member", c.w.mx_pk, [500])):
        h = b.header(author, wids, tag=b"m" + name.encode())
        sig = h["hsig"] if author != c.w.mx_pk else c.w.mixed_sign(h["id"], random.Random(2))
        out.append({"name": name, "hdr": h["hdr"], "id": h["id"], "author": author, "sig": sig, "count": h["count"]})
        out.append({"name": name + "_bad_sig", "hdr": h["hdr"], "id": h["id"], "author": author,
                    "sig": _flip(sig, 40), "count": h["count"]})
        out.append({"name": name + "_bad_id", "hdr": _flip(h["hdr"], 1), "id": h["id"], "author": author, "sig": sig,
                    "count": h["count"]})
    return tuple(out)


def header_arrays(cases):
    a = mc.header_arrays(cases)
    return a["header_inputs"], a["ids"], a["authors"], a["sigs"], [c["count"] for c in cases]


@functools.lru_cache(maxsize=None)
def expected_headers():
    cases, c = header_cases(), committee()
    bits = mc.expected_headers(cases)
    return np.array([_header_word(c, h["hdr"], h["count"], h["author"], bits[i] & 1, bits[i] & 2)
                     for i, h in enumerate(cases)], np.uint32)


@functools.lru_cache(maxsize=None)
def vote_cases():
    return tuple(mc.vote_cases(committee().w))


def vote_arrays(cases):
    a = mc.vote_arrays(cases)
    return a["ids"], a["rounds"], a["origins"], a["authors"], a["sigs"]


@functools.lru_cache(maxsize=None)
def expected_votes():
    cases, c = vote_cases(), committee()
    bad = mc.expected_votes(cases)
    return np.array([UNKNOWN_AUTHOR if c.stake_of.get(v["author"], 0) <= 0 else (BAD_SIG if bad[i] else OK)
                     for i, v in enumerate(cases)], np.uint32)


# ------------------------------------------ the case file of the C / C++ drivers
def write_case_file(path):
    """Every case with its expected word in the flat binary form that
    tests/sanitize/verdict_driver.cpp and tests/c_abi/verdict_harness.c read
    (little endian; arrays as the C ABI takes them):
      "VRDC" | u32 na | pks | stakes u32 | worker offsets u64 [na + 1] | worker ids u32
      u32 nc | u64 header bytes | u64 votes | header offsets u64 [nc + 1] | header data | ids | origins |
        header sigs | rounds u64 | vote offsets u64 [nc + 1] | vote pks | vote sigs | payload counts u32 | expect u32
      u32 nh | u64 header bytes | header offsets | header data | ids | authors | sigs | payload counts | expect
      u32 nv | ids | rounds u64 | origins | authors | sigs | expect"""
    c = committee()
    pks, stakes, workers = c.arrays()
    woff = np.zeros(len(workers) + 1, np.uint64)
    woff[1:] = np.cumsum([len(x) for x in workers])
    out = [b"VRDC", struct.pack("<I", len(stakes)), pks.tobytes(), np.array(stakes, np.uint32).tobytes(), woff.tobytes(),
           np.array([x for ws in workers for x in ws], np.uint32).tobytes()]

    def headers(hs):
        off = np.zeros(len(hs) + 1, np.uint64)
        off[1:] = np.cumsum([len(h) for h in hs])
        return struct.pack("<Q", int(off[-1])), off.tobytes() + b"".join(hs)

    cases = certificate_cases()
    h, ids, origins, hsigs, rounds, vp, vs, off, counts = certificate_arrays(cases)
    hb, hrest = headers(h)
    out += [struct.pack("<I", len(cases)), hb, struct.pack("<Q", vp.shape[0]), hrest, ids.tobytes(), origins.tobytes(),
            hsigs.tobytes(), rounds.tobytes(), off.tobytes(), vp.tobytes(), vs.tobytes(),
            np.array(counts, np.uint32).tobytes(), expected_certificates()[0].tobytes()]
    hc = header_cases()
    h, ids, authors, sigs, counts = header_arrays(hc)
    hb, hrest = headers(h)
    out += [struct.pack("<I", len(hc)), hb, hrest, ids.tobytes(), authors.tobytes(), sigs.tobytes(),
            np.array(counts, np.uint32).tobytes(), expected_headers().tobytes()]
    vt = vote_cases()
    ids, rounds, origins, authors, sigs = vote_arrays(vt)
    out += [struct.pack("<I", len(vt)), ids.tobytes(), rounds.tobytes(), origins.tobytes(), authors.tobytes(),
            sigs.tobytes(), expected_votes().tobytes()]
    with open(path, "wb") as f:
        f.write(b"".join(out))
    return len(cases), len(hc), len(vt)


# ------------------------------------------------- the objects of certificates.py
def as_objects(cases):
    """certificates.Committee and Certificate objects of the cases."""
    import certificates as cz
    from coa_crypto import Digest, PublicKey, Signature

    c = committee()
    com = cz.Committee(dict(zip(c.members, c.stakes)), {k: set(v) for k, v in zip(c.members, c.workers)})
    out = []
    for case in cases:
        h = cz.Header(PublicKey(case["origin"]), case["round"], {Digest(d): wid for d, wid in case["payload"]}, set(),
                      Digest(case["id"]), Signature.from_bytes(case["hsig"]))
        h._digest_input = case["hdr"]
        out.append(cz.Certificate(h, [(PublicKey(pk), Signature.from_bytes(sg)) for pk, sg in case["votes"]]))
    return com, out

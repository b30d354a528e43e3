"""Test infrastructure: Header / Vote messages with honest and adversarial
signatures for the Header::verify / Vote::verify crypto entry points
(tests/test_cpu_messages.py, tests/test_gpu_messages.py).

Everything is built with the Python reference (oracle/ed25519_ref.py) and
hashlib; the expected outputs come from hashlib.sha512 and the C restatement
of dalek (oracle/coa_oracle.py verify_strict), never from the engine:
  header status = (sha512(hdr)[:32] != id) | 2 * (!verify_strict(id, author, sig))
  vote verdict  = !verify_strict(sha512(id || round LE || origin)[:32], author, sig)

The committee is the one of tests/test_gpu_committee.py's World: 10 honest
keys, a mixed-order member A = aB + T8 with known a, a small-order key and an
off-curve key (all registered), and one honest outsider that is not."""
import hashlib
import random
import struct

import numpy as np

import coa_oracle as co
import ed25519_ref as o
from conftest import load_golden

L_ORDER = o.L
HEADER_LENGTHS = (40, 72, 111, 112, 128, 239, 240, 1000, 3336)


def _golden(cls):
    return [v for v in load_golden("verify_vectors.json") if v["class"] == cls]


def _flip(b, i, bit=1):
    x = bytearray(b)
    x[i] ^= bit
    return bytes(x)


def _bump_s(sig, delta):
    s = (int.from_bytes(sig[32:], "little") + delta) % (1 << 256)
    return sig[:32] + s.to_bytes(32, "little")


def vote_digest(id_, round_, origin):
    return hashlib.sha512(bytes(id_) + struct.pack("<Q", round_) + bytes(origin)).digest()[:32]


class World:
    def __init__(self, n_honest=10):
        self.seeds = [o.sha512(b"coa-key" + struct.pack("<Q", 7000 + i))[:32] for i in range(n_honest)]
        self.pks = [o.public_key(s) for s in self.seeds]
        self.T8 = next(T for T in o.torsion_points() if not o.is_identity(o.pdbl(o.pdbl(T))))
        self.mx_seed = o.sha512(b"mixed-member")[:32]
        self.mx_a, _ = o.expand_seed(self.mx_seed)
        self.mx_pk = o.compress(o.padd(o.pmul(self.mx_a, o.B), self.T8))
        self.small_pk = bytes.fromhex(_golden("small_order_A")[0]["pk"])
        self.off_pk = next(bytes.fromhex(v["pk"]) for v in _golden("off_curve")
                           if o.decompress(bytes.fromhex(v["pk"])) is None)
        self.out_seed = o.sha512(b"outsider")[:32]
        self.out_pk = o.public_key(self.out_seed)
        self.registered = self.pks + [self.mx_pk, self.small_pk, self.off_pk]
        self.so_r = o.small_order_encodings()[3]
        self.off_r = next(bytes.fromhex(v["sig"])[:32] for v in _golden("off_curve")
                          if o.decompress(bytes.fromhex(v["sig"])[:32]) is None)
        self.nc_r = bytes.fromhex(_golden("noncanonical_R")[0]["sig"])[:32]

    def registered_array(self):
        return np.array([list(k) for k in self.registered], np.uint8)

    def mixed_sign(self, msg, rng):
        """A signature by the mixed-order member whose R absorbs the torsion:
        the cofactorless equation holds, so verify_strict accepts."""
        while True:
            r = rng.getrandbits(256) % L_ORDER
            for j in range(8):
                Rb = o.compress(o.padd(o.pmul(r, o.B), o.pmul(j, self.T8)))
                k = o.scalar_from_hash(o.sha512(Rb + self.mx_pk + msg))
                if (j + k) % 8 == 0:
                    return Rb + ((r + k * self.mx_a) % L_ORDER).to_bytes(32, "little")

    def identity_r_sign(self, seed, msg):
        """R = identity, s = k a: [s]B - [k]A == R, which verify_strict
        rejects (small-order R)."""
        a, _ = o.expand_seed(seed)
        A = o.compress(o.pmul(a, o.B))
        Rb = o.compress(o.IDENT)
        k = o.scalar_from_hash(o.sha512(Rb + A + msg))
        return Rb + (k * a % L_ORDER).to_bytes(32, "little")

    def small_order_key_sign(self, msg, rng):
        """(R, s) that satisfies [s]B - [k]A == R under the registered
        small-order key A: only verify_strict's small-order test of A rejects."""
        A = o.decompress(self.small_pk)
        while True:
            r = rng.getrandbits(256) % L_ORDER
            for j in range(8):
                Rb = o.compress(o.padd(o.pmul(r, o.B), o.pmul(j, A)))
                k = o.scalar_from_hash(o.sha512(Rb + self.small_pk + msg))
                if o.is_identity(o.pmul(j + k, A)):
                    return Rb + r.to_bytes(32, "little")

    # a signature over msg in each adversarial class: name -> (author, sig)
    def signature_cases(self, msg, i, rng):
        a = i % len(self.seeds)
        good = o.sign(self.seeds[a], msg)
        return {
            "valid": (self.pks[a], good),
            "s_flip": (self.pks[a], _flip(good, 40)),
            "s_plus_l": (self.pks[a], _bump_s(good, L_ORDER)),
            "small_r": (self.pks[a], self.so_r + good[32:]),
            "identity_r": (self.pks[a], self.identity_r_sign(self.seeds[a], msg)),
            "off_curve_r": (self.pks[a], self.off_r + good[32:]),
            "noncanonical_r": (self.pks[a], self.nc_r + good[32:]),
            "other_member": (self.pks[a], o.sign(self.seeds[(a + 1) % len(self.seeds)], msg)),
            "mixed_author": (self.mx_pk, self.mixed_sign(msg, rng)),
            "small_author": (self.small_pk, good),
            "small_author_eq": (self.small_pk, self.small_order_key_sign(msg, rng)),
            "off_curve_author": (self.off_pk, good),
            "outsider_valid": (self.out_pk, o.sign(self.out_seed, msg)),
            "outsider_invalid": (self.out_pk, _flip(o.sign(self.out_seed, msg), 33)),
        }


def vote_cases(w, rounds=2, seed=5):
    """`rounds` passes over every vote case: dicts name, id, round, origin,
    author, sig.  The message mutations (wrong round / origin, flipped id)
    change what the engine hashes while the signature stays that of the
    original vote."""
    rng = random.Random(seed)
    out = []
    for p in range(rounds):
        for i in range(3):
            id_ = o.sha512(b"voted-header" + bytes([p, i]))[:32]
            rnd = 3 + 1000003 * p + ((1 << 40) if i == 2 else 0)
            origin = w.pks[(i + p) % len(w.pks)]
            msg = vote_digest(id_, rnd, origin)
            for name, (author, sig) in w.signature_cases(msg, i + 3 * p, rng).items():
                out.append({"name": name, "id": id_, "round": rnd, "origin": origin, "author": author, "sig": sig})
            a = (i + 5) % len(w.seeds)
            good = o.sign(w.seeds[a], msg)
            out.append({"name": "wrong_round", "id": id_, "round": rnd + 1, "origin": origin, "author": w.pks[a],
                        "sig": good})
            out.append({"name": "wrong_origin", "id": id_, "round": rnd, "origin": w.pks[(i + p + 1) % len(w.pks)],
                        "author": w.pks[a], "sig": good})
            out.append({"name": "id_flip", "id": _flip(id_, 7), "round": rnd, "origin": origin, "author": w.pks[a],
                        "sig": good})
    return out


def header_cases(w, seed=6):
    """One pass over every header case at every length of HEADER_LENGTHS:
    dicts name, hdr (the Header::digest bytes), id, author, sig."""
    rng = random.Random(seed)
    out = []
    for li, n in enumerate(HEADER_LENGTHS):
        hdr = bytes(rng.getrandbits(8) for _ in range(n))
        id_ = hashlib.sha512(hdr).digest()[:32]
        sigs = w.signature_cases(id_, li, rng)
        for name, (author, sig) in sigs.items():
            out.append({"name": name, "hdr": hdr, "id": id_, "author": author, "sig": sig})
        author, good = sigs["valid"]
        out.append({"name": "hdr_flip", "hdr": _flip(hdr, n // 2), "id": id_, "author": author, "sig": good})
        out.append({"name": "hdr_flip_last", "hdr": _flip(hdr, n - 1, 0x80), "id": id_, "author": author, "sig": good})
        out.append({"name": "both", "hdr": _flip(hdr, 0), "id": id_, "author": author, "sig": sigs["s_flip"][1]})
        out.append({"name": "both_outsider", "hdr": _flip(hdr, 1), "id": id_, "author": w.out_pk,
                    "sig": sigs["outsider_invalid"][1]})
    return out


def _rows(items, key, width):
    return np.array([list(x[key]) for x in items], np.uint8).reshape(-1, width)


def vote_arrays(cases):
    return {"ids": _rows(cases, "id", 32), "rounds": np.array([c["round"] for c in cases], np.uint64),
            "origins": _rows(cases, "origin", 32), "authors": _rows(cases, "author", 32),
            "sigs": _rows(cases, "sig", 64)}


def header_arrays(cases):
    return {"header_inputs": [c["hdr"] for c in cases], "ids": _rows(cases, "id", 32),
            "authors": _rows(cases, "author", 32), "sigs": _rows(cases, "sig", 64)}


def expected_votes(cases):
    a = vote_arrays(cases)
    msgs = np.array([list(vote_digest(c["id"], c["round"], c["origin"])) for c in cases], np.uint8)
    return co.verify_strict_many(msgs, a["authors"], a["sigs"])


def expected_headers(cases):
    a = header_arrays(cases)
    bad_sig = co.verify_strict_many(a["ids"], a["authors"], a["sigs"])
    bad_id = np.array([hashlib.sha512(c["hdr"]).digest()[:32] != c["id"] for c in cases], np.uint8)
    return (bad_id | (bad_sig << 1)).astype(np.uint8)


def take(cases, n):
    """n cases, cycling through the list."""
    return [cases[i % len(cases)] for i in range(n)]

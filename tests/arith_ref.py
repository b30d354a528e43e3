"""Big-integer references, path predicates and operand builders for the
device arithmetic primitives (csrc/coa_fe.h, coa_fe_wave.h, coa_sc.h,
coa_halve.h, coa_ge.h) as exposed by tests/arith/arith_check.hip.

Three kinds of thing live here, and they are kept apart on purpose:

* REFERENCES compute the expected value of a primitive with Python integers
  (and, for everything on the curve, with oracle/ed25519_ref.py).  They never
  look at limbs.
* PATH PREDICATES are small limb-level models of the carry chains.  They say
  which path an operand takes (the common one, the rare second pass, the carry
  out of the second pass; the number of final subtractions of l; the number of
  ripple passes of a row normalisation).  They are used only to CHOOSE and
  COUNT operands -- never to produce an expected value -- so a mistake in one
  shows as a coverage floor that fails (tests/test_arith_operands.py), not as a
  wrong verdict on the kernel.
* OPERAND BUILDERS construct operands that take each path on purpose; random
  data does not reach them (2^-21 .. 2^-26 per lane for the second pass, never
  for its carry out).

Used by tests/test_arith_operands.py (CPU) and tests/test_gpu_arith.py (GPU).
"""
import functools
import random
from collections import namedtuple

import ed25519_ref as o

P = o.P
L = o.L
M32 = 0xFFFFFFFF
B256 = 1 << 256
SENTINEL = 0xA5A5A5A5

# ---------------------------------------------------------------------------
# The ops of tests/arith/arith_check.hip, in the order of its enum.
#   na/nb/nc/nout: 32-bit words per item; rows: one item per 16-lane row.
# ---------------------------------------------------------------------------
Op = namedtuple("Op", "id name na nb nc nout rows")
_OPS = [
    ("fe_add", 8, 8, 0, 8, 0), ("fe_sub", 8, 8, 0, 8, 0), ("fe_addsub", 8, 8, 0, 16, 0), ("fe_neg", 8, 0, 0, 8, 0),
    ("fe_mul", 8, 8, 0, 8, 0), ("fe_sq", 8, 0, 0, 8, 0), ("fe_mul_n4", 8, 8, 8, 32, 0), ("fe_sq_n4", 8, 8, 8, 32, 0),
    ("fe_reduce512", 16, 0, 0, 8, 0), ("fe_mul_small", 8, 1, 0, 8, 0), ("fe_fold_word", 8, 1, 0, 8, 0),
    ("fe_canon", 8, 0, 0, 8, 0), ("fe_to_words", 8, 0, 0, 8, 0), ("fe_iszero", 8, 0, 0, 1, 0),
    ("fe_isneg", 8, 0, 0, 1, 0), ("fe_eq", 8, 8, 0, 1, 0), ("fe_from_words", 8, 0, 0, 8, 0),
    ("fe_pow_p58", 8, 0, 0, 8, 0), ("fe_invert", 8, 0, 0, 8, 0), ("fe_sqrt_ratio", 8, 8, 0, 9, 0),
    ("fw_add", 8, 8, 0, 8, 1), ("fw_sub", 8, 8, 0, 8, 1), ("fw_mul", 8, 8, 0, 8, 1), ("fw_sq", 8, 0, 0, 8, 1),
    ("fw_pow_p58", 8, 0, 0, 8, 1), ("fw_invert", 8, 0, 0, 8, 1), ("fw_sqrt_ratio", 8, 8, 0, 9, 1),
    ("sc_is_canonical", 8, 0, 0, 1, 0), ("sc_reduce512", 16, 0, 0, 8, 0), ("sc_muladd", 8, 8, 8, 8, 0),
    ("sc_mul", 8, 8, 0, 8, 0), ("sc_add", 8, 8, 0, 8, 0), ("sc_neg", 8, 0, 0, 8, 0),
    ("halve", 8, 0, 0, 18, 0),
    ("ge_add", 32, 32, 0, 32, 0), ("ge_sub", 32, 32, 0, 32, 0), ("ge_madd", 32, 24, 0, 32, 0),
    ("ge_p2_dbl", 32, 0, 0, 32, 0), ("ge_p3_dbl", 32, 0, 0, 32, 0), ("ge_add_il", 32, 32, 0, 32, 0),
    ("ge_madd_il", 32, 24, 0, 32, 0), ("ge_p2_dbl_il", 32, 0, 0, 32, 0), ("ge_p3_to_cached", 32, 0, 0, 32, 0),
    ("ge_is_small_order", 32, 0, 0, 1, 0), ("ge_p2_is_identity", 32, 0, 0, 1, 0), ("ge_p2_eq_p3", 32, 32, 0, 1, 0),
    ("ge_p2_compress", 32, 0, 0, 8, 0), ("ge_decompress", 8, 0, 0, 25, 0),
]
OPS = {t[0]: Op(i, *t) for i, t in enumerate(_OPS)}

# Ops whose operand set must hold at least FLOOR operands on each listed path
# class (tests/test_arith_operands.py).  sc_reduce512 class 2 is the issue's
# one exception: see SC_REDUCE_TWO_SUBS below.
FLOOR = 64
PATH_CLASSES = {
    "fe_add": (0, 1, 2), "fe_sub": (0, 1, 2), "fe_addsub": (0, 1, 2), "fe_reduce512": (0, 1, 2),
    "fe_mul": (0, 1, 2), "fe_sq": (0, 1, 2), "fe_mul_n4": (0, 1, 2), "fe_sq_n4": (0, 1, 2),
    "sc_reduce512": (0, 1), "fw_add": (0, 1), "fw_sub": (0, 1), "fw_mul": (0, 1), "fw_sq": (0, 1),
}

# One operand tuple: a, b, c are Python integers (None where the op has no
# such operand), cls the path class by the predicate (0 where the op has
# none), rare whether the layouts treat it as a rare-path / structured operand,
# rand whether it was drawn at random (it may still land on a rare path).
Item = namedtuple("Item", "a b c cls rare rand")


def words(v, n=8):
    assert 0 <= v < 1 << (32 * n), hex(v)
    return [(v >> (32 * i)) & M32 for i in range(n)]


def from_words(ws):
    return sum(int(w) << (32 * i) for i, w in enumerate(ws))


# ---------------------------------------------------------------------------
# Path predicates (limb models; choose and count only)
# ---------------------------------------------------------------------------
def fe_add_path(a, b):
    """fe_add: 0 common, 1 the second carry pass runs for this lane, 2 the
    second pass carries out of word 7 as well."""
    s = a + b
    x = words(s % B256)
    if x[0] + 38 * (s >> 256) <= M32:
        return 0
    return 2 if all(w == M32 for w in x[1:]) else 1


def fe_sub_path(a, b):
    d = a - b
    x = words(d % B256)
    if x[0] - 38 * (1 if d < 0 else 0) >= 0:
        return 0
    return 2 if all(w == 0 for w in x[1:]) else 1


def fe_addsub_path(a, b):
    """The shared out-of-line block of fe_addsub: the deeper of its chains."""
    return max(fe_add_path(a, b), fe_sub_path(a, b))


def fe_reduce512_path(t):
    """fe_reduce512 on the 512-bit integer t."""
    tw = words(t, 16)
    u = [38 * tw[8 + i] + tw[i] for i in range(8)]
    lo = [x & M32 for x in u]
    hi = [x >> 32 for x in u]
    r = [0] * 8
    c = 0
    for i in range(1, 8):
        s = lo[i] + hi[i - 1] + c
        r[i], c = s & M32, s >> 32
    w = (hi[7] + c) * 38
    if lo[0] + w <= M32:
        return 0
    return 2 if all(x == M32 for x in r[1:]) else 1


MU = (1 << 512) // L  # the Barrett constant of sc_reduce512 (HAC 14.42, b = 2^32, k = 8)


def sc_reduce512_subs(x):
    """How many of sc_reduce512's two conditional subtractions of l run."""
    q3 = ((x >> 224) * MU) >> 288
    t = (x % (1 << 288) - q3 * L) % (1 << 288)
    n = 0
    for _ in range(2):
        if t >= L:
            t -= L
            n += 1
    return n


FOUR_P = [0x1FFFFFFB4] + [0x1FFFFFFFE] * 7


def _fw_passes(m):
    """fw::normalize_dpp on the per-lane values m[0..7]: the number of trips
    through its rippling loop (0: the first pass left no carry)."""
    def step(v):
        return [(v[c] & M32) + (38 * (v[7] >> 32) if c == 0 else v[c - 1] >> 32) for c in range(8)]
    v = step(m)
    n = 0
    while any(x >> 32 for x in v):
        v = step(v)
        n += 1
    return n


def fw_add_passes(a, b):
    return _fw_passes([x + y for x, y in zip(words(a), words(b))])


def fw_sub_passes(a, b):
    return _fw_passes([x + f - y for x, y, f in zip(words(a), words(b), FOUR_P)])


def fw_mul_passes(a, b):
    aw, bw = words(a), words(b)
    s = [sum(aw[c - k] * bw[k] for k in range(8) if 0 <= c - k < 8) for c in range(16)]
    n = [(s[c] & M32) + ((s[c - 1] >> 32) & M32 if c >= 1 else 0) + (s[c - 2] >> 64 if c >= 2 else 0)
         for c in range(16)]
    return _fw_passes([n[c] + 38 * n[c + 8] for c in range(8)])


def path_class(name, it):
    """The path class of an operand tuple for ops that have paths, else 0."""
    if name in ("fe_add",):
        return fe_add_path(it.a, it.b)
    if name == "fe_sub":
        return fe_sub_path(it.a, it.b)
    if name == "fe_addsub":
        return fe_addsub_path(it.a, it.b)
    if name == "fe_neg":
        return fe_sub_path(0, it.a)
    if name in ("fe_mul", "fe_mul_n4"):
        return fe_reduce512_path(it.a * it.b)
    if name in ("fe_sq", "fe_sq_n4"):
        return fe_reduce512_path(it.a * it.a)
    if name == "fe_reduce512":
        return fe_reduce512_path(it.a)
    if name == "sc_reduce512":
        return sc_reduce512_subs(it.a)
    if name == "fw_add":
        return min(1, fw_add_passes(it.a, it.b))
    if name == "fw_sub":
        return min(1, fw_sub_passes(it.a, it.b))
    if name == "fw_mul":
        return min(1, fw_mul_passes(it.a, it.b))
    if name == "fw_sq":
        return min(1, fw_mul_passes(it.a, it.a))
    return 0


# ---------------------------------------------------------------------------
# Operand constructions
# ---------------------------------------------------------------------------
FE_EDGES = ([0, 1, 2, 19, 38, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, B256 - 1, B256 - 2, (P - 1) // 2,
             1 << 255, M32, M32 << 224, 1 << 32, (1 << 32) - 38, B256 - 38, B256 - 39]
            + list(range((1 << 255) - 20, (1 << 255) + 20)))

# Operands that exposed a device bug are pinned here by name, so that they stay
# in the sets whatever the random seeds become: {op name: [(a, b, c), ...]}.
REGRESSIONS = {}

# sc_reduce512 inputs on which the Barrett estimate is two short (both final
# subtractions run), found by searching the structured family j*l + delta of
# tests/test_arith_operands.py::test_sc_reduce512_two_subtractions_search.
SC_REDUCE_TWO_SUBS = []


def _rng(tag):
    return random.Random("coa-arith-" + tag)


def _r256(rng):
    return rng.getrandbits(256)


def _mk(name, triples, rare):
    out = []
    for t in triples:
        t = tuple(t) + (None,) * (3 - len(t))
        it = Item(t[0], t[1], t[2], 0, rare, not rare)
        cls = path_class(name, it)
        # one subtraction of l is an everyday path of sc_reduce512, not a rare one
        out.append(it._replace(cls=cls, rare=rare or (cls > 0 and name != "sc_reduce512")))
    return out


def add_pairs(rng):
    """fe_add: path 2 from (2^256-1-i) + (2^256-1-j); path 1 from sums >= 2^256
    whose low word lands within 38 of 2^32 with upper words not all ones."""
    p2 = [(B256 - 1 - i, B256 - 1 - j) for i in range(40) for j in range(40)]
    p1 = []
    for _ in range(160):
        s = B256 + ((rng.getrandbits(223) << 32) | (M32 - rng.randrange(38)))
        a = rng.randrange(s - B256 + 1, B256)
        p1.append((a, s - a))
    return p2, p1


def sub_pairs(rng):
    """fe_sub: the mirror images, i - (2^256-1-j) and differences < 0 whose low
    word lands below 38 with upper words not all zero."""
    p2 = [(i, B256 - 1 - j) for i in range(40) for j in range(40)]
    p1 = []
    for _ in range(160):
        x = ((rng.getrandbits(223) + 1) << 32) | rng.randrange(38)
        a = rng.randrange(0, x)
        p1.append((a, a + B256 - x))
    return p2, p1


def mul_pairs(rng, n1=160, square=False):
    """fe_reduce512 through a product.  Path 2: (2^256-1-i)(2^256-1-j).  Path
    1: a target residue r whose low word is in [19, 38) and b = r / a (+ p):
    the fold of the top word then lands word 0 just past 2^32 for most such
    pairs.  For squarings a is a square root of r."""
    if square:
        # (2^256-1-i)^2 gives only 62 path-2 squares, so also the large roots
        # a of small residues s = a^2 mod p: t_lo + 38 t_hi = s + m p lands
        # just below a multiple of 2^256 when m is even and s < 19 m (callers
        # keep the candidates that the predicate puts on path 2)
        p2 = [(B256 - 1 - i,) for i in range(2048)]
        for s in range(38, 1500):
            ok, a = o.sqrt_ratio_i(s, 1)
            if ok:
                p2 += [(a + P,), (2 * P - a,)]
    else:
        p2 = [(B256 - 1 - i, B256 - 1 - j) for j in range(64) for i in range(j + 1)]
    p1 = []
    while len(p1) < n1:
        r = (rng.getrandbits(223) << 32) | rng.randrange(19, 38)
        if square:
            ok, a = o.sqrt_ratio_i(r % P, 1)
            if not ok:
                continue
            if rng.getrandbits(1):
                a = P - a
            if rng.getrandbits(1):
                a += P
            p1.append((a,))
        else:
            a = _r256(rng)
            if a % P == 0:
                continue
            b = r * pow(a, P - 2, P) % P
            if rng.getrandbits(1):
                b += P
            p1.append((a, b))
    return p2, p1


def _fw_add_ripples(rng, n):
    """fw::add: lane c sums to 2^32 - 1 and lane c-1 carries into it."""
    out = []
    for _ in range(n):
        aw, bw = words(_r256(rng)), words(_r256(rng))
        c = rng.randrange(1, 8)
        bw[c] = M32 - aw[c]
        aw[c - 1] |= 1 << 31
        bw[c - 1] |= 1 << 31
        out.append((from_words(aw), from_words(bw)))
    return out


def _fw_sub_ripples(rng, n):
    """fw::sub: a_c - b_c = 1 leaves lane c at 2^32 - 1 under a carry."""
    out = []
    for _ in range(n):
        aw, bw = words(_r256(rng)), words(_r256(rng))
        c = rng.randrange(1, 8)
        aw[c] = rng.randrange(1, 1 << 32)
        bw[c] = aw[c] - 1
        out.append((from_words(aw), from_words(bw)))
    return out


def _fw_mul_ripples(rng, n, square):
    """fw::mul: a target residue with one word (c >= 1) below 20, so that for
    most pairs that word is a low word that wrapped under the carry from the
    lane below; kept when the model says a ripple pass runs."""
    out = []
    tries = 0
    while len(out) < n and tries < 40 * n:
        tries += 1
        rw = words(rng.getrandbits(255))
        rw[rng.randrange(1, 8)] = rng.randrange(20)
        r = from_words(rw) % P
        if square:
            ok, a = o.sqrt_ratio_i(r, 1)
            if not ok:
                continue
            a += P * rng.getrandbits(1)
            b = a
        else:
            a = _r256(rng)
            if a % P == 0:
                continue
            b = r * pow(a, P - 2, P) % P + P * rng.getrandbits(1)
        if fw_mul_passes(a, b):
            out.append((a,) if square else (a, b))
    return out


def scalar_family():
    """j*l + delta over every magnitude of j up to floor((2^512-1)/l), and
    the named edges: the inputs where the Barrett estimate is tested."""
    rng = _rng("sc-family")
    jmax = ((1 << 512) - 1) // L
    js = {0, 1, 2, 3, jmax, jmax - 1, jmax - 2}
    for e in range(1, jmax.bit_length() + 1):
        for j in ((1 << e) - 1, 1 << e, (1 << e) + 1, rng.getrandbits(e) | (1 << (e - 1))):
            if 0 <= j <= jmax:
                js.add(j)
    xs = []
    for j in sorted(js):
        for d in (-1, 0, 1):
            x = j * L + d
            if 0 <= x < 1 << 512:
                xs.append(x)
    xs += [(1 << 512) - 1, (1 << 512) - L, 1 << 252, B256 - 1, 2 * L - 1, 2 * L + 1, L - 1, L, L + 1, 0]
    return xs


def sc_two_subs_search(per_magnitude, seed="coa-arith-sc-search"):
    """The structured search for sc_reduce512 inputs that need both final
    subtractions: j*l + delta, delta in {-1, 0, 1}, per_magnitude random j of
    every bit length up to floor((2^512-1)/l).  Returns (candidates tried,
    {subtractions: count}, [inputs with two])."""
    rng = random.Random(seed)
    jmax = ((1 << 512) - 1) // L
    hist, found, tried = {0: 0, 1: 0, 2: 0}, [], 0
    for e in range(1, jmax.bit_length() + 1):
        for _ in range(per_magnitude):
            j = rng.getrandbits(e) | (1 << (e - 1))
            for d in (-1, 0, 1):
                x = j * L + d
                if j > jmax or x >= 1 << 512:
                    continue
                tried += 1
                s = sc_reduce512_subs(x)
                hist[s] += 1
                if s == 2:
                    found.append(x)
    return tried, hist, found


# ---- points --------------------------------------------------------------
def _affine(p):
    X, Y, Z, _ = p
    zi = pow(Z, P - 2, P)
    return X * zi % P, Y * zi % P


def scale(p, rng, lift=True):
    """The same point in another representation: all four coordinates times a
    random lambda (so Z != 1), then + p on a random subset (weakly reduced)."""
    lam = rng.randrange(2, P)
    q = [v * lam % P for v in p]
    if lift:
        q = [v + P * rng.getrandbits(1) for v in q]
    return tuple(q)


def pack_p3(p):
    return sum(v << (256 * i) for i, v in enumerate(p))


def unpack_p3(v):
    return tuple((v >> (256 * i)) & (B256 - 1) for i in range(4))


def pack_niels(p, rng):
    x, y = _affine(p)
    vals = [(y + x) % P, (y - x) % P, 2 * o.D * x * y % P]
    return sum((v + P * rng.getrandbits(1)) << (256 * i) for i, v in enumerate(vals))


@functools.lru_cache(maxsize=None)
def point_pool(n=256):
    """n prime-order-subgroup points [r]B (a chain of additions from a few
    random multiples), then mixed-order ones (each plus a torsion point)."""
    rng = _rng("points")
    step = o.pmul(rng.randrange(1, L), o.B)
    cur = o.pmul(rng.randrange(1, L), o.B)
    pts = []
    for _ in range(n):
        pts.append(cur)
        cur = o.padd(cur, step)
    tors = o.torsion_points()
    mixed = [o.padd(pts[i], tors[i % 8]) for i in range(64)]
    return pts, mixed, tors


def point_pairs(rng, n_random):
    pts, mixed, tors = point_pool()
    O = o.IDENT
    special = []
    for i in range(16):
        Pt = (pts + mixed)[rng.randrange(len(pts) + 64)]
        special += [(Pt, Pt), (Pt, o.pneg(Pt)), (Pt, O), (O, Pt)]
        special += [(Pt, t) for t in tors] if i < 4 else []
    special += [(O, O)] * 2
    special += [(s, t) for s in tors for t in tors]
    allp = pts + mixed
    rand = [(allp[rng.randrange(len(allp))], allp[rng.randrange(len(allp))]) for _ in range(n_random)]
    return special, rand


# ---------------------------------------------------------------------------
# The operand set of every op
# ---------------------------------------------------------------------------
N_RANDOM = 1024


@functools.lru_cache(maxsize=None)
def operands(name):
    """[Item] for op `name`: every constructed path class, the edges, the
    pinned regressions and the random operands, deterministic."""
    rng = _rng(name)
    r2 = lambda n=N_RANDOM: [(_r256(rng), _r256(rng)) for _ in range(n)]  # noqa: E731
    r1 = lambda n=N_RANDOM: [(_r256(rng),) for _ in range(n)]  # noqa: E731
    edges1 = [(v,) for v in FE_EDGES]
    edges2 = [(a, b) for a in FE_EDGES[:21] for b in FE_EDGES[:21]]
    items = _mk(name, REGRESSIONS.get(name, []), True)

    if name in ("fe_add", "fe_sub", "fe_addsub", "fw_add", "fw_sub"):
        ap2, ap1 = add_pairs(rng)
        sp2, sp1 = sub_pairs(rng)
        st = {"fe_add": ap2 + ap1, "fe_sub": sp2 + sp1, "fw_add": ap2[::7] + ap1, "fw_sub": sp2[::7] + sp1}.get(
            name, ap2[::2] + ap1 + sp2[::2] + sp1)
        if name == "fw_add":
            st += _fw_add_ripples(rng, 160)
        if name == "fw_sub":
            st += _fw_sub_ripples(rng, 160)
        items += _mk(name, st + edges2, True) + _mk(name, r2(), False)
    elif name == "fe_neg":
        st = [(B256 - 1 - j,) for j in range(64)] + [(B256 - ((rng.getrandbits(200) + 1) << 32) - rng.randrange(1, 38),)
                                                     for _ in range(96)]
        items += _mk(name, st + edges1, True) + _mk(name, r1(), False)
    elif name in ("fe_mul", "fw_mul"):
        p2, p1 = mul_pairs(rng)
        st = p2 + p1 if name == "fe_mul" else p2[::5] + p1[:64] + _fw_mul_ripples(rng, 160, False)
        items += _mk(name, st + edges2, True) + _mk(name, r2(), False)
    elif name in ("fe_sq", "fw_sq"):
        p2, p1 = mul_pairs(rng, square=True)
        p2 = [t for t in p2 if fe_reduce512_path(t[0] * t[0]) == 2]
        st = p2 + p1 if name == "fe_sq" else p2[::3] + p1[:64] + _fw_mul_ripples(rng, 160, True)
        items += _mk(name, st + edges1, True) + _mk(name, r1(), False)
    elif name == "fe_mul_n4":
        p2, p1 = mul_pairs(rng)
        st = [(a, b, _r256(rng)) for a, b in p2[::4] + p1]
        st += [(_r256(rng), a, b) for a, b in p2[1::16] + p1[::4]]  # the rare pair as the second product
        items += _mk(name, st, True) + _mk(name, [(_r256(rng), _r256(rng), _r256(rng)) for _ in range(N_RANDOM)], False)
    elif name == "fe_sq_n4":
        p2, p1 = mul_pairs(rng, square=True)
        p2 = [t for t in p2 if fe_reduce512_path(t[0] * t[0]) == 2]
        st = [(a, _r256(rng), _r256(rng)) for (a,) in p2 + p1]
        st += [(_r256(rng), _r256(rng), a) for (a,) in p2[::4] + p1[::4]]
        items += _mk(name, st, True) + _mk(name, [(_r256(rng), _r256(rng), _r256(rng)) for _ in range(N_RANDOM)], False)
    elif name == "fe_reduce512":
        p2, p1 = mul_pairs(rng)
        st = [(a * b,) for a, b in p2 + p1] + [((1 << 512) - 1,), (0,), ((1 << 512) - (1 << 256),), (B256 - 1,)]
        # non-products around the same edges: top half all ones, low half just below the wrap
        st += [(((B256 - 1) << 256) | (B256 - 1 - i),) for i in range(64)]
        st += [((rng.getrandbits(256) << 256) | (rng.getrandbits(224) << 32) | (M32 - rng.randrange(1500)),)
               for _ in range(256)]
        items += _mk(name, st, True) + _mk(name, [(rng.getrandbits(512),) for _ in range(N_RANDOM)], False)
    elif name == "fe_mul_small":
        cs = [0, 1, 2, 19, 38, 121666, (1 << 26) - 1]
        st = [(a, c) for a in [0, P, B256 - 1, P - 1, 2 * P + 1] + [_r256(rng) for _ in range(8)] for c in cs]
        items += _mk(name, st, True) + _mk(name, [(_r256(rng), rng.randrange(1 << 26)) for _ in range(N_RANDOM)], False)
    elif name == "fe_fold_word":
        wmax = (1 << 32) - (1 << 10) - 1
        st = [(a, w) for a in FE_EDGES[:21] + [B256 - 1 - i for i in range(3, 40)] for w in (0, 1, 37, 38, 39, wmax)]
        items += _mk(name, st, True) + _mk(name, [(_r256(rng), rng.randrange(wmax + 1)) for _ in range(N_RANDOM)], False)
    elif name in ("fe_canon", "fe_to_words", "fe_iszero", "fe_isneg", "fe_from_words"):
        st = edges1 + [(k * P + d,) for k in (0, 1, 2) for d in range(-3, 4) if 0 <= k * P + d < B256]
        st += [(int.from_bytes(bytes([0xFF] * k + [0] * (32 - k)), "little"),) for k in range(1, 33)]
        items += _mk(name, st, True) + _mk(name, r1(), False)
    elif name == "fe_eq":
        base = FE_EDGES[:21] + [_r256(rng) % P for _ in range(64)]
        st = []
        for a in base:
            for b in (a, a % P, a % P + P, (a + 1) % B256, (a + P) % B256, (a - P) % B256, B256 - 1 - a, (a ^ 1)):
                st.append((a, b % B256))
        items += _mk(name, st, True) + _mk(name, r2(), False)
    elif name in ("fe_pow_p58", "fe_invert", "fw_pow_p58", "fw_invert"):
        items += _mk(name, edges1, True) + _mk(name, r1(1024 - len(edges1)), False)
    elif name in ("fe_sqrt_ratio", "fw_sqrt_ratio"):
        st = [(0, 0), (0, 1), (1, 0), (1, 1), (P, 1), (P - 1, 1), (1, P - 1), (B256 - 1, B256 - 1), (2, 1), (1, 2)]
        for _ in range(96):
            r, v = _r256(rng) % P, _r256(rng) % P or 1
            for u in (r * r * v % P, -r * r * v % P, o.SQRT_M1 * r * r * v % P, -o.SQRT_M1 * r * r * v % P):
                st.append((u + P * rng.getrandbits(1), v + P * rng.getrandbits(1)))
        items += _mk(name, st, True) + _mk(name, r2(1024 - len(st)), False)
    elif name == "sc_is_canonical":
        st = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 1 << 252, (1 << 252) - 1, (1 << 253) - 1, B256 - 1,
              8 * L, 8 * L - 1]
        st += [L + s * (1 << (32 * k)) for k in range(8) for s in (1, -1)]
        st += [from_words(words(L)[:k] + [0] * (8 - k)) for k in range(8)]
        items += _mk(name, [(v,) for v in st], True)
        items += _mk(name, r1(512) + [(rng.randrange(L),) for _ in range(512)], False)
    elif name == "sc_reduce512":
        st = [(x,) for x in scalar_family() + SC_REDUCE_TWO_SUBS]
        items += _mk(name, st, True) + _mk(name, [(rng.getrandbits(512),) for _ in range(N_RANDOM)], False)
    elif name == "sc_muladd":
        e = [0, 1, L - 1, L, B256 - 1]
        st = [(a, b, c) for a in e for b in e for c in e]
        items += _mk(name, st, True)
        items += _mk(name, [(_r256(rng), _r256(rng), _r256(rng)) for _ in range(N_RANDOM)], False)
    elif name == "sc_mul":
        e = [0, 1, 2, L - 1, L, L + 1, 1 << 252, B256 - 1]
        items += _mk(name, [(a, b) for a in e for b in e], True) + _mk(name, r2(), False)
    elif name == "sc_add":  # canonical operands (the header's precondition)
        e = [0, 1, 2, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 1 << 252, (1 << 252) - 1, M32, 1 << 32]
        items += _mk(name, [(a, b) for a in e for b in e], True)
        items += _mk(name, [(rng.randrange(L), rng.randrange(L)) for _ in range(N_RANDOM)], False)
    elif name == "sc_neg":
        e = [0, 1, 2, L - 1, L - 2, (L - 1) // 2, (L + 1) // 2, 1 << 252, (1 << 252) - 1, M32, 1 << 32, 1 << 224]
        items += _mk(name, [(a,) for a in e], True) + _mk(name, [(rng.randrange(L),) for _ in range(N_RANDOM)], False)
    elif name == "halve":
        import test_gpu_halve  # the adversarial k list: imported, not copied

        ks = test_gpu_halve._ks(random.Random(7))
        items += _mk(name, [(k,) for k in ks], True)
        items += _mk(name, [(rng.randrange(1, L),) for _ in range(4096)], False)
    elif name in ("ge_add", "ge_sub", "ge_add_il", "ge_p2_eq_p3"):
        special, rand = point_pairs(rng, N_RANDOM)
        if name == "ge_p2_eq_p3":  # many equal pairs in different representations
            pts, mixed, tors = point_pool()
            special += [(p, p) for p in pts[:128] + mixed + tors]
            special += [(p, o.padd(p, tors[1 + i % 7])) for i, p in enumerate(pts[:64])]
        mk = lambda prs, lift=True: [(pack_p3(scale(p, rng, lift)), pack_p3(scale(q, rng, lift))) for p, q in prs]  # noqa
        items += _mk(name, mk(special) + mk(special[:64], False), True) + _mk(name, mk(rand), False)
    elif name in ("ge_madd", "ge_madd_il"):
        special, rand = point_pairs(rng, N_RANDOM)
        mk = lambda prs: [(pack_p3(scale(p, rng)), pack_niels(q, rng)) for p, q in prs]  # noqa: E731
        items += _mk(name, mk(special), True) + _mk(name, mk(rand), False)
    elif name in ("ge_p2_dbl", "ge_p3_dbl", "ge_p2_dbl_il", "ge_p3_to_cached", "ge_is_small_order",
                  "ge_p2_is_identity", "ge_p2_compress"):
        pts, mixed, tors = point_pool()
        sp = [t for t in tors for _ in range(6)] + mixed + [o.IDENT] * 4
        if name == "ge_p2_is_identity":
            sp += [o.IDENT] * 28
        n_rand = (1024 if name == "ge_p2_compress" else N_RANDOM) - len(sp) - 8
        rnd = [pts[rng.randrange(len(pts))] for _ in range(n_rand)]
        plain = [pack_p3(p) for p in tors]  # Z = 1, canonical coordinates
        items += _mk(name, [(pack_p3(scale(p, rng)),) for p in sp] + [(v,) for v in plain], True)
        items += _mk(name, [(pack_p3(scale(p, rng)),) for p in rnd], False)
    elif name == "ge_decompress":
        import test_gpu_fe_rows

        pts, mixed, tors = point_pool()
        st = [v for v in test_gpu_fe_rows._edge_values()]
        st += [int.from_bytes(e, "little") for e in o.small_order_encodings()]
        for p in (pts[:96] + mixed):
            y = int.from_bytes(o.compress(p), "little")
            st += [y, y ^ (1 << 255)]
        st += [v for v in FE_EDGES if v not in st]
        items += _mk(name, [(v,) for v in st], True) + _mk(name, r1(1024 - len(st)), False)
    else:
        raise KeyError(name)
    return items


# ---------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------
def _w8(out, k=0):
    return from_words(out[8 * k:8 * k + 8])


def _mod(got, want, what):
    if got % P != want % P:
        return f"{what}: got {got:#x}, want {want % P:#x} (mod p)"
    return None


def _exact(got, want, what):
    if got != want:
        return f"{what}: got {got:#x}, want exactly {want:#x}"
    return None


def _point(out, want, what):
    X, Y, Z, T = (_w8(out, k) for k in range(4))
    if Z % P == 0:
        return f"{what}: Z == 0 (mod p)"
    zi = pow(Z, P - 2, P)
    x, y = _affine(want)
    if (X * zi % P, Y * zi % P) != (x, y):
        return f"{what}: affine ({X * zi % P:#x}, {Y * zi % P:#x}), want ({x:#x}, {y:#x})"
    if (T * Z - X * Y) % P:
        return f"{what}: T*Z != X*Y (X={X:#x} Y={Y:#x} Z={Z:#x} T={T:#x})"
    return None


# The width the consumers of halve() process: both digit loops run
# H = (cost + 2 + 3) / 4 signed radix-16 digits of c + 0x88..8 and |d| + 0x88..8
# (csrc/coa_halved.hip:312 "c, d < 2^(4H - 2)", digit loops of k_verify_main at
# coa_halved.hip:531; csrc/coa_latency.hip:251 and horner()'s loop at
# coa_latency.hip:165), H is stored in 8 bits beside 8-word digit strings, so
# it cannot exceed the 64 nibbles of a word string.
def halve_width(cost):
    H = (cost + 2 + 3) // 4
    return H, 4 * H - 2


def check_halve(k, out):
    c, d, neg, cost = _w8(out, 0), _w8(out, 1), out[16], out[17]
    if neg not in (0, 1):
        return f"sign word {neg}"
    if d % 2 != 1:
        return f"d = {d:#x} is even"
    sd = -d if neg else d
    if (c - sd * k) % (8 * L):
        return f"c != {'-' if neg else '+'}d*k (mod 8l): c={c:#x} d={d:#x}"
    bits = max(c.bit_length(), d.bit_length())
    if cost != bits:  # coa_halve.h consider(): cost = max(bits(c), bits(t))
        return f"cost_out {cost} != max(bits(c), bits(d)) = {bits}"
    H, width = halve_width(cost)
    if H > 64 or bits > width:
        return f"{bits}-bit vector, but the consumers process H={H} digits ({width} bits)"
    return None


def _fe_results(name, it):
    a, b, c = it.a, it.b, it.c
    if name in ("fe_add", "fw_add"):
        return [a + b]
    if name in ("fe_sub", "fw_sub"):
        return [a - b]
    if name == "fe_addsub":
        return [a + b, a - b]
    if name == "fe_neg":
        return [-a]
    if name in ("fe_mul", "fw_mul"):
        return [a * b]
    if name in ("fe_sq", "fw_sq"):
        return [a * a]
    if name == "fe_mul_n4":
        return [a * b, b * c, c * a, b * b]
    if name == "fe_sq_n4":
        return [a * a, b * b, c * c, (a ^ b) ** 2]
    if name in ("fe_reduce512", "fe_canon"):
        return [a]
    if name in ("fe_mul_small",):
        return [a * b]
    if name == "fe_fold_word":
        return [a + b]
    if name == "fe_from_words":
        return [a & ((1 << 255) - 1)]
    if name in ("fe_pow_p58", "fw_pow_p58"):
        return [pow(a % P, (P - 5) // 8, P)]
    if name in ("fe_invert", "fw_invert"):
        return [pow(a % P, P - 2, P)]
    return None


def check(name, it, out):
    """None when the raw output words `out` of op `name` on operand tuple
    `it` are right, else a description of what is wrong."""
    out = [int(w) for w in out]
    a, b, c = it.a, it.b, it.c
    fr = _fe_results(name, it)
    if fr is not None:
        for k, want in enumerate(fr):
            err = _mod(_w8(out, k), want, f"result {k}")
            if err:
                return err
        if name == "fe_canon":
            return _exact(_w8(out), a % P, "canonical form")
        if name == "fe_from_words":
            return _exact(_w8(out), a & ((1 << 255) - 1), "words")
        return None
    if name == "fe_to_words":
        return _exact(_w8(out), a % P, "canonical words")
    if name == "fe_iszero":
        return _exact(out[0], int(a % P == 0), "flag")
    if name == "fe_isneg":
        return _exact(out[0], o.is_negative(a), "flag")
    if name == "fe_eq":
        return _exact(out[0], int((a - b) % P == 0), "flag")
    if name in ("fe_sqrt_ratio", "fw_sqrt_ratio"):
        ok, r = o.sqrt_ratio_i(a, b)
        return _exact(out[0], int(ok), "flag") or _mod(from_words(out[1:9]), r, "root")
    if name == "sc_is_canonical":
        return _exact(out[0], int(o.scalar_is_canonical(a.to_bytes(32, "little"))), "flag")
    if name == "sc_reduce512":
        return _exact(_w8(out), a % L, "scalar")
    if name == "sc_muladd":
        return _exact(_w8(out), (a * b + c) % L, "scalar")
    if name == "sc_mul":
        return _exact(_w8(out), a * b % L, "scalar")
    if name == "sc_add":
        return _exact(_w8(out), (a + b) % L, "scalar")
    if name == "sc_neg":
        return _exact(_w8(out), -a % L, "scalar")
    if name == "halve":
        return check_halve(a, out)
    if name in ("ge_add", "ge_add_il"):
        return _point(out, o.padd(unpack_p3(a), unpack_p3(b)), "P+Q")
    if name == "ge_sub":
        return _point(out, o.padd(unpack_p3(a), o.pneg(unpack_p3(b))), "P-Q")
    if name in ("ge_madd", "ge_madd_il"):
        ypx, ymx, _ = (b >> (256 * i) & (B256 - 1) for i in range(3))
        i2 = pow(2, P - 2, P)
        x, y = (ypx - ymx) * i2 % P, (ypx + ymx) * i2 % P
        return _point(out, o.padd(unpack_p3(a), (x, y, 1, x * y % P)), "P+q")
    if name in ("ge_p2_dbl", "ge_p3_dbl", "ge_p2_dbl_il"):
        return _point(out, o.pdbl(unpack_p3(a)), "2P")
    if name == "ge_p3_to_cached":
        X, Y, Z, T = unpack_p3(a)
        for k, want in enumerate((Y + X, Y - X, Z, o.D2 * T)):
            err = _mod(_w8(out, k), want, ("Y+X", "Y-X", "Z", "2dT")[k])
            if err:
                return err
        return None
    if name == "ge_is_small_order":
        return _exact(out[0], int(o.is_small_order(unpack_p3(a))), "flag")
    if name == "ge_p2_is_identity":
        return _exact(out[0], int(o.is_identity(unpack_p3(a))), "flag")
    if name == "ge_p2_eq_p3":
        return _exact(out[0], int(o.peq(unpack_p3(a), unpack_p3(b))), "flag")
    if name == "ge_p2_compress":
        return _exact(_w8(out), int.from_bytes(o.compress(unpack_p3(a)), "little"), "encoding")
    if name == "ge_decompress":
        pt = o.decompress(a.to_bytes(32, "little"))
        err = _exact(out[0], int(pt is not None), "flag")
        if err or pt is None:
            return err
        X, Y, _, T = pt
        return (_mod(from_words(out[1:9]), X, "X") or _mod(from_words(out[9:17]), Y, "Y")
                or _mod(from_words(out[17:25]), T, "T"))
    raise KeyError(name)


def describe(name, it):
    op = OPS[name]
    parts = []
    for tag, v, n in (("a", it.a, op.na), ("b", it.b, op.nb), ("c", it.c, op.nc)):
        if n:
            parts.append(f"{tag}={v:#x}")
    return f"path class {it.cls}{' (rare)' if it.rare else ''}: " + " ".join(parts)


# ---------------------------------------------------------------------------
# Layouts: where the rare operands sit in the waves
# ---------------------------------------------------------------------------
def group_size(name):
    """Items per wave: 64 lanes, or the 4 rows of a row op."""
    return 4 if OPS[name].rows else 64


def lane_mix_layout(name):
    """The item list of the main run.  Waves (of group_size items) in order:
    every position rare; only position 0; only the last; alternating; none;
    (row ops: only row 1, only row 2, so each of the four rows is the one that
    ripples); then every operand of the set, rare ones first, cut or padded so
    that the last wave is partial (n = 64 m + 37 for lane ops, 4 m + 3 rows)."""
    its = operands(name)
    rare = [it for it in its if it.rare]
    hot = [it for it in rare if it.cls > 0] or rare  # the rare-path operands proper where the op has paths
    common = [it for it in its if not it.rare]
    g = group_size(name)
    pats = [set(range(g)), {0}, {g - 1}, set(range(0, g, 2)), set()]
    if g == 4:
        pats += [{1}, {2}, {1, 3}]
    out = []
    hi = ci = 0
    for rep in range(2 if g == 64 else 8):  # two (eight) rounds with different rare operands
        for pat in pats:
            for pos in range(g):
                if pos in pat:
                    out.append(hot[hi % len(hot)])
                    hi += 1
                else:
                    out.append(common[ci % len(common)])
                    ci += 1
    out += rare + common
    tail = 37 if g == 64 else 3
    while len(out) % g != tail:
        out.append(common[ci % len(common)])
        ci += 1
    return out


def masked_layouts(name):
    """[(tag, items, mask)] for the divergent-caller runs: rare operands on
    every position of the first waves, on the odd positions of the next, none
    in the last; masks by position in the wave."""
    its = operands(name)
    rare = [it for it in its if it.cls > 0] or [it for it in its if it.rare]
    common = [it for it in its if not it.rare]
    g = group_size(name)
    waves = 6 if g == 64 else 24
    items = []
    for w in range(waves):
        for pos in range(g):
            k = w * g + pos
            if w % 3 == 0 or (w % 3 == 1 and pos % 2 == 1):
                items.append(rare[k % len(rare)])
            else:
                items.append(common[k % len(common)])
    if g == 64:
        masks = {"alternating": lambda p: p % 2 == 1, "lane5": lambda p: p == 5, "first32": lambda p: p < 32}
    else:  # whole rows sit out: one row, two rows, all but one
        masks = {"row2_out": lambda p: p != 2, "rows02_out": lambda p: p % 2 == 1, "rows12_out": lambda p: p in (0, 3),
                 "only_row1": lambda p: p == 1}
    return [(tag, items, [1 if f(k % g) else 0 for k in range(len(items))]) for tag, f in masks.items()]

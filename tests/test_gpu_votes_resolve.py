"""GPU: coa_certificate_votes_resolve_device -- the COA_DAG_VOTES_OPEN words a
device-resident verdict call leaves are closed on the device with dalek's
verify_batch answer, and nothing else moves.  Expected words never come from
the engine: they are tests/verdict_cases.py's restatement of
primary/src/messages.rs and, where the answer is the weights', the C
restatement of dalek (oracle/coa_oracle.py) under the very weights the call is
given."""
import functools
import random

import numpy as np
import pytest

import verdict_cases as vc

pytestmark = pytest.mark.gpu

WEIGHT_SEED = 5  # np.random.default_rng(5): the oracle answers 21 Ok and 107 Err over the 128 pairs of test 2


def _dev(x):
    import torch

    x = np.array(x)  # a writable copy
    if x.dtype == np.uint64:
        x = x.view(np.int64)
    elif x.dtype == np.uint32:
        x = x.view(np.int32)
    return torch.from_numpy(x).to(torch.device("cuda", 0))


def _words(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32).copy()


@pytest.fixture(scope="module")
def registered(engine):
    engine.committee_register_authorities(*vc.committee().arrays())
    yield engine
    engine.committee_register(np.zeros((0, 32), np.uint8))


class Round:
    """The cases' arrays on the device and the verdict call's words over them
    (computed once; a resolve call works on a copy)."""

    def __init__(self, engine, cases):
        import torch

        self.e, self.cases, self.n = engine, cases, len(cases)
        h, ids, origins, hsigs, rounds, vp, vs, off, counts = self.host = vc.certificate_arrays(cases)
        self.nv = int(off[-1])
        self.votes = np.diff(off.astype(np.int64))
        hdata = np.frombuffer(b"".join(h) + bytes(16), np.uint8)
        hoff = np.zeros(self.n + 1, np.uint64)
        hoff[1:] = np.cumsum([len(x) for x in h])
        # an empty vote array still needs an address
        self.d = [_dev(ids), _dev(origins), _dev(rounds), _dev(vp if self.nv else np.zeros((1, 32), np.uint8))[:self.nv],
                  _dev(vs if self.nv else np.zeros((1, 64), np.uint8))[:self.nv], _dev(off)]
        out = torch.full((self.n,), -1, dtype=torch.int32, device="cuda:0")
        engine.certificate_verdict_many_device(0, _dev(hdata), _dev(hoff), self.d[0], self.d[1], _dev(hsigs), self.d[2],
                                               self.d[3], self.d[4], self.d[5], _dev(np.array(counts, np.uint32)), out)
        self.before_t = out
        self.before = _words(out)
        self.open = self.before == vc.OPEN

    def zs(self, seed):
        return np.random.default_rng(seed).integers(0, 256, (max(self.nv, 1), 16), dtype=np.uint8)

    def resolve(self, zs=None, rng_seed=0, cap=0, own=False, words=None):
        """(words after, counts) of one resolve call over a copy of the
        verdict call's words (or over `words`); own: a caller workspace, on a
        stream that is not the default one."""
        import torch

        out = self.before_t.clone() if words is None else _dev(words)
        counts = torch.full((3,), -1, dtype=torch.int32, device="cuda:0")
        dz = _dev(zs) if zs is not None else None
        kw = dict(zs=dz, rng_seed=rng_seed, open_votes_cap=cap, counts=counts)
        if own:
            nbytes = self.e.certificate_votes_resolve_workspace_bytes(self.n, self.nv, cap)
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda:0")
            side = torch.cuda.Stream(device=0)
            side.wait_stream(torch.cuda.current_stream(0))
            with torch.cuda.stream(side):
                self.e.certificate_votes_resolve_device(0, *self.d, out, stream=side, workspace=ws, **kw)
            side.synchronize()
        else:
            self.e.certificate_votes_resolve_device(0, *self.d, out, **kw)
        return _words(out), [int(x) for x in _words(counts)]

    def oracle_words(self, zs):
        """OK / BAD_VOTES per certificate from the oracle's vote bit under zs."""
        import coa_oracle as co

        bits = np.asarray(co.certificate_verify_many(*self.host[:8], zs))
        return np.where(bits & 4, vc.BAD_VOTES, vc.OK).astype(np.uint32)


def _diff(cases, got, want):
    return [(c["name"], hex(int(g)), hex(int(w))) for c, g, w in zip(cases, got, want) if g != w]


# ---------------------------------------------------------------- test 1
@functools.lru_cache(maxsize=None)
def _all_cases(engine):
    return Round(engine, vc.certificate_cases())


@pytest.mark.parametrize("own", [False, True], ids=["engine_workspace", "caller_workspace_side_stream"])
def test_every_case_closed(registered, own):
    r = _all_cases(registered)
    want, _ = vc.expected_certificates()
    assert r.open.any()
    got, counts = r.resolve(zs=r.zs(1), own=own)  # any weights: these cases are weight-independent by construction
    print("open before:", [c["name"] for c, o in zip(r.cases, r.open) if o], "counts", counts)
    assert not _diff(r.cases, got, want)
    assert not (got == vc.OPEN).any()
    assert (got[~r.open] == r.before[~r.open]).all()  # bit for bit
    assert counts == [int(r.open.sum())] * 2 + [int(r.votes[r.open].sum())]


# ---------------------------------------------------------------- test 2
@functools.lru_cache(maxsize=None)
def weight_cases():
    """Four certificates whose answer is the weights' (a quorum of honest
    voters plus the mixed-order member, whose signature holds the cofactorless
    equation: the sum keeps [z]T for a torsion point T of order 8) and two of
    the same kind with one answer: the small-order member signing (Ok) and the
    off-curve member (Err)."""
    b = vc.Builder()
    c, w = b.c, b.c.w
    quorum_voters = [c.honest[i] for i in c.plain[:30]]
    rng = random.Random(23)
    for i in range(4):
        h = b.header(c.honest[0], [0, 1000], tag=b"w%d" % i)
        d = vc.cert_digest(h["id"], h["round"], h["origin"])
        b.add(f"mixed_{i}", h, b.votes(h, quorum_voters) + [(w.mx_pk, w.mixed_sign(d, rng))])
    h = b.header(c.honest[0], [0, 1000], tag=b"ws")
    d = vc.cert_digest(h["id"], h["round"], h["origin"])
    b.add("small_order_member", h, b.votes(h, quorum_voters) + [(w.small_pk, w.small_order_key_sign(d, rng))])
    h = b.header(c.honest[0], [0, 1000], tag=b"wo")
    b.add("off_curve_member", h, b.votes(h, quorum_voters) + [(w.off_pk, bytes(range(64)))])
    return tuple(b.cases)


@functools.lru_cache(maxsize=None)
def _weight_round(engine):
    return Round(engine, weight_cases())


def test_weight_dependent_groups_follow_the_oracle(registered):
    cases = weight_cases()
    nv = sum(len(c["votes"]) for c in cases)
    gen = np.random.default_rng(WEIGHT_SEED)
    vectors = [gen.integers(0, 256, (nv, 16), dtype=np.uint8) for _ in range(32)]
    import coa_oracle as co

    host = vc.certificate_arrays(cases)
    bits = np.array([co.certificate_verify_many(*host[:8], z) for z in vectors])
    assert not (bits & 3).any()
    bad = (bits & 4) != 0
    n_ok, n_err = int((~bad[:, :4]).sum()), int(bad[:, :4].sum())
    print("oracle over the 128 pairs: Ok", n_ok, "Err", n_err)
    assert n_ok >= 3 and n_err >= 3  # both sides before any device call
    assert (~bad[:, 4]).all() and bad[:, 5].all()

    r = _weight_round(registered)
    print("verdict words:", [hex(int(x)) for x in r.before])
    assert r.open[:4].all()  # the verdict call leaves the weight-dependent ones open
    for k, z in enumerate(vectors):
        got, counts = r.resolve(zs=z, own=bool(k & 1))
        want = np.where(bad[k], vc.BAD_VOTES, vc.OK).astype(np.uint32)
        assert not _diff(cases, got, want), k
        assert counts[0] == counts[1] == int(r.open.sum())


# ---------------------------------------------------------------- test 3
def _case(name):
    return next(c for c in vc.certificate_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def _interleaved(engine):
    """300 copies of one_vote_s_flip interleaved with 300 clean certificates:
    more open certificates than one 256-lane block, 9,000 open votes."""
    return Round(engine, [_case("one_vote_s_flip"), _case("clean_a")] * 300)


def test_one_open_certificate_alone(registered):
    r = Round(registered, [_case("one_vote_s_flip")])
    assert r.open.tolist() == [True]
    got, counts = r.resolve(zs=r.zs(2))
    assert got.tolist() == [vc.BAD_VOTES] and counts == [1, 1, 30]


def test_nothing_open(registered):
    r = Round(registered, [_case("clean_a"), _case("votes_0"), _case("fail_bad_id"), _case("clean_b")])
    assert not r.open.any()
    for own in (False, True):
        got, counts = r.resolve(zs=r.zs(2), own=own)
        assert (got == r.before).all() and counts == [0, 0, 0]
    # ... and a call without any vote
    r = Round(registered, [_case("votes_0")] * 3)
    got, counts = r.resolve(rng_seed=4)
    assert (got == r.before).all() and counts == [0, 0, 0]


def test_more_open_than_a_block(registered):
    r = _interleaved(registered)
    assert r.open.tolist() == [True, False] * 300
    assert int(r.open.sum()) > 256 and int(r.votes[r.open].sum()) > 256 * 32  # COA_VERIFY_BLOCK * 32
    got, counts = r.resolve(zs=r.zs(3), own=True)
    assert (got[0::2] == vc.BAD_VOTES).all()
    assert (got[1::2] == r.before[1::2]).all() and (got[1::2] == vc.OK).all()
    assert counts == [300, 300, 9000]


def test_open_certificate_wider_than_a_wave_first_and_last(registered):
    """68 votes in one open certificate (more than a wave), as the first and
    as the last certificate of the call; in between an open one of 30 votes
    and closed ones."""
    big = dict(_case("votes_68"))
    v = list(big["votes"])
    v[66] = (v[66][0], vc._flip(v[66][1], 40))
    big.update(name="votes_68_s_flip", votes=v)
    cases = [big, _case("clean_a"), _case("one_vote_s_flip"), _case("fail_reuse"), big]
    r = Round(registered, cases)
    assert r.open.tolist() == [True, False, True, False, True]
    zs = r.zs(6)
    got, counts = r.resolve(zs=zs)
    want = np.where(r.open, r.oracle_words(zs), r.before)
    assert not _diff(cases, got, want)
    assert got[[0, 2, 4]].tolist() == [vc.BAD_VOTES] * 3
    assert counts == [3, 3, 68 + 30 + 68]


# ---------------------------------------------------------------- test 4
def test_cap_takes_a_prefix_and_a_second_call_closes_the_rest(registered):
    r = _interleaved(registered)
    zs = r.zs(3)
    cap = 100 * 30 + 5
    got, counts = r.resolve(zs=zs, cap=cap, own=True)
    open_at = np.flatnonzero(r.open)
    assert (got[open_at[:100]] == vc.BAD_VOTES).all()  # exactly the first 100 in index order
    assert (got[open_at[100:]] == vc.OPEN).all()
    assert (got[~r.open] == r.before[~r.open]).all()
    assert counts == [300, 100, 3000]
    again, counts = r.resolve(zs=zs, words=got)
    assert counts == [200, 200, 6000]
    whole, _ = r.resolve(zs=zs)
    assert (again == whole).all() and not (whole == vc.OPEN).any()


# ---------------------------------------------------------------- test 5
def test_derived_weights(registered):
    r = _all_cases(registered)
    want, _ = vc.expected_certificates()
    a, _ = r.resolve(rng_seed=11)
    b, _ = r.resolve(rng_seed=11, own=True)
    fresh, _ = r.resolve(rng_seed=0)
    assert (a == b).all()
    assert not _diff(r.cases, a, want) and not _diff(r.cases, fresh, want)

    # independence from the cap and from what else is open: the weight-dependent
    # certificates get the same words from one call and from two capped ones
    w = _weight_round(registered)
    whole, counts = w.resolve(rng_seed=77)
    assert counts[0] == counts[1] == int(w.open.sum())
    open_at = np.flatnonzero(w.open)
    cap = int(w.votes[open_at[:2]].sum()) + 3
    part, counts = w.resolve(rng_seed=77, cap=cap)
    assert counts[:2] == [len(open_at), 2] and (part[open_at[2:]] == vc.OPEN).all()
    rest, counts = w.resolve(rng_seed=77, words=part)
    assert counts[:2] == [len(open_at) - 2] * 2
    print("derived weights, seed 77:", [hex(int(x)) for x in whole])
    assert (rest == whole).all() and not (whole == vc.OPEN).any()
    assert whole[4] == vc.OK and whole[5] == vc.BAD_VOTES

"""GPU: the digit cap of k_verify_main_sums (csrc/coa_halved.hip) and the row
prologue that gives the lanes above it their top digits (csrc/coa_sums_tail.h),
forced with COA_MAIN_SUMS=1 at every size (COA_LAT_MAX=0 keeps small calls off
the latency route).  Verdicts against the C oracle, bit for bit.

The pool is 32,768 triples signed on the device; one verify call leaves every
item's H in the workspace record.  About 1.2 % of the items have H = 34 and a
few H >= 35 (tests/test_halve_tail_host.py); they are the tail items the calls
below place among items with H <= 33:
* one tail item at lane 0, 63, 64 and 255 of a 256-item call;
* 2, 3, 5 and 9 tail items in one wave (above COA_SUMS_TAIL_MAX = 6 the workgroup
  loops max(H) times, the path without the prologue), and 5 with the threshold
  raised;
* all 64 lanes of one wave tail items (the fallback), and the same 64 with
  COA_SUMS_TAIL_MAX raised to 64 (the prologue 64 times over);
* an H >= 35 item alone, and in one wave with H = 34 items;
* tail items with one bit of s flipped beside their unmodified twins: rejected
  and accepted, so the prologue's point enters the verdict;
* a tail item beside items that fail the pre-check in its wave, and a wave of
  rejected items (H = 0) in a workgroup whose other waves have tail lanes;
* n = 200 with the only tail item last;
* the same arrays through COA_MAIN_SUMS=0: identical verdicts."""
import os

import numpy as np
import pytest

import coa_oracle as co

pytestmark = pytest.mark.gpu

POOL_N = 32768
CAP = 33


def _align(x, a=256):
    return (x + a - 1) // a * a


def _device_verify(engine, msgs, pks, sigs):
    """(verdicts, H of every item as k_pre_halve recorded it)."""
    import torch

    n = len(pks)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (msgs, pks, sigs)]
    out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = torch.zeros(engine.verify_workspace_bytes(n), dtype=torch.uint8, device=dev)
    engine.verify_strict_many_device(0, t[0], t[1], t[2], out, ws)
    torch.cuda.synchronize()
    # workspace: k [n][32] | rec [n][128] | ... (csrc/coa_sig.cpp ws_carve); word 24 = H | (d < 0) << 31
    rec = ws.cpu().numpy()[_align(n * 32):_align(n * 32) + n * 128].view(np.uint32).reshape(n, 32)
    return out.cpu().numpy(), (rec[:, 24] & 0xFF).astype(int)


class Pool:
    def __init__(self, engine):
        import torch

        from workloads import key_seeds, messages

        dev = torch.device("cuda", 0)
        self.msgs = messages(POOL_N, 8400)
        seeds = torch.from_numpy(key_seeds(POOL_N, 8400)).to(dev)
        m = torch.from_numpy(self.msgs).to(dev)
        pk = torch.empty((POOL_N, 32), dtype=torch.uint8, device=dev)
        sg = torch.empty((POOL_N, 64), dtype=torch.uint8, device=dev)
        engine.sign_many_device(0, seeds, m, pk, sg)
        torch.cuda.synchronize()
        self.pks, self.sigs = pk.cpu().numpy(), sg.cpu().numpy()
        got, self.H = _device_verify(engine, self.msgs, self.pks, self.sigs)
        assert (got == 0).all()
        self.flat = np.nonzero(self.H <= CAP)[0]
        self.t34 = np.nonzero(self.H == 34)[0]
        self.t35 = np.nonzero(self.H >= 35)[0]

    def call(self, n, tails):
        """n items with H <= 33, pool item tails[pos] at position pos."""
        idx = self.flat[:n].copy()
        for pos, item in tails.items():
            idx[pos] = item
        return idx, self.msgs[idx].copy(), self.pks[idx].copy(), self.sigs[idx].copy()


@pytest.fixture(scope="module")
def pool(engine):
    old = {k: os.environ.get(k) for k in ("COA_MAIN_SUMS", "COA_LAT_MAX")}
    os.environ.update(COA_MAIN_SUMS="1", COA_LAT_MAX="0")
    try:
        return Pool(engine)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture
def sums(monkeypatch):
    monkeypatch.setenv("COA_MAIN_SUMS", "1")
    monkeypatch.setenv("COA_LAT_MAX", "0")
    monkeypatch.delenv("COA_SUMS_TAIL_MAX", raising=False)


def _check(engine, pool, idx, msgs, pks, sigs, want=None):
    """Device verdicts == the oracle's (== want when given); the records hold the pool's H."""
    exp = co.verify_strict_many(msgs, pks, sigs, min(16, os.cpu_count() or 1))
    if want is not None:
        assert (exp == want).all(), np.nonzero(exp != want)[0][:20]
    got, H = _device_verify(engine, msgs, pks, sigs)
    assert (H == pool.H[idx]).all(), "k depends on (R, A, M) only: the items keep their H"
    mism = np.nonzero(got != exp)[0]
    assert mism.size == 0, [(int(i), int(H[i]), int(got[i]), int(exp[i])) for i in mism[:20]]
    return got


def test_pool_has_tail_items(pool):
    """The model expects about 390 items with H = 34 and about 13 above."""
    print("pool H histogram:", dict(zip(*[a.tolist() for a in np.unique(pool.H, return_counts=True)])))
    assert len(pool.t34) >= 64
    assert len(pool.t35) >= 1
    assert len(pool.flat) >= POOL_N * 0.97


@pytest.mark.parametrize("lane", [0, 63, 64, 255])
def test_one_tail_item(engine, sums, pool, lane):
    idx, m, p, s = pool.call(256, {lane: pool.t34[lane % 7]})
    _check(engine, pool, idx, m, p, s, np.zeros(256, np.uint8))
    s[lane, 32] ^= 1  # s stays below l (the oracle's verdict says so); k and H do not depend on s
    want = np.zeros(256, np.uint8)
    want[lane] = 1
    _check(engine, pool, idx, m, p, s, want)


@pytest.mark.parametrize("count,tail_max", [(2, None), (3, None), (5, None), (9, None), (5, 8)])
def test_several_tail_items_in_one_wave(engine, sums, pool, monkeypatch, count, tail_max):
    if tail_max is not None:
        monkeypatch.setenv("COA_SUMS_TAIL_MAX", str(tail_max))
    lanes = [64 + 7 * j for j in range(count)]  # wave 1 of a 300-item call
    idx, m, p, s = pool.call(300, {ln: pool.t34[j] for j, ln in enumerate(lanes)})
    _check(engine, pool, idx, m, p, s, np.zeros(300, np.uint8))
    for ln in lanes[::2]:
        s[ln, 32] ^= 1
    want = np.zeros(300, np.uint8)
    want[lanes[::2]] = 1
    _check(engine, pool, idx, m, p, s, want)


@pytest.mark.parametrize("tail_max", [None, 64], ids=["fallback", "threshold-raised"])
def test_whole_wave_of_tail_items(engine, sums, pool, monkeypatch, tail_max):
    if tail_max is not None:
        monkeypatch.setenv("COA_SUMS_TAIL_MAX", str(tail_max))
    tails = {128 + j: pool.t34[j] for j in range(64)}
    if tail_max is not None:
        tails[128 + 9] = pool.t35[0]
    idx, m, p, s = pool.call(512, tails)
    for ln in (128, 150, 191):
        s[ln, 32] ^= 1
    want = np.zeros(512, np.uint8)
    want[[128, 150, 191]] = 1
    _check(engine, pool, idx, m, p, s, want)


def test_deep_tail_item_alone(engine, sums, pool):
    deep = pool.t35[np.argmax(pool.H[pool.t35])]
    idx, m, p, s = pool.call(256, {100: deep})
    _check(engine, pool, idx, m, p, s, np.zeros(256, np.uint8))
    s[100, 32] ^= 1
    want = np.zeros(256, np.uint8)
    want[100] = 1
    _check(engine, pool, idx, m, p, s, want)


def test_deep_tail_item_among_others(engine, sums, pool):
    """Different excess lengths in one wave's loop."""
    tails = {70: pool.t34[0], 71: pool.t35[0], 127: pool.t34[2], 130: pool.t34[1], 200: pool.t35[-1]}
    idx, m, p, s = pool.call(256, tails)
    _check(engine, pool, idx, m, p, s, np.zeros(256, np.uint8))
    s[71, 32] ^= 1
    s[127, 40] ^= 0x10
    want = np.zeros(256, np.uint8)
    want[[71, 127]] = 1
    _check(engine, pool, idx, m, p, s, want)


def test_tail_item_beside_pre_check_failures(engine, sums, pool):
    idx, m, p, s = pool.call(256, {5: pool.t34[3], 40: pool.t34[4]})
    bad = [0, 4, 6, 39, 41, 63]
    for i in bad:
        s[i, 63] = 0xFF  # s >= l: rejected by k_pre_halve, H = 0 for the main kernel
    want = np.zeros(256, np.uint8)
    want[bad] = 1
    _check(engine, pool, idx, m, p, s, want)


def test_rejected_wave_beside_tail_waves(engine, sums, pool):
    tails = {3: pool.t34[5], 130: pool.t34[6], 255: pool.t35[0]}
    idx, m, p, s = pool.call(256, tails)
    for i in range(64, 128):
        s[i, 63] = 0xFF
    want = np.zeros(256, np.uint8)
    want[64:128] = 1
    _check(engine, pool, idx, m, p, s, want)


def test_tail_item_last_of_a_partial_workgroup(engine, sums, pool):
    idx, m, p, s = pool.call(200, {199: pool.t34[7]})
    _check(engine, pool, idx, m, p, s, np.zeros(200, np.uint8))
    s[199, 32] ^= 1
    want = np.zeros(200, np.uint8)
    want[199] = 1
    _check(engine, pool, idx, m, p, s, want)


def test_agrees_with_one_lane_kernels(engine, pool, monkeypatch):
    tails = {21 * j + 5: pool.t34[8 + j] for j in range(24)}  # three in every wave
    tails[299] = pool.t35[0]
    idx, m, p, s = pool.call(512, tails)
    flipped = sorted(tails)[::3] + [1, 2]
    for i in flipped:
        s[i, 32] ^= 1
    monkeypatch.setenv("COA_LAT_MAX", "0")
    monkeypatch.delenv("COA_SUMS_TAIL_MAX", raising=False)
    res = {}
    for v in ("0", "1"):
        monkeypatch.setenv("COA_MAIN_SUMS", v)
        res[v], _ = _device_verify(engine, m, p, s)
    assert (res["0"] == res["1"]).all(), np.nonzero(res["0"] != res["1"])[0][:20]
    want = np.zeros(512, np.uint8)
    want[flipped] = 1
    assert (res["1"] == want).all()
    assert (co.verify_strict_many(m, p, s, min(16, os.cpu_count() or 1)) == want).all()

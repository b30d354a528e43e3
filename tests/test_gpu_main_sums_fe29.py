"""GPU: k_verify_main_sums29 (csrc/coa_halved.hip), the digit-sums main kernel
with the consumers' accumulator on 29-bit limbs (csrc/coa_ge29.h), forced with
COA_MAIN_SUMS=1 at every size (COA_LAT_MAX=0 keeps small calls off the latency
route).  Verdicts against the C oracle, bit for bit, and every array again
through COA_SUMS_FE29=0 (the radix-2^32 accumulator, k_verify_main_sums) and
through COA_MAIN_SUMS=0 (the one-lane kernels): identical verdict arrays.

* ragged sizes on adversarial_mix with the mixed-order pool: one live lane
  (n = 1, the first launch of a kernel with more than 64 KiB of static LDS), a
  dead consumer / producer pair (64, 65), the 256-item workgroup edge (255, 256,
  257), a partial last workgroup (769);
* barrier uniformity at n = 512: a wave pair, and a whole workgroup, rejected
  by the pre-check (H = 0) beside pairs at ~33 digits;
* tail lanes (H >= 34, their top digits from the row prologue in the
  radix-2^32 field, converted to limbs once) from a device-signed pool of 8,192:
  one at lane 0, 63, 64 and 255 of a 256-item call; three in one wave; nine in
  one wave, which takes the uncapped fallback; a tail item with one bit of s
  flipped beside its unmodified twin."""
import os

import numpy as np
import pytest

import coa_oracle as co
from conftest import load_golden

pytestmark = pytest.mark.gpu

POOL_N = 8192
CAP = 33
# (COA_MAIN_SUMS, COA_SUMS_FE29): the kernel under test, then the two it must agree with
ROUTES = {"fe29": ("1", "1"), "radix32": ("1", "0"), "one-lane": ("0", "1")}


def _mixed_pool():
    return [(bytes.fromhex(v["msg"]), bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]))
            for v in load_golden("mixed_order_pool.json")]


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


def _all_routes(engine, monkeypatch, msgs, pks, sigs):
    """The oracle's verdicts, after asserting that all three routes give them."""
    exp = co.verify_strict_many(msgs, pks, sigs, min(16, os.cpu_count() or 1))
    monkeypatch.setenv("COA_LAT_MAX", "0")
    for name, (main_sums, fe29) in ROUTES.items():
        monkeypatch.setenv("COA_MAIN_SUMS", main_sums)
        monkeypatch.setenv("COA_SUMS_FE29", fe29)
        got, H = _device_verify(engine, msgs, pks, sigs)
        mism = np.nonzero(got != exp)[0]
        assert mism.size == 0, (name, [(int(i), int(H[i]), int(got[i]), int(exp[i])) for i in mism[:20]])
    return exp


def _signed(engine, n, tag):
    from workloads import key_seeds, messages

    msgs = messages(n, tag)
    pks, sigs = engine.sign_many(key_seeds(n, tag), msgs)
    return msgs, pks, sigs


@pytest.mark.parametrize("n", [1, 64, 65, 255, 256, 257, 769])
def test_ragged_sizes_vs_oracle(engine, monkeypatch, n):
    from workloads import adversarial_mix

    m0, pks, sigs = _signed(engine, n, 8500)
    msgs, pks, sigs, cls = adversarial_mix(m0, pks, sigs, frac=0.3, seed=n, mixed_pool=_mixed_pool())
    if n >= 64:  # round(0.3 n) >= 8 mutated items: one of each class at least
        assert set(np.unique(cls[cls >= 0])) == set(range(8))
    exp = _all_routes(engine, monkeypatch, msgs, pks, sigs)
    assert (exp[cls == -1] == 0).all()


@pytest.mark.parametrize("rejected", [range(64, 128), range(0, 256)], ids=["wave-pair", "workgroup"])
def test_barrier_uniformity(engine, monkeypatch, rejected):
    """Items whose s >= l fail k_pre_halve's check: their wave pair (or whole
    workgroup) has H = 0 of its own while the other pairs run ~33 digits."""
    n = 512
    msgs, pks, sigs = _signed(engine, n, 8600)
    for i in rejected:
        sigs[i, 63] = 0xFF
    want = np.zeros(n, np.uint8)
    want[list(rejected)] = 1
    assert (_all_routes(engine, monkeypatch, msgs, pks, sigs) == want).all()


# ------------------------------------------------------------------ tail lanes
class Pool:
    def __init__(self, engine):
        import torch

        from workloads import key_seeds, messages

        dev = torch.device("cuda", 0)
        self.msgs = messages(POOL_N, 8700)
        seeds = torch.from_numpy(key_seeds(POOL_N, 8700)).to(dev)
        m = torch.from_numpy(self.msgs).to(dev)
        pk = torch.empty((POOL_N, 32), dtype=torch.uint8, device=dev)
        sg = torch.empty((POOL_N, 64), dtype=torch.uint8, device=dev)
        engine.sign_many_device(0, seeds, m, pk, sg)
        torch.cuda.synchronize()
        self.pks, self.sigs = pk.cpu().numpy(), sg.cpu().numpy()
        got, self.H = _device_verify(engine, self.msgs, self.pks, self.sigs)
        assert (got == 0).all()
        self.flat = np.nonzero(self.H <= CAP)[0]
        self.tail = np.nonzero(self.H > CAP)[0]

    def call(self, n, tails):
        """n items with H <= 33, pool item tails[pos] at position pos."""
        idx = self.flat[:n].copy()
        for pos, item in tails.items():
            idx[pos] = item
        return self.msgs[idx].copy(), self.pks[idx].copy(), self.sigs[idx].copy()


@pytest.fixture(scope="module")
def pool(engine):
    old = {k: os.environ.get(k) for k in ("COA_MAIN_SUMS", "COA_LAT_MAX", "COA_SUMS_FE29")}
    os.environ.update(COA_MAIN_SUMS="1", COA_LAT_MAX="0", COA_SUMS_FE29="1")
    try:
        return Pool(engine)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_pool_has_tail_items(pool):
    """About 1.2 % of the items have H >= 34 (tests/test_halve_tail_host.py): ~95 of 8,192."""
    assert len(pool.tail) >= 40, len(pool.tail)
    assert len(pool.flat) >= POOL_N * 0.97


@pytest.mark.parametrize("lane", [0, 63, 64, 255])
def test_one_tail_item(engine, monkeypatch, pool, lane):
    m, p, s = pool.call(256, {lane: pool.tail[lane % 7]})
    assert (_all_routes(engine, monkeypatch, m, p, s) == 0).all()


@pytest.mark.parametrize("count", [3, 9], ids=["three-capped", "nine-uncapped-fallback"])
def test_several_tail_items_in_one_wave(engine, monkeypatch, pool, count):
    monkeypatch.delenv("COA_SUMS_TAIL_MAX", raising=False)  # 6: nine tail lanes in a wave lift the cap
    lanes = [64 + 7 * j for j in range(count)]  # wave 1 of a 300-item call
    m, p, s = pool.call(300, {ln: pool.tail[10 + j] for j, ln in enumerate(lanes)})
    assert (_all_routes(engine, monkeypatch, m, p, s) == 0).all()
    for ln in lanes[::2]:
        s[ln, 32] ^= 1  # s stays below l (the oracle's verdict says so); k and H do not depend on s
    want = np.zeros(300, np.uint8)
    want[lanes[::2]] = 1
    assert (_all_routes(engine, monkeypatch, m, p, s) == want).all()


def test_flipped_tail_item_beside_its_twin(engine, monkeypatch, pool):
    """The same tail item twice in one wave, one copy with a bit of s flipped:
    rejected and accepted, so the prologue's point enters the verdict."""
    item = pool.tail[20]
    m, p, s = pool.call(256, {130: item, 131: item})
    s[131, 32] ^= 1
    want = np.zeros(256, np.uint8)
    want[131] = 1
    assert (_all_routes(engine, monkeypatch, m, p, s) == want).all()

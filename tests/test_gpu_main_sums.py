"""GPU: k_verify_main_sums (csrc/coa_halved.hip), the main kernel whose digit
sums A_tab[dc] + R_tab[dr] come from a second wave through LDS, forced with
COA_MAIN_SUMS=1 at every size (COA_LAT_MAX=0 keeps small calls off the latency
route).  Verdicts against the C oracle, bit for bit.

* ragged sizes: one live lane, a dead consumer / producer pair (n = 64, 65),
  the 256-item workgroup edge (255, 256, 257), a partial last workgroup (769);
* barrier uniformity: a wave pair, and a whole workgroup, whose items are all
  rejected by k_pre_halve (H = 0) beside pairs at ~33 digits -- every wave of a
  workgroup must still execute the same barriers;
* signs: at n = 769 the halving records the kernel read hold both signs of d
  and positive and negative digits in both digit strings;
* the same mix through the one-lane kernels (COA_MAIN_SUMS=0) gives the same
  verdict array."""
import os

import numpy as np
import pytest

import coa_oracle as co
from conftest import load_golden

pytestmark = pytest.mark.gpu


def _pool():
    return [(bytes.fromhex(v["msg"]), bytes.fromhex(v["pk"]), bytes.fromhex(v["sig"]))
            for v in load_golden("mixed_order_pool.json")]


def _align(x, a=256):
    return (x + a - 1) // a * a


def _device_verify(engine, msgs, pks, sigs, want_ws=False):
    import torch

    n = len(pks)
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(a).to(dev) for a in (msgs, pks, sigs)]
    out = torch.full((n,), 7, dtype=torch.uint8, device=dev)
    ws = torch.zeros(engine.verify_workspace_bytes(n), dtype=torch.uint8, device=dev)
    engine.verify_strict_many_device(0, t[0], t[1], t[2], out, ws)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    return (got, ws.cpu().numpy()) if want_ws else got


def _signed(engine, n, tag):
    from workloads import key_seeds, messages

    msgs = messages(n, tag)
    pks, sigs = engine.sign_many(key_seeds(n, tag), msgs)
    return msgs, pks, sigs


@pytest.fixture
def sums(monkeypatch):
    monkeypatch.setenv("COA_MAIN_SUMS", "1")
    monkeypatch.setenv("COA_LAT_MAX", "0")


@pytest.mark.parametrize("n", [1, 64, 65, 255, 256, 257, 769])
def test_ragged_sizes_vs_oracle(engine, sums, n):
    from workloads import adversarial_mix

    m0, pks, sigs = _signed(engine, n, 8100)
    msgs, pks, sigs, cls = adversarial_mix(m0, pks, sigs, frac=0.3, seed=n, mixed_pool=_pool())
    if n >= 64:  # round(0.3 n) >= 8 mutated items: one of each class at least
        assert set(np.unique(cls[cls >= 0])) == set(range(8))
    exp = co.verify_strict_many(msgs, pks, sigs, 1)
    got, ws = _device_verify(engine, msgs, pks, sigs, want_ws=True)
    mism = np.nonzero(got != exp)[0]
    assert mism.size == 0, [(int(i), int(cls[i]), int(got[i])) for i in mism[:20]]
    assert (got[cls == -1] == 0).all()
    if n == 769:
        # the records k_pre_halve wrote (workspace: k [n][32] | rec [n][128] | ...,
        # csrc/coa_sig.cpp ws_carve): word 24 = H | (d < 0) << 31, words 0..7 /
        # 8..15 the digits of c / |d| as nibbles + 8; accepted items only
        rec = ws[_align(n * 32):_align(n * 32) + n * 128].view(np.uint32).reshape(n, 32)[got == 0]
        assert len(rec) > 400
        dneg = rec[:, 24] >> 31
        assert set(np.unique(dneg)) == {0, 1}, "both signs of d"
        for name, words in (("c", rec[:, 0:8]), ("d", rec[:, 8:16])):
            nib = np.stack([(words[:, p >> 3] >> np.uint32(4 * (p & 7))) & 15 for p in range(64)], axis=1).astype(int) - 8
            live = np.arange(64)[None, :] < (rec[:, 24] & 0xFF)[:, None]
            assert (nib[~live] == 0).all(), "digits at and above H are zero"
            assert (nib[live] < 0).any() and (nib[live] > 0).any() and (nib[live] == 0).any(), name
        # the R digit's effective sign is the digit's times d's: all four pairs of
        # (A digit < 0, R digit < 0) reach ge_add_cc_il
        hh = (rec[:, 24] & 0xFF).astype(int)
        pairs = set()
        for r, h, dn in zip(rec, hh, dneg):
            for p in range(h):
                dc = int((r[p >> 3] >> (4 * (p & 7))) & 15) - 8
                dd = int((r[8 + (p >> 3)] >> (4 * (p & 7))) & 15) - 8
                dr = -dd if dn else dd
                if dc and dr:
                    pairs.add((dc < 0, dr < 0))
            if len(pairs) == 4:
                break
        assert len(pairs) == 4


@pytest.mark.parametrize("rejected", [range(64, 128), range(0, 256)], ids=["wave-pair", "workgroup"])
def test_barrier_uniformity(engine, sums, rejected):
    """Items whose s >= l fail k_pre_halve's check: their wave pair (or whole
    workgroup) has H = 0 of its own while the other pairs run ~33 digits."""
    n = 512
    msgs, pks, sigs = _signed(engine, n, 8200)
    for i in rejected:
        sigs[i, 63] = 0xFF
    exp = co.verify_strict_many(msgs, pks, sigs, 1)
    want = np.zeros(n, np.uint8)
    want[list(rejected)] = 1
    assert (exp == want).all()
    got = _device_verify(engine, msgs, pks, sigs)
    assert (got == want).all(), np.nonzero(got != want)[0][:20]


def test_agrees_with_one_lane_kernels(engine, monkeypatch):
    from workloads import adversarial_mix

    n = 2048
    m0, pks, sigs = _signed(engine, n, 8300)
    msgs, pks, sigs, cls = adversarial_mix(m0, pks, sigs, frac=0.1, seed=83, mixed_pool=_pool())
    assert set(np.unique(cls[cls >= 0])) == set(range(8))
    monkeypatch.setenv("COA_LAT_MAX", "0")
    res = {}
    for v in ("0", "1"):
        monkeypatch.setenv("COA_MAIN_SUMS", v)
        res[v] = _device_verify(engine, msgs, pks, sigs)
    assert (res["0"] == res["1"]).all(), np.nonzero(res["0"] != res["1"])[0][:20]
    exp = co.verify_strict_many(msgs, pks, sigs, min(16, os.cpu_count() or 1))
    assert (res["1"] == exp).all()

"""Probe: how many radix-16 digits the halved scalars of a C2 call need, and
what the items above 33 digits cost k_verify_main_sums.

The halving record's word 24 holds H = (max(bits c, bits d) + 5) / 4.
k_verify_main_sums loops max(H) times over each 256-item workgroup, and at C2
(one workgroup per CU) the kernel lasts as long as its longest workgroup.

1. the bench's C2 inputs (workloads.key_seeds / messages, signed on the
   device), one verify call, H of every accepted item from the workspace
   (k [n][32] | rec [n][128] | ..., csrc/coa_sig.cpp ws_carve): histogram,
   per-256-item maxima, global maximum;
2. a second set of the same size whose items all have H <= 33 (sign ~7 % more,
   drop the tail items, keep the first n);
3. the verify call on both sets: HIP events around --calls calls after a
   warm-up, the sets alternated --reps times in this one process.  The
   difference is all that shortening the tail can win.

Writes one JSON (default profiles/halve_width_hist.json) with the CPU model's
figures (exact Euclid on (8l, k) with coa_halve.h's candidate rule, 400,000
uniform k; tests/test_halve_tail_host.py holds the model) beside the device's.

    python tools/halve_width_hist.py [--n 65536] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))

CAP = 33
CPU_MODEL = {"sample": "400,000 uniform k, exact Euclid with the candidate rule of coa_halve.h",
             "share_H_le_33": 0.9878, "share_H_34": 0.0118, "share_H_ge_35": 4.0e-4, "share_H_ge_36": 3.8e-5,
             "share_H_ge_37": 2.5e-6, "workgroups_256_max_ge_34": 0.957, "waves_64_max_ge_34": 0.54,
             "calls_65536_max_ge_35": 1.0, "calls_65536_max_ge_36": 0.91}


def _align(x, a=256):
    return (x + a - 1) // a * a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halve_width_hist.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import coa_crypto
    import workloads

    n = a.n
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    coa_crypto.init(1)
    # an explicit stream: a NULL handle selects the engine's own stream in the
    # C ABI, and the timing events below would then bracket nothing
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)

    def signed(count):
        seeds = torch.from_numpy(workloads.key_seeds(count)).to(dev)
        msgs = torch.from_numpy(workloads.messages(count)).to(dev)
        pks = torch.empty((count, 32), dtype=torch.uint8, device=dev)
        sigs = torch.empty((count, 64), dtype=torch.uint8, device=dev)
        coa_crypto.sign_many_device(0, seeds, msgs, pks, sigs)
        torch.cuda.synchronize()
        return msgs, pks, sigs

    def widths(msgs, pks, sigs):
        """H of every item (0 where the item was rejected)."""
        cnt = pks.shape[0]
        out = torch.ones(cnt, dtype=torch.uint8, device=dev)
        ws = torch.zeros(coa_crypto.verify_workspace_bytes(cnt), dtype=torch.uint8, device=dev)
        coa_crypto.verify_strict_many_device(0, msgs, pks, sigs, out, ws)
        torch.cuda.synchronize()
        rec = ws.cpu().numpy()[_align(cnt * 32):_align(cnt * 32) + cnt * 128].view(np.uint32).reshape(cnt, 32)
        acc = out.cpu().numpy() == 0
        return np.where(acc, rec[:, 24] & 0xFF, 0).astype(int), acc

    # 1. the bench's inputs
    nat = signed(n)
    h, acc = widths(*nat)
    assert acc.all(), "a valid benchmark signature was rejected"
    hist = {int(v): int(c) for v, c in zip(*np.unique(h, return_counts=True))}
    wg = h[:n // 256 * 256].reshape(-1, 256).max(axis=1)
    wv = h[:n // 64 * 64].reshape(-1, 64).max(axis=1)
    device = {"n": n, "hist_H": hist, "share_H_le_33": float((h <= CAP).mean()), "share_H_34": float((h == 34).mean()),
              "share_H_ge_35": float((h >= 35).mean()), "share_H_ge_36": float((h >= 36).mean()),
              "workgroup_256_max_hist": {int(v): int(c) for v, c in zip(*np.unique(wg, return_counts=True))},
              "workgroups_256_max_ge_34": float((wg >= 34).mean()), "waves_64_max_ge_34": float((wv >= 34).mean()),
              "mean_workgroup_max": float(wg.mean()), "global_max": int(h.max()),
              "mean_tail_lanes_per_wave": float((h > CAP).sum() / (n / 64))}

    # 2. the same size with no item above the cap
    big = signed(n + n // 14 + 256)
    hb, accb = widths(*big)
    keep = np.nonzero(accb & (hb <= CAP))[0][:n]
    assert len(keep) == n, "not enough items at or below the cap"
    idx = torch.from_numpy(keep).to(dev)
    flat = tuple(t[idx].contiguous() for t in big)
    del big
    hf, _ = widths(*flat)
    assert hf.max() <= CAP and hf.min() > 0

    # 3. timing, the two sets alternated
    out = torch.ones(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(coa_crypto.verify_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def timed(s, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            coa_crypto.verify_strict_many_device(0, s[0], s[1], s[2], out, ws, stream)
        e1.record(stream)
        torch.cuda.synchronize()
        assert int(out.sum().item()) == 0
        return e0.elapsed_time(e1) / calls

    for s in (nat, flat):
        timed(s, a.warmup)
    t_nat, t_flat = [], []
    for _ in range(a.reps):
        t_nat.append(timed(nat, a.calls))
        t_flat.append(timed(flat, a.calls))
    med_nat, med_flat = float(np.median(t_nat)), float(np.median(t_flat))
    res = {"cap": CAP, "cpu_model": CPU_MODEL, "device": device,
           "timing": {"calls": a.calls, "reps": a.reps, "natural_ms": [round(t, 5) for t in t_nat],
                      "all_le_cap_ms": [round(t, 5) for t in t_flat], "natural_median_ms": round(med_nat, 5),
                      "all_le_cap_median_ms": round(med_flat, 5), "upper_bound_ms": round(med_nat - med_flat, 5),
                      "upper_bound_share_of_call": round((med_nat - med_flat) / med_nat, 5),
                      "natural_spread": round((max(t_nat) - min(t_nat)) / med_nat, 5)}}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"device": {k: v for k, v in device.items() if k != "hist_H"}, "hist_H": hist,
                      "timing": res["timing"]}))


if __name__ == "__main__":
    main()

"""Probe: what one tail lane costs k_verify_main_sums' row prologue against one
more digit of the loop -- the break-even behind COA_SUMS_TAIL_MAX
(csrc/coa_sums_tail.h).

Signs 2^20 triples on the device, reads every item's H from the workspace
record, and builds C2-sized calls in which every 64-item wave holds exactly k
items with H = 34 among items with H <= 33.  Each call is timed (HIP events
around --calls calls) with the cap in force at every k (COA_SUMS_TAIL_MAX=64)
and without it (COA_SUMS_TAIL_MAX=-1: the loop runs max(H) digits), the two
alternated.  One digit time is the uncapped call minus the k = 0 call; one
tail lane's prologue is the slope of the capped calls over k.

    python tools/sums_tail_breakeven.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=1 << 20)
    ap.add_argument("--ks", default="0,1,2,4,8,12")
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sums_tail_breakeven.json"))
    a = ap.parse_args()

    import numpy as np
    import torch

    import coa_crypto
    import workloads

    n, ks = a.n, [int(x) for x in a.ks.split(",")]
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    coa_crypto.init(1)
    stream = torch.cuda.Stream(dev)  # never the NULL handle, which selects the engine's own stream
    torch.cuda.set_stream(stream)

    seeds = torch.from_numpy(workloads.key_seeds(a.pool, start=1 << 24)).to(dev)
    msgs = torch.from_numpy(workloads.messages(a.pool, start=1 << 24)).to(dev)
    pks = torch.empty((a.pool, 32), dtype=torch.uint8, device=dev)
    sigs = torch.empty((a.pool, 64), dtype=torch.uint8, device=dev)
    coa_crypto.sign_many_device(0, seeds, msgs, pks, sigs)
    out = torch.ones(a.pool, dtype=torch.uint8, device=dev)
    ws = torch.zeros(coa_crypto.verify_workspace_bytes(a.pool), dtype=torch.uint8, device=dev)
    coa_crypto.verify_strict_many_device(0, msgs, pks, sigs, out, ws, stream)
    torch.cuda.synchronize()
    assert int(out.sum().item()) == 0
    off = (a.pool * 32 + 255) // 256 * 256
    h = (ws[off:off + a.pool * 128].cpu().numpy().view(np.uint32).reshape(a.pool, 32)[:, 24] & 0xFF).astype(int)
    del ws, out, seeds
    flat, t34 = np.nonzero(h <= 33)[0], np.nonzero(h == 34)[0]
    assert len(t34) >= max(ks) * (n // 64), f"{len(t34)} items with H = 34"

    sets = {}
    for k in ks:
        idx = flat[:n].copy().reshape(n // 64, 64)
        if k:
            idx[:, 5:5 + 4 * k:4] = t34[:k * (n // 64)].reshape(n // 64, k)
        ii = torch.from_numpy(idx.reshape(-1)).to(dev)
        sets[k] = tuple(t[ii].contiguous() for t in (msgs, pks, sigs))
    del msgs, pks, sigs
    out = torch.ones(n, dtype=torch.uint8, device=dev)
    ws = torch.empty(coa_crypto.verify_workspace_bytes(n), dtype=torch.uint8, device=dev)

    def timed(s, tail_max, calls):
        os.environ["COA_SUMS_TAIL_MAX"] = str(tail_max)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            coa_crypto.verify_strict_many_device(0, s[0], s[1], s[2], out, ws, stream)
        e1.record(stream)
        torch.cuda.synchronize()
        assert int(out.sum().item()) == 0
        return e0.elapsed_time(e1) / calls

    for k in ks:
        timed(sets[k], 64, 10)
    rows = {k: {"capped_ms": [], "uncapped_ms": []} for k in ks}
    for _ in range(a.reps):
        for k in ks:
            rows[k]["capped_ms"].append(round(timed(sets[k], 64, a.calls), 5))
            rows[k]["uncapped_ms"].append(round(timed(sets[k], -1, a.calls), 5))
    med = {k: (float(np.median(r["capped_ms"])), float(np.median(r["uncapped_ms"]))) for k, r in rows.items()}
    kk = [k for k in ks if k]
    digit = float(np.median([med[k][1] for k in kk])) - med[0][1]
    slope = float(np.polyfit(ks, [med[k][0] for k in ks], 1)[0])
    res = {"n": n, "calls": a.calls, "reps": a.reps, "tail_lanes_per_wave": {str(k): rows[k] for k in ks},
           "median_ms": {str(k): {"capped": round(c, 5), "uncapped": round(u, 5)} for k, (c, u) in med.items()},
           "one_more_digit_ms": round(digit, 5), "per_tail_lane_ms": round(slope, 5),
           "break_even_tail_lanes": round(digit / slope, 2) if slope > 0 else None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "tail_lanes_per_wave"}))


if __name__ == "__main__":
    main()

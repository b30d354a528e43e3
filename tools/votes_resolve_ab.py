"""A/B: open certificates decided on the device
(coa_certificate_votes_resolve_device) against the route a device-resident
caller had before it, on the C3 round (committee 100, 10,000 certificates of 67
votes and 32 payload entries, resident in HBM) with 0 %, 1 % and 10 % of the
certificates made open by flipping one bit of one vote's s.

  a  coa_certificate_verdict_many_device alone (it leaves COA_DAG_VOTES_OPEN)
  b  a, then coa_certificate_votes_resolve_device on the same stream with a
     caller workspace (derived weights, --seed)
  c  a, then what the caller did itself: the words to the host, the open
     certificates' ids, rounds, origins and votes gathered on the device and
     copied to the host, Certificate::digest by hashlib,
     coa_ed25519_verify_batch_groups (the same seed), the words back

All three alternate in ONE process after a warm-up.  Every arm is timed by the
host's clock from its first call to the stream drained (c cannot be timed any
other way); a and b also by device events around their calls.

    python tools/votes_resolve_ab.py [--reps 12] [--cap 0] [--out FILE] [--git-head SHA]
"""
import argparse
import hashlib
import json
import os
import statistics
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))

import numpy as np  # noqa: E402

OK, INVALID_VOTES, OPEN = 0, 8, 9


def _git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--certs", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--cap", type=int, default=0, help="open_votes_cap of arm b (0 = every vote)")
    ap.add_argument("--percents", default="0,1,10")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "votes_resolve_ab.json"))
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    args = ap.parse_args()
    assert args.reps >= 10, "at least 10 alternating sets"
    import torch

    import certificates as C
    import coa_crypto as cc

    cc.init(1)
    L = cc.lib()
    n = args.certs
    committee, b = C.synth_certificates(n, committee_size=100, n_payload=32, seed=3)
    assert committee.register_authorities() == 100
    hdata = np.frombuffer(b"".join(b.header_inputs) + bytes(16), np.uint8)
    hoff = np.zeros(n + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in b.header_inputs])
    rounds = np.full(n, b.round, np.uint64)
    pcounts = np.full(n, 32, np.uint32)
    offs = np.ascontiguousarray(b.offsets, np.uint64)
    nv = int(offs[-1])
    dev = torch.device("cuda", 0)
    record = {"tool": "tools/votes_resolve_ab.py", "git_head": args.git_head or _git_head(),
              "device": torch.cuda.get_device_name(0), "committee": 100, "certificates": n, "votes": nv,
              "payload_entries": 32, "rng_seed": args.seed, "open_votes_cap": args.cap,
              "resolve_workspace_bytes": cc.certificate_votes_resolve_workspace_bytes(n, nv, args.cap),
              "timing": "host clock from the arm's first call to the stream drained; *_events: device events "
                        "around the calls", "rows": {}}

    def T(a):
        a = np.array(a)  # a writable, contiguous copy
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        return torch.from_numpy(a).to(dev)

    stream = torch.cuda.Stream(dev)
    ws_v = torch.empty(cc.certificate_verdict_workspace_bytes(n, nv), dtype=torch.uint8, device=dev)
    ws_r = torch.empty(max(record["resolve_workspace_bytes"], 16), dtype=torch.uint8, device=dev)
    words = torch.empty(n, dtype=torch.int32, device=dev)
    counts = torch.zeros(3, dtype=torch.int32, device=dev)
    d_pc = T(pcounts)
    fixed = [T(x) for x in (hdata, hoff, b.ids, b.authors, b.header_sigs, rounds, b.vote_pks)]
    d_off = T(offs)
    offs_i = offs.astype(np.int64)

    for pct in [int(x) for x in args.percents.split(",")]:
        vs = np.array(b.vote_sigs, np.uint8)
        rng = np.random.default_rng(0xC3 + pct)
        victims = np.sort(rng.permutation(n)[:n * pct // 100])
        at = offs_i[victims] + rng.integers(0, 67, victims.size)
        vs[at, 40] ^= 1  # one bit of s: the vote fails its own equation, the certificate stays well formed
        d_vs = T(vs)
        d = fixed + [d_vs, d_off]  # hdata hoff ids origins hsigs rounds vpks vsigs voff
        want = np.zeros(n, np.uint32)
        want[victims] = INVALID_VOTES
        open_votes = int((offs_i[victims + 1] - offs_i[victims]).sum())

        def verdict():
            cc.certificate_verdict_many_device(0, *d, d_pc, words, stream, ws_v)

        def resolve():
            cc.certificate_votes_resolve_device(0, d[2], d[3], d[5], d[6], d[7], d[8], words, rng_seed=args.seed,
                                                open_votes_cap=args.cap, counts=counts, stream=stream, workspace=ws_r)

        def arm_a():
            verdict()

        def arm_b():
            verdict()
            resolve()

        def arm_c():
            verdict()
            w = words.cpu().numpy().view(np.uint32)  # waits for the stream
            open_at = np.flatnonzero(w == OPEN)
            if open_at.size == 0:
                return
            lo, hi = offs_i[open_at], offs_i[open_at + 1]
            goff = np.zeros(open_at.size + 1, np.uint64)
            goff[1:] = np.cumsum(hi - lo)
            vidx = np.concatenate([np.arange(a_, b_) for a_, b_ in zip(lo, hi)])
            ci, vi = torch.from_numpy(open_at).to(dev), torch.from_numpy(vidx).to(dev)
            ids, origins, rnd, vp, vsg = (t.index_select(0, i).cpu().numpy()
                                          for t, i in ((d[2], ci), (d[3], ci), (d[5], ci), (d[6], vi), (d[7], vi)))
            msgs = np.frombuffer(b"".join(
                hashlib.sha512(ids[j].tobytes() + struct.pack("<Q", int(rnd[j]) & (2 ** 64 - 1)) +
                               origins[j].tobytes()).digest()[:32] for j in range(open_at.size)), np.uint8)
            out = np.full(open_at.size, 0xff, np.uint8)
            rc = L.coa_ed25519_verify_batch_groups(msgs.ctypes.data, vp.ctypes.data, vsg.ctypes.data, goff.ctypes.data,
                                                   open_at.size, out.ctypes.data, args.seed)
            assert rc == 0, rc
            w = w.copy()
            w[open_at] = np.where(out, INVALID_VOTES, OK)
            words.copy_(torch.from_numpy(w.view(np.int32)), non_blocking=False)

        def check(arm):
            torch.cuda.synchronize()
            got = words.cpu().numpy().view(np.uint32)
            if arm == "a":
                assert (got[victims] == OPEN).all() and not np.delete(got, victims).any(), "arm a: open exactly there"
            else:
                assert (got == want).all(), f"arm {arm}: INVALID_VOTES exactly at the flipped certificates"
            if arm == "b":
                assert counts.cpu().numpy().tolist() == [victims.size, victims.size, open_votes]

        wall = {"a": [], "b": [], "c": []}
        events = {"a": [], "b": []}
        arms = (("a", arm_a), ("b", arm_b), ("c", arm_c))
        with torch.cuda.stream(stream):
            for _ in range(2):  # warm-up, and each arm's answer checked once
                for name, fn in arms:
                    fn()
                    check(name)
            for _ in range(args.reps):
                for name, fn in arms:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    stream.synchronize()
                    wall[name].append((time.perf_counter() - t0) * 1e3)
                    if name in events:
                        events[name].append(e0.elapsed_time(e1))
        row = {"open_certificates": int(victims.size), "open_votes": open_votes,
               "a_verdict_alone": _stats(wall["a"]), "b_verdict_then_device_resolve": _stats(wall["b"]),
               "c_verdict_then_host_route": _stats(wall["c"]), "a_events": _stats(events["a"]),
               "b_events": _stats(events["b"])}
        bm, cm, am = (row[k]["median_ms"] for k in ("b_verdict_then_device_resolve", "c_verdict_then_host_route",
                                                    "a_verdict_alone"))
        row["b_minus_a_median_ms"] = round(bm - am, 4)
        row["b_minus_a_events_median_ms"] = round(row["b_events"]["median_ms"] - row["a_events"]["median_ms"], 4)
        row["c_over_b_median"] = round(cm / bm, 3)
        if pct:
            row["b_below_c"] = bool(bm < cm)
        else:
            row["b_within_a_spread"] = bool(row["a_verdict_alone"]["min_ms"] <= bm <= row["a_verdict_alone"]["max_ms"])
            row["b_events_within_a_events_spread"] = bool(
                row["a_events"]["min_ms"] <= row["b_events"]["median_ms"] <= row["a_events"]["max_ms"])
        record["rows"][f"{pct}_percent_open"] = row
        print(json.dumps({f"{pct}_percent_open": row}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    bad = [k for k, r in record["rows"].items() if r.get("b_below_c") is False]
    if bad:
        sys.exit(f"arm b is not below arm c at {bad}")


if __name__ == "__main__":
    main()

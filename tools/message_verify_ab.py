"""A/B: Header::verify / Vote::verify crypto for n device-resident messages.

  A  the per-primitive route of sanitize.py / PreVerifier:
     coa_sha512_many_device over the digest inputs, then
     coa_ed25519_verify_strict_many_device (k_pre_halve + k_verify_main: every
     signer a stranger).  Votes need the 32-byte digest prefixes packed in
     between (a strided device copy, timed as part of A; headers verify
     header.id, which is already packed).
  B  coa_header_verify_many_device / coa_vote_verify_many_device: one
     k_msg_verify launch over the registered committee's key combs.

Committee of 100 registered keys, signers drawn from it, C3-size header
digest inputs (3,336 B).  Both routes run in ONE process on one stream,
alternating, after a warm-up of every shape, with device events around each
run; the verdicts of A and B are compared.  A few items are corrupted so the
comparison is not between all-zero arrays.

    python tools/message_verify_ab.py [--sizes 128,2048,65536] [--reps 20] [--out FILE] [--only-b] [--git-head SHA]

Writes the record (median, min, max per route and size, git head, sha256 of
the kernel source) as JSON to --out and prints it.  --only-b runs route B
alone at the largest size (for a kernel trace of k_msg_verify).
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))

import numpy as np  # noqa: E402

HEADER_BYTES = 3336
KERNEL_SOURCE = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc", "coa_committee.hip")  # k_msg_verify


def _git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


class Inputs:
    """n headers and n votes signed on the device by committee members."""

    def __init__(self, cc, torch, n, seeds, pks, rng):
        dev = torch.device("cuda", 0)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.n = n
        who = rng.integers(0, len(pks), n)
        d_seeds = T(seeds[who])
        self.authors = T(pks[who])
        # headers: author || random bytes, id = SHA-512(bytes)[..32], signed by the author
        hdr = rng.integers(0, 256, (n, HEADER_BYTES), dtype=np.uint8)
        hdr[:, :32] = pks[who]
        self.hdata = T(hdr.reshape(-1))
        self.hoff = T((np.arange(n + 1, dtype=np.int64) * HEADER_BYTES))
        out64 = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        # (the engine's calls on torch's default stream go to the engine's own
        # non-blocking stream: wait for each before torch touches its output)
        cc.sha512_many_device(0, self.hdata, self.hoff, out64)
        torch.cuda.synchronize()
        self.hids = out64[:, :32].contiguous()
        self.hsigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        pk_out = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        cc.sign_many_device(0, d_seeds, self.hids, pk_out, self.hsigs)
        # votes: id || round LE || origin (72 B), signed by the voter over its digest
        vids = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        rounds = rng.integers(1, 1 << 40, n).astype(np.int64)
        origins = pks[rng.integers(0, len(pks), n)]
        vin = np.concatenate([vids, rounds.view(np.uint8).reshape(n, 8), origins], axis=1)
        self.vin = T(vin.reshape(-1))
        self.voff = T(np.arange(n + 1, dtype=np.int64) * 72)
        self.vids, self.rounds, self.origins = T(vids), T(rounds), T(origins)
        torch.cuda.synchronize()
        cc.sha512_many_device(0, self.vin, self.voff, out64)
        torch.cuda.synchronize()
        vdig = out64[:, :32].contiguous()
        self.vsigs = torch.empty((n, 64), dtype=torch.uint8, device=dev)
        cc.sign_many_device(0, d_seeds, vdig, pk_out, self.vsigs)
        torch.cuda.synchronize()
        assert bool((pk_out == self.authors).all())
        # corrupt a few items: signatures, a header byte, a vote's round
        k = max(1, n // 64)
        self.hsigs[:k, 40] ^= 1
        self.vsigs[:k, 40] ^= 1
        self.hdata.view(n, HEADER_BYTES)[k:2 * k, 100] ^= 1
        self.rounds[k:2 * k] += 1
        self.vin.view(n, 72)[k:2 * k, 32:40] = self.rounds[k:2 * k].view(torch.uint8).view(-1, 8)
        # outputs and workspaces
        self.out64 = out64
        self.msg32 = torch.empty((n, 32), dtype=torch.uint8, device=dev)
        self.verdicts = torch.empty(n, dtype=torch.uint8, device=dev)
        self.status = torch.empty(n, dtype=torch.int32, device=dev)
        self.ws_a = torch.empty(cc.verify_workspace_bytes(n), dtype=torch.uint8, device=dev)
        self.ws_b = torch.empty(cc.message_workspace_bytes(n), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()


def _routes(cc, x, stream):
    def a_headers():
        cc.sha512_many_device(0, x.hdata, x.hoff, x.out64, stream)
        cc.verify_strict_many_device(0, x.hids, x.authors, x.hsigs, x.verdicts, x.ws_a, stream)

    def a_votes():
        cc.sha512_many_device(0, x.vin, x.voff, x.out64, stream)
        x.msg32.copy_(x.out64[:, :32])
        cc.verify_strict_many_device(0, x.msg32, x.authors, x.vsigs, x.verdicts, x.ws_a, stream)

    def b_headers():
        cc.header_verify_many_device(0, x.hdata, x.hoff, x.hids, x.authors, x.hsigs, x.status, stream, x.ws_b)

    def b_votes():
        cc.vote_verify_many_device(0, x.vids, x.rounds, x.origins, x.authors, x.vsigs, x.status, stream, x.ws_b)

    return {"headers": (a_headers, b_headers), "votes": (a_votes, b_votes)}


def _results(torch, x, kind, route):
    """Status per item (headers: bit 1 id, bit 2 signature; votes: 0 / 1)."""
    torch.cuda.synchronize()
    if route == "A":
        v = x.verdicts.to(torch.int32)
        if kind == "votes":
            return v.cpu().numpy()
        bad_id = (x.out64[:, :32] != x.hids).any(dim=1).to(torch.int32)
        return (bad_id | (v << 1)).cpu().numpy()
    st = x.status.cpu().numpy()
    assert not (st & 16).any(), "an author is not registered"
    return st if kind == "headers" else (st >> 1)


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,2048,65536")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "message_verify_ab.json"))
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    args = ap.parse_args()
    import torch

    import coa_crypto as cc
    import workloads

    cc.init(1)
    seeds = workloads.key_seeds(100)
    pks = cc.public_keys(seeds)
    assert cc.committee_register(pks) == 100
    sizes = [int(s) for s in args.sizes.split(",")]
    rng = np.random.default_rng(12)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    record = {"tool": "tools/message_verify_ab.py", "git_head": args.git_head or _git_head(),
              "kernel_source": os.path.relpath(KERNEL_SOURCE, ROOT),
              "kernel_source_sha256": hashlib.sha256(open(KERNEL_SOURCE, "rb").read()).hexdigest(),
              "device": torch.cuda.get_device_name(0), "committee": 100, "header_bytes": HEADER_BYTES,
              "A": "coa_sha512_many_device + coa_ed25519_verify_strict_many_device",
              "B": "coa_header_verify_many_device / coa_vote_verify_many_device (k_msg_verify)", "results": []}
    if args.only_b:
        x = Inputs(cc, torch, max(sizes), seeds, pks, rng)
        with torch.cuda.stream(stream):
            for kind, (_, b) in _routes(cc, x, stream).items():
                for _ in range(3):
                    b()
        torch.cuda.synchronize()
        print(json.dumps({"only_b": max(sizes)}))
        return
    inputs = {n: Inputs(cc, torch, n, seeds, pks, rng) for n in sizes}
    with torch.cuda.stream(stream):
        for n in sizes:  # warm-up of every shape; the verdicts of A and B compared
            for kind, (a, b) in _routes(cc, inputs[n], stream).items():
                for _ in range(2):
                    a()
                    b()
                ra, rb = _results(torch, inputs[n], kind, "A"), _results(torch, inputs[n], kind, "B")
                assert (ra == rb).all(), (n, kind, int((ra != rb).sum()))
                assert 0 < int((ra != 0).sum()) < n, (n, kind, np.bincount(ra, minlength=4).tolist())
        for n in sizes:
            for kind, (a, b) in _routes(cc, inputs[n], stream).items():
                ta, tb = [], []
                for _ in range(args.reps):
                    for fn, acc in ((a, ta), (b, tb)):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        fn()
                        e1.record(stream)
                        e1.synchronize()
                        acc.append(e0.elapsed_time(e1))
                ra, rb = _results(torch, inputs[n], kind, "A"), _results(torch, inputs[n], kind, "B")
                row = {"kind": kind, "n": n, "A": _stats(ta), "B": _stats(tb), "verdicts_equal": bool((ra == rb).all()),
                       "rejected": int((rb != 0).sum())}
                row["A_over_B_median"] = round(row["A"]["median_ms"] / row["B"]["median_ms"], 3)
                row["B_beats_A_by_more_than_A_spread"] = bool(
                    row["A"]["median_ms"] - row["B"]["median_ms"] > row["A"]["max_ms"] - row["A"]["min_ms"])
                record["results"].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

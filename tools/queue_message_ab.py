"""Headers and votes through the aggregation queue: what the header / vote
request kinds and the message latency kernel are worth.

  (a) device-side sweep, window sizes 1 .. 8,192, headers and votes apart:
      L  k_msg_verify_lat (coa_msg_lat_verify_device, one workgroup per message)
      T  k_msg_verify (coa_header_verify_many_device / coa_vote_verify_many_device)
      alternated on one stream with device events around each run.  The
      largest swept size at which L is not slower than T, for both kinds, is
      what COA_QUEUE_MSG_LAT_MAX should default to (recorded as
      "msg_lat_max_supported").
  (b) per-request wait p50 / p99 (coa_queue_metrics) at 100 and 1,000
      requests/s from one paced producer, idle launch on;
  (c) time to drain 65,536 headers and 65,536 votes from 4 producers;
      (b) and (c) for both routes of tools/latc.c latc_queue_messages, in turn
      in one process on one queue:
      M  whole messages (coa_queue_submit_header / coa_queue_submit_vote)
      P  the parent route: the producer hashes on the host (and, for a
         header, does the id check) and calls coa_queue_submit_verify
      with the spread of the repeats.  Every answer is checked against the
      throughput kernels' verdicts.

Committee of 100 registered keys, signers drawn from it, C3-size header digest
inputs (3,336 B), a few items corrupted.  Every shape is warmed first.

    python tools/queue_message_ab.py [--reps 3] [--sweep-reps 20] [--out FILE] [--git-head SHA] [--skip-queue]

Writes the record as JSON to --out and prints each row.  No threshold is fixed
in advance: the file records what was found.
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from message_verify_ab import HEADER_BYTES, Inputs, _git_head, _stats  # noqa: E402

# k_msg_verify_lat
KERNEL_SOURCE = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc", "coa_cert_lat.hip")

SWEEP = (1, 16, 64, 128, 512, 2048, 8192)
DRAIN = 65536


def _sweep(cc, torch, x, stream, reps):
    """One size: rows for headers and votes, L and T alternated."""
    n = x.n
    st_l = torch.empty(n, dtype=torch.int32, device=x.status.device)
    heads = (x.hdata, x.hoff, x.hids, x.authors, x.hsigs)
    votes = (x.vids, x.rounds, x.origins, x.authors, x.vsigs)
    routes = {
        "headers": (lambda: cc.message_lat_verify_device(0, heads, None, st_l, stream),
                    lambda: cc.header_verify_many_device(0, *heads, x.status, stream, x.ws_b)),
        "votes": (lambda: cc.message_lat_verify_device(0, None, votes, st_l, stream),
                  lambda: cc.vote_verify_many_device(0, *votes, x.status, stream, x.ws_b)),
    }
    rows = []
    with torch.cuda.stream(stream):
        for kind, (lat, tp) in routes.items():
            for _ in range(3):  # warm-up of this shape, the words compared
                lat()
                tp()
            torch.cuda.synchronize()
            equal = bool((st_l == x.status).all())
            tl, tt = [], []
            for _ in range(reps):
                for fn, acc in ((lat, tl), (tp, tt)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    acc.append(e0.elapsed_time(e1))
            row = {"part": "a", "kind": kind, "n": n, "L": _stats(tl), "T": _stats(tt), "words_equal": equal}
            row["L_not_slower"] = row["L"]["median_ms"] <= row["T"]["median_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _host(x, torch):
    """Host arrays of the inputs and the expected answers (the throughput
    kernels' words, every author registered)."""
    torch.cuda.synchronize()
    c = lambda t: np.ascontiguousarray(t.cpu().numpy())  # noqa: E731
    return {"hdata": c(x.hdata), "hoff": c(x.hoff).view(np.uint64), "hids": c(x.hids), "authors": c(x.authors),
            "hsigs": c(x.hsigs), "vids": c(x.vids), "rounds": c(x.rounds).view(np.uint64), "origins": c(x.origins),
            "vsigs": c(x.vsigs)}


def _expected(cc, torch, x, stream):
    with torch.cuda.stream(stream):
        cc.header_verify_many_device(0, x.hdata, x.hoff, x.hids, x.authors, x.hsigs, x.status, stream, x.ws_b)
        torch.cuda.synchronize()
        h = x.status.cpu().numpy().astype(np.uint8)
        cc.vote_verify_many_device(0, x.vids, x.rounds, x.origins, x.authors, x.vsigs, x.status, stream, x.ws_b)
        torch.cuda.synchronize()
        v = (x.status.cpu().numpy() >> 1).astype(np.uint8)
    assert not ((h | v) & 0xF0).any() and 0 < int((h != 0).sum()) < x.n and 0 < int(v.sum()) < x.n
    return np.ascontiguousarray(h), np.ascontiguousarray(v)


class Producer:
    """tools/latc.c latc_queue_messages over one queue."""

    def __init__(self, cc):
        self.cc = cc
        self.latc = ctypes.CDLL(os.path.join(ROOT, "xrpl-coa-prototype_amd", "lib", "liblatc.so"))
        vp = ctypes.c_void_p
        self.latc.latc_queue_messages.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                                  ctypes.c_double, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp,
                                                  ctypes.POINTER(ctypes.c_double)]
        self.latc.latc_queue_messages.restype = ctypes.c_int
        self.q = cc.lib().coa_queue_create(65536, 500)
        assert self.q
        assert cc.lib().coa_queue_set_idle_launch(self.q, 1) == 0

    def run(self, h, expect, route, votes, producers, rate, n):
        """One run over the first n messages; (elapsed s, queue metrics)."""
        L = self.cc.lib()
        assert L.coa_queue_metrics_reset(self.q) == 0
        el = ctypes.c_double()
        p = lambda a: a.ctypes.data  # noqa: E731
        ids, sigs = (h["vids"], h["vsigs"]) if votes else (h["hids"], h["hsigs"])
        wrong = self.latc.latc_queue_messages(self.q, route, int(votes), producers, 1, float(rate), p(h["hdata"]),
                                              p(h["hoff"]), p(ids), p(h["rounds"]), p(h["origins"]), p(h["authors"]),
                                              p(sigs), n, p(expect), ctypes.byref(el))
        assert wrong == 0, (route, votes, n, wrong)
        m = self.cc.QueueMetrics()
        assert L.coa_queue_metrics(self.q, ctypes.byref(m)) == 0
        return el.value, self.cc.metrics_dict(m)

    def close(self):
        self.cc.lib().coa_queue_destroy(self.q)


def _spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "reps": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_message_ab.json"))
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    ap.add_argument("--skip-queue", action="store_true", help="part (a) only")
    args = ap.parse_args()
    import torch

    import coa_crypto as cc
    import workloads

    cc.init(1)
    seeds = workloads.key_seeds(100)
    pks = cc.public_keys(seeds)
    assert cc.committee_register(pks) == 100
    rng = np.random.default_rng(12)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    record = {"tool": "tools/queue_message_ab.py", "git_head": args.git_head or _git_head(),
              "kernel_source": os.path.relpath(KERNEL_SOURCE, ROOT),
              "kernel_source_sha256": hashlib.sha256(open(KERNEL_SOURCE, "rb").read()).hexdigest(),
              "device": torch.cuda.get_device_name(0), "committee": 100, "header_bytes": HEADER_BYTES,
              "L": "k_msg_verify_lat (coa_msg_lat_verify_device)", "T": "k_msg_verify (the throughput device forms)",
              "M": "coa_queue_submit_header / coa_queue_submit_vote",
              "P": "host SHA-512 (and header id check) + coa_queue_submit_verify",
              "msg_lat_max_env": os.environ.get("COA_QUEUE_MSG_LAT_MAX"), "results": []}
    # (a)
    for n in SWEEP:
        record["results"] += _sweep(cc, torch, Inputs(cc, torch, n, seeds, pks, rng), stream, args.sweep_reps)
    ok = {k: [r["n"] for r in record["results"] if r["kind"] == k and r["L_not_slower"]] for k in ("headers", "votes")}
    both = sorted(set(ok["headers"]) & set(ok["votes"]))
    record["msg_lat_max_supported"] = both[-1] if both else 0
    record["L_not_slower_at"] = ok
    print(json.dumps({"msg_lat_max_supported": record["msg_lat_max_supported"], "L_not_slower_at": ok}), flush=True)
    if not args.skip_queue:
        x = Inputs(cc, torch, DRAIN, seeds, pks, rng)
        hexp, vexp = _expected(cc, torch, x, stream)
        h = _host(x, torch)
        pr = Producer(cc)
        try:
            for votes, expect in ((False, hexp), (True, vexp)):
                kind = "votes" if votes else "headers"
                # (b) paced, one producer, ~1.5 s of arrivals per run
                for rate in (100, 1000):
                    n = int(rate * 1.5)
                    for route in (0, 1):  # warm-up of this shape
                        pr.run(h, expect, route, votes, 1, rate * 10, n)
                    acc = {0: {"p50": [], "p99": []}, 1: {"p50": [], "p99": []}}
                    windows = {0: [], 1: []}
                    for _ in range(args.reps):
                        for route in (0, 1):
                            _, m = pr.run(h, expect, route, votes, 1, rate, n)
                            acc[route]["p50"].append(m["wait_us_p50"])
                            acc[route]["p99"].append(m["wait_us_p99"])
                            windows[route].append(m["windows"])
                    row = {"part": "b", "kind": kind, "rate_per_s": rate, "requests": n,
                           "M_wait_us_p50": _spread(acc[0]["p50"]), "M_wait_us_p99": _spread(acc[0]["p99"]),
                           "P_wait_us_p50": _spread(acc[1]["p50"]), "P_wait_us_p99": _spread(acc[1]["p99"]),
                           "M_windows": windows[0], "P_windows": windows[1]}
                    record["results"].append(row)
                    print(json.dumps(row), flush=True)
                # (c) drain
                for route in (0, 1):
                    pr.run(h, expect, route, votes, 4, 0, DRAIN)
                t = {0: [], 1: []}
                for _ in range(args.reps):
                    for route in (0, 1):
                        el, m = pr.run(h, expect, route, votes, 4, 0, DRAIN)
                        t[route].append(el * 1e3)
                row = {"part": "c", "kind": kind, "n": DRAIN, "producers": 4, "M_drain_ms": _spread(t[0]),
                       "P_drain_ms": _spread(t[1])}
                row["P_over_M_median"] = round(row["P_drain_ms"]["median"] / row["M_drain_ms"]["median"], 3)
                record["results"].append(row)
                print(json.dumps(row), flush=True)
        finally:
            pr.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

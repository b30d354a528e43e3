"""Per-request wait of lone crypto header and vote requests
(coa_queue_submit_header / coa_queue_submit_vote) through the aggregation
queue of the build in --tree: one paced producer at 100 and 1,000 requests/s,
idle launch on, p50 / p99 from coa_queue_metrics.

Uses only what that tree has itself (its tools/queue_message_ab.py, its engine
library and its tools/latc.c), so it runs against an earlier build of the
project as well as this one: tools/queue_verdict_ab.py --parent-tree starts it
in processes of its own, the two builds alternated, for the parent's
lone-request p50.

    python tools/queue_paced_crypto.py --tree DIR [--reps 3]

Prints one JSON line per (kind, rate).
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", required=True, help="a built checkout of the project")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, os.path.join(tree, "xrpl-coa-prototype_amd"))
    sys.path.insert(0, os.path.join(tree, "tools"))
    import numpy as np
    import torch

    import coa_crypto as cc
    import workloads
    from message_verify_ab import Inputs
    from queue_message_ab import Producer, _expected, _host, _spread

    assert os.path.abspath(cc.__file__).startswith(tree), cc.__file__
    cc.init(1)
    seeds = workloads.key_seeds(100)
    pks = cc.public_keys(seeds)
    assert cc.committee_register(pks) == 100
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    x = Inputs(cc, torch, 2048, seeds, pks, np.random.default_rng(12))
    hexp, vexp = _expected(cc, torch, x, stream)
    h = _host(x, torch)
    pr = Producer(cc)
    try:
        for votes, expect in ((False, hexp), (True, vexp)):
            for rate in (100, 1000):
                n = int(rate * 1.5)
                pr.run(h, expect, 0, votes, 1, rate * 10, n)  # warm-up of this shape
                p50, p99 = [], []
                for _ in range(args.reps):
                    _, m = pr.run(h, expect, 0, votes, 1, rate, n)
                    p50.append(m["wait_us_p50"])
                    p99.append(m["wait_us_p99"])
                print(json.dumps({"kind": "votes" if votes else "headers", "rate_per_s": rate, "requests": n,
                                  "wait_us_p50": _spread(p50), "wait_us_p99": _spread(p99)}), flush=True)
    finally:
        pr.close()
        cc.committee_register(np.zeros((0, 32), np.uint8))


if __name__ == "__main__":
    main()

"""A/B of two builds of the aggregation queue's front end (csrc/coa_queue.cpp)
on the CPU, with tools/queue_host_bench.cpp: each binary is that program built
with one coa_queue.cpp and its stub backend (no GPU).

Shapes: 4 producers borrowed, 4 producers copied, 1 producer borrowed; 20,000
certificates per producer, device_us 300.  The two binaries alternate, `--pairs`
runs each per shape, the order within a pair swapped from one pair to the
next.  Per shape the figures are certificates/s and the intake, gather and
callbacks stages per window; the new build's median must lie within the
parent's own [min, max] over these runs, in both directions.

    g++ -O2 -std=c++17 -pthread -I include -I <tree>/xrpl-coa-prototype_amd/csrc \
        <tree>/xrpl-coa-prototype_amd/csrc/coa_queue.cpp tools/queue_host_bench.cpp -o <bin>
    python tools/queue_front_ab.py --parent-bin A --new-bin B --parent-head SHA --new-head SHA
"""
import argparse
import json
import os
import re
import statistics
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"4_producers_borrowed": (4, 1), "4_producers_copied": (4, 0), "1_producer_borrowed": (1, 1)}
FIGURES = ("certs_per_s", "intake", "gather", "callbacks")


def run(binary, producers, borrowed, per, device_us):
    r = subprocess.run([binary, str(producers), str(per), str(device_us), str(borrowed)], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    row = {"certs_per_s": float(re.search(r"([\d.]+) certs/s", r.stdout).group(1))}
    for stage in FIGURES[1:]:
        row[stage] = float(re.search(rf" {stage} ([\d.]+)", r.stdout).group(1))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-bin", required=True)
    ap.add_argument("--new-bin", required=True)
    ap.add_argument("--parent-head")
    ap.add_argument("--new-head")
    ap.add_argument("--pairs", type=int, default=10)
    ap.add_argument("--per-producer", type=int, default=20_000)
    ap.add_argument("--device-us", type=int, default=300)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_front_ab.json"))
    args = ap.parse_args()
    bins = {"parent": args.parent_bin, "new": args.new_bin}
    record = {"tool": "tools/queue_front_ab.py", "parent_head": args.parent_head, "new_head": args.new_head,
              "pairs": args.pairs, "certificates_per_producer": args.per_producer, "device_us": args.device_us,
              "stages": "microseconds per window",
              "margin": "the new build's median lies within [min, max] of the parent's own runs", "shapes": {}}
    verdict = True
    for shape, (producers, borrowed) in SHAPES.items():
        runs = {"parent": [], "new": []}
        for k in range(args.pairs):
            for which in (("parent", "new"), ("new", "parent"))[k % 2]:
                runs[which].append(run(bins[which], producers, borrowed, args.per_producer, args.device_us))
        rec = {}
        for fig in FIGURES:
            pa, nw = [r[fig] for r in runs["parent"]], [r[fig] for r in runs["new"]]
            med = statistics.median(nw)
            ok = min(pa) <= med <= max(pa)
            verdict = verdict and ok
            rec[fig] = {"parent": {"runs": pa, "median": statistics.median(pa), "min": min(pa), "max": max(pa)},
                        "new": {"runs": nw, "median": med, "min": min(nw), "max": max(nw)},
                        "within_parent_spread": ok}
            print(shape, fig, "parent", rec[fig]["parent"]["median"], [min(pa), max(pa)], "new", med, "within", ok,
                  flush=True)
        record["shapes"][shape] = rec
    record["within_parent_spread"] = verdict
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out, "verdict", verdict)


if __name__ == "__main__":
    main()

"""A/B of two builds of the engine library on the lines that go through the
aggregation queue's HIP backend (csrc/coa_queue_hip.cpp over coa_qstage.h),
measured with bench.py's own sections:

  c3_stream_4        streamed C3 (committee 100, 10,000 certificates of 67
                     votes a round, borrowed) from 4 producers: certificates/s,
                     and the `pack` and `scatter` entries of coa_queue_metrics'
                     stage_us per window on that run
  round_mix_1000     queue_round_mix at 1,000 rounds/s: certificate p50, p99
  round_mix_c1_10    queue_round_mix_c1 with idle launch at 10 rounds/s:
                     certificate and signature p50 (the inline and publish
                     routes, where a microsecond of host code shows)

Each measurement runs in a fresh child process that loads one library
(COA_VERIFY_LIB); parent and new alternate, `--pairs` of them, the order
within a pair swapped from one pair to the next.

    python tools/qstage_ab.py --parent-lib DIR/libcoa_verify.so --parent-head SHA --new-head SHA
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))


def child(args):
    import ctypes

    import numpy as np
    import torch  # noqa: F401  (first: one HIP runtime in the process)

    import bench
    import certificates as C
    import coa_crypto as cc

    cc.init(1)
    out = {"lib": cc.LIB_PATH}
    n = args.certs
    committee, batch = C.synth_certificates(n, committee_size=100, n_payload=32, seed=3)
    assert committee.register_authorities() == 100
    hd = np.frombuffer(b"".join(batch.header_inputs) + bytes(16), np.uint8)
    hoff = np.zeros(n + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in batch.header_inputs])
    arrs = [hd, hoff, np.ascontiguousarray(batch.ids), np.ascontiguousarray(batch.authors),
            np.ascontiguousarray(batch.header_sigs), np.full(n, batch.round, np.uint64),
            np.ascontiguousarray(batch.vote_pks), np.ascontiguousarray(batch.vote_sigs),
            np.ascontiguousarray(batch.offsets)]
    expect = np.zeros(n, np.uint8)
    lib = bench._latc()
    vp, sz, ci, dp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    lib.latc_stream_certificates.argtypes = [sz, ctypes.c_uint, ci, ci, ci, ctypes.c_double] + [vp] * 9 + [sz, vp, dp, vp]
    lib.latc_stream_certificates.restype = ci
    s = bench.c3_stream(lib, [a.ctypes.data for a in arrs], n, expect, producer_counts=(4,), borrowed_modes=(1,),
                        rates=())["producers_4"]
    st = s["diag"]["stage_us_per_window"]
    out["c3_stream_4"] = {"certs_per_s": s["certs_per_s"], "windows": s["windows"], "pack_us_per_window": st["pack"],
                          "scatter_us_per_window": st["scatter"], "staging_grows": s["diag"]["staging_grows"]}
    cc.committee_register(np.zeros((0, 32), np.uint8))

    r = bench.queue_round_mix(rates=(1000,))["rates"]["1000"]["certificate"]
    out["round_mix_1000"] = {"p50_ms": r["p50_ms"], "p99_ms": r["p99_ms"]}
    r = bench.queue_round_mix(rates=(10,), committee_size=4, n_payload=1)["rates_idle_launch"]["10"]
    out["round_mix_c1_10"] = {"certificate_p50_ms": r["certificate"]["p50_ms"],
                              "signature_p50_ms": r["signature"]["p50_ms"]}
    print("CHILD " + json.dumps(out), flush=True)


# line -> (how to read it from a child's row, whether higher is better)
FIGURES = {"c3_stream_4_certs_per_s": (lambda r: r["c3_stream_4"]["certs_per_s"], True),
           "c3_stream_4_pack_us_per_window": (lambda r: r["c3_stream_4"]["pack_us_per_window"], False),
           "c3_stream_4_scatter_us_per_window": (lambda r: r["c3_stream_4"]["scatter_us_per_window"], False),
           "round_mix_1000_p50_ms": (lambda r: r["round_mix_1000"]["p50_ms"], False),
           "round_mix_1000_p99_ms": (lambda r: r["round_mix_1000"]["p99_ms"], False),
           "round_mix_c1_10_idle_certificate_p50_ms": (lambda r: r["round_mix_c1_10"]["certificate_p50_ms"], False),
           "round_mix_c1_10_idle_signature_p50_ms": (lambda r: r["round_mix_c1_10"]["signature_p50_ms"], False)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--certs", type=int, default=10_000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-head")
    ap.add_argument("--new-head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qstage_ab.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = {"parent": args.parent_lib, "new": os.path.join(ROOT, "xrpl-coa-prototype_amd", "lib", "libcoa_verify.so")}
    runs = {"parent": [], "new": []}
    for k in range(args.pairs):
        for which in (("parent", "new"), ("new", "parent"))[k % 2]:  # neither build always runs second
            env = dict(os.environ, COA_VERIFY_LIB=libs[which])
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--certs", str(args.certs)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.exit(f"{which} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            row = json.loads(line[-1][6:])
            assert os.path.samefile(row["lib"], libs[which]), row["lib"]
            runs[which].append(row)
            print(k, which, json.dumps(row), flush=True)

    record = {"tool": "tools/qstage_ab.py", "parent_head": args.parent_head, "new_head": args.new_head,
              "certificates": args.certs, "votes_each": 67, "pairs": args.pairs,
              "margin": "the new build's median lies within [min, max] of the parent's own runs, or on the better side"}
    for name, (f, higher_better) in FIGURES.items():
        pa, nw = [f(r) for r in runs["parent"]], [f(r) for r in runs["new"]]
        med = statistics.median(nw)
        ok = med >= min(pa) if higher_better else med <= max(pa)
        record[name] = {"higher_is_better": higher_better,
                        "parent": {"runs": pa, "median": statistics.median(pa), "min": min(pa), "max": max(pa)},
                        "new": {"runs": nw, "median": med, "min": min(nw), "max": max(nw)},
                        "within_parent_spread": bool(ok)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    for name in FIGURES:
        print(name, "parent", record[name]["parent"], "new", record[name]["new"], "within",
              record[name]["within_parent_spread"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()

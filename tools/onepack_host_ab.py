"""A/B of two builds of the engine library on the host-pointer paths the
one-pack staging change touches, on the C3 round (committee 100, 10,000
certificates of 67 votes and 32 payload entries):

  host_round   coa_certificate_verify_many over the clean round, wall clock
  single_p50   coa_certificate_verify, one certificate per call, p50
  mix_c_calls  the mix pair again, the C calls alone over arrays packed once
  mix          tools/verdict_ab.py's `mix` section: the round with 1 % of the
               certificates holding a valid vote by a key outside the
               committee, coa_certificate_verdict_many against
               coa_certificate_verify_many, alternating

Each measurement runs in a fresh child process that loads one library
(COA_VERIFY_LIB); parent and new alternate, `--pairs` of them.

    python tools/onepack_host_ab.py --parent-lib DIR/libcoa_verify.so --parent-head SHA --new-head SHA
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))


def _ms(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4),
            "reps": len(xs)}


def child(args):
    import numpy as np
    import torch  # noqa: F401  (first: one HIP runtime in the process)

    import certificates as C
    import coa_crypto as cc
    import workloads

    cc.init(1)
    n = args.certs
    committee, b = C.synth_certificates(n, committee_size=100, n_payload=32, seed=3)
    assert committee.register_authorities() == 100
    rounds = np.full(n, b.round, np.uint64)
    pcounts = np.full(n, 32, np.uint32)
    offs = np.ascontiguousarray(b.offsets, np.uint64)
    clean = (b.header_inputs, b.ids, b.authors, b.header_sigs, rounds, b.vote_pks, b.vote_sigs, offs)
    out = {"lib": cc.LIB_PATH}

    t = []
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        st = cc.certificate_verify_many(*clean, rng_seed=5)
        t.append((time.perf_counter() - t0) * 1e3)
        assert not st.any()
    out["host_round"] = _ms(t[1:])

    vp, vs = b.vote_pks[:67], b.vote_sigs[:67]
    one = (b.header_inputs[0], b.ids[0], b.authors[0], b.header_sigs[0], b.round, vp, vs)
    t = []
    for k in range(args.single_calls + 50):
        t0 = time.perf_counter()
        assert cc.certificate_verify(*one, rng_seed=5) == 0
        t.append((time.perf_counter() - t0) * 1e3)
    out["single_p50_ms"] = round(statistics.median(t[50:]), 5)

    vp, vs = b.vote_pks.copy(), b.vote_sigs.copy()
    rng = np.random.default_rng(0xC3)
    victims = np.sort(rng.permutation(n)[:max(1, n // 100)])
    at = offs[victims].astype(np.int64) + rng.integers(0, 67, victims.size)
    p, s = cc.sign_many(workloads.key_seeds(victims.size, start=10 ** 6), b.cert_digests[victims])
    vp[at], vs[at] = p, s
    mixed = (b.header_inputs, b.ids, b.authors, b.header_sigs, rounds, vp, vs, offs)
    ta, tb = [], []
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        st = cc.certificate_verify_many(*mixed, rng_seed=5)
        t1 = time.perf_counter()
        vw = cc.certificate_verdict_many(*mixed, pcounts, rng_seed=5)
        t2 = time.perf_counter()
        if k:  # the first pair warms both paths up
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
    assert not st.any() and (np.flatnonzero(vw) == victims).all()
    assert ((vw[victims] & 0xff) == cc.DAG_UNKNOWN_VOTER).all()
    out["mix"] = {"crypto_only": _ms(ta), "verdict": _ms(tb),
                  "verdict_over_crypto_median": round(statistics.median(tb) / statistics.median(ta), 4)}

    # the same pair without the Python mirror's array packing: the C calls alone
    n_, hdata, hoff, ids, origins, hsigs, rnd, vpk, vsg, voff = cc._cert_arrays(*mixed)
    st8, vw32 = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    P, Q = cc._u8p, cc._u64p
    L = cc.lib()
    ta, tb = [], []
    for k in range(args.reps + 1):
        t0 = time.perf_counter()
        ra = L.coa_certificate_verify_many(P(hdata), Q(hoff), P(ids), P(origins), P(hsigs), Q(rnd), P(vpk), P(vsg),
                                           Q(voff), n, 5, P(st8))
        t1 = time.perf_counter()
        rb = L.coa_certificate_verdict_many(P(hdata), Q(hoff), P(ids), P(origins), P(hsigs), Q(rnd), P(vpk), P(vsg),
                                            Q(voff), n, 5, P(pcounts), P(vw32))
        t2 = time.perf_counter()
        assert ra == 0 and rb == 0
        if k:
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
    assert not st8.any() and (vw32 == vw).all()
    out["mix_c_calls"] = {"crypto_only": _ms(ta), "verdict": _ms(tb),
                          "verdict_over_crypto_median": round(statistics.median(tb) / statistics.median(ta), 4)}
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--certs", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--single-calls", type=int, default=400)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--parent-head")
    ap.add_argument("--new-head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onepack_host_ab.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = {"parent": args.parent_lib, "new": os.path.join(ROOT, "xrpl-coa-prototype_amd", "lib", "libcoa_verify.so")}
    runs = {"parent": [], "new": []}
    for k in range(args.pairs):
        for which in ("parent", "new"):
            env = dict(os.environ, COA_VERIFY_LIB=libs[which])
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--certs", str(args.certs), "--reps",
                   str(args.reps), "--single-calls", str(args.single_calls)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
            if r.returncode != 0 or not line:
                sys.exit(f"{which} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
            row = json.loads(line[-1][6:])
            runs[which].append(row)
            print(k, which, json.dumps(row), flush=True)

    def series(which, f):
        xs = [f(r) for r in runs[which]]
        return {"runs": xs, "median": round(statistics.median(xs), 5), "min": min(xs), "max": max(xs),
                "spread": round(max(xs) - min(xs), 5)}

    figures = {"host_round_median_ms": lambda r: r["host_round"]["median_ms"],
               "single_p50_ms": lambda r: r["single_p50_ms"],
               "mix_crypto_only_median_ms": lambda r: r["mix"]["crypto_only"]["median_ms"],
               "mix_verdict_median_ms": lambda r: r["mix"]["verdict"]["median_ms"],
               "mix_verdict_over_crypto": lambda r: r["mix"]["verdict_over_crypto_median"],
               "c_calls_crypto_only_median_ms": lambda r: r["mix_c_calls"]["crypto_only"]["median_ms"],
               "c_calls_verdict_median_ms": lambda r: r["mix_c_calls"]["verdict"]["median_ms"],
               "c_calls_verdict_over_crypto": lambda r: r["mix_c_calls"]["verdict_over_crypto_median"]}
    record = {"tool": "tools/onepack_host_ab.py", "parent_head": args.parent_head, "new_head": args.new_head,
              "certificates": args.certs, "votes_each": 67, "pairs": args.pairs,
              "margin": "new median - parent median <= parent spread (max - min of the parent's runs)"}
    for name, f in figures.items():
        pa, nw = series("parent", f), series("new", f)
        record[name] = {"parent": pa, "new": nw, "new_minus_parent_median": round(nw["median"] - pa["median"], 5),
                        "within_parent_spread": bool(nw["median"] - pa["median"] <= pa["spread"])}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    for name in figures:
        print(name, "parent", record[name]["parent"]["median"], "spread", record[name]["parent"]["spread"], "new",
              record[name]["new"]["median"], "within", record[name]["within_parent_spread"])
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""A/B of two builds of the engine library on the lines where the host runtime
(csrc/coa_engine.cpp, coa_sig.cpp, coa_dag.cpp) is a visible share of the
time -- a microsecond of entry prologue or thread-local access shows on a
one-item call -- measured with bench.py's own sections and liblatc's C loops:

  verify_single      one coa_ed25519_verify_strict per call from a C loop
                     (bench.verify_single's c_caller): p50 with the key in the
                     committee cache and with another key
  c1_certificate     one C1 coa_certificate_verify per call on an idle engine
                     (bench.latc_certificates): p50
  c2_host_65536      coa_ed25519_verify_strict_many, 65,536 host-pointer
                     triples per call, one C thread (bench.host_e2e's c2_host
                     loop, latc_verify_many): ms per call
  c3_host_round      a C3 round (10,000 certificates of 67 votes, committee
                     100) per coa_certificate_verify_many call -- the
                     pipelined path over CopyPool (host_e2e's c3_host loop,
                     latc_certificates_many): ms per round
  verify_batch_67    coa_ed25519_verify_batch_groups of one certificate's 67
                     votes (bench.verify_batch_config's single_group): p50

Each measurement runs in a fresh child process that loads one library
(COA_VERIFY_LIB, with its own liblatc.so beside it); parent and new alternate,
`--pairs` of them, the order within a pair swapped from one pair to the next.

    python tools/runtime_ab.py --parent-lib DIR/libcoa_verify.so [--new-lib LIB] --parent-head SHA --new-head SHA
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
    import torch  # first: one HIP runtime in the process

    import bench
    import certificates as C
    import coa_crypto as cc
    import workloads

    cc.init(1)
    dev = torch.device("cuda", 0)
    out = {"lib": cc.LIB_PATH}

    r = bench.verify_single(0, None, samples=2000)
    out["verify_single"] = {"committee_key_p50_ms": r["committee_key"]["c_caller"]["p50_ms"],
                            "other_key_p50_ms": r["uncached_key"]["c_caller"]["p50_ms"]}

    committee, batch = C.synth_certificates(20, committee_size=4, n_payload=1, seed=3)
    committee.register()
    out["c1_certificate"] = {"p50_ms": bench.latc_certificates(batch, 20, 1000)[0]}
    cc.committee_register(np.zeros((0, 32), np.uint8))

    out["verify_batch_67"] = {"p50_ms": bench.verify_batch_config(0, dev, torch.cuda.current_stream(dev), n_large=4096,
                                                                  samples=300, cpu_samples=1)["single_group"]["p50_ms"]}

    lib = bench._latc()
    vp, sz, ci, dp = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(ctypes.c_double)
    lib.latc_verify_many.argtypes = [vp, vp, vp, sz, ci, ci, dp]
    lib.latc_certificates_many.argtypes = [vp] * 9 + [sz, vp, ci, ci, dp]
    lib.latc_verify_many.restype = lib.latc_certificates_many.restype = ci
    el = ctypes.c_double()

    n = 65536
    msgs = workloads.messages(n)
    pks, sigs = cc.sign_many(workloads.key_seeds(n), msgs)
    m, p, s = (np.ascontiguousarray(a, dtype=np.uint8) for a in (msgs, pks, sigs))
    assert lib.latc_verify_many(m.ctypes.data, p.ctypes.data, s.ctypes.data, n, 2, 1, ctypes.byref(el)) == 0
    calls = 40
    assert lib.latc_verify_many(m.ctypes.data, p.ctypes.data, s.ctypes.data, n, calls, 1, ctypes.byref(el)) == 0
    out["c2_host_65536"] = {"ms_per_call": el.value / calls * 1e3}

    nc = args.certs
    committee, batch = C.synth_certificates(nc, committee_size=100, n_payload=32, seed=3)
    committee.register()
    hd = np.frombuffer(b"".join(batch.header_inputs) + bytes(16), np.uint8)
    hoff = np.zeros(nc + 1, np.uint64)
    hoff[1:] = np.cumsum([len(h) for h in batch.header_inputs])
    arrs = [hd, hoff, np.ascontiguousarray(batch.ids), np.ascontiguousarray(batch.authors),
            np.ascontiguousarray(batch.header_sigs), np.full(nc, batch.round, np.uint64),
            np.ascontiguousarray(batch.vote_pks), np.ascontiguousarray(batch.vote_sigs),
            np.ascontiguousarray(batch.offsets)]
    expect = np.zeros(nc, np.uint8)
    ptrs = [a.ctypes.data for a in arrs]
    assert lib.latc_certificates_many(*ptrs, nc, expect.ctypes.data, 1, 1, ctypes.byref(el)) == 0
    calls = 10
    assert lib.latc_certificates_many(*ptrs, nc, expect.ctypes.data, calls, 1, ctypes.byref(el)) == 0
    out["c3_host_round"] = {"ms_per_round": el.value / calls * 1e3}
    cc.committee_register(np.zeros((0, 32), np.uint8))
    print("CHILD " + json.dumps(out), flush=True)


# line -> how to read it from a child's row (every line: lower is better)
FIGURES = {"verify_single_committee_key_p50_ms": lambda r: r["verify_single"]["committee_key_p50_ms"],
           "verify_single_other_key_p50_ms": lambda r: r["verify_single"]["other_key_p50_ms"],
           "c1_certificate_verify_idle_p50_ms": lambda r: r["c1_certificate"]["p50_ms"],
           "c2_host_65536_ms_per_call": lambda r: r["c2_host_65536"]["ms_per_call"],
           "c3_host_round_ms": lambda r: r["c3_host_round"]["ms_per_round"],
           "verify_batch_67_p50_ms": lambda r: r["verify_batch_67"]["p50_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--certs", type=int, default=10_000)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--new-lib", default=os.path.join(ROOT, "xrpl-coa-prototype_amd", "lib", "libcoa_verify.so"),
                    help="the parent's library again measures the parent against itself (the spread to judge by)")
    ap.add_argument("--parent-head")
    ap.add_argument("--new-head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "runtime_split_ab.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    libs = {"parent": args.parent_lib, "new": args.new_lib}
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

    record = {"tool": "tools/runtime_ab.py", "parent_head": args.parent_head, "new_head": args.new_head,
              "certificates": args.certs, "votes_each": 67, "pairs": args.pairs,
              "margin": "the new build's median lies within [min, max] of the parent's own runs, or on the better side"}
    for name, f in FIGURES.items():
        pa, nw = [f(r) for r in runs["parent"]], [f(r) for r in runs["new"]]
        med = statistics.median(nw)
        record[name] = {"higher_is_better": False,
                        "parent": {"runs": pa, "median": statistics.median(pa), "min": min(pa), "max": max(pa)},
                        "new": {"runs": nw, "median": med, "min": min(nw), "max": max(nw)},
                        "within_parent_spread": bool(med <= max(pa))}
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

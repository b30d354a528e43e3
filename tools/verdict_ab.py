"""A/B: the verdict calls against the crypto-only calls on the C3 round
(committee 100, 10,000 certificates of 67 votes and 32 payload entries).

  device   coa_certificate_verdict_many_device (crypto launch + k_cert_protocol
           + k_verdict_merge) against coa_certificate_verify_many_device, the
           round resident in HBM, both on one stream of ONE process,
           alternating, device events around each call, after a warm-up.
  host     what the verdict call replaces on the host: one thread of the C++
           protocol checks alone (coa_cpu_certificate_verdict_from_status, the
           crypto bits supplied) over the same round, wall clock.
  mix      the host-pointer round with 1 % of the certificates holding a vote
           by a key outside the committee (valid signature):
           coa_certificate_verdict_many against coa_certificate_verify_many,
           alternating, wall clock.  The crypto-only call sends those
           certificates to the exact path; the verdict call answers them
           UNKNOWN_VOTER from the protocol word.

    python tools/verdict_ab.py [--reps 20] [--host-reps 5] [--out FILE] [--git-head SHA]
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

import numpy as np  # noqa: E402


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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verdict_ab.json"))
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    args = ap.parse_args()
    import torch

    import certificates as C
    import coa_crypto as cc
    import workloads

    cc.init(1)
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
    record = {"tool": "tools/verdict_ab.py", "git_head": args.git_head or _git_head(),
              "device": torch.cuda.get_device_name(0), "committee": 100, "certificates": n, "votes": nv,
              "payload_entries": 32}

    # ---- device-resident round
    dev = torch.device("cuda", 0)

    def T(a):
        a = np.array(a)  # a writable, contiguous copy
        if a.dtype == np.uint64:
            a = a.view(np.int64)
        elif a.dtype == np.uint32:
            a = a.view(np.int32)
        return torch.from_numpy(a).to(dev)

    d = [T(x) for x in (hdata, hoff, b.ids, b.authors, b.header_sigs, rounds, b.vote_pks, b.vote_sigs, offs)]
    d_pc = T(pcounts)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    words = torch.empty(n, dtype=torch.int32, device=dev)
    ws_a = torch.empty(cc.certificate_workspace_bytes(n, nv), dtype=torch.uint8, device=dev)
    ws_b = torch.empty(cc.certificate_verdict_workspace_bytes(n, nv), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream(dev)

    def crypto_only():
        cc.certificate_verify_many_device(0, *d, status, stream, ws_a)

    def verdict():
        cc.certificate_verdict_many_device(0, *d, d_pc, words, stream, ws_b)

    ta, tb = [], []
    with torch.cuda.stream(stream):
        for _ in range(3):
            crypto_only()
            verdict()
        torch.cuda.synchronize()
        assert not status.any().item() and not words.any().item(), "the clean round must be Ok in both forms"
        for _ in range(args.reps):
            for fn, acc in ((crypto_only, ta), (verdict, tb)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                e1.synchronize()
                acc.append(e0.elapsed_time(e1))
    row = {"crypto_only": _stats(ta), "verdict": _stats(tb)}
    row["verdict_over_crypto_median"] = round(row["verdict"]["median_ms"] / row["crypto_only"]["median_ms"], 4)
    row["within_10_percent"] = bool(row["verdict_over_crypto_median"] <= 1.10)
    record["device_resident"] = row
    print(json.dumps({"device_resident": row}), flush=True)

    # ---- the host side this replaces: one thread, protocol checks alone
    names = committee.authorities()
    cp, cs, cw, co, cn = cc._committee_arrays(np.array([list(bytes(k)) for k in names], np.uint8),
                                              [committee.stakes[k] for k in names],
                                              [sorted(committee.workers.get(k, {0})) for k in names])
    ids, authors, vpks = (np.ascontiguousarray(x, np.uint8) for x in (b.ids, b.authors, b.vote_pks))
    bits = np.zeros(n, np.uint8)
    out = np.full(n, 0xffffffff, np.uint32)
    th = []
    for _ in range(args.host_reps + 1):
        t0 = time.perf_counter()
        rc = cc.lib().coa_cpu_certificate_verdict_from_status(
            hdata.ctypes.data, hoff.ctypes.data, ids.ctypes.data, authors.ctypes.data, rounds.ctypes.data,
            vpks.ctypes.data, offs.ctypes.data, n, pcounts.ctypes.data, bits.ctypes.data, cp.ctypes.data,
            cs.ctypes.data, cw.ctypes.data, co.ctypes.data, cn, out.ctypes.data, 1)
        th.append((time.perf_counter() - t0) * 1e3)
        assert rc == 0 and not out.any()
    record["host_protocol_checks_one_thread"] = dict(_stats(th[1:]), what="coa_cpu_certificate_verdict_from_status")
    record["host_protocol_over_device_verdict_round"] = round(
        record["host_protocol_checks_one_thread"]["median_ms"] / row["verdict"]["median_ms"], 3)
    print(json.dumps({"host_protocol_checks_one_thread": record["host_protocol_checks_one_thread"]}), flush=True)

    # ---- host-pointer round, 1 % of the certificates with a key outside the committee
    vp, vs = b.vote_pks.copy(), b.vote_sigs.copy()
    rng = np.random.default_rng(0xC3)
    victims = np.sort(rng.permutation(n)[:max(1, n // 100)])
    at = offs[victims].astype(np.int64) + rng.integers(0, 67, victims.size)
    p, s = cc.sign_many(workloads.key_seeds(victims.size, start=10 ** 6), b.cert_digests[victims])
    vp[at], vs[at] = p, s
    host_args = (b.header_inputs, b.ids, b.authors, b.header_sigs, rounds, vp, vs, offs)
    tm_a, tm_b = [], []
    for k in range(args.host_reps + 1):
        t0 = time.perf_counter()
        st = cc.certificate_verify_many(*host_args, rng_seed=5)
        t1 = time.perf_counter()
        vw = cc.certificate_verdict_many(*host_args, pcounts, rng_seed=5)
        t2 = time.perf_counter()
        if k:  # the first pair warms both paths up
            tm_a.append((t1 - t0) * 1e3)
            tm_b.append((t2 - t1) * 1e3)
    assert not st.any(), "the outsiders' signatures are valid: the crypto bits are all Ok"
    bad = np.flatnonzero(vw)
    assert (bad == victims).all() and ((vw[victims] & 0xff) == cc.DAG_UNKNOWN_VOTER).all()
    assert ((vw[victims] >> 8).astype(np.int64) == at - offs[victims].astype(np.int64)).all()
    mix = {"outsider_certificates": int(victims.size), "crypto_only": _stats(tm_a), "verdict": _stats(tm_b),
           "note": "wall clock of the Python mirror's call, array packing included in both"}
    mix["verdict_over_crypto_median"] = round(mix["verdict"]["median_ms"] / mix["crypto_only"]["median_ms"], 4)
    record["host_pointer_adversarial_mix"] = mix
    print(json.dumps({"host_pointer_adversarial_mix": mix}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

"""Headers and votes through the aggregation queue as whole-verdict requests:
what deciding Header::verify / Vote::verify's protocol checks in the window
(k_msg_verdict_lat for a window of up to COA_QUEUE_MSG_LAT_MAX message
verdicts, k_window_verdict behind the crypto kernels otherwise) costs and saves
against the crypto requests of the same build.

  (a) device-side sweep, 1, 64, 128 and 512 messages, headers and votes apart,
      alternated: V k_msg_verdict_lat (coa_msg_lat_verdict_device) against
      L k_msg_verify_lat (coa_msg_lat_verify_device) -- what the protocol code
      in the signature job costs, and whether COA_QUEUE_MSG_LAT_MAX's default,
      found for L against the throughput kernels, holds for V;
  (b) per-request wait p50 / p99 (coa_queue_metrics) at 100 and 1,000
      requests/s from one paced producer, idle launch on -- a lone request per
      window;
  (c) time to drain 65,536 headers and 65,536 votes from 4 producers;
      both for the two routes of tools/latc.c latc_queue_verdict_messages,
      alternated in one process on one queue:
      V  verdict requests (coa_queue_submit_header_verdict /
         coa_queue_submit_vote_verdict): the word comes back with the window
      C  crypto requests (coa_queue_submit_header / coa_queue_submit_vote),
         then ONE host thread runs the protocol checks (stake lookup, worker
         ids) for all of them and merges the words; (b)'s waits are the crypto
         answers' alone, (c)'s time includes the host checks (reported apart)
      with the spread of the repeats.  Every word of either route is checked.

Committee of 100 registered authorities (two without stake), signers drawn
from it, C3-size header digest inputs (3,336 B) with 8 payload entries each;
every authority's worker ids are the ones its headers name, except for one
header in 97 whose last id stays foreign (MalformedHeader).  A few items carry
a bad id or signature.  The expected words restate primary/src/messages.rs
48-67 and 131-142 over the throughput kernels' crypto bits and the
construction above.  Every shape is warmed first.

  (d) a 10,000-certificate round (committee 100, 67 votes and 32 payload
      entries each, the round of tools/verdict_ab.py) drained from 4 producers:
      V coa_queue_submit_certificate_verdict against C
      coa_queue_submit_certificate followed by one host thread of
      coa_cpu_certificate_verdict_from_status; C without its host checks is the
      crypto round alone, so V over that is what the window's k_window_verdict
      adds end to end (the device-resident figure beside it: +4.2 %,
      profiles/verdict_ab.json);
  (p) with --parent-tree DIR (a built checkout of the parent commit): (b)'s
      crypto requests on that build and on this one, each in processes of its
      own (tools/queue_paced_crypto.py), the two builds alternated.

    python tools/queue_verdict_ab.py [--reps 3] [--sweep-reps 20] [--sweep-only] [--parent-tree DIR] [--out FILE]
                                     [--git-head SHA]

Writes the record as JSON to --out and prints each row.
"""
import argparse
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

from message_verify_ab import HEADER_BYTES, Inputs, _git_head, _stats  # noqa: E402
from queue_message_ab import DRAIN, _expected, _host, _spread  # noqa: E402

PAYLOAD = 8
SWEEP = (1, 64, 128, 512)
SOURCES = ("coa_cert_lat.hip", "coa_lat_job.h", "coa_job_bits.h", "coa_committee.h", "coa_prot_scan.h", "coa_protocol.hip", "coa_protocol.h",
           "coa_queue_hip.cpp", "coa_queue.cpp", "coa_qstage.h")
OK, BAD_ID, UNKNOWN_AUTHOR, MALFORMED, BAD_SIG = 0, 1, 2, 3, 4


def _committee(h, pks, n):
    """Stakes, worker ids and the expected protocol words of the n headers."""
    who = {bytes(k): i for i, k in enumerate(pks)}
    author = np.array([who[bytes(a)] for a in h["authors"]], np.int64)
    stakes = np.ones(len(pks), np.uint32)
    stakes[[3, 57]] = 0
    at = (np.arange(n, dtype=np.int64) * HEADER_BYTES)[:, None] + 40 + 36 * np.arange(PAYLOAD)[None, :] + 32
    ids = h["hdata"][at[..., None] + np.arange(4)].copy().view(np.uint32).reshape(n, PAYLOAD)
    foreign = np.arange(n) % 97 == 5
    keep = np.ones((n, PAYLOAD), bool)
    keep[foreign, PAYLOAD - 1] = False
    workers = [sorted(set(ids[(author == a)][keep[(author == a)]].tolist())) for a in range(len(pks))]
    # a foreign id that some other header of the author names after all is no longer foreign
    named = [set(w) for w in workers]
    foreign &= np.array([int(ids[k, PAYLOAD - 1]) not in named[author[k]] for k in range(n)])
    proto_h = np.where(stakes[author] == 0, UNKNOWN_AUTHOR, np.where(foreign, MALFORMED, OK)).astype(np.uint32)
    proto_v = np.where(stakes[author] == 0, UNKNOWN_AUTHOR, OK).astype(np.uint32)
    return stakes, workers, proto_h, proto_v


def _words(bits_h, bad_v, proto_h, proto_v):
    hw = np.where(bits_h & 1, BAD_ID, np.where(proto_h != 0, proto_h, np.where(bits_h & 2, BAD_SIG, OK)))
    vw = np.where(proto_v != 0, proto_v, np.where(bad_v != 0, BAD_SIG, OK))
    return np.ascontiguousarray(hw.astype(np.uint32)), np.ascontiguousarray(vw.astype(np.uint32))


def _source_sha256():
    """sha256 over the engine sources this measurement is about (ties the
    record to the code it was taken on, committed or not)."""
    h = hashlib.sha256()
    for name in SOURCES:
        with open(os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc", name), "rb") as f:
            h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()


def _sweep(cc, torch, x, stream, hw, vw, n, reps):
    """(a) at n messages: the first n headers, then the first n votes."""
    dev = x.status.device
    words = torch.empty(n, dtype=torch.int32, device=dev)
    raw = torch.empty(n, dtype=torch.int32, device=dev)
    pc = torch.full((n,), PAYLOAD, dtype=torch.int32, device=dev)
    heads = (x.hdata, x.hoff[:n + 1], x.hids[:n], x.authors[:n], x.hsigs[:n])
    votes = (x.vids[:n], x.rounds[:n], x.origins[:n], x.authors[:n], x.vsigs[:n])
    routes = {
        "headers": (lambda: cc.message_lat_verdict_device(0, heads, pc, None, words, stream),
                    lambda: cc.message_lat_verify_device(0, heads, None, raw, stream), hw),
        "votes": (lambda: cc.message_lat_verdict_device(0, None, None, votes, words, stream),
                  lambda: cc.message_lat_verify_device(0, None, votes, raw, stream), vw),
    }
    rows = []
    with torch.cuda.stream(stream):
        for kind, (verdict, crypto, expect) in routes.items():
            for _ in range(3):
                verdict()
                crypto()
            torch.cuda.synchronize()
            exact = bool((words.cpu().numpy().view(np.uint32) == expect[:n]).all())
            tv, tl = [], []
            for _ in range(reps):
                for fn, acc in ((verdict, tv), (crypto, tl)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream)
                    fn()
                    e1.record(stream)
                    e1.synchronize()
                    acc.append(e0.elapsed_time(e1))
            row = {"part": "a", "kind": kind, "n": n, "V": _stats(tv), "L": _stats(tl), "words_exact": exact}
            row["V_over_L_median"] = round(row["V"]["median_ms"] / row["L"]["median_ms"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _paced_crypto(tree, reps):
    """tools/queue_paced_crypto.py on the build in `tree`, a process of its own."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "queue_paced_crypto.py"), "--tree", tree,
                          "--reps", str(reps)], check=True, capture_output=True, text=True, timeout=300).stdout
    return [json.loads(line) for line in out.splitlines() if line.startswith("{")]


def _parent_rows(parent_tree, reps, passes=2):
    """(p): parent, this, parent, this; per (kind, rate) the p50 medians of
    every run of either build."""
    runs = {"parent": [], "this": []}
    for _ in range(passes):
        runs["parent"] += _paced_crypto(parent_tree, reps)
        runs["this"] += _paced_crypto(ROOT, reps)
    rows = []
    for kind in ("headers", "votes"):
        for rate in (100, 1000):
            row = {"part": "p", "kind": kind, "rate_per_s": rate}
            for build, rs in runs.items():
                mine = [r for r in rs if r["kind"] == kind and r["rate_per_s"] == rate]
                row[build + "_C_wait_us_p50"] = [r["wait_us_p50"] for r in mine]
                row[build + "_C_wait_us_p50_median"] = float(np.median([r["wait_us_p50"]["median"] for r in mine]))
            row["this_over_parent_p50"] = round(row["this_C_wait_us_p50_median"] / row["parent_C_wait_us_p50_median"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def _certificate_round(cc, pr, reps, n=10_000):
    """(d)"""
    import certificates as C

    committee, b = C.synth_certificates(n, committee_size=100, n_payload=32, seed=3)
    assert committee.register_authorities() == 100
    c8 = lambda a: np.ascontiguousarray(a, np.uint8)  # noqa: E731
    hdata = np.frombuffer(b"".join(b.header_inputs) + bytes(16), np.uint8)
    hoff = np.zeros(n + 1, np.uint64)
    hoff[1:] = np.cumsum([len(x) for x in b.header_inputs])
    rounds = np.full(n, b.round, np.uint64)
    pcounts = np.full(n, 32, np.uint32)
    voff = np.ascontiguousarray(b.offsets, np.uint64)
    ids, origins, hsigs, vpks, vsigs = (c8(x) for x in (b.ids, b.authors, b.header_sigs, b.vote_pks, b.vote_sigs))
    names = committee.authorities()
    cp, cs, cw, co, cn = cc._committee_arrays(np.array([list(bytes(k)) for k in names], np.uint8),
                                              [committee.stakes[k] for k in names],
                                              [sorted(committee.workers.get(k, {0})) for k in names])
    expect = np.zeros(n, np.uint32)  # the clean round: every word COA_DAG_OK
    vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
    f = pr.latc.latc_queue_verdict_certificates
    f.argtypes = [vp, ctypes.c_int, ctypes.c_int] + [vp] * 10 + [ctypes.c_size_t, vp, vp, vp, vp, vp, ctypes.c_size_t,
                                                               dp, dp]
    f.restype = ctypes.c_int
    p = lambda a: a.ctypes.data  # noqa: E731

    def run(route):
        assert cc.lib().coa_queue_metrics_reset(pr.q) == 0
        el, hc = ctypes.c_double(), ctypes.c_double()
        wrong = f(pr.q, route, 4, p(hdata), p(hoff), p(ids), p(origins), p(hsigs), p(rounds), p(vpks), p(vsigs),
                  p(voff), p(pcounts), n, p(expect), p(cp), p(cs), p(cw), p(co), cn, ctypes.byref(el), ctypes.byref(hc))
        assert wrong == 0, (route, wrong)
        m = cc.QueueMetrics()
        assert cc.lib().coa_queue_metrics(pr.q, ctypes.byref(m)) == 0
        return el.value * 1e3, hc.value * 1e3, cc.metrics_dict(m)

    for route in (0, 1):
        run(route)
    t, host, crypto, windows = {0: [], 1: []}, [], [], {0: [], 1: []}
    for _ in range(reps):
        for route in (0, 1):
            el, hc, m = run(route)
            t[route].append(el)
            windows[route].append(m["windows"])
            if route:
                host.append(hc)
                crypto.append(el - hc)
    row = {"part": "d", "kind": "certificates", "n": n, "votes": int(voff[-1]), "payload_entries": 32, "producers": 4,
           "V_drain_ms": _spread(t[0]), "C_drain_ms": _spread(t[1]), "C_host_checks_ms": _spread(host),
           "C_crypto_only_ms": _spread(crypto), "V_windows": windows[0], "C_windows": windows[1]}
    row["C_over_V_median"] = round(row["C_drain_ms"]["median"] / row["V_drain_ms"]["median"], 3)
    row["V_over_crypto_only_median"] = round(row["V_drain_ms"]["median"] / row["C_crypto_only_ms"]["median"], 3)
    print(json.dumps(row), flush=True)
    return row


class Producer:
    """tools/latc.c latc_queue_verdict_messages over one queue."""

    def __init__(self, cc, pks, stakes, workers):
        self.cc = cc
        self.latc = ctypes.CDLL(os.path.join(ROOT, "xrpl-coa-prototype_amd", "lib", "liblatc.so"))
        vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
        self.latc.latc_queue_verdict_messages.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                                          vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_size_t, vp, vp, vp,
                                                          vp, vp, ctypes.c_size_t, dp, dp]
        self.latc.latc_queue_verdict_messages.restype = ctypes.c_int
        order = sorted(range(len(pks)), key=lambda i: bytes(pks[i]))
        self.keys = np.ascontiguousarray(np.array([pks[i] for i in order], np.uint8))
        self.stakes = np.ascontiguousarray(stakes[order])
        self.woff = np.zeros(len(pks) + 1, np.uint64)
        self.woff[1:] = np.cumsum([len(workers[i]) for i in order])
        self.wids = np.ascontiguousarray(np.array([x for i in order for x in workers[i]], np.uint32))
        self.pcounts = None
        self.q = cc.lib().coa_queue_create(65536, 500)
        assert self.q
        assert cc.lib().coa_queue_set_idle_launch(self.q, 1) == 0

    def run(self, h, expect, route, votes, producers, rate, n):
        """One run over the first n messages; (elapsed s, host check s, queue metrics)."""
        L = self.cc.lib()
        assert L.coa_queue_metrics_reset(self.q) == 0
        el, hc = ctypes.c_double(), ctypes.c_double()
        p = lambda a: a.ctypes.data  # noqa: E731
        ids, sigs = (h["vids"], h["vsigs"]) if votes else (h["hids"], h["hsigs"])
        wrong = self.latc.latc_queue_verdict_messages(
            self.q, route, int(votes), producers, float(rate), p(h["hdata"]), p(h["hoff"]), p(ids), p(h["rounds"]),
            p(h["origins"]), p(h["authors"]), p(sigs), p(self.pcounts), n, p(expect), p(self.keys), p(self.stakes),
            p(self.woff), p(self.wids), len(self.keys), ctypes.byref(el), ctypes.byref(hc))
        assert wrong == 0, (route, votes, n, wrong)
        m = self.cc.QueueMetrics()
        assert L.coa_queue_metrics(self.q, ctypes.byref(m)) == 0
        return el.value, hc.value, self.cc.metrics_dict(m)

    def close(self):
        self.cc.lib().coa_queue_destroy(self.q)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep-reps", type=int, default=20)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit: part (p)")
    ap.add_argument("--n", type=int, default=DRAIN)
    ap.add_argument("--sweep-only", action="store_true", help="part (a) alone (an A/B of two libraries: COA_VERIFY_LIB)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "queue_verdict_ab.json"))
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    args = ap.parse_args()
    # (p) first: its processes come and go before this one opens the device
    parent_rows = _parent_rows(os.path.abspath(args.parent_tree), args.reps) if args.parent_tree else []
    import torch

    import coa_crypto as cc
    import workloads

    cc.init(1)
    seeds = workloads.key_seeds(100)
    pks = cc.public_keys(seeds)
    assert cc.committee_register(pks) == 100
    rng = np.random.default_rng(12)
    stream = torch.cuda.Stream(torch.device("cuda", 0))
    x = Inputs(cc, torch, args.n, seeds, pks, rng)
    bits_h, bad_v = _expected(cc, torch, x, stream)
    h = _host(x, torch)
    stakes, workers, proto_h, proto_v = _committee(h, pks, args.n)
    assert cc.committee_register_authorities(pks, stakes.tolist(), workers) == 100
    hw, vw = _words(bits_h, bad_v, proto_h, proto_v)
    record = {"tool": "tools/queue_verdict_ab.py", "git_head": args.git_head or _git_head(),
              "source_sha256": _source_sha256(), "sources": list(SOURCES),
              "device": torch.cuda.get_device_name(0), "committee": 100, "header_bytes": HEADER_BYTES,
              "payload_entries": PAYLOAD, "n": args.n,
              "V": "coa_queue_submit_header_verdict / coa_queue_submit_vote_verdict",
              "C": "coa_queue_submit_header / coa_queue_submit_vote, then one host thread of protocol checks",
              "header_words": {str(k): int((hw == k).sum()) for k in range(5)},
              "vote_words": {str(k): int((vw == k).sum()) for k in range(5)},
              "V_device": "k_msg_verdict_lat (coa_msg_lat_verdict_device)",
              "L_device": "k_msg_verify_lat (coa_msg_lat_verify_device)",
              "not_measured": [] if args.parent_tree else ["parent build"],
              "results": parent_rows}
    for n in SWEEP:
        record["results"] += _sweep(cc, torch, x, stream, hw, vw, min(n, args.n), args.sweep_reps)
    if args.sweep_only:
        cc.committee_register(np.zeros((0, 32), np.uint8))
        with open(args.out, "w") as f:
            json.dump(record, f, indent=1)
            f.write("\n")
        return
    pr = Producer(cc, pks, stakes, workers)
    pr.pcounts = np.full(args.n, PAYLOAD, np.uint32)
    try:
        for votes, expect in ((False, hw), (True, vw)):
            kind = "votes" if votes else "headers"
            for rate in (100, 1000):  # (b) paced, one producer, ~1.5 s of arrivals per run
                n = min(int(rate * 1.5), args.n)
                for route in (0, 1):
                    pr.run(h, expect, route, votes, 1, rate * 10, n)
                acc = {r: {"p50": [], "p99": [], "windows": [], "verdict_windows": []} for r in (0, 1)}
                for _ in range(args.reps):
                    for route in (0, 1):
                        _, _, m = pr.run(h, expect, route, votes, 1, rate, n)
                        acc[route]["p50"].append(m["wait_us_p50"])
                        acc[route]["p99"].append(m["wait_us_p99"])
                        acc[route]["windows"].append(m["windows"])
                row = {"part": "b", "kind": kind, "rate_per_s": rate, "requests": n,
                       "V_wait_us_p50": _spread(acc[0]["p50"]), "V_wait_us_p99": _spread(acc[0]["p99"]),
                       "C_wait_us_p50": _spread(acc[1]["p50"]), "C_wait_us_p99": _spread(acc[1]["p99"]),
                       "V_windows": acc[0]["windows"], "C_windows": acc[1]["windows"]}
                row["V_over_C_p50_median"] = round(row["V_wait_us_p50"]["median"] / row["C_wait_us_p50"]["median"], 3)
                record["results"].append(row)
                print(json.dumps(row), flush=True)
            for route in (0, 1):  # (c) drain
                pr.run(h, expect, route, votes, 4, 0, args.n)
            t, host = {0: [], 1: []}, []
            for _ in range(max(args.reps, 7)):  # the drains are short: more repeats than the paced runs
                for route in (0, 1):
                    el, hc, _ = pr.run(h, expect, route, votes, 4, 0, args.n)
                    t[route].append(el * 1e3)
                    if route:
                        host.append(hc * 1e3)
            row = {"part": "c", "kind": kind, "n": args.n, "producers": 4, "V_drain_ms": _spread(t[0]),
                   "C_drain_ms": _spread(t[1]), "C_host_checks_ms": _spread(host)}
            row["C_over_V_median"] = round(row["C_drain_ms"]["median"] / row["V_drain_ms"]["median"], 3)
            record["results"].append(row)
            print(json.dumps(row), flush=True)
        record["results"].append(_certificate_round(cc, pr, max(args.reps, 5)))
        vs = [ctypes.c_uint64() for _ in range(4)]
        assert cc.lib().coa_queue_verdict_stats(pr.q, *[ctypes.byref(v) for v in vs]) == 0
    finally:
        pr.close()
        cc.committee_register(np.zeros((0, 32), np.uint8))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

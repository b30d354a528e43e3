"""A/B: raw PrimaryMessage frames to verdict words, the route that existed
(host decoder, then the host-pointer verdict call) against the fused calls over
the device-resident wire decoder.

Workload: the 10,000-certificate C3 round of bench.py (committee 100, 67
votes, 32 payload entries, 67 parents) serialised once with tests/wire_codec.py,
outside the clock; 65,536 Header frames (the round's headers, cycled) and
65,536 Vote frames (the round's votes as Vote messages: Vote::digest is
Certificate::digest).

  a  coa_wire_scan + coa_wire_decode_* + coa_*_verdict_many on host pointers
  b  coa_wire_*_verdict_many

Both sides alternate in ONE process after a warm-up, timed by the host's clock
around the calls (each returns with its answer on the host); the words of a and
b are compared.  Side a's scan and decode are also timed on their own: the host
decoder's cost per frame on this machine's CPU.

Also: the device time of the decode alone (events around
coa_wire_decode_certificates_device, frames already in HBM, caller workspace),
of the scan pass alone, and of coa_certificate_verdict_many_device on the
decoded arrays, alternating in the same process; and the bytes the decode reads
and writes per frame against that time.

    python tools/wire_device_ab.py [--reps 7] [--out FILE] [--git-head SHA]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HEADER, VOTE, CERTIFICATE = 0, 1, 2


def _git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "reps": len(ms)}


class Frames:
    def __init__(self, frames):
        self.n = len(frames)
        self.data = np.frombuffer(b"".join(frames), np.uint8)
        self.offs = np.zeros(self.n + 1, np.uint64)
        self.offs[1:] = np.cumsum([len(f) for f in frames])
        self.bytes = int(self.offs[-1])


def host_route(L, kind, fr):
    """Side a over preallocated arrays: (run(), words, timings dict filled by run)."""
    n = fr.n
    kinds = np.zeros(n, np.int32)
    hb, nv = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    assert L.coa_wire_scan(fr.data.ctypes.data, fr.offs.ctypes.data, n, kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                           hb.ctypes.data, nv.ctypes.data) == 0
    assert (kinds == kind).all()
    hd = np.zeros(int(hb.sum()) + 16, np.uint8)
    hoff, voff = np.zeros(n + 1, np.uint64), np.zeros(n + 1, np.uint64)
    ids, a32, b32 = (np.zeros((n, 32), np.uint8) for _ in range(3))
    sigs, rounds, pc = np.zeros((n, 64), np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    tv = max(int(nv.sum()), 1)
    vp, vs = np.zeros((tv, 32), np.uint8), np.zeros((tv, 64), np.uint8)
    words = np.zeros(n, np.uint32)
    t = {"scan": [], "decode": [], "verdict": []}
    P = lambda a: a.ctypes.data  # noqa: E731
    pc_p = pc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))

    def run():
        t0 = time.perf_counter()
        rc = L.coa_wire_scan(P(fr.data), P(fr.offs), n, kinds.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), P(hb), P(nv))
        t1 = time.perf_counter()
        if kind == CERTIFICATE:
            rc |= L.coa_wire_decode_certificates(P(fr.data), P(fr.offs), n, P(hd), P(hoff), P(ids), P(a32), P(sigs), P(rounds),
                                                 P(vp), P(vs), P(voff), pc_p)
            t2 = time.perf_counter()
            rc |= L.coa_certificate_verdict_many(P(hd), P(hoff), P(ids), P(a32), P(sigs), P(rounds), P(vp), P(vs), P(voff), n,
                                                 5, P(pc), P(words))
        elif kind == HEADER:
            rc |= L.coa_wire_decode_headers(P(fr.data), P(fr.offs), n, P(hd), P(hoff), P(ids), P(a32), P(sigs), P(rounds), pc_p)
            t2 = time.perf_counter()
            rc |= L.coa_header_verdict_many(P(hd), P(hoff), P(ids), P(a32), P(sigs), n, P(pc), P(words))
        else:
            rc |= L.coa_wire_decode_votes(P(fr.data), P(fr.offs), n, P(ids), P(rounds), P(b32), P(a32), P(sigs))
            t2 = time.perf_counter()
            rc |= L.coa_vote_verdict_many(P(ids), P(rounds), P(b32), P(a32), P(sigs), n, P(words))
        t3 = time.perf_counter()
        assert rc == 0, rc
        t["scan"].append((t1 - t0) * 1e3)
        t["decode"].append((t2 - t1) * 1e3)
        t["verdict"].append((t3 - t2) * 1e3)

    return run, words, t, dict(hb=hb, nv=nv)


def fused_route(L, kind, fr):
    kinds, words = np.zeros(fr.n, np.int32), np.zeros(fr.n, np.uint32)
    P = lambda a: a.ctypes.data  # noqa: E731

    def run():
        if kind == CERTIFICATE:
            rc = L.coa_wire_certificate_verdict_many(P(fr.data), P(fr.offs), fr.n, 5, P(kinds), P(words))
        elif kind == HEADER:
            rc = L.coa_wire_header_verdict_many(P(fr.data), P(fr.offs), fr.n, P(kinds), P(words))
        else:
            rc = L.coa_wire_vote_verdict_many(P(fr.data), P(fr.offs), fr.n, P(kinds), P(words))
        assert rc == 0, rc

    return run, words, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--certs", type=int, default=10_000)
    ap.add_argument("--messages", type=int, default=65_536)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_device_ab.json"))
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    args = ap.parse_args()
    import torch

    import certificates as C
    import coa_crypto as cc
    import wire_codec as W

    cc.init(1)
    L = cc.lib()
    n = args.certs
    committee, b = C.synth_certificates(n, committee_size=100, n_payload=32, seed=3)
    assert committee.register_authorities() == 100
    offs = np.asarray(b.offsets, np.int64)
    t0 = time.perf_counter()
    headers, cert_frames, vote_frames = [], [], []
    for i in range(n):
        h = b.header_inputs[i]
        pay = [(h[40 + 36 * k:72 + 36 * k], int.from_bytes(h[72 + 36 * k:76 + 36 * k], "little")) for k in range(32)]
        par = [h[1192 + 32 * k:1224 + 32 * k] for k in range((len(h) - 1192) // 32)]
        author, id_ = bytes(b.authors[i]), bytes(b.ids[i])
        hb = W.header(author, b.round, pay, par, id_, bytes(b.header_sigs[i]))
        headers.append(W.primary_message(0, hb))
        votes = [(bytes(b.vote_pks[j]), bytes(b.vote_sigs[j])) for j in range(offs[i], offs[i + 1])]
        cert_frames.append(W.primary_message(2, W.certificate(hb, votes)))
        if len(vote_frames) < args.messages:
            vote_frames += [W.primary_message(1, W.vote(id_, b.round, author, pk, sg)) for pk, sg in votes]
    sets = {"certificates": (CERTIFICATE, Frames(cert_frames)),
            "headers": (HEADER, Frames([headers[i % n] for i in range(args.messages)])),
            "votes": (VOTE, Frames(vote_frames[:args.messages]))}
    print(f"serialised in {time.perf_counter() - t0:.1f} s", flush=True)
    record = {"tool": "tools/wire_device_ab.py", "git_head": args.git_head or _git_head(),
              "device": torch.cuda.get_device_name(0), "committee": 100, "votes_per_certificate": 67,
              "payload_entries": 32, "parents": 67,
              "timing": "host clock around the calls (each returns with the words on the host); device_*: device "
                        "events around the enqueued calls, frames and arrays resident in HBM",
              "rows": {}}
    scans = {}
    for name, (kind, fr) in sets.items():
        run_a, words_a, t_a, scans[name] = host_route(L, kind, fr)
        run_b, words_b, kinds_b = fused_route(L, kind, fr)
        run_b()
        run_a()  # warm-up, and the answers compared once
        run_b()
        assert (kinds_b == kind).all() and (words_a == words_b).all(), name
        for k in t_a:
            t_a[k].clear()
        wall = {"a": [], "b": []}
        for _ in range(args.reps):
            for arm, fn in (("a", run_a), ("b", run_b)):
                t1 = time.perf_counter()
                fn()
                wall[arm].append((time.perf_counter() - t1) * 1e3)
        row = {"frames": fr.n, "frame_bytes_total": fr.bytes, "frame_bytes_each": round(fr.bytes / fr.n, 1),
               "words_ok": int((words_b == 0).sum()), "a_host_decode_then_verdict": _stats(wall["a"]),
               "b_fused": _stats(wall["b"]), "a_scan": _stats(t_a["scan"]), "a_decode": _stats(t_a["decode"]),
               "a_verdict": _stats(t_a["verdict"])}
        row["a_over_b_median"] = round(row["a_host_decode_then_verdict"]["median_ms"] / row["b_fused"]["median_ms"], 2)
        row["host_scan_us_per_frame"] = round(row["a_scan"]["median_ms"] * 1e3 / fr.n, 3)
        row["host_decode_us_per_frame"] = round(row["a_decode"]["median_ms"] * 1e3 / fr.n, 3)
        row["b_frames_per_s"] = round(fr.n / (row["b_fused"]["median_ms"] * 1e-3))
        record["rows"][name] = row
        print(json.dumps({name: row}), flush=True)

    # ---- device time of the decode alone, beside the verdict call's, on the certificate round
    kind, fr = sets["certificates"]
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    d_frames = torch.from_numpy(np.concatenate([fr.data, np.zeros(4096, np.uint8)])).to(dev)
    d_offs = torch.from_numpy(fr.offs.view(np.int64)).to(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731
    nvb = cc.wire_votes_bound(fr.bytes)
    o = dict(hdata=E((fr.bytes + 16,), torch.uint8), hoff=E((n + 1,), torch.int64), ids=E((n, 32), torch.uint8),
             origins=E((n, 32), torch.uint8), hsigs=E((n, 64), torch.uint8), rounds=E((n,), torch.int64),
             vpks=E((nvb, 32), torch.uint8), vsigs=E((nvb, 64), torch.uint8), voff=E((n + 1,), torch.int64),
             pcounts=E((n,), torch.int32), kinds=E((n,), torch.int32), totals=E((4,), torch.int64))
    ws_w = E((max(cc.wire_workspace_bytes(n, fr.bytes), 16),), torch.uint8)
    d_hb, d_nv = E((n,), torch.int64), E((n,), torch.int64)

    def decode():
        cc.wire_decode_certificates_device(0, d_frames, d_offs, *o.values(), frame_bytes=fr.bytes, stream=stream,
                                           workspace=ws_w)

    def scan_only():
        cc.wire_scan_device(0, d_frames, d_offs, o["kinds"], d_hb, d_nv, frame_bytes=fr.bytes, stream=stream,
                            workspace=ws_w)

    with torch.cuda.stream(stream):
        decode()
        stream.synchronize()
        totals = o["totals"].cpu().numpy()
        nvotes = int(totals[1])
        scan = scans["certificates"]
        assert totals.tolist() == [int(scan["hb"].sum()), int(scan["nv"].sum()), n, 0]
        ws_v = E((cc.certificate_verdict_workspace_bytes(n, nvotes),), torch.uint8)
        words = E((n,), torch.int32)

        def verdict():
            cc.certificate_verdict_many_device(0, o["hdata"], o["hoff"], o["ids"], o["origins"], o["hsigs"], o["rounds"],
                                               o["vpks"][:nvotes], o["vsigs"][:nvotes], o["voff"], o["pcounts"], words,
                                               stream, ws_v)

        verdict()
        stream.synchronize()
        assert not words.cpu().numpy().any()
        ev = {"decode": [], "scan_pass": [], "verdict": []}
        arms = (("decode", decode), ("scan_pass", scan_only), ("verdict", verdict))
        for _ in range(args.device_reps):
            for arm, fn in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                fn()
                e1.record(stream)
                stream.synchronize()
                ev[arm].append(e0.elapsed_time(e1))
    dev_row = {"device_decode_three_passes": _stats(ev["decode"]), "device_scan_pass_alone": _stats(ev["scan_pass"]),
               "device_certificate_verdict_many_device": _stats(ev["verdict"])}
    # bytes of the decode per frame: both per-frame passes read the frame; the decode writes the arrays
    read = 2 * fr.bytes + 2 * (n + 1) * 8 + n * (4 + 8 + 8) * 2
    written = int(totals[0]) + n * (32 + 32 + 64 + 8 + 4 + 4 + 8 + 8) + nvotes * 96 + 2 * (n + 1) * 8
    ms = dev_row["device_decode_three_passes"]["median_ms"]
    dev_row.update(bytes_read_per_frame=round(read / n), bytes_written_per_frame=round(written / n),
                   decode_gb_per_s=round((read + written) / (ms * 1e-3) / 1e9, 1),
                   decode_us_per_frame=round(ms * 1e3 / n, 4),
                   decode_over_verdict_median=round(ms / dev_row["device_certificate_verdict_many_device"]["median_ms"], 3))
    record["rows"]["certificates_device_time"] = dev_row
    print(json.dumps({"certificates_device_time": dev_row}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

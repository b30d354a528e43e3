"""A/B: a receive buffer of interleaved PrimaryMessage frames to one verdict
word per frame.

  a  coa_wire_verdict_many: one upload, the partition by kind and the decode on
     the device, the three verdict calls over the compacted arrays, the scatter
  b  the route that existed: one host pass over each frame's first four bytes
     and a gather into three contiguous batches (tools/wire_gather.c, one
     core), then coa_wire_header_verdict_many, coa_wire_vote_verdict_many and
     coa_wire_certificate_verdict_many, and the merge of their words

Shapes (frames serialised once with tests/wire_codec.py, outside the clock):

  round    one committee-100 round as a primary sees it: 99 headers, 99 votes
           and 99 certificates (67 votes, 32 payload entries, 67 parents),
           interleaved
  backlog  10,000 of each kind, interleaved, 1 % of the frames cut short

Both sides alternate in ONE process after a warm-up, timed by the host's clock
around the calls (each returns with its words on the host); the words of a and
b are compared.  Side b's stages are timed on their own.  Also the device time
(events, frames resident in HBM, caller workspaces) of the mixed decode
against the three single-kind decodes, over their gathered batches (what
route b runs) and index-aligned over the whole batch (placeholders).

    python tools/wire_mixed_ab.py [--sets 7] [--out FILE] [--git-head SHA]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

HEADER, VOTE, CERTIFICATE = 0, 1, 2
NAMES = {HEADER: "headers", VOTE: "votes", CERTIFICATE: "certificates"}


def _git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True,
                              check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        return None


def _stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "sets": len(ms)}


def _gather_lib(tmp):
    so = os.path.join(tmp, "libwire_gather.so")
    subprocess.run(["gcc", "-O2", "-std=c11", "-shared", "-fPIC", os.path.join(ROOT, "tools", "wire_gather.c"), "-o", so],
                   check=True)
    lib = ctypes.CDLL(so)
    lib.wire_gather.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t] + [ctypes.c_void_p] * 4
    lib.wire_gather.restype = None
    return lib


class Frames:
    def __init__(self, frames):
        self.n = len(frames)
        self.data = np.frombuffer(b"".join(frames) + b"\0", np.uint8)
        self.offs = np.zeros(self.n + 1, np.uint64)
        self.offs[1:] = np.cumsum([len(f) for f in frames])
        self.bytes = int(self.offs[-1])


P = lambda a: a.ctypes.data  # noqa: E731


def route_a(L, fr, seed):
    kinds, words = np.zeros(fr.n, np.int32), np.zeros(fr.n, np.uint32)

    def run():
        assert L.coa_wire_verdict_many(P(fr.data), P(fr.offs), fr.n, seed, P(kinds), P(words)) == 0

    return run, kinds, words


def route_b(L, G, fr, seed):
    """The existing route over preallocated buffers: run(), its words, its
    per-stage times, and the gathered batches of its last run."""
    n = fr.n
    out = [np.zeros(fr.bytes + 1, np.uint8) for _ in range(3)]
    out_offs = [np.zeros(n + 1, np.uint64) for _ in range(3)]
    index = [np.zeros(n, np.uint32) for _ in range(3)]
    count = (ctypes.c_size_t * 3)()
    ptrs = [(ctypes.c_void_p * 3)(*[P(a) for a in arrs]) for arrs in (out, out_offs, index)]
    kinds = [np.zeros(n, np.int32) for _ in range(3)]
    sub = [np.zeros(n, np.uint32) for _ in range(3)]
    words = np.zeros(n, np.uint32)
    t = {"gather": [], "headers": [], "votes": [], "certificates": [], "merge": []}

    def run():
        t0 = time.perf_counter()
        G.wire_gather(P(fr.data), P(fr.offs), n, ptrs[0], ptrs[1], ptrs[2], count)
        t1 = time.perf_counter()
        t["gather"].append((t1 - t0) * 1e3)
        for k in (HEADER, VOTE, CERTIFICATE):
            if k == CERTIFICATE:
                rc = L.coa_wire_certificate_verdict_many(P(out[k]), P(out_offs[k]), count[k], seed, P(kinds[k]), P(sub[k]))
            elif k == HEADER:
                rc = L.coa_wire_header_verdict_many(P(out[k]), P(out_offs[k]), count[k], P(kinds[k]), P(sub[k]))
            else:
                rc = L.coa_wire_vote_verdict_many(P(out[k]), P(out_offs[k]), count[k], P(kinds[k]), P(sub[k]))
            assert rc == 0, rc
            t2 = time.perf_counter()
            t[NAMES[k]].append((t2 - t1) * 1e3)
            t1 = t2
        words[:] = 255
        for k in range(3):
            words[index[k][:count[k]]] = sub[k][:count[k]]
        t["merge"].append((time.perf_counter() - t1) * 1e3)

    def batches():
        return [(out[k], out_offs[k], int(count[k])) for k in range(3)]

    return run, words, t, batches


def device_times(cc, fr, gathered, reps):
    """Device time of the mixed decode, of the three single-kind decodes over
    their gathered batches and of the three index-aligned passes over the
    whole batch; events on one stream, alternating."""
    import torch

    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)  # noqa: E731

    def resident(data, offs, n, nbytes):
        d = torch.from_numpy(np.concatenate([data[:nbytes], np.zeros(4096, np.uint8)])).to(dev)
        return d, torch.from_numpy(offs[:n + 1].view(np.int64).copy()).to(dev)

    def arrays(kind, n, nbytes):
        nvb = max(cc.wire_votes_bound(nbytes), 1)
        a = dict(hdata=E((nbytes + 16,), torch.uint8), hoff=E((n + 1,), torch.int64), ids=E((n, 32), torch.uint8),
                 authors=E((n, 32), torch.uint8), origins=E((n, 32), torch.uint8), sigs=E((n, 64), torch.uint8),
                 hsigs=E((n, 64), torch.uint8), pcounts=E((n,), torch.int32), rounds=E((n,), torch.int64),
                 vpks=E((nvb, 32), torch.uint8), vsigs=E((nvb, 64), torch.uint8), voff=E((n + 1,), torch.int64))
        return {name: a[name] for name in cc.WIRE_MIXED_SET_NAMES[kind]}

    def single(kind, d_frames, d_offs, n, nbytes):
        s = arrays(kind, n, nbytes)
        kinds, totals = E((n,), torch.int32), E((4,), torch.int64)
        ws = E((max(cc.wire_workspace_bytes(n, nbytes), 16),), torch.uint8)
        call = {HEADER: cc.wire_decode_headers_device, VOTE: cc.wire_decode_votes_device,
                CERTIFICATE: cc.wire_decode_certificates_device}[kind]
        return lambda: call(0, d_frames, d_offs, *s.values(), kinds, totals, frame_bytes=nbytes, stream=stream, workspace=ws)

    n, nbytes = fr.n, fr.bytes
    d_frames, d_offs = resident(fr.data, fr.offs, n, nbytes)
    sets = {k: arrays(k, n, nbytes) for k in (HEADER, VOTE, CERTIFICATE)}
    kinds, slots, totals = E((n,), torch.int32), E((n,), torch.int32), E((8,), torch.int64)
    ws = E((cc.wire_mixed_workspace_bytes(n, nbytes),), torch.uint8)

    def mixed():
        cc.wire_decode_mixed_device(0, d_frames, d_offs, sets[HEADER], sets[VOTE], sets[CERTIFICATE], kinds, slots, totals,
                                    frame_bytes=nbytes, stream=stream, workspace=ws)

    per_kind = []
    for k, (data, offs, count) in enumerate(gathered):
        if count:
            nb = int(offs[count])
            per_kind.append(single(k, *resident(data, offs, count, nb), count, nb))
    aligned = [single(k, d_frames, d_offs, n, nbytes) for k in (HEADER, VOTE, CERTIFICATE)]
    arms = (("mixed_decode", [mixed]), ("three_single_kind_decodes_gathered", per_kind),
            ("three_index_aligned_passes", aligned))
    ev = {name: [] for name, _ in arms}
    with torch.cuda.stream(stream):
        for _, fns in arms:
            for fn in fns:
                fn()
        stream.synchronize()
        for _ in range(reps):
            for name, fns in arms:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                for fn in fns:
                    fn()
                e1.record(stream)
                stream.synchronize()
                ev[name].append(e0.elapsed_time(e1))
    row = {name: _stats(v) for name, v in ev.items()}
    row["totals"] = totals.cpu().numpy().tolist()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backlog", type=int, default=10_000, help="frames of each kind in the backlog shape")
    ap.add_argument("--sets", type=int, default=7)
    ap.add_argument("--device-reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_mixed_ab.json"))
    ap.add_argument("--git-head", default=None, help="recorded as is (for a tree run without its .git)")
    args = ap.parse_args()
    assert args.sets >= 7
    import torch

    import certificates as C
    import coa_crypto as cc
    import wire_codec as W

    cc.init(1)
    L = cc.lib()
    tmp = tempfile.mkdtemp(prefix="wire_mixed_ab_")
    G = _gather_lib(tmp)
    n = args.backlog
    committee, b = C.synth_certificates(n, committee_size=100, n_payload=32, seed=3)
    assert committee.register_authorities() == 100
    offs = np.asarray(b.offsets, np.int64)
    t0 = time.perf_counter()
    trios = []
    for i in range(n):
        h = b.header_inputs[i]
        pay = [(h[40 + 36 * k:72 + 36 * k], int.from_bytes(h[72 + 36 * k:76 + 36 * k], "little")) for k in range(32)]
        par = [h[1192 + 32 * k:1224 + 32 * k] for k in range((len(h) - 1192) // 32)]
        author, id_ = bytes(b.authors[i]), bytes(b.ids[i])
        hb = W.header(author, b.round, pay, par, id_, bytes(b.header_sigs[i]))
        votes = [(bytes(b.vote_pks[j]), bytes(b.vote_sigs[j])) for j in range(offs[i], offs[i + 1])]
        pk, sg = votes[i % len(votes)]
        trios.append((W.primary_message(0, hb), W.primary_message(1, W.vote(id_, b.round, author, pk, sg)),
                      W.primary_message(2, W.certificate(hb, votes))))
    round_frames = [f for trio in trios[:99] for f in trio]
    backlog = [f for trio in trios for f in trio]
    cut = list(range(50, len(backlog), 100))  # 1 % undecodable: cut short inside a field
    for i in cut:
        backlog[i] = backlog[i][:len(backlog[i]) * 2 // 3]
    print(f"serialised in {time.perf_counter() - t0:.1f} s", flush=True)
    record = {"tool": "tools/wire_mixed_ab.py", "git_head": args.git_head or _git_head(),
              "device": torch.cuda.get_device_name(0), "committee": 100, "votes_per_certificate": 67,
              "payload_entries": 32, "parents": 67,
              "timing": "host clock around the calls (each returns with the words on the host), sides alternating in one "
                        "process, median (min-max) over the sets; device_time: device events around the enqueued "
                        "decodes, frames resident in HBM, caller workspaces",
              "a": "coa_wire_verdict_many",
              "b": "host pass over the first four bytes + gather into three batches (one core), then the three "
                   "single-kind fused calls, then the merge",
              "shapes": {}}
    seed = 5
    for name, frames in (("round", round_frames), ("backlog", backlog)):
        fr = Frames(frames)
        run_a, kinds_a, words_a = route_a(L, fr, seed)
        run_b, words_b, t_b, batches = route_b(L, G, fr, seed)
        for _ in range(2):  # warm-up: the staging and device buffers grow once
            run_a()
            run_b()
        assert (words_a == words_b).all(), name
        for v in t_b.values():
            v.clear()
        wall = {"a": [], "b": []}
        for _ in range(args.sets):
            for arm, fn in (("a", run_a), ("b", run_b)):
                t1 = time.perf_counter()
                fn()
                wall[arm].append((time.perf_counter() - t1) * 1e3)
        sizes = {NAMES[k]: sorted({len(f) for f in frames if f[:4] == bytes([k, 0, 0, 0])})[-1] for k in (HEADER, VOTE, CERTIFICATE)}
        row = {"frames": fr.n, "frame_bytes_total": fr.bytes, "frame_bytes_each": sizes,
               "undecodable_frames": int((kinds_a < 0).sum()), "words_ok": int((words_a == 0).sum()),
               "words_no_message": int((words_a == 255).sum()),
               "a_mixed": _stats(wall["a"]), "b_gather_then_three_calls": _stats(wall["b"]),
               "b_stages": {k: _stats(v) for k, v in t_b.items()}}
        row["b_over_a_median"] = round(row["b_gather_then_three_calls"]["median_ms"] / row["a_mixed"]["median_ms"], 3)
        row["a_frames_per_s"] = round(fr.n / (row["a_mixed"]["median_ms"] * 1e-3))
        row["device_time"] = device_times(cc, fr, batches(), args.device_reps)
        d = row["device_time"]
        row["device_gathered_over_mixed_median"] = round(
            d["three_single_kind_decodes_gathered"]["median_ms"] / d["mixed_decode"]["median_ms"], 3)
        record["shapes"][name] = row
        print(json.dumps({name: row}), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

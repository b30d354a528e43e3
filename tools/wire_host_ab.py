"""A/B of two versions of the host wire decoder (csrc/coa_wire.cpp) on the
host, no GPU involved: coa_wire_scan and coa_wire_decode_* per frame on the
three frame shapes of tools/wire_device_ab.py (the C3 certificate of 11,252
bytes, its header of 3,472 and a vote of 212; unsigned -- nothing here
verifies), and both calls on one oversized header frame (300,000 payload
entries over 100,000 keys, 5,000 parents over 1,500: about 11 MB).

Both versions are compiled here with the flags build.py gives a .cpp file, each
into a library of its own; every measurement runs in a fresh child process
that loads one of them; parent and new alternate, `--pairs` of them.  Each
child also hashes every output array: the two versions must give the same
bytes.

    python tools/wire_host_ab.py --parent-src DIR/coa_wire.cpp --parent-head SHA --new-head SHA
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(ROOT, "tests"))
SHAPES = ("certificates", "headers", "votes", "oversized")


def compile_lib(src, out):
    cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-shared", src, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(f"compiling {src} failed:\n{r.stderr[-4000:]}")
    return out


def make_frames(n):
    import numpy as np

    import wire_codec as W

    rng = np.random.default_rng(3)
    B = lambda k: rng.integers(0, 256, k, dtype=np.uint8).tobytes()  # noqa: E731
    sets = {k: [] for k in SHAPES}
    for _ in range(n):  # sets in key order on the wire, as the reference's serialiser emits them
        pay = sorted((B(32), int(w)) for w in rng.integers(0, 4, 32))
        hb = W.header(B(32), 5, pay, sorted(B(32) for _ in range(67)), B(32), B(64))
        votes = [(B(32), B(64)) for _ in range(67)]
        sets["headers"].append(W.primary_message(0, hb))
        sets["certificates"].append(W.primary_message(2, W.certificate(hb, votes)))
        sets["votes"].append(W.primary_message(1, W.vote(B(32), 5, B(32), B(32), B(64))))
    keys = rng.integers(0, 256, (101_500, 32), dtype=np.uint8)
    pay = np.zeros((300_000, 36), np.uint8)
    pay[:, :32] = keys[rng.integers(0, 100_000, 300_000)]
    pay[:, 32:] = np.arange(300_000, dtype="<u4").view(np.uint8).reshape(-1, 4)
    par = keys[100_000 + rng.integers(0, 1_500, 5_000)]
    big = W.key(B(32)) + (77).to_bytes(8, "little") + (300_000).to_bytes(8, "little") + pay.tobytes() + \
        (5_000).to_bytes(8, "little") + par.tobytes() + B(96)
    sets["oversized"].append(W.primary_message(0, big))
    return sets


def child(args):
    import numpy as np

    L = ctypes.CDLL(args.lib)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    out = {"lib": args.lib}
    for name, frames in make_frames(args.frames).items():
        n = ctypes.c_size_t(len(frames))
        data = np.frombuffer(b"".join(frames), np.uint8)
        offs = np.zeros(len(frames) + 1, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in frames])
        kinds, hb, nv = np.zeros(len(frames), np.int32), np.zeros(len(frames), np.uint64), np.zeros(len(frames), np.uint64)
        scan = lambda: L.coa_wire_scan(P(data), P(offs), n, P(kinds), P(hb), P(nv))  # noqa: E731
        assert scan() == 0 and (kinds == {"certificates": 2, "votes": 1}.get(name, 0)).all(), (name, kinds[:4])
        hd, vp, vs = np.zeros(int(hb.sum()), np.uint8), np.zeros(int(nv.sum()) * 32, np.uint8), np.zeros(int(nv.sum()) * 64, np.uint8)
        hoff, voff = np.zeros(len(frames) + 1, np.uint64), np.zeros(len(frames) + 1, np.uint64)
        ids, a32, b32 = (np.zeros(len(frames) * 32, np.uint8) for _ in range(3))
        sigs, rounds, pc = np.zeros(len(frames) * 64, np.uint8), np.zeros(len(frames), np.uint64), np.zeros(len(frames), np.uint32)
        if name == "certificates":
            decode = lambda: L.coa_wire_decode_certificates(P(data), P(offs), n, P(hd), P(hoff), P(ids), P(a32), P(sigs),  # noqa: E731
                                                            P(rounds), P(vp), P(vs), P(voff), P(pc))
        elif name == "votes":
            decode = lambda: L.coa_wire_decode_votes(P(data), P(offs), n, P(ids), P(rounds), P(b32), P(a32), P(sigs))  # noqa: E731
        else:
            decode = lambda: L.coa_wire_decode_headers(P(data), P(offs), n, P(hd), P(hoff), P(ids), P(a32), P(sigs),  # noqa: E731
                                                       P(rounds), P(pc))
        ts, td = [], []
        for k in range(args.reps + 1):  # the first pair warms up
            t0 = time.perf_counter()
            ra = scan()
            t1 = time.perf_counter()
            rb = decode()
            t2 = time.perf_counter()
            assert ra == 0 and rb == 0, (name, ra, rb)
            if k:
                ts.append((t1 - t0) * 1e6 / len(frames))
                td.append((t2 - t1) * 1e6 / len(frames))
        h = hashlib.sha256()
        for a in (kinds, hb, nv, hd, hoff, ids, a32, b32, sigs, rounds, pc, vp, vs, voff):
            h.update(a.tobytes())
        out[name] = {"frames": len(frames), "frame_bytes": len(frames[0]), "scan_us_per_frame": round(statistics.median(ts), 3),
                     "decode_us_per_frame": round(statistics.median(td), 3), "outputs_sha256": h.hexdigest()}
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--lib")
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--parent-src")
    ap.add_argument("--parent-head")
    ap.add_argument("--new-head")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_host_grammar_ab.json"))
    args = ap.parse_args()
    if args.child:
        return child(args)
    srcs = {"parent": args.parent_src, "new": os.path.join(CSRC, "coa_wire.cpp")}
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as td:
        libs = {w: compile_lib(srcs[w], os.path.join(td, f"libcoa_wire_{w}.so")) for w in srcs}
        for k in range(args.pairs):
            for which in ("parent", "new"):
                cmd = [sys.executable, os.path.abspath(__file__), "--child", "--lib", libs[which], "--frames",
                       str(args.frames), "--reps", str(args.reps)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                line = [x for x in r.stdout.splitlines() if x.startswith("CHILD ")]
                if r.returncode != 0 or not line:
                    sys.exit(f"{which} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
                runs[which].append(json.loads(line[-1][6:]))
                print(k, which, line[-1][6:], flush=True)

    def series(which, shape, field):
        xs = [r[shape][field] for r in runs[which]]
        return {"runs": xs, "median": round(statistics.median(xs), 3), "min": min(xs), "max": max(xs)}

    record = {"tool": "tools/wire_host_ab.py", "parent_head": args.parent_head, "new_head": args.new_head,
              "coa_wire_cpp_lines": {w: sum(1 for _ in open(srcs[w])) for w in srcs}, "pairs": args.pairs,
              "reps_per_run": args.reps, "host_cpus": os.cpu_count(), "unit": "microseconds per frame, one thread",
              "condition": "the new runs' median is not above the parent runs' maximum", "shapes": {}}
    for shape in SHAPES:
        first = runs["new"][0][shape]
        row = {"frames": first["frames"], "frame_bytes": first["frame_bytes"],
               "outputs_equal": len({r[shape]["outputs_sha256"] for w in runs for r in runs[w]}) == 1}
        for field in ("scan_us_per_frame", "decode_us_per_frame"):
            pa, nw = series("parent", shape, field), series("new", shape, field)
            row[field] = {"parent": pa, "new": nw, "new_over_parent_median": round(nw["median"] / pa["median"], 4),
                          "new_median_not_above_parent_max": bool(nw["median"] <= pa["max"])}
            print(shape, field, "parent", pa["median"], [pa["min"], pa["max"]], "new", nw["median"], "ok",
                  row[field]["new_median_not_above_parent_max"])
        record["shapes"][shape] = row
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    ok = all(r["outputs_equal"] and r[f]["new_median_not_above_parent_max"] for r in record["shapes"].values()
             for f in ("scan_us_per_frame", "decode_us_per_frame"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()

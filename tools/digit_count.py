"""Static instruction counts of the C2 verify kernels from hipcc's -S output.

Per Horner digit of k_verify_main<1, true> (the hot path only: the rare carry
blocks assembled into `.subsection 1` are left out): the outermost loop of the
kernel is the digit loop, the loop nested in it the three-pass doubling loop,
so one digit issues  body(outer) - body(inner) + 3 * body(inner)  instructions
(the body includes the conversion that every digit but the last ends with).
k_verify_main_sums and k_verify_main_sums29 have one digit loop per role (the outermost loops with a
barrier in them): the consumer's is the one with the doubling loop nested in
it, the producer's the one without.
Also prints the straight-line hot-path count of both k_pre_halve<3, *>
instances and the register, spill, scratch and LDS figures of every kernel in
the file's metadata.

--json FILE writes, per kernel symbol, those figures, the hot-path instruction
count and a SHA-256 of the hot-path instruction text (labels, comments and
directives stripped, block labels renumbered per function), so two builds are
compared by diffing two small files.

For both k_pre_halve<3, *> instances it also lists the hot-path loops with
their body counts (the squaring runs of the (p-5)/8 chains are the loops
without memory instructions).  -D NAME=VALUE is passed to the compiler
(-D COA_PRE_POW29=0: the radix-2^32 decompression; -D COA_SUMS_FE29=0: no
k_verify_main_sums29).

usage: python tools/digit_count.py [--json FILE] [-D NAME=VALUE ...] [coa_halved.s]
       (without a .s argument the file is compiled here with build.py's flags)"""
import argparse
import collections
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))

MAIN = "_Z13k_verify_mainILi1ELb1EEv"
SUMS = "_Z18k_verify_main_sumsILi0ELb0EEv"
SUMS29 = "_Z20k_verify_main_sums29ILi0ELb0EEv"  # the limb-form accumulator (COA_SUMS_FE29)
PRE = "_Z11k_pre_halveILi3E"
WATCH = ("v_mad_u64_u32", "v_addc_co_u32", "v_mov_b32", "v_cndmask_b32", "s_nop")
KEYS = ["all"] + list(WATCH)
META = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def compile_s(src, extra=()):
    import build as B

    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [B.HIPCC] + B.COMMON + list(extra) + ["--cuda-device-only", "-S", os.path.join(B.CSRC, src), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        raise SystemExit(r.stderr[-4000:])
    return out


def function_lines(text, prefix):
    """The hot-path lines ((label | None, mnemonic | None) per line) of the
    function whose symbol starts with prefix."""
    out, on, sub = [], False, 0
    for line in text.splitlines():
        if not on:
            if line.startswith(prefix) and ":" in line:
                on = True
            continue
        s = line.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            break
        if not s:
            continue
        m = re.match(r"\.subsection\s+(\d+)", s)
        if m:
            sub = int(m.group(1))
            continue
        if sub:
            continue
        if s.endswith(":"):
            out.append((s[:-1], None, None))
        elif not s.startswith("."):
            parts = s.split()
            out.append((None, parts[0], s))
    return out


def loops(lines):
    """(start, end) line-index ranges of backward branches, outermost first."""
    label_at = {lab: i for i, (lab, _, _) in enumerate(lines) if lab}
    found = []
    for i, (_, op, s) in enumerate(lines):
        if op and op.startswith(("s_cbranch", "s_branch")):
            tgt = s.split()[-1]
            if tgt in label_at and label_at[tgt] < i:
                found.append((label_at[tgt], i))
    return sorted(found, key=lambda r: r[0] - r[1])


def tally(lines, lo, hi):
    c = collections.Counter()
    for _, op, _ in lines[lo:hi + 1]:
        if op:
            c["all"] += 1
            for w in WATCH:
                if op.startswith(w):
                    c[w] += 1
    return c


def inner_of(ls, outer):
    """The longest loop strictly inside outer (not outer's other back edges), or None."""
    inner = [r for r in ls if outer[0] < r[0] and r[1] <= outer[1]]
    return max(inner, key=lambda r: r[1] - r[0]) if inner else None


def digit(text):
    lines = function_lines(text, MAIN)
    ls = loops(lines)
    outer = ls[0]
    inner = inner_of(ls[1:], outer)
    o, i = tally(lines, *outer), tally(lines, *inner)
    return {k: o[k] + 2 * i[k] for k in KEYS}, {k: i[k] for k in KEYS}


def sums_digit(text, prefix=SUMS):
    """(consumer per digit, its doubling pass, producer per digit) of k_verify_main_sums / _sums29."""
    lines = function_lines(text, prefix)
    ls = loops(lines)
    top = [r for r in ls if not any(o != r and o[0] <= r[0] and r[1] <= o[1] for o in ls)]
    # a role's digit loop ends each iteration with the barrier; the consumer's
    # row prologue (coa_sums_tail.h) has loops too, and no barrier
    top = [r for r in top if any(op == "s_barrier" for _, op, _ in lines[r[0]:r[1] + 1])]
    cons = [r for r in top if inner_of(ls, r)]
    prod = [r for r in top if not inner_of(ls, r)]
    if len(cons) != 1 or len(prod) != 1:
        return None
    inner = inner_of(ls, cons[0])
    o, i, p = tally(lines, *cons[0]), tally(lines, *inner), tally(lines, *prod[0])
    return {k: o[k] + 2 * i[k] for k in KEYS}, {k: i[k] for k in KEYS}, {k: p[k] for k in KEYS}


def metadata(text):
    """{kernel symbol: {figure: value}} from the amdhsa.kernels metadata (keys in alphabetical order)."""
    out, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "name" and val.startswith("_Z"):
            cur["name"] = val
        elif key in META:
            cur[key] = int(val)
        if key == "vgpr_spill_count":
            if "name" in cur:
                out[cur.pop("name")] = cur
            cur = {}
    return out


def digest(lines):
    """(instruction count, SHA-256) of a function's hot-path instruction text."""
    h, n = hashlib.sha256(), 0
    for _, op, s in lines:
        if op:
            h.update((re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())) + "\n").encode())
            n += 1
    return n, h.hexdigest()


def fmt(c):
    return " ".join(f"{k}={c[k]}" for k in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", metavar="FILE")
    ap.add_argument("-D", dest="defines", action="append", default=[], metavar="NAME=VALUE")
    ap.add_argument("asm", nargs="?")
    a = ap.parse_args()
    text = open(a.asm or compile_s("coa_halved.hip", ["-D" + d for d in a.defines])).read()
    meta = metadata(text)
    report = {}
    for name, m in meta.items():
        n, h = digest(function_lines(text, name + ":"))
        report[name] = dict(m, hot_instructions=n, hot_sha256=h)
    main_k = next((k for k in meta if k.startswith(MAIN)), None)
    sums_k = next((k for k in meta if k.startswith(SUMS)), None)
    if main_k:
        d, inner = digit(text)
        print("k_verify_main<1,true> per digit:", fmt(d))
        print("  one doubling pass:", fmt(inner))
        report[main_k].update(per_digit=d, doubling_pass=inner)
    sd = sums_digit(text) if sums_k else None
    if sd:
        print("k_verify_main_sums<0,false> consumer per digit:", fmt(sd[0]))
        print("  one doubling pass:", fmt(sd[1]))
        print("k_verify_main_sums<0,false> producer per digit:", fmt(sd[2]))
        report[sums_k].update(consumer_per_digit=sd[0], doubling_pass=sd[1], producer_per_digit=sd[2])
    sums29_k = next((k for k in meta if k.startswith(SUMS29)), None)
    sd = sums_digit(text, SUMS29) if sums29_k else None
    if sd:
        print("k_verify_main_sums29<0,false> consumer per digit:", fmt(sd[0]))
        print("  one doubling pass:", fmt(sd[1]))
        print("k_verify_main_sums29<0,false> producer per digit:", fmt(sd[2]))
        report[sums29_k].update(consumer_per_digit=sd[0], doubling_pass=sd[1], producer_per_digit=sd[2])
    for name in meta:
        if name.startswith(PRE):
            lines = function_lines(text, name + ":")
            print(f"{name[:name.index('Ev') + 2]} hot-path text:", fmt(tally(lines, 0, len(lines) - 1)))
            bodies = [dict({k: tally(lines, lo, hi)[k] for k in KEYS}, memory=sum(1 for _, op, _ in lines[lo:hi + 1] if op and op.startswith(
                ("global_", "scratch_", "buffer_", "flat_", "ds_", "s_load")))) for lo, hi in sorted(loops(lines))]
            arith = [b for b in bodies if not b["memory"] and b["v_mad_u64_u32"] >= 40]
            print("  arithmetic loop bodies (instructions, mads):", [(b["all"], b["v_mad_u64_u32"]) for b in arith])
            report[name].update(arith_loops=arith)
    for name, m in meta.items():
        print(f"  {name[:44]:44s} vgpr {m['vgpr_count']:4d} spill {m['vgpr_spill_count']:3d} sgpr {m['sgpr_count']:3d}"
              f" private {m['private_segment_fixed_size']:4d} lds {m['group_segment_fixed_size']}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()

"""Static instruction counts of the C2 verify kernels from hipcc's -S output.

Per Horner digit of k_verify_main<1, true> (the hot path only: the rare carry
blocks assembled into `.subsection 1` are left out): the outermost loop of the
kernel is the digit loop, the loop nested in it the three-pass doubling loop,
so one digit issues  body(outer) - body(inner) + 3 * body(inner)  instructions
(the body includes the conversion that every digit but the last ends with).
Also prints the straight-line hot-path count of k_pre_halve<3> and the VGPR /
spill figures of every kernel in the file's metadata.

usage: python tools/digit_count.py [coa_halved.s]
       (without an argument the file is compiled here with build.py's flags)"""
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))

MAIN = "_Z13k_verify_mainILi1ELb1EEv"
PRE = "_Z11k_pre_halveILi3EEv"
WATCH = ("v_mad_u64_u32", "v_addc_co_u32", "v_mov_b32", "v_cndmask_b32", "s_nop")


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


def digit(text):
    lines = function_lines(text, MAIN)
    ls = loops(lines)
    outer = ls[0]
    inner = [r for r in ls[1:] if outer[0] < r[0] and r[1] <= outer[1]]  # not the digit loop's other back edge
    inner = max(inner, key=lambda r: r[1] - r[0])
    o, i = tally(lines, *outer), tally(lines, *inner)
    return {k: o[k] + 2 * i[k] for k in ["all"] + list(WATCH)}, i


def metadata(text):
    out, name = [], None
    for line in text.splitlines():
        m = re.match(r"\s+\.name:\s+(_Z\S+)", line)
        if m:
            name = m.group(1)
        m = re.match(r"\s+\.vgpr_count:\s+(\d+)", line)
        if m:
            v = int(m.group(1))
        m = re.match(r"\s+\.vgpr_spill_count:\s+(\d+)", line)
        if m and name:
            out.append((name, v, int(m.group(1))))
            name = None
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else compile_s("coa_halved.hip")
    text = open(path).read()
    if MAIN in text:
        d, inner = digit(text)
        print("k_verify_main<1,true> per digit:", " ".join(f"{k}={v}" for k, v in d.items()))
        print("  one doubling pass:", " ".join(f"{k}={inner[k]}" for k in ["all"] + list(WATCH)))
    if PRE in text:
        lines = function_lines(text, PRE)
        t = tally(lines, 0, len(lines) - 1)
        print("k_pre_halve<3> hot-path text:", " ".join(f"{k}={t[k]}" for k in ["all"] + list(WATCH)))
    for name, v, s in metadata(text):
        print(f"  {name[:60]:60s} vgpr {v:4d} spill {s}")


if __name__ == "__main__":
    main()

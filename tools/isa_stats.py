"""Static ISA statistics of a HIP translation unit for gfx950.

Compiles with -save-temps into a temp dir and reports per kernel: instruction
count, s_nop count, v_mad_u64_u32 / v_mov counts, VGPRs, spilled VGPRs and
private segment bytes.  Used to audit hipcc's hazard pads and register
pressure ("Field arithmetic").

usage: python tools/isa_stats.py SRC.hip [-DNAME=VAL ...]

--compare writes, for every kernel of two source trees side by side, the
figures a refactor must keep: instruction count, VGPRs, SGPRs, spills, private
and group segment, and a SHA-256 of the instruction text (labels, comments
and directives stripped: tools/digit_count.py's digest), compiled with
build.py's flags.

usage: python tools/isa_stats.py --compare PARENT_CSRC OUT.json [--alias NEW=PARENT ...] SRC.hip ...
  SRC.hip: file names under csrc/; every kernel of the two trees' files of
  those names is listed (a kernel that moved between them is matched by name).
  --alias 'k_cert_verify=k_cert_verify<2>': a kernel whose name changed.
"""
import collections
import concurrent.futures
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stats(src, defines=()):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffunction-sections", "-I" + os.path.join(ROOT, "include"),
               "-c", os.path.abspath(src), "-save-temps", "-o", os.path.join(d, "x.o")] + list(defines)
        subprocess.run(cmd, cwd=d, check=True, capture_output=True)
        base = os.path.splitext(os.path.basename(src))[0]
        s = open(os.path.join(d, f"{base}-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
    out = {}
    for name in re.findall(r"^(_Z\w+):", s, re.M):
        i = s.index(name + ":")
        j = s.find(".Lfunc_end", i)
        if j < 0:
            continue
        body = s[i:j].split("\n")
        ins = [l.strip().split()[0] for l in body
               if l.startswith("\t") and l.strip() and not l.startswith("\t.") and not l.startswith("\t;")]
        c = collections.Counter(ins)
        out[name] = dict(instrs=len(ins), s_nop=c["s_nop"], mad=c["v_mad_u64_u32"], mov=c["v_mov_b32_e32"])
    # metadata: one YAML entry per kernel, keys sorted; .name precedes the counts we want
    for ent in re.split(r"\n  - \.agpr_count:", s)[1:]:
        m = re.search(r"\.name:\s+(\S+)", ent)
        if not m or m.group(1) not in out:
            continue
        for key in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
            mm = re.search(r"\." + key + r":\s+(\d+)", ent)
            out[m.group(1)][key] = int(mm.group(1)) if mm else None
    return out


def kernels(csrc, names):
    """{demangled kernel name: figures} over the files `names` of the tree csrc that exist."""
    import digit_count as dc

    out = {}
    names = [n for n in names if os.path.exists(os.path.join(csrc, n))]
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(names)) as ex:
        s_files = list(ex.map(lambda n: dc.compile_s(os.path.join(csrc, n)), names))
    for n, s_file in zip(names, s_files):
        text = open(s_file).read()
        os.unlink(s_file)
        meta = dc.metadata(text)
        plain = subprocess.run(["c++filt"] + list(meta), capture_output=True, text=True, check=True).stdout.split("\n")
        for sym, dem in zip(meta, plain):
            # .Lpost_getpc<N> labels count through the whole file, not the function
            count, sha = dc.digest([(lab, op, s and re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", s))
                                    for lab, op, s in dc.function_lines(text, sym + ":")])
            name = re.sub(r"^void ", "", dem.replace("(anonymous namespace)::", "").split("(")[0])
            out[name] = dict(meta[sym], file=n, symbol=sym, instructions=count, text_sha256=sha)
    return out


def compare(parent_csrc, out_json, names, alias):
    import build as B

    new, old = kernels(B.CSRC, names), kernels(os.path.abspath(parent_csrc), names)
    rows = {}
    for k in sorted(set(new) | (set(old) - set(alias.values()))):
        n, p = new.get(k), old.get(alias.get(k, k))
        rows[k] = dict(parent=p, new=n, same_text=bool(n and p and n["text_sha256"] == p["text_sha256"]))
    for k in sorted(set(alias.values()) - {alias.get(k, k) for k in new}):
        rows[k] = dict(parent=old.get(k), new=None, same_text=False)
    with open(out_json, "w") as f:
        json.dump(dict(flags=B.COMMON[:-1], files=names, kernels=rows), f, indent=1, sort_keys=True)
        f.write("\n")
    for k, r in rows.items():
        fig = lambda e: "-" if not e else (f"{e['instructions']:6d} v{e['vgpr_count']} s{e['sgpr_count']} "
                                           f"spill{e['vgpr_spill_count']} priv{e['private_segment_fixed_size']} "
                                           f"lds{e['group_segment_fixed_size']}")
        print(f"{k:28s} {'same' if r['same_text'] else 'DIFF'}  parent {fig(r['parent'])}  new {fig(r['new'])}")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "xrpl-coa-prototype_amd"))
    if sys.argv[1] == "--compare":
        args = sys.argv[4:]
        alias = dict(a.split("=", 1) for i, a in enumerate(args) if i and args[i - 1] == "--alias")
        files = [a for i, a in enumerate(args) if a != "--alias" and not (i and args[i - 1] == "--alias")]
        compare(sys.argv[2], sys.argv[3], files, alias)
        sys.exit(0)
    for k, v in stats(sys.argv[1], sys.argv[2:]).items():
        print(f"{k[:48]:48s} " + " ".join(f"{a}={b}" for a, b in v.items()))

"""Build the gfx950 engine library in-tree: xrpl-coa-prototype_amd/lib/libcoa_verify.so.

hipcc cross-compiles for gfx950 without a GPU.  Each translation unit is
compiled separately (in parallel) and only when its sources changed, then
linked into one shared library exporting the C ABI of include/coa_verify.h.
"""
import concurrent.futures
import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
OBJDIR = os.path.join(LIBDIR, "obj")
LIB = os.path.join(LIBDIR, "libcoa_verify.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = "gfx950"

SOURCES = ["coa_kernels.hip", "coa_halved.hip", "coa_batch.hip", "coa_committee.hip", "coa_cert_lat.hip", "coa_keybuild.hip", "coa_msm.hip", "coa_latency.hip",
           "coa_protocol.hip", "coa_resolve.hip", "coa_wire_dev.hip", "coa_wire_dev.cpp", "coa_engine.cpp", "coa_sig.cpp", "coa_dag.cpp", "coa_queue.cpp", "coa_queue_hip.cpp",
           "coa_wire.cpp", "coa_wire_cpu.cpp", "coa_cpu.cpp"]
HEADERS = ["coa_fe.h", "coa_sc.h", "coa_ge.h", "coa_sha512.h", "coa_smul.h", "coa_kernels.h", "coa_batch.h", "coa_halved.h",
           "coa_committee.h", "coa_msm.h", "coa_fe_wave.h", "coa_ge_rows.h", "coa_halve.h", "coa_keycache.h",
           "coa_latency.h", "coa_queue.h", "coa_rcmp.h", "coa_lehmer.h", "coa_ge_sums.h", "coa_protocol.h",
           "coa_protocol_dev.h", "coa_prot_scan.h", "coa_stage.h", "coa_qstage.h", "coa_qmetrics.h", "coa_halved_dev.h", "coa_main_pick.h", "coa_engine.h",
           "coa_hostpool.h", "coa_job_bits.h", "coa_cert_scratch.h", "coa_lat_job.h", "coa_env.h", "coa_offsets.h", "coa_sums_tail.h", "coa_fe_pow29.h", "coa_ge_dec29.h", "coa_ge29.h",
           "coa_batch_dev.h", "coa_resolve.h", "coa_resolve_ws.h", "coa_wire_parse.h", "coa_wire_dev.h", "coa_wire_layout.h"]
COMMON = ["-O3", "-fPIC", "-std=c++17", "-ffunction-sections", f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include")]


def _newest(paths):
    return max(os.path.getmtime(p) for p in paths if os.path.exists(p))


def _compile(src):
    path = os.path.join(CSRC, src)
    obj = os.path.join(OBJDIR, src + ".o")
    deps = [path] + [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(ROOT, "include", "coa_verify.h")]
    if os.path.exists(obj) and os.path.getmtime(obj) >= _newest(deps):
        return obj, False
    cmd = [HIPCC] + COMMON + ["-c", path, "-o", obj]
    if src.endswith(".cpp"):
        cmd = [HIPCC, "-O3", "-fPIC", "-std=c++17", f"--offload-arch={ARCH}", "-I" + os.path.join(ROOT, "include"), "-c",
                   path, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr[-6000:]}")
    return obj, True


def build(verbose=False):
    """Compile (incrementally) and link; returns the library path."""
    os.makedirs(OBJDIR, exist_ok=True)
    srcs = [os.path.join(CSRC, f) for f in SOURCES + HEADERS] + [os.path.join(ROOT, "include", "coa_verify.h")]
    if os.path.exists(LIB) and os.path.getmtime(LIB) >= _newest(srcs) and \
            not all(os.path.exists(os.path.join(OBJDIR, s + ".o")) for s in SOURCES):
        # a tree that was copied with its library but without the object files:
        # the library is newer than every source, so it is the build
        results = []
    else:
        with concurrent.futures.ThreadPoolExecutor(max_workers=len(SOURCES)) as ex:
            results = list(ex.map(_compile, SOURCES))
    objs = [o for o, _ in results]
    rebuilt = any(b for _, b in results)
    if results and (rebuilt or not os.path.exists(LIB) or os.path.getmtime(LIB) < _newest(objs)):
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-pthread", "-o", LIB] + objs
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stderr[-6000:]}")
        if verbose:
            print("built", LIB)
    _build_latc()
    _build_arithcheck()
    return LIB


ARITH_HEADERS = ["coa_fe.h", "coa_fe_wave.h", "coa_sc.h", "coa_halve.h", "coa_lehmer.h", "coa_ge.h", "coa_smul.h",
                 "coa_halved.h", "coa_ge_sums.h", "coa_ge_rows.h", "coa_sums_tail.h", "coa_fe_pow29.h", "coa_ge29.h"]
# test-only device libraries around the arithmetic headers: (sources under tests/arith/, library under lib/)
ARITH_LIBS = [(["arith_check.hip", "pow29_check.hip"], "libcoa_arithcheck.so"),
              (["alias_check.hip"], "libcoa_aliascheck.so"), (["sums_check.hip"], "libcoa_sumscheck.so"),
              (["tail_check.hip"], "libcoa_tailcheck.so"), (["ge29_check.hip"], "libcoa_ge29check.so")]
ARITH_SRC = os.path.join(ROOT, "tests", "arith", ARITH_LIBS[0][0][0])
ARITH_LIB = os.path.join(LIBDIR, ARITH_LIBS[0][1])


def _build_arithcheck():
    """lib/libcoa_arithcheck.so, libcoa_aliascheck.so, libcoa_sumscheck.so, libcoa_tailcheck.so and
    libcoa_ge29check.so: the test-only
    kernels of tests/arith/*.hip around the arithmetic headers (no C-ABI
    entry).  Each source is compiled twice with the engine's COMMON flags, as
    is and with -DCOA_RARE_INLINE, so both assembled forms of the rare carry
    blocks of coa_fe.h are in its library (symbols *_out / *_inl)."""
    todo = []
    for src_names, lib_name in ARITH_LIBS:
        srcs = [os.path.join(ROOT, "tests", "arith", n) for n in src_names]
        srcs = [s for s in srcs if os.path.exists(s)]
        lib = os.path.join(LIBDIR, lib_name)
        if not srcs:
            continue
        deps = srcs + [os.path.abspath(__file__)] + [os.path.join(CSRC, h) for h in ARITH_HEADERS]
        if not (os.path.exists(lib) and os.path.getmtime(lib) >= _newest(deps)):
            todo.append((srcs, lib))
    if not todo:
        return

    def one(job):
        src, variant = job
        stem = os.path.splitext(os.path.basename(src))[0]
        obj = os.path.join(OBJDIR, f"{stem}_{variant}.o")
        cmd = [HIPCC] + COMMON + ["-I" + CSRC] + (["-DCOA_RARE_INLINE"] if variant == "inl" else []) + \
              ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {os.path.basename(src)} ({variant}):\n{r.stderr[-6000:]}")
        return obj

    jobs = [(src, v) for srcs, _ in todo for src in srcs for v in ("out", "inl")]
    with concurrent.futures.ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        objs = dict(zip(jobs, ex.map(one, jobs)))
    for srcs, lib in todo:
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", lib] + \
              [objs[(src, v)] for src in srcs for v in ("out", "inl")]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"{os.path.basename(lib)} link failed:\n{r.stderr[-6000:]}")


def _build_latc():
    """lib/liblatc.so: the C-caller latency loop of tools/latc.c (measurement
    only; bench.py loads it), linked against the engine library."""
    src = os.path.join(ROOT, "tools", "latc.c")
    out = os.path.join(LIBDIR, "liblatc.so")
    if not os.path.exists(src):
        return
    if os.path.exists(out) and os.path.getmtime(out) >= _newest([src, LIB, os.path.join(ROOT, "include", "coa_verify.h")]):
        return
    cmd = ["gcc", "-O2", "-std=c11", "-shared", "-fPIC", "-pthread", "-I" + os.path.join(ROOT, "include"), src, "-o", out,
           "-L" + LIBDIR, "-lcoa_verify", "-Wl,-rpath,$ORIGIN"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"liblatc build failed:\n{r.stderr[-3000:]}")


if __name__ == "__main__":
    build(verbose=True)
    sys.exit(0)

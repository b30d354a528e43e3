"""CPU: what the split runtime (csrc/coa_engine.h, namespace coa_rt, hidden
visibility) may and may not leave in the built library's symbol tables.

* Nothing of coa_rt is exported: the dynamic symbols are the C entries.
* No thread-local is read across source files.  An `extern thread_local`
  read from another file goes through a TLS wrapper that calls the variable's
  init function by a weak reference; for a variable without one that
  reference stays undefined, and with hidden visibility the wrapper's null
  check passes in position-independent code and it calls the library's load
  address.  (It did: with two contexts the batch code read the worker flag
  that way and the process died.)  The thread-locals are file-local to
  coa_engine.cpp and reached through functions, so no such reference exists."""
import shutil
import subprocess

import pytest

NM = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"


@pytest.fixture(scope="module")
def libpath():
    import build

    return build.build()


def _nm(*args):
    r = subprocess.run([NM, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return [line.split() for line in r.stdout.splitlines() if line.strip()]


def test_runtime_namespace_is_not_exported(libpath):
    exported = [row[-1] for row in _nm("-D", "--defined-only", libpath)]
    assert any(s == "coa_ed25519_verify_strict" for s in exported)
    assert not [s for s in exported if "coa_rt" in s]  # mangled names carry the namespace


def test_no_undefined_tls_init_reference(libpath):
    # _ZTH<name>: "TLS init function for <name>"; an undefined one is called through a wrapper
    undefined = [row[-1] for row in _nm(libpath) if row[0] in ("U", "w") and row[-1].startswith("_ZTH")]
    assert not undefined, undefined

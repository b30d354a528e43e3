"""CPU: the mixed mode of the wire decoder without a GPU.

* coa_cpu_wire_verdict_many -- the engine's CPU path of coa_wire_verdict_many
  -- on the verdict cases of tests/verdict_cases.py as one interleaved batch:
  the words of the case tables, COA_DAG_NO_MESSAGE and the host scan's kinds
  elsewhere, both seeds, and the reversed batch.
* the premises of tests/test_gpu_wire_mixed.py: what its interleaved pools hold,
  by the host scanner alone.
* the return codes of the new entries before any device work, and the
  workspace size.
* the host-only layout and partition header csrc/coa_wire_layout.h under a
  stand-alone program (tests/sanitize/wire_mixed_driver.cpp) built with
  -fsanitize=address,undefined and run as a child process."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import verdict_cases as vc
import wire_dev_cases as cases
import wire_mixed_cases as mixed
from wire_mixed_cases import CERT_REQUEST, CERTIFICATE, ECAPACITY, EFORMAT, EKEY, ETRUNC, HEADER, VOTE

COA_OK, COA_EINVAL, COA_ENODEVICE = 0, -1, -2
SRC = os.path.join(ROOT, "tests", "sanitize", "wire_mixed_driver.cpp")
INC = os.path.join(ROOT, "xrpl-coa-prototype_amd", "csrc")


@pytest.fixture(scope="module")
def e():
    import build

    build.build()
    import coa_crypto

    coa_crypto.lib()
    return coa_crypto


def _committee():
    pks, stakes, workers = vc.committee().arrays()
    return pks, stakes, workers


def _diff(names, got, want):
    return [(n, hex(int(g)), hex(int(w))) for n, g, w in zip(names, got, want) if g != w]


# ------------------------------------------------- the CPU path on the cases
@pytest.mark.parametrize("seed", [0, 11])
def test_cpu_path_on_the_verdict_cases(e, seed):
    frames, names, kinds, want = mixed.verdict_batch()
    assert {HEADER, VOTE, CERTIFICATE, CERT_REQUEST, None} == set(kinds)
    assert kinds.count(CERTIFICATE) == len(vc.certificate_cases()) and kinds.count(VOTE) == len(vc.vote_cases())
    got_kinds, words = e.cpu_wire_verdict_many(frames, _committee(), rng_seed=seed)
    assert not _diff(names, words, want)
    assert got_kinds.tolist() == e.wire_scan(frames)[0].tolist()
    msg = np.array([k in (HEADER, VOTE, CERTIFICATE) for k in kinds])
    assert (got_kinds[msg] == np.array([k for k in kinds if k in (HEADER, VOTE, CERTIFICATE)])).all()
    assert (words[~msg] == e.DAG_NO_MESSAGE).all() and (words[msg] != e.DAG_NO_MESSAGE).all()
    assert got_kinds[~msg].tolist().count(CERT_REQUEST) == 1 and (np.delete(got_kinds[~msg], -1) < 0).all()
    assert not ((words & 0xff) == e.DAG_VOTES_OPEN).any()
    # the case tables' words all occur: the batch is not a batch of one answer
    assert len(set(words[msg].tolist())) >= 8


def test_cpu_path_reversed_batch_gives_the_reversed_answer(e):
    frames, names, _, want = mixed.verdict_batch()
    kinds, words = e.cpu_wire_verdict_many(frames, _committee(), rng_seed=11)
    rk, rw = e.cpu_wire_verdict_many(frames[::-1], _committee(), rng_seed=11)
    assert rk.tolist() == kinds.tolist()[::-1]
    assert not _diff(names[::-1], rw, want[::-1])
    assert rw.tolist() == words.tolist()[::-1]


def test_cpu_path_answers_frames_over_the_device_cap(e):
    """No entry cap on the host: the two frames of mixed_frames() the device
    reports as COA_WIRE_ECAPACITY come back as their real kind with a real
    word; every other frame gets what the device answers."""
    items = cases.mixed_frames()
    frames = [c["frame"] for c in items]
    kinds, words = e.cpu_wire_verdict_many(frames, _committee())
    dk, _, _ = mixed.device_kinds(e, frames)
    over = np.flatnonzero(dk == ECAPACITY)
    assert len(over) == 2 and set(kinds[over].tolist()) == {HEADER, CERTIFICATE}
    assert (words[over] != e.DAG_NO_MESSAGE).all()
    rest = dk != ECAPACITY
    assert (kinds[rest] == dk[rest]).all()
    assert ((words == e.DAG_NO_MESSAGE) == ~((kinds >= 0) & (kinds <= 2))).all()


def test_cpu_path_arguments(e):
    L = e.lib()
    pks, stakes, workers = _committee()
    cp, cs, cw, co, cn = e._committee_arrays(pks, stakes, workers)
    com = (cp.ctypes.data, cs.ctypes.data, cw.ctypes.data, co.ctypes.data, cn)
    kinds, words = (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 4)()
    offs = (ctypes.c_uint64 * 3)(0, 5, 3)
    buf = (ctypes.c_uint8 * 8)()
    f = L.coa_cpu_wire_verdict_many
    assert f(None, None, 0, 0, None, None, None, None, 0, None, None, 1) == COA_OK
    assert f(buf, None, 2, 0, *com, kinds, words, 1) == COA_EINVAL
    assert f(buf, offs, 2, 0, *com, None, words, 1) == COA_EINVAL
    assert f(buf, offs, 2, 0, *com, kinds, None, 1) == COA_EINVAL
    assert f(buf, offs, 2, 0, *com, kinds, words, 1) == COA_EINVAL  # offsets decrease
    flat = (ctypes.c_uint64 * 3)(0, 0, 0)
    assert f(None, flat, 2, 0, *com, kinds, words, 1) == COA_OK  # two empty frames need no bytes
    assert list(kinds)[:2] == [ETRUNC, ETRUNC] and list(words)[:2] == [e.DAG_NO_MESSAGE] * 2


# ------------------------------------------- premises of the GPU tests' pools
EVERY_KIND = {HEADER, VOTE, CERTIFICATE, CERT_REQUEST}
EVERY_CODE = {ETRUNC, EFORMAT, EKEY, ECAPACITY}


@pytest.mark.parametrize("pool", ["work_split", "differential"])
def test_pools_hold_every_kind_and_every_code(e, pool):
    items = mixed.work_split_items() if pool == "work_split" else mixed.differential_items()
    frames = [c["frame"] for c in items]
    dk, hb, nv = mixed.device_kinds(e, frames)
    assert EVERY_KIND <= set(dk.tolist()) and EVERY_CODE <= set(dk.tolist()), sorted(set(dk.tolist()))
    assert any(cases.over_the_cap(f) for f, k in zip(frames, dk) if k == ECAPACITY)
    assert any(cases.over_the_cap(f) for f, k in zip(frames, dk) if k < 0 and k != ECAPACITY)  # the host's error wins
    if pool == "work_split":
        # staged and flat frames that decode, of both kinds that have a body, beside votes
        lens = np.array([len(f) for f in frames])
        for kind in (HEADER, CERTIFICATE):
            assert ((dk == kind) & (lens <= cases.STAGE)).any() and ((dk == kind) & (lens > cases.STAGE)).any()
        assert (dk[1:2 * len(cases.alignment_frames() + cases.stage_switch_frames()):2] == VOTE).all()
    else:
        assert min((dk == k).sum() for k in (HEADER, VOTE, CERTIFICATE)) >= 100
    assert hb[dk == CERTIFICATE].sum() > 0 and nv[dk == CERTIFICATE].sum() > 0


def test_mixed_frames_pool(e):
    frames = [c["frame"] for c in cases.mixed_frames()]
    dk, _, _ = mixed.device_kinds(e, frames)
    assert len(frames) == 29 and EVERY_KIND | {ETRUNC, ECAPACITY} <= set(dk.tolist())
    assert dk.tolist().count(ECAPACITY) == 2


@pytest.mark.parametrize("n", mixed.SUM_SIZES)
def test_sum_batches_are_arranged_as_the_gpu_test_says(e, n):
    pool = [c["frame"] for c in cases.prefix_pool()]
    pk = e.wire_scan(pool)[0]
    assert [int(pk[i]) for k in (HEADER, VOTE, CERTIFICATE, CERT_REQUEST) for i in mixed.POOL[k]] == \
        [k for k in (HEADER, VOTE, CERTIFICATE, CERT_REQUEST) for _ in mixed.POOL[k]]
    assert (pk[mixed.POOL[None]] < 0).all() and not any(cases.over_the_cap(f) for f in pool)
    lasts = []
    for last in mixed.LASTS:
        idx = mixed.sum_indices(n, last)
        kinds = pk[idx]
        assert len(kinds) == n and EVERY_KIND <= set(kinds.tolist()) and (kinds < 0).any()
        if n > 257:
            assert kinds[255:258].tolist() == [VOTE, HEADER, CERTIFICATE]
        if n == 513:
            assert not (kinds[256:512] == VOTE).any()
        if n >= 65536:
            b = mixed.BLOCK
            assert (kinds[mixed.ALL_CERTIFICATES_BLOCK * b:][:b] == CERTIFICATE).all()
            assert not (kinds[mixed.NO_VOTE_BLOCK * b:][:b] == VOTE).any()
            assert sum(len(pool[i]) for i in idx) < 16 << 20
        lasts.append(int(kinds[-1]))
    assert lasts[:3] == [HEADER, VOTE, CERTIFICATE] and lasts[3] < 0


# ----------------------------------------------------- ABI without a device
def _decode_mixed(L, n, null=None, frames=True, offs=True):
    buf = (ctypes.c_uint8 * 512)()
    base = ctypes.addressof(buf)
    arrays = [base + 8 * i for i in range(25)]  # 22 set arrays, kinds, slots, totals
    if null is not None:
        arrays[null] = None
    return L.coa_wire_decode_mixed_device(0, base + 300 if frames else None, base + 400 if offs else None, n, 64, *arrays,
                                          None, None)


def test_empty_calls_are_ok(e):
    L = e.lib()
    assert _decode_mixed(L, 0) == COA_OK
    assert _decode_mixed(L, 0, null=3) == COA_OK  # n = 0 is decided first, as in the other device forms
    assert L.coa_wire_verdict_many(None, None, 0, 0, None, None) == COA_OK
    k, w = e.wire_verdict_many([])
    assert len(k) == 0 and len(w) == 0


@pytest.mark.parametrize("null", list(range(25)) + ["frames", "offsets"])
def test_null_arrays_are_refused(e, null):
    L = e.lib()
    if null == "frames":
        assert _decode_mixed(L, 3, frames=False) == COA_EINVAL
    elif null == "offsets":
        assert _decode_mixed(L, 3, offs=False) == COA_EINVAL
    else:
        assert _decode_mixed(L, 3, null=null) == COA_EINVAL
    assert b"null" in L.coa_last_error()


def test_sizes_too_large_for_one_call_are_refused(e):
    L = e.lib()
    assert _decode_mixed(L, 1 << 40) == COA_EINVAL


def test_fused_call_arguments(e):
    L = e.lib()
    kinds, words = (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 4)()
    buf = (ctypes.c_uint8 * 8)()
    ok = (ctypes.c_uint64 * 3)(0, 3, 5)
    bad = (ctypes.c_uint64 * 3)(0, 5, 3)
    f = L.coa_wire_verdict_many
    assert f(buf, None, 2, 0, kinds, words) == COA_EINVAL
    assert f(buf, ok, 2, 0, None, words) == COA_EINVAL
    assert f(buf, ok, 2, 0, kinds, None) == COA_EINVAL
    assert f(None, ok, 2, 0, kinds, words) == COA_EINVAL
    assert f(buf, bad, 2, 0, kinds, words) == COA_EINVAL
    assert b"monotone" in L.coa_last_error()


def test_no_gpu_no_answer(e):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present: the calls would run; covered by tests/test_gpu_wire_mixed.py")
    L = e.lib()
    assert _decode_mixed(L, 3) == COA_ENODEVICE
    kinds, words = (ctypes.c_int32 * 4)(), (ctypes.c_uint32 * 4)()
    assert L.coa_wire_verdict_many((ctypes.c_uint8 * 8)(), (ctypes.c_uint64 * 3)(0, 3, 5), 2, 0, kinds, words) == COA_ENODEVICE


def test_workspace_size_is_monotone(e):
    f = e.wire_mixed_workspace_bytes
    ns = (0, 1, 2, 255, 256, 257, 513, 10_000, 65_536, 65_537, 1_000_000)
    sizes = [f(n, 0) for n in ns]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]
    assert all(s % 256 == 0 for s in sizes)
    assert [f(n, 1 << 30) for n in ns] == sizes  # nothing per frame byte is kept between the passes
    # two words per frame and six block totals per 256 frames; the single-kind workspace keeps its size
    assert f(65_536, 0) == 2 * 65_536 * 8 + 256 * 6 * 8
    assert e.wire_workspace_bytes(65_536, 0) == 2 * 65_536 * 8 + 256 * 3 * 8


# ------------------------------------------------------ the stand-alone driver
def test_layout_and_partition_under_sanitizers(tmp_path):
    exe = str(tmp_path / "wire_mixed_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-I", INC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("ok 233 cases")

"""GPU: the argument contract of the engine's C entries -- which call answers
COA_EINVAL with which coa_last_error() text, and which answers COA_OK at
n == 0 -- read off the entries' own checks, one table row per entry.

Every case returns before a kernel launch or a read through a data pointer,
so the pointers are one dummy host buffer and nothing runs on the device.
The CPU-only ordering (COA_ENODEVICE first) is in test_abi.py,
test_cpu_messages.py and tests/c_abi/abi_harness.c.

A row is (entry, signature, checks).  The signature names each parameter with
its kind: i int, z size_t, q uint64, u uint32, p a non-null pointer, p0 a
pointer that is null by default; `=value` overrides the default (2 for sizes,
1 for tags, 0 for the device)."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

OK, EINVAL = 0, -1
NULL_ARG = "null argument"
NO_DEV = "device not opened by coa_init"
TOO_LARGE = "n too large for one call"
NOT_MONO = "offsets not monotone"
NEVER_OPENED = 1 << 20
BIG = 0x80000000  # check_n: n > 0x7fffffff

BUF = (ctypes.c_uint8 * 4096)()  # zeros: as offsets, monotone from 0


def _u64(*v):
    return (ctypes.c_uint64 * len(v))(*v)


OFF_OK = _u64(0, 4, 8)
OFF_DOWN = _u64(0, 8, 4)  # three entries, the middle one lower than its neighbour allows
OFF_FROM4 = _u64(4, 8, 12)
ONES = (ctypes.c_uint32 * 4)(1, 1, 1, 1)


class MsgLatIn(ctypes.Structure):  # csrc/coa_committee.h CoaMsgLatIn
    _fields_ = [("hdr_data", ctypes.c_void_p), ("hdr_off", ctypes.c_void_p), ("hids", ctypes.c_void_p),
                ("hauthors", ctypes.c_void_p), ("hsigs", ctypes.c_void_p), ("nh", ctypes.c_uint64),
                ("vids", ctypes.c_void_p), ("vrounds", ctypes.c_void_p), ("vorigins", ctypes.c_void_p),
                ("vauthors", ctypes.c_void_p), ("vsigs", ctypes.c_void_p), ("nv", ctypes.c_uint64)]


def _lat_in(nh, nv, **null):
    b = ctypes.addressof(BUF)
    v = MsgLatIn(b, b, b, b, b, nh, b, b, b, b, b, nv)
    for k in null:
        setattr(v, k, None)
    return v


CERT_HOST = "hdr_data:p hdr_off:p ids:p origins:p hsigs:p rounds:p vpks:p vsigs:p voff:p n:z seed:q"
CERT_DEV = "dev:i hdr_data:p hdr_off:p ids:p origins:p hsigs:p rounds:p vpks:p vsigs:p voff:p n:z n_votes:z"
CERT_HOST_CHECKS = dict(
    n0=True, nulls="hdr_off ids origins hsigs rounds voff out",
    extra=[(dict(hdr_off=OFF_DOWN), EINVAL, NOT_MONO), (dict(voff=OFF_DOWN), EINVAL, NOT_MONO),
           (dict(voff=OFF_FROM4), EINVAL, "vote_offsets[0] must be 0"),
           (dict(hdr_off=OFF_OK, hdr_data=None), EINVAL, "null header data"),
           (dict(voff=OFF_OK, vpks=None), EINVAL, "null vote arrays"),
           (dict(voff=OFF_OK, vsigs=None), EINVAL, "null vote arrays")])
MSG_HOST_HDR = dict(
    n0=True, extra=[(dict(hdr_off=OFF_DOWN), EINVAL, NOT_MONO),
                    (dict(hdr_off=OFF_OK, hdr_data=None), EINVAL, "null header data")])
BATCH_GROUPS = [(dict(offs=OFF_FROM4), EINVAL, "group_offsets[0] must be 0"),
                (dict(offs=OFF_DOWN), EINVAL, "group_offsets not monotone"),
                (dict(offs=OFF_OK, pks=None), EINVAL, "null pks/sigs"),
                (dict(offs=OFF_OK, sigs=None), EINVAL, "null pks/sigs")]

TABLE = [
    ("coa_init_devices", "ids:p n:i=1", dict(extra=[(dict(ids=None), EINVAL, "empty device list"),
                                                    (dict(n=0), EINVAL, "empty device list")])),
    ("coa_device_ids", "ids:p cap:i=1", dict(extra=[(dict(ids=None), EINVAL, NULL_ARG)])),
    ("coa_self_test", "dev:i bad:p", dict(bad_dev=True, extra=[(dict(bad=None), EINVAL, "null output")])),
    # n == 0 is not answered early here: it still needs an opened device
    ("coa_fe_rows_check_device", "dev:i d_in:p n:z d_out:p stream:p0",
     dict(nulls="d_in d_out", bad_dev=True, extra=[(dict(n=(1 << 24) + 1), EINVAL, "n too large"),
                                                   (dict(n=0, dev=NEVER_OPENED), EINVAL, NO_DEV)])),
    ("coa_ed25519_verify_strict_many", "msgs:p msg_len:z=32 pks:p sigs:p n:z out:p",
     dict(n0=True, nulls="msgs pks sigs out", big="n")),
    ("coa_ed25519_verify_strict", "msg:p pk:p sig:p", dict(nulls="msg pk sig")),
    ("coa_ed25519_verify_strict_many_device", "dev:i msgs:p msg_len:z=32 pks:p sigs:p n:z out:p ws:p0 stream:p0",
     dict(n0=True, nulls="msgs pks sigs out", big="n", bad_dev=True)),
    ("coa_ed25519_challenge_many_device", "dev:i msgs:p msg_len:z=32 pks:p sigs:p n:z k_out:p stream:p0",
     dict(n0=True, nulls="msgs pks sigs k_out", big="n", bad_dev=True)),
    ("coa_ed25519_verify_prehashed_many_device", "dev:i k:p pks:p sigs:p n:z out:p ws:p0 stream:p0",
     dict(n0=True, nulls="k pks sigs out", big="n", bad_dev=True)),
    ("coa_ed25519_verify_batch_groups", "msgs:p pks:p sigs:p offs:p n:z out:p seed:q",
     dict(n0=True, nulls="msgs offs out", extra=BATCH_GROUPS)),
    ("coa_ed25519_verify_batch_groups_z", "msgs:p pks:p sigs:p offs:p n:z zs:p out:p",
     dict(n0=True, nulls="msgs offs out", extra=BATCH_GROUPS + [(dict(offs=OFF_OK, zs=None), EINVAL, "null zs")])),
    ("coa_ed25519_verify_batch", "msg:p pks:p sigs:p n:z seed:q",
     dict(nulls="msg", big="n", extra=[(dict(pks=None), EINVAL, "null pks/sigs"),
                                       (dict(sigs=None), EINVAL, "null pks/sigs")])),
    # no early answer at n == 0 (an empty batch is Ok and is written on the stream)
    ("coa_ed25519_verify_batch_device", "dev:i msg:p pks:p sigs:p n:z=4 zs:p0 seed:q out:p ws:p0 ws_bytes:z=0 stream:p0",
     dict(nulls="msg pks sigs out", big="n", bad_dev=True,
          extra=[(dict(n=0, msg=None), EINVAL, NULL_ARG), (dict(n=0, dev=NEVER_OPENED), EINVAL, NO_DEV),
                 (dict(ws=BUF, ws_bytes="batch_ws_minus_1"), EINVAL,
                  "workspace smaller than coa_verify_batch_workspace_bytes(n)")])),
    # the offsets are walked before check_n: no n > 0x7fffffff case (nor for the header forms)
    ("coa_sha512_many", "data:p offs:p n:z out:p",
     dict(n0=True, nulls="offs out", extra=[(dict(offs=OFF_DOWN), EINVAL, NOT_MONO),
                                            (dict(offs=OFF_OK, data=None), EINVAL, "null data")])),
    ("coa_sha512_trunc32_many", "data:p offs:p n:z out:p",
     dict(n0=True, nulls="offs out", extra=[(dict(offs=OFF_DOWN), EINVAL, NOT_MONO),
                                            (dict(offs=OFF_OK, data=None), EINVAL, "null data")])),
    ("coa_sha512_many_device", "dev:i data:p offs:p n:z out:p stream:p0",
     dict(n0=True, nulls="data offs out", big="n", bad_dev=True)),
    ("coa_ed25519_sign_many", "seeds:p msgs:p msg_len:z=32 n:z pks:p sigs:p",
     dict(n0=True, nulls="seeds msgs pks sigs", big="n")),
    ("coa_ed25519_public_keys", "seeds:p n:z pks:p", dict(n0=True, nulls="seeds pks", big="n")),
    ("coa_ed25519_sign_many_device", "dev:i seeds:p msgs:p msg_len:z=32 n:z pks:p sigs:p stream:p0",
     dict(n0=True, nulls="seeds msgs pks sigs", big="n", bad_dev=True)),
    ("coa_committee_register", "pks:p n:z",
     dict(nulls="pks", extra=[(dict(n=(1 << 20) + 1), EINVAL, "committee too large")])),
    ("coa_committee_register_authorities", "pks:p stakes:p wids:p woff:p n:z",
     dict(nulls="pks stakes woff",
          extra=[(dict(n=1025), EINVAL, "more than COA_MAX_AUTHORITIES authorities"),
                 (dict(woff=OFF_DOWN), EINVAL, "worker offsets not monotone"),
                 (dict(woff=OFF_OK, wids=None), EINVAL, NULL_ARG),
                 (dict(), EINVAL, "duplicate authority key")])),  # two all-zero keys
    ("coa_certificate_verify_many", CERT_HOST + " out:p", CERT_HOST_CHECKS),
    ("coa_certificate_verify", "hdr_data:p hdr_len:z=4 id:p origin:p hsig:p round:q vpks:p vsigs:p n_votes:z seed:q",
     dict(nulls="id origin hsig", extra=[(dict(hdr_data=None), EINVAL, "null header data"),
                                         (dict(vpks=None), EINVAL, "null vote arrays")])),
    ("coa_certificate_resolve_raw", "ids:p origins:p hsigs:p rounds:p vpks:p vsigs:p voff:p n:z raw:p out:p",
     dict(n0=True, nulls="ids origins hsigs rounds voff raw out",
          extra=[(dict(voff=OFF_OK, vpks=None), EINVAL, NULL_ARG), (dict(voff=OFF_OK, vsigs=None), EINVAL, NULL_ARG)])),
    ("coa_certificate_verify_many_device", CERT_DEV + "=0 status:p ws:p0 stream:p0",
     dict(n0=True, nulls="hdr_off ids origins hsigs rounds voff status", big="n", bad_dev=True,
          extra=[(dict(n_votes=3, vpks=None), EINVAL, NULL_ARG), (dict(n_votes=3, vsigs=None), EINVAL, NULL_ARG),
                 (dict(n_votes=BIG - 1), EINVAL, TOO_LARGE)])),
    ("coa_certificate_verify_many_device_order", CERT_DEV + "=0 status:p ws:p0 stream:p0 key_order:i=1",
     dict(n0=True, nulls="hdr_off ids origins hsigs rounds voff status", big="n", bad_dev=True)),
    ("coa_header_verify_many", "hdr_data:p hdr_off:p ids:p authors:p sigs:p n:z out:p",
     dict(nulls="hdr_off ids authors sigs out", **MSG_HOST_HDR)),
    ("coa_vote_verify_many", "ids:p rounds:p origins:p authors:p sigs:p n:z out:p",
     dict(n0=True, nulls="ids rounds origins authors sigs out", big="n")),
    ("coa_message_resolve_raw", "ids:p rounds:p origins:p authors:p sigs:p n:z raw:p",
     dict(n0=True, nulls="ids origins authors sigs raw")),  # origins: null beside rounds
    ("coa_header_verify_many_device", "dev:i hdr_data:p hdr_off:p ids:p authors:p sigs:p n:z status:p ws:p0 stream:p0",
     dict(n0=True, nulls="hdr_data hdr_off ids authors sigs status", big="n", bad_dev=True)),
    ("coa_vote_verify_many_device", "dev:i ids:p rounds:p origins:p authors:p sigs:p n:z status:p ws:p0 stream:p0",
     dict(n0=True, nulls="ids rounds origins authors sigs status", big="n", bad_dev=True)),
    ("coa_certificate_verdict_many", CERT_HOST + " pcounts:p out:p",
     dict(CERT_HOST_CHECKS, nulls=CERT_HOST_CHECKS["nulls"] + " pcounts",
          extra=CERT_HOST_CHECKS["extra"] + [(dict(hdr_off=OFF_OK, pcounts=ONES), EINVAL,
                                              "a payload count overruns its header")])),
    ("coa_header_verdict_many", "hdr_data:p hdr_off:p ids:p authors:p sigs:p n:z pcounts:p out:p",
     dict(n0=True, nulls="hdr_off ids authors sigs pcounts out",
          extra=MSG_HOST_HDR["extra"] + [(dict(hdr_off=OFF_OK, pcounts=ONES), EINVAL,
                                          "a payload count overruns its header")])),
    ("coa_vote_verdict_many", "ids:p rounds:p origins:p authors:p sigs:p n:z out:p",
     dict(n0=True, nulls="ids rounds origins authors sigs out", big="n")),
    ("coa_certificate_verdict_many_device", CERT_DEV + "=0 pcounts:p out:p ws:p0 stream:p0",
     dict(n0=True, nulls="hdr_off ids origins hsigs rounds voff pcounts out", big="n", bad_dev=True,
          extra=[(dict(n_votes=3, vpks=None), EINVAL, NULL_ARG), (dict(n_votes=3, vsigs=None), EINVAL, NULL_ARG)])),
    ("coa_header_verdict_many_device",
     "dev:i hdr_data:p hdr_off:p ids:p authors:p sigs:p n:z pcounts:p out:p ws:p0 stream:p0",
     dict(n0=True, nulls="hdr_data hdr_off ids authors sigs pcounts out", big="n", bad_dev=True)),
    ("coa_vote_verdict_many_device", "dev:i ids:p rounds:p origins:p authors:p sigs:p n:z out:p ws:p0 stream:p0",
     dict(n0=True, nulls="ids rounds origins authors sigs out", big="n", bad_dev=True)),
    # the entries the aggregation queue's backend calls (csrc/coa_latency.h, coa_committee.h)
    ("coa_lat_verify_device", "dev:i d_in:p n:z res:p stream:p0", dict(n0=True, nulls="d_in res", big="n", bad_dev=True)),
    ("coa_lat_verify_inline", "dev:i recs:p n:z res:p tag:u stream:p0",
     dict(n0=True, bad_dev=True, extra=[(dict(recs=None), EINVAL, "null argument or zero tag"),
                                        (dict(res=None), EINVAL, "null argument or zero tag"),
                                        (dict(tag=0), EINVAL, "null argument or zero tag"),
                                        (dict(n=17), EINVAL, "more records than the kernel arguments hold")])),
    ("coa_certificate_verify_publish",
     "dev:i h_base:p d_base:p in_bytes:z=64 pack:p n:z=1 n_votes:z=1 ctr:p res:p tag:u stream:p0",
     dict(n0=True, nulls="h_base d_base pack ctr res", bad_dev=True,
          extra=[(dict(tag=0), EINVAL, NULL_ARG), (dict(n=65), 1, None)])),  # 1: not the latency size, no text
    # the default `in_` is all zeros: no headers, no votes
    ("coa_msg_lat_verify_device", "dev:i in_:p status:p stream:p0",
     dict(extra=[(dict(in_=None), EINVAL, NULL_ARG), (dict(), OK, None), (dict(dev=NEVER_OPENED), OK, None),
                 (dict(in_=_lat_in(2, 2), status=None), EINVAL, NULL_ARG),
                 (dict(in_=_lat_in(2, 2), dev=NEVER_OPENED), EINVAL, NO_DEV),
                 (dict(in_=_lat_in(2, 2, hsigs=None)), EINVAL, NULL_ARG),
                 (dict(in_=_lat_in(2, 2, vrounds=None)), EINVAL, NULL_ARG),
                 (dict(in_=_lat_in(1 << 30, 0)), EINVAL, TOO_LARGE)])),  # 2 nh + nv blocks
    ("coa_msg_lat_verify_publish", "dev:i in_:p ctr:p res:p tag:u stream:p0",
     dict(extra=[(dict(in_=None), EINVAL, "null argument or zero tag"),
                 (dict(ctr=None), EINVAL, "null argument or zero tag"),
                 (dict(res=None), EINVAL, "null argument or zero tag"),
                 (dict(tag=0), EINVAL, "null argument or zero tag"),
                 (dict(in_=_lat_in(40, 25)), EINVAL, "more messages than the result words hold"),
                 (dict(in_=_lat_in(2, 2), dev=NEVER_OPENED), EINVAL, NO_DEV)])),
]

CTYPE = {"i": ctypes.c_int, "z": ctypes.c_size_t, "q": ctypes.c_uint64, "u": ctypes.c_uint32}
DEFAULT = {"i": 0, "z": 2, "q": 0, "u": 1}


def _params(sig):
    out = []
    for word in sig.split():
        name, kind = word.split(":")
        kind, _, dflt = kind.partition("=")
        if kind in ("p", "p0"):
            out.append((name, "p", BUF if kind == "p" else None))
        else:
            out.append((name, kind, int(dflt) if dflt else DEFAULT[kind]))
    return out


def _cases():
    """(id, entry, signature, overrides, rc, text) for every row's checks."""
    for entry, sig, checks in TABLE:
        names = [p[0] for p in _params(sig)]
        rows = []
        if checks.get("n0"):  # answered COA_OK whatever else is passed
            rows.append(("n0", dict(n=0), OK, None))
            if "dev" in names:
                rows.append(("n0-baddev", dict(n=0, dev=NEVER_OPENED), OK, None))
        for name in checks.get("nulls", "").split():
            rows.append(("null-" + name, {name: None}, EINVAL, NULL_ARG))
        if checks.get("big"):
            rows.append(("big-n", {checks["big"]: BIG}, EINVAL, TOO_LARGE))
        if checks.get("bad_dev"):
            rows.append(("baddev", dict(dev=NEVER_OPENED), EINVAL, NO_DEV))
        for k, (over, rc, text) in enumerate(checks.get("extra", [])):
            rows.append((f"x{k}", over, rc, text))
        for tag, over, rc, text in rows:
            assert set(over) <= set(names), (entry, over)
            yield pytest.param(entry, sig, over, rc, text, id=f"{entry}-{tag}")


@pytest.fixture(scope="module")
def lib(engine):
    import build

    L = ctypes.CDLL(build.LIB)  # its own handle: no argtypes set by the Python mirror
    L.coa_last_error.restype = ctypes.c_char_p
    L.coa_verify_batch_workspace_bytes.restype = ctypes.c_size_t
    L.coa_verify_batch_workspace_bytes.argtypes = [ctypes.c_size_t]
    return L


def _last_error(L):
    return L.coa_last_error().decode()


def _prime(L, avoid):
    """Leaves a known other text in coa_last_error(), so the text checked after
    the call is the call's own."""
    if avoid == "null output":
        assert L.coa_init_devices(None, 0) == EINVAL
    else:
        assert L.coa_self_test(0, None) == EINVAL
    assert _last_error(L) != avoid


@pytest.mark.parametrize("entry,sig,over,rc,text", list(_cases()))
def test_argument_contract(lib, entry, sig, over, rc, text):
    args = []
    for name, kind, value in _params(sig):
        value = over.get(name, value)
        if value == "batch_ws_minus_1":
            value = lib.coa_verify_batch_workspace_bytes(4) - 1
        if kind == "p":
            if isinstance(value, ctypes.Structure):
                value = ctypes.pointer(value)
            args.append(ctypes.cast(value, ctypes.c_void_p) if value is not None else ctypes.c_void_p(None))
        else:
            args.append(CTYPE[kind](value))
    fn = getattr(lib, entry)
    fn.restype = ctypes.c_int
    _prime(lib, text)
    got = fn(*args)
    assert got == rc, (got, _last_error(lib))
    if text is not None:
        assert _last_error(lib) == text


def test_device_ids_counts_without_a_buffer(lib):
    """cap == 0 needs no buffer: the call answers the number of contexts."""
    lib.coa_device_count.restype = ctypes.c_int
    assert lib.coa_device_ids(None, 0) == lib.coa_device_count() >= 1

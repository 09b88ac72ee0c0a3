"""The reference Serializer's update bytes without a GPU: the host scanner (fbm_wire_scan), the kernels' per-item
routines run on the host (fbm_test_wire_encode / fbm_test_wire_decode), the placeholder splice of
`wire.dumps_reference` and the message splice of `wire.loads_reference` with the device call replaced by that
host run, and the C ABI's additions (declared, bound, exported by both builds, the ABI still 7, argument errors
before any device call).  Expected bytes and values come from msgpack under the reference's rules
(`fedbiomed/common/serializer.py:96-110`, `:140-149`; tests/wire_reference_util.py), never from the code under
test."""
import ctypes
import os
import random
import re
import shutil
import struct
import subprocess

import msgpack
import numpy as np
import pytest

from fedbiomed_amd import _native as N
from fedbiomed_amd import wire
from tests import wire_reference_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIRE = ["fbm_wire_encode_bound", "fbm_wire_encode_workspace", "fbm_wire_encode", "fbm_wire_scan", "fbm_wire_decode"]
DEPTH = 32  # FBM_WIRE_MAX_DEPTH: containers open at once


@pytest.fixture(scope="module")
def libs():
    from fedbiomed_amd import _build

    _build.build()
    return N.load(), N.load_test()


@pytest.fixture()
def host_run(libs, monkeypatch):
    """`wire`'s two device calls replaced by the library's host run of the same per-item routines."""
    monkeypatch.setattr(wire, "_encode_rows", lambda scheme, rows: U.host_encode(scheme, rows))
    monkeypatch.setattr(wire, "_decode_arrays", U.host_decode)
    wire.reference_stats(reset=True)


def _scan(data, min_items=1):
    from fedbiomed_amd import _device as D

    return D.wire_scan(data, min_items)


def _map_item(value_bytes: bytes) -> bytes:
    head = b"\xc4" + bytes([len(value_bytes)]) if len(value_bytes) <= 255 else b"\xc5" + struct.pack(">H", len(value_bytes))
    return U.PREFIX + head + value_bytes


# ---- encode: the per-item routines -----------------------------------------------------------------
def test_prefix_is_what_msgpack_writes():
    assert U.packb([2**64]) == b"\x91" + U.PREFIX + b"\xc4\x0a\x00\x01" + bytes(8) and len(U.PREFIX) == 20
    assert len(U.packb([2**2048 - 1])) == 1 + 280  # a full-width ciphertext


@pytest.mark.parametrize("n", [0, 1, 15, 16, 41])
def test_host_encode_jl_equals_packb(libs, n):
    vals = U.edge_values()[:n] if n < 41 else U.edge_values()
    assert U.host_encode("jl", U.jl_rows(vals) if vals else np.zeros((0, 64), np.uint32)) == U.packb(vals)


def test_host_encode_lom_equals_packb(libs):
    rng = random.Random(3)
    vals = U.NATIVE_EDGES + [rng.getrandbits(rng.choice([3, 7, 8, 9, 16, 17, 32, 33, 64])) for _ in range(3000)]
    assert U.host_encode("lom", np.array(vals, dtype=np.uint64)) == U.packb(vals)
    assert U.host_encode("lom", np.zeros(0, np.uint64)) == U.packb([])


def test_size_queries(libs):
    lib, _ = libs
    for n in (0, 1, 1000):
        assert lib.fbm_wire_encode_bound(N.WIRE_JL, n) == 5 + 281 * n
        assert lib.fbm_wire_encode_bound(N.WIRE_LOM, n) == 5 + 9 * n
        assert lib.fbm_wire_encode_workspace(N.WIRE_JL, n) >= 8 * (n // 256 + 1) + 2 * n
        assert lib.fbm_wire_encode_workspace(N.WIRE_LOM, n) >= 8 * (n // 1024 + 1)
    assert lib.fbm_wire_encode_bound(2, 5) == 0 and lib.fbm_wire_encode_workspace(-1, 5) == 0


# ---- scanner + decode: accepted inputs -----------------------------------------------------------------
def _roundtrip(data, expect_schemes, min_items=1):
    arrays = _scan(data, min_items)
    assert arrays is not None and [a[3] for a in arrays] == expect_schemes
    rows = U.host_decode(data, arrays)
    for (b, e, n, scheme, ck), r in zip(arrays, rows):
        want = U.unpackb(data[b:e])
        assert n == len(want) and U.rows_to_ints(scheme, r) == want
        assert ck.size == (n if scheme == "jl" else -(-n // N.WIRE_LOM_GROUP))
    return arrays


def test_every_accepted_form_round_trips(libs):
    vals = U.edge_values()
    a = _roundtrip(U.packb(vals), ["jl"])
    assert (a[0][0], a[0][2]) == (0, len(vals)) and a[0][1] == len(U.packb(vals))
    native = [v for v in vals if v < 2**64]
    _roundtrip(U.packb(native * 20), ["lom"])  # 200 items: four groups, the last one partial
    _roundtrip(U.packb([2**64]), ["jl"])  # the first map form (L = 10)
    _roundtrip(U.packb([5] * 70 + [2**100] + [7] * 70), ["jl"])  # the table restarts per item at item 70


def test_non_minimal_forms_are_accepted(libs):
    items = [b"\xcc\x05", b"\xcd\x00\x05", b"\xce\x00\x00\x00\x05", b"\xcf" + bytes(7) + b"\x05", b"\x05",
             b"\xcf\x00\x00\x00\x00\xff\xff\xff\xff"]
    data = bytes([0x90 | len(items)]) + b"".join(items)
    assert U.unpackb(data) == [5, 5, 5, 5, 5, 2**32 - 1]
    _roundtrip(data, ["lom"])
    # map values with extra leading zeros, up to L = 257 (256 bytes hold the value)
    vals = [bytes(3) + b"\x01" + bytes(8), bytes(200) + b"\x7f" * 5, b"\x00" + b"\xff" * 256, bytes(250) + b"\x09", b"\x7f"]
    data = bytes([0x90 | len(vals)]) + b"".join(_map_item(v) for v in vals)
    assert U.unpackb(data) == [int.from_bytes(v, "big") for v in vals]
    _roundtrip(data, ["jl"])


def test_min_items_and_surrounding_fields(libs):
    vals = U.edge_values()
    msg = {"researcher_id": "r", "params": vals, "shape": [3, 4, 5], "nested": {"lom": list(range(300)), "f": 1.5}}
    data = U.packb(msg)
    assert [a[2] for a in _scan(data, 1)] == [len(vals), 3, 300]
    assert [a[2] for a in _scan(data, 4)] == [len(vals), 300]
    assert _scan(data, 301) == []
    _roundtrip(data, ["jl", "lom"], min_items=4)


# ---- scanner: refusals -----------------------------------------------------------------------------
def _refused(items: list, also=b""):
    """An array of these raw items among accepted ones is walked but not recorded; the message still scans."""
    good = [b"\x07", _map_item(b"\x00\x01" + bytes(8))]
    data = b"\x92" + bytes([0x90 | (len(items) + 2)]) + good[0] + b"".join(items) + good[1] + b"\x93\x01\x02\x03" + also
    arrays = _scan(data, 1)
    assert arrays is not None and [(a[2], a[3]) for a in arrays] == [(3, "lom")], data.hex()
    msgpack.unpackb(data, strict_map_key=False)  # (well-formed: msgpack reads it)


def test_scanner_refusals(libs):
    _refused([b"\xff"])  # a negative fixint
    _refused([b"\xd0\x80"])  # int8 -128
    _refused([_map_item(b"\x80" + bytes(9))])  # a sign byte >= 0x80
    _refused([_map_item(b"\xff" * 10)])
    _refused([_map_item(bytes(258))])  # L = 258
    _refused([_map_item(b"\x01" + bytes(256))])  # L = 257 with a nonzero first byte: 2^2048
    _refused([_map_item(b"")])  # L = 0
    _refused([b"\x82\xa5value\xc4\x02\x00\x01\xa8__type__\xa3int"])  # "value" before "__type__"
    _refused([b"\x82\xd9\x08__type__\xa3int\xa5value\xc4\x02\x00\x01"])  # a str8 key
    _refused([U.PREFIX + b"\xc6\x00\x00\x00\x02\x00\x01"])  # bin32
    _refused([b"\xca\x3f\x80\x00\x00"])  # a float among the ints
    _refused([b"\xcb" + struct.pack(">d", 2.0)])
    _refused([b"\xc0"])  # nil


def test_every_truncation_of_a_three_item_message(libs):
    data = U.packb([2**70, 300, 2**2047])
    assert _scan(data, 1) is not None and len(_scan(data, 1)) == 1
    for cut in range(len(data)):
        assert _scan(data[:cut], 1) is None, cut
    assert _scan(data + b"\x00", 1) is None  # trailing bytes: msgpack raises ExtraData


def test_nesting_past_the_bound(libs):
    inner = U.packb(list(range(200, 260)))

    def nested(depth):
        return b"\x91" * depth + inner

    ok = _scan(nested(DEPTH - 2), 1)  # the message and depth - 2 arrays open, then the recorded one
    assert ok is not None and [(a[2], a[3]) for a in ok] == [(60, "lom")]
    assert _scan(nested(DEPTH + 8), 1) is None
    assert _scan(b"\x91" * 100000 + b"\x01", 1) is None  # (no recursion: a deep message costs no stack)


def test_scanner_rejects_reserved_and_is_silent_on_plain_messages(libs):
    assert _scan(b"\xc1", 1) is None
    assert _scan(b"", 1) is None
    assert _scan(U.packb({"a": "b", "c": [1.0, None, True, b"xx", "s" * 40, -5]}), 1) == []


# ---- dumps_reference / loads_reference with the host run in place of the device --------------------------
def _updates():
    vals = U.edge_values()
    jl = wire.EncryptedParams.from_ints("jl", vals)
    lom = wire.EncryptedParams.from_ints("lom", [v for v in vals if v < 2**64] * 9)
    return jl, lom


def test_dumps_reference_splices_each_update(host_run):
    jl, lom = _updates()
    msg = {"a": 1, "params": jl, "mid": b"0123456789abcdef", "more": [lom, "x", 2**90], "z": None}
    plain = {"a": 1, "params": list(jl), "mid": b"0123456789abcdef", "more": [list(lom), "x", 2**90], "z": None}
    assert wire.dumps_reference(msg) == U.packb(plain)
    assert wire.dumps_reference(msg, default=U.ref_default) == U.packb(plain)
    st = wire.reference_stats()
    assert (st["fast"], st["fallback"]) == (4, 0)
    assert wire.dumps_reference({"k": [1, 2]}) == U.packb({"k": [1, 2]})  # nothing to splice


def test_dumps_reference_draws_again_on_a_collision(host_run, monkeypatch):
    jl, _ = _updates()
    clash = bytes(range(16))
    draws = iter([clash, bytes(range(1, 17)), bytes(range(2, 18))])
    monkeypatch.setattr(os, "urandom", lambda k: next(draws))
    msg = {"blob": clash, "params": jl}  # the message itself holds the first placeholder's 18 bytes
    assert wire.dumps_reference(msg) == U.packb({"blob": clash, "params": list(jl)})


def test_inconsistent_update_takes_the_ordinary_route(host_run):
    jl, _ = _updates()
    jl.append(3)
    assert not jl.consistent()
    assert wire.reference_bytes(jl) == U.packb(list(jl))
    assert wire.dumps_reference({"p": jl}) == U.packb({"p": list(jl)})
    st = wire.reference_stats()
    assert st["fast"] == 0 and st["fallback"] == 2
    with pytest.raises(TypeError):
        wire.reference_bytes([1, 2, 3])


def test_loads_reference_equals_unpackb(host_run):
    jl, lom = _updates()
    data = U.packb({"a": 1, "params": list(jl), "t": [1.5, "s"], "more": {"lom": list(lom), 7: [1, 2]}, "z": [2**80]})
    want = U.unpackb(data)
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=4)
    assert got == want
    p, q = got["params"], got["more"]["lom"]
    assert isinstance(p, wire.EncryptedParams) and p.scheme == "jl" and p.consistent()
    assert p.packed.tobytes() == jl.packed.tobytes()
    assert isinstance(q, wire.EncryptedParams) and q.scheme == "lom" and q.packed.tobytes() == lom.packed.tobytes()
    assert type(got["z"]) is list and type(got["more"][7]) is list  # below min_items: msgpack's
    st = wire.reference_stats()
    assert (st["fast"], st["fallback"]) == (2, 0)


def test_loads_reference_fallbacks(host_run):
    jl, lom = _updates()
    # no hook: an array of int maps unpacks to dicts, so only the native array is taken
    data = U.packb({"params": list(jl), "lom": list(lom)})
    got = wire.loads_reference(data, min_items=4)
    assert got == msgpack.unpackb(data, strict_map_key=False)
    assert type(got["params"]) is list and isinstance(got["lom"], wire.EncryptedParams)
    wire.reference_stats(reset=True)
    # refused arrays, a message with nothing to record, and one the scanner gives up on
    neg = U.packb({"params": list(jl)[:20] + [-1]})
    deep = b"\x91" * (DEPTH + 8) + U.packb(list(lom))  # msgpack reads it; the scanner's bound does not
    for data in (neg, U.packb({"a": [1.5] * 30}), deep):
        before = wire.reference_stats()["fallback"]
        assert wire.loads_reference(data, object_hook=U.ref_hook, min_items=4) == U.unpackb(data)
        assert wire.reference_stats()["fallback"] == before + 1
    assert wire.reference_stats()["fast"] == 0
    with pytest.raises(ValueError):  # truncated: exactly msgpack's call and its error
        wire.loads_reference(U.packb(list(lom))[:-1], object_hook=U.ref_hook, min_items=4)


# ---- the C ABI's additions -----------------------------------------------------------------------------
def _header(name="fbm_secagg.h"):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return fh.read()


def test_declared_bound_and_still_abi_7(libs):
    prod, test = libs
    h = _header()
    assert re.search(r"^#define FBM_ABI_VERSION 7\b", h, re.M) and N.ABI_VERSION == 7 and prod.fbm_abi_version() == 7
    for name in WIRE:
        assert re.search(rf"^(int|uint64_t) {name}\(", h, re.M), name
        assert name in N.SIGNATURES and hasattr(prod, name) and hasattr(test, name)
    assert "serializer.py:96-110" in h and "serializer.py:140-149" in h
    c_vp, c_int, c_u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert N.SIGNATURES["fbm_wire_encode"] == (c_int, [c_int, c_vp, c_u64, c_vp, c_u64, c_vp, c_vp, c_vp])
    assert N.SIGNATURES["fbm_wire_decode"] == (c_int, [c_int, c_vp, c_u64, c_u64, c_vp, c_u64, c_u64, c_vp, c_vp])
    assert ctypes.sizeof(N.WireArray) == 48 and (N.WIRE_JL, N.WIRE_LOM, N.WIRE_LOM_GROUP) == (0, 1, 64)
    for m, v in (("FBM_WIRE_JL", 0), ("FBM_WIRE_LOM", 1), ("FBM_WIRE_LOM_GROUP", 64)):
        assert re.search(rf"^#define {m} {v}\b", h, re.M)
    th = _header("fbm_secagg_test.h")
    for name in ("fbm_test_wire_encode", "fbm_test_wire_decode"):
        assert re.search(rf"^int {name}\(", th, re.M) and name in N.TEST_SIGNATURES
        assert hasattr(test, name) and not hasattr(prod, name)


def test_libraries_export_exactly_their_headers(libs):
    from fedbiomed_amd import _build

    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not found")
    hdr, thdr = (os.path.join(ROOT, "include", f) for f in ("fbm_secagg.h", "fbm_secagg_test.h"))
    for path, want in ((N.LIB_PATH, set(_build.declared(hdr))), (N.TEST_LIB_PATH, set(_build.declared(hdr, thdr)))):
        out = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("fbm_")}
        assert exported == want and set(WIRE) <= exported


def test_argument_errors_come_before_any_device_call(libs):
    """(On a machine without a GPU a device call would fail as FBM_E_HIP: FBM_E_ARG shows none was made.)"""
    lib, _ = libs
    buf = ctypes.create_string_buffer(4096)
    one = ctypes.addressof(buf)  # a non-null, 8-byte aligned stand-in: never read before the refusal
    one += (-one) % 8
    cap = lambda sch, n: lib.fbm_wire_encode_bound(sch, n)  # noqa: E731
    E = N.FBM_E_ARG
    assert lib.fbm_wire_encode(2, one, 1, one, 4096, one, one, None) == E and "scheme" in N.last_error()
    assert lib.fbm_wire_encode(N.WIRE_LOM, one, 2**32, one, 2**40, one, one, None) == E
    for rows, out, ws, total in ((None, one, one, one), (one, None, one, one), (one, one, None, one), (one, one, one, None)):
        assert lib.fbm_wire_encode(N.WIRE_JL, rows, 3, out, cap(0, 3), ws, total, None) == E
    assert lib.fbm_wire_encode(N.WIRE_JL, one, 3, one, cap(0, 3) - 1, one, one, None) == E and "out_cap" in N.last_error()
    assert lib.fbm_wire_encode(N.WIRE_LOM, one + 4, 3, one, cap(1, 3), one, one, None) == E
    assert lib.fbm_wire_encode(N.WIRE_LOM, one, 3, one, cap(1, 3), one, one + 4, None) == E
    # decode: a table that is not the scheme's size, null pointers, misaligned tables
    assert lib.fbm_wire_decode(5, one, 10, 0, one, 1, 1, one, None) == E
    assert lib.fbm_wire_decode(N.WIRE_JL, one, 10, 0, one, 2, 3, one, None) == E and "checkpoints" in N.last_error()
    assert lib.fbm_wire_decode(N.WIRE_LOM, one, 10, 0, one, 2, 64, one, None) == E
    assert lib.fbm_wire_decode(N.WIRE_LOM, one, 10, 0, one, 1, 65, one, None) == E
    for span, ck, rows in ((None, one, one), (one, None, one), (one, one, None)):
        assert lib.fbm_wire_decode(N.WIRE_JL, span, 10, 0, ck, 1, 1, rows, None) == E
    assert lib.fbm_wire_decode(N.WIRE_JL, one, 10, 0, one + 4, 1, 1, one, None) == E
    assert lib.fbm_wire_decode(N.WIRE_LOM, None, 0, 0, None, 0, 0, None, None) == N.FBM_OK  # nothing to do
    # scan: null pointers
    na, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    pa, pc = ctypes.addressof(na), ctypes.addressof(nc)
    assert lib.fbm_wire_scan(None, 4, 1, one, 1, pa, one, 1, pc) == E
    assert lib.fbm_wire_scan(one, 4, 1, None, 1, pa, one, 1, pc) == E
    assert lib.fbm_wire_scan(one, 4, 1, one, 1, None, one, 1, pc) == E
    assert lib.fbm_wire_scan(one, 4, 1, one, 1, pa, None, 1, pc) == E
    assert lib.fbm_wire_scan(one, 4, 1, one, 1, pa, one, 1, None) == E


def test_scan_reports_a_small_table(libs):
    lib, _ = libs
    data = np.frombuffer(U.packb(list(range(200))), dtype=np.uint8)
    arrays = (N.WireArray * 1)()
    ck = np.zeros(4, dtype=np.uint64)
    na, nc = ctypes.c_uint64(9), ctypes.c_uint64(9)
    args = lambda a_cap, c_cap: (data.ctypes.data, data.size, 1, ctypes.addressof(arrays), a_cap, ctypes.addressof(na),  # noqa: E731
                                 ck.ctypes.data, c_cap, ctypes.addressof(nc))
    assert lib.fbm_wire_scan(*args(1, 3)) == N.FBM_E_RANGE and (na.value, nc.value) == (0, 0)  # 200 items: 4 groups
    assert lib.fbm_wire_scan(*args(0, 4)) == N.FBM_E_RANGE
    assert lib.fbm_wire_scan(*args(1, 4)) == N.FBM_OK and (na.value, nc.value) == (1, 4)
    assert (arrays[0].begin, arrays[0].end, arrays[0].n_items, arrays[0].scheme) == (0, data.size, 200, N.WIRE_LOM)

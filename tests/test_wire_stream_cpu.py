"""The streamed receive path without a GPU: fbm_test_wire_stream_begin / _feed run the resumable tokenizers' segments
over host buffers through the kernels' per-tile routines, fbm_wire_scan_prefix is plain C++, and wire.StreamAssembler
runs with the library's host run in place of its device side (tests/wire_stream_util.HostStream), as the other CPU
wire tests replace their seams.

Shapes.  The LOM message has 2 500 items over all five native widths: about three 4096-byte tiles and 40 checkpoint
groups.  The JL message has 60 maps with L from {1, 2, 31, 32, 255, 256, 257}: about 10 KB, three tiles.  What a feed
may run changes at a tile's end plus an item's reach (8 bytes; 280 for maps), so every avail_len is a case: the
two-feed cuts take them all."""
import ctypes

import msgpack
import numpy as np
import pytest

from fedbiomed_amd import wire
from tests import wire_reference_util as U
from tests import wire_stream_util as S
from tests import wire_tokenize_jl_util as J
from tests.wire_tokenize_util import header, placed

STEPS = [1, 7, 64, 4096, 4097, 5000]


@pytest.fixture(scope="module")
def lib():
    from fedbiomed_amd import _build, _native

    _build.build()
    return _native.load_test()


@pytest.fixture(scope="module")
def cases(lib):
    """scheme -> (span from the array's header on, base, first, n, the one-shot's [count, end] and table): made once."""
    out = {}
    for scheme, (data, _) in (("lom", S.lom_message()), ("jl", S.jl_message())):
        b, first, e, n, sch, table = S.locate(data)
        assert sch == scheme and (e - first) > 2 * S.TILE
        buf = placed(data[b:], first - b, 1)
        res, ck = S.host_one_shot(lib, scheme, buf, b, first, n)
        assert res == [n, e] and ck == table  # the one-shot host tokenizer gives the scanner's table
        out[scheme] = (buf, b, first, n, res, ck)
    assert len(out["lom"][5]) >= 40
    return out


def test_entry_points_are_declared(lib):
    from fedbiomed_amd import _native as N

    for name in ("fbm_wire_stream_workspace", "fbm_wire_stream_begin", "fbm_wire_stream_feed", "fbm_wire_scan_prefix"):
        assert name in N.SIGNATURES and hasattr(N.load(), name)
    for name in ("fbm_test_wire_stream_begin", "fbm_test_wire_stream_feed"):
        assert name in N.TEST_SIGNATURES and hasattr(lib, name) and not hasattr(N.load(), name)
    assert lib.fbm_abi_version() == 7 and N.WIRE_MORE == 2


@pytest.mark.parametrize("scheme", ["lom", "jl"])
def test_every_two_feed_cut(lib, cases, scheme):
    buf, b, first, n, res, ck = cases[scheme]
    for a in range(first - b, buf.size + 1):
        rcs, got, tab = S.host_feeds(lib, scheme, buf, b, first, n, [a, buf.size])
        assert rcs == [0, 0, 0] and got == res and tab == ck, a


@pytest.mark.parametrize("scheme", ["lom", "jl"])
@pytest.mark.parametrize("step", STEPS)
def test_multi_feed_cuts(lib, cases, scheme, step):
    buf, b, first, n, res, ck = cases[scheme]
    avails = list(range(step, buf.size, step)) + [buf.size]
    rcs, got, tab = S.host_feeds(lib, scheme, buf, b, first, n, avails)
    assert set(rcs) == {0} and got == res and tab == ck


def _refusing():
    """(name, scheme, span, first, n): what the one-shot stops at, in the second tile."""
    from tests.wire_tokenize_util import pool_items

    out = []
    for name, bad in (("negative", b"\xd0\x85"), ("float", b"\xcb" + bytes(8))):
        items = pool_items(1500) + [bad] + pool_items(200)
        out.append((name, "lom", header(len(items)) + b"".join(items), len(header(len(items))), len(items)))
    for name, bad in (("native-among-maps", b"\x05"), ("bin32", J.PREFIX + b"\xc6\x00\x00\x00\x04\x01\x02\x03\x04")):
        items = J.filling(S.TILE + 700) + [bad] + J.filling(600)
        out.append((name, "jl", header(len(items)) + b"".join(items), len(header(len(items))), len(items)))
    items = pool_items(1500) + [b"\xcf" + bytes(7) + b"\x09"]
    out.append(("cut-off-lom", "lom", (header(len(items)) + b"".join(items))[:-3], len(header(len(items))), len(items)))
    items = J.filling(S.TILE + 900)
    out.append(("cut-off-jl", "jl", (header(len(items)) + b"".join(items))[:-7], len(header(len(items))), len(items)))
    return out


@pytest.mark.parametrize("case", _refusing(), ids=[c[0] for c in _refusing()])
def test_refusing_spans_stop_where_the_one_shot_stops(lib, case):
    _, scheme, span, first, n = case
    buf = placed(span, first, 2)
    res, ck = S.host_one_shot(lib, scheme, buf, 0, first, n)
    assert res[0] < n and res[1] == 0
    for avails in ([len(span)], [S.TILE, len(span)], list(range(700, len(span), 700)) + [len(span)],
                   [S.TILE + 8 + 3, S.TILE + 280 + 3, len(span)]):
        rcs, got, _ = S.host_feeds(lib, scheme, buf, 0, first, n, avails)
        assert set(rcs) == {0} and got == res, avails


def test_feed_argument_errors(lib, cases):
    from fedbiomed_amd import _native as N

    buf, b, first, n, res, ck = cases["lom"]
    sch = N.WIRE_LOM
    nck = len(ck)
    tab, state = np.zeros(nck, dtype=np.uint64), np.zeros(S.STATE_WORDS, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_stream_workspace(sch, buf.size)) // 8 + 1, dtype=np.uint64)

    def feed(avail, last, scheme=sch, span=buf.ctypes.data, base=b, n_ck=nck, st=state.ctypes.data):
        return lib.fbm_test_wire_stream_feed(scheme, span, base, avail, last, tab.ctypes.data, n_ck, st, ws.ctypes.data)

    assert feed(5000, 0) == N.FBM_E_ARG  # no stream begun on this state
    assert lib.fbm_test_wire_stream_begin(7, first, n, state.ctypes.data) == N.FBM_E_ARG
    assert lib.fbm_test_wire_stream_begin(sch, first, 0, state.ctypes.data) == N.FBM_E_ARG
    assert lib.fbm_test_wire_stream_begin(sch, first, 2**32, state.ctypes.data) == N.FBM_E_UNSUPPORTED
    assert lib.fbm_test_wire_stream_begin(sch, first, n, None) == N.FBM_E_ARG
    assert lib.fbm_test_wire_stream_begin(sch, first, n, state.ctypes.data) == 0
    assert feed(5000, 0, scheme=N.WIRE_JL, n_ck=n) == N.FBM_E_ARG and feed(5000, 0, n_ck=nck + 1) == N.FBM_E_ARG
    assert feed(5000, 0, span=None) == N.FBM_E_ARG and feed(5000, 0, st=state.ctypes.data + 4) == N.FBM_E_ARG
    assert feed(2**50, 0) == N.FBM_E_UNSUPPORTED
    assert feed(5000, 0) == 0
    assert feed(4999, 0) == N.FBM_E_ARG  # below what was already fed
    assert feed(6000, 0, base=b + 1) == N.FBM_E_ARG and feed(6000, 0, span=buf.ctypes.data + 4) == N.FBM_E_ARG
    assert feed(buf.size, 1) == 0 and state[3:5].tolist() == res and tab.tolist() == ck  # right after every refusal
    assert feed(buf.size, 1) == N.FBM_E_ARG  # behind the last feed
    assert lib.fbm_test_wire_stream_begin(sch, first, n, state.ctypes.data) == 0
    assert feed(first - b, 1) == N.FBM_E_ARG  # the last feed ends in front of item 0
    assert N.load().fbm_wire_stream_feed(sch, buf.ctypes.data, b, 5000, 0, tab.ctypes.data, nck, state.ctypes.data,
                                         ws.ctypes.data, None) == N.FBM_E_ARG  # the device entry: no record, no device call


# ---- fbm_wire_scan_prefix ------------------------------------------------------------------------------------
def _prefix(lib, data, min_items, dl, dj):
    from fedbiomed_amd import _native as N

    buf = np.frombuffer(data, dtype=np.uint8).copy()  # exactly len(data) bytes: a read past them leaves the copy
    pend = N.WirePending2()
    rc = lib.fbm_wire_scan_prefix(buf.ctypes.data if buf.size else None, buf.size, min_items, dl, dj, ctypes.addressof(pend))
    return rc, (pend.begin, pend.first, pend.n_items, pend.scheme)


def _deferred2(lib, data, min_items, dl, dj):
    from fedbiomed_amd import _native as N

    buf = np.frombuffer(data, dtype=np.uint8)
    arrays, ckpt = (N.WireArray * 64)(), np.zeros(len(data) + 16, dtype=np.uint64)
    na, nc, pend = ctypes.c_uint64(0), ctypes.c_uint64(0), N.WirePending2()
    rc = lib.fbm_wire_scan_deferred2(buf.ctypes.data, buf.size, min_items, dl, dj, None, 0, ctypes.addressof(arrays), 64,
                                     ctypes.addressof(na), ckpt.ctypes.data, ckpt.size, ctypes.addressof(nc), ctypes.addressof(pend))
    return rc, (pend.begin, pend.first, pend.n_items, pend.scheme)


def _prefix_messages():
    lom = U.packb(S.lom_values(150, 3))
    jl = header(12) + b"".join(J.item(*J.CLASSES[i % 7], fill=i) for i in range(12))
    small = U.packb([i % 100 for i in range(300)])  # 300 one-byte items behind a 3-byte header
    bad = bytearray(U.packb({"a": "xxxxxx", "b": [1, 2, 3], "params": S.lom_values(150, 3)}))
    bad[10] = 0xC1
    return [("front-lom", b"\x82" + U.packb("params") + lom + U.packb("n") + U.packb(5)),
            ("front-jl", b"\x82" + U.packb("params") + jl + U.packb("n") + U.packb(5)),
            ("behind-small-array", b"\x83" + U.packb("s") + small + U.packb("params") + lom + U.packb("n") + U.packb(5)),
            ("none", U.packb({"a": [1.5] * 40, "b": {"c": "x" * 300, "d": [2**70, 5]}, "e": None})),
            ("malformed-at-10", bytes(bad))]


@pytest.mark.parametrize("case", _prefix_messages(), ids=[c[0] for c in _prefix_messages()])
def test_prefix_scanner_agrees_with_deferred2_on_every_prefix(lib, case):
    from fedbiomed_amd import _native as N

    name, data = case
    for min_items, dl, dj in ((1, 100, 10), (1, 400, 0), (4, 1, 1)):
        want_rc, want = _deferred2(lib, data, min_items, dl, dj)
        answers = []
        for k in range(len(data) + 1):
            rc, got = _prefix(lib, data[:k], min_items, dl, dj)
            if rc == N.WIRE_MORE:
                assert not answers or name == "malformed-at-10", k  # once decided, every longer prefix decides
                continue
            assert rc == want_rc and (rc != N.WIRE_PENDING or got == want), (k, rc, got)
            answers.append(k)
        assert answers and answers[-1] == len(data)  # the whole message is always decided
        if want_rc == N.WIRE_PENDING:  # decided once the header and the bytes that make it a candidate are in
            assert answers[0] == want[1] + (1 if want[3] == N.WIRE_LOM else 21)
        if name == "malformed-at-10":
            assert want_rc == N.FBM_E_UNSUPPORTED and answers[0] == 11
    assert _prefix(lib, b"", 1, 1, 1)[0] == N.WIRE_MORE
    assert lib.fbm_wire_scan_prefix(None, 4, 1, 1, 1, None) == N.FBM_E_ARG


# ---- wire.StreamAssembler on the host run ------------------------------------------------------------------------
@pytest.fixture()
def host_run(lib, monkeypatch):
    monkeypatch.setattr(wire, "_open_stream", S.HostStream)
    monkeypatch.setattr(wire, "_upload_arrays", lambda data, arrays: [S.HostHandle(data, a) for a in arrays])
    monkeypatch.setattr(wire, "_decode_arrays", U.host_decode)
    S.HostStream.opened = S.HostStream.pushed = 0
    wire.reference_stats(reset=True)


FAR = 10**9  # a device_scan threshold no array reaches: the joined reference call walks on the host


def _same(got, want):
    assert type(got) is type(want) and list(got) == list(want)
    for k in want:
        a, b = got[k], want[k]
        if isinstance(b, wire.ResidentUpdate):
            assert type(a) is wire.ResidentUpdate and (a.scheme, a.n_items) == (b.scheme, b.n_items) and a.tolist() == b.tolist()
        else:
            assert a == b and type(a) is type(b)


@pytest.mark.parametrize("scheme", ["lom", "jl"])
def test_assembler_equals_the_joined_call(host_run, scheme):
    data, vals = S.lom_message() if scheme == "lom" else S.jl_message()
    b, first, e, n, _, _ = S.locate(data)
    want = wire.loads_reference(data, object_hook=U.ref_hook, min_items=16, resident=True, device_scan_min_items=FAR,
                                device_scan_jl_min_items=FAR)
    assert type(want["params"]) is wire.ResidentUpdate and want["params"].tolist() == vals
    kw = dict(object_hook=U.ref_hook, min_items=16, device_scan_min_items=32, device_scan_jl_min_items=32)
    asm = wire.StreamAssembler(**kw)  # one assembler, message after message
    sizes = STEPS[2:] + [b + 1, first - 1, first, first + 1, first + 10, first + 20, first + 21, len(data) - 1]
    for done, size in enumerate(sizes, 1):
        msg = S.stream(asm, S.chunked(data, size))
        assert type(msg) is wire.StreamedMessage and not isinstance(msg, bytes) and len(msg) == len(data)
        assert msg.streamed, size
        _same(wire.loads_reference(msg, resident=True, **kw), want)
        assert msg.joins == 0  # the lazy join was never made
        st = wire.reference_stats()
        assert (st["streamed"], st["stream_fallback"], st["resident"]) == (done, 0, done + 1) and S.HostStream.opened == done
    assert S.HostStream.pushed == len(sizes) * (len(data) - b)  # each message's bytes from the header on, once
    assert bytes(msg) == data and msg.joins == 1 and bytes(msg) is bytes(msg) and msg.joins == 1


def test_one_byte_chunks(host_run):
    """The first four chunks are four bytes: the message is the array itself, its 3-byte header and one item's byte."""
    vals = S.lom_values(120, 9)
    data = U.packb(vals)
    assert len(data) < 600
    kw = dict(min_items=8, device_scan_min_items=8)
    msg = S.stream(wire.StreamAssembler(**kw), S.chunked(data, 1))
    # (the block is bounded by size * len(first chunk): the message's length exactly)
    got = wire.loads_reference(msg, resident=True, **kw)
    assert type(got) is wire.ResidentUpdate and got.tolist() == vals and msg.joins == 0
    assert wire.reference_stats()["streamed"] == 1 and S.HostStream.opened == 1


def test_messages_that_are_not_streamed(host_run):
    data, vals = S.lom_message()
    kw = dict(object_hook=U.ref_hook, min_items=16, device_scan_min_items=32, device_scan_jl_min_items=32)
    asm = wire.StreamAssembler(**kw)
    one = asm.add(data, 1, 1)  # a single chunk
    assert not one.streamed and S.HostStream.opened == 0
    jl, _ = S.jl_message()
    nohook = dict(kw, object_hook=None)
    msg = S.stream(wire.StreamAssembler(**nohook), S.chunked(jl, 999))  # no hook that reads the map: never a candidate
    assert not msg.streamed and S.HostStream.opened == 0
    assert wire.loads_reference(msg, resident=True, **nohook) == msgpack.unpackb(jl, strict_map_key=False) and msg.joins == 1
    plain = U.packb({"a": [1.5] * 3000, "b": "x"})
    msg = S.stream(asm, S.chunked(plain, 1000))
    assert not msg.streamed and wire.loads_reference(msg, resident=True, **kw) == U.unpackb(plain)
    bad = bytearray(data)
    bad[9] = 0xC1  # where the second string's header stood
    msg = S.stream(asm, S.chunked(bytes(bad), 1000))
    assert not msg.streamed
    with pytest.raises(Exception) as e1:
        wire.loads_reference(msg, resident=True, **kw)
    with pytest.raises(Exception) as e2:
        wire.loads_reference(bytes(bad), resident=True, **kw)
    assert type(e1.value) is type(e2.value) and S.HostStream.opened == 0
    assert wire.reference_stats()["stream_fallback"] == 0  # none of them began


def test_fallbacks_on_the_host_run(host_run):
    data, vals = S.lom_message()
    kw = dict(object_hook=U.ref_hook, min_items=16, device_scan_min_items=32, device_scan_jl_min_items=32)
    far = dict(kw, device_scan_min_items=FAR, device_scan_jl_min_items=FAR)
    asm = wire.StreamAssembler(**kw)
    # other arguments than the assembler's, and resident=False: the call on the joined bytes
    msg = S.stream(asm, S.chunked(data, 3000))
    got = wire.loads_reference(msg, resident=True, **far)
    assert msg.joins == 1 and not msg.streamed and got["params"].tolist() == vals
    msg = S.stream(asm, S.chunked(data, 3000))
    got = wire.loads_reference(msg, object_hook=U.ref_hook, min_items=16)
    assert isinstance(got["params"], wire.EncryptedParams) and got["params"] == vals and msg.joins == 1
    assert wire.reference_stats()["stream_fallback"] == 2
    # a later chunk longer than the first
    chunks = [data[:3000], data[3000:6000], data[6000:]]
    assert len(chunks[2]) > 3000
    msg = S.stream(asm, chunks)
    assert not msg.streamed and wire.loads_reference(msg, resident=True, **far)["params"].tolist() == vals
    assert wire.reference_stats()["stream_fallback"] == 3
    # a truncated message (the tokenizer refuses the array the end cuts off) and trailing bytes (the reduced message does
    # not unpack) leave the streamed read for the joined call, which takes the device: tests/test_wire_stream_gpu.py has
    # what that call then returns or raises
    b, first, e, n, _, _ = S.locate(data)
    for bad in (data[:e - 1], data + b"\x01"):
        before = wire.reference_stats()
        msg = S.stream(asm, S.chunked(bad, 3000))
        assert msg.streamed
        assert wire._loads_streamed(msg, U.ref_hook, 16, True, 32, 32) is wire._NOT_STREAMED and not msg.streamed
        after = wire.reference_stats()
        assert after["stream_fallback"] == before["stream_fallback"] + 1 and after["resident"] == before["resident"]
    assert wire.reference_stats()["streamed"] == 0


def test_assembler_survives_a_device_side_that_raises(host_run, monkeypatch):
    """A block that cannot be had (the peer's `size` decides its bytes) and a push that raises leave `add` the plain
    assembler for that message, and the next message starts clean."""
    data, vals = S.lom_message()
    kw = dict(object_hook=U.ref_hook, min_items=16, device_scan_min_items=32, device_scan_jl_min_items=32)
    far = dict(kw, device_scan_min_items=FAR, device_scan_jl_min_items=FAR)
    asm = wire.StreamAssembler(**kw)
    calls = []

    def no_memory(*a):
        calls.append(a)
        raise RuntimeError("out of memory")

    monkeypatch.setattr(wire, "_open_stream", no_memory)
    msg = S.stream(asm, S.chunked(data, 3000))
    assert len(calls) == 1 and not msg.streamed and len(msg) == len(data) and bytes(msg) == data  # asked once, not per chunk
    assert wire.loads_reference(msg, resident=True, **far)["params"].tolist() == vals
    assert wire.reference_stats()["stream_fallback"] == 0  # it never began

    class Raising(S.HostStream):
        def push(self, chunk, offset, last):
            if offset >= 6000:
                raise RuntimeError("device error")
            return super().push(chunk, offset, last)

    monkeypatch.setattr(wire, "_open_stream", Raising)
    msg = S.stream(asm, S.chunked(data, 3000))
    assert not msg.streamed and bytes(msg) == data
    assert wire.loads_reference(msg, resident=True, **far)["params"].tolist() == vals
    assert wire.reference_stats()["stream_fallback"] == 1
    monkeypatch.setattr(wire, "_open_stream", S.HostStream)
    msg = S.stream(asm, S.chunked(data, 3000))  # the same assembler, the next message
    assert msg.streamed and len(msg) == len(data)
    assert wire.loads_reference(msg, resident=True, **kw)["params"].tolist() == vals and msg.joins == 0
    # a message whose announced size asks for more than max_block_bytes is kept, not streamed: no device call
    S.HostStream.opened = 0
    small = wire.StreamAssembler(max_block_bytes=4096, **kw)
    msg = S.stream(small, S.chunked(data, 3000))
    assert not msg.streamed and S.HostStream.opened == 0 and bytes(msg) == data
    huge = wire.StreamAssembler(**kw)
    assert huge.add(data[:3000], 2**40, 1) is None and S.HostStream.opened == 0  # size * 3000 bytes: far past 1 GiB


def test_push_decision_is_the_shipped_one():
    """`_device.wire_stream_step`, which `_device.WireStream.push` and the host stand-in both follow."""
    from fedbiomed_amd import _device as D

    begin, first, cap = 100, 103, 1000
    assert D.wire_stream_step(begin, first, cap, 0, 50, False) == (100, 50, -50, False)      # in front of the array
    assert D.wire_stream_step(begin, first, cap, 50, 53, False) == (100, 103, 3, False)      # the header only: nothing to feed
    assert D.wire_stream_step(begin, first, cap, 50, 54, False) == (100, 104, 4, True)       # item 0's first byte
    assert D.wire_stream_step(begin, first, cap, 200, 800, True) == (200, 1000, 900, True)   # to the bound exactly
    assert D.wire_stream_step(begin, first, cap, 200, 801, False) is None                    # past it
    assert D.wire_stream_step(begin, first, cap, 50, 53, True) is None                       # the message ends before item 0
    assert D.wire_stream_step(begin, first, cap, 0, 50, True) is None

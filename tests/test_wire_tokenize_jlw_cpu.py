"""The wide tokenizer (items of up to 536 bytes) without a GPU: the library's host run of the kernels' three passes
(fbm_test_wire_tokenize_jlw) against a plain walk of the bytes by the item rule, and the host run of the resumable scan
(fbm_test_wire_stream_*_jlw) against the whole-span run.  Shapes: `message` lays items so that one starts on a tile's
last byte (a 536-byte item then enters the next tile at offset 535, the largest) and inside its last 23 bytes; the
scan's run boundary takes more than 256 tiles, 2 MB of full-width items."""
import random
import struct

import numpy as np
import pytest

from tests import wire_reference_util as U
from tests.wire_tokenize_util import placed

TILE, GUARD = 4096, 0xA5A5A5A5A5A5A5A5
LENGTHS = (1, 2, 255, 256, 257, 258, 512, 513)


def item(L, form=None, first=None):
    """The map item of L value bytes (c4 up to 255 unless `form` says c5); the first byte 0 at L = 513."""
    form = form or (b"\xc4" if L <= 255 else b"\xc5")
    head = form + (bytes([L]) if form == b"\xc4" else struct.pack(">H", L) if form == b"\xc5" else struct.pack(">I", L))
    return U.PREFIX + head + bytes([(0 if L == 513 else 0x11) if first is None else first]) + b"\x5a" * (L - 1)


def walk(data, first, n):
    """The item rule: (leading accepted items inside the data, item n - 1's end or 0, the table's words)."""
    p, table = first, []
    while len(table) < n and data[p:p + 20] == U.PREFIX and data[p + 20:p + 21] in (b"\xc4", b"\xc5"):
        h = 2 if data[p + 20] == 0xC4 else 3
        L, v = int.from_bytes(data[p + 21:p + 20 + h], "big"), p + 20 + h
        if not 1 <= L <= 513 or v + L > len(data) or data[v] >= 0x80 or (L == 513 and data[v]):
            break
        table.append(v << 16 | L)
        p = v + L
    return len(table), (p if len(table) == n else 0), table


def message(starts=(), total=3 * TILE, tail=()):
    """dc + count, then items such that one starts at each offset of `starts` (ascending, from the aligned word that
    holds item 0: the first tile's beginning under head 3) and the items end at `total`; then `tail`'s items."""
    items, at = [], 3
    for stop in list(starts) + [total]:
        while at < stop:
            gap = stop - at
            size = gap if gap <= 536 else 536 if gap - 536 >= 23 else gap - 23
            items.append(item(1) if size == 23 else item(size - 23, b"\xc5"))
            at += size
    items += list(tail)
    return b"\xdc" + struct.pack(">H", len(items)) + b"".join(items), 3, len(items)


def host_run(lib, span, base, first, n, head=3):
    """fbm_test_wire_tokenize_jlw with span[first - base] at an address that is `head` mod 4: (rc, [count, end], table)."""
    buf = placed(span, first - base, head)
    ck, res = np.full(n + 1, GUARD, dtype=np.uint64), np.full(3, GUARD, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_tokenize_jlw_workspace(len(span))) // 8 + 1, dtype=np.uint64)
    rc = lib.fbm_test_wire_tokenize_jlw(buf.ctypes.data, len(span), base, first, n, ck.ctypes.data, n, res.ctypes.data,
                                        ws.ctypes.data)
    assert ck[n] == GUARD and res[2] == GUARD
    return rc, res[:2].tolist(), ck[:n].tolist()


def host_feeds(lib, buf, first, n, avails):
    """One stream over `buf` fed up to each of `avails` (the last one final): ([count, end], table)."""
    tab, state = np.full(n, GUARD, dtype=np.uint64), np.zeros(16, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_stream_jlw_workspace(buf.size)) // 8 + 1, dtype=np.uint64)
    assert lib.fbm_test_wire_stream_begin_jlw(first, n, state.ctypes.data) == 0
    for k, a in enumerate(avails):
        assert lib.fbm_test_wire_stream_feed_jlw(buf.ctypes.data, 0, a, int(k == len(avails) - 1), tab.ctypes.data, n,
                                                 state.ctypes.data, ws.ctypes.data) == 0, a
    return state[3:5].tolist(), tab.tolist()


@pytest.fixture(scope="module")
def lib():
    from fedbiomed_amd import _build, _native

    _build.build()
    return _native.load_test()


WHOLE = {
    "lengths": message(total=0, tail=[item(L) for L in LENGTHS] + [item(200, b"\xc5"), item(513)]),
    "tile-last-byte-exit-535": message([TILE - 1, TILE - 1 + 536], tail=[item(7)]),
    "header-straddles": message([TILE - 23, 2 * TILE - 12, 3 * TILE - 2], total=3 * TILE + 300),
    "runs-of-two-tiles": message(total=3 + 4000 * 536),
}


@pytest.mark.parametrize("name", WHOLE)
def test_host_run_equals_the_walk(lib, name):
    data, first, n = WHOLE[name]
    count, end, table = walk(data, first, n)
    assert count == n and end == len(data) and (name != "runs-of-two-tiles" or len(data) // TILE > 2 * 256)
    for head in ((0, 1, 2, 3) if len(data) < 100_000 else (3,)):  # item 0 at each of the four byte alignments
        assert host_run(lib, data, 0, first, n, head) == (0, [n, end], table), head
    assert host_run(lib, data[1:] + item(513), 1, first, n) == (0, [n, end], table)  # another base, an item behind the array
    assert host_run(lib, data[:-5], 0, first, n)[1] == [n - 1, 0] == list(walk(data[:-5], first, n)[:2])  # cut off by the span's end


REFUSED = {"native-int": b"\x05", "L513-nonzero": item(513, first=1), "L514": item(514, first=0),
           "sign-byte": item(9, first=0x80), "bin32": item(4, b"\xc6")}


@pytest.mark.parametrize("name", REFUSED)
@pytest.mark.parametrize("at", [2, 10])
def test_counting_stops_at_a_refused_item(lib, name, at):
    items = [item(513)] * at + [REFUSED[name]] + [item(30)] * 3  # (among the first tile's items, and in the second tile)
    data = b"\xdc" + struct.pack(">H", len(items)) + b"".join(items)
    assert walk(data, 3, len(items))[:2] == (at, 0)
    for head in (0, 3):
        rc, res, ck = host_run(lib, data, 0, 3, len(items), head)
        assert (rc, res, ck[:at]) == (0, [at, 0], walk(data, 3, len(items))[2])


def test_argument_errors_are_fbm_wire_tokenize_jls(lib):
    from fedbiomed_amd import _native as N

    data, first, n = WHOLE["lengths"]
    buf, ck, res, ws = placed(data, first, 0), np.zeros(n, np.uint64), np.zeros(2, np.uint64), np.zeros(4096, np.uint64)

    def run(span=buf.ctypes.data, f=first, items=n, tab=ck.ctypes.data, n_ck=n, out=res.ctypes.data, w=ws.ctypes.data):
        return lib.fbm_test_wire_tokenize_jlw(span, len(data), 0, f, items, tab, n_ck, out, w)

    assert run(items=0, span=None, n_ck=0) == N.FBM_OK and run() == N.FBM_OK and res.tolist() == [n, len(data)]
    assert [run(span=None), run(tab=None), run(out=None), run(w=None), run(n_ck=n - 1), run(tab=ck.ctypes.data + 4),
            run(f=len(data)), run(items=2**32, n_ck=2**32)] == [N.FBM_E_ARG] * 7 + [N.FBM_E_UNSUPPORTED]
    assert N.load().fbm_wire_stream_begin(N.WIRE_JLW, 3, 1, res.ctypes.data, None) == N.FBM_E_ARG  # the narrow stream's refusal


def test_streamed_feed_equals_the_whole_span_run(lib):
    """Every split point of a three-tile message as two feeds, then one random split sequence."""
    data, first, n = WHOLE["header-straddles"]
    buf = placed(data, first, 3)
    want = host_run(lib, data, 0, first, n)[1:]
    for a in range(first + 1, len(data) + 1):
        assert host_feeds(lib, buf, first, n, [a, len(data)]) == want, a
    cuts = sorted(random.Random(5).sample(range(first + 1, len(data)), 40)) + [len(data)]
    assert host_feeds(lib, buf, first, n, cuts) == want
    assert host_feeds(lib, buf[:len(data) - 5], first, n, [TILE, 2 * TILE + 536, len(data) - 5])[0] == [n - 1, 0]  # cut off


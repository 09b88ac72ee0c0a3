"""Shared by tests/test_wire_tokenize_jl_cpu.py and tests/test_wire_tokenize_jl_gpu.py: the inputs of the device
tokenizer for arrays of big-int maps (fbm_wire_tokenize_jl) and what it must answer, from a plain Python walk written
from the byte layout and from fbm_wire_scan's table -- never from the code under test.

An item is  82 a8 "__type__" a3 "int" a5 "value"  (20 bytes), then  c4 L  or  c5 Lhi Llo  (minimal or not), then L
value bytes, 1 <= L <= 257, the first of them < 0x80 and, where L == 257, zero.  Its table word is (offset of the
value's first byte) << 16 | L.

The implementation cuts the stream into tiles of 4096 bytes counted from item 0's ADDRESS rounded down to four bytes
and, in its scan of the tiles' maps, runs of ceil(tiles / 256) tiles per thread; `head` = (address of item 0) mod 4.
wire_tokenize_util.placed puts a span at the address that gives the wanted head."""
import ctypes

import numpy as np

from tests import wire_reference_util as U
from tests.wire_tokenize_util import GUARD, header, placed

TILE, REACH, SCAN_THREADS = 4096, 280, 256
PREFIX = b"\x82\xa8__type__\xa3int\xa5value"
assert len(PREFIX) == 20
HEAD = b"\x82" + U.packb("node") + U.packb("n0") + U.packb("params")


def walk(data, first, n, limit=None):
    """The sequential walk: (leading whole map items inside data[:limit], at most n; the offset one past item n - 1
    or 0; the table words of those items)."""
    limit = len(data) if limit is None else limit
    p, table = first, []
    while len(table) < n:
        if data[p:p + 20] != PREFIX or p + 22 > limit:
            break
        if data[p + 20] == 0xC4:
            L, v = data[p + 21], p + 22
        elif data[p + 20] == 0xC5 and p + 23 <= limit:
            L, v = data[p + 21] << 8 | data[p + 22], p + 23
        else:
            break
        if not 1 <= L <= 257 or v + L > limit or data[v] >= 0x80 or (L == 257 and data[v] != 0):
            break
        table.append(v << 16 | L)
        p = v + L
    return len(table), (p if len(table) == n else 0), table


def item(L, form=None, value=None, fill=0x5A):
    """One map item of L value bytes: bin8 ("c4", L <= 255) or bin16 ("c5"); the shortest form by default."""
    form = form or ("c4" if L <= 255 else "c5")
    if value is None:
        value = (b"\x00" if L == 257 else b"\x01") + bytes([fill]) * (L - 1)
    assert len(value) == L
    return PREFIX + (bytes([0xC4, L]) if form == "c4" else bytes([0xC5, L >> 8, L & 0xFF])) + value


def sized(size, fill=0x5A):
    """One accepted item of exactly `size` bytes, 23..280."""
    assert 23 <= size <= 280
    return item(size - 22, "c4", fill=fill) if size <= 277 else item(size - 23, "c5", fill=fill)


def filling(total):
    """Accepted items of exactly `total` bytes together (0, or at least 46)."""
    out = []
    while total > 560:
        out.append(sized(280))
        total -= 280
    if total > 280:
        out.append(sized(total // 2))
        total -= total // 2
    if total:
        out.append(sized(total))
    return out


def message(items, tail=b"", n=None):
    """(message, offset of item 0, n): the items as one array behind a small map's keys; `n`: the header's count where
    it is not the number of items (native ints among them, bytes cut off)."""
    n = len(items) if n is None else n
    data = HEAD + header(n) + b"".join(items) + tail
    return data, len(HEAD) + len(header(n)), n


# the size classes: (L, form)
CLASSES = [(1, "c4"), (9, "c4"), (10, "c4"), (255, "c4"), (255, "c5"), (256, "c5"), (257, "c5")]


def whole_cases():
    """(name, message, first, n) of the arrays the tokenizer takes whole: every case's table is fbm_wire_scan's."""
    out = []
    for L, form in CLASSES:
        out.append((f"all-{form}-{L}",) + message([item(L, form, fill=0x30 + i % 64) for i in range(40)]))
    out.append(("mixed",) + message([item(*CLASSES[(i * 5 + i // 7) % 7], fill=i % 251) for i in range(150)]))
    out.append(("one",) + message([item(257)]))
    out.append(("one-short",) + message([item(1)]))
    # an item whose header lies across the first tile boundary with s of its bytes in front of it: s = 0 starts on
    # the boundary, s = 23 is a bin16 header that ends on it; with head 0 the boundary is TILE bytes behind item 0
    for s in range(0, 24):
        items = filling(TILE - s) + [item(257 if s % 2 else 200, "c5")] + filling(600)
        out.append((f"split-{s}",) + message(items))
    out.append(("ends-on-tile",) + message(filling(TILE) + filling(300)))
    # decoys: a value that holds a whole accepted item, the decoy's first byte at offsets 30 and 279 of the second
    # tile (an entry of that tile's map which the chain never takes), and a value of 82 bytes only
    for at in (30, 279):
        decoy = item(3, "c4", value=b"\x01\x02\x03")
        start = TILE + at - 23 - 100  # the carrier's first byte: its value's byte 100 is the decoy's first
        value = b"\x00" + b"\x11" * 99 + decoy + b"\x22" * (257 - 100 - len(decoy))
        items = filling(start) + [item(257, "c5", value=value)] + filling(700)
        out.append((f"decoy-{at}",) + message(items))
    out.append(("all-82",) + message([item(257, value=b"\x00" + b"\x82" * 256)] * 40))
    out.append(("prefix-in-value",) + message([item(200, value=b"\x01" + (PREFIX + b"\xc4")[:199].ljust(199, b"\x82"))] * 50))
    # more than 256 tiles: a thread's run is two tiles, and thread 0 chains the runs
    out.append(("runs-258-tiles",) + message([item(257 if i % 3 else 120, fill=i % 256) for i in range(4700)]))
    return out


def bad_items():
    """(name, bytes) of what stands where an item should and is none."""
    wrong = bytearray(item(40))
    wrong[13] ^= 0x01  # one prefix byte
    return [("L0", PREFIX + b"\xc4\x00"), ("L258", item(258, "c5", value=b"\x00" * 258)),
            ("L257-nonzero", item(257, "c5", value=b"\x01" + b"\x33" * 256)), ("sign", item(8, value=b"\x80" + b"\x01" * 7)),
            ("bin32", PREFIX + b"\xc6\x00\x00\x00\x04\x01\x02\x03\x04"), ("prefix", bytes(wrong)), ("native", b"\x05")]


def refused_cases():
    """(name, message, first, n, want count): each bad item at item 0, in the middle and at n - 1 of 40."""
    out, n = [], 40
    for name, bad in bad_items():
        for k in (0, 17, n - 1):
            items = [item(*CLASSES[i % 7], fill=i) for i in range(n)]
            items[k] = bad
            out.append((f"{name}-at-{k}",) + message(items) + (k,))
    return out


def host_tokenize(lib, span: bytes, base: int, first: int, n: int, head: int = 0):
    """fbm_test_wire_tokenize_jl: (rc, [count, end], table); the words around the table and the result stay."""
    buf = placed(span, first - base, head)
    ck = np.full(n + 2, GUARD, dtype=np.uint64)
    res = np.full(4, GUARD, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_tokenize_jl_workspace(len(span))) // 8 + 1, dtype=np.uint64)
    rc = lib.fbm_test_wire_tokenize_jl(buf.ctypes.data, len(span), base, first, n, ck[1:].ctypes.data, n,
                                       res[1:].ctypes.data, ws.ctypes.data)
    assert ck[0] == GUARD and ck[-1] == GUARD and res[0] == GUARD and res[3] == GUARD
    return rc, res[1:3].tolist(), ck[1:-1].tolist()


def device_tokenize(span: bytes, base: int, first: int, n: int, head: int = 0):
    """fbm_wire_tokenize_jl on the device, same answer shape as host_tokenize."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd import _native as N

    lib, dev = N.load(), D.device()
    raw = torch.zeros(len(span) + 16, dtype=torch.uint8, device=dev)
    shift = (head - (raw.data_ptr() + first - base)) % 4
    buf = raw[shift:shift + len(span)]
    buf.copy_(torch.from_numpy(np.frombuffer(span, dtype=np.uint8).copy()))
    guard = np.array(GUARD, dtype=np.uint64).view(np.int64).item()
    ck = torch.full((n + 2,), guard, dtype=torch.int64, device=dev)
    res = torch.full((4,), guard, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.fbm_wire_tokenize_jl_workspace(len(span))), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.fbm_wire_tokenize_jl(ctypes.c_void_p(buf.data_ptr()), len(span), base, first, n,
                                      ctypes.c_void_p(ck[1:].data_ptr()), n, ctypes.c_void_p(res[1:].data_ptr()),
                                      ctypes.c_void_p(ws.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
    ck, res = ck.cpu().numpy().view(np.uint64), res.cpu().numpy().view(np.uint64)
    assert ck[0] == GUARD and ck[-1] == GUARD and res[0] == GUARD and res[3] == GUARD
    return rc, res[1:3].tolist(), ck[1:-1].tolist()


def scan_one(data):
    """fbm_wire_scan's record of the message's one array: (begin, end, n, scheme, table as a list)."""
    from fedbiomed_amd import _device as D

    (b, e, n, scheme, ck), = D.wire_scan(data, 1)
    return b, e, n, scheme, ck.tolist()

"""Shared by tests/test_wire_tokenize_cpu.py and tests/test_wire_tokenize_gpu.py: the inputs of the device tokenizer
(fbm_wire_tokenize_lom) and what it must answer, from a plain Python walk and from fbm_wire_scan's table -- never
from the code under test.

The implementation cuts the stream into sub-blocks of 64 bytes, tiles of 4096 bytes and, in its scan of the tiles'
maps, runs of ceil(tiles / 256) tiles per thread, all counted from item 0's ADDRESS rounded down to four bytes: `head`
= (address of item 0) mod 4 bytes lie in front of item 0 in the first sub-block.  `placed` puts a span at the
address that gives the wanted head, so that a case can put an item exactly on a boundary (head 0) and off it."""
import ctypes

import msgpack
import numpy as np

from tests import wire_fold_util as F
from tests import wire_reference_util as U

SUB, TILE, SCAN_THREADS, GROUP = 64, 4096, 256, 64
GUARD = 0xA5A5A5A5A5A5A5A5
LEN = {0xCC: 2, 0xCD: 3, 0xCE: 5, 0xCF: 9}
# items that are no native form: the big-int map's first bytes, a negative fixint, int8, float64, the unused byte
NON_NATIVE = [b"\x82\xa8__type__\xa3int\xa5value\xc4\x02\x00\x80", b"\xe0", b"\xd0\x05", b"\xcb" + bytes(8), b"\xc1"]


def header(n):
    return msgpack.Packer().pack_array_header(n)


def walk(data, first, n, limit=None):
    """The sequential walk: (leading whole native items inside data[:limit], at most n; the offset one past item
    n - 1 or 0; the offsets of items 0, 64, 128, ... among them)."""
    limit = len(data) if limit is None else limit
    p, table, count = first, [], 0
    while count < n and p < limit:
        b = data[p]
        size = 1 if b <= 0x7F else LEN.get(b, 0)
        if size == 0 or p + size > limit:
            break
        if count % GROUP == 0:
            table.append(p)
        p += size
        count += 1
    return count, (p if count == n else 0), table


def nine(payload_byte):
    return b"\xcf" + bytes([payload_byte]) * 8


def ones(k, v=0x11):
    return bytes([v]) * k


def boundary_items(boundary, how, total):
    """Items whose bytes, counted from item 0, put one 9-byte item at a boundary: "ends" on the boundary's last
    byte, "spans" it, or "starts" on it; 1-byte items in front, 9-byte items behind up to `total` bytes."""
    start = {"ends": boundary - 9, "spans": boundary - 4, "starts": boundary}[how]
    items = [ones(1)] * start + [nine(0xCF)]
    fill = max(0, total - start - 9)
    items += [nine(0x00)] * (fill // 9) + [ones(1)] * (fill % 9)
    return items


def array_message(items, tail=None):
    """(message, offset of item 0, n): the items as one array inside wire_fold_util's small message."""
    arr = header(len(items)) + b"".join(items)
    if tail is None:
        data, off = F.message(arr)
    else:
        head = b"\x82" + U.packb("params")
        data, off = head + arr + tail, len(head)
    return data, off + len(header(len(items))), len(items)


def boundary_cases():
    """(name, message, first, n) per boundary and position.  The run boundary needs more than 256 tiles: with 257 to
    512 tiles a thread's run is two tiles, so thread 1 starts at byte 8192."""
    out = []
    for name, boundary, total in (("sub", SUB, 3 * SUB), ("tile", TILE, TILE + 3 * SUB), ("run", 2 * TILE, 257 * TILE + 100)):
        for how in ("ends", "spans", "starts"):
            out.append((f"{name}-{how}",) + array_message(boundary_items(boundary, how, total)))
    return out


def pool_items(n, off=0):
    pool = F.item_pool()
    return [pool[(off + i) % len(pool)][0] for i in range(n)]


def placed(span: bytes, s0: int, head: int) -> np.ndarray:
    """The span in host memory such that (address of span[s0]) mod 4 == head."""
    raw = np.zeros(len(span) + 16, dtype=np.uint8)
    shift = (head - (raw.ctypes.data + s0)) % 4
    view = raw[shift:shift + len(span)]
    view[:] = np.frombuffer(span, dtype=np.uint8)
    assert (view.ctypes.data + s0) % 4 == head
    return view


def host_tokenize(lib, span: bytes, base: int, first: int, n: int, head: int = 0):
    """fbm_test_wire_tokenize_lom: (rc, [count, end], table); the words around the table and the result stay."""
    buf = placed(span, first - base, head)
    n_ck = (n + GROUP - 1) // GROUP
    ck = np.full(n_ck + 2, GUARD, dtype=np.uint64)
    res = np.full(4, GUARD, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_tokenize_workspace(len(span))) // 8 + 1, dtype=np.uint64)
    rc = lib.fbm_test_wire_tokenize_lom(buf.ctypes.data, len(span), base, first, n, ck[1:].ctypes.data, n_ck,
                                        res[1:].ctypes.data, ws.ctypes.data)
    assert ck[0] == GUARD and ck[-1] == GUARD and res[0] == GUARD and res[3] == GUARD
    return rc, res[1:3].tolist(), ck[1:-1].tolist()


def device_tokenize(span: bytes, base: int, first: int, n: int, head: int = 0):
    """fbm_wire_tokenize_lom on the device, same answer shape as host_tokenize."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd import _native as N

    lib, dev = N.load(), D.device()
    raw = torch.zeros(len(span) + 16, dtype=torch.uint8, device=dev)
    shift = (head - (raw.data_ptr() + first - base)) % 4
    buf = raw[shift:shift + len(span)]
    buf.copy_(torch.from_numpy(np.frombuffer(span, dtype=np.uint8).copy()))
    n_ck = (n + GROUP - 1) // GROUP
    guard = np.array(GUARD, dtype=np.uint64).view(np.int64).item()
    ck = torch.full((n_ck + 2,), guard, dtype=torch.int64, device=dev)
    res = torch.full((4,), guard, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.fbm_wire_tokenize_workspace(len(span))), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.fbm_wire_tokenize_lom(ctypes.c_void_p(buf.data_ptr()), len(span), base, first, n,
                                       ctypes.c_void_p(ck[1:].data_ptr()), n_ck, ctypes.c_void_p(res[1:].data_ptr()),
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


def whole_cases():
    """(name, message, first, n) of the arrays the tokenizer takes whole: every case's table is fbm_wire_scan's."""
    out = []
    for n in F.NS:
        arr, _ = F.lom_array(n)
        data, off = F.message(arr)
        out.append((f"pool-{n}", data, off + len(header(n)), n))
    out += boundary_cases()
    out.append(("ones-300",) + array_message([ones(1, i % 128) for i in range(300)]))
    for pb in (0xCF, 0xCC, 0x82, 0xC1, 0x00):
        out.append((f"nines-{pb:02x}",) + array_message([nine(pb)] * 130))
    return out


def refused_cases():
    """(name, message, first, n, want count): a non-native item at item 0, 1, 63, 64 and n - 1 of 200, and as the
    first byte of the second tile (head 0)."""
    out = []
    n = 200
    for k, bad in zip((0, 1, 63, 64, n - 1), NON_NATIVE):
        items = pool_items(n, 2)
        items[k] = bad
        out.append((f"bad-{k}",) + array_message(items) + (k,))
    for bad in (NON_NATIVE[0], NON_NATIVE[4]):
        items = [ones(1)] * TILE + [bad] + pool_items(70)
        out.append((f"bad-tile-edge-{bad[0]:02x}",) + array_message(items) + (TILE,))
    return out

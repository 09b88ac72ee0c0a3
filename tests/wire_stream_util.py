"""Shared by tests/test_wire_stream_cpu.py and tests/test_wire_stream_gpu.py: the two seeded messages of the streamed
receive path (fbm_wire_stream_begin / fbm_wire_stream_feed, wire.StreamAssembler), the feed runners over host and
device buffers, and the host stand-in for the device side of the assembler.  Expected tables are fbm_wire_scan's and
the one-shot tokenizers'; the messages are msgpack's own bytes (the reference encoder)."""
import ctypes
import random

import numpy as np

from tests import wire_reference_util as U
from tests.wire_tokenize_util import GUARD, placed

TILE, GROUP, STATE_WORDS = 4096, 64, 16
JL_LS = [1, 2, 31, 32, 255, 256, 257]


def lom_values(n=2500, seed=31):
    """Native ints over all five widths: 1, 2, 3, 5 and 9 bytes."""
    rng = random.Random(seed)
    tops = [127, 255, 65535, 2**32 - 1, 2**64 - 1]
    lows = [0, 128, 256, 65536, 2**32]
    out = []
    for i in range(n):
        k = rng.randrange(5)
        out.append(rng.randrange(lows[k], tops[k] + 1))
    return out


def jl_values(n=60, seed=37):
    """Big ints whose bin is L bytes, L over JL_LS (L = 257: a zero first byte; 256 and 257 are the c5 form)."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        L = JL_LS[i % len(JL_LS)] if i < 2 * len(JL_LS) else rng.choice(JL_LS)
        # the reference writes ceil(bits / 8) + 1 bytes, and a native form below 2^64: L >= 10 from an int, below by hand
        bits = 8 * (L - 1)
        out.append((1 << (bits - 1)) | rng.getrandbits(bits - 1) if L >= 10 else L)
    return out


def jl_item(v, L):
    """The map item of the value v in L bytes (c4 up to 255, c5 from 256 on), as the reference writes big ints."""
    from tests.wire_tokenize_jl_util import PREFIX

    return PREFIX + (bytes([0xC4, L]) if L <= 255 else bytes([0xC5, L >> 8, L & 255])) + v.to_bytes(L, "big")


def envelope(array_bytes, sample=1234):
    """A dict with a string key in front, "params" and "sample_size" behind it."""
    return b"\x83" + U.packb("node_id") + U.packb("node-7") + U.packb("params") + array_bytes + U.packb("sample_size") + U.packb(sample)


def lom_message(n=2500, seed=31):
    """(message, values): msgpack's bytes of the envelope with the native array."""
    vals = lom_values(n, seed)
    data = U.packb({"node_id": "node-7", "params": vals, "sample_size": 1234})
    assert data == envelope(U.packb(vals))
    return data, vals


def jl_message(n=60, seed=37):
    """(message, values): the envelope with n big-int maps; the items below L = 10 are written by hand (the reference
    packs such a value natively), the others are msgpack's own."""
    from tests.wire_tokenize_util import header

    vals = jl_values(n, seed)
    items = []
    for v in vals:
        L = v if v < 10 else (v.bit_length() + 7) // 8 + 1
        if v < 10:
            v = (1 << (8 * L - 2)) | 5 if L > 1 else 0x45  # L bytes with a first byte below 0x80
        items.append((v, L))
    data = envelope(header(n) + b"".join(jl_item(v, L) for v, L in items))
    out = [v for v, _ in items]
    big = [v for v, L in items if L >= 10]
    assert U.packb(big)[len(header(len(big))):] == b"".join(jl_item(v, L) for v, L in items if L >= 10)  # msgpack's own bytes
    assert U.unpackb(data)["params"] == out
    return data, out


def locate(data, min_items=1):
    """fbm_wire_scan's record of the message's first array: (begin, first, end, n, scheme, table list)."""
    from fedbiomed_amd import _device as D
    from tests.wire_tokenize_util import header

    b, e, n, scheme, ck = D.wire_scan(data, min_items)[0]
    return b, b + len(header(n)), e, n, scheme, ck.tolist()


def _sch(scheme):
    from fedbiomed_amd import _native as N

    return N.WIRE_JL if scheme == "jl" else N.WIRE_LOM


def n_ckpt(scheme, n):
    return n if scheme == "jl" else (n + GROUP - 1) // GROUP


def host_one_shot(lib, scheme, buf, base, first, n):
    """The one-shot host tokenizer over the placed span `buf`: ([count, end], table)."""
    nck = n_ckpt(scheme, n)
    ck, res = np.full(nck, GUARD, dtype=np.uint64), np.zeros(2, dtype=np.uint64)
    wsf, fn = (lib.fbm_wire_tokenize_jl_workspace, lib.fbm_test_wire_tokenize_jl) if scheme == "jl" else \
        (lib.fbm_wire_tokenize_workspace, lib.fbm_test_wire_tokenize_lom)
    ws = np.zeros(int(wsf(buf.size)) // 8 + 1, dtype=np.uint64)
    assert fn(buf.ctypes.data, buf.size, base, first, n, ck.ctypes.data, nck, res.ctypes.data, ws.ctypes.data) == 0
    return res.tolist(), ck.tolist()


def host_feeds(lib, scheme, buf, base, first, n, avails):
    """fbm_test_wire_stream_begin, then one feed per entry of `avails` (the last one with the last flag) over the placed
    span `buf`: (rcs, [count, end], table); the words around table and state stay."""
    nck = n_ckpt(scheme, n)
    ck = np.full(nck + 2, GUARD, dtype=np.uint64)
    state = np.full(STATE_WORDS + 2, GUARD, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_stream_workspace(_sch(scheme), buf.size)) // 8 + 1, dtype=np.uint64)
    rcs = [lib.fbm_test_wire_stream_begin(_sch(scheme), first, n, state[1:].ctypes.data)]
    for i, a in enumerate(avails):
        rcs.append(lib.fbm_test_wire_stream_feed(_sch(scheme), buf.ctypes.data, base, a, 1 if i == len(avails) - 1 else 0,
                                                 ck[1:].ctypes.data, nck, state[1:].ctypes.data, ws.ctypes.data))
    assert ck[0] == GUARD and ck[-1] == GUARD and state[0] == GUARD and state[-1] == GUARD
    return rcs, state[4:6].tolist(), ck[1:-1].tolist()


def device_feeds(scheme, span: bytes, base, first, n, avails, head=0, poison=0xC1):
    """fbm_wire_stream_begin and the feeds on the device.  The span lies in a block whose bytes in front of it and
    behind each feed's avail_len are `poison` until the feed that brings them: a read at or past avail_len, or in front
    of the span, would meet a byte that starts no item.  Returns (rcs, [count, end], table)."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd import _native as N

    lib, dev = N.load(), D.device()
    pad = 64
    raw = torch.full((len(span) + 2 * pad + 16,), poison, dtype=torch.uint8, device=dev)
    shift = pad + (head - (raw.data_ptr() + pad + first - base)) % 4
    buf = raw[shift:shift + len(span)]
    src = torch.from_numpy(np.frombuffer(span, dtype=np.uint8).copy()).to(dev)
    nck = n_ckpt(scheme, n)
    guard = np.array(GUARD, dtype=np.uint64).view(np.int64).item()
    ck = torch.full((nck + 2,), guard, dtype=torch.int64, device=dev)
    state = torch.full((STATE_WORDS + 2,), guard, dtype=torch.int64, device=dev)
    ws = torch.zeros(int(lib.fbm_wire_stream_workspace(_sch(scheme), len(span))), dtype=torch.uint8, device=dev)
    vp = ctypes.c_void_p
    with torch.cuda.device(dev):
        st = vp(torch.cuda.current_stream(dev).cuda_stream)
        rcs = [lib.fbm_wire_stream_begin(_sch(scheme), first, n, vp(state[1:].data_ptr()), st)]
        fed = 0
        for i, a in enumerate(avails):
            buf[fed:a].copy_(src[fed:a])
            fed = max(fed, a)
            rcs.append(lib.fbm_wire_stream_feed(_sch(scheme), vp(buf.data_ptr()), base, a, 1 if i == len(avails) - 1 else 0,
                                                vp(ck[1:].data_ptr()), nck, vp(state[1:].data_ptr()), vp(ws.data_ptr()), st))
        torch.cuda.synchronize()
    ck, state = ck.cpu().numpy().view(np.uint64), state.cpu().numpy().view(np.uint64)
    assert ck[0] == GUARD and ck[-1] == GUARD and state[0] == GUARD and state[-1] == GUARD
    assert bool((raw[:shift] == poison).all()) and bool((raw[shift + len(span):] == poison).all())
    return rcs, state[4:6].tolist(), ck[1:-1].tolist()


class HostHandle:
    """The streamed array's handle on the host run: decodes from the received block with the streamed table."""

    def __init__(self, data, array):
        self._data, self._array, self.released = data, array, False

    def rows_host(self):
        if self.released:
            raise RuntimeError("released")
        return U.host_decode(self._data, [self._array])[0]

    def release(self):
        self.released = True


class HostStream:
    """`_device.WireStream` on the library's host run (fbm_test_wire_stream_*): what `wire._open_stream` returns in the
    CPU tests.  `opened` counts the streams begun, `pushed` the bytes that went into blocks."""

    opened = 0
    pushed = 0

    def __init__(self, scheme, begin, first, n_items, cap, ctx):
        from fedbiomed_amd import _native as N

        HostStream.opened += 1
        self.lib = N.load_test()
        self.scheme, self.begin, self.first, self.n, self.cap, self.failed = scheme, begin, first, n_items, cap, False
        self.blk = placed(bytes(cap - begin), first - begin, 1)
        self.nck = n_ckpt(scheme, n_items)
        self.tab = np.zeros(self.nck, dtype=np.uint64)
        self.state = np.zeros(STATE_WORDS, dtype=np.uint64)
        self.ws = np.zeros(int(self.lib.fbm_wire_stream_workspace(_sch(scheme), cap - begin)) // 8 + 1, dtype=np.uint64)
        assert self.lib.fbm_test_wire_stream_begin(_sch(scheme), first, n_items, self.state.ctypes.data) == 0

    def push(self, chunk, offset, last):
        from fedbiomed_amd import _device as D

        if self.failed:
            return False
        step = D.wire_stream_step(self.begin, self.first, self.cap, offset, len(chunk), last)  # the shipped decision
        if step is None:
            self.failed = True
            return False
        lo, end, avail, feed = step
        if end > lo:
            self.blk[lo - self.begin:end - self.begin] = np.frombuffer(chunk, dtype=np.uint8)[lo - offset:]
            HostStream.pushed += end - lo
        if feed:
            rc = self.lib.fbm_test_wire_stream_feed(_sch(self.scheme), self.blk.ctypes.data, self.begin, avail, 1 if last else 0,
                                                    self.tab.ctypes.data, self.nck, self.state.ctypes.data, self.ws.ctypes.data)
            if rc != 0:
                self.failed = True
                return False
        return True

    def result(self):
        return int(self.state[3]), int(self.state[4])

    def handle(self, end):
        data = bytes(self.begin) + self.blk[:end - self.begin].tobytes()
        return HostHandle(data, (self.begin, end, self.n, self.scheme, self.tab.copy()))

    def abort(self):
        self.failed = True


def chunked(data: bytes, size: int):
    """The sender's cut: every chunk but the last `size` bytes."""
    return [data[i:i + size] for i in range(0, len(data), size)]


def stream(asm, chunks):
    """The transport's loop over `asm.add`: the message behind the last chunk, None asserted before."""
    out = None
    for i, c in enumerate(chunks, 1):
        out = asm.add(c, len(chunks), i)
        assert (out is None) == (i < len(chunks))
    return out

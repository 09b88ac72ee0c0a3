"""Shared by tests/test_wire_fold_cpu.py and tests/test_wire_fold_gpu.py: LOM arrays whose items cover every native
width boundary and every non-minimal form the scanner accepts, written by msgpack under the reference's rules
(tests/wire_reference_util.py) or byte by byte where msgpack itself would never write the form, placed inside a
small message; expected sums in Python integers."""
import random

import msgpack
import numpy as np

from tests import wire_reference_util as U

M64 = 2**64
NS = [1, 63, 64, 65, 127, 128, 129, 257, 1025]  # group (64) and workgroup (4 groups) edges
# a small value in each non-minimal form, and a 4-byte value in the 8-byte form
NON_MINIMAL = [(b"\xcc\x05", 5), (b"\xcd\x00\x05", 5), (b"\xce\x00\x00\x00\x05", 5), (b"\xcf" + bytes(7) + b"\x05", 5),
               (b"\xcf\x00\x00\x00\x00\xff\xff\xff\xff", 2**32 - 1)]


def item_pool(seed=11):
    """(bytes, value) of every boundary value in msgpack's own form, the non-minimal forms, and random values of
    every width."""
    rng = random.Random(seed)
    pool = [(U.packb(v), v) for v in U.NATIVE_EDGES] + list(NON_MINIMAL)
    for bits in (3, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64):
        v = rng.getrandbits(bits) | (1 << (bits - 1))
        pool.append((U.packb(v), v))
    return pool


def lom_array(n, off=0):
    """n items of the pool from position `off` on: (the array's bytes, its values)."""
    pool = item_pool()
    picks = [pool[(off + i) % len(pool)] for i in range(n)]
    data = msgpack.Packer().pack_array_header(n) + b"".join(b for b, _ in picks)
    vals = [v for _, v in picks]
    assert U.unpackb(data) == vals  # msgpack reads every form as that value
    return data, vals


def message(array_bytes, key="params"):
    """The array inside a small message, as a stock peer's reply holds it: (the message, the array's offset)."""
    head = b"\x83" + U.packb("researcher_id") + U.packb("r" * 37) + U.packb(key)
    tail = U.packb("round") + U.packb(3)
    return head + array_bytes + tail, len(head)


def minimal_values(n, seed=2):
    """n values a stock peer's packb writes (minimal forms only), every boundary among them."""
    rng = random.Random(seed)
    vals = list(U.NATIVE_EDGES) + [rng.getrandbits(rng.choice([3, 7, 8, 9, 16, 17, 32, 33, 64])) for _ in range(n)]
    rng.shuffle(vals)
    return vals[:n]


def folded(acc, vals, first):
    return [v % M64 if first else (a + v) % M64 for a, v in zip(acc, vals)]


def acc_values(n, seed=7):
    """A running accumulator: random words, with 2^64 - 1 where wrap-around shows."""
    rng = random.Random(seed)
    return [M64 - 1 if i % 5 == 0 else rng.getrandbits(64) for i in range(n)]


def u64(vals) -> np.ndarray:
    return np.array(vals, dtype=np.uint64)

"""The table path's exponent schedule as the library builds it (fbm_setup.hip build_schedule, read through
the test build's fbm_test_schedule hook), replayed in Python.  Host-only (no GPU).

The kernels run the schedule blindly: table[first], then per op `nsq` squarings and one product with
table[idx].  Replayed on the exponent itself -- e = 2 first + 1, then e = (e << nsq) + (2 idx + 1) -- it must
give |key| back.  What each key family is here for:

  - 2^k and 2^k - 1 at k = 1, 5, 6, 7 (the window width FBM_WIN = 6 and its neighbours), 31, 32, 33 (a key
    word's boundary), 1023, 1024, 1025 (a zero run at FBM_OP_MAXSQ = 1023: the split of a run of more
    squarings than an op's 10-bit field holds, on either side of the limit), 2047, 2048 (the widest key: all
    64 words);
  - 2^1100 + 1: a 1099-zero run INSIDE a window op (nsq = 1099 + 1: one split, then the op with its idx);
  - 2^2047 and 2^2047 + 1: two splits, in the trailing squarings and inside a window op;
  - 2^2048 - 1 and sum 2^(6 k), k < 342: one op per 6 bits, the densest schedule (341 ops after `first`);
  - seeded random keys of random length: everything in between.

Bounds: nsq <= 1023 and idx < 32 are the op's fields (FBM_OP_SHIFT = 6 bits of idx + 1, 10 bits of nsq in a
u16); n_ops <= 344 is one window op per 6 bits of a 2048-bit key (342) plus the two splits a key below 2^2048
can need (2047 = 2 x 1023 + 1) -- far below FBM_MAX_OPS = 512, so no key below 2^2048 may return FBM_E_ARG.
A zero key has no schedule (the hook returns 1: build_schedule's is_zero, n_ops = first = 0; the entry
points then compute h^0 = 1 without it)."""

import random

import numpy as np
import pytest

from fedbiomed_amd import _build, _native

MAX_OPS, OP_SHIFT, MAXSQ, WIN = 512, 6, 1023, 6  # fbm_internal.hpp FBM_MAX_OPS, FBM_OP_SHIFT, FBM_OP_MAXSQ, FBM_WIN
N_OPS_BOUND = 344

DENSE = sum(1 << (6 * k) for k in range(342))
EDGE_K = (1, 5, 6, 7, 31, 32, 33, 1023, 1024, 1025, 2047, 2048)
STRUCTURED = [1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1, (1 << 1100) + 1, 1 << 2047,
              (1 << 2047) + 1, (1 << 2048) - 1, DENSE, random.Random(2040).getrandbits(2040) | (1 << 2039)]
POWERS = [(1 << k) - d for k in EDGE_K for d in (0, 1) if (1 << k) - d < (1 << 2048)]


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _native.load_test()


def _schedule(lib, key):
    k64 = np.frombuffer(key.to_bytes(256, "little"), dtype=np.uint32).copy()
    ops = np.full(MAX_OPS, 0xFFFF, np.uint16)
    n_ops, first = np.full(1, -7, np.int32), np.full(1, -7, np.int32)
    rc = lib.fbm_test_schedule(k64.ctypes.data, ops.ctypes.data, n_ops.ctypes.data, first.ctypes.data)
    return rc, [int(v) for v in ops], int(n_ops[0]), int(first[0])


def _check(lib, key):
    """Replays the schedule of `key`; returns (n_ops, number of idx-less ops, widest nsq)."""
    rc, ops, n_ops, first = _schedule(lib, key)
    assert rc == _native.FBM_OK, (rc, hex(key))
    assert 0 <= n_ops <= N_OPS_BOUND, (n_ops, hex(key))
    assert 0 <= first < 32
    e = 2 * first + 1
    bare = widest = 0
    for op in ops[:n_ops]:
        nsq, idx = op >> OP_SHIFT, (op & ((1 << OP_SHIFT) - 1)) - 1
        assert nsq <= MAXSQ and idx < 32, (op, hex(key))
        assert nsq > 0 or idx >= 0, "an op that does nothing"
        e <<= nsq
        if idx >= 0:
            e += 2 * idx + 1
        else:
            bare += 1
        widest = max(widest, nsq)
    assert e == key, hex(key)
    assert all(op == 0 for op in ops[n_ops:]), "the hook copies the whole zero-initialised op array"
    return n_ops, bare, widest


@pytest.mark.parametrize("key", list(dict.fromkeys(STRUCTURED + POWERS)),
                         ids=lambda k: f"b{k.bit_length()}w{bin(k).count('1')}")  # bit length, set bits
def test_structured_keys_replay(lib, key):
    _check(lib, key)


def test_densest_schedules_and_splits(lib):
    """The figures the bounds rest on: 341 ops for the all-ones and the one-bit-in-six keys (one window op
    per 6 bits after the leading window), a split squaring run for 2^1100 + 1 and two for 2^2047 (+ 1)."""
    assert _check(lib, (1 << 2048) - 1)[0] == 341
    assert _check(lib, DENSE)[0] == 341
    # 2^1100 + 1: first = 0 (the lone top bit), then 1100 squarings and the product with table[0]: 1023 | 77 + idx
    assert _check(lib, (1 << 1100) + 1) == (2, 1, MAXSQ)
    # 2^2047: 2047 trailing squarings = 1023 + 1023 + 1, no product
    assert _check(lib, 1 << 2047) == (3, 3, MAXSQ)
    assert _check(lib, (1 << 2047) + 1) == (3, 2, MAXSQ)
    # a run of exactly 1023 squarings is one op; 1024 are two
    assert _check(lib, 1 << 1023) == (1, 1, MAXSQ)
    assert _check(lib, 1 << 1024) == (2, 2, MAXSQ)
    assert _check(lib, (1 << 1023) + 1) == (1, 0, MAXSQ)
    assert _check(lib, (1 << 1024) + 1) == (2, 1, MAXSQ)


def test_random_keys_replay(lib):
    rng = random.Random(670)
    most = 0
    for _ in range(4000):
        bits = rng.randint(1, 2048)
        key = rng.getrandbits(bits) | (1 << (bits - 1))
        if rng.random() < 0.25:  # long zero and one runs between random stretches
            lo, hi = sorted(rng.sample(range(bits + 1), 2))
            mask = ((1 << hi) - 1) ^ ((1 << lo) - 1)
            key = (key | mask) if rng.random() < 0.5 else (key & ~mask) | (1 << (bits - 1))
        most = max(most, _check(lib, key)[0])
    assert most > 300  # the sweep reaches full-width keys


def test_zero_key_has_no_schedule(lib):
    rc, ops, n_ops, first = _schedule(lib, 0)
    assert (rc, n_ops, first) == (1, 0, 0) and not any(ops)


def test_null_pointers_are_refused(lib):
    k64 = np.zeros(64, np.uint32)
    assert lib.fbm_test_schedule(k64.ctypes.data, None, None, None) == _native.FBM_E_ARG

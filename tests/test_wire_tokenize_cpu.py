"""The device tokenizer's per-block routines and the deferring host scanner without a GPU: fbm_test_wire_tokenize_lom
runs the kernels' three passes tile by tile over host buffers (the same `__host__ __device__` routines), and
fbm_wire_scan_deferred is plain C++.  Expected tables are fbm_wire_scan's, expected counts and ends a plain Python
walk's (tests/wire_tokenize_util.py).

Shapes.  The implementation's boundaries are the 64-byte sub-block, the 4096-byte tile and the scan's run of
ceil(tiles / 256) tiles per thread; each gets a 9-byte item ending on its last byte, spanning it and starting on it,
at head 0 (item 0 on a 4-byte address: the boundary falls exactly there) and at the other three heads.  The run
boundary needs more than 256 tiles, a message just over 1 MiB; everything else is a few hundred items."""
import ctypes

import numpy as np
import pytest

from tests import wire_fold_util as F
from tests import wire_reference_util as U
from tests import wire_tokenize_util as T


@pytest.fixture(scope="module")
def lib():
    from fedbiomed_amd import _build, _native

    _build.build()
    return _native.load_test()


WHOLE = T.whole_cases()
REFUSED = T.refused_cases()


def test_entry_points_are_declared(lib):
    from fedbiomed_amd import _native as N

    for name in ("fbm_wire_tokenize_workspace", "fbm_wire_tokenize_lom", "fbm_wire_scan_deferred"):
        assert name in N.SIGNATURES and hasattr(N.load(), name)
    assert "fbm_test_wire_tokenize_lom" in N.TEST_SIGNATURES and hasattr(lib, "fbm_test_wire_tokenize_lom")
    assert lib.fbm_abi_version() == 7


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_table_count_and_end_equal_the_scanner(lib, case):
    _, data, first, n = case
    b, e, n_scan, scheme, table = T.scan_one(data)
    assert (n_scan, scheme) == (n, "lom") and T.walk(data, first, n) == (n, e, table)
    heads = (0, 1, 2, 3) if len(data) < 100_000 else (0, 3)
    for head in heads:
        for base in (0, b):  # the whole message as the span, and the message from the array's header on
            rc, res, ck = T.host_tokenize(lib, data[base:], base, first, n, head)
            assert rc == 0 and res == [n, e] and ck == table, (head, base, res, e)
    rc, res, ck = T.host_tokenize(lib, data[b:e], b, first, n)  # the array's own span: nothing behind item n - 1
    assert rc == 0 and res == [n, e] and ck == table


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_counting_stops_at_a_non_native_item(lib, case):
    _, data, first, n, want = case
    assert T.walk(data, first, n)[0] == want
    for head in (0, 1, 2, 3):
        rc, res, _ = T.host_tokenize(lib, data, 0, first, n, head)
        assert rc == 0 and res == [want, 0], (head, res)


def test_span_cut_at_every_byte_of_the_last_item(lib):
    for n in (1, 64, 65, 200):
        items = T.pool_items(n - 1, 4) + [T.nine(0xCF)]
        data, first, _ = T.array_message(items)
        end = T.scan_one(data)[1]
        for cut in range(end - 9, end):  # item n - 1 starts at end - 9: 0..8 of its bytes are left
            assert T.walk(data, first, n, cut)[0] == n - 1
            if cut == first:  # (n == 1: item 0 itself lies outside such a span, an argument error)
                continue
            for head in (0, 2):
                rc, res, _ = T.host_tokenize(lib, data[:cut], 0, first, n, head)
                assert rc == 0 and res == [n - 1, 0], (n, cut, head, res)
    # a final partial sub-block shorter than the pending payload: the cut falls 2 bytes into a sub-block
    items = [T.ones(1)] * (T.SUB - 3) + [T.nine(0x00)]
    data, first, n = T.array_message(items)
    rc, res, _ = T.host_tokenize(lib, data[first:first + T.SUB + 2], first, first, n, 0)
    assert rc == 0 and res == [n - 1, 0]


def test_native_ints_behind_the_array_are_not_counted(lib):
    items = T.pool_items(130, 1)
    tail = b"\x05\x06\xcc\x80\xcf" + bytes(8) + b"\x07" * 200  # a key and values that are native ints themselves
    data, first, n = T.array_message(items, tail)
    count, end, table = T.walk(data, first, n)
    assert count == n and data[end:] == tail
    for head in (0, 1, 2, 3):
        rc, res, ck = T.host_tokenize(lib, data, 0, first, n, head)
        assert rc == 0 and res == [n, end] and ck == table
    # fewer items asked for than the array holds: capped, and the end is item n' - 1's
    for fewer in (1, 64, 65, 129):
        count, end, table = T.walk(data, first, fewer)
        rc, res, ck = T.host_tokenize(lib, data, 0, first, fewer)
        assert rc == 0 and res == [fewer, end] and ck == table


def test_random_arrays_against_the_walk(lib):
    """Seeded: native items of every width with payload bytes that look like markers, a non-native byte or a cut
    at a random place."""
    import random

    rng = random.Random(5)
    marks = [0xCC, 0xCD, 0xCE, 0xCF, 0x82, 0xC1, 0x00, 0x7F, 0xFF]
    for _ in range(300):
        n = rng.choice([1, 2, 63, 64, 65, 130, 500, 1000])
        items = []
        for _ in range(n):
            w = rng.choice([0, 0, 1, 2, 4, 8])
            items.append(bytes([rng.randrange(128)]) if w == 0 else
                         bytes([{1: 0xCC, 2: 0xCD, 4: 0xCE, 8: 0xCF}[w]]) + bytes(rng.choice(marks) for _ in range(w)))
        kind = rng.randrange(3)
        if kind == 1:
            items[rng.randrange(n)] = rng.choice(T.NON_NATIVE)
        data, first, _ = T.array_message(items)
        limit = rng.randrange(first + 1, len(data) + 1) if kind == 2 else len(data)
        count, end, table = T.walk(data, first, n, limit)
        rc, res, ck = T.host_tokenize(lib, data[:limit], 0, first, n, rng.randrange(4))
        assert rc == 0 and res == [count, end], (n, kind, limit, res, count, end)
        if count == n:
            assert ck == table


# ---- fbm_wire_scan_deferred ------------------------------------------------------------------------------
def _plain(lib, data, min_items=1):
    from fedbiomed_amd import _native as N

    buf = np.frombuffer(data, dtype=np.uint8)
    arrays, ckpt = (N.WireArray * 64)(), np.zeros(len(data) + 16, dtype=np.uint64)
    na, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.fbm_wire_scan(buf.ctypes.data, buf.size, min_items, ctypes.addressof(arrays), 64, ctypes.addressof(na),
                           ckpt.ctypes.data, ckpt.size, ctypes.addressof(nc))
    return rc, bytes(arrays)[:na.value * ctypes.sizeof(N.WireArray)], ckpt[:nc.value].tolist(), list(arrays[:na.value])


def _deferred(lib, data, defer_items, resolved, min_items=1):
    from fedbiomed_amd import _native as N

    buf = np.frombuffer(data, dtype=np.uint8)
    arrays, ckpt = (N.WireArray * 64)(), np.zeros(len(data) + 16, dtype=np.uint64)
    na, nc, pend = ctypes.c_uint64(0), ctypes.c_uint64(0), N.WirePending()
    res = np.array(resolved, dtype=np.uint64)
    rc = lib.fbm_wire_scan_deferred(buf.ctypes.data, buf.size, min_items, defer_items, res.ctypes.data if res.size else None,
                                    res.size, ctypes.addressof(arrays), 64, ctypes.addressof(na), ckpt.ctypes.data, ckpt.size,
                                    ctypes.addressof(nc), ctypes.addressof(pend))
    return rc, bytes(arrays)[:na.value * ctypes.sizeof(N.WireArray)], ckpt[:nc.value].tolist(), list(arrays[:na.value]), pend


def _two_arrays():
    a1, _ = F.lom_array(300, 1)
    a2, _ = F.lom_array(129, 6)
    small = U.packb([1, 2, 3])
    return b"\x84" + U.packb("a") + a1 + U.packb("s") + small + U.packb("b") + a2 + U.packb("round") + U.packb(3)


SCAN_MESSAGES = [(c[0], c[1]) for c in WHOLE if len(c[1]) < 100_000] + [("two-arrays", _two_arrays())]


@pytest.mark.parametrize("case", SCAN_MESSAGES, ids=[c[0] for c in SCAN_MESSAGES])
def test_deferred_scan_driven_by_the_plain_scan(lib, case):
    from fedbiomed_amd import _native as N

    _, data = case
    rc, raw, ckpt, arrays = _plain(lib, data)
    assert rc == 0 and arrays
    ends = {a.begin: a for a in arrays}
    resolved = []
    for _ in range(10):
        rc2, _, ck2, got, pend = _deferred(lib, data, 100, resolved)
        if rc2 != N.WIRE_PENDING:
            break
        assert (got, ck2) == ([], [])  # nothing recorded while an array is pending
        want = ends[pend.begin]
        assert pend.n_items == want.n_items >= 100 and data[pend.begin:pend.first] == T.header(want.n_items)
        resolved.append(want.end)
    assert rc2 == 0 and len(resolved) == sum(a.n_items >= 100 for a in arrays)
    assert [(a.begin, a.end, a.n_items, a.scheme) for a in got] == [(a.begin, a.end, a.n_items, a.scheme) for a in arrays]
    for a, g in zip(arrays, got):
        if a.n_items >= 100:
            assert (g.ckpt_count, g.pad) == (0, 1)
        else:
            assert g.pad == 0 and ck2[g.ckpt_first:g.ckpt_first + g.ckpt_count] == ckpt[a.ckpt_first:a.ckpt_first + a.ckpt_count]
    # every candidate answered with 0 (walk it on the host), and no deferral at all: fbm_wire_scan word for word
    assert _deferred(lib, data, 100, [0] * 8)[:3] == (0, raw, ckpt)
    assert _deferred(lib, data, 0, [])[:3] == (0, raw, ckpt)
    assert _deferred(lib, data, 10**9, [])[:3] == (0, raw, ckpt)


def test_deferred_scan_refuses_a_wrong_end_and_checks_arguments(lib):
    from fedbiomed_amd import _native as N

    data, first, n = T.array_message(T.pool_items(200))
    _, _, _, (a,) = _plain(lib, data)
    rc, *_, pend = _deferred(lib, data, 100, [])
    assert rc == N.WIRE_PENDING and (pend.begin, pend.first, pend.n_items) == (a.begin, first, n)
    for end in (first, first - 1, 1, len(data) + 1, 2**63):
        assert _deferred(lib, data, 100, [end])[0] == N.FBM_E_ARG, end
    assert _deferred(lib, data, 100, [len(data)])[0] == N.FBM_E_UNSUPPORTED  # inside, but the message does not end there
    assert _deferred(lib, data, 100, [a.end])[0] == 0
    # an array that claims more items than the message has bytes is no candidate
    assert _deferred(lib, b"\xdd\xff\xff\xff\xff\x01\x02", 1, [])[0] == N.FBM_E_UNSUPPORTED
    # a ninth candidate is walked on the host
    nine = b"\x99" + b"".join(F.lom_array(100, k)[0] for k in range(9))
    rc, _, _, arrays9 = _plain(lib, nine)
    assert rc == 0 and len(arrays9) == 9
    rc, _, ck, got, _ = _deferred(lib, nine, 100, [x.end for x in arrays9[:8]])
    assert rc == 0 and [g.pad for g in got] == [1] * 8 + [0] and got[8].ckpt_count == 2 and len(ck) == 2
    buf = np.frombuffer(data, dtype=np.uint8)
    one, pa, pc, pend = (N.WireArray * 1)(), ctypes.c_uint64(0), ctypes.c_uint64(0), N.WirePending()
    ck1 = np.zeros(8, dtype=np.uint64)
    args = [buf.ctypes.data, buf.size, 1, 100, None, 0, ctypes.addressof(one), 1, ctypes.addressof(pa), ck1.ctypes.data, 8,
            ctypes.addressof(pc), ctypes.addressof(pend)]
    assert lib.fbm_wire_scan_deferred(*args) == N.WIRE_PENDING
    for null in (0, 6, 8, 9, 11, 12):
        bad = list(args)
        bad[null] = None
        assert lib.fbm_wire_scan_deferred(*bad) == N.FBM_E_ARG, null
    bad = list(args)
    bad[5] = 1  # one resolved entry, no pointer
    assert lib.fbm_wire_scan_deferred(*bad) == N.FBM_E_ARG


def test_tokenizer_argument_errors(lib):
    from fedbiomed_amd import _native as N

    data, first, n = T.array_message(T.pool_items(130))
    buf = T.placed(data, first, 0)
    ck, res = np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_tokenize_workspace(len(data))) // 8 + 1, dtype=np.uint64)
    good = [buf.ctypes.data, len(data), 0, first, n, ck.ctypes.data, 3, res.ctypes.data, ws.ctypes.data]
    for fn, extra in ((lib.fbm_test_wire_tokenize_lom, []), (N.load().fbm_wire_tokenize_lom, [None])):
        E, host = N.FBM_E_ARG, not extra

        def call(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return fn(*a, *extra)

        if host:
            assert call() == 0 and res[0] == n
        for null in (0, 5, 7, 8):
            assert call(**{f"a{null}": None}) == E, null
        assert call(a6=2) == E and call(a6=4) == E                    # n_ckpt != ceil(n / 64)
        assert call(a5=ck.ctypes.data + 4) == E and call(a7=res.ctypes.data + 4) == E and call(a8=ws.ctypes.data + 2) == E
        assert call(a3=len(data)) == E and call(a2=first + 1) == E    # first past the span / before it
        assert call(a4=0, a6=7) == 0                                  # n_items == 0: nothing runs
        assert call(a4=2**32, a6=2**26) == N.FBM_E_UNSUPPORTED
        assert call(a1=2**50) == N.FBM_E_UNSUPPORTED                  # more workgroups than one launch's grid
    assert lib.fbm_wire_tokenize_workspace(0) > 0 and lib.fbm_wire_tokenize_workspace(10**6) >= (10**6 // T.TILE) * 48

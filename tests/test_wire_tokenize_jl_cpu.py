"""The device tokenizer for arrays of big-int maps and the deferring host scanner without a GPU:
fbm_test_wire_tokenize_jl runs the kernels' three passes tile by tile over host buffers (the same `__host__ __device__`
routines), and fbm_wire_scan_deferred2 is plain C++.  Expected tables are fbm_wire_scan's, expected counts and ends a
plain Python walk's (tests/wire_tokenize_jl_util.py).

Shapes.  The implementation's boundaries are the 4096-byte tile, the 280 entry offsets of a tile's map and the scan's
run of ceil(tiles / 256) tiles per thread.  The first tile boundary is crossed by a header at each of its splits (head
0: the boundary falls exactly TILE bytes behind item 0) and at the other three heads; the run boundary needs more
than 256 tiles, a message just over 1 MiB; everything else is a few dozen items."""
import ctypes

import numpy as np
import pytest

from tests import wire_fold_util as F
from tests import wire_reference_util as U
from tests import wire_tokenize_jl_util as J
from tests.wire_tokenize_util import placed


@pytest.fixture(scope="module")
def lib():
    from fedbiomed_amd import _build, _native

    _build.build()
    return _native.load_test()


WHOLE = J.whole_cases()
REFUSED = J.refused_cases()


def test_entry_points_are_declared(lib):
    from fedbiomed_amd import _native as N

    for name in ("fbm_wire_tokenize_jl_workspace", "fbm_wire_tokenize_jl", "fbm_wire_scan_deferred2"):
        assert name in N.SIGNATURES and hasattr(N.load(), name)
    assert "fbm_test_wire_tokenize_jl" in N.TEST_SIGNATURES and hasattr(lib, "fbm_test_wire_tokenize_jl")
    assert lib.fbm_abi_version() == 7 and ctypes.sizeof(N.WirePending2) == 32


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_table_count_and_end_equal_the_scanner(lib, case):
    name, data, first, n = case
    b, e, n_scan, scheme, table = J.scan_one(data)
    assert (n_scan, scheme) == (n, "jl") and J.walk(data, first, n) == (n, e, table)
    if name == "runs-258-tiles":
        assert (e - first) // J.TILE >= 258
    heads = (0, 1, 2, 3) if len(data) < 100_000 else (0, 3)
    for head in heads:
        for base in (0, b):  # the whole message as the span, and the message from the array's header on
            rc, res, ck = J.host_tokenize(lib, data[base:], base, first, n, head)
            assert rc == 0 and res == [n, e] and ck == table, (head, base, res, e)
    rc, res, ck = J.host_tokenize(lib, data[b:e], b, first, n)  # the array's own span: nothing behind item n - 1
    assert rc == 0 and res == [n, e] and ck == table


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_counting_stops_at_what_is_no_map_item(lib, case):
    _, data, first, n, want = case
    assert J.walk(data, first, n)[0] == want
    for head in (0, 1, 2, 3):
        rc, res, _ = J.host_tokenize(lib, data, 0, first, n, head)
        assert rc == 0 and res == [want, 0], (head, res)


def test_refusal_behind_a_tile_boundary(lib):
    """The chain dies in the second tile: the items of the first one count."""
    for name, bad in J.bad_items():
        items = J.filling(J.TILE + 100)
        data, first, n = J.message(items + [bad] + J.filling(300), n=len(items) + 3)
        rc, res, _ = J.host_tokenize(lib, data, 0, first, n)
        assert J.walk(data, first, n)[0] == len(items) and rc == 0 and res == [len(items), 0], name


def test_span_cut_inside_the_last_item(lib):
    for n, last in ((1, J.item(257)), (30, J.item(257)), (30, J.item(9, "c4")), (16, J.item(255, "c5"))):
        items = [J.item(*J.CLASSES[i % 7], fill=i) for i in range(n - 1)] + [last]
        data, first, _ = J.message(items)
        end = J.scan_one(data)[1]
        start = end - len(last)
        cuts = list(range(start, start + 24)) + [end - len(last) // 2, end - 1]  # every cut in the header, two in the value
        for cut in cuts:
            assert J.walk(data, first, n, cut)[0] == n - 1
            if cut <= first:  # (n == 1: item 0 itself lies outside such a span, an argument error)
                continue
            for head in (0, 3):
                rc, res, _ = J.host_tokenize(lib, data[:cut], 0, first, n, head)
                assert rc == 0 and res == [n - 1, 0], (n, cut, head, res)


def test_items_behind_the_array_are_not_counted(lib):
    items = [J.item(*J.CLASSES[i % 7], fill=i) for i in range(45)]
    tail = J.item(257) + J.item(3) + b"\x05"  # the next values of the message are accepted items themselves
    data, first, n = J.message(items, tail)
    count, end, table = J.walk(data, first, n)
    assert count == n and data[end:] == tail
    for head in (0, 1, 2, 3):
        rc, res, ck = J.host_tokenize(lib, data, 0, first, n, head)  # (the guards behind ck[n - 1] stand)
        assert rc == 0 and res == [n, end] and ck == table
    for fewer in (1, 17, 44):  # fewer items asked for than the array holds: capped, the end is item n' - 1's
        count, end, table = J.walk(data, first, fewer)
        rc, res, ck = J.host_tokenize(lib, data, 0, first, fewer)
        assert rc == 0 and res == [fewer, end] and ck == table


def test_first_at_every_residue_behind_poisoned_bytes(lib):
    """Tokenizing from item 1: the bytes in front of `first` are item 0's last value bytes, here the prefix's own."""
    poison = J.item(40, value=b"\x01" + b"\x11" * 19 + J.PREFIX)
    for pad in range(4):  # item 1 at every offset residue of the message as well
        items = [J.item(1 + pad), poison] + [J.item(*J.CLASSES[i % 7], fill=i) for i in range(30)]
        data, first, n = J.message(items)
        f1 = first + len(items[0]) + len(poison)
        want = J.walk(data, f1, n - 2)
        assert want[0] == n - 2 and data[f1 - 20:f1] == J.PREFIX
        for head in (0, 1, 2, 3):
            rc, res, ck = J.host_tokenize(lib, data, 0, f1, n - 2, head)
            assert rc == 0 and (res[0], res[1], ck) == want, (pad, head)
            rc, res, ck = J.host_tokenize(lib, data[f1 - 3:], f1 - 3, f1, n - 2, head)  # three poisoned bytes, no more
            assert rc == 0 and (res[0], res[1], ck) == want, (pad, head)
            rc, res, ck = J.host_tokenize(lib, data[f1:], f1, f1, n - 2, head)  # none: nothing in front is read
            assert rc == 0 and (res[0], res[1], ck) == want, (pad, head)


def test_random_arrays_against_the_walk(lib):
    """Seeded: items of random sizes whose values are full of marker bytes, a bad item or a cut at a random place."""
    import random

    rng = random.Random(11)
    marks = [0x82, 0xA8, 0xC4, 0xC5, 0x00, 0x01, 0x7F, 0x5F]
    bad = [b for _, b in J.bad_items()]
    for _ in range(150):
        n = rng.choice([1, 2, 15, 16, 40, 200])
        items = []
        for _ in range(n):
            L = rng.choice([1, 2, 22, 23, 255, 256, 257, rng.randrange(1, 258)])
            value = bytes([0 if L == 257 else rng.randrange(128)]) + bytes(rng.choice(marks) for _ in range(L - 1))
            items.append(J.item(L, "c5" if L > 255 or rng.random() < 0.2 else "c4", value=value))
        kind = rng.randrange(3)
        if kind == 1:
            items[rng.randrange(n)] = rng.choice(bad)
        data, first, _ = J.message(items)
        limit = rng.randrange(first + 1, len(data) + 1) if kind == 2 else len(data)
        count, end, table = J.walk(data, first, n, limit)
        rc, res, ck = J.host_tokenize(lib, data[:limit], 0, first, n, rng.randrange(4))
        assert rc == 0 and res == [count, end], (n, kind, limit, res, count, end)
        if count == n:
            assert ck == table


# ---- fbm_wire_scan_deferred2 -----------------------------------------------------------------------------
def _plain(lib, data, min_items=1):
    from fedbiomed_amd import _native as N

    buf = np.frombuffer(data, dtype=np.uint8)
    arrays, ckpt = (N.WireArray * 64)(), np.zeros(len(data) + 16, dtype=np.uint64)
    na, nc = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rc = lib.fbm_wire_scan(buf.ctypes.data, buf.size, min_items, ctypes.addressof(arrays), 64, ctypes.addressof(na),
                           ckpt.ctypes.data, ckpt.size, ctypes.addressof(nc))
    return rc, bytes(arrays)[:na.value * ctypes.sizeof(N.WireArray)], ckpt[:nc.value].tolist(), list(arrays[:na.value])


def _deferred2(lib, data, defer_lom, defer_jl, resolved, min_items=1):
    from fedbiomed_amd import _native as N

    buf = np.frombuffer(data, dtype=np.uint8)
    arrays, ckpt = (N.WireArray * 64)(), np.zeros(len(data) + 16, dtype=np.uint64)
    na, nc, pend = ctypes.c_uint64(0), ctypes.c_uint64(0), N.WirePending2()
    res = np.array(resolved, dtype=np.uint64)
    rc = lib.fbm_wire_scan_deferred2(buf.ctypes.data, buf.size, min_items, defer_lom, defer_jl,
                                     res.ctypes.data if res.size else None, res.size, ctypes.addressof(arrays), 64,
                                     ctypes.addressof(na), ckpt.ctypes.data, ckpt.size, ctypes.addressof(nc),
                                     ctypes.addressof(pend))
    return rc, bytes(arrays)[:na.value * ctypes.sizeof(N.WireArray)], ckpt[:nc.value].tolist(), list(arrays[:na.value]), pend


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


def _jl_array(n, seed=0):
    return J.header(n) + b"".join(J.item(*J.CLASSES[(i + seed) % 7], fill=(i * 3 + seed) % 256) for i in range(n))


def _jl_and_lom():
    lom, _ = F.lom_array(300, 1)
    return (b"\x84" + U.packb("a") + _jl_array(120) + U.packb("s") + U.packb([1, 2, 3]) + U.packb("b") + lom +
            U.packb("c") + _jl_array(101, 3))


def test_deferred2_pending_carries_the_scheme_and_slots_go_in_order(lib):
    from fedbiomed_amd import _native as N

    data = _jl_and_lom()
    rc, raw, ckpt, arrays = _plain(lib, data)
    assert rc == 0 and [(a.n_items, a.scheme) for a in arrays] == [(120, N.WIRE_JL), (3, N.WIRE_LOM), (300, N.WIRE_LOM),
                                                                   (101, N.WIRE_JL)]
    big = [a for a in arrays if a.n_items >= 100]
    resolved = []
    for a in big:
        rc2, _, ck2, got, pend = _deferred2(lib, data, 100, 100, resolved)
        assert rc2 == N.WIRE_PENDING and (got, ck2) == ([], [])
        assert (pend.begin, pend.n_items, pend.scheme, pend.pad) == (a.begin, a.n_items, a.scheme, 0)
        assert data[pend.begin:pend.first] == J.header(a.n_items)
        resolved.append(a.end)
    rc2, _, ck2, got, _ = _deferred2(lib, data, 100, 100, resolved)
    assert rc2 == 0
    assert [(g.begin, g.end, g.n_items, g.scheme) for g in got] == [(a.begin, a.end, a.n_items, a.scheme) for a in arrays]
    assert [(g.ckpt_count, g.pad) for g in got] == [(0, 1), (1, 0), (0, 1), (0, 1)] and ck2 == [arrays[1].begin + 1]
    # resolved = 0 everywhere: fbm_wire_scan's arrays and table exactly; so is a threshold no array reaches
    assert _deferred2(lib, data, 100, 100, [0] * 8)[:3] == (0, raw, ckpt)
    assert _deferred2(lib, data, 10**9, 10**9, [])[:3] == (0, raw, ckpt)
    assert _deferred2(lib, data, 0, 0, [])[:3] == (0, raw, ckpt)
    # the JL threshold alone: the LOM array is walked on the host, the two JL arrays take slots 0 and 1
    rc2, _, _, got, _ = _deferred2(lib, data, 0, 100, [big[0].end, big[2].end])
    assert rc2 == 0 and [g.pad for g in got] == [1, 0, 0, 1] and got[2].ckpt_count == 5
    # a wrong end, and one that is inside the message but not the array's
    for end in (big[0].begin, arrays[0].begin + len(J.header(120)), len(data) + 1, 2**63):
        assert _deferred2(lib, data, 0, 100, [end])[0] == N.FBM_E_ARG, end
    assert _deferred2(lib, data, 0, 100, [big[0].end - 1])[0] == N.FBM_E_UNSUPPORTED


def test_deferred2_candidates(lib):
    from fedbiomed_amd import _native as N

    # a first item that is native, one with a wrong prefix byte and a bin32 are no JL candidates: walked as always
    for first_item in (b"\x05", bytes(J.bad_items()[5][1]), J.bad_items()[4][1]):
        data = J.header(50) + first_item + b"".join(J.item(9) for _ in range(49))
        assert _deferred2(lib, data, 0, 10, [])[:3] == _plain(lib, data)[:3]
    # a header that claims more 23-byte items than bytes are left is none either: no table is sized by it
    lying = b"\xdd\x00\x0f\xff\xff" + J.item(9) * 3
    assert _deferred2(lib, lying, 0, 1, [])[0] == N.FBM_E_UNSUPPORTED
    exact = J.header(3) + J.item(1) * 3  # 23 n bytes exactly: a candidate
    assert _deferred2(lib, exact, 0, 1, [])[0] == N.WIRE_PENDING
    assert _deferred2(lib, exact[:-1], 0, 1, [])[0] == N.FBM_E_UNSUPPORTED  # one byte less: not one, and truncated
    # min_items bounds the candidates as it bounds the recorded arrays
    assert _deferred2(lib, exact, 0, 1, [], min_items=4)[:3] == _plain(lib, exact, 4)[:3]
    # the ninth candidate is walked on the host
    nine = b"\x99" + b"".join(_jl_array(20, k) for k in range(9))
    rc, _, _, arrays9 = _plain(lib, nine)
    assert rc == 0 and len(arrays9) == 9
    rc, _, ck, got, _ = _deferred2(lib, nine, 0, 20, [x.end for x in arrays9[:8]])
    assert rc == 0 and [g.pad for g in got] == [1] * 8 + [0] and got[8].ckpt_count == 20 and len(ck) == 20
    # null pointers
    data = _jl_and_lom()
    buf = np.frombuffer(data, dtype=np.uint8)
    one, pa, pc, pend = (N.WireArray * 4)(), ctypes.c_uint64(0), ctypes.c_uint64(0), N.WirePending2()
    ck1 = np.zeros(400, dtype=np.uint64)
    args = [buf.ctypes.data, buf.size, 1, 0, 100, None, 0, ctypes.addressof(one), 4, ctypes.addressof(pa), ck1.ctypes.data, 400,
            ctypes.addressof(pc), ctypes.addressof(pend)]
    assert lib.fbm_wire_scan_deferred2(*args) == N.WIRE_PENDING and pend.scheme == N.WIRE_JL
    for null in (0, 7, 9, 10, 12, 13):
        bad = list(args)
        bad[null] = None
        assert lib.fbm_wire_scan_deferred2(*bad) == N.FBM_E_ARG, null
    bad = list(args)
    bad[6] = 1  # one resolved entry, no pointer
    assert lib.fbm_wire_scan_deferred2(*bad) == N.FBM_E_ARG


def test_deferred2_without_a_jl_threshold_is_the_old_entry_point(lib):
    from fedbiomed_amd import _native as N
    from tests import wire_tokenize_util as T

    lom_cases = [c[1] for c in T.whole_cases() if len(c[1]) < 100_000][:6]
    for data in lom_cases + [_jl_and_lom(), WHOLE[7][1], b"\x91\xc1", b""]:
        for defer, resolved in ((100, []), (1, []), (100, [0]), (100, [0] * 8), (0, []), (100, [5]), (100, [len(data)])):
            old = _deferred(lib, data, defer, resolved)
            new = _deferred2(lib, data, defer, 0, resolved)
            assert old[:3] == new[:3], (len(data), defer, resolved)
            if old[0] == N.WIRE_PENDING:
                assert (old[4].begin, old[4].first, old[4].n_items) == (new[4].begin, new[4].first, new[4].n_items)
                assert new[4].scheme == N.WIRE_LOM
        _, _, _, arrays = _plain(lib, data)
        ends = [a.end for a in arrays if a.n_items >= 100 and a.scheme == N.WIRE_LOM]
        if ends:
            assert _deferred(lib, data, 100, ends)[:3] == _deferred2(lib, data, 100, 0, ends)[:3]


def test_tokenizer_argument_errors(lib):
    from fedbiomed_amd import _native as N

    data, first, n = J.message([J.item(*J.CLASSES[i % 7]) for i in range(20)])
    want = J.walk(data, first, n)
    buf = placed(data, first, 0)
    ck, res = np.zeros(n + 4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
    ws = np.zeros(int(lib.fbm_wire_tokenize_jl_workspace(len(data))) // 8 + 1, dtype=np.uint64)
    good = [buf.ctypes.data, len(data), 0, first, n, ck.ctypes.data, n, res.ctypes.data, ws.ctypes.data]
    for fn, extra in ((lib.fbm_test_wire_tokenize_jl, []), (N.load().fbm_wire_tokenize_jl, [None])):
        E, host = N.FBM_E_ARG, not extra

        def call(**kw):
            a = list(good)
            for k, v in kw.items():
                a[int(k[1:])] = v
            return fn(*a, *extra)

        for null in (0, 5, 7, 8):
            assert call(**{f"a{null}": None}) == E, null
        assert call(a6=n - 1) == E and call(a6=n + 1) == E and call(a6=1) == E  # n_ckpt != n_items
        assert call(a5=ck.ctypes.data + 4) == E and call(a7=res.ctypes.data + 4) == E and call(a8=ws.ctypes.data + 2) == E
        assert call(a3=len(data)) == E and call(a2=first + 1) == E     # first past the span / before it
        assert call(a4=0, a6=7) == 0                                   # n_items == 0: nothing runs
        assert call(a4=2**32, a6=2**32) == N.FBM_E_UNSUPPORTED
        assert call(a1=2**50) == N.FBM_E_UNSUPPORTED                   # more workgroups than one launch's grid
        if host:  # the library computes right after every refusal
            res[:] = 0
            assert call() == 0 and (int(res[0]), int(res[1]), ck[:n].tolist()) == want
    assert lib.fbm_wire_tokenize_jl_workspace(0) > 0 and lib.fbm_wire_tokenize_jl_workspace(10**6) >= (10**6 // J.TILE) * 72

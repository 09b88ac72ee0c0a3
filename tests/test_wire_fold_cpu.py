"""fbm_wire_fold_lom without a GPU: the kernel's per-item routine joined to the accumulate on the host
(fbm_test_wire_fold_lom -> host_wire_fold_lom), over the scanner's own tables and over foreign ones, the entry
point's argument errors, and `wire.ResidentUpdate` with the container's device call replaced by the library's host
run.  Bytes come from msgpack under the reference's rules (tests/wire_fold_util.py), tables from fbm_wire_scan,
expected sums from Python integers -- never from the code under test."""
import ctypes

import msgpack
import numpy as np
import pytest

from fedbiomed_amd import _native as N
from fedbiomed_amd import wire
from tests import wire_fold_util as F
from tests import wire_reference_util as U


@pytest.fixture(scope="module")
def libs():
    from fedbiomed_amd import _build

    _build.build()
    return N.load(), N.load_test()


def _scan(data, min_items=1):
    from fedbiomed_amd import _device as D

    return D.wire_scan(data, min_items)


def _exact(a: np.ndarray) -> np.ndarray:
    """A copy allocated at exactly the array's length (a read or write outside it leaves the allocation)."""
    out = np.empty(a.shape, dtype=a.dtype)
    out[...] = a
    return out


def host_fold(lib, span, span_len, base, ck, n, acc, first, n_ckpt=None):
    span, ck = _exact(np.frombuffer(span, dtype=np.uint8)), _exact(np.asarray(ck, dtype=np.uint64))
    acc = _exact(F.u64(acc))
    rc = lib.fbm_test_wire_fold_lom(span.ctypes.data, span_len, base, ck.ctypes.data, ck.size if n_ckpt is None else n_ckpt,
                                    n, acc.ctypes.data, 1 if first else 0)
    return rc, acc.tolist()


def _one_array(n, off):
    """The array inside a message, scanned: (message, (begin, end, n, scheme, table), values)."""
    arr, vals = F.lom_array(n, off)
    data, at = F.message(arr)
    arrays = _scan(data)
    assert arrays is not None and len(arrays) == 1
    a = arrays[0]
    assert (a[0], a[1], a[2], a[3]) == (at, at + len(arr), n, "lom") and at > 0
    assert a[4].size == -(-n // N.WIRE_LOM_GROUP)
    assert msgpack.unpackb(data, strict_map_key=False)["params"] == vals
    return data, a, vals


# ---- the scanner's tables ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.NS)
def test_fold_equals_python_sum(libs, n):
    _, test = libs
    pool = len(F.item_pool())
    for off in (range(pool) if n == 1 else (0, 5)):  # (n = 1: every form on its own)
        data, (b, e, _, _, ck), vals = _one_array(n, off)
        acc0 = F.acc_values(n)
        for first in (True, False):
            rc, got = host_fold(test, data[b:e], e - b, b, ck, n, acc0, first)  # span_base = b > 0
            assert rc == N.FBM_OK, N.last_error()
            assert got == F.folded(acc0, vals, first), (n, off, first)
        # a span that is more than the array's own: the whole message, base 0
        rc, got = host_fold(test, data, len(data), 0, ck, n, acc0, False)
        assert rc == N.FBM_OK and got == F.folded(acc0, vals, False)


def test_every_form_is_in_the_largest_case():
    _, vals = F.lom_array(1025)
    assert set(U.NATIVE_EDGES) <= set(vals)
    arr, _ = F.lom_array(1025)
    for raw, _ in F.NON_MINIMAL:
        assert raw in arr


def test_wrap_around(libs):
    _, test = libs
    vals = [1, F.M64 - 1, 0, 5]
    data, at = F.message(U.packb(vals))
    (b, e, n, _, ck), = _scan(data)
    rc, got = host_fold(test, data[b:e], e - b, b, ck, n, [F.M64 - 1] * 4, False)
    assert rc == N.FBM_OK and got == [0, F.M64 - 2, F.M64 - 1, 4]
    rc, got = host_fold(test, data[b:e], e - b, b, ck, n, [F.M64 - 1] * 4, True)
    assert rc == N.FBM_OK and got == vals


def test_two_folds_continue(libs):
    _, test = libs
    n = 129
    acc, total = [0xA5A5A5A5A5A5A5A5] * n, [0] * n
    for k, off in enumerate((0, 3, 9)):
        data, (b, e, _, _, ck), vals = _one_array(n, off)
        rc, acc = host_fold(test, data[b:e], e - b, b, ck, n, acc, k == 0)
        assert rc == N.FBM_OK
        total = [(t + v) % F.M64 for t, v in zip(total, vals)]
    assert acc == total


# ---- tables that are not the scanner's --------------------------------------------------------------------
def test_foreign_tables_give_zero(libs):
    """A checkpoint before the span, one past it, in its last 3 bytes, or far away yields the value 0: the
    accumulator keeps its value when continuing and becomes 0 on a first call.  Buffers are exactly sized."""
    _, test = libs
    n = 256
    vals = F.minimal_values(n - 1) + [F.M64 - 1]  # the last item: cf ff .. ff, so its last 3 bytes start no item
    data, at = F.message(U.packb(vals))
    (b, e, _, _, ck), = _scan(data)
    assert data[e - 9:e] == b"\xcf" + b"\xff" * 8 and ck.size == 4
    acc0 = F.acc_values(n)
    zero = [0] * 64
    for bad in (b - 1, 0, e, e + 1, 2**63, F.M64 - 1, e - 3, e - 2, e - 1):
        for slot in range(4):
            t = ck.copy()
            t[slot] = bad
            want_vals = list(vals)
            want_vals[64 * slot:64 * slot + 64] = zero
            for first in (True, False):
                rc, got = host_fold(test, data[b:e], e - b, b, t, n, acc0, first)
                assert rc == N.FBM_OK and got == F.folded(acc0, want_vals, first), (bad, slot, first)
    # a valid offset in another group's slot decodes that group's items there
    t = ck.copy()
    t[1], t[2] = ck[0], ck[3]
    rc, got = host_fold(test, data[b:e], e - b, b, t, n, acc0, False)
    assert rc == N.FBM_OK and got == F.folded(acc0, vals[:64] + vals[:64] + vals[192:] + vals[192:], False)
    # a span cut inside the last item: that item counts as 0, the items before it stand
    rc, got = host_fold(test, data[b:e - 4], e - b - 4, b, ck, n, acc0, False)
    assert rc == N.FBM_OK and got == F.folded(acc0, vals[:-1] + [0], False)
    # a table of zeros under a nonzero base: every group outside the span
    rc, got = host_fold(test, data[b:e], e - b, b, np.zeros(4, np.uint64), n, acc0, True)
    assert rc == N.FBM_OK and got == [0] * n


# ---- argument errors ------------------------------------------------------------------------------------
def test_argument_errors_and_a_correct_call_after_each(libs):
    """Every refusal returns its documented code before anything runs (on a machine without a GPU a device call
    of the product library would be FBM_E_HIP), and the next correct call succeeds."""
    prod, test = libs
    data, (b, e, n, _, ck), vals = _one_array(129, 0)
    span = _exact(np.frombuffer(data[b:e], dtype=np.uint8))
    ck = _exact(ck.astype(np.uint64))
    acc = np.zeros(n + 1, dtype=np.uint64)
    sp, cp, ap = span.ctypes.data, ck.ctypes.data, acc.ctypes.data

    def good():
        rc = test.fbm_test_wire_fold_lom(sp, e - b, b, cp, ck.size, n, ap, 1)
        assert rc == N.FBM_OK and acc[:n].tolist() == vals and acc[n] == 0

    good()
    E, S = N.FBM_E_ARG, N.FBM_E_UNSUPPORTED
    big = 64 * 4 * 0x80000000  # one workgroup more than a launch's grid holds
    cases = [((None, e - b, b, cp, ck.size, n, ap, 0), E, "null"),
             ((sp, e - b, b, None, ck.size, n, ap, 0), E, "null"),
             ((sp, e - b, b, cp, ck.size, n, None, 0), E, "null"),
             ((sp, e - b, b, cp, ck.size - 1, n, ap, 0), E, "checkpoints"),
             ((sp, e - b, b, cp, ck.size + 1, n, ap, 0), E, "checkpoints"),
             ((sp, e - b, b, cp, ck.size, 128, ap, 0), E, "checkpoints"),
             ((sp, e - b, b, cp, ck.size, n, ap + 4, 0), E, "aligned"),
             ((sp, e - b, b, cp + 4, ck.size, n, ap, 0), E, "aligned"),
             ((sp, e - b, b, cp, big // 64, big, ap, 0), S, "grid")]
    err = lambda lib: (lib.fbm_last_error() or b"").decode()  # noqa: E731 -- each build keeps its own message
    for args, code, word in cases:
        assert test.fbm_test_wire_fold_lom(*args) == code and word in err(test), (args, err(test))
        good()
        assert prod.fbm_wire_fold_lom(*args, None) == code and word in err(prod), (args, err(prod))
    # nothing to do: FBM_OK whatever the pointers
    assert prod.fbm_wire_fold_lom(None, 0, 0, None, 0, 0, None, 1, None) == N.FBM_OK
    assert test.fbm_test_wire_fold_lom(None, 0, 0, None, 0, 0, None, 0) == N.FBM_OK
    good()


def test_declared_bound_and_exported(libs):
    import os
    import re

    prod, test = libs
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    h = open(os.path.join(root, "include", "fbm_secagg.h")).read()
    th = open(os.path.join(root, "include", "fbm_secagg_test.h")).read()
    assert re.search(r"^int fbm_wire_fold_lom\(", h, re.M) and re.search(r"^int fbm_test_wire_fold_lom\(", th, re.M)
    assert re.search(r"^#define FBM_ABI_VERSION 7\b", h, re.M) and prod.fbm_abi_version() == 7
    c_vp, c_int, c_u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert N.SIGNATURES["fbm_wire_fold_lom"] == (c_int, [c_vp, c_u64, c_u64, c_vp, c_u64, c_u64, c_vp, c_int, c_vp])
    assert N.TEST_SIGNATURES["fbm_test_wire_fold_lom"] == (c_int, [c_vp, c_u64, c_u64, c_vp, c_u64, c_u64, c_vp, c_int])
    assert hasattr(prod, "fbm_wire_fold_lom") and hasattr(test, "fbm_wire_fold_lom")
    assert hasattr(test, "fbm_test_wire_fold_lom") and not hasattr(prod, "fbm_test_wire_fold_lom")


# ---- ResidentUpdate through the seam ------------------------------------------------------------------------
class HostHandle:
    """What `wire._upload_arrays` returns per array, on the library's host run: the message and the array's
    record stand in for the device block."""

    decodes = 0

    def __init__(self, data, array):
        self._data, self._array, self.released = data, array, False

    def rows_host(self):
        if self.released:
            raise RuntimeError("released")
        HostHandle.decodes += 1
        return U.host_decode(self._data, [self._array])[0]

    def release(self):
        self.released = True


@pytest.fixture()
def host_run(libs, monkeypatch):
    monkeypatch.setattr(wire, "_upload_arrays", lambda data, arrays: [HostHandle(data, a) for a in arrays])
    monkeypatch.setattr(wire, "_decode_arrays", U.host_decode)
    HostHandle.decodes = 0
    wire.reference_stats(reset=True)


def _reply():
    lom = F.minimal_values(300)
    jl = U.edge_values()
    return U.packb({"a": 1, "params": jl, "more": {"lom": lom, 7: [1, 2]}, "t": [1.5, "s"]}), jl, lom


def test_resident_update_is_lazy_and_equal(host_run):
    data, jl, lom = _reply()
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=4, resident=True)
    p, q = got["params"], got["more"]["lom"]
    assert type(p) is wire.ResidentUpdate and type(q) is wire.ResidentUpdate and not isinstance(p, list)
    assert (p.scheme, p.n_items, len(p)) == ("jl", len(jl), len(jl)) and (q.scheme, q.n_items, len(q)) == ("lom", 300, 300)
    assert type(got["more"][7]) is list and got["t"] == [1.5, "s"]  # below min_items: msgpack's
    assert not p.materialised and not q.materialised and HostHandle.decodes == 0
    st = wire.reference_stats()
    assert (st["resident"], st["fast"], st["fallback"]) == (2, 0, 0)
    assert q == lom and lom == q and q != lom[:-1] + [lom[-1] ^ 1]  # equality with the msgpack list, both ways
    assert q.materialised and not p.materialised and HostHandle.decodes == 1
    assert list(iter(p)) == jl and p.materialised and p[3] == jl[3] and p[-2:] == jl[-2:]
    assert q.tolist() is q.tolist() and all(type(v) is int for v in q.tolist())
    assert HostHandle.decodes == 2  # once per update: cached
    assert got == U.unpackb(data)  # the whole message compares as msgpack's
    with pytest.raises(TypeError):
        hash(q)


def test_release_then_use_raises(host_run):
    data, jl, lom = _reply()
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=4, resident=True)
    p, q = got["params"], got["more"]["lom"]
    assert q.tolist() == lom
    p.release()
    q.release()
    assert len(p) == len(jl) and not p.materialised
    with pytest.raises(RuntimeError):
        p.tolist()
    with pytest.raises(RuntimeError):
        p.handle
    with pytest.raises(RuntimeError):
        list(p)
    with pytest.raises(RuntimeError):
        q.handle
    assert q.tolist() == lom  # made before the release: still the list


def test_not_resident_is_unchanged(host_run):
    data, jl, lom = _reply()
    for kw in ({}, {"resident": False}):
        got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=4, **kw)
        p, q = got["params"], got["more"]["lom"]
        assert isinstance(p, wire.EncryptedParams) and isinstance(q, wire.EncryptedParams) and isinstance(p, list)
        assert p == jl and q == lom and p.consistent() and q.consistent()
    st = wire.reference_stats()
    assert (st["fast"], st["resident"], st["fallback"]) == (4, 0, 0) and HostHandle.decodes == 0


def test_resident_keeps_the_hook_rule_and_fallbacks(host_run):
    data, jl, lom = _reply()
    got = wire.loads_reference(data, min_items=4, resident=True)  # no hook: int maps stay msgpack's dicts
    assert type(got["params"]) is list and type(got["more"]["lom"]) is wire.ResidentUpdate
    assert got == msgpack.unpackb(data, strict_map_key=False)
    assert wire.reference_stats(reset=True)["resident"] == 1
    plain = U.packb({"a": [1.5] * 30})
    assert wire.loads_reference(plain, object_hook=U.ref_hook, min_items=4, resident=True) == U.unpackb(plain)
    st = wire.reference_stats()
    assert (st["resident"], st["fallback"]) == (0, 1)
    assert wire.reference_stats(reset=True)["fallback"] == 1 and wire.reference_stats()["resident"] == 0


def test_wrong_scheme_is_fb624(host_run):
    """(Raised before any device call: the scheme is checked first.)"""
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError
    from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

    data, jl, lom = _reply()
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=4, resident=True)
    p, q = got["params"], got["more"]["lom"]
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624"):
        SecaggLomCrypter(nonce="n").begin_aggregate(total_sample_size=3).add(p)
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624"):
        SecaggCrypter().begin_aggregate(1, 1, 5, 35, 3).add(q)
    assert not p.materialised and not q.materialised

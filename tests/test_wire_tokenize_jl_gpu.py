"""The big-int-map tokenizer on the GPU: fbm_wire_tokenize_jl (wire_tokj_maps_kernel, wire_tokj_scan_kernel,
wire_tokj_emit_kernel) against fbm_wire_scan's table and a plain Python walk on the inputs of
tests/test_wire_tokenize_jl_cpu.py, then `wire.loads_reference(resident=True, device_scan_jl_min_items=1)` -- refusals,
truncation, the counters, the object_hook probe -- and a Joye-Libert round end to end, bit for bit against `aggregate`
of the lists msgpack unpacks.

Shapes as in the CPU file (tests/wire_tokenize_jl_util.py): a header across the first tile boundary at each split,
decoys among a tile's entry offsets, and one array of more than 258 tiles (just over 1 MiB) for the scan's runs.  The
round is three parties of 70 ciphertexts, one reply a ciphertext short, a few ciphertexts replaced by shorter values
of every size class."""
import msgpack
import numpy as np
import pytest
import torch

from fedbiomed_amd import wire
from fedbiomed_amd import workload as W
from tests import wire_fold_util as F
from tests import wire_reference_util as U
from tests import wire_tokenize_jl_util as J

pytestmark = pytest.mark.gpu

WHOLE = J.whole_cases()
REFUSED = J.refused_cases()
OFF = 2**40  # a threshold no array reaches


@pytest.fixture(scope="module")
def dev():
    from fedbiomed_amd import _device as D

    return D.device()


@pytest.fixture(autouse=True)
def _fresh_stats():
    wire.reference_stats(reset=True)


def _bits(xs):
    return np.asarray(xs, dtype=np.float64).view(np.uint64).tolist()


@pytest.mark.parametrize("case", WHOLE, ids=[c[0] for c in WHOLE])
def test_kernel_table_count_and_end_equal_the_scanner(dev, case):
    _, data, first, n = case
    b, e, _, _, table = J.scan_one(data)
    assert J.walk(data, first, n) == (n, e, table)
    for head, base in ((0, 0), (3, 0), (1, b), (2, b)):
        rc, res, ck = J.device_tokenize(data[base:], base, first, n, head)
        assert rc == 0 and res == [n, e] and ck == table, (head, base, res, e)
    rc, res, ck = J.device_tokenize(data[b:e], b, first, n)  # the array's own span
    assert rc == 0 and res == [n, e] and ck == table


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_kernel_counting_stops_at_what_is_no_map_item(dev, case):
    _, data, first, n, want = case
    for head in (0, 1, 2, 3):
        rc, res, _ = J.device_tokenize(data, 0, first, n, head)
        assert rc == 0 and res == [want, 0], (head, res)


def test_kernel_span_cut_items_behind_and_poisoned_front(dev):
    last = J.item(257)
    items = [J.item(*J.CLASSES[i % 7], fill=i) for i in range(29)] + [last]
    data, first, n = J.message(items)
    end = J.scan_one(data)[1]
    start = end - len(last)
    for cut in list(range(start, start + 24)) + [end - 100, end - 1]:
        rc, res, _ = J.device_tokenize(data[:cut], 0, first, n, cut % 4)
        assert rc == 0 and res == [n - 1, 0], (cut, res)
    tail = J.item(257) + J.item(3) + b"\x05"
    data, first, n = J.message(items, tail)
    for ask in (n, 17, 1):
        count, end, table = J.walk(data, first, ask)
        rc, res, ck = J.device_tokenize(data, 0, first, ask, ask % 4)  # (the guard behind ck[ask - 1] stands)
        assert count == ask and rc == 0 and res == [ask, end] and ck == table, (ask, res)
    poison = J.item(40, value=b"\x01" + b"\x11" * 19 + J.PREFIX)
    data, first, n = J.message([J.item(2), poison] + items)
    f1 = first + len(J.item(2)) + len(poison)
    want = J.walk(data, f1, n - 2)
    for head in (0, 1, 2, 3):
        for base in (0, f1 - 3, f1):
            rc, res, ck = J.device_tokenize(data[base:], base, f1, n - 2, head)
            assert rc == 0 and (res[0], res[1], ck) == want, (head, base)


# ---- through loads_reference -----------------------------------------------------------------------------
def _both(data, hook=U.ref_hook):
    """The message read with the JL device scan forced on and with it disabled: (device route, host route)."""
    got = wire.loads_reference(data, object_hook=hook, min_items=1, resident=True, device_scan_jl_min_items=1)
    ref = wire.loads_reference(data, object_hook=hook, min_items=1, resident=True, device_scan_jl_min_items=OFF)
    return got, ref


def _cts(n, seed=0):
    return [(1 << 2040) + 977 * (k + seed) + (k << 700) for k in range(n)]


def test_loads_reference_counts_and_equals_the_host_route(dev):
    cts = _cts(70)
    cts[5], cts[9], cts[11] = 1 << 64, (1 << 2032) - 1, 1 << 2031
    data = U.packb({"node": "n0", "params": cts})
    got, ref = _both(data)
    assert type(got["params"]) is wire.ResidentUpdate and got["params"].scheme == "jl" and got["node"] == "n0"
    assert got["params"].handle._tab is not None and ref["params"].handle._tab is None
    assert got["params"].tolist() == ref["params"].tolist() == cts
    st = wire.reference_stats()
    assert (st["device_scan_jl"], st["device_scan_jl_refused"], st["device_scan"], st["device_scan_refused"]) == (1, 0, 0, 0)
    assert (st["resident"], st["fallback"]) == (2, 0)
    wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, device_scan_jl_min_items=1)
    assert {"scan", "h2d", "devscan"} <= set(wire.reference_stats()["last"])
    # device_scan_min_items means the LOM route only; resident=False never asks the device
    wire.reference_stats(reset=True)
    up = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, device_scan_min_items=1,
                              device_scan_jl_min_items=OFF)["params"]
    assert up.handle._tab is None and up.tolist() == cts
    assert wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, device_scan_jl_min_items=1)["params"] == cts
    st = wire.reference_stats()
    assert (st["device_scan_jl"], st["device_scan_jl_refused"], st["device_scan"], st["device_scan_refused"]) == (0, 0, 0, 0)
    assert (st["resident"], st["fast"]) == (1, 1)
    assert wire.DEVICE_SCAN_JL_MIN_ITEMS >= 256


def test_mixed_array_is_refused_and_takes_the_host_walk(dev):
    cts = _cts(70, 3)
    cts[40] = 5  # a native int among the maps: "jl" for the host scanner, a refusal for the tokenizer
    data = U.packb({"node": "n1", "params": cts})
    got, ref = _both(data)
    assert got["params"].scheme == ref["params"].scheme == "jl" and got["params"].tolist() == ref["params"].tolist() == cts
    assert got["params"].handle._tab is None
    st = wire.reference_stats()
    assert (st["device_scan_jl"], st["device_scan_jl_refused"], st["resident"]) == (0, 1, 2)
    # an array with a negative big int stays msgpack's on both routes
    wire.reference_stats(reset=True)
    vals = _cts(20) + [-(1 << 80)] + _cts(20)
    data = U.packb({"params": vals})
    got, ref = _both(data)
    assert got == ref == {"params": vals} and type(got["params"]) is list
    st = wire.reference_stats()
    assert (st["device_scan_jl"], st["device_scan_jl_refused"], st["resident"], st["fallback"]) == (0, 1, 0, 2)


def test_truncated_message_and_trailing_bytes_raise_what_msgpack_raises(dev):
    data = U.packb({"node": "n2", "params": _cts(40)})
    for cut in (len(data) - 1, len(data) - 30, len(data) - 300):
        with pytest.raises(Exception) as want:
            msgpack.unpackb(data[:cut], object_hook=U.ref_hook, strict_map_key=False)
        with pytest.raises(type(want.value)):
            wire.loads_reference(data[:cut], object_hook=U.ref_hook, min_items=1, resident=True, device_scan_jl_min_items=1)
    with pytest.raises(msgpack.exceptions.ExtraData):
        wire.loads_reference(data + b"\x01", object_hook=U.ref_hook, min_items=1, resident=True, device_scan_jl_min_items=1)
    st = wire.reference_stats()
    assert st["device_scan_jl_refused"] == 3 and st["device_scan_jl"] == 1 and st["resident"] == 0


def test_a_hook_that_reads_the_map_differently_never_reaches_the_device(dev):
    cts = _cts(40)
    data = U.packb({"params": cts})

    def other(o):  # the map as a tagged tuple, not the int
        return ("big", o["value"]) if o.get("__type__") == "int" else o

    for hook in (other, None):
        got = wire.loads_reference(data, object_hook=hook, min_items=1, resident=True, device_scan_jl_min_items=1)
        assert got == msgpack.unpackb(data, object_hook=hook, strict_map_key=False)
        st = wire.reference_stats()
        assert (st["device_scan_jl"], st["device_scan_jl_refused"], st["resident"]) == (0, 0, 0)
        assert "devscan" not in st["last"] and "h2d" not in st["last"]


# ---- end to end ------------------------------------------------------------------------------------------
def _receive(data):
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, device_scan_jl_min_items=1)
    assert type(got["params"]) is wire.ResidentUpdate and got["node"] == U.unpackb(data)["node"]
    assert got["params"].scheme == "jl" and got["params"].handle._tab is not None  # the device made the table
    return got["params"]


@pytest.fixture(scope="module")
def jl_round(dev):
    """Three parties of n_ct = 70, one reply a ciphertext short; a few ciphertexts replaced by values at the bin8 /
    bin16 edges of the reference's encoding and by short ones -- all of them 2^64 or more, so every item is a map."""
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    P, tau, n_ct = 3, 5, 70
    n = n_ct * D.jl_slot(None, P)[1]
    keys = [W.jl_user_key(p) for p in range(P)]
    ws = [W.party_weight(p) for p in range(P)]
    jc = SecaggCrypter()
    lists = [jc.encrypt(P, tau, W.party_params(p, n).astype(np.float64).tolist(), keys[p], W.BIPRIME0, weight=ws[p])
             for p in range(P)]
    assert [len(lst) for lst in lists] == [n_ct] * 3
    edges = [(1 << 2023) + 9, (1 << 2024) - 1, 1 << 2031, (1 << 2032) - 1, 1 << 2032, (1 << 2040) - 1, 1 << 2040, F.M64,
             (1 << 71) + 3]
    assert all(v < W.BIPRIME0 ** 2 for v in edges)
    for k, v in enumerate(edges):
        lists[k % P][2 + 7 * k] = v
    lists[1] = lists[1][:n_ct - 1]
    assert any(v.bit_length() < 2033 for lst in lists for v in lst) and all(v >= F.M64 for lst in lists for v in lst)
    msgs = [U.packb({"node": f"node-{p}", "params": lst}) for p, lst in enumerate(lists)]
    lists = [U.unpackb(m)["params"] for m in msgs]
    r = dict(jc=jc, P=P, tau=tau, n=n, n_ct=n_ct, sk0=-sum(keys), total=sum(ws), msgs=msgs, lists=lists)
    r["want"] = _bits(jc.aggregate(tau, P, lists, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=n))
    return r


def test_jl_round_end_to_end(dev, jl_round):
    r = jl_round
    assert len(r["want"]) == (r["n_ct"] - 1) * (r["n"] // r["n_ct"])  # truncated to the shortest reply
    for order in ([0, 1, 2], [1, 2, 0]):
        ups = [_receive(r["msgs"][p]) for p in order]
        agg = r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
        for u in ups:
            agg.add(u)
        assert _bits(agg.finish()) == r["want"], order
        assert not any(u.materialised for u in ups)
    ups = [_receive(m) for m in r["msgs"]]
    got = r["jc"].aggregate(r["tau"], r["P"], ups, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
    assert _bits(got) == r["want"]  # the one-shot aggregate
    mixed = [ups[0], r["lists"][1], ups[2]]
    got = r["jc"].aggregate(r["tau"], r["P"], mixed, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
    assert _bits(got) == r["want"] and not any(u.materialised for u in ups)
    st = wire.reference_stats()
    assert (st["device_scan_jl"], st["device_scan_jl_refused"], st["resident"], st["fallback"]) == (9, 0, 9, 0)
    h = ups[1].handle
    ups[1].release()
    assert h.released and h._tab is None
    with pytest.raises(RuntimeError):
        r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"]).add(ups[1])
    assert ups[0] == r["lists"][0] and ups[0].materialised  # a List[int] consumer still sees the reference's values


def test_jl_add_under_another_stream(dev, jl_round):
    """The upload and the tokenizer are on the current stream; the adds and the finish run under a side stream."""
    r = jl_round
    ups = [_receive(m) for m in r["msgs"]]
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        agg = r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
        for u in ups:
            agg.add(u)
        got = agg.finish_tensor().cpu().tolist()
    assert _bits(got) == r["want"] and not any(u.materialised for u in ups)


def test_a_jl_and_a_lom_array_in_one_message(dev, jl_round):
    from fedbiomed_amd import _device as D

    r = jl_round
    words = F.minimal_values(200, seed=4)
    data = U.packb({"a": r["lists"][0], "small": [1, 2, 3], "b": words, "node": "x"})
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=64, resident=True, device_scan_min_items=64,
                               device_scan_jl_min_items=64)
    a, b = got["a"], got["b"]
    assert type(a) is type(b) is wire.ResidentUpdate and (a.scheme, b.scheme) == ("jl", "lom") and got["small"] == [1, 2, 3]
    st = wire.reference_stats()
    assert (st["device_scan_jl"], st["device_scan"], st["device_scan_jl_refused"], st["device_scan_refused"]) == (1, 1, 0, 0)
    assert a.handle._blk is b.handle._blk and a.handle._tab is not b.handle._tab  # one upload block, a table each
    assert (a.handle._tab.numel(), b.handle._tab.numel()) == (r["n_ct"], 4)
    rows = D.wire_rows_device(b.handle).cpu().numpy().view(np.uint64).tolist()
    assert rows == words and a.tolist() == r["lists"][0] and b.tolist() == words

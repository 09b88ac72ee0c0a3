"""The device tokenizer on the GPU: fbm_wire_tokenize_lom (wire_tok_maps_kernel, wire_tok_scan_kernel,
wire_tok_emit_kernel) against fbm_wire_scan's table and a plain Python walk on the inputs of
tests/test_wire_tokenize_cpu.py, then `wire.loads_reference(resident=True, device_scan_min_items=1)` -- refusals,
truncation, the counters -- and a LOM round end to end, bit for bit against `aggregate` of the lists msgpack unpacks.

Shapes as in the CPU file (tests/wire_tokenize_util.py): the sub-block, tile and run boundaries at head 0 and off it;
the three "run" messages have 258 tiles, more than the summary scan's 256 threads, and are the largest at just over
1 MiB.  The round is tests/test_wire_fold_gpu.py's: three parties of n = 1025."""
import msgpack
import numpy as np
import pytest
import torch

from fedbiomed_amd import wire
from fedbiomed_amd import workload as W
from tests import wire_fold_util as F
from tests import wire_reference_util as U
from tests import wire_tokenize_util as T

pytestmark = pytest.mark.gpu

WHOLE = T.whole_cases()
REFUSED = T.refused_cases()


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
    b, e, _, _, table = T.scan_one(data)
    for head, base in ((0, 0), (3, 0), (1, b), (2, b)):
        rc, res, ck = T.device_tokenize(data[base:], base, first, n, head)
        assert rc == 0 and res == [n, e] and ck == table, (head, base, res, e)
    rc, res, ck = T.device_tokenize(data[b:e], b, first, n)  # the array's own span
    assert rc == 0 and res == [n, e] and ck == table


@pytest.mark.parametrize("case", REFUSED, ids=[c[0] for c in REFUSED])
def test_kernel_counting_stops_at_a_non_native_item(dev, case):
    _, data, first, n, want = case
    for head in (0, 1, 2, 3):
        rc, res, _ = T.device_tokenize(data, 0, first, n, head)
        assert rc == 0 and res == [want, 0], (head, res)


def test_kernel_span_cut_and_ints_behind_the_array(dev):
    items = T.pool_items(199, 4) + [T.nine(0xCF)]
    data, first, n = T.array_message(items)
    end = T.scan_one(data)[1]
    for cut in range(end - 9, end):
        rc, res, _ = T.device_tokenize(data[:cut], 0, first, n, cut % 4)
        assert rc == 0 and res == [n - 1, 0], (cut, res)
    tail = b"\x05\x06\xcc\x80\xcf" + bytes(8) + b"\x07" * 200
    data, first, n = T.array_message(T.pool_items(130, 1), tail)
    for ask in (n, 129, 65, 64, 1):
        count, end, table = T.walk(data, first, ask)
        rc, res, ck = T.device_tokenize(data, 0, first, ask, ask % 4)
        assert rc == 0 and res == [ask, end] and ck == table, (ask, res)


# ---- through loads_reference -----------------------------------------------------------------------------
def _both(data, hook=U.ref_hook):
    """The message read with the device scan forced on and with it disabled: (device route, host route)."""
    got = wire.loads_reference(data, object_hook=hook, min_items=1, resident=True, device_scan_min_items=1)
    ref = wire.loads_reference(data, object_hook=hook, min_items=1, resident=True, device_scan_min_items=2**40)
    return got, ref


def test_loads_reference_counts_and_equals_the_host_route(dev):
    arr, vals = F.lom_array(1025, 2)
    data = b"\x82" + U.packb("node") + U.packb("n0") + U.packb("params") + arr
    got, ref = _both(data)
    assert type(got["params"]) is wire.ResidentUpdate and got["params"].scheme == "lom" and got["node"] == "n0"
    assert got["params"].tolist() == ref["params"].tolist() == vals
    st = wire.reference_stats()
    assert (st["device_scan"], st["device_scan_refused"], st["resident"], st["fallback"]) == (1, 0, 2, 0)
    wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, device_scan_min_items=1)
    assert {"scan", "h2d", "devscan"} <= set(wire.reference_stats()["last"])
    # the default threshold leaves a small array to the host scanner; resident=False never asks the device
    wire.reference_stats(reset=True)
    wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True)
    wire.loads_reference(data, object_hook=U.ref_hook, min_items=1)
    st = wire.reference_stats()
    assert (st["device_scan"], st["device_scan_refused"], st["resident"], st["fast"]) == (0, 0, 1, 1)
    assert wire.DEVICE_SCAN_MIN_ITEMS >= 1024


def test_refused_arrays_take_the_host_walk(dev):
    # a JL update whose first ciphertext is below 2^64: a candidate, refused, and "jl" exactly as before
    cts = [5] + [(1 << 2040) + 17 * k for k in range(1, 70)] + [F.M64 - 1, 1 << 64]
    data = U.packb({"node": "n1", "params": cts})
    got, ref = _both(data)
    assert got["params"].scheme == ref["params"].scheme == "jl" and got["params"].tolist() == ref["params"].tolist() == cts
    st = wire.reference_stats()
    assert (st["device_scan"], st["device_scan_refused"], st["resident"]) == (0, 1, 2)
    # an array with a negative int stays msgpack's on both routes
    wire.reference_stats(reset=True)
    vals = list(range(100)) + [-1] + list(range(100))
    data = U.packb({"params": vals})
    got, ref = _both(data)
    assert got == ref == {"params": vals} and type(got["params"]) is list
    st = wire.reference_stats()
    assert (st["device_scan"], st["device_scan_refused"], st["resident"], st["fallback"]) == (0, 1, 0, 2)


def test_truncated_message_raises_what_msgpack_raises(dev):
    data = U.packb({"node": "n2", "params": F.minimal_values(300) + [F.M64 - 1]})
    for cut in (len(data) - 1, len(data) - 9, len(data) - 500):
        with pytest.raises(Exception) as want:
            msgpack.unpackb(data[:cut], object_hook=U.ref_hook, strict_map_key=False)
        with pytest.raises(type(want.value)):
            wire.loads_reference(data[:cut], object_hook=U.ref_hook, min_items=1, resident=True, device_scan_min_items=1)
    with pytest.raises(msgpack.exceptions.ExtraData):
        wire.loads_reference(data + b"\x01", object_hook=U.ref_hook, min_items=1, resident=True, device_scan_min_items=1)
    st = wire.reference_stats()
    assert st["device_scan_refused"] == 3 and st["device_scan"] == 1 and st["resident"] == 0


# ---- end to end ------------------------------------------------------------------------------------------
def _receive(data):
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, device_scan_min_items=1)
    assert type(got["params"]) is wire.ResidentUpdate and got["node"] == U.unpackb(data)["node"]
    return got["params"]


@pytest.fixture(scope="module")
def lom_round(dev):
    """Three stock peers' replies of n = 1025, as msgpack packs them, and the one-shot aggregate of the lists."""
    from fedbiomed_amd.secagg import SecaggLomCrypter

    P, n = 3, 1025
    lc = SecaggLomCrypter(W.LOM_NONCE)
    ws = [W.party_weight(p) for p in range(P)]
    lists = [F.minimal_values(n, seed=p + 2) for p in range(P)]
    msgs = [U.packb({"node": f"node-{p}", "params": lst, "n": n}) for p, lst in enumerate(lists)]
    lists = [U.unpackb(m)["params"] for m in msgs]
    return dict(lc=lc, total=sum(ws), msgs=msgs, lists=lists, want=_bits(lc.aggregate(lists, sum(ws))), n=n)


def test_lom_round_end_to_end(dev, lom_round):
    r = lom_round
    assert len(r["want"]) == r["n"]
    for order in ([0, 1, 2], [2, 0, 1]):
        ups = [_receive(r["msgs"][p]) for p in order]
        agg = r["lc"].begin_aggregate(r["total"])
        for u in ups:
            agg.add(u)
        assert _bits(agg.finish()) == r["want"]
        assert not any(u.materialised for u in ups)
    ups = [_receive(m) for m in r["msgs"]]
    assert _bits(r["lc"].aggregate(ups, r["total"])) == r["want"]  # the one-shot aggregate
    assert _bits(r["lc"].aggregate([ups[0], r["lists"][1], ups[2]], r["total"])) == r["want"]
    assert not any(u.materialised for u in ups)
    st = wire.reference_stats()
    assert (st["device_scan"], st["device_scan_refused"], st["resident"], st["fallback"]) == (9, 0, 9, 0)
    assert ups[0] == r["lists"][0] and ups[0].materialised  # a List[int] consumer still sees the reference's values


def test_lom_add_under_another_stream(dev, lom_round):
    """The upload and the tokenizer are on the current stream; the adds and the finish run under a side stream."""
    r = lom_round
    ups = [_receive(m) for m in r["msgs"]]
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        agg = r["lc"].begin_aggregate(r["total"])
        for u in ups:
            agg.add(u)
        got = agg.finish()
    assert _bits(got) == r["want"] and not any(u.materialised for u in ups)


def test_two_deferred_arrays_in_one_message_and_release(dev, lom_round):
    from fedbiomed_amd import _device as D

    r = lom_round
    small = [1, 2, 3]
    data = U.packb({"a": r["lists"][0], "small": small, "b": r["lists"][1], "node": "x"})
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=64, resident=True, device_scan_min_items=64)
    a, b = got["a"], got["b"]
    assert type(a) is type(b) is wire.ResidentUpdate and got["small"] == small and got["node"] == "x"
    st = wire.reference_stats()
    assert (st["device_scan"], st["device_scan_refused"], st["resident"]) == (2, 0, 2)
    assert a.handle._blk is b.handle._blk and a.handle._tab is not b.handle._tab  # one upload, a table each
    agg = r["lc"].begin_aggregate(r["total"])
    agg.add(a)
    agg.add(b)
    agg.add(r["lists"][2])
    assert _bits(agg.finish()) == r["want"]
    rows = D.wire_rows_device(b.handle).cpu().numpy().view(np.uint64).tolist()
    assert rows == r["lists"][1] and a.tolist() == r["lists"][0]
    # a tokenized array beside one the host scanner records (below the device threshold)
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, device_scan_min_items=64)
    assert type(got["small"]) is wire.ResidentUpdate and got["small"].tolist() == small and got["b"].tolist() == r["lists"][1]
    h = a.handle
    a.release()
    assert h.released and h._tab is None
    with pytest.raises(RuntimeError):
        r["lc"].begin_aggregate(r["total"]).add(a)
    with pytest.raises(RuntimeError):
        D.wire_fold_lom(h, torch.zeros(r["n"], dtype=torch.int64, device=dev), True)
    assert b.tolist() == r["lists"][1]  # the other array's table and the shared upload stand

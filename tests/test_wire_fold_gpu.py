"""A stock peer's reply folded into the aggregate without leaving the device: fbm_wire_fold_lom
(wire_fold_lom_kernel) against fbm_wire_decode followed by fbm_lom_fold and against Python's sum, then
`wire.loads_reference(resident=True)` -> `begin_aggregate().add` / `aggregate` for both schemes, bit for bit against
`aggregate` of the lists msgpack unpacks.

Shapes.  One wave folds a group of 64 items and a workgroup holds four groups: n = 1, 63, 64, 65, 127, 128, 129 are
the group's edges, 257 and 1025 the workgroup's (a partial last group in a second and a fifth workgroup).  Items take
every native width and every non-minimal form (tests/wire_fold_util.py), so a group's bytes start at every offset
residue.  The JL path reuses the two existing kernels: 130 ciphertexts are two of jl_fold's units and a part."""
import numpy as np
import pytest
import torch

from fedbiomed_amd import wire
from fedbiomed_amd import workload as W
from tests import wire_fold_util as F
from tests import wire_reference_util as U

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def dev():
    from fedbiomed_amd import _device as D

    return D.device()


@pytest.fixture(autouse=True)
def _fresh_stats():
    wire.reference_stats(reset=True)


def _i64(vals, dev):
    return torch.from_numpy(F.u64(vals).view(np.int64)).to(dev)


def _u64_list(t):
    return t.cpu().numpy().view(np.uint64).tolist()


def _framed(acc0, dev):
    """The accumulator at element offset 1 of a larger buffer (8-byte aligned only), sentinels around it."""
    n = len(acc0)
    big = torch.full((n + 3,), SENTINEL, dtype=torch.int64, device=dev)
    big[1:1 + n] = _i64(acc0, dev)
    return big, big[1:1 + n]


def _upload(data, table=None):
    from fedbiomed_amd import _device as D

    (b, e, n, scheme, ck), = D.wire_scan(data, 1)
    assert scheme == "lom" and b > 0
    h, = D.wire_upload(data, [(b, e, n, scheme, ck if table is None else table)])
    return h, (b, e, ck)


@pytest.mark.parametrize("n", F.NS)
def test_fused_equals_decode_then_fold_and_python(dev, n):
    from fedbiomed_amd import _device as D

    for off in (0, 5):
        arr, vals = F.lom_array(n, off)
        data, _ = F.message(arr)
        h, _ = _upload(data)
        acc0 = F.acc_values(n)
        for first in (True, False):
            big, acc = _framed(acc0, dev)
            D.wire_fold_lom(h, acc, first)
            big2, acc2 = _framed(acc0, dev)
            D.lom_fold(acc2, D.wire_rows_device(h), first)
            got = _u64_list(big)
            assert got[1:1 + n] == F.folded(acc0, vals, first), (n, off, first)
            assert got[0] == SENTINEL and got[1 + n:] == [SENTINEL] * 2  # the elements around it: untouched
            assert torch.equal(big, big2)


def test_wrap_around_and_three_folds(dev):
    from fedbiomed_amd import _device as D

    data, _ = F.message(U.packb([1, F.M64 - 1, 0, 5]))
    h, _ = _upload(data)
    acc = _i64([F.M64 - 1] * 4, dev)
    assert _u64_list(D.wire_fold_lom(h, acc, False)) == [0, F.M64 - 2, F.M64 - 1, 4]
    n, total = 1025, [0] * 1025
    acc = torch.full((n,), SENTINEL, dtype=torch.int64, device=dev)
    for k, off in enumerate((0, 3, 9)):
        arr, vals = F.lom_array(n, off)
        h, _ = _upload(F.message(arr)[0])
        D.wire_fold_lom(h, acc, k == 0)
        total = [(t + v) % F.M64 for t, v in zip(total, vals)]
    assert _u64_list(acc) == total


def test_a_foreign_table_counts_as_zero(dev):
    """Checkpoints before the span, past it and in its last bytes (where no item starts): those groups add 0 --
    the accumulator keeps its value when continuing and becomes 0 on a first call; the other groups stand."""
    from fedbiomed_amd import _device as D

    n = 256
    vals = F.minimal_values(n - 1) + [F.M64 - 1]
    data, _ = F.message(U.packb(vals))
    _, (b, e, ck) = _upload(data)
    table = ck.copy()
    table[0], table[1], table[3] = b - 1, e, e - 2
    h, _ = _upload(data, table)
    want = [0] * 128 + vals[128:192] + [0] * 64
    acc0 = F.acc_values(n)
    for first in (True, False):
        big, acc = _framed(acc0, dev)
        D.wire_fold_lom(h, acc, first)
        got = _u64_list(big)
        assert got[1:1 + n] == F.folded(acc0, want, first) and got[0] == SENTINEL and got[-2:] == [SENTINEL] * 2


def test_device_argument_checks(dev):
    from fedbiomed_amd import _device as D

    arr, _ = F.lom_array(65)
    h, _ = _upload(F.message(arr)[0])
    with pytest.raises(ValueError):
        D.wire_fold_lom(h, torch.zeros(64, dtype=torch.int64, device=dev), True)
    with pytest.raises(ValueError):
        D.wire_fold_lom(h, torch.zeros(65, dtype=torch.int32, device=dev), True)
    with pytest.raises(ValueError):
        D.wire_fold_lom(h, torch.zeros(130, dtype=torch.int64, device=dev)[::2], True)
    h.release()
    with pytest.raises(RuntimeError):
        D.wire_fold_lom(h, torch.zeros(65, dtype=torch.int64, device=dev), True)


# ---- end to end ------------------------------------------------------------------------------------------
def _bits(xs):
    return np.asarray(xs, dtype=np.float64).view(np.uint64).tolist()


def _receive(data):
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True)
    assert type(got["params"]) is wire.ResidentUpdate and got["node"] == U.unpackb(data)["node"]
    return got["params"]


@pytest.fixture(scope="module")
def lom_round(dev):
    """Three stock peers' replies of n = 1025, as msgpack packs them, and the one-shot aggregate of the lists."""
    from fedbiomed_amd.secagg import SecaggLomCrypter

    P, n, tau = 3, 1025, 2
    ids = W.node_ids(P)
    ws = [W.party_weight(p) for p in range(P)]
    lc = SecaggLomCrypter(W.LOM_NONCE)
    lists = [lc.encrypt(tau, u, W.party_params(p, n).astype(np.float64).tolist(), W.pairwise_secrets_for(u, ids), ids,
                        weight=ws[p]) for p, u in enumerate(ids)]
    msgs = [U.packb({"node": f"node-{p}", "params": lst, "n": n}) for p, lst in enumerate(lists)]
    lists = [U.unpackb(m)["params"] for m in msgs]
    return dict(lc=lc, total=sum(ws), msgs=msgs, lists=lists, want=_bits(lc.aggregate(lists, sum(ws))), n=n)


def test_lom_end_to_end(dev, lom_round):
    r = lom_round
    assert len(r["want"]) == r["n"]
    for order in ([0, 1, 2], [2, 0, 1]):
        for as_tensor in (False, True):
            ups = [_receive(r["msgs"][p]) for p in order]
            agg = r["lc"].begin_aggregate(r["total"])
            for u in ups:
                agg.add(u)
            if as_tensor:
                t = agg.finish_tensor()
                assert t.dtype == torch.float64 and _bits(t.cpu().tolist()) == r["want"]
            else:
                assert _bits(agg.finish()) == r["want"]
            assert not any(u.materialised for u in ups)
    st = wire.reference_stats()
    assert (st["resident"], st["fast"], st["fallback"]) == (12, 0, 0)


def test_lom_add_under_another_stream(dev, lom_round):
    """The upload is on the current stream; the adds and the finish run under a side stream."""
    r = lom_round
    ups = [_receive(m) for m in r["msgs"]]
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        agg = r["lc"].begin_aggregate(r["total"])
        for u in ups:
            agg.add(u)
        got = agg.finish()
    assert _bits(got) == r["want"] and not any(u.materialised for u in ups)


def test_lom_one_shot_mixed_and_errors(dev, lom_round):
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError

    r = lom_round
    ups = [_receive(m) for m in r["msgs"]]
    assert _bits(r["lc"].aggregate(ups, r["total"])) == r["want"]
    assert _bits(r["lc"].aggregate([ups[0], r["lists"][1], ups[2]], r["total"])) == r["want"]  # a list among them
    assert not any(u.materialised for u in ups)
    short = _receive(U.packb({"node": "x", "params": r["lists"][1][:-1]}))
    agg = r["lc"].begin_aggregate(r["total"])
    agg.add(ups[0])
    agg.add(short)  # unequal lengths: the stream's error, at finish
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624.*differ in length"):
        agg.finish()
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624.*differ in length"):
        r["lc"].aggregate([ups[0], short], r["total"])
    ups[1].release()
    with pytest.raises(RuntimeError):
        r["lc"].begin_aggregate(r["total"]).add(ups[1])
    assert ups[0] == r["lists"][0] and ups[0].materialised  # a List[int] consumer still sees the reference's values


@pytest.fixture(scope="module")
def jl_round(dev):
    """Three parties of n_ct = 130, one reply a ciphertext short; a few ciphertexts replaced by values at the
    bin8 / bin16 edges of the reference's encoding (L = 254, 255 | 256, 257 bytes) and by native ones (< 2^64)."""
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    P, tau, n_ct = 3, 5, 130
    n = n_ct * D.jl_slot(None, P)[1]
    keys = [W.jl_user_key(p) for p in range(P)]
    ws = [W.party_weight(p) for p in range(P)]
    jc = SecaggCrypter()
    lists = [jc.encrypt(P, tau, W.party_params(p, n).astype(np.float64).tolist(), keys[p], W.BIPRIME0, weight=ws[p])
             for p in range(P)]
    assert [len(lst) for lst in lists] == [n_ct] * 3
    edges = [(1 << 2023) + 9, (1 << 2024) - 1, 1 << 2031, (1 << 2032) - 1, 1 << 2032, (1 << 2040) - 1, 1 << 2040, 5,
             F.M64 - 1, F.M64, 0]
    assert all(v < W.BIPRIME0 ** 2 for v in edges)
    for k, v in enumerate(edges):
        lists[k % P][3 + 11 * k] = v
    lists[1] = lists[1][:129]
    sizes = {len(U.packb([v])) - 1 for lst in lists for v in lst}
    assert {1, 9, 20 + 2 + 254, 20 + 2 + 255, 20 + 3 + 256, 20 + 3 + 257} <= sizes
    msgs = [U.packb({"node": f"node-{p}", "params": lst}) for p, lst in enumerate(lists)]
    lists = [U.unpackb(m)["params"] for m in msgs]
    r = dict(jc=jc, P=P, tau=tau, n=n, sk0=-sum(keys), total=sum(ws), msgs=msgs, lists=lists)
    r["want"] = _bits(jc.aggregate(tau, P, lists, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=n))
    return r


def test_jl_end_to_end(dev, jl_round):
    r = jl_round
    assert len(r["want"]) == 129 * (r["n"] // 130)  # truncated to the shortest reply
    for order in ([0, 1, 2], [1, 2, 0]):  # the shorter reply second, then first
        ups = [_receive(r["msgs"][p]) for p in order]
        assert [u.scheme for u in ups] == ["jl"] * 3 and sorted(len(u) for u in ups) == [129, 130, 130]
        agg = r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
        for u in ups:
            agg.add(u)
        assert _bits(agg.finish()) == r["want"], order
        assert not any(u.materialised for u in ups)
    ups = [_receive(m) for m in r["msgs"]]
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):  # another stream than the upload's
        agg = r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
        for u in ups:
            agg.add(u)
        t = agg.finish_tensor()
        got = t.cpu().tolist()
    assert _bits(got) == r["want"]


def test_jl_one_shot_and_wrong_scheme(dev, jl_round, lom_round):
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError

    r = jl_round
    ups = [_receive(m) for m in r["msgs"]]
    got = r["jc"].aggregate(r["tau"], r["P"], ups, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
    assert _bits(got) == r["want"]
    mixed = [ups[0], r["lists"][1], ups[2]]
    got = r["jc"].aggregate(r["tau"], r["P"], mixed, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
    assert _bits(got) == r["want"] and not any(u.materialised for u in ups)
    lom_up = _receive(lom_round["msgs"][0])
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624"):
        r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"]).add(lom_up)
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624"):
        lom_round["lc"].begin_aggregate(lom_round["total"]).add(ups[0])
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624"):
        lom_round["lc"].aggregate([lom_up, ups[0]], lom_round["total"])
    assert ups[1] == r["lists"][1] and ups[1].materialised

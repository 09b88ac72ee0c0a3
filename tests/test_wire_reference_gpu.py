"""The reference Serializer's update bytes on the GPU: `wire.reference_bytes` / `dumps_reference` (the three encode
passes of csrc/fbm_wire.hip) and `wire.loads_reference` (host scan, then the two decode kernels) against msgpack
under the reference's rules (`fedbiomed/common/serializer.py:96-110`, `:140-149`; tests/wire_reference_util.py) --
every expected byte and value is msgpack's -- and the crypters' flows through them, bit for bit against the
plain-list path.

Shapes.  The JL encode works in tiles of 256 items, one wave per item, each item's bytes split at the 4-byte
boundaries of its (unaligned) offset: 600 items of every bit-length class in an order that puts items at all four
offset residues cross two tile boundaries; 4 096 full-width items are sixteen full tiles.  The LOM encode's tile
is 1 024 items (four per thread): 10 000 and 70 000 words leave a partial last tile, and 70 000 crosses the array
header's dc -> dd.  The LOM decode's group is K = 64 items (FBM_WIRE_LOM_GROUP), four groups per workgroup:
n = K - 1, K, K + 1, 2K + 1."""
import random

import numpy as np
import pytest
import torch

from fedbiomed_amd import _native as N
from fedbiomed_amd import wire
from fedbiomed_amd import workload as W
from tests import wire_reference_util as U

pytestmark = pytest.mark.gpu
K = N.WIRE_LOM_GROUP
_cache = {}


@pytest.fixture(scope="module")
def dev():
    from fedbiomed_amd import _device as D

    return D.device()


@pytest.fixture(autouse=True)
def _fresh_stats():
    wire.reference_stats(reset=True)


def _case(name):
    """(scheme, values, the reference's bytes), made once per name and left unchanged."""
    if name in _cache:
        return _cache[name]
    rng = random.Random(sum(map(ord, name)))
    if name == "jl_mixed_600":
        edges = U.edge_values()  # sizes 1, 2, 3, 5, 9, 32 .. 280: consecutive offsets take every residue
        vals = [edges[(7 * i) % len(edges)] if i % 3 else rng.getrandbits(rng.choice(U.MAP_BITS)) for i in range(600)]
        scheme = "jl"
    elif name == "jl_full_4096":
        vals, scheme = [rng.getrandbits(2048) | (1 << 2047) for _ in range(4096)], "jl"
    elif name == "jl_all_small":
        vals, scheme = [rng.getrandbits(rng.choice([1, 7, 8, 15, 16, 31, 33, 64])) for _ in range(700)], "jl"
    elif name == "lom_mixed_10000":
        vals = [U.NATIVE_EDGES[i % 10] if i % 4 == 0 else rng.getrandbits(rng.choice([7, 8, 16, 32, 64]))
                for i in range(10000)]
        scheme = "lom"
    elif name == "lom_random_70000":
        vals, scheme = np.random.default_rng(7).integers(0, 2**64, size=70000, dtype=np.uint64).tolist(), "lom"
    elif name.startswith("lom_n"):
        n = int(name[5:])
        vals, scheme = [rng.getrandbits(rng.choice([5, 8, 13, 30, 64])) for _ in range(n)], "lom"
    else:
        raise KeyError(name)
    _cache[name] = (scheme, vals, U.packb(vals))
    return _cache[name]


def _update(scheme, vals):
    return wire.EncryptedParams.from_ints(scheme, vals)


JL_CASES = ["jl_mixed_600", "jl_full_4096", "jl_all_small"]
LOM_CASES = ["lom_mixed_10000", "lom_random_70000"]
HEADER_CASES = [f"lom_n{n}" for n in (0, 1, 15, 16, 65535, 65536)]
GROUP_CASES = [f"lom_n{n}" for n in (K - 1, K, K + 1, 2 * K + 1)]


def test_the_mixed_case_meets_every_offset_residue_and_size_class():
    _, vals, ref = _case("jl_mixed_600")
    sizes = [len(U.packb([v])) - 1 for v in vals]
    offs = np.cumsum([3] + sizes[:-1])
    assert {int(o) % 4 for o in offs} == {0, 1, 2, 3} and 3 + sum(sizes) == len(ref)
    assert {1, 2, 3, 5, 9, 32, 33, 276, 277, 279, 280} <= set(sizes)
    for s in (280, 279, 32, 9):  # the widest forms at every residue
        assert {int(o) % 4 for o, z in zip(offs, sizes) if z == s} == {0, 1, 2, 3}, s


@pytest.mark.parametrize("name", JL_CASES + LOM_CASES + HEADER_CASES)
def test_reference_bytes_equals_packb(dev, name):
    scheme, vals, ref = _case(name)
    got = wire.reference_bytes(_update(scheme, vals))
    assert len(got) == len(ref) and got == ref
    st = wire.reference_stats()
    assert (st["fast"], st["fallback"]) == (1, 0)


@pytest.mark.parametrize("name", JL_CASES + LOM_CASES + HEADER_CASES[1:] + GROUP_CASES)
def test_loads_reference_equals_unpackb(dev, name):
    """Once on the bytes this code makes inside a message built around them, once on a message that plain packb
    built from Python ints, as a stock peer sends it."""
    scheme, vals, ref = _case(name)
    mine = wire.dumps_reference({"id": "node-03", "n": len(vals), "params": _update(scheme, vals), "after": [1.5, None]})
    stock = U.packb({"id": "node-03", "n": len(vals), "params": vals, "after": [1.5, None]})
    assert mine == stock
    for data in (mine, stock):
        wire.reference_stats(reset=True)
        got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1)
        assert got == U.unpackb(data)
        p = got["params"]
        assert isinstance(p, wire.EncryptedParams) and p.consistent() and list(p) == vals
        native = all(v < 2**64 for v in vals)
        assert p.scheme == ("lom" if native else "jl")  # "lom" when every item is native
        want = np.array(vals, dtype=np.uint64) if native else U.jl_rows(vals)
        assert p.packed.dtype == want.dtype and p.packed.shape == want.shape and np.array_equal(p.packed, want)
        st = wire.reference_stats()
        assert st["fallback"] == 0 and st["fast"] == 1  # ("after" holds a float: not recorded)


def test_several_updates_in_one_message(dev):
    cases = [_case(n) for n in ("jl_mixed_600", "lom_n65", "jl_all_small", "lom_mixed_10000")]
    msg = {"a": [_update(s, v) for s, v, _ in cases], "b": "x", "c": _update(*cases[0][:2])}
    plain = {"a": [v for _, v, _ in cases], "b": "x", "c": cases[0][1]}
    data = wire.dumps_reference(msg, default=U.ref_default)
    assert data == U.packb(plain)
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1)
    assert got == plain
    assert [p.scheme for p in got["a"]] == ["jl", "lom", "lom", "lom"] and got["c"].scheme == "jl"
    assert wire.reference_stats()["fallback"] == 0


def test_refused_arrays_fall_back_and_still_equal_unpackb(dev):
    _, vals, _ = _case("jl_mixed_600")
    _, lom, _ = _case("lom_n65")
    for bad in ([-1], [2**2048], [1.5]):
        wire.reference_stats(reset=True)
        data = U.packb({"params": vals[:50] + bad, "n": 3})
        assert wire.loads_reference(data, object_hook=U.ref_hook, min_items=1) == U.unpackb(data)
        st = wire.reference_stats()
        assert (st["fast"], st["fallback"]) == (0, 1), bad
    wire.reference_stats(reset=True)
    data = U.packb({"bad": vals[:50] + [-1], "good": lom})  # one array refused, the other taken
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=2)
    assert got == U.unpackb(data) and type(got["bad"]) is list and isinstance(got["good"], wire.EncryptedParams)
    e = _update("jl", vals)
    e.pop()  # the packed form is dropped: the ordinary route
    wire.reference_stats(reset=True)
    assert wire.reference_bytes(e) == U.packb(vals[:-1])
    assert wire.reference_stats()["fallback"] == 1


def test_device_tensor_input(dev):
    from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

    P, n, tau = 3, 300, 4
    x = W.party_params(1, n).astype(np.float64)
    ids = W.node_ids(P)
    jc, lc = SecaggCrypter(), SecaggLomCrypter(W.LOM_NONCE)
    xt = torch.from_numpy(x).to(dev)
    ct = jc.encrypt_tensor(P, tau, xt, W.jl_user_key(1), W.BIPRIME0, weight=W.party_weight(1))
    lst = jc.encrypt(P, tau, x.tolist(), W.jl_user_key(1), W.BIPRIME0, weight=W.party_weight(1))
    assert wire.reference_bytes(ct) == U.packb(lst)
    y = lc.encrypt_tensor(tau, ids[1], xt, W.pairwise_secrets_for(ids[1], ids), ids, weight=W.party_weight(1))
    lst = lc.encrypt(tau, ids[1], x.tolist(), W.pairwise_secrets_for(ids[1], ids), ids, weight=W.party_weight(1))
    assert wire.reference_bytes(y) == U.packb(lst)
    assert wire.reference_stats()["fallback"] == 0
    with pytest.raises(ValueError):
        wire.reference_bytes(xt)


def _bits(xs):
    return np.asarray(xs, dtype=np.float64).view(np.uint64)


def test_end_to_end_with_a_stock_peer(dev):
    """This side patched, the peer stock, in both directions, on `workload`'s small JL and LOM cases."""
    from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

    P, n, tau = 3, 500, 2
    ws = [W.party_weight(p) for p in range(P)]
    xs = [W.party_params(p, n).astype(np.float64).tolist() for p in range(P)]
    keys = [W.jl_user_key(p) for p in range(P)]
    ids = W.node_ids(P)
    jc, lc = SecaggCrypter(), SecaggLomCrypter(W.LOM_NONCE)
    try:
        plain_j = [jc.encrypt(P, tau, xs[p], keys[p], W.BIPRIME0, weight=ws[p]) for p in range(P)]
        plain_l = [lc.encrypt(tau, u, xs[p], W.pairwise_secrets_for(u, ids), ids, weight=ws[p]) for p, u in enumerate(ids)]
        wire.enable()
        enc_j = [jc.encrypt(P, tau, xs[p], keys[p], W.BIPRIME0, weight=ws[p]) for p in range(P)]
        enc_l = [lc.encrypt(tau, u, xs[p], W.pairwise_secrets_for(u, ids), ids, weight=ws[p]) for p, u in enumerate(ids)]
    finally:
        wire.enable(False)
    # a patched node to the stock researcher: dumps_reference, then the stock unpackb with the reference hook
    for enc, plain in ((enc_j, plain_j), (enc_l, plain_l)):
        for e, p in zip(enc, plain):
            assert isinstance(e, wire.EncryptedParams)
            data = wire.dumps_reference({"params": e, "node": "n"}, default=U.ref_default)
            assert data == U.packb({"params": p, "node": "n"}) and U.unpackb(data)["params"] == p
    # stock nodes to the patched researcher: stock packb of plain lists, then loads_reference, then the aggregates
    recv_j = [wire.loads_reference(U.packb({"params": p}), object_hook=U.ref_hook, min_items=1)["params"] for p in plain_j]
    recv_l = [wire.loads_reference(U.packb({"params": p}), object_hook=U.ref_hook, min_items=1)["params"] for p in plain_l]
    assert wire.packed_rows(recv_j, "jl", len(recv_j[0])) is not None and wire.packed_rows(recv_l, "lom") is not None
    assert wire.reference_stats()["fallback"] == 0
    want = _bits(jc.aggregate(tau, P, plain_j, -sum(keys), W.BIPRIME0, sum(ws), num_expected_params=n))
    assert np.array_equal(_bits(jc.aggregate(tau, P, recv_j, -sum(keys), W.BIPRIME0, sum(ws), num_expected_params=n)), want)
    agg = jc.begin_aggregate(tau, P, -sum(keys), W.BIPRIME0, sum(ws), num_expected_params=n)
    for r in recv_j:
        agg.add(r)
    assert np.array_equal(_bits(agg.finish()), want)
    want = _bits(lc.aggregate(plain_l, sum(ws)))
    assert np.array_equal(_bits(lc.aggregate(recv_l, sum(ws))), want)
    lagg = lc.begin_aggregate(sum(ws))
    for r in recv_l:
        lagg.add(r)
    assert np.array_equal(_bits(lagg.finish()), want)

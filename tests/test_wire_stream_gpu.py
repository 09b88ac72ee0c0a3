"""The streamed receive path on the device: fbm_wire_stream_begin / fbm_wire_stream_feed word for word against the host
run and fbm_wire_scan's table over the cuts where a feed's work changes, and wire.StreamAssembler ->
`loads_reference(msg, resident=True)` -> `begin_aggregate().add` bit for bit against the list path's aggregate and against the oracle's recorded rounds
(tests/golden: the reference's `enc` lists and `agg` results), with the counters that show the streamed
path was the one taken.  The messages are tests/wire_stream_util.py's: about three tiles each."""
import msgpack
import numpy as np
import pytest
import torch

from fedbiomed_amd import wire
from fedbiomed_amd import workload as W
from tests import wire_fold_util as F
from tests import wire_reference_util as U
from tests import wire_stream_util as S
from tests.wire_tokenize_util import placed

pytestmark = pytest.mark.gpu

KW = dict(object_hook=U.ref_hook, min_items=16, device_scan_min_items=32, device_scan_jl_min_items=32)


@pytest.fixture(scope="module")
def dev():
    from fedbiomed_amd import _device as D

    return D.device()


@pytest.fixture(autouse=True)
def _fresh_stats():
    wire.reference_stats(reset=True)


def _bits(xs):
    return np.asarray(xs, dtype=np.float64).view(np.uint64).tolist()


def _cuts(span_len, s0, item, group, scheme):
    """About 40 avail_len values: +-1 around `first`, around 64-byte and 4096-byte boundaries of the block (head 0: the
    tiles are counted from `first`), around a tile's end plus an item's reach (where a feed's work changes), around an
    item boundary and a checkpoint group's (`item`, `group`: span offsets), and the last byte."""
    reach = 280 if scheme == "jl" else 8
    at = [s0, s0 + 64, s0 + 64 * 9, s0 + S.TILE, s0 + 2 * S.TILE, s0 + S.TILE + reach, s0 + 2 * S.TILE + reach, S.TILE, 2 * S.TILE,
          item, group, span_len - 1]
    cuts = sorted({c + d for c in at for d in (-1, 0, 1) if s0 <= c + d <= span_len})
    assert 30 <= len(cuts) <= 45
    return cuts


@pytest.mark.parametrize("scheme", ["lom", "jl"])
def test_kernel_feeds_equal_the_host_run_and_the_scanner(dev, scheme):
    from fedbiomed_amd import _native as N

    data, _ = S.lom_message() if scheme == "lom" else S.jl_message()
    b, first, e, n, _, table = S.locate(data)
    tail = data[e:]
    assert tail  # the bytes behind the array: "sample_size" and its value
    lib = N.load_test()
    for head, base in ((0, 0), (3, b)):
        span = data[base:]
        buf = placed(span, first - base, head)
        want, ck = S.host_one_shot(lib, scheme, buf, base, first, n)
        assert want == [n, e] and ck == table
        # span offsets of a value's first byte (an item boundary lies 22 or 23 bytes in front) / of groups' first items
        marks = [(c >> 16) - base for c in table] if scheme == "jl" else [c - base for c in table]
        cuts = _cuts(len(span), first - base, marks[len(marks) // 2] - (22 if scheme == "jl" else 0), marks[17], scheme)
        for a in cuts:
            hrc, hres, htab = S.host_feeds(lib, scheme, buf, base, first, n, [a, len(span)])
            rcs, res, tab = S.device_feeds(scheme, span, base, first, n, [a, len(span)], head)
            assert rcs == hrc == [0, 0, 0] and res == hres == want and tab == htab == table, (head, base, a)
    # several feeds, and the whole span in one
    span = data[b:]
    for avails in (list(range(1000, len(span), 1000)) + [len(span)], [len(span)]):
        rcs, res, tab = S.device_feeds(scheme, span, b, first, n, avails, 2)
        assert set(rcs) == {0} and res == [n, e] and tab == table
    # a span the end cuts inside the last item: the one-shot's refusal
    cut = e - 1 - b
    buf = placed(span[:cut], first - b, 1)
    want, _ = S.host_one_shot(lib, scheme, buf, b, first, n)
    rcs, res, _ = S.device_feeds(scheme, span[:cut], b, first, n, [S.TILE + 300, cut], 1)
    assert set(rcs) == {0} and res == want == [n - 1, 0]


# ---- end to end ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lom_round(dev):
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


@pytest.fixture(scope="module")
def jl_round(dev):
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    P, tau, n_ct = 3, 5, 70
    n = n_ct * D.jl_slot(None, P)[1]
    keys = [W.jl_user_key(p) for p in range(P)]
    ws = [W.party_weight(p) for p in range(P)]
    jc = SecaggCrypter()
    lists = [jc.encrypt(P, tau, W.party_params(p, n).astype(np.float64).tolist(), keys[p], W.BIPRIME0, weight=ws[p])
             for p in range(P)]
    for k, v in enumerate([(1 << 2023) + 9, (1 << 2032) - 1, 1 << 2040, F.M64, (1 << 71) + 3]):
        lists[k % P][2 + 7 * k] = v  # bin8 / bin16 edges and short values, all of them maps
    msgs = [U.packb({"node": f"node-{p}", "params": lst}) for p, lst in enumerate(lists)]
    lists = [U.unpackb(m)["params"] for m in msgs]
    r = dict(jc=jc, P=P, tau=tau, n=n, n_ct=n_ct, sk0=-sum(keys), total=sum(ws), msgs=msgs, lists=lists)
    r["want"] = _bits(jc.aggregate(tau, P, lists, r["sk0"], W.BIPRIME0, r["total"], num_expected_params=n))
    return r


def _receive(asm, data, size, scheme):
    msg = S.stream(asm, S.chunked(data, size))
    assert msg.streamed
    got = wire.loads_reference(msg, resident=True, **KW)
    up = got["params"]
    assert type(up) is wire.ResidentUpdate and up.scheme == scheme and got["node"] == U.unpackb(data)["node"]
    assert msg.joins == 0 and up.handle._tab is not None
    return up


def test_lom_round_streamed_with_three_chunkings(dev, lom_round):
    r = lom_round
    asm = wire.StreamAssembler(**KW)
    ups = [_receive(asm, m, size, "lom") for m, size in zip(r["msgs"], (4096, 1000, 5001))]
    agg = r["lc"].begin_aggregate(r["total"])
    for u in ups:
        agg.add(u)
    assert _bits(agg.finish()) == r["want"] and not any(u.materialised for u in ups)
    st = wire.reference_stats()
    assert (st["streamed"], st["stream_fallback"], st["resident"], st["fallback"]) == (3, 0, 3, 0)
    assert st["device_scan"] == 0  # nothing went up a second time
    assert ups[0] == r["lists"][0]  # a List[int] consumer still sees the reference's values


def test_jl_round_streamed_with_three_chunkings(dev, jl_round):
    r = jl_round
    asm = wire.StreamAssembler(**KW)
    ups = [_receive(asm, m, size, "jl") for m, size in zip(r["msgs"], (4096, 777, 9000))]
    agg = r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
    for u in ups:
        agg.add(u)
    assert _bits(agg.finish()) == r["want"] and not any(u.materialised for u in ups)
    st = wire.reference_stats()
    assert (st["streamed"], st["stream_fallback"], st["resident"], st["fallback"]) == (3, 0, 3, 0)
    assert st["device_scan_jl"] == 0
    assert ups[2] == r["lists"][2]


def test_add_under_another_current_stream(dev, lom_round, jl_round):
    """The uploads and feeds are on the assembler's stream; the adds and the finish run under a side stream."""
    asm = wire.StreamAssembler(**KW)
    side = torch.cuda.Stream(device=dev)
    r = lom_round
    ups = [_receive(asm, m, 3000, "lom") for m in r["msgs"]]
    with torch.cuda.stream(side):
        agg = r["lc"].begin_aggregate(r["total"])
        for u in ups:
            agg.add(u)
        got = agg.finish_tensor().cpu().tolist()
    assert _bits(got) == r["want"]
    r = jl_round
    ups = [_receive(asm, m, 3000, "jl") for m in r["msgs"]]
    with torch.cuda.stream(side):
        agg = r["jc"].begin_aggregate(r["tau"], r["P"], r["sk0"], W.BIPRIME0, r["total"], num_expected_params=r["n"])
        for u in ups:
            agg.add(u)
        got = agg.finish_tensor().cpu().tolist()
    assert _bits(got) == r["want"]


def _same(got, want):
    assert type(got) is type(want) and list(got) == list(want)
    for k in want:
        a, b = got[k], want[k]
        if isinstance(b, wire.ResidentUpdate):
            assert type(a) is wire.ResidentUpdate and (a.scheme, a.n_items) == (b.scheme, b.n_items) and a.tolist() == b.tolist()
        else:
            assert a == b and type(a) is type(b)


def test_fallbacks_return_what_the_joined_call_returns_or_raises(dev, jl_round):
    data, vals = S.lom_message()
    b, first, e, n, _, _ = S.locate(data)
    asm = wire.StreamAssembler(**KW)
    mixed_vals = list(vals)
    mixed_vals[1700] = 1 << 70  # a map among the native items: "jl" for the host scanner, a refusal for the tokenizer
    mixed = U.packb({"node_id": "node-7", "params": mixed_vals, "sample_size": 1234})
    long_later = [data[:3000], data[3000:6000], data[6000:]]
    for name, chunks in (("mixed", S.chunked(mixed, 3000)), ("later-chunk-longer", long_later),
                         ("truncated", S.chunked(data[:e - 1], 3000)), ("trailing", S.chunked(data + b"\x01", 3000))):
        joined = b"".join(chunks)
        before = wire.reference_stats()["stream_fallback"]
        msg = S.stream(asm, chunks)
        assert msg.streamed == (name != "later-chunk-longer"), name
        try:
            want = wire.loads_reference(joined, resident=True, **KW)
        except Exception as err:
            with pytest.raises(type(err)):
                wire.loads_reference(msg, resident=True, **KW)
        else:
            assert name in ("mixed", "later-chunk-longer")
            _same(wire.loads_reference(msg, resident=True, **KW), want)
        st = wire.reference_stats()
        assert st["stream_fallback"] == before + 1 and st["streamed"] == 0 and msg.joins == 1, name
    # a hook that reads the map differently: the array of maps never reaches the device
    def other(o):
        return ("big", o["value"]) if o.get("__type__") == "int" else o

    wire.reference_stats(reset=True)
    kw = dict(KW, object_hook=other)
    msg = S.stream(wire.StreamAssembler(**kw), S.chunked(jl_round["msgs"][0], 3000))
    assert not msg.streamed and msg._rx is None
    got = wire.loads_reference(msg, resident=True, **kw)
    assert got == msgpack.unpackb(jl_round["msgs"][0], object_hook=other, strict_map_key=False)
    st = wire.reference_stats()
    assert (st["streamed"], st["stream_fallback"], st["resident"], st["device_scan_jl"]) == (0, 0, 0, 0)
    assert "devscan" not in st["last"] and "h2d" not in st["last"]


def test_a_jl_and_a_lom_array_in_one_message(dev, jl_round):
    """The first is streamed; the second goes the existing way on the reduced message."""
    words = F.minimal_values(200, seed=4)
    data = U.packb({"a": jl_round["lists"][0], "small": [1, 2, 3], "b": words, "node": "x"})
    kw = dict(KW, min_items=64, device_scan_min_items=64, device_scan_jl_min_items=64)
    want = wire.loads_reference(data, resident=True, **kw)
    wire.reference_stats(reset=True)
    msg = S.stream(wire.StreamAssembler(**kw), S.chunked(data, 4096))
    got = wire.loads_reference(msg, resident=True, **kw)
    _same(got, want)
    a, b = got["a"], got["b"]
    assert (a.scheme, b.scheme) == ("jl", "lom") and a.handle._blk is not b.handle._blk and msg.joins == 0
    st = wire.reference_stats()
    assert (st["streamed"], st["stream_fallback"], st["resident"], st["device_scan"], st["device_scan_jl"]) == (1, 0, 2, 1, 0)


# ---- the oracle's recorded rounds (tests/golden), their replies packed by msgpack and streamed ------------------
def _golden_rounds():
    from tests.golden_util import I, load

    lom = load("lom.json")["crypter"][1]   # three parties of 1000 words
    jl = load("jl.json")["crypter"][3]     # three parties of 4 ciphertexts, a clipping range and a target range
    sweep = [c for c in load("crypter_sweep.json")["jl"] if c["P"] == 3 and all("ok" in e for e in c["enc"]) and "ok" in c["agg"]
             and len(c["enc"][0]["ok"]) == 4][0]  # three parties of 4 ciphertexts: every chunking below is several chunks
    return I, lom, jl, sweep


def _stream_all(kw, msgs, sizes, scheme):
    asm = wire.StreamAssembler(**kw)
    ups = []
    for m, size in zip(msgs, sizes):
        msg = S.stream(asm, S.chunked(m, size))
        assert msg.streamed
        up = wire.loads_reference(msg, resident=True, **kw)["params"]
        assert type(up) is wire.ResidentUpdate and up.scheme == scheme and msg.joins == 0
        ups.append(up)
    return ups


def test_lom_golden_round_streamed_equals_the_oracle(dev):
    from fedbiomed_amd.secagg import SecaggLomCrypter

    I, c, _, _ = _golden_rounds()
    encs = [[I(v) for v in c["enc"][u]] for u in c["ids"]]
    assert len(encs) == 3
    want = [s[2:] for s in c["agg"]]
    msgs = [U.packb({"node": u, "params": e, "n": len(e)}) for u, e in zip(c["ids"], encs)]
    ups = _stream_all(KW, msgs, (4096, 1000, 5001), "lom")
    agg = SecaggLomCrypter("nonce").begin_aggregate(c["total"], clipping_range=c["clip"],
                                                    target_range=I(c["target"]) if c["target"] else None)
    for u in ups:
        agg.add(u)
    from tests.golden_util import fbits

    assert [fbits(v) for v in agg.finish()] == want
    st = wire.reference_stats()
    assert (st["streamed"], st["stream_fallback"], st["resident"], st["device_scan"]) == (3, 0, 3, 0)


def test_jl_golden_rounds_streamed_equal_the_oracle(dev):
    from fedbiomed_amd.secagg import SecaggCrypter
    from tests.golden_util import fbits

    I, _, g, sw = _golden_rounds()
    rounds = [dict(P=g["n_parties"], tau=g["tau"], clip=g["clip"], target=g["target"], total=g["total"], sk0=I(g["sk0"]),
                   biprime=I(g["biprime"]), n=len(g["x"][0]), enc=g["enc"], agg=g["agg"]),
              dict(P=sw["P"], tau=sw["tau"], clip=sw["clip"], target=sw["target"], total=sw["total"],
                   sk0=-sum(I(k) for k in sw["keys"]), biprime=W.BIPRIME0, n=sw["n"], enc=[e["ok"] for e in sw["enc"]],
                   agg=sw["agg"]["ok"])]
    kw = dict(object_hook=U.ref_hook, min_items=1, device_scan_min_items=1, device_scan_jl_min_items=1)
    for c in rounds:
        wire.reference_stats(reset=True)
        encs = [[I(v) for v in e] for e in c["enc"]]
        assert len(encs) == 3 and all(v >= F.M64 for e in encs for v in e)  # every item a map
        msgs = [U.packb({"node": f"n{p}", "params": e}) for p, e in enumerate(encs)]
        assert all(len(m) > 1000 for m in msgs)
        ups = _stream_all(kw, msgs, (100, 333, 600), "jl")  # a few hundred bytes a chunk: the replies are 4 ciphertexts
        target = I(c["target"]) if c["target"] else None
        agg = SecaggCrypter().begin_aggregate(c["tau"], c["P"], c["sk0"], c["biprime"], c["total"], clipping_range=c["clip"],
                                              num_expected_params=c["n"], target_range=target)
        for u in ups:
            agg.add(u)
        assert [fbits(v) for v in agg.finish()] == [s[2:] for s in c["agg"]]
        st = wire.reference_stats()
        assert (st["streamed"], st["stream_fallback"], st["resident"], st["device_scan_jl"]) == (3, 0, 3, 0)


def test_more_chunks_than_staging_buffers(dev):
    """Forty chunks through the ring of four pinned buffers, handed over back to back: a buffer is rewritten only after
    its last copy has finished, or the block would hold a later chunk's bytes where an earlier one belongs."""
    from fedbiomed_amd import _device as D

    vals = S.lom_values(400_000, seed=5)  # about 1.7 MB: chunks of 44 KB, each copy still in flight when the next is staged
    data = U.packb({"node": "n", "params": vals, "n": len(vals)})
    chunks = S.chunked(data, len(data) // 40 + 1)
    assert len(chunks) == 40 > 4 * D.WIRE_STREAM_SLOTS
    msg = S.stream(wire.StreamAssembler(**KW), chunks)
    up = wire.loads_reference(msg, resident=True, **KW)["params"]
    got = D.wire_rows_device(up.handle).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np.array(vals, dtype=np.uint64)) and msg.joins == 0
    assert wire.reference_stats()["streamed"] == 1

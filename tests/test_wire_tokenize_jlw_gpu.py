"""The wide tokenizer on the device against the library's host run, `wire.loads_reference(resident=True, jl_limbs=128)`
through it and `wire.StreamAssembler(jl_limbs=128)`, both folded by `SecaggCrypter.aggregate` and held bit for bit to the
aggregate over msgpack's lists.  On the parent: no "device_scan_jl" counted, a TypeError for the assembler's keyword."""
import random

import numpy as np
import pytest

from fedbiomed_amd import wire
from tests import wire_reference_util as U
from tests.test_jl_wide import MODULI
from tests.test_wire_tokenize_jlw_cpu import GUARD, REFUSED, WHOLE, host_run, item
from tests.wire_stream_util import chunked, stream

pytestmark = pytest.mark.gpu
TAU, PARAMS = 7, 700  # 700 parameters: 31 ciphertexts a reply, four tiles
_REFUSING = {name: b"\xdc\x00\x0e" + b"".join([item(513)] * 10 + [bad] + [item(30)] * 3) for name, bad in REFUSED.items()}
MESSAGES = {**{k: v[0] for k, v in WHOLE.items()}, **_REFUSING, "cut-off": WHOLE["header-straddles"][0][:-5]}


def device_run(span, first, n, head):
    """fbm_wire_tokenize_jlw with span[first] at a device address that is `head` mod 4: host_run's answer shape."""
    import torch
    from fedbiomed_amd import _device as D
    from fedbiomed_amd import _native as N

    lib, dev = N.load(), D.device()
    raw = torch.zeros(len(span) + 16, dtype=torch.uint8, device=dev)
    shift = (head - (raw.data_ptr() + first)) % 4
    raw[shift:shift + len(span)].copy_(torch.from_numpy(np.frombuffer(span, dtype=np.uint8).copy()))
    guard = np.array(GUARD, dtype=np.uint64).view(np.int64).item()
    ck, res = (torch.full((k,), guard, dtype=torch.int64, device=dev) for k in (n + 1, 3))
    ws = torch.zeros(int(lib.fbm_wire_tokenize_jlw_workspace(len(span))), dtype=torch.uint8, device=dev)
    rc = lib.fbm_wire_tokenize_jlw(raw.data_ptr() + shift, len(span), 0, first, n, ck.data_ptr(), n, res.data_ptr(),
                                   ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    ck, res = ck.cpu().numpy().view(np.uint64), res.cpu().numpy().view(np.uint64)  # (the copies synchronise)
    assert ck[n] == GUARD and res[2] == GUARD
    return rc, res[:2].tolist(), ck[:n].tolist()


@pytest.mark.parametrize("name", MESSAGES)
def test_device_tokenizer_equals_the_host_run(name):
    from fedbiomed_amd import _native as N

    data = MESSAGES[name]
    n = int.from_bytes(data[1:3], "big")
    for head in ((0, 1, 2, 3) if len(data) < 100_000 else (3,)):
        rc, res, ck = host_run(N.load_test(), data, 0, 3, n, head)
        assert rc == 0 and (res[0] == n) == (name in WHOLE)
        got = device_run(data, 3, n, head)
        assert (got[0], got[1], got[2][:res[0]]) == (0, res, ck[:res[0]]), head


@pytest.fixture(scope="module")
def replies():
    """Three nodes' wide updates as a stock Serializer writes them, and the aggregate over the lists msgpack unpacks."""
    import torch
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    n, rng, sc = MODULI["p_squared"], random.Random(71), SecaggCrypter()
    keys = [rng.getrandbits(4090) for _ in range(3)]
    cts = [sc.encrypt_tensor(3, TAU, torch.tensor([rng.uniform(-2.5, 2.5) for _ in range(PARAMS)], dtype=torch.float64,
                                                  device=D.device()), k, n) for k in keys]
    packed = [wire.EncryptedParams.from_packed("jlw", D.to_host(c).numpy()) for c in cts]

    def aggregate(params):
        out = sc.aggregate(current_round=TAU, num_nodes=3, params=params, key=-sum(keys), biprime=n, total_sample_size=3,
                           num_expected_params=PARAMS)
        return np.asarray(out, np.float64).tobytes()

    data = wire.dumps_reference({"round": TAU, "params": packed})
    return packed, aggregate, aggregate(U.unpackb(data)["params"]), data


def test_loads_reference_takes_wide_arrays_through_the_tokenizer(replies):
    _, aggregate, want, data = replies
    wire.reference_stats(reset=True)
    ups = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, jl_limbs=128,
                               device_scan_jl_min_items=1)["params"]
    stats = wire.reference_stats()
    assert (stats["device_scan_jl"], stats["device_scan_jl_refused"], stats["fallback"], stats["resident"]) == (3, 0, 0, 3)
    assert [(type(u), u.scheme, len(u)) for u in ups] == [(wire.ResidentUpdate, "jlw", len(replies[0][0]))] * 3
    assert aggregate(ups) == want and not any(u.materialised for u in ups)


@pytest.mark.parametrize("pad", [0, 7000], ids=["header-in-chunk-1", "header-in-chunk-2"])
def test_stream_assembler_takes_a_wide_reply_chunk_by_chunk(replies, pad):
    packed, aggregate, want, _ = replies
    datas = [wire.dumps_reference({"pad": bytes(pad), "params": p, "round": TAU}) for p in packed]
    size = -(-len(datas[0]) // 5)
    assert len(chunked(datas[0], size)) == 5 and datas[0].index(b"\xdc") // size == bool(pad)  # (the array's header: dc 00 1f)
    args = dict(object_hook=U.ref_hook, min_items=1, device_scan_jl_min_items=1)
    wire.reference_stats(reset=True)
    asm, ups = wire.StreamAssembler(jl_limbs=128, **args), []
    for data in datas:
        msg = stream(asm, chunked(data, size))
        ups.append(wire.loads_reference(msg, resident=True, jl_limbs=128, **args)["params"])
        assert msg.streamed and msg.joins == 0 and (type(ups[-1]), ups[-1].scheme) == (wire.ResidentUpdate, "jlw")
    stats = wire.reference_stats(reset=True)
    assert (stats["streamed"], stats["stream_fallback"], stats["fallback"]) == (3, 0, 0)
    assert aggregate(ups) == want
    msg = stream(wire.StreamAssembler(jl_limbs=64, **args), chunked(datas[0], size))  # the assembler's arguments differ
    first = wire.loads_reference(msg, resident=True, jl_limbs=128, **args)["params"]
    assert (wire.reference_stats()["stream_fallback"], wire.reference_stats()["streamed"], msg.joins) == (1, 0, 1)
    assert aggregate([first] + ups[1:]) == want

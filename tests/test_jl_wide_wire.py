"""A stock peer's wide-biprime update (ciphertexts below 2^4096, items of up to 536 bytes) written, read and folded on
the device: `wire.reference_bytes` / `wire.loads_reference(jl_limbs=128)` against msgpack under the reference's rules
(tests/wire_reference_util.py), `D.wire_fold_jlw` against Python's integers and `D.jlw_fold`, `SecaggCrypter.aggregate`
on resident replies against the oracle, and without a GPU the scanner `fbm_wire_scan_jlw` and the kernels' digit
extraction through the library's host run.  On the parent every test here fails with a TypeError (the `jl_limbs`
keyword), an AttributeError (the new entry points) or the ValueError on the scheme."""
import random
import struct

import numpy as np
import pytest

from fedbiomed_amd import _native as N
from fedbiomed_amd import wire
from oracle import secagg_oracle as O
from tests import wire_reference_util as U
from tests.test_jl_wide import MODULI, _limbs

_RNG = random.Random(17)
# seeded full-width values first (an array's first map item makes it "jlw"), then one value of each bit length at the
# encoding's edges -- native forms, the first map form, c4 -> c5 at L = 256, the old bound 2^2048, L = 513 -- and 2^4096 - 1
VALUES = [_RNG.getrandbits(4096) | 1 << 4095 for _ in range(3)] + [(1 << 4096) - 1] + [
    (1 << b - 1 | _RNG.getrandbits(b - 1)) if b else 0
    for b in (0, 7, 8, 63, 64, 65, 2032, 2033, 2040, 2047, 2048, 2049, 4088, 4089, 4095)]


def _map_item(value_bytes: bytes) -> bytes:
    head = b"\xc4" + bytes([len(value_bytes)]) if len(value_bytes) <= 255 else b"\xc5" + struct.pack(">H", len(value_bytes))
    return U.PREFIX + head + value_bytes


def _host_decode(span: bytes, base: int, table, shift: int = 0) -> list:
    """fbm_test_wire_decode_jlw: the kernels' digit extraction run on the host over a copy of the span that begins
    `shift` bytes behind an aligned address."""
    buf, ck = np.zeros(len(span) + 8, dtype=np.uint8)[shift:shift + len(span)], np.array(table, dtype=np.uint64)
    buf[:] = np.frombuffer(span, dtype=np.uint8)
    rows = np.full((ck.size, 128), 0xA5A5A5A5, dtype=np.uint32)
    rc = N.load_test().fbm_test_wire_decode_jlw(buf.ctypes.data, buf.size, base, ck.ctypes.data, ck.size, rows.ctypes.data)
    assert rc == N.FBM_OK, N.last_error()
    return [int.from_bytes(r.tobytes(), "little") for r in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4, 5, 65, 257])
def test_bytes_both_ways(n):
    """One wave, a full workgroup, one past it, a workgroup slot's second round, one past the encoder's tile."""
    import torch
    from fedbiomed_amd import _device as D

    vals = [VALUES[i % len(VALUES)] for i in range(n)]
    data = U.packb(vals)
    if n >= 65:  # the inputs reach every misalignment (voff + vlen) & 3 of a value's end against a dword
        sizes = [len(U.packb([v])) - 1 for v in vals]
        ends = np.cumsum([len(data) - sum(sizes)] + sizes)[1:]
        assert {int(e) & 3 for e in ends} == {0, 1, 2, 3}
    rows = torch.from_numpy(_limbs(vals, 128).copy()).to(D.device())
    assert wire.reference_bytes(rows) == data
    assert wire.reference_bytes(wire.EncryptedParams.from_ints("jlw", vals)) == data
    wire.reference_stats(reset=True)
    got = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, jl_limbs=128)
    assert got == U.unpackb(data) and got.scheme == "jlw" and got.packed.shape == (n, 128)
    assert wire.reference_stats()["fallback"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("mod", MODULI)
def test_fold_from_the_bytes_matches_python(mod):
    """Three resident replies of 65 items folded straight from their bytes, the first seeding: every row Python's
    product mod N^2, and bit for bit D.jlw_fold of the decoded rows.  Nothing is made into ints on the way."""
    import torch
    from fedbiomed_amd import _device as D

    n = MODULI[mod]
    m = n * n
    pool = [0, 1, m - 1, m, (1 << 4096) - 1, 77, random.Random(65).getrandbits(4096)]
    replies = [[pool[(c * (j + 2) + j) % 7] for c in range(65)] for j in range(3)]
    ups = [wire.loads_reference(U.packb(r), object_hook=U.ref_hook, min_items=1, resident=True, jl_limbs=128)
           for r in replies]
    assert [(type(u), u.scheme, len(u)) for u in ups] == [(wire.ResidentUpdate, "jlw", 65)] * 3
    acc = torch.empty((65, 128), dtype=torch.int32, device=D.device())
    for j, u in enumerate(ups):
        D.wire_fold_jlw(u.handle, acc, n, seed_ops=3 if j == 0 else 0)
    assert D.limbs_to_ints_w(acc, 128) == [a * b * c % m for a, b, c in zip(*replies)]
    rows = torch.stack([D.wire_rows_device(u.handle) for u in ups])
    assert torch.equal(acc, D.jlw_fold(torch.empty_like(acc), rows, n, seed_ops=3))
    assert not any(u.materialised for u in ups) and ups[1] == replies[1]


@pytest.mark.gpu
@pytest.mark.parametrize("short", [False, True])
def test_stock_peer_round_trip(short):
    """encrypt_tensor x 3, the message a stock Serializer would have written, read back resident and aggregated: the
    oracle's bytes and floats.  short: the last reply one ciphertext shorter (the reference's zip rule)."""
    import torch
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    n, tau, rng, sc = MODULI["p_squared"], 7, random.Random(70), SecaggCrypter()
    keys = [rng.getrandbits(4090) for _ in range(3)]
    xs = [[rng.uniform(-2.5, 2.5) for _ in range(70)] for _ in range(3)]
    cts = [sc.encrypt_tensor(3, tau, torch.tensor(x, dtype=torch.float64, device=D.device()), k, n) for x, k in zip(xs, keys)]
    want_ct = [O.jl_encrypt(x, tau, k, n, 3) for x, k in zip(xs, keys)]
    if short:
        cts[2], want_ct[2] = cts[2][:-1], want_ct[2][:-1]
    msg = {"round": tau, "params": [wire.EncryptedParams.from_packed("jlw", D.to_host(c).numpy()) for c in cts]}
    data = wire.dumps_reference(msg)
    assert data == U.packb({"round": tau, "params": want_ct})
    wire.reference_stats(reset=True)
    ups = wire.loads_reference(data, object_hook=U.ref_hook, min_items=1, resident=True, jl_limbs=128)["params"]
    assert [(type(u), u.scheme) for u in ups] == [(wire.ResidentUpdate, "jlw")] * 3 and wire.reference_stats()["fallback"] == 0
    got = sc.aggregate(current_round=tau, num_nodes=3, params=ups, key=-sum(keys), biprime=n, total_sample_size=3,
                       num_expected_params=70)
    want = O.jl_crypter_aggregate(want_ct, tau, -sum(keys), n, 3, 70)
    assert np.asarray(got, np.float64).tobytes() == np.asarray(want, np.float64).tobytes()
    assert not any(u.materialised for u in ups)


REFUSED = {"L514": _map_item(bytes(513) + b"\x01"), "L513_nonzero": _map_item(b"\x01" + bytes(512)),
           "sign_byte": _map_item(b"\x80" + bytes(9)), "negative_native": b"\xff", "float": b"\xca\x3f\x80\x00\x00"}


@pytest.mark.parametrize("form", REFUSED)
def test_scan_jlw_refusals(form):
    """An array with one refused item among accepted ones is walked, not recorded, by both scanners."""
    from fedbiomed_amd import _device as D

    data = b"\x92\x93\x07" + REFUSED[form] + _map_item(b"\x00\x01" + bytes(8)) + b"\x93\x01\x02\x03"
    assert len(U.unpackb(data)[0]) == 3  # (well-formed: msgpack reads it)
    for limbs in (128, 64):
        assert [(a[2], a[3]) for a in D.wire_scan(data, 1, jl_limbs=limbs)] == [(3, "lom")]


@pytest.mark.parametrize("value", [b"\x00" + b"\xff" * 512, bytes(257) + b"\x01", b"\x00" + b"\x80" + bytes(255)])
def test_scan_jlw_accepts_what_fbm_wire_scan_refuses(value):
    """L = 513 with a zero first byte, L = 258 and the value 2^2047 at L = 257 (inside the old bound too), behind a
    one-byte map key that shifts the value's alignment; the host run of the digit extraction reads the value back."""
    from fedbiomed_amd import _device as D

    data = b"\x81\x05\x92\x07" + _map_item(value)
    (b, e, n, scheme, ck), = D.wire_scan(data, 1, jl_limbs=128)
    assert (b, e, n, scheme) == (2, len(data), 2, "jlw")
    assert _host_decode(data[b:e], b, ck) == U.unpackb(data)[5]
    assert [a[3] for a in D.wire_scan(data, 1)] == (["jl"] if len(value) <= 257 else [])


def test_host_run_gives_zero_rows_for_a_table_outside_the_span():
    """A checkpoint that begins in front of the span, one whose bytes run past its end, vlen = 514 and vlen = 0 count as
    the value 0; the span's own first and last value decode, at every alignment of the span's address."""
    vals = [VALUES[0], 2**64, VALUES[1]]
    data, base = U.packb(vals), 100
    first, last = 1 + 23, len(data) - 513  # the values' first bytes: header, prefix, c5 + BE16
    good = [(base + first) << 16 | 513, (base + last) << 16 | 513]
    bad = [(base - 1) << 16 | 8, (base + len(data) - 7) << 16 | 8, (base + first) << 16 | 514, (base + first) << 16]
    for shift in range(4):
        assert _host_decode(data, base, good + bad, shift) == [vals[0], vals[2], 0, 0, 0, 0]

"""Shared by tests/test_wire_reference_cpu.py and tests/test_wire_reference_gpu.py: msgpack under the reference
Serializer's rules (`fedbiomed/common/serializer.py:96-110`, `:140-149`, restated as tests/test_wire.py does) --
where every expected byte comes from, never from the code under test -- the values at every boundary of the
encoding, and the library's host run of the per-item routines (include/fbm_secagg_test.h)."""
import ctypes
import math
import random

import msgpack
import numpy as np

from fedbiomed_amd import _native as N

PREFIX = b"\x82\xa8__type__\xa3int\xa5value"  # what msgpack writes before the bin of a big int
NATIVE_EDGES = [0, 127, 128, 255, 256, 65535, 65536, 2**32 - 1, 2**32, 2**64 - 1]
MAP_BITS = [65, 72, 73, 2024, 2025, 2032, 2033, 2040, 2041, 2048]  # bit lengths: L = 10, 10, 11, 254, 255, 255, 256, 256, 257, 257


def ref_default(obj):
    if isinstance(obj, int):
        return {"__type__": "int", "value": obj.to_bytes(length=math.ceil(obj.bit_length() / 8) + 1,
                                                         byteorder="big", signed=True)}
    raise TypeError(f"Cannot serialize object of type '{type(obj)}'.")


def ref_hook(obj):
    if isinstance(obj, dict) and obj.get("__type__") == "int":
        return int.from_bytes(obj["value"], byteorder="big", signed=True)
    return obj


def packb(obj):
    return msgpack.packb(obj, default=ref_default, strict_types=True)


def unpackb(data, hook=ref_hook):
    return msgpack.unpackb(data, object_hook=hook, strict_map_key=False)


def edge_values(seed=5):
    """Every native boundary value, 2^64, and each map bit length at its minimum, its maximum and a random value."""
    rng = random.Random(seed)
    vals = list(NATIVE_EDGES) + [2**64]
    for b in MAP_BITS:
        vals += [1 << (b - 1), (1 << b) - 1, rng.getrandbits(b) | (1 << (b - 1))]
    return vals


def jl_rows(values) -> np.ndarray:
    blob = b"".join(int(v).to_bytes(256, "little") for v in values)
    return np.frombuffer(blob, dtype="<u4").reshape(len(values), 64).copy()


def rows_to_ints(scheme, rows):
    if scheme == "jl":
        return [int.from_bytes(r.tobytes(), "little") for r in np.ascontiguousarray(rows).view(np.uint32).reshape(-1, 64)]
    return np.ascontiguousarray(rows).view(np.uint64).reshape(-1).tolist()


def host_encode(scheme: str, rows) -> bytes:
    """fbm_test_wire_encode: the kernels' per-item routines run on the host."""
    lib = N.load_test()
    sch = N.WIRE_JL if scheme == "jl" else N.WIRE_LOM
    rows = np.ascontiguousarray(rows)
    n = rows.shape[0]
    cap = lib.fbm_wire_encode_bound(sch, n)
    out = np.zeros(cap, dtype=np.uint8)
    total = ctypes.c_uint64(0)
    rc = lib.fbm_test_wire_encode(sch, rows.ctypes.data if n else None, n, out.ctypes.data, cap, ctypes.addressof(total))
    assert rc == N.FBM_OK, N.last_error()
    return out[:total.value].tobytes()


def host_decode(data: bytes, arrays: list) -> list:
    """fbm_test_wire_decode over wire_scan's arrays, the span of each copied out on its own (so a read outside
    it would leave the copy)."""
    lib = N.load_test()
    buf = np.frombuffer(data, dtype=np.uint8)
    out = []
    for b, e, n, scheme, ck in arrays:
        span = buf[b:e].copy()
        ck = np.ascontiguousarray(ck)
        rows = np.full((n, 64), 0xA5A5A5A5, dtype=np.uint32) if scheme == "jl" else np.full(n, 0xA5, dtype=np.uint64)
        rc = lib.fbm_test_wire_decode(N.WIRE_JL if scheme == "jl" else N.WIRE_LOM, span.ctypes.data, e - b, b,
                                      ck.ctypes.data, ck.size, n, rows.ctypes.data)
        assert rc == N.FBM_OK, N.last_error()
        out.append(rows)
    return out

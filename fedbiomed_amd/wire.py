"""Wire format for encrypted model updates.

The reference ships a JL update as a list of Python ints through its msgpack `Serializer`
(`fedbiomed/common/serializer.py:96-110`): every ciphertext >= 2^64 goes through
`Serializer._default` and becomes its own ``{"__type__": "int", "value": <big-endian
bytes>}`` map -- one Python call, one ``to_bytes`` and ~270 bytes of framing per ciphertext
(333 334 of them per party for a 10M-parameter model), and on the researcher one
``object_hook`` call + ``int.from_bytes`` each, then ``int.to_bytes`` again to reach the
device.  A LOM update (uint64 ints) packs natively, but still one msgpack item per element.

`EncryptedParams` is a ``list`` of the same Python ints the reference API returns, which
also carries the device's packed form (JL: ``[n_ct, 64]`` little-endian u32 limbs; LOM:
``[n]`` u64 words).  It is only returned by the crypters once `enable()` has been called --
by default they return plain lists, so an unmodified reference `Serializer` (msgpack with
``strict_types=True`` hands list subclasses to ``_default``, which would refuse them) keeps
working.  With it enabled:

* the maintainer adds two lines to `Serializer._default` / `_object_hook`
  (INTEGRATION.md §Wire format) calling `to_wire` / `from_wire`: one msgpack ``bin`` per
  update instead of one map per ciphertext;
* `SecaggCrypter.aggregate` / `SecaggLomCrypter.aggregate` take the packed form straight to
  the device when every row is an `EncryptedParams` (no ``int.to_bytes`` per ciphertext).

`from_wire` materialises the Python ints as well, so every consumer that treats the update as
``List[int]`` sees exactly the reference's values.

The blob needs the hook on both ends.  Where only one side is patched, `dumps_reference` /
`loads_reference` (below) write and read the reference's own per-item encoding on the device instead,
byte for byte what the stock `Serializer` writes, so the peer needs nothing ("One
patched side"); `reference_stats` counts the updates that took that path and those left to msgpack.  A researcher
that only adds a reply to the aggregate reads it with ``loads_reference(..., resident=True)``: the update comes
back as a `ResidentUpdate` -- its bytes on the device, no rows on the host, no Python ints -- and
`begin_aggregate().add` / `aggregate` fold it from there.

`ChunkAssembler` is the other half of §8(f)2: the gRPC transport streams a serialized message in
chunks of `MAX_MESSAGE_BYTES_LENGTH` (4 MB) and the receiver rebuilds it with ``reply += chunk``
(`fedbiomed/transport/server.py:236-239`, `client.py:599-602` in `_call_researcher`), which copies the growing message at
every chunk -- quadratic in the chunk count (a 10M-parameter JL update is 22-24 chunks).  The
assembler keeps the chunks and joins them once.

`StreamAssembler` is `ChunkAssembler` for the resident path: the same ``add`` in the transport's loop, but the reply's
large integer array goes up to the device and is tokenized there chunk by chunk while the transport delivers the
message, so that behind the last chunk neither the join nor the upload is left; `loads_reference` takes the
`StreamedMessage` it returns where it takes ``bytes``.
"""

from __future__ import annotations

import logging
from typing import Any, Dict, Iterable, Optional

import numpy as np

_log = logging.getLogger(__name__)  # the causes of `StreamAssembler`'s fallbacks (a counter alone would hide a device error)
WIRE_TYPE = "fedbiomed_amd.EncryptedParams"
_ENABLED = False


def enable(on: bool = True) -> None:
    """Make the crypters return `EncryptedParams` (call once the Serializer hook is in)."""
    global _ENABLED
    _ENABLED = bool(on)


def enabled() -> bool:
    return _ENABLED


class EncryptedParams(list):
    """A reference-compatible ``List[int]`` update plus its packed device form.

    scheme "jl": ``packed`` is uint32 ``[n_ct, 64]`` (ciphertext k = little-endian limbs);
    scheme "lom": ``packed`` is uint64 ``[n]``.
    """

    __slots__ = ("scheme", "packed")

    def __init__(self, values: Iterable[int], scheme: str, packed: np.ndarray):
        super().__init__(values)
        if scheme not in ("jl", "lom"):
            raise ValueError("scheme must be 'jl' or 'lom'")
        self.scheme = scheme
        self.packed = packed

    @classmethod
    def from_ints(cls, scheme: str, values) -> "EncryptedParams":
        """Pack a plain update (JL ciphertexts must lie in [0, 2^2048), LOM words in [0, 2^64))."""
        values = [int(v) for v in values]
        if scheme == "jl":
            blob = b"".join(v.to_bytes(256, "little") for v in values)
            packed = np.frombuffer(blob, dtype="<u4").reshape(len(values), 64).copy()
        else:
            packed = np.array(values, dtype=np.uint64)
        return cls(values, scheme, packed)

    @classmethod
    def from_packed(cls, scheme: str, packed: np.ndarray) -> "EncryptedParams":
        packed = np.ascontiguousarray(packed)
        if scheme == "jl":
            from . import _device as D  # (the C conversion module: the ints' digits written on host threads)

            packed = packed.view(np.uint32).reshape(-1, 64)
            values = D.limbs_to_ints(packed)
        else:
            packed = packed.view(np.uint64).reshape(-1)
            values = packed.tolist()
        return cls(values, scheme, packed)

    def _drop(self) -> None:
        self.packed = None  # mutated: the ints are the truth from now on

    def __setitem__(self, i, v):
        self._drop()
        super().__setitem__(i, v)

    def __delitem__(self, i):
        self._drop()
        super().__delitem__(i)

    def __iadd__(self, other):
        self._drop()
        return super().__iadd__(other)

    def __imul__(self, k):
        self._drop()
        return super().__imul__(k)

    def _mutator(name):  # noqa: N805 - class-body helper
        def f(self, *a, **k):
            self._drop()
            return getattr(list, name)(self, *a, **k)
        f.__name__ = name
        return f

    append = _mutator("append")
    extend = _mutator("extend")
    insert = _mutator("insert")
    pop = _mutator("pop")
    remove = _mutator("remove")
    clear = _mutator("clear")
    sort = _mutator("sort")
    reverse = _mutator("reverse")
    del _mutator

    def consistent(self) -> bool:
        """True while the packed form still mirrors the list (every mutating list method
        drops it; the aggregate then converts the ints like a plain list)."""
        return self.packed is not None and self.packed.shape[0] == len(self)

    def to_wire(self) -> Dict[str, Any]:
        """The Serializer-hook form: one msgpack map holding one bin."""
        if not self.consistent():  # mutated: re-pack from the ints
            self.packed = (EncryptedParams.from_ints(self.scheme, list(self)).packed)
        return {"__type__": WIRE_TYPE, "value": [self.scheme, self.packed.dtype.str, list(self.packed.shape),
                                                 self.packed.tobytes()]}


def to_wire(obj: Any) -> Optional[Dict[str, Any]]:
    """For `Serializer._default`: the wire map of an `EncryptedParams`, else None."""
    return obj.to_wire() if isinstance(obj, EncryptedParams) else None


def from_wire(obj: Any) -> Any:
    """For `Serializer._object_hook`: rebuild an `EncryptedParams` from its wire map
    (anything else is returned unchanged)."""
    if isinstance(obj, dict) and obj.get("__type__") == WIRE_TYPE:
        scheme, dtype, shape, data = obj["value"]
        if scheme not in ("jl", "lom") or np.dtype(dtype) not in (np.dtype("<u4"), np.dtype("<u8")):
            raise ValueError("malformed EncryptedParams wire map")
        arr = np.frombuffer(data, dtype=np.dtype(dtype)).reshape(shape).copy()
        return EncryptedParams.from_packed(scheme, arr)
    return obj


def packed_rows(params, scheme: str, n: Optional[int] = None) -> Optional[np.ndarray]:
    """The stacked packed form of an aggregate's rows when every row is a consistent
    `EncryptedParams` of `scheme` (first `n` entries of each), else None."""
    if not params or not all(isinstance(p, EncryptedParams) and p.scheme == scheme for p in params):
        return None
    if not all(p.consistent() for p in params):
        return None
    if n is None:  # LOM: rows must agree in length (the reference's np.array raises otherwise)
        if len({len(p) for p in params}) != 1:
            return None
        n = len(params[0])
    return np.stack([p.packed[:n] for p in params])


class ChunkAssembler:
    """Rebuilds a message streamed as chunks numbered ``iteration`` = 1 .. ``size`` (the transport's
    `TaskResult` / `TaskResponse` fields) in linear time.  ``add`` returns the whole message on its last
    chunk (``iteration == size``, the reference's completion test) and None before; the assembler is
    then empty for the next message, as the reference's loop is after ``Serializer.loads``."""

    __slots__ = ("_parts",)

    def __init__(self) -> None:
        self._parts: list = []

    def add(self, chunk: bytes, size: int, iteration: int) -> Optional[bytes]:
        self._parts.append(chunk)
        if size != iteration:
            return None
        out = b"".join(self._parts)
        self._parts = []
        return out


# ---- one patched side: the reference's own bytes, made and read on the device -----------------------
# A stock peer speaks only the reference Serializer's encoding (`fedbiomed/common/serializer.py:96-110`,
# `:140-149`): one msgpack item per ciphertext / element.  `dumps_reference` / `loads_reference` produce and
# consume exactly those bytes from the packed device form (the C ABI's fbm_wire_encode / fbm_wire_scan /
# fbm_wire_decode), so only this side needs its two Serializer lines ("One patched side").
_STATS = {"fast": 0, "fallback": 0, "resident": 0, "device_scan": 0, "device_scan_refused": 0, "device_scan_jl": 0,
          "device_scan_jl_refused": 0, "streamed": 0, "stream_fallback": 0}
# `loads_reference(resident=True)` leaves an all-native array of at least this many items to the device tokenizer
# (fbm_wire_tokenize_lom) instead of the host scanner's walk: the smallest power of two from which on the device
# route's take was the faster one on an MI355X (tools/wire_ref_ab.py --devscan, profiles/wire_devscan_ab.jsonl,
# 0.71 ms against 0.76 here, 1.3 against 2.8 at 2^20, 10.1 against 38.1 at 2^24).
DEVICE_SCAN_MIN_ITEMS = 1 << 16
# The same for an array of at least this many big-int maps (a JL update; fbm_wire_tokenize_jl): the smallest power of
# two from which on the device route's median take was the lower one (tools/wire_ref_ab.py --devscan-jl,
# profiles/wire_devscan_jl_ab.jsonl, DESIGN.md 4.2: 0.95 ms against 1.00 here, 2.8 against 4.0 at 2^17, 8.8 against
# 14.6 at 2^19).
DEVICE_SCAN_JL_MIN_ITEMS = 1 << 14
_LAST: Dict[str, Any] = {}  # the last call's phases in seconds (tools/wire_ref_ab.py)
_PHASE_TIMING = False  # tools/wire_ref_ab.py sets it: the resident upload then synchronises to time its "h2d"


def reference_stats(reset: bool = False) -> Dict[str, Any]:
    """Updates that took the device path ("fast"), updates that stayed on the device (`loads_reference` with
    ``resident=True``: "resident") and updates or messages that took msgpack's ("fallback") since the last
    reset, the arrays whose table the device made ("device_scan") and those its tokenizer refused, which the host
    scanner then walked ("device_scan_refused") -- both count all-native arrays; "device_scan_jl" and
    "device_scan_jl_refused" count the arrays of big-int maps in the same way --, the arrays whose bytes and table
    were on the device when their message's last chunk came (`StreamAssembler`: "streamed") and the messages that
    began to go up that way and were then read from their joined bytes ("stream_fallback"), and the last call's phase times
    ("last": scan / h2d / devscan / kernel / d2h seconds; devscan covers both tokenizers)."""
    out = dict(_STATS, last=dict(_LAST))
    if reset:
        _STATS.update(fast=0, fallback=0, resident=0, device_scan=0, device_scan_refused=0, device_scan_jl=0,
                      device_scan_jl_refused=0, streamed=0, stream_fallback=0)
        _LAST.clear()
    return out


class ResidentUpdate:
    """An update `loads_reference(..., resident=True)` read: its bytes and the scanner's table on the device, no
    rows decoded and no Python int made.  `begin_aggregate().add` and `aggregate` fold it from there.  Not a
    list, but a consumer that treats it as the reference's ``List[int]`` (iteration, indexing, ``==``) still
    sees exactly those values: the first such use decodes, copies back and builds the ints (`tolist`, once).
    `release` drops the device bytes; what needs them afterwards raises RuntimeError."""

    __slots__ = ("scheme", "n_items", "_handle", "_values")

    def __init__(self, scheme: str, n_items: int, handle):
        if scheme not in ("jl", "lom"):
            raise ValueError("scheme must be 'jl' or 'lom'")
        self.scheme, self.n_items, self._handle, self._values = scheme, int(n_items), handle, None

    @property
    def handle(self):
        """The device handle (`_device.WireHandle`) `_device.wire_fold_lom` / `wire_rows_device` take."""
        if self._handle is None or self._handle.released:
            raise RuntimeError("this ResidentUpdate's device bytes have been released")
        return self._handle

    @property
    def materialised(self) -> bool:
        """Whether the Python ints have been made."""
        return self._values is not None

    def tolist(self) -> list:
        """The reference's ints: what `EncryptedParams.from_packed` holds for the same rows.  Made once."""
        if self._values is None:
            self._values = list(EncryptedParams.from_packed(self.scheme, self.handle.rows_host()))
        return self._values

    def release(self) -> None:
        if self._handle is not None:
            self._handle.release()
        self._handle = None

    def __len__(self) -> int:
        return self.n_items

    def __iter__(self):
        return iter(self.tolist())

    def __getitem__(self, i):
        return self.tolist()[i]

    def __eq__(self, other):
        if isinstance(other, ResidentUpdate):
            other = other.tolist()
        return self.tolist() == other if isinstance(other, list) else NotImplemented

    __hash__ = None

    def __repr__(self) -> str:
        return f"ResidentUpdate(scheme={self.scheme!r}, n_items={self.n_items}, materialised={self.materialised})"


def _reference_default(obj: Any) -> Dict[str, Any]:
    """The reference's `Serializer._default` rule for ints (serializer.py:103-110)."""
    if isinstance(obj, int):
        return {"__type__": "int", "value": obj.to_bytes(length=(obj.bit_length() + 7) // 8 + 1, byteorder="big",
                                                         signed=True)}
    raise TypeError(f"Cannot serialize object of type '{type(obj)}'.")


def _encode_rows(scheme: str, rows) -> bytes:
    """The device call of `reference_bytes` (a seam: the CPU tests put the library's host run here)."""
    from . import _device as D

    timing: Dict[str, float] = {}
    data = D.wire_encode(scheme, rows, timing)
    for k, v in timing.items():
        _LAST[k] = _LAST.get(k, 0.0) + v
    return data


def _decode_arrays(data: bytes, arrays: list) -> list:
    """The device call of `loads_reference` (the same seam)."""
    from . import _device as D

    timing: Dict[str, float] = {}
    rows = D.wire_decode(data, arrays, timing)
    _LAST.update(timing)
    return rows


def reference_bytes(update) -> bytes:
    """Exactly ``msgpack.packb(list_of_ints, default=<reference _default>, strict_types=True)`` for a consistent
    `EncryptedParams` or a device tensor in either layout (int32 ``[n_ct, 64]``: JL; int64 ``[n]``: LOM), made on
    the device.  An `EncryptedParams` whose packed form was dropped goes through msgpack like a plain list."""
    if isinstance(update, EncryptedParams):
        if update.consistent():
            _STATS["fast"] += 1
            return _encode_rows(update.scheme, update.packed)
        import msgpack

        _STATS["fallback"] += 1
        return msgpack.packb(list(update), default=_reference_default, strict_types=True)
    import torch

    if isinstance(update, torch.Tensor) and update.is_cuda:
        if update.dtype == torch.int32 and update.dim() == 2 and update.shape[1] == 64:
            scheme = "jl"
        elif update.dtype == torch.int64 and update.dim() == 1:
            scheme = "lom"
        else:
            raise ValueError("reference_bytes takes int32 [n_ct, 64] (JL) or int64 [n] (LOM) device tensors")
        _STATS["fast"] += 1
        return _encode_rows(scheme, update)
    raise TypeError("reference_bytes takes an EncryptedParams or a device tensor")


def dumps_reference(obj: Any, default=None) -> bytes:
    """`Serializer.dumps` for a message that holds `EncryptedParams`: byte for byte what
    ``packb(obj, default=default, strict_types=True)`` gives for the same message holding plain lists
    (`default`: the Serializer's own `_default`; None: the reference's int rule).  Each consistent
    `EncryptedParams` goes to the packer as a bin of 16 random bytes, which is then replaced by
    `reference_bytes` of that update; a placeholder that does not occur exactly once (the message itself holds
    those 18 bytes) is drawn again."""
    import os

    import msgpack

    _LAST.clear()
    inner = default or _reference_default
    for _ in range(8):
        held: Dict[bytes, EncryptedParams] = {}

        def wrapped(o):
            if isinstance(o, EncryptedParams):
                if o.consistent():
                    tok = os.urandom(16)
                    held[tok] = o
                    return tok
                _STATS["fallback"] += 1
                return list(o)
            return inner(o)

        fb = _STATS["fallback"]
        body = msgpack.packb(obj, default=wrapped, strict_types=True)
        marks = {tok: b"\xc4\x10" + tok for tok in held}
        if all(body.count(m) == 1 for m in marks.values()):
            break
        _STATS["fallback"] = fb  # (counted again on the retry)
    else:
        raise RuntimeError("dumps_reference: no unique placeholder in 8 draws")
    if not held:
        return body
    order = sorted((body.index(m), tok) for tok, m in marks.items())
    parts, pos = [], 0
    for at, tok in order:
        parts += [body[pos:at], reference_bytes(held[tok])]
        pos = at + 18
    parts.append(body[pos:])
    return b"".join(parts)


def _hook_reads_ints(object_hook) -> bool:
    """Whether `object_hook` turns the reference's int map into the int (serializer.py:140-149): only then
    does an array of those maps unpack to the ints a "jl" `EncryptedParams` holds."""
    if object_hook is None:
        return False
    try:
        v = object_hook({"__type__": "int", "value": b"\x00\x80" + bytes(8)})
    except Exception:
        return False
    return type(v) is int and v == 1 << 71


def _upload_arrays(data: bytes, arrays: list) -> list:
    """The device call of `loads_reference(resident=True)` (the same seam): one handle per array, with
    ``rows_host()``, ``release()`` and ``released``."""
    from . import _device as D

    if not _PHASE_TIMING:  # nothing waits for the upload here: the consumers' streams do, through its event
        return D.wire_upload(data, arrays)
    timing: Dict[str, float] = {}
    handles = D.wire_upload(data, arrays, timing)
    _LAST.update(timing)
    return handles


def _scan_resident(data: bytes, min_items: int, defer_items: int, defer_jl_items: int = 0):
    """The scan of `loads_reference(resident=True)` (the same seam): `_device.wire_scan_resident`'s (arrays, handles)."""
    from . import _device as D

    timing: Dict[str, float] = {}
    out = D.wire_scan_resident(data, min_items, defer_items, timing, _STATS, sync_phases=_PHASE_TIMING,
                               defer_jl_items=defer_jl_items)
    _LAST.update(timing)
    return out


# ---- a stock peer's reply taken onto the device chunk by chunk as it arrives -------------------------------------
def _scan_prefix(data: bytes, min_items: int, defer_items: int, defer_jl_items: int):
    """The host's prefix scan of `StreamAssembler` (a seam like the others): `_device.wire_scan_prefix`."""
    from . import _device as D

    return D.wire_scan_prefix(data, min_items, defer_items, defer_jl_items)


def _open_stream(scheme: str, begin: int, first: int, n_items: int, cap: int, ctx: dict):
    """The device side of `StreamAssembler` (the same seam): a `_device.WireStream` -- ``push(chunk, offset, last)``,
    ``result()``, ``handle(end)``, ``abort()``, ``failed``."""
    from . import _device as D

    return D.WireStream(scheme, begin, first, n_items, cap, ctx)


def _part_slices(parts: list, lo: int, hi: int) -> list:
    """The bytes [lo, hi) of the chunks `parts` as slices of them, nothing joined."""
    out, pos = [], 0
    for p in parts:
        a, b = max(lo - pos, 0), min(hi - pos, len(p))
        if a < b:
            out.append(memoryview(p)[a:b])
        pos += len(p)
    return out


class StreamedMessage:
    """What `StreamAssembler.add` returns on a message's last chunk: the chunks as they came, and, where an array of
    the message went up while they arrived (`streamed`), the device block, table and tokenizer state of that array.
    ``bytes(msg)`` joins the chunks, once (`joins` counts it); `loads_reference` takes the message itself and, for a
    streamed one read with ``resident=True`` and the assembler's arguments, never joins."""

    __slots__ = ("_parts", "_len", "_joined", "joins", "_rx", "_cand", "_params", "_began", "_counted")

    def __init__(self, parts: list, rx=None, cand=None, params=None, began: bool = False):
        self._parts, self._len, self._joined, self.joins = parts, sum(len(p) for p in parts), None, 0
        self._rx, self._cand, self._params, self._began, self._counted = rx, cand, params, began, False

    def __len__(self) -> int:
        return self._len

    def __bytes__(self) -> bytes:
        if self._joined is None:
            self._joined = b"".join(self._parts)
            self.joins += 1
        return self._joined

    @property
    def streamed(self) -> bool:
        """Whether the device holds the message's array and the table the tokenizer made while the chunks came."""
        return self._rx is not None and not self._rx.failed

    def _fell_back(self) -> None:
        if self._began and not self._counted:
            _STATS["stream_fallback"] += 1
            self._counted = True
        if self._rx is not None:
            self._rx.abort()
            self._rx = None


class StreamAssembler:
    """`ChunkAssembler` for a researcher that reads the reply with ``loads_reference(msg, resident=True)``: the same
    ``add(chunk, size, iteration)`` in the transport's loop, chunks in arrival order, ``iteration == size`` the
    completion test, None before the last chunk -- and on it a `StreamedMessage`, not ``bytes``.

    While the chunks arrive the message's first large integer array goes up and is tokenized behind the wait for the
    next chunk.  The chunks are kept as they come.  After each of the first four the host's prefix scanner
    (fbm_wire_scan_prefix) looks for the array `loads_reference` would leave to a device tokenizer first: at least
    ``max(min_items, device_scan_min_items)`` native items, or, under an `object_hook` that reads the reference's int
    map, ``max(min_items, device_scan_jl_min_items)`` of those maps (the arguments and defaults are
    `loads_reference`'s; they are needed when the first chunk arrives, and a `loads_reference` call with other
    values reads ``bytes(msg)``).  Until one is found no device call is made; a message of one chunk, one without such
    an array in its first four chunks and a malformed one are kept as `ChunkAssembler` keeps them.  Once it is known
    a device block takes the message from the array's header on -- ``size * len(first chunk)`` bytes bound it: the
    reference's sender cuts every chunk but the last to ``MAX_MESSAGE_BYTES_LENGTH`` --, the kept chunks and then
    every further one go up through a pinned staging ring on a stream the assembler owns, and after each upload the
    tokenizer is fed the tiles that have become final (fbm_wire_stream_feed).  `add` never synchronises the device.
    A chunk that does not fit the block ends streaming for the message, and so does anything the device side raises;
    a message whose announced ``size`` asks for a block of more than `max_block_bytes` (1 GiB: ten times the largest
    reply of a 10M-parameter model) or for more device memory than there is is not streamed at all -- `add` keeps
    the chunks as `ChunkAssembler` does, whatever the peer announces.  (Where the first chunk does not
    decide, the scan runs over a growing copy of the chunks so far, each of the first four copied into it once; the
    message itself is never joined here.  What ends streaming is logged under this module's logger.)"""

    def __init__(self, object_hook=None, min_items: int = 1024, device_scan_min_items: Optional[int] = None,
                 device_scan_jl_min_items: Optional[int] = None, max_block_bytes: int = 1 << 30) -> None:
        self._max_block = int(max_block_bytes)
        dmin = DEVICE_SCAN_MIN_ITEMS if device_scan_min_items is None else int(device_scan_min_items)
        jmin = DEVICE_SCAN_JL_MIN_ITEMS if device_scan_jl_min_items is None else int(device_scan_jl_min_items)
        self._params = (object_hook, int(min_items), dmin, jmin)
        self._jl = _hook_reads_ints(object_hook)
        self._ctx: dict = {}  # the device side's stream and staging ring, kept from message to message
        self._reset()

    def _reset(self) -> None:
        self._parts: list = []
        self._got, self._rx, self._cand, self._looking, self._began = 0, None, None, True, False
        self._prefix: Optional[bytearray] = None  # the chunks so far, while the prefix scan still asks for more

    def _look(self, size: int) -> None:
        """After one of the first four chunks: the prefix scan, and where it finds the array, the device block."""
        _, min_items, dmin, jmin = self._params
        if len(self._parts) == 1:
            prefix = self._parts[0]
        else:  # (rare: the array begins behind the first chunk.  Each chunk is copied once into the growing prefix)
            if self._prefix is None:
                self._prefix = bytearray(self._parts[0])
            self._prefix += self._parts[-1]
            prefix = self._prefix
        kind, cand = _scan_prefix(prefix, min_items, max(dmin, 1), max(jmin, 1) if self._jl else 0)
        if kind != "more" or len(self._parts) >= 4:
            self._prefix = None
        if kind == "more":
            return
        self._looking = False
        if kind != "pending":
            return
        begin, first, n_items, scheme = cand
        cap = size * len(self._parts[0])
        # (deferred2's bound, which the prefix cannot see: the items at their smallest fit what is still to come)
        if n_items * (23 if scheme == "jl" else 1) > cap - first:
            return
        if cap - begin > self._max_block:
            return
        try:
            rx = _open_stream(scheme, begin, first, n_items, cap, self._ctx)
        except Exception as err:  # (no device memory for a block of the announced size, ...): the plain assembler's message
            _log.warning("StreamAssembler: the device side did not open (%s: %s); the message is kept on the host",
                         type(err).__name__, err)
            return
        self._began, self._cand, self._rx = True, cand, rx
        pos = 0
        for p in self._parts[:-1]:
            self._push(p, pos, False)
            pos += len(p)

    def _push(self, chunk, offset: int, last: bool) -> None:
        """One chunk to the device side; whatever it raises ends streaming for this message, never `add`."""
        try:
            self._rx.push(chunk, offset, last)
        except Exception as err:
            _log.warning("StreamAssembler: streaming ended for this message (%s: %s); it will be read from its joined bytes",
                         type(err).__name__, err)
            self._rx.abort()

    def add(self, chunk: bytes, size: int, iteration: int):
        self._parts.append(chunk)
        last = size == iteration
        if self._looking and size > 1:
            self._looking = len(self._parts) < 4  # (set before the look: an exception there does not bring it back)
            self._look(size)
        elif size == 1:
            self._looking = False
        if self._rx is not None and not self._rx.failed:
            self._push(chunk, self._got, last)
        self._got += len(chunk)
        if not last:
            return None
        msg = StreamedMessage(self._parts, self._rx, self._cand, self._params, self._began)
        self._reset()
        return msg


_NOT_STREAMED = object()


def _loads_streamed(msg: StreamedMessage, object_hook, min_items: int, resident: bool, dmin: int, jmin: int):
    """`loads_reference` of a streamed message without joining it, or _NOT_STREAMED where the call is the one on
    ``bytes(msg)``: read without ``resident``, with other arguments than the assembler's, refused by the tokenizer, or
    with a reduced message that does not unpack."""
    import os

    import msgpack

    if not msg._began:
        return _NOT_STREAMED
    if not resident or not msg.streamed or msg._params != (object_hook, int(min_items), dmin, jmin):
        msg._fell_back()
        return _NOT_STREAMED
    begin, first, n_items, scheme = msg._cand
    got, end = msg._rx.result()
    if got != n_items or not first < end <= len(msg):
        msg._fell_back()
        return _NOT_STREAMED
    token = "fedbiomed_amd.stream." + os.urandom(12).hex()
    reduced = b"".join(_part_slices(msg._parts, 0, begin) + [msgpack.packb({"__type__": token, "value": 0})] +
                       _part_slices(msg._parts, end, len(msg)))
    handle = msg._rx.handle(end)

    def hook(o):
        if o.get("__type__") == token:
            _STATS["resident"] += 1
            _STATS["streamed"] += 1
            return ResidentUpdate(scheme, n_items, handle)
        return o if object_hook is None else object_hook(o)

    before = dict(_STATS)
    try:
        return _loads_reference(reduced, hook, min_items, True, dmin, jmin, count_plain=False)
    except Exception as err:  # what msgpack raises for the reduced message it raises for the whole one: that call decides
        _log.info("loads_reference: the streamed message did not unpack (%s: %s); reading its joined bytes", type(err).__name__, err)
        _STATS.update(before)
        msg._fell_back()
        return _NOT_STREAMED


def loads_reference(data, object_hook=None, min_items: int = 1024, resident: bool = False,
                    device_scan_min_items: Optional[int] = None, device_scan_jl_min_items: Optional[int] = None) -> Any:
    """``msgpack.unpackb(data, object_hook=object_hook, strict_map_key=False)`` with every integer array of at
    least `min_items` items the host scanner records read on the device: it comes back as an `EncryptedParams`
    (which compares as the list of ints msgpack would have made) whose ``packed`` is ready for `aggregate` /
    `begin_aggregate().add`.  Arrays the scanner refuses stay msgpack's; where it records nothing or gives up,
    this is exactly that call.  (Arrays of the big-int map are taken only when `object_hook` reads that map as
    the reference's does.)

    ``resident=True``: each recorded array comes back as a `ResidentUpdate` instead -- its bytes uploaded, nothing
    decoded, copied back or made into ints; `begin_aggregate().add` and `aggregate` fold it on the device.  An
    array of at least `device_scan_min_items` native items (None: `DEVICE_SCAN_MIN_ITEMS`; a value past any array's
    size disables it) is not walked by the host scanner: the message goes up from that array's header on and the
    device finds the items' starts (`reference_stats` counts "device_scan"); what its tokenizer refuses -- an array
    that is not all native, such as a JL update whose first ciphertext is below 2^64 -- takes the host walk as
    before ("device_scan_refused").  An array of at least `device_scan_jl_min_items` big-int maps (None:
    `DEVICE_SCAN_JL_MIN_ITEMS`) goes the same way through the tokenizer for that form ("device_scan_jl"; a mixed
    array is refused and walked on the host: "device_scan_jl_refused") -- only where `object_hook` reads the map as
    the reference's does.  ``resident=False`` keeps the host scan: its cost is the Python ints.

    `data` may be a `StreamedMessage` (`StreamAssembler`): the result is that of the same call on ``bytes(data)``.
    Where an array of it went up while its chunks arrived and the call has ``resident=True`` and the assembler's
    arguments, the chunks are not joined and that array is not uploaded again: the tokenizer's two result words come
    back (the one synchronising copy), the message without the array -- its head, a token and its tail, from the
    chunks' slices -- is read as above (a further large array in the tail goes the usual way), and the array comes
    back as a `ResidentUpdate` on the streamed block and table (`reference_stats` counts "streamed").  An array the
    tokenizer refuses (mixed, a negative int, cut off by the message's end) and a reduced message that does not
    unpack make this the call on ``bytes(data)``, with that call's result or error ("stream_fallback")."""
    dmin = DEVICE_SCAN_MIN_ITEMS if device_scan_min_items is None else int(device_scan_min_items)
    jmin = DEVICE_SCAN_JL_MIN_ITEMS if device_scan_jl_min_items is None else int(device_scan_jl_min_items)
    if isinstance(data, StreamedMessage):
        out = _loads_streamed(data, object_hook, min_items, resident, dmin, jmin)
        if out is not _NOT_STREAMED:
            return out
        data = bytes(data)
    return _loads_reference(data, object_hook, min_items, resident, dmin, jmin)


def _loads_reference(data: bytes, object_hook, min_items: int, resident: bool, dmin: int, jmin: int,
                     count_plain: bool = True) -> Any:
    """`loads_reference` for ``bytes``; count_plain: whether a message without arrays counts as "fallback"."""
    import os
    import time

    import msgpack

    from . import _device as D

    _LAST.clear()
    held: Dict[int, Any] = {}  # the arrays the device tokenized: index -> handle
    if resident:
        # (an array of maps is this library's only under a hook that reads them: otherwise it never goes up)
        arrays, held = _scan_resident(data, min_items, max(dmin, 1), max(jmin, 1) if _hook_reads_ints(object_hook) else 0)
    else:
        t0 = time.perf_counter()
        arrays = D.wire_scan(data, min_items)
        _LAST["scan"] = time.perf_counter() - t0
    if arrays and not _hook_reads_ints(object_hook):
        keep = [i for i, a in enumerate(arrays) if a[3] != "jl"]  # (a tokenized "jl" array exists only under such a hook)
        arrays, held = [arrays[i] for i in keep], {k: held[i] for k, i in enumerate(keep) if i in held}
    if not arrays:
        _STATS["fallback"] += 1 if count_plain else 0
        return msgpack.unpackb(data, object_hook=object_hook, strict_map_key=False)
    if resident:  # the arrays the scan recorded the old way go up with their host tables in a block of their own
        rest = [i for i in range(len(arrays)) if i not in held]
        rows = dict(held)
        if rest:
            before = _LAST.pop("h2d", None)  # (the tokenized arrays' upload)
            rows.update(zip(rest, _upload_arrays(data, [arrays[i] for i in rest])))
            if before is not None:
                _LAST["h2d"] = _LAST.get("h2d", 0.0) + before
    else:
        rows = _decode_arrays(data, arrays)
    token = "fedbiomed_amd.ref." + os.urandom(12).hex()
    view = memoryview(data)
    parts, pos = [], 0
    for i, (b, e, _, _, _) in enumerate(arrays):
        parts += [view[pos:b], msgpack.packb({"__type__": token, "value": i})]
        pos = e
    parts.append(view[pos:])

    def hook(o):
        if o.get("__type__") == token:
            i = o["value"]
            if resident:
                _STATS["resident"] += 1
                return ResidentUpdate(arrays[i][3], arrays[i][2], rows[i])
            _STATS["fast"] += 1
            return EncryptedParams.from_packed(arrays[i][3], rows[i])
        return o if object_hook is None else object_hook(o)

    return msgpack.unpackb(b"".join(parts), object_hook=hook, strict_map_key=False)

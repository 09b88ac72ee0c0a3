#!/usr/bin/env python
"""A/B of the reference Serializer's encoding made and read on the device against msgpack itself.

One node's 10M-element update per scheme -- JL: ceil(10M / 30) = 333 334 ciphertexts of 2 048 bits (about one in
256 a byte shorter); LOM: 10M uint64 words -- inside a message `{"node_id": ..., "params": update, "n": ...}`:

  leg          new                                      reference (msgpack under the reference's rules)
  jl_dumps     wire.dumps_reference(EncryptedParams)    packb(list of ints, default=_default, strict_types=True)
  jl_loads     wire.loads_reference(bytes, hook)        unpackb(bytes, object_hook=_object_hook, strict_map_key=False)
  lom_dumps / lom_loads likewise

Alternating new / reference, five runs of each per leg, one process, one session.  Every run is one JSON line in
profiles/wire_reference_ab.jsonl with its wall time and, for the new side, the phases (`scan`: the host scanner,
`h2d`: staging + upload, `kernel`, `d2h`: download + the bytes object; the remainder is msgpack on the message
without the update, the splice and -- on loads -- `EncryptedParams.from_packed`'s Python ints).  The last line
is the summary and the condition fixed in advance: per leg, the slowest new run is faster than the fastest
reference run.  Both sides' outputs are compared before anything is timed.

    python tools/wire_ref_ab.py [--elements 10000000] [--runs 5] [--out profiles/wire_reference_ab.jsonl]
"""
import argparse
import gc
import json
import math
import os
import sys
import time

import msgpack
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from fedbiomed_amd import wire  # noqa: E402


def ref_default(obj):
    if isinstance(obj, int):
        return {"__type__": "int", "value": obj.to_bytes(length=math.ceil(obj.bit_length() / 8) + 1,
                                                         byteorder="big", signed=True)}
    raise TypeError(f"Cannot serialize object of type '{type(obj)}'.")


def ref_hook(obj):
    if isinstance(obj, dict) and obj.get("__type__") == "int":
        return int.from_bytes(obj["value"], byteorder="big", signed=True)
    return obj


def timed(fn):
    gc.collect()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wire_reference_ab.jsonl"))
    a = ap.parse_args()

    from fedbiomed_amd import _device as D

    D.device()
    rng = np.random.default_rng(2026)
    n_ct = -(-a.elements // 30)
    updates = {
        "jl": wire.EncryptedParams.from_packed("jl", rng.integers(0, 2**32, size=(n_ct, 64), dtype=np.uint64).astype(np.uint32)),
        "lom": wire.EncryptedParams.from_packed("lom", rng.integers(0, 2**64, size=a.elements, dtype=np.uint64)),
    }
    lines, legs = [], {}
    for scheme, upd in updates.items():
        msg_new = {"node_id": "node-00", "params": upd, "n": len(upd)}
        msg_ref = {"node_id": "node-00", "params": list(upd), "n": len(upd)}
        new_dumps = lambda: wire.dumps_reference(msg_new, default=ref_default)  # noqa: E731
        ref_dumps = lambda: msgpack.packb(msg_ref, default=ref_default, strict_types=True)  # noqa: E731
        data = ref_dumps()
        assert new_dumps() == data, f"{scheme}: dumps_reference differs from packb"
        new_loads = lambda: wire.loads_reference(data, object_hook=ref_hook)  # noqa: E731
        ref_loads = lambda: msgpack.unpackb(data, object_hook=ref_hook, strict_map_key=False)  # noqa: E731
        got = new_loads()
        assert got == ref_loads() and got["params"].packed.tobytes() == upd.packed.tobytes(), f"{scheme}: loads differ"
        assert wire.reference_stats(reset=True)["fallback"] == 0
        del got
        for leg, new, ref in ((f"{scheme}_dumps", new_dumps, ref_dumps), (f"{scheme}_loads", new_loads, ref_loads)):
            times = {"new": [], "reference": []}
            for run in range(a.runs):
                for impl, fn in (("new", new), ("reference", ref)):
                    dt, out = timed(fn)
                    del out
                    rec = {"leg": leg, "impl": impl, "run": run, "ms": round(dt * 1e3, 3), "items": len(upd),
                           "message_bytes": len(data)}
                    if impl == "new":
                        rec["phases_ms"] = {k: round(v * 1e3, 3) for k, v in wire.reference_stats()["last"].items()}
                    times[impl].append(dt * 1e3)
                    lines.append(rec)
                    print(json.dumps(rec), flush=True)
            legs[leg] = {"new_ms": [round(t, 3) for t in times["new"]], "reference_ms": [round(t, 3) for t in times["reference"]],
                         "slowest_new_ms": round(max(times["new"]), 3), "fastest_reference_ms": round(min(times["reference"]), 3),
                         "holds": max(times["new"]) < min(times["reference"]),
                         "median_ratio": round(float(np.median(times["reference"]) / np.median(times["new"])), 2)}
    st = wire.reference_stats()
    summary = {"summary": legs, "condition": "per leg: slowest new run < fastest reference run",
               "holds": all(v["holds"] for v in legs.values()), "elements": a.elements, "runs": a.runs,
               "fast": st["fast"], "fallback": st["fallback"], "msgpack": ".".join(map(str, msgpack.version))}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    return 0 if summary["holds"] else 1


if __name__ == "__main__":
    sys.exit(main())

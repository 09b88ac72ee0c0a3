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

--resident: the two "researcher takes one reply" legs instead (profiles/wire_resident_ab.jsonl), same protocol:

  leg          new                                                  reference (what a stock researcher runs)
  lom_take     loads_reference(bytes, hook, resident=True), add     unpackb(bytes, object_hook=_object_hook), add(list)
  jl_take      likewise at ceil(10M / 30) ciphertexts

each into a running accumulator (`begin_aggregate()` with one reply already folded in), every run ending in a device
synchronise; the accumulators of both sides are compared first.  The new side's phases: `scan` (the host scanner's
passes), `h2d` (staging + upload, synchronised for the timing), `devscan` (the device tokenizer and the copy of its
two result words, where an array took that route), `fold` (add + synchronise: the kernels).
--device-scan-min-items N sets `loads_reference`'s keyword (default: the module's `wire.DEVICE_SCAN_MIN_ITEMS`),
--device-scan-jl-min-items N the one of the JL leg (default: `wire.DEVICE_SCAN_JL_MIN_ITEMS`).

--devscan: the LOM take leg with the device scan forced on against the device scan disabled (the host scanner's
walk), alternating, --runs of each, at every item count 2^10 .. 2^24 (profiles/wire_devscan_ab.jsonl).  The last line
names the smallest power of two from which on the device route's median take is the faster one: the value for
`wire.DEVICE_SCAN_MIN_ITEMS` on that box.

--devscan-jl: the same sweep for the JL take leg (`device_scan_jl_min_items` forced on against disabled) at every
ciphertext count 2^8 .. 2^19, the updates' bytes made by `wire.dumps_reference` (profiles/wire_devscan_jl_ab.jsonl);
the last line names the value for `wire.DEVICE_SCAN_JL_MIN_ITEMS`.

--kernels: for a kernel trace (`rocprofv3 --kernel-trace --stats -- python tools/wire_ref_ab.py --kernels`): one LOM
update's bytes uploaded once, then four launches of wire_fold_lom_kernel (continuing) and four of
wire_decode_lom_kernel + lom_fold_kernel on the same bytes, then four reads of the message with the device scan
forced on (wire_tok_maps_kernel, wire_tok_scan_kernel, wire_tok_emit_kernel; the printed line has the stream's bytes),
then four reads of a JL update of ceil(elements / 30) ciphertexts with the JL device scan forced on
(wire_tokj_maps_kernel, wire_tokj_scan_kernel, wire_tokj_emit_kernel; a second line).

--stream: the receive path behind the last chunk (profiles/wire_stream_ab.jsonl).  One node's LOM reply of --elements
words and one JL reply of ceil(elements / 30) ciphertexts, cut into 4 MB chunks as the reference's sender cuts them,
handed to `add` one by one; timed from handing over the last chunk until `loads_reference` returns:

  streamed     wire.StreamAssembler.add ..., loads_reference(msg, hook, resident=True)
  parent       wire.ChunkAssembler.add ..., loads_reference(bytes, hook, resident=True)    (the parent commit's path)

Alternating, --runs fresh processes of each (one warm-up message per scheme, then one timed message per scheme and
pacing), one session.  Chunks are paced 1.3 ms apart (4 MB at 25 Gb/s, faster than any link a hospital node has); an
unpaced leg (gap 0) is recorded beside it without a condition, and so is the host time spent inside all `add` calls.
The condition: on both schemes the slowest paced streamed run is below the fastest paced parent run.
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


def _lom_words(rng, n):
    return rng.integers(0, 2**64, size=n, dtype=np.uint64)


def _jl_rows(rng, n_ct):
    rows = rng.integers(0, 2**32, size=(n_ct, 64), dtype=np.uint64).astype(np.uint32)
    rows[:, 63] &= 0x3FFFFFFF  # below 2^2046 <= N^2: a ciphertext's range
    return rows


def kernels(a):
    """The launches a kernel trace compares (see the module's docstring)."""
    import torch

    from fedbiomed_amd import _device as D

    dev = D.device()
    data = msgpack.packb({"node_id": "node-00", "params": _lom_words(np.random.default_rng(2026), a.elements).tolist()})
    arrays = D.wire_scan(data, 1024)
    (h,) = D.wire_upload(data, arrays)
    acc = torch.zeros(h.n, dtype=torch.int64, device=dev)
    ref = torch.zeros(h.n, dtype=torch.int64, device=dev)
    rows = torch.empty(h.n, dtype=torch.int64, device=dev)
    for _ in range(4):
        D.wire_fold_lom(h, acc, False)
        torch.cuda.synchronize()
    for _ in range(4):
        D.lom_fold(ref, D.wire_rows_device(h, out=rows), False)
        torch.cuda.synchronize()
    assert torch.equal(acc, ref)
    for _ in range(4):
        upd = wire.loads_reference(data, resident=True, device_scan_min_items=1)["params"]
        torch.cuda.synchronize()
    assert wire.reference_stats()["device_scan"] == 4 and torch.equal(D.wire_rows_device(upd.handle), rows)
    print(json.dumps({"kernels": "4 x wire_fold_lom_kernel, 4 x (wire_decode_lom_kernel + lom_fold_kernel), "
                                 "4 x (wire_tok_maps_kernel + wire_tok_scan_kernel + wire_tok_emit_kernel)", "items": h.n,
                      "tokenized_stream_bytes": len(data) - upd.handle.base}))
    del upd, h, acc, ref, rows, data
    packed = _jl_rows(np.random.default_rng(2027), -(-a.elements // 30))
    data = wire.dumps_reference({"node_id": "node-00", "params": wire.EncryptedParams.from_packed("jl", packed)},
                                default=ref_default)
    want = D.wire_decode(data, D.wire_scan(data, 1024))[0]
    assert np.array_equal(want, packed)
    wire.reference_stats(reset=True)
    for _ in range(4):
        upd = wire.loads_reference(data, object_hook=ref_hook, resident=True, device_scan_jl_min_items=1)["params"]
        torch.cuda.synchronize()
    assert wire.reference_stats()["device_scan_jl"] == 4 and np.array_equal(upd.handle.rows_host(), packed)
    print(json.dumps({"kernels": "4 x (wire_tokj_maps_kernel + wire_tokj_scan_kernel + wire_tokj_emit_kernel)",
                      "items": upd.handle.n, "tokenized_stream_bytes": len(data) - upd.handle.base}))
    return 0


def devscan(a, jl=False):
    """The sweep that fixes wire.DEVICE_SCAN_MIN_ITEMS, or with jl wire.DEVICE_SCAN_JL_MIN_ITEMS (see the module's
    docstring)."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd import workload as W
    from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

    dev = D.device()
    wire._PHASE_TIMING = False  # nothing but the take is timed: no synchronise inside it
    rng = np.random.default_rng(2026)
    routes = (("device", 1), ("host", 2**62))
    keyword = "device_scan_jl_min_items" if jl else "device_scan_min_items"
    counter = "device_scan_jl" if jl else "device_scan"
    sk0 = -sum(W.jl_user_key(p) for p in range(3))
    lines, medians = [], {}
    for k in (range(8, 20) if jl else range(10, 25)):
        n = 1 << k
        if jl:
            words = _jl_rows(rng, n)
            first = torch.from_numpy(words.view(np.int32)).to(dev)
            data = wire.dumps_reference({"node_id": "node-00", "params": wire.EncryptedParams.from_packed("jl", words),
                                         "n": n}, default=ref_default)
        else:
            words = _lom_words(rng, n)
            first = torch.from_numpy(words.view(np.int64)).to(dev)
            data = msgpack.packb({"node_id": "node-00", "params": words.tolist(), "n": n})
        del words
        aggs = {}
        for impl, _ in routes:
            aggs[impl] = SecaggCrypter().begin_aggregate(3, 64, sk0, W.BIPRIME0, 1000, num_expected_params=30 * n) if jl else \
                SecaggLomCrypter(W.LOM_NONCE).begin_aggregate(1000)
            aggs[impl].add(first)
        torch.cuda.synchronize()

        def take(impl, dmin):
            # (jl: the sweep starts below loads_reference's default min_items, so both routes lower it)
            upd = wire.loads_reference(data, object_hook=ref_hook, resident=True, min_items=256 if jl else 1024,
                                       **{keyword: dmin})["params"]
            aggs[impl].add(upd)
            torch.cuda.synchronize()
            return upd

        wire.reference_stats(reset=True)
        for impl, dmin in routes:  # warm-up, and both routes' accumulators compared
            del_me = take(impl, dmin)
            assert type(del_me) is wire.ResidentUpdate and not del_me.materialised
            del del_me
        st = wire.reference_stats()
        assert (st[counter], st[counter + "_refused"], st["resident"]) == (1, 0, 2), st
        assert torch.equal(aggs["device"]._acc, aggs["host"]._acc), f"2^{k}: the accumulators differ"
        times = {impl: [] for impl, _ in routes}
        for run in range(a.runs):
            for impl, dmin in routes:
                dt, out = timed(lambda: take(impl, dmin))
                del out
                rec = {"leg": "jl_take_sweep" if jl else "lom_take_sweep", "impl": impl, "items": n, "run": run, "ms": round(dt * 1e3, 3),
                       "message_bytes": len(data),
                       "phases_ms": {p: round(v * 1e3, 3) for p, v in wire.reference_stats()["last"].items()}}
                times[impl].append(dt * 1e3)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
        assert torch.equal(aggs["device"]._acc, aggs["host"]._acc), f"2^{k}: the accumulators differ after the runs"
        medians[n] = {impl: round(float(np.median(t)), 3) for impl, t in times.items()}
        medians[n].update(device_max=round(max(times["device"]), 3), host_min=round(min(times["host"]), 3))
        for g in aggs.values():
            g.abort()
        del aggs, first, data
    sizes = sorted(medians)
    chosen = None
    for n in reversed(sizes):  # the smallest power of two from which on the device route is the faster one
        if medians[n]["device"] < medians[n]["host"]:
            chosen = n
        else:
            break
    summary = {"summary": {str(n): medians[n] for n in sizes}, keyword: chosen, "runs": a.runs,
               "rule": "smallest 2^k such that the device route's median take is below the host route's at 2^k and above"}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    return 0


def resident(a):
    """The two "researcher takes one reply" legs (see the module's docstring)."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd import workload as W
    from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

    dev = D.device()
    wire._PHASE_TIMING = True
    scan_kw = {} if a.device_scan_min_items is None else {"device_scan_min_items": a.device_scan_min_items}
    if a.device_scan_jl_min_items is not None:
        scan_kw["device_scan_jl_min_items"] = a.device_scan_jl_min_items
    rng = np.random.default_rng(2026)
    n_ct = -(-a.elements // 30)
    sk0 = -sum(W.jl_user_key(p) for p in range(3))
    lines, legs = [], {}
    for scheme in ("lom", "jl"):
        packed = _lom_words(rng, a.elements) if scheme == "lom" else _jl_rows(rng, n_ct)
        first = torch.from_numpy(packed.view(np.int64 if scheme == "lom" else np.int32)).to(dev)
        data = msgpack.packb({"node_id": "node-00", "params": list(wire.EncryptedParams.from_packed(scheme, packed)),
                              "n": len(packed)}, default=ref_default, strict_types=True)
        del packed

        def begin():  # a running accumulator: one reply folded in, the JL factor done
            agg = SecaggLomCrypter(W.LOM_NONCE).begin_aggregate(1000) if scheme == "lom" else \
                SecaggCrypter().begin_aggregate(3, 64, sk0, W.BIPRIME0, 1000, num_expected_params=a.elements)
            agg.add(first)
            torch.cuda.synchronize()
            return agg

        aggs = {"new": begin(), "reference": begin()}
        phases = {}

        def new():
            t0 = time.perf_counter()
            upd = wire.loads_reference(data, object_hook=ref_hook, resident=True, **scan_kw)["params"]
            phases.clear()
            phases.update(wire.reference_stats()["last"])
            t1 = time.perf_counter()
            aggs["new"].add(upd)
            torch.cuda.synchronize()
            phases["fold"] = time.perf_counter() - t1
            phases["loads"] = t1 - t0
            return upd

        def ref():
            lst = msgpack.unpackb(data, object_hook=ref_hook, strict_map_key=False)["params"]
            aggs["reference"].add(lst)
            torch.cuda.synchronize()
            return lst

        upd = new()
        ref()
        assert type(upd) is wire.ResidentUpdate and not upd.materialised
        assert torch.equal(aggs["new"]._acc, aggs["reference"]._acc), f"{scheme}: the accumulators differ"
        del upd
        leg = f"{scheme}_take"
        times = {"new": [], "reference": []}
        for run in range(a.runs):
            for impl, fn in (("new", new), ("reference", ref)):
                dt, out = timed(fn)
                del out
                rec = {"leg": leg, "impl": impl, "run": run, "ms": round(dt * 1e3, 3), "items": len(first),
                       "message_bytes": len(data)}
                if impl == "new":
                    rec["phases_ms"] = {k: round(v * 1e3, 3) for k, v in phases.items()}
                times[impl].append(dt * 1e3)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
        assert torch.equal(aggs["new"]._acc, aggs["reference"]._acc), f"{scheme}: the accumulators differ after the runs"
        legs[leg] = {"new_ms": [round(t, 3) for t in times["new"]], "reference_ms": [round(t, 3) for t in times["reference"]],
                     "slowest_new_ms": round(max(times["new"]), 3), "fastest_reference_ms": round(min(times["reference"]), 3),
                     "holds": max(times["new"]) < min(times["reference"]),
                     "median_ratio": round(float(np.median(times["reference"]) / np.median(times["new"])), 2)}
        for g in aggs.values():
            g.abort()
        del aggs, first, data
    st = wire.reference_stats()
    summary = {"summary": legs, "condition": "per leg: slowest new run < fastest reference run",
               "holds": all(v["holds"] for v in legs.values()), "elements": a.elements, "runs": a.runs,
               "resident": st["resident"], "fallback": st["fallback"], "device_scan": st.get("device_scan", 0),
               "device_scan_refused": st.get("device_scan_refused", 0), "device_scan_jl": st.get("device_scan_jl", 0),
               "device_scan_jl_refused": st.get("device_scan_jl_refused", 0), "scan_keywords": scan_kw,
               "msgpack": ".".join(map(str, msgpack.version))}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    return 0 if summary["holds"] else 1


CHUNK = 4 * 1024 * 1024  # the reference's MAX_MESSAGE_BYTES_LENGTH
STREAM_GAPS_MS = (1.3, 0.0)


def stream_one(a):
    """One process of --stream: `a.stream_one` = "streamed" or "parent"; one JSON line per scheme and pacing."""
    import torch

    from fedbiomed_amd import _device as D

    dev = D.device()
    rng = np.random.default_rng(2026)
    n_ct = -(-a.elements // 30)
    updates = {"lom": wire.EncryptedParams.from_packed("lom", _lom_words(rng, a.elements)),
               "jl": wire.EncryptedParams.from_packed("jl", _jl_rows(rng, n_ct))}
    streamed = a.stream_one == "streamed"
    for scheme, upd in updates.items():
        data = wire.dumps_reference({"node_id": "node-00", "params": upd, "n": len(upd)}, default=ref_default)
        chunks = [data[i:i + CHUNK] for i in range(0, len(data), CHUNK)]
        asm = wire.StreamAssembler(object_hook=ref_hook) if streamed else wire.ChunkAssembler()

        def receive(gap):
            t_add, start, msg = 0.0, time.perf_counter(), None
            for i, c in enumerate(chunks, 1):
                # chunk i arrives at start + (i - 1) * gap whatever `add` cost: both sides see the same link, and the
                # host time of `add` counts against the side that spends it
                while time.perf_counter() < start + (i - 1) * gap:
                    pass
                t0 = time.perf_counter()
                msg = asm.add(c, len(chunks), i)
                t_add += time.perf_counter() - t0
            got = wire.loads_reference(msg, object_hook=ref_hook, resident=True)
            t1 = time.perf_counter()
            return t1 - t0, t_add, got, msg

        _, _, got, msg = receive(0.0)  # warm-up: allocations, the pinned ring, the library's first launches
        assert type(got["params"]) is wire.ResidentUpdate and got["params"].n_items == len(upd)
        if a.elements <= 100_000:  # (a small run also checks the values)
            assert got["params"].tolist() == list(upd)
        del got, msg
        for gap_ms in STREAM_GAPS_MS:
            wire.reference_stats(reset=True)
            gc.collect()
            torch.cuda.synchronize(dev)
            dt, t_add, got, msg = receive(gap_ms * 1e-3)
            st = wire.reference_stats()
            rec = {"leg": f"{scheme}_last_chunk", "impl": a.stream_one, "gap_ms": gap_ms, "ms": round(dt * 1e3, 3),
                   "add_total_ms": round(t_add * 1e3, 3), "chunks": len(chunks), "chunk_bytes": CHUNK, "message_bytes": len(data),
                   "items": len(upd), "streamed": st["streamed"], "stream_fallback": st["stream_fallback"],
                   "joined": bool(getattr(msg, "joins", 1))}
            print(json.dumps(rec), flush=True)
            del got, msg
    return 0


def stream(a):
    """--stream: alternating fresh processes of both implementations (see the module's docstring)."""
    import subprocess

    lines = []
    for run in range(a.runs):
        for impl in ("streamed", "parent"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--stream-one", impl, "--elements", str(a.elements)],
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            for ln in out.splitlines():
                rec = dict(json.loads(ln), run=run)
                lines.append(rec)
                print(json.dumps(rec), flush=True)
    legs = {}
    for leg in sorted({r["leg"] for r in lines}):
        for gap in STREAM_GAPS_MS:
            t = {impl: [r["ms"] for r in lines if (r["leg"], r["gap_ms"], r["impl"]) == (leg, gap, impl)] for impl in ("streamed", "parent")}
            adds = {impl: [r["add_total_ms"] for r in lines if (r["leg"], r["gap_ms"], r["impl"]) == (leg, gap, impl)]
                    for impl in ("streamed", "parent")}
            legs[f"{leg}@{gap}ms"] = {"streamed_ms": t["streamed"], "parent_ms": t["parent"], "slowest_streamed_ms": max(t["streamed"]),
                                      "fastest_parent_ms": min(t["parent"]), "holds": max(t["streamed"]) < min(t["parent"]),
                                      "add_total_ms": adds, "conditioned": gap > 0}
    paced = [v for v in legs.values() if v["conditioned"]]
    summary = {"summary": legs, "condition": "paced legs, both schemes: slowest streamed run < fastest parent run",
               "holds": all(v["holds"] for v in paced), "pacing_ms": STREAM_GAPS_MS[0], "chunk_bytes": CHUNK, "elements": a.elements,
               "processes_each": a.runs, "all_streamed": all(r["streamed"] == 1 and not r["joined"] for r in lines if r["impl"] == "streamed")}
    lines.append(summary)
    print(json.dumps(summary), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.writelines(json.dumps(ln) + "\n" for ln in lines)
    return 0 if summary["holds"] else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--elements", type=int, default=10_000_000)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--devscan", action="store_true")
    ap.add_argument("--devscan-jl", action="store_true")
    ap.add_argument("--device-scan-min-items", type=int, default=None)
    ap.add_argument("--device-scan-jl-min-items", type=int, default=None)
    ap.add_argument("--stream", action="store_true")
    ap.add_argument("--stream-one", choices=("streamed", "parent"), default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.stream_one:
        return stream_one(a)
    a.out = a.out or os.path.join(ROOT, "profiles", "wire_stream_ab.jsonl" if a.stream else "wire_devscan_jl_ab.jsonl" if a.devscan_jl else
                                  "wire_devscan_ab.jsonl" if a.devscan else
                                  "wire_resident_ab.jsonl" if a.resident else "wire_reference_ab.jsonl")
    if a.stream:
        return stream(a)
    if a.kernels:
        return kernels(a)
    if a.devscan or a.devscan_jl:
        return devscan(a, jl=a.devscan_jl)
    if a.resident:
        return resident(a)

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

#!/usr/bin/env python3
"""Times of the wide Joye-Libert engine, one JSON line per run: a factor launch at several
ciphertext counts with a 4090-bit key in both signs (the difference is the negative key's inversion), the
encrypt rate at --elements, and host Python `pow` per exponentiation as the comparison.  2048-bit
N = (2^1024 - 105)^2; host clock around the call and a synchronise; one warm-up, then --reps runs.

    python tools/jl_wide_sweep.py [--out profiles/jl_wide_sweep.jsonl] [--reps 3] [--elements 1000000]

--engine wave group: the factor launch (negative key) and encrypt_tensor under each forced engine of
the test build instead, the engines alternating within a repetition, every row with its "engine":

    python tools/jl_wide_sweep.py --engine wave group --out profiles/jl_wide_group_sweep.jsonl \
        --counts 256 1024 2048 4096 8192 16384 31250 65536

--seal: at --elements, the unprepared encrypt_tensor, decrypt_factor_tensor alone, encrypt_tensor(factor=)
alone and a continuing D.jlw_fold of one row, alternating within a repetition, then the slowest prepared run over the
fastest unprepared one:

    python tools/jl_wide_sweep.py --seal --out profiles/jl_wide_seal.jsonl

--wire ("wide items"): a stock peer's reply of --items ciphertexts, resident on the device: its decode
into rows followed by D.jlw_fold, D.wire_fold_jlw straight from the bytes, wire.reference_bytes of the rows, and
on the host msgpack's unpackb with the reference's hook and packb of the same message; then whether the slowest fused
run lies below the fastest split one:

    python tools/jl_wide_sweep.py --wire --out profiles/jl_wide_wire.jsonl

--take ("wide items"): at each of --counts full-width items, (a) `wire.loads_reference(resident=True,
jl_limbs=128)` of one reply through the wide device tokenizer (device_scan_jl_min_items=1) against the host scanner's
walk (the threshold past the array's size), and (b) the last chunk to the `ResidentUpdate` through
`StreamAssembler(jl_limbs=128)` against `ChunkAssembler` + the host walk, chunks of 4 MB paced 1.3 ms apart as
tools/wire_ref_ab.py --stream paces them, with the host time inside all `add` calls.  One session, one warm-up of
every leg, the legs alternating within a repetition; the rows are appended to --out:

    python tools/jl_wide_sweep.py --take --counts 4096 16384 31250 131072 333334 --out profiles/jl_wide_wire.jsonl
"""
import argparse
import json
import math
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jl_wide_sweep.jsonl"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--elements", type=int, default=1000000)
    ap.add_argument("--counts", type=int, nargs="+", default=[1, 256, 2048, 4096])
    ap.add_argument("--engine", nargs="+", choices=["auto", "wave", "group"], default=None)
    ap.add_argument("--seal", action="store_true")
    ap.add_argument("--wire", action="store_true")
    ap.add_argument("--items", type=int, default=31250)
    ap.add_argument("--take", action="store_true")
    args = ap.parse_args()
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    n = ((1 << 1024) - 105) ** 2
    key = random.Random(41).getrandbits(4090) | (1 << 4089)
    dev, sc = D.device(), SecaggCrypter()
    props = torch.cuda.get_device_properties(dev)
    rows = [{"what": "device", "name": props.name, "cus": props.multi_processor_count}]

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3

    if args.seal:  # the legs alternate within a repetition, after one warm-up of each
        x = torch.rand(args.elements, dtype=torch.float64, device=dev) * 4 - 2
        n_ct = -(-args.elements // D.jl_slot(None, 3)[1])
        f = sc.decrypt_factor_tensor(5, n_ct, key, n)
        acc = sc.encrypt_tensor(3, 5, x, key, n)
        assert torch.equal(acc, sc.encrypt_tensor(3, 5, x, key, n, factor=f))
        legs = [("encrypt_tensor", lambda: sc.encrypt_tensor(3, 5, x, key, n)),
                ("decrypt_factor_tensor", lambda: sc.decrypt_factor_tensor(5, n_ct, key, n)),
                ("encrypt_tensor_factor", lambda: sc.encrypt_tensor(3, 5, x, key, n, factor=f)),
                ("jlw_fold_k1", lambda: D.jlw_fold(acc, f, n))]
        timed(legs[3][1])
        for rep in range(args.reps):
            for what, fn in legs:
                rows.append({"what": what, "elements": args.elements, "n_ct": n_ct, "num_nodes": 3, "rep": rep,
                             "n_bits": n.bit_length(), "ms": timed(fn)})
        ms = {w: [r["ms"] for r in rows if r["what"] == w] for w, _ in legs}
        rows.append({"what": "seal_summary", "n_ct": n_ct,
                     "slowest_prepared_over_fastest_unprepared": max(ms["encrypt_tensor_factor"]) / min(ms["encrypt_tensor"]),
                     "fold_bytes": 512 * 3 * n_ct, "fold_gb_per_s": 512 * 3 * n_ct / min(ms["jlw_fold_k1"]) / 1e6})
        return emit(rows, args.out)
    if args.take:  # DESIGN 4.2, "wide items": the reply's way onto the device, at once and chunk by chunk
        from fedbiomed_amd import wire

        def int_hook(o):  # the reference Serializer's rule (serializer.py:140-149)
            return int.from_bytes(o["value"], "big", signed=True) if o.get("__type__") == "int" else o

        chunk, gap = 4 << 20, 1.3e-3
        for items in args.counts:
            r = torch.randint(-2**31, 2**31, (items, 128), dtype=torch.int64, device=dev).to(torch.int32)
            r[:, 127] |= -2**31  # full width: every item 536 bytes
            data = wire.reference_bytes(r)
            del r
            chunks = [data[i:i + chunk] for i in range(0, len(data), chunk)]
            kw = dict(object_hook=int_hook, min_items=1, resident=True, jl_limbs=128)

            def take(jmin, key):
                wire.reference_stats(reset=True)
                up = wire.loads_reference(data, device_scan_jl_min_items=jmin, **kw)
                assert up.n_items == items and wire.reference_stats()[key] == 1

            def receive(asm, jmin, rec):
                t_add, start = 0.0, time.perf_counter()
                for i, c in enumerate(chunks, 1):  # chunk i arrives at start + (i - 1) * gap whatever `add` cost
                    while time.perf_counter() < start + (i - 1) * gap:
                        pass
                    t0 = time.perf_counter()
                    msg = asm.add(c, len(chunks), i)
                    t_add += time.perf_counter() - t0
                up = wire.loads_reference(msg, device_scan_jl_min_items=jmin, **kw)
                torch.cuda.synchronize(dev)
                rec.update(ms=(time.perf_counter() - t0) * 1e3, add_total_ms=t_add * 1e3, chunks=len(chunks))
                assert up.n_items == items and getattr(msg, "joins", 1) == (0 if jmin == 1 else 1)

            sa = wire.StreamAssembler(object_hook=int_hook, min_items=1, device_scan_jl_min_items=1, jl_limbs=128)
            legs = [("take_device_route", lambda rec: rec.update(ms=timed(lambda: take(1, "device_scan_jl")))),
                    ("take_host_walk", lambda rec: rec.update(ms=timed(lambda: take(items + 1, "resident")))),
                    ("stream_last_chunk", lambda rec: receive(sa, 1, rec)),
                    ("joined_last_chunk", lambda rec: receive(wire.ChunkAssembler(), items + 1, rec))]
            for what, fn in legs:
                if len(chunks) > 1 or "take" in what:  # (a message of one chunk is not streamed)
                    fn({})
            for rep in range(args.reps):
                for what, fn in legs:
                    if len(chunks) > 1 or "take" in what:
                        rows.append({"what": what, "items": items, "message_bytes": len(data), "rep": rep})
                        fn(rows[-1])
            ms = {w: [x["ms"] for x in rows if x["what"] == w and x["items"] == items] for w, _ in legs}
            rows.append({"what": "take_summary", "items": items,
                         "device_route_wins": max(ms["take_device_route"]) < min(ms["take_host_walk"]),
                         "stream_wins": bool(ms["stream_last_chunk"]) and max(ms["stream_last_chunk"]) < min(ms["joined_last_chunk"])})
        return emit(rows, args.out, "a")
    if args.wire:  # DESIGN 4.2, "wide items": a stock peer's reply of --items full-width ciphertexts
        import msgpack

        from fedbiomed_amd import wire

        def ref_default(o):  # the reference Serializer's rules (serializer.py:96-110, :140-149)
            return {"__type__": "int", "value": o.to_bytes((o.bit_length() + 7) // 8 + 1, "big", signed=True)}

        def ref_hook(o):
            return int.from_bytes(o["value"], "big", signed=True) if o.get("__type__") == "int" else o

        rng = random.Random(5)
        vals = [rng.randrange(n * n) for _ in range(args.items)]
        data = msgpack.packb(vals, default=ref_default, strict_types=True)
        up = wire.loads_reference(data, object_hook=ref_hook, min_items=1, resident=True, jl_limbs=128)
        acc = D.wire_rows_device(up.handle).clone()
        rows_buf = torch.empty_like(acc)
        assert wire.reference_bytes(acc) == data and D.limbs_to_ints_w(acc[:64], 128) == vals[:64]
        a2 = acc.clone()
        assert torch.equal(D.wire_fold_jlw(up.handle, a2, n), D.jlw_fold(acc.clone(), acc, n))

        def host_route():
            msgpack.packb(msgpack.unpackb(data, object_hook=ref_hook, strict_map_key=False), default=ref_default,
                          strict_types=True)

        legs = [("decode_then_fold", lambda: D.jlw_fold(acc, D.wire_rows_device(up.handle, out=rows_buf), n)),
                ("wire_fold_jlw", lambda: D.wire_fold_jlw(up.handle, acc, n)),
                ("reference_bytes", lambda: wire.reference_bytes(rows_buf)),
                ("host_unpackb_packb", host_route)]
        for _, fn in legs:
            timed(fn)
        for rep in range(args.reps):
            for what, fn in legs:
                rows.append({"what": what, "items": args.items, "message_bytes": len(data), "rep": rep,
                             "n_bits": n.bit_length(), "ms": timed(fn)})
        ms = {w: [r["ms"] for r in rows if r["what"] == w] for w, _ in legs}
        rows.append({"what": "wire_summary", "items": args.items,
                     "slowest_fused_over_fastest_split": max(ms["wire_fold_jlw"]) / min(ms["decode_then_fold"]),
                     "fused_wins": max(ms["wire_fold_jlw"]) < min(ms["decode_then_fold"])})
        return emit(rows, args.out)
    for n_ct in args.counts if args.engine else []:
        def run_engine(eng):
            with D.jlw_engine(eng):
                sc.decrypt_factor_tensor(5, n_ct, -key, n)
        for eng in args.engine:
            run_engine(eng)
        for rep in range(args.reps):
            for eng in args.engine:
                rows.append({"what": "factor_launch", "engine": eng, "n_ct": n_ct, "key_bits": 4090,
                             "key_negative": True, "n_bits": n.bit_length(), "rep": rep,
                             "ms": timed(lambda: run_engine(eng))})
    for n_ct in [] if args.engine else args.counts:
        for k in (-key, key):
            def run():
                sc.decrypt_factor_tensor(5, n_ct, k, n)
            run()
            for rep in range(args.reps):
                rows.append({"what": "factor_launch", "n_ct": n_ct, "key_bits": 4090, "key_negative": k < 0,
                             "n_bits": n.bit_length(), "rep": rep, "ms": timed(run)})
    x = torch.rand(args.elements, dtype=torch.float64, device=dev) * 4 - 2
    for rep in range(args.reps + 1):
        for eng in args.engine or ["auto"]:
            with D.jlw_engine(eng):
                ms = timed(lambda: sc.encrypt_tensor(3, 5, x, key, n))
            rows.append({"what": "encrypt_tensor", "engine": eng, "elements": args.elements, "num_nodes": 3, "rep": rep,
                         "warmup": rep == 0, "ms": ms, "params_per_s": args.elements / ms * 1e3})
    h = random.Random(7).getrandbits(4090) % (n * n)
    while math.gcd(h, n) != 1:
        h += 1
    for rep in range(args.reps):
        t0 = time.perf_counter()
        pow(h, -key, n * n)
        rows.append({"what": "host_python_pow", "key_bits": 4090, "key_negative": True, "n_bits": n.bit_length(),
                     "rep": rep, "ms": (time.perf_counter() - t0) * 1e3})
    emit(rows, args.out)


def emit(rows, out, mode="w"):
    with open(out, mode) as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
            print(json.dumps(r))


if __name__ == "__main__":
    main()

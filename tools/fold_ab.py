#!/usr/bin/env python3
"""Streaming aggregation (begin_aggregate / add / finish, fbm_jl_fold, fbm_lom_fold) against the one-shot
aggregate it stands beside, alternated inside one process.  The one-shot entry points are the parent commit's
code unchanged (the feature only adds), so they are the yardstick.

    python tools/fold_ab.py [--small] [--out profiles/fold_ab.jsonl]

Three cases, one JSON line each; per case one warm-up round, then ROUNDS rounds, every round running every
variant once in an order shuffled per round from a fixed seed; the figures are the median and the [min, max]
of the rounds.

  tail      Joye-Libert 10M x 8: host wall time from "the last party's reply is in hand" to the result in
            hand (a device synchronise, or the List[float]).  One-shot unprepared and prepared against the stream
            with seven adds already done (and the device idle again), for the list API and for device tensors.
  lom_fold  lom_fold_kernel (first call, k = 8, n = 10M) against lom_aggregate on the same rows: both read 8
            rows and write one 8-byte row.  Cold: a 512 MB scratch write (twice the MALL) before each, kernel
            time from the test build's HIP events.  And a continuing k = 1 fold (24 bytes per element).
  jl_fold   the jl_fold_kernel time of 8 single-row adds plus the finish's jl_prod_kernel (one party: the
            accumulator, and the factor) against one jl_prod_kernel launch over the 8 rows and the factor, at
            10M x 8 (333 334 ciphertexts): P + 2 products against P + 1, plus the accumulator's read and
            write per add.
"""
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 7


def alternate(variants: dict, rounds: int = ROUNDS) -> dict:
    """{name: fn -> ms} run rounds + 1 times, shuffled; {name: median ms, name + '_minmax': [min, max]}."""
    names = list(variants)
    ts = {k: [] for k in names}
    order = random.Random(len(names))
    for r in range(rounds + 1):
        for k in order.sample(names, len(names)):
            ms = variants[k]()
            if r:
                ts[k].append(ms)
    out = {}
    for k in names:
        s = sorted(ts[k])
        out[k] = round(s[len(s) // 2], 4)
        out[k + "_minmax"] = [round(s[0], 4), round(s[-1], 4)]
    return out


def wall_ms(fn) -> float:
    import torch

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def jl_round(n: int, P: int):
    """An honest round: [P, n_ct, 64] ciphertexts in HBM, the server key, the total weight."""
    import torch

    from fedbiomed_amd import _device as D, workload as W
    from fedbiomed_amd.secagg import SecaggCrypter

    dev = D.device()
    jc = SecaggCrypter()
    keys = [W.jl_user_key(p) for p in range(P)]
    ws = [W.party_weight(p) for p in range(P)]
    cts = torch.stack([jc.encrypt_tensor(P, 1, torch.from_numpy(W.party_params(p, n)).to(dev), keys[p], W.BIPRIME0,
                                         weight=ws[p]) for p in range(P)])
    return cts, -sum(keys), sum(ws)


def tail_case(n: int, P: int) -> dict:
    import numpy as np
    import torch

    from fedbiomed_amd import _device as D, workload as W
    from fedbiomed_amd.secagg import SecaggCrypter

    cts, sk0, total = jl_round(n, P)
    lists = [D.limbs_to_ints(cts[p].cpu().numpy().view(np.uint32)) for p in range(P)]
    jc = SecaggCrypter()
    args = (sk0, W.BIPRIME0, total)
    ref = jc.aggregate(1, P, lists, *args, num_expected_params=n)

    got = {}

    def check(name):  # (outside the clock: comparing 10M floats is host time of the tool's own)
        assert got.pop(name) == ref, "streamed and one-shot results differ: " + name

    def list_one_shot(prepared):
        if prepared:
            assert jc.prepare_aggregate(1, P, sk0, W.BIPRIME0, n)
        ms = wall_ms(lambda: got.__setitem__("one-shot", jc.aggregate(1, P, lists, *args, num_expected_params=n)))
        check("one-shot")
        return ms

    def list_stream(prepared):
        if prepared:
            assert jc.prepare_aggregate(1, P, sk0, W.BIPRIME0, n)
        agg = jc.begin_aggregate(1, P, *args, num_expected_params=n)
        for p in range(P - 1):
            agg.add(lists[p])

        def last():
            agg.add(lists[P - 1])
            got["stream"] = agg.finish()

        ms = wall_ms(last)
        check("stream")
        return ms

    out = {}

    def tensor_one_shot(with_factor):
        f = jc.decrypt_factor_tensor(1, cts.shape[1], sk0, W.BIPRIME0) if with_factor else None
        return wall_ms(lambda: out.__setitem__("a", jc.aggregate_tensor(1, cts, *args, num_expected_params=n,
                                                                        decrypt_factor=f)))

    def tensor_stream():
        agg = jc.begin_aggregate(1, P, *args, num_expected_params=n)
        for p in range(P - 1):
            agg.add(cts[p])

        def last():
            agg.add(cts[P - 1])
            out["b"] = agg.finish_tensor()

        return wall_ms(last)

    res = alternate({"list_one_shot": lambda: list_one_shot(False), "list_one_shot_prepared": lambda: list_one_shot(True),
                     "list_stream": lambda: list_stream(False), "list_stream_prepared": lambda: list_stream(True),
                     "tensor_one_shot": lambda: tensor_one_shot(False),
                     "tensor_one_shot_factor_ahead": lambda: tensor_one_shot(True), "tensor_stream": tensor_stream})
    assert torch.equal(out["a"].view(torch.int64), out["b"].view(torch.int64))
    return {"case": "tail", "scheme": "jl", "n": n, "P": P, "n_ct": int(cts.shape[1]), "unit": "ms",
            "what": "host wall time from the last reply in hand to the result in hand", **res}


def lom_fold_case(n: int, k: int) -> dict:
    import torch

    from fedbiomed_amd import _device as D, _native

    dev = D.device()
    Y = torch.randint(0, 2**40, (k, n), dtype=torch.int64, device=dev)
    acc = torch.empty(n, dtype=torch.int64, device=dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    scratch = torch.empty(512 * 2**20 // 8, dtype=torch.int64, device=dev)

    def kernel_ms(name, fn, cold=True):
        if cold:
            scratch.fill_(1)  # twice the MALL: the rows are evicted
        torch.cuda.synchronize()
        _native.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        _native.prof_enable(False)
        c, t = _native.prof_report()[name]
        return t / c

    with _native.test_hooks():
        res = alternate({
            "aggregate_a": lambda: kernel_ms("lom_aggregate", lambda: D.lom_aggregate(Y, 1000 * k, out=out)),
            "aggregate_b": lambda: kernel_ms("lom_aggregate", lambda: D.lom_aggregate(Y, 1000 * k, out=out)),
            "fold_first_k": lambda: kernel_ms("lom_fold", lambda: D.lom_fold(acc, Y, first=True)),
            "fold_continue_1": lambda: kernel_ms("lom_fold", lambda: D.lom_fold(acc, Y[0], first=False)),
        })
    want = Y.sum(dim=0)
    D.lom_fold(acc, Y, first=True)
    assert torch.equal(acc, want)
    lo = min(res["aggregate_a_minmax"][0], res["aggregate_b_minmax"][0])
    hi = max(res["aggregate_a_minmax"][1], res["aggregate_b_minmax"][1])
    nbytes = {"aggregate": 8 * n * (k + 1), "fold_first_k": 8 * n * (k + 1), "fold_continue_1": 24 * n}
    return {"case": "lom_fold", "n": n, "k": k, "unit": "ms", "cold": True, "bytes": nbytes, **res,
            "aggregate_kernel": D.lom_aggregate_kernel(k, Y), "aggregate_range": [lo, hi],
            "fold_within_aggregate_range": lo <= res["fold_first_k"] <= hi,
            "TBps": {"aggregate": round(nbytes["aggregate"] / ((res["aggregate_a"] + res["aggregate_b"]) / 2) / 1e9, 3),
                     "fold_first_k": round(nbytes["fold_first_k"] / res["fold_first_k"] / 1e9, 3),
                     "fold_continue_1": round(nbytes["fold_continue_1"] / res["fold_continue_1"] / 1e9, 3)}}


def jl_fold_case(n: int, P: int) -> dict:
    import torch

    from fedbiomed_amd import _device as D, _native, workload as W

    cts, sk0, total = jl_round(n, P)
    n_ct = int(cts.shape[1])
    factor = D.jl_decrypt_factor(n_ct, W.BIPRIME0, sk0, 1)
    slot = D.jl_slot(None, P)
    acc = torch.empty((n_ct, 64), dtype=torch.int32, device=cts.device)
    outs = {}

    def report(fn):
        torch.cuda.synchronize()
        _native.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        _native.prof_enable(False)
        return _native.prof_report()

    def one_shot():
        def run():
            outs["a"] = D.jl_aggregate(cts, W.BIPRIME0, sk0, 1, n, total, factor=factor)[0]
        return report(run)["jl_prod"][1]

    def stream():
        def run():
            for p in range(P):
                D.jl_fold(acc, cts[p], W.BIPRIME0, seed_ops=P if p == 0 else 0)
            outs["b"] = D.jl_aggregate(acc[None], W.BIPRIME0, sk0, 1, n, total, slot=slot, factor=factor)[0]
        rep = report(run)
        assert rep["jl_fold"][0] == P and rep["jl_prod"][0] == 1
        outs["fold_ms"], outs["finish_ms"] = rep["jl_fold"][1], rep["jl_prod"][1]
        return rep["jl_fold"][1] + rep["jl_prod"][1]

    with _native.test_hooks():
        res = alternate({"one_shot_prod_a": one_shot, "one_shot_prod_b": one_shot, "folds_plus_finish": stream})
    assert torch.equal(outs["a"].view(torch.int64), outs["b"].view(torch.int64))
    base = (res["one_shot_prod_a"] + res["one_shot_prod_b"]) / 2
    return {"case": "jl_fold", "n": n, "P": P, "n_ct": n_ct, "unit": "ms", **res,
            "last_round_folds_ms": round(outs["fold_ms"], 4), "last_round_finish_prod_ms": round(outs["finish_ms"], 4),
            "products": {"one_shot": P + 1, "stream": P + 2}, "ratio": round(res["folds_plus_finish"] / base, 3)}


def main():
    argv = sys.argv[1:]
    small = "--small" in argv  # a rehearsal of the tool itself: shapes that take no time
    dst = argv[argv.index("--out") + 1] if "--out" in argv else None
    n = 100_000 if small else 10_000_000
    lines = []
    for case in (lambda: tail_case(n, 8), lambda: lom_fold_case(n, 8), lambda: jl_fold_case(n, 8)):
        import torch

        line = {"rounds": ROUNDS, "small": small, **case()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        torch.cuda.empty_cache()
    if dst:
        with open(dst, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""16-bit inputs and narrow outputs against what they replace, and this build's float64 / float32 paths against
a base library (the parent commit's build), alternated inside one process.

    FBM_AB_VARIANT=1 FBM_LIB_PATH=build/ab/parent.so python tools/dtype_ab.py [--small]

Kernel times are the library's own per-kernel HIP events (the test build's timer; a base library built by
`python -m fedbiomed_amd._build --out ...` has it too); a torch cast beside a kernel (`x.float()`, `.to(bfloat16)`)
is timed with a torch event pair around that one op on the same stream, and a two-step form's time is the sum.
Per case: one warm-up round, then 7 rounds; every round runs every variant once, in an order shuffled per round
from a fixed seed (a kernel's time depends a little on what ran before it: no variant keeps one predecessor);
the figure is the median over the rounds.  The base library runs the float64 / float32 variants TWICE per
round (base_a, base_b): the gap between their medians and the range of their single runs are the spread this
process shows between runs of identical code, which this build's figure is to be read against.  One JSON line
per case; without FBM_LIB_PATH the base variants are left out.

  LOM protect, 10M elements x 7 peers:  float32 input | bfloat16 input, fused | bfloat16 by x.float() + protect
  LOM aggregate, 10M x 8 and 100M x 16: float64 | float64 + .to(bfloat16) | fused bfloat16 | fused float32
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BASE = os.environ.get("FBM_LIB_PATH")
ROUNDS = 7


class library:
    """Routes the calling thread's library calls to the base library (FBM_LIB_PATH, FBM_AB_VARIANT=1) or to this
    tree's test build, and collects the per-kernel events of the calls made inside."""

    def __init__(self, base: bool):
        self.base = base

    def __enter__(self):
        from fedbiomed_amd import _native

        if self.base:
            os.environ["FBM_LIB_PATH"], os.environ["FBM_AB_VARIANT"] = BASE, "1"
        else:
            os.environ.pop("FBM_LIB_PATH", None)
            os.environ.pop("FBM_AB_VARIANT", None)
        self.hooks = _native.test_hooks()
        self.hooks.__enter__()
        _native.prof_enable(True)
        return self

    def kernel_ms(self, name: str) -> float:
        from fedbiomed_amd import _native

        return _native.prof_report()[name][1]

    def __exit__(self, *exc):
        from fedbiomed_amd import _native

        _native.prof_enable(False)
        self.hooks.__exit__(*exc)
        return False


def torch_ms(fn):
    """(fn(), its duration on the current stream in ms): an event pair around one torch op."""
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return r, a.elapsed_time(b)


def alternate(variants: dict) -> dict:
    """{name: fn -> ms} run ROUNDS + 1 times, shuffled; {name: median ms, name + '_minmax': [min, max]}."""
    import random

    names = list(variants)
    ts = {k: [] for k in names}
    order = random.Random(len(names))
    for r in range(ROUNDS + 1):
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


def spread(res: dict, line: dict, this: str) -> None:
    """The base library against itself -- the gap between its two medians, and the range of its 2 x ROUNDS single
    runs -- and this build's median against it."""
    if "base_a" in res:
        a, b = res["base_a"], res["base_b"]
        lo = min(res["base_a_minmax"][0], res["base_b_minmax"][0])
        hi = max(res["base_a_minmax"][1], res["base_b_minmax"][1])
        line["base_self_spread"] = round(abs(a - b) / min(a, b), 4)
        line["base_range"] = [lo, hi]
        line["this_vs_base"] = round(res[this] / ((a + b) / 2) - 1, 4)
        line["this_within_base_range"] = lo <= res[this] <= hi


def protect_case(n: int, peers: int) -> dict:
    import torch

    from fedbiomed_amd import _device as D

    dev = D.device()
    g = torch.Generator(device=dev).manual_seed(1)
    x32 = torch.randn(n, generator=g, device=dev, dtype=torch.float32).clamp_(-3, 3)  # (inside the clipping range)
    x16 = x32.to(torch.bfloat16)
    y = torch.empty(n, dtype=torch.int64, device=dev)
    secrets = [bytes([p + 1]) * 32 for p in range(peers)]
    signs = [1 if p % 2 else -1 for p in range(peers)]

    def protect(x, base):
        with library(base) as lib:
            D.lom_protect(x, secrets, signs, b"dtype_ab".zfill(16), 3, peers + 1, out=y)
            torch.cuda.synchronize()
            return lib.kernel_ms("lom_protect")

    def cast_then_protect(base):
        xf, cast = torch_ms(lambda: x16.float())
        return cast + protect(xf, base)

    variants = {"f32": lambda: protect(x32, False), "bf16_fused": lambda: protect(x16, False),
                "bf16_cast_then_f32": lambda: cast_then_protect(False)}
    if BASE:
        variants.update({"base_a": lambda: protect(x32, True), "base_b": lambda: protect(x32, True),
                         "base_bf16_cast_then_f32": lambda: cast_then_protect(True)})
    res = alternate(variants)
    line = {"case": "lom_protect", "n": n, "peers": peers, "unit": "ms",
            "bytes": {"f32": 12 * n, "bf16_fused": 10 * n, "bf16_cast_then_f32": 6 * n + 12 * n}, **res}
    spread(res, line, "f32")
    return line


def aggregate_case(P: int, n: int) -> dict:
    import torch

    from fedbiomed_amd import _device as D

    dev = D.device()
    Y = torch.randint(0, 2**40, (P, n), dtype=torch.int64, device=dev)
    outs = {dt: torch.empty(n, dtype=dt, device=dev) for dt in (torch.float64, torch.float32, torch.bfloat16)}

    def aggregate(dt, base):
        with library(base) as lib:
            D.lom_aggregate(Y, 1000 * P, out=outs[dt])
            torch.cuda.synchronize()
            return lib.kernel_ms("lom_aggregate")

    def aggregate_then_cast(base):
        ms = aggregate(torch.float64, base)
        return ms + torch_ms(lambda: outs[torch.float64].to(torch.bfloat16))[1]

    f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
    variants = {"f64": lambda: aggregate(f64, False), "f64_then_bf16": lambda: aggregate_then_cast(False),
                "bf16_fused": lambda: aggregate(bf16, False), "f32_fused": lambda: aggregate(f32, False)}
    if BASE:
        variants.update({"base_a": lambda: aggregate(f64, True), "base_b": lambda: aggregate(f64, True),
                         "base_f64_then_bf16": lambda: aggregate_then_cast(True)})
    res = alternate(variants)
    nbytes = {"f64": 8 * (P + 1) * n, "f64_then_bf16": 8 * (P + 1) * n + 10 * n, "bf16_fused": (8 * P + 2) * n,
              "f32_fused": (8 * P + 4) * n}
    line = {"case": "lom_aggregate", "P": P, "n": n, "unit": "ms", "bytes": nbytes, **res,
            "TBps": {k: round(b / res[k] / 1e9, 3) for k, b in nbytes.items()}}
    if BASE:
        line["TBps"]["base"] = round(nbytes["f64"] / ((res["base_a"] + res["base_b"]) / 2) / 1e9, 3)
    spread(res, line, "f64")
    return line


def main():
    small = "--small" in sys.argv[1:]  # a rehearsal of the tool itself: shapes that take no time
    scale = 100 if small else 1
    meta = {"base": os.path.basename(BASE) if BASE else None, "rounds": ROUNDS, "small": small}
    print(json.dumps({**meta, **protect_case(10_000_000 // scale, 7)}), flush=True)
    for P, n in ((8, 10_000_000 // scale), (16, 100_000_000 // scale)):
        print(json.dumps({**meta, **aggregate_case(P, n)}), flush=True)
        import torch

        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

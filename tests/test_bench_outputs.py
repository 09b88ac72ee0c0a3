"""bench.py's plain run and --dump-outputs: a plain run carries the headline only (what else the
benchmark measures needs --full), --steps sets the number of timed steps, and --dump-outputs writes
the last timed step's averaged vector -- the same bytes from run to run, equal to what the tensor
API returns for the bench's seeded inputs (fedbiomed_amd/workload.py)."""

import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, P = 30011, 3  # odd: the last ciphertext is partly filled
FULL_ONLY = ("roofline", "roofline_valu", "kernels_ms", "stages", "lom", "end_to_end", "cpu_baseline", "gpu_over_cpu")


def _load_bench(monkeypatch):
    """bench.py as a module (it sets its HIP queue default at import: kept out of this process' environment)."""
    monkeypatch.delenv("GPU_MAX_HW_QUEUES", raising=False)
    monkeypatch.setattr(sys, "path", list(sys.path))
    spec = importlib.util.spec_from_file_location("_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bench(args, timeout=110):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT,
                       env=dict(os.environ, PYTHONUNBUFFERED="1"), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    bench = _load_bench(monkeypatch)
    assert bench.DUMP_LIMIT_BYTES <= 64 * 10 ** 6
    a = np.random.default_rng(1).standard_normal(5000)
    b = np.arange(700, dtype=np.float32).reshape(7, 100)
    rep = bench.dump_outputs(str(tmp_path / "whole"), {"a": a, "b": b})
    assert not rep["a"]["sampled"] and not rep["b"]["sampled"]
    got_a, got_b = np.load(tmp_path / "whole" / "a.npy"), np.load(tmp_path / "whole" / "b.npy")
    assert got_a.dtype == np.float64 and np.array_equal(got_a, a)
    assert got_b.dtype == np.float32 and np.array_equal(got_b, b)
    # over the limit: a sample at fixed ascending positions, the same on every call, files within the limit
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 24000)
    sizes = []
    for d in ("s1", "s2"):
        rep = bench.dump_outputs(str(tmp_path / d), {"a": a, "b": b})
        assert rep["a"]["sampled"] and not rep["b"]["sampled"]
        sizes.append(sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)))
    s1, s2 = np.load(tmp_path / "s1" / "a.npy"), np.load(tmp_path / "s2" / "a.npy")
    assert max(sizes) <= 24000 and s1.dtype == np.float64 and s1.size == rep["a"]["elements"] < a.size
    assert np.array_equal(s1, s2)
    idx = np.flatnonzero(np.isin(a, s1))  # the sample is a's elements at ascending positions
    assert idx.size == s1.size and np.array_equal(a[idx], s1)


def test_plain_and_full_are_separate_options(monkeypatch):
    bench = _load_bench(monkeypatch)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 2
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full is True and args.dump_outputs == "d"


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_last_step(tmp_path):
    import torch

    from fedbiomed_amd import workload as W
    from fedbiomed_amd.secagg import SecaggCrypter

    args = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--elements", str(N), "--parties", str(P)]
    lines = [_bench(args + ["--dump-outputs", str(tmp_path / d)]) for d in ("r1", "r2")]
    for d in lines:
        assert d["steps"] == 2 and d["warmup"] == 1 and d["n_gpus"] == 1
        assert d["unit"] == "params/s" and d["higher_is_better"] is True and d["dtype"]
        assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(N / (d["ms_per_step"] / 1000), rel=1e-9)
        assert d["outputs"]["aggregate"] == {"file": "aggregate.npy", "dtype": "float64", "elements": N,
                                             "sampled": False}
        assert not [k for k in FULL_ONLY if k in d]
    r1, r2 = np.load(tmp_path / "r1" / "aggregate.npy"), np.load(tmp_path / "r2" / "aggregate.npy")
    assert r1.dtype == np.float64 and r1.shape == (N,)
    assert np.array_equal(r1.view(np.uint64), r2.view(np.uint64))
    # what the step's caller receives for these inputs: every party's encrypt_tensor, then aggregate_tensor
    dev, jc, tau = torch.device("cuda", 0), SecaggCrypter(), 1
    keys, ws = [W.jl_user_key(p) for p in range(P)], [W.party_weight(p) for p in range(P)]
    cts = torch.stack([jc.encrypt_tensor(P, tau, torch.from_numpy(W.party_params(p, N)).to(dev), keys[p], W.BIPRIME0,
                                         weight=ws[p]) for p in range(P)])
    ref = jc.aggregate_tensor(tau, cts, -sum(keys), W.BIPRIME0, sum(ws), num_expected_params=N).cpu().numpy()
    assert np.array_equal(r1.view(np.uint64), ref.view(np.uint64))

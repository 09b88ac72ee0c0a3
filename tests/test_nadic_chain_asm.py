"""The register-resident chain body of the exponentiation's short path (tools/gen_nadic_asm.py
chain_short, fbm_na_chain_short in fedbiomed_amd/csrc/fbm_nadic_chain_asm.hpp) on the CPU simulator: its
square and short product as one-product bodies, registers in and registers out, limb for limb against
the per-call products square_unrolled() and mul_short_reg(); the whole body against pow()."""

import random

import pytest

from tests.asm_sim_chain import ChainLane
from tests.test_nadic_asm import GEN, KS, LB, L, MASK, R, consts, limbs, run, run_short, sq_pairs, SQ_UNROLLED

CH_SQ, CH_MS, CHAIN = GEN.chain_one(False), GEN.chain_one(True), GEN.chain_short()
NK, DADDR = 0x4000, 74 * 1024  # the LDS row of the pairs: the short product's 36, then the square's
B0, B1 = GEN.SB00, GEN.SB10


def short_pairs(N):
    return [v + (MASK if j < KS else 0) + (1 if j == 0 else 0) for j, v in enumerate(limbs(N - (1 << (LB * KS))))]


def pair_row(N):
    lds = {}
    for j, v in enumerate(short_pairs(N) + sq_pairs(N)):
        lds[DADDR + 8 * j], lds[DADDR + 8 * j + 4] = v, 0
    return lds


def _is_prime(n, rng):
    if n % 2 == 0:
        return False
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(24):
        x = pow(rng.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def small_biprime():
    """A biprime just above 2^262 (the short path's domain starts there): two 132-bit primes."""
    rng, ps = random.Random(262), []
    while len(ps) < 2:
        p = rng.getrandbits(132) | (1 << 131) | 1
        if _is_prime(p, rng):
            ps.append(p)
    assert ps[0] * ps[1] > 1 << 262
    return ps[0] * ps[1]


def run_one(N, a, h=None):
    """One product of the chain: X = a in the B registers; the result from the B registers."""
    words, np_ = consts(N)
    smem = {NK + 4 * i: w for i, w in enumerate(words)}
    args = {"p": DADDR + (0 if h is not None else GEN.KOFF), "NK": NK, "np": np_}
    if h is not None:
        args.update({f"h{i}": v for i, v in enumerate(limbs(h, KS))})
    lane = ChainLane(args, lds=pair_row(N), smem=smem)
    for k in range(L):
        lane.r[f"v{B0 + k}"], lane.r[f"v{B1 + k}"] = limbs(a[0])[k], limbs(a[1])[k]
    before = dict(args)
    lane.run(CH_MS if h is not None else CH_SQ)  # the simulator asserts every column below 2^64
    assert lane.args == before, "an asm input changed"
    out = [lane.r[f"v{B0 + k}"] for k in range(L)], [lane.r[f"v{B1 + k}"] for k in range(L)]
    assert all(v <= MASK for d in out for v in d)
    assert not any(k < 72 * 1024 for k in lane.lds), "a chain product touched the lane's LDS column"
    return tuple(sum(v << (LB * k) for k, v in enumerate(d)) for d in out)


def _moduli():
    from fedbiomed_amd import workload as W

    return [W.BIPRIME0, small_biprime()]


MODULI = _moduli()


@pytest.mark.parametrize("mi", [0, 1])
def test_chain_products_equal_the_per_call_products(mi):
    N, rng = MODULI[mi], random.Random(70 + mi)
    top = min(3 * N + 1, R - 1)  # (a digit has 36 limbs of 29 bits)
    hmax = (1 << (LB * KS)) - 1
    sq_cases = [(rng.randrange(2 * N), rng.randrange(2 * N)), (2 * N - 1, 2 * N - 1), (top, top), (hmax, 0)]
    for a in sq_cases:
        assert run_one(N, a) == run(N, a, square=SQ_UNROLLED)[:2]
    ms_cases = [((rng.randrange(2 * N), rng.randrange(2 * N)), rng.getrandbits(256)),
                ((2 * N - 1, 2 * N - 1), hmax), ((hmax, 0), hmax)]
    for a, h in ms_cases:
        got = run_one(N, a, h)
        assert got == run_short(N, a, h)[:2]
        assert run_one(N, got) == run(N, got, square=SQ_UNROLLED)[:2]  # digits up to 3N + 1 into the square


def test_looped_short_rows_variant(monkeypatch):
    """The generator's A/B switch: rows 1 .. 8 as a loop that rotates h's registers -- the same product, and
    the asm's input registers as they were."""
    monkeypatch.setattr(GEN, "CHAIN_SHORT_LOOPED", not GEN.CHAIN_SHORT_LOOPED)
    body = GEN.chain_one(True)
    assert len(body) != len(CH_MS)
    monkeypatch.setitem(globals(), "CH_MS", body)
    N, rng = MODULI[0], random.Random(9)
    for a, h in (((rng.randrange(2 * N), rng.randrange(2 * N)), rng.getrandbits(256)),
                 ((2 * N - 1, 2 * N - 1), (1 << (LB * KS)) - 1)):
        assert run_one(N, a, h) == run_short(N, a, h)[:2]


def run_chain(N, h, key):
    words, np_ = consts(N)
    KW = 0x8000
    smem = {NK + 4 * i: w for i, w in enumerate(words)}
    smem.update({KW + 4 * i: (key >> (32 * i)) & 0xFFFFFFFF for i in range(64)})
    args = {"a": 0, "d": DADDR, "kw": KW, "sb": key.bit_length() - 1, "NK": NK, "np": np_}
    args.update({f"h{i}": v for i, v in enumerate(limbs(h, KS))})
    lane = ChainLane(args, lds=pair_row(N), smem=smem)
    counts = lane.run(CHAIN, max_steps=100_000_000)
    out = [lane.lds[k * 1024] for k in range(2 * L)]
    assert all(v <= MASK for v in out)
    return (sum(v << (LB * k) for k, v in enumerate(out[:L])), sum(v << (LB * k) for k, v in enumerate(out[L:])),
            counts)


KEYS = [1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1, (1 << 64) + 1,
        random.Random(7).getrandbits(70) | (1 << 69)]


@pytest.mark.parametrize("mi", [0, 1])
def test_chain_body_is_the_power(mi):
    """Zero iterations (key 1), both bit values, both exponent-word boundaries: chain x C = h^key R^2."""
    N = MODULI[mi]
    M, rng = N * N, random.Random(5 + mi)
    for key in KEYS:
        h = rng.getrandbits(256) if key != 3 else (1 << (LB * KS)) - 1
        s = key.bit_length() - 1
        t, sd, counts = run_chain(N, h, key)
        C = pow(2, LB * L * ((1 << s) + 1) + LB * KS * (key - (1 << s)), M)  # the host's constant
        assert (t + sd * N) * C * pow(R, -2, M) % M == pow(h, key, M), hex(key)
        ones = bin(key).count("1") - 1
        assert counts.get("ds_write_b32", 0) == 2 * L                      # the exit's one store
        assert counts.get("ds_read_b64", 0) == L * (s + ones)              # 36 pairs per product, nothing else
        assert counts.get("ds_read_b32", 0) == 0
        assert counts.get("s_load_dword", 0) == (0 if s == 0 else 1 + (s - 1) // 32)
        mads = counts.get("v_mad_u64_u32", 0) + counts.get("v_mad_i64_i32", 0)
        assert mads == s * GEN.sq_mads() + ones * GEN.ms_mads()


def test_chain_counts():
    c = GEN.chain_counts()
    assert c["CHAIN_SQ"][1:] == (L, 0) and c["CHAIN_SHORT"][1:] == (L, 0)
    assert c["CHAIN_SQ"][0] <= c["CALL_SQ"][0] and c["CHAIN_SHORT"][0] <= c["CALL_SHORT"][0]
    assert c["CALL_SQ"][1] == 216 and c["CALL_SHORT"][1] == 180


def test_chain_header_matches_generator(tmp_path, capsys):
    """fbm_nadic_chain_asm.hpp is what the generator writes beside fbm_nadic_asm.hpp now."""
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("_hdr_chain", os.path.join(root, "tools", "gen_nadic_asm.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.OUT = str(tmp_path / "fbm_nadic_asm.hpp")
    mod.main()
    with open(tmp_path / mod.CHAIN_NAME) as f, open(os.path.join(root, "fedbiomed_amd", "csrc", mod.CHAIN_NAME)) as g:
        assert f.read() == g.read(), "fbm_nadic_chain_asm.hpp is stale: run python tools/gen_nadic_asm.py"


def test_shipped_header_expands_to_the_simulated_body():
    """The shipped header states the body through preprocessor macros (the generator's chain_macros): expanded
    by a C preprocessor, the asm text of fbm_na_chain_short is chain_short()'s instruction list, line for line."""
    import os
    import re
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "fedbiomed_amd", "csrc", GEN.CHAIN_NAME)) as f:
        src = "".join(ln for ln in f if not ln.startswith(("#include", "#pragma")))
    cpp = next((c for c in (os.environ.get("CC"), "gcc", "cc", "/opt/rocm/llvm/bin/clang") if c and shutil.which(c)), None)
    assert cpp, "no C preprocessor"
    out = subprocess.run([cpp, "-E", "-P", "-x", "c", "-"], input=src, capture_output=True, text=True, check=True).stdout
    asm = out[out.index("asm volatile("):]
    asm = asm[:re.search(r"\n\s*:\s*\n?\s*:\s*\[a\]", asm).start()]
    text = "".join(m.encode().decode("unicode_escape") for m in re.findall(r'"((?:[^"\\]|\\.)*)"', asm))
    assert text.splitlines() == CHAIN
    assert text.count("\n") == len(CHAIN)

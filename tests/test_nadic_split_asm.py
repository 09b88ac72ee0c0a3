"""The split exponentiation's assembly bodies (tools/gen_nadic_asm.py chain_modn / chain_seg,
fbm_na_chain_modn / fbm_na_chain_seg in fedbiomed_amd/csrc/fbm_nadic_chain_asm.hpp) on the CPU simulator.

|key| = k1 N + k0 and h^|key| = (h^k1 mod N)^N h^k0 (mod N^2).  Phase 1 (chain_modn) is the binary chain
with only the t half of the square and of the short product; phase 2 runs N's sliding-window schedule with
the chain's segments (chain_seg) over k0's bits between the window products.  Checked here: phase 1's
products limb for limb against the t half of the per-call products (whatever the s digit) and its whole
body against pow(h, k1, N); a segment limb for limb against the per-call products; the whole split
exponentiation, host constants included (a Python model of the host's: tests/test_split_host.py pins the
library's to the same formulas), against pow(h, key, N^2); the column bounds on intervals."""

import random

import pytest

from tests.asm_sim_chain import ChainLane
from tests.test_nadic_asm import GEN, KS, LB, L, MASK, R, SQ_UNROLLED, consts, limbs, run, run_short
from tests.test_nadic_chain_asm import DADDR, MODULI, NK, pair_row

MODN_SQ, MODN_MS, MODN, SEG = GEN.modn_one(False), GEN.modn_one(True), GEN.chain_modn(), GEN.chain_seg()
B0, B1 = GEN.SB00, GEN.SB10
KW = 0x8000
WIN = 6  # the library's window width (FBM_WIN)


def _smem(N, words32=None):
    words, np_ = consts(N)
    smem = {NK + 4 * i: w for i, w in enumerate(words)}
    if words32 is not None:
        smem.update({KW + 4 * i: (words32 >> (32 * i)) & 0xFFFFFFFF for i in range(64)})
    return smem, np_


def run_modn_one(N, x0, h=None):
    smem, np_ = _smem(N)
    args = {"NK": NK, "np": np_}
    if h is not None:
        args.update({f"h{i}": v for i, v in enumerate(limbs(h, KS))})
    lane = ChainLane(args, smem=smem)
    for k in range(L):
        lane.r[f"v{B0 + k}"] = limbs(x0)[k]
    before = dict(args)
    lane.run(MODN_MS if h is not None else MODN_SQ)
    assert lane.args == before and not lane.lds, "a phase-1 product touched LDS or an asm input"
    out = [lane.r[f"v{B0 + k}"] for k in range(L)]
    assert all(v <= MASK for v in out)
    return sum(v << (LB * k) for k, v in enumerate(out))


@pytest.mark.parametrize("mi", [0, 1])
def test_modn_products_are_the_t_half_of_the_per_call_products(mi):
    N, rng = MODULI[mi], random.Random(80 + mi)
    top = min(3 * N + 1, R - 1)
    hmax = (1 << (LB * KS)) - 1
    for x0 in (rng.randrange(2 * N), 2 * N - 1, top, hmax, 0):
        for x1 in (0, rng.randrange(2 * N), top):  # the t half never reads the s digit
            assert run_modn_one(N, x0) == run(N, (x0, x1), square=SQ_UNROLLED)[0]
        assert run_modn_one(N, x0) * R % N == x0 * x0 % N
    for x0, h in ((rng.randrange(2 * N), rng.getrandbits(256)), (2 * N - 1, hmax), (hmax, hmax)):
        got = run_modn_one(N, x0, h)
        assert got == run_short(N, (x0, rng.randrange(2 * N)), h)[0]
        assert got * (1 << (LB * KS)) % N == x0 * h % N
        assert run_modn_one(N, got) == run(N, (got, 0), square=SQ_UNROLLED)[0]  # digits up to 3N into the square


def run_modn(N, h, k1):
    smem, np_ = _smem(N, k1)
    args = {"a": 0, "kw": KW, "sb": k1.bit_length() - 1, "NK": NK, "np": np_}
    args.update({f"h{i}": v for i, v in enumerate(limbs(h, KS))})
    lds = {k * 1024: 0x1234567 for k in range(2 * L)}  # stale column contents: all overwritten
    lane = ChainLane(args, lds=lds, smem=smem)
    before = dict(args)
    counts = lane.run(MODN, max_steps=100_000_000)
    assert lane.args == before
    out = [lane.lds[k * 1024] for k in range(2 * L)]
    assert all(v <= MASK for v in out[:L]) and not any(out[L:]), "phase 1 stores (x0, 0)"
    return sum(v << (LB * k) for k, v in enumerate(out[:L])), counts


def f_of(e):
    """The power of two a binary chain over e leaves: h^e 2^-f."""
    s = e.bit_length() - 1
    return LB * L * ((1 << s) - 1) + LB * KS * (e - (1 << s))


K1S = [1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) + 1, random.Random(8).getrandbits(70) | (1 << 69)]


@pytest.mark.parametrize("mi", [0, 1])
def test_modn_chain_is_the_power_modulo_n(mi):
    """Zero iterations (k1 = 1), both bit values, both exponent-word boundaries: x0 2^f1 = h^k1 (mod N); no LDS
    access but the exit's store; the t half's multiply counts."""
    N, rng = MODULI[mi], random.Random(15 + mi)
    for k1 in K1S:
        h = rng.getrandbits(256) if k1 != 3 else (1 << (LB * KS)) - 1
        x0, counts = run_modn(N, h, k1)
        assert x0 * pow(2, f_of(k1), N) % N == pow(h, k1, N), hex(k1)
        s, ones = k1.bit_length() - 1, bin(k1).count("1") - 1
        assert counts.get("ds_write_b32", 0) == 2 * L
        assert counts.get("ds_read_b64", 0) == 0 and counts.get("ds_read_b32", 0) == 0
        assert counts.get("s_load_dword", 0) == (0 if s == 0 else 1 + (s - 1) // 32)
        mads = counts.get("v_mad_u64_u32", 0) + counts.get("v_mad_i64_i32", 0)
        assert mads == s * GEN.modn_sq_mads() + ones * GEN.modn_short_mads()
    assert GEN.modn_sq_mads() == 1968 and GEN.modn_short_mads() == 648


def run_seg(N, x, h, k0, hi, lo):
    smem, np_ = _smem(N, k0)
    args = {"a": 0, "d": DADDR, "kw": KW, "hi": hi, "lo": lo, "NK": NK, "np": np_}
    args.update({f"h{i}": v for i, v in enumerate(limbs(h, KS))})
    lds = pair_row(N)
    for k, v in enumerate(limbs(x[0]) + limbs(x[1])):
        lds[k * 1024] = v
    lane = ChainLane(args, lds=lds, smem=smem)
    before = dict(args)
    counts = lane.run(SEG, max_steps=100_000_000)
    assert lane.args == before
    out = [lane.lds[k * 1024] for k in range(2 * L)]
    assert all(v <= MASK for v in out)
    return (sum(v << (LB * k) for k, v in enumerate(out[:L])), sum(v << (LB * k) for k, v in enumerate(out[L:]))), counts


def per_call_seg(N, x, h, k0, hi, lo):
    for j in range(hi - 1, lo - 1, -1):
        x = run(N, x, square=SQ_UNROLLED)[:2]
        if (k0 >> j) & 1:
            x = run_short(N, x, h)[:2]
    return x


@pytest.mark.parametrize("mi", [0, 1])
def test_segment_equals_the_per_call_products(mi):
    """Bit ranges inside a word, across a word boundary, ending at bit 0, of one bit and of none (the column
    untouched, limb 35 included), from digits up to a general product's output bound."""
    N, rng = MODULI[mi], random.Random(90 + mi)
    k0 = rng.getrandbits(96) | (1 << 95) | (1 << 32) | 1
    h = rng.getrandbits(256)
    top = min(3 * N + 1, R - 1)
    for x, hi, lo in (((rng.randrange(2 * N), rng.randrange(2 * N)), 6, 2), ((2 * N - 1, 2 * N - 1), 35, 30),
                      ((top, top), 3, 0), ((rng.randrange(2 * N), 0), 33, 32), ((top, top), 64, 63)):
        got, counts = run_seg(N, x, h, k0, hi, lo)
        assert got == per_call_seg(N, x, h, k0, hi, lo), (hi, lo)
        ones = bin((k0 >> lo) & ((1 << (hi - lo)) - 1)).count("1")
        assert counts.get("ds_read_b32", 0) == 2 * L and counts.get("ds_write_b32", 0) == 2 * L
        assert counts.get("ds_read_b64", 0) == L * (hi - lo + ones)
    x = (top, top)
    got, counts = run_seg(N, x, h, k0, 40, 40)
    assert got == x and not counts.get("v_mad_u64_u32", 0) and not counts.get("ds_write_b32", 0)


def window_schedule(e, win=WIN):
    """[(squarings, table index or -1)] of a left-to-right sliding window over e > 0, from the accumulator 1:
    the library's schedule of N (the leading window an op like the others)."""
    ops, i, pend = [], e.bit_length() - 1, 0
    while i >= 0:
        if not (e >> i) & 1:
            pend, i = pend + 1, i - 1
            continue
        lo = max(i - win + 1, 0)
        while not (e >> lo) & 1:
            lo += 1
        val = (e >> lo) & ((1 << (i - lo + 1)) - 1)
        ops.append((pend + i - lo + 1, (val - 1) // 2))
        pend, i = 0, lo - 1
    if pend:
        ops.append((pend, -1))
    return ops


def digits(v, N):
    return (v % N, v // N)


def split_pow(N, h, key):
    """h^key R (mod N^2) the way jl_exp_kernel's split path sequences it, every product on the simulator."""
    M = N * N
    k1, k0 = divmod(key, N)
    assert k1 >= 1
    x0, _ = run_modn(N, h, k1)                                        # phase 1: h^k1 2^-f1 (mod N)
    c1 = pow(2, f_of(k1), N) * R * R % N
    g = run(N, (x0, 0), (c1, 0))[:2]                                  # g1 R (+ a multiple of N)
    table = [g]
    g2 = run(N, g)[:2]
    for _ in range(1, 1 << (WIN - 1)):
        table.append(run(N, table[-1], g2)[:2])
    x, j = digits(R % M, N), N.bit_length()                           # phase 2 from the Montgomery one
    for nsq, idx in window_schedule(N):
        x, _ = run_seg(N, x, h, k0, j, j - nsq)
        j -= nsq
        if idx >= 0:
            x = run(N, x, table[idx])[:2]
    assert j == 0
    cp = pow(2, LB * KS * k0, M) * R % M                              # C': the short products' 2^(-261 k0)
    return run(N, x, digits(cp, N))[:2]


def test_split_exponentiation_is_the_power():
    """The whole split path on the small biprime (264 bits: phase 2 stays short): keys N (k0 = 0), N + 1
    (an empty phase-1 chain), 2N - 1, a key whose k0 has its top bits set inside N's first window, a random
    key of twice N's length and N^2 - 1."""
    N = MODULI[1]
    M, rng = N * N, random.Random(33)
    nb = N.bit_length()
    k0_top = N - (1 << (nb - 4)) - 2  # below N, bits set among the six of N's first window
    assert 0 < k0_top < N and k0_top >> (nb - 6)
    keys = [N, N + 1, 5 * N + k0_top, M - 1]
    for key in keys:
        h = rng.getrandbits(256)
        t, s = split_pow(N, h, key)
        assert (t + s * N) % M == pow(h, key, M) * R % M, hex(key)


def test_split_exponentiation_default_biprime():
    """One key just above N on the 1024-bit default biprime: N's real schedule, a short phase 1."""
    from fedbiomed_amd import workload as W

    N = W.BIPRIME0
    M, rng = N * N, random.Random(34)
    key = 0x1D * N + (rng.getrandbits(1023) | (1 << 1022))
    assert key % N >> 1022
    h = rng.getrandbits(256)
    t, s = split_pow(N, h, key)
    assert (t + s * N) % M == pow(h, key, M) * R % M


def _bound_regs(lane, top, digits_=2):
    for k in range(L):
        iv = (0, MASK if k < L - 1 else top)
        lane.r[f"v{B0 + k}"] = iv
        if digits_ == 2:
            lane.r[f"v{B1 + k}"] = iv


def test_column_bounds_of_the_new_bodies():
    """tests/asm_bounds.py's interval run, for the input bounds the existing chain's products are proved for
    (digits < 2^1026: limb 35 < 2^11; any N < 2^1024; any np; h < 2^261): phase 1's square and short product,
    and the chain's own products that a segment runs (registers in, pairs from LDS)."""
    from tests.test_nadic_asm import KADDR, _bound_lane

    top = (1 << 11) - 1
    nmax = lambda j: MASK if j < L - 1 else (1 << 9) - 1  # noqa: E731
    kp = lambda j: (MASK, MASK + nmax(j))  # noqa: E731
    dp = lambda j: (MASK + (j == 0), 2 * MASK + 1) if j < KS else (0, nmax(j))  # noqa: E731
    hs = {f"h{i}": (0, MASK) for i in range(KS)}
    for body, short in ((MODN_SQ, False), (MODN_MS, True)):
        lane = _bound_lane(top)
        lane.args.update(hs)
        _bound_regs(lane, top, 1)
        lane.run(body)
        assert lane.max_mad < 1 << 64
    for short in (False, True):
        lane = _bound_lane(top, KADDR, dp if short else kp)
        lane.args.update(hs)
        lane.args["p"] = (KADDR, KADDR)
        _bound_regs(lane, top)
        lane.run(GEN.chain_one(short))
        assert lane.max_mad < 1 << 64

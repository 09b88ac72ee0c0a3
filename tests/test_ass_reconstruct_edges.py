"""Hostile operands for the additive-share reconstruct kernels (fbm_ass_reconstruct: ass_reconstruct_kernel and,
at 16 shares, ass_reconstruct_ws_kernel<8, 16>; fbm_ass_reconstruct_wide: ass_reconstruct_wide_kernel), and the
int128 / wide-limb dispatch of secagg/_additive_ss.py:_reconstruct.

The rest of the suite reconstructs only what a split made: shares in [0, 2^b] and one last share, whose
column sums are small.  The rows here are built in place.  The reference is Python's own sum, reduced to two's
complement at the kernel's width (the kernels wrap there by contract: the caller sizes the width); through the
class, where the Python layer picks the width, it is the plain sum.  Everything is exact integer equality.

Columns of a launch cycle through the patterns below, so every block of a launch holds all of them; a launch
of one element runs once per pattern.
  int128  all 2^127 - 1; all -2^127; alternating extremes that cancel to 0, to -1 and to +1; lo = 2^64 - 1 under
          hi = 0 (the carry out of the low word reaches P - 1); hi = -1 over lo = 0; random.
  wide    every limb 0xffffffff (-1: the carry into each limb reaches P - 1 and more); top limb 0x7fffffff over
          all-ones (the largest value); top limb 0x80000000 over zeros (the smallest); random.
"""

import random

import numpy as np
import pytest
import torch

from fedbiomed_amd import _device as D

I128_MAX, I128_MIN = 2**127 - 1, -(2**127)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return D.device()


def _wrap(v, bits):
    """v mod 2^bits read as a two's-complement value of that width."""
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


# ---- int128 lanes ----------------------------------------------------------------------------
def _alternate(P, a, b, tail):
    """a, b, a, b, ... over P rows; an odd P ends in `tail` instead of a."""
    col = [a if s % 2 == 0 else b for s in range(P)]
    if P % 2:
        col[-1] = tail
    return col


def _minus_one(P):
    col = _alternate(P, I128_MAX, -I128_MAX, 0 if P > 1 else -1)
    if P > 1:
        col[1] = I128_MIN  # 2^127 - 1, -2^127, then pairs that cancel
    return col


def _plus_one(P):
    col = _alternate(P, I128_MAX, -I128_MAX, 1)
    if P % 2 == 0:
        col[-1] += 1  # ..., 2^127 - 1, -(2^127 - 2)
    return col


I128_PATTERNS = {
    "max": lambda P, rnd: [I128_MAX] * P,
    "min": lambda P, rnd: [I128_MIN] * P,
    "cancel0": lambda P, rnd: _alternate(P, I128_MAX, -I128_MAX, 0),
    "cancel-1": lambda P, rnd: _minus_one(P),
    "cancel+1": lambda P, rnd: _plus_one(P),
    "lo_ones": lambda P, rnd: [2**64 - 1] * P,
    "hi_ones": lambda P, rnd: [-(2**64)] * P,
    "random": lambda P, rnd: [rnd.getrandbits(128) - 2**127 for _ in range(P)],
}
I128_NAMES = list(I128_PATTERNS)


def test_int128_patterns_are_what_they_say():
    rnd = random.Random(1)
    for P in (1, 2, 3, 15, 16, 17, 300):
        cols = {k: f(P, rnd) for k, f in I128_PATTERNS.items()}
        assert all(len(c) == P and all(I128_MIN <= v <= I128_MAX for v in c) for c in cols.values())
        assert sum(cols["cancel0"]) == 0 and sum(cols["cancel-1"]) == -1 and sum(cols["cancel+1"]) == 1
        if P > 1:
            assert I128_MAX in cols["cancel-1"] and I128_MIN in cols["cancel-1"] and I128_MAX in cols["cancel+1"]
        lo = D.ints_to_int128(cols["lo_ones"]).view(np.uint64)
        assert (lo[:, 0] == 2**64 - 1).all() and (lo[:, 1] == 0).all()
        assert sum(int(v) for v in lo[:, 0]) >> 64 == P - 1  # the carry out of the low word
        hi = D.ints_to_int128(cols["hi_ones"])
        assert (hi[:, 0] == 0).all() and (hi[:, 1] == -1).all()


def _int128_launch(P, n, shift):
    rnd = random.Random(1000 * P + n)
    cols = [I128_PATTERNS[I128_NAMES[(i + shift) % len(I128_NAMES)]](P, rnd) for i in range(n)]
    rows = np.stack([D.ints_to_int128([c[s] for c in cols]) for s in range(P)])  # [P, n, 2]
    return cols, rows


I128_CASES = [(P, n) for P in (1, 2, 3, 15, 16, 17, 300)
              for n in ((1, 63, 64, 65, 129) if P == 16 else (1, 255, 256, 257))]


@pytest.mark.gpu
@pytest.mark.parametrize("P,n", I128_CASES)
def test_reconstruct_int128_hostile_rows(dev, P, n):
    for shift in (range(len(I128_NAMES)) if n == 1 else (0,)):
        cols, rows = _int128_launch(P, n, shift)
        assert rows.shape == (P, n, 2)
        got = D.int128_to_ints(D.ass_reconstruct(torch.from_numpy(rows).to(dev)).cpu().numpy())
        want = [_wrap(sum(c), 128) for c in cols]
        bad = [(i, I128_NAMES[(i + shift) % len(I128_NAMES)], hex(g), hex(w))
               for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert len(got) == n and not bad, bad[:4]


# ---- wide limbs --------------------------------------------------------------------------------
WIDE_PATTERNS = {
    "ones": lambda L, rnd: -1,
    "top7f": lambda L, rnd: 2**(32 * L - 1) - 1,
    "top80": lambda L, rnd: -(2**(32 * L - 1)),
    "random": lambda L, rnd: rnd.getrandbits(32 * L) - 2**(32 * L - 1),
}
WIDE_NAMES = list(WIDE_PATTERNS)


def test_wide_patterns_are_what_they_say():
    for L in (1, 2, 3, 65):
        limbs = {k: D.ints_to_limbs_tc([f(L, random.Random(2))], L).view(np.uint32)[:, 0]
                 for k, f in WIDE_PATTERNS.items()}
        assert (limbs["ones"] == 0xFFFFFFFF).all()
        assert limbs["top7f"][-1] == 0x7FFFFFFF and (limbs["top7f"][:-1] == 0xFFFFFFFF).all()
        assert limbs["top80"][-1] == 0x80000000 and (limbs["top80"][:-1] == 0).all()


def _wide_launch(P, L, n, shift):
    """Column i: pattern (i + shift) in every row -- and, every fifth column, the patterns in turn down the rows."""
    rnd = random.Random(100 * P + L)
    cols = []
    for i in range(n):
        if i % 5 == 4:
            cols.append([WIDE_PATTERNS[WIDE_NAMES[(s + i) % 4]](L, rnd) for s in range(P)])
        else:
            cols.append([WIDE_PATTERNS[WIDE_NAMES[(i + shift) % 4]](L, rnd) for _ in range(P)])
    rows = np.stack([D.ints_to_limbs_tc([c[s] for c in cols], L) for s in range(P)])  # [P, L, n]
    return cols, rows


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 17, 300])
@pytest.mark.parametrize("L", [1, 2, 3, 65])
def test_reconstruct_wide_hostile_rows(dev, L, P):
    for n, shift in [(257, 0)] + [(1, k) for k in range(4)]:
        cols, rows = _wide_launch(P, L, n, shift)
        assert rows.shape == (P, L, n)
        got = D.limbs_tc_to_ints(D.ass_reconstruct_wide(torch.from_numpy(rows).to(dev)).cpu().numpy())
        want = [_wrap(sum(c), 32 * L) for c in cols]
        bad = [(n, i, hex(g), hex(w)) for i, (g, w) in enumerate(zip(got, want)) if g != w]
        assert len(got) == n and not bad, bad[:4]


# ---- the Python layer's dispatch -----------------------------------------------------------------
R_WIDTHS = tuple(range(118, 129))
R_PS = (2, 15, 16, 17, 31, 32)


def test_dispatch_sweep_lands_on_the_bound():
    """_reconstruct takes int128 lanes while bits + len(rows).bit_length() < 126: the sweep puts that sum on
    125, 126 and 127 (and well to both sides), at the wave-split kernel's 16 shares too."""
    sums = {(P, w + P.bit_length()) for P in R_PS for w in R_WIDTHS}
    for P in R_PS:
        assert {s for p, s in sums if p == P} >= {125, 126, 127}
    assert min(s for _, s in sums) <= 120 and max(s for _, s in sums) >= 134


@pytest.mark.gpu
@pytest.mark.parametrize("P", R_PS)
def test_reconstruct_dispatch_bound(dev, P):
    """AdditiveShares.reconstruct() of P shares whose widest value has w bits, w = 118 .. 128, both signs:
    list shares (all-largest, all-smallest, alternating, random and narrow columns) and int shares, against
    Python's sum -- whichever kernel the layer picked, and at whatever width."""
    from fedbiomed_amd.secagg import AdditiveShare, AdditiveShares

    rnd = random.Random(P)
    bad = []
    for w in R_WIDTHS:
        top = 2**w - 1
        for sign in (1, -1):
            cols = [[sign * top] * P,
                    [sign * top if s % 2 == 0 else -sign * top for s in range(P)],
                    [sign * rnd.getrandbits(w) for _ in range(P)],
                    [rnd.randrange(-top, top + 1) for _ in range(P)],
                    [sign * s for s in range(P)]]
            cols[3][0] = sign * top  # the launch's widest value has w bits in every column mix
            got = AdditiveShares([AdditiveShare([c[s] for c in cols]) for s in range(P)]).reconstruct()
            want = [sum(c) for c in cols]
            if got != want:
                bad.append((w, P, sign, "list", [hex(g - x) for g, x in zip(got, want)]))
            got = AdditiveShares([AdditiveShare(v) for v in cols[0]]).reconstruct()
            if got != sum(cols[0]):
                bad.append((w, P, sign, "int", hex(got - sum(cols[0]))))
    assert not bad, bad[:6]

"""Adversarial (numerator, divisor) pairs for the average step's int / int true division
(`fbm_true_div_u128`, fedbiomed_amd/csrc/fbm_common.hpp): plain Python, seeded, no project import.

`groups(width)` returns {divisor: [numerators below 2^width]} -- one launch has one divisor.  The LOM
aggregate takes width 64 (a column sum mod 2^64), the JL decode width 100 (a VES slot), fbm_int_ops width
128.  Per divisor W the families are

  ties        (2m + 1) W 2^sh, m a 53-bit value with its top bit set, of either parity: the exact quotient
              is a 54-bit odd number times 2^sh, halfway between two doubles (round half to even), and its
              neighbours at -1 and +1, where the remainder (the sticky bit) decides;
  carry-out   (2^54 - 1) W 2^sh and its neighbours: the rounded significand becomes 2^53;
  integer     m W - 1, m W, m W + 1 for m in [2^51, 2^53) and W >= 5: Python's quotient of m W - 1 rounds up
  boundary    to m, which a later truncation keeps and a truncating division turns into m - 1;
  fast/slow   numerators 2^53 - 1, 2^53, 2^53 + 1 (the routine's exact-double path ends at 2^53);
  extremes    0, 1, W - 1, W and 2^width - 1 (1 over 2^64 - 1 and all-ones over 1 are the widest gaps
              between the operands' bit lengths, either way);
  random      one seeded value of every bit length up to the width.

Only pairs that fit the width are kept.  `wrong_models` are four plausible wrong divisions; a list is
worth running only if each of them differs from Python's `/` on it (tests/test_true_div_edges.py checks
that on the CPU, for every list a device consumer runs)."""

import math
import random

DIVISORS = (1, 2, 3, 7, 10, 1000, 1023, 8017,  # small: ties are possible at every width
            2**32 - 1, 2**32 + 1,  # the 32-bit boundary
            2**53 - 1, 2**53, 2**53 + 1,  # the fast path's divisor edge
            2**63, 2**64 - 1)  # large
TIE_MANTISSAS = 3  # per parity and shift


def _shifts(width, bits):
    """Several shifts for a product of `bits` bits: the smallest, a middle one and the largest that fit."""
    top = width - bits
    return sorted({s for s in (0, 1, 2, top // 2, top - 1, top) if 0 <= s <= top})


def numerators(w, width, rng):
    """The families' numerators for divisor w, below 2^width, without repeats, in a fixed order."""
    lim = 1 << width
    out = []
    # ties and their neighbours
    for sh in _shifts(width, 54 + w.bit_length()):
        for parity in (0, 1):
            for _ in range(TIE_MANTISSAS):
                m = (1 << 52) | (rng.getrandbits(51) << 1) | parity
                t = ((2 * m + 1) * w) << sh
                out += [t - 1, t, t + 1]
    # carry-out of the rounded significand
    for sh in _shifts(width, 54 + w.bit_length()):
        t = (((1 << 54) - 1) * w) << sh
        out += [t - 1, t, t + 1]
    # integer boundary
    if w >= 5:
        hi = min(1 << 53, lim // w)
        for lo_m in (1 << 51, 1 << 52):
            if lo_m < hi:
                for m in (lo_m, rng.randrange(lo_m, min(hi, 2 * lo_m)), min(hi, 2 * lo_m) - 1):
                    out += [m * w - 1, m * w, m * w + 1]
    # the fast path's numerator edge, the extremes
    out += [2**53 - 1, 2**53, 2**53 + 1, 0, 1, w - 1, w, lim - 1]
    # every bit length
    out += [(1 << (b - 1)) | rng.getrandbits(b - 1) for b in range(1, width + 1)]
    seen, kept = set(), []
    for v in out:
        if 0 <= v < lim and v not in seen:
            seen.add(v)
            kept.append(v)
    return kept


def groups(width, seed=20250):
    """{divisor: numerators below 2^width} for every divisor of DIVISORS."""
    rng = random.Random(seed * 1000 + width)
    return {w: numerators(w, width, rng) for w in DIVISORS}


def pairs(width, seed=20250):
    return [(v, w) for w, vs in groups(width, seed).items() for v in vs]


def below_2_64(vs, w):
    """The numerators whose Python quotient reverse_quantize accepts (a float below 2^64)."""
    return [v for v in vs if v / w < 2.0**64]


# ------------------------------------------------------------------------------------------
# the routine, transcribed, with switches for the wrong versions
# ------------------------------------------------------------------------------------------
def model(a, b, rounding="even", sticky=True):
    """fbm_true_div_u128 step by step in Python ints (a < 2^128, 1 <= b < 2^64).  rounding: "even" (the
    routine), "up" (ties away from zero) or "none" (truncation); sticky=False ignores the remainder."""
    if a == 0:
        return 0.0
    if a < 2**53 and b < 2**53:  # exact doubles, one IEEE division: right in every version
        return float(a) / float(b)
    k = 55 - (a.bit_length() - b.bit_length())
    A, B = (a << k, b) if k >= 0 else (a, b << -k)
    q, r = divmod(A, B)
    extra = q.bit_length() - 53
    assert extra in (2, 3)
    low, half, m = q & ((1 << extra) - 1), 1 << (extra - 1), q >> extra
    st = sticky and r != 0
    if rounding == "even":
        up = low > half or (low == half and (st or m & 1))
    elif rounding == "up":
        up = low >= half
    else:
        up = False
    m += 1 if up else 0
    return math.ldexp(float(m), extra - k)  # exact: m <= 2^53


def _double_div(a, b):
    return float(a) / float(b)


wrong_models = {
    "truncation": lambda a, b: model(a, b, rounding="none"),
    "ties up": lambda a, b: model(a, b, rounding="up"),
    "no sticky bit": lambda a, b: model(a, b, sticky=False),
    "double / double": _double_div,
}

"""The JL exponentiation (fbm_jl_powmod: jl_exp_kernel, jl_expg_kernel<3|4>, the generic engine) on
caller-given bases, moduli and keys at the operands' edges, against Python integers: pow(h, key, N^2), times
(N pt + 1) with a plaintext.  No fixture: Python's pow is the reference, computed once per (N, |key|) for the
launch's ~22 distinct bases and shared by every engine and path parametrisation.

The rest of the suite feeds these kernels FDH digests (random, below 2^256), its own ciphertexts, random
odd moduli and random keys.  What each operand family here is for:

  BASES -- the wave-level short decision.  A wave takes the short chain only when every lane's h is below
  2^261 (`!__any(wide || mid)`); a narrow wave and a table-path wave of one workgroup then share the LDS
  constant pairs.  The launch (201 rows) is laid out in runs of 64:
      rows   0 ..  63  narrow only (h < 2^261);
      rows  64 .. 127  narrow, but row 101 is 2^261 (the smallest mid value: one lane turns its wave);
      rows 128 .. 191  narrow, mid (2^261 <= h < 2^1044), wide (h >= 2^1044) in turn: every wave mixes all three;
      rows 192 .. 200  a partial run (lanes past n_ct redo the last row and store nothing).
  `_assert_layout` checks, for the engine's ciphertexts per wave and per workgroup (64 / 256 single, 16 / 64
  quad, 21 / 84 triple; read back from the kernels' source by test_layout_constants_match_the_kernels), that
  some workgroup holds a narrow-only wave next to a wave with a row >= 2^261, that some wave mixes the three
  classes, and that every base of the pool is in the launch: a change of geometry that loses the edge fails.
  The values: 0 (non-negative keys), 1, 2, 3; 2^260, 2^261 - 1 | 2^261 (the short threshold), 2^290 - 1 (mid,
  yet inside the triple engine's lane-0 slice of limbs 0..11: the boundary sits inside one lane); 2^1043,
  2^1044 - 1 | 2^1044 (R: the wide threshold, h = h_lo + h_hi R); N - 1, N, N + 1 (closed form 1 + (key mod
  N) N, asserted too); N^2 - 1, N^2, N^2 + 1, 2^2047, 2^2048 - 1 (at and above the modulus: the library must
  compute or reduce them); seeded random values of 256, 1000 and 2048 bits.

  MODULI -- the host constant builders, na_final_digits, mont_csub.  BIPRIME0; 2^1024 - 105 (all-ones
  limbs); 2^1023 + 1 (sparse limbs, np = 2^29 - 1); 2^522 - 1 and 2^522 + 1 (divisors of R - 1 = 2^1044 - 1:
  K = 0, every K' limb 2^29 - 1; np = 1 and 2^29 - 1); 2^262 + 1 (the smallest modulus with a short
  schedule) and 2^262 - 1 (the largest that stays table-only).

  KEYS -- the schedule and the short chain's word reload at (j & 31) == 31.  1, 2, 3; 2^31, 2^32 - 1, 2^32,
  2^32 + 1, 2^64 - 1 (word boundaries); 2^1100 + 1 (a 1099-zero run: the window op needs the 1023-split);
  2^2047, 2^2047 + 1, 2^2048 - 1 (all 64 words set); sum 2^(6 k), k < 342 (one op per 6 bits: the densest
  schedule); a seeded 2040-bit key; each also negated (the inverse: jl_inv), and key 0 once.

Which pairs run: on the single, quad and triple engines every modulus takes every key.  On the generic
engine (a launch costs it ~0.4 s at a full-width key, whatever the row count) BIPRIME0 takes every key and each
other modulus the keys that stress it -- 2^2048 - 1, 2^2047, sum 2^(6 k), 2^1100 + 1 and 1, and their
negations.  Every modulus also runs one positive and one negative key with a plaintext, pt cycling 0, 1,
N - 1, N, 2^1024 - 1 over the rows.  Each (modulus, engine, path) is one test and the keys loop inside; the
generic engine's key lists are dealt into several tests (keysIofN) so that each stays within a few seconds.
Paths: short on and off where the modulus has a short schedule (N > 2^262); the generic engine has no short
path and never reads the switch (fbm_jl_powmod branches to it before build_short), so it runs once.

Negative keys use bases coprime to N by construction -- powers of two, 1, N +- 1, N^2 +- 1, and for
BIPRIME0 and 2^1024 - 105 the all-ones 2^261 - 1, 2^1044 - 1, 2^2048 - 1 (gcd asserted, never filtered).
Bases without an inverse (N, 0, and 3 under 2^522 - 1) have their own test: alone and inside an otherwise
invertible launch the call raises ZeroDivisionError."""

import math
import os
import random
import re

import numpy as np
import pytest

from fedbiomed_amd import workload as W

T_SHORT, T_WIDE = 1 << 261, 1 << 1044  # 9 and 36 limbs of 29 bits (FBM_NA_SHORT_LIMBS, FBM_NA_LIMBS)

MODULI = {
    "biprime0": W.BIPRIME0,
    "2p1024m105": (1 << 1024) - 105,
    "2p1023p1": (1 << 1023) + 1,
    "2p522m1": (1 << 522) - 1,
    "2p522p1": (1 << 522) + 1,
    "2p262p1": (1 << 262) + 1,
    "2p262m1": (1 << 262) - 1,
}
# ciphertexts per wave, per workgroup (fbm_jl.hip: FBM_BLOCK lanes of one; GroupEng<4>, GroupEng<3>)
GEOMETRY = {"single": (64, 256), "quad": (16, 64), "triple": (21, 84)}
ENGINES = ("single", "quad", "triple", "generic")

K_DENSE = sum(1 << (6 * k) for k in range(342))
K_RAND = random.Random(2040).getrandbits(2040) | (1 << 2039)
KEYS_ALL = [1, 2, 3, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 64) - 1, (1 << 1100) + 1, 1 << 2047,
            (1 << 2047) + 1, (1 << 2048) - 1, K_DENSE, K_RAND]
KEYS_STRESS = [(1 << 2048) - 1, 1 << 2047, K_DENSE, (1 << 1100) + 1, 1]
PT_KEYS = (K_DENSE, -((1 << 1100) + 1))

N_ROWS, MID_ROW = 201, 101


def _keys(mod, engine):
    if mod == "biprime0":
        return [s * k for k in KEYS_ALL for s in (1, -1)] + [0]
    return [s * k for k in (KEYS_STRESS if engine == "generic" else KEYS_ALL) for s in (1, -1)]


def _has_short(n):
    return n > (1 << 262)


def _cases():
    """(modulus, engine, short, (i, parts)): the test runs keys[i::parts] (an odd stride: both signs in each)."""
    out = []
    for m, n in MODULI.items():
        for e in ENGINES:
            if e == "generic":
                parts = 5 if m == "biprime0" else (3 if n.bit_length() > 1000 else 1)
                out += [pytest.param(m, e, True, (i, parts), id=f"{m}-{e}-keys{i + 1}of{parts}") for i in range(parts)]
            else:
                out += [pytest.param(m, e, s, (0, 1), id=f"{m}-{e}-{'short' if s else 'table'}")
                        for s in ((True, False) if _has_short(n) else (True,))]
    return out


def _pt_cases():
    return [pytest.param(m, e, s, id=f"{m}-{e}-{'short' if s else 'table'}") for m, n in MODULI.items() for e in ENGINES
            for s in ((True, False) if _has_short(n) and e != "generic" else (True,))]


def _cls(h):
    return 0 if h < T_SHORT else (1 if h < T_WIDE else 2)


def _pool(n, invertible):
    """The distinct bases of a launch, in a fixed order; `invertible`: only bases coprime to N by construction."""
    m = n * n
    if invertible:
        pool = [1, 2, 1 << 260, 1 << 261, 1 << 1043, 1 << 1044, n - 1, n + 1, m - 1, m + 1, 1 << 2047]
        if n in (MODULI["biprime0"], MODULI["2p1024m105"]):
            pool += [(1 << 261) - 1, (1 << 1044) - 1, (1 << 2048) - 1]
        assert all(math.gcd(h, n) == 1 for h in pool), "a base of the negative-key pool shares a factor with N"
        return pool
    rng = random.Random(n % 1000003)
    return [0, 1, 2, 3, 1 << 260, (1 << 261) - 1, 1 << 261, (1 << 290) - 1, 1 << 1043, (1 << 1044) - 1, 1 << 1044,
            n - 1, n, n + 1, m - 1, m, m + 1, 1 << 2047, (1 << 2048) - 1,
            rng.getrandbits(256) | (1 << 255), rng.getrandbits(1000) | (1 << 999), rng.getrandbits(2048) | (1 << 2047)]


_ROWS = {}


def _rows(n, invertible):
    """The launch's bases (see the module docstring's layout)."""
    if (n, invertible) not in _ROWS:
        pool = _pool(n, invertible)
        by_cls = [[h for h in pool if _cls(h) == c] for c in range(3)]
        narrow = by_cls[0]
        assert len(narrow) >= 3 and by_cls[1] and by_cls[2]
        rows = [narrow[i % len(narrow)] for i in range(64)]
        rows += [narrow[(i + 3) % len(narrow)] for i in range(64)]
        rows[MID_ROW] = T_SHORT
        rows += [by_cls[i % 3][(i // 3) % len(by_cls[i % 3])] for i in range(64)]
        rows += [pool[(5 * i + 11) % len(pool)] for i in range(N_ROWS - 192)]
        assert len(rows) == N_ROWS and set(rows) == set(pool) and all(0 <= h < (1 << 2048) for h in rows)
        _ROWS[(n, invertible)] = rows
    return _ROWS[(n, invertible)]


def _assert_layout(rows, ct_wave, ct_wg):
    """The launch keeps its edges under this engine's geometry: a workgroup with a narrow-only wave next to a
    wave that holds a row >= 2^261, a wave that mixes narrow, mid and wide rows, and both thresholds' values."""
    split_wg = mixed_wave = False
    for g0 in range(0, len(rows), ct_wg):
        wg = rows[g0:g0 + ct_wg]
        waves = [{_cls(h) for h in wg[w0:w0 + ct_wave]} for w0 in range(0, len(wg), ct_wave)]
        split_wg |= any(w == {0} for w in waves) and any(w - {0} for w in waves)
        mixed_wave |= any(w == {0, 1, 2} for w in waves)
    assert split_wg, "no workgroup holds a narrow-only wave next to a wave with a row >= 2^261"
    assert mixed_wave, "no wave mixes narrow, mid and wide rows"
    w0 = MID_ROW // ct_wg * ct_wg + (MID_ROW % ct_wg) // ct_wave * ct_wave  # the wave that 2^261 alone turns
    wave = rows[w0:min(w0 + ct_wave, MID_ROW // ct_wg * ct_wg + ct_wg)]
    assert [h for h in wave if h >= T_SHORT] == [T_SHORT], "row 2^261 is not the only wide-or-mid row of its wave"
    assert {T_SHORT, T_WIDE} <= set(rows)
    assert len(rows) % ct_wave and len(rows) % ct_wg, "no partial last wave"


_REF = {}


def _ref(n, key):
    """{h: pow(h, key, N^2)} over the launch's distinct bases: one pow per base and |key|, then shared; a negative
    key's is the positive one's inverse (over the coprime pool)."""
    if (n, key) not in _REF:
        m = n * n
        if key >= 0:
            _REF[(n, key)] = {h: pow(h, key, m) for h in _pool(n, False)}
        else:
            pos = _ref(n, -key)
            _REF[(n, key)] = {h: pow(pos[h], -1, m) for h in _pool(n, True)}
        assert _REF[(n, key)][n + 1] == (1 + (key % n) * n) % m  # (1 + N)^key = 1 + (key mod N) N
    return _REF[(n, key)]


def _limbs(vals, words):
    blob = b"".join(int(v).to_bytes(4 * words, "little") for v in vals)
    return np.frombuffer(blob, dtype="<u4").reshape(len(vals), words).view(np.int32)


_DEV = {}


def _on_device(tag, vals, words):
    import torch

    from fedbiomed_amd import _device as D

    if tag not in _DEV:
        _DEV[tag] = torch.from_numpy(_limbs(vals, words).copy()).to(D.device())
    return _DEV[tag]


def _pts(n):
    vals = [0, 1, n - 1, n, (1 << 1024) - 1]
    return [vals[i % len(vals)] for i in range(N_ROWS)]


def _run(n, key, engine, short, with_pt=False):
    from fedbiomed_amd import _device as D

    rows = _rows(n, key < 0)
    h = _on_device(("h", n, key < 0), rows, 64)
    pt = _on_device(("pt", n), _pts(n), 32) if with_pt else None
    with D.jl_engine(engine), D.jl_short(short):
        assert D.jl_engine_for(len(rows)) == engine
        out = D.jl_powmod(h, n, key, pt)
    return rows, D.limbs_to_ints(D.to_host(out).numpy().view(np.uint32))


def _compare(n, key, rows, got, want, what):
    bad = [i for i in range(len(rows)) if got[i] != want[i]]
    assert not bad, (f"{what}: {len(bad)} of {len(rows)} rows differ from Python, first at row {bad[0]} "
                     f"(base of {rows[bad[0]].bit_length()} bits, class {_cls(rows[bad[0]])}, key "
                     f"{'-' if key < 0 else ''}{abs(key).bit_length()} bits / {bin(abs(key)).count('1')} set): "
                     f"got {got[bad[0]]:#x} want {want[bad[0]]:#x}")


def test_layout_keeps_its_edges_under_every_engine():
    """CPU: the launch's layout assertions for every modulus, both pools and every engine's geometry."""
    for n in MODULI.values():
        for invertible in (False, True):
            for ct_wave, ct_wg in GEOMETRY.values():
                _assert_layout(_rows(n, invertible), ct_wave, ct_wg)


def test_layout_constants_match_the_kernels():
    """CPU: the geometry the layout is checked against is the kernels' (csrc/fbm_jl.hip)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "fedbiomed_amd", "csrc", "fbm_jl.hip")) as fh:
        src = fh.read()
    assert int(re.search(r"^#define FBM_BLOCK (\d+)", src, re.M).group(1)) == GEOMETRY["single"][1]
    got = {m.group(1): (int(m.group(2)), int(m.group(3)))
           for m in re.finditer(r"struct GroupEng<(\d)> \{[^}]*?CT_WAVE = (\d+), CT_WG = (\d+)", src)}
    assert got == {"4": GEOMETRY["quad"], "3": GEOMETRY["triple"]}
    assert GEOMETRY["single"][0] == 64  # the wave: `!__any(...)` decides per 64 lanes, one ciphertext each


def test_moduli_are_the_edges_they_claim():
    """CPU: the structural facts the module docstring states about the moduli."""
    R = 1 << 1044
    for name, n in MODULI.items():
        assert n % 2 == 1 and n.bit_length() <= 1024
        np29 = (-pow(n, -1, 1 << 29)) % (1 << 29)
        assert (np29 in (1, (1 << 29) - 1)) == (name != "biprime0" and name != "2p1024m105"), name
    assert (R - 1) % MODULI["2p522m1"] == 0 and (R - 1) % MODULI["2p522p1"] == 0  # K = R mod N - 1 = 0
    assert not _has_short(MODULI["2p262m1"]) and _has_short(MODULI["2p262p1"])


@pytest.mark.gpu
@pytest.mark.parametrize("mod,engine,short,part", _cases())
def test_powmod_matches_python(mod, engine, short, part):
    n = MODULI[mod]
    for key in _keys(mod, engine)[part[0]::part[1]]:
        rows, got = _run(n, key, engine, short)
        if engine in GEOMETRY:
            _assert_layout(rows, *GEOMETRY[engine])
        ref = _ref(n, key)
        _compare(n, key, rows, got, [ref[h] for h in rows], f"{mod} {engine} short={short}")
        closed = (1 + (key % n) * n) % (n * n)
        assert all(g == closed for h, g in zip(rows, got) if h == n + 1), "(1 + N)^key != 1 + (key mod N) N"


@pytest.mark.gpu
@pytest.mark.parametrize("mod,engine,short", _pt_cases())
def test_powmod_with_plaintext_matches_python(mod, engine, short):
    """(N pt + 1) h^key mod N^2 with pt at 0, 1, N - 1, N and 2^1024 - 1 (the nude operand's digit 1 at its
    extremes), a positive key (the exponentiation's last product) and a negative one (jl_inv's)."""
    n = MODULI[mod]
    m = n * n
    for key in PT_KEYS:
        rows, got = _run(n, key, engine, short, with_pt=True)
        ref = _ref(n, key)
        want = [(n * pt + 1) * ref[h] % m for h, pt in zip(rows, _pts(n))]
        _compare(n, key, rows, got, want, f"{mod} {engine} short={short} with pt")


@pytest.mark.gpu
@pytest.mark.parametrize("engine", ENGINES)
@pytest.mark.parametrize("mod,bad", [("biprime0", "N"), ("biprime0", "0"), ("2p522m1", "N"), ("2p522m1", "0"),
                                     ("2p522m1", "3")])
def test_base_without_inverse_raises(mod, bad, engine):
    """A negative key inverts h^|key|: a base that shares a factor with N has no inverse, alone in its launch
    or among invertible rows -- ZeroDivisionError, as jl_powmod's docstring promises (gmpy2.powmod's error)."""
    import torch

    from fedbiomed_amd import _device as D

    n = MODULI[mod]
    h = {"N": n, "0": 0, "3": 3}[bad]
    assert math.gcd(h, n) != 1
    with pytest.raises(ValueError):
        pow(h, -3, n * n)  # the reference: no inverse
    rows = list(_rows(n, True))
    rows[150] = h
    with D.jl_engine(engine):
        for launch in ([h], rows):
            t = torch.from_numpy(_limbs(launch, 64).copy()).to(D.device())
            with pytest.raises(ZeroDivisionError):
                D.jl_powmod(t, n, -3)

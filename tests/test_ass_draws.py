"""The device's own additive-share draws (fbm_ass_split: ass_split_kernel; fbm_ass_split_wide:
ass_split_wide_kernel), share for share against a model of them in Python integers (oracle/secagg_oracle.py:
ass_share_words, ass_share_draws and their _wide forms, on the oracle's ChaCha20).

The default split -- the one a deployment runs, a node's 2040-bit JL key included -- draws from ChaCha20 on
the device.  The rest of the suite sees it through its invariants only (exact sum, ranges, shards that
concatenate, draws that are not degenerate), and those hold for a kernel that hands two shares the same
keystream words, that can never draw the endpoint 2^b, that masks the wrong top word, or that reads a stale
block.  With a fixed seed and nonce the model makes every share an exact expectation:

  narrow  draw s of element i reads words 4 (s & 3) .. + 3 of block (elem_offset + i) ceil((P - 1) / 4) + (s >> 2)
          as a 128-bit little-endian x; the share is floor(x (2^b + 1) / 2^128).
  wide    draw s of element i reads the first b + 64 bits of the stream that starts at block
          ((elem_offset + i) (P - 1) + s) blocks, blocks = ceil((bmax + 64) / 512); the share is
          floor(x (2^b + 1) / 2^(b + 64)).
  both    the last share is secret - sum(draws).

CPU tests (unmarked) hold the model to what makes it a fit reference: the word ranges it reads are pairwise
disjoint over a launch and over adjacent shards, and at small b every value of [0, 2^b] -- the endpoint
2^b too -- occurs in every share row.  The GPU tests compare exact Python ints, no tolerance anywhere.

The class sweep (AdditiveSecret.split at the widths where its l_in / l_out / path decisions change) is
checked with Python's own sum of the shares, never the device's reconstruct: that wraps at the same width
and would hide a share that wrapped.  A negative secret with a given bit_length raises ValueError there, as
in the reference (log2 of a negative number, _additive_ss.py:90), so the given-bit_length sweeps put the
positive secrets through the split and pin the exception for the negative ones.
"""

import random

import numpy as np
import pytest
import torch

from fedbiomed_amd import _device as D
from oracle import secagg_oracle as O

SEED, NONCE = bytes(range(32)), b"abcdefgh"


# ---- CPU: the model itself -------------------------------------------------------------------
def _global_words(words):
    """Every keystream word (16 block + word) of a launch's draws, one entry per read."""
    return [16 * blk + w + j for row in words for blk, w, nw in row for j in range(nw)]


@pytest.mark.parametrize("draws", [1, 4, 5, 8, 9, 16])
def test_model_narrow_words_are_disjoint(draws):
    n, cut, off = 37, 20, 2**32 - 9
    whole = O.ass_share_words(n, draws + 1, off)
    assert len(whole) == draws and all(len(r) == n for r in whole)
    assert all(w + nw <= 16 and nw == 4 for row in whole for _, w, nw in row)  # a draw stays inside its block
    g = _global_words(whole)
    assert len(set(g)) == len(g) == 4 * draws * n
    # two shards with adjacent element ranges read what the unsharded launch reads, so nothing twice
    a, b = O.ass_share_words(cut, draws + 1, off), O.ass_share_words(n - cut, draws + 1, off + cut)
    assert [ra + rb for ra, rb in zip(a, b)] == whole
    # an element's blocks are its own: ceil(draws / 4) of them, next to its neighbour's
    bpe = (draws + 3) // 4
    assert {blk for row in whole for blk, _, _ in row} == set(range(off * bpe, (off + n) * bpe))


@pytest.mark.parametrize("blocks,bmax", [(1, 448), (2, 960), (5, 2040)])
def test_model_wide_words_are_disjoint(blocks, bmax):
    assert O.ass_wide_blocks(bmax) == blocks
    assert O.ass_wide_blocks(512 * blocks - 64) == blocks and O.ass_wide_blocks(512 * blocks - 63) == blocks + 1
    n, cut, off = 23, 11, 2**33 - 5
    bls = [bmax, 0, 1, bmax - 1] + [(7 * i) % (bmax + 1) for i in range(n - 4)]
    for draws in (1, 2, 16):
        whole = O.ass_share_words_wide(bls, draws + 1, blocks, off)
        assert all(w == 0 and nw == (b + 64 + 31) // 32 and nw <= 16 * blocks
                   for row in whole for (_, w, nw), b in zip(row, bls))  # a draw stays inside its blocks
        g = _global_words(whole)
        assert len(set(g)) == len(g)
        a = O.ass_share_words_wide(bls[:cut], draws + 1, blocks, off)
        b = O.ass_share_words_wide(bls[cut:], draws + 1, blocks, off + cut)
        assert [ra + rb for ra, rb in zip(a, b)] == whole
        starts = sorted(blk for row in whole for blk, _, _ in row)
        assert starts == [blocks * k for k in range(off * draws, (off + n) * draws)]


def test_model_reads_the_documented_stream():
    """The model's x against the keystream taken another way (chacha20_keystream from block 0): narrow draw
    (element 1, share 5) of a 9-share split is bytes [64 * 3 + 16, + 16) (block 1 * 2 + 1, words 4..7);
    wide draw (element 1, share 1) of a 3-share split with 2 blocks a draw is the stream from byte 64 * 6."""
    ks = O.chacha20_keystream(SEED, b"\x00" * 8 + NONCE, 64 * 16)
    x = int.from_bytes(ks[64 * 3 + 16:64 * 3 + 32], "little")
    assert O.ass_share_draws(SEED, NONCE, [64, 64], 9)[5][1] == (x * (2**64 + 1)) >> 128
    assert O.ass_share_draws(SEED, NONCE, [64], 9, elem_offset=1)[5][0] == (x * (2**64 + 1)) >> 128
    b = 700
    x = int.from_bytes(ks[64 * 6:64 * 8], "little") & (2**(b + 64) - 1)
    assert O.ass_share_draws_wide(SEED, NONCE, [3, b], 3, 2)[1][1] == (x * (2**b + 1)) >> (b + 64)
    rows = O.ass_split_model([10, -3], [[1, 2], [3, 4]])
    assert rows == [[1, 2], [3, 4], [6, -9]]


ENDPOINT_CASES = [("narrow", 0), ("narrow", 1), ("narrow", 2), ("wide", 0), ("wide", 1)]


def _endpoint_model(path, b):
    if path == "narrow":
        return O.ass_share_draws(SEED, NONCE, [b] * 2048, 4)
    return O.ass_share_draws_wide(SEED, NONCE, [b] * 512, 3, 1)


@pytest.mark.parametrize("path,b", ENDPOINT_CASES)
def test_model_reaches_every_value(path, b):
    rows = _endpoint_model(path, b)
    assert len(rows) == (3 if path == "narrow" else 2)
    for row in rows:
        assert set(row) == set(range(2**b + 1))


# ---- GPU -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return D.device()


def _assert_rows(got, want, what):
    """Exact equality of share rows, with the first differing (share, element) named."""
    assert len(got) == len(want), what
    for s, (g, w) in enumerate(zip(got, want)):
        if g != w:
            i = next(k for k, (a, b) in enumerate(zip(g, w)) if a != b) if len(g) == len(w) else -1
            raise AssertionError(f"{what}: share {s} of {len(want)}, element {i}: got {g[i]:#x}, model {w[i]:#x}")


# -- narrow path -------------------------------------------------------------------------------
N_NS = (1, 255, 256, 257, 1000)
N_PS = (1, 2, 5, 6, 9, 10, 17, 65)
N_BLS = (None, 0, 1, 2, 31, 32, 33, 63, 64)
N_OFFS = (0, 1, 2**32 - 3, 2**40)


def _narrow_cases():
    """72 launches: j walks the 8 x 9 (n_shares, bit_length) pairs (8 and 9 are coprime), n and the offset
    cycle with their own periods, the dtype follows the parity of (j mod 8) + (j mod 9).  Then the launches whose
    block counter crosses 2^32: offset 2^32 - 3 at one block an element; offset floor(2^32 / 5) - 1 at five
    blocks an element (18 shares: the crossing falls inside element 1) and, as listed, with 17 shares (four
    blocks: that launch stays below 2^32, so floor(2^32 / 4) - 1 with 17 shares crosses too)."""
    out = []
    for j in range(72):
        P, bl = N_PS[j % 8], N_BLS[j % 9]
        n, off = N_NS[(j + j // 8) % 5], N_OFFS[(j + j // 9) % 4]
        if off == 2**32 - 3 and P > 5:  # that offset goes with one block an element
            off = 2**40
        out.append((n, P, bl, bool((j % 8 + j % 9) & 1), off))
    for unsigned, P in ((False, 2), (True, 5)):
        out.append((257, P, None, unsigned, 2**32 - 3))
    out.append((256, 17, 33, False, 2**32 // 5 - 1))
    out.append((257, 18, None, True, 2**32 // 5 - 1))
    out.append((255, 17, 64, True, 2**32 // 4 - 1))
    return out


NARROW = _narrow_cases()


def _crosses_2_32(n, P, off):
    bpe = (P - 1 + 3) // 4
    return bpe > 0 and off * bpe < 2**32 < (off + n) * bpe


def test_narrow_parametrisation_holds_every_edge():
    for u in (False, True):
        mine = [c for c in NARROW if c[3] == u]
        assert {c[0] for c in mine} == set(N_NS) and {c[1] for c in mine} == set(N_PS) | ({18} if u else set())
        assert {c[2] for c in mine} == set(N_BLS) and {c[4] for c in mine} >= set(N_OFFS)
    assert {(c[1], c[2]) for c in NARROW} >= {(P, bl) for P in N_PS for bl in N_BLS}
    assert {(c[0], c[1]) for c in NARROW} >= {(n, P) for n in N_NS for P in N_PS}
    # one block an element across 2^32; five blocks an element with the crossing inside an element; four blocks
    cross = [c for c in NARROW if _crosses_2_32(c[0], c[1], c[4])]
    assert {(c[1] + 2) // 4 for c in cross} >= {1, 4, 5}
    assert any(c[4] == 2**32 - 3 and (c[1] + 2) // 4 == 1 for c in cross)
    assert any(c[4] == 2**32 // 5 - 1 and c[1] == 18 and 2**32 % 5 != 0 for c in cross)
    assert (256, 17, 33, False, 2**32 // 5 - 1) in NARROW
    assert len(NARROW) == 77
    for u in (False, True):  # a bit_length=None launch of 255 elements or more holds every b of 0 .. 64
        assert {abs(v).bit_length() for v in _narrow_secrets(255, None, u)} == set(range(65))


def _narrow_secrets(n, bl, unsigned):
    """bit_length=None: the edges, then one value (signed: and its negative) of every bit length, then random
    ones; a given bit_length: the dtype's extremes, then random ones."""
    rnd = random.Random(n * 131 + (64 if bl is None else bl) * 2 + unsigned)
    if unsigned:
        vals = [0, 1, 2**31, 2**32, 2**63 - 1, 2**63, 2**64 - 1] + [2**(b - 1) for b in range(1, 65)]
    else:
        vals = [0, 1, -1, 2**31, -(2**31), 2**32, -(2**32), 2**63 - 1, -(2**63)]
        vals += [s * 2**(b - 1) for b in range(1, 64) for s in (1, -1)]
    if bl is not None:
        vals = vals[:9]
    while len(vals) < n:
        w = rnd.randrange(65)
        vals.append(rnd.getrandbits(w) if unsigned else rnd.getrandbits(w) - (2**w >> 1))
    vals = vals[:n]
    assert all((0 if unsigned else -(2**63)) <= v < (2**64 if unsigned else 2**63) for v in vals)
    return vals


def _split_narrow(dev, vals, P, bl, unsigned, off):
    host = np.array([v - 2**64 if v >= 2**63 else v for v in vals], dtype=np.int64)
    got = D.ass_split(torch.from_numpy(host).to(dev), P, bl, unsigned=unsigned, seed=SEED, nonce=NONCE,
                      elem_offset=off)
    assert got.shape == (P, len(vals), 2)
    return [D.int128_to_ints(s) for s in got.cpu().numpy()]


@pytest.mark.gpu
@pytest.mark.parametrize("n,P,bl,unsigned,off", NARROW,
                         ids=[f"n{c[0]}-P{c[1]}-b{c[2]}-{'u' if c[3] else 'i'}64-off{c[4]:#x}" for c in NARROW])
def test_narrow_split_equals_model(dev, n, P, bl, unsigned, off):
    vals = _narrow_secrets(n, bl, unsigned)
    bls = [abs(v).bit_length() if bl is None else bl for v in vals]
    want = O.ass_split_model(vals, O.ass_share_draws(SEED, NONCE, bls, P, off))
    assert all(0 <= r <= 2**b for row in want[:-1] for r, b in zip(row, bls))
    _assert_rows(_split_narrow(dev, vals, P, bl, unsigned, off), want, f"n={n} P={P} bit_length={bl} off={off}")


@pytest.mark.gpu
@pytest.mark.parametrize("path,b", ENDPOINT_CASES)
def test_device_reaches_every_value(dev, path, b):
    """The endpoint cases of test_model_reaches_every_value on the device: equal to the model, and every
    value of [0, 2^b], 2^b included, in every share row the kernel wrote."""
    draws = _endpoint_model(path, b)
    if path == "narrow":
        vals = list(range(2048))
        got = _split_narrow(dev, vals, 4, b, False, 0)
    else:
        vals = list(range(-256, 256))
        got = _split_wide(dev, vals, 1, 3, _min_l_out(1, b, 3), b, 0)
    _assert_rows(got, O.ass_split_model(vals, draws), f"{path} b={b}")
    for row in got[:-1]:
        assert set(row) == set(range(2**b + 1))


# -- wide path ---------------------------------------------------------------------------------
W_BLS = (0, 1, 31, 32, 33, 63, 64, 65, 447, 448, 449, 959, 960, 961, 1984, 2040)
W_PS = (1, 2, 3, 17)
W_OFFS = (0, 7, 2**33)
W_NONE = [0, 1, -1, 2**31, -(2**31), 2**32, -(2**32), -(2**32 + 1), 2**127, -(2**127), 2**159 - 1, -(2**159)]


def _min_l_out(l_in, bmax, P):
    """The smallest l_out fbm_ass_split_wide accepts: l_in, and the words of bmax + ceil(log2 P) + 2 bits."""
    return max(l_in, (bmax + (P - 1).bit_length() + 2 + 31) // 32)


def _wide_cases():
    """(n, l_in, P, bit_length, extra limbs over the smallest l_out, offset).  Every bit length twice, with
    two of the drawing share counts 2, 3, 17, both l_out settings, two offsets and both n; n_shares = 1 (no
    draw: the secret comes back sign-extended) and the per-element launches (bit_length None, l_in 5) after."""
    out = []
    for j, bl in enumerate(W_BLS):
        out.append((257 if j & 1 else 1, 3 if j & 1 else 1, W_PS[1 + j % 3], bl, 0, W_OFFS[j % 3]))
        out.append((1 if j & 1 else 257, 1 if j & 1 else 3, W_PS[1 + (j + 1) % 3], bl, 3, W_OFFS[(j + 2) % 3]))
    out += [(257, 3, 1, 65, 0, 7), (1, 5, 1, None, 3, 0)]
    out += [(257, 5, 3, None, 0, 7), (257, 5, 17, None, 3, 2**33), (1, 5, 2, None, 0, 0)]
    return out


WIDE = _wide_cases()


def test_wide_parametrisation_holds_every_edge():
    assert {c[3] for c in WIDE} == set(W_BLS) | {None} and {c[2] for c in WIDE} == set(W_PS)
    assert {c[5] for c in WIDE} == set(W_OFFS) and {c[0] for c in WIDE} == {1, 257}
    for bl in W_BLS:  # each bit length: two drawing share counts, l_out smallest and + 3, two offsets, both n
        mine = [c for c in WIDE if c[3] == bl and c[2] > 1]
        assert len({c[2] for c in mine}) == 2 and {c[4] for c in mine} == {0, 3}
        assert len({c[5] for c in mine}) == 2 and {c[0] for c in mine} == {1, 257}
    assert {(c[2], c[4]) for c in WIDE if c[3] is None} >= {(3, 0), (17, 3)}
    # b + 64 on a block edge, one bit either side of the first two; b + 64 a multiple of 32 (the top-word mask)
    assert {448, 960, 1984} <= set(W_BLS) and {447, 449, 959, 961} <= set(W_BLS)
    assert all((b + 64) % 512 == 0 for b in (448, 960, 1984))
    assert {b for b in W_BLS if (b + 64) % 32 == 0} >= {0, 32, 64, 448, 960, 1984}
    assert {O.ass_wide_blocks(b) for b in W_BLS} == {1, 2, 3, 4, 5}
    # the per-element launch: the minimum of l_in = 5 limbs has b = 32 l_in
    assert abs(W_NONE[-1]).bit_length() == 160 and W_NONE[-1] == -(2**(32 * 5 - 1))
    assert len(WIDE) == 37


def _wide_secrets(n, l_in, bl):
    rnd = random.Random(n * 7 + l_in)
    if bl is None:
        vals = list(W_NONE)
        while len(vals) < n:
            w = rnd.randrange(32 * l_in)
            vals.append(rnd.getrandbits(w) - (2**w >> 1))
        return vals[:n] if n > 1 else [W_NONE[-1]]
    # headroom under the limbs: the last share, secret - sum(draws), must fit the smallest l_out
    top = 32 * l_in - 6
    vals = [-(2**top), 2**top - 1, 0, -1, 1]
    while len(vals) < n:
        vals.append(rnd.getrandbits(top + 1) - 2**top)
    return vals[:n]


def _split_wide(dev, vals, l_in, P, l_out, bl, off):
    sec = torch.from_numpy(D.ints_to_limbs_tc(vals, l_in)).to(dev)
    got = D.ass_split_wide(sec, P, l_out, bl, seed=SEED, nonce=NONCE, elem_offset=off)
    assert got.shape == (P, l_out, len(vals))
    return [D.limbs_tc_to_ints(s) for s in got.cpu().numpy()]


@pytest.mark.gpu
@pytest.mark.parametrize("n,l_in,P,bl,extra,off", WIDE,
                         ids=[f"n{c[0]}-lin{c[1]}-P{c[2]}-b{c[3]}-lout+{c[4]}-off{c[5]:#x}" for c in WIDE])
def test_wide_split_equals_model(dev, n, l_in, P, bl, extra, off):
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError

    vals = _wide_secrets(n, l_in, bl)
    bmax = 32 * l_in if bl is None else bl
    l_out = _min_l_out(l_in, bmax, P)
    bls = [abs(v).bit_length() if bl is None else bl for v in vals]
    want = O.ass_split_model(vals, O.ass_share_draws_wide(SEED, NONCE, bls, P, O.ass_wide_blocks(bmax), off))
    assert all(0 <= r <= 2**b for row in want[:-1] for r, b in zip(row, bls))
    assert all(-(2**(32 * l_out - 1)) <= v < 2**(32 * l_out - 1) for row in want for v in row)  # nothing wraps
    if l_out > l_in and not extra:  # it is the smallest: one limb fewer is refused
        with pytest.raises(FedbiomedSecaggCrypterError):
            _split_wide(dev, vals, l_in, P, l_out - 1, bl, off)
    _assert_rows(_split_wide(dev, vals, l_in, P, l_out + extra, bl, off), want,
                 f"n={n} l_in={l_in} P={P} bit_length={bl} l_out={l_out + extra} off={off}")


# -- through the class: the Python layer's sizing ------------------------------------------------
C_KS = (62, 63, 64, 65, 94, 95, 96, 97, 126, 127, 128, 129, 2046, 2047, 2048, 2049)
C_PS = (2, 3, 5, 9, 17, 33, 257)
C_BLS = ("none", "k", "k+1", "300")


@pytest.mark.gpu
@pytest.mark.parametrize("P", C_PS)
@pytest.mark.parametrize("mode", C_BLS)
def test_class_split_sizing(dev, mode, P):
    """AdditiveSecret(v).split(P[, bit_length]) for v = +-(2^k - 1), +-2^k around every width at which the layer
    changes path or limb count: Python's sum of the shares is the secret and the first P - 1 lie in
    [0, 2^b].  Where the reference raises (a negative secret or a bit_length below int(log2(v)), with a
    bit_length given) the split raises the same; every failing (k, P, v) is collected and named."""
    from fedbiomed_amd.exceptions import FedbiomedValueError
    from fedbiomed_amd.secagg import AdditiveSecret

    bad, ran = [], 0
    for k in C_KS:
        bl = {"none": None, "k": k, "k+1": k + 1, "300": 300}[mode]
        for name, v in (("2^k-1", 2**k - 1), ("-(2^k-1)", -(2**k - 1)), ("2^k", 2**k), ("-2^k", -(2**k))):
            tag = f"k={k} P={P} v={name} bit_length={bl}"
            if bl is not None and (v < 0 or bl < v.bit_length() - 1):
                with pytest.raises(ValueError if v < 0 else FedbiomedValueError):
                    AdditiveSecret(v).split(P, bl)
                continue
            shares = AdditiveSecret(v).split(P, bl).to_list()
            ran += 1
            b = abs(v).bit_length() if bl is None else bl
            if len(shares) != P or not all(isinstance(s, int) for s in shares):
                bad.append((tag, "shape"))
            elif sum(shares) != v:
                bad.append((tag, f"sum is off by {sum(shares) - v:#x}"))
            elif not all(0 <= s <= 2**b for s in shares[:-1]):
                bad.append((tag, "a share outside [0, 2^b]"))
    assert not bad, bad
    assert ran == {"none": 64, "k": 32, "k+1": 32, "300": 24}[mode]

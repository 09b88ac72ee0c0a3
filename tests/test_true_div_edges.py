"""The average step's int / int true division (`fbm_true_div_u128`, fedbiomed_amd/csrc/fbm_common.hpp) at the
operands where a hand-written rounding goes wrong -- constructed ties, the carry out of the significand, the
fast/slow boundary, quotients just below an integer (tests/true_div_cases.py) -- on the host and in each of
its device consumers: `int_ops_kernel` (ops 1, 2, 3), `lom_aggregate_kernel`, both `lom_aggregate_ws_kernel`
forms and the host-buffer call, and `jl_decode_kernel`.  Every comparison is of float64 bit patterns against
Python's own `/` (the operation the reference's `_apply_average` runs, `_secagg_crypter.py:233-249`,
`_secagg_utils.py:137-149`) or the oracle's `reverse_quantize` of it (`_secagg_utils.py:152-187`).

The aggregates show the quotient only through the dequantiser, -c + step * trunc(q).  With clip = 2^52 and
target = 2^53 + 1 that is trunc(q) - 2^52 with step == 1.0: exact for every q < 2^64 and one-to-one, so a
quotient that is off by an ulp is an output that is off.  That the lists tell a wrong division from the right
one at all is checked on the CPU (test_lists_expose_wrong_models), so the GPU tests cannot pass vacuously.

`SecaggLomCrypter.begin_aggregate().finish()` ends in `lom_aggregate` of its one accumulator row, the P = 1
launch below."""

import ctypes

import numpy as np
import pytest

from oracle import secagg_oracle as O
from tests import true_div_cases as C

CLIP, TARGET = 2**52, 2**53 + 1
JL_DIVISORS = (1, 7, 2**53 + 1, 2**64 - 1)
JL_SLOT, JL_SLOT_64 = (100, 10), (64, 16)
JL_DIVISOR_64 = 1023


def _bits(xs):
    return np.asarray(xs, dtype=np.float64).view(np.uint64).tolist()


# ------------------------------------------------------------------ the lists each consumer runs
def int_ops_lists():
    return C.groups(128)


def lom_lists():
    return {w: C.below_2_64(vs, w) for w, vs in C.groups(64).items()}


def jl_lists():
    """[(slot, divisor, numerators)]: four divisors at the 100-bit slot, one at a 64-bit slot.  The guard
    leaves few of the 100-bit list's ties for a small divisor (q < 2^64), so the 64-bit list's ride along."""
    from fedbiomed_amd import workload as W

    g, g64 = C.groups(100), C.groups(64)
    out = [(JL_SLOT, w, C.below_2_64(list(dict.fromkeys(g[w] + g64[w])), w)) for w in JL_DIVISORS]
    es, cr = JL_SLOT_64  # 16 slots of 64 bits fill the plaintext's 1024: its top slot has to keep it below N
    vs = _top_slot_below(C.below_2_64(g64[JL_DIVISOR_64], JL_DIVISOR_64), cr, W.BIPRIME0 >> (es * (cr - 1)))
    out.append((JL_SLOT_64, JL_DIVISOR_64, vs))
    return out


def _top_slot_below(vs, cr, lim):
    """A permutation of vs whose every cr-th value, a packed plaintext's top slot, is below lim."""
    n_top = len(vs) // cr
    top_at = [i for i, v in enumerate(vs) if v < lim][:n_top]
    assert len(top_at) == n_top
    skip = set(top_at)
    tops, rest = iter([vs[i] for i in top_at]), iter([v for i, v in enumerate(vs) if i not in skip])
    return [next(tops) if i % cr == cr - 1 else next(rest) for i in range(len(vs))]


def _dequantised(quotients):
    return _bits(O.reverse_quantize(quotients, CLIP, TARGET))


def _odd_part(q):
    return q >> ((q & -q).bit_length() - 1)


# ------------------------------------------------------------------ CPU
def test_case_lists_are_as_specified():
    """Every divisor and family is present at each width, nothing exceeds the width, and the lists are
    reproducible (seeded)."""
    for width in (64, 100, 128):
        g = C.groups(width)
        assert tuple(g) == C.DIVISORS and g == C.groups(width)
        for w, vs in g.items():
            assert all(0 <= v < 2**width for v in vs) and len(set(vs)) == len(vs)
            assert {0, 1, w - 1, w, 2**width - 1, 2**53 - 1, 2**53, 2**53 + 1} <= set(vs)
            assert {v.bit_length() for v in vs} >= set(range(1, width + 1))
            if 54 + w.bit_length() <= width:  # exact ties of either parity, a carry-out
                ties = [_odd_part(v // w) for v in vs if v and v % w == 0 and _odd_part(v // w).bit_length() == 54]
                m = [t >> 1 for t in ties]  # the 53 bits kept: the tie goes to the even one
                assert any(x & 1 for x in m) and any(not x & 1 for x in m) and 2**53 - 1 in m
        assert sum(len(vs) for vs in g.values()) >= 1000
    assert (1, 2**64 - 1) in C.pairs(64) and (2**128 - 1, 1) in C.pairs(128)
    assert 2**64 - 1 not in lom_lists()[1] and 2**64 - 1 in lom_lists()[2]
    from fedbiomed_amd import workload as W

    for (es, cr), w, vs in jl_lists():  # every value fits its slot, every packed plaintext is below N
        assert all(v < 2**es and v / w < 2.0**64 for v in vs) and len(set(vs)) == len(vs)
        assert all(pt < W.BIPRIME0 for pt in O.ves_encode(vs, es, cr))
    assert sorted(jl_lists()[-1][2]) == sorted(C.below_2_64(C.groups(64)[JL_DIVISOR_64], JL_DIVISOR_64))


def test_model_is_pythons_division():
    """The transcription the wrong models are cut from agrees with Python's `/` on the 128-bit list."""
    for v, w in C.pairs(128):
        assert _bits([C.model(v, w)]) == _bits([v / w]), (v, w)


def test_host_routine_vs_python():
    """The routine as the host compiles it (test hook fbm_test_true_div_u128) against Python's `v / k` on the
    128-bit list: float64 bit patterns."""
    from fedbiomed_amd import _native as N

    lib = N.load_test()
    total = 0
    for w, vs in C.groups(128).items():
        x = np.array([[v & (2**64 - 1), v >> 64] for v in vs], dtype=np.uint64)
        out = np.full(len(vs), np.nan)
        rc = lib.fbm_test_true_div_u128(ctypes.c_void_p(x.ctypes.data), len(vs), w, ctypes.c_void_p(out.ctypes.data))
        assert rc == 0, N.last_error()
        got, want = _bits(out), _bits([v / w for v in vs])
        bad = [(v, w) for v, g, e in zip(vs, got, want) if g != e]
        assert not bad, bad[:5]
        total += len(vs)
    assert total >= 1000
    assert lib.fbm_test_true_div_u128(ctypes.c_void_p(x.ctypes.data), 1, 0, ctypes.c_void_p(out.ctypes.data)) != 0


def test_lists_expose_wrong_models():
    """A condition on the inputs, not on the code: through each consumer's visible output -- the float itself
    for fbm_int_ops, the dequantised value for the aggregates -- truncation, ties rounded up, a dropped sticky
    bit and double(a) / double(b) each differ from Python on at least 10 cases of the list that consumer runs.
    (float(v), op 2's conversion, is v / 1: there double / double is the conversion itself, not a wrong one.)"""
    pairs = C.pairs(128)
    for name, wrong in C.wrong_models.items():
        assert sum(_bits([wrong(v, w)]) != _bits([v / w]) for v, w in pairs) >= 10, ("int_ops 1/3", name)
        if name != "double / double":
            vals = int_ops_lists()[1]
            for kd in (7.0, 7.5):
                assert sum(_bits([wrong(v, 1) / kd]) != _bits([v / kd]) for v in vals) >= 10, ("int_ops 2", name)
        lom = [(v, w) for w, vs in lom_lists().items() for v in vs]
        got, want = _dequantised([wrong(v, w) for v, w in lom]), _dequantised([v / w for v, w in lom])
        assert sum(g != e for g, e in zip(got, want)) >= 10, ("lom", name)
        jl = [(v, w) for _, w, vs in jl_lists() for v in vs]
        got, want = _dequantised([wrong(v, w) for v, w in jl]), _dequantised([v / w for v, w in jl])
        assert sum(g != e for g, e in zip(got, want)) >= 10, ("jl", name)


def test_dequantiser_is_one_to_one_here():
    """clip = 2^52, target = 2^53 + 1: -c = -2^52 and step = 1.0 exactly, so the aggregates' output is
    trunc(q) - 2^52, exact below 2^64; and the guard's two sides."""
    from fedbiomed_amd import _device as D

    assert D.dequant_params(CLIP, TARGET) == (-2.0**52, 1.0)
    assert (2**64 - 1025) / 1 == 2.0**64 - 2048 and (2**64 - 1024) / 1 == 2.0**64 == (7 * 2**64 - 1) / 7
    assert _dequantised([2.0**64 - 2048]) == _bits([2.0**64 - 2048 - 2.0**52])
    with pytest.raises(O.OracleError, match="Cannot reverse quantize"):
        O.reverse_quantize([2.0**64], CLIP, TARGET)


# ------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_int_ops_kernel_vs_python():
    """fbm_int_ops ops 1 (+k), 3 (-k) and 2 (float(k), and k + 0.5) on the 128-bit list, one launch per divisor
    and op: Python's `v / k` bit for bit (the W = 1 group holds op 2's float(v) ties, odd54 * 2^sh)."""
    from fedbiomed_amd import _device as D

    for w, vs in int_ops_lists().items():
        t = D.ints_to_u128(vs)
        for k in (w, -w, float(w), float(w) + 0.5):
            got, want = _bits(D.int_true_divide(t, k)), _bits([v / k for v in vs])
            bad = [(v, k) for v, g, e in zip(vs, got, want) if g != e]
            assert not bad, bad[:5]


def _rows(rng, P, sums):
    """Random u64 rows whose column sums mod 2^64 are `sums` (as tests/test_agg_ws.py's)."""
    y = np.frombuffer(rng.bytes(8 * P * len(sums)), dtype=np.uint64).reshape(P, len(sums)).copy()
    with np.errstate(over="ignore"):
        y[P - 1] = np.array(sums, dtype=np.uint64) - np.sum(y[:P - 1], axis=0, dtype=np.uint64)
    return y


def _padded(vs, rng, P, odd):
    """The list at a length of the parity asked for; for 8 and 16 parties at least one full 128-element
    tile and a tail."""
    vs = list(vs)
    if P in (8, 16):
        vs += [rng.integers(1, 2**62) for _ in range(max(0, 130 - len(vs)))]
    if len(vs) % 2 != odd:
        vs.append(int(rng.integers(1, 2**62)))
    if P in (8, 16) and len(vs) % 128 == 0:
        vs += [5, 6]
    return [int(v) for v in vs]


def _lom_check(y, w, host=False, kernel=None):
    import torch

    from fedbiomed_amd import _device as D

    want = _bits(O.lom_crypter_aggregate(y, w, CLIP, TARGET))
    if host:
        got = _bits(D.lom_aggregate_host(y, w, CLIP, TARGET))
    else:
        Y = torch.from_numpy(y.view(np.int64)).to(D.device())
        assert D.lom_aggregate_kernel(y.shape[0], Y).startswith(kernel)
        out, sums = D.lom_aggregate(Y, w, clip=CLIP, target=TARGET, want_sums=True)
        assert np.array_equal(sums.cpu().numpy().view(np.uint64), O.lom_aggregate(y))
        got = _bits(out.cpu().numpy())
    s = O.lom_aggregate(y).tolist()
    bad = [(v, w) for v, g, e in zip(s, got, want) if g != e]
    assert not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 5, 8, 16])
def test_lom_aggregate_vs_oracle(P):
    """The 64-bit list as column sums, one launch per divisor: lom_aggregate_kernel (1 and 5 parties, an even
    length and an odd one for the element-access path) and lom_aggregate_ws_kernel (8 and 16 parties, a full tile
    and a tail) against the oracle's LOM.aggregate + _apply_average + reverse_quantize in Python ints."""
    from fedbiomed_amd import _device as D

    assert D.dequant_params(CLIP, TARGET) == (-2.0**52, 1.0)
    rng = np.random.default_rng(5300 + P)
    for w, vs in lom_lists().items():
        for odd in ((0, 1) if P in (1, 5) else (0,)):
            sums = _padded(vs, rng, P, odd)
            assert len(sums) % 2 == odd and (P in (1, 5) or (len(sums) > 128 and len(sums) % 128))
            _lom_check(_rows(rng, P, sums), w,
                       kernel="lom_aggregate_ws_kernel<" if P in (8, 16) else "lom_aggregate_kernel<")


@pytest.mark.gpu
def test_lom_aggregate_host_call_vs_oracle():
    """One divisor group with ties through the host-buffer call (fbm_lom_aggregate_host)."""
    rng = np.random.default_rng(5307)
    _lom_check(_rows(rng, 3, lom_lists()[7]), 7, host=True)


@pytest.mark.gpu
def test_jl_decode_vs_oracle():
    """The 100-bit list through one party's encrypt and jl_decode_kernel (slot (100, 10); one group at
    (64, 16)): the decoded sums are the list and the averages the oracle's reverse_quantize of Python's `/`."""
    from fedbiomed_amd import _device as D, workload as W

    key, tau = 0x5DEECE66D, 11
    for slot, w, vs in jl_lists():
        assert len(vs) >= 100
        cts = D.jl_encrypt(D.ints_to_u128(vs), W.BIPRIME0, key, tau, 1, kind="u128", slot=slot)
        out, sums = D.jl_aggregate(cts[None], W.BIPRIME0, -key, tau, len(vs), w, clip=CLIP, target=TARGET, slot=slot,
                                   want_sums=True)
        assert D.u128_to_ints(sums) == vs
        got, want = _bits(out.cpu().numpy()), _dequantised(O.apply_average(vs, w))
        bad = [(v, w) for v, g, e in zip(vs, got, want) if g != e]
        assert not bad, bad[:5]


@pytest.mark.gpu
def test_range_guard_at_its_edge():
    """reverse_quantize's guard on the rounded quotient: (2^64 - 1025) / 1 = 2^64 - 2048 is the largest that
    passes; (2^64 - 1024) / 1 is a tie that rounds to even, 2^64, and raises the reference's error (as the
    oracle does), and so does (7 * 2^64 - 1) / 7 in the JL decode.  Each in a launch of its own, among valid
    elements, on the device-tensor call, the host-buffer call and the JL aggregate."""
    import torch

    from fedbiomed_amd import _device as D, workload as W
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError

    rng = np.random.default_rng(64)
    valid = [3, 2**53 + 1, 2**63 + 12345, 10**12, 7]
    last_ok = valid[:2] + [2**64 - 1025] + valid[2:]
    want = _dequantised([v / 1 for v in last_ok])
    assert want[2] == _bits([2.0**64 - 2048 - 2.0**52])[0]
    key, tau = 0x5DEECE66D, 12

    def lom(vs, host):
        y = _rows(rng, 2, vs)
        if host:
            return _bits(D.lom_aggregate_host(y, 1, CLIP, TARGET))
        return _bits(D.lom_aggregate(torch.from_numpy(y.view(np.int64)).to(D.device()), 1, clip=CLIP,
                                     target=TARGET)[0].cpu().numpy())

    def jl(vs, w):
        cts = D.jl_encrypt(D.ints_to_u128(vs), W.BIPRIME0, key, tau, 1, kind="u128", slot=JL_SLOT)
        return _bits(D.jl_aggregate(cts[None], W.BIPRIME0, -key, tau, len(vs), w, clip=CLIP, target=TARGET,
                                    slot=JL_SLOT)[0].cpu().numpy())

    assert lom(last_ok, False) == want and lom(last_ok, True) == want and jl(last_ok, 1) == want
    tie = valid[:2] + [2**64 - 1024] + valid[2:]
    for run in (lambda: lom(tie, False), lambda: lom(tie, True), lambda: jl(tie, 1),
                lambda: jl(valid[:2] + [7 * 2**64 - 1] + valid[2:], 7)):
        with pytest.raises(FedbiomedSecaggCrypterError, match="Cannot reverse quantize"):
            run()

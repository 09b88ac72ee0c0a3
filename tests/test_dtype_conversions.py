"""The conversions behind the 16-bit inputs (FBM_F16 / FBM_BF16) and the narrow outputs (the *_as entry points),
run on the host through the test build's hooks fbm_test_widen16 / fbm_test_narrow: the same host/device source
the kernels run (fedbiomed_amd/csrc/fbm_common.hpp).  No GPU.

Widening is exact -- the reference's `encrypt` takes List[float] (fedbiomed/common/secagg/_secagg_crypter.py:45,
318), so a 16-bit parameter reaches its quantiser as the Python float of that value: all 65 536 patterns of each
type against host torch's `.double()`.  Narrowing is what `torch.tensor(v, dtype=float64).to(dtype)` gives on the
host (float64 -> float32 RN-even, and the 16-bit types from that float32), bitwise, on every representable
value, every midpoint between neighbours and its two double neighbours, the double-rounding cases, overflow and
random doubles.
"""
import ctypes

import numpy as np
import pytest
import torch

from fedbiomed_amd import _native as N
from oracle import secagg_oracle as O

HALVES = {"f16": (torch.float16, N.FBM_F16), "bf16": (torch.bfloat16, N.FBM_BF16)}
NARROW = {**HALVES, "f32": (torch.float32, N.FBM_F32)}


@pytest.fixture(scope="module")
def lib():
    from fedbiomed_amd import _build

    _build.build()
    return N.load_test()


def all_patterns(dtype) -> torch.Tensor:
    """Every bit pattern of a 16-bit dtype, in pattern order."""
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def widen(lib, code) -> np.ndarray:
    out = np.empty(65536, dtype=np.float64)
    d = ctypes.c_double()
    for b in range(65536):
        assert lib.fbm_test_widen16(b, code, ctypes.byref(d)) == 0
        out[b] = d.value
    return out


def narrow(lib, vals: np.ndarray, code) -> np.ndarray:
    out = np.empty(len(vals), dtype=np.uint32)
    w = ctypes.c_uint32()
    for i, v in enumerate(vals.tolist()):
        assert lib.fbm_test_narrow(v, code, ctypes.byref(w)) == 0
        out[i] = w.value
    return out


def torch_narrow(vals: np.ndarray, dtype) -> np.ndarray:
    """The bits of torch's host conversion of float64 values to dtype, zero-extended to uint32."""
    t = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float64)).to(dtype)
    if dtype == torch.float32:
        return t.view(torch.int32).numpy().view(np.uint32).copy()
    return t.view(torch.int16).numpy().view(np.uint16).astype(np.uint32)


def is_nan_bits(bits: np.ndarray, dtype) -> np.ndarray:
    if dtype == torch.float32:
        return (bits & 0x7FFFFFFF) > 0x7F800000
    inf = 0x7C00 if dtype == torch.float16 else 0x7F80
    return (bits & 0x7FFF) > inf


def assert_narrow_matches(lib, vals, name):
    dtype, code = NARROW[name]
    vals = np.asarray(vals, dtype=np.float64)
    got, want = narrow(lib, vals, code), torch_narrow(vals, dtype)
    gn, wn = is_nan_bits(got, dtype), is_nan_bits(want, dtype)
    assert np.array_equal(gn, wn)
    bad = np.nonzero((got != want) & ~gn)[0]
    assert bad.size == 0, [(vals[i].hex(), hex(got[i]), hex(want[i])) for i in bad[:5]]


@pytest.mark.parametrize("name", sorted(HALVES))
def test_widening_is_exact_on_every_pattern(lib, name):
    dtype, code = HALVES[name]
    got = widen(lib, code)
    want = all_patterns(dtype).double().numpy()
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])  # signed zeros, subnormals, inf
    # the inputs the issue names: the subnormal extremes are normal doubles, not flushed
    tiny = all_patterns(dtype)[1].double().item()
    assert got[1] == tiny > 0 and got[0x8001] == -tiny and np.signbit(got[0x8000]) and got[0x8000] == 0


def representable(dtype) -> np.ndarray:
    """Every finite value of a narrow dtype as a double, ascending, zero once."""
    if dtype == torch.float32:
        # a float32 sample: the edges of every binade, the denormals' ends, and seeded patterns
        rng = np.random.default_rng(32)
        bits = np.concatenate([np.arange(0, 0x7F800000, 1 << 23, dtype=np.int64) + d for d in (0, 1, 2, (1 << 23) - 1)]
                              + [rng.integers(0, 0x7F800000, 20000)])
        v = np.unique(bits[bits < 0x7F800000].astype(np.uint32)).view(np.float32).astype(np.float64)
        return np.unique(np.concatenate([-v, v]))
    v = all_patterns(dtype).double().numpy()
    return np.unique(v[np.isfinite(v)])


@pytest.mark.parametrize("name", sorted(NARROW))
def test_narrowing_of_every_16_bit_value(lib, name):
    """The exact double of every finite pattern of BOTH 16-bit types (a binary16 value rounds in bfloat16 and
    the other way round), and every value the target itself represents (float32: a sample), which must come
    back as itself."""
    both = np.concatenate([representable(torch.float16), representable(torch.bfloat16)])
    assert_narrow_matches(lib, np.unique(np.concatenate([both, representable(NARROW[name][0])])), name)


@pytest.mark.parametrize("name", sorted(NARROW))
def test_narrowing_at_the_midpoints(lib, name):
    """Ties and their double neighbours: the midpoint of each pair of neighbouring representable values (exact
    in float64: at most 25 significant bits) and that midpoint -/+ 1 ulp of double.  For the 16-bit types a
    midpoint +/- 1 ulp is where the FIRST rounding, to float32, makes the tie that one rounding would not."""
    v = representable(NARROW[name][0])
    if name == "f32":  # neighbours of a sample are not neighbours in float32: step to the true one
        with np.errstate(over="ignore"):  # (the step past FLT_MAX is inf: dropped below)
            nxt = np.nextafter(v.astype(np.float32), np.float32(np.inf)).astype(np.float64)
        mid = (v + nxt) / 2
        mid = mid[np.isfinite(mid)]
    else:
        mid = (v[:-1] + v[1:]) / 2
    pts = np.concatenate([mid, np.nextafter(mid, -np.inf), np.nextafter(mid, np.inf)])
    assert_narrow_matches(lib, pts, name)


def test_double_rounding_cases(lib):
    """The two values the fused output is defined by: one rounding would give 1.0078125 / 1.0009765625."""
    b = ctypes.c_uint32()
    lib.fbm_test_narrow(1 + 2.0**-8 + 2.0**-40, N.FBM_BF16, ctypes.byref(b))
    assert b.value == 0x3F80 == torch_narrow(np.array([1 + 2.0**-8 + 2.0**-40]), torch.bfloat16)[0]
    lib.fbm_test_narrow(1 + 2.0**-11 + 2.0**-40, N.FBM_F16, ctypes.byref(b))
    assert b.value == 0x3C00 == torch_narrow(np.array([1 + 2.0**-11 + 2.0**-40]), torch.float16)[0]
    for name in NARROW:
        assert_narrow_matches(lib, [1 + 2.0**-8 + 2.0**-40, 1 + 2.0**-11 + 2.0**-40], name)


def test_overflow_underflow_and_specials(lib):
    special = [np.inf, -np.inf, 0.0, -0.0, np.nan, 65504.0, -65504.0, 65519.99, 65520.0, -65520.0, 1e-8, -1e-8,
               3.4e38, 6.8e38, -6.8e38, 2.0**-24, 2.0**-25, 2.0**-149, 2.0**-150, 2.0**-151, 5e-324, 1.7976931348623157e308]
    for name in NARROW:
        assert_narrow_matches(lib, special, name)
    b = ctypes.c_uint32()
    lib.fbm_test_narrow(65520.0, N.FBM_F16, ctypes.byref(b))
    assert b.value == 0x7C00  # past 65 504 + half an ulp: +inf, as IEEE and torch
    lib.fbm_test_narrow(65519.99, N.FBM_F16, ctypes.byref(b))
    assert b.value == 0x7BFF
    lib.fbm_test_narrow(6.8e38, N.FBM_BF16, ctypes.byref(b))
    assert b.value == 0x7F80
    lib.fbm_test_narrow(-np.inf, N.FBM_F32, ctypes.byref(b))
    assert b.value == 0xFF800000


@pytest.mark.parametrize("name", sorted(NARROW))
def test_narrowing_random_doubles(lib, name):
    assert_narrow_matches(lib, np.random.default_rng(7).uniform(-3, 3, 100_000), name)


def test_hooks_refuse_other_dtypes(lib):
    d, b = ctypes.c_double(), ctypes.c_uint32()
    assert lib.fbm_test_widen16(1, N.FBM_F32, ctypes.byref(d)) == N.FBM_E_ARG
    assert lib.fbm_test_narrow(1.0, N.FBM_F64, ctypes.byref(b)) == N.FBM_E_ARG
    assert lib.fbm_test_narrow(1.0, N.FBM_U64, ctypes.byref(b)) == N.FBM_E_ARG


@pytest.mark.parametrize("name", sorted(HALVES))
@pytest.mark.parametrize("clip", [1, 3, 2**16, None])
def test_oracle_quantises_every_pattern(name, clip):
    """The expected input of the GPU test over all patterns (tests/test_half_inputs.py): the oracle's quantiser
    takes every pattern as a double without raising, NaN -> T - 1, and at clip 1 the binary16 subnormals map to
    distinct integers (so a kernel that flushed them would be seen)."""
    T = 2**40
    x = all_patterns(HALVES[name][0]).double().numpy()
    q = O.quantize(x, clip, T)
    assert q.dtype == np.uint64 and q.shape == (65536,) and int(q.max()) == T - 1
    assert np.all(q[np.isnan(x)] == T - 1)
    c = 3 if clip is None else clip
    assert np.all(q[x > c] == T - 1) and np.all(q[x < -c] == 0)
    if name == "f16" and clip == 1:
        sub = q[1:0x400]  # the positive subnormals, ascending
        assert np.all(np.diff(sub.astype(np.int64)) > 0)

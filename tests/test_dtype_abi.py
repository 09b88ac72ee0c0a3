"""The C ABI's additions for 16-bit inputs and narrow outputs (include/fbm_secagg.h, still ABI 7: additions only):
the dtype codes FBM_F16 / FBM_BF16, the four *_as entry points and the two host hooks are declared, exported and
bound; an out_dtype that is no floating-point code is FBM_E_ARG with a message; the entry points that take no
quantised input (additive sharing) still refuse the new codes.  Argument checks only: no kernel runs, no GPU.
No reference counterpart: the reference's crypter takes and returns Python lists
(fedbiomed/common/secagg/_secagg_crypter.py:45,139,318,394)."""
import ctypes
import os
import re

import pytest

from fedbiomed_amd import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AS_ENTRY_POINTS = ["fbm_lom_aggregate_as", "fbm_jl_aggregate_as", "fbm_jl_aggregate_factor_as", "fbm_dequantize_as"]
HOOKS = ["fbm_test_widen16", "fbm_test_narrow"]


@pytest.fixture(scope="module")
def libs():
    from fedbiomed_amd import _build

    _build.build()
    return N.load(), N.load_test()


def _header(name):
    with open(os.path.join(ROOT, "include", name)) as fh:
        return fh.read()


def test_dtype_codes():
    h = _header("fbm_secagg.h")
    assert re.search(r"^#define FBM_F16 6\b", h, re.M) and re.search(r"^#define FBM_BF16 7\b", h, re.M)
    assert (N.FBM_F16, N.FBM_BF16) == (6, 7)
    assert re.search(r"^#define FBM_ABI_VERSION 7\b", h, re.M)  # additions only


def test_as_entry_points_declared_exported_and_bound(libs):
    prod, test = libs
    h = _header("fbm_secagg.h")
    for name in AS_ENTRY_POINTS:
        assert re.search(rf"^int {name}\(", h, re.M), name
        assert name in N.SIGNATURES and hasattr(prod, name) and hasattr(test, name)
        # the namesake's signature with `double* out` as `void* out, int out_dtype`
        base, args = N.SIGNATURES[name[:-3]][1], N.SIGNATURES[name][1]
        assert any(args[i] is ctypes.c_int and args[i - 1] is ctypes.c_void_p and args[:i] + args[i + 1:] == base
                   for i in range(1, len(args))), name


def test_hooks_in_the_test_build_only(libs):
    prod, test = libs
    th = _header("fbm_secagg_test.h")
    for name in HOOKS:
        assert re.search(rf"^int {name}\(", th, re.M) and name in N.TEST_SIGNATURES
        assert hasattr(test, name) and not hasattr(prod, name)


@pytest.mark.parametrize("bad", [99, -1, N.FBM_U64, N.FBM_I64, N.FBM_U128, N.FBM_PT])
def test_bad_out_dtype_is_an_argument_error(libs, bad):
    lib, _ = libs
    z = None  # the dtype is checked before any pointer is read
    calls = {
        "fbm_dequantize_as": lambda: lib.fbm_dequantize_as(z, 0, -3.0, 1.0, z, bad, z),
        "fbm_lom_aggregate_as": lambda: lib.fbm_lom_aggregate_as(z, 2, 0, 1, -3.0, 1.0, z, bad, z, z, z),
        "fbm_jl_aggregate_as": lambda: lib.fbm_jl_aggregate_as(z, 2, 0, 34, 30, 0, z, z, 0, z, 0, 1, -3.0, 1.0, z, bad,
                                                               z, z, z, z),
        "fbm_jl_aggregate_factor_as": lambda: lib.fbm_jl_aggregate_factor_as(z, 2, 0, 34, 30, 0, z, z, 1, -3.0, 1.0, z,
                                                                             bad, z, z, z, z),
    }
    for name, call in calls.items():
        assert call() == N.FBM_E_ARG, name
        assert "out_dtype" in N.last_error() and str(bad) in N.last_error(), (name, N.last_error())


def test_additive_sharing_refuses_the_16_bit_codes(libs):
    lib, _ = libs
    seed, nonce = ctypes.create_string_buffer(32), ctypes.create_string_buffer(8)
    args = (0, 3, 8, ctypes.addressof(seed), ctypes.addressof(nonce), 0, None, None)
    assert lib.fbm_ass_split(None, N.FBM_U64, *args) == N.FBM_OK  # (an empty secret: nothing launched)
    for code in (N.FBM_F16, N.FBM_BF16):
        assert lib.fbm_ass_split(None, code, *args) == N.FBM_E_ARG
        assert "64-bit secrets" in N.last_error()


def test_python_dtype_mapping():
    import torch

    from fedbiomed_amd import _device as D

    assert D._x_dtype(torch.empty(0, dtype=torch.float16)) == N.FBM_F16
    assert D._x_dtype(torch.empty(0, dtype=torch.bfloat16)) == N.FBM_BF16
    assert D._OUT_DTYPES == {torch.float64: N.FBM_F64, torch.float32: N.FBM_F32, torch.float16: N.FBM_F16,
                             torch.bfloat16: N.FBM_BF16}
    out = torch.empty(5, dtype=torch.bfloat16)
    assert D._out_tensor(5, out.device, None, out)[0] is out
    for bad in (dict(out_dtype=torch.float16, out=out), dict(out_dtype=None, out=out[:4]),
                dict(out_dtype=None, out=torch.empty(10, dtype=torch.bfloat16)[::2]),
                dict(out_dtype=torch.int32, out=None)):
        with pytest.raises(ValueError):
            D._out_tensor(5, out.device, bad["out_dtype"], bad["out"])

"""Streaming aggregation without a GPU: the C ABI's two additions (fbm_jl_fold, fbm_lom_fold: declared, bound,
exported by both builds, the ABI still 7), their argument errors that return before any device call, and the
crypters' accumulator objects where no device work is needed -- the wrong-count FB624 at finish, the type
errors at add, use after finish / abort, a zero-length party.  No reference counterpart: the reference's
aggregate takes every node's list at once (fedbiomed/common/secagg/_secagg_crypter.py:139-230, 394-455)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from fedbiomed_amd import _native as N
from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError
from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOLDS = ["fbm_jl_fold", "fbm_lom_fold"]
BIPRIME = 2**61 - 1  # (any odd N: the checks under test come before the modulus is looked at)


@pytest.fixture(scope="module")
def libs():
    from fedbiomed_amd import _build

    _build.build()
    return N.load(), N.load_test()


def _header():
    with open(os.path.join(ROOT, "include", "fbm_secagg.h")) as fh:
        return fh.read()


def test_declared_bound_and_still_abi_7(libs):
    prod, test = libs
    h = _header()
    assert re.search(r"^#define FBM_ABI_VERSION 7\b", h, re.M) and N.ABI_VERSION == 7 and prod.fbm_abi_version() == 7
    for name in FOLDS:
        assert re.search(rf"^int {name}\(", h, re.M), name
        assert name in N.SIGNATURES and hasattr(prod, name) and hasattr(test, name)
    # the header's argument lists, pointer for pointer
    c_vp, c_int, c_u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    assert N.SIGNATURES["fbm_jl_fold"] == (c_int, [c_vp, c_vp, c_int, c_u64, c_vp, c_int, c_vp, c_vp])
    assert N.SIGNATURES["fbm_lom_fold"] == (c_int, [c_vp, c_vp, c_int, c_u64, c_int, c_vp])
    assert "_jls.py:353-374" in h and "_lom.py:177-192" in h  # each entry cites the reference lines it stands for


def test_product_library_exports_exactly_its_header(libs):
    from fedbiomed_amd import _build

    nm = shutil.which("nm")
    if nm is None:
        pytest.skip("nm not found")
    out = subprocess.run([nm, "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("fbm_")}
    declared = set(_build.declared(os.path.join(ROOT, "include", "fbm_secagg.h")))
    assert exported == declared
    assert set(FOLDS) <= exported and declared == set(N.SIGNATURES)


def test_jl_fold_argument_errors(libs):
    lib, _ = libs
    bp = (ctypes.c_uint32 * 32)(*([BIPRIME & 0xFFFFFFFF, BIPRIME >> 32] + [0] * 30))
    bpp = ctypes.addressof(bp)
    one = ctypes.addressof(ctypes.create_string_buffer(256))  # a non-null stand-in: never read before the refusal
    for k in (0, -1):
        assert lib.fbm_jl_fold(one, one, k, 4, bpp, 0, one, None) == N.FBM_E_ARG, k
        assert N.last_error()
    assert lib.fbm_jl_fold(one, one, 1, 4, None, 1, one, None) == N.FBM_E_ARG  # null biprime
    for k, seed in ((2, 1), (9, 8), (1, -1)):  # more rows than the accumulator was seeded for
        assert lib.fbm_jl_fold(one, one, k, 4, bpp, seed, one, None) == N.FBM_E_ARG, (k, seed)
        assert "seeded" in N.last_error()
    assert lib.fbm_jl_fold(one, one, 1, 14_000_001, bpp, 1, one, None) == N.FBM_E_UNSUPPORTED  # FBM_JL_MAX_CT
    assert lib.fbm_jl_fold(None, None, 1, 0, bpp, 1, None, None) == N.FBM_OK  # n_ct == 0: nothing to do
    for acc, rows, ws in ((None, one, one), (one, None, one), (one, one, None)):
        assert lib.fbm_jl_fold(acc, rows, 1, 4, bpp, 1, ws, None) == N.FBM_E_ARG
        assert "null pointer" in N.last_error()


def test_lom_fold_argument_errors(libs):
    lib, _ = libs
    one = ctypes.addressof(ctypes.create_string_buffer(64))
    for k in (0, -3):
        assert lib.fbm_lom_fold(one, one, k, 4, 1, None) == N.FBM_E_ARG, k
    assert lib.fbm_lom_fold(None, one, 1, 4, 1, None) == N.FBM_E_ARG
    assert lib.fbm_lom_fold(one, None, 1, 4, 0, None) == N.FBM_E_ARG
    assert "fold" in N.last_error()
    assert lib.fbm_lom_fold(None, None, 1, 0, 1, None) == N.FBM_OK  # n == 0: nothing to do


# ---- the accumulator objects, where no device is needed -----------------------------------------
def _jl(num_nodes=2, key=-5, total=7):
    return SecaggCrypter().begin_aggregate(3, num_nodes, key, BIPRIME, total, num_expected_params=4)


def test_jl_wrong_count_is_raised_at_finish():
    agg = _jl(num_nodes=2)
    agg.add([])  # one of two replies
    with pytest.raises(FedbiomedSecaggCrypterError, match="Num of parameters that are received from nodes"):
        agg.finish()
    agg = _jl(num_nodes=0)  # the one-shot's aggregate(.., 0, [], ..): the non-empty check
    with pytest.raises(FedbiomedSecaggCrypterError, match="non-empty list"):
        agg.finish()


def test_jl_type_errors_are_raised_at_add():
    agg = _jl()
    with pytest.raises(FedbiomedSecaggCrypterError, match="list containing list of parameters"):
        agg.add((1, 2))
    with pytest.raises(FedbiomedSecaggCrypterError, match="should be of type of integers"):
        agg.add([1, 2.0])
    with pytest.raises(FedbiomedSecaggCrypterError, match="should be of type of integers"):
        agg.add([1, "2"])
    with pytest.raises(TypeError, match="The key should be type of integer"):
        _jl(key=5.0).add([])


def test_jl_zero_length_party_and_use_after_the_end():
    agg = _jl(num_nodes=2)
    agg.add([])
    agg.add([])
    assert agg.finish() == []
    for call in (lambda: agg.add([]), agg.finish, agg.finish_tensor, agg.abort):
        with pytest.raises(FedbiomedSecaggCrypterError, match="has ended"):
            call()
    agg = _jl()
    agg.abort()
    for call in (lambda: agg.add([]), agg.finish, agg.finish_tensor, agg.abort):
        with pytest.raises(FedbiomedSecaggCrypterError, match="has ended"):
            call()
    agg = _jl(num_nodes=1)
    agg.add([])
    assert agg.finish_tensor() is None


def test_total_sample_size_is_read_at_finish_only():
    """A caller that learns the total with the last reply assigns it before finish (both accumulators)."""
    agg = _jl(num_nodes=1, total=0)
    assert agg.total_sample_size == 0
    agg.total_sample_size = 11
    assert agg.total_sample_size == 11 and agg._total == 11
    lagg = SecaggLomCrypter("n").begin_aggregate(0)
    lagg.total_sample_size = 9
    assert lagg.total_sample_size == 9 and lagg._total == 9


def test_lom_accumulator_without_a_device():
    lagg = SecaggLomCrypter("n").begin_aggregate(5)
    with pytest.raises(FedbiomedSecaggCrypterError, match="list containing list of parameters"):
        lagg.add("12")
    with pytest.raises(FedbiomedSecaggCrypterError, match="should be of type of integers"):
        lagg.add([1.5])
    lagg.add([])
    lagg.add([])
    assert lagg.finish() == []
    for call in (lambda: lagg.add([]), lagg.finish, lagg.finish_tensor, lagg.abort):
        with pytest.raises(FedbiomedSecaggCrypterError, match="has ended"):
            call()
    assert SecaggLomCrypter("n").begin_aggregate(5).finish() == []  # no reply at all: aggregate([], 5) is []
    lagg = SecaggLomCrypter("n").begin_aggregate(5)
    lagg.abort()
    with pytest.raises(FedbiomedSecaggCrypterError, match="has ended"):
        lagg.add([1])


def test_state_is_the_objects_own():
    a, b = _jl(num_nodes=1), _jl(num_nodes=3)
    a.add([])
    assert (a._adds, b._adds) == (1, 0) and a.finish() == []
    b.add([])
    with pytest.raises(FedbiomedSecaggCrypterError, match="Num of parameters"):
        b.finish()
    before = dict(vars(SecaggCrypter))
    c = _jl(num_nodes=1)
    c.add([])
    c.abort()
    assert dict(vars(SecaggCrypter)) == before  # nothing class-wide is written

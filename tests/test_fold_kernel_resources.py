"""The streaming-aggregation kernels' resources, read from the shipped library's gfx950 code objects
(tools/kernel_resources.py; CPU only), pinning what DESIGN.md section 4 states:
  * jl_fold_kernel is built as jl_prod_kernel: no scratch, at least two waves per SIMD by registers, at most
    80 KB of LDS per workgroup (two workgroups in a CU's 160 KB);
  * lom_fold_kernel (HBM-bound) has no scratch;
  * neither has a dynamic stack."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fedbiomed_amd", "_lib", "libfbm_secagg.so")


@pytest.fixture(scope="module")
def res():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not os.path.exists(LIB):
        pytest.skip("library not built (python -m fedbiomed_amd._build)")
    if not os.path.exists(kr.READELF):
        pytest.skip("llvm-readelf not found")
    r = kr.kernels(LIB)
    assert r, "no gfx950 kernel metadata found in the library"
    return kr, r


def _one(kr, r, name):
    hits = kr.find(r, name)
    assert hits, f"{name} not in the library"
    return hits


def test_jl_fold_kernel_two_waves_no_scratch(res):
    kr, r = res
    for k, v in _one(kr, r, "jl_fold_kernel").items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)
        assert v["vgpr"] <= 256 and v["waves_per_simd_by_registers"] >= 2, (k, v)
        assert v["lds_bytes_per_workgroup"] <= 80 * 1024, (k, v)
        assert v["max_workgroup_size"] == 256, (k, v)  # one lane per ciphertext, 256 lanes


def test_lom_fold_kernel_no_scratch(res):
    kr, r = res
    for k, v in _one(kr, r, "lom_fold_kernel").items():
        assert v["scratch_bytes_per_lane"] == 0 and v["lds_bytes_per_workgroup"] == 0, (k, v)


@pytest.mark.parametrize("name", ["jl_fold_kernel", "lom_fold_kernel", "jl_gen_fold_kernel"])
def test_no_dynamic_stack(res, name):
    kr, r = res
    for k, v in _one(kr, r, name).items():
        assert not v["dynamic_stack"], (k, v)


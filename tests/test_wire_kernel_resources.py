"""The wire kernels' resources, read from the shipped library's gfx950 code objects (tools/kernel_resources.py; CPU
only), as tests/test_kernel_resources.py does for the others: both directions are HBM-bound re-layouts, so none of
them may spill to scratch or carry a dynamic stack, and their LDS (a tile's bytes, a group's bytes) stays small
enough for several workgroups per CU."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fedbiomed_amd", "_lib", "libfbm_secagg.so")
KERNELS = ["wire_sizes_jl_kernel", "wire_sizes_lom_kernel", "wire_scan_kernel", "wire_emit_jl_kernel",
           "wire_emit_lom_kernel", "wire_decode_jl_kernel", "wire_decode_lom_kernel"]


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


@pytest.mark.parametrize("name", KERNELS)
def test_wire_kernels_no_scratch(res, name):
    kr, r = res
    hits = kr.find(r, name)
    assert hits, f"{name} not in the library"
    for k, v in hits.items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)
        assert not v["dynamic_stack"], (k, v)
        assert v["lds_bytes_per_workgroup"] <= 16 * 1024, (k, v)
        assert v["waves_per_simd_by_registers"] >= 4, (k, v)

"""wire_fold_lom_kernel's resources, read from the shipped library's gfx950 code object (tools/kernel_resources.py;
CPU only), as tests/test_wire_kernel_resources.py does for the other wire kernels: an HBM-bound pass may not spill to
scratch or carry a dynamic stack, and its LDS is one group's bytes (64 items of at most 9) per wave of the
workgroup's four."""
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


def test_wire_fold_lom_kernel_resources(res):
    kr, r = res
    hits = kr.find(r, "wire_fold_lom_kernel")
    assert hits, "wire_fold_lom_kernel not in the library"
    for k, v in hits.items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)
        assert not v["dynamic_stack"], (k, v)
        assert v["lds_bytes_per_workgroup"] == 4 * 64 * 9, (k, v)
        assert v["waves_per_simd_by_registers"] >= 4, (k, v)

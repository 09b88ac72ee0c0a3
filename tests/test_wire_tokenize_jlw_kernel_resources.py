"""The wide tokenizer's kernels' resources from the shipped library's gfx950 code object (tools/kernel_resources.py; CPU
only), as tests/test_wire_tokenize_jl_kernel_resources.py: no scratch, no spilled VGPRs, no dynamic stack, and DESIGN.md
4.2's LDS -- the JL tokenizer's staging for maps and emit; 256 * 32 * 8 + 256 * 8 bytes for the two scans."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fedbiomed_amd", "_lib", "libfbm_secagg.so")
LDS = {"wire_jlwtok_maps_kernel": 16512, "wire_jlwtok_emit_kernel": 22272, "wire_jlwtok_scan_kernel": 67584,
       "wire_jlwseg_scan_kernel": 67584}


def test_wide_tokenizer_kernels_resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    if not os.path.exists(LIB) or not os.path.exists(kr.READELF):
        pytest.skip("library not built (python -m fedbiomed_amd._build) or llvm-readelf not found")
    r = kr.kernels(LIB)
    assert sorted(k for k in r if "wire_jlw" in k and ("tok_" in k or "seg_" in k)) == sorted(kr.find(r, n).popitem()[0] for n in LDS)
    for name, lds in LDS.items():
        (k, v), = kr.find(r, name).items()
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spill"] == 0 and not v["dynamic_stack"], (k, v)
        assert v["lds_bytes_per_workgroup"] == lds, (k, v)

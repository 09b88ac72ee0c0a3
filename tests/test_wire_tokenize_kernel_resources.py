"""The device tokenizer's kernels' resources, read from the shipped library's gfx950 code object
(tools/kernel_resources.py; CPU only), as tests/test_wire_fold_kernel_resources.py does for the fold kernel: no
scratch, no dynamic stack, at least 4 waves per SIMD by registers, and the LDS the design gives.

LDS, wire_tok_maps_kernel and wire_tok_emit_kernel: a workgroup is four waves, one 4096-byte tile each.  A tile
lies in LDS as its 64 sub-blocks of 16 words, 17 words apart (so that the 64 lanes reading word i of their own
sub-block hit 32 different banks twice, not two banks 32 times): 64 * 17 * 4 = 4352 bytes; the sub-blocks' maps are
64 * 10 entries of 2 bytes (items << 4 | phase, at most 64 items): 1280 bytes.  4 * (4352 + 1280) = 22528, seven
workgroups in a CU's 160 KiB.
wire_tok_scan_kernel: one workgroup of 256 threads, each thread's composed map as 10 words of 8 bytes (items << 4 |
phase, the items of a whole message) and its entry state, 8 bytes: 256 * 10 * 8 + 256 * 8 = 22528 as well."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fedbiomed_amd", "_lib", "libfbm_secagg.so")
LDS = {"wire_tok_maps_kernel": 4 * (64 * 17 * 4 + 64 * 10 * 2), "wire_tok_emit_kernel": 4 * (64 * 17 * 4 + 64 * 10 * 2),
       "wire_tok_scan_kernel": 256 * 10 * 8 + 256 * 8}


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


def test_wire_tok_kernels_resources(res):
    kr, r = res
    hits = [k for k in r if "wire_tok_" in k]
    assert len(hits) == len(LDS), sorted(hits)  # every wire_tok_ kernel is listed above
    for name, lds in LDS.items():
        (k, v), = kr.find(r, name).items()
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert not v["dynamic_stack"], (k, v)
        assert v["lds_bytes_per_workgroup"] == lds == 22528, (k, v)
        assert v["waves_per_simd_by_registers"] >= 4, (k, v)

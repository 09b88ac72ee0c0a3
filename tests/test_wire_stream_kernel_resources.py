"""The resumable tokenizers' own kernels' resources, read from the shipped library's gfx950 code object
(tools/kernel_resources.py; CPU only), as tests/test_wire_tokenize_jl_kernel_resources.py does for the one-shot ones: no
scratch, no spill, no dynamic stack, and the LDS the design gives.

A feed launches the one-shot maps and emit kernels over its tiles (their resources are pinned by the one-shot tests)
and, between them, a scan with a device-side carry.  The two scans hold what the one-shot scans hold -- one workgroup
of 256 threads: wire_seg_scan_lom_kernel each thread's composed run as FBM_WIRE_TOK_MAP = 10 states of 8 bytes and its
entry state, 256 * 10 * 8 + 256 * 8 = 22528 bytes; wire_seg_scan_jl_kernel FBM_WIRE_TOKJ_SLOTS = 16 states and the
entry state, 256 * 16 * 8 + 256 * 8 = 34816 --; the carry lives in the stream's record in device memory.
wire_seg_begin_kernel writes that record's 16 words and uses no LDS."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fedbiomed_amd", "_lib", "libfbm_secagg.so")
THREADS, MAP, SLOTS = 256, 10, 16
LDS = {"wire_seg_begin_kernel": 0, "wire_seg_scan_lom_kernel": THREADS * MAP * 8 + THREADS * 8,
       "wire_seg_scan_jl_kernel": THREADS * SLOTS * 8 + THREADS * 8}
OLD = ["wire_sizes_jl_kernel", "wire_sizes_lom_kernel", "wire_scan_kernel", "wire_emit_jl_kernel", "wire_emit_lom_kernel",
       "wire_decode_jl_kernel", "wire_decode_lom_kernel", "wire_fold_lom_kernel", "wire_tok_maps_kernel", "wire_tok_scan_kernel",
       "wire_tok_emit_kernel", "wire_tokj_maps_kernel", "wire_tokj_scan_kernel", "wire_tokj_emit_kernel"]


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


def test_source_constants():
    """The figures above are the source's: the maps' sizes in fbm_wire.hpp, the scan workgroup's threads in fbm_wire.hip."""
    import re

    for path, names in (("fbm_wire.hpp", (("FBM_WIRE_TOK_MAP", str(MAP)), ("FBM_WIRE_TOKJ_SLOTS", str(SLOTS)))),
                        ("fbm_wire.hip", (("FBM_WIRE_SCAN_THREADS", str(THREADS)),))):
        src = open(os.path.join(ROOT, "fedbiomed_amd", "csrc", path)).read()
        for name, text in names:
            m = re.search(r"#define %s (\S.*?)\s*(//.*)?$" % name, src, re.M)
            assert m and m.group(1) == text, name
        if path.endswith(".hip"):  # the new kernels are launched and bounded with that figure
            assert src.count("__launch_bounds__(FBM_WIRE_SCAN_THREADS) wire_seg_scan_") == 2


def test_wire_seg_kernels_resources(res):
    kr, r = res
    hits = [k for k in r if "wire_seg_" in k]
    assert len(hits) == len(LDS), sorted(hits)  # every wire_seg_ kernel is listed above
    for name, lds in LDS.items():
        (k, v), = kr.find(r, name).items()
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert not v["dynamic_stack"], (k, v)
        assert v["lds_bytes_per_workgroup"] == lds, (k, v)
    assert LDS == {"wire_seg_begin_kernel": 0, "wire_seg_scan_lom_kernel": 22528, "wire_seg_scan_jl_kernel": 34816}
    # the existing resource tests find their kernels by substring: the library's new names hold none of the old ones
    for new in hits:
        assert not any(old in new for old in OLD) and "wire_tok_" not in new and "wire_tokj_" not in new, new
    for old in OLD:  # ... and every old name still finds its own kernel alone
        assert len(kr.find(r, old)) == 1, old

"""The big-int-map tokenizer's kernels' resources, read from the shipped library's gfx950 code object
(tools/kernel_resources.py; CPU only), as tests/test_wire_tokenize_kernel_resources.py does for the LOM tokenizer: no
scratch, no dynamic stack, and the LDS the design gives.

LDS, from fbm_wire.hpp's constants.  A workgroup is four waves, one 4096-byte tile each.  A staged tile is its 1024
words, the 24 bytes behind it that decide the size of an item starting on its last byte (6 words) and two words so
that an unaligned 4-byte read may touch the word behind: FBM_WIRE_TOKJ_WORDS = (4096 + 24) / 4 + 2 = 1032 words.
wire_tokj_maps_kernel holds nothing else: 4 * 1032 * 4 = 16512 bytes.  wire_tokj_emit_kernel adds, per wave, the table
words of the items that start in a tile, FBM_WIRE_TOKJ_ITEMS = ceil(4096 / 23) = 179 of 8 bytes, and two 4-byte
words (how many, and item n - 1's end): 16512 + 4 * (179 * 8 + 8) = 22272.
wire_tokj_scan_kernel: one workgroup of 256 threads, each thread's composed run from each of the FBM_WIRE_TOKJ_SLOTS =
16 entries of its first tile's map as a state of 8 bytes, and its entry state: 256 * 16 * 8 + 256 * 8 = 34816."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fedbiomed_amd", "_lib", "libfbm_secagg.so")
TILE, HEAD, SLOTS, WAVES, THREADS = 4096, 24, 16, 4, 256
WORDS = (TILE + HEAD) // 4 + 2
ITEMS = (TILE + 22) // 23
LDS = {"wire_tokj_maps_kernel": WAVES * WORDS * 4, "wire_tokj_emit_kernel": WAVES * (WORDS * 4 + ITEMS * 8 + 8),
       "wire_tokj_scan_kernel": THREADS * SLOTS * 8 + THREADS * 8}


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
    """The figures above are the source's."""
    import re

    src = open(os.path.join(ROOT, "fedbiomed_amd", "csrc", "fbm_wire.hpp")).read()
    for name, text in (("FBM_WIRE_TOK_TILE", "(FBM_WIRE_TOK_SUB * FBM_WIRE_TOK_SUBS)"), ("FBM_WIRE_TOKJ_HEAD", str(HEAD)),
                       ("FBM_WIRE_TOKJ_SLOTS", str(SLOTS)),
                       ("FBM_WIRE_TOKJ_WORDS", "((FBM_WIRE_TOK_TILE + FBM_WIRE_TOKJ_HEAD) / 4 + 2)"),
                       ("FBM_WIRE_TOKJ_ITEMS", "((FBM_WIRE_TOK_TILE + 22) / 23)")):
        m = re.search(r"#define %s (\S.*?)\s*(//.*)?$" % name, src, re.M)
        assert m and m.group(1) == text, name
    assert (WORDS, ITEMS) == (1032, 179)


def test_wire_tokj_kernels_resources(res):
    kr, r = res
    hits = [k for k in r if "wire_tokj_" in k]
    assert len(hits) == len(LDS), sorted(hits)  # every wire_tokj_ kernel is listed above
    for name, lds in LDS.items():
        (k, v), = kr.find(r, name).items()
        assert v["scratch_bytes_per_lane"] == 0 and v["vgpr_spill"] == 0, (k, v)
        assert not v["dynamic_stack"], (k, v)
        assert v["lds_bytes_per_workgroup"] == lds, (k, v)
    assert LDS == {"wire_tokj_maps_kernel": 16512, "wire_tokj_emit_kernel": 22272, "wire_tokj_scan_kernel": 34816}

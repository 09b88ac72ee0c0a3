"""The 16-bit input and narrow output instantiations in the shipped library's gfx950 code objects
(tools/kernel_resources.py, as tests/test_kernel_resources.py; CPU only): every instantiation is there, none
spills, and the new lom_protect_kernel instantiations keep what its __launch_bounds__(256, 8) states -- at most 64
VGPRs, 8 waves per SIMD (the ChaCha20 chains need the latency hiding: fedbiomed_amd/csrc/fbm_lom.hip)."""

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


def test_protect_kernel_instantiations_keep_eight_waves(res):
    kr, r = res
    hits = kr.find(r, "lom_protect_kernel")
    assert len(hits) >= 5, sorted(hits)  # float, double, uint64 + fbm_f16, fbm_bf16
    for k, v in hits.items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)
        assert v["vgpr"] <= 64 and v["waves_per_simd_by_registers"] >= 8, (k, v)


@pytest.mark.parametrize("name", ["lom_aggregate_kernel", "lom_aggregate_ws_kernel", "jl_decode_kernel",
                                  "dequantize_kernel"])
def test_output_kernels_have_every_output_type(res, name):
    kr, r = res
    hits = kr.find(r, name)
    assert len(hits) >= 4, sorted(hits)  # float64, float32, binary16, bfloat16
    for k, v in hits.items():
        assert v["scratch_bytes_per_lane"] == 0, (k, v)


def test_float64_aggregate_kernels_keep_their_names(res):
    """The committed HBM-traffic profiles and the bench's lookup are keyed on these names."""
    kr, r = res
    names = " ".join(kr.find(r, "lom_aggregate_ws_kernel"))
    for demangled, mangled in (("lom_aggregate_ws_kernel<2, 4, 8>(", "lom_aggregate_ws_kernelILi2ELi4ELi8EJEE"),
                               ("lom_aggregate_ws_kernel<2, 8, 16>(", "lom_aggregate_ws_kernelILi2ELi8ELi16EJEE")):
        assert demangled in names or mangled in names, names  # (mangled: a box without a demangler)

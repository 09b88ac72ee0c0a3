"""Aggregates written in the model's dtype by the kernels (`out_dtype=` / `out=` of aggregate_tensor,
D.lom_aggregate, D.jl_aggregate, D.dequantize; the *_as entry points of include/fbm_secagg.h).

The float64 result v is pinned against the reference elsewhere (test_gpu_parity, test_configs:
SecaggLomCrypter.aggregate / SecaggCrypter.aggregate, fedbiomed/common/secagg/_secagg_crypter.py:139-230,
394-455).  The narrow outputs are DEFINED from it: float32 = RN-even(v), float16 / bfloat16 = RN-even of that
float32 -- the two roundings of the unfused `aggregate_tensor(...).to(dtype)` callers write today, which is how
torch converts on the host.  So every case here is a bitwise comparison of the fused output with the host's
`.to(dtype)` of the float64 output: all three kernels of the LOM aggregate (generic, and the wave-split ones for 8
and 16 parties), full tiles, a partial last tile, the element-wise fallback, destinations at odd elements, the
overflow to +/-inf, the range error, and the double rounding itself where the aggregate's inputs cannot reach it
(fbm_dequantize_as through ctypes)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from fedbiomed_amd import _device as D, _native as N, workload as W
from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError
from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter

pytestmark = pytest.mark.gpu

NARROW = [torch.float32, torch.float16, torch.bfloat16]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bit patterns on the host (NaN-proof, sign-of-zero-proof comparison)."""
    t = t.cpu()
    return t.view({8: torch.int64, 4: torch.int32, 2: torch.int16}[t.element_size()])


def assert_is_host_cast(got: torch.Tensor, ref64: torch.Tensor, dtype):
    assert got.dtype == dtype and got.shape == ref64.shape
    assert torch.equal(bits(got), bits(ref64.cpu().to(dtype)))


@functools.lru_cache(maxsize=None)
def lom_case(P: int, n: int):
    """P parties' masked rows of seeded vectors (real protects), the total weight, and today's float64 result."""
    dev = D.device()
    ids = W.node_ids(P)
    lc = SecaggLomCrypter("out_dtype")
    g = torch.Generator().manual_seed(1000 * P + n)
    ws = [1 + (p % 3) for p in range(P)]
    Y = torch.stack([lc.encrypt_tensor(2, u, (torch.rand(n, generator=g, dtype=torch.float64) * 6.4 - 3.2).to(dev),
                                       W.pairwise_secrets_for(u, ids), ids, weight=ws[p]) for p, u in enumerate(ids)])
    ref, sums = lc.aggregate_tensor(Y, sum(ws), want_sums=True)
    return lc, Y, sum(ws), ref, sums


@pytest.mark.parametrize("P", [3, 8, 16])       # lom_aggregate_kernel, lom_aggregate_ws_kernel<2, 4, 8> and <2, 8, 16>
@pytest.mark.parametrize("n", [1024, 1000, 1027])  # full tiles, a partial last tile, odd: the element-wise fallback
def test_lom_aggregate_out_dtype(P, n):
    lc, Y, tw, ref, sums = lom_case(P, n)
    dev = Y.device
    again = lc.aggregate_tensor(Y, tw, out_dtype=None)
    assert again.dtype == torch.float64 and torch.equal(bits(again), bits(ref))
    assert torch.equal(bits(lc.aggregate_tensor(Y, tw, out_dtype=torch.float64)), bits(ref))
    for dt in NARROW:
        assert_is_host_cast(lc.aggregate_tensor(Y, tw, out_dtype=dt), ref, dt)
        got, s = lc.aggregate_tensor(Y, tw, want_sums=True, out_dtype=dt)
        assert_is_host_cast(got, ref, dt)
        assert torch.equal(s, sums)
        for off in (0, 1):  # a flat parameter buffer: the destination at an even and at an odd element
            buf = torch.full((n + 3,), 7.0, dtype=dt, device=dev)
            view = buf[off:off + n]
            ret = lc.aggregate_tensor(Y, tw, out=view)
            assert ret is view
            assert_is_host_cast(view, ref, dt)
            assert (buf[:off] == 7).all() and (buf[off + n:] == 7).all()  # nothing written around it
    f64 = torch.zeros(n + 1, dtype=torch.float64, device=dev)
    view = f64[1:]  # float64 at an odd element: 8-byte aligned only
    assert lc.aggregate_tensor(Y, tw, out=view) is view
    assert torch.equal(bits(view), bits(ref)) and f64[0] == 0


def test_lom_aggregate_out_argument_errors():
    lc, Y, tw, ref, _ = lom_case(3, 1000)
    dev, n = Y.device, Y.shape[1]
    bad = [dict(out=torch.empty(n, dtype=torch.float16, device=dev), out_dtype=torch.bfloat16),  # disagreeing dtypes
           dict(out=torch.empty(n + 1, dtype=torch.float32, device=dev)),                         # wrong length
           dict(out=torch.empty(2 * n, dtype=torch.float32, device=dev)[::2]),                    # not contiguous
           dict(out=torch.empty((n, 1), dtype=torch.float32, device=dev)),                        # not 1-D
           dict(out=torch.empty(n, dtype=torch.float32)),                                          # wrong device
           dict(out_dtype=torch.int32)]
    for kw in bad:
        with pytest.raises(ValueError):
            lc.aggregate_tensor(Y, tw, **kw)
        with pytest.raises(ValueError):
            D.lom_aggregate(Y, tw, **kw)


@pytest.mark.parametrize("P", [3, 8])
def test_overflow_goes_to_infinity(P):
    """A clipping range above 65 504 with values at +/-clip: +/-inf in float16, as IEEE's and torch's conversion."""
    dev = D.device()
    ids = W.node_ids(P)
    lc = SecaggLomCrypter("out_inf")
    n, clip = 130, 70000
    x = torch.tensor([clip, -clip, 65504.0, 65519.0, 65520.0, -65520.0, 0.25] * 19, dtype=torch.float64)[:n].to(dev)
    Y = torch.stack([lc.encrypt_tensor(1, u, x, W.pairwise_secrets_for(u, ids), ids, clipping_range=clip,
                                       target_range=2**40) for u in ids])
    ref = lc.aggregate_tensor(Y, P, clipping_range=clip, target_range=2**40)
    for dt in NARROW:
        got = lc.aggregate_tensor(Y, P, clipping_range=clip, target_range=2**40, out_dtype=dt)
        assert_is_host_cast(got, ref, dt)
    h = lc.aggregate_tensor(Y, P, clipping_range=clip, target_range=2**40, out_dtype=torch.float16).cpu()
    assert h[0] == float("inf") and h[1] == -float("inf") and torch.isfinite(h[2]) and torch.isfinite(h[6])


@pytest.mark.parametrize("P", [3, 8, 16])
@pytest.mark.parametrize("dt", [None] + NARROW)
def test_range_error_for_every_out_dtype(P, dt):
    """An average that rounds to 2^64 (reverse_quantize's guard, common/utils/_secagg_utils.py:152-187): FB624
    whatever the output type; the status path is the float64 one's."""
    Y = torch.zeros((P, 256), dtype=torch.int64, device=D.device())
    Y[0, 5] = -1  # the column sum 2^64 - 1 over a total weight of 1
    with pytest.raises(FedbiomedSecaggCrypterError, match="Cannot reverse quantize"):
        SecaggLomCrypter("out_range").aggregate_tensor(Y, 1, out_dtype=dt)


@pytest.fixture(scope="module")
def jl_case():
    dev = D.device()
    jc, P, n, tau = SecaggCrypter(), 2, 100, 4
    keys = [W.jl_user_key(p) for p in range(P)]
    g = torch.Generator().manual_seed(100)
    cts = torch.stack([jc.encrypt_tensor(P, tau, (torch.rand(n, generator=g, dtype=torch.float64) * 6.4 - 3.2).to(dev),
                                         keys[p], W.BIPRIME0, weight=p + 1) for p in range(P)])
    sk0 = -sum(keys)
    ref, sums = jc.aggregate_tensor(tau, cts, sk0, W.BIPRIME0, 3, num_expected_params=n, want_sums=True)
    f = jc.decrypt_factor_tensor(tau, cts.shape[1], sk0, W.BIPRIME0)
    return jc, cts, sk0, tau, n, ref, sums, f


@pytest.mark.parametrize("dt", NARROW)
@pytest.mark.parametrize("with_factor", [False, True])
def test_jl_aggregate_out_dtype(jl_case, dt, with_factor):
    jc, cts, sk0, tau, n, ref, sums, f = jl_case
    kw = dict(num_expected_params=n, decrypt_factor=f if with_factor else None)
    assert torch.equal(bits(jc.aggregate_tensor(tau, cts, sk0, W.BIPRIME0, 3, out_dtype=None, **kw)), bits(ref))
    got, s = jc.aggregate_tensor(tau, cts, sk0, W.BIPRIME0, 3, want_sums=True, out_dtype=dt, **kw)
    assert_is_host_cast(got, ref, dt)
    assert torch.equal(s, sums)
    buf = torch.full((n + 2,), 7.0, dtype=dt, device=cts.device)
    view = buf[1:1 + n]  # misaligned by one element
    assert jc.aggregate_tensor(tau, cts, sk0, W.BIPRIME0, 3, out=view, **kw) is view
    assert_is_host_cast(view, ref, dt)
    assert buf[0] == 7 and buf[n + 1] == 7
    with pytest.raises(ValueError):
        jc.aggregate_tensor(tau, cts, sk0, W.BIPRIME0, 3, out=buf[:n], out_dtype=torch.float64, **kw)


def _dequantize_as(neg_clip: float, step: float, u: int, code: int, dtype) -> int:
    lib = N.load()
    dev = D.device()
    ut = torch.tensor([u, u, u], dtype=torch.int64, device=dev)
    out = torch.zeros(3, dtype=dtype, device=dev)
    vp = ctypes.c_void_p
    rc = lib.fbm_dequantize_as(vp(ut.data_ptr()), 3, neg_clip, step, vp(out.data_ptr()), code,
                               vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, N.last_error()
    b = bits(out)
    assert b[0] == b[1] == b[2]
    return int(b[0]) & (0xFFFF if out.element_size() == 2 else 0xFFFFFFFF)


def test_dequantize_as_pins_the_double_rounding():
    """neg_clip + step * u = 1 + 2^-8 + 2^-40: float32 rounds it to the bfloat16 tie 1 + 2^-8, which goes to the
    even 1.0 -- one rounding would give 1.0078125.  Likewise 1 + 2^-11 + 2^-40 in float16 (one rounding:
    1.0009765625).  The float32 results are the ties themselves."""
    s = 2.0**-40
    assert _dequantize_as(1 + 2.0**-8, s, 1, N.FBM_BF16, torch.bfloat16) == 0x3F80
    assert _dequantize_as(1 + 2.0**-11, s, 1, N.FBM_F16, torch.float16) == 0x3C00
    assert _dequantize_as(1 + 2.0**-8, s, 1, N.FBM_F32, torch.float32) == 0x3F808000
    assert _dequantize_as(1 + 2.0**-11, s, 1, N.FBM_F32, torch.float32) == 0x3F801000
    # the other formats see no tie: 1 + 2^-8 is a float16 value; bfloat16 drops 2^-11 entirely
    assert _dequantize_as(1 + 2.0**-8, s, 1, N.FBM_F16, torch.float16) == 0x3C04
    assert _dequantize_as(1 + 2.0**-11, s, 1, N.FBM_BF16, torch.bfloat16) == 0x3F80
    ut = torch.tensor([1], dtype=torch.int64, device=D.device())
    out = torch.zeros(1, dtype=torch.float64, device=D.device())
    vp = ctypes.c_void_p
    assert N.load().fbm_dequantize_as(vp(ut.data_ptr()), 1, 1 + 2.0**-8, s, vp(out.data_ptr()), N.FBM_F64,
                                      vp(torch.cuda.current_stream().cuda_stream)) == 0
    assert out.item() == 1 + 2.0**-8 + 2.0**-40


def test_device_dequantize_out_dtype():
    dev = D.device()
    u = torch.arange(0, 8191, 7, dtype=torch.int64, device=dev)
    ref = D.dequantize(u)
    assert ref.dtype == torch.float64
    for dt in NARROW:
        assert_is_host_cast(D.dequantize(u, out_dtype=dt), ref, dt)

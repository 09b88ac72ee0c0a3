"""float16 / bfloat16 device tensors through the encrypt paths (FBM_F16 / FBM_BF16, include/fbm_secagg.h).

The reference's `encrypt` takes List[float] (fedbiomed/common/secagg/_secagg_crypter.py:45-137, 318-392): a 16-bit
parameter reaches its quantiser (common/utils/_secagg_utils.py:82-119) as the exact Python float of that value.  So
the device path on a 16-bit tensor has one correct answer, bit for bit: the oracle's on `x.double().tolist()`,
which is also what the device returns for `x.double()`.  Checked over ALL 65 536 bit patterns of each type
(subnormals, signed zeros, infinities, every NaN payload), on partial blocks and 2-byte aligned slices (the
kernel's 16-byte load needs a full, aligned block), across shards, through every variant of the JL encrypt, and
through the host-buffer C call.
"""
import ctypes

import numpy as np
import pytest
import torch

from fedbiomed_amd import _device as D, _native as N, workload as W
from fedbiomed_amd.secagg import SecaggCrypter, SecaggLomCrypter
from oracle import secagg_oracle as O

pytestmark = pytest.mark.gpu

DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
T40 = 2**40
CLIP_MSG = "exceeds clipping range"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def all_patterns(dtype) -> torch.Tensor:
    return torch.arange(65536, dtype=torch.int32).to(torch.int16).view(dtype)


def u64(t: torch.Tensor) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def lom():
    """3 nodes; the middle one has a peer of each mask sign."""
    ids = W.node_ids(3)
    return SecaggLomCrypter("half_inputs"), ids, ids[1], W.pairwise_secrets_for(ids[1], ids)


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("clip", [1, 3, 2**16])
@pytest.mark.parametrize("weight", [1, 3])
def test_lom_protect_every_pattern(lom, caplog, name, clip, weight):
    lc, ids, u, sec = lom
    x = all_patterns(DTYPES[name])
    xd = x.double()
    with caplog.at_level("WARNING"):
        got = lc.encrypt_tensor(5, u, x.to(D.device()), sec, ids, clipping_range=clip, weight=weight, target_range=T40)
        torch.cuda.synchronize()
    warned = sum(CLIP_MSG in r.getMessage() for r in caplog.records)
    # _check_clipping_range (common/utils/_secagg_utils.py:189-204): some x < -c or x > c; NaN is neither
    assert warned == int(bool(((xd < -clip) | (xd > clip)).any())) == 1  # (+/-inf are among the patterns)
    ref = O.lom_encrypt(xd.tolist(), 5, u, sec, ids, lc.nonce, clip=clip, weight=weight, target=T40)
    assert np.array_equal(u64(got), ref)
    wide = lc.encrypt_tensor(5, u, xd.to(D.device()), sec, ids, clipping_range=clip, weight=weight, target_range=T40)
    assert torch.equal(got, wide)


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_no_clip_warning_inside_the_range(lom, caplog, name):
    """NaN and signed zeros are inside every range: no warning, as the reference's rule (NaN compares false)."""
    lc, ids, u, sec = lom
    x = torch.tensor([0.0, -0.0, float("nan"), 1.0, -1.0, 0.5], dtype=DTYPES[name])
    with caplog.at_level("WARNING"):
        got = lc.encrypt_tensor(1, u, x.to(D.device()), sec, ids, clipping_range=1, target_range=T40)
        torch.cuda.synchronize()
    assert not [r for r in caplog.records if CLIP_MSG in r.getMessage()]
    assert np.array_equal(u64(got), O.lom_encrypt(x.double().tolist(), 1, u, sec, ids, lc.nonce, clip=1, target=T40))


@pytest.mark.parametrize("name", sorted(DTYPES))
@pytest.mark.parametrize("n", [1, 7, 8, 9, 1027])
def test_tails_and_alignment(lom, name, n):
    """Partial last blocks, inputs that start 2 and 6 bytes past a 16-byte boundary (element loads), an aligned
    one (the 16-byte load), and a destination that is a row of a larger matrix: all equal the float64 call."""
    lc, ids, u, sec = lom
    dev = D.device()
    g = torch.Generator().manual_seed(n)
    buf = (torch.randn(n + 8, generator=g) * 2).to(DTYPES[name]).to(dev)  # past the default clip of 3 too
    for off in (0, 1, 3):
        x = buf[off:off + n]
        assert x.data_ptr() % 16 == 2 * off
        want = lc.encrypt_tensor(3, u, x.double(), sec, ids, weight=5)
        assert torch.equal(lc.encrypt_tensor(3, u, x, sec, ids, weight=5), want)
        Y = torch.zeros((3, n), dtype=torch.int64, device=dev)
        assert lc.encrypt_tensor(3, u, x, sec, ids, weight=5, out=Y[1]).data_ptr() == Y[1].data_ptr()
        assert torch.equal(Y[1], want) and not Y[0].any() and not Y[2].any()


def test_sharding_by_elem_offset(lom):
    lc, ids, u, sec = lom
    x = all_patterns(torch.bfloat16)[0x3C00:0x3C00 + 1027].to(D.device())
    whole = lc.encrypt_tensor(9, u, x, sec, ids, weight=2)
    assert torch.equal(lc.encrypt_tensor(9, u, x[8:], sec, ids, weight=2, elem_offset=8), whole[8:])


def test_negative_weight_branch(lom):
    """A negative weight passes only all-zero products (SecaggLomCrypter.encrypt_tensor's second call reads the
    quantised values): the same outcome for a 16-bit tensor as for its float64 copy."""
    lc, ids, u, sec = lom
    dev = D.device()
    zeros = torch.full((9,), -4.0, dtype=torch.bfloat16, device=dev)  # below -clip: every q is 0
    assert torch.equal(lc.encrypt_tensor(1, u, zeros, sec, ids, weight=-3),
                       lc.encrypt_tensor(1, u, zeros.double(), sec, ids, weight=-3))
    x = torch.tensor([-4.0, 0.5], dtype=torch.float16, device=dev)
    errs = []
    for t in (x, x.double()):
        with pytest.raises(OverflowError) as e:
            lc.encrypt_tensor(1, u, t, sec, ids, weight=-3)
        errs.append(str(e.value))
    assert errs[0] == errs[1]


@pytest.fixture(scope="module")
def jl_sample():
    """4 096 elements per type: seeded patterns, then the named edge values."""
    out = {}
    for name, dt in DTYPES.items():
        rng = np.random.default_rng(16)
        bits = rng.integers(0, 65536, 4096).astype(np.uint16)
        inf = 0x7C00 if dt == torch.float16 else 0x7F80
        edge = [0x0000, 0x8000, inf, inf | 0x8000, inf | 1, 0x0001, 0x8001, (inf & -inf) - 1, 0xFFFF]
        bits[:len(edge)] = edge  # +/-0, +/-inf, NaNs, the smallest and the largest subnormal
        out[name] = torch.from_numpy(bits.view(np.int16).copy()).view(dt)
    return out


@pytest.mark.parametrize("name", sorted(DTYPES))
def test_jl_encrypt(jl_sample, name):
    dev = D.device()
    jc, key, tau, P = SecaggCrypter(), W.jl_user_key(0), 3, 2
    x = jl_sample[name].to(dev)
    xd = x.double()
    got = jc.encrypt_tensor(P, tau, x, key, W.BIPRIME0, weight=3)
    want = jc.encrypt_tensor(P, tau, xd, key, W.BIPRIME0, weight=3)
    assert torch.equal(got, want)  # every limb
    k = 100 // D.jl_slot(None, P)[1]  # the ciphertexts that the first 100 elements fill
    ref = O.jl_encrypt(xd[:k * D.jl_slot(None, P)[1]].cpu().tolist(), tau, key, W.BIPRIME0, P, weight=3)
    assert k >= 2 and len(ref) == k and D.limbs_to_ints(got[:k].cpu().numpy()) == ref
    # the other routes into the same kernels take the dtype through unchanged
    f = jc.decrypt_factor_tensor(tau, got.shape[0], key, W.BIPRIME0)
    assert torch.equal(jc.encrypt_tensor(P, tau, x, key, W.BIPRIME0, weight=3, factor=f), want)
    assert torch.equal(jc.encrypt_tensor(P, tau, x, key, W.BIPRIME0, weight=3, defer_exp=True).finish(), want)
    assert torch.equal(jc.encrypt_tensor(P, tau, x, key, W.BIPRIME0, weight=-3),
                       jc.encrypt_tensor(P, tau, xd, key, W.BIPRIME0, weight=-3))


@pytest.mark.parametrize("name,code", [("f16", N.FBM_F16), ("bf16", N.FBM_BF16)])
def test_host_buffer_c_call(lom, name, code):
    """fbm_lom_protect_host on a HOST buffer of 16-bit elements (2 bytes each in the staging copy) equals the
    device call, as tests/test_lom_host_call.py::test_host_call_separate_status_buffer for float64."""
    lc, ids, u, sec = lom
    lib = N.load()
    sm, sg = lc._peer_masks(u, sec, ids)
    g = torch.Generator().manual_seed(333)
    x = (torch.randn(333, generator=g) * 2).to(DTYPES[name])
    ref = lc.encrypt_tensor(4, u, x.to(D.device()), sec, ids, weight=3)
    c, c2, tf, tm1 = D.quant_params(None, 2**13)
    secb = np.frombuffer(b"".join(sm), dtype=np.uint8).copy()
    sgn = np.asarray(sg, dtype=np.int8)
    nb = np.frombuffer(lc.nonce, dtype=np.uint8).copy()
    y = np.full(333, 7, dtype=np.uint64)
    st = np.full(N.STATS_WORDS, 9, dtype=np.uint32)
    ws = torch.empty(int(lib.fbm_lom_host_workspace(333, 1)), dtype=torch.uint8, device=D.device())
    vp = ctypes.c_void_p
    rc = lib.fbm_lom_protect_host(vp(x.data_ptr()), code, 333, c, c2, tf, tm1, 3, vp(secb.ctypes.data),
                                  vp(sgn.ctypes.data), 2, 0, vp(nb.ctypes.data), 4, 0, vp(y.ctypes.data),
                                  vp(st.ctypes.data), vp(ws.data_ptr()), vp(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, N.last_error()
    assert np.array_equal(y, u64(ref))
    assert lib.fbm_check_stats(vp(st.ctypes.data), 3, None) == 0

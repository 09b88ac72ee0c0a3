"""The one-lane engine's short path as one register-resident chain body (fbm_na_chain_short) on the GPU:
encrypt_tensor and decrypt_factor_tensor bit-exact against the oracle and against the per-product loop it
replaced (D.jl_chain("per_call"), the test build's fbm_jl_set_chain) at the chunk edges (a chunk is 256
ciphertexts) and the exponent shapes -- zero iterations, both exponent-word boundaries, squares only, a short
product at every bit, both signs; one batched launch whose segments differ in exponent length; key 0 and a
small modulus, which stay on the table path."""

import random

import pytest
import torch

from fedbiomed_amd import _device as D, workload as W
from oracle import secagg_oracle as O

_RNG = random.Random(2040)
_K2040 = _RNG.getrandbits(2040) | (1 << 2039)
KEYS = [1, 3, (1 << 32) - 1, 1 << 32, 1 << 2039, (1 << 2040) - 1, _K2040, -_K2040]
P, TAU = 3, 5


def _params(n_ct, cr, seed):
    return torch.from_numpy(W.party_params(seed, n_ct * cr))


def _check_rows(n_ct):
    return sorted({0, n_ct - 1, min(n_ct - 1, 63), min(n_ct - 1, 255)})


@pytest.mark.gpu
@pytest.mark.parametrize("n_ct", [1, 64, 65, 257])
def test_chain_body_equals_oracle_and_per_call_chain(n_ct):
    from fedbiomed_amd.secagg import SecaggCrypter

    dev, jc, n2 = D.device(), SecaggCrypter(), W.BIPRIME0 ** 2
    _, cr = O.jl_slot(None, P)
    x = _params(n_ct, cr, 1)
    xd, w = x.to(dev), W.party_weight(1)
    qw = [int(v) * w for v in O.quantize(x.numpy().astype("float64"))]
    rows = _check_rows(n_ct)
    h = {k: O.fdh((k << 512) | TAU, n2) for k in rows}
    for key in KEYS:
        with D.jl_engine("single"):
            ct = jc.encrypt_tensor(P, TAU, xd, key, W.BIPRIME0, weight=w)
            f = jc.decrypt_factor_tensor(TAU, n_ct, key, W.BIPRIME0)
            with D.jl_chain("per_call"):
                ct_old = jc.encrypt_tensor(P, TAU, xd, key, W.BIPRIME0, weight=w)
                f_old = jc.decrypt_factor_tensor(TAU, n_ct, key, W.BIPRIME0)
        assert ct.shape[0] == n_ct and f.shape[0] == n_ct
        assert torch.equal(ct, ct_old), hex(key)
        assert torch.equal(f, f_old), hex(key)
        got_f = D.limbs_to_ints(f[rows].cpu().numpy())
        got_c = D.limbs_to_ints(ct[rows].cpu().numpy())
        for i, k in enumerate(rows):
            hk = O.powmod(h[k], key, n2)
            assert got_f[i] == hk, (hex(key), k)
            assert got_c[i] == O.jl_encrypt_ints(qw[k * cr:(k + 1) * cr], TAU, key, W.BIPRIME0, P, k0=k)[0], (hex(key), k)


@pytest.mark.gpu
def test_chain_body_in_a_batched_launch():
    """Three segments of 65 ciphertexts, exponents of 1, 33 and 2040 bits, in ONE launch: the exponent words
    and the bit count are per segment.  Each segment equals its own launch, under either chain form."""
    from fedbiomed_amd.secagg import SecaggCrypter

    dev, jc = D.device(), SecaggCrypter()
    _, cr = O.jl_slot(None, P)
    keys = [1, (1 << 32) | _RNG.getrandbits(32), _K2040]
    assert [k.bit_length() for k in keys] == [1, 33, 2040]
    xs = [_params(65, cr, p).to(dev) for p in range(P)]
    ws = [W.party_weight(p) for p in range(P)]
    with D.jl_engine("single"):
        ref = [jc.encrypt_tensor(P, TAU, xs[p], keys[p], W.BIPRIME0, weight=ws[p]) for p in range(P)]
        with D.jl_chain("per_call"):
            ref_old = [jc.encrypt_tensor(P, TAU, xs[p], keys[p], W.BIPRIME0, weight=ws[p]) for p in range(P)]
    for form in ("body", "per_call"):
        with D.jl_chain(form), D.deferred_checks():
            pend = [jc.encrypt_tensor(P, TAU, xs[p], keys[p], W.BIPRIME0, weight=ws[p], defer_exp=True)
                    for p in range(P)]
            with D.jl_exp_batch(dev):
                cts = [q.finish() for q in pend]
        for p in range(P):
            assert cts[p].shape[0] == 65
            assert torch.equal(cts[p], ref[p]), (form, p)
            assert torch.equal(ref[p], ref_old[p]), p


@pytest.mark.gpu
def test_key_zero_stays_on_the_table_path():
    from fedbiomed_amd.secagg import SecaggCrypter

    dev, jc = D.device(), SecaggCrypter()
    _, cr = O.jl_slot(None, P)
    x = _params(65, cr, 2)
    w = W.party_weight(2)
    qw = [int(v) * w for v in O.quantize(x.numpy().astype("float64"))]
    with D.jl_engine("single"):
        ct = jc.encrypt_tensor(P, TAU, x.to(dev), 0, W.BIPRIME0, weight=w)
    for k, got in zip((0, 64), D.limbs_to_ints(ct[[0, 64]].cpu().numpy())):
        assert got == O.jl_encrypt_ints(qw[k * cr:(k + 1) * cr], TAU, 0, W.BIPRIME0, P, k0=k)[0]


@pytest.mark.gpu
def test_small_modulus_stays_on_the_table_path():
    rng = random.Random(300)
    N = rng.getrandbits(200) | (1 << 199) | 1  # below 2^262: no short path
    n2, key = N * N, rng.getrandbits(700)
    x = torch.tensor([rng.getrandbits(63) for _ in range(65)], dtype=torch.int64, device=D.device())
    with D.jl_engine("single"):
        ct = D.jl_encrypt(x, N, key, TAU, P, slot=(100, 1))
    for k, got in zip((0, 64), D.limbs_to_ints(ct[[0, 64]].cpu().numpy())):
        assert got == ((N * int(x[k]) + 1) % n2) * O.powmod(O.fdh((k << 512) | TAU, n2), key, n2) % n2

"""The short path's split exponentiation on the GPU (|key| = k1 N + k0 >= N,
h^|key| = (h^k1 mod N)^N h^k0 mod N^2; fbm_na_chain_modn, fbm_na_chain_seg and N's window schedule in
jl_exp_kernel): encrypt_tensor and decrypt_factor_tensor bit-exact against the oracle and against the forced
unsplit chain (D.jl_split(False), the test build's fbm_jl_set_split) at the chunk boundary (a chunk is 256
ciphertexts) and at the key's edges -- N - 1 (no split), N (k0 = 0), N + 1 (an empty phase-1 chain), a k0
with bits inside N's first window, 2 040 bits, a negative key through the decryption factor's N-adic
output --; one batched launch that mixes a split segment, an unsplit one and the key 0; a 512-bit modulus."""

import random

import pytest
import torch

from fedbiomed_amd import _device as D, workload as W
from oracle import secagg_oracle as O
from tests.test_split_host import biprime

_RNG = random.Random(1023)
N0 = W.BIPRIME0
_K2040 = _RNG.getrandbits(2040) | (1 << 2039)
_K0_TOP = N0 - (1 << (N0.bit_length() - 4)) - 2  # below N, bits set among the six of N's first window
assert 0 < _K0_TOP < N0 and _K0_TOP >> (N0.bit_length() - 6)
EDGE_KEYS = [N0 - 1, N0, N0 + 1, 7 * N0 + _K0_TOP, _K2040, -_K2040]
P, TAU = 3, 6


def _params(n_ct, cr, seed):
    return torch.from_numpy(W.party_params(seed, n_ct * cr))


def _rows(n_ct):
    return sorted({0, n_ct - 1, min(n_ct - 1, 255)})


def _both(jc, xd, w, n_ct, key, biprime_=N0):
    """(ciphertexts, factor) under the split path and under the forced unsplit chain."""
    with D.jl_engine("single"):
        ct = jc.encrypt_tensor(P, TAU, xd, key, biprime_, weight=w)
        f = jc.decrypt_factor_tensor(TAU, n_ct, key, biprime_)
        with D.jl_split(False):
            ct_u = jc.encrypt_tensor(P, TAU, xd, key, biprime_, weight=w)
            f_u = jc.decrypt_factor_tensor(TAU, n_ct, key, biprime_)
    return ct, f, ct_u, f_u


def _check(n_ct, keys):
    from fedbiomed_amd.secagg import SecaggCrypter

    dev, jc, n2 = D.device(), SecaggCrypter(), N0 ** 2
    _, cr = O.jl_slot(None, P)
    x = _params(n_ct, cr, 1)
    xd, w = x.to(dev), W.party_weight(1)
    qw = [int(v) * w for v in O.quantize(x.numpy().astype("float64"))]
    rows = _rows(n_ct)
    h = {k: O.fdh((k << 512) | TAU, n2) for k in rows}
    for key in keys:
        ct, f, ct_u, f_u = _both(jc, xd, w, n_ct, key)
        assert ct.shape[0] == n_ct and f.shape[0] == n_ct
        assert torch.equal(ct, ct_u), hex(key)
        assert torch.equal(f, f_u), hex(key)
        got_f = D.limbs_to_ints(f[rows].cpu().numpy())
        got_c = D.limbs_to_ints(ct[rows].cpu().numpy())
        for i, k in enumerate(rows):
            assert got_f[i] == O.powmod(h[k], key, n2), (hex(key), k)
            assert got_c[i] == O.jl_encrypt_ints(qw[k * cr:(k + 1) * cr], TAU, key, N0, P, k0=k)[0], (hex(key), k)


@pytest.mark.gpu
@pytest.mark.parametrize("n_ct", [1, 255, 256, 257])
def test_split_at_the_chunk_boundary(n_ct):
    _check(n_ct, [_K2040, -_K2040])


@pytest.mark.gpu
def test_split_at_the_key_edges():
    _check(65, EDGE_KEYS)


@pytest.mark.gpu
def test_split_in_a_batched_launch():
    """Segments of 65 ciphertexts with a 2 040-bit key (split), a 1 000-bit key (below N: the unsplit chain) and
    the key 0 (the table path's one), in ONE launch: each equals its own launch and its own unsplit launch."""
    from fedbiomed_amd.secagg import SecaggCrypter

    dev, jc = D.device(), SecaggCrypter()
    _, cr = O.jl_slot(None, P)
    keys = [_K2040, _RNG.getrandbits(1000) | (1 << 999), 0]
    xs = [_params(65, cr, p).to(dev) for p in range(P)]
    ws = [W.party_weight(p) for p in range(P)]
    with D.jl_engine("single"):
        ref = [jc.encrypt_tensor(P, TAU, xs[p], keys[p], N0, weight=ws[p]) for p in range(P)]
        with D.jl_split(False):
            ref_u = [jc.encrypt_tensor(P, TAU, xs[p], keys[p], N0, weight=ws[p]) for p in range(P)]
    for split in (True, False):
        with D.jl_split(split), D.deferred_checks():
            pend = [jc.encrypt_tensor(P, TAU, xs[p], keys[p], N0, weight=ws[p], defer_exp=True) for p in range(P)]
            with D.jl_exp_batch(dev):
                cts = [q.finish() for q in pend]
        for p in range(P):
            assert cts[p].shape[0] == 65
            assert torch.equal(cts[p], ref[p]), (split, p)
            assert torch.equal(ref[p], ref_u[p]), p
    x = _params(65, cr, 0)
    qw = [int(v) * ws[0] for v in O.quantize(x.numpy().astype("float64"))]
    for k, got in zip((0, 64), D.limbs_to_ints(ref[0][[0, 64]].cpu().numpy())):
        assert got == O.jl_encrypt_ints(qw[k * cr:(k + 1) * cr], TAU, keys[0], N0, P, k0=k)[0]


@pytest.mark.gpu
def test_split_with_a_512_bit_modulus():
    """Another length of N: its schedule, bit count and word counts are the host's bookkeeping."""
    rng = random.Random(512)
    N = biprime(512, 2)
    n2 = N * N
    x = torch.tensor([rng.getrandbits(63) for _ in range(257)], dtype=torch.int64, device=D.device())
    for key in (N, 3 * N + rng.randrange(N), rng.getrandbits(1020) | (1 << 1019), N - 1):
        with D.jl_engine("single"):
            ct = D.jl_encrypt(x, N, key, TAU, P, slot=(100, 1))
            with D.jl_split(False):
                ct_u = D.jl_encrypt(x, N, key, TAU, P, slot=(100, 1))
        assert torch.equal(ct, ct_u), hex(key)
        for k, got in zip((0, 255, 256), D.limbs_to_ints(ct[[0, 255, 256]].cpu().numpy())):
            h = O.fdh((k << 512) | TAU, n2)
            assert h < 1 << 261  # one digest: the short path
            assert got == ((N * int(x[k]) + 1) % n2) * O.powmod(h, key, n2) % n2, (hex(key), k)

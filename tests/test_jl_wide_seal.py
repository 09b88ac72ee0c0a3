"""The wide family's encrypt from a factor computed ahead (jlw_seal_kernel: encrypt_tensor(factor=)) against the
oracle and the unprepared encrypt, and its streaming product (jlw_fold_kernel: D.jlw_fold) against Python's
integers.  Ciphertext counts 1, 4, 5 and 65: one wave, a full workgroup, one past it, a workgroup slot's second
round.  On the parent every call here is FB624 or an AttributeError."""
import random

import numpy as np
import pytest

from oracle import secagg_oracle as O
from tests.test_jl_wide import K_RAND, MODULI, _limbs

pytestmark = pytest.mark.gpu
TAU = 12  # a round whose H(t_k), k < 70, all exist on the all-ones modulus (round 11 has one that is FDH's OverflowError)
CASES = {"plain": (K_RAND, [None]), "negative_key": (-K_RAND, [None]), "weights": (K_RAND, [3, -2, 5]),
         "all_zero": (K_RAND, [None])}


def _env():
    import torch
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter
    return torch, D, SecaggCrypter(), D.jl_slot(None, 3)[1]


def _sealed(x, key, n, weight=None, off=0, clip=None, out=None):  # from the factor: limb for limb the unprepared call's
    torch, _, sc, cr = _env()
    f = sc.decrypt_factor_tensor(TAU, -(-x.numel() // cr), key, n, ct_offset=off)
    got = sc.encrypt_tensor(3, TAU, x, key, n, clipping_range=clip, weight=weight, factor=f, out=out)
    assert torch.equal(got, sc.encrypt_tensor(3, TAU, x, key, n, clipping_range=clip, weight=weight, ct_offset=off))
    return got, f


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("mod", MODULI)
def test_seal_matches_oracle(mod, case):
    """65 ciphertexts' worth of elements less one (a partial last plaintext), and its prefixes of 1, 4 and 5 full
    ciphertexts.  all_zero: integer zeros, pt = 0, the ciphertext is the factor itself."""
    torch, D, _, cr = _env()
    n, rng, (key, weights) = MODULI[mod], random.Random(5), CASES[case]
    for w in weights:
        if case == "all_zero":
            xs, dt = [0] * (65 * cr - 1), torch.int64
            want = O.jl_encrypt_ints(xs, TAU, key, n, 3)
        else:
            xs, dt = [rng.uniform(-2.5, 2.5) for _ in range(65 * cr - 1)], torch.float64
            want = O.jl_encrypt(xs, TAU, key, n, 3, weight=w)
        for n_ct in (1, 4, 5, 65):
            got, f = _sealed(torch.tensor(xs[:n_ct * cr], dtype=dt, device=D.device()), key, n, weight=w)
            assert D.limbs_to_ints_w(got, 128) == want[:n_ct], f"{mod} {case} weight {w} n_ct {n_ct}"
            assert case != "all_zero" or torch.equal(got, f)


@pytest.mark.parametrize("variant", ["clip_extremes", "ct_offset", "random"])
def test_seal_into_a_block_then_aggregate_and_fold(variant):
    """Three parties seal into the rows of one [3, 5, 128] block (out=): every slot at its extreme (x = +-clip), the
    factor made at ct_offset 3, or random inputs.  The block's aggregate is the oracle's floats as bytes, and so
    is the aggregate of its fold (one accumulator row, the slot of three parties)."""
    torch, D, sc, cr = _env()
    n, rng, m = MODULI["p_squared"], random.Random(6), 5 * cr - 1
    keys, off = [K_RAND, K_RAND >> 7, -(K_RAND >> 3)], 3 if variant == "ct_offset" else 0
    block = torch.empty((3, 5, 128), dtype=torch.int32, device=D.device())
    want_ct = []
    for p, key in enumerate(keys):
        xs = [rng.uniform(-3, 3) for _ in range(m)]
        if variant == "clip_extremes":  # all slots at the maximum, all at zero, a mix of both
            xs = [(3.0, -3.0, rng.choice((-3.0, 3.0)))[p] for _ in range(m)]
        x = torch.tensor(xs, dtype=torch.float64, device=D.device())
        assert _sealed(x, key, n, off=off, clip=3, out=block[p])[0].data_ptr() == block[p].data_ptr()
        want_ct.append(O.jl_encrypt(xs, TAU, key, n, 3, clip=3, k0=off))
    assert [D.limbs_to_ints_w(r, 128) for r in block] == want_ct
    got = sc.aggregate_tensor(TAU, block, -sum(keys), n, 3, clipping_range=3, num_expected_params=m, ct_offset=off)
    want = O.jl_crypter_aggregate(want_ct, TAU, -sum(keys), n, 3, m, clip=3, k0=off)
    assert got.cpu().numpy().tobytes() == np.asarray(want, np.float64).tobytes()
    acc = D.jlw_fold(torch.empty_like(block[0]), block, n, seed_ops=3)
    f = sc.decrypt_factor_tensor(TAU, 5, -sum(keys), n, ct_offset=off)
    folded, _ = D.jlw_aggregate(acc[None], n, -sum(keys), TAU, m, 3, clip=3, factor=f, slot=D.jl_slot(None, 3))
    assert torch.equal(folded, got)


@pytest.mark.parametrize("bad,match", [("shape", "FB624.*factor must be"), ("dtype", "FB624.*factor must be"),
                                       ("defer_exp", "FB624.*takes no `defer_exp`")])
def test_seal_refusals(bad, match):
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError
    torch, D, sc, _ = _env()
    f = torch.zeros((1, 64 if bad == "shape" else 128), dtype=torch.int64 if bad == "dtype" else torch.int32,
                    device=D.device())
    kw = {"defer_exp": True} if bad == "defer_exp" else {"factor": f}
    with pytest.raises(FedbiomedSecaggCrypterError, match=match):
        sc.encrypt_tensor(3, TAU, torch.zeros(3, dtype=torch.float64, device=D.device()), K_RAND, MODULI["3p"], **kw)


@pytest.mark.parametrize("n_ct", [1, 5, 65])
@pytest.mark.parametrize("mod", MODULI)
def test_fold_matches_python(mod, n_ct):
    """Rows from {0, 1, N^2 - 1, N^2, 2^4096 - 1, a seeded value} by the base-6 digits of 101 + c (c = 0: seeded,
    2^4096 - 1, N^2 - 1).  One call of k = 3, and a seeding k = 1 continued by k = 2, both give prod % N^2."""
    torch, D, _, _ = _env()
    n = MODULI[mod]
    pool = [0, 1, n * n - 1, n * n, (1 << 4096) - 1, random.Random(n_ct).getrandbits(4096)]
    rows = [[pool[(101 + c) // 6 ** j % 6] for c in range(n_ct)] for j in range(3)]
    t = torch.from_numpy(np.stack([_limbs(r, 128) for r in rows])).to(D.device())
    want = [a * b * c % (n * n) for a, b, c in zip(*rows)]
    one = D.jlw_fold(torch.empty_like(t[0]), t, n, seed_ops=3)
    two = D.jlw_fold(D.jlw_fold(torch.empty_like(t[0]), t[0], n, seed_ops=1), t[1:], n)
    assert D.limbs_to_ints_w(one, 128) == want and D.limbs_to_ints_w(two, 128) == want


@pytest.mark.parametrize("k,n_ct,null,want", [(0, 1, False, "FBM_E_ARG"), (1, 1, True, "FBM_E_ARG"),
                                              (1, 0, True, "FBM_OK")])
def test_fold_c_argument_checks(k, n_ct, null, want):
    from fedbiomed_amd import _native as N
    torch, D, _, _ = _env()
    buf = torch.zeros(4096, dtype=torch.uint8, device=D.device())
    bp = D.int_limbs(MODULI["3p"], 64)
    rc = N.load().fbm_jlw_fold(None if null else buf.data_ptr(), buf.data_ptr(), k, n_ct, bp.ctypes.data, 0,
                               buf.data_ptr(), None)
    assert rc == getattr(N, want)

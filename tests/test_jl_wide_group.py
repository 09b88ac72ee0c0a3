"""The wide family's group engine (csrc/fbm_jl_wide.hip, DESIGN 5.10: four lanes per ciphertext, 27-bit limbs, the
bases from jlw_base_kernel) forced by D.jlw_engine("group"), against Python's `pow` and the oracle; moduli, bases and
keys as tests/test_jl_wide.py's.  Without the engine every test fails at D.jlw_engine / D.jlw_engine_for."""

import random

import numpy as np
import pytest

from oracle import secagg_oracle as O
from tests.test_jl_wide import K_RAND, MODULI, _bases, _powmod

gpu = pytest.mark.gpu
T_GROUP = 8192  # the policy's measured crossover


def _group_powmod(n, key, rows, pts=None):
    from fedbiomed_amd import _device as D

    with D.jlw_engine("group"):
        return _powmod(n, key, rows, pts)


@gpu
@pytest.mark.parametrize("mod", MODULI)
def test_group_powmod_matches_python(mod):
    """h^key mod N^2 at 17 rows (a full group-wave plus one ciphertext) for every key; 1, 15, 16 and 65 rows (65: one
    past a 4-wave workgroup) and the plaintexts with the seeded 4090-bit key."""
    n = MODULI[mod]
    m, pool = n * n, _bases(n)
    for key in (0, 1, 1 << 4095, (1 << 4096) - 1, K_RAND, -K_RAND):
        ref = {h: pow(h, key, m) for h in pool}
        rows = [pool[i % len(pool)] for i in range(65)]
        assert _group_powmod(n, key, rows[:17]) == [ref[h] for h in rows[:17]], f"{mod} key {key.bit_length()} bits"
        if key == K_RAND:
            for count in (1, 15, 16, 65):
                assert _group_powmod(n, key, rows[:count]) == [ref[h] for h in rows[:count]], count
            pts = [0, 1, (1 << 1024) - 2, (1 << 1024) - 1]
            want = [(n * pt + 1) * ref[h] % m for h, pt in zip(pool, pts)]
            assert _group_powmod(n, key, pool, pts) == want


@gpu
def test_group_second_grid_pass():
    """One ciphertext more than the resident grid holds (2 workgroups a CU, 64 ciphertexts each): workgroup 0 runs its
    grid-stride loop twice."""
    import torch

    from fedbiomed_amd import _device as D

    n = MODULI["p_squared"]
    pool = _bases(n)
    ref = [pow(h, K_RAND, n * n) for h in pool]
    count = torch.cuda.get_device_properties(D.device()).multi_processor_count * 2 * 64 + 1
    got = _group_powmod(n, K_RAND, [pool[i % 4] for i in range(count)])
    assert got == [ref[i % 4] for i in range(count)]


@gpu
def test_group_flags():
    from fedbiomed_amd import _device as D

    n, tau = MODULI["all_ones"], (1 << 700) + 12345
    with pytest.raises(ZeroDivisionError):
        _group_powmod(n, -K_RAND, [1, 3 * 5 * 17, 1])
    assert _group_powmod(n, K_RAND, [15, 0]) == [pow(15, K_RAND, n * n), 0]

    def overflows(k):
        try:
            O.fdh((k << 512) | tau, n * n)
        except OverflowError:
            return True
        return False

    bad = next(k for k in range(1 << 20) if overflows(k))
    with D.jlw_engine("group"), pytest.raises(OverflowError):
        D.jlw_decrypt_factor(1, n, 1, tau, ct_offset=bad)


@gpu
def test_crypter_round_trip_under_the_group_engine():
    """encrypt_tensor x 3 parties and aggregate_tensor at 70 elements: the oracle's integers, its floats bit for bit;
    the decryption factor the wave engine's."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    n, tau, rng = MODULI["p_squared"], 7, random.Random(70)
    keys = [rng.getrandbits(4090) for _ in range(3)]
    xs = [[rng.uniform(-2.5, 2.5) for _ in range(70)] for _ in range(3)]
    sc = SecaggCrypter()
    want_ct = [O.jl_encrypt(x, tau, k, n, 3) for x, k in zip(xs, keys)]
    with D.jlw_engine("group"):
        cts = [sc.encrypt_tensor(3, tau, torch.tensor(x, dtype=torch.float64, device=D.device()), k, n)
               for x, k in zip(xs, keys)]
        got = sc.aggregate_tensor(tau, torch.stack(cts), -sum(keys), n, 3, num_expected_params=70)
        f_group = sc.decrypt_factor_tensor(tau, len(want_ct[0]), -sum(keys), n)
    assert [D.limbs_to_ints_w(c, 128) for c in cts] == want_ct
    want = O.jl_crypter_aggregate(want_ct, tau, -sum(keys), n, 3, 70)
    assert got.cpu().numpy().tobytes() == np.asarray(want, np.float64).tobytes()
    with D.jlw_engine("wave"):
        f_wave = sc.decrypt_factor_tensor(tau, len(want_ct[0]), -sum(keys), n)
    assert torch.equal(f_group, f_wave)


def test_policy():
    from fedbiomed_amd import _device as D

    assert [D.jlw_engine_for(c) for c in (1, T_GROUP - 1, T_GROUP, 1 << 20)] == ["wave", "wave", "group", "group"]
    for mode in ("wave", "group"):
        with D.jlw_engine(mode):
            assert [D.jlw_engine_for(c) for c in (1, 1 << 20)] == [mode, mode]
    assert D.jlw_engine_for(1) == "wave"

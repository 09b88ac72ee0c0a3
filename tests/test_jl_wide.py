"""Joye-Libert for biprimes of 1025 to 2048 bits (csrc/fbm_jl_wide.hip: one ciphertext per wave64, modulo
N^2 < 2^4096) against Python's own integers and hashlib: the kernels through D.jlw_powmod / D.jlw_decrypt_factor,
then SecaggCrypter's one-shot calls against the oracle, which takes any N.

Moduli: 3 (2^1024 - 105), just past the old bound (N^2's high words nearly empty); (2^1024 - 105)^2, 2048 bits,
every word used; 2^2048 - 1, all-ones words (maximal carries; about half of all digests share a factor with it,
so FDH's retries and the gcd's "no inverse" run on ordinary inputs).  On the parent every call here is FB624."""

import math
import random

import numpy as np
import pytest

from fedbiomed_amd import workload as W
from oracle import secagg_oracle as O

P1 = (1 << 1024) - 105
MODULI = {"3p": 3 * P1, "p_squared": P1 * P1, "all_ones": (1 << 2048) - 1}
K_RAND = random.Random(41).getrandbits(4090) | (1 << 4089)
pytestmark = pytest.mark.gpu


def _keys(n):
    return [1, 1 << 4095, (1 << 4096) - 1, K_RAND, -K_RAND, n * (K_RAND >> 2100)]


def _bases(n):
    """1, N^2 - 1, a value whose low word is zero, a seeded one: all coprime to N (a negative key inverts them)."""
    rng = random.Random(n % 1000003)
    z = rng.randrange(n * n >> 32) << 32
    r = rng.randrange(n * n)
    while math.gcd(z, n) != 1:
        z += 1 << 32
    while math.gcd(r, n) != 1:
        r += 1
    return [1, n * n - 1, z, r]


def _limbs(vals, words):
    blob = b"".join(int(v).to_bytes(4 * words, "little") for v in vals)
    return np.frombuffer(blob, dtype="<u4").reshape(len(vals), words).view(np.int32)


def _powmod(n, key, rows, pts=None):
    import torch

    from fedbiomed_amd import _device as D

    h = torch.from_numpy(_limbs(rows, 128).copy()).to(D.device())
    pt = None if pts is None else torch.from_numpy(_limbs(pts, 32).copy()).to(D.device())
    return D.limbs_to_ints_w(D.jlw_powmod(h, n, key, pt), 128)


@pytest.mark.parametrize("mod", MODULI)
def test_wide_powmod_matches_python(mod):
    """h^key mod N^2 at 65 rows (a second round of a workgroup slot's four waves) for every key; 1, 4 and 5 rows
    (one wave, a full workgroup, one past it) and the plaintexts with the 4090-bit key in both signs."""
    n = MODULI[mod]
    m, pool = n * n, _bases(n)
    for key in _keys(n):
        ref = {h: pow(h, key, m) for h in pool}
        rows = [pool[i % len(pool)] for i in range(65)]
        assert _powmod(n, key, rows) == [ref[h] for h in rows], f"{mod} key {key.bit_length()} bits, sign {key < 0}"
        if abs(key) == K_RAND:
            for count in (1, 4, 5):
                assert _powmod(n, key, rows[:count]) == [ref[h] for h in rows[:count]]
            pts = [0, 1, (1 << 1024) - 2, (1 << 1024) - 1]  # (the plaintext row is 1024 bits: N - 1 does not fit)
            want = [(n * pt + 1) * ref[h] % m for h, pt in zip(pool, pts)]
            assert _powmod(n, key, pool, pts) == want


def test_wide_powmod_refuses_a_base_without_inverse():
    from fedbiomed_amd import _device as D

    n = MODULI["all_ones"]
    with pytest.raises(ZeroDivisionError):
        _powmod(n, -K_RAND, [1, 3 * 5 * 17, 1])
    assert _powmod(n, K_RAND, [15, 0]) == [pow(15, K_RAND, n * n), 0]
    assert D.jl_wide(n) and not D.jl_wide(n + 1) and not D.jl_wide(W.BIPRIME0) and not D.jl_wide((1 << 2048) + 1)


def test_wide_fdh_matches_hashlib():
    """FDH(2048, N^2).H of 32 consecutive t on the all-ones modulus (the factor of key 1 is H itself), from an
    offset chosen here so that some need a second digest; then one t whose seven r all share a factor with N:
    the reference's OverflowError."""
    from fedbiomed_amd import _device as D

    n, tau = MODULI["all_ones"], (1 << 700) + 12345

    def fdh(k):
        try:
            return O.fdh((k << 512) | tau, n * n)
        except OverflowError:
            return None

    off = next(o for o in range(1 << 33, 1 << 34, 32) if all(fdh(o + k) for k in range(32)))
    want = [fdh(off + k) for k in range(32)]
    assert any(r.bit_length() > 256 for r in want)  # at least one retry
    assert D.limbs_to_ints_w(D.jlw_decrypt_factor(32, n, 1, tau, ct_offset=off), 128) == want
    bad = next(k for k in range(1 << 20) if fdh(k) is None)
    with pytest.raises(OverflowError):
        D.jlw_decrypt_factor(1, n, 1, tau, ct_offset=bad)


@pytest.mark.parametrize("mod,case", [(m, "plain") for m in MODULI] + [
    ("p_squared", "negative_keys"), ("p_squared", "weights"), ("3p", "negative_weight")])
def test_crypter_tensor_round_trip(mod, case):
    """encrypt_tensor x 3 parties, then aggregate_tensor, at 70 elements with the default target range: each
    ciphertext the oracle's integer, the aggregate the oracle's floats bit for bit.  The server key -sum(keys)
    is negative (its factor inverts H first); once the parties' keys are instead, once with weights, and once
    with a negative weight (the reference passes it: a negative plaintext, the ciphertext of N^2 - N|pt| + 1)."""
    import torch

    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter

    n, tau, rng = MODULI[mod], 7, random.Random(70)
    keys = [rng.getrandbits(4090) for _ in range(3)]
    if case == "negative_keys":
        keys = [-k for k in keys]
    weights = {"weights": [3, 1, 5], "negative_weight": [3, -2, 5]}.get(case, [None] * 3)
    xs = [[rng.uniform(-2.5, 2.5) for _ in range(70)] for _ in range(3)]
    sc = SecaggCrypter()
    cts = [sc.encrypt_tensor(3, tau, torch.tensor(x, dtype=torch.float64, device=D.device()), k, n, weight=w)
           for x, k, w in zip(xs, keys, weights)]
    want_ct = [O.jl_encrypt(x, tau, k, n, 3, weight=w) for x, k, w in zip(xs, keys, weights)]
    assert [D.limbs_to_ints_w(c, 128) for c in cts] == want_ct
    total = sum(w or 1 for w in weights)
    got = sc.aggregate_tensor(tau, torch.stack(cts), -sum(keys), n, total, num_expected_params=70)
    want = O.jl_crypter_aggregate(want_ct, tau, -sum(keys), n, total, 70)
    assert got.cpu().numpy().tobytes() == np.asarray(want, np.float64).tobytes()
    f = sc.decrypt_factor_tensor(tau, len(want_ct[0]), -sum(keys), n)
    again = sc.aggregate_tensor(tau, torch.stack(cts), -sum(keys), n, total, num_expected_params=70,
                                decrypt_factor=f, out_dtype=torch.float32)
    assert torch.equal(again, got.float())


@pytest.mark.parametrize("mod", MODULI)
def test_crypter_list_round_trip(mod):
    """The list API: every ciphertext the formula's integer below N^2, the aggregate the oracle's."""
    from fedbiomed_amd.secagg import SecaggCrypter

    n, tau, rng = MODULI[mod], 3, random.Random(9)
    keys = [rng.getrandbits(4090) for _ in range(2)]
    xs = [[rng.uniform(-3, 3) for _ in range(5)] for _ in range(2)]
    sc = SecaggCrypter()
    enc = [sc.encrypt(num_nodes=2, current_round=tau, params=x, key=k, biprime=n) for x, k in zip(xs, keys)]
    assert enc == [O.jl_encrypt(x, tau, k, n, 2) for x, k in zip(xs, keys)]
    agg = sc.aggregate(current_round=tau, num_nodes=2, params=enc, key=-sum(keys), biprime=n, total_sample_size=2,
                       num_expected_params=5)
    want = O.jl_crypter_aggregate(enc, tau, -sum(keys), n, 2, 5)
    assert np.asarray(agg, np.float64).tobytes() == np.asarray(want, np.float64).tobytes()


def test_prepare_and_streaming_still_refuse_a_wide_biprime():
    """Out of the wide engine's scope: prepare_* prepare nothing (so no factor stays behind), and a streaming
    aggregation raises FB624 at finish, in the one-shot's order, not a bare error out of add()."""
    from fedbiomed_amd.secagg import SecaggCrypter
    from fedbiomed_amd.exceptions import FedbiomedSecaggCrypterError

    n, sc = MODULI["3p"], SecaggCrypter()
    assert sc.prepare_encrypt(1, 2, K_RAND, n, 5) is False and SecaggCrypter._enc_prep is None
    assert sc.prepare_aggregate(1, 2, -K_RAND, n, 5) is False and getattr(sc, "_prepared", None) is None
    agg = sc.begin_aggregate(1, 1, -K_RAND, n, 1, num_expected_params=1)
    agg.add([n * n - 2])
    with pytest.raises(FedbiomedSecaggCrypterError, match="FB624.*biprime must be"):
        agg.finish()


def test_narrow_biprime_takes_the_code_it_took():
    """The dispatch did not move: the 1024-bit benchmark biprime still gives the oracle's 64-limb ciphertexts."""
    from fedbiomed_amd.secagg import SecaggCrypter

    x, key = [0.5, -1.25, 2.0], random.Random(2).getrandbits(2040)
    got = SecaggCrypter().encrypt(num_nodes=2, current_round=1, params=x, key=key, biprime=W.BIPRIME0)
    assert got == O.jl_encrypt(x, 1, key, W.BIPRIME0, 2)

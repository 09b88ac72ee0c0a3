"""The wave engine (csrc/fbm_jl_wave.hip: one ciphertext per wave64, FBM_ENGINE_WAVE = 5): its place in the
engine policy (CPU), the kernel against Python's pow through D.jl_powmod (GPU), and the crypter's small calls,
which take it under the default policy, against the oracle and against the quad engine (GPU).

Bases: 0, 1, 2, N, N + 1, N^2 - 1, N^2, 2^2048 - 1 (at or above the modulus), 2^256 - 1 and 2^261 (the short
path's thresholds: this engine has no short path, so the switch must change nothing), seeded values below
N^2; a negative key takes the ones coprime to N.  Row counts: 7 (a partial last workgroup of 4 waves whose
last chunk holds 3, and 5 = a lone last wave, with the plaintexts) and twice the resident waves plus three
(the chunk loop), tiled from at most 16 bases."""

import math
import random

import numpy as np
import pytest

from fedbiomed_amd import workload as W

MODULI = {"biprime0": W.BIPRIME0, "2p1024m105": (1 << 1024) - 105, "below2p262": (1 << 261) + 2**200 + 1}
K_RAND = random.Random(31).getrandbits(2040) | (1 << 2039)
KEYS = [0, 1, 2, (1 << 2040) - 1, K_RAND, -K_RAND, -1]


def _pool(n, invertible):
    m, rng = n * n, random.Random(n % 1000003)
    pool = [1, 2, n + 1, m - 1, (1 << 2048) - 1, (1 << 256) - 1, 1 << 261] + [rng.randrange(m) for _ in range(3)]
    if invertible:
        return [h for h in pool if math.gcd(h, n) == 1]
    return [0, n, m] + pool


_REF = {}


def _ref(n, key):
    """{h: pow(h, key, N^2)}, one pow per base; a negative key's is the positive one's inverse."""
    if (n, key) not in _REF:
        m = n * n
        _REF[(n, key)] = ({h: pow(h, key, m) for h in _pool(n, False)} if key >= 0 else
                          {h: pow(_ref(n, -key)[h], -1, m) for h in _pool(n, True)})
    return _REF[(n, key)]


def _limbs(vals, words):
    blob = b"".join(int(v).to_bytes(4 * words, "little") for v in vals)
    return np.frombuffer(blob, dtype="<u4").reshape(len(vals), words).view(np.int32)


def _powmod(n, key, rows, pts=None, short=True):
    import torch

    from fedbiomed_amd import _device as D

    h = torch.from_numpy(_limbs(rows, 64).copy()).to(D.device())
    pt = None if pts is None else torch.from_numpy(_limbs(pts, 32).copy()).to(D.device())
    with D.jl_engine("wave"), D.jl_short(short):
        assert D.jl_engine_for(len(rows)) == "wave"
        out = D.jl_powmod(h, n, key, pt)
    return D.limbs_to_ints(D.to_host(out).numpy().view(np.uint32))


def test_engine_policy():
    """CPU: the engine id is accepted, auto takes it for one ciphertext and leaves 1 000 to the quad engine."""
    from fedbiomed_amd import _device as D, _native as N

    lib = N.load_test()
    prev = lib.fbm_jl_set_engine(0)
    try:
        assert lib.fbm_jl_set_engine(5) == 0 and lib.fbm_jl_set_engine(0) == 5
        assert lib.fbm_jl_set_engine(7) < 0  # FBM_E_ARG, the policy unchanged
        assert lib.fbm_jl_engine_for(1) == 5 and lib.fbm_jl_engine_for(1000) == 4
        with D.jl_engine("wave"):
            assert D.jl_engine_for(1000) == "wave"
        assert lib.fbm_jl_set_engine(0) == 0
    finally:
        lib.fbm_jl_set_engine(prev)


@pytest.mark.gpu
@pytest.mark.parametrize("mod", MODULI)
def test_wave_powmod_matches_python(mod):
    n = MODULI[mod]
    m = n * n
    for key in KEYS:
        pool = _pool(n, key < 0)
        rows = [pool[i % len(pool)] for i in range(max(7, len(pool)))]
        rows = rows[:len(rows) - (len(rows) % 4 == 0)]  # never a whole number of workgroups
        ref = _ref(n, key)
        got = _powmod(n, key, rows)
        assert got == [ref[h] for h in rows], f"{mod} key {key.bit_length()} bits, sign {key < 0}"
        if key in (K_RAND, -K_RAND):  # with plaintexts, 5 rows (a lone last wave), and the short switch off
            pts = [0, 1, n - 1, n, (1 << 1024) - 1]
            want = [(n * pt + 1) * ref[h] % m for h, pt in zip(rows, pts)]
            assert _powmod(n, key, rows[:5], pts) == want
            assert _powmod(n, key, rows[:5], pts, short=False) == want


@pytest.mark.gpu
def test_wave_chunk_loop():
    """Twice the resident waves plus three rows: every workgroup pulls more than one chunk."""
    import torch

    n = W.BIPRIME0
    resident = 2 * 4 * torch.cuda.get_device_properties(0).multi_processor_count
    pool = _pool(n, False)[:16]
    rows = [pool[i % len(pool)] for i in range(2 * resident + 3)]
    ref = _ref(n, K_RAND)
    assert _powmod(n, K_RAND, rows) == [ref[h] for h in rows]


@pytest.mark.gpu
@pytest.mark.parametrize("n_params", [1, 40])
def test_crypter_small_calls_take_the_wave_engine(n_params):
    """Default policy: encrypt and a three-party aggregate with a negative server key (N-adic output, inverse,
    lift), bit for bit the oracle's and the quad engine's."""
    from fedbiomed_amd import _device as D
    from fedbiomed_amd.secagg import SecaggCrypter
    from oracle import secagg_oracle as O

    rng = random.Random(n_params)
    keys = [rng.getrandbits(2040) for _ in range(3)]
    xs = [[rng.uniform(-2.5, 2.5) for _ in range(n_params)] for _ in range(3)]
    sc = SecaggCrypter()

    def run():
        enc = [sc.encrypt(num_nodes=3, current_round=4, params=x, key=k, biprime=W.BIPRIME0) for x, k in zip(xs, keys)]
        return enc, sc.aggregate(current_round=4, num_nodes=3, params=enc, key=-sum(keys), biprime=W.BIPRIME0,
                                 total_sample_size=3, num_expected_params=n_params)

    with D.jl_engine("auto"):
        assert D.jl_engine_for(n_params) == "wave"
        enc, agg = run()
    assert enc == [O.jl_encrypt(x, 4, k, W.BIPRIME0, 3) for x, k in zip(xs, keys)]
    want = O.jl_crypter_aggregate(enc, 4, -sum(keys), W.BIPRIME0, 3, n_params)
    assert np.asarray(agg, np.float64).tobytes() == np.asarray(want, np.float64).tobytes()
    with D.jl_engine("quad"):
        assert run() == (enc, agg)

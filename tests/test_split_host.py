"""The split exponentiation's host schedule (fbm_setup.hip build_split, through the test build's
fbm_test_split_consts; no GPU): for |key| = k1 N + k0 >= N the words of k1 and k0, C1 = 2^f1 R^2 mod N,
C' = 2^(261 k0) R mod N^2, the Montgomery one and N's window schedule, against Python integers -- keys at
the edges (N - 1 has no split; N: k0 = 0, C' = R; N + 1 and 2N - 1: k1 = 1, an empty phase-1 chain, f1 = 0;
N^2 - 1), the bench's keys, a negative key (its magnitude), biprimes of 512 and 1024 bits; the replayed
schedule is N; the constants survive the cache and a clear."""

import random

import numpy as np
import pytest

from fedbiomed_amd import _build, _native, workload as W
from tests.test_nadic_chain_asm import _is_prime

LB, L, KS = 29, 36, 9
R = 1 << (LB * L)


def limbs(x, n=L):
    return [(x >> (LB * k)) & ((1 << LB) - 1) for k in range(n)]


def biprime(bits, seed):
    rng, ps = random.Random(seed), []
    while len(ps) < 2:
        p = rng.getrandbits(bits // 2) | (3 << (bits // 2 - 2)) | 1
        if _is_prime(p, rng):
            ps.append(p)
    assert (ps[0] * ps[1]).bit_length() == bits
    return ps[0] * ps[1]


def split_consts(lib, N, key):
    n32 = np.frombuffer(N.to_bytes(128, "little"), dtype=np.uint32).copy()
    k64 = np.frombuffer(abs(key).to_bytes(256, "little"), dtype=np.uint32).copy()
    k1w, k0w, c1 = np.zeros(64, np.uint32), np.zeros(32, np.uint32), np.zeros(36, np.uint32)
    cp, one, nops = np.zeros(72, np.uint32), np.zeros(72, np.uint32), np.zeros(512, np.uint16)
    n_nops, nbn, win = (np.zeros(1, np.int32) for _ in range(3))
    r = lib.fbm_test_split_consts(*(a.ctypes.data for a in (n32, k64, k1w, k0w, c1, cp, one, nops, n_nops, nbn, win)))
    words = lambda a: sum(int(v) << (32 * i) for i, v in enumerate(a))  # noqa: E731
    return r, words(k1w), words(k0w), [int(v) for v in c1], [int(v) for v in cp], [int(v) for v in one], \
        [int(v) for v in nops[:int(n_nops[0])]], int(nbn[0]), int(win[0])


def check(lib, N, key):
    M, e = N * N, abs(key)
    r, k1, k0, c1, cp, one, nops, nbn, win = split_consts(lib, N, key)
    if e < N:
        assert r == -1
        return
    assert (k1, k0) == divmod(e, N) and r == k1.bit_length() - 1 and nbn == N.bit_length()
    s1 = k1.bit_length() - 1
    f1 = LB * L * ((1 << s1) - 1) + LB * KS * (k1 - (1 << s1))
    assert c1 == limbs(pow(2, f1, N) * R * R % N)
    v = pow(2, LB * KS * k0, M) * R % M
    assert cp == limbs(v % N) + limbs(v // N)
    assert one == limbs(R % M % N) + limbs(R % M // N)
    # N's schedule, replayed from the accumulator 1: every window an op, odd digits below 2^win
    acc = 0
    assert 3 <= win <= 6 and nops
    for op in nops:
        nsq, idx = op >> 6, (op & 63) - 1
        assert 1 <= nsq and idx < 1 << (win - 1)
        acc <<= nsq
        if idx >= 0:
            assert nsq >= (2 * idx + 1).bit_length()  # the window fits the squarings that precede its product
            acc += 2 * idx + 1
    assert acc == N and sum(op >> 6 for op in nops) == nbn


@pytest.fixture(scope="module")
def lib():
    _build.build()
    lib = _native.load_test()
    lib.fbm_jl_clear_caches()
    yield lib
    lib.fbm_jl_clear_caches()


@pytest.mark.parametrize("N", [W.BIPRIME0, biprime(1024, 1), biprime(512, 2)], ids=["biprime0", "b1024", "b512"])
def test_split_constants_at_the_key_edges(lib, N):
    rng = random.Random(N % 1000)
    for key in (N - 1, N, N + 1, 2 * N - 1, N * N - 1, -(3 * N + rng.randrange(N)), rng.getrandbits(2040) | (1 << 2039)):
        check(lib, N, key)


def test_split_constants_of_the_bench_keys(lib):
    keys = [W.jl_user_key(p) for p in range(8)] + [W.jl_server_key(8)]
    for key in keys:
        assert abs(key) >= W.BIPRIME0
        check(lib, W.BIPRIME0, key)
    # served from the cache, and rebuilt after a clear: the same constants
    first = split_consts(lib, W.BIPRIME0, keys[0])
    assert split_consts(lib, W.BIPRIME0, keys[0]) == first
    lib.fbm_jl_clear_caches()
    assert split_consts(lib, W.BIPRIME0, keys[0]) == first


def test_no_split_outside_the_short_path(lib):
    assert split_consts(lib, (1 << 262) - 1, 1 << 300)[0] == -2   # N at or below 2^262
    assert split_consts(lib, W.BIPRIME0 + 1, 1 << 1500)[0] == -2  # an even modulus
    assert split_consts(lib, W.BIPRIME0, 0)[0] == -1               # the key 0 has no chain

"""The host big integers of the C ABI's setup (fedbiomed_amd/csrc/fbm_bigint.hpp: the one library under
fbm_setup.hip's per-modulus and per-key constants) against Python's integers, on the CPU.  The header is
host-only standard C++, so the test builds tools/bigint_host_check.cpp (a stand-alone program that
includes nothing else of the project) with the host compiler and feeds it `op operands expected` lines;
the program exits non-zero at the first mismatch.

Covered: mul, mullo, divmod (odd and even divisors), shr, ctz, to_limbs at 28 and 29 bits, inv_mod_pow2 at
1 / 31 / 32 / 33 / 1024 / 2046 bits, and pow2_mod -- exponents 0, 1, 63, 64, 2 088 and a 2 060-bit one over
the moduli 1, 3, a one-word one, a 33-word one whose top word is zero and a 64-word one.  The modulus 1 is
pinned to 1, not 0: the doubling loop pow2_mod replaced gave that, and fbm_jl_fdh_msg hands it to its wide
kernel for a power-of-two modulus (odd part 1).

`python -c "from tests.test_host_bigint import vectors; print('\\n'.join(vectors()))"` prints the same
vectors for a run of the program built with -fsanitize=address,undefined (see its header comment)."""

import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "bigint_host_check.cpp")
HEADER = os.path.join(ROOT, "fedbiomed_amd", "csrc", "fbm_bigint.hpp")


def vectors():
    rng = random.Random(0xB161)
    h = lambda v: format(v, "x")
    out = []

    def rnd(bits):  # exactly `bits` bits
        return rng.getrandbits(bits) | (1 << (bits - 1)) if bits else 0

    sizes = [0, 1, 31, 32, 33, 64, 261, 1024, 1044, 2048, 2080]
    for a_bits in sizes:
        for b_bits in (0, 1, 32, 1024, 2048):
            a, b = rnd(a_bits), rnd(b_bits)
            out.append(f"mul {h(a)} {h(b)} {h(a * b)}")
    for n in (1, 2, 3, 32, 64):
        for a_bits, b_bits in ((1, 1), (32 * n, 32 * n), (32 * n + 40, 17), (17, 32 * n + 40), (32 * n - 1, 2048)):
            a, b = rnd(a_bits), rnd(b_bits)
            out.append(f"mullo {h(a)} {h(b)} {n:x} {h(a * b % (1 << (32 * n)))}")
    for a_bits in (0, 1, 32, 33, 1024, 2048, 2088, 4129):
        for m in (1, 2, 3, rnd(32), rnd(32) | 1, rnd(1024) | 1, rnd(1024) & ~1 | 2, rnd(2048) | 1, 1 << 1023,
                  rnd(900) << 40):
            a = rnd(a_bits)
            out.append(f"divmod {h(a)} {h(m)} {h(a // m)} {h(a % m)}")
    a = rnd(1024)
    out.append(f"divmod {h(a)} {h(a)} 1 0")
    out.append(f"divmod {h(a - 1)} {h(a)} 0 {h(a - 1)}")
    for a_bits in (1, 32, 33, 1024, 2048):
        a = rnd(a_bits)
        for s in (0, 1, 31, 32, 33, 63, 64, 1000, a_bits - 1, a_bits, a_bits + 31):
            out.append(f"shr {h(a)} {s:x} {h(a >> s)}")
    for tz in (0, 1, 31, 32, 33, 40, 1023, 2046):
        a = (rnd(64) | 1) << tz
        out.append(f"ctz {h(a)} {tz:x}")
    out.append("ctz 0 0")
    for lb, nls in ((28, (37, 74)), (29, (36, 72))):
        for nl in nls:
            for a in (0, 1, rnd(nl * lb), (1 << (nl * lb)) - 1, rnd(1024), rnd(nl * lb - 35), rnd(nl * lb + 50)):
                limbs = [(a >> (lb * k)) & ((1 << lb) - 1) for k in range(nl)]
                out.append(f"to_limbs {h(a)} {nl:x} {lb:x} {h(sum(v << (32 * k) for k, v in enumerate(limbs)))}")
    moduli = ["1", "3", h(rnd(32) | 1), h(rnd(31) | 1), h(rnd(1024) | 1), h(rnd(2048) | 1), h((1 << 2048) - 1),
              format(rnd(1010) | 1, "0264x"),  # 33 words, the top one zero
              "0000000000000001"]  # the modulus 1 in two words
    exps = [0, 1, 63, 64, 2088, rnd(2060), 1044, 3132, 1280, 2048, 4144, rnd(33), rnd(64)]
    for mh in moduli:
        m = int(mh, 16)
        for e in exps:
            want = pow(2, e, m) if m > 1 else 1
            out.append(f"pow2_mod {h(e)} {mh} {h(want)}")
            if e < 1 << 64:
                out.append(f"pow2_mod_u64 {h(e)} {mh} {h(want)}")
    for bits in (1, 31, 32, 33, 1024, 2046):
        for a_bits in (1, 32, 64, 1024, 2048):
            for _ in range(2):
                a = rnd(a_bits) | 1
                out.append(f"inv_mod_pow2 {h(a)} {bits:x} {h(pow(a, -1, 1 << bits))}")
    return out


@pytest.fixture(scope="module")
def cxx():
    c = shutil.which(os.environ.get("CXX", "g++"))
    if not c:
        pytest.skip("no g++")
    return c


@pytest.fixture(scope="module")
def exe(cxx, tmp_path_factory):
    out = tmp_path_factory.mktemp("bigint") / "bigint_host_check"
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", SRC, "-o", str(out)], check=True)
    return str(out)


def test_header_compiles_alone(cxx):
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", HEADER], check=True)


def test_bigint_against_python_integers(exe):
    vs = vectors()
    assert 300 <= len(vs) <= 2000
    r = subprocess.run([exe], input="\n".join(vs) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[0] == str(len(vs))


def test_check_program_reports_a_mismatch(exe):
    """The program's verdict is its exit status: a wrong expectation must fail it (2^64 mod 3 is 1)."""
    r = subprocess.run([exe], input="pow2_mod 40 3 2\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "MISMATCH" in r.stderr

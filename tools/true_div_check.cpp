// Host check of the average step's int / int true division (fbm_true_div_u128 in fedbiomed_amd/csrc/fbm_common.hpp:
// the source the LOM aggregate, the JL decode and fbm_int_ops run on the device) under the host sanitizers.  The
// routine shifts 128-bit values by up to 118 bits, and by amounts it derives from the operands' bit lengths (k, -k,
// extra): UndefinedBehaviorSanitizer sees every family of tests/true_div_cases.py, generated here in C++ -- ties
// (2m + 1) W 2^sh of either parity and their neighbours, the carry out of the significand, quotients just below an
// integer, the fast path's edge at 2^53 in either operand, the extremes (1 over 2^64 - 1, all-ones over 1) -- and
// seeded random operands of every pair of bit lengths.  Each result is compared, bit for bit, with a reference of
// its own: the numerator normalised to 128 bits, a bit-serial restoring division of the 192-bit a' 2^64 by b, and one
// round-half-even of the quotient's bits with the remainder as the sticky bit.  A stand-alone program: it is never
// loaded into Python.
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -fno-sanitize-recover=all tools/true_div_check.cpp -o true_div_check && ./true_div_check [random pairs, default 200000]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../fedbiomed_amd/csrc/fbm_common.hpp"

typedef unsigned __int128 u128;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dull;
}

static int bitlen(u128 v) {
  int n = 0;
  while (v) ++n, v >>= 1;
  return n;
}

// the correctly rounded double of a / b (a < 2^128, 1 <= b < 2^64), by long division
static double reference(u128 a, uint64_t b) {
  if (a == 0) return 0.0;
  const int norm = 128 - bitlen(a);  // a' = a 2^norm has its top bit at 127
  u128 an = a;
  for (int i = 0; i < norm; ++i) an += an;
  unsigned char q[192];  // q = floor(a' 2^64 / b), bit i at q[i]: at least 128 bits
  u128 rem = 0;          // < b after every step
  for (int i = 191; i >= 0; --i) {
    const unsigned bit = i >= 64 ? (unsigned)((an >> (i - 64)) & 1) : 0u;
    rem = rem + rem + bit;
    q[i] = rem >= b;
    if (q[i]) rem -= b;
  }
  int top = 191;
  while (!q[top]) --top;
  uint64_t m = 0;  // the 53 leading bits
  for (int i = top; i > top - 53; --i) m = 2 * m + q[i];
  const bool half = q[top - 53];
  bool sticky = rem != 0;
  for (int i = top - 54; i >= 0; --i) sticky = sticky || q[i];
  if (half && (sticky || (m & 1))) ++m;  // 2^53 after a carry: still exact below
  return ldexp((double)m, (top - 52) - 64 - norm);
}

static long g_checked = 0;
static void check(u128 a, uint64_t b) {
  const double got = fbm_true_div_u128(a, b), want = reference(a, b);
  ++g_checked;
  if (memcmp(&got, &want, sizeof(got)) != 0) {
    fprintf(stderr, "FAILED: 0x%016llx%016llx / 0x%016llx: got %a, long division gives %a\n",
            (unsigned long long)(uint64_t)(a >> 64), (unsigned long long)(uint64_t)a, (unsigned long long)b, got, want);
    exit(1);
  }
}

// t - 1, t, t + 1 where t = v W 2^sh fits 128 bits (v of `bits` bits at most)
static void around(uint64_t v, int bits, uint64_t w, int sh) {
  if (bits + bitlen(w) + sh > 128) return;
  const u128 t = ((u128)v * w) << sh;
  check(t - 1, w), check(t, w);
  if (t + 1 != 0) check(t + 1, w);
}

int main(int argc, char** argv) {
  const long n_random = argc > 1 ? atol(argv[1]) : 200000;
  const uint64_t divisors[] = {1, 2, 3, 7, 10, 1000, 1023, 8017, 0xffffffffull, 0x100000001ull,
                               (1ull << 53) - 1, 1ull << 53, (1ull << 53) + 1, 1ull << 63, ~0ull};
  for (uint64_t w : divisors) {
    const int room = 128 - 54 - bitlen(w);
    for (int sh = 0; sh <= room; ++sh) {
      for (int rep = 0; rep < 8; ++rep) {  // ties, either parity of the kept bits, and their neighbours
        const uint64_t m = (1ull << 52) | (((rnd() >> 13) << 1) & ((1ull << 52) - 1)) | (uint64_t)(rep & 1);
        around(2 * m + 1, 54, w, sh);
      }
      around((1ull << 54) - 1, 54, w, sh);  // the rounded significand carries out
    }
    if (w >= 5)  // m W - 1 rounds up to the integer m
      for (int rep = 0; rep < 64; ++rep) {
        const uint64_t lo = rep & 1 ? 1ull << 52 : 1ull << 51;
        around(rep < 2 ? lo : rep < 4 ? 2 * lo - 1 : lo + rnd() % lo, 53, w, 0);
      }
    const u128 edge[] = {((u128)1 << 53) - 1, (u128)1 << 53, ((u128)1 << 53) + 1, 0, 1, w - 1, w, ~(u128)0,
                         ((u128)1 << 64) - 1, (u128)1 << 64, ((u128)1 << 64) - 1025, ((u128)1 << 64) - 1024};
    for (u128 a : edge) check(a, w);
  }
  // every pair of bit lengths
  for (int la = 1; la <= 128; ++la)
    for (int lb = 1; lb <= 64; ++lb)
      for (int rep = 0; rep < 4; ++rep) {
        const u128 a = ((((u128)rnd() << 64) | rnd()) >> (128 - la)) | ((u128)1 << (la - 1));
        const uint64_t b = (rnd() >> (64 - lb)) | (1ull << (lb - 1));
        check(a, b);
        check(rep & 1 ? (u128)1 << (la - 1) : a, rep & 2 ? 1ull << (lb - 1) : b);  // powers of two
      }
  for (long i = 0; i < n_random; ++i) {
    const int la = 1 + (int)(rnd() % 128), lb = 1 + (int)(rnd() % 64);
    u128 a = (((u128)rnd() << 64) | rnd()) >> (128 - la);
    const uint64_t b = (rnd() >> (64 - lb)) | 1ull;
    if (rnd() % 4 == 0) a -= a % b;  // an exact quotient
    check(a, b);
  }
  printf("true_div_check: %ld divisions over %zu divisors and every pair of bit lengths; no finding\n", g_checked,
         sizeof(divisors) / sizeof(divisors[0]));
  return 0;
}

// Stand-alone host run of the 16-bit widening and the narrowing helpers of fedbiomed_amd/csrc/fbm_common.hpp
// (the source the kernels run), for a sanitizer build -- shifts, casts and index arithmetic over every input:
//
//   hipcc --cuda-host-only -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -fno-sanitize-recover=all -Iinclude tools/conv_host_check.cpp -o /tmp/conv_host_check && /tmp/conv_host_check
//
// Every one of the 65 536 patterns of both 16-bit types is widened and compared with the compiler's own
// conversion; every finite 16-bit value, every midpoint between neighbours and its two double neighbours, the
// overflow edges and 1M random doubles are narrowed and compared with the compiler's float64 -> float32 ->
// 16-bit casts (round-to-nearest-even, twice).  Prints the counts and returns 1 on a mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../fedbiomed_amd/csrc/fbm_common.hpp"

static uint32_t f32_bits(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
static float f32_from(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint16_t f16_bits(_Float16 h) {
  uint16_t b;
  memcpy(&b, &h, 2);
  return b;
}
static _Float16 f16_from(uint16_t b) {
  _Float16 h;
  memcpy(&h, &b, 2);
  return h;
}
// the compiler's bfloat16 of a float32: RN-even on the upper half, NaN kept a NaN
static uint16_t bf16_of(float f) {
  const uint32_t b = f32_bits(f);
  if (f != f) return (uint16_t)((b >> 16) | 0x40u);
  return (uint16_t)((b + 0x7fffu + ((b >> 16) & 1u)) >> 16);
}

static long bad = 0;
static void expect(bool ok, const char* what, double v, uint32_t got, uint32_t want) {
  if (ok) return;
  if (++bad <= 10) printf("MISMATCH %s: v=%a got=%#x want=%#x\n", what, v, got, want);
}

static void narrow_all(double v) {
  const float f = (float)v;
  const bool nan = v != v;
  const uint32_t g32 = fbm_out<float>::bits(v);
  expect(nan ? f32_from(g32) != f32_from(g32) : g32 == f32_bits(f), "f32", v, g32, f32_bits(f));
  const uint16_t g16 = fbm_out<fbm_f16>::bits(v), w16 = f16_bits((_Float16)f);
  expect(nan ? (g16 & 0x7fffu) > 0x7c00u : g16 == w16, "f16", v, g16, w16);
  const uint16_t gb = fbm_out<fbm_bf16>::bits(v), wb = bf16_of(f);
  expect(nan ? (gb & 0x7fffu) > 0x7f80u : gb == wb, "bf16", v, gb, wb);
}

int main() {
  long widened = 0, narrowed = 0;
  std::vector<double> v16[2];
  for (uint32_t b = 0; b < 65536; ++b) {
    const fbm_f16 h{(uint16_t)b};
    const fbm_bf16 g{(uint16_t)b};
    const double dh = fbm_widen(h), wh = (double)f16_from((uint16_t)b);
    const double dg = fbm_widen(g), wg = (double)f32_from(b << 16);
    expect(wh != wh ? dh != dh : fbm_f64_bits(dh) == fbm_f64_bits(wh), "widen f16", wh, b, b);
    expect(wg != wg ? dg != dg : fbm_f64_bits(dg) == fbm_f64_bits(wg), "widen bf16", wg, b, b);
    widened += 2;
    if (std::isfinite(wh) && !(b & 0x8000u)) v16[0].push_back(wh);  // ascending in the pattern
    if (std::isfinite(wg) && !(b & 0x8000u)) v16[1].push_back(wg);
  }
  for (const auto& vals : v16) {
    for (size_t i = 0; i < vals.size(); ++i) {
      for (double s : {1.0, -1.0}) {
        narrow_all(s * vals[i]);
        ++narrowed;
        if (i + 1 == vals.size()) continue;
        const double mid = s * (vals[i] + vals[i + 1]) / 2;
        for (double p : {mid, std::nextafter(mid, -INFINITY), std::nextafter(mid, INFINITY)}) {
          narrow_all(p);
          ++narrowed;
        }
      }
    }
  }
  for (double v : {(double)INFINITY, -(double)INFINITY, (double)NAN, 65504.0, 65519.99, 65520.0, -65520.0, 1e-8, 3.4e38,
                   6.8e38, 1 + 0x1p-8 + 0x1p-40, 1 + 0x1p-11 + 0x1p-40, 0x1p-149, 0x1p-150, 0x1p-151, 4.9e-324, 1.7e308}) {
    narrow_all(v);
    ++narrowed;
  }
  std::mt19937_64 rng(7);
  std::uniform_real_distribution<double> u(-3.0, 3.0);
  for (int i = 0; i < 1000000; ++i) {
    narrow_all(u(rng));
    ++narrowed;
  }
  for (int i = 0; i < 1000000; ++i) {  // any double at all: every exponent, NaN payloads
    narrow_all(fbm_f64_from_bits(rng()));
    ++narrowed;
  }
  printf("widened %ld patterns, narrowed %ld values to 3 types: %ld mismatches\n", widened, narrowed, bad);
  return bad ? 1 : 0;
}

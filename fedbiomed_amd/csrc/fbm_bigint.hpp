// fedbiomed_amd -- the host big-integer helpers of the C ABI's per-modulus and per-key setup
// (fbm_setup.hip).  Host only, standard C++17, no HIP: tools/bigint_host_check.cpp runs it
// against Python's integers (tests/test_host_bigint.py).  Tiny operands (at most ~4 200 bits), a
// few calls per modulus or key: schoolbook throughout.
#ifndef FBM_BIGINT_HPP  // (a guard, not #pragma once: the file also compiles on its own)
#define FBM_BIGINT_HPP
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace fbm {

typedef std::vector<uint32_t> Big;  // little-endian 32-bit limbs

inline int big_bits(const Big& a) {
  for (int i = (int)a.size() - 1; i >= 0; --i)
    if (a[i]) return 32 * i + 32 - __builtin_clz(a[i]);
  return 0;
}

inline void big_trim(Big& a) {
  while (a.size() > 1 && a.back() == 0u) a.pop_back();
}

inline int big_ctz(const Big& a) {
  for (size_t i = 0; i < a.size(); ++i)
    if (a[i]) return 32 * (int)i + __builtin_ctz(a[i]);
  return 0;
}

inline int big_cmp(const Big& a, const Big& b) {
  const size_t n = a.size() > b.size() ? a.size() : b.size();
  for (size_t k = n; k-- > 0;) {
    const uint32_t x = k < a.size() ? a[k] : 0u, y = k < b.size() ? b[k] : 0u;
    if (x != y) return x > y ? 1 : -1;
  }
  return 0;
}

inline void big_sub_inplace(Big& a, const Big& b) {  // a >= b
  int64_t br = 0;
  for (size_t k = 0; k < a.size(); ++k) {
    const int64_t d = (int64_t)a[k] - (int64_t)(k < b.size() ? b[k] : 0u) + br;
    a[k] = (uint32_t)d;
    br = d < 0 ? -1 : 0;
  }
}

// a <- 2 a + c over n limbs of either width (c: the bit shifted in); returns the bit shifted out
template <class T>
inline T shl1(T* a, size_t n, T c = 0) {
  for (size_t k = 0; k < n; ++k) {
    const T nc = a[k] >> (8 * sizeof(T) - 1);
    a[k] = (T)(a[k] << 1) | c;
    c = nc;
  }
  return c;
}

inline Big big_mul(const Big& a, const Big& b) {
  Big r(a.size() + b.size(), 0u);
  for (size_t i = 0; i < a.size(); ++i) {
    uint64_t c = 0;
    for (size_t j = 0; j < b.size(); ++j) {
      const uint64_t t = (uint64_t)a[i] * b[j] + r[i + j] + c;
      r[i + j] = (uint32_t)t;
      c = t >> 32;
    }
    r[i + b.size()] = (uint32_t)c;
  }
  return r;
}

// a b mod 2^(32 n)
inline Big big_mullo(const Big& a, const Big& b, size_t n) {
  Big r(n, 0u);
  for (size_t i = 0; i < n && i < a.size(); ++i) {
    uint64_t c = 0;
    for (size_t j = 0; i + j < n; ++j) {
      const uint64_t t = (uint64_t)a[i] * (j < b.size() ? b[j] : 0u) + r[i + j] + c;
      r[i + j] = (uint32_t)t;
      c = t >> 32;
    }
  }
  return r;
}

inline Big big_shr(const Big& a, int s) {
  Big r(a.size(), 0u);
  const int w = s >> 5, b = s & 31;
  for (size_t i = 0; i + w < a.size(); ++i) {
    const uint64_t lo = a[i + w], hi = i + w + 1 < a.size() ? a[i + w + 1] : 0u;
    r[i] = (uint32_t)((((hi << 32) | lo) >> b));
  }
  big_trim(r);
  return r;
}

// (q, r) = (a div m, a mod m) by binary long division (m >= 1, odd or even)
inline void big_divmod(const Big& a, const Big& m, Big& q, Big& r) {
  q.assign(a.size(), 0u);
  r.assign(m.size() + 1, 0u);
  for (int i = big_bits(a) - 1; i >= 0; --i) {
    shl1(r.data(), r.size(), (a[i >> 5] >> (i & 31)) & 1u);
    if (big_cmp(r, m) >= 0) {
      big_sub_inplace(r, m);
      q[i >> 5] |= 1u << (i & 31);
    }
  }
}

// a's nl limbs of lb bits (lb <= 32; bits past a read as zero)
inline void to_limbs(const Big& a, uint32_t* o, int nl, int lb) {
  for (int k = 0; k < nl; ++k) {
    const int bit = k * lb, wi = bit >> 5, sh = bit & 31;
    const uint64_t lo = wi < (int)a.size() ? a[wi] : 0u;
    const uint64_t hi = wi + 1 < (int)a.size() ? a[wi + 1] : 0u;
    o[k] = (uint32_t)(((hi << 32) | lo) >> sh) & (uint32_t)((1ull << lb) - 1u);
  }
}

// -m0^-1 modulo the width of T (uint32_t or uint64_t; m0 odd) by Newton: m0 is its own inverse
// to 3 bits, six steps reach 192
template <class T>
inline T neg_inv(T m0) {
  T inv = m0;
  for (int i = 0; i < 6; ++i) inv *= (T)2 - m0 * inv;
  return (T)0 - inv;
}

// a^-1 mod 2^bits (a odd, bits >= 1) in ceil(bits / 32) words: Newton's y <- y (2 - a y), 32 -> 64 -> ... bits
inline Big inv_mod_pow2(const Big& a, int bits) {
  const size_t W = (size_t)((bits + 31) / 32);
  Big y(W, 0u);
  y[0] = 0u - neg_inv<uint32_t>(a[0]);
  for (size_t prec = 32; prec < 32 * W; prec *= 2) {
    Big t = big_mullo(a, y, W);
    uint64_t c = 3;  // 2 - t = ~t + 3 (mod 2^(32 W))
    for (size_t i = 0; i < W; ++i) {
      c += (uint32_t)~t[i];
      t[i] = (uint32_t)c;
      c >>= 32;
    }
    y = big_mullo(y, t, W);
  }
  if (bits & 31) y[W - 1] &= (1u << (bits & 31)) - 1u;
  return y;
}

// 2^E mod m for an ODD m of at most 2048 bits (N^2 of the largest biprime; a wider m gives an empty result)
// and any E.  An even m must not get here: Montgomery needs m^-1 mod 2^64.
// Left-to-right over E: Montgomery squarings (64-bit limbs, CIOS) and modular doublings -- one
// product per bit of E.  The result has an even number of words (m's 64-bit limbs).
// m = 1 gives 1, not 0: the doubling loop this routine replaced subtracted m at most once per
// step, and fbm_jl_fdh_msg hands the result for a power-of-two modulus (odd part 1) to its kernel.
constexpr size_t POW2_MOD_LIMBS = 32;
inline Big pow2_mod(const Big& E, Big m) {
  big_trim(m);
  if (m.size() == 1 && m[0] == 1u) return Big{1u, 0u};
  const size_t n = (m.size() + 1) / 2;
  if (n > POW2_MOD_LIMBS) return Big();
  uint64_t M[POW2_MOD_LIMBS] = {0}, x[POW2_MOD_LIMBS] = {0}, one[POW2_MOD_LIMBS] = {0};
  for (size_t i = 0; i < m.size(); ++i) M[i / 2] |= (uint64_t)m[i] << (32 * (i & 1));
  const uint64_t mi = neg_inv<uint64_t>(M[0]);
  auto ge_sub = [&, n](uint64_t* a, uint64_t top) {  // a <- a - M if (top:a) >= M
    bool ge = top != 0;
    if (!ge) {
      ge = true;
      for (size_t k = n; k-- > 0;)
        if (a[k] != M[k]) {
          ge = a[k] > M[k];
          break;
        }
    }
    if (!ge) return;
    unsigned __int128 br = 0;
    for (size_t k = 0; k < n; ++k) {
      const unsigned __int128 d = (unsigned __int128)a[k] - M[k] - br;
      a[k] = (uint64_t)d;
      br = (d >> 64) & 1u;
    }
  };
  auto mul = [&, n, mi](const uint64_t* a, const uint64_t* b, uint64_t* r) {  // a b 2^-64n mod M (CIOS)
    uint64_t t[POW2_MOD_LIMBS + 2] = {0};  // (a local the operands cannot alias: the loops stay in registers)
    for (size_t i = 0; i < n; ++i) {
      const uint64_t bi = b[i];
      unsigned __int128 c = 0;
      for (size_t j = 0; j < n; ++j) {
        c += (unsigned __int128)a[j] * bi + t[j];
        t[j] = (uint64_t)c;
        c >>= 64;
      }
      c += t[n];
      t[n] = (uint64_t)c;
      t[n + 1] = (uint64_t)(c >> 64);
      const uint64_t q = t[0] * mi;
      c = ((unsigned __int128)q * M[0] + t[0]) >> 64;
      for (size_t j = 1; j < n; ++j) {
        c += (unsigned __int128)q * M[j] + t[j];
        t[j - 1] = (uint64_t)c;
        c >>= 64;
      }
      c += t[n];
      t[n - 1] = (uint64_t)c;
      t[n] = t[n + 1] + (uint64_t)(c >> 64);
    }
    ge_sub(t, t[n]);
    for (size_t k = 0; k < n; ++k) r[k] = t[k];
  };
  auto dbl = [&, n](uint64_t* a) { ge_sub(a, shl1(a, n)); };
  // 1 in Montgomery form, 2^(64 n) mod M: from 2^(bits(M) - 1) < M, at most 64 doublings
  const int top = big_bits(m) - 1;
  x[(size_t)top / 64] = 1ull << (top % 64);
  for (size_t i = (size_t)top; i < 64 * n; ++i) dbl(x);
  for (int b = big_bits(E) - 1; b >= 0; --b) {
    mul(x, x, x);
    if ((E[b >> 5] >> (b & 31)) & 1u) dbl(x);
  }
  one[0] = 1;
  mul(x, one, x);
  Big r(2 * n, 0u);
  for (size_t k = 0; k < n; ++k) {
    r[2 * k] = (uint32_t)x[k];
    r[2 * k + 1] = (uint32_t)(x[k] >> 32);
  }
  return r;
}

inline Big pow2_mod(uint64_t e, const Big& m) {
  const Big E = {(uint32_t)e, (uint32_t)(e >> 32)};
  return pow2_mod(E, m);
}

}  // namespace fbm

#endif  // FBM_BIGINT_HPP

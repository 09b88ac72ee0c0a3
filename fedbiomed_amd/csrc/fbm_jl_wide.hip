// fedbiomed_amd -- Joye-Libert for biprimes of 1025 to 2048 bits: one ciphertext per wave64, all arithmetic
// modulo M = N^2 < 2^4096 with R = 2^4096.  The word-per-lane picture of fbm_jl_wave.hip with
// two words per lane:
//   * lane j owns the 64-bit digit j of a residue (words 2j and 2j + 1), of the operand and of M; residues are
//     canonical (< M) between products;
//   * the product is scanned by the 128 words of B: b_i is wave-uniform (v_readlane); every lane adds a_j b_i
//     and m_j q_i into its accumulators with v_mad_u64_u32 -- one 64-bit accumulator per word position and per
//     operand (U0, U1 for a b; V0, V1 for m q), so none of them can pass 2^64 - 1 and no carry is tracked;
//   * the quotient digit q_i = lo(acc at word 0) (-M^-1) mod 2^32 is formed on the scalar unit from lane 0
//     (v_readfirstlane); the carry of lane 0's retired word stays a scalar (K);
//   * a row retires one word: position p takes hi(acc_p) + lo(acc_{p+1}).  Word 2j + 1 is the same lane's, so
//     only word 2j + 2 crosses lanes: one DPP move (wave_shl:1) per accumulator pair and row;
//   * carries are resolved once per product on the 64-bit digits: generate / propagate masks by __ballot, one
//     64-bit scalar add, for T and for T + 2^4096 - M (the conditional subtraction picks by the latter's carry).
// Exponent: |key| < 2^4096 in fixed windows of 5 bits, left to right; the wave's table of the powers 1..31 lives
// in LDS (31 x 512 B per wave, lane j reads its own digit).  Inverse and coprimality: one wave-wide binary
// extended gcd in Kaliski's almost-Montgomery form (jw_kaliski).  FDH(2048, N^2).H runs in the wave: lanes
// 0..6 hash the digests of the counters 1..7, r is gathered by ds_bpermute.  No scratch, no global tables.
#include "fbm_internal.hpp"

namespace fbm {

#define FBM_JW_WAVES 4  // waves (ciphertexts) per workgroup: 4 x 15.5 KB of LDS
#define FBM_JW_BLOCK (64 * FBM_JW_WAVES)
#define FBM_JW_WGS_PER_CU 2  // 124 KB of the CU's 160 KB of LDS; two waves per SIMD
#define FBM_JW_WIN 5
#define FBM_JW_TABLE ((1 << FBM_JW_WIN) - 1)  // g^1 .. g^31

typedef unsigned __int128 jw_u128;

__device__ __forceinline__ uint32_t jw_up32(uint32_t v) {  // lane j <- lane j + 1 (lane 63 <- 0)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t jw_down32(uint32_t v) {  // lane j <- lane j - 1 (lane 0 <- 0)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint64_t jw_up64(uint64_t v) {
  return ((uint64_t)jw_up32((uint32_t)(v >> 32)) << 32) | jw_up32((uint32_t)v);
}
__device__ __forceinline__ uint64_t jw_down64(uint64_t v) {
  return ((uint64_t)jw_down32((uint32_t)(v >> 32)) << 32) | jw_down32((uint32_t)v);
}
__device__ __forceinline__ uint32_t jw_first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t jw_lane(uint32_t v, int i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, i); }
__device__ __forceinline__ uint64_t jw_bit(uint64_t mask, int lane) { return (mask >> lane) & 1ull; }

// carry (or borrow) into every digit from the digits that generate one (G) and those that pass one on (P; no digit
// does both): the adder's chain, one scalar add.  out: the carry out of digit 63.
__device__ __forceinline__ uint64_t jw_chain(uint64_t G, uint64_t P, uint32_t& out) {
  const uint64_t g = G << 1, S = P + g;
  out = (uint32_t)(G >> 63) + (S < P ? 1u : 0u);
  return S ^ P;
}

// sum_j (L_j + H_j 2^64) 2^(64 j) -> its digits (lane j: digit j) and what lies at or above 2^4096 (ovf)
__device__ __forceinline__ uint64_t jw_resolve(uint64_t L, uint64_t H, int lane, uint32_t& ovf) {
  const uint64_t t = L + jw_down64(H);
  uint32_t co;
  const uint64_t cin = jw_chain(__ballot(t < L), __ballot(t == ~0ull), co);
  ovf = jw_lane((uint32_t)H, 63) + co;  // (H < 2^32 wherever the overflow is looked at)
  return t + jw_bit(cin, lane);
}

// a + b (no carry out of digit 63 is reported) / a - b for a >= b, lt = the digits with a_j < b_j
__device__ __forceinline__ uint64_t jw_add(uint64_t a, uint64_t b, int lane) {
  const uint64_t t = a + b;
  uint32_t co;
  return t + jw_bit(jw_chain(__ballot(t < a), __ballot(t == ~0ull), co), lane);
}
__device__ __forceinline__ uint64_t jw_sub(uint64_t a, uint64_t b, uint64_t lt, int lane) {
  uint32_t bo;
  return a - b - jw_bit(jw_chain(lt, __ballot(a == b), bo), lane);
}
__device__ __forceinline__ bool jw_less(uint64_t a, uint64_t b) {  // the highest digit that differs decides
  return __ballot(a < b) > __ballot(a > b);
}
__device__ __forceinline__ uint64_t jw_shr1(uint64_t v) { return (v >> 1) | (jw_up64(v) << 63); }
__device__ __forceinline__ uint64_t jw_shl1(uint64_t v) { return (v << 1) | (jw_down64(v) >> 63); }

// one row of the scan: the word bi of B
__device__ __forceinline__ void jw_row(uint64_t& U0, uint64_t& U1, uint64_t& V0, uint64_t& V1, uint32_t& K, uint32_t a0,
                                       uint32_t a1, uint32_t m0, uint32_t m1, uint32_t bi, uint32_t m00, uint32_t mp) {
  const uint32_t sv = jw_first((uint32_t)V0);
  U0 += (uint64_t)a0 * bi;
  U1 += (uint64_t)a1 * bi;
  const uint32_t su = jw_first((uint32_t)U0);
  const uint32_t q = (su + sv + K) * mp;
  V0 += (uint64_t)m0 * q;
  V1 += (uint64_t)m1 * q;
  // lane 0's retired words: lo U0 + lo V0 + K = 0 (mod 2^32), its carry stays at word 0
  const uint32_t sv2 = sv + q * m00;
  K = (uint32_t)(((uint64_t)su + sv2 + K) >> 32);
  const uint32_t u0 = (uint32_t)U0, v0 = (uint32_t)V0;
  U0 = (U0 >> 32) + (uint32_t)U1;
  V0 = (V0 >> 32) + (uint32_t)V1;
  U1 = (U1 >> 32) + jw_up32(u0);
  V1 = (V1 >> 32) + jw_up32(v0);
}

// a b 2^-4096 mod the odd modulus m (lane j: digit j; m00 = m's word 0, mp = -m^-1 mod 2^32), canonical, for
// a b < m 2^4096 (one operand below m, the other below 2^4096)
__device__ __forceinline__ uint64_t jw_mul(uint64_t a, uint64_t b, uint64_t m, uint32_t m00, uint32_t mp, int lane) {
  const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
  const uint32_t m0 = (uint32_t)m, m1 = (uint32_t)(m >> 32);
  uint64_t U0 = 0, U1 = 0, V0 = 0, V1 = 0;
  uint32_t K = 0;
#pragma unroll 2
  for (int i = 0; i < 64; ++i) {
    jw_row(U0, U1, V0, V1, K, a0, a1, m0, m1, jw_lane(b0, i), m00, mp);
    jw_row(U0, U1, V0, V1, K, a0, a1, m0, m1, jw_lane(b1, i), m00, mp);
  }
  const jw_u128 sT = (jw_u128)U0 + V0 + (lane == 0 ? K : 0u) + (((jw_u128)U1 + V1) << 32);
  uint32_t ovT, ovD;
  const uint64_t wT = jw_resolve((uint64_t)sT, (uint64_t)(sT >> 64), lane, ovT);
  const jw_u128 sD = (jw_u128)wT + ~m + (lane == 0 ? 1u : 0u);  // T + 2^4096 - m
  const uint64_t wD = jw_resolve((uint64_t)sD, (uint64_t)(sD >> 64), lane, ovD);
  return (ovT | ovD) ? wD : wT;
}

// a b mod 2^2048 for a, b < 2^2048 (lanes 32..63 hold zeros): the same scan without a modulus, the retired word
// of row i is word i of the product
__device__ __forceinline__ uint64_t jw_mullo(uint64_t a, uint64_t b, int lane) {
  const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
  uint64_t U0 = 0, U1 = 0, x = 0;
#pragma unroll 2
  for (int i = 0; i < 32; ++i) {
#pragma unroll
    for (int hw = 0; hw < 2; ++hw) {
      const uint32_t bi = jw_lane(hw ? b1 : b0, i);
      U0 += (uint64_t)a0 * bi;
      U1 += (uint64_t)a1 * bi;
      const uint32_t w = jw_first((uint32_t)U0), u0 = (uint32_t)U0;
      if (lane == i) x |= (uint64_t)w << (32 * hw);
      U0 = (U0 >> 32) + (uint32_t)U1;
      U1 = (U1 >> 32) + jw_up32(u0);
    }
  }
  return x;
}

// Kaliski's almost-Montgomery inverse on the digit-per-lane layout: the binary extended gcd of the odd p and
// 0 < a, with a r = -u 2^k and a s = v 2^k (mod p) kept throughout (u s + v r = p, so r, s <= p fit the digits).
// Each step is wave-uniform: a compare by two ballots, a subtraction with a ballot borrow chain, shifts by DPP.
// The loop stops at u == v (= the gcd) instead of running the last step to v = 0: that step would double r past
// 2^4096.  Returns gcd == 1.  INV: x = a^-1 2^k mod p for a < p (k steps, the last one included; p's bit length <=
// k <= 8192); else only the gcd is formed (any a < 2^4096).  A loop that passes its bound (it cannot) is flagged.
template <bool INV>
__device__ __forceinline__ bool jw_kaliski(uint64_t a, uint64_t p, int lane, uint64_t& x, int& kout, uint32_t& err) {
  uint64_t u = p, v = a, r = 0, s = lane == 0 ? 1u : 0u;
  if (__ballot(v != 0) == 0) return false;
  int k = 0;
  bool met = false;
#pragma unroll 1
  for (; k < 8192; ++k) {
    if (!(jw_first((uint32_t)u) & 1u)) {
      u = jw_shr1(u);
      if (INV) s = jw_shl1(s);
    } else if (!(jw_first((uint32_t)v) & 1u)) {
      v = jw_shr1(v);
      if (INV) r = jw_shl1(r);
    } else {
      const uint64_t lt = __ballot(u < v), gt = __ballot(u > v);
      if ((lt | gt) == 0) {
        met = true;
        break;
      }
      if (gt > lt) {
        u = jw_shr1(jw_sub(u, v, lt, lane));
        if (INV) {
          r = jw_add(r, s, lane);
          s = jw_shl1(s);
        }
      } else {
        v = jw_shr1(jw_sub(v, u, gt, lane));
        if (INV) {
          s = jw_add(s, r, lane);
          r = jw_shl1(r);
        }
      }
    }
  }
  if (!met) {
    err |= FBM_ERR_ITER_CAP;
    return false;
  }
  if (__ballot(u != (lane == 0 ? 1u : 0u)) != 0) return false;
  if (!INV) return true;
  // the last step: r <- 2 r (< 2 p, the bit shifted out of digit 63 included) mod p, then x = p - r
  const bool top = (jw_lane((uint32_t)(r >> 32), 63) >> 31) != 0;
  r = jw_shl1(r);
  if (top || !jw_less(r, p)) r = jw_sub(r, p, __ballot(r < p), lane);
  x = jw_sub(p, r, __ballot(p < r), lane);
  kout = k + 1;
  return true;
}

// the call's constants in the workspace (JlwConsts, written by jlw_setup_kernel)
struct JwMod {
  uint64_t m, one, r2;  // M, R mod M, R^2 mod M: this lane's digits
  uint32_t m00, mp;
};
__device__ __forceinline__ uint64_t jw_digit(const uint32_t* w, int lane) {
  return reinterpret_cast<const uint64_t*>(w)[lane];
}
__device__ __forceinline__ uint64_t jw_digit_lo(const uint32_t* w, int lane) {  // a 64-word constant, zero above
  return lane < 32 ? reinterpret_cast<const uint64_t*>(w)[lane] : 0ull;
}
__device__ __forceinline__ JwMod jw_mod(const JlwConsts* c, int lane) {
  JwMod k;
  k.m = jw_digit(c->M, lane);
  k.one = jw_digit(c->one, lane);
  k.r2 = jw_digit(c->R2, lane);
  k.m00 = jw_first((uint32_t)k.m);
  k.mp = c->mp;
  return k;
}
__device__ __forceinline__ uint64_t jw_mm(uint64_t a, uint64_t b, const JwMod& k, int lane) {
  return jw_mul(a, b, k.m, k.m00, k.mp, lane);
}

// a^-1 R mod M from the canonical a; false: no inverse
__device__ __forceinline__ bool jw_inverse(uint64_t a, const JwMod& k, int lane, uint64_t& out, uint32_t& err) {
  uint64_t x = 0;
  int kk = 0;
  if (!jw_kaliski<true>(a, k.m, lane, x, kk, err)) return false;
  // x = a^-1 2^kk: one product by a power of two (after one by R^2 where kk <= 4096) leaves a^-1 2^4096
  int e = 8192 - kk;
  if (kk <= 4096) {
    x = jw_mm(x, k.r2, k, lane);
    e = 4096 - kk;
  }
  out = jw_mm(x, lane == (e >> 6) ? 1ull << (e & 63) : 0ull, k, lane);
  return true;
}

// g^|key| R from g R (the Montgomery one for a zero key): fixed windows of FBM_JW_WIN bits, the powers 1..31 in
// the wave's LDS table
__device__ __forceinline__ uint32_t jw_window(const uint32_t* kw, int w) {
  const int bit = FBM_JW_WIN * w, wi = bit >> 5;
  uint64_t v = kw[wi];
  if (wi + 1 < 128) v |= (uint64_t)kw[wi + 1] << 32;
  return (uint32_t)(v >> (bit & 31)) & ((1u << FBM_JW_WIN) - 1u);
}
__device__ __forceinline__ uint64_t jw_pow(uint64_t g, const JlwConsts* c, const JwMod& k, uint64_t* tbl, int lane) {
  const int kbits = c->key_bits;
  if (kbits == 0) return k.one;
  uint64_t acc = g;
  tbl[0] = g;
#pragma unroll 1
  for (int t = 1; t < FBM_JW_TABLE; ++t) {
    acc = jw_mm(acc, g, k, lane);
    tbl[t * 64] = acc;
  }
  int w = (kbits - 1) / FBM_JW_WIN;
  acc = tbl[(jw_first(jw_window(c->key, w)) - 1u) * 64];  // the leading window holds the key's top bit
#pragma unroll 1
  for (--w; w >= 0; --w) {
#pragma unroll 1
    for (int q = 0; q < FBM_JW_WIN; ++q) acc = jw_mm(acc, acc, k, lane);
    const uint32_t d = jw_first(jw_window(c->key, w));
    if (d) acc = jw_mm(acc, tbl[(d - 1u) * 64], k, lane);
  }
  return acc;
}

// FDH(2048, N^2).H(t), t = (idx << 512) | tau (fbm_jl.hip's jl_fdh_kernel, _jls.py:727-762): r = D1 || .. || Dc for
// the first c in 1..7 with gcd(r, N) == 1 (gcd(r, N^2) == 1 is that); none: the reference's OverflowError.
// Every lane runs the two blocks of t, lane l < 7 the digest of counter l + 1; lane j of r (words 2j, 2j + 1)
// gathers its two words from the lane of its digest.
__device__ __forceinline__ uint64_t jw_fdh(const JlwConsts* c, uint64_t idx, int lane, uint32_t& err) {
  uint32_t st[8], d[8], W[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) st[i] = c->mid[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) W[i] = c->tau14_w[i];
  W[14] |= (uint32_t)(idx >> 32);
  W[15] |= (uint32_t)idx;
  fbm_sha256_compress(st, W);
#pragma unroll
  for (int i = 0; i < 16; ++i) W[i] = c->tau_w[i];
  fbm_sha256_compress(st, W);
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] = st[i];
#pragma unroll
  for (int i = 0; i < 16; ++i) W[i] = 0u;
  W[0] = ((uint32_t)(lane % 7 + 1) << 24) | (0x80u << 16);
  W[15] = 8200u;
  fbm_sha256_compress(d, W);
  const uint64_t n = jw_digit_lo(c->N, lane);
  uint64_t r = 0;
  bool ok = false;
#pragma unroll 1
  for (int cc = 1; cc <= 7 && !ok; ++cc) {
    // r's word w is word 7 - w % 8 of digest cc - 1 - w / 8 (D1 is the most significant)
    const bool in = lane < 4 * cc;
    const int src = in ? cc - 1 - (lane >> 2) : 0, at = (2 * lane) & 7;
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint32_t t = (uint32_t)__shfl((int)d[i], src);
      lo = (7 - at) == i ? t : lo;
      hi = (6 - at) == i ? t : hi;
    }
    r = in ? ((uint64_t)hi << 32) | lo : 0ull;
    uint64_t x;
    int kk;
    ok = jw_kaliski<false>(r, n, lane, x, kk, err);
  }
  if (!ok) err |= FBM_ERR_FDH_OVERFLOW;
  return r;
}

// H(t_k)^key mod N^2 (ENC: times N pt_k + 1), one ciphertext per wave.  Hin != nullptr: the bases h_k given as rows
// of 128 words (< 2^4096) instead of the hash.  A negative key inverts the base first, as gmpy2's powmod does; a
// base with no inverse is flagged and its row is zero.  pt: |pt| < 2^1024 as rows of 32 words, neg_pt its sign.
template <bool ENC>
__device__ __forceinline__ void jw_exp_body(const uint32_t* __restrict__ Hin, const uint32_t* __restrict__ pt, int neg_pt,
                                            uint64_t n_ct, const JlwConsts* __restrict__ c, uint32_t* __restrict__ out,
                                            uint32_t* __restrict__ stats, uint64_t* tbl_s) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t* tbl = tbl_s + wv * (FBM_JW_TABLE * 64) + lane;
  const JwMod k = jw_mod(c, lane);
  uint32_t err = 0;
#pragma unroll 1
  for (uint64_t ct = (uint64_t)blockIdx.x * FBM_JW_WAVES + wv; ct < n_ct; ct += (uint64_t)gridDim.x * FBM_JW_WAVES) {
    const uint64_t h = Hin ? jw_digit(Hin + ct * 128, lane) : jw_fdh(c, ct + c->ct_offset, lane, err);
    uint64_t g = jw_mm(h, k.r2, k, lane);  // h R
    bool ok = true;
    if (c->key_negative && c->key_bits) {
      ok = jw_inverse(jw_mm(g, lane == 0 ? 1u : 0u, k, lane), k, lane, g, err);
      if (!ok) err |= FBM_ERR_NOT_INVERTIBLE;
    }
    uint64_t v = 0;
    if (ok) {
      g = jw_pow(g, c, k, tbl, lane);
      uint64_t last = lane == 0 ? 1u : 0u;
      if (ENC) {  // N |pt| mod M, a multiple of N below M: +1, or M - it + 1 for a negative plaintext
        const uint64_t p = lane < 16 ? jw_digit(pt + ct * 32, lane) : 0ull;
        const uint64_t np = jw_mm(p, jw_digit(c->NR, lane), k, lane);
        uint32_t ov;
        if (neg_pt && __ballot(np != 0) != 0) {
          const jw_u128 s = (jw_u128)k.m + ~np + (lane == 0 ? 2u : 0u);
          last = jw_resolve((uint64_t)s, (uint64_t)(s >> 64), lane, ov);
        } else {
          const jw_u128 s = (jw_u128)np + (lane == 0 ? 1u : 0u);
          last = jw_resolve((uint64_t)s, (uint64_t)(s >> 64), lane, ov);
        }
      }
      v = jw_mm(g, last, k, lane);
    }
    reinterpret_cast<uint64_t*>(out + ct * 128)[lane] = v;
  }
  if (err && lane == 0) atomicOr(stats + FBM_STAT_ERRFLAGS, err);
}

__global__ void __launch_bounds__(FBM_JW_BLOCK, FBM_JW_WGS_PER_CU)
    jlw_encrypt_kernel(const uint32_t* __restrict__ Hin, const uint32_t* __restrict__ pt, int neg_pt, uint64_t n_ct,
                       const JlwConsts* __restrict__ c, uint32_t* __restrict__ out, uint32_t* __restrict__ stats) {
  __shared__ uint64_t tbl_s[FBM_JW_WAVES * FBM_JW_TABLE * 64];
  jw_exp_body<true>(Hin, pt, neg_pt, n_ct, c, out, stats, tbl_s);
}

__global__ void __launch_bounds__(FBM_JW_BLOCK, FBM_JW_WGS_PER_CU)
    jlw_factor_kernel(const uint32_t* __restrict__ Hin, uint64_t n_ct, const JlwConsts* __restrict__ c,
                      uint32_t* __restrict__ out, uint32_t* __restrict__ stats) {
  __shared__ uint64_t tbl_s[FBM_JW_WAVES * FBM_JW_TABLE * 64];
  jw_exp_body<false>(Hin, nullptr, 0, n_ct, c, out, stats, tbl_s);
}

// v = prod_u cts[u][k] * factor[k] mod N^2, then x = (v - 1) / N -- exact for the scheme's ciphertexts, as the
// product ((v - 1) mod 2^2048) N^-1 mod 2^2048 -- written as the 32-word plaintext row jl_decode_kernel reads
// (x < N; VES.decode reads its low es cr <= 1024 bits).  v = 0 gives N - 1, Python's (-1) // N mod N.
__global__ void __launch_bounds__(FBM_JW_BLOCK)
    jlw_combine_kernel(const uint32_t* __restrict__ cts, int n_parties, uint64_t n_ct, const uint32_t* __restrict__ factor,
                       const JlwConsts* __restrict__ c, uint32_t* __restrict__ xout) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const JwMod k = jw_mod(c, lane);
  const uint64_t n = jw_digit_lo(c->N, lane), ninv = jw_digit_lo(c->Ninv, lane);
#pragma unroll 1
  for (uint64_t ct = (uint64_t)blockIdx.x * FBM_JW_WAVES + wv; ct < n_ct; ct += (uint64_t)gridDim.x * FBM_JW_WAVES) {
    uint64_t acc = jw_mm(jw_digit(factor + ct * 128, lane), k.r2, k, lane);  // F R
#pragma unroll 1
    for (int u = 0; u < n_parties; ++u) {
      const uint64_t cu = jw_mm(jw_digit(cts + ((uint64_t)u * n_ct + ct) * 128, lane), k.r2, k, lane);
      acc = jw_mm(acc, cu, k, lane);
    }
    const uint64_t v = jw_mm(acc, lane == 0 ? 1u : 0u, k, lane);
    uint64_t x;
    if (__ballot(v != 0) == 0) {
      x = jw_sub(n, lane == 0 ? 1u : 0u, __ballot(n < (lane == 0 ? 1u : 0u)), lane);
    } else {
      const uint64_t one = lane == 0 ? 1u : 0u;
      const uint64_t vm1 = jw_sub(v, one, __ballot(v < one), lane);
      x = jw_mullo(lane < 32 ? vm1 : 0ull, ninv, lane);
    }
    if (lane < 16) reinterpret_cast<uint64_t*>(xout + ct * 32)[lane] = x;
  }
}

__global__ void jlw_setup_kernel(JlwConsts c, uint32_t* __restrict__ dst) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&c);
  for (int i = threadIdx.x; i < (int)(sizeof(JlwConsts) / 4); i += blockDim.x) dst[i] = src[i];
}

static unsigned jlw_grid(uint64_t n_ct, int wgs_per_cu) {
  uint64_t g = (n_ct + FBM_JW_WAVES - 1) / FBM_JW_WAVES;
  const uint64_t gmax = (uint64_t)device_num_cu() * wgs_per_cu;
  return (unsigned)(g > gmax ? gmax : g);
}

int launch_jlw_setup(const JlwConsts& c, uint32_t* cst, hipStream_t s) {
  hipLaunchKernelGGL(jlw_setup_kernel, dim3(1), dim3(256), 0, s, c, cst);
  return check_launch("jlw_setup_kernel");
}

int launch_jlw_exp(const uint32_t* Hin, const uint32_t* pt, int neg_pt, uint64_t n_ct, const uint32_t* cst,
                   uint32_t* out, uint32_t* stats, hipStream_t s) {
  const dim3 grid(jlw_grid(n_ct, FBM_JW_WGS_PER_CU)), block(FBM_JW_BLOCK);
  if (pt) {
    hipLaunchKernelGGL(jlw_encrypt_kernel, grid, block, 0, s, Hin, pt, neg_pt, n_ct, (const JlwConsts*)cst, out, stats);
    return check_launch("jlw_encrypt_kernel");
  }
  hipLaunchKernelGGL(jlw_factor_kernel, grid, block, 0, s, Hin, n_ct, (const JlwConsts*)cst, out, stats);
  return check_launch("jlw_factor_kernel");
}

int launch_jlw_combine(const uint32_t* cts, int n_parties, uint64_t n_ct, const uint32_t* factor, const uint32_t* cst,
                       uint32_t* xout, hipStream_t s) {
  hipLaunchKernelGGL(jlw_combine_kernel, dim3(jlw_grid(n_ct, 8)), dim3(FBM_JW_BLOCK), 0, s, cts, n_parties, n_ct, factor,
                     (const JlwConsts*)cst, xout);
  return check_launch("jlw_combine_kernel");
}

}  // namespace fbm

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
#include "fbm_wire.hpp"

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

// ---- the encrypt from a factor computed ahead, and the streaming product ----
// lane j <- lane j - 16 of a 64-bit value (lanes 0..15: lane j + 48's, dropped by the caller)
__device__ __forceinline__ uint64_t jw_from16(uint64_t v, int lane) {
  const int src = (lane - 16) & 63;
  return ((uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)v, src);
}

// N p as an integer, for p < 2^1024 (its digits in lanes 0..15, zeros above) and N < 2^2048 (n: lanes 0..31, zeros
// above): jw_mullo's scan by the 32 words of p, without a modulus, kept whole.  Row i retires word i of the product
// (into lane i / 2); what the accumulators hold after the last row are the words 32 and up, so they move up by 16
// lanes.  N p < 2^3072: nothing reaches digit 48.
__device__ __forceinline__ uint64_t jw_npt(uint64_t n, uint64_t p, int lane) {
  const uint32_t n0 = (uint32_t)n, n1 = (uint32_t)(n >> 32), p0 = (uint32_t)p, p1 = (uint32_t)(p >> 32);
  uint64_t U0 = 0, U1 = 0, x = 0;
#pragma unroll 2
  for (int i = 0; i < 16; ++i) {
#pragma unroll
    for (int hw = 0; hw < 2; ++hw) {
      const uint32_t bi = jw_lane(hw ? p1 : p0, i);
      U0 += (uint64_t)n0 * bi;
      U1 += (uint64_t)n1 * bi;
      const uint32_t w = jw_first((uint32_t)U0), u0 = (uint32_t)U0;
      if (lane == i) x |= (uint64_t)w << (32 * hw);
      U0 = (U0 >> 32) + (uint32_t)U1;
      U1 = (U1 >> 32) + jw_up32(u0);
    }
  }
  const jw_u128 s = (jw_u128)U0 + ((jw_u128)U1 << 32);  // words 32 + 2 j and up, of lane j
  const uint64_t L = jw_from16((uint64_t)s, lane), H = jw_from16((uint64_t)(s >> 64), lane);
  uint32_t ov;
  return jw_resolve(lane < 16 ? x : L, lane < 16 ? 0ull : H, lane, ov);
}

// out[k] = (1 + N pt_k) F_k mod M from the factor rows F (any value below 2^4096; jlw_factor_kernel's H(t_k)^key):
// bit for bit jlw_encrypt_kernel's ciphertext, at two products.  N >= 2^1024 > |pt| gives 1 + N |pt| <= M - N + 1:
// the last factor G needs no reduction, so it is formed by jw_npt's 32 plain rows; a negative plaintext takes
// jw_exp_body's signed pass.  No key, no table.
__global__ void __launch_bounds__(FBM_JW_BLOCK)
    jlw_seal_kernel(const uint32_t* __restrict__ pt, int neg_pt, uint64_t n_ct, const uint32_t* __restrict__ factor,
                    const JlwConsts* __restrict__ c, uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const JwMod k = jw_mod(c, lane);
  const uint64_t n = jw_digit_lo(c->N, lane);
#pragma unroll 1
  for (uint64_t ct = (uint64_t)blockIdx.x * FBM_JW_WAVES + wv; ct < n_ct; ct += (uint64_t)gridDim.x * FBM_JW_WAVES) {
    const uint64_t f = jw_digit(factor + ct * 128, lane);  // (under way behind G's rows)
    const uint64_t np = jw_npt(n, lane < 16 ? jw_digit(pt + ct * 32, lane) : 0ull, lane);
    uint64_t g;
    uint32_t ov;
    if (neg_pt && __ballot(np != 0) != 0) {
      const jw_u128 s = (jw_u128)k.m + ~np + (lane == 0 ? 2u : 0u);  // M - N |pt| + 1
      g = jw_resolve((uint64_t)s, (uint64_t)(s >> 64), lane, ov);
    } else {
      const jw_u128 s = (jw_u128)np + (lane == 0 ? 1u : 0u);
      g = jw_resolve((uint64_t)s, (uint64_t)(s >> 64), lane, ov);
    }
    reinterpret_cast<uint64_t*>(out + ct * 128)[lane] = jw_mm(jw_mm(f, k.r2, k, lane), g, k, lane);
  }
}

// acc[k] <- (seed ? 1 : acc[k]) prod_j rows[j][k] mod M in place, rows [n_rows][n_ct][128] of any values below
// 2^4096: two products a row (the row to Montgomery form, then into the accumulator), so acc is the plain canonical
// product after every call.  A lane reads its digit of the next row before the current row's products run.
__global__ void __launch_bounds__(FBM_JW_BLOCK)
    jlw_fold_kernel(uint32_t* __restrict__ acc, const uint32_t* __restrict__ rows, int n_rows, uint64_t n_ct, int seed,
                    const JlwConsts* __restrict__ c) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const JwMod k = jw_mod(c, lane);
#pragma unroll 1
  for (uint64_t ct = (uint64_t)blockIdx.x * FBM_JW_WAVES + wv; ct < n_ct; ct += (uint64_t)gridDim.x * FBM_JW_WAVES) {
    uint64_t next = jw_digit(rows + ct * 128, lane);
    uint64_t a = seed ? (lane == 0 ? 1ull : 0ull) : jw_digit(acc + ct * 128, lane);
#pragma unroll 1
    for (int j = 0; j < n_rows; ++j) {
      const uint64_t row = next;
      if (j + 1 < n_rows) next = jw_digit(rows + ((uint64_t)(j + 1) * n_ct + ct) * 128, lane);
      a = jw_mm(a, jw_mm(row, k.r2, k, lane), k, lane);
    }
    reinterpret_cast<uint64_t*>(acc + ct * 128)[lane] = a;
  }
}

// jlw_fold_kernel with its rows read straight from a stock peer's message ("wide items"): acc[i] <-
// (seed ? 1 : acc[i]) item_i mod M, item i the big-endian bytes the table word ckpt[i] names (fbm_wire.hpp:
// wire_jlw_load / wire_jlw_digit; one item per wave, lane j its digit j).  The [n][128] rows are never written.
// A wave holds the next item's three raw dwords a lane across the current item's two products, as jlw_fold_kernel
// holds its next row; the table word goes through the scalar unit (the wave's item is uniform), so the item's place,
// length and shift cost no vector register.  Bounds: wire_jlw_item_of admits a table word only with its bytes inside
// [span, span + span_len); wire_jlw_load reads a dword whole only where all four bytes lie inside, bytewise (inside
// only) otherwise, and nothing for a digit above the value; ckpt and acc are read and written at i < n_items only.
__device__ __forceinline__ uint64_t jw_uniform64(uint64_t v) {
  return ((uint64_t)jw_first((uint32_t)(v >> 32)) << 32) | jw_first((uint32_t)v);
}
__global__ void __launch_bounds__(FBM_JW_BLOCK)
    jlw_wire_fold_kernel(const uint8_t* __restrict__ span, uint64_t span_len, uint64_t base,
                         const uint64_t* __restrict__ ckpt, uint64_t n_items, uint32_t* __restrict__ acc, int seed,
                         const JlwConsts* __restrict__ c) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const JwMod k = jw_mod(c, lane);
  const uint64_t stride = (uint64_t)gridDim.x * FBM_JW_WAVES;
  uint64_t i = (uint64_t)blockIdx.x * FBM_JW_WAVES + wv;
  if (i >= n_items) return;
  wire_jlw_item next = wire_jlw_item_of(jw_uniform64(ckpt[i]), base, span_len);
  uint32_t d[3];
  wire_jlw_load(span, span_len, next, lane, d);
#pragma unroll 1
  for (; i < n_items; i += stride) {
    const wire_jlw_item it = next;
    uint64_t a = seed ? (lane == 0 ? 1ull : 0ull) : jw_digit(acc + i * 128, lane);
    const uint64_t row = wire_jlw_digit(d, wire_jlw_shift(span, it), it, lane);
    if (i + stride < n_items) {
      next = wire_jlw_item_of(jw_uniform64(ckpt[i + stride]), base, span_len);
      wire_jlw_load(span, span_len, next, lane, d);
    }
    a = jw_mm(a, jw_mm(row, k.r2, k, lane), k, lane);
    reinterpret_cast<uint64_t*>(acc + i * 128)[lane] = a;
  }
}

// ---- the group engine: four lanes per ciphertext, 16 ciphertexts per wave64, for large launches ----
// A residue is 152 limbs of 27 bits, R' = 2^4104 >= 2^8 M: a Montgomery product of two values below 2 M (+ 1) is
// below 2 M again, so nothing is subtracted between products; one compare-and-subtract ends a ciphertext.
//   * lane l of a group (l = lane & 3) owns limbs 38 l .. 38 l + 37 of the running value a, of M, and of the
//     window of 38 accumulator slots; one 64-bit accumulator per slot takes a_j b_i and m_j q_i alike;
//   * b lives in the group's LDS block (b_i is one word for the group's four lanes); q_i is formed in the
//     group's lane 0 and broadcast by DPP quad_perm:[0,0,0,0];
//   * a row retires slot 0 of every lane: its low 27 bits become the top slot of the lane below
//     (quad_perm:[1,2,3,3], the top lane takes 0), the rest is added into the lane's own next slot.  The window
//     shift is register renaming: 38 rows are unrolled (slot r of row i is acc[(r + i) % 38]), run four times;
//   * limbs are lazy between products: below 2^27 + 2^11 (jg_mul's closing carry pass), so a product is below
//     2^54.001 and a slot, 2 products a row over its 38 rows in a lane plus one carry below 2^35, below 2^61.
// Bases (FDH, the gcd, a negative key's inverse) stay on the wave layout: jlw_base_kernel writes the canonical base
// into the output row, jlw_group_kernel raises it to |key| in place.  Exponent: fixed windows of FBM_JG_WIN bits;
// the powers 1 .. 2^WIN - 1 (and the encrypt's last factor) in the call's workspace, one block per resident wave,
// [entry][limb][lane] so that a wave's loads coalesce.
#define FBM_JG_BITS 27
#define FBM_JG_MASK ((1u << FBM_JG_BITS) - 1u)
#define FBM_JG_NL 152   // limbs of a residue
#define FBM_JG_PER 38   // limbs (and accumulator slots) per lane
#define FBM_JG_STRIDE 153  // LDS words per ciphertext: odd, so the 16 groups' b_i fall into distinct banks
#define FBM_JG_CT_PER_WAVE 16
#define FBM_JG_CT_PER_WG (FBM_JG_CT_PER_WAVE * FBM_JW_WAVES)
#ifndef FBM_JG_WIN
#define FBM_JG_WIN 4
#endif
#define FBM_JG_TABLE ((1 << FBM_JG_WIN) - 1)
#define FBM_JG_ENTRY_WORDS (FBM_JG_PER * 64)  // one table entry of a wave's 16 ciphertexts
#define FBM_JG_WAVE_WORDS ((FBM_JG_TABLE + 1) * FBM_JG_ENTRY_WORDS)  // + the row that keeps the last factor

__device__ __forceinline__ uint32_t jg_lane0(uint32_t v) {  // the group's lane 0 to all four
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x00 /* quad_perm:[0,0,0,0] */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t jg_above(uint32_t v) {  // lane l <- lane l + 1 (the top lane: its own, masked by the caller)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xF9 /* quad_perm:[1,2,3,3] */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t jg_below(uint32_t v) {  // lane l <- lane l - 1 (lane 0: its own, masked by the caller)
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x90 /* quad_perm:[0,0,1,2] */, 0xF, 0xF, false);
}
// what one lane wrote to the group's LDS block is read by the other three (one wave: program order on the LDS)
__device__ __forceinline__ void jg_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// limb k (27 bits) of the little-endian words w[0 .. nw)
__device__ __forceinline__ uint32_t jg_limb(const uint32_t* w, int k, int nw) {
  const int bit = FBM_JG_BITS * k, wi = bit >> 5;
  uint64_t v = wi < nw ? w[wi] : 0u;
  if (wi + 1 < nw) v |= (uint64_t)w[wi + 1] << 32;
  return (uint32_t)(v >> (bit & 31)) & FBM_JG_MASK;
}

struct JgLane {
  uint32_t m[FBM_JG_PER];  // this lane's limbs of M
  uint32_t mp;             // -M^-1 mod 2^27
  uint32_t keep_above, keep_below;  // all ones, or zero in the group's top / bottom lane
};

// rows R .. 37 of a block of 38: slot s of row R is acc[(s + R) % 38], every index a constant (a template recursion
// rather than a loop: the unroller's size bound refuses 38 rows)
template <int R>
__device__ __forceinline__ void jg_rows(uint64_t (&acc)[FBM_JG_PER], const uint32_t (&a)[FBM_JG_PER], const uint32_t* bo,
                                        const JgLane& k) {
  if constexpr (R < FBM_JG_PER) {
    const uint32_t b = bo[R];
    acc[R] += (uint64_t)a[0] * b;
    const uint32_t q = jg_lane0(((uint32_t)acc[R] * k.mp) & FBM_JG_MASK);
#pragma unroll
    for (int s = 1; s < FBM_JG_PER; ++s) acc[(s + R) % FBM_JG_PER] += (uint64_t)a[s] * b;
#pragma unroll
    for (int s = 0; s < FBM_JG_PER; ++s) acc[(s + R) % FBM_JG_PER] += (uint64_t)k.m[s] * q;
    const uint64_t t = acc[R];  // slot 0 retires (lane 0: its low 27 bits are zero)
    acc[(R + 1) % FBM_JG_PER] += t >> FBM_JG_BITS;
    acc[R] = jg_above((uint32_t)t & FBM_JG_MASK) & k.keep_above;
    jg_rows<R + 1>(acc, a, bo, k);
  }
}

// a <- a b 2^-4104 mod M (any representative below 2 M for a b < 2 M (2 M + 1)); b: the group's LDS block
__device__ __forceinline__ void jg_mul(uint32_t (&a)[FBM_JG_PER], const uint32_t* bl, const JgLane& k) {
  uint64_t acc[FBM_JG_PER];
#pragma unroll
  for (int s = 0; s < FBM_JG_PER; ++s) acc[s] = 0;
#pragma unroll 1
  for (int o = 0; o < FBM_JG_NL / FBM_JG_PER; ++o) {
    // the limbs pass through an empty asm in every block (fbm_mont.hpp's laundering): hoisted out of the loop, their
    // zero-extensions to 64 bits would each hold a register pair across the product, and spill
    JgLane kl = k;
#pragma unroll
    for (int s = 0; s < FBM_JG_PER; ++s) {
      asm volatile("" : "+v"(a[s]));
      asm volatile("" : "+v"(kl.m[s]));
    }
    jg_rows<0>(acc, a, bl + o * FBM_JG_PER, kl);
  }
  // back to limbs: the lane's own carries, then the carry out of the lane below into limbs 0 and 1 (the top
  // lane's own carry out is zero: the value is below 2^4104)
  uint64_t c = 0;
#pragma unroll
  for (int s = 0; s < FBM_JG_PER; ++s) {
    const uint64_t t = acc[s] + c;
    a[s] = (uint32_t)t & FBM_JG_MASK;
    c = t >> FBM_JG_BITS;
  }
  const uint64_t cin = ((uint64_t)(jg_below((uint32_t)(c >> 32)) & k.keep_below) << 32) |
                       (jg_below((uint32_t)c) & k.keep_below);
  const uint64_t t = a[0] + cin;
  a[0] = (uint32_t)t & FBM_JG_MASK;
  a[1] += (uint32_t)(t >> FBM_JG_BITS);
}

__device__ __forceinline__ void jg_put(uint32_t* bl, int l, const uint32_t (&a)[FBM_JG_PER]) {
#pragma unroll
  for (int s = 0; s < FBM_JG_PER; ++s) bl[FBM_JG_PER * l + s] = a[s];
}
__device__ __forceinline__ void jg_words(uint32_t (&a)[FBM_JG_PER], const uint32_t* w, int nw, int l) {
#pragma unroll
  for (int s = 0; s < FBM_JG_PER; ++s) a[s] = w ? jg_limb(w, FBM_JG_PER * l + s, nw) : 0u;
}

// one lane, on a group's LDS block of lazy limbs: the value (below 2 M) to the canonical limbs of its residue
__device__ __forceinline__ void jg_canonical(uint32_t* bl, const uint32_t* M) {
  uint32_t c = 0;
  for (int i = 0; i < FBM_JG_NL; ++i) {
    const uint32_t t = bl[i] + c;
    bl[i] = t & FBM_JG_MASK;
    c = t >> FBM_JG_BITS;
  }
  bool ge = true;
  for (int i = FBM_JG_NL - 1; i >= 0; --i) {
    const uint32_t mi = jg_limb(M, i, 128);
    if (bl[i] != mi) {
      ge = bl[i] > mi;
      break;
    }
  }
  if (!ge) return;
  uint32_t bw = 0;
  for (int i = 0; i < FBM_JG_NL; ++i) {
    const uint32_t t = bl[i] - jg_limb(M, i, 128) - bw;
    bl[i] = t & FBM_JG_MASK;
    bw = t >> 31;
  }
}
// one lane: x (lazy limbs, below 2 M) to the limbs of 2 M - x + 1 (a negative plaintext's 1 - N |pt|)
__device__ __forceinline__ void jg_negate_plus1(uint32_t* bl, const uint32_t* M) {
  int64_t c = 1;
  for (int i = 0; i < FBM_JG_NL; ++i) {
    const int64_t t = 2 * (int64_t)jg_limb(M, i, 128) - (int64_t)bl[i] + c;
    bl[i] = (uint32_t)t & FBM_JG_MASK;
    c = t >> FBM_JG_BITS;
  }
}

__device__ __forceinline__ uint32_t jg_window(const uint32_t* kw, int w) {
  const int bit = FBM_JG_WIN * w, wi = bit >> 5;
  uint64_t v = kw[wi];
  if (wi + 1 < 128) v |= (uint64_t)kw[wi + 1] << 32;
  return (uint32_t)(v >> (bit & 31)) & ((1u << FBM_JG_WIN) - 1u);
}

// the canonical base of every ciphertext into its output row, on the wave layout: H(t_k), or the row of Hin reduced
// mod M; its inverse for a negative non-zero key (none: flagged, a zero row)
__global__ void __launch_bounds__(FBM_JW_BLOCK, FBM_JW_WGS_PER_CU)
    jlw_base_kernel(const uint32_t* __restrict__ Hin, uint64_t n_ct, const JlwConsts* __restrict__ c,
                    uint32_t* __restrict__ out, uint32_t* __restrict__ stats) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const JwMod k = jw_mod(c, lane);
  const uint64_t unit = lane == 0 ? 1u : 0u;
  uint32_t err = 0;
#pragma unroll 1
  for (uint64_t ct = (uint64_t)blockIdx.x * FBM_JW_WAVES + wv; ct < n_ct; ct += (uint64_t)gridDim.x * FBM_JW_WAVES) {
    const uint64_t h = Hin ? jw_digit(Hin + ct * 128, lane) : jw_fdh(c, ct + c->ct_offset, lane, err);
    uint64_t v = jw_mm(jw_mm(h, k.r2, k, lane), unit, k, lane);  // h mod M
    if (c->key_negative && c->key_bits) {
      uint64_t gi;
      if (jw_inverse(v, k, lane, gi, err)) {
        v = jw_mm(gi, unit, k, lane);
      } else {
        err |= FBM_ERR_NOT_INVERTIBLE;
        v = 0;
      }
    }
    reinterpret_cast<uint64_t*>(out + ct * 128)[lane] = v;
  }
  if (err && lane == 0) atomicOr(stats + FBM_STAT_ERRFLAGS, err);
}

// out[k] <- out[k]^|key| (N pt_k + 1, or 1) mod M over the base rows jlw_base_kernel left.  tbl: FBM_JG_WAVE_WORDS
// words per wave of the grid.
__global__ void __launch_bounds__(FBM_JW_BLOCK, FBM_JW_WGS_PER_CU)
    jlw_group_kernel(const uint32_t* __restrict__ pt, int neg_pt, uint64_t n_ct, const JlwConsts* __restrict__ c,
                     uint32_t* __restrict__ out, uint32_t* __restrict__ tbl_g) {
  __shared__ uint32_t b_s[FBM_JW_WAVES * FBM_JG_CT_PER_WAVE * FBM_JG_STRIDE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l = lane & 3;
  uint32_t* bl = b_s + (wv * FBM_JG_CT_PER_WAVE + (lane >> 2)) * FBM_JG_STRIDE;
  uint32_t* tbl = tbl_g + ((uint64_t)blockIdx.x * FBM_JW_WAVES + wv) * FBM_JG_WAVE_WORDS + lane;
  JgLane k;
  jg_words(k.m, c->M, 128, l);
  k.mp = c->mp & FBM_JG_MASK;
  k.keep_above = l == 3 ? 0u : ~0u;
  k.keep_below = l == 0 ? 0u : ~0u;
  const int kbits = c->key_bits;
  uint32_t a[FBM_JG_PER];
#pragma unroll 1
  for (uint64_t ct0 = ((uint64_t)blockIdx.x * FBM_JW_WAVES + wv) * FBM_JG_CT_PER_WAVE; ct0 < n_ct;
       ct0 += (uint64_t)gridDim.x * FBM_JG_CT_PER_WG) {
    const uint64_t ct = ct0 + (lane >> 2);
    const bool live = ct < n_ct;
    if (pt) {  // the last factor N |pt| + 1 (negative: 2 M - N |pt| + 1) into the table block's spare row
      jg_words(a, c->R2g, 128, l);
      jg_put(bl, l, a);
      jg_sync();
      jg_words(a, c->N, 64, l);
#pragma unroll 1
      for (int e = 0; e < 2; ++e) {  // N R' = N R'^2 / R', then N |pt| = |pt| (N R') / R'
        if (e) {
          jg_put(bl, l, a);
          jg_sync();
          jg_words(a, live ? pt + ct * 32 : nullptr, 32, l);
        }
        jg_mul(a, bl, k);
      }
      if (neg_pt) {
        jg_put(bl, l, a);
        jg_sync();
        if (l == 0) jg_negate_plus1(bl, c->M);
        jg_sync();
#pragma unroll
        for (int s = 0; s < FBM_JG_PER; ++s) a[s] = bl[FBM_JG_PER * l + s];
      } else if (l == 0) {
        a[0] += 1u;
      }
#pragma unroll
      for (int s = 0; s < FBM_JG_PER; ++s) tbl[FBM_JG_TABLE * FBM_JG_ENTRY_WORDS + s * 64] = a[s];
    }
    // g R' and its powers: the table's entry t is g^(t + 1) R'.  A zero key: the base is 1, the power its entry 0.
    jg_words(a, c->R2g, 128, l);
    jg_put(bl, l, a);
    jg_sync();
    jg_words(a, live && kbits ? out + ct * 128 : nullptr, 128, l);
    if (!kbits && l == 0) a[0] = 1u;
    const int nt = kbits ? FBM_JG_TABLE : 1;
#pragma unroll 1
    for (int t = 0; t < nt; ++t) {
      jg_mul(a, bl, k);
#pragma unroll
      for (int s = 0; s < FBM_JG_PER; ++s) tbl[t * FBM_JG_ENTRY_WORDS + s * 64] = a[s];
      if (t == 0) {
        jg_sync();
        jg_put(bl, l, a);
        jg_sync();
      }
    }
    int w = kbits ? (kbits - 1) / FBM_JG_WIN : 0;
    const uint32_t top = kbits ? jw_first(jg_window(c->key, w)) : 1u;  // (it holds the key's top bit)
#pragma unroll
    for (int s = 0; s < FBM_JG_PER; ++s) a[s] = tbl[(top - 1u) * FBM_JG_ENTRY_WORDS + s * 64];
#pragma unroll 1
    for (--w; w >= 0; --w) {
      const uint32_t d = jw_first(jg_window(c->key, w));
      const int np = FBM_JG_WIN + (d ? 1 : 0);
#pragma unroll 1
      for (int p = 0; p < np; ++p) {  // WIN squares, then the window's product: a is the table entry, b the value
        jg_sync();
        jg_put(bl, l, a);
        jg_sync();
        if (p == FBM_JG_WIN) {
#pragma unroll
          for (int s = 0; s < FBM_JG_PER; ++s) a[s] = tbl[(d - 1u) * FBM_JG_ENTRY_WORDS + s * 64];
        }
        jg_mul(a, bl, k);
      }
    }
    // times the last factor (out of Montgomery form), to the residue, to 32-bit words
    jg_sync();
    if (pt) {
#pragma unroll
      for (int s = 0; s < FBM_JG_PER; ++s) bl[FBM_JG_PER * l + s] = tbl[FBM_JG_TABLE * FBM_JG_ENTRY_WORDS + s * 64];
    } else {
#pragma unroll
      for (int s = 0; s < FBM_JG_PER; ++s) bl[FBM_JG_PER * l + s] = (l == 0 && s == 0) ? 1u : 0u;
    }
    jg_sync();
    jg_mul(a, bl, k);
    jg_sync();
    jg_put(bl, l, a);
    jg_sync();
    if (l == 0) jg_canonical(bl, c->M);
    jg_sync();
    if (live) {
#pragma unroll 4
      for (int j = 0; j < 32; ++j) {
        const int wd = 4 * j + l, bit = 32 * wd, k0 = bit / FBM_JG_BITS;
        uint64_t v = bl[k0] | ((uint64_t)bl[k0 + 1] << FBM_JG_BITS);
        if (k0 + 2 < FBM_JG_NL) v |= (uint64_t)bl[k0 + 2] << (2 * FBM_JG_BITS);
        out[ct * 128 + wd] = (uint32_t)(v >> (bit - FBM_JG_BITS * k0));
      }
    }
    jg_sync();
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

// Engine choice: the wave engine is the latency of a small launch, the group engine the throughput of
// a large one.  FBM_JLW_GROUP_MIN_CT is the measured crossover (profiles/jl_wide_group_sweep.jsonl).  The policy is per
// thread, as the narrow engines'; the product library never sets it.
#define FBM_JLW_GROUP_MIN_CT 8192u
static thread_local int t_jlw_engine = FBM_JLW_ENGINE_AUTO;

int jlw_engine_set(int mode) {
  const int prev = t_jlw_engine;
  t_jlw_engine = mode;
  return prev;
}

int jlw_engine_for(uint64_t n_ct) {
  if (t_jlw_engine != FBM_JLW_ENGINE_AUTO) return t_jlw_engine;
  return n_ct >= FBM_JLW_GROUP_MIN_CT ? FBM_JLW_ENGINE_GROUP : FBM_JLW_ENGINE_WAVE;
}

static unsigned jlw_group_grid(uint64_t n_ct) {
  uint64_t g = (n_ct + FBM_JG_CT_PER_WG - 1) / FBM_JG_CT_PER_WG;
  const uint64_t gmax = (uint64_t)device_num_cu() * FBM_JW_WGS_PER_CU;
  return (unsigned)(g > gmax ? gmax : g);
}

// the group engine's table of powers: one block per wave of the grid, so by min(n_ct, the resident slots)
uint64_t jlw_table_bytes(uint64_t n_ct) {
  if (n_ct == 0 || jlw_engine_for(n_ct) != FBM_JLW_ENGINE_GROUP) return 0;
  return (uint64_t)jlw_group_grid(n_ct) * FBM_JW_WAVES * FBM_JG_WAVE_WORDS * sizeof(uint32_t);
}

int launch_jlw_exp(const uint32_t* Hin, const uint32_t* pt, int neg_pt, uint64_t n_ct, const uint32_t* cst,
                   uint32_t* out, uint32_t* stats, hipStream_t s) {
  const dim3 grid(jlw_grid(n_ct, FBM_JW_WGS_PER_CU)), block(FBM_JW_BLOCK);
  if (jlw_engine_for(n_ct) == FBM_JLW_ENGINE_GROUP) {  // the table lies behind the constants and the n_ct plaintext rows
    uint32_t* tbl = (uint32_t*)((char*)cst + FBM_JLW_CST_BYTES) + n_ct * 32;
    hipLaunchKernelGGL(jlw_base_kernel, grid, block, 0, s, Hin, n_ct, (const JlwConsts*)cst, out, stats);
    const int rc = check_launch("jlw_base_kernel");
    if (rc) return rc;
    hipLaunchKernelGGL(jlw_group_kernel, dim3(jlw_group_grid(n_ct)), block, 0, s, pt, neg_pt, n_ct, (const JlwConsts*)cst,
                       out, tbl);
    return check_launch("jlw_group_kernel");
  }
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

int launch_jlw_seal(const uint32_t* pt, int neg_pt, uint64_t n_ct, const uint32_t* factor, const uint32_t* cst,
                    uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(jlw_seal_kernel, dim3(jlw_grid(n_ct, 8)), dim3(FBM_JW_BLOCK), 0, s, pt, neg_pt, n_ct, factor,
                     (const JlwConsts*)cst, out);
  return check_launch("jlw_seal_kernel");
}

int launch_jlw_fold(uint32_t* acc, const uint32_t* rows, int k, uint64_t n_ct, bool seed, const uint32_t* cst,
                    hipStream_t s) {
  hipLaunchKernelGGL(jlw_fold_kernel, dim3(jlw_grid(n_ct, 8)), dim3(FBM_JW_BLOCK), 0, s, acc, rows, k, n_ct, seed ? 1 : 0,
                     (const JlwConsts*)cst);
  return check_launch("jlw_fold_kernel");
}

int launch_jlw_wire_fold(const uint8_t* span, uint64_t span_len, uint64_t base, const uint64_t* ckpt, uint64_t n,
                         uint32_t* acc, bool seed, const uint32_t* cst, hipStream_t s) {
  hipLaunchKernelGGL(jlw_wire_fold_kernel, dim3(jlw_grid(n, 8)), dim3(FBM_JW_BLOCK), 0, s, span, span_len, base, ckpt, n,
                     acc, seed ? 1 : 0, (const JlwConsts*)cst);
  return check_launch("jlw_wire_fold_kernel");
}

}  // namespace fbm

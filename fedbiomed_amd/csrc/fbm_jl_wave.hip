// fedbiomed_amd -- the Joye-Libert exponentiation on the WAVE engine (FBM_ENGINE_WAVE): one ciphertext
// per wave64, for launches that hold fewer ciphertexts than the chip has SIMDs to spare.
//
// The throughput engines (fbm_jl.hip) give a ciphertext 1, 3 or 4 lanes, so a product's dependent chain is
// thousands of multiply-adds long and a launch never costs less than one such chain, however small it is.
// Here a product is spread over the whole wave:
//   * residues are plain Montgomery residues modulo M = N^2 with R = 2^2048, canonical (< M) between
//     products; lane j owns word j (32 bits) of the running value, of the operand and of M;
//   * the product is scanned by the rows of B: row i's word b_i is wave-uniform, read with v_readlane
//     into an SGPR; every lane runs v_mad_u64_u32 (a_j b_i, then m_j q_i) into a carry-save accumulator
//     of 64 bits and a carry word (the assembly body WV_ROW; the 32-row C++ form wv_rows, used once per
//     N-adic output, keeps two 64-bit accumulators and lane 0's carry as a scalar instead);
//   * the quotient digit q_i = lo(acc_0) * (-M^-1) mod 2^32 is formed on the scalar unit from lane 0's
//     word (readfirstlane);
//   * the retiring word goes one lane down by DPP (wave_shl:1): X_j <- hi X_j + lo X_{j+1};
//   * carries are resolved once per product: generate / propagate masks by __ballot, one 64-bit scalar
//     add, for T and for T + 2^2048 - M at once (the conditional subtraction picks by the latter's carry).
// Exponent: the launch-uniform sliding-window schedule the other engines use (JlSched: width FBM_WIN,
// odd powers), the wave's table of FBM_TABLE odd powers in LDS (64 words each, lane j reads its own
// word).  The short path is NOT taken: every launch runs the window table, so the
// short-path switch cannot change a bit.  Edges (h, nude, the N-adic digits) convert in plain C++.
// No global table space, no scratch; constants come from the call's constants block (28-bit limbs).
#include "fbm_internal.hpp"
#include "fbm_quad_asm.hpp"

namespace fbm {

#define FBM_WV_WAVES 4  // waves (ciphertexts) per workgroup
#define FBM_WV_BLOCK (64 * FBM_WV_WAVES)
// resident workgroups per CU = waves per SIMD: a lone wave issues one instruction per slot and leaves the
// SIMD's other slots idle, a second one fills part of them (6.4 ms for two against 4.5 for one); more would
// only stretch each chain, which is what a latency engine is for
#define FBM_WV_WGS_PER_CU 2

// lane j <- lane j + 1 (lane 63 <- 0) / lane j <- lane j - 1 (lane 0 <- 0)
__device__ __forceinline__ uint32_t wv_lane_up(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t wv_lane_down(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t wv_first(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint32_t wv_lane(uint32_t v, int i) { return (uint32_t)__builtin_amdgcn_readlane((int)v, i); }

// sum_j s_j 2^(32 j) -> its words (lane j: word j) and what lies at or above 2^2048 (ovf)
__device__ __forceinline__ uint32_t wv_resolve(uint64_t s, int lane, uint32_t& ovf) {
  const uint32_t c = (uint32_t)(s >> 32);
  const uint64_t t = (uint64_t)(uint32_t)s + wv_lane_down(c);
  const uint64_t G = __ballot((t >> 32) != 0), P = __ballot((uint32_t)t == 0xFFFFFFFFu);
  // a word takes a carry in when the word below generates one or propagates its own: the adder's chain
  const uint64_t g = G << 1, S = P + g, cin = S ^ P;
  ovf = wv_lane(c, 63) + (uint32_t)(G >> 63) + (S < P ? 1u : 0u);
  return (uint32_t)t + (uint32_t)((cin >> lane) & 1ull);
}

// ROWS rows of the scan on (U, V, K): the first ROWS words of b; q != nullptr: lane i keeps row i's digit
template <int ROWS>
__device__ __forceinline__ void wv_rows(uint64_t& U, uint64_t& V, uint32_t& K, uint32_t a, uint32_t b, uint32_t m,
                                        uint32_t m0, uint32_t mp, int lane, uint32_t* q) {
#pragma unroll 8
  for (int i = 0; i < ROWS; ++i) {
    const uint32_t bi = wv_lane(b, i);
    const uint32_t sv = wv_first((uint32_t)V);
    U += (uint64_t)a * bi;
    const uint32_t su = wv_first((uint32_t)U);
    const uint32_t qi = (su + sv + K) * mp;
    V += (uint64_t)m * qi;
    // lane 0's retired words: lo U_0 + lo V_0 + K = 0 (mod 2^32), its carry stays at word 0
    const uint32_t sv2 = sv + qi * m0;
    K = (uint32_t)(((uint64_t)su + sv2 + K) >> 32);
    if (q && lane == i) *q = qi;
    U = (U >> 32) + wv_lane_up((uint32_t)U);
    V = (V >> 32) + wv_lane_up((uint32_t)V);
  }
}

// a b 2^-2048 mod the odd modulus m (lane j: word j; m0 = word 0, mp = -m^-1 mod 2^32), canonical,
// for a b <= m 2^2048
// The 64 rows are one assembly body on fixed registers: a wave alone on its SIMD issues one instruction
// per slot, scalar or vector, so a row's cost is its instruction count -- ten here.  One accumulator of
// three words per lane, v[120:121] and the carry word v122: both products of a row go into it with
// v_mad_u64_u32's carry out, so the retired word of lane 0 is exactly zero and no carry is tracked
// beside it.  s80 = b_i (read a row ahead: the v_readlane is also the second wait state the DPP read of
// v120 needs after the multiply-add), s81 = q_i.
#define WV_ROW(nx)                                                                                \
  "v_mad_u64_u32 v[120:121], vcc, %[a], s80, v[120:121]\n"                                         \
  "v_addc_co_u32 v122, vcc, 0, v122, vcc\n"                                                        \
  "v_readfirstlane_b32 s81, v120\n"                                                                \
  "s_mul_i32 s81, s81, %[mp]\n"                                                                    \
  "v_mad_u64_u32 v[120:121], vcc, %[m], s81, v[120:121]\n"                                         \
  "v_addc_co_u32 v122, vcc, 0, v122, vcc\n"                                                        \
  "v_readlane_b32 s80, %[b], " #nx "\n"                                                            \
  "v_add_co_u32_dpp v120, vcc, v120, v121 wave_shl:1 row_mask:0xf bank_mask:0xf bound_ctrl:0\n"    \
  "v_addc_co_u32 v121, vcc, 0, v122, vcc\n"                                                        \
  "v_mov_b32 v122, 0\n"
#define WV_ROW8(a, b, c, d, e, f, g, h) WV_ROW(a) WV_ROW(b) WV_ROW(c) WV_ROW(d) WV_ROW(e) WV_ROW(f) WV_ROW(g) WV_ROW(h)

__device__ __forceinline__ uint32_t wv_mul(uint32_t a, uint32_t b, uint32_t m, uint32_t m0, uint32_t mp, int lane) {
  uint32_t lo, hi;
  asm("v_mov_b32 v120, 0\n"
      "v_mov_b32 v121, 0\n"
      "v_mov_b32 v122, 0\n"
      "v_readlane_b32 s80, %[b], 0\n"  //
      WV_ROW8(1, 2, 3, 4, 5, 6, 7, 8) WV_ROW8(9, 10, 11, 12, 13, 14, 15, 16)
      WV_ROW8(17, 18, 19, 20, 21, 22, 23, 24) WV_ROW8(25, 26, 27, 28, 29, 30, 31, 32)
      WV_ROW8(33, 34, 35, 36, 37, 38, 39, 40) WV_ROW8(41, 42, 43, 44, 45, 46, 47, 48)
      WV_ROW8(49, 50, 51, 52, 53, 54, 55, 56) WV_ROW8(57, 58, 59, 60, 61, 62, 63, 0)
      "v_mov_b32 %[lo], v120\n"
      "v_mov_b32 %[hi], v121\n"
      : [lo] "=&v"(lo), [hi] "=&v"(hi)
      : [a] "v"(a), [b] "v"(b), [m] "v"(m), [mp] "s"(mp)
      : "v120", "v121", "v122", "s80", "s81", "vcc");
  (void)m0;
  const uint64_t sT = ((uint64_t)hi << 32) | lo;  // (hi <= 3 after the last row's shift)
  const uint64_t sD = sT + (uint32_t)~m + (lane == 0 ? 1u : 0u);  // T + 2^2048 - m
  uint32_t ovT, ovD;
  const uint32_t wT = wv_resolve(sT, lane, ovT);
  const uint32_t wD = wv_resolve(sD, lane, ovD);
  return ovD ? wD : wT;
}

// word j of a number held as nl limbs of lb bits in global memory (limb k at p[k * stride])
__device__ __forceinline__ uint32_t wv_word(const uint32_t* p, int nl, int lb, int stride, int j) {
  const int bit = 32 * j, k = bit / lb, sh = bit % lb;
  uint64_t v = 0;
  if (k < nl) v |= (uint64_t)p[k * stride] >> sh;
  if (k + 1 < nl) v |= (uint64_t)p[(k + 1) * stride] << (lb - sh);
  if (k + 2 < nl) v |= (uint64_t)p[(k + 2) * stride] << (2 * lb - sh);
  return (uint32_t)v;
}

__device__ __forceinline__ uint32_t wv_neg_inv32(uint32_t m0) {  // -m0^-1 mod 2^32, m0 odd
  uint32_t x = m0;
#pragma unroll
  for (int i = 0; i < 5; ++i) x *= 2u - m0 * x;
  return 0u - x;
}

// jl_exp_kernel's contract (fbm_jl.hip): mode 0 out = nude H^key, FBM_EXP_DEC out = H^key (mod N^2),
// | FBM_EXP_OUT_NADIC the digits (v mod N | v div N) instead; `ops` the schedule's device copy.  Waves
// past n_ct (the last chunk) redo the last ciphertext and store nothing.
__global__ void __launch_bounds__(FBM_WV_BLOCK, FBM_WV_WGS_PER_CU)
    jl_expw_kernel(const uint32_t* __restrict__ H, uint64_t n_ct, uint32_t* __restrict__ cst,
                   const uint32_t* __restrict__ ops, int n_ops, int first, int mode, int key_is_zero,
                   const uint32_t* __restrict__ nude, uint32_t* __restrict__ out, const uint32_t* __restrict__ Hc) {
  __shared__ uint32_t tbl_s[FBM_WV_WAVES * FBM_TABLE * 64];
  __shared__ uint32_t chunk_s;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t* tbl = tbl_s + wv * (FBM_TABLE * 64) + lane;
  // M = N^2 and N (zero-extended), word per lane, and their Montgomery constants
  const uint32_t m = wv_word(cst + FBM_CST_M, FBM_NL, FBM_LB, 1, lane);
  const uint32_t nn = wv_word(cst + FBM_CST_MN, FBM_NLN, FBM_LB, 1, lane);
  const uint32_t m0 = wv_first(m), n0 = wv_first(nn);
  const uint32_t mp = wv_neg_inv32(m0), np = wv_neg_inv32(n0);
  // the block's R'^2 have R' = 2^2072 (M) and 2^1036 (N): one product by a power of two makes them 2^4096 mod M
  // and 2^2048 mod N
  const uint32_t r2 = wv_mul(wv_word(cst + FBM_CST_R2, FBM_NL, FBM_LB, 1, lane), lane == 62 ? 1u << 16 : 0u, m, m0,
                             mp, lane);
  const uint32_t nr = wv_mul(nn, r2, m, m0, mp, lane);  // N R mod M
  const uint32_t cn = wv_mul(wv_word(cst + FBM_CST_MN + FBM_NLN, FBM_NLN, FBM_LB, 1, lane), lane == 63 ? 1u << 8 : 0u,
                             nn, n0, np, lane);
  const uint32_t n_chunks = (uint32_t)((n_ct + FBM_WV_WAVES - 1) / FBM_WV_WAVES);
#pragma unroll 1
  for (;;) {
    if (tid == 0) chunk_s = atomicAdd(cst + FBM_CST_CTR, 1u);
    __syncthreads();
    const uint32_t chunk = wv_first(chunk_s);
    __syncthreads();
    if (chunk >= n_chunks) break;
    const uint64_t ct_raw = (uint64_t)chunk * FBM_WV_WAVES + wv;
    const bool valid = ct_raw < n_ct;
    const uint64_t ct = valid ? ct_raw : n_ct - 1;
    uint32_t h;
    if (key_is_zero) {
      h = lane == 0 ? 1u : 0u;
    } else {
      // the compact row (8 words) unless it holds the sentinel (or there is none): the whole row
      bool full = true;
      uint32_t c = 0;
      if (Hc) {
        c = lane < 8 ? Hc[ct * 8 + lane] : ~0u;
        full = __ballot(c != ~0u) == 0;
      }
      h = full ? H[ct * 64 + lane] : lane < 8 ? c : 0u;
    }
    uint32_t acc = wv_mul(h, r2, m, m0, mp, lane);  // h R
    if (!key_is_zero) {
      tbl[0] = acc;
      const uint32_t x2 = wv_mul(acc, acc, m, m0, mp, lane);
#pragma unroll 1
      for (int t = 1; t < FBM_TABLE; ++t) {
        acc = wv_mul(acc, x2, m, m0, mp, lane);
        tbl[t * 64] = acc;
      }
      acc = tbl[first * 64];
#pragma unroll 1
      for (int k = 0; k < n_ops; ++k) {
        const uint32_t op = wv_first(ops[k]);
        const int nsq = (int)(op >> FBM_OP_SHIFT);
        const int idx = (int)(op & ((1u << FBM_OP_SHIFT) - 1u)) - 1;
#pragma unroll 1
        for (int q = 0; q < nsq; ++q) acc = wv_mul(acc, acc, m, m0, mp, lane);
        if (idx >= 0) acc = wv_mul(acc, tbl[idx * 64], m, m0, mp, lane);
      }
    }
    uint32_t last = lane == 0 ? 1u : 0u;
    if ((mode & FBM_EXP_DEC) == 0) {  // x nude = N pt + 1 (jl_nude_kernel's 29-bit rows of pt < 2^1044)
      const uint32_t* nb = nude + (ct >> 8) * (FBM_NUDE_ROWS * 256) + (ct & 255) + FBM_NUDE_D1 * 256;
      const uint32_t npt = wv_mul(wv_word(nb, FBM_QA_L, FBM_QA_LB, 256, lane), nr, m, m0, mp, lane);
      uint32_t ov;
      last = wv_resolve((uint64_t)npt + last, lane, ov);
    }
    const uint32_t v = wv_mul(acc, last, m, m0, mp, lane);
    if (!(mode & FBM_EXP_OUT_NADIC)) {
      if (valid) out[ct * 64 + lane] = v;
      continue;
    }
    // v = d0 + d1 N: d0 = v mod N (a product modulo N by 2^2048 mod N); E = v - d0 = d1 N, and 32 rows of the
    // reduction modulo N on E give Q with E + Q N = 0 (mod 2^1024): d1 = -Q mod 2^1024
    const uint32_t d0 = wv_mul(v, cn, nn, n0, np, lane);
    uint32_t ov;
    const uint32_t e = wv_resolve((uint64_t)v + (uint32_t)~d0 + (lane == 0 ? 1u : 0u), lane, ov);
    uint64_t U = 0, V = e;
    uint32_t K = 0, q = 0;
    wv_rows<32>(U, V, K, 0u, 0u, nn, n0, np, lane, &q);
    const uint32_t d1 = wv_resolve(lane < 32 ? (uint64_t)(uint32_t)~q + (lane == 0 ? 1u : 0u) : 0ull, lane, ov);
    if (valid && lane < 32) {
      out[ct * 64 + lane] = d0;
      out[ct * 64 + 32 + lane] = d1;
    }
  }
}

uint64_t wave_resident_ct() { return (uint64_t)device_num_cu() * FBM_WV_WGS_PER_CU * FBM_WV_WAVES; }

int launch_jl_expw(const uint32_t* H, uint64_t n_ct, const JlSched& sc, int mode, int key_is_zero,
                   const uint32_t* nude, const uint32_t* ops, const uint32_t* cst, uint32_t* out, hipStream_t s,
                   const uint32_t* Hc) {
  uint64_t g = (n_ct + FBM_WV_WAVES - 1) / FBM_WV_WAVES;
  const uint64_t gmax = (uint64_t)device_num_cu() * FBM_WV_WGS_PER_CU;
  if (g > gmax) g = gmax;
  hipLaunchKernelGGL(jl_expw_kernel, dim3((unsigned)g), dim3(FBM_WV_BLOCK), 0, s, H, n_ct, (uint32_t*)cst, ops, sc.n_ops,
                     sc.first, mode, key_is_zero, nude, out, Hc);
  return check_launch("jl_expw_kernel");
}

}  // namespace fbm

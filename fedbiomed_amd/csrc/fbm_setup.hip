// fedbiomed_amd -- the C ABI's host setup: the per-modulus and per-key constants the kernels take
// (Montgomery / N-adic / lane-group constants, the generic engine's GenCtx, FDH's message blocks and
// midstate, the sliding-window schedules, the short path's and the split exponentiation's constants)
// and the four bounded caches that keep them between calls.  Nothing here runs on the GPU or depends
// on FBM_TEST_HOOKS: compiled once and linked into both libraries, like the kernel objects.  The big
// integers are fbm_bigint.hpp's.
#include <string.h>

#include <mutex>

#include "fbm_bigint.hpp"
#include "fbm_internal.hpp"
#include "fbm_nadic_asm.hpp"
#include "fbm_quad_asm.hpp"

namespace fbm {

void wipe(void* p, size_t n) {  // a zeroing the optimiser keeps
  volatile uint8_t* v = (volatile uint8_t*)p;
  while (n--) *v++ = 0;
}

// ---------------------------------------------------------------------------------------
// the caches: at most CAP entries found by their leading `key` words, oldest evicted first (WIPE:
// zeroed when evicted or cleared), all under one mutex
// ---------------------------------------------------------------------------------------
static std::mutex g_cache_mu;

template <class E, size_t CAP, bool WIPE>
struct BoundedCache {
  std::vector<E> v;  // oldest first

  bool find(const uint32_t* key, E& out, bool to_back = false) {  // to_back: a hit becomes the newest
    std::lock_guard<std::mutex> lk(g_cache_mu);
    for (size_t i = 0; i < v.size(); ++i)
      if (memcmp(v[i].key, key, sizeof(v[i].key)) == 0) {
        out = v[i];
        if (to_back) {
          v.erase(v.begin() + i);
          v.push_back(out);
        }
        return true;
      }
    return false;
  }
  void insert(const E& e) {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (v.size() >= CAP) {
      if (WIPE) wipe(&v.front(), sizeof(E));
      v.erase(v.begin());
    }
    v.push_back(e);
  }
  void clear() {
    std::lock_guard<std::mutex> lk(g_cache_mu);
    if (WIPE)
      for (E& e : v) wipe(&e, sizeof(E));
    v.clear();
  }
};

// The modulus-dependent part of JlParams, per biprime (a round's encrypts and aggregate, and every
// round of an experiment, share one biprime); most recently used last
struct JlParamsCacheEntry {
  uint32_t key[32];  // N
  JlParams jp;
};
static BoundedCache<JlParamsCacheEntry, 8, false> g_jp_cache;

// R^(P+1) mod N^2 in 28-bit limbs (the ciphertext product's first operand), per (N, P)
struct JlRkCacheEntry {
  uint32_t key[33];  // N, then P
  JlRk rk;
};
static BoundedCache<JlRkCacheEntry, 16, false> g_rk_cache;

// The short path's constant C per (N, |key|), cached so a round's repeated calls skip the ~2 050
// host squarings.  An entry holds no key material: it is found by a SHA-256 digest of (N, |key|)
// and holds only C (a public function of the key, like the ciphertexts it is used for); entries
// are zeroed when evicted or cleared (fbm_jl_clear_caches).  The reference keeps nothing between
// calls (a fresh SecaggCrypter per call: fedbiomed/node/secagg/_secagg_round.py:142).
struct JlShortCacheEntry {
  uint32_t key[8];  // SHA-256(N's 32 words || |key|'s 64 words, little-endian bytes)
  uint32_t corr[72];
};
static BoundedCache<JlShortCacheEntry, 32, true> g_short_cache;

// The split exponentiation's constants per (N, |key|) (JlShort: c1, cp, one), cached beside C under the same
// digest and on the same terms: public functions of the key, zeroed when evicted or cleared.
struct JlSplitCacheEntry {
  uint32_t key[8];
  uint32_t c1[36];
  uint32_t cp[72];
  uint32_t one[72];
};
static BoundedCache<JlSplitCacheEntry, 32, true> g_split_cache;

void setup_clear_caches() {
  g_short_cache.clear();  // the only ones derived from a key (zeroed)
  g_split_cache.clear();
  g_jp_cache.clear();  // per-N public parameters
  g_rk_cache.clear();
}

int short_cache_dump(uint32_t* out, int cap_words) {
  std::lock_guard<std::mutex> lk(g_cache_mu);
  const int need = (int)(g_short_cache.v.size() * sizeof(JlShortCacheEntry) / 4);
  if (out && cap_words >= need && need) memcpy(out, g_short_cache.v.data(), (size_t)need * 4);
  return need;
}

// ---------------------------------------------------------------------------------------
// per-modulus constants
// ---------------------------------------------------------------------------------------
template <int NL>
static void build_mont(const Big& m, MontCtxT<NL>& c) {  // m odd >= 3
  to_limbs(m, c.M, NL, FBM_LB);
  to_limbs(pow2_mod(2 * NL * FBM_LB, m), c.R2, NL, FBM_LB);
  c.mp = neg_inv<uint32_t>(m[0]) & FBM_LMASK;
}

// v as the digit pair (v mod N, v div N) in the N-adic engines' 29-bit limbs
static void digit_pair(const Big& v, const Big& N, uint32_t* dst) {
  Big q, r;
  big_divmod(v, N, q, r);
  to_limbs(r, dst, FBM_QA_L, FBM_QA_LB);
  to_limbs(q, dst + FBM_QA_L, FBM_QA_L, FBM_QA_LB);
}

// Constants of the quad engine (tools/gen_quad_asm.py): 29-bit limbs, R = 2^(36*29) = 2^1044.  N odd >= 3, M = N^2.
static void build_quad(const Big& N, const Big& M, QuadCtx& qa) {
  memset(&qa, 0, sizeof(qa));
  const int LB = FBM_QA_LB, L = FBM_QA_L;
  Big Rm = pow2_mod(L * LB, N);  // R mod N
  Big K(N.size() + 1, 0u);
  K[0] = 1u;
  if (big_cmp(Rm, K) > 0) {  // K = N + 1 - Rm
    Big t(N.begin(), N.end());
    t.push_back(0u);
    uint64_t c = 1;
    for (size_t k = 0; k < t.size(); ++k) {
      c += t[k];
      t[k] = (uint32_t)c;
      c >>= 32;
    }
    big_sub_inplace(t, Rm);
    K = t;
  } else {
    K.assign(1, 0u);
  }
  uint32_t k29[FBM_QA_L];
  to_limbs(K, k29, L, LB);
  for (int j = 0; j < L; ++j) qa.kp[j] = ((1u << LB) - 1u) + k29[j];
  {  // the one-lane square's initial s window: 2^29 - 1 + P'_j, P' = (K - E) mod N (fbm_nadic_asm.hpp)
    Big E(40, 0u);
    for (int c = 0; c < 64; ++c)
      if ((FBM_NA_SQ_ONE_MASK >> c) & 1ull) {
        const int bit = 32 + LB * c;
        E[bit >> 5] |= 1u << (bit & 31);
      }
    Big q, r;
    big_divmod(E, N, q, r);  // E mod N
    Big P(K.begin(), K.end());
    P.resize(N.size() + 1, 0u);
    if (big_cmp(P, r) < 0) {  // P' = K - r (+ N)
      uint64_t c = 0;
      for (size_t k = 0; k < P.size(); ++k) {
        c += (uint64_t)P[k] + (k < N.size() ? N[k] : 0u);
        P[k] = (uint32_t)c;
        c >>= 32;
      }
    }
    big_sub_inplace(P, r);
    uint32_t p29[FBM_QA_L];
    to_limbs(P, p29, L, LB);
    for (int j = 0; j < L; ++j) qa.sqp[j] = ((1u << LB) - 1u) + p29[j];
  }
  to_limbs(N, qa.n, L, LB);
  digit_pair(pow2_mod(2 * L * LB, M), N, qa.r2);
  digit_pair(pow2_mod(3 * L * LB, M), N, qa.r3);
  qa.np = neg_inv<uint32_t>(N[0]) & ((1u << LB) - 1u);
}

// Constants of the one-lane N-adic engine (tools/gen_nadic_asm.py): the group engines' 29-bit
// N and K'_i (the same R = 2^1044) in the layout of its scalar loads, and N's 28-bit limbs
// for the final step shared by all N-adic engines (na_final_digits).
static void build_nadic(const MontCtxN& mn, const QuadCtx& qa, NadicCtx& na) {
  static_assert(FBM_NA_LIMBS == FBM_QA_L && FBM_NA_LIMB_BITS == FBM_QA_LB, "one R for all N-adic engines");
  memset(&na, 0, sizeof(na));
  for (int j = 0; j < FBM_NLN; ++j) na.nk[j < 10 ? j : 6 + j] = mn.M[j];
  for (int j = 0; j < FBM_QA_L; ++j) na.nk29[j < 10 ? j : 6 + j] = qa.n[j];
  for (int j = 0; j < FBM_QA_L; ++j) na.nk29[42 + j] = qa.kp[j];
}

// SHA-256 midstate over the 14 leading blocks of t.to_bytes(1024,'big') (FDH.H), t = (k << 512) | tau:
// bytes 0..895 = t's bits 1024..8191 = tau's words 32..255 (k < 2^64 never reaches them).  Block b's
// SHA word j is t's little-endian word 255 - 16 b - j.  All-zero for a round below 2^1024.
static void fdh_midstate(uint32_t mid[8], const uint32_t* tau = nullptr) {
  static uint32_t zero_mid[8];
  static std::once_flag once;
  std::call_once(once, [] {
    uint32_t st[8], W[16];
    fbm_sha256_init(st);
    memset(W, 0, sizeof(W));
    for (int b = 0; b < 14; ++b) fbm_sha256_compress(st, W);
    memcpy(zero_mid, st, sizeof(st));
  });
  bool hi = false;
  for (int i = 32; tau && i < FBM_TAU_LIMBS; ++i) hi |= tau[i] != 0u;
  if (!hi) {
    memcpy(mid, zero_mid, sizeof(zero_mid));
    return;
  }
  uint32_t st[8], W[16];
  fbm_sha256_init(st);
  for (int b = 0; b < 14; ++b) {
    for (int j = 0; j < 16; ++j) W[j] = tau[255 - 16 * b - j];
    fbm_sha256_compress(st, W);
  }
  memcpy(mid, st, sizeof(st));
}

// the round tau (FBM_TAU_LIMBS little-endian words, < 2^8192) -> FDH's message blocks: block 15 = tau's
// words 0..15, block 14 = words 16..31 (the kernel ORs k into its last two words), blocks 0..13 into the
// midstate -- t.to_bytes(1024, 'big') of t = (k << 512) | tau (_jls.py:451-467, 744-748) for any round
static void set_tau(JlParams& jp, const uint32_t* tau) {
  for (int i = 0; i < 16; ++i) jp.tau_w[i] = tau ? tau[15 - i] : 0u;
  for (int i = 0; i < 16; ++i) jp.tau14_w[i] = tau ? tau[31 - i] : 0u;
  fdh_midstate(jp.mid, tau);
}

int fdh_params(const uint32_t* n_odd, int even, const uint32_t* tau, uint64_t ct_offset, JlParams& jp) {
  if (!(n_odd[0] & 1u)) {
    set_error("FDH: the gcd modulus' odd part must be odd");
    return FBM_E_ARG;
  }
  memset(&jp, 0, sizeof(jp));
  for (int i = 0; i < 32; ++i) jp.N32[i] = n_odd[i];
  jp.fdh_even = even ? 1 : 0;
  set_tau(jp, tau);
  jp.ct_offset = ct_offset;
  return FBM_OK;
}

int fdh_params_for_biprime(const uint32_t* biprime, const uint32_t* tau, uint64_t ct_offset, JlParams& jp) {
  Big N(biprime, biprime + 32);
  const int s = big_ctz(N);
  Big m = big_shr(N, s);
  m.resize(32, 0u);
  return fdh_params(m.data(), s > 0, tau, ct_offset, jp);
}

void fdh_wide_consts(const uint32_t* modulus_odd, uint32_t k1[32], uint32_t k2[32], uint32_t& mp) {
  const Big m(modulus_odd, modulus_odd + 32);  // odd (the caller checked); 1 for a power-of-two modulus
  Big a = pow2_mod(1024 + 256, m), b = pow2_mod(2048, m);
  a.resize(32, 0u);
  b.resize(32, 0u);
  memcpy(k1, a.data(), 32 * 4);
  memcpy(k2, b.data(), 32 * 4);
  mp = neg_inv<uint32_t>(m[0]);
}

// M = N^2, Barrett constants of M and N, M = 2^e m2 with m2 odd, m2^-1 mod 2^e.  The only builder that takes
// an even N: divisions, products and shifts only, nothing of Montgomery's.
int build_gen_ctx(const uint32_t* biprime, const uint32_t* key, int key_negative, GenCtx& g) {
  memset(&g, 0, sizeof(g));
  Big N(biprime, biprime + 32);
  big_trim(N);
  if (big_bits(N) < 1) {
    set_error("biprime must be >= 1");
    return FBM_E_UNSUPPORTED;
  }
  Big M = big_mul(N, N);
  big_trim(M);
  auto mu = [](const Big& m) {  // floor(2^(64 k) / m), k = words of m
    Big a(2 * m.size() + 1, 0u), q, r;
    a.back() = 1u;
    big_divmod(a, m, q, r);
    big_trim(q);
    return q;
  };
  const Big muM = mu(M), muN = mu(N);
  g.kM = (int)M.size();
  g.kN = (int)N.size();
  for (size_t i = 0; i < M.size(); ++i) g.M[i] = M[i];
  for (size_t i = 0; i < muM.size() && i < 68; ++i) g.muM[i] = muM[i];
  for (size_t i = 0; i < N.size(); ++i) g.N[i] = N[i];
  for (size_t i = 0; i < muN.size() && i < 36; ++i) g.muN[i] = muN[i];
  const int s = big_ctz(N);
  const Big m = big_shr(N, s);
  Big m2 = big_mul(m, m);
  big_trim(m2);
  g.km2 = (int)m2.size();
  g.e = 2 * s;
  for (size_t i = 0; i < m2.size(); ++i) g.m2[i] = m2[i];
  if (g.e > 0) {
    const Big y = inv_mod_pow2(m2, g.e);
    for (size_t i = 0; i < y.size(); ++i) g.m2inv[i] = y[i];
  }
  if (key) {
    Big K(key, key + 64);
    g.key_bits = big_bits(K);
    for (int i = 0; i < 64; ++i) g.key[i] = key[i];
    g.key_negative = key_negative ? 1 : 0;
  }
  return FBM_OK;
}

static int ves_checks(int es, int cr) {
  if (es < 1 || cr < 1 || es > 100 || (int64_t)es * cr > 1024) {
    set_error("invalid VES parameters es=%d cr=%d", es, cr);
    return FBM_E_ARG;
  }
  return FBM_OK;
}

// The modulus-dependent part of JlParams (Montgomery / N-adic / group-engine constants, N^-1
// mod 2^1024, the FDH midstate): host big-integer work per call, so it is built once per biprime
// and kept in g_jp_cache.
static int build_jl_params_uncached(const uint32_t* biprime, int es, int cr, const uint32_t* tau, uint64_t ct_offset,
                                    JlParams& jp) {
  memset(&jp, 0, sizeof(jp));
  Big N(biprime, biprime + 32);
  const int nb = big_bits(N);
  if (nb < 2 || (N[0] & 1u) == 0u) {  // an even N takes the generic engine before this (jl_generic)
    set_error("biprime must be >= 2 (the Montgomery engines take an odd N >= 3); got %d bits, %s", nb,
              (N[0] & 1u) ? "odd" : "even");
    return FBM_E_UNSUPPORTED;
  }
  int rc = ves_checks(es, cr);
  if (rc) return rc;
  Big M = big_mul(N, N);  // 64 limbs
  while (M.size() > 64) M.pop_back();
  build_mont<FBM_NL>(M, jp.mc);
  build_mont<FBM_NLN>(N, jp.mn);
  build_quad(N, M, jp.qa);
  build_nadic(jp.mn, jp.qa, jp.na);
  for (int i = 0; i < 32; ++i) jp.N32[i] = biprime[i];
  memcpy(jp.Ninv32, inv_mod_pow2(N, 1024).data(), sizeof(jp.Ninv32));
  jp.n_bits = nb;
  {  // M = N << (1036 - nb): 0 mod N, in [2^1035, 2^1036) (negative-weight nude digit)
    Big m(N.begin(), N.end());
    m.resize(34, 0u);
    for (int i = FBM_NLN * FBM_LB - nb; i > 0; --i) shl1(m.data(), m.size());
    to_limbs(m, jp.mneg, FBM_NLN, FBM_LB);
  }
  fbm_n30_setup(jp.N32, jp.n30);
  jp.es = es;
  jp.cr = cr;
  set_tau(jp, tau);
  jp.ct_offset = ct_offset;
  return FBM_OK;
}

int build_jl_params(const uint32_t* biprime, int es, int cr, const uint32_t* tau, uint64_t ct_offset, JlParams& jp) {
  int rc = ves_checks(es, cr);
  if (rc) return rc;
  JlParamsCacheEntry e;
  if (g_jp_cache.find(biprime, e, true)) {
    jp = e.jp;
    jp.es = es;
    jp.cr = cr;
    set_tau(jp, tau);
    jp.ct_offset = ct_offset;
    jp.key_is_zero = 0;
    return FBM_OK;
  }
  if ((rc = build_jl_params_uncached(biprime, es, cr, tau, ct_offset, jp))) return rc;
  memcpy(e.key, biprime, sizeof(e.key));
  e.jp = jp;
  g_jp_cache.insert(e);
  return FBM_OK;
}

void jl_rk_for(const uint32_t* n32, int n_parties, JlRk& r) {  // n32: an odd N >= 3 (build_jl_params took it)
  uint32_t key[33];
  memcpy(key, n32, 32 * 4);
  key[32] = (uint32_t)n_parties;
  JlRkCacheEntry e;
  if (g_rk_cache.find(key, e)) {
    r = e.rk;
    return;
  }
  Big M(n32, n32 + 32);
  M = big_mul(M, M);
  const Big rk = pow2_mod((uint64_t)(n_parties + 1) * FBM_NL * FBM_LB, M);
  memset(&r, 0, sizeof(r));
  to_limbs(rk, r.w, FBM_NL, FBM_LB);
  memcpy(e.key, key, sizeof(e.key));
  e.rk = r;
  g_rk_cache.insert(e);
}

// ---------------------------------------------------------------------------------------
// per-key schedules and constants
// ---------------------------------------------------------------------------------------
// Left-to-right sliding window of `width` bits over K, odd-power table: op = squarings << FBM_OP_SHIFT |
// (table index + 1), squarings past FBM_OP_MAXSQ as multiply-free ops before it.  first != nullptr: the
// leading window is the accumulator's start, its table index goes to *first; nullptr: an op like the others
// (from the accumulator 1).  split_tail: trailing squarings past FBM_OP_MAXSQ are split like the others,
// else refused.  n counts the ops as they are written; false where they would pass FBM_MAX_OPS.
static bool sliding_window(const Big& K, int width, int* first, bool split_tail, uint16_t* op, int& n) {
  auto bit = [&](int i) -> int { return (K[i >> 5] >> (i & 31)) & 1; };
  auto emit = [&](int nsq, int idx1) {  // idx1: table index + 1, 0 = squarings only
    for (; nsq > FBM_OP_MAXSQ; nsq -= FBM_OP_MAXSQ) {
      if (n >= FBM_MAX_OPS) return false;
      op[n++] = (uint16_t)(FBM_OP_MAXSQ << FBM_OP_SHIFT);
    }
    if (n >= FBM_MAX_OPS) return false;
    op[n++] = (uint16_t)((nsq << FBM_OP_SHIFT) | idx1);
    return true;
  };
  int pending = 0;
  bool lead = first != nullptr;
  for (int i = big_bits(K) - 1; i >= 0;) {
    if (!bit(i)) {
      ++pending;
      --i;
      continue;
    }
    int l = i - width + 1;
    if (l < 0) l = 0;
    while (!bit(l)) ++l;
    int val = 0;
    for (int j = i; j >= l; --j) val = (val << 1) | bit(j);
    if (lead)
      *first = (val - 1) / 2;
    else if (!emit(pending + i - l + 1, (val - 1) / 2 + 1))
      return false;
    lead = false;
    pending = 0;
    i = l - 1;
  }
  if (pending > FBM_OP_MAXSQ && !split_tail) return false;
  for (; pending > 0; pending -= FBM_OP_MAXSQ)
    if (!emit(pending > FBM_OP_MAXSQ ? FBM_OP_MAXSQ : pending, 0)) return false;
  return true;
}

int build_schedule(const uint32_t* key, JlSched& sc, int& is_zero) {
  memset(&sc, 0, sizeof(sc));
  sc.sbits = sc.sb1 = -1;  // (build_short)
  Big K(key, key + 64);
  is_zero = big_bits(K) == 0;
  const bool ok = is_zero || sliding_window(K, FBM_WIN, &sc.first, true, sc.op, sc.n_ops);
  wipe(K.data(), K.size() * 4);
  return ok ? FBM_OK : FBM_E_ARG;
}

// SHA-256 of a little-endian word message (host; the FDH kernel's compression function)
static void sha256_words(const uint32_t* w, int nw, uint32_t out[8]) {
  uint32_t st[8], W[16];
  fbm_sha256_init(st);
  const uint64_t nbytes = (uint64_t)nw * 4;
  const int nblocks = (int)((nbytes + 9 + 63) / 64);
  auto byte_at = [&](uint64_t i) -> uint32_t {
    if (i < nbytes) return (w[i / 4] >> (8 * (i % 4))) & 0xffu;  // little-endian words
    if (i == nbytes) return 0x80u;
    const uint64_t tail = (uint64_t)nblocks * 64 - i;  // the 8-byte big-endian bit length
    if (tail <= 8) return (uint32_t)(((nbytes * 8) >> (8 * (tail - 1))) & 0xffu);
    return 0u;
  };
  for (int b = 0; b < nblocks; ++b) {
    for (int j = 0; j < 16; ++j) {
      const uint64_t i = (uint64_t)b * 64 + 4 * j;
      W[j] = (byte_at(i) << 24) | (byte_at(i + 1) << 16) | (byte_at(i + 2) << 8) | byte_at(i + 3);
    }
    fbm_sha256_compress(st, W);
  }
  memcpy(out, st, sizeof(st));
  wipe(W, sizeof(W));
}

// E = L (2^s + 1) + 261 (e - 2^s), L = 1044, s = bit length of e - 1: a binary chain over e (squares that
// drop R, short products that drop 2^261) leaves h^e 2^-(E - 2L), so 2^E = 2^f R^2 brings it to h^e R
static Big chain_exponent(const Big& K) {
  const int KSB = FBM_QA_LB * FBM_NA_SHORT_LIMBS;  // 261
  const int s = big_bits(K) - 1;
  Big v(K.begin(), K.end());
  v.resize(64, 0u);
  v[s >> 5] &= ~(1u << (s & 31));
  Big E(66, 0u);
  uint64_t c = 0;
  for (int i = 0; i < 64; ++i) {  // 261 v
    c += (uint64_t)v[i] * (uint64_t)KSB;
    E[i] = (uint32_t)c;
    c >>= 32;
  }
  E[64] = (uint32_t)c;
  auto add_at = [&](uint64_t val, int bit) {  // E += val << bit
    const int w = bit >> 5, sh2 = bit & 31;
    unsigned __int128 add = (unsigned __int128)val << sh2;
    uint64_t cy = 0;
    for (int i = w; i < (int)E.size(); ++i) {
      const uint64_t t = (uint64_t)E[i] + (uint64_t)(uint32_t)add + cy;
      E[i] = (uint32_t)t;
      cy = t >> 32;
      add >>= 32;
      if (!add && !cy) break;
    }
  };
  const int Lb = FBM_QA_L * FBM_QA_LB;  // 1044
  add_at((uint64_t)Lb, s);
  add_at((uint64_t)Lb, 0);
  wipe(v.data(), v.size() * 4);
  return E;
}

// The split exponentiation's half of JlShort / JlSched (fbm_internal.hpp) for a key with |key| >= N on the
// short path's domain (N odd, > 2^262); keys below N leave sc.sb1 = -1 (the unsplit chain).  dg: the digest
// of (N, |key|).
static void build_split(const Big& N, const uint32_t* key, const uint32_t dg[8], JlSched& sc, JlShort& sh) {
  Big K(key, key + 64);
  if (big_cmp(K, N) < 0) return;
  Big k1, k0;
  big_divmod(K, N, k1, k0);
  k1.resize(64, 0u);
  k0.resize(32, 0u);
  int n_nops = 0;
  // N's schedule (width FBM_WIN_N) from the accumulator 1: every window, the leading one included, is an op
  if (sliding_window(N, FBM_WIN_N, nullptr, false, sh.nop, n_nops)) {
    memcpy(sh.k1w, k1.data(), sizeof(sh.k1w));
    memcpy(sh.k0w, k0.data(), sizeof(sh.k0w));
    JlSplitCacheEntry e;
    if (g_split_cache.find(dg, e)) {
      memcpy(sh.c1, e.c1, sizeof(sh.c1));
      memcpy(sh.cp, e.cp, sizeof(sh.cp));
      memcpy(sh.one, e.one, sizeof(sh.one));
    } else {
      Big M = big_mul(N, N);
      Big E1 = chain_exponent(k1);  // C1 = 2^f1 R^2 mod N
      to_limbs(pow2_mod(E1, N), sh.c1, FBM_QA_L, FBM_QA_LB);
      Big Ep(34, 0u);  // C' = 2^(261 k0 + 1044) mod N^2
      uint64_t c = (uint64_t)(FBM_QA_L * FBM_QA_LB);
      for (int i = 0; i < 32; ++i) {
        c += (uint64_t)k0[i] * (uint64_t)(FBM_QA_LB * FBM_NA_SHORT_LIMBS);
        Ep[i] = (uint32_t)c;
        c >>= 32;
      }
      Ep[32] = (uint32_t)c;
      digit_pair(pow2_mod(Ep, M), N, sh.cp);
      digit_pair(pow2_mod(FBM_QA_L * FBM_QA_LB, M), N, sh.one);  // the Montgomery one, R mod N^2
      wipe(E1.data(), E1.size() * 4);
      wipe(Ep.data(), Ep.size() * 4);
      memcpy(e.key, dg, sizeof(e.key));
      memcpy(e.c1, sh.c1, sizeof(e.c1));
      memcpy(e.cp, sh.cp, sizeof(e.cp));
      memcpy(e.one, sh.one, sizeof(e.one));
      g_split_cache.insert(e);
    }
    wipe(&e, sizeof(e));
    sc.sb1 = big_bits(k1) - 1;
    sc.n_nops = n_nops;
    sc.nbn = big_bits(N);
  }
  wipe(K.data(), K.size() * 4);
  wipe(k1.data(), k1.size() * 4);
  wipe(k0.data(), k0.size() * 4);
}

bool build_short(const uint32_t* biprime, const uint32_t* key, int is_zero, JlSched& sc, JlShort& sh, bool short_on) {
  memset(&sh, 0, sizeof(sh));
  sc.sbits = sc.sb1 = -1;
  sc.n_nops = sc.nbn = 0;
  if (!short_on) return false;
  Big N(biprime, biprime + 32);
  big_trim(N);
  const int KSB = FBM_QA_LB * FBM_NA_SHORT_LIMBS;  // 261
  if (big_bits(N) < KSB + 2 || !(N[0] & 1u)) return false;
  {  // D = N - 2^261
    Big D(N.begin(), N.end());
    Big p(KSB / 32 + 1, 0u);
    p[KSB / 32] = 1u << (KSB % 32);
    big_sub_inplace(D, p);
    to_limbs(D, sh.d, FBM_QA_L, FBM_QA_LB);
  }
  if (is_zero) return true;
  Big K(key, key + 64);
  for (int i = 0; i < 64; ++i) sh.kw[i] = key[i];
  sc.sbits = big_bits(K) - 1;
  uint32_t dg[8];
  {
    uint32_t msg[96];
    memcpy(msg, biprime, 32 * 4);
    memcpy(msg + 32, key, 64 * 4);
    sha256_words(msg, 96, dg);
    wipe(msg, sizeof(msg));
  }
  build_split(N, key, dg, sc, sh);
  JlShortCacheEntry e;
  if (!g_short_cache.find(dg, e)) {
    // E = L (2^s + 1) + 261 (|key| - 2^s), L = 1044, s = nb - 1: the chain leaves h^|key| 2^-(E - 2L)
    Big E = chain_exponent(K);
    digit_pair(pow2_mod(E, big_mul(N, N)), N, e.corr);
    wipe(E.data(), E.size() * 4);  // (K, E: the key and its exponent -- not kept)
    memcpy(e.key, dg, sizeof(e.key));
    g_short_cache.insert(e);
  }
  memcpy(sh.corr, e.corr, sizeof(sh.corr));
  wipe(K.data(), K.size() * 4);
  wipe(&e, sizeof(e));
  return true;
}

}  // namespace fbm

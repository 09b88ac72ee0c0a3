// fedbiomed_amd -- C ABI (include/fbm_secagg.h): argument validation, call policy (engine and
// path of a call), workspace layouts and kernel launches, and the test build's hooks.  The
// per-modulus and per-key constants the launches take are built in fbm_setup.hip.  All device
// memory belongs to the caller.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "fbm_internal.hpp"
#include "fbm_nadic_asm.hpp"
#include "fbm_quad_asm.hpp"
#include "fbm_tri_asm.hpp"
#include "fbm_safegcd.hpp"
#include "fbm_wire.hpp"
#include "fbm_wire_scan.hpp"
#ifdef FBM_TEST_HOOKS
#include "../../include/fbm_secagg_test.h"
#endif

namespace fbm {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s launch failed: %s", what, hipGetErrorString(e));
    return FBM_E_HIP;
  }
  return FBM_OK;
}

static int zero_stats(uint32_t* stats, hipStream_t s) {
  if (!stats) {
    set_error("stats buffer is required");
    return FBM_E_ARG;
  }
  hipError_t e = hipMemsetAsync(stats, 0, FBM_STATS_WORDS * sizeof(uint32_t), s);
  if (e != hipSuccess) {
    set_error("hipMemsetAsync(stats): %s", hipGetErrorString(e));
    return FBM_E_HIP;
  }
  return FBM_OK;
}

static int quant_params(double clip, double two_clip, double target_f, uint64_t target_m1, QuantParams& qp) {
  if (!(clip > 0.0) || !(two_clip > 0.0) || !(target_f >= 1.0)) {
    set_error("invalid quantisation parameters (clip=%g, target=%g)", clip, target_f);
    return FBM_E_ARG;
  }
  qp.c = clip;
  qp.two_c = two_clip;
  qp.tf = target_f;
  qp.tm1 = target_m1;
  return FBM_OK;
}

// N = 1: the reference computes everything modulo N^2 = 1 (every ciphertext 0) and its decryption's
// invert(delta^2, N^2) raises; only the generic engine's Barrett products take a modulus of 1
static bool jl_is_one(const uint32_t* biprime) {
  if (biprime[0] != 1u) return false;
  for (int i = 1; i < 32; ++i)
    if (biprime[i]) return false;
  return true;
}

// the generic engine (fbm_gen.hip) takes every even N and N = 1, and every N under FBM_ENGINE_GENERIC
static bool jl_generic(const uint32_t* biprime) {
  return (biprime[0] & 1u) == 0u || jl_is_one(biprime) || jl_engine_policy() == FBM_ENGINE_GENERIC;
}

// the short path on (1) or off (0: every wave runs the window-table path) for this thread's calls; only the
// test build's fbm_jl_set_short changes it (include/fbm_secagg_test.h)
static thread_local int t_short_on = 1;

// The path a split call (fbm_jl_encrypt_phase / fbm_jl_decrypt_factor_phase) took at its phase 1
// -- generic or Montgomery engine, short path or not -- keyed by its workspace: the later phases
// read the constants phase 1 wrote, so they follow phase 1's choice even if the process-wide
// switches (the test build's fbm_jl_set_engine, fbm_jl_set_short) changed in between.  A later phase whose record is
// missing (phase 1 never ran on this workspace, or its record was evicted by FBM_PATH_RECS newer
// split calls) is refused with FBM_E_ARG: it would read constants laid out for a path it cannot know.
// fbm_jl_clear_caches leaves the records alone (they hold no key material).
struct JlPathRec {
  const void* ws;
  bool generic, short_on;
};
static constexpr size_t FBM_PATH_RECS = 4096;
static std::mutex g_path_mu;
static std::vector<JlPathRec> g_path_recs;  // most recent last, at most FBM_PATH_RECS

static int jl_path_for(const void* ws, int phase, int full, const uint32_t* biprime, bool& generic, bool& short_on) {
  if (!(phase & 1)) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    for (size_t i = g_path_recs.size(); i-- > 0;)
      if (g_path_recs[i].ws == ws) {
        generic = g_path_recs[i].generic || (biprime[0] & 1u) == 0u || jl_is_one(biprime);
        short_on = g_path_recs[i].short_on;
        return FBM_OK;
      }
    set_error("phase %d of a split call on a workspace with no phase-1 record (run phase 1 on it first)", phase);
    return FBM_E_ARG;
  }
  generic = jl_generic(biprime);
  short_on = t_short_on != 0;
  if (phase != full) {
    std::lock_guard<std::mutex> lk(g_path_mu);
    for (size_t i = 0; i < g_path_recs.size(); ++i)
      if (g_path_recs[i].ws == ws) {
        g_path_recs.erase(g_path_recs.begin() + i);
        break;
      }
    if (g_path_recs.size() >= FBM_PATH_RECS) g_path_recs.erase(g_path_recs.begin());
    g_path_recs.push_back(JlPathRec{ws, generic, short_on});
  }
  return FBM_OK;
}

static uint64_t table_slots_for(uint64_t n_ct) {
  const uint64_t cap = jl_table_slots();
  uint64_t g = ((n_ct + 255) / 256) * 256;
  return g < cap ? g : cap;
}

static uint64_t align256(uint64_t v) { return (v + 255) & ~255ull; }

// ---------------------------------------------------------------------------------------
// optional per-kernel event timer (test build only: fbm_prof_enable / fbm_prof_report,
// include/fbm_secagg_test.h): records a HIP event pair on the launch stream around each kernel
// launch; costs nothing when disabled.  The product library launches directly.
// ---------------------------------------------------------------------------------------
#ifdef FBM_TEST_HOOKS
struct ProfRec {
  const char* name;
  hipEvent_t a, b;
};
static std::mutex g_prof_mu;
static bool g_prof_on = false;
static std::vector<ProfRec> g_prof;
static std::map<std::string, std::pair<long, double>> g_prof_agg;

template <class F>
static int timed(const char* name, hipStream_t s, F f) {
  if (!g_prof_on) return f();
  ProfRec r{name, nullptr, nullptr};
  if (hipEventCreate(&r.a) != hipSuccess) return f();
  if (hipEventCreate(&r.b) != hipSuccess) {
    (void)hipEventDestroy(r.a);
    return f();
  }
  // Drain the stream first: a marker can otherwise complete while the previous kernel is
  // still running, and its interval would absorb that kernel's tail (measured: per-kernel
  // sums 2.3x the wall time).  Profiling mode therefore serialises host and device.
  // A failed drain or marker only loses this timing record, never the launch itself.
  if (hipStreamSynchronize(s) != hipSuccess || hipEventRecord(r.a, s) != hipSuccess) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
    return f();
  }
  const int rc = f();
  if (hipEventRecord(r.b, s) != hipSuccess) {
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
    return rc;
  }
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_prof.push_back(r);
  return rc;
}
#else
template <class F>
static int timed(const char*, hipStream_t, F f) {
  return f();
}
#endif

static void fill_peers(LomPeers& pe, const uint8_t* nonce, uint64_t tau) {
  memset(&pe, 0, sizeof(pe));
  uint32_t iv[4];
  memcpy(iv, nonce, 16);
  pe.ctr0 = (uint64_t)iv[0] | ((uint64_t)iv[1] << 32);
  pe.n14 = iv[2];
  pe.n15 = iv[3];
  pe.tau = tau;
  uint8_t tb[16] = {0};
  for (int b = 0; b < 8; ++b) tb[15 - b] = (uint8_t)(tau >> (8 * b));
  memcpy(pe.tau_be, tb, 16);
}

}  // namespace fbm

using namespace fbm;

extern "C" {

int fbm_abi_version(void) { return FBM_ABI_VERSION; }

void fbm_jl_clear_caches(void) { setup_clear_caches(); }

const char* fbm_last_error(void) { return g_err; }

int fbm_check_stats(const uint32_t* st, int lom_nodes, uint32_t* max_bits_out) {
  if (!st) return FBM_E_ARG;
  if (max_bits_out) *max_bits_out = st[FBM_STAT_MAXBITS];
  const uint32_t f = st[FBM_STAT_ERRFLAGS];
  if (f & FBM_ERR_FDH_OVERFLOW) {
    set_error("FDH: no r of 1..7 digests with gcd(r, N^2) == 1 (reference: OverflowError)");
    return FBM_E_FDH;
  }
  if (f & FBM_ERR_FDH_WIDE) {  // (no kernel reports it since round 5: r of up to 255 digests runs on the device)
    set_error("FDH: r wider than the device path's rows");
    return FBM_E_UNSUPPORTED;
  }
  if (f & FBM_ERR_NOT_INVERTIBLE) {
    set_error("invert() no inverse exists");
    return FBM_E_INVERSE;
  }
  if (f & FBM_ERR_ITER_CAP) {
    set_error("bounded device loop hit its iteration cap");
    return FBM_E_ITER;
  }
  if (f & FBM_ERR_PT_WIDE) {
    set_error("VES: a packed value spills past the 1024-bit plaintext (a value wider than its slot); "
              "outside the device path's domain");
    return FBM_E_UNSUPPORTED;
  }
  if (f & FBM_ERR_DEQUANT_RANGE) {
    set_error("Cannot reverse quantize, received values exceed maximum number");
    return FBM_E_RANGE;
  }
  if (lom_nodes > 0) {
    int node_bits = 0;
    while ((1ll << node_bits) < (long long)lom_nodes) ++node_bits;  // ceil(log2(P))
    if ((int)st[FBM_STAT_MAXBITS] >= 64 - node_bits) {
      set_error("Secure aggregation overflow detected: values need %u bits, %d available", st[FBM_STAT_MAXBITS],
                64 - node_bits);
      return FBM_E_OVERFLOW;
    }
  }
  if (f & FBM_ERR_ROUND_RANGE) {
    set_error("int too big to convert");
    return FBM_E_ROUND;
  }
  return FBM_OK;
}

// the element types that are quantised (inputs) and that an *_as entry point writes (outputs)
static bool float_dtype(int dtype) {
  return dtype == FBM_F32 || dtype == FBM_F64 || dtype == FBM_F16 || dtype == FBM_BF16;
}

static int check_out_dtype(int out_dtype) {
  if (float_dtype(out_dtype)) return FBM_OK;
  set_error("out_dtype=%d must be FBM_F64, FBM_F32, FBM_F16 or FBM_BF16", out_dtype);
  return FBM_E_ARG;
}

int fbm_lom_protect(const void* x, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                    uint64_t target_m1, uint64_t weight, const uint8_t* secrets, const int8_t* signs, int n_peers,
                    int raw_seeds, const uint8_t* nonce, uint64_t tau, uint64_t elem_offset, uint64_t* y,
                    uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  QuantParams qp;
  if ((rc = quant_params(clip, two_clip, target_f, target_m1, qp))) return rc;
  if (!float_dtype(x_dtype) && x_dtype != FBM_U64) {
    set_error("x_dtype must be FBM_F16, FBM_BF16, FBM_F32, FBM_F64 or FBM_U64");
    return FBM_E_ARG;
  }
  if (n_peers < 0) {
    set_error("n_peers=%d < 0", n_peers);
    return FBM_E_ARG;
  }
  if ((n > 0 && ((!x && x_dtype != FBM_U64) || !y)) || !nonce || (n_peers > 0 && (!secrets || !signs))) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  // PRF.eval_vector guard (_lom.py:74-78), on global indices
  if ((elem_offset & 7ull) != 0) {
    set_error("elem_offset must be a multiple of 8 (ChaCha20 block aligned shard)");
    return FBM_E_ARG;
  }
  const uint64_t n_glob = elem_offset + n;
  if (n_glob < n || n_glob + 1000ull > (1ull << 61)) {
    set_error("Can not perform encryiton due to large input vector");
    return FBM_E_ARG;
  }
  // (i + tau).to_bytes(8, 'big') (_lom.py:81) past 2^64 is the reference's OverflowError, raised
  // after its overflow guard and only when there are peers (no PRF call without one): reported
  // through the status words in that order (fbm_check_stats), the counters wrapping meanwhile
  const int round_range = n_peers > 0 && n > 0 && tau > ~0ull - (n_glob - 1);
  // peers in groups of FBM_MAX_PEERS (the kernel-argument block): the first group with the
  // quantise/weight/overflow statistics, later groups accumulated in place
  for (int g0 = 0; g0 == 0 || g0 < n_peers; g0 += FBM_MAX_PEERS) {
    const int gn = n_peers - g0 < FBM_MAX_PEERS ? n_peers - g0 : FBM_MAX_PEERS;
    LomPeers pe;
    fill_peers(pe, nonce, tau);
    pe.n_peers = gn < 0 ? 0 : gn;
    pe.raw_seeds = raw_seeds;
    pe.elem_offset = elem_offset;
    pe.round_range = g0 == 0 ? round_range : 0;
    for (int p = 0; p < pe.n_peers; ++p) {
      memcpy(pe.secret[p], secrets + 32 * (g0 + p), 32);
      if (signs[g0 + p] >= 0) pe.add_bits |= 1ull << p;
    }
    if (g0 == 0)
      rc = timed("lom_protect", s, [&] { return launch_lom_protect(x, x_dtype, n, qp, weight, pe, y, stats, s); });
    else
      rc = timed("lom_protect", s, [&] { return launch_lom_mask_accumulate(n, pe, y, s); });
    if (rc) return rc;
  }
  return FBM_OK;
}

int fbm_prf_key(const uint8_t* secret, const uint8_t* nonce, uint64_t tau, uint8_t* seed_out, void* stream) {
  if (!secret || !nonce || !seed_out) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  LomPeers pe;
  fill_peers(pe, nonce, tau);
  pe.n_peers = 1;
  memcpy(pe.secret[0], secret, 32);
  return launch_prf_key(pe, (uint32_t*)seed_out, (hipStream_t)stream);
}

int fbm_dequantize_as(const uint64_t* u, uint64_t n, double neg_clip, double step, void* out, int out_dtype,
                      void* stream) {
  int rc = check_out_dtype(out_dtype);
  if (rc) return rc;
  if (n > 0 && (!u || !out)) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return launch_dequantize(u, n, neg_clip, step, out, out_dtype, (hipStream_t)stream);
}

int fbm_dequantize(const uint64_t* u, uint64_t n, double neg_clip, double step, double* out, void* stream) {
  return fbm_dequantize_as(u, n, neg_clip, step, out, FBM_F64, stream);
}

int fbm_lom_aggregate(const uint64_t* y, int n_parties, uint64_t n, uint64_t total_weight, double neg_clip,
                      double step, double* out, uint64_t* sums, uint32_t* stats, void* stream) {
  return fbm_lom_aggregate_as(y, n_parties, n, total_weight, neg_clip, step, out, FBM_F64, sums, stats, stream);
}

int fbm_lom_aggregate_as(const uint64_t* y, int n_parties, uint64_t n, uint64_t total_weight, double neg_clip,
                         double step, void* out, int out_dtype, uint64_t* sums, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = check_out_dtype(out_dtype);  // (first: an argument error that needs no device)
  if (rc) return rc;
  if ((rc = zero_stats(stats, s))) return rc;
  if (n_parties < 1 || total_weight == 0 || (n > 0 && !y)) {
    set_error("invalid aggregate arguments (n_parties=%d, total_weight=%llu)", n_parties,
              (unsigned long long)total_weight);
    return FBM_E_ARG;
  }
  return timed("lom_aggregate", s, [&] { return launch_lom_aggregate(y, n_parties, n, total_weight, neg_clip, step, out, out_dtype, sums, stats, s); });
}

// ---- host-buffer LOM calls (small vectors): copy in, kernel, copy out, one stream synchronisation ----
// A 1 000-element list call is launch-bound; these fold its H2D copy, kernel, output and status copies
// and the wait into one C call (no device tensors made per call on the host side).

static int host_copy(void* dst, const void* src, uint64_t bytes, hipMemcpyKind kind, hipStream_t s, const char* what) {
  if (!bytes) return FBM_OK;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, s);
  if (e != hipSuccess) {
    set_error("hipMemcpyAsync(%s): %s", what, hipGetErrorString(e));
    return FBM_E_HIP;
  }
  return FBM_OK;
}

static int host_wait(hipStream_t s) {
  hipError_t e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_error("hipStreamSynchronize: %s", hipGetErrorString(e));
    return FBM_E_HIP;
  }
  return FBM_OK;
}

// workspace: input rows | output (n words) immediately followed by the status words, so that a caller
// whose host output and status words are adjacent too gets both back in one copy
uint64_t fbm_lom_host_workspace(uint64_t n, int n_parties) {
  const uint64_t rows = n_parties > 1 ? (uint64_t)n_parties : 1u;
  return align256(rows * n * 8) + align256(n * 8 + FBM_STATS_WORDS * 4);
}

static int host_copy_back(void* out_host, const void* out, uint64_t n, uint32_t* stats_host, const uint32_t* st,
                          hipStream_t s) {
  if ((uint8_t*)stats_host == (uint8_t*)out_host + n * 8)  // adjacent on the host as on the device: one copy
    return host_copy(out_host, out, n * 8 + FBM_STATS_WORDS * 4, hipMemcpyDeviceToHost, s, "output+stats");
  int rc = host_copy(out_host, out, n * 8, hipMemcpyDeviceToHost, s, "output");
  return rc ? rc : host_copy(stats_host, st, FBM_STATS_WORDS * 4, hipMemcpyDeviceToHost, s, "stats");
}

int fbm_lom_protect_host(const void* x_host, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                         uint64_t target_m1, uint64_t weight, const uint8_t* secrets, const int8_t* signs, int n_peers,
                         int raw_seeds, const uint8_t* nonce, uint64_t tau, uint64_t elem_offset, uint64_t* y_host,
                         uint32_t* stats_host, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!workspace || !stats_host || (n > 0 && (!x_host || !y_host))) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  if (!float_dtype(x_dtype) && x_dtype != FBM_U64) {
    set_error("x_dtype must be FBM_F16, FBM_BF16, FBM_F32, FBM_F64 or FBM_U64");
    return FBM_E_ARG;
  }
  uint8_t* w = (uint8_t*)workspace;
  void* x = w;
  uint64_t* y = (uint64_t*)(w + align256(n * 8));
  uint32_t* st = (uint32_t*)(w + align256(n * 8) + n * 8);
  const uint64_t xb = n * (x_dtype == FBM_F16 || x_dtype == FBM_BF16 ? 2u : x_dtype == FBM_F32 ? 4u : 8u);
  int rc = host_copy(x, x_host, xb, hipMemcpyHostToDevice, s, "x");
  if (!rc) rc = fbm_lom_protect(x, x_dtype, n, clip, two_clip, target_f, target_m1, weight, secrets, signs, n_peers,
                                raw_seeds, nonce, tau, elem_offset, y, st, stream);
  if (!rc) rc = host_copy_back(y_host, y, n, stats_host, st, s);
  const int wrc = host_wait(s);  // (also after an error: nothing of this call left in flight on the buffers)
  return rc ? rc : wrc;
}

int fbm_lom_aggregate_host(const uint64_t* y_host, int n_parties, uint64_t n, uint64_t total_weight, double neg_clip,
                           double step, double* out_host, uint32_t* stats_host, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!workspace || !stats_host || (n > 0 && (!y_host || !out_host))) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  if (n_parties < 1) {
    set_error("invalid aggregate arguments (n_parties=%d, total_weight=%llu)", n_parties,
              (unsigned long long)total_weight);
    return FBM_E_ARG;
  }
  uint8_t* w = (uint8_t*)workspace;
  const uint64_t yb = (uint64_t)n_parties * n * 8;
  uint64_t* y = (uint64_t*)w;
  double* out = (double*)(w + align256(yb));
  uint32_t* st = (uint32_t*)(w + align256(yb) + n * 8);
  int rc = host_copy(y, y_host, yb, hipMemcpyHostToDevice, s, "y");
  if (!rc) rc = fbm_lom_aggregate(y, n_parties, n, total_weight, neg_clip, step, out, nullptr, st, stream);
  if (!rc) rc = host_copy_back(out_host, out, n, stats_host, st, s);
  const int wrc = host_wait(s);
  return rc ? rc : wrc;
}

// FBM_COMPACT_H=0 (A/B builds with -DFBM_AB_KNOBS): whole 256-byte H rows for every engine, as before round 4
static bool jl_compact_h() {
#ifdef FBM_AB_KNOBS
  static const bool on = !(getenv("FBM_COMPACT_H") && !strcmp(getenv("FBM_COMPACT_H"), "0"));
  return on;
#else
  return true;
#endif
}

// A workspace as its members in order, each 256-byte aligned; `off` after the last one is its size, so
// a layout and the size its *_workspace function reports come from the same walk.
struct WsWalk {
  uintptr_t base;
  uint64_t off;
  uint32_t* take(uint64_t bytes) {
    uint32_t* p = (uint32_t*)(base + off);
    off += align256(bytes);
    return p;
  }
};
static uint64_t blocked_bytes(uint64_t n_ct) { return ((n_ct + 255) / 256) * 256 * FBM_NL * 4; }

// encrypt workspace: ops | cst | pt [n_ct][32] | nude (blocked) | H [n_ct][64] | table |
//                    H^-1 [n_ct][64] + y [n_ct][32] (negative keys) | Hc [n_ct][8] (compact H rows)
struct JlEncWs {
  uint32_t *ops, *cst, *pt, *nude, *H, *table, *Hinv, *Y, *Hc;
  uint64_t slots, bytes;
};
static JlEncWs enc_ws(void* workspace, uint64_t n_ct) {
  WsWalk k{(uintptr_t)workspace, 0};
  JlEncWs w;
  w.slots = table_slots_for(n_ct);
  w.ops = k.take(FBM_OPS_WORDS * 4);
  w.cst = k.take(FBM_CST_WORDS * 4);
  w.pt = k.take(n_ct * 32 * 4);
  w.nude = k.take(blocked_bytes(n_ct));
  w.H = k.take(n_ct * 64 * 4);
  w.table = k.take(jl_table_bytes(n_ct));
  w.Hinv = k.take(n_ct * 64 * 4);  // negative keys only: H^|key| digits (after the table)
  w.Y = k.take(n_ct * 32 * 4);
  w.Hc = k.take(n_ct * 8 * 4);  // compact H rows: 32 B per ciphertext
  if (!jl_compact_h()) w.Hc = nullptr;
  w.bytes = k.off;
  return w;
}

// aggregate workspace: ops | cst | X (blocked) | H [n_ct][64] | E [n_ct][64] | F [n_ct][64] |
//                      xs [n_ct][32] | table | Hc [n_ct][8]
struct JlAggWs {
  uint32_t *ops, *cst, *X, *H, *E, *F, *xs, *table, *Hc;
  uint64_t slots, bytes;
};
static JlAggWs agg_ws(void* workspace, uint64_t n_ct) {
  WsWalk k{(uintptr_t)workspace, 0};
  JlAggWs w;
  w.slots = table_slots_for(n_ct);
  w.ops = k.take(FBM_OPS_WORDS * 4);
  w.cst = k.take(FBM_CST_WORDS * 4);
  w.X = k.take(blocked_bytes(n_ct));
  w.H = k.take(n_ct * 64 * 4);
  w.E = k.take(n_ct * 64 * 4);
  w.F = k.take(n_ct * 64 * 4);
  w.xs = k.take(n_ct * 32 * 4);
  w.table = k.take(jl_table_bytes(n_ct));
  w.Hc = k.take(n_ct * 8 * 4);
  if (!jl_compact_h()) w.Hc = nullptr;
  w.bytes = k.off;
  return w;
}

uint64_t fbm_jl_encrypt_workspace(uint64_t n_ct) { return enc_ws(nullptr, n_ct).bytes; }

uint64_t fbm_jl_aggregate_workspace(uint64_t n_ct) { return agg_ws(nullptr, n_ct).bytes; }

// The argument checks fbm_jl_encrypt (its phases) and fbm_jl_encrypt_factor share, in the order both report
// them.  by_factor: the caller brings the factor rows instead of key and round.  zero: zero the status words
// first.  n_ct = 0 with FBM_OK: an empty call, nothing to launch.
static int jl_encrypt_checks(const void* x, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                             uint64_t target_m1, uint64_t weight, int cr, const uint32_t* biprime, const uint32_t* key,
                             const uint32_t* tau, bool by_factor, const uint32_t* factor, const uint32_t* ct_out,
                             const void* workspace, uint32_t* stats, hipStream_t s, bool zero, QuantParams& qp,
                             uint64_t& n_ct) {
  int rc;
  n_ct = 0;
  if (zero && (rc = zero_stats(stats, s))) return rc;
  if ((rc = quant_params(clip, two_clip, target_f, target_m1, qp))) return rc;
  if (!float_dtype(x_dtype) && x_dtype != FBM_U64 && x_dtype != FBM_U128 && x_dtype != FBM_PT) {
    set_error("x_dtype must be FBM_F16, FBM_BF16, FBM_F32, FBM_F64, FBM_U64, FBM_U128 or FBM_PT");
    return FBM_E_ARG;
  }
  if ((x_dtype == FBM_U128 || x_dtype == FBM_PT) && weight != 1) {
    set_error("raw-integer / plaintext inputs take weight 1");
    return FBM_E_ARG;
  }
  if (x_dtype == FBM_PT && cr != 1) {
    set_error("plaintext input (FBM_PT) takes cr = 1");
    return FBM_E_ARG;
  }
  if (!biprime || (!by_factor && !key)) {
    set_error(by_factor ? "null biprime" : "null biprime/key");
    return FBM_E_ARG;
  }
  if (!by_factor && !tau) {  // the round is FDH's input: never defaulted (a NULL would silently mean round 0)
    set_error("null tau (the round's %d limbs)", FBM_TAU_LIMBS);
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (cr < 1) {
    set_error("invalid cr=%d", cr);
    return FBM_E_ARG;
  }
  const uint64_t cts = (n + (uint64_t)cr - 1) / (uint64_t)cr;
  if (cts > FBM_JL_MAX_CT) {
    set_error("%llu ciphertexts exceed FBM_JL_MAX_CT per call; split the range with ct_offset",
              (unsigned long long)cts);
    return FBM_E_UNSUPPORTED;
  }
  if (!x || (by_factor && !factor) || !ct_out || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  if (by_factor) {  // jl_encf_kernel stages N pt + 1 in the output rows before it reads the factor rows
    const uintptr_t o0 = (uintptr_t)ct_out, o1 = o0 + cts * 256, f0 = (uintptr_t)factor, f1 = f0 + cts * 256;
    if (o0 < f1 && f0 < o1) {
      set_error("fbm_jl_encrypt_factor: ct_out must not overlap factor");
      return FBM_E_ARG;
    }
  }
  if ((int64_t)weight <= -(int64_t)(1 << 17)) {  // negative: the two's complement of a weight > -2^17
    set_error("negative weight %lld outside (-2^17, 0)", (long long)(int64_t)weight);
    return FBM_E_ARG;
  }
  n_ct = cts;
  return FBM_OK;
}

// phase bit 1: the prologue (status word, constants, pack, nude, FDH, and the inverse of H
// for a negative key); bit 2: the exponentiation.  Both phases rebuild the same host
// parameters from the same arguments and use the same workspace, so (1 then 2) == 3.
static int jl_encrypt_impl(const void* x, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                           uint64_t target_m1, uint64_t weight, int es, int cr, const uint32_t* biprime,
                           const uint32_t* key, int key_negative, const uint32_t* tau, uint64_t ct_offset, uint32_t* ct_out,
                           void* workspace, uint32_t* stats, void* stream, int phase) {
  hipStream_t s = (hipStream_t)stream;
  QuantParams qp;
  uint64_t n_ct;
  int rc = jl_encrypt_checks(x, x_dtype, n, clip, two_clip, target_f, target_m1, weight, cr, biprime, key, tau, false,
                             nullptr, ct_out, workspace, stats, s, (phase & 1) != 0, qp, n_ct);
  if (rc || !n_ct) return rc;
  bool generic, short_on;
  if ((rc = jl_path_for(workspace, phase, 3, biprime, generic, short_on))) return rc;
  const JlEncWs w = enc_ws(workspace, n_ct);
  uint32_t *const cst = w.cst, *const pt = w.pt, *const H = w.H;
  if (generic) {  // any N (fbm_gen.hip): pack -> FDH -> H^key (N pt + 1) mod N^2
    if (es < 1 || es > 100 || (int64_t)es * cr > 1024) {
      set_error("invalid VES parameters es=%d cr=%d", es, cr);
      return FBM_E_ARG;
    }
    GenCtx g;
    JlParams fp;
    if ((rc = build_gen_ctx(biprime, key, key_negative, g)) || (rc = fdh_params_for_biprime(biprime, tau, ct_offset, fp)))
      return rc;
    const uint32_t* ptp = x_dtype == FBM_PT ? (const uint32_t*)x : pt;
    if (phase & 1) {
      if ((rc = launch_jl_gen_setup(g, cst, s))) return rc;
      if (x_dtype != FBM_PT &&
          (rc = timed("jl_pack", s, [&] { return launch_jl_pack(x, x_dtype, n, qp, weight, es, cr, n_ct, pt, stats, s); })))
        return rc;
      if ((rc = timed("jl_fdh", s, [&] { return launch_jl_fdh(n_ct, fp, H, stats, s); }))) return rc;
    }
    if (!(phase & 2)) return FBM_OK;
    const int negw = (int64_t)weight < 0 ? 1 : 0;
    return timed("jl_gen_exp", s, [&] { return launch_jl_gen_exp(H, ptp, negw, n_ct, cst, ct_out, stats, s); });
  }
  JlParams jp;
  if ((rc = build_jl_params(biprime, es, cr, tau, ct_offset, jp))) return rc;
  JlSched sc;
  int is_zero = 0;
  if ((rc = build_schedule(key, sc, is_zero))) {
    set_error("exponent schedule overflow");
    return rc;
  }
  jp.key_is_zero = is_zero;
  JlShort sh;
  const bool shq = build_short(biprime, key, is_zero, sc, sh, short_on);
  const bool inverse = key_negative && !is_zero;
  if (phase & 1) {
    if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, sc, w.ops, cst, s, shq ? &sh : nullptr); })))
      return rc;
    if (x_dtype != FBM_PT &&
        (rc = timed("jl_pack", s, [&] { return launch_jl_pack(x, x_dtype, n, qp, weight, es, cr, n_ct, pt, stats, s); })))
      return rc;
    const uint32_t* ptp = x_dtype == FBM_PT ? (const uint32_t*)x : pt;  // UserKey.encrypt: packed already
    const int negw = (int64_t)weight < 0 ? 1 : 0;
    if ((rc = timed("jl_nude", s, [&] { return launch_jl_nude(ptp, n_ct, jp, negw, w.nude, s); }))) return rc;
    if (!is_zero && (rc = timed("jl_fdh", s, [&] { return launch_jl_fdh(n_ct, jp, H, stats, s, w.Hc); }))) return rc;
  }
  if (!(phase & 2)) return FBM_OK;
  if (inverse) {
    // gmpy2.powmod with a negative exponent (_jls.py:60-73) is (H^-1)^|key| = (H^|key|)^-1:
    // the power's N-adic digits (any H < 2^2048), then the lift inverts it and multiplies
    // by nude in the same pass
    if ((rc = timed("jl_exp", s, [&] {
           return launch_jl_exp(H, n_ct, jp, sc, FBM_EXP_DEC | FBM_EXP_OUT_NADIC, nullptr, w.table, w.slots, w.ops, cst,
                                w.Hinv, s, w.Hc);
         })))
      return rc;
    return timed("jl_inv", s, [&] { return launch_jl_inv(n_ct, jp, cst, w.Hinv, w.Y, w.nude, ct_out, stats, s); });
  }
  // a phase-2-only call inside an open batch (fbm_jl_batch_begin) is recorded, not launched
  // (and not timed: the batch's one launch is, at the flush)
  auto go = [&] { return launch_jl_exp(H, n_ct, jp, sc, 0, w.nude, w.table, w.slots, w.ops, cst, ct_out, s, w.Hc); };
  const bool rec = phase == 2 && jl_batch_active();
  const bool acc = jl_batch_accept(rec);
  rc = rec ? go() : timed("jl_exp", s, go);
  jl_batch_accept(acc);
  return rc;
}

int fbm_jl_encrypt(const void* x, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                   uint64_t target_m1, uint64_t weight, int es, int cr, const uint32_t* biprime, const uint32_t* key,
                   int key_negative, const uint32_t* tau, uint64_t ct_offset, uint32_t* ct_out, void* workspace,
                   uint32_t* stats, void* stream) {
  return jl_encrypt_impl(x, x_dtype, n, clip, two_clip, target_f, target_m1, weight, es, cr, biprime, key,
                         key_negative, tau, ct_offset, ct_out, workspace, stats, stream, 3);
}

// The encrypt with its factor computed ahead: c_k = (N pt_k + 1) F_k mod N^2, F_k = H(t_k)^sk the
// decryption-factor kernels' output for the party's key (fbm_jl_decrypt_factor) -- fbm_jl_encrypt's
// ciphertexts bit for bit (the exponentiation's only input besides the plaintext is H(t_k)).  Any
// engine policy; the modulus must be odd and >= 3 (other moduli: fbm_jl_encrypt).
int fbm_jl_encrypt_factor(const void* x, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                          uint64_t target_m1, uint64_t weight, int es, int cr, const uint32_t* biprime,
                          const uint32_t* factor, uint32_t* ct_out, void* workspace, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  QuantParams qp;
  uint64_t n_ct;
  int rc = jl_encrypt_checks(x, x_dtype, n, clip, two_clip, target_f, target_m1, weight, cr, biprime, nullptr, nullptr,
                             true, factor, ct_out, workspace, stats, s, true, qp, n_ct);
  if (rc || !n_ct) return rc;
  if ((biprime[0] & 1u) == 0u || jl_is_one(biprime)) {
    set_error("fbm_jl_encrypt_factor takes an odd N >= 3 (fbm_jl_encrypt takes any N)");
    return FBM_E_UNSUPPORTED;
  }
  JlParams jp;
  if ((rc = build_jl_params(biprime, es, cr, nullptr, 0, jp))) return rc;
  JlSched none;
  memset(&none, 0, sizeof(none));
  const JlEncWs w = enc_ws(workspace, n_ct);  // of the encrypt workspace: ops | cst | pt
  uint32_t *const cst = w.cst, *const pt = w.pt;
  if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, none, w.ops, cst, s); }))) return rc;
  {  // R^2 mod N^2: two products, each dropping one R
    JlRk r;
    jl_rk_for(jp.N32, 1, r);
    if ((rc = timed("jl_rk", s, [&] { return launch_jl_rk(r, cst, s); }))) return rc;
  }
  if (x_dtype != FBM_PT &&
      (rc = timed("jl_pack", s, [&] { return launch_jl_pack(x, x_dtype, n, qp, weight, es, cr, n_ct, pt, stats, s); })))
    return rc;
  const uint32_t* ptp = x_dtype == FBM_PT ? (const uint32_t*)x : pt;
  const int negw = (int64_t)weight < 0 ? 1 : 0;
  return timed("jl_encf", s, [&] { return launch_jl_encf(ptp, n_ct, jp, cst, negw, factor, ct_out, s); });
}

int fbm_jl_encrypt_phase(const void* x, int x_dtype, uint64_t n, double clip, double two_clip, double target_f,
                         uint64_t target_m1, uint64_t weight, int es, int cr, const uint32_t* biprime,
                         const uint32_t* key, int key_negative, const uint32_t* tau, uint64_t ct_offset, uint32_t* ct_out,
                         void* workspace, uint32_t* stats, void* stream, int phase) {
  if (phase < 1 || phase > 3) {
    set_error("fbm_jl_encrypt_phase: phase must be 1, 2 or 3");
    return FBM_E_ARG;
  }
  return jl_encrypt_impl(x, x_dtype, n, clip, two_clip, target_f, target_m1, weight, es, cr, biprime, key,
                         key_negative, tau, ct_offset, ct_out, workspace, stats, stream, phase);
}

// ServerKey's factor H(t_k)^sk0 mod N^2 (inverse first for sk0 < 0): depends on the round,
// the ciphertext index and the key only -- not on the parties' ciphertexts.
// phase bits: 1 = constants + FDH, 2 = the exponentiation, 4 = the inverse (negative key)
static int jl_factor_impl(uint64_t n_ct, const uint32_t* biprime, const uint32_t* key, int key_negative, const uint32_t* tau,
                          uint64_t ct_offset, uint32_t* factor, const JlAggWs& w, uint32_t* stats, hipStream_t s,
                          int phase = 7) {
  JlParams jp;
  int rc;
  if (!tau) {
    set_error("null tau (the round's %d limbs)", FBM_TAU_LIMBS);
    return FBM_E_ARG;
  }
  bool generic, short_on;
  if ((rc = jl_path_for(w.ops, phase, 7, biprime, generic, short_on))) return rc;
  if (generic) {  // any N: FDH, then H^key mod N^2 with the inverse in the same kernel
    GenCtx g;
    if ((rc = build_gen_ctx(biprime, key, key_negative, g)) || (rc = fdh_params_for_biprime(biprime, tau, ct_offset, jp)))
      return rc;
    if (phase & 1) {
      if ((rc = launch_jl_gen_setup(g, w.cst, s))) return rc;
      if ((rc = timed("jl_fdh", s, [&] { return launch_jl_fdh(n_ct, jp, w.H, stats, s); }))) return rc;
    }
    if (phase & 2)
      return timed("jl_gen_exp", s, [&] { return launch_jl_gen_exp(w.H, nullptr, 0, n_ct, w.cst, factor, stats, s); });
    return FBM_OK;
  }
  if ((rc = build_jl_params(biprime, 1, 1, tau, ct_offset, jp))) return rc;
  JlSched sc;
  int is_zero = 0;
  if ((rc = build_schedule(key, sc, is_zero))) {
    set_error("exponent schedule overflow");
    return rc;
  }
  jp.key_is_zero = is_zero;
  JlShort sh;
  const bool shq = build_short(biprime, key, is_zero, sc, sh, short_on);
  const bool inv = key_negative && !is_zero;
  uint32_t* E = inv ? w.E : factor;
  if (phase & 1) {
    if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, sc, w.ops, w.cst, s, shq ? &sh : nullptr); })))
      return rc;
    if (!is_zero && (rc = timed("jl_fdh", s, [&] { return launch_jl_fdh(n_ct, jp, w.H, stats, s, w.Hc); })))
      return rc;
  }
  if (phase & 2) {
    // the inverse starts from the power's N-adic digits (no division by N needed)
    auto go = [&] {
      return launch_jl_exp(w.H, n_ct, jp, sc, FBM_EXP_DEC | (inv ? FBM_EXP_OUT_NADIC : 0), nullptr, w.table, w.slots,
                           w.ops, w.cst, E, s, w.Hc);
    };
    const bool rec = phase == 2 && jl_batch_active();  // recorded (not launched, not timed) in an open batch
    const bool acc = jl_batch_accept(rec);
    rc = rec ? go() : timed("jl_exp", s, go);
    jl_batch_accept(acc);
    if (rc) return rc;
  }
  if ((phase & 4) && inv && jl_batch_active()) {
    set_error("the decryption factor's inverse needs its exponentiation: flush the open batch first");
    return FBM_E_ARG;
  }
  if ((phase & 4) && inv &&
      (rc = timed("jl_inv", s, [&] { return launch_jl_inv(n_ct, jp, w.cst, E, w.xs, nullptr, factor, stats, s); })))  // xs: y scratch
    return rc;
  return FBM_OK;
}

// v = prod_u c_u * factor mod N^2, x = (v-1)/N, decode + average + dequantise
// x_raw != NULL: ServerKey.decrypt's x to x_raw [n_ct][32] instead of decode/average/dequantise
static int jl_combine_impl(const uint32_t* cts, int n_parties, uint64_t n_ct, int es, int cr, uint64_t n_out,
                           const uint32_t* biprime, const uint32_t* factor, uint64_t total_weight, double neg_clip,
                           double step, void* out, int out_dtype, uint64_t* sums, const JlAggWs& w, uint32_t* stats,
                           hipStream_t s, uint32_t* x_raw = nullptr) {
  JlParams jp;
  int rc;
  if (jl_is_one(biprime)) {  // the reference's invert(delta^2, N^2) has no nonzero result modulo 1
    set_error("invert() no inverse exists");
    return FBM_E_INVERSE;
  }
  if (jl_generic(biprime)) {  // any N: product, factor, ((v - 1) // N) mod N, then the decode
    if (es < 1 || cr < 1 || es > 100 || (int64_t)es * cr > 1024) {
      set_error("invalid VES parameters es=%d cr=%d", es, cr);
      return FBM_E_ARG;
    }
    GenCtx g;
    if ((rc = build_gen_ctx(biprime, nullptr, 0, g)) || (rc = launch_jl_gen_setup(g, w.cst, s))) return rc;
    uint32_t* xs = x_raw ? x_raw : w.xs;
    if ((rc = timed("jl_gen_combine", s, [&] {
           return launch_jl_gen_combine(cts, n_parties, n_ct, factor, w.cst, FBM_GEN_DECRYPT, xs, stats, s);
         })))
      return rc;
    if (x_raw) return FBM_OK;
    return timed("jl_decode", s, [&] {
      return launch_jl_decode(w.xs, es, cr, n_out, total_weight, neg_clip, step, out, out_dtype, sums, stats, s);
    });
  }
  if ((rc = build_jl_params(biprime, es, cr, nullptr, 0, jp))) return rc;
  JlSched none;
  memset(&none, 0, sizeof(none));
  if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, none, w.ops, w.cst, s); }))) return rc;
  {  // R^(P+1) mod N^2: the product's uniform first operand (P + 1 products each drop one R)
    JlRk r;
    jl_rk_for(jp.N32, n_parties, r);
    if ((rc = timed("jl_rk", s, [&] { return launch_jl_rk(r, w.cst, s); }))) return rc;
  }
  uint32_t* xs = x_raw ? x_raw : w.xs;
  if ((rc = timed("jl_prod", s, [&] { return launch_jl_prod(cts, n_parties, n_ct, jp, w.cst, factor, xs, s); })))
    return rc;
  if (x_raw) return FBM_OK;
  return timed("jl_decode", s, [&] {
    return launch_jl_decode(w.xs, es, cr, n_out, total_weight, neg_clip, step, out, out_dtype, sums, stats, s);
  });
}

static int jl_agg_checks(int n_parties, uint64_t n_ct, const uint32_t* biprime, uint64_t total_weight) {
  if (n_parties < 1 || !biprime || total_weight == 0) {
    set_error("invalid aggregate arguments");
    return FBM_E_ARG;
  }
  if (n_ct > FBM_JL_MAX_CT) {
    set_error("%llu ciphertexts exceed FBM_JL_MAX_CT per call; split the range with ct_offset",
              (unsigned long long)n_ct);
    return FBM_E_UNSUPPORTED;
  }
  return FBM_OK;
}

int fbm_jl_aggregate(const uint32_t* cts, int n_parties, uint64_t n_ct, int es, int cr, uint64_t n_out,
                     const uint32_t* biprime, const uint32_t* key, int key_negative, const uint32_t* tau, uint64_t ct_offset,
                     uint64_t total_weight, double neg_clip, double step, double* out, uint64_t* sums,
                     void* workspace, uint32_t* stats, void* stream) {
  return fbm_jl_aggregate_as(cts, n_parties, n_ct, es, cr, n_out, biprime, key, key_negative, tau, ct_offset,
                             total_weight, neg_clip, step, out, FBM_F64, sums, workspace, stats, stream);
}

int fbm_jl_aggregate_as(const uint32_t* cts, int n_parties, uint64_t n_ct, int es, int cr, uint64_t n_out,
                        const uint32_t* biprime, const uint32_t* key, int key_negative, const uint32_t* tau,
                        uint64_t ct_offset, uint64_t total_weight, double neg_clip, double step, void* out,
                        int out_dtype, uint64_t* sums, void* workspace, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = check_out_dtype(out_dtype);  // (first: an argument error that needs no device)
  if (rc) return rc;
  if ((rc = zero_stats(stats, s))) return rc;
  if ((rc = jl_agg_checks(n_parties, n_ct, biprime, total_weight))) return rc;
  if (!key) {
    set_error("null key");
    return FBM_E_ARG;
  }
  if (n_ct == 0) return FBM_OK;
  if (n_out > n_ct * (uint64_t)cr) n_out = n_ct * (uint64_t)cr;
  if (!cts || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const JlAggWs w = agg_ws(workspace, n_ct);
  if ((rc = jl_factor_impl(n_ct, biprime, key, key_negative, tau, ct_offset, w.F, w, stats, s))) return rc;
  return jl_combine_impl(cts, n_parties, n_ct, es, cr, n_out, biprime, w.F, total_weight, neg_clip, step, out, out_dtype,
                         sums, w, stats, s);
}

int fbm_jl_decrypt_factor(uint64_t n_ct, const uint32_t* biprime, const uint32_t* key, int key_negative, const uint32_t* tau,
                          uint64_t ct_offset, uint32_t* factor, void* workspace, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if ((rc = jl_agg_checks(1, n_ct, biprime, 1))) return rc;
  if (n_ct == 0) return FBM_OK;
  if (!key || !factor || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return jl_factor_impl(n_ct, biprime, key, key_negative, tau, ct_offset, factor, agg_ws(workspace, n_ct), stats, s);
}

int fbm_jl_decrypt_factor_phase(uint64_t n_ct, const uint32_t* biprime, const uint32_t* key, int key_negative,
                                const uint32_t* tau, uint64_t ct_offset, uint32_t* factor, void* workspace, uint32_t* stats,
                                void* stream, int phase) {
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (phase < 1 || phase > 7) {
    set_error("fbm_jl_decrypt_factor_phase: phase must be a non-empty subset of {1, 2, 4}");
    return FBM_E_ARG;
  }
  if ((phase & 1) && (rc = zero_stats(stats, s))) return rc;
  if ((rc = jl_agg_checks(1, n_ct, biprime, 1))) return rc;
  if (n_ct == 0) return FBM_OK;
  if (!key || !factor || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return jl_factor_impl(n_ct, biprime, key, key_negative, tau, ct_offset, factor, agg_ws(workspace, n_ct), stats, s,
                        phase);
}

int fbm_jl_aggregate_factor(const uint32_t* cts, int n_parties, uint64_t n_ct, int es, int cr, uint64_t n_out,
                            const uint32_t* biprime, const uint32_t* factor, uint64_t total_weight, double neg_clip,
                            double step, double* out, uint64_t* sums, void* workspace, uint32_t* stats, void* stream) {
  return fbm_jl_aggregate_factor_as(cts, n_parties, n_ct, es, cr, n_out, biprime, factor, total_weight, neg_clip, step,
                                    out, FBM_F64, sums, workspace, stats, stream);
}

int fbm_jl_aggregate_factor_as(const uint32_t* cts, int n_parties, uint64_t n_ct, int es, int cr, uint64_t n_out,
                               const uint32_t* biprime, const uint32_t* factor, uint64_t total_weight, double neg_clip,
                               double step, void* out, int out_dtype, uint64_t* sums, void* workspace, uint32_t* stats,
                               void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = check_out_dtype(out_dtype);  // (first: an argument error that needs no device)
  if (rc) return rc;
  if ((rc = zero_stats(stats, s))) return rc;
  if ((rc = jl_agg_checks(n_parties, n_ct, biprime, total_weight))) return rc;
  if (n_ct == 0) return FBM_OK;
  if (n_out > n_ct * (uint64_t)cr) n_out = n_ct * (uint64_t)cr;
  if (!cts || !factor || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return jl_combine_impl(cts, n_parties, n_ct, es, cr, n_out, biprime, factor, total_weight, neg_clip, step, out,
                         out_dtype, sums, agg_ws(workspace, n_ct), stats, s);
}

// ---- the JoyeLibert object API (fedbiomed_amd/secagg/_jls.py) ----
int fbm_jl_pack(const void* x, int x_dtype, uint64_t n, int es, int cr, uint32_t* pt, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if (x_dtype != FBM_U128) {
    set_error("fbm_jl_pack takes FBM_U128 values");
    return FBM_E_ARG;
  }
  if (es < 1 || cr < 1 || (int64_t)es * cr > 1024) {
    set_error("invalid VES parameters es=%d cr=%d", es, cr);
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!x || !pt) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const uint64_t n_ct = (n + (uint64_t)cr - 1) / (uint64_t)cr;
  QuantParams qp{};
  return timed("jl_pack", s, [&] { return launch_jl_pack(x, x_dtype, n, qp, 1, es, cr, n_ct, pt, stats, s); });
}

int fbm_jl_unpack(const uint32_t* pt, uint64_t n_ct, int es, int cr, uint64_t n_out, uint64_t* vals, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (es < 1 || es > 128 || cr < 1 || (int64_t)es * cr > 1024) {
    set_error("invalid VES parameters es=%d cr=%d (device decode: es <= 128)", es, cr);
    return FBM_E_ARG;
  }
  if (n_out > n_ct * (uint64_t)cr) n_out = n_ct * (uint64_t)cr;
  if (n_out == 0) return FBM_OK;
  if (!pt || !vals) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("jl_decode", s, [&] { return launch_jl_decode(pt, es, cr, n_out, 1, 0.0, 1.0, nullptr, FBM_F64, vals, nullptr, s); });
}

int fbm_jl_fdh(uint64_t n_ct, const uint32_t* modulus_odd, int modulus_even, const uint32_t* tau, uint64_t ct_offset,
               uint32_t* h, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if (!modulus_odd || !tau) {
    set_error("null modulus or tau");
    return FBM_E_ARG;
  }
  JlParams jp;
  if ((rc = fdh_params(modulus_odd, modulus_even, tau, ct_offset, jp))) return rc;
  if (n_ct == 0) return FBM_OK;
  if (!h) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("jl_fdh", s, [&] { return launch_jl_fdh(n_ct, jp, h, stats, s); });
}

int fbm_jl_fdh_msg(uint64_t n, const uint32_t* t, int t_words, int bits_size, const uint32_t* modulus_odd,
                   int modulus_even, uint32_t* h, int h_words, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if (!modulus_odd || bits_size < 0 || t_words < 0) {
    set_error("fbm_jl_fdh_msg: null modulus or negative size");
    return FBM_E_ARG;
  }
  const int msg_bytes = bits_size / 2;  // int(t).to_bytes(bits_size // 2, 'big')
  if ((int64_t)t_words * 4 < msg_bytes) {
    set_error("fbm_jl_fdh_msg: %d words hold no %d-byte message", t_words, msg_bytes);
    return FBM_E_ARG;
  }
  if (!(modulus_odd[0] & 1u)) {
    set_error("fbm_jl_fdh_msg: the modulus's odd part must be odd");
    return FBM_E_ARG;
  }
  // digests r may hold: the reference's inner loop breaks while r is shorter than bits_size // 8 bytes
  const int bytes = bits_size / 8;
  const int kmax = bytes >= 1 ? (bytes - 1) / 32 : 0;
  if (n == 0) return FBM_OK;
  if (kmax == 0) {  // a single digest is already bits_size // 8 bytes: the counter byte overflows at 256
    set_error("FDH of bits_size %d: r never shorter than bits_size // 8 bytes (reference: OverflowError)", bits_size);
    return FBM_E_FDH;
  }
  if (!t || !h) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const int need = fbm_jl_fdh_msg_row_words(bits_size);
  if (h_words < need) {
    set_error("fbm_jl_fdh_msg: rows of %d words hold no r of bits_size %d (%d words)", h_words, bits_size, need);
    return FBM_E_ARG;
  }
  if (kmax <= FBM_FDH_MSG_DIGESTS) {
    if (h_words != FBM_FDH_MSG_ROW) {
      set_error("fbm_jl_fdh_msg: bits_size %d takes rows of %d words", bits_size, FBM_FDH_MSG_ROW);
      return FBM_E_ARG;
    }
    return timed("jl_fdh", s, [&] {
      return launch_jl_fdh_msg(n, t, t_words, msg_bytes, kmax, modulus_odd, modulus_even ? 1 : 0, h, stats, s);
    });
  }
  // r of up to 255 digests: the incremental Montgomery residue of the wide kernel (fbm_jl.hip)
  uint32_t k1[32], k2[32], mp;
  fdh_wide_consts(modulus_odd, k1, k2, mp);
  return timed("jl_fdh", s, [&] {
    return launch_jl_fdh_msg_wide(n, t, t_words, msg_bytes, kmax, modulus_odd, k1, k2, mp, modulus_even ? 1 : 0, h,
                                  h_words, stats, s);
  });
}

int fbm_jl_fdh_msg_row_words(int bits_size) {
  const int bytes = bits_size / 8;
  int kmax = bytes >= 1 ? (bytes - 1) / 32 : 0;
  if (kmax > 255) kmax = 255;
  return kmax <= FBM_FDH_MSG_DIGESTS ? FBM_FDH_MSG_ROW : 8 * kmax;
}

int fbm_jl_product(const uint32_t* cts, int n_parties, uint64_t n_ct, const uint32_t* biprime, uint32_t* out,
                   void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = jl_agg_checks(n_parties, n_ct, biprime, 1))) return rc;
  if (n_ct == 0) return FBM_OK;
  if (!cts || !out || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const JlAggWs w = agg_ws(workspace, n_ct);
  if (jl_generic(biprime)) {
    GenCtx g;
    if ((rc = build_gen_ctx(biprime, nullptr, 0, g)) || (rc = launch_jl_gen_setup(g, w.cst, s))) return rc;
    return timed("jl_gen_combine", s, [&] {
      return launch_jl_gen_combine(cts, n_parties, n_ct, nullptr, w.cst, FBM_GEN_PRODUCT, out, nullptr, s);
    });
  }
  JlParams jp;
  if ((rc = build_jl_params(biprime, 1, 1, nullptr, 0, jp))) return rc;
  JlSched none;
  memset(&none, 0, sizeof(none));
  if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, none, w.ops, w.cst, s); }))) return rc;
  {  // R^P: P products, each dropping one R
    JlRk r;
    jl_rk_for(jp.N32, n_parties - 1, r);
    if ((rc = timed("jl_rk", s, [&] { return launch_jl_rk(r, w.cst, s); }))) return rc;
  }
  return timed("jl_prod", s, [&] { return launch_jl_prod(cts, n_parties, n_ct, jp, w.cst, nullptr, out, s); });
}

// the streaming product: acc <- acc * prod_j rows[j] mod N^2 in place (jl_fold_kernel; generic: jl_gen_fold_kernel)
int fbm_jl_fold(uint32_t* acc, const uint32_t* rows, int k, uint64_t n_ct, const uint32_t* biprime, int seed_ops,
                void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if ((rc = jl_agg_checks(k, n_ct, biprime, 1))) return rc;
  if (seed_ops < 0 || (seed_ops > 0 && k > seed_ops)) {
    set_error("fbm_jl_fold: %d rows into an accumulator seeded for %d", k, seed_ops);
    return FBM_E_ARG;
  }
  if (n_ct == 0) return FBM_OK;
  if (!acc || !rows || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const JlAggWs w = agg_ws(workspace, 1);  // (ops and cst only: their place does not depend on n_ct)
  if (jl_generic(biprime)) {
    GenCtx g;
    if ((rc = build_gen_ctx(biprime, nullptr, 0, g)) || (rc = launch_jl_gen_setup(g, w.cst, s))) return rc;
    return timed("jl_gen_fold", s, [&] { return launch_jl_gen_fold(acc, rows, k, n_ct, w.cst, seed_ops > 0, s); });
  }
  JlParams jp;
  if ((rc = build_jl_params(biprime, 1, 1, nullptr, 0, jp))) return rc;
  JlSched none;
  memset(&none, 0, sizeof(none));
  if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, none, w.ops, w.cst, s); }))) return rc;
  if (seed_ops > 0) {  // R^seed_ops: every folded row drops one R
    JlRk r;
    jl_rk_for(jp.N32, seed_ops - 1, r);
    if ((rc = timed("jl_rk", s, [&] { return launch_jl_rk(r, w.cst, s); }))) return rc;
  }
  return timed("jl_fold", s, [&] { return launch_jl_fold(acc, rows, k, n_ct, jp, w.cst, seed_ops > 0, s); });
}

int fbm_lom_fold(uint64_t* acc, const uint64_t* y, int k, uint64_t n, int first, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (k < 1 || (n > 0 && (!acc || !y))) {
    set_error("invalid fold arguments (k=%d)", k);
    return FBM_E_ARG;
  }
  return timed("lom_fold", s, [&] { return launch_lom_fold(acc, y, k, n, first, s); });
}

int fbm_jl_decrypt(const uint32_t* cts, int n_parties, uint64_t n_ct, const uint32_t* biprime, const uint32_t* key,
                   int key_negative, const uint32_t* tau, uint64_t ct_offset, uint32_t* x, void* workspace, uint32_t* stats,
                   void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if ((rc = jl_agg_checks(n_parties, n_ct, biprime, 1))) return rc;
  if (!key) {
    set_error("null key");
    return FBM_E_ARG;
  }
  if (n_ct == 0) return FBM_OK;
  if (!cts || !x || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const JlAggWs w = agg_ws(workspace, n_ct);
  if ((rc = jl_factor_impl(n_ct, biprime, key, key_negative, tau, ct_offset, w.F, w, stats, s))) return rc;
  return jl_combine_impl(cts, n_parties, n_ct, 1, 1, 0, biprime, w.F, 1, 0.0, 1.0, nullptr, FBM_F64, nullptr, w, stats, s,
                         x);
}

// out[k] = nude_k * h[k]^key mod N^2 for caller-given bases (a PublicParam whose hashing function
// is not FBM's FDH): the encrypt's exponentiation without its FDH (nude = N pt + 1), or with
// pt == NULL the decryption factor's (the power alone).  Workspace: the encrypt's layout.
int fbm_jl_powmod(const uint32_t* h, const uint32_t* pt, uint64_t n_ct, const uint32_t* biprime, const uint32_t* key,
                  int key_negative, uint32_t* out, void* workspace, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if ((rc = jl_agg_checks(1, n_ct, biprime, 1))) return rc;
  if (!key) {
    set_error("null key");
    return FBM_E_ARG;
  }
  if (n_ct == 0) return FBM_OK;
  if (!h || !out || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const JlEncWs w = enc_ws(workspace, n_ct);  // (its pt, H and Hc rows unused: h and pt are the caller's)
  uint32_t *const ops = w.ops, *const cst = w.cst, *const nude = w.nude, *const table = w.table;
  if (jl_generic(biprime)) {
    GenCtx g;
    if ((rc = build_gen_ctx(biprime, key, key_negative, g)) || (rc = launch_jl_gen_setup(g, cst, s))) return rc;
    return timed("jl_gen_exp", s, [&] { return launch_jl_gen_exp(h, pt, 0, n_ct, cst, out, stats, s); });
  }
  JlParams jp;
  if ((rc = build_jl_params(biprime, 1, 1, nullptr, 0, jp))) return rc;
  JlSched sc;
  int is_zero = 0;
  if ((rc = build_schedule(key, sc, is_zero))) {
    set_error("exponent schedule overflow");
    return rc;
  }
  jp.key_is_zero = is_zero;
  JlShort sh;
  const bool shq = build_short(biprime, key, is_zero, sc, sh, t_short_on != 0);
  if ((rc = timed("jl_setup", s, [&] { return launch_jl_setup(jp, sc, ops, cst, s, shq ? &sh : nullptr); })))
    return rc;
  const int mode = pt ? 0 : FBM_EXP_DEC;
  if (pt && (rc = timed("jl_nude", s, [&] { return launch_jl_nude(pt, n_ct, jp, 0, nude, s); }))) return rc;
  if (key_negative && !is_zero) {  // powmod with a negative exponent: (h^|key|)^-1, then * nude
    if ((rc = timed("jl_exp", s, [&] {
           return launch_jl_exp(h, n_ct, jp, sc, FBM_EXP_DEC | FBM_EXP_OUT_NADIC, nullptr, table, w.slots, ops, cst, w.Hinv,
                                s);
         })))
      return rc;
    return timed("jl_inv", s, [&] { return launch_jl_inv(n_ct, jp, cst, w.Hinv, w.Y, pt ? nude : nullptr, out, stats, s); });
  }
  return timed("jl_exp", s, [&] {
    return launch_jl_exp(h, n_ct, jp, sc, mode, pt ? nude : nullptr, table, w.slots, ops, cst, out, s);
  });
}

// ServerKey.decrypt's last step with a caller-computed factor (fbm_jl_powmod, pt == NULL):
// x = ((prod_u cts[u] * factor mod N^2) - 1) // N mod N
int fbm_jl_decrypt_with(const uint32_t* cts, int n_parties, uint64_t n_ct, const uint32_t* biprime,
                        const uint32_t* factor, uint32_t* x, void* workspace, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if ((rc = jl_agg_checks(n_parties, n_ct, biprime, 1))) return rc;
  if (n_ct == 0) return FBM_OK;
  if (!cts || !factor || !x || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return jl_combine_impl(cts, n_parties, n_ct, 1, 1, 0, biprime, factor, 1, 0.0, 1.0, nullptr, FBM_F64, nullptr,
                         agg_ws(workspace, n_ct), stats, s, x);
}

int fbm_int_ops(const uint64_t* x, uint64_t n, uint64_t k, int op, void* out, uint32_t* stats, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = zero_stats(stats, s);
  if (rc) return rc;
  if (op < 0 || op > 3 || ((op == 1 || op == 3) && k == 0)) {
    set_error("fbm_int_ops: op must be 0 (multiply), 1 / 3 (divide by k / -k, k >= 1) or 2 (divide by a float64)");
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!x || !out) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("int_ops", s, [&] {
    return launch_int_ops(x, n, k, op, op == 0 ? (uint64_t*)out : nullptr, op != 0 ? (double*)out : nullptr, stats, s);
  });
}

int fbm_ves_pack(const uint32_t* x, uint64_t n, int wv, int es, int cr, int pw, int is_signed, uint32_t* pt,
                 void* stream) {
  if (wv < 1 || es < 1 || cr < 1 || pw < 1 || (int64_t)es * (cr - 1) + 32ll * wv > 32ll * pw) {
    set_error("fbm_ves_pack: bad shape (wv=%d es=%d cr=%d pw=%d)", wv, es, cr, pw);
    return FBM_E_ARG;
  }
  if (n > 0 && (!x || !pt)) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("ves_pack", (hipStream_t)stream,
               [&] { return launch_ves_pack(x, n, wv, es, cr, pw, is_signed ? 1 : 0, pt, (hipStream_t)stream); });
}

int fbm_ves_unpack(const uint32_t* pt, uint64_t n_ct, int pw, int es, int cr, uint64_t n_out, int ow, uint32_t* vals,
                   void* stream) {
  if (pw < 1 || es < 1 || cr < 1 || ow < (es + 31) / 32 || (int64_t)es * cr > 32ll * pw || n_out > n_ct * (uint64_t)cr) {
    set_error("fbm_ves_unpack: bad shape (pw=%d es=%d cr=%d ow=%d)", pw, es, cr, ow);
    return FBM_E_ARG;
  }
  if (n_out > 0 && (!pt || !vals)) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("ves_unpack", (hipStream_t)stream,
               [&] { return launch_ves_unpack(pt, pw, es, cr, n_out, ow, vals, (hipStream_t)stream); });
}

int fbm_int_true_div_big(const uint64_t* x, uint64_t n, const uint32_t* k, int k_words, int negative, double* out,
                         void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!k || k_words < 1) {
    set_error("fbm_int_true_div_big: null or empty divisor");
    return FBM_E_ARG;
  }
  int nz = 0;
  for (int i = 0; i < k_words; ++i) nz |= k[i] != 0u;
  if (!nz) {
    set_error("division by zero");
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!x || !out) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("int_ops", s, [&] { return launch_int_true_div_big(x, n, k, k_words, negative ? 1 : 0, out, s); });
}

int fbm_jl_batch_begin(void) { return jl_batch_begin(); }

void fbm_jl_batch_abort(void) { jl_batch_abort(); }

int fbm_jl_batch_count(void) { return jl_batch_count(); }

uint64_t fbm_jl_batch_workspace(void) { return jl_batch_workspace(); }

int fbm_jl_batch_flush(void* workspace, uint64_t workspace_bytes, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  return timed("jl_exp", s, [&] { return jl_batch_flush(workspace, workspace_bytes, s); });
}

int fbm_ass_split(const void* secret, int secret_dtype, uint64_t n, int n_shares, int bit_length,
                  const uint8_t* seed, const uint8_t* nonce, uint64_t elem_offset, int64_t* shares, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_shares < 1 || bit_length > 64 || !seed || !nonce || (secret_dtype != FBM_U64 && secret_dtype != FBM_I64)) {
    set_error("invalid additive-sharing arguments (n_shares >= 1, bit_length <= 64, 64-bit secrets)");
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!secret || !shares) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  uint32_t key[8], nw[2];
  memcpy(key, seed, 32);
  memcpy(nw, nonce, 8);
  return timed("ass_split", s, [&] {
    return launch_ass_split((const uint64_t*)secret, n, key, nw[0], nw[1], elem_offset, n_shares, bit_length,
                            secret_dtype == FBM_I64, shares, s);
  });
}

int fbm_ass_reconstruct(const int64_t* shares, int n_shares, uint64_t n, int64_t* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_shares < 1) {
    set_error("n_shares must be >= 1");
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!shares || !out) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("ass_reconstruct", s, [&] { return launch_ass_reconstruct(shares, n_shares, n, out, s); });
}

int fbm_ass_split_wide(const uint32_t* secret, uint64_t n, int l_in, int n_shares, int bit_length, int l_out,
                       const uint8_t* seed, const uint8_t* nonce, uint64_t elem_offset, uint32_t* shares,
                       void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const int bmax = bit_length >= 0 ? bit_length : 32 * l_in;
  int pbits = 0;
  while ((1ll << pbits) < (long long)n_shares) ++pbits;
  if (n_shares < 1 || l_in < 1 || l_in > 4096 || l_out < l_in || !seed || !nonce ||
      32ll * l_out < (long long)bmax + pbits + 2 || bmax > (1 << 20)) {
    set_error("invalid wide additive-sharing arguments (n_shares >= 1, 1 <= l_in <= l_out, "
              "32*l_out >= bits + ceil(log2 n_shares) + 2)");
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!secret || !shares) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  uint32_t key[8], nw[2];
  memcpy(key, seed, 32);
  memcpy(nw, nonce, 8);
  return timed("ass_split_wide", s, [&] {
    return launch_ass_split_wide(secret, n, l_in, key, nw[0], nw[1], elem_offset, n_shares, bit_length, l_out,
                                 shares, s);
  });
}

int fbm_ass_reconstruct_wide(const uint32_t* shares, int n_shares, int l, uint64_t n, uint32_t* out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_shares < 1 || l < 1) {
    set_error("n_shares and l must be >= 1");
    return FBM_E_ARG;
  }
  if (n == 0) return FBM_OK;
  if (!shares || !out) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  return timed("ass_reconstruct_wide", s,
               [&] { return launch_ass_reconstruct_wide(shares, n_shares, l, n, out, s); });
}

// ---- the reference Serializer's update bytes (serializer.py:96-110 / :140-149) -----------------------
static bool wire_scheme(int scheme) { return scheme == FBM_WIRE_JL || scheme == FBM_WIRE_LOM; }

uint64_t fbm_wire_encode_bound(int scheme, uint64_t n) {
  return !wire_scheme(scheme) ? 0 : 5 + n * (scheme == FBM_WIRE_JL ? FBM_WIRE_ITEM_MAX + 1 : FBM_WIRE_NATIVE_MAX);
}

uint64_t fbm_wire_encode_workspace(int scheme, uint64_t n) {
  return wire_scheme(scheme) ? wire_encode_workspace(scheme, n) : 0;
}

// the checks fbm_wire_encode and its host hook share
static int wire_encode_checks(int scheme, const void* rows, uint64_t n, const uint8_t* out, uint64_t out_cap,
                              const uint64_t* total) {
  if (!wire_scheme(scheme)) {
    set_error("fbm_wire_encode: scheme=%d must be FBM_WIRE_JL or FBM_WIRE_LOM", scheme);
    return FBM_E_ARG;
  }
  if (n > 0xffffffffull) {
    set_error("fbm_wire_encode: %llu items exceed a msgpack array", (unsigned long long)n);
    return FBM_E_ARG;
  }
  if (!out || !total || (n > 0 && !rows)) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  if (out_cap < fbm_wire_encode_bound(scheme, n)) {
    set_error("fbm_wire_encode: out_cap=%llu below fbm_wire_encode_bound's %llu", (unsigned long long)out_cap,
              (unsigned long long)fbm_wire_encode_bound(scheme, n));
    return FBM_E_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(rows) % (scheme == FBM_WIRE_JL ? 4 : 8)) || (reinterpret_cast<uintptr_t>(total) % 8)) {
    set_error("fbm_wire_encode: rows / total not aligned to their element size");
    return FBM_E_ARG;
  }
  return FBM_OK;
}

int fbm_wire_encode(int scheme, const void* rows, uint64_t n, uint8_t* out, uint64_t out_cap, void* workspace,
                    uint64_t* total, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = wire_encode_checks(scheme, rows, n, out, out_cap, total);
  if (rc) return rc;
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) % 8)) {
    set_error("fbm_wire_encode: null or misaligned workspace");
    return FBM_E_ARG;
  }
  return timed("wire_encode", s, [&] { return launch_wire_encode(scheme, rows, n, out, out_cap, workspace, total, s); });
}

int fbm_wire_scan(const uint8_t* data, uint64_t len, uint64_t min_items, fbm_wire_array* arrays, uint64_t arrays_cap,
                  uint64_t* n_arrays, uint64_t* ckpt, uint64_t ckpt_cap, uint64_t* n_ckpt) {
  if ((len > 0 && !data) || !n_arrays || !n_ckpt || (arrays_cap > 0 && !arrays) || (ckpt_cap > 0 && !ckpt)) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  fbm_wire_scan_out o = {arrays, arrays_cap, 0, ckpt, ckpt_cap, 0};
  const int r = fbm_wire_scan_impl(data, len, min_items, &o);
  *n_arrays = o.n_arrays, *n_ckpt = o.n_ckpt;
  if (r == FBM_WIRE_SCAN_GAVE_UP) {
    set_error("fbm_wire_scan: not one well-formed msgpack object within the nesting bound");
    return FBM_E_UNSUPPORTED;
  }
  if (r == FBM_WIRE_SCAN_FULL) {
    set_error("fbm_wire_scan: arrays_cap / ckpt_cap too small");
    return FBM_E_RANGE;
  }
  return FBM_OK;
}

static int wire_decode_checks(int scheme, const uint8_t* span, const uint64_t* ckpt, uint64_t n_ckpt, uint64_t n_items,
                              const void* rows) {
  if (!wire_scheme(scheme)) {
    set_error("fbm_wire_decode: scheme=%d must be FBM_WIRE_JL or FBM_WIRE_LOM", scheme);
    return FBM_E_ARG;
  }
  const uint64_t want = scheme == FBM_WIRE_JL ? n_items : (n_items + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP;
  if (n_ckpt != want) {
    set_error("fbm_wire_decode: %llu checkpoints for %llu items (the scheme takes %llu)", (unsigned long long)n_ckpt,
              (unsigned long long)n_items, (unsigned long long)want);
    return FBM_E_ARG;
  }
  if (n_items > 0 && (!span || !ckpt || !rows)) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(ckpt) % 8) || (reinterpret_cast<uintptr_t>(rows) % (scheme == FBM_WIRE_JL ? 4 : 8))) {
    set_error("fbm_wire_decode: ckpt / rows not aligned to their element size");
    return FBM_E_ARG;
  }
  return FBM_OK;
}

int fbm_wire_decode(int scheme, const uint8_t* span, uint64_t span_len, uint64_t span_base, const uint64_t* ckpt,
                    uint64_t n_ckpt, uint64_t n_items, void* rows, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = wire_decode_checks(scheme, span, ckpt, n_ckpt, n_items, rows);
  if (rc) return rc;
  if (n_items == 0) return FBM_OK;
  return timed("wire_decode", s,
               [&] { return launch_wire_decode(scheme, span, span_len, span_base, ckpt, n_ckpt, n_items, rows, s); });
}

// the checks fbm_wire_fold_lom and its host hook share (n_items > 0)
static int wire_fold_lom_checks(const uint8_t* span, const uint64_t* ckpt, uint64_t n_ckpt, uint64_t n_items,
                                const uint64_t* acc) {
  if (!span || !ckpt || !acc) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const uint64_t want = (n_items + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP;
  if (n_ckpt != want) {
    set_error("fbm_wire_fold_lom: %llu checkpoints for %llu items (one per %d items: %llu)", (unsigned long long)n_ckpt,
              (unsigned long long)n_items, FBM_WIRE_LOM_GROUP, (unsigned long long)want);
    return FBM_E_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(ckpt) % 8) || (reinterpret_cast<uintptr_t>(acc) % 8)) {
    set_error("fbm_wire_fold_lom: ckpt / acc not aligned to 8 bytes");
    return FBM_E_ARG;
  }
  if ((n_ckpt + 3) / 4 > 0x7fffffffull) {  // four groups per workgroup (launch_wire_fold_lom checks it again)
    set_error("fbm_wire_fold_lom: %llu items exceed one launch's grid", (unsigned long long)n_items);
    return FBM_E_UNSUPPORTED;
  }
  return FBM_OK;
}

int fbm_wire_fold_lom(const uint8_t* span, uint64_t span_len, uint64_t span_base, const uint64_t* ckpt, uint64_t n_ckpt,
                      uint64_t n_items, uint64_t* acc, int first, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_items == 0) return FBM_OK;
  int rc = wire_fold_lom_checks(span, ckpt, n_ckpt, n_items, acc);
  if (rc) return rc;
  return timed("wire_fold_lom", s,
               [&] { return launch_wire_fold_lom(span, span_len, span_base, ckpt, n_ckpt, n_items, acc, first, s); });
}

uint64_t fbm_wire_tokenize_workspace(uint64_t span_len) { return wire_tokenize_workspace(span_len); }

// the checks fbm_wire_tokenize_lom / fbm_wire_tokenize_jl and their host hooks share (n_items > 0); `group`: items per
// table word.  (The messages name the LOM entry point for both.)
static int wire_tokenize_checks(const uint8_t* span, uint64_t span_len, uint64_t span_base, uint64_t first, uint64_t n_items,
                                const uint64_t* ckpt, uint64_t n_ckpt, const uint64_t* result, const void* workspace,
                                int group = FBM_WIRE_LOM_GROUP) {
  if (!span || !ckpt || !result || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const uint64_t want = (n_items + group - 1) / group;
  if (n_ckpt != want) {
    set_error("fbm_wire_tokenize_lom: %llu checkpoints for %llu items (one per %d items: %llu)", (unsigned long long)n_ckpt,
              (unsigned long long)n_items, group, (unsigned long long)want);
    return FBM_E_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(ckpt) % 8) || (reinterpret_cast<uintptr_t>(result) % 8) ||
      (reinterpret_cast<uintptr_t>(workspace) % 8)) {
    set_error("fbm_wire_tokenize_lom: ckpt / result / workspace not aligned to 8 bytes");
    return FBM_E_ARG;
  }
  if (first < span_base || first - span_base >= span_len) {
    set_error("fbm_wire_tokenize_lom: first=%llu outside the span [%llu, %llu + %llu)", (unsigned long long)first,
              (unsigned long long)span_base, (unsigned long long)span_base, (unsigned long long)span_len);
    return FBM_E_ARG;
  }
  if (n_items > 0xffffffffull) {
    set_error("fbm_wire_tokenize_lom: %llu items exceed a msgpack array", (unsigned long long)n_items);
    return FBM_E_UNSUPPORTED;
  }
  if (span_len > (1ull << 62) || !wire_tokenize_fits(span_len)) {
    set_error("fbm_wire_tokenize_lom: a span of %llu bytes exceeds one launch's grid", (unsigned long long)span_len);
    return FBM_E_UNSUPPORTED;
  }
  return FBM_OK;
}

int fbm_wire_tokenize_lom(const uint8_t* span, uint64_t span_len, uint64_t span_base, uint64_t first, uint64_t n_items,
                          uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_items == 0) return FBM_OK;
  int rc = wire_tokenize_checks(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace);
  if (rc) return rc;
  return timed("wire_tokenize_lom", s, [&] {
    return launch_wire_tokenize_lom(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace, s);
  });
}

uint64_t fbm_wire_tokenize_jl_workspace(uint64_t span_len) { return wire_tokenize_jl_workspace(span_len); }

int fbm_wire_tokenize_jl(const uint8_t* span, uint64_t span_len, uint64_t span_base, uint64_t first, uint64_t n_items,
                         uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (n_items == 0) return FBM_OK;
  int rc = wire_tokenize_checks(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace, 1);
  if (rc) return rc;
  return timed("wire_tokenize_jl", s, [&] {
    return launch_wire_tokenize_jl(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace, s);
  });
}

int fbm_wire_scan_deferred(const uint8_t* data, uint64_t len, uint64_t min_items, uint64_t defer_items,
                           const uint64_t* resolved, uint64_t n_resolved, fbm_wire_array* arrays, uint64_t arrays_cap,
                           uint64_t* n_arrays, uint64_t* ckpt, uint64_t ckpt_cap, uint64_t* n_ckpt,
                           fbm_wire_pending* pending) {
  fbm_wire_pending2 p2 = {0, 0, 0, 0, 0};
  const int rc = fbm_wire_scan_deferred2(data, len, min_items, defer_items, 0, resolved, n_resolved, arrays, arrays_cap,
                                         n_arrays, ckpt, ckpt_cap, n_ckpt, defer_items > 0 && !pending ? nullptr : &p2);
  if (rc == FBM_WIRE_PENDING) pending->begin = p2.begin, pending->first = p2.first, pending->n_items = p2.n_items;
  return rc;
}

int fbm_wire_scan_deferred2(const uint8_t* data, uint64_t len, uint64_t min_items, uint64_t defer_items,
                            uint64_t defer_items_jl, const uint64_t* resolved, uint64_t n_resolved,
                            fbm_wire_array* arrays, uint64_t arrays_cap, uint64_t* n_arrays, uint64_t* ckpt,
                            uint64_t ckpt_cap, uint64_t* n_ckpt, fbm_wire_pending2* pending) {
  if ((len > 0 && !data) || !n_arrays || !n_ckpt || (arrays_cap > 0 && !arrays) || (ckpt_cap > 0 && !ckpt) ||
      ((defer_items > 0 || defer_items_jl > 0) && (!pending || (n_resolved > 0 && !resolved)))) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  fbm_wire_scan_out o = {arrays, arrays_cap, 0, ckpt, ckpt_cap, 0};
  const fbm_wire_defer df = {defer_items, resolved, n_resolved, nullptr, defer_items_jl, pending};
  const int r = fbm_wire_scan_run(data, len, min_items, &o, &df);
  *n_arrays = o.n_arrays, *n_ckpt = o.n_ckpt;
  if (r == FBM_WIRE_SCAN_PENDING) return FBM_WIRE_PENDING;
  if (r == FBM_WIRE_SCAN_BAD_END) {
    set_error("fbm_wire_scan_deferred: a resolved end offset outside (first, len]");
    return FBM_E_ARG;
  }
  if (r == FBM_WIRE_SCAN_GAVE_UP) {
    set_error("fbm_wire_scan: not one well-formed msgpack object within the nesting bound");
    return FBM_E_UNSUPPORTED;
  }
  if (r == FBM_WIRE_SCAN_FULL) {
    set_error("fbm_wire_scan: arrays_cap / ckpt_cap too small");
    return FBM_E_RANGE;
  }
  return FBM_OK;
}

int fbm_wire_scan_prefix(const uint8_t* data, uint64_t len, uint64_t min_items, uint64_t defer_items_lom,
                         uint64_t defer_items_jl, fbm_wire_pending2* pending) {
  if ((len > 0 && !data) || !pending) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  const int r = fbm_wire_scan_prefix_run(data, len, min_items, defer_items_lom, defer_items_jl, pending);
  if (r == FBM_WIRE_SCAN_PENDING) return FBM_WIRE_PENDING;
  if (r == FBM_WIRE_SCAN_MORE) return FBM_WIRE_MORE;
  if (r == FBM_WIRE_SCAN_GAVE_UP) {
    set_error("fbm_wire_scan: not one well-formed msgpack object within the nesting bound");
    return FBM_E_UNSUPPORTED;
  }
  return FBM_OK;
}

}  // extern "C"

// The host's records of the streams fbm_wire_stream_begin opened on device states, under the state's address: a feed
// plans its launches from its record (the device's copy is not read back).  A begin on a state that has a record takes
// it over, the last feed frees it; with FBM_WIRE_STREAMS_OPEN unfinished streams open, a further begin takes the slot of
// the one begun longest ago (every record carries its begin's serial number) -- a stream that was begun and never fed
// to its end goes that way -- and a feed whose record is gone is FBM_E_ARG.
#define FBM_WIRE_STREAMS_OPEN 64
namespace {
struct wire_stream_rec {
  uint64_t* state;
  uint64_t begun;  // the serial number of its begin
  uint64_t rec[FBM_WIRE_STREAM_STATE_WORDS];
};
std::mutex g_wire_streams_mu;
wire_stream_rec g_wire_streams[FBM_WIRE_STREAMS_OPEN];
uint64_t g_wire_streams_begun = 0;

wire_stream_rec* wire_stream_find(uint64_t* state) {  // (the mutex held)
  for (auto& r : g_wire_streams)
    if (r.state == state) return &r;
  return nullptr;
}
}  // namespace

// the argument checks fbm_wire_stream_begin / _feed and their host hooks share
static int wire_stream_begin_checks(int scheme, uint64_t n_items, const uint64_t* state) {
  if (scheme != FBM_WIRE_JL && scheme != FBM_WIRE_LOM) {
    set_error("fbm_wire_stream_begin: scheme=%d must be FBM_WIRE_JL or FBM_WIRE_LOM", scheme);
    return FBM_E_ARG;
  }
  if (!state || reinterpret_cast<uintptr_t>(state) % 8) {
    set_error("fbm_wire_stream_begin: null or misaligned state");
    return FBM_E_ARG;
  }
  if (n_items == 0) {
    set_error("fbm_wire_stream_begin: an array without items has nothing to stream");
    return FBM_E_ARG;
  }
  if (n_items > 0xffffffffull) {
    set_error("fbm_wire_stream_begin: %llu items exceed a msgpack array", (unsigned long long)n_items);
    return FBM_E_UNSUPPORTED;
  }
  return FBM_OK;
}

static int wire_stream_feed_checks(int scheme, const uint8_t* span, uint64_t avail_len, const uint64_t* ckpt, uint64_t n_ckpt,
                                   const uint64_t* state, const void* workspace, const uint64_t* rec) {
  if (scheme != FBM_WIRE_JL && scheme != FBM_WIRE_LOM) {
    set_error("fbm_wire_stream_feed: scheme=%d must be FBM_WIRE_JL or FBM_WIRE_LOM", scheme);
    return FBM_E_ARG;
  }
  if (!span || !ckpt || !state || !workspace) {
    set_error("null pointer argument");
    return FBM_E_ARG;
  }
  if ((reinterpret_cast<uintptr_t>(ckpt) % 8) || (reinterpret_cast<uintptr_t>(state) % 8) || (reinterpret_cast<uintptr_t>(workspace) % 8)) {
    set_error("fbm_wire_stream_feed: ckpt / state / workspace not aligned to 8 bytes");
    return FBM_E_ARG;
  }
  if (!rec) {
    set_error("fbm_wire_stream_feed: no stream begun on this state");
    return FBM_E_ARG;
  }
  if (rec[FBM_WIRE_SEG_SCHEME] == (uint64_t)scheme + 1) {  // (any other: wire_seg_plan_of's refusal)
    const uint64_t n = rec[FBM_WIRE_SEG_ITEMS], group = scheme == FBM_WIRE_JL ? 1 : FBM_WIRE_LOM_GROUP;
    if (n_ckpt != (n + group - 1) / group) {
      set_error("fbm_wire_stream_feed: %llu checkpoints for %llu items (one per %llu items)", (unsigned long long)n_ckpt,
                (unsigned long long)n, (unsigned long long)group);
      return FBM_E_ARG;
    }
  }
  if (avail_len > (1ull << 62) || !wire_tokenize_fits(avail_len)) {
    set_error("fbm_wire_stream_feed: a span of %llu bytes exceeds one launch's grid", (unsigned long long)avail_len);
    return FBM_E_UNSUPPORTED;
  }
  return FBM_OK;
}

extern "C" {

uint64_t fbm_wire_stream_workspace(int scheme, uint64_t cap_len) {
  return scheme == FBM_WIRE_JL ? wire_tokenize_jl_workspace(cap_len) : wire_tokenize_workspace(cap_len);
}

int fbm_wire_stream_begin(int scheme, uint64_t first, uint64_t n_items, uint64_t* state, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  int rc = wire_stream_begin_checks(scheme, n_items, state);
  if (rc) return rc;
  rc = timed("wire_stream_begin", s, [&] { return launch_wire_stream_begin(scheme, first, n_items, state, s); });
  if (rc) return rc;
  std::lock_guard<std::mutex> lock(g_wire_streams_mu);
  wire_stream_rec* r = wire_stream_find(state);
  if (!r) r = wire_stream_find(nullptr);  // a free one
  if (!r) {  // the one begun longest ago
    r = &g_wire_streams[0];
    for (auto& q : g_wire_streams)
      if (q.begun < r->begun) r = &q;
  }
  r->state = state, r->begun = ++g_wire_streams_begun;
  wire_seg_begin(scheme, first, n_items, r->rec);
  return FBM_OK;
}

int fbm_wire_stream_feed(int scheme, const uint8_t* span, uint64_t span_base, uint64_t avail_len, int last, uint64_t* ckpt,
                         uint64_t n_ckpt, uint64_t* state, void* workspace, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  uint64_t rec[FBM_WIRE_STREAM_STATE_WORDS];
  bool have = false;
  {
    std::lock_guard<std::mutex> lock(g_wire_streams_mu);
    if (wire_stream_rec* r = state ? wire_stream_find(state) : nullptr) memcpy(rec, r->rec, sizeof rec), have = true;
  }
  int rc = wire_stream_feed_checks(scheme, span, avail_len, ckpt, n_ckpt, state, workspace, have ? rec : nullptr);
  if (rc) return rc;
  wire_seg_plan p;
  if (const char* err = wire_seg_plan_of(rec, scheme, span, span_base, avail_len, last, &p)) {
    set_error("fbm_wire_stream_feed: %s", err);
    return FBM_E_ARG;
  }
  if (p.hi > p.lo) {
    rc = timed("wire_stream_feed", s, [&] {
      return launch_wire_stream_feed(scheme, span, span_base, avail_len, last, ckpt, n_ckpt, state, workspace, rec, p, s);
    });
    if (rc) return rc;
  }
  wire_seg_fed(rec, p, span, span_base, avail_len, last);
  std::lock_guard<std::mutex> lock(g_wire_streams_mu);
  if (wire_stream_rec* r = wire_stream_find(state)) {
    if (last)
      r->state = nullptr;  // the stream is over: a further feed finds no record
    else
      memcpy(r->rec, rec, sizeof rec);
  }
  return FBM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------
// The test build's entry points (include/fbm_secagg_test.h; libfbm_secagg_test.so, compiled with
// -DFBM_TEST_HOOKS from this same file and linked with the same kernel objects): host runs of device
// routines, engine / short-path switches of the calling thread, engine and multiply counts, and the
// per-kernel event timer.  The product library (libfbm_secagg.so) exports none of them.
// ---------------------------------------------------------------------------------------
#ifdef FBM_TEST_HOOKS
extern "C" {

int fbm_test_wire_encode(int scheme, const void* rows, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* total) {
  int rc = wire_encode_checks(scheme, rows, n, out, out_cap, total);
  return rc ? rc : host_wire_encode(scheme, rows, n, out, out_cap, total);
}

int fbm_test_wire_decode(int scheme, const uint8_t* span, uint64_t span_len, uint64_t span_base, const uint64_t* ckpt,
                         uint64_t n_ckpt, uint64_t n_items, void* rows) {
  int rc = wire_decode_checks(scheme, span, ckpt, n_ckpt, n_items, rows);
  if (rc == FBM_OK && n_items) host_wire_decode(scheme, span, span_len, span_base, ckpt, n_ckpt, n_items, rows);
  return rc;
}

int fbm_test_wire_fold_lom(const uint8_t* span, uint64_t span_len, uint64_t span_base, const uint64_t* ckpt,
                           uint64_t n_ckpt, uint64_t n_items, uint64_t* acc, int first) {
  if (n_items == 0) return FBM_OK;
  int rc = wire_fold_lom_checks(span, ckpt, n_ckpt, n_items, acc);
  if (rc == FBM_OK) host_wire_fold_lom(span, span_len, span_base, ckpt, n_ckpt, n_items, acc, first);
  return rc;
}

int fbm_test_wire_tokenize_jl(const uint8_t* span, uint64_t span_len, uint64_t span_base, uint64_t first,
                              uint64_t n_items, uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  if (n_items == 0) return FBM_OK;
  int rc = wire_tokenize_checks(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace, 1);
  if (rc == FBM_OK) host_wire_tokenize_jl(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace);
  return rc;
}

int fbm_test_wire_tokenize_lom(const uint8_t* span, uint64_t span_len, uint64_t span_base, uint64_t first,
                               uint64_t n_items, uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  if (n_items == 0) return FBM_OK;
  int rc = wire_tokenize_checks(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace);
  if (rc == FBM_OK) host_wire_tokenize_lom(span, span_len, span_base, first, n_items, ckpt, n_ckpt, result, workspace);
  return rc;
}

int fbm_test_wire_stream_begin(int scheme, uint64_t first, uint64_t n_items, uint64_t* state) {
  int rc = wire_stream_begin_checks(scheme, n_items, state);
  if (rc == FBM_OK) wire_seg_begin(scheme, first, n_items, state);
  return rc;
}

int fbm_test_wire_stream_feed(int scheme, const uint8_t* span, uint64_t span_base, uint64_t avail_len, int last,
                              uint64_t* ckpt, uint64_t n_ckpt, uint64_t* state, void* workspace) {
  int rc = wire_stream_feed_checks(scheme, span, avail_len, ckpt, n_ckpt, state, workspace, state);
  if (rc) return rc;
  if (const char* err = wire_seg_host_feed(scheme, span, span_base, avail_len, last, ckpt, n_ckpt, state, workspace)) {
    set_error("fbm_wire_stream_feed: %s", err);
    return FBM_E_ARG;
  }
  return FBM_OK;
}

int fbm_jl_window(void) { return FBM_WIN; }
int fbm_jl_mads(int square) {  // 0: general product, 1: square, 2: short-base product
  return square == 2 ? FBM_NA_MADS_SHORT : square ? FBM_NA_MADS_SQR : FBM_NA_MADS_MUL;
}
int fbm_jl_quad_mads(int square) {
  return 4 * (square == 2 ? FBM_QA_MADS_SHORT : square ? FBM_QA_MADS_SQR : FBM_QA_MADS_MUL);
}
int fbm_jl_triple_mads(int square) {
  return 3 * (square == 2 ? FBM_TA_MADS_SHORT : square ? FBM_TA_MADS_SQR : FBM_TA_MADS_MUL);
}

int fbm_jl_set_engine(int mode) {
  if (mode != FBM_ENGINE_AUTO && mode != FBM_ENGINE_SINGLE && mode != FBM_ENGINE_GENERIC && mode != FBM_ENGINE_QUAD &&
      mode != FBM_ENGINE_TRIPLE) {
    set_error("fbm_jl_set_engine: mode must be 0 (auto), 1 (one lane per ciphertext), 2 (generic: any modulus), "
              "3 (three lanes) or 4 (four)");
    return FBM_E_ARG;
  }
  return jl_engine_set(mode);
}

int fbm_jl_engine_for(uint64_t n_ct) { return jl_engine_for(n_ct); }

int fbm_jl_set_chain(int percall) { return jl_chain_set(percall); }

int fbm_jl_set_split(int on) { return jl_split_set(on); }

int fbm_jl_set_short(int on) {
  const int prev = t_short_on;
  t_short_on = on ? 1 : 0;
  return prev;
}

int fbm_test_short_cache(uint32_t* out, int cap_words) {
  const int need = short_cache_dump(out, cap_words);
  if (out && cap_words < need) {
    set_error("fbm_test_short_cache: %d words needed", need);
    return FBM_E_ARG;
  }
  return need;
}

int fbm_test_true_div_big(const uint64_t* x, uint64_t n, const uint32_t* k, int k_words, int negative, double* out) {
  if (!k || k_words < 1 || (n > 0 && (!x || !out))) {
    set_error("fbm_test_true_div_big: bad arguments");
    return FBM_E_ARG;
  }
  host_true_div_big(x, n, k, k_words, negative, out);
  return FBM_OK;
}

int fbm_test_true_div_u128(const uint64_t* x, uint64_t n, uint64_t k, double* out) {
  if (k == 0 || (n > 0 && (!x || !out))) {
    set_error("fbm_test_true_div_u128: null pointer or zero divisor");
    return FBM_E_ARG;
  }
  for (uint64_t i = 0; i < n; ++i)
    out[i] = fbm_true_div_u128(((unsigned __int128)x[2 * i + 1] << 64) | x[2 * i], k);
  return FBM_OK;
}

int fbm_test_widen16(uint16_t bits, int dtype, double* out) {
  if (!out || (dtype != FBM_F16 && dtype != FBM_BF16)) {
    set_error("fbm_test_widen16: dtype must be FBM_F16 or FBM_BF16, out not NULL");
    return FBM_E_ARG;
  }
  if (dtype == FBM_F16) {
    const fbm_f16 h{bits};
    *out = fbm_widen(h);
  } else {
    const fbm_bf16 h{bits};
    *out = fbm_widen(h);
  }
  return FBM_OK;
}

int fbm_test_narrow(double v, int dtype, uint32_t* bits_out) {
  if (!bits_out || (dtype != FBM_F32 && dtype != FBM_F16 && dtype != FBM_BF16)) {
    set_error("fbm_test_narrow: dtype must be FBM_F32, FBM_F16 or FBM_BF16, bits_out not NULL");
    return FBM_E_ARG;
  }
  *bits_out = dtype == FBM_F32 ? fbm_out<float>::bits(v)
                               : dtype == FBM_F16 ? (uint32_t)fbm_out<fbm_f16>::bits(v) : (uint32_t)fbm_out<fbm_bf16>::bits(v);
  return FBM_OK;
}

int fbm_test_fdh_gcd(const uint32_t* r8, const uint32_t* n32, uint32_t* err) {
  if (!r8 || !n32 || !err || !(n32[0] & 1u)) {
    set_error("fbm_test_fdh_gcd: null pointer or even modulus");
    return FBM_E_ARG;
  }
  return host_gcd_is_one_r8(r8, n32, err);
}

int fbm_test_gen_exp(const uint32_t* h, const uint32_t* pt, int negative, const uint32_t* biprime, const uint32_t* key,
                     int key_negative, uint32_t* out, uint32_t* err) {
  if (!h || !biprime || !key || !out || !err) {
    set_error("fbm_test_gen_exp: null pointer");
    return FBM_E_ARG;
  }
  GenCtx g;
  const int rc = build_gen_ctx(biprime, key, key_negative, g);
  if (rc) return rc;
  *err = host_gen_exp(h, pt, negative, g, out);
  return FBM_OK;
}

int fbm_test_gen_combine(const uint32_t* cts, int n_parties, const uint32_t* factor, const uint32_t* biprime,
                         int mode, uint32_t* out, uint32_t* err) {
  if (!cts || n_parties < 1 || !biprime || !out || !err || (mode != FBM_GEN_PRODUCT && mode != FBM_GEN_DECRYPT)) {
    set_error("fbm_test_gen_combine: bad arguments");
    return FBM_E_ARG;
  }
  GenCtx g;
  const int rc = build_gen_ctx(biprime, nullptr, 0, g);
  if (rc) return rc;
  *err = host_gen_combine(cts, n_parties, factor, g, mode, out);
  return FBM_OK;
}

int fbm_test_nadic_consts(const uint32_t* n32, uint32_t* nk, uint32_t* r2na, uint32_t* r3na, uint32_t* np) {
  if (!n32 || !nk || !r2na || !r3na || !np) {
    set_error("fbm_test_nadic_consts: null pointer");
    return FBM_E_ARG;
  }
  JlParams jp;
  uint32_t tau1[FBM_TAU_LIMBS] = {1u};
  int rc = build_jl_params(n32, 34, 30, tau1, 0, jp);
  if (rc) return rc;
  memcpy(nk, jp.na.nk29, sizeof(jp.na.nk29));
  memcpy(r2na, jp.qa.r2, sizeof(jp.qa.r2));
  memcpy(r3na, jp.qa.r3, sizeof(jp.qa.r3));
  *np = jp.qa.np;
  return FBM_OK;
}

int fbm_test_short_consts(const uint32_t* n32, const uint32_t* key, uint32_t* kw, uint32_t* corr, uint32_t* d) {
  if (!n32 || !key || !kw || !corr || !d) {
    set_error("fbm_test_short_consts: null pointer");
    return FBM_E_ARG;
  }
  JlSched sc;
  int is_zero = 0;
  int rc = build_schedule(key, sc, is_zero);
  if (rc) return rc;
  JlShort sh;
  const bool q = build_short(n32, key, is_zero, sc, sh, true);
  memcpy(kw, sh.kw, sizeof(sh.kw));
  memcpy(corr, sh.corr, sizeof(sh.corr));
  memcpy(d, sh.d, sizeof(sh.d));
  return q ? sc.sbits : -2;
}

int fbm_test_split_consts(const uint32_t* n32, const uint32_t* key, uint32_t* k1w, uint32_t* k0w, uint32_t* c1,
                          uint32_t* cp, uint32_t* one, uint16_t* nops512, int* n_nops, int* nbn, int* win) {
  if (!n32 || !key || !k1w || !k0w || !c1 || !cp || !one || !nops512 || !n_nops || !nbn || !win) {
    set_error("fbm_test_split_consts: null pointer");
    return FBM_E_ARG;
  }
  JlSched sc;
  int is_zero = 0;
  int rc = build_schedule(key, sc, is_zero);
  if (rc) return rc;
  JlShort sh;
  const bool q = build_short(n32, key, is_zero, sc, sh, true);
  memcpy(k1w, sh.k1w, sizeof(sh.k1w));
  memcpy(k0w, sh.k0w, sizeof(sh.k0w));
  memcpy(c1, sh.c1, sizeof(sh.c1));
  memcpy(cp, sh.cp, sizeof(sh.cp));
  memcpy(one, sh.one, sizeof(sh.one));
  memcpy(nops512, sh.nop, sizeof(sh.nop));
  *n_nops = sc.n_nops;
  *nbn = sc.nbn;
  *win = FBM_WIN_N;
  wipe(&sh, sizeof(sh));
  return q ? sc.sb1 : -2;
}

int fbm_test_schedule(const uint32_t* key64, uint16_t* ops512, int* n_ops, int* first) {
  if (!key64 || !ops512 || !n_ops || !first) {
    set_error("fbm_test_schedule: null pointer");
    return FBM_E_ARG;
  }
  JlSched sc;
  int is_zero = 0;
  const int rc = build_schedule(key64, sc, is_zero);
  memcpy(ops512, sc.op, sizeof(sc.op));
  *n_ops = sc.n_ops;
  *first = sc.first;
  return rc ? rc : (is_zero ? 1 : FBM_OK);
}

int fbm_test_modinv(const uint32_t* x, const uint32_t* n, uint32_t* out, int* batches) {
  if (!x || !n || !out || !(n[0] & 1u)) {
    set_error("fbm_test_modinv: null pointer or even modulus");
    return FBM_E_ARG;
  }
  FbmN30 N;
  fbm_n30_setup(n, N);
  FbmInvState st;
  fbm_modinv_init(st, x, N);
  int b = 0;
  while (!fbm_s30_is_zero(st.g) && b < FBM_INV_MAX_BATCHES) {
    fbm_modinv_batch(st, N);
    ++b;
  }
  if (batches) *batches = b;
  if (!fbm_s30_is_zero(st.g)) {
    set_error("modular inverse did not converge");
    return FBM_E_ITER;
  }
  if (!fbm_modinv_finish(st, N, out)) {
    set_error("not invertible");
    return FBM_E_INVERSE;
  }
  return FBM_OK;
}

int fbm_test_lom_aggregate_kernel(int n_parties, uint64_t n, const void* y, char* buf, int len) {
  const int rc = lom_aggregate_kernel_name(n_parties, n, y, buf, len);
  if (rc) set_error("fbm_test_lom_aggregate_kernel: bad arguments or buffer too small");
  return rc;
}

int fbm_prof_enable(int on) {
  std::lock_guard<std::mutex> g(g_prof_mu);
  g_prof_on = on != 0;
  return FBM_OK;
}

// Synchronises the recorded events and writes "name count total_ms\n" lines (sorted by
// name) into buf; clears the records.  Returns the number of bytes needed.
int fbm_prof_report(char* buf, int len) {
  // Folds completed event pairs into g_prof_agg; the aggregate is only handed out (and
  // cleared) when buf can hold all of it, so a size query (buf == NULL) loses nothing.
  std::lock_guard<std::mutex> g(g_prof_mu);
  for (auto& r : g_prof) {
    float ms = 0.f;
    const bool ok = hipEventSynchronize(r.b) == hipSuccess && hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess;
    if (ok) {
      auto& e = g_prof_agg[r.name];
      e.first += 1;
      e.second += ms;
    }
    (void)hipEventDestroy(r.a);
    (void)hipEventDestroy(r.b);
  }
  g_prof.clear();
  std::string out;
  for (auto& kv : g_prof_agg) {
    char line[160];
    snprintf(line, sizeof(line), "%s %ld %.6f\n", kv.first.c_str(), kv.second.first, kv.second.second);
    out += line;
  }
  const int need = (int)out.size() + 1;
  if (buf && len >= need) {
    memcpy(buf, out.c_str(), (size_t)need);
    g_prof_agg.clear();
  }
  return need;
}

}  // extern "C"
#endif  // FBM_TEST_HOOKS

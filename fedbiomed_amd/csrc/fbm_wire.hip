// fedbiomed_amd -- the reference Serializer's update bytes, written and read on the device (gfx950).
//
// Encode (fedbiomed/common/serializer.py:96-110): JL rows [n, 64] u32 / LOM words [n] u64 -> the msgpack
// array the reference's packb writes for the same ints.
//   1. wire_sizes_*_kernel    each item's encoded size from its bit length; a tile's sum -> partial[tile]
//   2. wire_scan_kernel       exclusive scan of the tile sums (one workgroup) + the array header; the total
//   3. wire_emit_*_kernel     a tile's in-LDS scan gives every item its offset; header and big-endian bytes
// Item offsets are unaligned.  JL: one wave per item (<= 280 bytes): the bytes before the first 4-byte
// boundary and after the last go out as byte stores, every aligned dword between is composed by one lane
// from the row (which the L1 holds after the first touch) and stored whole -- <= 71 dword stores per item,
// consecutive lanes consecutive dwords.  LOM: a tile's items (<= 9 bytes each) are laid out in LDS at their
// tile-local offsets, then the tile's one contiguous span is copied out the same way (byte edges, aligned
// dwords between, consecutive lanes consecutive dwords).
// Algorithmic bytes per item: JL 4 (top limb, pass 1; a 64-byte sector in practice) + 2 + 2 (size) + 256
// read, <= 280 written; LOM 8 + 8 read (passes 1 and 3), <= 9 written.
//
// Decode (serializer.py:140-149), from the host scanner's checkpoints (fbm_wire_scan.hpp):
//   wire_decode_jl_kernel   one wave per item: lane j assembles limb j from the <= 257 big-endian bytes
//                           (byte loads of one contiguous run; 256-byte coalesced row store)
//   wire_decode_lom_kernel  one wave per group of FBM_WIRE_LOM_GROUP = 64 items: the group's <= 576 bytes
//                           into LDS with consecutive lanes on consecutive bytes, lane j walks j items
//                           there (every lane still walking reads the same LDS byte: a broadcast), one
//                           coalesced 512-byte store of the 64 words
//   wire_fold_lom_kernel    the same read side joined to lom_fold_kernel's accumulate side (fbm_wire_fold_lom):
//                           one wave per group, lane j adds its item to acc[g * 64 + j] -- one coalesced
//                           512-byte load of the accumulator (none on the first call) and one 512-byte
//                           store; the decoded words never reach HBM.  Algorithmic bytes per item:
//                           <= 9 + 1/8 (the table) + 8 read and 8 written when continuing, 8 fewer read on
//                           the first call.  Bound: HBM by these bytes; measured, the walk's instruction
//                           issue, as for wire_decode_lom_kernel.
//   wire_tok_*_kernel      the FBM_WIRE_LOM table itself, made on the device from the array's bytes
//                           (fbm_wire_tokenize_lom): see "tokenize" below
//   wire_tokj_*_kernel     the FBM_WIRE_JL table of an array of big-int maps (fbm_wire_tokenize_jl): "tokenize (JL)"
// Every read of the message is checked against its length and every write against the output's capacity,
// whatever the table holds.
#include "fbm_internal.hpp"
#include "fbm_wire.hpp"

namespace fbm {

#define FBM_WIRE_BLOCK 256
#define FBM_WIRE_TILE_JL 256                    // items per workgroup, one per thread in passes 1 and 3's scan
#define FBM_WIRE_LOM_PER_THREAD 4
#define FBM_WIRE_TILE_LOM (FBM_WIRE_BLOCK * FBM_WIRE_LOM_PER_THREAD)
#define FBM_WIRE_SCAN_THREADS 256

// exclusive scan of one value per thread over the workgroup's 256 threads; total = the tile's sum
__device__ __forceinline__ uint32_t wire_block_scan(uint32_t v, uint32_t* sh, uint32_t& total) {
  const int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int d = 1; d < FBM_WIRE_BLOCK; d <<= 1) {
    const uint32_t x = t >= d ? sh[t - d] : 0u;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const uint32_t incl = sh[t];
  total = sh[FBM_WIRE_BLOCK - 1];
  __syncthreads();
  return incl - v;
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_sizes_jl_kernel(const uint32_t* __restrict__ rows, uint64_t n,
                                                                       uint16_t* __restrict__ sz,
                                                                       uint64_t* __restrict__ partial) {
  __shared__ uint32_t sh[FBM_WIRE_BLOCK];
  const uint64_t i = (uint64_t)blockIdx.x * FBM_WIRE_TILE_JL + threadIdx.x;
  uint32_t s = 0;
  if (i < n) {
    const uint32_t* row = rows + i * 64;
    s = wire_jl_size(row, wire_jl_bits(row));
    sz[i] = (uint16_t)s;
  }
  uint32_t total;
  wire_block_scan(s, sh, total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_sizes_lom_kernel(const uint64_t* __restrict__ vals, uint64_t n,
                                                                        uint64_t* __restrict__ partial) {
  __shared__ uint32_t sh[FBM_WIRE_BLOCK];
  const uint64_t i0 = (uint64_t)blockIdx.x * FBM_WIRE_TILE_LOM + (uint64_t)threadIdx.x * FBM_WIRE_LOM_PER_THREAD;
  uint32_t s = 0;
#pragma unroll
  for (int e = 0; e < FBM_WIRE_LOM_PER_THREAD; ++e)
    if (i0 + e < n) s += wire_native_size(vals[i0 + e]);
  uint32_t total;
  wire_block_scan(s, sh, total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// partial[b] <- header size + sum of the tiles before b; the header's bytes; *total = the message's length
__global__ void __launch_bounds__(FBM_WIRE_SCAN_THREADS) wire_scan_kernel(uint64_t* __restrict__ partial, uint64_t nb,
                                                                          uint64_t n, uint8_t* __restrict__ out,
                                                                          uint64_t out_cap, uint64_t* __restrict__ total) {
  __shared__ uint64_t sh[FBM_WIRE_SCAN_THREADS];
  const int t = threadIdx.x;
  const uint64_t chunk = (nb + FBM_WIRE_SCAN_THREADS - 1) / FBM_WIRE_SCAN_THREADS;
  const uint64_t b0 = (uint64_t)t * chunk, b1 = b0 + chunk < nb ? b0 + chunk : nb;
  uint64_t s = 0;
  for (uint64_t b = b0; b < b1; ++b) s += partial[b];
  sh[t] = s;
  __syncthreads();
  for (int d = 1; d < FBM_WIRE_SCAN_THREADS; d <<= 1) {
    const uint64_t x = t >= d ? sh[t - d] : 0ull;
    __syncthreads();
    sh[t] += x;
    __syncthreads();
  }
  const uint32_t hdr = wire_header_size(n);
  uint64_t run = hdr + sh[t] - s;
  for (uint64_t b = b0; b < b1; ++b) {
    const uint64_t v = partial[b];
    partial[b] = run;
    run += v;
  }
  if (t == 0) {
    *total = hdr + sh[FBM_WIRE_SCAN_THREADS - 1];
    for (uint32_t k = 0; k < hdr && k < out_cap; ++k) out[k] = wire_header_byte(n, k);
  }
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_emit_jl_kernel(const uint32_t* __restrict__ rows, uint64_t n,
                                                                      const uint16_t* __restrict__ sz,
                                                                      const uint64_t* __restrict__ partial,
                                                                      uint8_t* __restrict__ out, uint64_t out_cap) {
  __shared__ uint32_t sh[FBM_WIRE_BLOCK];
  __shared__ uint32_t sh_off[FBM_WIRE_TILE_JL];
  __shared__ uint32_t sh_sz[FBM_WIRE_TILE_JL];
  const int t = threadIdx.x;
  const uint64_t tile0 = (uint64_t)blockIdx.x * FBM_WIRE_TILE_JL;
  const uint32_t s = tile0 + t < n ? sz[tile0 + t] : 0u;
  uint32_t total;
  sh_off[t] = wire_block_scan(s, sh, total);
  sh_sz[t] = s;
  __syncthreads();
  const uint64_t base = partial[blockIdx.x];
  const int wave = t >> 6, lane = t & 63;
  for (int it = wave; it < FBM_WIRE_TILE_JL; it += FBM_WIRE_BLOCK / 64) {
    const uint64_t i = tile0 + it;
    if (i >= n) break;
    const uint32_t S = sh_sz[it];
    const uint64_t p = base + sh_off[it];
    if (p > out_cap || out_cap - p < S) continue;  // (the caller's bound holds every item: never taken)
    const uint32_t* row = rows + i * 64;
    // the bit length, one limb per lane: the highest nonzero limb, then its width
    const uint64_t nz = __ballot(row[lane] != 0);
    int bits = 0;
    if (nz) {
      const int top = 63 - __builtin_clzll(nz);
      bits = 32 * top + 32 - __builtin_clz(row[top]);
    }
    uint8_t* o = out + p;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(o) & 3u);
    uint32_t head = mis ? 4u - mis : 0u;
    if (head > S) head = S;
    const uint32_t ndw = (S - head) / 4;
    const uint32_t tail0 = head + 4 * ndw;
    if ((uint32_t)lane < head) o[lane] = wire_jl_byte(row, bits, lane);
    for (uint32_t d = lane; d < ndw; d += 64) {
      const uint32_t k = head + 4 * d;
      const uint32_t w = (uint32_t)wire_jl_byte(row, bits, k) | ((uint32_t)wire_jl_byte(row, bits, k + 1) << 8) |
                         ((uint32_t)wire_jl_byte(row, bits, k + 2) << 16) | ((uint32_t)wire_jl_byte(row, bits, k + 3) << 24);
      *reinterpret_cast<uint32_t*>(o + k) = w;
    }
    if (tail0 + lane < S) o[tail0 + lane] = wire_jl_byte(row, bits, tail0 + lane);
  }
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_emit_lom_kernel(const uint64_t* __restrict__ vals, uint64_t n,
                                                                       const uint64_t* __restrict__ partial,
                                                                       uint8_t* __restrict__ out, uint64_t out_cap) {
  __shared__ uint32_t sh[FBM_WIRE_BLOCK];
  __shared__ uint8_t buf[FBM_WIRE_TILE_LOM * FBM_WIRE_NATIVE_MAX];
  const int t = threadIdx.x;
  const uint64_t i0 = (uint64_t)blockIdx.x * FBM_WIRE_TILE_LOM + (uint64_t)t * FBM_WIRE_LOM_PER_THREAD;
  uint64_t v[FBM_WIRE_LOM_PER_THREAD];
  uint32_t sz[FBM_WIRE_LOM_PER_THREAD], s = 0;
#pragma unroll
  for (int e = 0; e < FBM_WIRE_LOM_PER_THREAD; ++e) {
    v[e] = i0 + e < n ? vals[i0 + e] : 0ull;
    sz[e] = i0 + e < n ? wire_native_size(v[e]) : 0u;
    s += sz[e];
  }
  uint32_t total;
  uint32_t lo = wire_block_scan(s, sh, total);
#pragma unroll
  for (int e = 0; e < FBM_WIRE_LOM_PER_THREAD; ++e) {
    for (uint32_t k = 0; k < sz[e]; ++k) buf[lo + k] = wire_native_byte(v[e], sz[e], k);
    lo += sz[e];
  }
  __syncthreads();
  const uint64_t p = partial[blockIdx.x];
  if (p > out_cap || out_cap - p < total) return;  // (the caller's bound holds every tile: never taken)
  uint8_t* o = out + p;
  const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(o) & 3u);
  uint32_t head = mis ? 4u - mis : 0u;
  if (head > total) head = total;
  const uint32_t ndw = (total - head) / 4;
  const uint32_t tail0 = head + 4 * ndw;
  if ((uint32_t)t < head) o[t] = buf[t];
  for (uint32_t d = t; d < ndw; d += FBM_WIRE_BLOCK) {
    const uint32_t k = head + 4 * d;
    *reinterpret_cast<uint32_t*>(o + k) =
        (uint32_t)buf[k] | ((uint32_t)buf[k + 1] << 8) | ((uint32_t)buf[k + 2] << 16) | ((uint32_t)buf[k + 3] << 24);
  }
  if (tail0 + t < total) o[tail0 + t] = buf[tail0 + t];
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_decode_jl_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                        uint64_t base, const uint64_t* __restrict__ ckpt,
                                                                        uint64_t n, uint32_t* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * (FBM_WIRE_BLOCK / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (i >= n) return;
  const uint64_t c = ckpt[i];
  const uint64_t voff = c >> 16;
  const uint32_t vlen = (uint32_t)(c & 0xffff);
  uint32_t w = 0;
  if (voff >= base && voff - base <= span_len && span_len - (voff - base) >= vlen && vlen <= 257)
    w = wire_jl_limb(span + (voff - base), vlen, lane);
  rows[i * 64 + lane] = w;
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_decode_lom_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                         uint64_t base, const uint64_t* __restrict__ ckpt,
                                                                         uint64_t n_groups, uint64_t n,
                                                                         uint64_t* __restrict__ out) {
  constexpr int GB = FBM_WIRE_LOM_GROUP * FBM_WIRE_NATIVE_MAX;  // a group's bytes at most
  __shared__ uint8_t buf[FBM_WIRE_BLOCK / 64][GB];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t g = (uint64_t)blockIdx.x * (FBM_WIRE_BLOCK / 64) + wave;
  uint32_t avail = 0;
  if (g < n_groups) {
    const uint64_t c = ckpt[g];
    if (c >= base && c - base < span_len) {
      const uint64_t goff = c - base, left = span_len - goff;
      avail = left < (uint64_t)GB ? (uint32_t)left : (uint32_t)GB;
      for (uint32_t k = lane; k < avail; k += 64) buf[wave][k] = span[goff + k];
    }
  }
  __syncthreads();
  const uint64_t i = g * FBM_WIRE_LOM_GROUP + lane;
  if (g < n_groups && i < n) out[i] = wire_lom_group_item(buf[wave], avail, lane);
}

// acc[i] = (first ? 0 : acc[i]) + item i  mod 2^64.  A group whose checkpoint lies outside the span has avail = 0,
// so its items are 0: acc keeps its value (continuing) or becomes 0 (first).  acc is only 8-byte aligned.
__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_fold_lom_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                       uint64_t base, const uint64_t* __restrict__ ckpt,
                                                                       uint64_t n_groups, uint64_t n,
                                                                       uint64_t* __restrict__ acc, int first) {
  constexpr int GB = FBM_WIRE_LOM_GROUP * FBM_WIRE_NATIVE_MAX;  // a group's bytes at most
  __shared__ uint8_t buf[FBM_WIRE_BLOCK / 64][GB];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t g = (uint64_t)blockIdx.x * (FBM_WIRE_BLOCK / 64) + wave;
  const uint64_t i = g * FBM_WIRE_LOM_GROUP + lane;
  const bool mine = g < n_groups && i < n;
  uint64_t a = 0;
  if (mine && !first) a = acc[i];  // issued ahead of the group's bytes: in flight during the walk
  uint32_t avail = 0;
  if (g < n_groups) {
    const uint64_t c = ckpt[g];
    if (c >= base && c - base < span_len) {
      const uint64_t goff = c - base, left = span_len - goff;
      avail = left < (uint64_t)GB ? (uint32_t)left : (uint32_t)GB;
      for (uint32_t k = lane; k < avail; k += 64) buf[wave][k] = span[goff + k];
    }
  }
  __syncthreads();
  if (mine) acc[i] = a + wire_lom_group_item(buf[wave], avail, lane);
}

// ---- tokenize: the table of an all-native array made on the device (fbm_wire_tokenize_lom) ---------
// fbm_wire.hpp has the automaton and the stream's cut into sub-blocks and tiles.  Three launches:
//   1. wire_tok_maps_kernel   one wave per tile (4 KiB; four tiles per workgroup): the tile's aligned dwords into
//                             LDS, consecutive lanes consecutive dwords; lane j reads sub-block j's 16 words back
//                             (rows 17 words apart: 32 different banks) and walks them once, backwards, for its map;
//                             lanes 0..9 then follow one entry phase each through the 64 maps -> maps[tile]
//   2. wire_tok_scan_kernel   one workgroup: thread t composes its run of tiles' maps, thread 0 chains the 256 runs
//                             from the stream's entry phase, every thread then steps through its run again and
//                             writes each tile's entry state; the count of whole items -> result[0]
//   3. wire_tok_emit_kernel   pass 1's staging and maps again, the tile's entry state chained through them (every
//                             lane reads the same LDS word: a broadcast), then lane j walks its sub-block forwards
//                             from its own entry state: at most one group's first item and at most the last item
//                             start there -- one 8-byte store each
// Algorithmic bytes: the stream read twice, 48 bytes per tile written and read back, 8 per 64 items written.
// Bound: not HBM -- per 4 KiB tile a wave issues 64 backward steps of about 50 instructions in each of passes 1
// and 3, the forward walk in pass 3, and a chain of 64 dependent LDS reads; the scan kernel is its runs' dependent
// loads (DESIGN.md 4.2 has the measured times).
#define FBM_WIRE_TOK_WAVES (FBM_WIRE_BLOCK / 64)  // tiles per workgroup
#define FBM_WIRE_TOK_ROW 17                       // words between two sub-blocks in LDS
static_assert(FBM_WIRE_TOK_SUB == 64 && FBM_WIRE_TOK_SUBS == 64 && FBM_WIRE_LOM_GROUP == 64, "one lane per sub-block");
static_assert(FBM_WIRE_TOK_SCAN_THREADS == FBM_WIRE_SCAN_THREADS, "the host run cuts the tiles into the kernel's runs");

// a tile's words into sh_tile, then this lane's sub-block into w[16], its valid bytes and its map into sh_map;
// every wave of the workgroup comes through here (two barriers), a wave past the last tile on zeros
__device__ __forceinline__ int wire_tok_stage(const uint8_t* __restrict__ span, uint64_t span_len, int64_t tbase,
                                              uint32_t* sh_tile, uint16_t* sh_map, uint32_t* w) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int r = 0; r < FBM_WIRE_TOK_TILE / 4 / 64; ++r) {
    const int d = r * 64 + lane;
    const int64_t off = tbase + 4 * d;
    uint32_t v;
    if (off >= 0 && (uint64_t)off + 4 <= span_len)
      v = *reinterpret_cast<const uint32_t*>(span + off);  // (span + tbase is 4-byte aligned)
    else
      v = wire_tok_word(span, span_len, off);
    sh_tile[(d >> 4) * FBM_WIRE_TOK_ROW + (d & 15)] = v;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 16; ++i) w[i] = sh_tile[lane * FBM_WIRE_TOK_ROW + i];
  const int valid = wire_tok_valid(span_len, tbase + (int64_t)FBM_WIRE_TOK_SUB * lane);
  uint32_t g[9];
  wire_tok_block_map(w, valid, g);
#pragma unroll
  for (int p = 0; p < 9; ++p) sh_map[lane * FBM_WIRE_TOK_MAP + p] = (uint16_t)g[p];
  sh_map[lane * FBM_WIRE_TOK_MAP + 9] = (uint16_t)FBM_WIRE_TOK_BAD;
  __syncthreads();
  return valid;
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK, 4) wire_tok_maps_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                       int64_t origin, uint64_t tiles,
                                                                       uint32_t* __restrict__ maps) {
  __shared__ uint32_t sh_tile[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOK_SUBS * FBM_WIRE_TOK_ROW];
  __shared__ uint16_t sh_map[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOK_SUBS * FBM_WIRE_TOK_MAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t tile = (uint64_t)blockIdx.x * FBM_WIRE_TOK_WAVES + wave;
  uint32_t w[16];
  wire_tok_stage(span, span_len, origin + (int64_t)(tile * FBM_WIRE_TOK_TILE), sh_tile[wave], sh_map[wave], w);
  if (tile >= tiles || lane >= FBM_WIRE_TOK_MAP) return;
  uint64_t st = (uint64_t)lane;
#pragma unroll 1
  for (int t = 0; t < FBM_WIRE_TOK_SUBS; ++t) st = wire_tok_step(st, sh_map[wave] + t * FBM_WIRE_TOK_MAP);
  maps[tile * FBM_WIRE_TOK_MAP + lane] = (uint32_t)st;  // <= 4096 items << 4
}

// The scan of `tiles` maps by one workgroup: in() is the state in front of the first tile (thread 0 asks), out(st) takes
// the state behind the last (thread 0); every tile's entry state -> entry[].  wire_tok_scan_kernel and the resumable
// wire_seg_scan_lom_kernel differ in those two alone.
template <class In, class Out>
__device__ __forceinline__ void wire_tok_scan_body(const uint32_t* __restrict__ maps, uint64_t tiles, uint64_t* __restrict__ entry,
                                                   In in, Out out) {
  __shared__ uint64_t comp[FBM_WIRE_SCAN_THREADS][FBM_WIRE_TOK_MAP];
  __shared__ uint64_t ent[FBM_WIRE_SCAN_THREADS];
  const int t = threadIdx.x;
  uint64_t b0, b1;
  wire_tok_run(tiles, t, &b0, &b1);
  uint64_t run[9];
#pragma unroll
  for (int p = 0; p < 9; ++p) run[p] = (uint64_t)p;
  for (uint64_t b = b0; b < b1; ++b) {
#pragma unroll
    for (int p = 0; p < 9; ++p) run[p] = wire_tok_step(run[p], maps + b * FBM_WIRE_TOK_MAP);
  }
#pragma unroll
  for (int p = 0; p < 9; ++p) comp[t][p] = run[p];
  comp[t][9] = FBM_WIRE_TOK_BAD;
  __syncthreads();
  if (t == 0) {
    uint64_t st = in();
    for (int u = 0; u < FBM_WIRE_SCAN_THREADS; ++u) {
      ent[u] = st;
      st = wire_tok_step(st, comp[u]);
    }
    out(st);
  }
  __syncthreads();
  uint64_t st = ent[t];
  for (uint64_t b = b0; b < b1; ++b) {
    entry[b] = st;
    st = wire_tok_step(st, maps + b * FBM_WIRE_TOK_MAP);
  }
}

__global__ void __launch_bounds__(FBM_WIRE_SCAN_THREADS) wire_tok_scan_kernel(const uint32_t* __restrict__ maps, uint64_t tiles,
                                                                              uint32_t head, uint64_t n,
                                                                              uint64_t* __restrict__ entry,
                                                                              uint64_t* __restrict__ result) {
  wire_tok_scan_body(maps, tiles, entry, [&] { return (uint64_t)head; }, [&](uint64_t st) {
    result[0] = wire_tok_whole_items(st, n);
    result[1] = 0;  // wire_tok_emit_kernel writes the end where item n - 1 lies wholly inside the span
  });
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK, 4) wire_tok_emit_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                       int64_t origin, uint64_t tiles,
                                                                       const uint64_t* __restrict__ entry, uint64_t base,
                                                                       uint64_t n, uint64_t* __restrict__ ckpt,
                                                                       uint64_t n_ckpt, uint64_t* __restrict__ result) {
  __shared__ uint32_t sh_tile[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOK_SUBS * FBM_WIRE_TOK_ROW];
  __shared__ uint16_t sh_map[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOK_SUBS * FBM_WIRE_TOK_MAP];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t tile = (uint64_t)blockIdx.x * FBM_WIRE_TOK_WAVES + wave;
  const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
  uint32_t w[16];
  const int valid = wire_tok_stage(span, span_len, tbase, sh_tile[wave], sh_map[wave], w);
  if (tile >= tiles) return;
  uint64_t st = entry[tile], mine = 0;
#pragma unroll 1  // (unrolled, the 64 comparisons with the lane are all made first and outgrow the registers)
  for (int t = 0; t < FBM_WIRE_TOK_SUBS; ++t) {
    if (t == lane) mine = st;
    st = wire_tok_step(st, sh_map[wave] + t * FBM_WIRE_TOK_MAP);
  }
  if ((mine & 15) == FBM_WIRE_TOK_BAD) return;
  int ck, end;
  wire_tok_block_walk(sh_tile[wave] + lane * FBM_WIRE_TOK_ROW, valid, (uint32_t)(mine & 15), mine >> 4, n, &ck, &end);
  const int64_t sub = tbase + (int64_t)FBM_WIRE_TOK_SUB * lane;  // (an item starts at or behind `first`: sub + ck >= 0)
  if (ck >= 0) {
    const uint64_t group = ((mine >> 4) + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP;
    if (group < n_ckpt) ckpt[group] = base + (uint64_t)(sub + ck);
  }
  if (end >= 0 && (uint64_t)(sub + end) <= span_len) result[1] = base + (uint64_t)(sub + end);
}

// ---- tokenize (JL): the table of an array of big-int maps made on the device (fbm_wire_tokenize_jl) -----------
// fbm_wire.hpp has the item's step, the tile's transfer map and the running state.  The stream is cut into the LOM
// tokenizer's tiles (wire_tok_cut_of); one wave per tile, four tiles per workgroup.  Three launches:
//   1. wire_tokj_maps_kernel  the tile's aligned dwords and the 24 bytes behind it into LDS, consecutive lanes
//                             consecutive dwords; lane l tests the entry offsets l, l + 64, .. < 280 for the prefix
//                             (a ballot packs the <= 14 matches into slots) and follows the chain of each match
//                             through the tile -> maps[tile], 16 words
//   2. wire_tokj_scan_kernel  one workgroup: thread t follows every entry of its run's first tile through the run,
//                             thread 0 chains the 256 runs from the stream's entry offset, every thread then steps
//                             through its run again and writes each tile's entry state; the items -> result[0]
//   3. wire_tokj_emit_kernel  pass 1's staging again; lane 0 walks the tile's <= 179 items from its entry state and
//                             leaves their table words in LDS, the wave stores them as consecutive 8-byte words
// Algorithmic bytes: the stream read twice, 72 bytes per tile written and read back, 8 per item written.
// LDS: FBM_WIRE_TOK_WAVES staged tiles of FBM_WIRE_TOKJ_WORDS words (pass 1: 16512 bytes); pass 3 adds
// FBM_WIRE_TOKJ_ITEMS 8-byte words and two 4-byte words per wave (22272 bytes); pass 2 FBM_WIRE_TOKJ_SLOTS + 1 8-byte
// words per thread (34816 bytes).  Bound: not HBM -- a tile's chain is a dependent walk of about 15 items by one
// lane, each step seven LDS reads (DESIGN.md 4.2 has the measured times).
static_assert(FBM_WIRE_TOKJ_REACH <= 5 * 64, "five rounds of 64 lanes cover the entry offsets");

// a tile's words and the header bytes behind it into sh_tile; every wave of the workgroup comes through here (one
// barrier), a wave past the last tile on zeros.  span + tbase is 4-byte aligned.
__device__ __forceinline__ void wire_tokj_stage(const uint8_t* __restrict__ span, uint64_t span_len, int64_t tbase,
                                                uint32_t* sh_tile) {
  const int lane = threadIdx.x & 63;
  for (int d = lane; d < FBM_WIRE_TOKJ_WORDS; d += 64) {
    const int64_t off = tbase + 4 * d;
    uint32_t v;
    if (off >= 0 && (uint64_t)off + 4 <= span_len)
      v = *reinterpret_cast<const uint32_t*>(span + off);
    else
      v = wire_tok_word(span, span_len, off);
    sh_tile[d] = v;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_tokj_maps_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                        int64_t origin, uint64_t tiles,
                                                                        uint32_t* __restrict__ maps) {
  __shared__ uint32_t sh_tile[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOKJ_WORDS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t tile = (uint64_t)blockIdx.x * FBM_WIRE_TOK_WAVES + wave;
  const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
  wire_tokj_stage(span, span_len, tbase, sh_tile[wave]);
  if (tile >= tiles) return;  // (the whole wave)
  const uint32_t* w = sh_tile[wave];
  const int64_t left = (int64_t)span_len - tbase;
  uint32_t used = 0;
#pragma unroll 1
  for (int r = 0; r < (FBM_WIRE_TOKJ_REACH + 63) / 64; ++r) {
    const uint32_t e = (uint32_t)(r * 64 + lane);
    const bool match = e < FBM_WIRE_TOKJ_REACH && wire_tokj_prefix(w, e);
    const uint64_t found = __ballot(match);
    if (match) {
      const uint32_t slot = used + (uint32_t)__builtin_popcountll(found & ((1ull << lane) - 1ull));
      if (slot < FBM_WIRE_TOKJ_SLOTS) {  // (always: matches are 20 bytes apart)
        uint32_t items = 0;
        const uint32_t exit = wire_tokj_chain(w, e, left, &items);
        maps[tile * FBM_WIRE_TOKJ_SLOTS + slot] = wire_tokj_entry(e, exit, items);
      }
    }
    used += (uint32_t)__builtin_popcountll(found);
  }
  if (lane < FBM_WIRE_TOKJ_SLOTS && (uint32_t)lane >= used) maps[tile * FBM_WIRE_TOKJ_SLOTS + lane] = ~0u;
}

// (wire_tokj_scan_body: in() and out(st) as wire_tok_scan_body's; wire_tokj_scan_kernel and wire_seg_scan_jl_kernel)
template <class In, class Out>
__device__ __forceinline__ void wire_tokj_scan_body(const uint32_t* __restrict__ maps, uint64_t tiles, uint64_t* __restrict__ entry,
                                                    In in, Out out) {
  __shared__ uint64_t comp[FBM_WIRE_TOKJ_SLOTS][FBM_WIRE_SCAN_THREADS];  // [slot][thread]: consecutive threads, consecutive banks
  __shared__ uint64_t ent[FBM_WIRE_SCAN_THREADS];
  const int t = threadIdx.x;
  uint64_t b0, b1;
  wire_tok_run(tiles, t, &b0, &b1);
#pragma unroll 1
  for (int k = 0; k < FBM_WIRE_TOKJ_SLOTS; ++k) {
    uint64_t s = FBM_WIRE_TOKJ_GONE;
    if (b0 < b1) {
      const uint32_t m = maps[b0 * FBM_WIRE_TOKJ_SLOTS + k];
      if (m != ~0u) {
        s = (uint64_t)(m & 0x1ffu);
        for (uint64_t b = b0; b < b1 && (s & 0xffffull) != FBM_WIRE_TOKJ_GONE; ++b) s = wire_tokj_apply(s, maps + b * FBM_WIRE_TOKJ_SLOTS);
      }
    }
    comp[k][t] = s;
  }
  __syncthreads();
  if (t == 0) {
    uint64_t st = in();
    for (int u = 0; u < FBM_WIRE_SCAN_THREADS; ++u) {
      ent[u] = st;
      uint64_t c0, c1;
      wire_tok_run(tiles, u, &c0, &c1);
      if (c0 < c1) st = wire_tokj_apply_run(st, maps + c0 * FBM_WIRE_TOKJ_SLOTS, &comp[0][u], FBM_WIRE_SCAN_THREADS);
    }
    out(st);
  }
  __syncthreads();
  uint64_t st = ent[t];
  for (uint64_t b = b0; b < b1; ++b) {
    entry[b] = st;
    st = wire_tokj_apply(st, maps + b * FBM_WIRE_TOKJ_SLOTS);
  }
}

__global__ void __launch_bounds__(FBM_WIRE_SCAN_THREADS) wire_tokj_scan_kernel(const uint32_t* __restrict__ maps, uint64_t tiles,
                                                                               uint32_t head, uint64_t n,
                                                                               uint64_t* __restrict__ entry,
                                                                               uint64_t* __restrict__ result) {
  wire_tokj_scan_body(maps, tiles, entry, [&] { return (uint64_t)head; }, [&](uint64_t st) {
    result[0] = (st >> 16) < n ? (st >> 16) : n;
    result[1] = 0;  // wire_tokj_emit_kernel writes the end where item n - 1 is one of the chain's
  });
}

__global__ void __launch_bounds__(FBM_WIRE_BLOCK) wire_tokj_emit_kernel(const uint8_t* __restrict__ span, uint64_t span_len,
                                                                        int64_t origin, uint64_t tiles,
                                                                        const uint64_t* __restrict__ entry, uint64_t base,
                                                                        uint64_t n, uint64_t* __restrict__ ckpt,
                                                                        uint64_t n_ckpt, uint64_t* __restrict__ result) {
  __shared__ uint32_t sh_tile[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOKJ_WORDS];
  __shared__ uint64_t sh_out[FBM_WIRE_TOK_WAVES][FBM_WIRE_TOKJ_ITEMS];
  __shared__ int sh_meta[FBM_WIRE_TOK_WAVES][2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t tile = (uint64_t)blockIdx.x * FBM_WIRE_TOK_WAVES + wave;
  const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
  wire_tokj_stage(span, span_len, tbase, sh_tile[wave]);
  const uint64_t st = tile < tiles ? entry[tile] : FBM_WIRE_TOKJ_GONE;
  if (lane == 0) {
    int end = -1;
    const uint32_t cnt = wire_tokj_emit_walk(sh_tile[wave], st, (int64_t)span_len - tbase, (int64_t)base + tbase, n, sh_out[wave], &end);
    sh_meta[wave][0] = (int)cnt, sh_meta[wave][1] = end;
  }
  __syncthreads();
  const uint32_t cnt = (uint32_t)sh_meta[wave][0];
  const int end = sh_meta[wave][1];
  const uint64_t k0 = st >> 16;
  for (uint32_t j = lane; j < cnt; j += 64)
    if (k0 + j < n_ckpt) ckpt[k0 + j] = sh_out[wave][j];
  if (lane == 0 && end >= 0) result[1] = (uint64_t)((int64_t)base + tbase + end);
}

// ---- the tokenizers as resumable scans (fbm_wire_stream_feed) --------------------------------------------------
// fbm_wire.hpp has the stream's record and which tiles a feed runs.  A feed is the one-shot call's three launches over
// its tiles [lo, hi): the maps and emit kernels above, given tile lo's span offset as their origin, and between them a
// scan whose entry state is not the stream's `head` but the carry the last feed left in the record:
//   wire_seg_scan_lom_kernel / wire_seg_scan_jl_kernel   wire_tok_scan_kernel's / wire_tokj_scan_kernel's body with thread 0
//       reading its entry state from state[CARRY] (fresh: the stream's first tiles, `head`) and writing the state behind
//       the segment back there, result[0] beside it -- and leaving result[1] alone: wire_seg_begin_kernel zeroed it and
//       the one emit launch whose tiles hold item n - 1's start writes it
// LDS: the one-shot scans' (LOM 22528 bytes, JL 34816 bytes).  Bound: their runs' dependent loads, as the one-shot's.
__global__ void wire_seg_begin_kernel(uint64_t* __restrict__ state, uint64_t first, uint64_t n, uint64_t scheme) {
  const int t = threadIdx.x;
  if (t >= FBM_WIRE_STREAM_STATE_WORDS) return;
  state[t] = t == FBM_WIRE_SEG_FIRST ? first : t == FBM_WIRE_SEG_ITEMS ? n : t == FBM_WIRE_SEG_SCHEME ? scheme + 1 : 0ull;
}

// thread 0's bookkeeping behind a segment's scan
__device__ __forceinline__ void wire_seg_note(uint64_t* __restrict__ state, uint64_t st, uint64_t count, uint64_t fed,
                                              uint64_t tiles_done, int last) {
  state[FBM_WIRE_SEG_CARRY] = st;
  state[FBM_WIRE_SEG_RESULT] = count;
  state[FBM_WIRE_SEG_FED] = fed, state[FBM_WIRE_SEG_TILES] = tiles_done;
  if (last) state[FBM_WIRE_SEG_SCHEME] |= FBM_WIRE_SEG_DONE;
}

__global__ void __launch_bounds__(FBM_WIRE_SCAN_THREADS) wire_seg_scan_lom_kernel(const uint32_t* __restrict__ maps, uint64_t tiles,
                                                                                  uint32_t head, int fresh, uint64_t n,
                                                                                  uint64_t* __restrict__ entry,
                                                                                  uint64_t* __restrict__ state, uint64_t fed,
                                                                                  uint64_t tiles_done, int last) {
  wire_tok_scan_body(maps, tiles, entry, [&] { return fresh ? (uint64_t)head : state[FBM_WIRE_SEG_CARRY]; },
                     [&](uint64_t st) { wire_seg_note(state, st, wire_tok_whole_items(st, n), fed, tiles_done, last); });
}

__global__ void __launch_bounds__(FBM_WIRE_SCAN_THREADS) wire_seg_scan_jl_kernel(const uint32_t* __restrict__ maps, uint64_t tiles,
                                                                                 uint32_t head, int fresh, uint64_t n,
                                                                                 uint64_t* __restrict__ entry,
                                                                                 uint64_t* __restrict__ state, uint64_t fed,
                                                                                 uint64_t tiles_done, int last) {
  wire_tokj_scan_body(maps, tiles, entry, [&] { return fresh ? (uint64_t)head : state[FBM_WIRE_SEG_CARRY]; },
                      [&](uint64_t st) { wire_seg_note(state, st, (st >> 16) < n ? (st >> 16) : n, fed, tiles_done, last); });
}

static int wire_grid(uint64_t blocks, const char* what, unsigned& g) {
  if (blocks > 0x7fffffffull) {
    set_error("%s: %llu workgroups exceed one launch's grid", what, (unsigned long long)blocks);
    return FBM_E_UNSUPPORTED;
  }
  g = (unsigned)blocks;
  return FBM_OK;
}

static uint64_t wire_tiles(int scheme, uint64_t n) {
  const uint64_t tile = scheme == FBM_WIRE_JL ? FBM_WIRE_TILE_JL : FBM_WIRE_TILE_LOM;
  return (n + tile - 1) / tile;
}

// workspace: the tile sums (u64 each, rounded up to 256 bytes), then JL's item sizes (u16 each)
uint64_t wire_encode_workspace(int scheme, uint64_t n) {
  const uint64_t part = (wire_tiles(scheme, n) * 8 + 255) / 256 * 256 + 256;
  return part + (scheme == FBM_WIRE_JL ? (n * 2 + 255) / 256 * 256 : 0);
}

int launch_wire_encode(int scheme, const void* rows, uint64_t n, uint8_t* out, uint64_t out_cap, void* workspace,
                       uint64_t* total, hipStream_t s) {
  const uint64_t nb = wire_tiles(scheme, n);
  unsigned g = 0;
  int rc = wire_grid(nb, "fbm_wire_encode", g);
  if (rc) return rc;
  uint64_t* partial = reinterpret_cast<uint64_t*>(workspace);
  uint16_t* sz = reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(workspace) + (nb * 8 + 255) / 256 * 256 + 256);
  if (g) {
    if (scheme == FBM_WIRE_JL)
      hipLaunchKernelGGL(wire_sizes_jl_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, (const uint32_t*)rows, n, sz, partial);
    else
      hipLaunchKernelGGL(wire_sizes_lom_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, (const uint64_t*)rows, n, partial);
    if ((rc = check_launch("wire_sizes_kernel"))) return rc;
  }
  hipLaunchKernelGGL(wire_scan_kernel, dim3(1), dim3(FBM_WIRE_SCAN_THREADS), 0, s, partial, nb, n, out, out_cap, total);
  if ((rc = check_launch("wire_scan_kernel"))) return rc;
  if (g) {
    if (scheme == FBM_WIRE_JL)
      hipLaunchKernelGGL(wire_emit_jl_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, (const uint32_t*)rows, n, sz, partial, out,
                         out_cap);
    else
      hipLaunchKernelGGL(wire_emit_lom_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, (const uint64_t*)rows, n, partial, out,
                         out_cap);
    if ((rc = check_launch("wire_emit_kernel"))) return rc;
  }
  return FBM_OK;
}

int launch_wire_decode(int scheme, const uint8_t* span, uint64_t span_len, uint64_t base, const uint64_t* ckpt,
                       uint64_t n_ckpt, uint64_t n, void* rows, hipStream_t s) {
  if (n == 0) return FBM_OK;
  const uint64_t waves = scheme == FBM_WIRE_JL ? n : n_ckpt;
  unsigned g = 0;
  int rc = wire_grid((waves + FBM_WIRE_BLOCK / 64 - 1) / (FBM_WIRE_BLOCK / 64), "fbm_wire_decode", g);
  if (rc) return rc;
  if (scheme == FBM_WIRE_JL)
    hipLaunchKernelGGL(wire_decode_jl_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, base, ckpt, n,
                       (uint32_t*)rows);
  else
    hipLaunchKernelGGL(wire_decode_lom_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, base, ckpt, n_ckpt, n,
                       (uint64_t*)rows);
  return check_launch("wire_decode_kernel");
}

int launch_wire_fold_lom(const uint8_t* span, uint64_t span_len, uint64_t base, const uint64_t* ckpt, uint64_t n_ckpt,
                         uint64_t n, uint64_t* acc, int first, hipStream_t s) {
  if (n == 0) return FBM_OK;
  unsigned g = 0;
  int rc = wire_grid((n_ckpt + FBM_WIRE_BLOCK / 64 - 1) / (FBM_WIRE_BLOCK / 64), "fbm_wire_fold_lom", g);
  if (rc) return rc;
  hipLaunchKernelGGL(wire_fold_lom_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, base, ckpt, n_ckpt, n, acc,
                     first);
  return check_launch("wire_fold_lom_kernel");
}

uint64_t wire_tokenize_workspace(uint64_t span_len) {
  const uint64_t tiles = (span_len + 3 + FBM_WIRE_TOK_TILE - 1) / FBM_WIRE_TOK_TILE;  // whatever the alignment
  return wire_tok_maps_at(tiles) + (tiles * FBM_WIRE_TOK_MAP * 4 + 255) / 256 * 256 + 256;
}
// more workgroups than one launch's grid: the caller's check before any device call
bool wire_tokenize_fits(uint64_t span_len) {
  return ((span_len + 3 + FBM_WIRE_TOK_TILE - 1) / FBM_WIRE_TOK_TILE + FBM_WIRE_TOK_WAVES - 1) / FBM_WIRE_TOK_WAVES <= 0x7fffffffull;
}

int launch_wire_tokenize_lom(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                             uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace, hipStream_t s) {
  const wire_tok_cut c = wire_tok_cut_of(span, span_len, first - base);
  unsigned g = 0;
  int rc = wire_grid((c.tiles + FBM_WIRE_TOK_WAVES - 1) / FBM_WIRE_TOK_WAVES, "fbm_wire_tokenize_lom", g);
  if (rc) return rc;
  uint64_t* entry = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* maps = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(workspace) + wire_tok_maps_at(c.tiles));
  hipLaunchKernelGGL(wire_tok_maps_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, c.origin, c.tiles, maps);
  if ((rc = check_launch("wire_tok_maps_kernel"))) return rc;
  hipLaunchKernelGGL(wire_tok_scan_kernel, dim3(1), dim3(FBM_WIRE_SCAN_THREADS), 0, s, maps, c.tiles, c.head, n, entry, result);
  if ((rc = check_launch("wire_tok_scan_kernel"))) return rc;
  hipLaunchKernelGGL(wire_tok_emit_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, c.origin, c.tiles, entry, base,
                     n, ckpt, n_ckpt, result);
  return check_launch("wire_tok_emit_kernel");
}

uint64_t wire_tokenize_jl_workspace(uint64_t span_len) {
  const uint64_t tiles = (span_len + 3 + FBM_WIRE_TOK_TILE - 1) / FBM_WIRE_TOK_TILE;  // whatever the alignment
  return (wire_tokj_workspace_of(tiles) + 255) / 256 * 256 + 256;
}

int launch_wire_tokenize_jl(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                            uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace, hipStream_t s) {
  const wire_tok_cut c = wire_tok_cut_of(span, span_len, first - base);
  unsigned g = 0;
  int rc = wire_grid((c.tiles + FBM_WIRE_TOK_WAVES - 1) / FBM_WIRE_TOK_WAVES, "fbm_wire_tokenize_jl", g);
  if (rc) return rc;
  uint64_t* entry = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* maps = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(workspace) + wire_tok_maps_at(c.tiles));
  hipLaunchKernelGGL(wire_tokj_maps_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, c.origin, c.tiles, maps);
  if ((rc = check_launch("wire_tokj_maps_kernel"))) return rc;
  hipLaunchKernelGGL(wire_tokj_scan_kernel, dim3(1), dim3(FBM_WIRE_SCAN_THREADS), 0, s, maps, c.tiles, c.head, n, entry, result);
  if ((rc = check_launch("wire_tokj_scan_kernel"))) return rc;
  hipLaunchKernelGGL(wire_tokj_emit_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, span_len, c.origin, c.tiles, entry, base,
                     n, ckpt, n_ckpt, result);
  return check_launch("wire_tokj_emit_kernel");
}

int launch_wire_stream_begin(int scheme, uint64_t first, uint64_t n, uint64_t* state, hipStream_t s) {
  hipLaunchKernelGGL(wire_seg_begin_kernel, dim3(1), dim3(64), 0, s, state, first, n, (uint64_t)scheme);
  return check_launch("wire_seg_begin_kernel");
}

// one feed's launches: `rec` is the host's record of the stream, `p` its plan (wire_seg_plan_of) with p.hi > p.lo
int launch_wire_stream_feed(int scheme, const uint8_t* span, uint64_t base, uint64_t avail, int last, uint64_t* ckpt,
                            uint64_t n_ckpt, uint64_t* state, void* workspace, const uint64_t* rec, const wire_seg_plan& p,
                            hipStream_t s) {
  const uint64_t tiles = p.hi - p.lo, n = rec[FBM_WIRE_SEG_ITEMS];
  unsigned g = 0;
  int rc = wire_grid((tiles + FBM_WIRE_TOK_WAVES - 1) / FBM_WIRE_TOK_WAVES, "fbm_wire_stream_feed", g);
  if (rc) return rc;
  uint64_t* entry = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* maps = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(workspace) + wire_tok_maps_at(tiles));
  uint64_t* result = state + FBM_WIRE_SEG_RESULT;
  const int fresh = p.lo == 0;
  if (scheme == FBM_WIRE_JL) {
    hipLaunchKernelGGL(wire_tokj_maps_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, avail, p.origin, tiles, maps);
    if ((rc = check_launch("wire_tokj_maps_kernel"))) return rc;
    hipLaunchKernelGGL(wire_seg_scan_jl_kernel, dim3(1), dim3(FBM_WIRE_SCAN_THREADS), 0, s, maps, tiles, p.head, fresh, n, entry,
                       state, avail, p.hi, last);
    if ((rc = check_launch("wire_seg_scan_jl_kernel"))) return rc;
    hipLaunchKernelGGL(wire_tokj_emit_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, avail, p.origin, tiles, entry, base, n,
                       ckpt, n_ckpt, result);
    return check_launch("wire_tokj_emit_kernel");
  }
  hipLaunchKernelGGL(wire_tok_maps_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, avail, p.origin, tiles, maps);
  if ((rc = check_launch("wire_tok_maps_kernel"))) return rc;
  hipLaunchKernelGGL(wire_seg_scan_lom_kernel, dim3(1), dim3(FBM_WIRE_SCAN_THREADS), 0, s, maps, tiles, p.head, fresh, n, entry,
                     state, avail, p.hi, last);
  if ((rc = check_launch("wire_seg_scan_lom_kernel"))) return rc;
  hipLaunchKernelGGL(wire_tok_emit_kernel, dim3(g), dim3(FBM_WIRE_BLOCK), 0, s, span, avail, p.origin, tiles, entry, base, n, ckpt,
                     n_ckpt, result);
  return check_launch("wire_tok_emit_kernel");
}

// ---- the same per-item routines on the host (the test build's hooks) ------------------------------
int host_wire_encode(int scheme, const void* rows, uint64_t n, uint8_t* out, uint64_t out_cap, uint64_t* total) {
  uint64_t p = 0;
  const uint32_t hdr = wire_header_size(n);
  for (uint32_t k = 0; k < hdr; ++k, ++p)
    if (p < out_cap) out[p] = wire_header_byte(n, k);
  for (uint64_t i = 0; i < n; ++i) {
    if (scheme == FBM_WIRE_JL) {
      const uint32_t* row = (const uint32_t*)rows + i * 64;
      const int bits = wire_jl_bits(row);
      const uint32_t S = wire_jl_size(row, bits);
      for (uint32_t k = 0; k < S; ++k, ++p)
        if (p < out_cap) out[p] = wire_jl_byte(row, bits, k);
    } else {
      const uint64_t v = ((const uint64_t*)rows)[i];
      const uint32_t S = wire_native_size(v);
      for (uint32_t k = 0; k < S; ++k, ++p)
        if (p < out_cap) out[p] = wire_native_byte(v, S, k);
    }
  }
  *total = p;
  return p <= out_cap ? FBM_OK : FBM_E_ARG;
}

void host_wire_decode(int scheme, const uint8_t* span, uint64_t span_len, uint64_t base, const uint64_t* ckpt,
                      uint64_t n_ckpt, uint64_t n, void* rows) {
  if (scheme == FBM_WIRE_JL) {
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t voff = ckpt[i] >> 16;
      const uint32_t vlen = (uint32_t)(ckpt[i] & 0xffff);
      const bool ok = voff >= base && voff - base <= span_len && span_len - (voff - base) >= vlen && vlen <= 257;
      for (int j = 0; j < 64; ++j) ((uint32_t*)rows)[i * 64 + j] = ok ? wire_jl_limb(span + (voff - base), vlen, j) : 0u;
    }
    return;
  }
  constexpr uint64_t GB = FBM_WIRE_LOM_GROUP * FBM_WIRE_NATIVE_MAX;
  for (uint64_t g = 0; g < n_ckpt; ++g) {
    uint32_t avail = 0;
    const uint8_t* buf = span;
    if (ckpt[g] >= base && ckpt[g] - base < span_len) {
      const uint64_t left = span_len - (ckpt[g] - base);
      avail = (uint32_t)(left < GB ? left : GB);
      buf = span + (ckpt[g] - base);
    }
    for (int j = 0; j < FBM_WIRE_LOM_GROUP; ++j)
      if (g * FBM_WIRE_LOM_GROUP + j < n) ((uint64_t*)rows)[g * FBM_WIRE_LOM_GROUP + j] = wire_lom_group_item(buf, avail, j);
  }
}

void host_wire_fold_lom(const uint8_t* span, uint64_t span_len, uint64_t base, const uint64_t* ckpt, uint64_t n_ckpt,
                        uint64_t n, uint64_t* acc, int first) {
  wire_fold_lom_groups(span, span_len, base, ckpt, n_ckpt, n, acc, first, FBM_WIRE_LOM_GROUP);
}


void host_wire_tokenize_lom(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                            uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  wire_tokenize_host(span, span_len, base, first, n, ckpt, n_ckpt, result, workspace);
}

void host_wire_tokenize_jl(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                           uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  wire_tokenize_jl_host(span, span_len, base, first, n, ckpt, n_ckpt, result, workspace);
}

}  // namespace fbm

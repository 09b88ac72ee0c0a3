// fedbiomed_amd -- the reference Serializer's integer encoding, one item at a time (host and device).
//
// fedbiomed/common/serializer.py:96-110 packs a list of non-negative ints as a msgpack array whose items are
//   v < 2^64   the shortest native form: the byte itself (v <= 127), cc / cd / ce / cf + 1 / 2 / 4 / 8 bytes
//   v >= 2^64  82 a8 "__type__" a3 "int" a5 "value" (20 bytes), then a bin of L = ceil(bit_length / 8) + 1
//              big-endian bytes (c4 L for L <= 255, c5 + BE16 from 256 on): the reference's signed
//              to_bytes, so the first byte is a 00 sign byte.  2048 bits: L = 257, 280 bytes in all.
// The kernels of fbm_wire.hip and the test build's host hooks both run these routines.
#pragma once
#include "../../include/fbm_secagg.h"
#include "fbm_common.hpp"

#define FBM_WIRE_ITEM_MAX 280  // a 2048-bit value
#define FBM_WIRE_NATIVE_MAX 9

namespace fbm {

// ---- encode -----------------------------------------------------------------------------------------
FBM_HD uint32_t wire_header_size(uint64_t n) { return n <= 15 ? 1u : n <= 65535 ? 3u : 5u; }
// byte k of the array header of n items (n < 2^32)
FBM_HD uint8_t wire_header_byte(uint64_t n, uint32_t k) {
  if (n <= 15) return (uint8_t)(0x90 | n);
  if (n <= 65535) return k == 0 ? 0xdc : (uint8_t)(n >> (8 * (2 - k)));
  return k == 0 ? 0xdd : (uint8_t)(n >> (8 * (4 - k)));
}

FBM_HD uint32_t wire_native_size(uint64_t v) {
  return v <= 127 ? 1u : v < (1ull << 8) ? 2u : v < (1ull << 16) ? 3u : v < (1ull << 32) ? 5u : 9u;
}
// byte k of the native form of v, size = wire_native_size(v)
FBM_HD uint8_t wire_native_byte(uint64_t v, uint32_t size, uint32_t k) {
  if (size == 1) return (uint8_t)v;
  if (k == 0) return size == 2 ? 0xcc : size == 3 ? 0xcd : size == 5 ? 0xce : 0xcf;
  return (uint8_t)(v >> (8 * (size - 1 - k)));
}

// bit length of a 64-limb little-endian row, read from the top (a ciphertext's top limb is rarely zero)
FBM_HD int wire_jl_bits(const uint32_t* row) {
  for (int j = 63; j >= 0; --j) {
    const uint32_t w = row[j];
    if (w) return 32 * j + 32 - __builtin_clz(w);
  }
  return 0;
}
FBM_HD uint32_t wire_jl_bin_len(int bits) { return (uint32_t)(bits + 7) / 8 + 1; }
FBM_HD uint32_t wire_jl_size(const uint32_t* row, int bits) {
  if (bits <= 64) return wire_native_size((uint64_t)row[0] | ((uint64_t)row[1] << 32));
  const uint32_t L = wire_jl_bin_len(bits);
  return 20u + (L <= 255 ? 2u : 3u) + L;
}
// byte k of the item of a row of `bits` bits (k < wire_jl_size)
FBM_HD uint8_t wire_jl_byte(const uint32_t* row, int bits, uint32_t k) {
  if (bits <= 64) {
    const uint64_t v = (uint64_t)row[0] | ((uint64_t)row[1] << 32);
    return wire_native_byte(v, wire_native_size(v), k);
  }
  if (k < 20) {  // 82 a8 __type__ a3 int a5 value
    const uint64_t p = k < 8 ? 0x657079745f5fa882ull : k < 16 ? 0x76a5746e69a35f5full : 0x65756c61ull;
    return (uint8_t)(p >> (8 * (k & 7)));
  }
  const uint32_t L = wire_jl_bin_len(bits);
  uint32_t hdr;
  if (L <= 255) {
    if (k == 20) return 0xc4;
    if (k == 21) return (uint8_t)L;
    hdr = 22;
  } else {
    if (k == 20) return 0xc5;
    if (k == 21) return (uint8_t)(L >> 8);
    if (k == 22) return (uint8_t)L;
    hdr = 23;
  }
  const uint32_t i = L - 1 - (k - hdr);  // the byte's little-endian index
  return i >= 256 ? 0 : (uint8_t)(row[i >> 2] >> (8 * (i & 3)));
}

// ---- decode -----------------------------------------------------------------------------------------
// limb j of the value whose vlen big-endian bytes start at v (bytes past the 256th are the sign byte: zero)
FBM_HD uint32_t wire_jl_limb(const uint8_t* v, uint32_t vlen, int j) {
  uint32_t w = 0;
  for (uint32_t t = 0; t < 4; ++t) {
    const uint32_t i = 4u * (uint32_t)j + t;
    if (i < vlen) w |= (uint32_t)v[vlen - 1 - i] << (8 * t);
  }
  return w;
}
// bytes of the native unsigned form that starts with b; 0: not one
FBM_HD uint32_t wire_native_len(uint8_t b) {
  return b <= 0x7f ? 1u : b == 0xcc ? 2u : b == 0xcd ? 3u : b == 0xce ? 5u : b == 0xcf ? 9u : 0u;
}
// item j of a group of native items whose first `avail` bytes are at buf: j steps over the items before it,
// never reading at or past avail.  Anything else than the scanner's promise (an item that is no native form,
// or that runs past avail) gives 0.
FBM_HD uint64_t wire_lom_group_item(const uint8_t* buf, uint32_t avail, int j) {
  uint32_t pos = 0;
  bool ok = true;
  for (int s = 0; s < j; ++s) {
    const uint32_t l = pos < avail ? wire_native_len(buf[pos]) : 0u;
    ok = ok && l != 0;
    pos += l ? l : 1u;
  }
  if (!ok || pos >= avail) return 0;
  const uint32_t l = wire_native_len(buf[pos]);
  if (l == 0 || avail - pos < l) return 0;
  if (l == 1) return buf[pos];
  uint64_t v = 0;
  for (uint32_t t = 1; t < l; ++t) v = (v << 8) | buf[pos + t];
  return v;
}

// wire_fold_lom_kernel's work on the host, group by group (host_wire_fold_lom; tools/wire_fold_check.cpp runs it
// under the host sanitizers): acc[i] = (first ? 0 : acc[i]) + item i, a group whose checkpoint lies outside the
// span adding 0; `group` = FBM_WIRE_LOM_GROUP.  Reads span[0, span_len), ckpt[0, n_ckpt), acc[0, n) and no more.
inline void wire_fold_lom_groups(const uint8_t* span, uint64_t span_len, uint64_t base, const uint64_t* ckpt,
                                 uint64_t n_ckpt, uint64_t n, uint64_t* acc, int first, int group) {
  const uint64_t gb = (uint64_t)group * FBM_WIRE_NATIVE_MAX;  // a group's bytes at most
  for (uint64_t g = 0; g < n_ckpt; ++g) {
    uint32_t avail = 0;
    const uint8_t* buf = span;
    if (ckpt[g] >= base && ckpt[g] - base < span_len) {
      const uint64_t left = span_len - (ckpt[g] - base);
      avail = (uint32_t)(left < gb ? left : gb);
      buf = span + (ckpt[g] - base);
    }
    for (int j = 0; j < group; ++j) {
      const uint64_t i = g * (uint64_t)group + j;
      if (i < n) acc[i] = (first ? 0ull : acc[i]) + wire_lom_group_item(buf, avail, j);
    }
  }
}

// ---- tokenize: where the items of an all-native array start ------------------------------------------
// An item's start depends on every length before it: a 9-state automaton over bytes, the state ("phase") being the
// payload bytes still to skip, 0..8, plus one absorbing state for a byte that starts no native form.  A stretch
// of bytes maps each entry phase to an exit phase and a number of items started; the maps compose
// associatively, so the walk is a scan over blocks.  A map entry is packed as  items << 4 | exit phase.
//
// The stream is cut into sub-blocks of 64 bytes (one lane each) and tiles of 64 sub-blocks (one wave each),
// counted from the message byte `first` rounded down to a 4-byte boundary of the span's ADDRESS: the h <= 3
// bytes in front of `first` are skipped by entering the whole stream in phase h, and every tile is whole
// aligned dwords.  A byte outside the span is never read: it counts as 0 and lies outside `valid`.
#define FBM_WIRE_TOK_SUB 64                                       // bytes per sub-block
#define FBM_WIRE_TOK_SUBS 64                                      // sub-blocks per tile
#define FBM_WIRE_TOK_TILE (FBM_WIRE_TOK_SUB * FBM_WIRE_TOK_SUBS)  // bytes per tile
#define FBM_WIRE_TOK_BAD 9u                                       // the absorbing phase
#define FBM_WIRE_TOK_MAP 10                                       // entries of a map: phases 0..8 and the absorbing one

// wire_native_len of the byte b (0..255) without a branch: two selects
FBM_HD uint32_t wire_tok_len(uint32_t b) {
  const uint32_t wide = (b & 0xfcu) == 0xccu ? 1u + (1u << (b & 3u)) : 0u;  // cc cd ce cf: 2 3 5 9
  return b < 0x80u ? 1u : wide;
}

// the 4 bytes at span[off, off + 4) as a little-endian word, bytes outside [0, span_len) as 0 and not read
FBM_HD uint32_t wire_tok_word(const uint8_t* span, uint64_t span_len, int64_t off) {
  uint32_t w = 0;
  for (int k = 0; k < 4; ++k) {
    const int64_t o = off + k;
    if (o >= 0 && (uint64_t)o < span_len) w |= (uint32_t)span[o] << (8 * k);
  }
  return w;
}

// how many of a sub-block's 64 bytes, the first of them at span offset `off`, lie before the span's end
FBM_HD int wire_tok_valid(uint64_t span_len, int64_t off) {
  const int64_t left = (int64_t)span_len - off;
  return left <= 0 ? 0 : left >= FBM_WIRE_TOK_SUB ? FBM_WIRE_TOK_SUB : (int)left;
}

// One sub-block's map, g[p] for the entry phases p = 0..8, from its 16 words and its `valid` leading bytes.
// Backwards: the result of starting an item at byte i is that of the byte behind the item plus one item, so
// one pass with the nine results behind byte i in hand gives all nine entry phases at once (entering in phase
// p is starting an item at byte p).  A position at or past `valid` lies behind the stream's end: it keeps
// as its exit phase the payload bytes the end cut off, so a truncated item shows as a nonzero final phase.
FBM_HD void wire_tok_block_map(const uint32_t* w, int valid, uint32_t* g) {
  // the results of starting at bytes i + 1 .. i + 9, newest lowest: exit phases 4 bits each, items 7 bits each
  uint64_t ex = 0, it = 0;
#pragma unroll
  for (int k = 8; k >= 0; --k) {
    const int past = FBM_WIRE_TOK_SUB + k - valid;  // >= 0
    ex = ex << 4 | (uint64_t)(past > 8 ? FBM_WIRE_TOK_BAD : (uint32_t)past);
  }
#pragma unroll
  for (int i = FBM_WIRE_TOK_SUB - 1; i >= 0; --i) {
    const uint32_t l = wire_tok_len((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
    const uint32_t s = l ? l - 1 : 0u;  // the item's last byte is s bytes on: the result behind it
    uint32_t e = (uint32_t)(ex >> (4 * s)) & 15u, c = ((uint32_t)(it >> (7 * s)) & 127u) + 1u;
    e = l ? e : FBM_WIRE_TOK_BAD, c = l ? c : 0u;
    const int past = i - valid;  // >= 0: behind the stream's end
    e = past >= 0 ? (past > 8 ? FBM_WIRE_TOK_BAD : (uint32_t)past) : e, c = past >= 0 ? 0u : c;
    ex = ex << 4 | e, it = it << 7 | c;  // (older results leave through the top; the nine newest are all that is read)
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) g[k] = ((uint32_t)(it >> (7 * k)) & 127u) << 4 | ((uint32_t)(ex >> (4 * k)) & 15u);
}

// The forward walk of one sub-block entered in `phase` (0..8) with item `k0` the next to start.  Of the <= 64
// items that start here at most one has an index that is a multiple of `group` = 64 and at most one is item
// n - 1: *ck_pos receives the byte position (0..63) of the first, *end_pos the position one past the second
// (1..72: it may end in a later sub-block), each -1 where there is none.
FBM_HD void wire_tok_block_walk(const uint32_t* w, int valid, uint32_t phase, uint64_t k0, uint64_t n, int* ck_pos,
                                int* end_pos) {
  const uint32_t to_ck = (uint32_t)((0 - k0) & (FBM_WIRE_LOM_GROUP - 1));  // items from k0 to the next group's first
  const uint32_t to_last = n - 1 - k0 < FBM_WIRE_TOK_SUB ? (uint32_t)(n - 1 - k0) : ~0u;  // ... to item n - 1, if it can start here
  const uint32_t dead = 1u << 16;  // as `rem`: no byte starts an item any more (never counted down to 0 in 64 steps)
  uint32_t rem = phase, j = 0;     // payload bytes still to skip; items started here
  int ck = -1, end = -1;
#pragma unroll 1  // (a rolled loop over the words, read where they lie: unrolled, the 64 steps' flags outgrow the registers)
  for (int q = 0; q < FBM_WIRE_TOK_SUB / 4; ++q) {
    const uint32_t word = w[q];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int i = 4 * q + t;
      // a byte at or past `valid` starts nothing: the walk ends there as at a byte that is no native form
      const uint32_t l = i < valid ? wire_tok_len((word >> (8 * t)) & 0xffu) : 0u;
      const bool item = rem == 0 && l != 0;
      if (item && j == to_ck) ck = i;
      if (item && j == to_last) end = i + (int)l;
      j += item ? 1u : 0u;
      rem = rem ? rem - 1 : l ? l - 1 : dead;
    }
  }
  *ck_pos = ck, *end_pos = end;
}

// state (items << 4 | phase) stepped through one map (FBM_WIRE_TOK_MAP packed entries, [9] = the absorbing one)
template <class T>
FBM_HD uint64_t wire_tok_step(uint64_t state, const T* map) {
  const uint64_t e = (uint64_t)map[state & 15];
  return ((state >> 4) + (e >> 4)) << 4 | (e & 15);
}

#define FBM_WIRE_TOK_SCAN_THREADS 256  // threads of the one workgroup that scans the tiles' maps

// thread t's run of tiles: [b0, b1)
FBM_HD void wire_tok_run(uint64_t tiles, int t, uint64_t* b0, uint64_t* b1) {
  const uint64_t chunk = (tiles + FBM_WIRE_TOK_SCAN_THREADS - 1) / FBM_WIRE_TOK_SCAN_THREADS;
  *b0 = (uint64_t)t * chunk < tiles ? (uint64_t)t * chunk : tiles;
  *b1 = *b0 + chunk < tiles ? *b0 + chunk : tiles;
}
// result[0] from the stream's final state: an item the end cut off was started, not completed
FBM_HD uint64_t wire_tok_whole_items(uint64_t st, uint64_t n) {
  const uint64_t phase = st & 15, started = st >> 4;
  const uint64_t whole = phase >= 1 && phase <= 8 && started > 0 ? started - 1 : started;
  return whole < n ? whole : n;
}

// the stream's cut: the span offset of its first sub-block (first rounded down to an aligned address; negative by
// up to 3 where first is the span's first byte), the bytes in front of first, the tiles down to the span's end
struct wire_tok_cut {
  int64_t origin;
  uint32_t head;
  uint64_t tiles;
};
inline wire_tok_cut wire_tok_cut_of(const uint8_t* span, uint64_t span_len, uint64_t s0) {
  wire_tok_cut c;
  c.head = (uint32_t)((reinterpret_cast<uintptr_t>(span) + s0) & 3u);
  c.origin = (int64_t)s0 - (int64_t)c.head;
  c.tiles = (uint64_t)((int64_t)span_len - c.origin + FBM_WIRE_TOK_TILE - 1) / FBM_WIRE_TOK_TILE;
  return c;
}
// workspace: every tile's entry state (u64 each, rounded up to 256 bytes), then every tile's map (10 u32 each)
inline uint64_t wire_tok_maps_at(uint64_t tiles) { return (tiles * 8 + 255) / 256 * 256; }

// fbm_wire_tokenize_lom's three kernels (fbm_wire.hip) over host buffers, tile by tile and run by run as the kernels
// cut them, through the same per-block routines (host_wire_tokenize_lom; tools/wire_tokenize_check.cpp runs it under the
// host sanitizers).  Reads span[0, span_len) and no more; writes ckpt[0, n_ckpt), result[0, 2) and the workspace.
inline void wire_tok_host_sub(const uint8_t* span, uint64_t span_len, int64_t sub, uint32_t* w, int* valid, uint16_t* map) {
  for (int i = 0; i < 16; ++i) w[i] = wire_tok_word(span, span_len, sub + 4 * i);
  *valid = wire_tok_valid(span_len, sub);
  uint32_t g[9];
  wire_tok_block_map(w, *valid, g);
  for (int p = 0; p < 9; ++p) map[p] = (uint16_t)g[p];
  map[9] = (uint16_t)FBM_WIRE_TOK_BAD;
}

inline void wire_tokenize_host(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                            uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  const wire_tok_cut c = wire_tok_cut_of(span, span_len, first - base);
  uint64_t* entry = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* maps = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(workspace) + wire_tok_maps_at(c.tiles));
  uint32_t w[16];
  uint16_t map[FBM_WIRE_TOK_SUBS][FBM_WIRE_TOK_MAP];
  int valid = 0;
  for (uint64_t tile = 0; tile < c.tiles; ++tile) {  // wire_tok_maps_kernel
    const int64_t tbase = c.origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
    for (int j = 0; j < FBM_WIRE_TOK_SUBS; ++j) wire_tok_host_sub(span, span_len, tbase + FBM_WIRE_TOK_SUB * j, w, &valid, map[j]);
    for (int p = 0; p < FBM_WIRE_TOK_MAP; ++p) {
      uint64_t st = (uint64_t)p;
      for (int j = 0; j < FBM_WIRE_TOK_SUBS; ++j) st = wire_tok_step(st, map[j]);
      maps[tile * FBM_WIRE_TOK_MAP + p] = (uint32_t)st;
    }
  }
  uint64_t st = c.head;  // wire_tok_scan_kernel
  for (int t = 0; t < FBM_WIRE_TOK_SCAN_THREADS; ++t) {
    uint64_t b0, b1, comp[FBM_WIRE_TOK_MAP];
    wire_tok_run(c.tiles, t, &b0, &b1);
    for (int p = 0; p < FBM_WIRE_TOK_MAP; ++p) {
      comp[p] = (uint64_t)p;
      for (uint64_t b = b0; b < b1; ++b) comp[p] = wire_tok_step(comp[p], maps + b * FBM_WIRE_TOK_MAP);
    }
    uint64_t in = st;
    for (uint64_t b = b0; b < b1; ++b) {
      entry[b] = in;
      in = wire_tok_step(in, maps + b * FBM_WIRE_TOK_MAP);
    }
    st = wire_tok_step(st, comp);  // (= in: the run's composite and its tiles one by one agree)
  }
  result[0] = wire_tok_whole_items(st, n);
  result[1] = 0;
  for (uint64_t tile = 0; tile < c.tiles; ++tile) {  // wire_tok_emit_kernel
    const int64_t tbase = c.origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
    uint64_t in = entry[tile];
    for (int j = 0; j < FBM_WIRE_TOK_SUBS; ++j) {
      const int64_t sub = tbase + FBM_WIRE_TOK_SUB * j;
      wire_tok_host_sub(span, span_len, sub, w, &valid, map[j]);
      const uint64_t mine = in;
      in = wire_tok_step(in, map[j]);
      if ((mine & 15) == FBM_WIRE_TOK_BAD) continue;
      int ck, end;
      wire_tok_block_walk(w, valid, (uint32_t)(mine & 15), mine >> 4, n, &ck, &end);
      if (ck >= 0) {
        const uint64_t group = ((mine >> 4) + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP;
        if (group < n_ckpt) ckpt[group] = base + (uint64_t)(sub + ck);
      }
      if (end >= 0 && (uint64_t)(sub + end) <= span_len) result[1] = base + (uint64_t)(sub + end);
    }
  }
}

}  // namespace fbm

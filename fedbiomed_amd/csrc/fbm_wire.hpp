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

// The three passes over the `tiles` tiles that begin at span offset `origin`, entered in the running state `carry`
// (the whole stream: wire_tok_cut_of's origin, tiles and head); returns the state behind them.  result[0] is written,
// result[1] only where item n - 1 ends in these tiles: the caller zeroes it first.
inline uint64_t wire_seg_host_lom(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t n, int64_t origin,
                                  uint64_t tiles, uint64_t carry, uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result,
                                  void* workspace) {
  uint64_t* entry = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* maps = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(workspace) + wire_tok_maps_at(tiles));
  uint32_t w[16];
  uint16_t map[FBM_WIRE_TOK_SUBS][FBM_WIRE_TOK_MAP];
  int valid = 0;
  for (uint64_t tile = 0; tile < tiles; ++tile) {  // wire_tok_maps_kernel
    const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
    for (int j = 0; j < FBM_WIRE_TOK_SUBS; ++j) wire_tok_host_sub(span, span_len, tbase + FBM_WIRE_TOK_SUB * j, w, &valid, map[j]);
    for (int p = 0; p < FBM_WIRE_TOK_MAP; ++p) {
      uint64_t st = (uint64_t)p;
      for (int j = 0; j < FBM_WIRE_TOK_SUBS; ++j) st = wire_tok_step(st, map[j]);
      maps[tile * FBM_WIRE_TOK_MAP + p] = (uint32_t)st;
    }
  }
  uint64_t st = carry;  // wire_tok_scan_kernel
  for (int t = 0; t < FBM_WIRE_TOK_SCAN_THREADS; ++t) {
    uint64_t b0, b1, comp[FBM_WIRE_TOK_MAP];
    wire_tok_run(tiles, t, &b0, &b1);
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
  for (uint64_t tile = 0; tile < tiles; ++tile) {  // wire_tok_emit_kernel
    const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
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
  return st;
}

inline void wire_tokenize_host(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                               uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  const wire_tok_cut c = wire_tok_cut_of(span, span_len, first - base);
  result[1] = 0;
  wire_seg_host_lom(span, span_len, base, n, c.origin, c.tiles, c.head, ckpt, n_ckpt, result, workspace);
}

// ---- tokenize (JL): where the values of an array of big-int maps start ------------------------------
// An item is 23..280 bytes and its size is a function of the 24 bytes at its start (the 20-byte prefix, c4 L or
// c5 BE16 L, the value's first byte), so whether an accepted item starts at a byte and how long it is can be
// asked of any position on its own.  With tiles of FBM_WIRE_TOK_TILE >= 280 bytes, cut as the LOM stream is cut
// (wire_tok_cut_of), the chain of items that enters a tile at offset e < 280 leaves it at an offset < 280 into the
// next one: a tile's transfer map takes an entry offset to (exit offset, items completed in between), or to "dead"
// with the items completed before the position that holds no accepted item.  Only an entry offset at which the
// whole prefix stands can start anything, and the prefix holds 82 at its head alone, so two such offsets are at
// least 20 bytes apart: at most 14 of them in [0, 280).  A map is FBM_WIRE_TOKJ_SLOTS packed words,
//   entry offset | exit offset << 9 | items << 18      (an unused slot: all ones; a dead exit: FBM_WIRE_TOKJ_DEAD)
// and maps compose by looking the exit offset up among the next map's entries; an offset that is not there is dead.
// A running state is  items << 16 | offset  (offset FBM_WIRE_TOKJ_GONE: dead, the items stay).  An item the span's
// end cuts off is no item: the chain dies in front of it, so the items of a state are all whole.
#define FBM_WIRE_TOKJ_REACH 280                                   // = FBM_WIRE_ITEM_MAX: entry and exit offsets lie below
#define FBM_WIRE_TOKJ_SLOTS 16                                    // words of a tile's map (14 entries at most)
#define FBM_WIRE_TOKJ_HEAD 24                                     // bytes that decide an item's size
#define FBM_WIRE_TOKJ_WORDS ((FBM_WIRE_TOK_TILE + FBM_WIRE_TOKJ_HEAD) / 4 + 2)  // a staged tile: its words, a header across its end
#define FBM_WIRE_TOKJ_ITEMS ((FBM_WIRE_TOK_TILE + 22) / 23)       // items that start in one tile at most: 179
#define FBM_WIRE_TOKJ_DEAD 0x1ffu                                 // a map entry's exit: the chain ended in the tile
#define FBM_WIRE_TOKJ_GONE 0xffffull                              // a state's offset: the chain has ended
static_assert(FBM_WIRE_TOK_TILE >= FBM_WIRE_TOKJ_REACH && FBM_WIRE_TOKJ_REACH == FBM_WIRE_ITEM_MAX, "a chain skips no tile");
static_assert(FBM_WIRE_TOKJ_ITEMS < 256 && FBM_WIRE_TOKJ_REACH < (int)FBM_WIRE_TOKJ_DEAD, "a map entry's fields");
static_assert((FBM_WIRE_TOKJ_REACH + 19) / 20 <= FBM_WIRE_TOKJ_SLOTS, "prefix matches are 20 bytes apart");

// the 4 bytes at byte offset `off` of a staged tile (w: its aligned words) as a little-endian word
FBM_HD uint32_t wire_tokj_u32(const uint32_t* w, uint32_t off) {
  const uint32_t q = off >> 2, sh = 8 * (off & 3);
  const uint64_t two = (uint64_t)w[q] | ((uint64_t)w[q + 1] << 32);
  return (uint32_t)(two >> sh);
}
// whether the 20-byte prefix stands at offset `off` of a staged tile
FBM_HD bool wire_tokj_prefix(const uint32_t* w, uint32_t off) {
  return wire_tokj_u32(w, off) == 0x5f5fa882u && wire_tokj_u32(w, off + 4) == 0x65707974u &&
         wire_tokj_u32(w, off + 8) == 0x69a35f5fu && wire_tokj_u32(w, off + 12) == 0x76a5746eu &&
         wire_tokj_u32(w, off + 16) == 0x65756c61u;
}
// The item at offset `off` (< FBM_WIRE_TOK_TILE) of a staged tile, `left` bytes of the span being left from there
// (<= 0: none): its size, 0 where fbm_wire_item accepts no map form there or the item runs past the span; *L its
// value's bytes.  Reads the staged words only (bytes outside the span are staged as 0).
FBM_HD uint32_t wire_tokj_step(const uint32_t* w, uint32_t off, int64_t left, uint32_t* L) {
  if (!wire_tokj_prefix(w, off)) return 0;
  const uint32_t h = wire_tokj_u32(w, off + 20);  // c4 L v0 .. / c5 Lhi Llo v0
  const uint32_t b = h & 0xffu;
  uint32_t len, hdr, v0;
  if (b == 0xc4u)
    len = (h >> 8) & 0xffu, hdr = 22, v0 = (h >> 16) & 0xffu;
  else if (b == 0xc5u)
    len = ((h >> 8) & 0xffu) << 8 | ((h >> 16) & 0xffu), hdr = 23, v0 = h >> 24;
  else
    return 0;
  if (len < 1 || len > 257 || (int64_t)(hdr + len) > left) return 0;
  if (v0 >= 0x80u || (len == 257 && v0 != 0)) return 0;  // a negative value, or one of 2^2048 or more
  *L = len;
  return hdr + len;
}
// The chain that enters a staged tile at offset `e` (`left` bytes of the span from the tile's first byte on): the
// offset into the next tile at which it leaves, or FBM_WIRE_TOKJ_DEAD; *items the items completed on the way.
FBM_HD uint32_t wire_tokj_chain(const uint32_t* w, uint32_t e, int64_t left, uint32_t* items) {
  uint32_t off = e, c = 0, L = 0;
  while (off < FBM_WIRE_TOK_TILE) {
    const uint32_t s = wire_tokj_step(w, off, left - (int64_t)off, &L);
    if (s == 0) {
      *items = c;
      return FBM_WIRE_TOKJ_DEAD;
    }
    off += s, ++c;
  }
  *items = c;
  return off - FBM_WIRE_TOK_TILE;
}
FBM_HD uint32_t wire_tokj_entry(uint32_t e, uint32_t exit, uint32_t items) { return e | exit << 9 | items << 18; }
// a state stepped through one map (FBM_WIRE_TOKJ_SLOTS words)
FBM_HD uint64_t wire_tokj_apply(uint64_t state, const uint32_t* map) {
  const uint64_t off = state & 0xffffull;
  if (off == FBM_WIRE_TOKJ_GONE) return state;
  for (int k = 0; k < FBM_WIRE_TOKJ_SLOTS; ++k) {
    const uint32_t m = map[k];
    if ((m & 0x1ffu) == off) {  // (an unused slot's entry offset is 511: never an offset)
      const uint32_t exit = (m >> 9) & 0x1ffu;
      return ((state >> 16) + (m >> 18 & 0xffu)) << 16 | (exit == FBM_WIRE_TOKJ_DEAD ? FBM_WIRE_TOKJ_GONE : (uint64_t)exit);
    }
  }
  return state | FBM_WIRE_TOKJ_GONE;
}
// a state stepped through a run of tiles whose composite from each of its first map's entries is comp[]
FBM_HD uint64_t wire_tokj_apply_run(uint64_t state, const uint32_t* first_map, const uint64_t* comp, int stride) {
  const uint64_t off = state & 0xffffull;
  if (off == FBM_WIRE_TOKJ_GONE) return state;
  for (int k = 0; k < FBM_WIRE_TOKJ_SLOTS; ++k)
    if ((first_map[k] & 0x1ffu) == off) {
      const uint64_t c = comp[k * stride];
      return ((state >> 16) + (c >> 16)) << 16 | (c & 0xffffull);
    }
  return state | FBM_WIRE_TOKJ_GONE;
}
// The emit walk of one staged tile from its entry state: word j of `out` (FBM_WIRE_TOKJ_ITEMS words) is the table's
// word of item (state >> 16) + j -- (absolute offset of the value's first byte) << 16 | L --; returns how many;
// *end_off the tile offset one past item n - 1 where that item is among them, else -1.  abs0 = the absolute offset
// of the tile's first byte (as a signed value: the first tile may begin up to 3 bytes in front of the span).
FBM_HD uint32_t wire_tokj_emit_walk(const uint32_t* w, uint64_t state, int64_t left, int64_t abs0, uint64_t n, uint64_t* out,
                                    int* end_off) {
  const uint64_t k0 = state >> 16;
  uint32_t off = (uint32_t)(state & 0xffffull), c = 0, L = 0;
  *end_off = -1;
  if (off == (uint32_t)FBM_WIRE_TOKJ_GONE) return 0;
  while (off < FBM_WIRE_TOK_TILE && c < FBM_WIRE_TOKJ_ITEMS && k0 + c < n) {
    const uint32_t s = wire_tokj_step(w, off, left - (int64_t)off, &L);
    if (s == 0) break;
    out[c] = (uint64_t)(abs0 + (int64_t)(off + s - L)) << 16 | L;
    off += s;
    if (k0 + c == n - 1) *end_off = (int)off;
    ++c;
  }
  return c;
}

// workspace: every tile's entry state (u64 each, rounded up to 256 bytes), then every tile's map
inline uint64_t wire_tokj_workspace_of(uint64_t tiles) { return wire_tok_maps_at(tiles) + tiles * FBM_WIRE_TOKJ_SLOTS * 4; }

// one tile staged on the host as the kernels stage it
inline void wire_tokj_host_stage(const uint8_t* span, uint64_t span_len, int64_t tbase, uint32_t* w) {
  for (int d = 0; d < FBM_WIRE_TOKJ_WORDS; ++d) w[d] = wire_tok_word(span, span_len, tbase + 4 * d);
}
inline void wire_tokj_host_map(const uint32_t* w, int64_t left, uint32_t* map) {
  int slot = 0;
  for (int k = 0; k < FBM_WIRE_TOKJ_SLOTS; ++k) map[k] = ~0u;
  for (uint32_t e = 0; e < FBM_WIRE_TOKJ_REACH; ++e)
    if (wire_tokj_prefix(w, e) && slot < FBM_WIRE_TOKJ_SLOTS) {
      uint32_t items = 0;
      const uint32_t exit = wire_tokj_chain(w, e, left, &items);
      map[slot++] = wire_tokj_entry(e, exit, items);
    }
}

// fbm_wire_tokenize_jl's three kernels (fbm_wire.hip) over host buffers, tile by tile and run by run as the kernels
// cut them, through the same routines (host_wire_tokenize_jl; tools/wire_tokenize_jl_check.cpp runs it under the host
// sanitizers).  Reads span[0, span_len) and no more; writes ckpt[0, n_ckpt), result[0, 2) and the workspace.
// (wire_seg_host_jl: the passes over the `tiles` tiles from span offset `origin` on, entered in the state `carry`, as
// wire_seg_host_lom)
inline uint64_t wire_seg_host_jl(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t n, int64_t origin,
                                 uint64_t tiles, uint64_t carry, uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result,
                                 void* workspace) {
  uint64_t* entry = reinterpret_cast<uint64_t*>(workspace);
  uint32_t* maps = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(workspace) + wire_tok_maps_at(tiles));
  uint32_t w[FBM_WIRE_TOKJ_WORDS];
  for (uint64_t tile = 0; tile < tiles; ++tile) {  // wire_tokj_maps_kernel
    const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
    wire_tokj_host_stage(span, span_len, tbase, w);
    wire_tokj_host_map(w, (int64_t)span_len - tbase, maps + tile * FBM_WIRE_TOKJ_SLOTS);
  }
  uint64_t st = carry;  // wire_tokj_scan_kernel
  for (int t = 0; t < FBM_WIRE_TOK_SCAN_THREADS; ++t) {
    uint64_t b0, b1, comp[FBM_WIRE_TOKJ_SLOTS];
    wire_tok_run(tiles, t, &b0, &b1);
    if (b0 == b1) continue;
    for (int k = 0; k < FBM_WIRE_TOKJ_SLOTS; ++k) {
      const uint32_t m = maps[b0 * FBM_WIRE_TOKJ_SLOTS + k];
      uint64_t s = m == ~0u ? FBM_WIRE_TOKJ_GONE : (uint64_t)(m & 0x1ffu);
      for (uint64_t b = b0; b < b1; ++b) s = wire_tokj_apply(s, maps + b * FBM_WIRE_TOKJ_SLOTS);
      comp[k] = s;
    }
    uint64_t in = st;
    for (uint64_t b = b0; b < b1; ++b) {
      entry[b] = in;
      in = wire_tokj_apply(in, maps + b * FBM_WIRE_TOKJ_SLOTS);
    }
    st = wire_tokj_apply_run(st, maps + b0 * FBM_WIRE_TOKJ_SLOTS, comp, 1);  // (= in)
  }
  result[0] = (st >> 16) < n ? (st >> 16) : n;
  uint64_t out[FBM_WIRE_TOKJ_ITEMS];
  for (uint64_t tile = 0; tile < tiles; ++tile) {  // wire_tokj_emit_kernel
    const int64_t tbase = origin + (int64_t)(tile * FBM_WIRE_TOK_TILE);
    wire_tokj_host_stage(span, span_len, tbase, w);
    int end = -1;
    const uint32_t cnt = wire_tokj_emit_walk(w, entry[tile], (int64_t)span_len - tbase, (int64_t)base + tbase, n, out, &end);
    for (uint32_t j = 0; j < cnt; ++j)
      if ((entry[tile] >> 16) + j < n_ckpt) ckpt[(entry[tile] >> 16) + j] = out[j];
    if (end >= 0) result[1] = (uint64_t)((int64_t)base + tbase + end);
  }
  return st;
}

inline void wire_tokenize_jl_host(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n,
                                  uint64_t* ckpt, uint64_t n_ckpt, uint64_t* result, void* workspace) {
  const wire_tok_cut c = wire_tok_cut_of(span, span_len, first - base);
  result[1] = 0;
  wire_seg_host_jl(span, span_len, base, n, c.origin, c.tiles, c.head, ckpt, n_ckpt, result, workspace);
}

// ---- the tokenizers as resumable scans (fbm_wire_stream_begin / fbm_wire_stream_feed) ---------------------------
// Both tokenizers are a scan over tiles, and a tile's place depends on the span's address, its base and `first` alone,
// not on the span's length: a span that grows keeps its tiles.  A feed runs the three passes over the tiles that have
// become final since the last one, the scan entered in the running state the last feed left in the stream's record and
// leaving its own there.  A tile is final once every item that starts in it lies wholly below avail_len -- the tile's
// end plus the longest item's reach, FBM_WIRE_NATIVE_MAX - 1 or FBM_WIRE_ITEM_MAX bytes --: then its map, its items'
// table words and whether item n - 1 ends inside the span are what the whole span's one call finds.  The last feed
// takes every tile left, the partial one included, under the span's final length.  The passes write a segment's entry
// states and maps at the front of the workspace, each feed over the last one's (the stream orders them).
//
// The record, FBM_WIRE_STREAM_STATE_WORDS u64 words.  The device's copy holds what the kernels read and write (carry,
// the two result words; FED and TILES as of the last feed that ran a tile); the library keeps the host's copy of a
// device stream, which plans the launches, beside it (fbm_capi.hip), and the host run uses its record for both.
#define FBM_WIRE_SEG_FED 0     // bytes fed: the largest avail_len so far
#define FBM_WIRE_SEG_TILES 1   // tiles done
#define FBM_WIRE_SEG_CARRY 2   // the running state behind them (LOM: items << 4 | phase; JL: items << 16 | offset)
#define FBM_WIRE_SEG_RESULT 3  // the one-shot calls' result[0], result[1]
#define FBM_WIRE_SEG_FIRST 5
#define FBM_WIRE_SEG_ITEMS 6
#define FBM_WIRE_SEG_SCHEME 7  // scheme + 1; | FBM_WIRE_SEG_DONE behind the last feed; 0: no stream begun
#define FBM_WIRE_SEG_SPAN 8    // the first feed's span address (0: none yet) and base: every feed's
#define FBM_WIRE_SEG_BASE 9
#define FBM_WIRE_SEG_DONE 0x100ull
static_assert(FBM_WIRE_STREAM_STATE_WORDS >= 10, "the record's words");

inline void wire_seg_begin(int scheme, uint64_t first, uint64_t n, uint64_t* rec) {
  for (int k = 0; k < FBM_WIRE_STREAM_STATE_WORDS; ++k) rec[k] = 0;
  rec[FBM_WIRE_SEG_FIRST] = first, rec[FBM_WIRE_SEG_ITEMS] = n, rec[FBM_WIRE_SEG_SCHEME] = (uint64_t)scheme + 1;
}

struct wire_seg_plan {
  int64_t origin;   // the span offset of tile `lo`
  uint64_t lo, hi;  // the tiles this feed runs: [lo, hi)
  uint32_t head;    // the stream's entry state (tile 0's)
};
// What a feed of avail_len bytes runs, from the host's record; a message where the arguments do not continue the
// record's stream (FBM_E_ARG), else nullptr.
inline const char* wire_seg_plan_of(const uint64_t* rec, int scheme, const uint8_t* span, uint64_t base, uint64_t avail,
                                    int last, wire_seg_plan* p) {
  if (rec[FBM_WIRE_SEG_SCHEME] != (uint64_t)scheme + 1)
    return rec[FBM_WIRE_SEG_SCHEME] & FBM_WIRE_SEG_DONE ? "the stream has had its last feed" : "no stream of this scheme begun on this state";
  if (rec[FBM_WIRE_SEG_SPAN] && (rec[FBM_WIRE_SEG_SPAN] != (uint64_t)reinterpret_cast<uintptr_t>(span) || rec[FBM_WIRE_SEG_BASE] != base))
    return "span / span_base differ from the stream's first feed";
  if (avail < rec[FBM_WIRE_SEG_FED]) return "avail_len below what was already fed";
  const uint64_t first = rec[FBM_WIRE_SEG_FIRST];
  if (first < base || (last && first - base >= avail)) return "first outside the span";
  const wire_tok_cut c = wire_tok_cut_of(span, avail, first - base);
  p->head = c.head, p->lo = rec[FBM_WIRE_SEG_TILES];
  if (last) {
    p->hi = c.tiles;
  } else {
    const int64_t reach = scheme == FBM_WIRE_JL ? FBM_WIRE_ITEM_MAX : FBM_WIRE_NATIVE_MAX - 1;
    const int64_t room = (int64_t)avail - reach - c.origin;
    p->hi = room > 0 ? (uint64_t)room / FBM_WIRE_TOK_TILE : 0;
  }
  if (p->hi < p->lo) p->hi = p->lo;  // (never: avail_len only grows)
  p->origin = c.origin + (int64_t)(p->lo * FBM_WIRE_TOK_TILE);
  return nullptr;
}
// the record behind a planned feed
inline void wire_seg_fed(uint64_t* rec, const wire_seg_plan& p, const uint8_t* span, uint64_t base, uint64_t avail, int last) {
  rec[FBM_WIRE_SEG_FED] = avail, rec[FBM_WIRE_SEG_TILES] = p.hi;
  rec[FBM_WIRE_SEG_SPAN] = (uint64_t)reinterpret_cast<uintptr_t>(span), rec[FBM_WIRE_SEG_BASE] = base;
  if (last) rec[FBM_WIRE_SEG_SCHEME] |= FBM_WIRE_SEG_DONE;
}

// fbm_wire_stream_feed over host buffers (the record is the state): the kernels' passes through the same routines
inline const char* wire_seg_host_feed(int scheme, const uint8_t* span, uint64_t base, uint64_t avail, int last, uint64_t* ckpt,
                                      uint64_t n_ckpt, uint64_t* state, void* workspace) {
  wire_seg_plan p;
  const char* err = wire_seg_plan_of(state, scheme, span, base, avail, last, &p);
  if (err) return err;
  if (p.hi > p.lo) {
    const uint64_t carry = p.lo == 0 ? (uint64_t)p.head : state[FBM_WIRE_SEG_CARRY];
    const uint64_t n = state[FBM_WIRE_SEG_ITEMS];
    state[FBM_WIRE_SEG_CARRY] =
        scheme == FBM_WIRE_JL
            ? wire_seg_host_jl(span, avail, base, n, p.origin, p.hi - p.lo, carry, ckpt, n_ckpt, state + FBM_WIRE_SEG_RESULT, workspace)
            : wire_seg_host_lom(span, avail, base, n, p.origin, p.hi - p.lo, carry, ckpt, n_ckpt, state + FBM_WIRE_SEG_RESULT, workspace);
  }
  wire_seg_fed(state, p, span, base, avail, last);
  return nullptr;
}

}  // namespace fbm

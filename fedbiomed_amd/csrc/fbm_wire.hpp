// fedbiomed_amd -- the reference Serializer's integer encoding, one item at a time (host and device).
//
// fedbiomed/common/serializer.py:96-110 packs a list of non-negative ints as a msgpack array whose items are
//   v < 2^64   the shortest native form: the byte itself (v <= 127), cc / cd / ce / cf + 1 / 2 / 4 / 8 bytes
//   v >= 2^64  82 a8 "__type__" a3 "int" a5 "value" (20 bytes), then a bin of L = ceil(bit_length / 8) + 1
//              big-endian bytes (c4 L for L <= 255, c5 + BE16 from 256 on): the reference's signed
//              to_bytes, so the first byte is a 00 sign byte.  2048 bits: L = 257, 280 bytes in all.
// The kernels of fbm_wire.hip and the test build's host hooks both run these routines.
#pragma once
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

}  // namespace fbm

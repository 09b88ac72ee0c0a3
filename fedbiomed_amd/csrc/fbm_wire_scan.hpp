// fedbiomed_amd -- host scanner of a msgpack message for the reference Serializer's integer arrays
// (fedbiomed/common/serializer.py:96-110 writes them, :140-149 reads them).  Plain C++, no HIP: the bytes
// come from the network, so this file also compiles on its own under the host sanitizers.
//
// One iterative pass with a bounded nesting depth skips every msgpack object and never reads at or past
// `len`.  An array of at least min_items items, each of them
//   * a native unsigned int (positive fixint, cc / cd / ce / cf; minimal or not: the value is the same), or
//   * the 20-byte map prefix  82 a8 "__type__" a3 "int" a5 "value"  then bin8 / bin16 of 1 <= L <= 257
//     bytes with a first byte < 0x80 and a value < 2^2048 (L == 257: the first byte is 0),
// is recorded with its byte span, item count, scheme (FBM_WIRE_LOM when every item is native, else
// FBM_WIRE_JL) and checkpoints; any other array is walked like every other object and stays msgpack's.
//
// Checkpoints (absolute byte offsets into the message):
//   FBM_WIRE_JL   one per item: (offset of the value's first big-endian byte) << 16 | byte count
//   FBM_WIRE_LOM  one per FBM_WIRE_LOM_GROUP items: the offset of the group's first item
// While an array's items are all native only group checkpoints are written; the first map item restarts the
// array's table per item (one re-walk of the items before it, at most once per array).
//
// fbm_wire_scan_deferred is the same pass (fbm_wire_scan_run) with one more branch: a large array whose first byte is
// a native form is not walked here when the caller brings its end offset from the device tokenizer
// (fbm_wire_tokenize_lom); fbm_wire_scan_deferred2 does the same for a large array of big-int maps
// (fbm_wire_tokenize_jl); see fbm_wire_defer below.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/fbm_secagg.h"

#define FBM_WIRE_MAX_DEPTH 32  // containers open at once; deeper: the scan gives up
#define FBM_WIRE_PREFIX_LEN 20
#define FBM_WIRE_SCAN_GAVE_UP 1  // malformed, truncated, trailing bytes or too deep: nothing is recorded
#define FBM_WIRE_SCAN_FULL 2     // a table of the caller's is too small
#define FBM_WIRE_SCAN_PENDING 3  // a deferral candidate without an answer yet: `pending` is filled, nothing is recorded
#define FBM_WIRE_SCAN_BAD_END 4  // a resolved end offset that is not behind the array's first item and within the message
#define FBM_WIRE_MAX_DEFERRED 8  // deferral candidates per message; later ones are walked here

static const uint8_t FBM_WIRE_PREFIX[FBM_WIRE_PREFIX_LEN] = {0x82, 0xa8, '_', '_', 't', 'y', 'p', 'e', '_', '_',
                                                             0xa3, 'i',  'n', 't', 0xa5, 'v', 'a', 'l', 'u', 'e'};

// One accepted item at d[pos..]: returns its byte count (0: not an accepted form, or truncated), the span of
// its big-endian value bytes and whether it is a native form.
static inline uint64_t fbm_wire_item(const uint8_t* d, uint64_t pos, uint64_t len, uint64_t* voff, uint32_t* vlen,
                                     int* native) {
  if (pos >= len) return 0;
  const uint64_t left = len - pos;  // >= 1
  const uint8_t b = d[pos];
  if (b <= 0x7f) {
    *voff = pos, *vlen = 1, *native = 1;
    return 1;
  }
  if (b >= 0xcc && b <= 0xcf) {
    const uint32_t w = 1u << (b - 0xcc);
    if (left < 1ull + w) return 0;
    *voff = pos + 1, *vlen = w, *native = 1;
    return 1ull + w;
  }
  if (b != 0x82 || left < FBM_WIRE_PREFIX_LEN + 2 || memcmp(d + pos, FBM_WIRE_PREFIX, FBM_WIRE_PREFIX_LEN) != 0) return 0;
  const uint64_t p = pos + FBM_WIRE_PREFIX_LEN;  // p + 1 < len
  uint64_t v;
  uint32_t L;
  if (d[p] == 0xc4) {
    L = d[p + 1], v = p + 2;
  } else if (d[p] == 0xc5) {
    if (len - p < 3) return 0;
    L = ((uint32_t)d[p + 1] << 8) | d[p + 2], v = p + 3;
  } else {
    return 0;
  }
  if (L < 1 || L > 257 || len - v < L) return 0;
  if (d[v] >= 0x80 || (L == 257 && d[v] != 0)) return 0;  // a negative value, or one of 2^2048 or more
  *voff = v, *vlen = L, *native = 0;
  return v + L - pos;
}

struct fbm_wire_scan_out {
  fbm_wire_array* arrays;
  uint64_t arrays_cap, n_arrays;
  uint64_t* ckpt;
  uint64_t ckpt_cap, n_ckpt;
};

// items [first, first + n) of a candidate array: 1 recorded (*end = one past it), 0 not, -1 a table is full
static inline int fbm_wire_candidate(const uint8_t* d, uint64_t len, uint64_t begin, uint64_t first, uint64_t n,
                                     fbm_wire_scan_out* o, uint64_t* end) {
  if (o->n_arrays >= o->arrays_cap) return -1;
  const uint64_t ck0 = o->n_ckpt;
  int lom = 1, native = 0;
  uint64_t p = first, voff = 0;
  uint32_t vlen = 0;
  for (uint64_t i = 0; i < n; ++i) {
    if (lom && i % FBM_WIRE_LOM_GROUP == 0) {
      if (o->n_ckpt >= o->ckpt_cap) return -1;
      o->ckpt[o->n_ckpt++] = p;
    }
    const uint64_t c = fbm_wire_item(d, p, len, &voff, &vlen, &native);
    if (c == 0) {
      o->n_ckpt = ck0;
      return 0;
    }
    if (lom && !native) {  // the first map item: the table again, per item
      lom = 0;
      o->n_ckpt = ck0;
      uint64_t q = first, qo = 0;
      uint32_t ql = 0;
      int qn = 0;
      for (uint64_t j = 0; j < i; ++j) {
        const uint64_t cj = fbm_wire_item(d, q, len, &qo, &ql, &qn);  // (accepted once already: cj > 0)
        if (o->n_ckpt >= o->ckpt_cap) return -1;
        o->ckpt[o->n_ckpt++] = (qo << 16) | ql;
        q += cj;
      }
    }
    if (!lom) {
      if (o->n_ckpt >= o->ckpt_cap) return -1;
      o->ckpt[o->n_ckpt++] = (voff << 16) | vlen;
    }
    p += c;
  }
  fbm_wire_array* a = &o->arrays[o->n_arrays++];
  a->begin = begin, a->end = p, a->n_items = n;
  a->ckpt_first = ck0, a->ckpt_count = o->n_ckpt - ck0;
  a->scheme = lom ? FBM_WIRE_LOM : FBM_WIRE_JL, a->pad = 0;
  *end = p;
  return 1;
}

static inline uint64_t fbm_wire_be(const uint8_t* p, int bytes) {
  uint64_t v = 0;
  for (int i = 0; i < bytes; ++i) v = (v << 8) | p[i];
  return v;
}

// What fbm_wire_scan_deferred adds to the pass: an array of at least max(min_items, defer_items) items whose first
// byte is a native form is a deferral candidate (an array with more items than bytes left is none: no table is
// ever sized by it).  The k-th candidate, k < FBM_WIRE_MAX_DEFERRED: resolved[k] != 0 is its end offset from
// elsewhere (the device tokenizer) -- it is recorded as FBM_WIRE_LOM with no checkpoints and pad = 1, and the
// pass goes on behind it; resolved[k] == 0: walked here like every other; k >= n_resolved: the pass stops with
// FBM_WIRE_SCAN_PENDING and *pending says which array the caller is to resolve before it runs the pass again.
//
// fbm_wire_scan_deferred2 adds the arrays of big-int maps: an array of at least max(min_items, defer_items_jl) items
// whose first item begins with the whole 20-byte prefix and c4 / c5, and whose items at their smallest (23 bytes
// each) fit the bytes left, is a candidate too (for fbm_wire_tokenize_jl).  Candidates of both kinds take the
// message's FBM_WIRE_MAX_DEFERRED slots in order of appearance; a resolved one is recorded under its own scheme.
struct fbm_wire_defer {
  uint64_t defer_items;  // 0: no all-native array is a candidate
  const uint64_t* resolved;
  uint64_t n_resolved;
  fbm_wire_pending* pending;    // either may be null
  uint64_t defer_items_jl;      // 0: no array of maps is a candidate
  fbm_wire_pending2* pending2;  // as pending, with the candidate's scheme
};
#define FBM_WIRE_JL_ITEM_MIN 23  // the smallest map item: prefix, c4 01, one byte

// FBM_OK, FBM_WIRE_SCAN_GAVE_UP or FBM_WIRE_SCAN_FULL, with df also FBM_WIRE_SCAN_PENDING or FBM_WIRE_SCAN_BAD_END; on
// anything but FBM_OK the counts are zero.  df == nullptr: fbm_wire_scan's pass.
static inline int fbm_wire_scan_run(const uint8_t* d, uint64_t len, uint64_t min_items, fbm_wire_scan_out* o,
                                    const fbm_wire_defer* df) {
  uint64_t candidates = 0;  // deferral candidates met so far
  uint64_t stack[FBM_WIRE_MAX_DEPTH];  // objects still to read in each open container
  int depth = 1;
  uint64_t pos = 0;
  stack[0] = 1;  // the message is one object
  o->n_arrays = o->n_ckpt = 0;
  if (min_items < 1) min_items = 1;
  while (depth > 0) {
    if (stack[depth - 1] == 0) {
      --depth;
      continue;
    }
    --stack[depth - 1];
    if (pos >= len) goto gave_up;
    {
      const uint8_t b = d[pos];
      const uint64_t left = len - pos;
      uint64_t skip = 0, children = 0;  // a scalar's whole size / a container's header size and objects
      int container = 0, is_array = 0;
      if (b <= 0x7f || b >= 0xe0 || b == 0xc0 || b == 0xc2 || b == 0xc3) {
        skip = 1;
      } else if (b <= 0x8f) {
        container = 1, skip = 1, children = 2ull * (b & 0x0f);
      } else if (b <= 0x9f) {
        container = 1, is_array = 1, skip = 1, children = b & 0x0f;
      } else if (b <= 0xbf) {
        skip = 1ull + (b & 0x1f);
      } else {
        int lb = 0;  // bytes of a length field
        uint64_t extra = 0;
        switch (b) {
          case 0xc4: case 0xd9: lb = 1; break;
          case 0xc5: case 0xda: lb = 2; break;
          case 0xc6: case 0xdb: lb = 4; break;
          case 0xc7: lb = 1, extra = 1; break;
          case 0xc8: lb = 2, extra = 1; break;
          case 0xc9: lb = 4, extra = 1; break;
          case 0xca: case 0xce: case 0xd2: skip = 5; break;
          case 0xcb: case 0xcf: case 0xd3: skip = 9; break;
          case 0xcc: case 0xd0: skip = 2; break;
          case 0xcd: case 0xd1: skip = 3; break;
          case 0xd4: skip = 3; break;
          case 0xd5: skip = 4; break;
          case 0xd6: skip = 6; break;
          case 0xd7: skip = 10; break;
          case 0xd8: skip = 18; break;
          case 0xdc: container = 1, is_array = 1, lb = 2; break;
          case 0xdd: container = 1, is_array = 1, lb = 4; break;
          case 0xde: container = 1, lb = 2; break;
          case 0xdf: container = 1, lb = 4; break;
          default: goto gave_up;  // 0xc1: never used
        }
        if (lb) {
          if (left < 1ull + lb) goto gave_up;
          const uint64_t v = fbm_wire_be(d + pos + 1, lb);
          if (container) {
            skip = 1ull + lb, children = is_array ? v : 2 * v;
          } else {
            skip = 1ull + lb + extra + v;
          }
        }
      }
      if (left < skip) goto gave_up;
      if (!container) {
        pos += skip;
        continue;
      }
      int cand = -1;  // the scheme a deferral candidate is recorded under
      if (is_array && children >= min_items && df && candidates < FBM_WIRE_MAX_DEFERRED) {
        const uint64_t body = left - skip;
        if (df->defer_items && children >= df->defer_items && children <= body &&
            (d[pos + skip] <= 0x7f || (d[pos + skip] >= 0xcc && d[pos + skip] <= 0xcf)))
          cand = FBM_WIRE_LOM;
        else if (df->defer_items_jl && children >= df->defer_items_jl && children <= body / FBM_WIRE_JL_ITEM_MIN &&
                 memcmp(d + pos + skip, FBM_WIRE_PREFIX, FBM_WIRE_PREFIX_LEN) == 0 &&
                 (d[pos + skip + FBM_WIRE_PREFIX_LEN] == 0xc4 || d[pos + skip + FBM_WIRE_PREFIX_LEN] == 0xc5))
          cand = FBM_WIRE_JL;  // (children >= 1 and 23 children <= body: the 21 bytes compared lie inside the message)
      }
      if (cand >= 0) {
        const uint64_t k = candidates++;
        if (k >= df->n_resolved) {
          if (df->pending) df->pending->begin = pos, df->pending->first = pos + skip, df->pending->n_items = children;
          if (df->pending2) {
            df->pending2->begin = pos, df->pending2->first = pos + skip, df->pending2->n_items = children;
            df->pending2->scheme = cand, df->pending2->pad = 0;
          }
          o->n_arrays = o->n_ckpt = 0;
          return FBM_WIRE_SCAN_PENDING;
        }
        const uint64_t end = df->resolved[k];
        if (end) {
          if (end <= pos + skip || end > len) {
            o->n_arrays = o->n_ckpt = 0;
            return FBM_WIRE_SCAN_BAD_END;
          }
          if (o->n_arrays >= o->arrays_cap) {
            o->n_arrays = o->n_ckpt = 0;
            return FBM_WIRE_SCAN_FULL;
          }
          fbm_wire_array* a = &o->arrays[o->n_arrays++];
          a->begin = pos, a->end = end, a->n_items = children;
          a->ckpt_first = o->n_ckpt, a->ckpt_count = 0;
          a->scheme = cand, a->pad = 1;  // the table is on the device
          pos = end;
          continue;
        }
      }
      if (is_array && children >= min_items) {
        uint64_t end = 0;
        const int r = fbm_wire_candidate(d, len, pos, pos + skip, children, o, &end);
        if (r < 0) {
          o->n_arrays = o->n_ckpt = 0;
          return FBM_WIRE_SCAN_FULL;
        }
        if (r > 0) {
          pos = end;
          continue;
        }
      }
      pos += skip;
      if (children) {
        if (depth >= FBM_WIRE_MAX_DEPTH) goto gave_up;
        stack[depth++] = children;
      }
    }
  }
  if (pos != len) goto gave_up;  // trailing bytes: msgpack raises ExtraData
  return FBM_OK;
gave_up:
  o->n_arrays = o->n_ckpt = 0;
  return FBM_WIRE_SCAN_GAVE_UP;
}

// ---- the same pass over a message's PREFIX (fbm_wire_scan_prefix) ------------------------------------------------
// What fbm_wire_scan_deferred2 with n_resolved = 0 answers for the whole message, as far as its first len bytes decide it:
// FBM_WIRE_SCAN_PENDING with the first deferral candidate once its header and the bytes that make it a candidate are in
// (1 byte behind the header for a native first item, 21 for a map), FBM_OK where the prefix is a whole message without
// one, FBM_WIRE_SCAN_GAVE_UP for what no further byte mends (c1, the nesting bound, bytes behind the message's end),
// and FBM_WIRE_SCAN_MORE wherever the pass would read at or past len.  The candidate test "the items at their
// smallest fit the bytes left" needs the message's length and is not made.  An array of at least min_items items that
// is no candidate is walked item by item as fbm_wire_candidate walks it -- accepted whole, the pass goes on behind it
// without the nesting depth its items would take --, nothing being recorded.
#define FBM_WIRE_SCAN_MORE 5

// fbm_wire_item over a prefix: the item's byte count, 0 where no further byte makes it an accepted form, -1 where
// that takes bytes at or past len
static inline int64_t fbm_wire_item_prefix(const uint8_t* d, uint64_t pos, uint64_t len) {
  if (pos >= len) return -1;
  const uint64_t left = len - pos;
  const uint8_t b = d[pos];
  if (b <= 0x7f) return 1;
  if (b >= 0xcc && b <= 0xcf) {
    const uint32_t w = 1u << (b - 0xcc);
    return left < 1ull + w ? -1 : (int64_t)(1ull + w);
  }
  const uint64_t have = left < FBM_WIRE_PREFIX_LEN ? left : FBM_WIRE_PREFIX_LEN;
  if (memcmp(d + pos, FBM_WIRE_PREFIX, have) != 0) return 0;
  if (left < FBM_WIRE_PREFIX_LEN + 1) return -1;
  const uint64_t p = pos + FBM_WIRE_PREFIX_LEN;
  uint64_t v;
  uint32_t L;
  if (d[p] == 0xc4) {
    if (len - p < 2) return -1;
    L = d[p + 1], v = p + 2;
  } else if (d[p] == 0xc5) {
    if (len - p < 3) return -1;
    L = ((uint32_t)d[p + 1] << 8) | d[p + 2], v = p + 3;
  } else {
    return 0;
  }
  if (L < 1 || L > 257) return 0;
  if (v >= len) return -1;
  if (d[v] >= 0x80 || (L == 257 && d[v] != 0)) return 0;
  if (len - v < L) return -1;
  return (int64_t)(v + L - pos);
}

static inline int fbm_wire_scan_prefix_run(const uint8_t* d, uint64_t len, uint64_t min_items, uint64_t defer_items,
                                           uint64_t defer_items_jl, fbm_wire_pending2* pending) {
  uint64_t stack[FBM_WIRE_MAX_DEPTH];
  int depth = 1;
  uint64_t pos = 0;
  stack[0] = 1;
  if (min_items < 1) min_items = 1;
  while (depth > 0) {
    if (stack[depth - 1] == 0) {
      --depth;
      continue;
    }
    --stack[depth - 1];
    if (pos >= len) return FBM_WIRE_SCAN_MORE;
    const uint8_t b = d[pos];
    const uint64_t left = len - pos;
    uint64_t skip = 0, children = 0;
    int container = 0, is_array = 0;
    if (b <= 0x7f || b >= 0xe0 || b == 0xc0 || b == 0xc2 || b == 0xc3) {
      skip = 1;
    } else if (b <= 0x8f) {
      container = 1, skip = 1, children = 2ull * (b & 0x0f);
    } else if (b <= 0x9f) {
      container = 1, is_array = 1, skip = 1, children = b & 0x0f;
    } else if (b <= 0xbf) {
      skip = 1ull + (b & 0x1f);
    } else {
      int lb = 0;
      uint64_t extra = 0;
      switch (b) {
        case 0xc4: case 0xd9: lb = 1; break;
        case 0xc5: case 0xda: lb = 2; break;
        case 0xc6: case 0xdb: lb = 4; break;
        case 0xc7: lb = 1, extra = 1; break;
        case 0xc8: lb = 2, extra = 1; break;
        case 0xc9: lb = 4, extra = 1; break;
        case 0xca: case 0xce: case 0xd2: skip = 5; break;
        case 0xcb: case 0xcf: case 0xd3: skip = 9; break;
        case 0xcc: case 0xd0: skip = 2; break;
        case 0xcd: case 0xd1: skip = 3; break;
        case 0xd4: skip = 3; break;
        case 0xd5: skip = 4; break;
        case 0xd6: skip = 6; break;
        case 0xd7: skip = 10; break;
        case 0xd8: skip = 18; break;
        case 0xdc: container = 1, is_array = 1, lb = 2; break;
        case 0xdd: container = 1, is_array = 1, lb = 4; break;
        case 0xde: container = 1, lb = 2; break;
        case 0xdf: container = 1, lb = 4; break;
        default: return FBM_WIRE_SCAN_GAVE_UP;  // 0xc1
      }
      if (lb) {
        if (left < 1ull + lb) return FBM_WIRE_SCAN_MORE;
        const uint64_t v = fbm_wire_be(d + pos + 1, lb);
        if (container)
          skip = 1ull + lb, children = is_array ? v : 2 * v;
        else
          skip = 1ull + lb + extra + v;
      }
    }
    if (left < skip) return FBM_WIRE_SCAN_MORE;
    if (!container) {
      pos += skip;
      continue;
    }
    if (is_array && children >= min_items) {
      const uint64_t first = pos + skip;
      int cand = -1;
      if (first >= len) return FBM_WIRE_SCAN_MORE;  // (the array's first byte decides)
      const uint8_t f = d[first];
      if (defer_items && children >= defer_items && (f <= 0x7f || (f >= 0xcc && f <= 0xcf))) {
        cand = FBM_WIRE_LOM;
      } else if (defer_items_jl && children >= defer_items_jl) {
        const uint64_t have = len - first < FBM_WIRE_PREFIX_LEN ? len - first : FBM_WIRE_PREFIX_LEN;
        if (memcmp(d + first, FBM_WIRE_PREFIX, have) == 0) {
          if (len - first < FBM_WIRE_PREFIX_LEN + 1) return FBM_WIRE_SCAN_MORE;
          if (d[first + FBM_WIRE_PREFIX_LEN] == 0xc4 || d[first + FBM_WIRE_PREFIX_LEN] == 0xc5) cand = FBM_WIRE_JL;
        }
      }
      if (cand >= 0) {
        pending->begin = pos, pending->first = first, pending->n_items = children;
        pending->scheme = cand, pending->pad = 0;
        return FBM_WIRE_SCAN_PENDING;
      }
      uint64_t p = first, i = 0;  // fbm_wire_candidate's walk
      for (; i < children; ++i) {
        const int64_t c = fbm_wire_item_prefix(d, p, len);
        if (c < 0) return FBM_WIRE_SCAN_MORE;
        if (c == 0) break;
        p += (uint64_t)c;
      }
      if (i == children) {
        pos = p;
        continue;
      }
    }
    pos += skip;
    if (children) {
      if (depth >= FBM_WIRE_MAX_DEPTH) return FBM_WIRE_SCAN_GAVE_UP;
      stack[depth++] = children;
    }
  }
  return pos == len ? FBM_OK : FBM_WIRE_SCAN_GAVE_UP;  // trailing bytes: msgpack raises ExtraData
}

static inline int fbm_wire_scan_impl(const uint8_t* d, uint64_t len, uint64_t min_items, fbm_wire_scan_out* o) {
  return fbm_wire_scan_run(d, len, min_items, o, nullptr);
}

// Host check of fbm_wire_tokenize_jl's work (wire_tokenize_jl_host in fedbiomed_amd/csrc/fbm_wire.hpp: the routine the
// test build's fbm_test_wire_tokenize_jl runs, over the kernels' own per-tile routines) and of
// fbm_wire_scan_deferred2's pass (fbm_wire_scan_run in fbm_wire_scan.hpp) under the host sanitizers: the bytes come
// from the network.  Builds arrays of big-int maps -- every size class (L = 1, 9, 10, 255 as bin8; 255, 256, 257 as
// bin16) alone and mixed, a header across the tile boundary at each split, an item ending and one starting on it,
// values that hold a whole item or 82 bytes only, more tiles than the scan has threads -- takes table and end from
// the scanner's record and compares; then tokenizes under seeded mutations of the bytes, of `first`, of n_items and
// of the span's length, each compared with a sequential walk of fbm_wire_item that stops at the first item that is
// not the map form; then drives the deferring pass with the ends found, with zeros and with wrong ends.  Span,
// table, result and workspace each sit in a heap block of exactly their size, the span at every address residue mod
// 4 in turn, so any access outside them is an AddressSanitizer report.  A stand-alone program: it is never loaded
// into Python.
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -Iinclude tools/wire_tokenize_jl_check.cpp -o wire_tokenize_jl_check && ./wire_tokenize_jl_check [mutations, default 1500]
#include <sanitizer/asan_interface.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../fedbiomed_amd/csrc/fbm_wire.hpp"
#include "../fedbiomed_amd/csrc/fbm_wire_scan.hpp"

typedef std::string Bytes;

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {  // xorshift64*
  g_state ^= g_state >> 12, g_state ^= g_state << 25, g_state ^= g_state >> 27;
  return g_state * 0x2545f4914f6cdd1dull;
}

static void be(Bytes& o, uint64_t v, int bytes) {
  for (int i = bytes - 1; i >= 0; --i) o.push_back((char)(v >> (8 * i)));
}
// a map item of L value bytes, as bin16 where wide (or L > 255); the value's bytes behind the first are `fill` (-1: random)
static void item(Bytes& o, unsigned L, bool wide, int fill) {
  o.append((const char*)FBM_WIRE_PREFIX, FBM_WIRE_PREFIX_LEN);
  if (wide || L > 255) o.push_back((char)0xc5), be(o, L, 2);
  else o.push_back((char)0xc4), o.push_back((char)L);
  o.push_back((char)(L == 257 ? 0 : rnd() & 0x7f));
  for (unsigned i = 1; i < L; ++i) o.push_back((char)(fill < 0 ? rnd() : fill));
}
// an item of exactly `size` bytes, 23..280
static void sized(Bytes& o, unsigned size) {
  if (size <= 277) item(o, size - 22, false, -1);
  else item(o, size - 23, true, -1);
}
// items of exactly `total` bytes together (0, or at least 46); returns how many
static uint64_t filling(Bytes& o, uint64_t total) {
  uint64_t n = 0;
  for (; total > 560; total -= 280, ++n) sized(o, 280);
  if (total > 280) sized(o, (unsigned)(total / 2)), total -= total / 2, ++n;
  if (total) sized(o, (unsigned)total), ++n;
  return n;
}

static void expect(bool cond, const char* what) {
  if (!cond) {
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
  }
}

struct Answer {
  uint64_t count, end;
  std::vector<uint64_t> table;
};

// the sequential walk over span[0, span_len) from absolute offset first: fbm_wire_item, the map form only
static Answer walk(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n) {
  Answer a = {0, 0, {}};
  uint64_t p = first - base, voff = 0;
  uint32_t vlen = 0;
  int native = 0;
  while (a.count < n) {
    const uint64_t c = fbm_wire_item(span, p, span_len, &voff, &vlen, &native);
    if (c == 0 || native) break;
    a.table.push_back((base + voff) << 16 | vlen);
    p += c, ++a.count;
  }
  if (a.count == n) a.end = base + p;
  return a;
}

// one tokenize over exactly-sized blocks, the span's first byte at every address residue mod 4 in turn
static long g_calls = 0;
static Answer tokenize(const uint8_t* bytes, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n) {
  const unsigned shift = (unsigned)(g_calls++ & 3);
  uint8_t* block = (uint8_t*)malloc(span_len + shift);  // malloc's blocks are 16-byte aligned: the span starts `shift` in,
  uint8_t* s = block + shift;                           // and the bytes in front of it are poisoned: not the span's
  memcpy(s, bytes, span_len);
  ASAN_POISON_MEMORY_REGION(block, shift);
  uint64_t* c = (uint64_t*)malloc(n ? n * 8 : 1);
  uint64_t* r = (uint64_t*)malloc(16);
  void* w = malloc(fbm::wire_tokj_workspace_of(fbm::wire_tok_cut_of(s, span_len, first - base).tiles));  // exactly what is used
  fbm::wire_tokenize_jl_host(s, span_len, base, first, n, c, n, r, w);
  Answer a = {r[0], r[1], {}};
  if (a.count == n) a.table.assign(c, c + n);
  ASAN_UNPOISON_MEMORY_REGION(block, shift);
  free(block), free(c), free(r), free(w);
  return a;
}

static void same(const Answer& got, const Answer& want, const char* what) {
  expect(got.count == want.count, what);
  expect(got.end == want.end, what);
  if (want.end) expect(got.table == want.table, what);  // (all n items: the table counts)
}

static Bytes message(const Bytes& items, uint64_t n, uint64_t* begin, uint64_t* first) {
  Bytes msg("\x83\xa2id\xa7node-07\xa6params", 19);  // fixmap{"id": "node-07", "params": [...], and a third pair main() appends}
  *begin = msg.size();
  if (n <= 15) msg.push_back((char)(0x90 | n));
  else if (n <= 65535) msg.push_back((char)0xdc), be(msg, n, 2);
  else msg.push_back((char)0xdd), be(msg, n, 4);
  *first = msg.size();
  return msg + items;
}

int main(int argc, char** argv) {
  const long mutations = argc > 1 ? atol(argv[1]) : 1500;
  std::vector<std::pair<Bytes, uint64_t>> arrays;  // (items' bytes, n)
  const unsigned cls[7][2] = {{1, 0}, {9, 0}, {10, 0}, {255, 0}, {255, 1}, {256, 1}, {257, 1}};
  for (const auto& c : cls) {  // every size class alone
    Bytes it;
    for (int i = 0; i < 40; ++i) item(it, c[0], c[1] != 0, -1);
    arrays.push_back({it, 40});
  }
  for (uint64_t n : {1ull, 2ull, 150ull}) {  // mixed
    Bytes it;
    for (uint64_t i = 0; i < n; ++i) {
      const auto& c = cls[rnd() % 7];
      item(it, c[0], c[1] != 0, -1);
    }
    arrays.push_back({it, n});
  }
  // a header across the first tile boundary with s of its bytes in front (0: starts on it; 23: a bin16 header ends on
  // it), and an item that ends on it.  (The boundary lies FBM_WIRE_TOK_TILE bytes behind item 0 where item 0's address is a
  // multiple of 4; tokenize() shifts the span through all four residues.)
  for (uint64_t s = 0; s <= 24; ++s) {
    Bytes it;
    uint64_t n = filling(it, FBM_WIRE_TOK_TILE - (s == 24 ? 0 : s));
    if (s < 24) item(it, s % 2 ? 257 : 200, true, -1), ++n;
    n += filling(it, 600);
    arrays.push_back({it, n});
  }
  for (int fill : {0x82, 0xa8, 0xc4, 0x00}) {  // values of marker bytes only
    Bytes it;
    for (int i = 0; i < 40; ++i) item(it, 257, true, fill);
    arrays.push_back({it, 40});
  }
  for (uint64_t at : {30ull, 150ull, 279ull}) {  // a value that holds a whole item, the decoy's first byte at offset `at` of tile 1
    Bytes it, decoy, carrier;
    item(decoy, 3, false, 0x02);
    uint64_t n = filling(it, FBM_WIRE_TOK_TILE + at - 123);
    carrier.append((const char*)FBM_WIRE_PREFIX, FBM_WIRE_PREFIX_LEN);
    carrier.push_back((char)0xc5), be(carrier, 257, 2);
    carrier += Bytes(100, '\0') + decoy + Bytes(257 - 100 - decoy.size(), '\x22');
    it += carrier, ++n;
    n += filling(it, 700);
    arrays.push_back({it, n});
  }
  {  // more tiles than the scan has threads: runs of two tiles, chained by thread 0
    Bytes it;
    uint64_t n = 0;
    for (; it.size() < 258ull * FBM_WIRE_TOK_TILE + 100; ++n) item(it, n % 3 ? 257 : 120, false, (int)(n & 0xff));
    arrays.push_back({it, n});
  }

  long runs = 0, passes = 0;
  for (const auto& arr : arrays) {
    const uint64_t n = arr.second;
    uint64_t begin, first;
    Bytes tail;
    item(tail, 40, false, -1);  // what follows the array, the third pair's value, is an accepted item itself
    Bytes msg = message(arr.first, n, &begin, &first) + Bytes("\xa1v", 2) + tail;
    const uint8_t* d = (const uint8_t*)msg.data();
    // the scanner's record of the array: table and end
    std::vector<fbm_wire_array> rec(4);
    std::vector<uint64_t> table(n + 1024);
    fbm_wire_scan_out o = {rec.data(), rec.size(), 0, table.data(), table.size(), 0};
    expect(fbm_wire_scan_impl(d, msg.size(), 1, &o) == FBM_OK && o.n_arrays == 1, "the message scans");
    expect(rec[0].begin == begin && rec[0].n_items == n && rec[0].scheme == FBM_WIRE_JL && rec[0].pad == 0 && o.n_ckpt == n,
           "recorded as maps");
    const Answer want = {n, rec[0].end, std::vector<uint64_t>(table.begin(), table.begin() + o.n_ckpt)};
    same(walk(d, msg.size(), 0, first, n), want, "the walk is the scanner's");
    same(tokenize(d, msg.size(), 0, first, n), want, "whole message as the span");
    same(tokenize(d + begin, msg.size() - begin, begin, first, n), want, "the message from the array's header on");
    same(tokenize(d + first, rec[0].end - first, first, first, n), want, "the items alone");
    runs += 3;
    for (int k = 0; k < 4; ++k, ++runs)  // the same span at the other address residues
      same(tokenize(d + begin, msg.size() - begin, begin, first, n), want, "every residue");
    // the deferring pass: pending with the scheme, then the end the tokenizer found; zeros; wrong ends
    {
      uint64_t resolved[1] = {0};
      fbm_wire_pending2 pend = {0, 0, 0, -1, -1};
      std::vector<fbm_wire_array> rec2(4);
      std::vector<uint64_t> table2(table.size());
      fbm_wire_scan_out o2 = {rec2.data(), rec2.size(), 0, table2.data(), table2.size(), 0};
      fbm_wire_defer df = {0, resolved, 0, nullptr, 1, &pend};
      expect(fbm_wire_scan_run(d, msg.size(), 1, &o2, &df) == FBM_WIRE_SCAN_PENDING && o2.n_arrays == 0, "pending");
      expect(pend.begin == begin && pend.first == first && pend.n_items == n && pend.scheme == FBM_WIRE_JL && pend.pad == 0,
             "the pending array");
      df.n_resolved = 1;
      resolved[0] = want.end;
      expect(fbm_wire_scan_run(d, msg.size(), 1, &o2, &df) == FBM_OK && o2.n_arrays == 1 && o2.n_ckpt == 0, "resolved");
      expect(rec2[0].begin == begin && rec2[0].end == want.end && rec2[0].n_items == n && rec2[0].pad == 1 &&
                 rec2[0].ckpt_count == 0 && rec2[0].scheme == FBM_WIRE_JL, "recorded with its table on the device");
      resolved[0] = 0;
      expect(fbm_wire_scan_run(d, msg.size(), 1, &o2, &df) == FBM_OK && o2.n_arrays == 1 && o2.n_ckpt == o.n_ckpt &&
                 memcmp(&rec2[0], &rec[0], sizeof(rec[0])) == 0 && memcmp(table2.data(), table.data(), o.n_ckpt * 8) == 0,
             "resolved as 0: the plain scan word for word");
      for (uint64_t bad : {first, first - 1, (uint64_t)msg.size() + 1, (uint64_t)~0ull}) {
        resolved[0] = bad;
        expect(fbm_wire_scan_run(d, msg.size(), 1, &o2, &df) == FBM_WIRE_SCAN_BAD_END && o2.n_arrays == 0, "a wrong end");
      }
      passes += 7;
    }
    if (msg.size() > 100000) continue;  // (the large array: no mutations)
    for (long k = 0; k < mutations; ++k, ++runs) {
      Bytes m = msg;
      uint64_t len = m.size(), base = 0, f = first, items = n;
      const int kind = (int)(rnd() % 7);
      if (kind == 0) m[first + rnd() % (len - first)] = (char)rnd();                               // a byte
      else if (kind == 1) m[first + rnd() % (len - first)] = "\x82\xc4\xc5\xc6\x80\x00\x01\xa8"[rnd() % 8];  // a marker
      else if (kind == 2) len = first + 1 + rnd() % (len - first);                                // a truncated span
      else if (kind == 3) f = first + rnd() % (len - first);                                      // another first, inside the span
      else if (kind == 4) items = 1 + rnd() % (2 * n + 70);                                       // another item count
      else if (kind == 5) base = rnd() % (first + 1);                                             // the span starts later
      else {  // a header byte of a random item: where the chain looks
        const uint64_t i = rnd() % n, at = (table[i] >> 16) - 1 - rnd() % 23;
        if (at >= first) m[at] = (char)(rnd() % 3 ? rnd() : m[at] ^ 1);
      }
      const uint8_t* md = (const uint8_t*)m.data();
      const Answer w = walk(md + base, len - base, base, f, items);
      const Answer got = tokenize(md + base, len - base, base, f, items);
      same(got, w, "a mutation: the tokenizer is the sequential walk");
      // the same mutated message through the deferring pass, answered by the tokenizer: never outside its tables
      if (kind <= 2 || kind == 6) {
        uint64_t resolved[FBM_WIRE_MAX_DEFERRED + 1] = {0};
        fbm_wire_pending2 pend = {0, 0, 0, 0, 0};
        fbm_wire_array* rec2 = (fbm_wire_array*)malloc(2 * sizeof(fbm_wire_array));
        uint64_t* table2 = (uint64_t*)malloc((len / 8 + 8) * 8);
        fbm_wire_scan_out o2 = {rec2, 2, 0, table2, len / 8 + 8, 0};
        fbm_wire_defer df = {8, resolved, 0, nullptr, 8, &pend};
        uint8_t* exact = (uint8_t*)malloc(len);
        memcpy(exact, md, len);
        int r;
        while ((r = fbm_wire_scan_run(exact, len, 1, &o2, &df)) == FBM_WIRE_SCAN_PENDING && df.n_resolved < FBM_WIRE_MAX_DEFERRED) {
          expect(pend.first < len && pend.n_items <= len - pend.first, "a pending array fits the message");
          expect(pend.scheme == FBM_WIRE_LOM || pend.n_items * FBM_WIRE_JL_ITEM_MIN <= len - pend.first, "no table sized by a lying header");
          Answer t = {0, 0, {}};
          if (pend.scheme == FBM_WIRE_JL) t = tokenize(exact, len, 0, pend.first, pend.n_items);
          resolved[df.n_resolved++] = t.count == pend.n_items ? t.end : 0;
          ++passes;
        }
        expect(r != FBM_WIRE_SCAN_BAD_END && r != FBM_WIRE_SCAN_PENDING, "the tokenizer's ends are accepted");
        free(rec2), free(table2), free(exact);
      }
    }
  }
  printf("wire_tokenize_jl_check: %ld tokenizer runs and %ld scanner passes over %zu arrays; no finding\n", runs, passes,
         arrays.size());
  return 0;
}

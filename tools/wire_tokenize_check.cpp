// Host check of fbm_wire_tokenize_lom's work (wire_tokenize_host in fedbiomed_amd/csrc/fbm_wire.hpp: the routine the
// test build's fbm_test_wire_tokenize_lom runs, over the kernels' own per-block routines) and of
// fbm_wire_scan_deferred's pass (fbm_wire_scan_run in fbm_wire_scan.hpp) under the host sanitizers: the bytes come
// from the network.  Builds arrays of native items -- every width, non-minimal forms, only 1-byte items, only
// 9-byte items whose payloads look like markers, items on the sub-block, tile and run boundaries, more tiles than
// the scan has threads -- takes table and end from the scanner's sequential walk and compares; then tokenizes under
// seeded mutations of the bytes, of `first`, of n_items and of the span's length, each compared with a plain
// sequential walk; then drives the deferring pass with the ends found, with zeros and with wrong ends.  Span,
// table, result and workspace each sit in a heap block of exactly their size, so any access outside them is an
// AddressSanitizer report.  A stand-alone program: it is never loaded into Python.
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -Iinclude tools/wire_tokenize_check.cpp -o wire_tokenize_check && ./wire_tokenize_check [mutations, default 3000]
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
// an item of `width` value bytes (0: the byte itself) whose payload bytes are `fill` (-1: random)
static void native(Bytes& o, int width, int fill) {
  static const unsigned char tag[9] = {0, 0xcc, 0xcd, 0, 0xce, 0, 0, 0, 0xcf};
  if (width == 0) {
    o.push_back((char)(rnd() & 0x7f));
    return;
  }
  o.push_back((char)tag[width]);
  for (int i = 0; i < width; ++i) o.push_back((char)(fill < 0 ? rnd() : fill));
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

// the sequential walk over span[0, span_len) from absolute offset first (span_base + index)
static Answer walk(const uint8_t* span, uint64_t span_len, uint64_t base, uint64_t first, uint64_t n) {
  Answer a = {0, 0, {}};
  uint64_t p = first - base;
  while (a.count < n && p < span_len) {
    const uint8_t b = span[p];
    const uint64_t l = b <= 0x7f ? 1 : b == 0xcc ? 2 : b == 0xcd ? 3 : b == 0xce ? 5 : b == 0xcf ? 9 : 0;
    if (l == 0 || span_len - p < l) break;
    if (a.count % FBM_WIRE_LOM_GROUP == 0) a.table.push_back(base + p);
    p += l, ++a.count;
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
  const uint64_t n_ckpt = (n + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP;
  uint64_t* c = (uint64_t*)malloc(n_ckpt ? n_ckpt * 8 : 1);
  uint64_t* r = (uint64_t*)malloc(16);
  void* w = malloc(fbm::wire_tok_maps_at(fbm::wire_tok_cut_of(s, span_len, first - base).tiles) +
                   fbm::wire_tok_cut_of(s, span_len, first - base).tiles * FBM_WIRE_TOK_MAP * 4);  // exactly what is used
  fbm::wire_tokenize_host(s, span_len, base, first, n, c, n_ckpt, r, w);
  Answer a = {r[0], r[1], {}};
  if (a.count == n) a.table.assign(c, c + n_ckpt);
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
  Bytes msg("\x83\xa2id\xa7node-07\xa6params", 19);  // fixmap{"id": "node-07", "params": [...], "round": 3}
  *begin = msg.size();
  if (n <= 15) msg.push_back((char)(0x90 | n));
  else if (n <= 65535) msg.push_back((char)0xdc), be(msg, n, 2);
  else msg.push_back((char)0xdd), be(msg, n, 4);
  *first = msg.size();
  return msg + items;
}

int main(int argc, char** argv) {
  const long mutations = argc > 1 ? atol(argv[1]) : 3000;
  std::vector<std::pair<Bytes, uint64_t>> arrays;  // (items' bytes, n)
  const int widths[] = {0, 1, 2, 4, 8};
  for (uint64_t n : {1ull, 63ull, 64ull, 65ull, 129ull, 1025ull, 5000ull}) {  // every width, random payloads
    Bytes it;
    for (uint64_t i = 0; i < n; ++i) native(it, widths[rnd() % 5], -1);
    arrays.push_back({it, n});
  }
  {
    Bytes it;
    for (int i = 0; i < 300; ++i) native(it, 0, -1);  // 64 items in one sub-block
    arrays.push_back({it, 300});
  }
  for (int fill : {0xcf, 0xcc, 0x82, 0xc1, 0x00}) {  // payloads that look like markers
    Bytes it;
    for (int i = 0; i < 130; ++i) native(it, 8, fill);
    arrays.push_back({it, 130});
  }
  // a 9-byte item ending on, spanning and starting on the sub-block, tile and run boundaries (the run: 2 tiles, with 258)
  const uint64_t bounds[3][2] = {{FBM_WIRE_TOK_SUB, 200}, {FBM_WIRE_TOK_TILE, FBM_WIRE_TOK_TILE + 200},
                                 {2 * FBM_WIRE_TOK_TILE, 257 * FBM_WIRE_TOK_TILE + 100}};
  for (const auto& bd : bounds)
    for (uint64_t start : {bd[0] - 9, bd[0] - 4, bd[0]}) {
      Bytes it;
      uint64_t n = 0;
      for (; it.size() < start; ++n) native(it, 0, -1);
      native(it, 8, 0xcf), ++n;
      for (; it.size() + 9 <= bd[1]; ++n) native(it, 8, 0x00);
      arrays.push_back({it, n});
    }

  long runs = 0, passes = 0;
  for (const auto& arr : arrays) {
    const uint64_t n = arr.second;
    uint64_t begin, first;
    Bytes msg = message(arr.first, n, &begin, &first) + Bytes("\xa5round\x03", 7);
    const uint8_t* d = (const uint8_t*)msg.data();
    // the scanner's record of the array: table and end
    std::vector<fbm_wire_array> rec(4);
    std::vector<uint64_t> table(msg.size() / 8 + 1024);
    fbm_wire_scan_out o = {rec.data(), rec.size(), 0, table.data(), table.size(), 0};
    expect(fbm_wire_scan_impl(d, msg.size(), 1, &o) == FBM_OK && o.n_arrays == 1, "the message scans");
    expect(rec[0].begin == begin && rec[0].n_items == n && rec[0].scheme == FBM_WIRE_LOM && rec[0].pad == 0, "recorded as native");
    const Answer want = {n, rec[0].end, std::vector<uint64_t>(table.begin(), table.begin() + o.n_ckpt)};
    same(walk(d, msg.size(), 0, first, n), want, "the walk is the scanner's");
    same(tokenize(d, msg.size(), 0, first, n), want, "whole message as the span");
    same(tokenize(d + begin, msg.size() - begin, begin, first, n), want, "the message from the array's header on");
    same(tokenize(d + first, rec[0].end - first, first, first, n), want, "the items alone");
    runs += 3;
    // the deferring pass: pending, then the end the tokenizer found; zeros; wrong ends
    {
      uint64_t resolved[1] = {0};
      fbm_wire_pending pend = {0, 0, 0};
      std::vector<fbm_wire_array> rec2(4);
      std::vector<uint64_t> table2(table.size());
      fbm_wire_scan_out o2 = {rec2.data(), rec2.size(), 0, table2.data(), table2.size(), 0};
      fbm_wire_defer df = {1, resolved, 0, &pend};
      expect(fbm_wire_scan_run(d, msg.size(), 1, &o2, &df) == FBM_WIRE_SCAN_PENDING && o2.n_arrays == 0, "pending");
      expect(pend.begin == begin && pend.first == first && pend.n_items == n, "the pending array");
      df.n_resolved = 1;
      resolved[0] = want.end;
      expect(fbm_wire_scan_run(d, msg.size(), 1, &o2, &df) == FBM_OK && o2.n_arrays == 1 && o2.n_ckpt == 0, "resolved");
      expect(rec2[0].begin == begin && rec2[0].end == want.end && rec2[0].n_items == n && rec2[0].pad == 1 &&
                 rec2[0].ckpt_count == 0 && rec2[0].scheme == FBM_WIRE_LOM, "recorded with its table on the device");
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
    if (msg.size() > 100000) continue;  // (the large arrays: no mutations)
    for (long k = 0; k < mutations; ++k, ++runs) {
      Bytes m = msg;
      uint64_t len = m.size(), base = 0, f = first, items = n;
      const int kind = (int)(rnd() % 6);
      if (kind == 0) m[first + rnd() % (len - first)] = (char)rnd();                           // a byte
      else if (kind == 1) m[first + rnd() % (len - first)] = "\xc1\x82\xcf\xcc\xe0\xd0"[rnd() % 6];  // a marker or a non-native byte
      else if (kind == 2) len = first + 1 + rnd() % (len - first);                            // a truncated span
      else if (kind == 3) f = first + rnd() % (len - first);                                  // another first, inside the span
      else if (kind == 4) items = 1 + rnd() % (2 * n + 70);                                   // another item count
      else base = rnd() % (first + 1);                                                         // the span starts later
      const uint8_t* md = (const uint8_t*)m.data();
      const Answer w = walk(md + base, len - base, base, f, items);
      const Answer got = tokenize(md + base, len - base, base, f, items);
      same(got, w, "a mutation: the tokenizer is the sequential walk");
      // the same mutated message through the deferring pass, answered by the tokenizer: never outside its tables
      if (kind <= 2) {
        uint64_t resolved[FBM_WIRE_MAX_DEFERRED + 1] = {0};
        fbm_wire_pending pend = {0, 0, 0};
        fbm_wire_array* rec2 = (fbm_wire_array*)malloc(2 * sizeof(fbm_wire_array));
        uint64_t* table2 = (uint64_t*)malloc((len / 8 + 8) * 8);
        fbm_wire_scan_out o2 = {rec2, 2, 0, table2, len / 8 + 8, 0};
        fbm_wire_defer df = {32, resolved, 0, &pend};
        uint8_t* exact = (uint8_t*)malloc(len);
        memcpy(exact, md, len);
        int r;
        while ((r = fbm_wire_scan_run(exact, len, 1, &o2, &df)) == FBM_WIRE_SCAN_PENDING && df.n_resolved < FBM_WIRE_MAX_DEFERRED) {
          expect(pend.first < len && pend.n_items <= len - pend.first, "a pending array fits the message");
          const Answer t = tokenize(exact, len, 0, pend.first, pend.n_items);
          resolved[df.n_resolved++] = t.count == pend.n_items ? t.end : 0;
          ++passes;
        }
        expect(r != FBM_WIRE_SCAN_BAD_END && r != FBM_WIRE_SCAN_PENDING, "the tokenizer's ends are accepted");
        free(rec2), free(table2), free(exact);
      }
    }
  }
  printf("wire_tokenize_check: %ld tokenizer runs and %ld scanner passes over %zu arrays; no finding\n", runs, passes,
         arrays.size());
  return 0;
}

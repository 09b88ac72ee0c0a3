// Host check of fbm_wire_fold_lom's work (wire_fold_lom_groups in fedbiomed_amd/csrc/fbm_wire.hpp: the routine the
// test build's fbm_test_wire_fold_lom runs, over the kernel's own per-item walk) under the host sanitizers: the
// span's bytes come from the network and the table need not be the scanner's.  Builds arrays of native items of
// every width and non-minimal form, takes their tables from the scanner (fbm_wire_scan.hpp), folds them and
// compares with the sum of the values; then folds under seeded mutations of the table, of the span's length and of
// its bytes -- span, table and accumulator each in a heap block of exactly its length, so any access outside them
// is an AddressSanitizer report -- and checks that a group whose checkpoint lies outside the span leaves the
// accumulator as it was (or zero on a first call).  A stand-alone program: it is never loaded into Python.
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -Iinclude tools/wire_fold_check.cpp -o wire_fold_check && ./wire_fold_check [mutations, default 4000]
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
// v in the form of `width` value bytes (0: the byte itself), minimal or not
static void native(Bytes& o, uint64_t v, int width) {
  static const unsigned char tag[9] = {0, 0xcc, 0xcd, 0, 0xce, 0, 0, 0, 0xcf};
  if (width == 0) o.push_back((char)v);
  else o.push_back((char)tag[width]), be(o, v, width);
}
static int min_width(uint64_t v) { return v <= 127 ? 0 : v < (1ull << 8) ? 1 : v < (1ull << 16) ? 2 : v < (1ull << 32) ? 4 : 8; }

static void expect(bool cond, const char* what) {
  if (!cond) {
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
  }
}

template <class T>
static T* exact(const T* src, size_t n) {  // exactly n elements: ASan guards the rest
  T* p = (T*)malloc(n ? n * sizeof(T) : 1);
  if (n) memcpy(p, src, n * sizeof(T));
  return p;
}

// one fold over exactly-sized copies; returns the accumulator
static std::vector<uint64_t> fold(const Bytes& span, uint64_t span_len, uint64_t base, const std::vector<uint64_t>& ckpt,
                                  uint64_t n, const std::vector<uint64_t>& acc0, int first) {
  uint8_t* s = exact((const uint8_t*)span.data(), span_len);
  uint64_t* c = exact(ckpt.data(), ckpt.size());
  uint64_t* a = exact(acc0.data(), n);
  fbm::wire_fold_lom_groups(s, span_len, base, c, ckpt.size(), n, a, first, FBM_WIRE_LOM_GROUP);
  std::vector<uint64_t> out(a, a + n);
  free(s), free(c), free(a);
  return out;
}

int main(int argc, char** argv) {
  const long mutations = argc > 1 ? atol(argv[1]) : 4000;
  const uint64_t sizes[] = {1, 63, 64, 65, 127, 128, 129, 257, 1025};
  long folds = 0;
  for (uint64_t n : sizes) {
    // the array inside a message: fixmap{"id": "node-07", "params": [...]}
    Bytes msg("\x82\xa2id\xa7node-07\xa6params", 19);
    const uint64_t begin = msg.size();
    if (n <= 15) msg.push_back((char)(0x90 | n));
    else msg.push_back((char)0xdc), be(msg, n, 2);
    std::vector<uint64_t> vals(n);
    for (uint64_t i = 0; i < n; ++i) {
      const uint64_t v = i % 7 == 0 ? ~0ull >> (rnd() % 64) : rnd() >> (rnd() % 64);
      int w = min_width(v);
      if (rnd() % 4 == 0)  // a non-minimal form: the next wider ones
        while (w < 8 && rnd() % 2) w = w == 0 ? 1 : w * 2;
      native(msg, v, w);
      vals[i] = v;
    }
    const uint64_t end = msg.size();
    std::vector<fbm_wire_array> arrays(4);
    std::vector<uint64_t> table(msg.size() + 16);
    fbm_wire_scan_out o = {arrays.data(), arrays.size(), 0, table.data(), table.size(), 0};
    expect(fbm_wire_scan_impl((const uint8_t*)msg.data(), msg.size(), 1, &o) == FBM_OK && o.n_arrays == 1, "the message scans");
    expect(arrays[0].begin == begin && arrays[0].end == end && arrays[0].n_items == n && arrays[0].scheme == FBM_WIRE_LOM,
           "the array is recorded as native");
    const uint64_t n_ckpt = (n + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP;
    expect(arrays[0].ckpt_count == n_ckpt, "one checkpoint per group");
    const std::vector<uint64_t> ckpt(table.begin() + arrays[0].ckpt_first, table.begin() + arrays[0].ckpt_first + n_ckpt);
    const Bytes span = msg.substr(begin, end - begin);
    std::vector<uint64_t> acc0(n);
    for (uint64_t& a : acc0) a = rnd() % 3 ? rnd() : ~0ull;
    // the scanner's table: the sum, first and continuing, on the array's own span and on the whole message
    for (int first = 0; first < 2; ++first) {
      const std::vector<uint64_t> got = fold(span, span.size(), begin, ckpt, n, acc0, first);
      const std::vector<uint64_t> whole = fold(msg, msg.size(), 0, ckpt, n, acc0, first);
      for (uint64_t i = 0; i < n; ++i)
        expect(got[i] == (first ? 0 : acc0[i]) + vals[i] && whole[i] == got[i], "the fold is the sum");
      folds += 2;
    }
    // mutations: the table, the span's length, the span's bytes
    for (long k = 0; k < mutations; ++k, ++folds) {
      std::vector<uint64_t> t = ckpt;
      Bytes s = span;
      uint64_t len = s.size(), base = begin;
      const int first = (int)(rnd() % 2);
      const int kind = (int)(rnd() % 5);
      const size_t slot = rnd() % t.size();
      if (kind == 0) t[slot] = rnd() % 4 ? begin + rnd() % (len + 8) - 4 : rnd();  // around and inside the span, or anywhere
      else if (kind == 1) t[slot] = end - 1 - rnd() % 3;                           // in the last 3 bytes
      else if (kind == 2) len = rnd() % (len + 1), s.resize(len);                  // a truncated span (0 included)
      else if (kind == 3) s[rnd() % len] = (char)rnd();                            // a byte of the span
      else base = rnd() % 3 ? begin + rnd() % 16 - 8 : rnd();                      // another base
      const std::vector<uint64_t> got = fold(s, len, base, t, n, acc0, first);
      for (size_t g = 0; g < t.size(); ++g) {
        if (t[g] >= base && t[g] - base < len) continue;
        for (uint64_t i = g * FBM_WIRE_LOM_GROUP; i < n && i < (g + 1) * FBM_WIRE_LOM_GROUP; ++i)
          expect(got[i] == (first ? 0 : acc0[i]), "a checkpoint outside the span adds 0");
      }
      if (kind <= 1)  // the other groups stand
        for (size_t g = 0; g < t.size(); ++g)
          if (g != slot)
            for (uint64_t i = g * FBM_WIRE_LOM_GROUP; i < n && i < (g + 1) * FBM_WIRE_LOM_GROUP; ++i)
              expect(got[i] == (first ? 0 : acc0[i]) + vals[i], "groups with their own checkpoint keep their sum");
    }
  }
  printf("wire_fold_check: %ld folds over %zu array sizes; no finding\n", folds, sizeof(sizes) / sizeof(sizes[0]));
  return 0;
}

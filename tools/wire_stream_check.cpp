// Host check of the resumable tokenizers' segment logic (wire_seg_begin / wire_seg_host_feed in
// fedbiomed_amd/csrc/fbm_wire.hpp: what the test build's fbm_test_wire_stream_begin / _feed run, over the kernels' own
// per-tile routines) and of the prefix scanner (fbm_wire_scan_prefix_run in fbm_wire_scan.hpp) under the host
// sanitizers: the bytes come from the network.  Builds seeded messages -- a small map's keys, an array of native ints
// of all five widths or of big-int maps of every size class, a key and a value behind it --, then
//   * feeds each span in every two-feed cut and in steps of 1, 7, 64, 4096, 4097 and 5000 bytes and compares count,
//     end and table word for word with the one-shot host tokenizer over the same span at the same address;
//   * does the same for truncations of the span and for seeded mutations of its bytes (compared with the one-shot's
//     answer for the same bytes, whatever it is), with a random cut;
//   * runs the prefix scanner over every prefix of each message, of messages without a candidate and of mutated ones,
//     against fbm_wire_scan_deferred2's pass over the whole message: FBM_WIRE_SCAN_MORE, or that pass's answer.
// The bytes of each feed sit in a heap block of exactly avail_len bytes in use -- the rest of the block is poisoned for
// AddressSanitizer until a later feed brings it --, table, state and workspace in blocks of exactly their size, so a
// read at or past avail_len or a write outside the three is a report.  A stand-alone program: never loaded into Python.
//
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined \
//       -fno-sanitize-recover=all -Iinclude tools/wire_stream_check.cpp -o wire_stream_check && ./wire_stream_check [mutations, default 400]
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
static void expect(bool cond, const char* what) {
  if (!cond) {
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
  }
}
static void header(Bytes& o, uint64_t n) {
  for (uint32_t k = 0; k < fbm::wire_header_size(n); ++k) o.push_back((char)fbm::wire_header_byte(n, k));
}
static void native(Bytes& o) {
  static const int widths[5] = {1, 2, 3, 5, 9};
  const int w = widths[rnd() % 5];
  if (w == 1) {
    o.push_back((char)(rnd() & 0x7f));
    return;
  }
  o.push_back((char)(w == 2 ? 0xcc : w == 3 ? 0xcd : w == 5 ? 0xce : 0xcf));
  for (int i = 1; i < w; ++i) o.push_back((char)rnd());
}
static void map_item(Bytes& o) {
  static const unsigned Ls[7] = {1, 2, 31, 32, 255, 256, 257};
  const unsigned L = Ls[rnd() % 7];
  o.append((const char*)FBM_WIRE_PREFIX, FBM_WIRE_PREFIX_LEN);
  if (L > 255 || rnd() % 5 == 0) o.push_back((char)0xc5), be(o, L, 2);
  else o.push_back((char)0xc4), o.push_back((char)L);
  o.push_back((char)(L == 257 ? 0 : rnd() & 0x7f));
  for (unsigned i = 1; i < L; ++i) o.push_back((char)rnd());
}
struct Message {
  Bytes data;
  uint64_t begin, first, n;
  int scheme;
};
static Message message(int scheme, uint64_t n) {
  Message m;
  m.scheme = scheme, m.n = n;
  m.data = "\x83\xa7node_id\xa6node-7\xa6params";
  m.begin = m.data.size();
  header(m.data, n);
  m.first = m.data.size();
  for (uint64_t i = 0; i < n; ++i) scheme == FBM_WIRE_JL ? map_item(m.data) : native(m.data);
  m.data += "\xabsample_size\xcd\x04\xd2";
  return m;
}

struct Answer {
  uint64_t count, end;
  std::vector<uint64_t> table;
};
static uint64_t n_ckpt_of(int scheme, uint64_t n) { return scheme == FBM_WIRE_JL ? n : (n + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP; }
static uint64_t workspace_of(int scheme, uint64_t len) {
  const uint64_t tiles = (len + 3 + FBM_WIRE_TOK_TILE - 1) / FBM_WIRE_TOK_TILE;
  return (scheme == FBM_WIRE_JL ? fbm::wire_tokj_workspace_of(tiles) : fbm::wire_tok_maps_at(tiles) + tiles * FBM_WIRE_TOK_MAP * 4) + 8;
}

// A span of `len` bytes at address residue `head` (of span[s0]) inside a heap block; bytes at or past `avail` poisoned.
struct Block {
  uint8_t* raw;
  uint8_t* span;
  uint64_t len;
  Block(const uint8_t* src, uint64_t n, uint64_t s0, int head) : len(n) {
    raw = (uint8_t*)malloc(n + 8);
    const uint64_t shift = (uint64_t)(head - (int)((reinterpret_cast<uintptr_t>(raw) + s0) & 3) + 8) & 3;
    span = raw + shift;
    memcpy(span, src, n);
    ASAN_POISON_MEMORY_REGION(raw, shift);
    ASAN_POISON_MEMORY_REGION(span + n, 8 - shift);
  }
  void avail(uint64_t a) {  // only the first a bytes may be read
    ASAN_UNPOISON_MEMORY_REGION(span, len);
    if (a < len) ASAN_POISON_MEMORY_REGION(span + a, len - a);
  }
  ~Block() {
    ASAN_UNPOISON_MEMORY_REGION(raw, len + 8);
    free(raw);
  }
};

static Answer one_shot(int scheme, Block& b, uint64_t len, uint64_t base, uint64_t first, uint64_t n) {
  const uint64_t nck = n_ckpt_of(scheme, n);
  std::vector<uint64_t> ck(nck, 0xA5A5A5A5A5A5A5A5ull), ws(workspace_of(scheme, len) / 8 + 1);
  uint64_t res[2] = {0, 0};
  b.avail(len);
  if (scheme == FBM_WIRE_JL)
    fbm::wire_tokenize_jl_host(b.span, len, base, first, n, ck.data(), nck, res, ws.data());
  else
    fbm::wire_tokenize_host(b.span, len, base, first, n, ck.data(), nck, res, ws.data());
  return Answer{res[0], res[1], ck};
}

static Answer fed(int scheme, Block& b, uint64_t len, uint64_t base, uint64_t first, uint64_t n, const std::vector<uint64_t>& avails) {
  const uint64_t nck = n_ckpt_of(scheme, n);
  std::vector<uint64_t> ck(nck, 0xA5A5A5A5A5A5A5A5ull), ws(workspace_of(scheme, len) / 8 + 1);
  std::vector<uint64_t> state(FBM_WIRE_STREAM_STATE_WORDS);
  fbm::wire_seg_begin(scheme, first, n, state.data());
  for (size_t i = 0; i < avails.size(); ++i) {
    b.avail(avails[i]);
    const char* err = fbm::wire_seg_host_feed(scheme, b.span, base, avails[i], i + 1 == avails.size(), ck.data(), nck, state.data(), ws.data());
    expect(err == nullptr, "a feed of a growing span is accepted");
  }
  return Answer{state[FBM_WIRE_SEG_RESULT], state[FBM_WIRE_SEG_RESULT + 1], ck};
}

static void same(const Answer& a, const Answer& want, const char* what) {
  expect(a.count == want.count && a.end == want.end, what);
  expect(a.table == want.table, what);  // (words no feed wrote keep the fill in both)
}

static void all_cuts(const Message& m, const uint8_t* bytes, uint64_t len, int head, bool every) {
  const uint64_t base = m.begin, first = m.first, s0 = first - base;
  if (len <= s0) return;
  Block b(bytes, len, s0, head);
  const Answer want = one_shot(m.scheme, b, len, base, first, m.n);
  if (every)
    for (uint64_t a = s0; a <= len; ++a) same(fed(m.scheme, b, len, base, first, m.n, {a, len}), want, "two feeds");
  static const uint64_t steps[6] = {1, 7, 64, 4096, 4097, 5000};
  for (uint64_t step : steps) {
    if (step == 1 && !every) continue;
    std::vector<uint64_t> av;
    for (uint64_t a = step; a < len; a += step) av.push_back(a);
    av.push_back(len);
    same(fed(m.scheme, b, len, base, first, m.n, av), want, "stepped feeds");
  }
  const uint64_t a1 = s0 + rnd() % (len - s0 + 1), a2 = a1 + rnd() % (len - a1 + 1);
  same(fed(m.scheme, b, len, base, first, m.n, {a1, a2, len}), want, "random cuts");
}

// fbm_wire_scan_deferred2's pass with nothing resolved, over the whole message
static int deferred(const Bytes& d, uint64_t min_items, uint64_t dl, uint64_t dj, fbm_wire_pending2* p) {
  std::vector<fbm_wire_array> arrays(64);
  std::vector<uint64_t> ck(d.size() + 16);
  fbm_wire_scan_out o = {arrays.data(), arrays.size(), 0, ck.data(), ck.size(), 0};
  const fbm_wire_defer df = {dl, nullptr, 0, nullptr, dj, p};
  return fbm_wire_scan_run((const uint8_t*)d.data(), d.size(), min_items, &o, &df);
}

static void prefixes(const Bytes& d, uint64_t min_items, uint64_t dl, uint64_t dj) {
  fbm_wire_pending2 want = {0, 0, 0, 0, 0};
  const int wrc = deferred(d, min_items, dl, dj, &want);
  if (wrc == FBM_WIRE_SCAN_FULL) return;
  for (uint64_t k = 0; k <= d.size(); ++k) {
    uint8_t* p = (uint8_t*)malloc(k ? k : 1);  // exactly the prefix: a read at or past k is a report
    memcpy(p, d.data(), k);
    fbm_wire_pending2 got = {0, 0, 0, 0, 0};
    const int rc = fbm_wire_scan_prefix_run(p, k, min_items, dl, dj, &got);
    free(p);
    if (rc == FBM_WIRE_SCAN_MORE) continue;
    const bool same_cand = wrc == FBM_WIRE_SCAN_PENDING && got.begin == want.begin && got.first == want.first &&
                           got.n_items == want.n_items && got.scheme == want.scheme;
    if (rc == FBM_WIRE_SCAN_PENDING && !same_cand) {
      // the one test the prefix cannot make: the items at their smallest fit the bytes left
      const uint64_t body = d.size() - got.first;
      expect(got.n_items > (got.scheme == FBM_WIRE_JL ? body / FBM_WIRE_JL_ITEM_MIN : body), "a candidate deferred2 has not: the size test only");
      continue;
    }
    if (rc == FBM_OK && k < d.size()) {
      expect(wrc == FBM_WIRE_SCAN_GAVE_UP, "a whole message in a proper prefix: the rest is trailing bytes");
      continue;
    }
    expect(rc == wrc, "the prefix's answer is the whole message's");
    if (rc == FBM_WIRE_SCAN_PENDING)
      expect(got.begin == want.begin && got.first == want.first && got.n_items == want.n_items && got.scheme == want.scheme, "the same candidate");
  }
}

int main(int argc, char** argv) {
  const int mutations = argc > 1 ? atoi(argv[1]) : 400;
  const Message lom = message(FBM_WIRE_LOM, 2500), jl = message(FBM_WIRE_JL, 60);
  for (const Message* m : {&lom, &jl}) {
    const uint8_t* span = (const uint8_t*)m->data.data() + m->begin;
    const uint64_t len = m->data.size() - m->begin;
    for (int head = 0; head < 4; ++head) all_cuts(*m, span, len, head, head == 1);
    for (int t = 0; t < 40; ++t) all_cuts(*m, span, (m->first - m->begin) + 1 + rnd() % (len - (m->first - m->begin)), (int)(rnd() & 3), false);  // truncations
    for (int t = 0; t < mutations; ++t) {
      Bytes mut((const char*)span, len);
      for (int k = 1 + (int)(rnd() % 3); k > 0; --k) {
        static const uint8_t marks[8] = {0x82, 0xc4, 0xc5, 0xcf, 0xcc, 0xd0, 0xc1, 0x00};
        mut[rnd() % len] = (char)(rnd() & 1 ? marks[rnd() % 8] : rnd());
      }
      all_cuts(*m, (const uint8_t*)mut.data(), len, (int)(rnd() & 3), false);
    }
    prefixes(m->data, 1, 32, 32);
    prefixes(m->data, 16, 100000, 10);
    prefixes(m->data, 4, 0, 0);
  }
  // the prefix scanner: a candidate behind a small array, none at all, mutated messages
  Bytes behind = "\x83\xa1s";
  header(behind, 300);
  for (int i = 0; i < 300; ++i) behind.push_back((char)(rnd() & 0x7f));
  behind += "\xa6params";
  header(behind, 150);
  for (int i = 0; i < 150; ++i) native(behind);
  behind += "\xa1n\x05";
  prefixes(behind, 1, 100, 10);
  prefixes(behind, 1, 400, 0);
  Bytes none = "\x82\xa1" "a";
  header(none, 40);
  for (int i = 0; i < 40; ++i) none += Bytes("\xcb\x3f\xf8\x00\x00\x00\x00\x00\x00", 9);
  none += "\xa1" "b\xd9\x05hello";
  prefixes(none, 1, 10, 10);
  const Message small_lom = message(FBM_WIRE_LOM, 150), small_jl = message(FBM_WIRE_JL, 12);
  for (const Message* m : {&small_lom, &small_jl, (const Message*)nullptr}) {
    const Bytes& src = m ? m->data : behind;
    for (int t = 0; t < mutations; ++t) {
      Bytes mut = src;
      static const uint8_t marks[10] = {0x82, 0xc4, 0xc5, 0xdc, 0xdd, 0x9f, 0x8f, 0xc1, 0xdf, 0xc6};
      for (int k = 1 + (int)(rnd() % 2); k > 0; --k) mut[rnd() % mut.size()] = (char)(rnd() & 1 ? marks[rnd() % 10] : rnd());
      prefixes(mut, 1 + rnd() % 4, rnd() % 3 ? 20 : 0, rnd() % 3 ? 5 : 0);
    }
  }
  printf("wire_stream_check: ok (%d mutations)\n", mutations);
  return 0;
}

// Host check of the msgpack scanner (fedbiomed_amd/csrc/fbm_wire_scan.hpp) under the host sanitizers: the bytes it
// walks come from the network.  Builds valid messages (the reference Serializer's integer arrays among other
// fields), then runs the scanner over the refusal cases and over seeded byte mutations and truncations of them,
// each input in a heap block of exactly its length, so a read at or past `len` is an AddressSanitizer report.
// On every FBM_OK the recorded spans and checkpoints must lie inside the message and re-parse item by item.
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/wire_scan_check.cpp -o wire_scan_check && ./wire_scan_check [mutations per message, default 4000]
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

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
static void array_header(Bytes& o, uint64_t n) {
  if (n <= 15) o.push_back((char)(0x90 | n));
  else if (n <= 65535) o.push_back((char)0xdc), be(o, n, 2);
  else o.push_back((char)0xdd), be(o, n, 4);
}
static void native(Bytes& o, uint64_t v) {
  if (v <= 127) o.push_back((char)v);
  else if (v < (1ull << 8)) o.push_back((char)0xcc), be(o, v, 1);
  else if (v < (1ull << 16)) o.push_back((char)0xcd), be(o, v, 2);
  else if (v < (1ull << 32)) o.push_back((char)0xce), be(o, v, 4);
  else o.push_back((char)0xcf), be(o, v, 8);
}
static void map_item(Bytes& o, const Bytes& value) {
  o.append((const char*)FBM_WIRE_PREFIX, FBM_WIRE_PREFIX_LEN);
  if (value.size() <= 255) o.push_back((char)0xc4), be(o, value.size(), 1);
  else o.push_back((char)0xc5), be(o, value.size(), 2);
  o += value;
}
static Bytes random_value(size_t L) {  // L bytes, the first one a sign byte
  Bytes v(L, '\0');
  for (size_t i = 1; i < L; ++i) v[i] = (char)rnd();
  return v;
}
static void str(Bytes& o, const char* s) {
  o.push_back((char)(0xa0 | strlen(s)));
  o += s;
}

static long g_ok = 0, g_gave_up = 0, g_recorded = 0;

static int scan(const Bytes& msg, uint64_t min_items, std::vector<fbm_wire_array>* arrays_out = nullptr) {
  uint8_t* d = (uint8_t*)malloc(msg.size() ? msg.size() : 1);  // exactly len bytes: ASan guards the rest
  memcpy(d, msg.data(), msg.size());
  std::vector<fbm_wire_array> arrays(64);
  std::vector<uint64_t> ckpt(msg.size() + 16);
  fbm_wire_scan_out o = {arrays.data(), arrays.size(), 0, ckpt.data(), ckpt.size(), 0};
  const int r = fbm_wire_scan_impl(msg.size() ? d : d, msg.size(), min_items, &o);
  if (r != FBM_OK && (o.n_arrays || o.n_ckpt)) {
    fprintf(stderr, "counts not cleared on status %d\n", r);
    exit(1);
  }
  if (r == FBM_OK) {
    ++g_ok;
    uint64_t prev_end = 0;
    for (uint64_t a = 0; a < o.n_arrays; ++a, ++g_recorded) {
      const fbm_wire_array& A = arrays[a];
      bool good = A.begin >= prev_end && A.begin < A.end && A.end <= msg.size() && A.n_items >= min_items &&
                  A.ckpt_first + A.ckpt_count <= o.n_ckpt;
      good = good && A.ckpt_count == (A.scheme == FBM_WIRE_JL ? A.n_items
                                                             : (A.n_items + FBM_WIRE_LOM_GROUP - 1) / FBM_WIRE_LOM_GROUP);
      uint64_t p = A.begin + (A.n_items <= 15 ? 1 : A.n_items <= 65535 ? 3 : 5), voff = 0;
      uint32_t vlen = 0;
      int nat = 0, any_map = 0;
      for (uint64_t i = 0; good && i < A.n_items; ++i) {
        const uint64_t c = fbm_wire_item(d, p, A.end, &voff, &vlen, &nat);
        good = c != 0;
        any_map |= !nat;
        if (good && A.scheme == FBM_WIRE_JL) good = ckpt[A.ckpt_first + i] == ((voff << 16) | vlen);
        if (good && A.scheme == FBM_WIRE_LOM && i % FBM_WIRE_LOM_GROUP == 0)
          good = ckpt[A.ckpt_first + i / FBM_WIRE_LOM_GROUP] == p;
        p += c;
      }
      good = good && p == A.end && any_map == (A.scheme == FBM_WIRE_JL);
      if (!good) {
        fprintf(stderr, "inconsistent record: array %llu of a %zu-byte message\n", (unsigned long long)a, msg.size());
        exit(1);
      }
      prev_end = A.end;
    }
    if (arrays_out) arrays_out->assign(arrays.begin(), arrays.begin() + o.n_arrays);
  } else {
    ++g_gave_up;
  }
  free(d);
  return r;
}

static void expect(bool cond, const char* what) {
  if (!cond) {
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
  }
}

int main(int argc, char** argv) {
  const long mutations = argc > 1 ? atol(argv[1]) : 4000;
  // valid messages: a map with a JL update, a LOM update, and other fields before, between and after
  std::vector<Bytes> valid;
  for (int m = 0; m < 3; ++m) {
    Bytes o;
    o.push_back((char)0x85);
    str(o, "id"), str(o, "node-07");
    str(o, "params");
    const uint64_t n_jl = m == 0 ? 3 : m == 1 ? 40 : 300;
    array_header(o, n_jl);
    for (uint64_t i = 0; i < n_jl; ++i) {
      const uint64_t pick = rnd() % 8;
      if (pick == 0) native(o, rnd() >> (rnd() % 64));
      else map_item(o, random_value(pick == 1 ? 10 + rnd() % 246 : 257));
    }
    str(o, "f"), o.push_back((char)0xcb), be(o, 0x3ff8000000000000ull, 8);
    str(o, "lom");
    const uint64_t n_lom = m == 0 ? 65 : m == 1 ? 1000 : 70000;
    array_header(o, n_lom);
    for (uint64_t i = 0; i < n_lom; ++i) native(o, rnd() >> (rnd() % 64));
    str(o, "tail"), o.push_back((char)0x93), o.push_back((char)0xc0), o.push_back((char)0xc3), o.push_back((char)0xff);
    valid.push_back(o);
  }
  for (const Bytes& v : valid) {
    std::vector<fbm_wire_array> a;
    expect(scan(v, 2, &a) == FBM_OK && a.size() == 2, "a valid message records its two updates");
    expect(a[0].scheme == FBM_WIRE_JL && a[1].scheme == FBM_WIRE_LOM, "schemes");
  }
  // refusals: the array is not recorded (the rest of the message still scans), or the scan gives up
  struct Case {
    const char* what;
    Bytes item;
  };
  Bytes l258, l257nz, sign, swapped, str8, flt;
  map_item(l258, random_value(258));
  { Bytes v = random_value(257); v[0] = 1; map_item(l257nz, v); }
  { Bytes v = random_value(12); v[0] = (char)0x80; map_item(sign, v); }
  swapped = Bytes("\x82\xa5value\xc4\x02\x00\x01\xa8__type__\xa3int", 24);
  str8 = Bytes("\x82\xd9\x08__type__\xa3int\xa5value\xc4\x02\x00\x01", 25);
  flt = Bytes("\xca\x3f\x80\x00\x00", 5);
  const Case cases[] = {{"a negative int", Bytes("\xff", 1)}, {"int8", Bytes("\xd0\x80", 2)}, {"sign byte", sign},
                        {"L = 258", l258}, {"L = 257, nonzero first byte", l257nz}, {"value before __type__", swapped},
                        {"str8 key", str8}, {"a float", flt}};
  for (const Case& c : cases) {
    Bytes o;
    o.push_back((char)0x92);
    array_header(o, 3);
    native(o, 7), o += c.item, map_item(o, random_value(20));
    array_header(o, 3), native(o, 1), native(o, 300), native(o, 70000);
    std::vector<fbm_wire_array> a;
    expect(scan(o, 1, &a) == FBM_OK && a.size() == 1 && a[0].n_items == 3 && a[0].scheme == FBM_WIRE_LOM, c.what);
  }
  {
    Bytes three;
    array_header(three, 3);
    map_item(three, random_value(10)), native(three, 300), map_item(three, random_value(257));
    expect(scan(three, 1) == FBM_OK, "three items");
    for (size_t cut = 0; cut < three.size(); ++cut)
      expect(scan(three.substr(0, cut), 1) == FBM_WIRE_SCAN_GAVE_UP, "every truncation gives up");
    expect(scan(three + Bytes(1, '\0'), 1) == FBM_WIRE_SCAN_GAVE_UP, "trailing bytes");
    expect(scan(Bytes(FBM_WIRE_MAX_DEPTH + 4, (char)0x91) + three, 1) == FBM_WIRE_SCAN_GAVE_UP, "nesting past the bound");
    expect(scan(Bytes(FBM_WIRE_MAX_DEPTH - 2, (char)0x91) + three, 1) == FBM_OK, "nesting within the bound");
    expect(scan(Bytes(1 << 20, (char)0x91), 1) == FBM_WIRE_SCAN_GAVE_UP, "a deep message costs no stack");
  }
  // seeded mutations and truncations of the valid messages (the 70 000-item one through its first 64 KB too)
  long runs = 0;
  for (size_t m = 0; m < valid.size(); ++m) {
    for (long k = 0; k < mutations; ++k, ++runs) {
      Bytes v = valid[m];
      const int kind = (int)(rnd() % 4);
      if (kind == 0 || v.size() > (1u << 16)) v.resize(1 + rnd() % (v.size() < (1u << 16) ? v.size() : (1u << 16)));
      const int flips = kind == 0 ? 0 : 1 + (int)(rnd() % 4);
      for (int f = 0; f < flips; ++f) {
        const size_t at = rnd() % v.size();
        if (kind == 1) v[at] = (char)rnd();
        else if (kind == 2) v[at] ^= (char)(1u << (rnd() % 8));
        else v[at] = (char)(0xc0 + rnd() % 0x20);  // a type byte: lengths, containers, ints
      }
      scan(v, 1 + rnd() % 3);
    }
  }
  for (long k = 0; k < mutations; ++k, ++runs) {  // and pure noise
    Bytes v(1 + rnd() % 300, '\0');
    for (char& c : v) c = (char)rnd();
    scan(v, 1);
  }
  printf("wire_scan_check: %ld mutated inputs; %ld scans ok (%ld arrays re-parsed), %ld gave up; no finding\n", runs, g_ok,
         g_recorded, g_gave_up);
  return 0;
}

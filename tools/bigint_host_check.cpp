// Runs fedbiomed_amd/csrc/fbm_bigint.hpp (the host big integers of the C ABI's setup) against vectors
// computed elsewhere: reads lines "op hex-operands hex-expected" from stdin and exits non-zero at the first
// mismatch.  tests/test_host_bigint.py builds it and feeds it vectors from Python's integers; by hand, under
// the sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/bigint_host_check.cpp
//       -o /tmp/bigint_host_check && /tmp/bigint_host_check < vectors.txt
// Numbers are hexadecimal; a number's word count is that of its digits (leading zeros kept, so a modulus
// with a zero top word can be given).  Lines:
//   mul a b r | mullo a b words r | divmod a m q r | shr a bits r | ctz a r | to_limbs a nl lb r
//   pow2_mod E m r | pow2_mod_u64 e m r | inv_mod_pow2 a bits r
// to_limbs' r holds limb k in its 32-bit word k.
#include <stdio.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../fedbiomed_amd/csrc/fbm_bigint.hpp"

using namespace fbm;

static Big parse(const std::string& h) {
  Big a((h.size() + 7) / 8 ? (h.size() + 7) / 8 : 1, 0u);
  for (size_t i = 0; i < h.size(); ++i) {
    const char c = h[h.size() - 1 - i];
    const uint32_t d = c <= '9' ? (uint32_t)(c - '0') : (uint32_t)((c | 32) - 'a' + 10);
    a[i / 8] |= d << (4 * (i % 8));
  }
  return a;
}

static bool same(Big a, Big b) {
  big_trim(a);
  big_trim(b);
  return a == b;
}

int main() {
  std::string line;
  long n = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream in(line);
    std::string op;
    std::vector<std::string> f;
    in >> op;
    for (std::string t; in >> t;) f.push_back(t);
    auto num = [&](size_t i) { return parse(f.at(i)); };
    auto small = [&](size_t i) { return std::stoull(f.at(i), nullptr, 16); };
    bool ok = false;
    if (op == "mul") {
      ok = same(big_mul(num(0), num(1)), num(2));
    } else if (op == "mullo") {
      ok = same(big_mullo(num(0), num(1), (size_t)small(2)), num(3));
    } else if (op == "divmod") {
      Big q, r;
      big_divmod(num(0), num(1), q, r);
      ok = same(q, num(2)) && same(r, num(3));
    } else if (op == "shr") {
      ok = same(big_shr(num(0), (int)small(1)), num(2));
    } else if (op == "ctz") {
      ok = (unsigned long long)big_ctz(num(0)) == small(1);
    } else if (op == "to_limbs") {
      Big o((size_t)small(1), 0xffffffffu);
      to_limbs(num(0), o.data(), (int)o.size(), (int)small(2));
      ok = same(o, num(3));
    } else if (op == "pow2_mod") {
      ok = same(pow2_mod(num(0), num(1)), num(2));
    } else if (op == "pow2_mod_u64") {
      ok = same(pow2_mod((uint64_t)small(0), num(1)), num(2));
    } else if (op == "inv_mod_pow2") {
      const Big y = inv_mod_pow2(num(0), (int)small(1));
      ok = y.size() == (size_t)((small(1) + 31) / 32) && same(y, num(2));
    } else {
      fprintf(stderr, "unknown op in: %s\n", line.c_str());
      return 2;
    }
    if (!ok) {
      fprintf(stderr, "MISMATCH: %s\n", line.c_str());
      return 1;
    }
    ++n;
  }
  printf("%ld vectors ok\n", n);
  return 0;
}

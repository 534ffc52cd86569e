// The coefficient rule of the random linear combination (handel_amd/csrc/
// bn256_rlc.h) on the host: the digest-to-coefficient mapping, whose
// replacement of 0 by 1 no search over seeds can reach, and one derived
// coefficient against the mapping applied to the digest by hand.
#include <cstdio>
#include <cstring>

#include "bn256_rlc.h"

static int fails = 0;
#define CHECK(c)                                      \
  do {                                                \
    if (!(c)) {                                       \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      fails++;                                        \
    }                                                 \
  } while (0)

int main() {
  using namespace hg;
  // digest bytes 01 02 03 04 05 06 07 08: words 0x01020304, 0x05060708 (big-endian)
  CHECK(rlc_coeff_from_digest(0x01020304u, 0x05060708u) == 0x0807060504030201ull);
  CHECK(rlc_coeff_from_digest(0u, 0u) == 1);            // 0 would drop the check from its group
  CHECK(rlc_coeff_from_digest(0x01000000u, 0u) == 1);   // a genuine 1 stays 1
  CHECK(rlc_coeff_from_digest(0u, 0x00000080u) == 0x8000000000000000ull);  // byte 7 is the top byte
  CHECK(rlc_coeff_from_digest(0xffffffffu, 0xffffffffu) == ~0ull);
  // rlc_coeff = the mapping over SHA-256("hg-rlc-v1" || seed || LE64(i))
  uint8_t seed[32];
  for (int k = 0; k < 32; k++) seed[k] = (uint8_t)(7 * k + 1);
  const uint64_t idx[] = {0, 1, 0xffffffffull, 0x100000000ull, 0xfedcba9876543210ull};
  for (uint64_t i : idx) {
    uint8_t m[49];
    std::memcpy(m, "hg-rlc-v1", 9);
    std::memcpy(m + 9, seed, 32);
    for (int k = 0; k < 8; k++) m[41 + k] = (uint8_t)(i >> (8 * k));
    uint32_t h[8];
    sha256_words(m, sizeof m, h);
    CHECK(rlc_coeff(seed, i) == rlc_coeff_from_digest(h[0], h[1]));
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}

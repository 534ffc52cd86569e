// The scaling of hashedMessage's scalar by a coefficient (handel_amd/csrc/
// bn256_mrlc.h: mrlc_scale, k' = r k mod Order) on the host, by the code the
// device runs. Prints one line "r k k'" (hexadecimal) per fixed pair;
// tests/test_aggregate_msgs_rlc_host.py holds them against Python integers.
#include <cinttypes>
#include <cstdio>

#include "bn256_mrlc.h"

static void print_words(const uint32_t w[8]) {
  for (int i = 7; i >= 0; i--) std::printf("%08" PRIx32, w[i]);
}

int main() {
  using namespace hg;
  const uint32_t kZero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t kOne[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t kOrderM1[8] = {0x57ac7260u, 0x1a2ef45bu, 0xf82b3924u, 0x2e8d8e12u,
                                0x6184dc21u, 0xaa6fecb8u, 0x4aa387f9u, 0x8fb501e3u};
  // an ordinary scalar below Order
  const uint32_t kAny[8] = {0xc4c216acu, 0xf04e0f58u, 0xbd2a385cu, 0x18ed3e16u,
                            0x627b0ce9u, 0x9de4614du, 0xce33ac91u, 0x04a1e9c5u};
  // 3 k = 2 Order + 1
  const uint32_t kThird[8] = {0x8fc84c41u, 0x1174a2e7u, 0xa5722618u, 0xc9b3b40cu,
                              0x965892c0u, 0x719ff325u, 0x31c25aa6u, 0x5fce0142u};
  // (2^64 - 1) k = 2^63 Order + (less than 2^64)
  const uint32_t kTop[8] = {0xfe0007d1u, 0xc170b884u, 0x5229ce9fu, 0xb4593e57u,
                            0xd614320du, 0x1d12774du, 0xa551c3fdu, 0x47da80f1u};
  // 0x9e3779b97f4a7c15 k = 12345678901234567 Order + (less than 2^64)
  const uint32_t kMid[8] = {0xd0087cb5u, 0x1720edd1u, 0x26540a30u, 0xd10d0e96u,
                            0xb5b63066u, 0x0c1c3096u, 0xd5a20f56u, 0x0027d69bu};
  // above Order (not a hashedMessage scalar: the function reduces it first)
  const uint32_t kAll[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                            0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  const uint64_t rs[] = {1, 2, 3, 0x8000000000000000ull, 0x9e3779b97f4a7c15ull, 0xffffffffffffffffull};
  const uint32_t* ks[] = {kZero, kOne, kOrderM1, kAny, kThird, kTop, kMid, kAll};
  for (uint64_t r : rs)
    for (const uint32_t* k : ks) {
      uint32_t out[8];
      mrlc_scale(out, r, k);
      std::printf("%016" PRIx64 " ", r);
      print_words(k);
      std::printf(" ");
      print_words(out);
      std::printf("\n");
    }
  return 0;
}

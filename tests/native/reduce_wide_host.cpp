// Host harness for the one-chain reduction tail (handel_amd/csrc/bn256_redq.h):
// the same header the device code includes, compiled for the CPU.
//
// stdin, one case per line:  QMAX LAZY c0 .. c9   (decimal, decimal, ten hex
// 64-bit columns: the accumulator's columns 11..20 after the REDC digits)
// stdout, one line per case: r0 .. r9 (hex limbs)
// Built with -fsanitize=address,undefined by tests/test_reduce_wide_host.py.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "bn256_redq.h"

namespace {

template <int QMAX>
void run(bool lazy, uint32_t (&r)[10], const uint64_t* c) {
  if (lazy) hg::redq_tail<QMAX, true>(r, c);
  else hg::redq_tail<QMAX, false>(r, c);
}

bool dispatch(int qmax, bool lazy, uint32_t (&r)[10], const uint64_t* c) {
  switch (qmax) {
    case 1: run<1>(lazy, r, c); return true;
    case 2: run<2>(lazy, r, c); return true;
    case 3: run<3>(lazy, r, c); return true;
    case 13: run<13>(lazy, r, c); return true;
    case 30: run<30>(lazy, r, c); return true;
    case 64: run<64>(lazy, r, c); return true;
    default: return false;
  }
}

}  // namespace

int main() {
  static_assert(hg::kRedqMaxQ == 64 && hg::kRedqCompareQ == 2, "the forms this harness instantiates");
  int qmax, lazy;
  // heap copies, so the sanitizer sees any access past the ten columns / limbs
  std::vector<uint64_t> c(10);
  while (std::scanf("%d %d", &qmax, &lazy) == 2) {
    for (int j = 0; j < 10; j++)
      if (std::scanf("%" SCNx64, &c[j]) != 1) return 2;
    uint32_t r[10];
    if (!dispatch(qmax, lazy != 0, r, c.data())) return 3;
    for (int j = 0; j < 10; j++) std::printf("%x%c", r[j], j == 9 ? '\n' : ' ');
  }
  return 0;
}

// hg_sha256.h — SHA-256 and hashedMessage's scalar (bn256/go/bn256.go:210-218),
// one definition for the host (hg_set_message, hg_debug_hash_scalar) and the
// device (k_hash_scalars, bn256_msgs.hip: one thread per message). Written so
// that the device copy stays in registers: the message schedule is the rolling
// 16-word form under fully unrolled loops, and the padding is computed per byte
// position instead of staged in a buffer.
#pragma once
#include <cstddef>
#include <cstdint>

#include "bn256_constants.h"

#ifndef HG_HD
#if defined(__HIPCC__)
#define HG_HD __host__ __device__ inline
#else
#define HG_HD static inline
#endif
#endif

namespace hg {

// FIPS 180-4 (an immediate per round once the rounds are unrolled)
HG_HD uint32_t sha_k(int i) {
  const uint32_t k[64] = {
      0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5,
      0xd807aa98, 0x12835b01, 0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174,
      0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da,
      0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967,
      0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
      0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070,
      0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3,
      0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
  return k[i];
}

HG_HD uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }

// one compression: w holds the block's 16 big-endian words (overwritten)
HG_HD void sha256_block(uint32_t h[8], uint32_t (&w)[16]) {
  uint32_t a = h[0], bb = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int i = 0; i < 64; i++) {
    if (i >= 16) {
      const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
      const uint32_t s0 = rotr(w15, 7) ^ rotr(w15, 18) ^ (w15 >> 3);
      const uint32_t s1 = rotr(w2, 17) ^ rotr(w2, 19) ^ (w2 >> 10);
      w[i & 15] += s0 + w[(i + 9) & 15] + s1;
    }
    uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + sha_k(i) + w[i & 15];
    uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & bb) ^ (a & c) ^ (bb & c));
    hh = g;
    g = f;
    f = e;
    e = d + t1;
    d = c;
    c = bb;
    bb = a;
    a = t1 + t2;
  }
  h[0] += a; h[1] += bb; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// byte `pos` of the padded message: the message, 0x80, zeros, and the bit
// length in the last 8 of `total` bytes
HG_HD uint32_t sha256_padded_byte(const uint8_t* m, size_t len, size_t total, size_t pos) {
  if (pos < len) return m[pos];
  if (pos == len) return 0x80;
  if (pos + 8 < total) return 0;
  return (uint32_t)(((uint64_t)len * 8) >> (8 * (total - 1 - pos))) & 255u;
}

// the digest as 8 big-endian words (digest byte 4k is the top byte of h[k])
HG_HD void sha256_words(const uint8_t* m, size_t len, uint32_t h[8]) {
  const uint32_t iv[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
#pragma unroll
  for (int k = 0; k < 8; k++) h[k] = iv[k];
  const size_t total = (len + 9 + 63) / 64 * 64;
  for (size_t base = 0; base < total; base += 64) {
    uint32_t w[16];
    if (base + 64 <= len) {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const uint8_t* b = m + base + 4 * i;
        w[i] = (uint32_t)b[0] << 24 | (uint32_t)b[1] << 16 | (uint32_t)b[2] << 8 | b[3];
      }
    } else {
#pragma unroll
      for (int i = 0; i < 16; i++) {
        const size_t p = base + 4 * i;
        w[i] = sha256_padded_byte(m, len, total, p) << 24 | sha256_padded_byte(m, len, total, p + 1) << 16 |
               sha256_padded_byte(m, len, total, p + 2) << 8 | sha256_padded_byte(m, len, total, p + 3);
      }
    }
    sha256_block(h, w);
  }
}

HG_HD void sha256(const uint8_t* m, size_t len, uint8_t out[32]) {
  uint32_t h[8];
  sha256_words(m, len, h);
  for (int k = 0; k < 8; k++) {
    out[4 * k] = (uint8_t)(h[k] >> 24);
    out[4 * k + 1] = (uint8_t)(h[k] >> 16);
    out[4 * k + 2] = (uint8_t)(h[k] >> 8);
    out[4 * k + 3] = (uint8_t)h[k];
  }
}

// crypto/rand.Int(bytes.NewBuffer(d), Order) as used by hashedMessage: the
// single 32-byte read is accepted iff 0 < int(d) < n; otherwise the next
// read hits EOF. h: the digest's 8 big-endian words; k: the
// integer's 8 little-endian words.
HG_HD bool hash_scalar_words(const uint32_t h[8], uint32_t k[8]) {
  const uint32_t order[8] = {HG_ORDER32};
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    k[i] = h[7 - i];
    any |= k[i];
  }
  // k < Order: the borrow out of k - Order
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)k[i] - order[i] - br;
    br = (uint32_t)(d >> 63);
  }
  return any != 0 && br != 0;
}

HG_HD bool hash_scalar(const uint8_t d[32], uint32_t k[8]) {
  uint32_t h[8];
  for (int i = 0; i < 8; i++)
    h[i] = (uint32_t)d[4 * i] << 24 | (uint32_t)d[4 * i + 1] << 16 | (uint32_t)d[4 * i + 2] << 8 | d[4 * i + 3];
  return hash_scalar_words(h, k);
}

}  // namespace hg

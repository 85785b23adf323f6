// sampler_stream.hip.hpp -- the samplers' stream on the device (keygen_kernels.hip.hpp, mp_refresh_kernels.hip.hpp): one BLAKE2b compression per block.
#pragma once
#include "modarith.hip.hpp"

// ---- the sampler stream: BLAKE2b in counter mode, one substream per (call, poly, row, group of 8 coefficients) ------------------------------------
// Block t of a substream is the 64-byte BLAKE2b digest, keyed and personalised on the host, of the 40-byte message (call, poly, row, group, t)
// as five little-endian words.  The chaining value after the padded key block (RFC 7693 section 3.3: a keyed hash starts with the key as a
// block of its own) does not depend on the message: the host computes it once (SampArgs::h) and a block costs ONE compression here, the final
// one: byte counter 128 + 40, last-block flag set.  Word w of block t is candidate t of coefficient 8 * group + w.
struct SampArgs { u64 h[8]; u64 call, poly0, row0; };

RH_DEV u64 b2b_rotr(u64 x, int r) { return (x >> r) | (x << (64 - r)); }

// the final compression of a 40-byte message block m[0..5) (m[5..16) = 0) on the chaining value h: out = the eight digest words
RH_DEV void b2b_block(const u64* __restrict__ h, const u64 (&m5)[5], u64 (&out)[8]) {
  constexpr u64 IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                         0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  // SIGMA as immediates: the rounds are unrolled, so every index below is a constant and the eleven zero words fold away
  constexpr unsigned char S[12][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0},
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3}};
  u64 m[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = i < 5 ? m5[i] : 0;
  u64 v[16];
#pragma unroll
  for (int i = 0; i < 8; ++i) { v[i] = h[i]; v[8 + i] = IV[i]; }
  v[12] ^= 168;                        // t0: 128 bytes of key block + 40 of message; t1 = 0
  v[14] = ~v[14];                      // last block
#define RH_B2B_G(a, b, c, d, x, y)                                   \
  v[a] = v[a] + v[b] + (x); v[d] = b2b_rotr(v[d] ^ v[a], 32);        \
  v[c] = v[c] + v[d];       v[b] = b2b_rotr(v[b] ^ v[c], 24);        \
  v[a] = v[a] + v[b] + (y); v[d] = b2b_rotr(v[d] ^ v[a], 16);        \
  v[c] = v[c] + v[d];       v[b] = b2b_rotr(v[b] ^ v[c], 63);
#pragma unroll
  for (int r = 0; r < 12; ++r) {
    RH_B2B_G(0, 4, 8, 12, m[S[r][0]], m[S[r][1]])
    RH_B2B_G(1, 5, 9, 13, m[S[r][2]], m[S[r][3]])
    RH_B2B_G(2, 6, 10, 14, m[S[r][4]], m[S[r][5]])
    RH_B2B_G(3, 7, 11, 15, m[S[r][6]], m[S[r][7]])
    RH_B2B_G(0, 5, 10, 15, m[S[r][8]], m[S[r][9]])
    RH_B2B_G(1, 6, 11, 12, m[S[r][10]], m[S[r][11]])
    RH_B2B_G(2, 7, 8, 13, m[S[r][12]], m[S[r][13]])
    RH_B2B_G(3, 4, 9, 14, m[S[r][14]], m[S[r][15]])
  }
#undef RH_B2B_G
#pragma unroll
  for (int i = 0; i < 8; ++i) out[i] = h[i] ^ v[i] ^ v[8 + i];
}

// mp_refresh_kernels.hip.hpp -- the kernels of the collective refresh's share conversion (mp_refresh.hip): multiword integers per coefficient.
// A big-integer block holds npoly * n values of W 64-bit words, little-endian, two's complement, WORD-MAJOR: word w of value i of poly p is at
// blk[(p * W + w) * n + i], so the lanes of a wavefront read and write consecutive words.  A lane owns a value from its source to its
// destination; every array below is indexed by unrolled loops over the template's W, so a value stays in registers.
#pragma once
#include "modarith.hip.hpp"
#include "stream_kernels.hip.hpp"
#include "sampler_stream.hip.hpp"

#define MPB_MAX_W 8              // words per value
#define MPB_MAX_LIMBS 16         // limbs of a from-RNS source

// ---- multiword helpers ----------------------------------------------------------------------------------------------------------------------------
template <int K> RH_DEV bool mpb_geq(const u64 (&a)[K], const u64 (&b)[K]) {          // a >= b, unsigned
  bool ge = true;
#pragma unroll
  for (int w = 0; w < K; ++w) ge = a[w] > b[w] || (a[w] == b[w] && ge);
  return ge;
}
template <int K> RH_DEV void mpb_sub(u64 (&a)[K], const u64 (&b)[K]) {                // a -= b mod 2^(64 K)
  u64 borrow = 0;
#pragma unroll
  for (int w = 0; w < K; ++w) {
    const u64 t = a[w] - b[w], u = t - borrow;
    borrow = (u64)(a[w] < b[w]) | (u64)(t < borrow);
    a[w] = u;
  }
}
template <int K> RH_DEV void mpb_neg(u64 (&a)[K]) {                                   // a = -a mod 2^(64 K)
  u64 carry = 1;
#pragma unroll
  for (int w = 0; w < K; ++w) { const u64 t = ~a[w] + carry; carry = (u64)(t < carry); a[w] = t; }
}

// ---- rh_mp_big_sample: logBound uniform bits sign-extended from bit logBound - 1 (multiparty/mpckks/sharing.go:120-129) -------------------------------
// RandInt(prng, 2^logBound), then - 2^logBound when >= 2^(logBound - 1).  Word w of value i of poly p is word i % 8 of block t = 0 of substream
// (call, poly0 + p, row = w, group = i / 8); the words above bit logBound - 1 are the sign's.  A lane serves a group of eight values (n < 8: the first n of one group).
// grid (npoly, chunks)
template <int W>
__global__ void __launch_bounds__(256)
mp_big_sample_kernel(SampArgs a, u64* __restrict__ blk, unsigned n, int logBound) {
  const u32 poly = blockIdx.x;
  const int top = (logBound - 1) >> 6, kbits = logBound - 64 * top;                   // the word that holds the sign bit; its bits, 1..64
  const unsigned groups = (n + 7) >> 3;                                               // n = 2 or 4 (one or two slots): one group, its first n words
  for (unsigned g = blockIdx.y * blockDim.x + threadIdx.x; g < groups; g += gridDim.y * blockDim.x) {
    u64 sign[8];
#pragma unroll
    for (int w = 0; w < W; ++w) {
      u64 x[8];
      if (w <= top) {
        const u64 m[5] = {a.call, a.poly0 + poly, (u64)w, g, 0};
        b2b_block(a.h, m, x);
        if (w == top) {
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            x[k] = (u64)((long long)(x[k] << (64 - kbits)) >> (64 - kbits));
            sign[k] = (u64)((long long)x[k] >> 63);
          }
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = sign[k];
      }
      u64* row = blk + ((size_t)poly * W + w) * n + 8 * (size_t)g;
      if (n >= 8) {
#pragma unroll
        for (int k = 0; k < 8; k += 2) rh_st2(row + k, make_ulonglong2(x[k], x[k + 1]), false);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) if ((unsigned)k < n) row[k] = x[k];
      }
    }
  }
}

// ---- the recode kernel: source -> [Quo(x m, d)] -> destination, one lane per value -----------------------------------------------------------------
// SRC_RNS: x = PolyToBigintCentered (ring/ring.go:503-543): v = CRT(residues) in [0, Q), x = v - Q when v >= floor(Q / 2) (note the >=), from
//          a coefficient-domain poly read at stride gap_in; else x is read from the block `src`.
//          v = sum_k ((r_k yinv_k) mod q_k) (Q / q_k), reduced below Q by at most L - 1 subtractions; the sum is held in W + 1 words.
// MULDIV:  x = Quo(x m, d), truncated toward zero like big.Int.Quo (multiparty/mpckks/transform.go:363-376): |x| m in W + 2 words, a
//          shift-subtract division by d (at most 4 words), the sign put back.
// DST_RNS: SetCoefficientsBigint (ring/ring.go:433-447) with the spread of NTTSparseAndMontgomery (core/rlwe/utils.go:187-245): limb l of
//          coefficient i gap_out is x mod q_l, Euclidean and canonical; acc = 0 writes it and zeros between, +1 / -1 adds / subtracts it in place.
//          else x is written to the block `dst`, or with acc != 0 added to the value there (the Add of mpckks/sharing.go:172-178).
struct MpbCrt {                   // from-RNS tables of (ringIn, levelIn), by value
  u64 qhat[MPB_MAX_LIMBS][MPB_MAX_W];    // Q / q_k
  u64 yinv[MPB_MAX_LIMBS];               // (Q / q_k)^-1 mod q_k
  u64 Q[MPB_MAX_W + 1], half[MPB_MAX_W + 1];    // Q and floor(Q / 2)
};
struct MpbArgs {
  const u64* src; u64* dst;       // blocks (npoly, W, n), or polys: src rows (poly, limb) at (poly * in_rows + limb) * N_in, dst dense (npoly, Lout, N_out)
  unsigned n; int in_rows, Lin, Lout, log_gap_in, log_gap_out, acc;
  unsigned Nin, Nout;
  u64 m[2], d[4];
};

template <int W> RH_DEV void mpb_from_rns(const MpbArgs& a, const MpbCrt& t, const LimbConsts* __restrict__ cin, u32 poly, unsigned i, u64 (&x)[W]) {
  u64 s[W + 1];
#pragma unroll
  for (int w = 0; w <= W; ++w) s[w] = 0;
  const u64* row = a.src + (size_t)poly * (size_t)a.in_rows * a.Nin + ((size_t)i << a.log_gap_in);
  for (int k = 0; k < a.Lin; ++k) {
    const LimbConsts c = cin[k];
    const u64 y = bred(row[(size_t)k * a.Nin], t.yinv[k], c.q, c.bred0, c.bred1);
    u64 carry = 0;                                            // s += y * qhat[k]
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const u128 p = (u128)y * t.qhat[k][w] + s[w] + carry;
      s[w] = (u64)p; carry = (u64)(p >> 64);
    }
    s[W] += carry;
  }
  u64 Q[W + 1], H[W + 1];
#pragma unroll
  for (int w = 0; w <= W; ++w) { Q[w] = t.Q[w]; H[w] = t.half[w]; }
  for (int k = 1; k < a.Lin; ++k) if (mpb_geq<W + 1>(s, Q)) mpb_sub<W + 1>(s, Q);     // s < L Q
  if (mpb_geq<W + 1>(s, H)) mpb_sub<W + 1>(s, Q);
#pragma unroll
  for (int w = 0; w < W; ++w) x[w] = s[w];
}

template <int W> RH_DEV void mpb_muldiv(const MpbArgs& a, u64 (&x)[W]) {
  const bool neg = (long long)x[W - 1] < 0;
  if (neg) mpb_neg<W>(x);
  u64 p[W + 2];                                               // |x| m
#pragma unroll
  for (int w = 0; w < W + 2; ++w) p[w] = 0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    u64 carry = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const u128 t = (u128)x[w] * a.m[j] + p[w + j] + carry;
      p[w + j] = (u64)t; carry = (u64)(t >> 64);
    }
    p[W + j] += carry;                                        // p[W + j] is still 0 for j = 1 and below 2^64 - 1 for j = 0: no carry out
  }
  const u64 d[5] = {a.d[0], a.d[1], a.d[2], a.d[3], 0};
  u64 r[5] = {0, 0, 0, 0, 0};
  for (int it = 0; it < 64 * (W + 2); ++it) {                 // the quotient's bits replace the numerator's as they are shifted out
    u64 in = p[W + 1] >> 63;
#pragma unroll
    for (int w = W + 1; w > 0; --w) p[w] = (p[w] << 1) | (p[w - 1] >> 63);
    p[0] <<= 1;
#pragma unroll
    for (int w = 4; w > 0; --w) r[w] = (r[w] << 1) | (r[w - 1] >> 63);
    r[0] = (r[0] << 1) | in;
    if (mpb_geq<5>(r, d)) { mpb_sub<5>(r, d); p[0] |= 1; }
  }
#pragma unroll
  for (int w = 0; w < W; ++w) x[w] = p[w];
  if (neg) mpb_neg<W>(x);
}

template <int W> RH_DEV void mpb_to_rns(const MpbArgs& a, const LimbConsts* __restrict__ cout, u32 poly, unsigned i, u64 (&x)[W]) {
  const bool neg = (long long)x[W - 1] < 0;
  if (neg) mpb_neg<W>(x);
  u64* o = a.dst + (size_t)poly * (size_t)a.Lout * a.Nout + ((size_t)i << a.log_gap_out);
  const unsigned gap = 1u << a.log_gap_out;
  for (int l = 0; l < a.Lout; ++l, o += a.Nout) {
    const LimbConsts c = cout[l];
    const u64 R = mform(1, c.q, c.bred0, c.bred1);            // 2^64 mod q
    u64 v = 0;
#pragma unroll
    for (int w = W - 1; w >= 0; --w) v = cred(bred(v, R, c.q, c.bred0, c.bred1) + bred_add(x[w], c.q, c.bred0), c.q);
    if (neg && v) v = c.q - v;
    if (a.acc == 0) {
      o[0] = v;
      for (unsigned g = 1; g < gap; ++g) o[g] = 0;
    } else {
      o[0] = cred(o[0] + (a.acc > 0 ? v : (v ? c.q - v : 0)), c.q);
    }
  }
}

// grid (npoly, chunks)
template <int W, bool SRC_RNS, bool MULDIV, bool DST_RNS>
__global__ void __launch_bounds__(256)
mp_big_recode_kernel(MpbArgs a, MpbCrt t, const LimbConsts* __restrict__ cin, const LimbConsts* __restrict__ cout) {
  const u32 poly = blockIdx.x;
  for (unsigned i = blockIdx.y * blockDim.x + threadIdx.x; i < a.n; i += gridDim.y * blockDim.x) {
    u64 x[W];
    if (SRC_RNS) mpb_from_rns<W>(a, t, cin, poly, i, x);
    else {
#pragma unroll
      for (int w = 0; w < W; ++w) x[w] = a.src[((size_t)poly * W + w) * a.n + i];
    }
    if (MULDIV) mpb_muldiv<W>(a, x);
    if (DST_RNS) mpb_to_rns<W>(a, cout, poly, i, x);
    else {
      u64 carry = 0;                                            // acc: added to the value that is there
#pragma unroll
      for (int w = 0; w < W; ++w) {
        u64* o = a.dst + ((size_t)poly * W + w) * a.n + i;
        if (a.acc) { const u64 t = *o + x[w], u = t + carry; carry = (u64)(t < x[w]) | (u64)(u < t); x[w] = u; }
        *o = x[w];
      }
    }
  }
}

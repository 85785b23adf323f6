// ckks_encoder_kernels.hip.hpp -- device side of schemes/ckks/encoder.go (float64 path, standard rings): the special FFT / IFFT of
// ckks_vector_ops.go:18-76, the quantizer of utils.go:130-234 and the exact CRT reconstruction of encoder.go:796-1003.
//
// All floating point is IEEE double with real and imaginary parts as separate scalars, one operation per source operation (the library is
// built with -ffp-contract=off and the pragma below keeps it so for this header whatever the command line says).  A butterfly of either
// transform is a pure function of its two inputs and one root, so the grouping of stages into launches and LDS rounds below gives the bits of
// the reference's loops; only the ORDER of the stages is the reference's.
#pragma once
#include <hip/hip_runtime.h>
#include "ring_types.hip.hpp"

#pragma clang fp contract(off)

struct EncCplx { double re, im; };

// (a + bi)(c + di) = (ac - bd, ad + bc), the four products and two sums of Go's complex128 multiply
__device__ __forceinline__ EncCplx enc_cmul(EncCplx x, EncCplx w) {
  EncCplx r;
  r.re = x.re * w.re - x.im * w.im;
  r.im = x.re * w.im + x.im * w.re;
  return r;
}

// root of the stage with len = 1 << loglen for the butterfly whose upper element sits at offset j < len/2 of its block
// IFFT: roots[(lenq - (rotGroup[j] & mask)) << logGap]    FFT: roots[(rotGroup[j] & mask) << logGap]      (lenq = 4 len, mask = lenq - 1)
template <bool INVERSE>
__device__ __forceinline__ EncCplx enc_root(const EncCplx* __restrict__ roots, const unsigned* __restrict__ rot, unsigned j, int loglen, int logm) {
  const unsigned lenq = 4u << loglen, r = rot[j] & (lenq - 1);
  const int loggap = logm - 2 - loglen;
  return roots[(size_t)(INVERSE ? lenq - r : r) << loggap];
}

// IFFT: u, v = u + v, (u - v) * w      FFT: v *= w; u, v = u + v, u - v
template <bool INVERSE>
__device__ __forceinline__ void enc_bfly(EncCplx& u, EncCplx& v, EncCplx w) {
  if (INVERSE) {
    EncCplx d; d.re = u.re - v.re; d.im = u.im - v.im;
    u.re = u.re + v.re; u.im = u.im + v.im;
    v = enc_cmul(d, w);
  } else {
    const EncCplx t = enc_cmul(v, w);
    v.re = u.re - t.re; v.im = u.im - t.im;
    u.re = u.re + t.re; u.im = u.im + t.im;
  }
}

// values[i] /= complex(float64(n), 0) as Go's runtime divides complex128 (Smith's algorithm with |re m| >= |im m|): ratio = 0 / n,
// denom = n + ratio * 0, e = (re + im * ratio) / denom, f = (im - re * ratio) / denom -- the products with the zero ratio decide the sign of a zero
__device__ __forceinline__ EncCplx enc_div_n(EncCplx x, double n) {
  const double ratio = 0.0 / n, denom = n + ratio * 0.0;
  EncCplx r;
  r.re = (x.re + x.im * ratio) / denom;
  r.im = (x.im - x.re * ratio) / denom;
  return r;
}

// One stage in global memory: len = 1 << loglen over vectors of n = 1 << logn values; grid (ceil(n/2 / 256), nvec).  src == dst: in place
// (each thread reads its two values before it writes them; the two pointers may alias, so neither is restrict).
template <bool INVERSE>
__global__ void __launch_bounds__(256)
ckks_fft_stage_kernel(const EncCplx* src, EncCplx* dst, int logn, int loglen, int logm,
                      const EncCplx* __restrict__ roots, const unsigned* __restrict__ rot) {
  const unsigned half = 1u << (logn - 1), t = blockIdx.x * 256u + threadIdx.x;
  if (t >= half) return;
  const unsigned lenh = 1u << (loglen - 1), j = t & (lenh - 1), k = ((t >> (loglen - 1)) << loglen) + j;
  const size_t base = (size_t)blockIdx.y << logn;
  EncCplx u = src[base + k], v = src[base + k + lenh];
  enc_bfly<INVERSE>(u, v, enc_root<INVERSE>(roots, rot, j, loglen, logm));
  dst[base + k] = u; dst[base + k + lenh] = v;
}

// The stages with len <= 1 << logb of one block of 1 << logb values in LDS (real and imaginary parts in separate arrays), two stages per
// exchange: each thread holds the four values of a radix-4 group in registers for a pair of stages.  grid (n >> logb, nvec); dynamic LDS
// 16 << logb bytes.
//   INVERSE: block b of src in natural order, stages len = 1 << logb down to 2, then the division by n and the bit reversal of the whole
//            vector folded into the store: dst[bitrev(i)] = x[i] / n.
//   forward: the load gathers dst-order position p from src[bitrev(p)], stages len = 2 up to 1 << logb, natural-order store.
// src == dst is safe only when one block holds the whole vector (logb == logn): every value is in LDS before the first store.
template <bool INVERSE>
__global__ void __launch_bounds__(256)
ckks_fft_lds_kernel(const EncCplx* src, EncCplx* dst, int logn, int logb, int logm,
                    const EncCplx* __restrict__ roots, const unsigned* __restrict__ rot) {
  extern __shared__ double enc_lds[];
  const unsigned nb = 1u << logb;
  double* sre = enc_lds; double* sim = enc_lds + nb;
  const size_t vbase = (size_t)blockIdx.y << logn;
  const unsigned b0 = blockIdx.x << logb;
  for (unsigned i = threadIdx.x; i < nb; i += 256) {
    const EncCplx x = src[vbase + (INVERSE ? b0 + i : rh_brev(b0 + i, logn))];
    sre[i] = x.re; sim[i] = x.im;
  }
  __syncthreads();
  // stage pairs (hi, hi - 1): a group is {k, k + q, k + 2q, k + 3q} with q = 1 << (hi - 2)... (len = 1 << hi, then 1 << (hi - 1))
  int done = 0;
  while (logb - done >= 2) {
    const int hi = INVERSE ? logb - done : done + 2;            // the larger len of the pair
    const unsigned q = 1u << (hi - 2);
    for (unsigned t = threadIdx.x; t < (nb >> 2); t += 256) {
      const unsigned j = t & (q - 1), k = ((t >> (hi - 2)) << hi) + j;
      EncCplx x0{sre[k], sim[k]}, x1{sre[k + q], sim[k + q]}, x2{sre[k + 2 * q], sim[k + 2 * q]}, x3{sre[k + 3 * q], sim[k + 3 * q]};
      if (INVERSE) {
        enc_bfly<true>(x0, x2, enc_root<true>(roots, rot, j, hi, logm));            // len = 1 << hi: pairs (k, k + len/2)
        enc_bfly<true>(x1, x3, enc_root<true>(roots, rot, j + q, hi, logm));
        const EncCplx w = enc_root<true>(roots, rot, j, hi - 1, logm);                // len = 1 << (hi - 1): pairs (k, k + len/4) in both halves
        enc_bfly<true>(x0, x1, w);
        enc_bfly<true>(x2, x3, w);
      } else {
        const EncCplx w = enc_root<false>(roots, rot, j, hi - 1, logm);
        enc_bfly<false>(x0, x1, w);
        enc_bfly<false>(x2, x3, w);
        enc_bfly<false>(x0, x2, enc_root<false>(roots, rot, j, hi, logm));
        enc_bfly<false>(x1, x3, enc_root<false>(roots, rot, j + q, hi, logm));
      }
      sre[k] = x0.re; sim[k] = x0.im; sre[k + q] = x1.re; sim[k + q] = x1.im;
      sre[k + 2 * q] = x2.re; sim[k + 2 * q] = x2.im; sre[k + 3 * q] = x3.re; sim[k + 3 * q] = x3.im;
    }
    __syncthreads();
    done += 2;
  }
  if (logb - done == 1) {                                         // odd stage count: the last single stage
    const int ll = INVERSE ? 1 : logb;
    const unsigned lenh = 1u << (ll - 1);
    for (unsigned t = threadIdx.x; t < (nb >> 1); t += 256) {
      const unsigned j = t & (lenh - 1), k = ((t >> (ll - 1)) << ll) + j;
      EncCplx u{sre[k], sim[k]}, v{sre[k + lenh], sim[k + lenh]};
      if (INVERSE) enc_bfly<true>(u, v, enc_root<true>(roots, rot, j, ll, logm));
      else enc_bfly<false>(u, v, enc_root<false>(roots, rot, j, ll, logm));
      sre[k] = u.re; sim[k] = u.im; sre[k + lenh] = v.re; sim[k + lenh] = v.im;
    }
    __syncthreads();
  }
  const double n = (double)(1u << logn);
  for (unsigned i = threadIdx.x; i < nb; i += 256) {
    EncCplx x{sre[i], sim[i]};
    if (INVERSE) dst[vbase + rh_brev(b0 + i, logn)] = enc_div_n(x, n);
    else dst[vbase + b0 + i] = x;
  }
}

// buffCmplx[i] = complex(real(values[i]), 0): the copy into the encoder's buffer on a conjugate-invariant ring (encoder.go:225-228)
__global__ void __launch_bounds__(256)
ckks_copy_real_kernel(const double* __restrict__ vals, double* __restrict__ out, size_t count) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  out[2 * i] = vals[2 * i];
  out[2 * i + 1] = 0.0;
}

// ---- quantizer (SingleFloat64ToFixedPointCRT, utils.go:171-234) -------------------------------------------------------------------------
// (m * 2^e) mod q for a 53-bit m and e >= 0: the integer the reference's big.Float path holds (its 53-bit + 0.5 is a no-op at >= 2^64)
__device__ __forceinline__ u64 enc_big_mod(u64 m, int e, const LimbConsts& c) {
  u64 r = bred_add(m, c.q, c.bred0);
  const u64 p32 = bred_add(1ull << 32, c.q, c.bred0);
  for (; e >= 32; e -= 32) r = bred(r, p32, c.q, c.bred0, c.bred1);
  if (e) r = bred(r, bred_add(1ull << e, c.q, c.bred0), c.q, c.bred0, c.bred1);
  return r;
}

// One thread per coefficient, limb loop inside; out: (nvec, L, N).  grid (N / 256 rounded up, nvec).
//   batched:  vals (nvec, slots) complex: coefficient i = k * gap takes re[k] for k < slots, im[k - slots] for k < 2 slots; zero elsewhere
//             (Complex128ToFixedPointCRT, then the stride-gap spread of NTTSparseAndMontgomery)
//             real (conjugate-invariant ring, gap = N / slots): coefficient i = k * gap takes re[k] for k < slots and nothing reads the
//             imaginary parts (the `else` arm, utils.go:145-147): half the value traffic, no second coefficient block
//   !batched: vals (nvec, nvals) doubles: coefficient i < nvals takes vals[i] (Float64ToFixedPointCRT)
// canonical: the word is reduced to [0, q) -- the reference stores positive words unreduced and q for a negative multiple of q; what follows
//            (NTT, MForm) maps either to the canonical residue of the class, so the reduction happens here.  mont: then MForm.
__global__ void __launch_bounds__(256)
ckks_quantize_kernel(const double* __restrict__ vals, u64* __restrict__ out, unsigned n, int L, const LimbConsts* __restrict__ consts,
                     double scale, int batched, unsigned slots, unsigned nvals, int loggap, int canonical, int mont, int real) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const size_t vec = blockIdx.y;
  double v = 0.0;
  if (batched) {
    const unsigned k = i >> loggap;
    if ((k << loggap) == i && k < (real ? slots : 2 * slots)) v = k < slots ? vals[(vec * slots + k) * 2] : vals[(vec * slots + (k - slots)) * 2 + 1];
  } else if (i < nvals) {
    v = vals[vec * nvals + i];
  }
  u64* o = out + vec * (size_t)L * n + i;
  if (v == 0) {                                                   // (:173-179), +0.0 and -0.0 alike
    for (int j = 0; j < L; ++j) o[(size_t)j * n] = 0;
    return;
  }
  const bool neg = v < 0;
  if (neg) scale *= -1;                                           // the sign goes onto the scale (:189-192)
  v *= scale;
  const bool big = v >= 1.8446744073709552e+19;
  u64 cw = 0, mant = 0; int e = 0;
  if (big) {
    const u64 bits = (u64)__double_as_longlong(v);
    mant = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    e = (int)((bits >> 52) & 0x7ff) - 1075;                       // >= 12 here
  } else {
    cw = (u64)(v + 0.5);                                          // (:215)
  }
  for (int j = 0; j < L; ++j) {
    const LimbConsts c = consts[j];
    u64 w;
    if (big) {
      const u64 r = enc_big_mod(mant, e, c);
      w = neg ? c.q - r : r;                                      // (:203-210): q - 0 = q
    } else if (neg) {
      w = cw > c.q ? c.q - bred_add(cw, c.q, c.bred0) : c.q - cw; // (:217-223): the word q when q divides c
    } else {
      w = cw > 0x1fffffffffffffffull ? bred_add(cw, c.q, c.bred0) : cw;   // (:225-231): unreduced up to 2^61 - 1
    }
    if (canonical) w = bred_add(w, c.q, c.bred0);
    if (mont) w = mform(w, c.q, c.bred0, c.bred1);
    o[(size_t)j * n] = w;
  }
}

// ---- decoder: residues -> centred integer -> nearest double -> / scale (encoder.go:796-1003, scaling.go:46-52) -----------------------------
struct EncCrtTables {
  const u64* garner;    // (Lmax): (q_0 ... q_{j-1})^-1 mod q_j
  const u64* qmod;      // (Lmax, Lmax): q_i mod q_j at [j * Lmax + i]
  const u64* Q;         // (Lmax levels, Lmax words): q_0 ... q_level, little endian
  const u64* Qhalf;     // ... >> 1
  int Lmax;
};

// One thread per gathered coefficient: k < slots the real part of slot k (coefficient k * gap), else the imaginary part of slot k - slots
// (coefficient N/2 + (k - slots) * gap).  The integer is rebuilt exactly: mixed-radix digits d_j (Garner), Horner over words, c >= Q >> 1
// gives c - Q, then the top 64 bits and a sticky bit round to nearest, ties to even -- big.Float.Float64 (level > 0) and float64(uint64)
// (level 0) are that rounding.  vals: (nvec, slots) complex, written whole.  grid (2 slots / 256 rounded up, nvec).
// coeffs == 1 (polyToFloatNoCRT / polyToFloatCRT, encoder.go:1006-1185): no gather -- thread k takes coefficient k of all N, vals is
// (nvec, N) doubles.  grid (N / 256 rounded up, nvec).
// coeffs == 2 (the `isreal` arms, :825-831, :938-944; n / slots = gap): thread k < slots takes coefficient k * gap, x, and writes
// re[k] = x / scale and im[slots - k] = 0 - x / scale (im[0] = 0): "values[i] -= complex(0, real(values[slots-i]))" for i >= 1, with the
// division before (CRT) or after (level 0) the subtraction -- the same double, division being odd.  grid (slots / 256 rounded up, nvec).
__global__ void __launch_bounds__(256)
ckks_crt_to_double_kernel(const u64* __restrict__ poly, double* __restrict__ vals, unsigned n, int L, const LimbConsts* __restrict__ consts,
                          EncCrtTables tb, double scale, unsigned slots, int loggap, int coeffs) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k >= (coeffs == 1 ? n : coeffs == 2 ? slots : 2 * slots)) return;
  const size_t vec = blockIdx.y;
  const bool imag = !coeffs && k >= slots;
  const unsigned s = imag ? k - slots : k, idx = coeffs == 1 ? k : (imag ? (n >> 1) : 0u) + (s << loggap);
  const u64* p = poly + vec * (size_t)L * n + idx;
  u64 d[RH_MAX_LIMBS_K], acc[RH_MAX_LIMBS_K];
  for (int j = 0; j < L; ++j) {                                   // d_j = (r_j - (d_0 + q_0 (d_1 + q_1 (...))) mod q_j) * garner_j mod q_j
    const LimbConsts c = consts[j];
    const u64 r = bred_add(p[(size_t)j * n], c.q, c.bred0);
    u64 t = 0;
    for (int i = j - 1; i >= 0; --i) {
      t = bred(t, tb.qmod[j * tb.Lmax + i], c.q, c.bred0, c.bred1);
      t = cred(t + bred_add(d[i], c.q, c.bred0), c.q);
    }
    const u64 diff = r >= t ? r - t : r + c.q - t;
    d[j] = j ? bred(diff, tb.garner[j], c.q, c.bred0, c.bred1) : diff;
  }
  for (int j = 0; j < L; ++j) acc[j] = 0;
  for (int j = L - 1; j >= 0; --j) {                              // acc = acc * q_j + d_j; the value stays below Q: L words hold it
    const u64 q = consts[j].q;
    u64 carry = d[j];
    for (int w = 0; w < L; ++w) {
      const u128 m = (u128)acc[w] * q + carry;
      acc[w] = (u64)m; carry = (u64)(m >> 64);
    }
  }
  const u64* Q = tb.Q + (size_t)(L - 1) * tb.Lmax;
  const u64* Qh = tb.Qhalf + (size_t)(L - 1) * tb.Lmax;
  int cmp = 0;                                                    // acc vs Q >> 1
  for (int w = L - 1; w >= 0 && !cmp; --w) cmp = acc[w] > Qh[w] ? 1 : acc[w] < Qh[w] ? -1 : 0;
  const bool neg = cmp >= 0;
  if (neg) {                                                      // |acc - Q| = Q - acc
    u64 borrow = 0;
    for (int w = 0; w < L; ++w) {
      const u64 a = Q[w], b = acc[w], x = a - b, y = x - borrow;
      borrow = (a < b) | (x < borrow);
      acc[w] = y;
    }
  }
  int top = L - 1;
  while (top > 0 && acc[top] == 0) --top;
  double x;
  if (top == 0) {
    x = (double)acc[0];                                           // one word: the conversion rounds to nearest even
  } else {
    const int lz = __clzll((long long)acc[top]);
    u64 hi = acc[top] << lz;
    if (lz) hi |= acc[top - 1] >> (64 - lz);
    u64 sticky = lz ? acc[top - 1] << lz : acc[top - 1];
    for (int w = top - 2; w >= 0; --w) sticky |= acc[w];
    u64 mant = hi >> 11;
    const u64 rem = hi & 0x7ff;
    if (rem > 0x400 || (rem == 0x400 && (sticky || (mant & 1)))) ++mant;
    x = ldexp((double)mant, 64 * top - lz + 11);
  }
  if (neg) x = -x;
  if (coeffs == 2) {
    const double y = x / scale;
    vals[(vec * slots + s) * 2] = y;
    vals[(vec * slots + (s ? slots - s : 0u)) * 2 + 1] = s ? 0.0 - y : 0.0;
  } else if (coeffs) vals[vec * n + k] = x / scale;
  else vals[(vec * slots + s) * 2 + (imag ? 1 : 0)] = x / scale;
}

// do_round: math.Round(x * 2^logprec) / 2^logprec on both parts (encoder.go:511-525; round() is half away from zero, as math.Round);
// real_only: the imaginary part becomes zero (the []float64 / []*big.Float outputs read the real parts alone)
__global__ void __launch_bounds__(256)
ckks_round_prec_kernel(double* __restrict__ vals, size_t count, double p2, int do_round, int real_only) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= count) return;
  if (do_round) vals[2 * i] = round(vals[2 * i] * p2) / p2;
  if (real_only) vals[2 * i + 1] = 0.0;
  else if (do_round) vals[2 * i + 1] = round(vals[2 * i + 1] * p2) / p2;
}

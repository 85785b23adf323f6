// matrix_ckks_kernels.hip.hpp -- the kernels of the Matrix CKKS encoder (matrix_ckks.hip): schemes/matrix_ckks/encoder.go:367-445.
#pragma once
#include "modarith.hip.hpp"
#include "ring_types.hip.hpp"

enum { MCK_U64 = 0, MCK_F64 = 1, MCK_C128 = 2 };       // []uint64, []float64, []complex128 (real parts, encoder.go:237-241)

// the float64 a value of the block stands for: float64(val) for uint64 (round to nearest even above 2^53, encoder.go:187-190)
RH_DEV double mck_value(const void* values, int vtype, size_t at) {
  if (vtype == MCK_U64) return (double)reinterpret_cast<const u64*>(values)[at];
  if (vtype == MCK_F64) return reinterpret_cast<const double*>(values)[at];
  return reinterpret_cast<const double*>(values)[2 * at];
}

// ---- Encode: SingleFloat64ToFixedPointCRT (encoder.go:384-426) for every coefficient of every vector, one launch -----------------------------------
// values: (nvec, nvals) of vtype.  out: dense (nvec, L, n) words, coefficient domain; coefficients i >= nvals are 0 (:196-201).
// The sign goes onto the scale, the product is TRUNCATED (uint64(value)), and
//   value <  2^64: c = uint64(value), negative: c = -c modulo 2^64
//   value >= 2^64: the LOW 64 bits of the integer m 2^e the float is (big.Int.Uint64), no sign applied
// The reference stores CRed(word, q) (one conditional subtraction: it can stay >= q); this kernel stores the canonical residue of that word.
// SIGNED (negatives="signed"): a negative value stores q - (|c| mod q), on the big path q - (m 2^e mod q) -- what polyToFloatNoCRT's centring decodes.
// grid (nvec, chunks): a thread owns one coefficient and walks the limbs; a wave writes 512 contiguous bytes per limb.
template <bool SIGNED>
__global__ void __launch_bounds__(256)
matrix_ckks_encode_kernel(const void* __restrict__ values, int vtype, unsigned nvals, double scale, u64* __restrict__ out, unsigned n,
                          const LimbConsts* __restrict__ consts, int L) {
  const u32 vec = blockIdx.x;
  u64* dst = out + (size_t)vec * (size_t)L * n;
  for (unsigned i = blockIdx.y * blockDim.x + threadIdx.x; i < n; i += gridDim.y * blockDim.x) {
    double v = i < nvals ? mck_value(values, vtype, (size_t)vec * nvals + i) : 0.0;
    if (v == 0) {
      for (int l = 0; l < L; ++l) dst[(size_t)l * n + i] = 0;
      continue;
    }
    const bool neg = v < 0;
    v *= neg ? -scale : scale;                                         // (:399-404)
    const bool big = v >= 1.8446744073709552e+19;
    u64 word, m = 0;
    int e = 0;
    if (big) {                                                          // the float is the integer m 2^e, e >= 12
      const u64 bits = (u64)__double_as_longlong(v);
      m = (bits & 0xfffffffffffffull) | (1ull << 52);
      e = (int)((bits >> 52) & 0x7ff) - 1075;
      word = e >= 64 ? 0 : m << e;
    } else {
      word = (u64)v;
      if (neg && !SIGNED) word = (u64)0 - word;
    }
    for (int l = 0; l < L; ++l) {
      const u64 q = consts[l].q, b0 = consts[l].bred0;
      u64 r;
      if (SIGNED && neg) {
        if (big) {
          r = bred_add(m, q, b0);
          for (int k = 0; k < e; ++k) r = cred(r + r, q);
        } else {
          r = bred_add(word, q, b0);
        }
        r = r ? q - r : 0;
      } else {
        r = bred_add(word, q, b0);
      }
      dst[(size_t)l * n + i] = r;
    }
  }
}

// ---- Decode: polyToFloatNoCRT (encoder.go:430-445) on limb 0 alone --------------------------------------------------------------------------------
// in: coefficient-domain rows, limb 0 of vector v at in + v * in_rows * n.  c >= q0 >> 1 ? -float64(q0 - c) / scale : float64(c) / scale with IEEE
// conversions and division, for the first nvals coefficients, into (nvec, nvals) float64, complex128 (imaginary part 0) or uint64 (truncated;
// a negative value's word is not defined by the reference: 0 here).  grid (nvec, chunks)
__global__ void __launch_bounds__(256)
matrix_ckks_decode_kernel(const u64* __restrict__ in, int in_rows, unsigned n, u64 q0, double scale, void* __restrict__ values, int vtype,
                          unsigned nvals) {
  const u32 vec = blockIdx.x;
  const u64* src = in + (size_t)vec * (size_t)in_rows * n;
  for (unsigned i = blockIdx.y * blockDim.x + threadIdx.x; i < nvals; i += gridDim.y * blockDim.x) {
    const u64 c = src[i];
    const double v = c >= (q0 >> 1) ? -(double)(q0 - c) / scale : (double)c / scale;
    const size_t at = (size_t)vec * nvals + i;
    if (vtype == MCK_F64) reinterpret_cast<double*>(values)[at] = v;
    else if (vtype == MCK_C128) reinterpret_cast<double2*>(values)[at] = make_double2(v, 0.0);
    else reinterpret_cast<u64*>(values)[at] = v >= 0 ? (v >= 1.8446744073709552e+19 ? ~0ull : (u64)v) : 0;
  }
}

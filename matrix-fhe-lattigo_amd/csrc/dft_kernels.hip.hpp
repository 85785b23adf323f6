// dft_kernels.hip.hpp -- device side of circuits/ckks/dft/dft.go GenMatrices (float64 path): the vectors of one FFT level (fftPlainVec /
// ifftPlainVec :362-490), the merge of a factor with the next level (genFFTDiagMatrix :775-804, multiplyFFTMatrixWithNextFFTLevel :831-862) as a
// gather, and the scaling / repack zeroing / BSGS pre-rotation pass that hands a factor to the encoder.
//
// All floating point is IEEE double, real and imaginary parts as separate scalars, one operation per source operation: a complex product is four
// rounded products and one rounded sum and difference (ComplexMultiplier.Mul), never an FMA (the library is built with -ffp-contract=off and the
// pragma below keeps it so for this header).  The ORDER of the additions into a diagonal is the host program's (dft.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "ring_types.hip.hpp"

#pragma clang fp contract(off)

struct DftCplx { double re, im; };

__device__ __forceinline__ DftCplx dft_cmul(DftCplx x, DftCplx w) {
  DftCplx r;
  r.re = x.re * w.re - x.im * w.im;
  r.im = x.re * w.im + x.im * w.re;
  return r;
}

__device__ __forceinline__ unsigned dft_bitrev(unsigned x, int bits) { return bits ? __brev(x) >> (32 - bits) : 0u; }

// out: (3, dslots) = a, b, c of the level with butterflies of span m = 1 << logm over `slots` = 1 << log_slots values; dslots = slots or 2 slots
// (the second copy).  DECODE: fftPlainVec (b = roots[k], c = 1 with k = (pow5[j] & mask) gap); else ifftPlainVec (b = 1, c = roots[k] with
// k = (4 m - (pow5[j] & mask)) gap); a = 1 on the upper half of a butterfly and -roots[k] on the lower.  bitrev: every block of `slots` values
// bit-reversed (utils.BitReverseInPlaceSlice), written as a gather.  roots: 4 slots + 1 entries; pow5: at least slots / 2.
template <bool DECODE>
__global__ void __launch_bounds__(256)
dft_level_vectors_kernel(DftCplx* __restrict__ out, const DftCplx* __restrict__ roots, const u64* __restrict__ pow5, int log_slots, int logm,
                         unsigned dslots, int bitrev) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= dslots) return;
  const unsigned slots = 1u << log_slots, m = 1u << logm, tt = m >> 1;
  unsigned p = x & (slots - 1);
  if (bitrev) p = dft_bitrev(p, log_slots);
  const unsigned jj = p & (m - 1), j = jj & (tt - 1);
  const unsigned gap = slots >> logm, mask = (m << 2) - 1, r = (unsigned)pow5[j] & mask;
  const size_t k = (size_t)(DECODE ? r : (m << 2) - r) * gap;
  const DftCplx w = roots[k], one = roots[0], zero = {0.0, 0.0};
  DftCplx a, b, c;
  if (jj < tt) { a = one; b = DECODE ? w : one; c = zero; }
  else { a.re = -w.re; a.im = -w.im; b = zero; c = DECODE ? one : w; }
  out[x] = a; out[(size_t)dslots + x] = b; out[2 * (size_t)dslots + x] = c;
}

// One program word per contribution, three per output diagonal: DFT_NONE, or kind << 32 | (source row + 1); source row + 1 = 0: the level's
// vector itself (genFFTDiagMatrix); kind 0 a, 1 b (the source rotated by rot), 2 c (by -rot).  The rotation is modulo dslots.
#define DFT_NONE (~(u64)0)
// grid: (chunks of 256 slots, nout)
__global__ void __launch_bounds__(256)
dft_merge_level_kernel(DftCplx* __restrict__ out, const DftCplx* __restrict__ vec, const DftCplx* __restrict__ abc, const u64* __restrict__ program,
                       unsigned dslots, unsigned rot) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y;
  if (x >= dslots) return;
  const unsigned mask = dslots - 1;
  DftCplx acc = {0.0, 0.0};
  bool first = true;
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const u64 w = program[3 * (size_t)d + t];                            // wave-uniform
    if (w == DFT_NONE) continue;
    const unsigned kind = (unsigned)(w >> 32), src = (unsigned)w;
    DftCplx v = abc[(size_t)kind * dslots + x];
    if (src) {
      const unsigned xs = kind == 0 ? x : kind == 1 ? (x + rot) & mask : (x - rot) & mask;
      v = dft_cmul(v, vec[(size_t)(src - 1) * dslots + xs]);
    }
    if (first) { acc = v; first = false; }                               // addToDiagMatrix: the first contribution is copied
    else { acc.re = acc.re + v.re; acc.im = acc.im + v.im; }
  }
  out[(size_t)d * dslots + x] = acc;
}

// out[d][x] = in[d][(x + rots[d]) mod dslots] * scaling, both parts; zero_upper: slots [dslots / 2, dslots) of the source are zero (the repack
// after a sparse HomomorphicEncode, :733-740).  rots null: no rotation (and out may be in).  grid: (chunks of 256 slots, ndiag)
__global__ void __launch_bounds__(256)
dft_finish_kernel(DftCplx* out, const DftCplx* in, const u64* __restrict__ rots, unsigned dslots, double scaling, int zero_upper) {
  const unsigned x = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y;
  if (x >= dslots) return;
  const unsigned xs = rots ? (x + (unsigned)rots[d]) & (dslots - 1) : x;
  DftCplx v = in[(size_t)d * dslots + xs];
  if (zero_upper && xs >= (dslots >> 1)) { v.re = 0.0; v.im = 0.0; }
  v.re = v.re * scaling; v.im = v.im * scaling;
  out[(size_t)d * dslots + x] = v;
}

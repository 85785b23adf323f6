// dft.hip -- circuits/ckks/dft/dft.go GenMatrices on the device (float64 path): every factor of the factorised encoding matrices as ONE
// (ndiag, dslots) complex128 block in HBM, built by three kernels (dft_kernels.hip.hpp):
//   rh_ckks_dft_level_vectors  a, b, c of one FFT level (fftPlainVec / ifftPlainVec :362-490), the second copy and the bit reversal included
//   rh_ckks_dft_merge_level    genFFTDiagMatrix (:775-804) or multiplyFFTMatrixWithNextFFTLevel (:831-862) as a gather: per output diagonal
//                              up to three contributions, in the order the host program lists them
//   rh_ckks_dft_finish         the real scaling (:762-770), the repack zeroing (:733-740) and the rotation by -j of giant step j
//                              (lintrans.Encode :246-262), so that the block goes to the encoder as it is
// The reference adds the contributions in the order of a Go map; the program fixes it (ascending source diagonal, then a, b, c), and the kernel
// adds in program order.  The ring handle gives the device and the stream; no modulus is involved.
#include <hip/hip_runtime.h>
#include "engine_internal.hpp"
#include "dft_kernels.hip.hpp"

#define DFT_MAX_LOG_SLOTS 16

static int dft_shape(const rh_ring* r, int log_slots, unsigned dslots, const char* who) {
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (log_slots < 1 || log_slots > DFT_MAX_LOG_SLOTS) return rh_fail(RH_ERR_ARG, "%s: log_slots %d out of range [1,%d]", who, log_slots, DFT_MAX_LOG_SLOTS);
  const unsigned slots = 1u << log_slots;
  if (dslots != slots && dslots != 2 * slots) return rh_fail(RH_ERR_ARG, "%s: dslots %u is neither slots = %u nor 2 slots", who, dslots, slots);
  return RH_OK;
}

static int dft_block(unsigned dslots, int ndiag, const char* who) {
  if (dslots < 2 || (dslots & (dslots - 1)) || dslots > (2u << DFT_MAX_LOG_SLOTS)) return rh_fail(RH_ERR_ARG, "%s: dslots %u must be a power of two in [2, 2^%d]", who, dslots, DFT_MAX_LOG_SLOTS + 1);
  if (ndiag < 1 || ndiag > 65535) return rh_fail(RH_ERR_ARG, "%s: %d diagonals, need 1 .. 65535", who, ndiag);
  return RH_OK;
}

extern "C" int rh_ckks_dft_level_vectors(rh_ring* r, int decode, int log_slots, unsigned dslots, int fft_level, int bit_reversed,
                                         const double* roots_dev, size_t nroots, const uint64_t* pow5_dev, size_t npow5, double* abc_dev) {
  const char* who = "rh_ckks_dft_level_vectors";
  if (int rc = dft_shape(r, log_slots, dslots, who)) return rc;
  if (!roots_dev || !pow5_dev || !abc_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (fft_level < 1 || fft_level > log_slots) return rh_fail(RH_ERR_ARG, "%s: fft_level %d out of range [1,%d]", who, fft_level, log_slots);
  const size_t slots = (size_t)1 << log_slots;
  if (nroots != 4 * slots + 1) return rh_fail(RH_ERR_ARG, "%s: %zu roots given, 4 slots + 1 = %zu expected", who, nroots, 4 * slots + 1);
  if (npow5 < (slots >> 1) || npow5 < 1) return rh_fail(RH_ERR_ARG, "%s: %zu powers of five given, at least %zu expected", who, npow5, slots >> 1 ? slots >> 1 : 1);
  const int logm = decode ? log_slots - fft_level + 1 : fft_level;       // a[logSlots - fftLevel]: m = 2 << index (fft), slots >> index (ifft)
  (void)hipSetDevice(r->device);
  (void)hipGetLastError();
  hipStream_t st = rh_stream(r);
  const unsigned blocks = (dslots + 255) / 256;
  if (decode) dft_level_vectors_kernel<true><<<blocks, 256, 0, st>>>((DftCplx*)abc_dev, (const DftCplx*)roots_dev, pow5_dev, log_slots, logm, dslots, bit_reversed ? 1 : 0);
  else dft_level_vectors_kernel<false><<<blocks, 256, 0, st>>>((DftCplx*)abc_dev, (const DftCplx*)roots_dev, pow5_dev, log_slots, logm, dslots, bit_reversed ? 1 : 0);
  return rh_launch_ok("dft_level_vectors_kernel");
}

extern "C" int rh_ckks_dft_merge_level(rh_ring* r, unsigned dslots, int rot, const double* abc_dev, const double* vec_dev, int nin, const int* program,
                                       int nout, double* out_dev, uint64_t* table_dev, size_t table_words) {
  const char* who = "rh_ckks_dft_merge_level";
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (int rc = dft_block(dslots, nout, who)) return rc;
  if (!abc_dev || !program || !out_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (!table_dev) return rh_fail(RH_ERR_ARG, "%s: null table (device scratch of 3 words per output diagonal)", who);
  if (nin < 0 || (nin > 0 && !vec_dev)) return rh_fail(RH_ERR_ARG, "%s: %d source diagonals without a source block", who, nin);
  if (rot < 0 || (unsigned)rot >= dslots) return rh_fail(RH_ERR_ARG, "%s: rot %d out of range [0,%u)", who, rot, dslots);
  const size_t words = 3 * (size_t)nout;
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the table holds %zu words, %d diagonals need %zu", who, table_words, nout, words);
  const RhBlock written[2] = {{out_dev, 2 * (size_t)nout * dslots}, {table_dev, words}};
  const RhBlock read[2] = {{abc_dev, 6 * (size_t)dslots}, {vec_dev ? vec_dev : abc_dev, vec_dev ? 2 * (size_t)nin * dslots : 0}};
  if (int rc = rh_blocks_ok(written, 2, read, 2, who, "the output (or the table) overlaps an input: a level is not merged in place")) return rc;
  if (int rc = rh_blocks_disjoint(written, 2, who, "the output overlaps the table")) return rc;
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  // program: per output diagonal three (source, kind) pairs; source -2: no contribution, -1: the level's vector alone, else a row of vec
  for (int d = 0; d < nout; ++d) {
    int used = 0;
    for (int t = 0; t < 3; ++t) {
      const int src = program[6 * (size_t)d + 2 * t], kind = program[6 * (size_t)d + 2 * t + 1];
      if (src == -2) { stage->h[3 * (size_t)d + t] = DFT_NONE; continue; }
      if (src < -1 || src >= nin) return rh_fail(RH_ERR_ARG, "%s: diagonal %d names source %d of %d", who, d, src, nin);
      if (kind < 0 || kind > 2) return rh_fail(RH_ERR_ARG, "%s: diagonal %d names kind %d (0 a, 1 b, 2 c)", who, d, kind);
      stage->h[3 * (size_t)d + t] = (u64)kind << 32 | (u64)(unsigned)(src + 1);
      ++used;
    }
    if (!used) return rh_fail(RH_ERR_ARG, "%s: diagonal %d has no contribution", who, d);
  }
  (void)hipSetDevice(r->device);
  (void)hipGetLastError();
  hipStream_t st = rh_stream(r);
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  const dim3 grid((dslots + 255) / 256, (unsigned)nout);
  dft_merge_level_kernel<<<grid, 256, 0, st>>>((DftCplx*)out_dev, (const DftCplx*)vec_dev, (const DftCplx*)abc_dev, table_dev, dslots, (unsigned)rot);
  return rh_launch_ok("dft_merge_level_kernel");
}

extern "C" int rh_ckks_dft_finish(rh_ring* r, unsigned dslots, int ndiag, const double* in_dev, double* out_dev, double scaling, int zero_upper,
                                  const int* rots, uint64_t* table_dev, size_t table_words) {
  const char* who = "rh_ckks_dft_finish";
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (int rc = dft_block(dslots, ndiag, who)) return rc;
  if (!in_dev || !out_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  (void)hipSetDevice(r->device);
  (void)hipGetLastError();
  hipStream_t st = rh_stream(r);
  if (rots) {
    if (!table_dev) return rh_fail(RH_ERR_ARG, "%s: null table (device scratch of one word per diagonal)", who);
    if (table_words < (size_t)ndiag) return rh_fail(RH_ERR_ARG, "%s: the table holds %zu words, %d diagonals need %d", who, table_words, ndiag, ndiag);
    const RhBlock written[2] = {{out_dev, 2 * (size_t)ndiag * dslots}, {table_dev, (size_t)ndiag}};
    const RhBlock read[1] = {{in_dev, 2 * (size_t)ndiag * dslots}};
    if (int rc = rh_blocks_ok(written, 2, read, 1, who, "the output (or the table) overlaps the input: rotated diagonals are not written in place")) return rc;
    if (int rc = rh_blocks_disjoint(written, 2, who, "the output overlaps the table")) return rc;
    RhStage* stage;
    if (int rc = rh_stage_slot((size_t)ndiag, &stage, who)) return rc;
    for (int d = 0; d < ndiag; ++d) {
      if (rots[d] < 0 || (unsigned)rots[d] >= dslots) return rh_fail(RH_ERR_ARG, "%s: rotation %d of diagonal %d out of range [0,%u)", who, rots[d], d, dslots);
      stage->h[d] = (u64)rots[d];
    }
    if (int rc = rh_stage_upload(stage, table_dev, (size_t)ndiag, st, who)) return rc;
  } else if (in_dev != out_dev) {
    const RhBlock written[1] = {{out_dev, 2 * (size_t)ndiag * dslots}};
    const RhBlock read[1] = {{in_dev, 2 * (size_t)ndiag * dslots}};
    if (int rc = rh_blocks_ok(written, 1, read, 1, who, "the output overlaps the input without being the input")) return rc;
  }
  const dim3 grid((dslots + 255) / 256, (unsigned)ndiag);
  dft_finish_kernel<<<grid, 256, 0, st>>>((DftCplx*)out_dev, (const DftCplx*)in_dev, rots ? table_dev : nullptr, dslots, scaling, zero_upper ? 1 : 0);
  return rh_launch_ok("dft_finish_kernel");
}

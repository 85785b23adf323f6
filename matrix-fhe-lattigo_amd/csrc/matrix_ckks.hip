// matrix_ckks.hip -- the Matrix CKKS encoder on the device (kernels: matrix_ckks_kernels.hip.hpp):
//   rh_matrix_ckks_encode    Encoder.Encode: EncodePolynomial / EncodeFloat64 / EncodeComplex, schemes/matrix_ckks/encoder.go:163-257, through
//                            Float64ToFixedPointCRT and SingleFloat64ToFixedPointCRT, :367-426
//   rh_matrix_ckks_decode    polyToFloatNoCRT, :430-445, with the conversions of DecodePolynomial / DecodeFloat64 / DecodeComplex, :276-351
// The inverse transform of an NTT-domain plaintext (:314-317) is the ring's own, driven from the host (matrix_ckks.py).
#include <hip/hip_runtime.h>
#include "engine_internal.hpp"
#include "matrix_ckks_kernels.hip.hpp"

static int mck_ok(const rh_ring* r, int level, int nvec, int nvals, int vtype, double scale, const void* a, const void* b, const char* who) {
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (r->kind != RH_RING_3N) return rh_fail(RH_ERR_UNSUPPORTED, "%s: the Matrix CKKS encoder is defined on 3N rings", who);
  if (level < 0 || level >= r->L || level + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, r->L);
  if (nvec < 0 || nvals < 0) return rh_fail(RH_ERR_ARG, "%s: negative count", who);
  if (nvals > r->N) return rh_fail(RH_ERR_ARG, "too many values: %d > %d", nvals, r->N);
  if (vtype != MCK_U64 && vtype != MCK_F64 && vtype != MCK_C128) return rh_fail(RH_ERR_ARG, "%s: supported types are uint64 (0), float64 (1) and complex128 (2)", who);
  if (!(scale > 0) || scale > 1.7976931348623157e+308) return rh_fail(RH_ERR_ARG, "%s: the scale must be positive and finite", who);
  if (!b || (!a && nvals)) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (((uintptr_t)a & 15) || ((uintptr_t)b & 15)) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  if ((size_t)nvec > 0x7fffffffu / (size_t)(level + 1)) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  return RH_OK;
}
static unsigned mck_chunks(unsigned count) {                              // blockIdx.y extent: one coefficient per thread, at most 64 chunks
  unsigned chunks = (count + 255) / 256;
  return chunks > 64 ? 64 : (chunks ? chunks : 1);
}

extern "C" int rh_matrix_ckks_encode(rh_ring* r, int level, double scale, const void* values_dev, int vtype, int nvals, int nvec, int negatives_signed,
                                     uint64_t* pt_dev) {
  const char* who = "rh_matrix_ckks_encode";
  if (int rc = mck_ok(r, level, nvec, nvals, vtype, scale, values_dev, pt_dev, who)) return rc;
  if (!nvec) return RH_OK;
  const int L = level + 1;
  (void)rh_stream_begin(r, (unsigned)nvec * (unsigned)L);
  const dim3 grid((unsigned)nvec, mck_chunks((unsigned)r->N));
  if (negatives_signed) matrix_ckks_encode_kernel<true><<<grid, 256, 0, rh_stream(r)>>>(values_dev, vtype, (unsigned)nvals, scale, pt_dev, (unsigned)r->N, r->d_consts, L);
  else matrix_ckks_encode_kernel<false><<<grid, 256, 0, rh_stream(r)>>>(values_dev, vtype, (unsigned)nvals, scale, pt_dev, (unsigned)r->N, r->d_consts, L);
  return rh_launch_ok("matrix_ckks_encode_kernel");
}

extern "C" int rh_matrix_ckks_decode(rh_ring* r, double scale, const uint64_t* pt_dev, int pt_rows, int nvec, int nvals, int vtype, void* values_dev) {
  const char* who = "rh_matrix_ckks_decode";
  if (int rc = mck_ok(r, 0, nvec, nvals, vtype, scale, pt_dev, values_dev, who)) return rc;
  if (pt_rows < 1) return rh_fail(RH_ERR_ARG, "%s: fewer rows per poly than limbs", who);
  if (!nvec || !nvals) return RH_OK;
  (void)rh_stream_begin(r, (unsigned)nvec);
  matrix_ckks_decode_kernel<<<dim3((unsigned)nvec, mck_chunks((unsigned)nvals)), 256, 0, rh_stream(r)>>>(pt_dev, pt_rows, (unsigned)r->N, r->moduli[0], scale,
                                                                                                        values_dev, vtype, (unsigned)nvals);
  return rh_launch_ok("matrix_ckks_decode_kernel");
}

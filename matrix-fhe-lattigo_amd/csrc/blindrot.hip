// blindrot.hip -- rh_blindrot_core: the accumulator loops of a batch of blind rotations (core/rgsw/blindrot/evaluator.go:134-229) in one launch,
// one workgroup per accumulator (blindrot_kernels.hip.hpp).  The host derives each accumulator's program from its discrete-log sets
// (getDiscreteLogSets :258-280, evaluateFromDiscreteLogSets :189-229) and uploads it; the key tables are uploaded once per key set.
#include <hip/hip_runtime.h>
#include "engine_internal.hpp"
#include "blindrot_kernels.hip.hpp"

template <int PER, bool TWL>
static void br_launch(rh_ring* r, int nacc, u64* c0, u64* c1, const u64* rgsw, int nkeys, const u64* gal, const BrGalois& ge, int ngal, const int* off,
                      const int* ops, int nops, int pw2, int digits) {
  blindrot_core_kernel<PER, TWL><<<dim3((unsigned)nacc), BR_THREADS, 0, rh_stream(r)>>>(c0, c1, rgsw, nkeys, gal, ge, ngal, off, ops, nops, r->d_tw_fwd,
                                                                                       r->d_tw_inv, r->d_consts, r->logN, pw2, digits);
}

extern "C" int rh_blindrot_core(rh_ring* r, int pw2, int digits, const uint64_t* rgsw, int nkeys, const uint64_t* galois, const uint64_t* galois_elements,
                                int ngalois, const int32_t* prog_offsets, const int32_t* prog_ops, int nops, uint64_t* c0, uint64_t* c1, int nacc) {
  const char* who = "rh_blindrot_core";
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (r->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
  if (r->logN < BR_MIN_LOGN || r->logN > BR_MAX_LOGN)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: ring degree 2^%d outside 2^%d .. 2^%d, what one workgroup holds", who, r->logN, BR_MIN_LOGN, BR_MAX_LOGN);
  if (r->moduli[0] >> 61) return rh_fail(RH_ERR_ARG, "%s: modulus 0 is not below 2^61", who);
  if (pw2 < 1 || pw2 > 63 || digits < 1 || (long)(digits - 1) * pw2 >= 64)
    return rh_fail(RH_ERR_ARG, "%s: need a power-of-two decomposition, 1 <= pw2 <= 63, with digits >= 1 and (digits - 1) pw2 < 64 (pw2 = %d, digits = %d)", who, pw2, digits);
  if (nkeys < 0 || ngalois < 0 || nops < 0 || nacc < 0) return rh_fail(RH_ERR_ARG, "%s: negative count", who);
  if (ngalois > BR_MAX_GALOIS) return rh_fail(RH_ERR_ARG, "%s: at most %d automorphism keys", who, BR_MAX_GALOIS);
  if ((nkeys && !rgsw) || (ngalois && (!galois || !galois_elements)) || (nops && !prog_ops) || !prog_offsets || !c0 || !c1)
    return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  BrGalois ge{};
  for (int e = 0; e < ngalois; ++e) {
    if ((galois_elements[e] & 1) == 0) return rh_fail(RH_ERR_ARG, "%s: the Galois element must be odd (slot %d)", who, e);
    ge.g[e] = (u32)(galois_elements[e] & (2 * (u64)r->N - 1));
  }
  {
    const size_t w = (size_t)nacc * r->N;
    if (rh_overlap({c0, w}, {c1, w})) return rh_fail(RH_ERR_ARG, "%s: the two components of the accumulators overlap", who);
  }
  if (!nacc) return RH_OK;
  (void)hipSetDevice(r->device);
  (void)hipGetLastError();
  switch (r->logN) {
    case 6: case 7: case 8: br_launch<1, true>(r, nacc, c0, c1, rgsw, nkeys, galois, ge, ngalois, prog_offsets, prog_ops, nops, pw2, digits); break;
    case 9:                 br_launch<2, true>(r, nacc, c0, c1, rgsw, nkeys, galois, ge, ngalois, prog_offsets, prog_ops, nops, pw2, digits); break;
    case 10:                br_launch<4, true>(r, nacc, c0, c1, rgsw, nkeys, galois, ge, ngalois, prog_offsets, prog_ops, nops, pw2, digits); break;
    default:                br_launch<8, false>(r, nacc, c0, c1, rgsw, nkeys, galois, ge, ngalois, prog_offsets, prog_ops, nops, pw2, digits); break;
  }
  return rh_launch_ok("blindrot_core_kernel");
}

// blindrot.hip -- rh_blindrot_core: the accumulator loops of a batch of blind rotations (core/rgsw/blindrot/evaluator.go:134-229) in one launch,
// one workgroup per accumulator (blindrot_kernels.hip.hpp).  The host derives each accumulator's program from its discrete-log sets
// (getDiscreteLogSets :258-280, evaluateFromDiscreteLogSets :189-229) and uploads it; the key tables are uploaded once per key set.
// rh_blindrot_mod_switch, rh_blindrot_program and rh_blindrot_monomials are the front end of Evaluate (:46-132) on the device: the programs are
// then derived there, in the same encoding, and neither a coefficient nor a program crosses to the host.
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

// ---- the front end of Evaluate (evaluator.go:46-132) on the device: no coefficient and no program crosses to the host ---------------------------
static int br_front_ring(const rh_ring* r, const char* who) {
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (r->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
  return RH_OK;
}
static int br_front_logn(int logN, const char* who) {
  if (logN < BR_MIN_LOGN || logN > BR_MAX_LOGN)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: blind rotation ring degree 2^%d outside 2^%d .. 2^%d", who, logN, BR_MIN_LOGN, BR_MAX_LOGN);
  return RH_OK;
}

extern "C" int rh_blindrot_mod_switch(rh_ring* rlwe, int logN_br, const uint64_t* x, int ncts, int32_t* a2n, const int32_t* jobs, int njobs, int32_t* b) {
  const char* who = "rh_blindrot_mod_switch";
  if (int rc = br_front_ring(rlwe, who)) return rc;
  if (int rc = br_front_logn(logN_br, who)) return rc;
  if (rlwe->moduli[0] >> 63) return rh_fail(RH_ERR_ARG, "%s: modulus 0 is not below 2^63", who);
  if (ncts < 0 || njobs < 0) return rh_fail(RH_ERR_ARG, "%s: negative count", who);
  if ((ncts && (!x || !a2n)) || (njobs && (!jobs || !b || !a2n))) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((size_t)ncts * 2 * rlwe->N >> 31) return rh_fail(RH_ERR_ARG, "%s: too many sample ciphertexts", who);
  (void)hipSetDevice(rlwe->device);
  (void)hipGetLastError();
  if (ncts) {
    const size_t total = (size_t)ncts * 2 * rlwe->N;
    blindrot_mod_switch_kernel<<<dim3((unsigned)((total + BRP_THREADS - 1) / BRP_THREADS)), BRP_THREADS, 0, rh_stream(rlwe)>>>(
        x, a2n, total, (u32)rlwe->N, rlwe->moduli[0], logN_br + 1);
    if (int rc = rh_launch_ok("blindrot_mod_switch_kernel")) return rc;
  }
  if (njobs) {
    blindrot_gather_b_kernel<<<dim3((unsigned)((njobs + BRP_THREADS - 1) / BRP_THREADS)), BRP_THREADS, 0, rh_stream(rlwe)>>>(a2n, ncts, rlwe->N, jobs, njobs, b);
    return rh_launch_ok("blindrot_gather_b_kernel");
  }
  return RH_OK;
}

// EXT ops: n_lwe.  AUTO ops: one before each non-empty set but the first of a run (at most min(n_lwe, N - 1)), one per full window ((N - 2) / 10 at
// most), the one of k == 1 and Automorphism(2N - g).
extern "C" int rh_blindrot_program_stride(int n_br, int n_lwe) {
  if (n_br < 2 || n_lwe < 0) return 0;
  return n_lwe + (n_lwe < n_br - 1 ? n_lwe : n_br - 1) + (n_br - 2) / BR_WINDOW + 3;
}

extern "C" int rh_blindrot_program(rh_ring* rbr, int n_lwe, const int32_t* a2n, int ncts, const int32_t* jobs, int njobs, const int32_t* dlog_pos,
                                   const int32_t* slots, int stride, int32_t* offsets, int32_t* ops, int32_t* flag) {
  const char* who = "rh_blindrot_program";
  if (int rc = br_front_ring(rbr, who)) return rc;
  if (int rc = br_front_logn(rbr->logN, who)) return rc;
  if (n_lwe < 1 || n_lwe > BRP_MAX_NLWE) return rh_fail(RH_ERR_UNSUPPORTED, "%s: LWE degree %d outside 1 .. %d, what one workgroup holds", who, n_lwe, BRP_MAX_NLWE);
  if (ncts < 0 || njobs < 0) return rh_fail(RH_ERR_ARG, "%s: negative count", who);
  if (stride < rh_blindrot_program_stride(rbr->N, n_lwe))
    return rh_fail(RH_ERR_ARG, "%s: stride %d below rh_blindrot_program_stride = %d", who, stride, rh_blindrot_program_stride(rbr->N, n_lwe));
  if (((size_t)njobs + 1) * (size_t)stride >> 31) return rh_fail(RH_ERR_ARG, "%s: %d jobs of stride %d do not fit int32 offsets", who, njobs, stride);
  if (!slots || !offsets || !flag || (njobs && (!a2n || !jobs || !dlog_pos || !ops))) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  BrSlots sl{};
  for (int v = 0; v <= BR_WINDOW; ++v) {
    if (slots[v] < 0 || slots[v] >= BR_MAX_GALOIS) return rh_fail(RH_ERR_ARG, "%s: key slot %d of Galois element %d outside 0 .. %d", who, slots[v], v, BR_MAX_GALOIS - 1);
    if (v < BR_WINDOW) sl.pw[v + 1] = -(slots[v] + 1); else sl.mid = -(slots[v] + 1);
  }
  (void)hipSetDevice(rbr->device);
  (void)hipGetLastError();
  if (!njobs) {
    if (hipMemsetAsync(offsets, 0, sizeof(int32_t), rh_stream(rbr)) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "%s: hipMemsetAsync failed", who);
    return RH_OK;
  }
  blindrot_program_kernel<<<dim3((unsigned)njobs), BRP_THREADS, 0, rh_stream(rbr)>>>(a2n, ncts, n_lwe, jobs, dlog_pos, sl, rbr->logN, stride, offsets, ops, flag);
  return rh_launch_ok("blindrot_program_kernel");
}

extern "C" int rh_blindrot_monomials(rh_ring* rbr, int level, const int32_t* b, int njobs, uint64_t* out) {
  const char* who = "rh_blindrot_monomials";
  if (int rc = br_front_ring(rbr, who)) return rc;
  if (level < 0 || level >= rbr->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range", who, level);
  if (njobs < 0) return rh_fail(RH_ERR_ARG, "%s: negative count", who);
  if (njobs && (!b || !out)) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (!njobs) return RH_OK;
  (void)hipSetDevice(rbr->device);
  (void)hipGetLastError();
  const size_t total = (size_t)njobs * (level + 1) * rbr->N;
  if ((total + BRP_THREADS - 1) / BRP_THREADS >> 31) return rh_fail(RH_ERR_ARG, "%s: too many jobs", who);
  blindrot_monomials_kernel<<<dim3((unsigned)((total + BRP_THREADS - 1) / BRP_THREADS)), BRP_THREADS, 0, rh_stream(rbr)>>>(b, out, total, level + 1, rbr->logN,
                                                                                                                       rbr->d_consts);
  return rh_launch_ok("blindrot_monomials_kernel");
}

// bootstrap.hip -- the two passes of CKKS bootstrapping that no other entry point covers (kernels: bootstrap_kernels.hip.hpp):
//   rh_ckks_bootstrap_modup  Evaluator.ModUp's lift from q0 to Q (and P), circuits/ckks/bootstrapping/evaluator.go:678-696, :703-722, :762-775,
//                            with the message scaling of :735-750 / :781-789 folded in; both components of a batch in ONE launch
//   rh_ckks_double_angle     Add(res, res, res) and Add(res, -sqrt2pi, res) of a double-angle round, circuits/ckks/mod1/mod1_evaluator.go:108-114
// Everything else of the circuit is the library's own (the key switch, the transforms, Trace, the DFT, the polynomial evaluator), driven from
// the host (bootstrapping.py, mod1.py).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "qp_rows_host.hpp"
#include "bootstrap_kernels.hip.hpp"

// residues of the message scalar per limb -> MForm, as MulScalar takes its scalar (ring/operations.go: MForm(BRedAdd(scalar)))
static int modup_scalars(const rh_ring* r, int L, const u64* in, u64* out, const char* who, const char* of) {
  for (int i = 0; i < L; ++i) {
    if (in[i] >= r->moduli[i]) return rh_fail(RH_ERR_ARG, "%s: scalar %d%s is not a residue of its limb", who, i, of);
    out[i] = rh::mform(in[i], r->moduli[i]);
  }
  return RH_OK;
}

extern "C" int rh_ckks_bootstrap_modup(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* in0, const uint64_t* in1, int in_rows,
                                       uint64_t* out0, uint64_t* out1, uint64_t* c1Q, uint64_t* c1P, int npoly, const uint64_t* scalarQ,
                                       const uint64_t* scalarP) {
  const char* who = "rh_ckks_bootstrap_modup";
  if (int rc = rh_ring_ok(rQ, levelQ, npoly, who, "npoly < 0")) return rc;
  const bool encap = rP != nullptr;
  if (encap) {
    if (rP->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
    if (rP->N != rQ->N || rP->device != rQ->device) return rh_fail(RH_ERR_ARG, "%s: ringQ and ringP differ in degree or device", who);
    if (levelP < 0 || levelP >= rP->L || levelP + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: levelP %d out of range [0,%d)", who, levelP, rP->L);
    if (!c1Q || !c1P || out1) return rh_fail(RH_ERR_ARG, "%s: with ringP component 1 goes to c1Q and c1P, and out1 must be NULL", who);
    if ((scalarQ == nullptr) != (scalarP == nullptr)) return rh_fail(RH_ERR_ARG, "%s: the scalar needs its residues modulo Q and modulo P, or neither", who);
  } else if (c1Q || c1P || scalarP || !out1) {
    return rh_fail(RH_ERR_ARG, "%s: without ringP component 1 goes to out1, and c1Q, c1P and scalarP must be NULL", who);
  }
  if (!in0 || !in1 || !out0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (in_rows < 1) return rh_fail(RH_ERR_ARG, "%s: in_rows < 1", who);
  const int LQ = levelQ + 1, LP = encap ? levelP + 1 : 0;
  const size_t N = (size_t)rQ->N, wq = (size_t)npoly * LQ * N, wp = (size_t)npoly * LP * N, wi = (size_t)npoly * (size_t)in_rows * N;
  if ((size_t)npoly * (size_t)(2 * LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  // the lift is out of place: a lane reads limb 0 of its input and writes every limb of its outputs
  const RhBlock rd[2] = {{in0, wi}, {in1, wi}};
  const RhBlock wr[3] = {{out0, wq}, {encap ? c1Q : out1, wq}, {c1P, wp}};
  const int nw = encap ? 3 : 2;
  if (int rc = rh_blocks_ok(wr, nw, rd, 2, who, "an output overlaps an input: the lift is not computed in place")) return rc;
  if (int rc = rh_blocks_disjoint(wr, nw, who, "two outputs overlap")) return rc;
  RhScalars s; memset(&s, 0, sizeof(s));
  if (scalarQ) if (int rc = modup_scalars(rQ, LQ, scalarQ, s.a, who, " of Q")) return rc;
  if (scalarP) if (int rc = modup_scalars(rP, LP, scalarP, s.b, who, " of P")) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)npoly * (unsigned)(2 * LQ + LP));   // cache policy by the bytes WRITTEN; the grid is this kernel's own
  unsigned chunks = ((unsigned)N / 2 + 255) / 256; if (chunks > 65535) chunks = 65535;      // one coefficient pair per lane
  const dim3 grid(2u * (unsigned)npoly, chunks);
  hipStream_t st = rh_stream(rQ);
  const ModUpArgs p{{in0, in1}, {out0, out1}, c1Q, c1P};
  const unsigned n = (unsigned)N;
  const LimbConsts* cP = encap ? rP->d_consts : rQ->d_consts;
#define BTS_MODUP(E, S) bootstrap_modup_kernel<E, S><<<grid, 256, 0, st>>>(p, n, in_rows, rQ->d_consts, cP, LQ, LP, npoly, s, g.nt)
  if (encap) { if (scalarQ) BTS_MODUP(true, true); else BTS_MODUP(true, false); }
  else { if (scalarQ) BTS_MODUP(false, true); else BTS_MODUP(false, false); }
#undef BTS_MODUP
  return rh_launch_ok("bootstrap_modup_kernel");
}

extern "C" int rh_ckks_double_angle(rh_ring* r, int level, uint64_t* c0, uint64_t* c1, int npoly, const uint64_t* s0, const uint64_t* s1) {
  const char* who = "rh_ckks_double_angle";
  if (int rc = rh_scheme_args(r, level, npoly, 1u << RH_RING_STANDARD | 1u << RH_RING_CI, 4, who)) return rc;
  if (!c0 || !c1 || !s0 || !s1) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const int L = level + 1;
  if ((size_t)npoly * 2 * (size_t)L > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  const size_t words = (size_t)npoly * L * (size_t)r->N;
  const RhBlock wr[2] = {{c0, words}, {c1, words}};
  if (((uintptr_t)c0 | (uintptr_t)c1) & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  if (int rc = rh_blocks_disjoint(wr, 2, who, "the two components overlap")) return rc;
  RhScalars s;                                                          // Add of a scalar (:82-101): the residues as they are
  if (int rc = rh_pack_scalars(r, level, s0, s1, false, &s, who)) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, 2u * (unsigned)npoly * (unsigned)L);
  ckks_double_angle_kernel<<<g.grid, 256, 0, rh_stream(r)>>>(c0, c1, (unsigned)r->N, r->d_consts, L, npoly, s, g.nt);
  return rh_launch_ok("ckks_double_angle_kernel");
}

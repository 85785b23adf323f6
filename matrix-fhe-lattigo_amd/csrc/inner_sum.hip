// inner_sum.hip -- sums of rotations (core/rlwe/inner_sum.go): PartialTracesSum (:152-291) as one C-ABI call, and the two kernels it is
// built on (inner_sum_kernels.hip.hpp): the NTT-domain automorphism of a hoisted gadget product fused with the addition that follows it,
// modulo QP for the lazily accumulated rotations and modulo Q for the doubling steps.
//
// Everything else of the sequence is the library's own: rh_bext_decompose_ntt, rh_bext_gadget_product_hoisted_lazy,
// rh_bext_gadget_product_hoisted_then_add, rh_bext_moddown_qp_to_q_ntt_pair.  Scratch: the extender's buffers 3, 4 (the decomposition), 6 (ctInNTT),
// 9 (the accumulator modulo QP) and 10 (the product modulo QP), sized by rh_bext_reserve.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "inner_sum_kernels.hip.hpp"
#include "qp_rows_host.hpp"

// AutomorphismHoistedLazy's tail (core/rlwe/evaluator_automorphism.go:107-160) + ringQP.Add (core/rlwe/inner_sum.go:245-246); see ringhip.h
extern "C" int rh_rlwe_rotate_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* ct0, const uint64_t* tmpQ0,
                                            const uint64_t* tmpQ1, const uint64_t* tmpP0, const uint64_t* tmpP1, uint64_t* accQ0, uint64_t* accQ1,
                                            uint64_t* accP0, uint64_t* accP1, int npoly, int first) {
  const char* who = "rotate_accumulate_qp";
  rh_ring *RQ = nullptr, *RP = nullptr; u32 g = 0;
  const uint64_t* tmp[4] = {tmpQ0, tmpQ1, tmpP0, tmpP1};
  uint64_t* acc[4] = {accQ0, accQ1, accP0, accP1};
  const QpExtra extra[1] = {{ct0, QP_BATCH_Q}};
  if (int rc = qp_accumulate_args(be, levelQ, levelP, gen, who, tmp, extra, 1, acc, npoly, "the accumulator cannot overlap the permuted operands", &RQ, &RP, &g)) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const int LQ = levelQ + 1, LP = levelP + 1;
  const RhPmodQ pq = is_pmodq(RQ, RP, LQ, LP);
  const RhStreamGrid sg = rh_stream_begin(RQ, 2u * (unsigned)npoly * (unsigned)(LQ + LP));
  const RhQP a{{accQ0, accQ1}, {accP0, accP1}};
  const RhQPc t{{tmpQ0, tmpQ1}, {tmpP0, tmpP1}};
  rotate_accumulate_qp_kernel<<<sg.grid, 256, 0, rh_stream(RQ)>>>(a, t, ct0, RQ->logN, g, RQ->d_consts, RP->d_consts, LQ, LP, npoly, pq, first ? 1 : 0, sg.nt);
  return rh_launch_ok("rotate_accumulate_qp_kernel");
}

// The AutomorphismNTT pair of AutomorphismHoisted (evaluator_automorphism.go:90-95) + ringQ.Add (inner_sum.go:279-280); see ringhip.h
extern "C" int rh_rlwe_rotate_add_q(rh_ring* r, int level, uint64_t gen, const uint64_t* tmp0, const uint64_t* tmp1, uint64_t* ct0, uint64_t* ct1,
                                    int npoly) {
  const char* who = "rotate_add_q";
  if (!r || !tmp0 || !tmp1 || !ct0 || !ct1) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (int rc = rh_ring_ok(r, level, npoly, who, "npoly < 0")) return rc;
  {
    const size_t w = (size_t)npoly * (level + 1) * r->N;
    const RhBlock wr[2] = {{ct0, w}, {ct1, w}}, rd[2] = {{tmp0, w}, {tmp1, w}};
    if (int rc = rh_blocks_ok(wr, 2, rd, 2, who, "the permuted operand cannot be the ciphertext it is added to")) return rc;
  }
  u32 g; if (int rc = is_gen(r, gen, who, &g)) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * (unsigned)npoly * (unsigned)(level + 1));
  rotate_add_q_kernel<<<sg.grid, 256, 0, rh_stream(r)>>>(ct0, ct1, tmp0, tmp1, r->logN, g, r->d_consts, level + 1, npoly, sg.nt);
  return rh_launch_ok("rotate_add_q_kernel");
}

// ---- PartialTracesSum -----------------------------------------------------------------------------------------------------------------
// Parameters.GaloisElement (core/rlwe/params.go:671-675): GaloisGen^k mod 2N, a negative k taken modulo 2N
static u64 galois_element(long k, u64 nthroot) {
  const long m = (long)nthroot;
  const u64 e = (u64)(((k % m) + m) % m);
  return rh::powmod(5, e, nthroot);
}
enum { IS_LAZY = 0, IS_CLOSE = 1, IS_DOUBLE = 2 };
struct IsStep { int kind; u64 gen; bool decompose; };
// The binary reading of n (:216-282) as a list of steps; `decompose`: the step is the first of its iteration that reads the decomposition
static std::vector<IsStep> is_plan(long offset, long n, u64 nthroot) {
  std::vector<IsStep> plan;
  bool state = false;
  int i = 0;
  for (long j = n; j > 0; ++i, j >>= 1) {
    bool fresh = true;
    if (j & 1) {
      const long k = (n - (n & ((2L << i) - 1))) * offset;
      if (k != 0) { plan.push_back({IS_LAZY, galois_element(k, nthroot), fresh}); fresh = false; }
      else { state = true; plan.push_back({IS_CLOSE, 0, false}); }
    }
    if (!state) plan.push_back({IS_DOUBLE, galois_element((1L << i) * offset, nthroot), fresh});
  }
  return plan;
}

extern "C" int rh_rlwe_partial_traces_sum(rh_bext* be, int levelQ, int levelP, const uint64_t* in0, const uint64_t* in1, int is_ntt, int offset,
                                          int n, const rh_galois_key* keys, int nkeys, uint64_t* out0, uint64_t* out1, int npoly, int fused) {
  const char* who = "partial_traces_sum";
  if (n <= 0 || offset == 0) return rh_fail(RH_ERR_ARG, "partialtrace: invalid parameter (n = 0 or batchSize = 0)");
  rh_ring *RQ, *RP;
  if (int rc = is_rings(be, levelQ, levelP, who, &RQ, &RP)) return rc;
  if (levelP < 1) return rh_fail(RH_ERR_UNSUPPORTED, "%s: keys with one P modulus are not supported by the hoisted product (levelP >= 1)", who);
  if (!in0 || !in1 || !out0 || !out1 || (nkeys > 0 && !keys) || nkeys < 0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((in0 == out0) != (in1 == out1) || in0 == out1 || in1 == out0) return rh_fail(RH_ERR_ARG, "%s: opOut is ctIn or another ciphertext", who);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  const int LQ = levelQ + 1, LP = levelP + 1, N = RQ->N;
  const int beta = (levelQ + levelP + 1) / (levelP + 1);
  const std::vector<IsStep> plan = n > 1 ? is_plan(offset, n, 2 * (u64)N) : std::vector<IsStep>();
  std::vector<const rh_galois_key*> key(plan.size(), nullptr);
  for (size_t s = 0; s < plan.size(); ++s) {          // every key before the first launch
    if (plan[s].kind == IS_CLOSE || (plan[s].kind == IS_DOUBLE && plan[s].gen == 1)) continue;
    for (int k = 0; k < nkeys && !key[s]; ++k) if (keys[k].galois_element == plan[s].gen) key[s] = &keys[k];
    if (!key[s]) return rh_fail(RH_ERR_ARG, "%s: GaloisKey[%llu] is missing", who, (unsigned long long)plan[s].gen);
    if (!key[s]->evkQ_dev || !key[s]->evkP_dev) return rh_fail(RH_ERR_ARG, "%s: GaloisKey[%llu] has a null part", who, (unsigned long long)plan[s].gen);
    if (key[s]->digits < beta) return rh_fail(RH_ERR_ARG, "%s: GaloisKey[%llu] has %d digits, level needs %d", who, (unsigned long long)plan[s].gen, key[s]->digits, beta);
  }
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  (void)hipSetDevice(RQ->device);
  const size_t wq = (size_t)npoly * LQ * N, wp = (size_t)npoly * LP * N;
  u64 *decQ, *decP, *ct, *acc, *c;
  if (int rc = rh_bext_scratch(be, 3, (size_t)beta * wq, &decQ)) return rc;
  if (int rc = rh_bext_scratch(be, 4, (size_t)beta * wp, &decP)) return rc;
  if (int rc = rh_bext_scratch(be, 6, 2 * wq, &ct)) return rc;
  if (int rc = rh_bext_scratch(be, 9, 2 * (wq + wp), &acc)) return rc;
  if (int rc = rh_bext_scratch(be, 10, 2 * (wq + wp), &c)) return rc;
  u64 *rQ = nullptr, *rP = nullptr;                   // composed form: the rotated product, in the ModDown buffers (idle while it is needed)
  if (!fused) { if (int rc = rh_bext_scratch(be, 0, 2 * wq, &rQ)) return rc; if (int rc = rh_bext_scratch(be, 1, 2 * wp, &rP)) return rc; }
  const RhPmodQ pq = is_pmodq(RQ, RP, LQ, LP);
  u64 *ct0 = ct, *ct1 = ct + wq;
  u64 *aQ0 = acc, *aQ1 = acc + wq, *aP0 = acc + 2 * wq, *aP1 = aP0 + wp;      // the P parts back to back: ModDown takes them as one batch
  u64 *cQ0 = c, *cQ1 = c + wq, *cP0 = c + 2 * wq, *cP1 = cP0 + wp;
  hipStream_t st = rh_stream(RQ);
  auto copy = [&](u64* dst, const u64* src) {
    return hipMemcpyAsync(dst, src, wq * 8, hipMemcpyDeviceToDevice, st) == hipSuccess ? RH_OK : rh_fail(RH_ERR_DEVICE, "%s: copy failed", who);
  };
  // ctInNTT (:169-186)
  if (is_ntt) { if (int rc = copy(ct0, in0)) return rc; if (int rc = copy(ct1, in1)) return rc; }
  else { if (int rc = rh_ring_ntt_any(RQ, in0, ct0, npoly, LQ, 0, false)) return rc; if (int rc = rh_ring_ntt_any(RQ, in1, ct1, npoly, LQ, 0, false)) return rc; }
  if (n == 1) {                                         // (:188-192)
    if (in0 != out0) { if (int rc = copy(out0, in0)) return rc; if (int rc = copy(out1, in1)) return rc; }
  }
  bool first = true;
  for (size_t s = 0; s < plan.size(); ++s) {
    const IsStep& p = plan[s];
    if (p.decompose) if (int rc = rh_bext_decompose_ntt(be, levelQ, levelP, ct1, 1, decQ, decP, npoly)) return rc;      // (:222)
    if (p.kind == IS_LAZY) {                            // accQP (+)= AutomorphismHoistedLazy(ctInNTT) (:236-247)
      if (int rc = rh_bext_gadget_product_hoisted_lazy(be, levelQ, levelP, decQ, decP, key[s]->evkQ_dev, key[s]->evkP_dev, key[s]->digits, cQ0, cQ1, cP0, cP1, npoly)) return rc;
      if (fused) {
        if (int rc = rh_rlwe_rotate_accumulate_qp(be, levelQ, levelP, p.gen, ct0, cQ0, cQ1, cP0, cP1, aQ0, aQ1, aP0, aP1, npoly, first ? 1 : 0)) return rc;
      } else {
        // the reference's own passes: + P ctIn[0], four automorphisms, four additions
        if (int rc = rh_ring_vec_op(RQ, RH_OP_MUL_SCALAR_MONT_THEN_ADD, ct0, nullptr, cQ0, npoly, levelQ, pq.s, nullptr)) return rc;
        u64* dQ = first ? aQ0 : rQ; u64* dP = first ? aP0 : rP;
        if (int rc = rh_ring_automorphism_ntt(RQ, levelQ, cQ0, p.gen, dQ, 2 * npoly, 0)) return rc;      // cQ0, cQ1 and cP0, cP1 lie back to back
        if (int rc = rh_ring_automorphism_ntt(RP, levelP, cP0, p.gen, dP, 2 * npoly, 0)) return rc;
        if (!first) {
          if (int rc = rh_ring_vec_op(RQ, RH_OP_ADD, aQ0, rQ, aQ0, 2 * npoly, levelQ, nullptr, nullptr)) return rc;
          if (int rc = rh_ring_vec_op(RP, RH_OP_ADD, aP0, rP, aP0, 2 * npoly, levelP, nullptr, nullptr)) return rc;
        }
      }
      first = false;
    } else if (p.kind == IS_CLOSE) {                    // (:252-267)
      if (n & (n - 1)) {
        if (int rc = rh_bext_moddown_qp_to_q_ntt_pair(be, levelQ, levelP, aQ0, aQ1, aP0, aP1, out0, out1, npoly)) return rc;
        if (int rc = rh_ring_vec_op(RQ, RH_OP_ADD, out0, ct0, out0, npoly, levelQ, nullptr, nullptr)) return rc;
        if (int rc = rh_ring_vec_op(RQ, RH_OP_ADD, out1, ct1, out1, npoly, levelQ, nullptr, nullptr)) return rc;
      } else { if (int rc = copy(out0, ct0)) return rc; if (int rc = copy(out1, ct1)) return rc; }
    } else if (p.gen == 1) {                            // AutomorphismHoisted of the identity copies (:68-73): ctInNTT is doubled
      if (int rc = rh_ring_vec_op(RQ, RH_OP_ADD, ct0, ct0, ct0, 2 * npoly, levelQ, nullptr, nullptr)) return rc;
    } else {                                            // ctInNTT += AutomorphismHoisted(ctInNTT) (:276-280)
      if (int rc = rh_bext_gadget_product_hoisted_then_add(be, levelQ, levelP, decQ, decP, key[s]->evkQ_dev, key[s]->evkP_dev, key[s]->digits, ct0, nullptr, cQ0, cQ1, npoly)) return rc;
      if (fused) { if (int rc = rh_rlwe_rotate_add_q(RQ, levelQ, p.gen, cQ0, cQ1, ct0, ct1, npoly)) return rc; }
      else {
        if (int rc = rh_ring_automorphism_ntt(RQ, levelQ, cQ0, p.gen, rQ, 2 * npoly, 0)) return rc;
        if (int rc = rh_ring_vec_op(RQ, RH_OP_ADD, ct0, rQ, ct0, 2 * npoly, levelQ, nullptr, nullptr)) return rc;
      }
    }
  }
  if (!is_ntt) {                                        // (:285-288), n == 1 included
    if (int rc = rh_ring_ntt_any(RQ, out0, out0, npoly, LQ, 0, true)) return rc;
    if (int rc = rh_ring_ntt_any(RQ, out1, out1, npoly, LQ, 0, true)) return rc;
  }
  return RH_OK;
}

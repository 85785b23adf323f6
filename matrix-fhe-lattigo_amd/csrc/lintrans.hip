// lintrans.hip -- the three streaming passes of the diagonal matrix x ciphertext product (circuits/common/lintrans/lintrans_evaluator.go) as
// C-ABI calls over the kernels of lintrans_kernels.hip.hpp:
//   rh_rlwe_diag_mac_qp               the inner loop of MultiplyByDiagMatrixBSGS for one giant step (:311-357)
//   rh_rlwe_rotate_sum_accumulate_qp  its giant-step tail (:384-393)
//   rh_rlwe_rotate_mul_accumulate_qp  one diagonal of MultiplyByDiagMatrix (:200-218)
// Everything else of the two circuits is the library's own (rh_bext_decompose_ntt, rh_bext_gadget_product_hoisted_lazy, the lazy gadget product,
// rh_bext_moddown_qp_to_q_ntt_pair); the circuits themselves are driven from the host (lintrans.py).
#include <hip/hip_runtime.h>
#include "engine_internal.hpp"
#include "lintrans_kernels.hip.hpp"
#include "qp_rows_host.hpp"

extern "C" size_t rh_rlwe_diag_mac_qp_table_words(int nterms, int levelQ, int levelP) {
  return nterms < 0 || levelQ < 0 || levelP < 0 ? 0 : (size_t)nterms * LT_TERM_WORDS;
}

// The inner loop of MultiplyByDiagMatrixBSGS for one giant step (lintrans_evaluator.go:311-357); see ringhip.h
extern "C" int rh_rlwe_diag_mac_qp(rh_bext* be, int levelQ, int levelP, int nterms, const uint64_t* const* ptQ, const uint64_t* const* ptP,
                                   const uint64_t* const* x, uint64_t* tmpQ0, uint64_t* tmpQ1, uint64_t* tmpP0, uint64_t* tmpP1, int npoly,
                                   uint64_t* table, size_t table_words) {
  const char* who = "rh_rlwe_diag_mac_qp";
  rh_ring *RQ, *RP;
  if (int rc = is_rings(be, levelQ, levelP, who, &RQ, &RP)) return rc;
  if (nterms < 0) return rh_fail(RH_ERR_ARG, "%s: nterms < 0", who);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  if (!tmpQ0 || !tmpQ1 || !tmpP0 || !tmpP1 || (nterms && (!ptQ || !ptP || !x))) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (nterms && !table) return rh_fail(RH_ERR_ARG, "%s: null table (device scratch of rh_rlwe_diag_mac_qp_table_words(nterms, levelQ, levelP) words)", who);
  const int LQ = levelQ + 1, LP = levelP + 1;
  const size_t N = (size_t)RQ->N, words = (size_t)nterms * LT_TERM_WORDS;
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the table holds %zu words, %d terms need %zu", who, table_words, nterms, words);
  if (int rc = rh_moduli_below(RQ, LQ, LC_MODULUS_BITS, LC_CHUNK, who, " of Q")) return rc;
  if (int rc = rh_moduli_below(RP, LP, LC_MODULUS_BITS, LC_CHUNK, who, " of P")) return rc;
  const size_t wq = (size_t)npoly * LQ * N, wp = (size_t)npoly * LP * N;
  const RhBlock written[5] = {{tmpQ0, wq}, {tmpQ1, wq}, {tmpP0, wp}, {tmpP1, wp}, {table, words}};
  const int nw = nterms ? 5 : 4;
  for (int k = 0; k < nterms; ++k) {
    const uint64_t* const* xk = x + 4 * (size_t)k;
    if (!ptQ[k] || !ptP[k]) return rh_fail(RH_ERR_ARG, "%s: term %d has no diagonal", who, k);
    if (!xk[0] || !xk[1] || (xk[2] == nullptr) != (xk[3] == nullptr)) return rh_fail(RH_ERR_ARG, "%s: term %d needs both components modulo Q, and modulo P both or neither", who, k);
    const RhBlock read[6] = {{ptQ[k], LQ * N}, {ptP[k], LP * N}, {xk[0], wq}, {xk[1], wq}, {xk[2] ? xk[2] : xk[0], xk[2] ? wp : wq}, {xk[3] ? xk[3] : xk[1], xk[3] ? wp : wq}};
    if (int rc = rh_blocks_ok(written, nw, read, 6, who, "an output (or the table) overlaps a term: the sum is not computed in place")) return rc;
  }
  if (nterms) if (int rc = rh_blocks_ok(written, 4, written + 4, 1, who, "an output overlaps the table")) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const RhStreamGrid sg = rh_stream_begin(RQ, (unsigned)npoly * (unsigned)(LQ + LP));
  hipStream_t st = rh_stream(RQ);
  if (nterms) {
    RhStage* stage;
    if (int rc = rh_stage_slot(words, &stage, who)) return rc;
    for (int k = 0; k < nterms; ++k) {
      u64* e = stage->h + (size_t)k * LT_TERM_WORDS;
      e[0] = (u64)(uintptr_t)ptQ[k]; e[1] = (u64)(uintptr_t)ptP[k];
      for (int j = 0; j < 4; ++j) e[2 + j] = (u64)(uintptr_t)x[4 * (size_t)k + j];
    }
    if (int rc = rh_stage_upload(stage, table, words, st, who)) return rc;
  }
  const RhQP out{{tmpQ0, tmpQ1}, {tmpP0, tmpP1}};
  diag_mac_qp_kernel<<<sg.grid, 256, 0, st>>>(out, table, nterms, RQ->logN, RQ->d_consts, RP->d_consts, LQ, LP, sg.nt);
  return rh_launch_ok("diag_mac_qp_kernel");
}

// The giant-step tail of MultiplyByDiagMatrixBSGS (lintrans_evaluator.go:384-393); see ringhip.h
extern "C" int rh_rlwe_rotate_sum_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* cQ0, const uint64_t* cQ1,
                                                const uint64_t* cP0, const uint64_t* cP1, const uint64_t* tmpQ0, const uint64_t* tmpP0,
                                                uint64_t* accQ0, uint64_t* accQ1, uint64_t* accP0, uint64_t* accP1, int npoly, int first) {
  const char* who = "rh_rlwe_rotate_sum_accumulate_qp";
  rh_ring *RQ = nullptr, *RP = nullptr; u32 g = 0;
  const uint64_t* cqp[4] = {cQ0, cQ1, cP0, cP1};
  uint64_t* acc[4] = {accQ0, accQ1, accP0, accP1};
  const QpExtra extra[2] = {{tmpQ0, QP_BATCH_Q}, {tmpP0, QP_BATCH_P}};
  if (int rc = qp_accumulate_args(be, levelQ, levelP, gen, who, cqp, extra, 2, acc, npoly, "the accumulator cannot overlap cQP or tmp0, which are permuted", &RQ, &RP, &g)) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const int LQ = levelQ + 1, LP = levelP + 1;
  const RhStreamGrid sg = rh_stream_begin(RQ, 2u * (unsigned)npoly * (unsigned)(LQ + LP));
  const RhQP a{{accQ0, accQ1}, {accP0, accP1}};
  const RhQPc c{{cQ0, cQ1}, {cP0, cP1}};
  rotate_sum_accumulate_qp_kernel<<<sg.grid, 256, 0, rh_stream(RQ)>>>(a, c, tmpQ0, tmpP0, RQ->logN, g, RQ->d_consts, RP->d_consts, LQ, LP, npoly, first ? 1 : 0, sg.nt);
  return rh_launch_ok("rotate_sum_accumulate_qp_kernel");
}

// One diagonal of MultiplyByDiagMatrix (lintrans_evaluator.go:200-218); see ringhip.h
extern "C" int rh_rlwe_rotate_mul_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* ptQ, const uint64_t* ptP,
                                                const uint64_t* ct0, const uint64_t* cQ0, const uint64_t* cQ1, const uint64_t* cP0,
                                                const uint64_t* cP1, uint64_t* accQ0, uint64_t* accQ1, uint64_t* accP0, uint64_t* accP1, int npoly,
                                                int first) {
  const char* who = "rh_rlwe_rotate_mul_accumulate_qp";
  rh_ring *RQ = nullptr, *RP = nullptr; u32 g = 0;
  const uint64_t* cqp[4] = {cQ0, cQ1, cP0, cP1};
  uint64_t* acc[4] = {accQ0, accQ1, accP0, accP1};
  const QpExtra extra[3] = {{ct0, QP_BATCH_Q}, {ptQ, QP_ROW_Q}, {ptP, QP_ROW_P}};
  if (int rc = qp_accumulate_args(be, levelQ, levelP, gen, who, cqp, extra, 3, acc, npoly, "the accumulator cannot overlap cQP, ct0 or the diagonal", &RQ, &RP, &g)) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const int LQ = levelQ + 1, LP = levelP + 1;
  const RhPmodQ pq = is_pmodq(RQ, RP, LQ, LP);
  const RhStreamGrid sg = rh_stream_begin(RQ, 2u * (unsigned)npoly * (unsigned)(LQ + LP));
  const RhQP a{{accQ0, accQ1}, {accP0, accP1}};
  const RhQPc c{{cQ0, cQ1}, {cP0, cP1}};
  rotate_mul_accumulate_qp_kernel<<<sg.grid, 256, 0, rh_stream(RQ)>>>(a, c, ct0, ptQ, ptP, RQ->logN, g, RQ->d_consts, RP->d_consts, LQ, LP, npoly, pq, first ? 1 : 0, sg.nt);
  return rh_launch_ok("rotate_mul_accumulate_qp_kernel");
}

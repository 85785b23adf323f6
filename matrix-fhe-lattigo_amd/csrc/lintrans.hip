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

// Page-locked staging of the term table on its way to the device: a few slots per calling thread, each reused once the copy that read it has
// run (its event).  Nothing of a call lives in the handle; the slots stay with their thread.
struct LtStage { u64* h = nullptr; size_t words = 0; hipEvent_t done = nullptr; };
static int lt_stage(size_t words, LtStage** out, const char* who) {
  static thread_local LtStage slots[4];
  static thread_local unsigned next = 0;
  LtStage& s = slots[next++ % 4];
  if (s.done && hipEventSynchronize(s.done) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "%s: waiting for an earlier table copy failed", who);
  if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "%s: hipEventCreate failed", who);
  if (s.words < words) {
    if (s.h) (void)hipHostFree(s.h);
    s.h = nullptr; s.words = 0;
    if (hipHostMalloc((void**)&s.h, words * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return rh_fail(RH_ERR_NOMEM, "%s: hipHostMalloc(%zu words) failed", who, words); }
    s.words = words;
  }
  *out = &s;
  return RH_OK;
}

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
  for (int i = 0; i < LQ; ++i)
    if (RQ->moduli[i] >> LC_MODULUS_BITS) return rh_fail(RH_ERR_ARG, "%s: modulus %d of Q is not below 2^%d, the bound the %d-term chunks are sized for", who, i, LC_MODULUS_BITS, LC_CHUNK);
  for (int i = 0; i < LP; ++i)
    if (RP->moduli[i] >> LC_MODULUS_BITS) return rh_fail(RH_ERR_ARG, "%s: modulus %d of P is not below 2^%d, the bound the %d-term chunks are sized for", who, i, LC_MODULUS_BITS, LC_CHUNK);
  const size_t wq = (size_t)npoly * LQ * N, wp = (size_t)npoly * LP * N;
  const IsBlock written[5] = {{tmpQ0, wq}, {tmpQ1, wq}, {tmpP0, wp}, {tmpP1, wp}, {table, words}};
  const int nw = nterms ? 5 : 4;
  for (int k = 0; k < nterms; ++k) {
    const uint64_t* const* xk = x + 4 * (size_t)k;
    if (!ptQ[k] || !ptP[k]) return rh_fail(RH_ERR_ARG, "%s: term %d has no diagonal", who, k);
    if (!xk[0] || !xk[1] || (xk[2] == nullptr) != (xk[3] == nullptr)) return rh_fail(RH_ERR_ARG, "%s: term %d needs both components modulo Q, and modulo P both or neither", who, k);
    const IsBlock read[6] = {{ptQ[k], LQ * N}, {ptP[k], LP * N}, {xk[0], wq}, {xk[1], wq}, {xk[2] ? xk[2] : xk[0], xk[2] ? wp : wq}, {xk[3] ? xk[3] : xk[1], xk[3] ? wp : wq}};
    if (int rc = is_blocks(written, nw, read, 6, who, "an output (or the table) overlaps a term: the sum is not computed in place")) return rc;
  }
  if (nterms) if (int rc = is_blocks(written, 4, written + 4, 1, who, "an output overlaps the table")) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const RhStreamGrid sg = rh_stream_begin(RQ, (unsigned)npoly * (unsigned)(LQ + LP));
  hipStream_t st = rh_stream(RQ);
  if (nterms) {
    LtStage* stage;
    if (int rc = lt_stage(words, &stage, who)) return rc;
    for (int k = 0; k < nterms; ++k) {
      u64* e = stage->h + (size_t)k * LT_TERM_WORDS;
      e[0] = (u64)(uintptr_t)ptQ[k]; e[1] = (u64)(uintptr_t)ptP[k];
      for (int j = 0; j < 4; ++j) e[2 + j] = (u64)(uintptr_t)x[4 * (size_t)k + j];
    }
    if (hipMemcpyAsync(table, stage->h, words * 8, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(stage->done, st) != hipSuccess)
      return rh_fail(RH_ERR_DEVICE, "%s: table copy failed", who);
  }
  const LtQP out{{tmpQ0, tmpQ1}, {tmpP0, tmpP1}};
  diag_mac_qp_kernel<<<sg.grid, 256, 0, st>>>(out, table, nterms, RQ->logN, RQ->d_consts, RP->d_consts, LQ, LP, sg.nt);
  return rh_launch_ok("diag_mac_qp_kernel");
}

// The blocks of the two rotate calls: the accumulator may overlap nothing that is gathered
static int lt_rotate_args(rh_bext* be, int levelQ, int levelP, uint64_t gen, const char* who, const uint64_t* const* cqp, const IsBlock* extra,
                          int nextra, uint64_t* const* acc, int npoly, const char* text, rh_ring** RQ, rh_ring** RP, u32* g) {
  if (int rc = is_rings(be, levelQ, levelP, who, RQ, RP)) return rc;
  for (int j = 0; j < 4; ++j) if (!cqp[j] || !acc[j]) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  for (int j = 0; j < nextra; ++j) if (!extra[j].p) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  const size_t N = (size_t)(*RQ)->N, wq = (size_t)npoly * (levelQ + 1) * N, wp = (size_t)npoly * (levelP + 1) * N;
  const IsBlock wr[4] = {{acc[0], wq}, {acc[1], wq}, {acc[2], wp}, {acc[3], wp}};
  IsBlock rd[8] = {{cqp[0], wq}, {cqp[1], wq}, {cqp[2], wp}, {cqp[3], wp}};
  for (int j = 0; j < nextra; ++j) rd[4 + j] = extra[j];
  if (int rc = is_blocks(wr, 4, rd, 4 + nextra, who, text)) return rc;
  return is_gen(*RQ, gen, who, g);
}

// The giant-step tail of MultiplyByDiagMatrixBSGS (lintrans_evaluator.go:384-393); see ringhip.h
extern "C" int rh_rlwe_rotate_sum_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* cQ0, const uint64_t* cQ1,
                                                const uint64_t* cP0, const uint64_t* cP1, const uint64_t* tmpQ0, const uint64_t* tmpP0,
                                                uint64_t* accQ0, uint64_t* accQ1, uint64_t* accP0, uint64_t* accP1, int npoly, int first) {
  const char* who = "rh_rlwe_rotate_sum_accumulate_qp";
  rh_ring *RQ = nullptr, *RP = nullptr; u32 g = 0;
  const uint64_t* cqp[4] = {cQ0, cQ1, cP0, cP1};
  uint64_t* acc[4] = {accQ0, accQ1, accP0, accP1};
  size_t wq = 0, wp = 0;
  if (be && npoly > 0 && levelQ >= 0 && levelP >= 0) { const size_t N = (size_t)rh_bext_ringQ(be)->N; wq = (size_t)npoly * (levelQ + 1) * N; wp = (size_t)npoly * (levelP + 1) * N; }
  const IsBlock extra[2] = {{tmpQ0, wq}, {tmpP0, wp}};
  if (int rc = lt_rotate_args(be, levelQ, levelP, gen, who, cqp, extra, 2, acc, npoly, "the accumulator cannot overlap cQP or tmp0, which are permuted", &RQ, &RP, &g)) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const int LQ = levelQ + 1, LP = levelP + 1;
  const RhStreamGrid sg = rh_stream_begin(RQ, 2u * (unsigned)npoly * (unsigned)(LQ + LP));
  const LtQP a{{accQ0, accQ1}, {accP0, accP1}};
  const LtQPc c{{cQ0, cQ1}, {cP0, cP1}};
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
  size_t wq = 0, N = 0;
  if (be && npoly > 0 && levelQ >= 0 && levelP >= 0) { N = (size_t)rh_bext_ringQ(be)->N; wq = (size_t)npoly * (levelQ + 1) * N; }
  const IsBlock extra[3] = {{ct0, wq}, {ptQ, levelQ >= 0 ? (size_t)(levelQ + 1) * N : 0}, {ptP, levelP >= 0 ? (size_t)(levelP + 1) * N : 0}};
  if (int rc = lt_rotate_args(be, levelQ, levelP, gen, who, cqp, extra, 3, acc, npoly, "the accumulator cannot overlap cQP, ct0 or the diagonal", &RQ, &RP, &g)) return rc;
  if (!npoly) return RH_OK;
  RhBextGuard guard(be);
  const int LQ = levelQ + 1, LP = levelP + 1;
  const RhPmodQ pq = is_pmodq(RQ, RP, LQ, LP);
  const RhStreamGrid sg = rh_stream_begin(RQ, 2u * (unsigned)npoly * (unsigned)(LQ + LP));
  const LtQP a{{accQ0, accQ1}, {accP0, accP1}};
  const LtQPc c{{cQ0, cQ1}, {cP0, cP1}};
  rotate_mul_accumulate_qp_kernel<<<sg.grid, 256, 0, rh_stream(RQ)>>>(a, c, ct0, ptQ, ptP, RQ->logN, g, RQ->d_consts, RP->d_consts, LQ, LP, npoly, pq, first ? 1 : 0, sg.nt);
  return rh_launch_ok("rotate_mul_accumulate_qp_kernel");
}

// lintrans_kernels.hip.hpp -- the three streaming passes of circuits/common/lintrans/lintrans_evaluator.go (diagonal matrix x ciphertext), on
// the scaffold of stream_kernels.hip.hpp: one (poly, limb) row per blockIdx.x, the row's coefficient pairs over blockIdx.y, 16-byte moves, the
// runtime `nt`.  Each launch covers the LQ rows of Q and the LP rows of P of BOTH ciphertext components, as rotate_accumulate_qp_kernel does
// (inner_sum_kernels.hip.hpp).  A diagonal is ONE PolyQP shared by every ciphertext of the batch: row l of its Q part and row l of its P part are
// read for every poly.
//
// Output values.  The reference accumulates lazily (MulCoeffsMontgomeryLazy(ThenAddLazy), AddLazy, AutomorphismNTTWithIndexThenAddLazy, reduced
// every QiOverF / PiOverF steps), but every sum ends in Reduce before anything reads it: the inner sums at lintrans_evaluator.go:349-357, the
// outer ones at :419-427, MultiplyByDiagMatrix's at :220-239.  So what the rest of the circuit sees is the canonical residue in [0, q) of the
// exact sum, whatever the schedule of those reductions, and that is what these kernels write.
#pragma once
#include "paired_gather.hip.hpp"
#include "lc_reduce.hip.hpp"

// The device table of rh_rlwe_diag_mac_qp: per term { ptQ, ptP, xQ0, xQ1, xP0, xP1 } as device addresses; xP0 = xP1 = 0 marks the baby step 0
// term, which lives modulo Q only.
#define LT_TERM_WORDS 6

// The inner loop of MultiplyByDiagMatrixBSGS for one giant step (:311-357):
//   tmp_c[j] = (sum_k pt_k[j] * x_{k,c}[j]) * 2^-64 mod q      c = 0, 1, canonical (:349-357)
// A term is a pre-rotated ciphertext modulo QP (:327-333), or the pair (P ct0, P ct1) modulo Q (:316-325), which adds nothing on the P rows; P rows
// without any other term are written as zero (:320-321).  Each pt_k word is loaded once for both components.  The products are summed in 128
// bits and reduced once per LC_CHUNK terms (lc_reduce.hip.hpp: operands below q < 2^61), LC_WIDTH terms' loads in flight together.
// grid: (npoly * (LQ + LP), chunks): StreamRowQP, one component.  The term loops run on table words alone: wave-uniform.
__global__ void __launch_bounds__(256)
diag_mac_qp_kernel(RhQP out, const u64* __restrict__ table, int nterms, int logN, const LimbConsts* __restrict__ constsQ,
                   const LimbConsts* __restrict__ constsP, int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, logN);
  u64* o0 = r.of(out, 0);
  u64* o1 = r.of(out, 1);
  const int sel = r.inQ ? 0 : 1;                                                        // table words of this row's kind: pt at sel, x at 2 + 2 sel
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const size_t w = 2 * (size_t)i;
    ulonglong2 res0 = make_ulonglong2(0, 0), res1 = make_ulonglong2(0, 0);
    for (int k0 = 0; k0 < nterms; k0 += LC_CHUNK) {
      const int k1 = min(k0 + LC_CHUNK, nterms);
      u128 a0x = 0, a0y = 0, a1x = 0, a1y = 0;
      for (int k = k0; k < k1; k += LC_WIDTH) {
        ulonglong2 pt[LC_WIDTH], x0[LC_WIDTH], x1[LC_WIDTH];
#pragma unroll
        for (int g = 0; g < LC_WIDTH; ++g) {
          pt[g] = x0[g] = x1[g] = make_ulonglong2(0, 0);
          if (k + g >= k1) break;
          const u64* t = table + (size_t)(k + g) * LT_TERM_WORDS;
          const u64 ax0 = t[2 + 2 * sel], ax1 = t[3 + 2 * sel];
          if (!ax0) continue;                                                           // the Q-only term on a P row
          pt[g] = *reinterpret_cast<const ulonglong2*>(lc_block(t[sel]) + r.po + w);       // shared by every poly: default cache policy
          x0[g] = rh_ld2(lc_block(ax0) + r.ro + w, nt);
          x1[g] = rh_ld2(lc_block(ax1) + r.ro + w, nt);
        }
#pragma unroll
        for (int g = 0; g < LC_WIDTH; ++g) {
          if (k + g >= k1) break;
          a0x += (u128)pt[g].x * x0[g].x; a0y += (u128)pt[g].y * x0[g].y;
          a1x += (u128)pt[g].x * x1[g].x; a1y += (u128)pt[g].y * x1[g].y;
        }
      }
      res0.x = cred(res0.x + lc_reduce(a0x, r.c), r.c.q); res0.y = cred(res0.y + lc_reduce(a0y, r.c), r.c.q);
      res1.x = cred(res1.x + lc_reduce(a1x, r.c), r.c.q); res1.y = cred(res1.y + lc_reduce(a1y, r.c), r.c.q);
    }
    rh_st2(o0 + w, res0, nt);
    rh_st2(o1 + w, res1, nt);
  }
}

// The giant-step tail of MultiplyByDiagMatrixBSGS (:384-393): ringQP.Add(cQP[0], tmp0QP, cQP[0]) and the two AutomorphismNTTWithIndex
// (ThenAddLazy) passes modulo QP, the sum canonical (:406-427):
//   acc_c[j] = [first ? 0 : acc_c[j]] + (c_c + [c == 0] tmp0)[index(j)]      on the Q and the P rows
// grid of both rotate kernels: (2 * npoly * (LQ + LP), chunks): StreamComp, then StreamRowQP, as rotate_accumulate_qp_kernel
__global__ void __launch_bounds__(256)
rotate_sum_accumulate_qp_kernel(RhQP acc, RhQPc cqp, const u64* tmpQ0, const u64* tmpP0, int logN, u32 gen, const LimbConsts* __restrict__ constsQ,
                                const LimbConsts* __restrict__ constsP, int LQ, int LP, int npoly, int first, int nt) {
  const StreamComp sc((u32)npoly * (u32)(LQ + LP));
  const StreamRowQP r(sc.row, constsQ, constsP, LQ, LP, logN);
  u64* a = r.of(acc, sc.comp);
  const u64* x = r.of(cqp, sc.comp);
  const u64* t0 = (r.inQ ? tmpQ0 : tmpP0) + r.ro;                                        // read only by component 0
  const u64 q = r.c.q;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const u32 idx = rh_galois_index_even(i, logN, gen);
    ulonglong2 t = rh_gather2(x, idx);
    if (sc.comp == 0) { const ulonglong2 u = rh_gather2(t0, idx); t.x = cred(t.x + u.x, q); t.y = cred(t.y + u.y, q); }
    rh_accumulate2(a, i, t, q, first, nt);
  }
}

// One diagonal of MultiplyByDiagMatrix (:200-218): ringQ.Add(cQP[0].Q, ct0TimesP), the two AutomorphismNTTWithIndex passes modulo QP and
// MulCoeffsMontgomery(ThenAdd) by the diagonal, the sum canonical (:220-239):
//   acc_c[j] = [first ? 0 : acc_c[j]] + pt[j] * (c_c + [c == 0, Q rows] MForm(P mod q_i) * ct0)[index(j)] * 2^-64
__global__ void __launch_bounds__(256)
rotate_mul_accumulate_qp_kernel(RhQP acc, RhQPc cqp, const u64* ct0, const u64* ptQ, const u64* ptP, int logN, u32 gen,
                                const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP, int LQ, int LP, int npoly, RhPmodQ pq,
                                int first, int nt) {
  const StreamComp sc((u32)npoly * (u32)(LQ + LP));
  const StreamRowQP r(sc.row, constsQ, constsP, LQ, LP, logN);
  u64* a = r.of(acc, sc.comp);
  const u64* x = r.of(cqp, sc.comp);
  const u64* pt = (r.inQ ? ptQ : ptP) + r.po;
  const bool with_ct0 = r.inQ && sc.comp == 0;
  const u64* c0 = ct0 + r.ro;                                                            // read only when with_ct0
  const u64 s = r.inQ ? pq.s[r.l] : 0;
  const u64 q = r.c.q, qinv = r.c.qinv;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const u32 idx = rh_galois_index_even(i, logN, gen);
    ulonglong2 t = rh_gather2(x, idx);
    if (with_ct0) {
      const ulonglong2 u = rh_gather2(c0, idx);
      t.x = cred(t.x + mred(u.x, s, q, qinv), q); t.y = cred(t.y + mred(u.y, s, q, qinv), q);
    }
    const ulonglong2 d = *reinterpret_cast<const ulonglong2*>(pt + 2 * (size_t)i);      // shared by every poly: default cache policy
    rh_accumulate2(a, i, make_ulonglong2(mred(d.x, t.x, q, qinv), mred(d.y, t.y, q, qinv)), q, first, nt);
  }
}

// inner_sum_kernels.hip.hpp -- the two kernels of core/rlwe/inner_sum.go's PartialTracesSum: an NTT-domain automorphism of the output of a
// hoisted gadget product FUSED with the canonical addition that follows it, on the scaffold of stream_kernels.hip.hpp (one (poly, limb) row per
// blockIdx.x, the row's coefficient pairs over blockIdx.y, 16-byte moves).
//
// The index map (ring/automorphism.go:12-35, standard rings): index(j) = bitrev(((gen * (2 bitrev(j) + 1) mod 2N) - 1) / 2).  In bit-reversed terms
// the source of output j' is s' = gen j' + (gen - 1) / 2 mod N.  Outputs 2i and 2i + 1 differ in the TOP bit of j', so their sources differ by
// gen N / 2 = N / 2 mod N, the top bit of s' again: index(2i + 1) = index(2i) ^ 1.  An output pair therefore reads ONE aligned input pair, swapped
// when index(2i) is odd -- the gathered operand moves as 16 bytes too, and a wavefront's 64 pairs come from one aligned 1 KiB span of the row.
#pragma once
#include "paired_gather.hip.hpp"

// The tail of AutomorphismHoistedLazy (core/rlwe/evaluator_automorphism.go:107-160, NTT-domain ctQP) followed by ringQP.Add (inner_sum.go:245-246):
//   acc_c[j] = [first ? 0 : acc_c[j]] + tmp_c[index(j)] + [c == 0 and the row is a Q row] (P mod q_i) * ct0[index(j)]      (canonical)
// Every intermediate of the reference's sequence is a canonical residue (MulScalarBigintThenAdd and Add end in CRed), so the value is the reference's.
// tmp: the lazy hoisted product; ct0: ctIn[0], LQ limbs per poly.   grid: (2 * npoly * (LQ + LP), chunks): StreamComp, then StreamRowQP
__global__ void __launch_bounds__(256)
rotate_accumulate_qp_kernel(RhQP acc, RhQPc tmp, const u64* ct0, int logN, u32 gen, const LimbConsts* __restrict__ constsQ,
                            const LimbConsts* __restrict__ constsP, int LQ, int LP, int npoly, RhPmodQ pq, int first, int nt) {
  const StreamComp sc((u32)npoly * (u32)(LQ + LP));
  const StreamRowQP r(sc.row, constsQ, constsP, LQ, LP, logN);
  u64* a = r.of(acc, sc.comp);
  const u64* x = r.of(tmp, sc.comp);
  const bool with_ct0 = r.inQ && sc.comp == 0;
  const u64* c0 = ct0 + r.ro;                   // read only when with_ct0
  const u64 s = r.inQ ? pq.s[r.l] : 0;
  const u64 q = r.c.q, qinv = r.c.qinv;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const u32 idx = rh_galois_index_even(i, logN, gen);
    ulonglong2 t = rh_gather2(x, idx);
    if (with_ct0) {
      const ulonglong2 u = rh_gather2(c0, idx);
      t.x = cred(t.x + mred(u.x, s, q, qinv), q); t.y = cred(t.y + mred(u.y, s, q, qinv), q);
    }
    rh_accumulate2(a, i, t, q, first, nt);
  }
}

// The two AutomorphismNTT calls that end AutomorphismHoisted (evaluator_automorphism.go:90-95) followed by ringQ.Add (inner_sum.go:279-280):
//   ct_c[j] = ct_c[j] + tmp_c[index(j)] mod q, in place on ct; tmp is another buffer.   grid: (2 * npoly * L, chunks)
__global__ void __launch_bounds__(256)
rotate_add_q_kernel(u64* ct0, u64* ct1, const u64* tmp0, const u64* tmp1, int logN, u32 gen, const LimbConsts* __restrict__ consts, int L, int npoly, int nt) {
  const StreamComp sc((u32)npoly * (u32)L);
  const u64 q = consts[sc.row % (u32)L].q;
  const size_t ro = (size_t)sc.row << logN;
  u64* ct = (sc.comp ? ct1 : ct0) + ro;
  const u64* tmp = (sc.comp ? tmp1 : tmp0) + ro;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const ulonglong2 t = rh_gather2(tmp, rh_galois_index_even(i, logN, gen));
    ulonglong2 v = rh_ld2(ct + 2 * (size_t)i, nt);
    v.x = cred(v.x + t.x, q); v.y = cred(v.y + t.y, q);
    rh_st2(ct + 2 * (size_t)i, v, nt);
  }
}

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

struct InnerSumQP {
  u64* accQ[2]; u64* accP[2];                   // accumulators modulo Q (LQ limbs per poly) and modulo P (LP limbs per poly), dense
  const u64* tmpQ[2]; const u64* tmpP[2];       // the lazy hoisted product, same shapes
  const u64* ct0;                               // ctIn[0], LQ limbs per poly
};

// The tail of AutomorphismHoistedLazy (core/rlwe/evaluator_automorphism.go:107-160, NTT-domain ctQP) followed by ringQP.Add (inner_sum.go:245-246):
//   acc_c[j] = [first ? 0 : acc_c[j]] + tmp_c[index(j)] + [c == 0 and the row is a Q row] (P mod q_i) * ct0[index(j)]      (canonical)
// Every intermediate of the reference's sequence is a canonical residue (MulScalarBigintThenAdd and Add end in CRed), so the value is the reference's.
// grid: (2 * npoly * (LQ + LP), chunks): component, poly, then the LQ rows of Q and the LP rows of P.
__global__ void __launch_bounds__(256)
rotate_accumulate_qp_kernel(InnerSumQP a, int logN, u32 gen, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP,
                            int LQ, int LP, int npoly, RhPmodQ pq, int first, int nt) {
  const u32 LT_ = (u32)(LQ + LP), per = (u32)npoly * LT_;
  const u32 comp = blockIdx.x / per, rem = blockIdx.x % per, poly = rem / LT_, l = rem % LT_;
  const bool inQ = l < (u32)LQ;
  const LimbConsts c = inQ ? constsQ[l] : constsP[l - LQ];
  const size_t ro = (inQ ? (size_t)poly * LQ + l : (size_t)poly * LP + (l - LQ)) << logN;
  u64* acc = (inQ ? a.accQ[comp] : a.accP[comp]) + ro;
  const u64* tmp = (inQ ? a.tmpQ[comp] : a.tmpP[comp]) + ro;
  const bool with_ct0 = inQ && comp == 0;
  const u64* ct0 = a.ct0 + ro;                  // read only when with_ct0
  const u64 s = inQ ? pq.s[l] : 0;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const u32 idx = is_index_even(i, logN, gen);
    const ulonglong2 t = is_gather2(tmp, idx);
    ulonglong2 v = first ? make_ulonglong2(0, 0) : rh_ld2(acc + 2 * (size_t)i, nt);
    v.x = cred(v.x + t.x, c.q); v.y = cred(v.y + t.y, c.q);
    if (with_ct0) {
      const ulonglong2 x = is_gather2(ct0, idx);
      v.x = cred(v.x + mred(x.x, s, c.q, c.qinv), c.q); v.y = cred(v.y + mred(x.y, s, c.q, c.qinv), c.q);
    }
    rh_st2(acc + 2 * (size_t)i, v, nt);
  }
}

// The two AutomorphismNTT calls that end AutomorphismHoisted (evaluator_automorphism.go:90-95) followed by ringQ.Add (inner_sum.go:279-280):
//   ct_c[j] = ct_c[j] + tmp_c[index(j)] mod q, in place on ct; tmp is another buffer.   grid: (2 * npoly * L, chunks)
__global__ void __launch_bounds__(256)
rotate_add_q_kernel(u64* ct0, u64* ct1, const u64* tmp0, const u64* tmp1, int logN, u32 gen, const LimbConsts* __restrict__ consts, int L, int npoly, int nt) {
  const u32 per = (u32)npoly * (u32)L;
  const u32 comp = blockIdx.x / per, rem = blockIdx.x % per;
  const u64 q = consts[rem % (u32)L].q;
  const size_t ro = (size_t)rem << logN;
  u64* ct = (comp ? ct1 : ct0) + ro;
  const u64* tmp = (comp ? tmp1 : tmp0) + ro;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const ulonglong2 t = is_gather2(tmp, is_index_even(i, logN, gen));
    ulonglong2 v = rh_ld2(ct + 2 * (size_t)i, nt);
    v.x = cred(v.x + t.x, q); v.y = cred(v.y + t.y, q);
    rh_st2(ct + 2 * (size_t)i, v, nt);
  }
}

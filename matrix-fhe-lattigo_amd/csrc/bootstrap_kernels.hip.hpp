// bootstrap_kernels.hip.hpp -- the streaming kernels of CKKS bootstrapping (bootstrap.hip), on the scaffold of stream_kernels.hip.hpp.
#pragma once
#include "modarith.hip.hpp"
#include "stream_kernels.hip.hpp"

// ---- ModUp: the lift of circuits/ckks/bootstrapping/evaluator.go:678-696 (c0), :703-722 (c1, sparse-secret encapsulation), :762-775 (c1, dense) ----
// in[j]:  limb 0 of component j in the coefficient domain, blocks of in_rows limbs per poly (only row 0 of a poly is read).
// out[j]: blocks (npoly, LQ, N).  ENCAP: component 1 goes to qp_q (npoly, LQ, N) and qp_p (npoly, LP, N) and out[1] is not touched.
// Per coefficient: centred around q0 (coeff >= q0 >> 1, or coeff > q0 >> 1 for the encapsulated c1: :687, :707, :766), |coeff| reduced by ONE
// BRedAdd per limb, negated back.  The reference's (Q[i] - tmp) * neg is Q[i] when Q[i] divides |coeff|; the canonical 0 is written here.
// SCALE: the message scalar of :735-750 / :781-789 as MForm residues per limb (s.a: Q, s.b: P), multiplied in before the store -- MulScalar
// after the NTT gives the same bits, the NTT being linear and both ends canonical.
// Every limb of the outputs is written, limb 0 included (its own lift, times the scalar); no output may overlap an input.
// grid: (2 * npoly, chunks): one (component, poly) per blockIdx.x, a lane owns a coefficient pair and walks the output limbs, so every store is a
// coalesced row segment and the limb constants are wave-uniform.  8 bytes read, 8 * (LQ [+ LP]) written per coefficient and component.
struct ModUpArgs { const u64* in[2]; u64* out[2]; u64* qp_q; u64* qp_p; };

template <bool ENCAP, bool SCALE>
__global__ void __launch_bounds__(256)
bootstrap_modup_kernel(ModUpArgs p, unsigned n, int in_rows, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP,
                       int LQ, int LP, int npoly, RhScalars s, int nt) {
  const StreamComp sc((u32)npoly);
  const bool enc = ENCAP && sc.comp == 1;
  const u64 q0 = constsQ[0].q, half = q0 >> 1;
  const u64* in = p.in[sc.comp] + (size_t)sc.row * (size_t)in_rows * n;
  u64* outQ = (enc ? p.qp_q : p.out[sc.comp]) + (size_t)sc.row * (size_t)LQ * n;
  u64* outP = enc ? p.qp_p + (size_t)sc.row * (size_t)LP * n : nullptr;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const ulonglong2 x = rh_ld2(in + 2 * (size_t)i, nt);
    const bool nx = enc ? x.x > half : x.x >= half, ny = enc ? x.y > half : x.y >= half;
    const u64 ax = nx ? q0 - x.x : x.x, ay = ny ? q0 - x.y : x.y;
    auto lift = [&](const LimbConsts& c, u64 sm) -> ulonglong2 {
      u64 tx = bred_add(ax, c.q, c.bred0), ty = bred_add(ay, c.q, c.bred0);
      if (nx && tx) tx = c.q - tx;
      if (ny && ty) ty = c.q - ty;
      if (SCALE) { tx = mred(tx, sm, c.q, c.qinv); ty = mred(ty, sm, c.q, c.qinv); }
      return make_ulonglong2(tx, ty);
    };
    for (int l = 0; l < LQ; ++l) rh_st2(outQ + (size_t)l * n + 2 * (size_t)i, lift(constsQ[l], s.a[l]), nt);
    if (enc)
      for (int l = 0; l < LP; ++l) rh_st2(outP + (size_t)l * n + 2 * (size_t)i, lift(constsP[l], s.b[l]), nt);
  }
}

// ---- the double-angle step of circuits/ckks/mod1/mod1_evaluator.go:108-114 between MulRelin and Rescale ----
// c0 <- CRed(CRed(c0 + c0) + k), c1 <- CRed(c1 + c1): Add(res, res, res) and Add(res, -sqrt2pi, res) in one launch over both components;
// k = s.a[limb] on coefficients [0, N/2), s.b[limb] on the rest (the double RNS scalar of evaluateWithScalar).
// grid: (2 * npoly * L, chunks)
__global__ void __launch_bounds__(256)
ckks_double_angle_kernel(u64* c0, u64* c1, unsigned n, const LimbConsts* __restrict__ consts, int L, int npoly, RhScalars s, int nt) {
  const StreamComp sc((u32)npoly * (u32)L);
  const u32 limb = sc.row % (u32)L;
  const u64 q = consts[limb].q, sa = s.a[limb], sb = s.b[limb];
  u64* c = (sc.comp ? c1 : c0) + (size_t)sc.row * n;
  const unsigned half = n >> 2;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    ulonglong2 x = rh_ld2(c + 2 * (size_t)i, nt);
    x.x = cred(x.x + x.x, q); x.y = cred(x.y + x.y, q);
    if (sc.comp == 0) { const u64 k = i < half ? sa : sb; x.x = cred(x.x + k, q); x.y = cred(x.y + k, q); }
    rh_st2(c + 2 * (size_t)i, x, nt);
  }
}

// ---- pack / unpack of BootstrapMany (circuits/ckks/bootstrapping/evaluator.go:1035-1058, :985-1001) ----
// One launch covers T tree levels lo .. lo + T - 1 of one component pair: tbl holds their T rows per limb, NTT domain, Montgomery form, as a
// block (T, tbl_rows, N) -- xPow2[logGap - i] (pack) or xPow2Inv[logGap - i] (unpack), i the level.  Groups of 2^T polys: group j of the wide side
// is polys j 2^T .. of `cnt_wide`, the last group holding what is left (m, the same for every lane of a workgroup).
// The reference's tree, level by level over a group, is a depth-first walk here: fold<T> is fold<T-1> of the lower half, plus fold<T-1> of the
// upper half times the level's row when the upper half exists -- the tree's own operations on the tree's own operands (a ciphertext that has
// no partner at a level moves up as it is: :1052-1057), so the words are the reference's.  T is a template argument and the walk is unrolled, so
// the T + 1 live pairs and the T table pairs sit in registers under static names.
struct PackArgs { const u64* in[2]; u64* out[2]; };

template <int T, bool FULL>
RH_DEV ulonglong2 bts_fold(const u64* in, size_t stride, unsigned k0, unsigned m, const ulonglong2* t, u64 q, u64 qi, bool nt) {
  if constexpr (T == 0) {
    return rh_ld2(in + (size_t)k0 * stride, nt);
  } else {
    ulonglong2 eve = bts_fold<T - 1, FULL>(in, stride, k0, m, t, q, qi, nt);
    if (FULL || k0 + (1u << (T - 1)) < m) {
      const ulonglong2 odd = bts_fold<T - 1, FULL>(in, stride, k0 + (1u << (T - 1)), m, t, q, qi, nt);
      eve.x = cred(eve.x + mred(odd.x, t[T - 1].x, q, qi), q);                  // MulCoeffsMontgomeryThenAdd(odd, xPow2[logGap - i], eve)
      eve.y = cred(eve.y + mred(odd.y, t[T - 1].y, q, qi), q);
    }
    return eve;
  }
}

template <int T, bool FULL>
RH_DEV void bts_spread(u64* out, size_t stride, unsigned k0, unsigned m, ulonglong2 v, const ulonglong2* t, u64 q, u64 qi, bool nt) {
  if constexpr (T == 0) {
    rh_st2(out + (size_t)k0 * stride, v, nt);
  } else {
    bts_spread<T - 1, FULL>(out, stride, k0, m, v, t, q, qi, nt);
    if (FULL || k0 + (1u << (T - 1)) < m) {
      v.x = mred(v.x, t[T - 1].x, q, qi);                                      // MulCoeffsMontgomery(ct, xPow2Inv[logGap - i], ct)
      v.y = mred(v.y, t[T - 1].y, q, qi);
      bts_spread<T - 1, FULL>(out, stride, k0 + (1u << (T - 1)), m, v, t, q, qi, nt);
    }
  }
}

// Pack: in (cnt_wide, in_rows, N) -> out (ceil(cnt_wide / 2^T), out_rows, N) per component.  grid: (2 * cnt_narrow * L, chunks): one output row per
// blockIdx.x.  Every input word is read once; the table rows (T per limb) are read by every group and stay in cache (default policy always).
template <int T>
__global__ void __launch_bounds__(256)
bootstrap_pack_kernel(PackArgs p, unsigned n, const LimbConsts* __restrict__ consts, int L, int in_rows, int out_rows, unsigned cnt_wide,
                      unsigned cnt_narrow, const u64* __restrict__ tbl, int tbl_rows, int nt) {
  const StreamComp sc(cnt_narrow * (u32)L);
  const u32 limb = sc.row % (u32)L, j = sc.row / (u32)L;
  const u64 q = consts[limb].q, qi = consts[limb].qinv;
  const unsigned m = min(1u << T, cnt_wide - (j << T));
  const size_t stride = (size_t)in_rows * n;
  const u64* in = p.in[sc.comp] + ((size_t)(j << T) * in_rows + limb) * n;
  u64* out = p.out[sc.comp] + ((size_t)j * out_rows + limb) * n;
  const u64* trow = tbl + (size_t)limb * n;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    ulonglong2 t[T];
#pragma unroll
    for (int l = 0; l < T; ++l) t[l] = rh_ld2(trow + (size_t)l * tbl_rows * n + 2 * (size_t)i, false);
    const ulonglong2 v = m == (1u << T) ? bts_fold<T, true>(in + 2 * (size_t)i, stride, 0, m, t, q, qi, nt)
                                        : bts_fold<T, false>(in + 2 * (size_t)i, stride, 0, m, t, q, qi, nt);
    rh_st2(out + 2 * (size_t)i, v, nt);
  }
}

// Unpack: in (cnt_narrow, in_rows, N) -> out (cnt_wide, out_rows, N) per component, a new block: out[j 2^T + k] = in[j] times the rows of the set
// bits of k, out[j 2^T] a copy.  grid: (2 * cnt_narrow * L, chunks): one input row per blockIdx.x.
template <int T>
__global__ void __launch_bounds__(256)
bootstrap_unpack_kernel(PackArgs p, unsigned n, const LimbConsts* __restrict__ consts, int L, int in_rows, int out_rows, unsigned cnt_wide,
                        unsigned cnt_narrow, const u64* __restrict__ tbl, int tbl_rows, int nt) {
  const StreamComp sc(cnt_narrow * (u32)L);
  const u32 limb = sc.row % (u32)L, j = sc.row / (u32)L;
  const u64 q = consts[limb].q, qi = consts[limb].qinv;
  const unsigned m = min(1u << T, cnt_wide - (j << T));
  const size_t stride = (size_t)out_rows * n;
  const u64* in = p.in[sc.comp] + ((size_t)j * in_rows + limb) * n;
  u64* out = p.out[sc.comp] + ((size_t)(j << T) * out_rows + limb) * n;
  const u64* trow = tbl + (size_t)limb * n;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    ulonglong2 t[T];
#pragma unroll
    for (int l = 0; l < T; ++l) t[l] = rh_ld2(trow + (size_t)l * tbl_rows * n + 2 * (size_t)i, false);
    const ulonglong2 v = rh_ld2(in + 2 * (size_t)i, nt);
    if (m == (1u << T)) bts_spread<T, true>(out + 2 * (size_t)i, stride, 0, m, v, t, q, qi, nt);
    else bts_spread<T, false>(out + 2 * (size_t)i, stride, 0, m, v, t, q, qi, nt);
  }
}

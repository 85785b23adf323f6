// bext_kernels.hip.hpp -- the per-coefficient arithmetic of the RNS basis extension (ring/basis_extension.go: reconstructRNS :550-594,
// multSum :596-673 and the post steps of ModUpQtoP / ModDownQPtoP) as device functions, shared by the kernels of bext.hip and by the
// fused two-extension quantize of bfv.hip.  One definition of every formula: a kernel that chains extensions calls these, it does not restate them.
#pragma once
#include "modarith.hip.hpp"
#include "bext_internal.hpp"

// acc += a * b with the carry out of the 64-bit accumulator counted in cnt; b wave-uniform (a scalar-loaded constant)
RH_DEV void mac_carry(u64& acc, u32& cnt, u32 a, u32 b) {
  asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32 %1, vcc, 0, %1, vcc" : "+v"(acc), "+v"(cnt) : "v"(a), "s"(b) : "vcc");
}

// reconstructRNS for one source limb: y_i = MRed(x_i [+ half_i], (Q/q_i)^-1), and its term of the float sum that decides v
RH_DEV u64 bext_source(u64 x, const BextSource& s, int add_mode, double& vi) {
  if (add_mode == BEXT_ADD_CRED) x = cred(x + s.half, s.q);              // AddScalarBigint -> addscalarvec
  else if (add_mode == BEXT_ADD_RAW) x = x + s.half;                      // reconstructRNSCentered :522
  const u64 y = mred(x, s.qstar_inv, s.q, s.qinv);
  vi += (double)y / (double)s.q;                                          // :576-593, one rounding per op
  return y;
}

// multSum :612-649 for one target with the y_i in registers, the 128-bit sum by columns: y = y1*2^32 + y0, c = c1*2^32 + c0 with
// y, c < 2^61, so y1, c1 < 2^29.  L = sum y0*c0 (carries counted in cL), M1 = sum y0*c1, M2 = sum y1*c0 (each term < 2^61: no
// overflow up to 8 terms, carries counted in cM beyond), H = sum y1*c1 (< 2^63 for 32 terms).  One multiply-add per partial product
// instead of a 128-bit add with compare-and-select carries per term.  NS: compile-time bound on nsrc; EXACT: nsrc == NS.
template <int NS, bool EXACT>
RH_DEV void bext_mult_sum(const u64 (&yr)[NS], int nsrc, const u64* __restrict__ cj, u64& rlo, u64& rhi) {
  u64 Lc = 0, M1 = 0, M2 = 0, H = 0;
  u32 cL = 0, cM = 0;
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    if (EXACT || i < nsrc) {
      const u64 cw = cj[i];
      const u32 c0 = (u32)cw, c1 = (u32)(cw >> 32);
      const u32 y0 = (u32)yr[i], y1 = (u32)(yr[i] >> 32);
      mac_carry(Lc, cL, y0, c0);
      if constexpr (NS <= 8) {
        M1 += (u64)y0 * c1;
        M2 += (u64)y1 * c0;
      } else {
        mac_carry(M1, cM, y0, c1);
        mac_carry(M2, cM, y1, c0);
      }
      H += (u64)y1 * c1;
    }
  }
  const u64 mid = M1 + M2;
  const u64 cm = (u64)(mid < M1) + cM;                                    // weight 2^96
  rlo = Lc + (mid << 32);
  rhi = H + cL + (mid >> 32) + (u64)(rlo < Lc) + (cm << 32);
}

// the close of multSum (:651-672): one lazy Montgomery reduction of the 128-bit sum plus vtimesqmodp[j][v] -- NOT canonical
RH_DEV u64 bext_close(u64 rlo, u64 rhi, const BextTarget& t, u64 vt_entry) {
  const u64 hhi = mulhi64(rlo * t.pinv, t.p);
  return rhi - hhi + t.p + vt_entry;
}
// post steps: the centred subtraction (SubScalarBigint -> subscalarvec) and ModDown's SubThenMulScalarMontgomeryTwoModulus against `other`
RH_DEV u64 bext_post_center(u64 r, const BextTarget& t) { return cred(r + t.p - t.half, t.p); }
RH_DEV u64 bext_post_moddown(u64 r, u64 other, const BextTarget& t) { return mred(2 * t.p - other + r, t.md_scalar, t.p, t.pinv); }

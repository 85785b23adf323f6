// ckks.hip -- schemes/ckks/evaluator.go on device-resident (poly, limb, coefficient) blocks, NTT domain, residues in [0, q_i) in and out: one
// launch per evaluator call where the reference issues four to eight ring calls.
//
// Every reference call in the sequences below ends in MRed or CRed (Neg excepted, see ckks_scale_then_add_kernel), so each output word is the
// canonical residue of its class; the kernels apply the reference's own formulas element by element, in its order, and give the same bits.
//
//   ckks_tensor_kernel          the ct x ct branch of mulRelin (:821-835) and of mulRelinThenAdd (:1135-1162): MForm of op0's two components and
//                               the four products in registers.  Traffic per coefficient and limb: 8 * 7 bytes (overwrite; 8 * 23 call by call),
//                               8 * 5 (squaring), 8 * 10 (accumulate into a degree-2 output; 8 * 20 call by call), 8 * 9 (relin form).
//   ckks_mul_plain_kernel       the plaintext branches (:856-878, :1165-1175): out_j (+)= MRed(MForm(pt), ct_j), the plaintext word read once.
//   ckks_scalar_kernel          evaluateWithScalar (:433-447): Add / Sub / Mul / Mul-then-add of a double RNS scalar, one scalar for coefficients
//                               [0, N/2) and one for [N/2, N), on every component given.
//   ckks_scale_then_add_kernel  the scale-matching Add / Sub of evaluateInPlace (:246-431): Mul(ct, ratioInt, tmp) of the operand with the smaller
//                               scale, Add / Sub on the shared components, the rest copied (:422-430) and negated under Sub (:173-177).
//   ckks_axpby_kernel           out_j = ra x_j - rb t_j - [j == 0] s: the Chebyshev step of the power basis (power_basis.go:148-176) and the
//                               2 - x, 1 - x, 1 - z^2 of the inverse circuits; x and t are AtLevel views like the linear combination's terms.
//   ckks_linear_combination_kernel  a baby step of the polynomial evaluator (circuits/common/polynomial/polynomial_evaluator.go:342-355): an Add of
//                               a constant and K calls of MulThenAdd(X[k], c_k, res), out_j = [j == 0] const + sum_k MRed(X_k,j, MForm(s_k)), as ONE pass:
//                               K + 1 rows of traffic per component where the sequence moves 3 K, the products summed in 128 bits and reduced once
//                               per LC_CHUNK terms.  Its terms are AtLevel views of blocks at higher levels; its outputs may alias no input.
//
// Each thread reads all of its operands before it writes, so any output may be any input (the linear combination excepted).  Bandwidth-bound, no LDS; 16-byte loads and
// stores, rows (one limb of one poly) on blockIdx.x so the per-limb constants are wave-uniform, non-temporal beyond the Infinity Cache: the
// scaffold of stream_kernels.hip.hpp, as the BGV kernels (bgv.hip).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "stream_kernels.hip.hpp"
#include "lc_reduce.hip.hpp"

struct CkksComps { const u64* in[3]; const u64* in2[3]; u64* out[3]; };

// ACC 0: c0, c1, c2 written; 1: all three read and added to; 2: c0, c1 read and added to, c2 written (the relin form :1150).
// MFORM false: op0 comes in Montgomery form already (matrix_ckks.Evaluator.Mul, evaluator.go:166-173).
// grid: (npoly * L, chunks); L = level + 1 rows per poly.
template <bool SQUARE, int ACC, bool MFORM>
__global__ void __launch_bounds__(256)
ckks_tensor_kernel(const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* c0, u64* c1, u64* c2, unsigned n,
                   const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  auto one = [&](u64 x0, u64 x1, u64 y0, u64 y1, u64 z0, u64 z1, u64 z2, u64& o0, u64& o1, u64& o2) {
    const u64 m0 = MFORM ? mform(x0, c.q, c.bred0, c.bred1) : x0, m1 = MFORM ? mform(x1, c.q, c.bred0, c.bred1) : x1;   // (:821-822 / :1135-1136)
    if (SQUARE) { y0 = x0; y1 = x1; }
    const u64 p0 = mred(m0, y0, c.q, c.qinv), p2 = mred(m1, y1, c.q, c.qinv), p01 = mred(m0, y1, c.q, c.qinv);
    if (ACC) {
      o0 = cred(z0 + p0, c.q);                                                                 // (:1138)
      o1 = cred(cred(z1 + p01, c.q) + mred(m1, y0, c.q, c.qinv), c.q);                         // (:1139-1140)
      o2 = ACC == 1 ? cred(z2 + p2, c.q) : p2;                                                 // (:1161 / :1150)
    } else {
      o0 = p0; o2 = p2;
      o1 = SQUARE ? cred(p01 + p01, c.q) : cred(p01 + mred(m1, y0, c.q, c.qinv), c.q);         // (:827-828 / :833-834)
    }
  };
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    const ulonglong2 x0 = rh_ld2(a0 + o, nt), x1 = rh_ld2(a1 + o, nt);
    ulonglong2 y0 = make_ulonglong2(0, 0), y1 = y0, z0 = y0, z1 = y0, z2 = y0;
    if (!SQUARE) { y0 = rh_ld2(b0 + o, nt); y1 = rh_ld2(b1 + o, nt); }
    if (ACC) { z0 = rh_ld2(c0 + o, nt); z1 = rh_ld2(c1 + o, nt); }
    if (ACC == 1) z2 = rh_ld2(c2 + o, nt);
    u64 lo0, lo1, lo2, hi0, hi1, hi2;
    one(x0.x, x1.x, y0.x, y1.x, z0.x, z1.x, z2.x, lo0, lo1, lo2);
    one(x0.y, x1.y, y0.y, y1.y, z0.y, z1.y, z2.y, hi0, hi1, hi2);
    rh_st2(c0 + o, make_ulonglong2(lo0, hi0), nt); rh_st2(c1 + o, make_ulonglong2(lo1, hi1), nt); rh_st2(c2 + o, make_ulonglong2(lo2, hi2), nt);
  }
}

// out[j] (+)= MRed(MForm(pt), ct[j]) for j < NC; pt: one block (npoly, L, N) shared by the components
template <int NC, bool ACC>
__global__ void __launch_bounds__(256)
ckks_mul_plain_kernel(CkksComps p, const u64* pt, unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    const ulonglong2 w = rh_ld2(pt + o, nt);
    ulonglong2 x[NC], z[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      x[j] = rh_ld2(p.in[j] + o, nt);
      if (ACC) z[j] = rh_ld2(p.out[j] + o, nt);
    }
    const u64 mx = mform(w.x, c.q, c.bred0, c.bred1), my = mform(w.y, c.q, c.bred0, c.bred1);   // (:864 / :869 / :1171)
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      ulonglong2 r = make_ulonglong2(mred(x[j].x, mx, c.q, c.qinv), mred(x[j].y, my, c.q, c.qinv));
      if (ACC) { r.x = cred(z[j].x + r.x, c.q); r.y = cred(z[j].y + r.y, c.q); }
      rh_st2(p.out[j] + o, r, nt);
    }
  }
}

// OP 0: out = CRed(in + s); 1: out = CRed(in + q - s); 2: out = MRed(in, s); 3: out = CRed(out + MRed(in, s)) with s = s.a[limb] on the pairs
// below `half` (coefficients [0, N/2)) and s.b[limb] above; for OP >= 2 the host has put the scalars in Montgomery form.
template <int OP, int NC>
__global__ void __launch_bounds__(256)
ckks_scalar_kernel(CkksComps p, unsigned n, const LimbConsts* __restrict__ consts, int L, RhScalars s, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 sa = s.a[row.limb], sb = s.b[row.limb];
  const unsigned half = n >> 2;
  auto one = [&](u64 x, u64 z, u64 sc) -> u64 {
    if (OP == 0) return cred(x + sc, c.q);
    if (OP == 1) return cred(x + c.q - sc, c.q);
    const u64 m = mred(x, sc, c.q, c.qinv);
    return OP == 2 ? m : cred(z + m, c.q);
  };
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    const u64 sc = i < half ? sa : sb;
    ulonglong2 x[NC], z[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      x[j] = rh_ld2(p.in[j] + o, nt);
      z[j] = OP == 3 ? rh_ld2(p.out[j] + o, nt) : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) rh_st2(p.out[j] + o, make_ulonglong2(one(x[j].x, z[j].x, sc), one(x[j].y, z[j].y, sc)), nt);
  }
}

// Component j: a = in[j], b = in2[j] (either may be null).  With both: out = a' +- b' where the operand named by scaled_b is first multiplied by
// MForm(ratio) (has_ratio 0: none is).  With a alone: out = a'.  With b alone: out = b', and q - b' under Sub -- ring.Neg, which like the
// reference's maps 0 to q_i (ring/vec_ops.go:103).
__global__ void __launch_bounds__(256)
ckks_scale_then_add_kernel(CkksComps p, unsigned n, const LimbConsts* __restrict__ consts, int L, RhScalars s, int has_ratio, int sub,
                           int scaled_b, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 k = s.a[row.limb];
  const bool sa = has_ratio && !scaled_b, sb = has_ratio && scaled_b;
  auto one = [&](u64 x, u64 y, bool ha, bool hb) -> u64 {
    if (ha && sa) x = mred(x, k, c.q, c.qinv);
    if (hb && sb) y = mred(y, k, c.q, c.qinv);
    if (ha && hb) return sub ? cred(x + c.q - y, c.q) : cred(x + y, c.q);
    if (ha) return x;
    return sub ? c.q - y : y;
  };
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    ulonglong2 x[3], y[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = p.in[j] ? rh_ld2(p.in[j] + o, nt) : make_ulonglong2(0, 0);
      y[j] = p.in2[j] ? rh_ld2(p.in2[j] + o, nt) : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (!p.out[j]) continue;
      const bool ha = p.in[j] != nullptr, hb = p.in2[j] != nullptr;
      rh_st2(p.out[j] + o, make_ulonglong2(one(x[j].x, y[j].x, ha, hb), one(x[j].y, y[j].y, ha, hb)), nt);
    }
  }
}

// out_j = CRed(CRed(MRed(x_j, MForm(ra)) + q - MRed(t_j, MForm(rb))) + q - [j == 0] s): the step after a product of the Chebyshev power basis
// (circuits/common/polynomial/power_basis.go:148-176: Add(X, X, X), then Add(X, -1, X) or the scale-matching Sub(X, T_c, X)) and, with
// ra = q - 1, the 2 - x, 1 - x and 1 - z^2 of the inverse circuits (Mul by -1, Add of a constant).  k.a / k.b: ra / rb in Montgomery form;
// s.a / s.b: the constant on coefficients [0, N/2) / [N/2, N).  x and t are AtLevel views of blocks with x_rows / t_rows limbs per poly; a
// component whose t is null has no second term.  4 reads and 2 writes of a row where the composed calls move up to 8 and 6.
struct CkksAxpby { const u64* x[3]; const u64* t[3]; u64* out[3]; };

template <bool HAS_T, bool HAS_S>
__global__ void __launch_bounds__(256)
ckks_axpby_kernel(CkksAxpby p, int x_rows, int t_rows, unsigned n, const LimbConsts* __restrict__ consts, int L, RhScalars k, RhScalars s, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 ka = k.a[row.limb], kb = k.b[row.limb], sa = s.a[row.limb], sb = s.b[row.limb];
  const size_t xo = row.at(x_rows, n), to = row.at(t_rows, n);
  const unsigned half = n >> 2;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const u64 sc = i < half ? sa : sb;
    ulonglong2 x[3], t[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      x[j] = p.x[j] ? rh_ld2(p.x[j] + xo + 2 * (size_t)i, nt) : make_ulonglong2(0, 0);
      t[j] = HAS_T && p.t[j] ? rh_ld2(p.t[j] + to + 2 * (size_t)i, nt) : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (!p.out[j]) continue;
      ulonglong2 v = make_ulonglong2(mred(x[j].x, ka, c.q, c.qinv), mred(x[j].y, ka, c.q, c.qinv));
      if (HAS_T && p.t[j]) {
        v.x = cred(v.x + c.q - mred(t[j].x, kb, c.q, c.qinv), c.q);
        v.y = cred(v.y + c.q - mred(t[j].y, kb, c.q, c.qinv), c.q);
      }
      if (HAS_S && j == 0) { v.x = cred(v.x + c.q - sc, c.q); v.y = cred(v.y + c.q - sc, c.q); }
      rh_st2(p.out[j] + row.ro + 2 * (size_t)i, v, nt);
    }
  }
}

// ---- real / imaginary split and merge of the homomorphic DFT (circuits/ckks/dft/dft.go) -----------------------------------------------------
struct CkksPair { const u64* a[2]; const u64* b[2]; u64* o0[2]; u64* o1[2]; };

// SPLIT: a = z, b = zc = Conjugate(z); o0 = re = CRed(zc + z) (Add, :276), o1 = im = MRed(CRed(z + q - zc), MForm(-i)) (Sub :267, Mul :271).
// else:  a = re, b = im; o0 = out = CRed(MRed(im, MForm(i)) + re) (Mul :324, Add :328).  The scalar as ckks_scalar_kernel takes it: s.a on
// coefficients [0, N/2), s.b on [N/2, N), in Montgomery form.  Both components in one launch; 5 reads and 3 writes of a row become 2 and 2.
template <bool SPLIT>
__global__ void __launch_bounds__(256)
ckks_real_imag_kernel(CkksPair p, unsigned n, const LimbConsts* __restrict__ consts, int L, RhScalars s, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 sa = s.a[row.limb], sb = s.b[row.limb];
  const unsigned half = n >> 2;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    const u64 sc = i < half ? sa : sb;
    ulonglong2 x[2], y[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) { x[j] = rh_ld2(p.a[j] + o, nt); y[j] = rh_ld2(p.b[j] + o, nt); }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (SPLIT) {
        const ulonglong2 re = make_ulonglong2(cred(y[j].x + x[j].x, c.q), cred(y[j].y + x[j].y, c.q));
        const ulonglong2 im = make_ulonglong2(mred(cred(x[j].x + c.q - y[j].x, c.q), sc, c.q, c.qinv), mred(cred(x[j].y + c.q - y[j].y, c.q), sc, c.q, c.qinv));
        rh_st2(p.o0[j] + o, re, nt); rh_st2(p.o1[j] + o, im, nt);
      } else {
        rh_st2(p.o0[j] + o, make_ulonglong2(cred(mred(y[j].x, sc, c.q, c.qinv) + x[j].x, c.q), cred(mred(y[j].y, sc, c.q, c.qinv) + x[j].y, c.q)), nt);
      }
    }
  }
}

// ---- linear combination ---------------------------------------------------------------------------------------------------------------
// The 128-bit accumulate-then-reduce, its chunk bound (LC_CHUNK, LC_WIDTH, LC_MODULUS_BITS) and lc_reduce: lc_reduce.hip.hpp, shared with lintrans.hip.
// The device table of a call, in words: the constant's scalars a[L], b[L] (coefficients [0, N/2), [N/2, N)), then per term
// { block of component 0, 1, 2; limbs per poly of the blocks; a[L]; b[L] }, the scalars in Montgomery form.
#define LC_TERM_HEAD 4
static inline size_t lc_table_words(int nterms, int L) { return 2 * (size_t)L + (size_t)nterms * (LC_TERM_HEAD + 2 * (size_t)L); }

// grid: (npoly * L, chunks).  The term loops run on kernel arguments and table words alone: wave-uniform.
template <int NC>
__global__ void __launch_bounds__(256)
ckks_linear_combination_kernel(CkksComps p, const u64* __restrict__ table, int nterms, int has_const, unsigned n, const LimbConsts* __restrict__ consts,
                               int L, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const unsigned half = n >> 2;
  const size_t stride = LC_TERM_HEAD + 2 * (size_t)L;
  const u64* terms = table + 2 * (size_t)L;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const bool lower = i < half;
    ulonglong2 res[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) res[j] = make_ulonglong2(0, 0);
    if (has_const) { const u64 ca = table[row.limb], cb = table[L + row.limb]; res[0].x = res[0].y = lower ? ca : cb; }
    for (int k0 = 0; k0 < nterms; k0 += LC_CHUNK) {
      const int k1 = min(k0 + LC_CHUNK, nterms);
      u128 acc[NC][2];
#pragma unroll
      for (int j = 0; j < NC; ++j) acc[j][0] = acc[j][1] = 0;
      for (int k = k0; k < k1; k += LC_WIDTH) {
        ulonglong2 x[LC_WIDTH][NC];
        u64 sc[LC_WIDTH];
#pragma unroll
        for (int w = 0; w < LC_WIDTH; ++w) {
          if (k + w >= k1) break;
          const u64* t = terms + (size_t)(k + w) * stride;
          const size_t o = row.at((int)t[3], n) + 2 * (size_t)i;
#pragma unroll
          for (int j = 0; j < NC; ++j) x[w][j] = rh_ld2(lc_block(t[j]) + o, nt);
          const u64 sa = t[LC_TERM_HEAD + row.limb], sb = t[LC_TERM_HEAD + L + row.limb];
          sc[w] = lower ? sa : sb;
        }
#pragma unroll
        for (int w = 0; w < LC_WIDTH; ++w) {
          if (k + w >= k1) break;
#pragma unroll
          for (int j = 0; j < NC; ++j) { acc[j][0] += (u128)x[w][j].x * sc[w]; acc[j][1] += (u128)x[w][j].y * sc[w]; }
        }
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) { res[j].x = cred(res[j].x + lc_reduce(acc[j][0], c), c.q); res[j].y = cred(res[j].y + lc_reduce(acc[j][1], c), c.q); }
    }
    const size_t o = row.ro + 2 * (size_t)i;
#pragma unroll
    for (int j = 0; j < NC; ++j) rh_st2(p.out[j] + o, res[j], nt);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static const unsigned CKKS_RINGS = 1u << RH_RING_STANDARD | 1u << RH_RING_CI;    // the CKKS evaluator's rings; N a multiple of 4 (two scalar halves of pairs)

static int tensor_launch(rh_ring* r, int level, const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* c0, u64* c1, u64* c2, int npoly,
                         int accumulate, bool square, bool mform_first, const char* what = "ckks_tensor_kernel") {
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const LimbConsts* lc = r->d_consts;
  const int L = level + 1;
#define CKKS_T(SQ, ACC, MF) ckks_tensor_kernel<SQ, ACC, MF><<<g.grid, 256, 0, st>>>(a0, a1, b0, b1, c0, c1, c2, n, lc, L, g.nt)
  if (!mform_first) CKKS_T(false, 0, false);
  else if (square) CKKS_T(true, 0, true);
  else if (accumulate == 0) CKKS_T(false, 0, true);
  else if (accumulate == 1) CKKS_T(false, 1, true);
  else CKKS_T(false, 2, true);
#undef CKKS_T
  return rh_launch_ok(what);
}

extern "C" int rh_ckks_tensor(rh_ring* r, int level, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                              uint64_t* c0, uint64_t* c1, uint64_t* c2, int npoly, int accumulate, int square) {
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, "rh_ckks_tensor")) return rc;
  if (!a0 || !a1 || !c0 || !c1 || !c2 || ((b0 == nullptr) != (b1 == nullptr))) return rh_fail(RH_ERR_ARG, "rh_ckks_tensor: null argument");
  if (accumulate < 0 || accumulate > 2) return rh_fail(RH_ERR_ARG, "rh_ckks_tensor: accumulate must be 0 (overwrite), 1 (c0, c1, c2) or 2 (c0, c1; c2 overwritten)");
  if (square && accumulate) return rh_fail(RH_ERR_ARG, "rh_ckks_tensor: the squaring case comes without accumulate");
  if (square && b0 && (b0 != a0 || b1 != a1)) return rh_fail(RH_ERR_ARG, "rh_ckks_tensor: the squaring case takes b = NULL or b == a");
  if (!square && !b0) return rh_fail(RH_ERR_ARG, "rh_ckks_tensor: null argument");
  return tensor_launch(r, level, a0, a1, b0, b1, c0, c1, c2, npoly, accumulate, square != 0, true);
}

// The degree-1 x degree-1 tensoring alone (ringhip.h), on any ring kind: the 3N ring of matrix_ckks.Evaluator.Mul calls it with
// mform_first = 0.  With mform_first = 1 it is rh_ckks_tensor(accumulate 0, square 0).
extern "C" int rh_ring_tensor_degree1(rh_ring* r, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                                      uint64_t* c0, uint64_t* c1, uint64_t* c2, int npoly, int level, int mform_first) {
  if (!r || !a0 || !a1 || !b0 || !b1 || !c0 || !c1 || !c2) return rh_fail(RH_ERR_ARG, "tensor_degree1: null argument");
  if (int rc = rh_scheme_args(r, level, npoly, ~0u, 2, "tensor_degree1")) return rc;
  return tensor_launch(r, level, a0, a1, b0, b1, c0, c1, c2, npoly, 0, false, mform_first != 0, "tensor_degree1");
}

extern "C" int rh_ckks_mul_plain(rh_ring* r, int level, const uint64_t* ct0, const uint64_t* ct1, const uint64_t* ct2, const uint64_t* pt,
                                 uint64_t* out0, uint64_t* out1, uint64_t* out2, int npoly, int accumulate) {
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, "rh_ckks_mul_plain")) return rc;
  if (!pt) return rh_fail(RH_ERR_ARG, "rh_ckks_mul_plain: null argument");
  if (int rc = rh_comps3(ct0, ct1, ct2, out0, out1, out2, "rh_ckks_mul_plain")) return rc;
  if (accumulate < 0 || accumulate > 1) return rh_fail(RH_ERR_ARG, "rh_ckks_mul_plain: accumulate must be 0 or 1");
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const CkksComps p{{ct0, ct1, ct2}, {nullptr, nullptr, nullptr}, {out0, out1, out2}};
  const int nc = ct2 ? 3 : ct1 ? 2 : 1, L = level + 1;
#define CKKS_P(NC, ACC) ckks_mul_plain_kernel<NC, ACC><<<g.grid, 256, 0, st>>>(p, pt, n, r->d_consts, L, g.nt)
  if (accumulate) { if (nc == 1) CKKS_P(1, true); else if (nc == 2) CKKS_P(2, true); else CKKS_P(3, true); }
  else { if (nc == 1) CKKS_P(1, false); else if (nc == 2) CKKS_P(2, false); else CKKS_P(3, false); }
#undef CKKS_P
  return rh_launch_ok("ckks_mul_plain_kernel");
}

extern "C" int rh_ckks_scalar(rh_ring* r, int level, int op, const uint64_t* in0, const uint64_t* in1, const uint64_t* in2,
                              uint64_t* out0, uint64_t* out1, uint64_t* out2, int npoly, const uint64_t* s0, const uint64_t* s1) {
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, "rh_ckks_scalar")) return rc;
  if (!s0 || !s1) return rh_fail(RH_ERR_ARG, "rh_ckks_scalar: null argument");
  if (int rc = rh_comps3(in0, in1, in2, out0, out1, out2, "rh_ckks_scalar")) return rc;
  if (op < RH_CKKS_ADD_SCALAR || op > RH_CKKS_MUL_SCALAR_THEN_ADD) return rh_fail(RH_ERR_ARG, "rh_ckks_scalar: op must be 0 (add), 1 (sub), 2 (mul) or 3 (mul then add)");
  RhScalars s;                                                          // MulDoubleRNSScalar(ThenAdd): MForm(scalar) (ring/operations.go:250-266)
  if (int rc = rh_pack_scalars(r, level, s0, s1, op >= RH_CKKS_MUL_SCALAR, &s, "rh_ckks_scalar")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const CkksComps p{{in0, in1, in2}, {nullptr, nullptr, nullptr}, {out0, out1, out2}};
  const int nc = in2 ? 3 : in1 ? 2 : 1, L = level + 1;
#define CKKS_S(OP, NC) ckks_scalar_kernel<OP, NC><<<g.grid, 256, 0, st>>>(p, n, r->d_consts, L, s, g.nt)
#define CKKS_SN(OP) do { if (nc == 1) CKKS_S(OP, 1); else if (nc == 2) CKKS_S(OP, 2); else CKKS_S(OP, 3); } while (0)
  if (op == RH_CKKS_ADD_SCALAR) CKKS_SN(0);
  else if (op == RH_CKKS_SUB_SCALAR) CKKS_SN(1);
  else if (op == RH_CKKS_MUL_SCALAR) CKKS_SN(2);
  else CKKS_SN(3);
#undef CKKS_SN
#undef CKKS_S
  return rh_launch_ok("ckks_scalar_kernel");
}

extern "C" int rh_ckks_scale_then_add(rh_ring* r, int level, const uint64_t* a0, const uint64_t* a1, const uint64_t* a2, const uint64_t* b0,
                                      const uint64_t* b1, const uint64_t* b2, uint64_t* out0, uint64_t* out1, uint64_t* out2, int npoly,
                                      const uint64_t* ratio, int sub, int scaled_is_b) {
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, "rh_ckks_scale_then_add")) return rc;
  if (!a0 || !b0 || !out0) return rh_fail(RH_ERR_ARG, "rh_ckks_scale_then_add: null argument");
  if ((a2 && !a1) || (b2 && !b1) || (out2 && !out1)) return rh_fail(RH_ERR_ARG, "rh_ckks_scale_then_add: component 2 needs component 1");
  if ((out1 != nullptr) != (a1 || b1) || (out2 != nullptr) != (a2 || b2))
    return rh_fail(RH_ERR_ARG, "rh_ckks_scale_then_add: the output has the components of the larger operand, no more and no fewer");
  RhScalars s;                                                          // Mul(ct, ratioInt, tmp) -> MulDoubleRNSScalar: MForm(ratio mod q_i)
  if (int rc = rh_pack_scalars(r, level, ratio, nullptr, true, &s, "rh_ckks_scale_then_add", "ratio")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  const CkksComps p{{a0, a1, a2}, {b0, b1, b2}, {out0, out1, out2}};
  ckks_scale_then_add_kernel<<<g.grid, 256, 0, rh_stream(r)>>>(p, n, r->d_consts, level + 1, s, ratio ? 1 : 0, sub ? 1 : 0, scaled_is_b ? 1 : 0, g.nt);
  return rh_launch_ok("ckks_scale_then_add_kernel");
}

extern "C" int rh_ckks_axpby(rh_ring* r, int level, const uint64_t* x0, const uint64_t* x1, const uint64_t* x2, int x_rows, const uint64_t* t0,
                             const uint64_t* t1, const uint64_t* t2, int t_rows, uint64_t* out0, uint64_t* out1, uint64_t* out2, int npoly,
                             const uint64_t* ra, const uint64_t* rb, const uint64_t* s0, const uint64_t* s1) {
  const char* who = "rh_ckks_axpby";
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, who)) return rc;
  if (int rc = rh_comps3(x0, x1, x2, out0, out1, out2, who)) return rc;
  if (!ra || (s0 == nullptr) != (s1 == nullptr) || (t0 != nullptr) != (rb != nullptr)) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((!t0 && (t1 || t2)) || (t2 && !t1) || (t1 && !x1) || (t2 && !x2))
    return rh_fail(RH_ERR_ARG, "%s: t has components 0 .. k only, and no more components than x", who);
  const int L = level + 1;
  if (x_rows < L) return rh_fail(RH_ERR_ARG, "%s: x holds %d limbs per poly, fewer than level %d needs", who, x_rows, level);
  if (t0 && t_rows < L) return rh_fail(RH_ERR_ARG, "%s: t holds %d limbs per poly, fewer than level %d needs", who, t_rows, level);
  // an output is the dense block at this level; it may BE an input block of that same shape (each thread reads its words of every input before
  // it writes), and is otherwise apart from every input and from the other outputs
  const size_t N = (size_t)r->N, dense = (size_t)npoly * L * N;
  const u64* xs[3] = {x0, x1, x2};
  const u64* ts[3] = {t0, t1, t2};
  u64* outs[3] = {out0, out1, out2};
  RhBlock written[3];
  int nw = 0;
  for (int j = 0; j < 3; ++j) {
    if (!outs[j]) continue;
    written[nw++] = {outs[j], dense};
    for (int i = 0; i < 3; ++i) {
      const RhBlock in[2] = {{xs[i], (size_t)npoly * (size_t)x_rows * N}, {ts[i], (size_t)npoly * (size_t)t_rows * N}};
      const int rows[2] = {x_rows, t_rows};
      for (int b = 0; b < 2; ++b) {
        if (!in[b].p) continue;
        if (((uintptr_t)in[b].p | (uintptr_t)outs[j]) & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
        if (!(in[b].p == outs[j] && rows[b] == L) && rh_overlap(written[nw - 1], in[b]))
          return rh_fail(RH_ERR_ARG, "%s: an output overlaps an input without being that input at the same level", who);
      }
    }
  }
  if (int rc = rh_blocks_disjoint(written, nw, who, "two outputs overlap")) return rc;
  RhScalars k, s;
  if (int rc = rh_pack_scalars(r, level, ra, rb, true, &k, who, "factor")) return rc;        // Mul(ct, int, ct) -> MulDoubleRNSScalar: MForm(scalar)
  if (int rc = rh_pack_scalars(r, level, s0, s1, false, &s, who, "constant")) return rc;     // Add of a scalar (:82-101): the residues as they are
  const unsigned rows = (unsigned)npoly * (unsigned)L, n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const CkksAxpby p{{x0, x1, x2}, {t0, t1, t2}, {out0, out1, out2}};
#define CKKS_AX(T, S) ckks_axpby_kernel<T, S><<<g.grid, 256, 0, st>>>(p, x_rows, t0 ? t_rows : L, n, r->d_consts, L, k, s, g.nt)
  if (t0) { if (s0) CKKS_AX(true, true); else CKKS_AX(true, false); }
  else { if (s0) CKKS_AX(false, true); else CKKS_AX(false, false); }
#undef CKKS_AX
  return rh_launch_ok("ckks_axpby_kernel");
}

// every output block is an input block or apart from it (element-wise kernels: a thread reads its words of every input before it writes), and
// the outputs are apart from each other
static int real_imag_blocks(const u64* const* in, int nin, u64* const* out, int nout, size_t words, const char* who) {
  RhBlock w[4];
  for (int i = 0; i < nout; ++i) {
    w[i] = {out[i], words};
    if ((uintptr_t)out[i] & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
    for (int j = 0; j < nin; ++j) {
      if ((uintptr_t)in[j] & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
      if (out[i] != in[j] && rh_overlap(w[i], RhBlock{in[j], words})) return rh_fail(RH_ERR_ARG, "%s: an output overlaps an input without being that input", who);
    }
  }
  return rh_blocks_disjoint(w, nout, who, "two outputs overlap");
}

static int real_imag_launch(rh_ring* r, int level, const CkksPair& p, int npoly, const u64* s0, const u64* s1, bool split, const char* who) {
  RhScalars s;                                                          // Mul(ct, -+i, ct) -> MulDoubleRNSScalar: MForm(scalar)
  if (int rc = rh_pack_scalars(r, level, s0, s1, true, &s, who)) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  if (split) ckks_real_imag_kernel<true><<<g.grid, 256, 0, st>>>(p, n, r->d_consts, level + 1, s, g.nt);
  else ckks_real_imag_kernel<false><<<g.grid, 256, 0, st>>>(p, n, r->d_consts, level + 1, s, g.nt);
  return rh_launch_ok("ckks_real_imag_kernel");
}

extern "C" int rh_ckks_split_real_imag(rh_ring* r, int level, const uint64_t* const* z, const uint64_t* const* zc, uint64_t* const* re,
                                       uint64_t* const* im, int npoly, const uint64_t* s0, const uint64_t* s1) {
  const char* who = "rh_ckks_split_real_imag";
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, who)) return rc;
  if (r->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (the homomorphic DFT is not defined on conjugate-invariant rings)", who);
  if (!z || !zc || !re || !im || !s0 || !s1) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  for (int j = 0; j < 2; ++j) if (!z[j] || !zc[j] || !re[j] || !im[j]) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const u64* in[4] = {z[0], z[1], zc[0], zc[1]};
  u64* out[4] = {re[0], re[1], im[0], im[1]};
  if (int rc = real_imag_blocks(in, 4, out, 4, (size_t)npoly * (level + 1) * (size_t)r->N, who)) return rc;
  const CkksPair p{{z[0], z[1]}, {zc[0], zc[1]}, {re[0], re[1]}, {im[0], im[1]}};
  return real_imag_launch(r, level, p, npoly, s0, s1, true, who);
}

extern "C" int rh_ckks_merge_real_imag(rh_ring* r, int level, const uint64_t* const* re, const uint64_t* const* im, uint64_t* const* out,
                                       int npoly, const uint64_t* s0, const uint64_t* s1) {
  const char* who = "rh_ckks_merge_real_imag";
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, who)) return rc;
  if (r->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (the homomorphic DFT is not defined on conjugate-invariant rings)", who);
  if (!re || !im || !out || !s0 || !s1) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  for (int j = 0; j < 2; ++j) if (!re[j] || !im[j] || !out[j]) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const u64* in[4] = {re[0], re[1], im[0], im[1]};
  u64* outs[2] = {out[0], out[1]};
  if (int rc = real_imag_blocks(in, 4, outs, 2, (size_t)npoly * (level + 1) * (size_t)r->N, who)) return rc;
  const CkksPair p{{re[0], re[1]}, {im[0], im[1]}, {out[0], out[1]}, {nullptr, nullptr}};
  return real_imag_launch(r, level, p, npoly, s0, s1, false, who);
}

extern "C" size_t rh_ckks_linear_combination_table_words(int nterms, int level) { return nterms < 0 || level < 0 ? 0 : lc_table_words(nterms, level + 1); }
extern "C" int rh_ckks_linear_combination_chunk(void) { return LC_CHUNK; }
extern "C" int rh_ckks_linear_combination_width(void) { return LC_WIDTH; }

extern "C" int rh_ckks_linear_combination(rh_ring* r, int level, int nterms, const uint64_t* const* x, const int* x_rows, const uint64_t* s0,
                                          const uint64_t* s1, const uint64_t* c0, const uint64_t* c1, uint64_t* out0, uint64_t* out1, uint64_t* out2,
                                          int npoly, uint64_t* table, size_t table_words) {
  const char* who = "rh_ckks_linear_combination";
  if (int rc = rh_scheme_args(r, level, npoly, CKKS_RINGS, 4, who)) return rc;
  if (nterms < 0) return rh_fail(RH_ERR_ARG, "%s: nterms < 0", who);
  if (!out0 || (out2 && !out1) || (c0 == nullptr) != (c1 == nullptr) || (nterms && (!x || !x_rows || !s0 || !s1))) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (!table) return rh_fail(RH_ERR_ARG, "%s: null table (device scratch of rh_ckks_linear_combination_table_words(nterms, level) words)", who);
  const int L = level + 1, nc = out2 ? 3 : out1 ? 2 : 1;
  const size_t words = lc_table_words(nterms, L), N = (size_t)r->N;
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the table holds %zu words, %d terms at level %d need %zu", who, table_words, nterms, level, words);
  if (int rc = rh_moduli_below(r, L, LC_MODULUS_BITS, LC_CHUNK, who)) return rc;
  u64* outs[3] = {out0, out1, out2};
  RhBlock written[4], read[3];
  for (int j = 0; j < nc; ++j) written[j] = {outs[j], (size_t)npoly * L * N};
  written[nc] = {table, words};
  for (int k = 0; k < nterms; ++k) {
    if (x_rows[k] < L) return rh_fail(RH_ERR_ARG, "%s: term %d holds %d limbs per poly, fewer than level %d needs", who, k, x_rows[k], level);
    for (int j = 0; j < nc; ++j) {
      if (!x[3 * k + j]) return rh_fail(RH_ERR_ARG, "%s: term %d has no component %d", who, k, j);
      read[j] = {x[3 * k + j], (size_t)npoly * (size_t)x_rows[k] * N};
    }
    if (int rc = rh_blocks_ok(written, nc + 1, read, nc, who, "an output (or the table) overlaps a term: the sum is not computed in place")) return rc;
  }
  if (int rc = rh_blocks_ok(written, nc, written + nc, 1, who, "an output overlaps the table")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)L;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  u64* t = stage->h;
  RhScalars s;
  if (int rc = rh_pack_scalars(r, level, c0, c1, false, &s, who, "constant")) return rc;   // Add of a scalar (:82-101): the residues as they are
  for (int i = 0; i < L; ++i) { t[i] = s.a[i]; t[L + i] = s.b[i]; }
  for (int k = 0; k < nterms; ++k) {
    u64* e = t + 2 * (size_t)L + (size_t)k * (LC_TERM_HEAD + 2 * (size_t)L);
    for (int j = 0; j < 3; ++j) e[j] = j < nc ? (u64)(uintptr_t)x[3 * k + j] : 0;
    e[3] = (u64)x_rows[k];
    if (int rc = rh_pack_scalars(r, level, s0 + (size_t)k * L, s1 + (size_t)k * L, true, &s, who)) return rc;   // MulDoubleRNSScalarThenAdd: MForm(scalar)
    for (int i = 0; i < L; ++i) { e[LC_TERM_HEAD + i] = s.a[i]; e[LC_TERM_HEAD + L + i] = s.b[i]; }
  }
  if (int rc = rh_stage_upload(stage, table, words, st, who)) return rc;
  if (rows == 0) return RH_OK;
  const CkksComps p{{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {out0, out1, out2}};
  const unsigned n = (unsigned)r->N;
#define CKKS_LC(NC) ckks_linear_combination_kernel<NC><<<g.grid, 256, 0, st>>>(p, table, nterms, c0 ? 1 : 0, n, r->d_consts, L, g.nt)
  if (nc == 1) CKKS_LC(1); else if (nc == 2) CKKS_LC(2); else CKKS_LC(3);
#undef CKKS_LC
  return rh_launch_ok("ckks_linear_combination_kernel");
}

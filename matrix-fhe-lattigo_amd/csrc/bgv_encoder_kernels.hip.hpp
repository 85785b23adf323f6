// bgv_encoder_kernels.hip.hpp -- device side of schemes/bgv/encoder.go on standard rings: the slot permutation (permuteMatrix :98-121 with the
// value rules of EncodeRingT :187-246 / DecodeRingT :323-353), the lift from the plaintext ring into Q (RingT2Q :357-386 with the scalar
// multiplies around it) and the return from Q to T (RingQ2T :391-439, scaleDown = true).  Integer arithmetic only; the one floating-point
// value is reconstructRNS's own, taken from bext_kernels.hip.hpp so that the gap = 1 branch rounds where the reference rounds.
#pragma once
#include <hip/hip_runtime.h>
#include "stream_kernels.hip.hpp"
#include "bext_kernels.hip.hpp"

struct BgvModT { u64 t, tinv, bred0, bred1; };   // T with its MRedConstant and BRedConstant

// ---- slots -----------------------------------------------------------------------------------------------------------------------------
// One thread per word of the contiguous side; the other side is gathered through idx (nullptr: the identity, IsBatched = false).
//   ENCODE: pT[j] = rule(values[idx[j]]) for idx[j] < nvals, else 0; idx is the INVERSE of indexMatrix, so the store is contiguous.
//           []uint64: BRedAdd (ringT.Reduce :208); []int64: the sign / abs rule (:221-228).  That rule stores T for a negative multiple of T;
//           what follows in the reference (INTT :242, MulScalar :175) maps T and 0 to the same canonical word, so the word is reduced here.
//   DECODE: values[i] = pT[idx[i]], i < nvals; idx is indexMatrix.  Signed: minus T when the word is >= T >> 1 (:342).
// values: (nvec, nvals); pT: (nvec, n).  grid (ceil(n / 256), nvec).
template <bool ENCODE>
__global__ void __launch_bounds__(256)
bgv_slots_kernel(const u64* __restrict__ src, u64* __restrict__ dst, const unsigned* __restrict__ idx, unsigned n, unsigned nvals, BgvModT m,
                 int is_signed) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  const size_t vec = blockIdx.y;
  if (ENCODE) {
    if (j >= n) return;
    const unsigned i = idx ? idx[j] : j;
    u64 w = 0;
    if (i < nvals) {
      const u64 c = src[vec * nvals + i];
      if (is_signed) {
        const u64 sign = c >> 63;
        const u64 abs = bred_add(sign ? (u64)0 - c : c, m.t, m.bred0);         // uint64(c * ((sign ^ 1) - sign)): int64 min stays 2^63
        w = cred(sign * (m.t - abs) | (sign ^ 1) * abs, m.t);
      } else {
        w = bred_add(c, m.t, m.bred0);
      }
    }
    dst[vec * n + j] = w;
  } else {
    if (j >= nvals) return;
    const u64 v = src[vec * n + (idx ? idx[j] : j)];
    dst[vec * nvals + j] = (is_signed && v >= (m.t >> 1)) ? v - m.t : v;
  }
}

// ---- lift ------------------------------------------------------------------------------------------------------------------------------
// ringT.MulScalar(scale) (:175, :243) + RingT2Q (:357-386) + MForm (:274-276) as one pass over the output: row (vec, limb) of N words takes
// pT[vec][k] at coefficient k * gap and zero elsewhere.  Per word, in the reference's order:
//   y = MRed(x, MForm(scale), T)                     when has_scale (s_mont: the scalar in Montgomery form modulo T)
//   w = y                                            copied UNREDUCED into every limb (:368), also where T > q_i
//   w = MRed(w, MForm(T^-1 mod Q_level), q_i)        when scale_up (MulScalarBigint :384; k.a holds the per-limb constants)
//   w = BRedAdd(w, q_i)                              when canonical: a transform or MForm follows, which maps the raw word and its residue alike
//   w = MForm(w)                                     when mont
// Without scale_up, transform and MForm (Embed in the coefficient domain) the raw word is what the reference leaves, and so it is here.
// pT: (nvec, n); out: (nvec, L, N).  grid (nvec * L, chunks): the row-streaming scaffold.
__global__ void __launch_bounds__(256)
bgv_lift_kernel(const u64* __restrict__ pT, u64* __restrict__ out, unsigned n, unsigned N, int loggap, const LimbConsts* __restrict__ consts, int L,
                RhScalars k, BgvModT m, u64 s_mont, int has_scale, int scale_up, int canonical, int mont, int nt) {
  const StreamRow row(consts, L, N);
  const LimbConsts& c = row.c;
  const u64 tinv_q = k.a[row.limb];
  const u64* src = pT + (size_t)row.poly * n;
  auto one = [&](u64 x) -> u64 {
    if (has_scale) x = mred(x, s_mont, m.t, m.tinv);
    if (scale_up) x = mred(x, tinv_q, c.q, c.qinv);
    if (canonical) x = bred_add(x, c.q, c.bred0);
    if (mont) x = mform(x, c.q, c.bred0, c.bred1);
    return x;
  };
  const unsigned mask = (1u << loggap) - 1;
  RH_FOR_EACH_PAIR(i, 0, N >> 1) {
    const unsigned j = 2 * i;
    ulonglong2 w = make_ulonglong2(0, 0);
    if (loggap == 0) {
      w = rh_ld2(src + j, false);
      w.x = one(w.x); w.y = one(w.y);
    } else if ((j & mask) == 0) {                  // gap >= 2: the odd word of a pair is never on the stride
      w.x = one(src[j >> loggap]);
    }
    rh_st2(out + row.ro + j, w, nt);
  }
}

// ---- a whole linear transformation (circuits/common/lintrans/lintrans.go:271-292 + Embed into a ringqp.Poly) ------------------------------
// The gather of rh_bgv_embed_qp: rotateAndEncodeDiagonal's row rotation and the slot permutation in one pass, one thread per word of pT.
//   pT[vec][j] = rule(values[vec][r * cols + ((c + rot[vec]) & (cols - 1))]),   (r, c) the row and column of i = inv[j] in the 2 x cols matrix
// with the value rules of bgv_slots_kernel<true> unchanged (BRedAdd / sign-abs, zero past nvals).  rot: one word per vector, already reduced
// modulo cols, or nullptr (no rotation: the index is inv[j] itself, whatever nvals and cols).  With rot the host side has checked
// nvals == n == 2 * cols, so every index read is below nvals.  values: (nvec, nvals); pT: (nvec, n).  grid (ceil(n / 256), nvec).
__global__ void __launch_bounds__(256)
bgv_embed_gather_kernel(const u64* __restrict__ values, u64* __restrict__ pT, const unsigned* __restrict__ inv, const u64* __restrict__ rot,
                        unsigned n, unsigned nvals, unsigned cols, BgvModT m, int is_signed) {
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  const size_t vec = blockIdx.y;
  unsigned i = inv[j];
  if (rot) i = (i & ~(cols - 1)) | ((i + (unsigned)rot[vec]) & (cols - 1));
  u64 w = 0;
  if (i < nvals) {
    const u64 c = values[vec * nvals + i];
    if (is_signed) {
      const u64 sign = c >> 63;
      const u64 abs = bred_add(sign ? (u64)0 - c : c, m.t, m.bred0);
      w = cred(sign * (m.t - abs) | (sign ^ 1) * abs, m.t);
    } else {
      w = bred_add(c, m.t, m.bred0);
    }
  }
  pT[vec * n + j] = w;
}

// the row rotation alone (utils.RotateSliceAllocFree per row, :283-285), for the call-by-call form.  grid (ceil(2 * cols / 256), nvec).
__global__ void __launch_bounds__(256)
bgv_rotate_rows_kernel(const u64* __restrict__ values, u64* __restrict__ out, const u64* __restrict__ rot, unsigned cols) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= 2 * cols) return;
  const size_t vec = blockIdx.y;
  out[vec * 2 * cols + i] = values[vec * 2 * cols + ((i & ~(cols - 1)) | ((i + (unsigned)rot[vec]) & (cols - 1)))];
}

// The lift of rh_bgv_embed_qp: bgv_lift_kernel (has_scale, no scale_up) onto the rows of Q and of P in ONE launch -- row (vec, limb) of
// nvec * (LQ + LP) reads its constants from the table of its own ring and writes its own block.  Per word: MRed by MForm(scale) modulo T,
// canonical BRedAdd, MForm.  outQ: (nvec, LQ, N); outP: (nvec, LP, N).  grid (nvec * (LQ + LP), chunks).
__global__ void __launch_bounds__(256)
bgv_lift_qp_kernel(const u64* __restrict__ pT, u64* __restrict__ outQ, u64* __restrict__ outP, unsigned n, int logN, int loggap,
                   const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP, int LQ, int LP, BgvModT m, u64 s_mont,
                   int canonical, int mont, int nt) {
  const StreamRowQP row(blockIdx.x, constsQ, constsP, LQ, LP, logN);
  const LimbConsts& c = row.c;
  const u64* src = pT + (size_t)row.poly * n;
  u64* out = (row.inQ ? outQ : outP) + row.ro;
  auto one = [&](u64 x) -> u64 {
    x = mred(x, s_mont, m.t, m.tinv);
    if (canonical) x = bred_add(x, c.q, c.bred0);
    if (mont) x = mform(x, c.q, c.bred0, c.bred1);
    return x;
  };
  const unsigned mask = (1u << loggap) - 1, N = 1u << logN;
  RH_FOR_EACH_PAIR(i, 0, N >> 1) {
    const unsigned j = 2 * i;
    ulonglong2 w = make_ulonglong2(0, 0);
    if (loggap == 0) {
      w = rh_ld2(src + j, false);
      w.x = one(w.x); w.y = one(w.y);
    } else if ((j & mask) == 0) {                  // gap >= 2: the odd word of a pair is never on the stride
      w.x = one(src[j >> loggap]);
    }
    rh_st2(out + j, w, nt);
  }
}

// the copy of RingT2Q alone (:364-381), for the call-by-call form of the lift.  grid (nvec * L, ceil(N / 256)).
__global__ void __launch_bounds__(256)
bgv_spread_kernel(const u64* __restrict__ pT, u64* __restrict__ out, unsigned n, unsigned N, int loggap, int L) {
  const unsigned j = blockIdx.y * 256u + threadIdx.x;
  if (j >= N) return;
  const unsigned row = blockIdx.x, vec = row / (unsigned)L, mask = (1u << loggap) - 1;
  out[(size_t)row * N + j] = (j & mask) == 0 ? pT[(size_t)vec * n + (j >> loggap)] : 0;
}

// out[vec][k] = in[vec][limb 0][k * gap]: the gather of the level-0 strided branch (:429-431), for the call-by-call form
__global__ void __launch_bounds__(256)
bgv_gather_kernel(const u64* __restrict__ in, u64* __restrict__ out, unsigned n, unsigned N, int loggap, int in_rows) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  out[(size_t)blockIdx.y * n + k] = in[(size_t)blockIdx.y * in_rows * N + ((size_t)k << loggap)];
}

// ---- Q to T ----------------------------------------------------------------------------------------------------------------------------
struct BgvQ2TTables {
  const u64* tmont;     // (Lmax): MForm(T) modulo q_i, the scalar of ringQ.MulScalar(pQ, T) (:398)
  const u64* garner;    // (Lmax): (q_0 ... q_{j-1})^-1 mod q_j
  const u64* qmod;      // (Lmax, Lmax): q_i mod q_j at [j * Lmax + i]
  const u64* qhalf;     // (Lmax levels, Lmax digits): the mixed-radix digits of floor(Q_level / 2)
  const u64* qmodt;     // (Lmax): q_i mod T
  const u64* Qmodt;     // (Lmax): Q_level mod T
  int Lmax;
};
enum { BGV_Q2T_LEVEL0 = 0, BGV_Q2T_MODUP = 1, BGV_Q2T_EXACT = 2 };

// RingQ2T with scaleDown = true, one thread per gathered coefficient k < n (coefficient k * gap of the poly), then the MulScalar by
// scale^-1 mod T of DecodeRingT (:325) / Decode (:457) when has_sinv.  NQ: a compile-time bound on the limb count -- digits and y_i in
// registers, loops unrolled; EXACT: L == NQ (1 .. 8), else L <= NQ (16, 32), the variants bext_kernel has -- or 0 for any count (per-thread
// arrays).  in: (nvec, L, N); out: (nvec, n).  grid (ceil(n / 256), nvec).
//   LEVEL0 (:417-438)  x = MRed(in, MForm(T), q_0); CRed(x + (q_0 >> 1), q_0); BRedAdd modulo T; CRed(. + T - BRedAdd(q_0 >> 1, T), T)
//   MODUP  (:408-411)  gap = 1: per limb MRed by MForm(T), then AddScalarBigint(Q/2) + reconstructRNS + multSum onto T + SubScalarBigint(Q/2):
//                      bext_source / bext_mult_sum / bext_close / bext_post_center with the plan of ModUpQtoP onto the single modulus T.  The
//                      word is NOT canonical (multSum's is not), exactly as the reference leaves it for the MulScalar that follows.
//   EXACT  (:413-414)  gap > 1, through big integers in the reference: the mixed-radix digits of x = T * in mod Q are compared with those
//                      of floor(Q / 2) from the top digit down (the representation is unique, so the order is the integers'), x mod T comes
//                      from Horner over the digits, and x >= floor(Q / 2) subtracts Q mod T.
template <int NQ, bool EXACT>
__global__ void __launch_bounds__(256)
bgv_q2t_kernel(const u64* __restrict__ in, u64* __restrict__ out, unsigned n, unsigned N, int loggap, int L, int mode,
               const LimbConsts* __restrict__ consts, BgvQ2TTables tb, BgvModT m, const BextSource* __restrict__ S, BextTarget tgt,
               const u64* __restrict__ coef, const u64* __restrict__ vt, u64 sinv_mont, int has_sinv) {
  const unsigned k = blockIdx.x * 256u + threadIdx.x;
  if (k >= n) return;
  const size_t vec = blockIdx.y;
  const u64* p = in + vec * (size_t)L * N + ((size_t)k << loggap);
  constexpr int NA = NQ > 0 ? NQ : RH_MAX_LIMBS_K;
  u64 r;
  if (mode == BGV_Q2T_LEVEL0) {
    const LimbConsts c = consts[0];
    u64 x = mred(p[0], tb.tmont[0], c.q, c.qinv);
    x = cred(x + (c.q >> 1), c.q);
    x = bred_add(x, m.t, m.bred0);
    r = cred(x + m.t - bred_add(c.q >> 1, m.t, m.bred0), m.t);
  } else if (mode == BGV_Q2T_MODUP) {
    u64 y[NA];
    double vi = 0.0;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      y[j] = 0;
      if ((NQ > 0 && EXACT) || j < L) {
        const LimbConsts c = consts[j];
        y[j] = bext_source(mred(p[(size_t)j * N], tb.tmont[j], c.q, c.qinv), S[j], BEXT_ADD_CRED, vi);
      }
    }
    const u64 v = (u64)vi;
    u64 rlo, rhi;
    if constexpr (NQ > 0) {
      bext_mult_sum<NA, EXACT>(y, L, coef, rlo, rhi);
    } else {                                        // the same 128-bit sum, term by term
      u128 acc = 0;
      for (int j = 0; j < L; ++j) acc += (u128)y[j] * coef[j];
      rlo = (u64)acc; rhi = (u64)(acc >> 64);
    }
    r = bext_post_center(bext_close(rlo, rhi, tgt, vt[v]), tgt);
  } else {
    u64 d[NA];
    int cmp = 0;                                    // x against floor(Q / 2), decided by the highest digit that differs
    const u64* qh = tb.qhalf + (size_t)(L - 1) * tb.Lmax;
#pragma unroll
    for (int j = 0; j < NA; ++j) {
      if ((NQ > 0 && EXACT) || j < L) {
        const LimbConsts c = consts[j];
        const u64 x = mred(p[(size_t)j * N], tb.tmont[j], c.q, c.qinv);
        u64 t = 0;
        for (int i = j - 1; i >= 0; --i) {          // (d_0 + q_0 (d_1 + q_1 (...))) mod q_j
          t = bred(t, tb.qmod[j * tb.Lmax + i], c.q, c.bred0, c.bred1);
          t = cred(t + bred_add(d[i], c.q, c.bred0), c.q);
        }
        const u64 diff = x >= t ? x - t : x + c.q - t;
        d[j] = j ? bred(diff, tb.garner[j], c.q, c.bred0, c.bred1) : diff;
        if (d[j] != qh[j]) cmp = d[j] > qh[j] ? 1 : -1;
      }
    }
    u64 acc = 0;
#pragma unroll
    for (int j = NA - 1; j >= 0; --j) {
      if ((NQ > 0 && EXACT) || j < L) {
        acc = bred(acc, tb.qmodt[j], m.t, m.bred0, m.bred1);
        acc = cred(acc + bred_add(d[j], m.t, m.bred0), m.t);
      }
    }
    r = cmp >= 0 ? cred(acc + m.t - tb.Qmodt[L - 1], m.t) : acc;
  }
  if (has_sinv) r = mred(r, sinv_mont, m.t, m.tinv);
  out[vec * n + k] = r;
}

// bgv.hip -- the BGV half of schemes/bgv/evaluator.go (standard tensoring, scale matching) on device-resident (poly, limb, coefficient)
// blocks, NTT domain, residues in [0, q_i) in and out.
//
// Every reference call in the sequences below ends in MRed or CRed, so each output word is the canonical residue of its class and a fused
// kernel is free to fold constants and to sum lazily (worst case z + 2 MRed < 3q < 2^63) as long as its last step reduces to [0, q).
//
//   bgv_tensor_kernel     tensorStandard ct x ct (:665-734) and the ct x ct branch of mulRelinThenAdd (:1299-1367) in one launch.  The
//                         host folds T, the scale-matching factor r0 and both Montgomery factors into one constant per limb,
//                         k_i = T * r0 * 2^128 mod q_i, so that MRed(MRed(x, k_i), y) = x * y * T * r0: the two MulRNSScalarMontgomery
//                         passes and the two MulScalar(c0x, r0) passes cost two MReds per coefficient and no traffic.  With `accumulate`
//                         the outputs are read first and (optionally) scaled by r1 (MulScalar(opOut.Value[i], r1) :1324-1326).
//                         Traffic per coefficient and limb: 8 * 7 bytes (regular, overwrite; 8 * 17 issued call by call), 8 * 5 (squaring),
//                         8 * 10 (accumulate into a degree-2 output; up to 8 * 32 call by call with r0, r1 != 1).
//   bgv_mul_plain_kernel  the plaintext branches (:737-748, :1370-1400): out[i] (+)= ct[i] * (pt * T * r0) for every component, the
//                         plaintext word and k_i read once per coefficient.
//   bgv_axpby_kernel      matchScaleThenEvaluateInPlace (:288-305): out = r0 * a +- r1 * b, out = r0 * a, out = +- r1 * b.
//   bgv_plain_combination_kernel  a baby step of the BGV polynomial evaluator over a PolynomialVector with a mapping
//                         (circuits/common/polynomial/polynomial_evaluator.go:281-319): the Add of the encoded constant vector (:235-262) and
//                         one MulThenAdd by an encoded vector per power (:1202-1239, :1370-1400) in one launch.  Every plaintext is ONE poly
//                         shared by the batch; the products are summed in 128 bits and reduced once per LC_CHUNK terms (lc_reduce.hip.hpp).
//                         Its terms are AtLevel views of blocks at higher levels; its outputs may alias no input.
//
// Each thread reads all of its operands before it writes, so outputs may alias inputs element-wise (opOut is op0 / op1) in the first three
// kernels.  Bandwidth-bound,
// no LDS; 16-byte loads and stores, non-temporal beyond the Infinity Cache: the scaffold of stream_kernels.hip.hpp.
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "stream_kernels.hip.hpp"
#include "lc_reduce.hip.hpp"

// The per-limb constants travel by value as RhScalars: a = k (tensor, mul_plain) or MForm(r0) (axpby), b = r1.

// ACC 0: c0, c1, c2 written; 1: all three read and added to; 2: c0, c1 read and added to, c2 written (the relin form :1353).
// grid: (npoly * L, chunks); L = level + 1 rows per poly.
template <bool SQUARE, int ACC>
__global__ void __launch_bounds__(256)
bgv_tensor_kernel(const u64* a0, const u64* a1, const u64* b0, const u64* b1, u64* c0, u64* c1, u64* c2, unsigned n,
                  const LimbConsts* __restrict__ consts, int L, RhScalars s, int has_r1, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 k = s.a[row.limb], r1 = s.b[row.limb];
  auto one = [&](u64 x0, u64 x1, u64 y0, u64 y1, u64 z0, u64 z1, u64 z2, u64& o0, u64& o1, u64& o2) {
    const u64 m0 = mred(x0, k, c.q, c.qinv), m1 = mred(x1, k, c.q, c.qinv);          // x * T * r0 * 2^64
    u64 p0, p1, p2;
    if (SQUARE) {
      p0 = mred(m0, x0, c.q, c.qinv); p2 = mred(m1, x1, c.q, c.qinv);
      const u64 t = mred(m0, x1, c.q, c.qinv);
      p1 = t + t;                                                                     // < 2q
    } else {
      p0 = mred(m0, y0, c.q, c.qinv); p2 = mred(m1, y1, c.q, c.qinv);
      p1 = mred(m0, y1, c.q, c.qinv) + mred(m1, y0, c.q, c.qinv);                     // < 2q
    }
    if (ACC) {
      if (has_r1) { z0 = mred(z0, r1, c.q, c.qinv); z1 = mred(z1, r1, c.q, c.qinv); if (ACC == 1) z2 = mred(z2, r1, c.q, c.qinv); }
      o0 = cred(z0 + p0, c.q);
      o1 = cred(cred(z1 + p1, 2 * c.q), c.q);                                         // z1 + p1 < 3q
      o2 = ACC == 1 ? cred(z2 + p2, c.q) : p2;
    } else {
      o0 = p0; o1 = cred(p1, c.q); o2 = p2;
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

struct BgvComps { const u64* in[3]; u64* out[3]; };

// out[j] (+)= ct[j] * pt * T * r0 for j < NC; pt: one block (npoly, L, N) shared by the components
template <int NC, bool ACC>
__global__ void __launch_bounds__(256)
bgv_mul_plain_kernel(BgvComps p, const u64* pt, unsigned n, const LimbConsts* __restrict__ consts, int L, RhScalars s, int has_r1, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 k = s.a[row.limb], r1 = s.b[row.limb];
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    const ulonglong2 w = rh_ld2(pt + o, nt);
    ulonglong2 x[NC], z[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      x[j] = rh_ld2(p.in[j] + o, nt);
      if (ACC) z[j] = rh_ld2(p.out[j] + o, nt);
    }
    const u64 mx = mred(w.x, k, c.q, c.qinv), my = mred(w.y, k, c.q, c.qinv);         // pt * T * r0 * 2^64
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      ulonglong2 r = make_ulonglong2(mred(x[j].x, mx, c.q, c.qinv), mred(x[j].y, my, c.q, c.qinv));
      if (ACC) {
        if (has_r1) { z[j].x = mred(z[j].x, r1, c.q, c.qinv); z[j].y = mred(z[j].y, r1, c.q, c.qinv); }
        r.x = cred(z[j].x + r.x, c.q); r.y = cred(z[j].y + r.y, c.q);
      }
      rh_st2(p.out[j] + o, r, nt);
    }
  }
}

// MODE 0: out = r0 a + r1 b; 1: out = r0 a - r1 b; 2: out = r0 a; 3: out = r1 b; 4: out = -r1 b.  s.a = MForm(r0), s.b = MForm(r1).
template <int MODE>
__global__ void __launch_bounds__(256)
bgv_axpby_kernel(const u64* a, const u64* b, u64* out, unsigned n, const LimbConsts* __restrict__ consts, int L, RhScalars s, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 r0 = s.a[row.limb], r1 = s.b[row.limb];
  auto one = [&](u64 x, u64 y) -> u64 {
    const u64 u = MODE <= 2 ? mred(x, r0, c.q, c.qinv) : 0;
    if (MODE == 2) return u;
    const u64 v = mred(y, r1, c.q, c.qinv);
    return (MODE == 0 || MODE == 3) ? cred(u + v, c.q) : cred(u + c.q - v, c.q);
  };
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = row.ro + 2 * (size_t)i;
    ulonglong2 x = make_ulonglong2(0, 0), y = x;
    if (MODE <= 2) x = rh_ld2(a + o, nt);
    if (MODE != 2) y = rh_ld2(b + o, nt);
    rh_st2(out + o, make_ulonglong2(one(x.x, y.x), one(x.y, y.y)), nt);
  }
}

// ---- plain combination ------------------------------------------------------------------------------------------------------------------
// out_j = [j == 0] c cs + sum_k X_k,j (.) m_k, the canonical residue.  m_k and c: one (L, N) poly each, NTT domain, Montgomery form, read for
// every poly of the batch (default cache policy, like a diagonal of lintrans); cs: the per-limb scalar the constant is multiplied by (T^-1
// mod q_i for an encoder constant: Encode's scale-up).  Each sum is T = sum x m 2^64 in 128 bits, taken to x m by lc_reduce's Montgomery step.
// The device table of a call, in words: per term { block of component 0, 1, 2; limbs per poly of the blocks; the plaintext poly }.
#define BPC_TERM_WORDS 5
static inline size_t bpc_table_words(int nterms) { return (size_t)nterms * BPC_TERM_WORDS; }

// grid: (npoly * L, chunks).  The term loops run on kernel arguments and table words alone: wave-uniform.
template <int NC>
__global__ void __launch_bounds__(256)
bgv_plain_combination_kernel(BgvComps p, const u64* __restrict__ table, int nterms, const u64* cpoly, unsigned n, const LimbConsts* __restrict__ consts,
                             int L, RhScalars s, int nt) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const size_t po = (size_t)row.limb * n;                                               // the row of a shared plaintext poly
  const u64 cs = s.a[row.limb];
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t w = 2 * (size_t)i;
    ulonglong2 res[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) res[j] = make_ulonglong2(0, 0);
    if (cpoly) {
      const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(cpoly + po + w);
      res[0] = make_ulonglong2(lc_reduce((u128)v.x * cs, c), lc_reduce((u128)v.y * cs, c));
    }
    for (int k0 = 0; k0 < nterms; k0 += LC_CHUNK) {
      const int k1 = min(k0 + LC_CHUNK, nterms);
      u128 acc[NC][2];
#pragma unroll
      for (int j = 0; j < NC; ++j) acc[j][0] = acc[j][1] = 0;
      for (int k = k0; k < k1; k += LC_WIDTH) {
        ulonglong2 x[LC_WIDTH][NC], m[LC_WIDTH];
#pragma unroll
        for (int g = 0; g < LC_WIDTH; ++g) {
          if (k + g >= k1) break;
          const u64* t = table + (size_t)(k + g) * BPC_TERM_WORDS;
          const size_t o = row.at((int)t[3], n) + w;
          m[g] = *reinterpret_cast<const ulonglong2*>(lc_block(t[4]) + po + w);          // shared by every poly: default cache policy
#pragma unroll
          for (int j = 0; j < NC; ++j) x[g][j] = rh_ld2(lc_block(t[j]) + o, nt);
        }
#pragma unroll
        for (int g = 0; g < LC_WIDTH; ++g) {
          if (k + g >= k1) break;
#pragma unroll
          for (int j = 0; j < NC; ++j) { acc[j][0] += (u128)x[g][j].x * m[g].x; acc[j][1] += (u128)x[g][j].y * m[g].y; }
        }
      }
#pragma unroll
      for (int j = 0; j < NC; ++j) { res[j].x = cred(res[j].x + lc_reduce(acc[j][0], c), c.q); res[j].y = cred(res[j].y + lc_reduce(acc[j][1], c), c.q); }
    }
    const size_t o = row.ro + w;
#pragma unroll
    for (int j = 0; j < NC; ++j) rh_st2(p.out[j] + o, res[j], nt);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
static const unsigned BGV_RINGS = 1u << RH_RING_STANDARD;

extern "C" int rh_bgv_tensor(rh_ring* r, int level, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                             uint64_t* c0, uint64_t* c1, uint64_t* c2, int npoly, const uint64_t* k, const uint64_t* r1, int accumulate) {
  if (int rc = rh_scheme_args(r, level, npoly, BGV_RINGS, 2, "rh_bgv_tensor")) return rc;
  if (!a0 || !a1 || !c0 || !c1 || !c2 || !k || ((b0 == nullptr) != (b1 == nullptr))) return rh_fail(RH_ERR_ARG, "rh_bgv_tensor: null argument");
  if (accumulate < 0 || accumulate > 2) return rh_fail(RH_ERR_ARG, "rh_bgv_tensor: accumulate must be 0 (overwrite), 1 (c0, c1, c2) or 2 (c0, c1; c2 overwritten)");
  if (r1 && !accumulate) return rh_fail(RH_ERR_ARG, "rh_bgv_tensor: an accumulator scalar without accumulate");
  RhScalars s;
  if (int rc = rh_pack_scalars(r, level, k, r1, false, &s, "rh_bgv_tensor")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const bool square = !b0 || (b0 == a0 && b1 == a1);                 // op0 == op1 (:704): the same values with two operands less to read
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const LimbConsts* lc = r->d_consts;
  const int L = level + 1, h = r1 ? 1 : 0;
#define BGV_T(SQ, ACC) bgv_tensor_kernel<SQ, ACC><<<g.grid, 256, 0, st>>>(a0, a1, b0, b1, c0, c1, c2, n, lc, L, s, h, g.nt)
  if (square) { if (accumulate == 0) BGV_T(true, 0); else if (accumulate == 1) BGV_T(true, 1); else BGV_T(true, 2); }
  else { if (accumulate == 0) BGV_T(false, 0); else if (accumulate == 1) BGV_T(false, 1); else BGV_T(false, 2); }
#undef BGV_T
  return rh_launch_ok("bgv_tensor_kernel");
}

extern "C" int rh_bgv_mul_plain(rh_ring* r, int level, const uint64_t* ct0, const uint64_t* ct1, const uint64_t* ct2, const uint64_t* pt,
                                uint64_t* out0, uint64_t* out1, uint64_t* out2, int npoly, const uint64_t* k, const uint64_t* r1, int accumulate) {
  if (int rc = rh_scheme_args(r, level, npoly, BGV_RINGS, 2, "rh_bgv_mul_plain")) return rc;
  if (!pt || !k) return rh_fail(RH_ERR_ARG, "rh_bgv_mul_plain: null argument");
  if (int rc = rh_comps3(ct0, ct1, ct2, out0, out1, out2, "rh_bgv_mul_plain")) return rc;
  if (accumulate < 0 || accumulate > 1) return rh_fail(RH_ERR_ARG, "rh_bgv_mul_plain: accumulate must be 0 or 1");
  if (r1 && !accumulate) return rh_fail(RH_ERR_ARG, "rh_bgv_mul_plain: an accumulator scalar without accumulate");
  RhScalars s;
  if (int rc = rh_pack_scalars(r, level, k, r1, false, &s, "rh_bgv_mul_plain")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const BgvComps p{{ct0, ct1, ct2}, {out0, out1, out2}};
  const int nc = ct2 ? 3 : ct1 ? 2 : 1, L = level + 1, h = r1 ? 1 : 0;
#define BGV_P(NC, ACC) bgv_mul_plain_kernel<NC, ACC><<<g.grid, 256, 0, st>>>(p, pt, n, r->d_consts, L, s, h, g.nt)
  if (accumulate) { if (nc == 1) BGV_P(1, true); else if (nc == 2) BGV_P(2, true); else BGV_P(3, true); }
  else { if (nc == 1) BGV_P(1, false); else if (nc == 2) BGV_P(2, false); else BGV_P(3, false); }
#undef BGV_P
  return rh_launch_ok("bgv_mul_plain_kernel");
}

extern "C" int rh_bgv_axpby(rh_ring* r, int level, const uint64_t* a, const uint64_t* b, uint64_t* out, int npoly, const uint64_t* r0,
                            const uint64_t* r1, int sub) {
  if (int rc = rh_scheme_args(r, level, npoly, BGV_RINGS, 2, "rh_bgv_axpby")) return rc;
  if (!out || (!a && !b)) return rh_fail(RH_ERR_ARG, "rh_bgv_axpby: null argument");
  if ((a != nullptr) != (r0 != nullptr) || (b != nullptr) != (r1 != nullptr)) return rh_fail(RH_ERR_ARG, "rh_bgv_axpby: every operand comes with its scalar and every scalar with its operand");
  RhScalars s;
  if (int rc = rh_pack_scalars(r, level, r0, r1, false, &s, "rh_bgv_axpby")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1), n = (unsigned)r->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  const int L = level + 1;
#define BGV_A(MODE) bgv_axpby_kernel<MODE><<<g.grid, 256, 0, st>>>(a, b, out, n, r->d_consts, L, s, g.nt)
  if (a && b) { if (sub) BGV_A(1); else BGV_A(0); }
  else if (a) BGV_A(2);
  else if (sub) BGV_A(4);
  else BGV_A(3);
#undef BGV_A
  return rh_launch_ok("bgv_axpby_kernel");
}

extern "C" size_t rh_bgv_plain_combination_table_words(int nterms) { return nterms < 0 ? 0 : bpc_table_words(nterms); }

extern "C" int rh_bgv_plain_combination(rh_ring* r, int level, int nterms, const uint64_t* const* x, const int* x_rows, const uint64_t* const* m,
                                        const uint64_t* c, const uint64_t* c_scalar, uint64_t* out0, uint64_t* out1, uint64_t* out2, int npoly,
                                        uint64_t* table, size_t table_words) {
  const char* who = "rh_bgv_plain_combination";
  if (int rc = rh_scheme_args(r, level, npoly, BGV_RINGS, 2, who)) return rc;
  if (nterms < 0) return rh_fail(RH_ERR_ARG, "%s: nterms < 0", who);
  if (!out0 || (out2 && !out1) || (c == nullptr) != (c_scalar == nullptr) || (nterms && (!x || !x_rows || !m))) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (nterms && !table) return rh_fail(RH_ERR_ARG, "%s: null table (device scratch of rh_bgv_plain_combination_table_words(nterms) words)", who);
  const int L = level + 1, nc = out2 ? 3 : out1 ? 2 : 1;
  const size_t words = bpc_table_words(nterms), N = (size_t)r->N;
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the table holds %zu words, %d terms need %zu", who, table_words, nterms, words);
  if (int rc = rh_moduli_below(r, L, LC_MODULUS_BITS, LC_CHUNK, who)) return rc;
  u64* outs[3] = {out0, out1, out2};
  RhBlock written[4], read[4];
  for (int j = 0; j < nc; ++j) written[j] = {outs[j], (size_t)npoly * L * N};
  if (int rc = rh_blocks_disjoint(written, nc, who, "two outputs overlap")) return rc;
  const int nw = nterms ? nc + 1 : nc;
  if (nterms) written[nc] = {table, words};
  for (int k = 0; k < nterms; ++k) {
    if (x_rows[k] < L) return rh_fail(RH_ERR_ARG, "%s: term %d holds %d limbs per poly, fewer than level %d needs", who, k, x_rows[k], level);
    if (!m[k]) return rh_fail(RH_ERR_ARG, "%s: term %d has no plaintext", who, k);
    for (int j = 0; j < nc; ++j) {
      if (!x[3 * k + j]) return rh_fail(RH_ERR_ARG, "%s: term %d has no component %d", who, k, j);
      read[j] = {x[3 * k + j], (size_t)npoly * (size_t)x_rows[k] * N};
    }
    read[nc] = {m[k], (size_t)L * N};
    if (int rc = rh_blocks_ok(written, nw, read, nc + 1, who, "an output (or the table) overlaps a term or its plaintext: the sum is not computed in place")) return rc;
  }
  if (c) {
    read[0] = {c, (size_t)L * N};
    if (int rc = rh_blocks_ok(written, nw, read, 1, who, "an output (or the table) overlaps the constant")) return rc;
  }
  if (nterms) if (int rc = rh_blocks_ok(written, nc, written + nc, 1, who, "an output overlaps the table")) return rc;
  RhScalars s;
  if (int rc = rh_pack_scalars(r, level, c_scalar, nullptr, false, &s, who, "constant's scalar")) return rc;
  const unsigned rows = (unsigned)npoly * (unsigned)L;
  const RhStreamGrid g = rh_stream_begin(r, rows);
  hipStream_t st = rh_stream(r);
  if (nterms) {
    RhStage* stage;
    if (int rc = rh_stage_slot(words, &stage, who)) return rc;
    for (int k = 0; k < nterms; ++k) {
      u64* e = stage->h + (size_t)k * BPC_TERM_WORDS;
      for (int j = 0; j < 3; ++j) e[j] = j < nc ? (u64)(uintptr_t)x[3 * k + j] : 0;
      e[3] = (u64)x_rows[k];
      e[4] = (u64)(uintptr_t)m[k];
    }
    if (int rc = rh_stage_upload(stage, table, words, st, who)) return rc;
  }
  if (rows == 0) return RH_OK;
  const BgvComps p{{nullptr, nullptr, nullptr}, {out0, out1, out2}};
  const unsigned n = (unsigned)r->N;
#define BGV_PC(NC) bgv_plain_combination_kernel<NC><<<g.grid, 256, 0, st>>>(p, table, nterms, c, n, r->d_consts, L, s, g.nt)
  if (nc == 1) BGV_PC(1); else if (nc == 2) BGV_PC(2); else BGV_PC(3);
#undef BGV_PC
  return rh_launch_ok("bgv_plain_combination_kernel");
}

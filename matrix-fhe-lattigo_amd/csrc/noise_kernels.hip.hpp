// noise_kernels.hip.hpp -- the kernels of noise.hip: exact centred moments of coefficient-domain polys, and the phase of gadget ciphertexts.
//
// ---- moments ------------------------------------------------------------------------------------------------------------------------------------
// A coefficient is never rebuilt as a multiword integer.  Its residues under the L moduli m_0 .. m_{L-1} (the limbs of Q, then those of P) give the
// mixed-radix (Garner) digits d_0 .. d_{L-1}, 0 <= d_i < m_i, of v = CRT(residues) = sum_i R_i d_i with R_i = m_0 ... m_{i-1}.  The order of the
// digit vectors read from the top is the order of the integers, so v >= floor(M / 2) is a digit comparison, and with c the 0 / 1 flag of it
//   x = v - c M,   sum x = sum_i R_i D_i - M sum c,   sum x^2 = sum_{i <= j} (2 - [i = j]) R_i R_j P_ij - 2 M sum_i R_i C_i + M^2 sum c
// where D_i = sum d_i, C_i = sum c d_i and P_ij = sum d_i d_j over the lanes.  With two more "digits", d_L = 1 and d_{L+1} = c, all of them are
// pair sums P_ij over L + 2 rows: the kernel emits every P_ij, i <= j <= L + 1, as a 192-bit integer (d < 2^61 and at most 2^19 lanes: < 2^141), and
// the digit vectors of the smallest and the largest |x| (|x| = M - v on a centred lane: the digits m_i - 1 - d_i, plus one).  The host multiplies
// by the R_i.  Integer sums only: the result does not depend on the launch geometry.
#pragma once
#include "ring_types.hip.hpp"
#include "lc_reduce.hip.hpp"
#include "stream_kernels.hip.hpp"

#define NOISE_MAX_PPT 9          // pair sums per thread: (64 + 2) (64 + 3) / 2 = 2211 pairs over 256 threads

// the tables of one (Q level, P level) basis, one device block: consts | garner | rmod | half | pairs
struct NoiseTables {
  const LimbConsts* c;   // (L) the limbs of Q, then those of P
  const u64* garner;     // (L) R_j^-1 mod m_j, Montgomery form
  const u64* rmod;       // (L, L) R_i mod m_j at [j * L + i], i < j, Montgomery form
  const u64* half;       // (L) the mixed-radix digits of floor(M / 2)
  const u64* pairs;      // (NP) pair k as i | j << 8: the upper triangle of (L + 2)^2, row-major
};
struct NoiseMomArgs {
  const u64* q; const u64* p;      // row (poly, limb) at (poly * q_rows + limb) * N words; p likewise (NULL without P)
  int q_rows, p_rows, LQ, L;       // L = LQ + LP
  unsigned N, n, gap;              // n = N / gap values per poly: the coefficients 0, gap, 2 gap ...
  unsigned C, CS, nchunks;         // lanes per chunk (a power of two <= 256), row stride of the digit image in LDS (C + 1), chunks per poly
  unsigned NP, W;                  // pair count; words of one partial: 3 NP + 2 L
  u64* part;                       // (npoly, gridDim.x, W)
};

struct Acc192 { u128 lo; u64 hi; };
RH_DEV void acc192_add(Acc192& a, u128 p) { a.lo += p; a.hi += (u64)(a.lo < p); }

// digit vectors, most significant digit last, `stride` words apart: is a < b?
RH_DEV bool noise_less(const u64* a, unsigned sa, const u64* b, unsigned sb, int L) {
  for (int i = L - 1; i >= 0; --i) {
    const u64 x = a[(size_t)i * sa], y = b[(size_t)i * sb];
    if (x != y) return x < y;
  }
  return false;
}

// grid (G, npoly), G <= nchunks; dynamic LDS: (L + 2) CS + 2 L words, then 2 C + 4 ints
template <int PPT> __global__ void __launch_bounds__(256)
noise_moments_kernel(NoiseMomArgs a, NoiseTables tb) {
  extern __shared__ u64 noise_lds[];
  const int L = a.L;
  const unsigned t = threadIdx.x, C = a.C, CS = a.CS;
  u64* dg = noise_lds;                                   // digit i of lane l at dg[i * CS + l]; row L: ones, row L + 1: the centring flag
  u64* best = dg + (size_t)(L + 2) * CS;                 // the smallest |x| so far (L digits), then the largest
  unsigned* idx = (unsigned*)(best + 2 * L);             // tournament: lane of the smallest (C entries), of the largest (C entries)
  int* flag = (int*)(idx + 2 * C);                       // [0]: best holds a value; [1], [2]: this chunk's winner replaces the smallest / largest
  const size_t poly = blockIdx.y;
  if (t == 0) flag[0] = 0;
  Acc192 acc[PPT];
  unsigned pi[PPT], pj[PPT];
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    acc[s].lo = 0; acc[s].hi = 0;
    const unsigned k = t + 256u * s;
    const u64 pr = k < a.NP ? tb.pairs[k] : 0;
    pi[s] = (unsigned)(pr & 0xff) * CS; pj[s] = (unsigned)(pr >> 8) * CS;
  }
  for (unsigned chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {
    __syncthreads();                                     // the last chunk's image is no longer read
    bool centred = false, valid = false;
    if (t < C) {
      const unsigned k = chunk * C + t;
      valid = k < a.n;
      const size_t at = (size_t)k * a.gap;
      for (int j = 0; j < L; ++j) {                      // d_j = (r_j - sum_{i < j} d_i R_i) R_j^-1 mod m_j
        const LimbConsts c = tb.c[j];
        const u64* row = j < a.LQ ? a.q + (poly * a.q_rows + j) * a.N : a.p + (poly * a.p_rows + (j - a.LQ)) * a.N;
        const u64 r = valid ? bred_add(row[at], c.q, c.bred0) : 0;
        u64 s = 0; u128 T = 0; int cnt = 0;
        for (int i = 0; i < j; ++i) {
          T += (u128)dg[(size_t)i * CS + t] * tb.rmod[(size_t)j * L + i];
          if (++cnt == LC_CHUNK) { s = cred(s + lc_reduce(T, c), c.q); T = 0; cnt = 0; }
        }
        s = cred(s + lc_reduce(T, c), c.q);
        const u64 diff = r >= s ? r - s : r + c.q - s;
        dg[(size_t)j * CS + t] = j ? mred(diff, tb.garner[j], c.q, c.qinv) : diff;
      }
      int cmp = 0;                                       // v against floor(M / 2), from the top digit
      for (int i = L - 1; i >= 0 && !cmp; --i) {
        const u64 d = dg[(size_t)i * CS + t], h = tb.half[i];
        cmp = d > h ? 1 : d < h ? -1 : 0;
      }
      centred = valid && cmp >= 0;
      dg[(size_t)L * CS + t] = 1;
      dg[(size_t)(L + 1) * CS + t] = centred ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < PPT; ++s) {
      if (t + 256u * s < a.NP) {
        const u64* x = dg + pi[s]; const u64* y = dg + pj[s];
        for (unsigned l = 0; l < C; ++l) acc192_add(acc[s], (u128)x[l] * y[l]);
      }
    }
    __syncthreads();
    if (t < C) {                                         // |x| in place: M - v = (M - 1 - v) + 1, and M - 1 has the digits m_i - 1
      if (centred) {
        u64 carry = 1;
        for (int i = 0; i < L; ++i) {
          const u64 m = tb.c[i].q;
          u64 v = m - 1 - dg[(size_t)i * CS + t] + carry;
          carry = v == m ? 1 : 0;
          if (carry) v = 0;
          dg[(size_t)i * CS + t] = v;
        }
      }
      idx[t] = idx[C + t] = valid ? t : 0xffffffffu;
    }
    __syncthreads();
    for (unsigned s = C >> 1; s > 0; s >>= 1) {
      if (t < s) {
        unsigned x = idx[t], y = idx[t + s];
        if (y != 0xffffffffu && (x == 0xffffffffu || noise_less(dg + y, CS, dg + x, CS, L))) idx[t] = y;
        x = idx[C + t]; y = idx[C + t + s];
        if (y != 0xffffffffu && (x == 0xffffffffu || noise_less(dg + x, CS, dg + y, CS, L))) idx[C + t] = y;
      }
      __syncthreads();
    }
    if (t == 0) {                                        // every chunk holds one valid lane at least
      flag[1] = !flag[0] || noise_less(dg + idx[0], CS, best, 1, L);
      flag[2] = !flag[0] || noise_less(best + L, 1, dg + idx[C], CS, L);
      flag[0] = 1;
    }
    __syncthreads();
    if (t < (unsigned)L) {
      if (flag[1]) best[t] = dg[(size_t)t * CS + idx[0]];
      if (flag[2]) best[L + t] = dg[(size_t)t * CS + idx[C]];
    }
  }
  __syncthreads();
  u64* out = a.part + (poly * gridDim.x + blockIdx.x) * a.W;
#pragma unroll
  for (int s = 0; s < PPT; ++s) {
    const unsigned k = t + 256u * s;
    if (k < a.NP) { out[3 * (size_t)k] = (u64)acc[s].lo; out[3 * (size_t)k + 1] = (u64)(acc[s].lo >> 64); out[3 * (size_t)k + 2] = acc[s].hi; }
  }
  if (t < 2u * (unsigned)L) out[3 * (size_t)a.NP + t] = best[t];
}

// out[poly] = the sum of the G partials' pair sums, and the smallest / largest of their extreme vectors.  grid (npoly), 256 threads
__global__ void __launch_bounds__(256)
noise_moments_reduce_kernel(const u64* __restrict__ part, u64* __restrict__ out, unsigned G, unsigned NP, unsigned W, int L) {
  __shared__ unsigned lo[256], hi[256];
  const unsigned t = threadIdx.x;
  const u64* p = part + (size_t)blockIdx.x * G * W;
  u64* o = out + (size_t)blockIdx.x * W;
  for (unsigned k = t; k < NP; k += 256) {
    Acc192 s; s.lo = 0; s.hi = 0;
    for (unsigned g = 0; g < G; ++g) {
      const u64* w = p + (size_t)g * W + 3 * (size_t)k;
      acc192_add(s, ((u128)w[1] << 64) | w[0]);
      s.hi += w[2];
    }
    o[3 * (size_t)k] = (u64)s.lo; o[3 * (size_t)k + 1] = (u64)(s.lo >> 64); o[3 * (size_t)k + 2] = s.hi;
  }
  const u64* v = p + 3 * (size_t)NP;                      // partial g: its smallest at v + g W, its largest at v + g W + L
  unsigned a = 0xffffffffu, b = 0xffffffffu;
  for (unsigned g = t; g < G; g += 256) {
    if (a == 0xffffffffu || noise_less(v + (size_t)g * W, 1, v + (size_t)a * W, 1, L)) a = g;
    if (b == 0xffffffffu || noise_less(v + (size_t)b * W + L, 1, v + (size_t)g * W + L, 1, L)) b = g;
  }
  lo[t] = a; hi[t] = b;
  __syncthreads();
  for (unsigned s = 128; s > 0; s >>= 1) {
    if (t < s) {
      unsigned x = lo[t], y = lo[t + s];
      if (y != 0xffffffffu && (x == 0xffffffffu || noise_less(v + (size_t)y * W, 1, v + (size_t)x * W, 1, L))) lo[t] = y;
      x = hi[t]; y = hi[t + s];
      if (y != 0xffffffffu && (x == 0xffffffffu || noise_less(v + (size_t)x * W + L, 1, v + (size_t)y * W + L, 1, L))) hi[t] = y;
    }
    __syncthreads();
  }
  if (t < (unsigned)L) {
    o[3 * (size_t)NP + t] = v[(size_t)lo[0] * W + t];
    o[3 * (size_t)NP + L + t] = v[(size_t)hi[0] * W + L + t];
  }
}

// ---- rh_rlwe_gadget_phase: the phase of many gadget ciphertexts in one launch (core/rlwe/utils.go:51-102 up to the INTT) -----------------------------
// Output poly o is one (key, power-of-two index j): on every limb of Q and of P
//   out = sum over the key's RNS digits i of (Value[i][j][0] + Value[i][j][1] sk) [- pt s_o on the limbs of Q],   s_o = MForm(P 2^(j pw2)),
// the canonical residue the reference's MulCoeffsMontgomeryThenAdd, Add, MulScalarBigint / MulScalar and Sub reach.  The products are summed in
// 128 bits and reduced once per LC_CHUNK terms (lc_reduce.hip.hpp); every row of the key is read once.
// rowtab: `stride` words per output poly: the key's Q table address, its P table address, the rows of the key (host check only), the secret,
// the plaintext (NOISE_NO_PT: none), the term count m, m_max row numbers (the first m read), then s_o per limb of Q.
// A key table is (rows, 2, LQ | LP, N): component 0 of row r at (2 r LQ + limb) n words, component 1 LQ rows further.
// sk: (nsk, LQ | LP, N), pt: (npt, LQ, N), NTT domain, Montgomery form.  out: (outs, LQ | LP, N).  grid (outs * (LQ + LP), chunks)
#define NOISE_NO_PT 0xffffffffffffffffull
#define NOISE_PHASE_HEAD 6
struct GadgetPhaseArgs { const u64* skQ; const u64* skP; const u64* ptQ; u64* outQ; u64* outP; const u64* rowtab; unsigned stride, m_max; };

__global__ void __launch_bounds__(256)
rlwe_gadget_phase_kernel(GadgetPhaseArgs p, unsigned n, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP, int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, StreamRowQP::RowLen{n});
  const u64* rt = p.rowtab + (size_t)r.poly * p.stride;
  const int Lr = r.inQ ? LQ : LP;
  const u64* tab = lc_block(r.inQ ? rt[0] : rt[1]);
  const u64* sk = (r.inQ ? p.skQ : p.skP) + ((size_t)rt[3] * Lr + r.l) * n;
  const unsigned m = (unsigned)rt[5];
  const u64 s = r.inQ && rt[4] != NOISE_NO_PT ? rt[NOISE_PHASE_HEAD + p.m_max + r.l] : 0;
  const u64* pt = s ? p.ptQ + ((size_t)rt[4] * LQ + r.l) * n : nullptr;
  u64* out = (r.inQ ? p.outQ : p.outP) + r.ro;
  const LimbConsts c = r.c;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const ulonglong2 sv = rh_ld2(sk + 2 * (size_t)i, false);
    u128 Tx = 0, Ty = 0;
    u64 bx = 0, by = 0;
    unsigned cnt = 0;
    for (unsigned k = 0; k < m; ++k) {
      const u64* b = tab + ((size_t)rt[NOISE_PHASE_HEAD + k] * 2 * Lr + r.l) * n;
      const ulonglong2 bv = rh_ld2(b + 2 * (size_t)i, nt), av = rh_ld2(b + (size_t)Lr * n + 2 * (size_t)i, nt);
      bx = cred(bx + bv.x, c.q); by = cred(by + bv.y, c.q);
      Tx += (u128)av.x * sv.x; Ty += (u128)av.y * sv.y;
      if (++cnt == LC_CHUNK) {
        bx = cred(bx + lc_reduce(Tx, c), c.q); by = cred(by + lc_reduce(Ty, c), c.q);
        Tx = 0; Ty = 0; cnt = 0;
      }
    }
    bx = cred(bx + lc_reduce(Tx, c), c.q); by = cred(by + lc_reduce(Ty, c), c.q);
    if (s) {
      const ulonglong2 pv = rh_ld2(pt + 2 * (size_t)i, false);
      const u64 tx = mred(pv.x, s, c.q, c.qinv), ty = mred(pv.y, s, c.q, c.qinv);
      bx = bx >= tx ? bx - tx : bx + c.q - tx;
      by = by >= ty ? by - ty : by + c.q - ty;
    }
    rh_st2(out + 2 * (size_t)i, make_ulonglong2(bx, by), nt);
  }
}

// blindrot_kernels.hip.hpp -- the accumulator loop of a blind rotation (core/rgsw/blindrot/evaluator.go:134-229, Algorithm 3 of eprint 2022/198)
// as ONE kernel: a workgroup owns one accumulator (c0, c1) of a single-modulus ring of degree 64 .. 2048 and walks that accumulator's program,
// a list of external products with RGSW keys and of key-switched automorphisms, from its first op to its last.
//
// Replaces, per op, the launch sequences of rgsw.Evaluator.ExternalProduct (core/rgsw/evaluator.go:42-186, levelQ = 0, levelP = -1, pw2 > 0: the
// 32-bit branch :82-117 and the Montgomery branch :119-186 both end in the canonical residue of sum_d NTT(digit_d) * key_d * 2^-64) and of
// rlwe.Evaluator.Automorphism (core/rlwe/evaluator_automorphism.go:14-60: GadgetProduct, ringQ.Add, AutomorphismNTTWithIndex).
//
// Layout.  Thread x owns coefficients x + 256 k, k < PER = max(1, N / 256), of both components: the accumulator, the running sums and the
// coefficient-domain polynomial whose digits are being taken live in registers.  LDS holds the one transform buffer (N words) and, for N <= 1024,
// the ring's forward and inverse twiddle tables (32 N bytes; N = 2048 reads them from the caches: 80 KiB would need the large-LDS opt-in).
// The multiply-accumulate is point-wise, so key rows go from global memory straight to the registers of the thread that needs them; the loads are
// issued before the digit's transform and land during it.
//
// Control flow is uniform in the workgroup: ops, op counts and bounds are read from the same words by every thread, butterfly loops run over
// the units of a stage with the barrier outside, so a workgroup with fewer butterflies than threads (N = 64 .. 256) reaches every barrier.
#pragma once
#include "ring_types.hip.hpp"

#define BR_THREADS 256
#define BR_MAX_GALOIS 16
#define BR_MIN_LOGN 6
#define BR_MAX_LOGN 11
struct BrGalois { u32 g[BR_MAX_GALOIS]; };          // Galois element of each slot of the automorphism key table, already taken modulo 2N

// the butterflies of ntt_kernels.hip.hpp's ShoupPolicy: forward U < 8q, V any -> both < 8q; inverse U, V < 4q -> both < 4q
RH_DEV void br_fwd(u64& U, u64& V, const tw2 w, u64 nq, u64 q4) {
  const u64 u = csub(U, q4);
  const u64 X = shoup_mul_acc(V, w.w, w.wp, nq, u);
  V = ((u << 1) + q4) - X;
  U = X;
}
RH_DEV void br_inv(u64& U, u64& V, const tw2 w, u64 nq, u64 q4) {
  const u64 d = U + q4 - V;
  U = csub(U + V, q4);
  V = shoup_mul(d, w.w, w.wp, nq);
}

// In-LDS transforms over buf[0 .. N), stage numbering of ring/ntt.go (forward stage s: m = 2^s blocks, RootsForward[m + i]; inverse t = 1, 2, 4 ..:
// RootsBackward[h + i]).  Two stages per pass: a thread takes the four points of a radix-4 unit through both in registers, which halves the
// barriers and the LDS round trips of a workgroup that has one wave per SIMD and nothing to hide them behind; an odd log2(N) leaves one radix-2
// stage (the first forward, the last inverse).  Called by every thread with buf written and a barrier passed; return with a barrier passed.
RH_DEV void br_ntt(u64* buf, const tw2* tw, int logN, u64 nq, u64 q4) {
  const int half = 1 << (logN - 1), quarter = half >> 1;
  int s = 0;
  if (logN & 1) {
    for (int bf = threadIdx.x; bf < half; bf += BR_THREADS) {
      u64 U = buf[bf], V = buf[bf + half];
      br_fwd(U, V, tw[1], nq, q4);
      buf[bf] = U; buf[bf + half] = V;
    }
    __syncthreads();
    s = 1;
  }
  for (; s < logN; s += 2) {
    const int lt = logN - 2 - s;                                     // log2 of the second stage's stride
    for (int u = threadIdx.x; u < quarter; u += BR_THREADS) {
      const int i = u >> lt, j = (i << (lt + 2)) + (u & ((1 << lt) - 1));
      u64 x0 = buf[j], x1 = buf[j + (1 << lt)], x2 = buf[j + (2 << lt)], x3 = buf[j + (3 << lt)];
      const tw2 w = tw[(1 << s) + i];
      br_fwd(x0, x2, w, nq, q4);
      br_fwd(x1, x3, w, nq, q4);
      br_fwd(x0, x1, tw[(2 << s) + 2 * i], nq, q4);
      br_fwd(x2, x3, tw[(2 << s) + 2 * i + 1], nq, q4);
      buf[j] = x0; buf[j + (1 << lt)] = x1; buf[j + (2 << lt)] = x2; buf[j + (3 << lt)] = x3;
    }
    __syncthreads();
  }
}
RH_DEV void br_intt(u64* buf, const tw2* tw, int logN, u64 nq, u64 q4) {
  const int half = 1 << (logN - 1), quarter = half >> 1;
  int lt = 0;
  for (; lt + 1 < logN; lt += 2) {
    const int h = half >> lt;                                        // first stage: h blocks of 2t, t = 2^lt
    for (int u = threadIdx.x; u < quarter; u += BR_THREADS) {
      const int i = u >> lt, j = (i << (lt + 2)) + (u & ((1 << lt) - 1));
      u64 x0 = buf[j], x1 = buf[j + (1 << lt)], x2 = buf[j + (2 << lt)], x3 = buf[j + (3 << lt)];
      br_inv(x0, x1, tw[h + 2 * i], nq, q4);
      br_inv(x2, x3, tw[h + 2 * i + 1], nq, q4);
      const tw2 w = tw[(h >> 1) + i];
      br_inv(x0, x2, w, nq, q4);
      br_inv(x1, x3, w, nq, q4);
      buf[j] = x0; buf[j + (1 << lt)] = x1; buf[j + (2 << lt)] = x2; buf[j + (3 << lt)] = x3;
    }
    __syncthreads();
  }
  if (lt < logN) {                                                   // odd log2(N): the last stage, t = N / 2, one block
    for (int bf = threadIdx.x; bf < half; bf += BR_THREADS) {
      u64 U = buf[bf], V = buf[bf + half];
      br_inv(U, V, tw[1], nq, q4);
      buf[bf] = U; buf[bf + half] = V;
    }
    __syncthreads();
  }
}

// out0 += <digits(INTT(x)), key[.][0]>, out1 += <digits(INTT(x)), key[.][1]>: one component's share of an external product, or the gadget product
// of a key switch.  key: [digit][component < 2][N], NTT domain, Montgomery form.  x, out0, out1: this thread's PER coefficients, canonical.
template <int PER>
RH_DEV void br_gadget(const u64 (&x)[PER], u64 (&out0)[PER], u64 (&out1)[PER], const u64* __restrict__ key, u64* buf, const tw2* twf,
                      const tw2* twi, const LimbConsts& c, int logN, int pw2, int digits) {
  const u32 N = 1u << logN;
  const u64 q4 = 4 * c.q, mask = ((u64)1 << pw2) - 1;
  u64 t[PER];
  __syncthreads();                                                   // whoever read buf last is done with it
#pragma unroll
  for (int k = 0; k < PER; ++k) { const u32 j = threadIdx.x + BR_THREADS * k; if (j < N) buf[j] = x[k]; }
  __syncthreads();
  br_intt(buf, twi, logN, c.nq, q4);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const u32 j = threadIdx.x + BR_THREADS * k;
    t[k] = j < N ? canon4(shoup_mul(buf[j], c.ninv_w, c.ninv_wp, c.nq), c.q) : 0;
  }
  for (int d = 0; d < digits; ++d) {
    u64 k0[PER], k1[PER];
    const u64* row = key + ((size_t)d * 2 << logN);
#pragma unroll
    for (int k = 0; k < PER; ++k) {                                  // the key rows of this digit: in flight during the transform
      const u32 j = threadIdx.x + BR_THREADS * k;
      k0[k] = j < N ? row[j] : 0;
      k1[k] = j < N ? row[N + j] : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) { const u32 j = threadIdx.x + BR_THREADS * k; if (j < N) buf[j] = (t[k] >> (d * pw2)) & mask; }   // ring.MaskVec
    __syncthreads();
    br_ntt(buf, twf, logN, c.nq, q4);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const u32 j = threadIdx.x + BR_THREADS * k;
      if (j < N) {
        const u64 w = canon8(buf[j], c.q);
        out0[k] = cred(out0[k] + mred(w, k0[k], c.q, c.qinv), c.q);  // MulCoeffsMontgomeryThenAdd
        out1[k] = cred(out1[k] + mred(w, k1[k], c.q, c.qinv), c.q);
      }
    }
  }
}

// x[j] = x[index(j)], index(j) = bitrev(((g (2 bitrev(j) + 1) mod 2N) - 1) / 2): AutomorphismNTTIndex (ring/automorphism.go:12-35)
template <int PER>
RH_DEV void br_permute(u64 (&x)[PER], u64* buf, int logN, u32 g) {
  const u32 N = 1u << logN, mask = 2 * N - 1;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) { const u32 j = threadIdx.x + BR_THREADS * k; if (j < N) buf[j] = x[k]; }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const u32 j = threadIdx.x + BR_THREADS * k;
    if (j < N) x[k] = buf[rh_brev((((g * (2 * rh_brev(j, logN) + 1)) & mask) - 1) >> 1, logN)];
  }
}

// Program: accumulator b runs ops[off[b] .. off[b + 1]).  op >= 0: external product with RGSW key `op`; op < 0: automorphism with key slot -op - 1.
// An op or an offset outside the tables is skipped, never dereferenced (the entry point checks what it can see from the host: the counts).
// rgsw: [key][k < 2][digit][component < 2][N]; gal: [slot][digit][component < 2][N].  TWL: the twiddle tables are staged into LDS.
template <int PER, bool TWL>
__global__ void __launch_bounds__(BR_THREADS)
blindrot_core_kernel(u64* c0, u64* c1, const u64* __restrict__ rgsw, int nkeys, const u64* __restrict__ gal, BrGalois ge, int ngal,
                     const int* __restrict__ off, const int* __restrict__ ops, int nops, const tw2* __restrict__ twf_g,
                     const tw2* __restrict__ twi_g, const LimbConsts* __restrict__ consts, int logN, int pw2, int digits) {
  __shared__ u64 buf[BR_THREADS * PER];
  __shared__ tw2 tws[TWL ? 2 * BR_THREADS * PER : 1];
  const u32 N = 1u << logN;
  const LimbConsts c = consts[0];
  const tw2 *twf = twf_g, *twi = twi_g;
  if (TWL) {
    for (u32 j = threadIdx.x; j < N; j += BR_THREADS) { tws[j] = twf_g[j]; tws[N + j] = twi_g[j]; }
    twf = tws; twi = tws + N;                                        // the first barrier of the first op orders these writes
  }
  const size_t base = (size_t)blockIdx.x << logN;
  u64 a0[PER], a1[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const u32 j = threadIdx.x + BR_THREADS * k;
    a0[k] = j < N ? c0[base + j] : 0;
    a1[k] = j < N ? c1[base + j] : 0;
  }
  int pc = off[blockIdx.x], end = off[blockIdx.x + 1];
  if (pc < 0) pc = 0;
  if (end > nops) end = nops;
  const size_t krow = (size_t)digits * 2 << logN;                    // words of one gadget ciphertext
  for (; pc < end; ++pc) {
    const int op = ops[pc];
    const bool is_auto = op < 0;
    const int idx = is_auto ? -(op + 1) : op;
    if (idx >= (is_auto ? ngal : nkeys)) continue;
    u64 o0[PER], o1[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) { o0[k] = 0; o1[k] = 0; }
    if (!is_auto) {                                                  // (core/rgsw/evaluator.go:101-116, :143-185)
      br_gadget<PER>(a0, o0, o1, rgsw + (size_t)idx * 2 * krow, buf, twf, twi, c, logN, pw2, digits);
      br_gadget<PER>(a1, o0, o1, rgsw + ((size_t)idx * 2 + 1) * krow, buf, twf, twi, c, logN, pw2, digits);
    } else {                                                         // (core/rlwe/evaluator_automorphism.go:42-56)
      br_gadget<PER>(a1, o0, o1, gal + (size_t)idx * krow, buf, twf, twi, c, logN, pw2, digits);
#pragma unroll
      for (int k = 0; k < PER; ++k) o0[k] = cred(o0[k] + a0[k], c.q);
      br_permute<PER>(o0, buf, logN, ge.g[idx]);
      br_permute<PER>(o1, buf, logN, ge.g[idx]);
    }
#pragma unroll
    for (int k = 0; k < PER; ++k) { a0[k] = o0[k]; a1[k] = o1[k]; }
  }
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const u32 j = threadIdx.x + BR_THREADS * k;
    if (j < N) { c0[base + j] = a0[k]; c1[base + j] = a1[k]; }
  }
}

// ---- the front end of Evaluate (core/rgsw/blindrot/evaluator.go:46-132): mod switch, per-job program, X^b rows ---------------------------------
#define BRP_THREADS 256
#define BRP_MAX_NLWE 2048                           // what the program kernel keeps in LDS: a set index per LWE coefficient
#define BR_OP_SKIP 0x7fffffff                       // an external product with a key no table holds: blindrot_core_kernel skips it
#define BR_WINDOW 10                                // windowSize (keys.go:12-15)
struct BrSlots { int pw[BR_WINDOW + 1]; int mid; }; // ops of Automorphism by GaloisGen^v, 1 <= v <= windowSize (pw[0] unused), and by 2N - GaloisGen

// modSwitchRLWETo2NLvl (:284-307) at level 0: round(x 2^s / q) mod 2^s, half rounding up, as s steps of a binary long division -- the remainder
// stays below q < 2^63, so every step is exact in 64 bits.  x: [ct][component < 2][n]; component 1 is made odd (an even non-zero result ^ 1).
__global__ void __launch_bounds__(BRP_THREADS)
blindrot_mod_switch_kernel(const u64* __restrict__ x, int* __restrict__ out, size_t total, u32 n, u64 q, int s) {
  const size_t i = (size_t)blockIdx.x * BRP_THREADS + threadIdx.x;
  if (i >= total) return;
  u64 r = x[i];
  if (r >= q) r %= q;
  u32 y = 0;
  for (int k = 0; k < s; ++k) {
    r <<= 1;
    const u32 bit = r >= q;
    if (bit) r -= q;
    y = (y << 1) | bit;
  }
  if (2 * r >= q) ++y;
  y &= (1u << s) - 1;
  if (((i / n) & 1) && y != 0 && (y & 1) == 0) y ^= 1;
  out[i] = (int)y;
}

// b of every job: b[j] = a2n[ct_j][0][index_j]; a job outside the samples reads as 0
__global__ void __launch_bounds__(BRP_THREADS)
blindrot_gather_b_kernel(const int* __restrict__ a2n, int ncts, int n, const int* __restrict__ jobs, int njobs, int* __restrict__ b) {
  const int j = blockIdx.x * BRP_THREADS + threadIdx.x;
  if (j >= njobs) return;
  const int ct = jobs[2 * j], index = jobs[2 * j + 1];
  b[j] = (ct >= 0 && ct < ncts && index >= 0 && index < n) ? a2n[(size_t)ct * 2 * n + index] : 0;
}

// inclusive scan of one value per thread over the workgroup; returns with s[] holding the inclusive values and a barrier passed
template <bool MAX>
RH_DEV int brp_scan(int* s, int v) {
  s[threadIdx.x] = v;
  __syncthreads();
  for (int d = 1; d < BRP_THREADS; d <<= 1) {
    const int t = (int)threadIdx.x >= d ? s[threadIdx.x - d] : (MAX ? -1 : 0);
    __syncthreads();
    v = MAX ? (v > t ? v : t) : v + t;
    s[threadIdx.x] = v;
    __syncthreads();
  }
  return v;
}

// The ops that step t of the walk issues around its external products.  The walk of BlindRotateCore visits the discrete-log sets in the order
//   t = 0 .. h - 2: k = -(h - 1) .. -1;   t = h - 1 .. 2 h - 3: k = h - 1 .. 1;   t = 2 h - 2: k = 0        (h = N / 2, T = N - 1 steps)
// with Automorphism(2N - g) before step h - 1 (the look-up of set 2N before it finds nothing and its counter is dropped).  The counter v of
// evaluateFromDiscreteLogSets before step t is (t - p) mod windowSize, p the last step before t with a non-empty set (0 when there is none): a
// non-empty set leaves v = 1, an empty one adds 1, and v = windowSize resets.  k == 1 (step T - 2) always resets, and the last step is called
// with v = 0 and never reaches the window.
struct BrpStep { int pre, post; };                  // the window exponent of the automorphism before / after the external products, 0: none
RH_DEV BrpStep brp_step(int t, int p, int c, int T) {
  BrpStep s{0, 0};
  if (t == T - 1) return s;
  const int vb = (t - (p > 0 ? p : 0)) % BR_WINDOW;
  const bool k1 = t == T - 2;
  if (c > 0) { s.pre = vb; s.post = k1 ? 1 : 0; }
  else { const int v = vb + 1; s.post = (v == BR_WINDOW || k1) ? v : 0; }
  return s;
}

// One workgroup per job (ct, index): the job's vector a (evaluator.go:62-103: the reversal a_0, -a_{n-1}, .., -a_1 of the switched c1, times
// X^index modulo X^n + 1 and 2N) is read through its index map, never stored; its discrete-log sets (getDiscreteLogSets :258-280) are a histogram
// over the walk positions; and the steps of BlindRotateCore (:134-186, evaluateFromDiscreteLogSets :189-229) are written in blindrot_core_kernel's
// encoding into ops[job * stride ..), the tail filled with BR_OP_SKIP; off[job] = job * stride.
//   pos: 2N int32, the walk position of the set of each value of Z_2N (0 and 2N - 1 read as set 0, like 1); negative: an even non-zero value,
//        which raises *flag |= 1 and is filed under set 0.  *flag |= 2: a program longer than stride (the entry point sizes stride so that none is).
__global__ void __launch_bounds__(BRP_THREADS)
blindrot_program_kernel(const int* __restrict__ a2n, int ncts, int n, const int* __restrict__ jobs, const int* __restrict__ pos, BrSlots sl,
                        int logN, int stride, int* __restrict__ off, int* __restrict__ ops, int* flag) {
  __shared__ unsigned short tpos[BRP_MAX_NLWE];
  __shared__ int cnt[1 << BR_MAX_LOGN], cur[1 << BR_MAX_LOGN], sc[BRP_THREADS];
  const int job = blockIdx.x, tid = threadIdx.x;
  const int N = 1 << logN, h = N >> 1, T = N - 1, mask = 2 * N - 1;
  int* my = ops + (size_t)job * stride;
  if (tid == 0) {
    off[job + 1] = (job + 1) * stride;
    if (job == 0) off[0] = 0;
  }
  const int ct = jobs[2 * job], index = jobs[2 * job + 1];
  if (ct < 0 || ct >= ncts || index < 0 || index >= n) {              // uniform in the workgroup: an empty program
    for (int j = tid; j < stride; j += BRP_THREADS) my[j] = BR_OP_SKIP;
    return;
  }
  const int* a = a2n + ((size_t)ct * 2 + 1) * n;
  for (int t = tid; t < T; t += BRP_THREADS) cnt[t] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += BRP_THREADS) {
    int j = i - index;
    const bool neg = j < 0;
    if (neg) j += n;
    int v = j == 0 ? a[0] : -a[n - j];
    if (neg) v = -v;
    int p = pos[v & mask];
    if ((unsigned)p >= (unsigned)T) { atomicOr(flag, p < 0 ? 1 : 4); p = T - 1; }
    tpos[i] = (unsigned short)p;
    atomicAdd(&cnt[p], 1);
  }
  __syncthreads();
  const int S = (T + BRP_THREADS - 1) / BRP_THREADS, t0 = tid * S, t1 = t0 + S < T ? t0 + S : T;
  int last = -1;
  for (int t = t0; t < t1; ++t) if (cnt[t]) last = t;
  brp_scan<true>(sc, last);
  const int carry = tid ? sc[tid - 1] : -1;
  __syncthreads();
  int len = 0, p = carry;
  for (int t = t0; t < t1; ++t) {
    const int c = cnt[t];
    const BrpStep s = brp_step(t, p, c, T);
    len += (t == h - 1) + (s.pre != 0) + c + (s.post != 0);
    if (c) p = t;
  }
  int at = brp_scan<false>(sc, len) - len;
  const int count = sc[BRP_THREADS - 1];
  p = carry;
  for (int t = t0; t < t1; ++t) {
    const int c = cnt[t];
    const BrpStep s = brp_step(t, p, c, T);
    if (t == h - 1) { if (at < stride) my[at] = sl.mid; ++at; }
    if (s.pre) { if (at < stride) my[at] = sl.pw[s.pre]; ++at; }
    cur[t] = at;
    at += c;
    if (s.post) { if (at < stride) my[at] = sl.pw[s.post]; ++at; }
    if (c) p = t;
  }
  if (count > stride && tid == 0) atomicOr(flag, 2);
  for (int j = count + tid; j < stride; j += BRP_THREADS) my[j] = BR_OP_SKIP;
  __syncthreads();
  // the external products of a set in ascending index order: chunks of 256 indices in order, ranked inside a chunk by counting
  for (int c0 = 0; c0 < n; c0 += BRP_THREADS) {
    const int i = c0 + tid;
    const bool have = i < n;
    const int q = have ? tpos[i] : 0;
    if (have) {
      int r = 0;
      for (int i2 = c0; i2 < i; ++i2) r += tpos[i2] == q;
      const int dst = cur[q] + r;
      if (dst < stride) my[dst] = i;
    }
    __syncthreads();
    if (have) atomicAdd(&cur[q], 1);
    __syncthreads();
  }
}

// MForm(X^b) per job and limb (evaluator.go:108, ring.NewMonomialXi): out[job][u][b mod N] = +-2^64 mod q_u, minus for b >= N, zero elsewhere
__global__ void __launch_bounds__(BRP_THREADS)
blindrot_monomials_kernel(const int* __restrict__ b, u64* __restrict__ out, size_t total, int L, int logN, const LimbConsts* __restrict__ consts) {
  const size_t i = (size_t)blockIdx.x * BRP_THREADS + threadIdx.x;
  if (i >= total) return;
  const u32 N = 1u << logN, j = (u32)(i & (N - 1));
  const size_t row = i >> logN;
  const u32 bv = (u32)b[row / (size_t)L] & (2 * N - 1);
  u64 w = 0;
  if (j == (bv & (N - 1))) {
    const LimbConsts c = consts[row % (size_t)L];
    const u64 r = c.nq % c.q;
    w = bv < N ? r : c.q - r;
  }
  out[i] = w;
}

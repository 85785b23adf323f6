// keygen_kernels.hip.hpp -- the kernels of the samplers, the key generator, the encryptor and the decryptor (keygen.hip).
#pragma once
#include "modarith.hip.hpp"
#include "stream_kernels.hip.hpp"
#include "sampler_stream.hip.hpp"

// ---- UniformSampler.Read (ring/sampler_uniform.go:77-101): candidate = word & Mask, accepted when < q -----------------------------------------------
// out: rows of N words, row (poly, limb) at out + (poly * out_rows + limb) * n (out_rows >= L: a strided write into a larger block).
// grid (npoly * L, chunks): one row per blockIdx.x, a lane owns a GROUP of eight coefficients (64 contiguous bytes, four 16-byte stores) and
// computes further blocks only while one of its eight is still rejected.  Substream (call, poly0 + poly, row0 + limb, group).
__global__ void __launch_bounds__(256)
sample_uniform_kernel(SampArgs a, u64* __restrict__ out, int out_rows, unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const u32 limb = blockIdx.x % (u32)L, poly = blockIdx.x / (u32)L;
  const u64 q = consts[limb].q;
  const u64 mask = ~0ull >> __clzll((long long)((q - 1) | 1));          // 2^Len64(q - 1) - 1 (ring/subring.go:94)
  u64* row = out + ((size_t)poly * (size_t)out_rows + limb) * n;
  for (unsigned g = blockIdx.y * blockDim.x + threadIdx.x; g < (n >> 3); g += gridDim.y * blockDim.x) {
    u64 m[5] = {a.call, a.poly0 + poly, a.row0 + limb, g, 0}, w[8], x[8];
    unsigned pending = 0xff;
    while (pending) {
      b2b_block(a.h, m, w);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const u64 c = w[k] & mask;
        if (((pending >> k) & 1) && c < q) { x[k] = c; pending &= ~(1u << k); }
      }
      ++m[4];
    }
#pragma unroll
    for (int k = 0; k < 8; k += 2) rh_st2(row + 8 * (size_t)g + k, make_ulonglong2(x[k], x[k + 1]), nt);
  }
}

// ---- the small-norm samplers: one word per coefficient (block 0 of its group), int32 (npoly, N) out -------------------------------------------------
// GAUSS: the rounded, truncated Gaussian of ring/sampler_gaussian.go:159-172 from the cumulative table T[k] = floor(P(|x| <= k) 2^63),
// k = 0 .. len - 1 (T[len - 1] = 2^63): |x| = #{k : T[k] <= word & (2^63 - 1)}, a branch-free scan of the whole table; negative when bit 63 is set.
// else TERNARY with density P (ring/sampler_ternary.go): non-zero when (word >> 1) < thr = floor(P 2^63); negative when bit 0 is set.
// grid (npoly, chunks); substream (call, poly0 + poly, 0, group)
template <bool GAUSS>
__global__ void __launch_bounds__(256)
sample_small_kernel(SampArgs a, int* __restrict__ out, unsigned n, const u64* __restrict__ table, int len, u64 thr) {
  __shared__ u64 T[1024];
  if (GAUSS) {
    for (int k = threadIdx.x; k < len; k += blockDim.x) T[k] = table[k];
    __syncthreads();
  }
  const u32 poly = blockIdx.x;
  int* row = out + (size_t)poly * n;
  for (unsigned g = blockIdx.y * blockDim.x + threadIdx.x; g < (n >> 3); g += gridDim.y * blockDim.x) {
    const u64 m[5] = {a.call, a.poly0 + poly, 0, g, 0};
    u64 w[8];
    b2b_block(a.h, m, w);
    int x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (GAUSS) {
        const u64 u = w[k] & 0x7fffffffffffffffull;
        int mag = 0;
        for (int j = 0; j < len; ++j) mag += T[j] <= u ? 1 : 0;
        x[k] = (w[k] >> 63) ? -mag : mag;
      } else {
        const int nz = (w[k] >> 1) < thr ? 1 : 0;
        x[k] = (w[k] & 1) ? -nz : nz;
      }
    }
    int4* o = reinterpret_cast<int4*>(row + 8 * (size_t)g);
    o[0] = make_int4(x[0], x[1], x[2], x[3]);
    o[1] = make_int4(x[4], x[5], x[6], x[7]);
  }
}

// ---- lifting small coefficients: Read + ExtendBasisSmallNormAndCenter (ring/sampler_gaussian.go:170-172, ring/ringqp/operations.go) ------------------
// in: int32 (npoly, N).  outQ / outP: rows (poly, limb) at + (poly * rows + limb) * n.  x >= 0 ? x : q - |x| under every limb of Q and of P (the
// canonical 0 for x = 0, |x| reduced by one BRedAdd so that small moduli are served too); ACC: the ReadAndAdd form, out = CRed(out + lift).
// grid (npoly, chunks): a lane owns a coefficient pair and walks the limbs, like the ModUp lift (bootstrap_kernels.hip.hpp).
template <bool ACC>
__global__ void __launch_bounds__(256)
small_lift_kernel(const int* __restrict__ in, u64* outQ, int q_rows, u64* outP, int p_rows, unsigned n, const LimbConsts* __restrict__ constsQ,
                  const LimbConsts* __restrict__ constsP, int LQ, int LP, int nt) {
  const u32 poly = blockIdx.x;
  const int2* src = reinterpret_cast<const int2*>(in + (size_t)poly * n);
  u64* oq = outQ + (size_t)poly * (size_t)q_rows * n;
  u64* op = LP ? outP + (size_t)poly * (size_t)p_rows * n : nullptr;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const int2 x = src[i];
    const u64 ax = (u64)(x.x < 0 ? -(long long)x.x : (long long)x.x), ay = (u64)(x.y < 0 ? -(long long)x.y : (long long)x.y);
    auto put = [&](u64* p, const LimbConsts& c) {
      const u64 q = c.q;
      u64 tx = bred_add(ax, q, c.bred0), ty = bred_add(ay, q, c.bred0);
      if (x.x < 0 && tx) tx = q - tx;
      if (x.y < 0 && ty) ty = q - ty;
      ulonglong2 v = make_ulonglong2(tx, ty);
      if (ACC) { const ulonglong2 o = rh_ld2(p, nt); v.x = cred(o.x + v.x, q); v.y = cred(o.y + v.y, q); }
      rh_st2(p, v, nt);
    };
    for (int l = 0; l < LQ; ++l) put(oq + (size_t)l * n + 2 * (size_t)i, constsQ[l]);
    for (int l = 0; l < LP; ++l) put(op + (size_t)l * n + 2 * (size_t)i, constsP[l]);
  }
}

// ---- rh_rlwe_gadget_encrypt: every row of one or many gadget ciphertexts in one launch -------------------------------------------------------------
// Per row r, limb l of Q then P:   b = CRed(CRed(MForm(e) + (q - MRed(a, skOut))) + MRed(skIn, s))    (the last term only where s != 0)
// which is MForm, MulCoeffsMontgomeryThenSub (core/rlwe/encryptor.go:449-452) and the MulScalarMontgomery + Add of
// AddPolyTimesGadgetVectorToGadgetCiphertext (core/rlwe/gadgetciphertext.go:225-230) on the row's digit limbs.
// e: the NTT of the lifted error, (rows, LQ | LP, N).  tab: (rows, 2, LQ | LP, N); component 1 holds a and is read, component 0 is written.
// skOut: (nkeys, LQ | LP, N), skIn: (nkeys, LQ, N) or, si_shared, (LQ, N) for every key; NTT domain and Montgomery form.  rowtab: rows x (1 + LQ) words: the row's key index, then its
// scalar P 2^(j pw2) per limb of Q in Montgomery form, 0 off the digit.  grid (rows * (LQ + LP), chunks)
struct GadgetEncArgs { const u64* eQ; const u64* eP; u64* tabQ; u64* tabP; const u64* soQ; const u64* soP; const u64* siQ; const u64* rowtab; int si_shared; };

__global__ void __launch_bounds__(256)
rlwe_gadget_encrypt_kernel(GadgetEncArgs p, unsigned n, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP,
                           int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, StreamRowQP::RowLen{n});       // rows of n words: n = 3 * 2^k on 3N rings
  const u64* rt = p.rowtab + (size_t)r.poly * (size_t)(1 + LQ);
  const size_t key = (size_t)rt[0];
  const u64 s = r.inQ ? rt[1 + r.l] : 0;
  const int Lr = r.inQ ? LQ : LP;
  const u64* e = (r.inQ ? p.eQ : p.eP) + r.ro;
  u64* tab = (r.inQ ? p.tabQ : p.tabP) + ((size_t)r.poly * 2 * Lr + r.l) * n;
  const u64* a = tab + (size_t)Lr * n;
  const u64* so = (r.inQ ? p.soQ : p.soP) + (key * Lr + r.l) * n;
  const u64* si = s ? p.siQ + ((p.si_shared ? 0 : key) * LQ + r.l) * n : nullptr;
  const LimbConsts c = r.c;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const ulonglong2 ev = rh_ld2(e + 2 * (size_t)i, nt), av = rh_ld2(a + 2 * (size_t)i, nt), sv = rh_ld2(so + 2 * (size_t)i, false);
    ulonglong2 b;
    b.x = cred(mform(ev.x, c.q, c.bred0, c.bred1) + (c.q - mred(av.x, sv.x, c.q, c.qinv)), c.q);
    b.y = cred(mform(ev.y, c.q, c.bred0, c.bred1) + (c.q - mred(av.y, sv.y, c.q, c.qinv)), c.q);
    if (s) {
      const ulonglong2 iv = rh_ld2(si + 2 * (size_t)i, false);
      b.x = cred(b.x + mred(iv.x, s, c.q, c.qinv), c.q);
      b.y = cred(b.y + mred(iv.y, s, c.q, c.qinv), c.q);
    }
    rh_st2(tab + 2 * (size_t)i, b, nt);
  }
}

// ---- rh_rgsw_encrypt: every row of many RGSW ciphertexts under ONE secret (core/rgsw/encryptor.go:25-118) ---------------------------------------------
// As rlwe_gadget_encrypt_kernel, with a plaintext index apart from the (single) output key and the row's RGSW half: rowtab: rows x (2 + LQ) words:
// the plaintext of the row, the half k of the RGSW value it belongs to, then the scalar P 2^(j pw2) per limb of Q in Montgomery form, 0 off the
// digit.  Every row is an encryption of zero, b = MForm(e) - a sk with a as sampled; AddPolyTimesGadgetVectorToGadgetCiphertext then adds pt s to
// component 0 of a Value[0] row and to component 1 of a Value[1] row: there a + pt s is written over a by the lane that read it.
// pt: (npt, LQ, N), sk: (LQ | LP, N); NTT domain, Montgomery form.  grid (rows * (LQ + LP), chunks)
struct RgswEncArgs { const u64* eQ; const u64* eP; u64* tabQ; u64* tabP; const u64* skQ; const u64* skP; const u64* ptQ; const u64* rowtab; };

__global__ void __launch_bounds__(256)
rgsw_encrypt_kernel(RgswEncArgs p, unsigned n, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP, int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, StreamRowQP::RowLen{n});
  const u64* rt = p.rowtab + (size_t)r.poly * (size_t)(2 + LQ);
  const size_t pi = (size_t)rt[0];
  const bool half1 = rt[1] != 0;
  const u64 s = r.inQ ? rt[2 + r.l] : 0;
  const int Lr = r.inQ ? LQ : LP;
  const u64* e = (r.inQ ? p.eQ : p.eP) + r.ro;
  u64* tab = (r.inQ ? p.tabQ : p.tabP) + ((size_t)r.poly * 2 * Lr + r.l) * n;
  u64* a = tab + (size_t)Lr * n;
  const u64* sk = (r.inQ ? p.skQ : p.skP) + (size_t)r.l * n;
  const u64* pt = s ? p.ptQ + (pi * LQ + r.l) * n : nullptr;
  const LimbConsts c = r.c;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const ulonglong2 ev = rh_ld2(e + 2 * (size_t)i, nt), av = rh_ld2(a + 2 * (size_t)i, nt), sv = rh_ld2(sk + 2 * (size_t)i, false);
    ulonglong2 b;
    b.x = cred(mform(ev.x, c.q, c.bred0, c.bred1) + (c.q - mred(av.x, sv.x, c.q, c.qinv)), c.q);
    b.y = cred(mform(ev.y, c.q, c.bred0, c.bred1) + (c.q - mred(av.y, sv.y, c.q, c.qinv)), c.q);
    if (s) {
      const ulonglong2 pv = rh_ld2(pt + 2 * (size_t)i, false);
      const u64 tx = mred(pv.x, s, c.q, c.qinv), ty = mred(pv.y, s, c.q, c.qinv);
      if (half1) rh_st2(a + 2 * (size_t)i, make_ulonglong2(cred(av.x + tx, c.q), cred(av.y + ty, c.q)), nt);
      else { b.x = cred(b.x + tx, c.q); b.y = cred(b.y + ty, c.q); }
    }
    rh_st2(tab + 2 * (size_t)i, b, nt);
  }
}

// ---- rh_rlwe_encrypt_sk: c0 = -c1 sk + NTT(e) [+ pt] in one launch (core/rlwe/encryptor.go:398-424 with addPtToCt :512-530 folded in) ------------------
// c1: uniform, NTT domain; sk: (L, N) NTT domain, Montgomery form; e: the NTT of the lifted error; pt: NTT domain or null.
// c0 = CRed(CRed((q - MRed(c1, sk)) + e) [+ pt]): MulCoeffsMontgomery, Neg (q - x: q for x = 0, folded by the Add's CRed), Add, Add.
// E: the error is added here (NTT-domain ciphertexts); without it only -c1 sk (coefficient-domain ciphertexts add e and pt after the INTT).
// grid (npoly * L, chunks)
template <bool E>
__global__ void __launch_bounds__(256)
rlwe_encrypt_sk_kernel(const u64* c1, const u64* __restrict__ sk, const u64* e, const u64* pt, u64* c0,
                       unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow r(consts, L, n);
  const u64* s = sk + (size_t)r.limb * n;
  const u64 q = r.c.q, qinv = r.c.qinv;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = r.ro + 2 * (size_t)i;
    const ulonglong2 a = rh_ld2(c1 + o, nt), sv = rh_ld2(s + 2 * (size_t)i, false);
    ulonglong2 b = make_ulonglong2(q - mred(a.x, sv.x, q, qinv), q - mred(a.y, sv.y, q, qinv));
    if (!E) { b.x = cred(b.x, q); b.y = cred(b.y, q); }
    if (E) {
      const ulonglong2 ev = rh_ld2(e + o, nt);
      b.x = cred(b.x + ev.x, q); b.y = cred(b.y + ev.y, q);
      if (pt) { const ulonglong2 pv = rh_ld2(pt + o, nt); b.x = cred(b.x + pv.x, q); b.y = cred(b.y + pv.y, q); }
    }
    rh_st2(c0 + o, b, nt);
  }
}

// ---- rh_rlwe_decrypt: the Horner sum of core/rlwe/decryptor.go:62-83 in one launch, every component read once ----------------------------------------
// DEG 1: out = CRed(MRed(c1, sk) + c0); DEG 2: out = CRed(MRed(CRed(MRed(c2, sk) + c1), sk) + c0).  NTT domain in and out; canonical.
// (the reference keeps the middle sums lazy and reduces once at the end: the canonical result is the same residue)
// grid (npoly * L, chunks)
template <int DEG>
__global__ void __launch_bounds__(256)
rlwe_decrypt_kernel(const u64* c0, const u64* c1, const u64* c2, const u64* __restrict__ sk, u64* out,
                    unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow r(consts, L, n);
  const u64* s = sk + (size_t)r.limb * n;
  const u64 q = r.c.q, qinv = r.c.qinv;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = r.ro + 2 * (size_t)i;
    const ulonglong2 sv = rh_ld2(s + 2 * (size_t)i, false);
    ulonglong2 acc = rh_ld2((DEG == 2 ? c2 : c1) + o, nt);
    if (DEG == 2) {
      const ulonglong2 v = rh_ld2(c1 + o, nt);
      acc.x = cred(mred(acc.x, sv.x, q, qinv) + v.x, q); acc.y = cred(mred(acc.y, sv.y, q, qinv) + v.y, q);
    }
    const ulonglong2 v0 = rh_ld2(c0 + o, nt);
    acc.x = cred(mred(acc.x, sv.x, q, qinv) + v0.x, q); acc.y = cred(mred(acc.y, sv.y, q, qinv) + v0.y, q);
    rh_st2(out + o, acc, nt);
  }
}

// ---- the two products of the public-key encryptor in one launch: ct0 = MRed(u, pk0), ct1 = MRed(u, pk1), u read once (encryptor.go:259-260) ------------
// u: (npoly, L, N) NTT domain (not Montgomery); pk0, pk1: (L, N) NTT domain, Montgomery form, shared by the batch.  grid (npoly * L, chunks)
__global__ void __launch_bounds__(256)
rlwe_mul_pk_kernel(const u64* __restrict__ u, const u64* __restrict__ pk0, const u64* __restrict__ pk1, u64* __restrict__ ct0, u64* __restrict__ ct1,
                   unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow r(consts, L, n);
  const u64 q = r.c.q, qinv = r.c.qinv;
  const size_t ko = (size_t)r.limb * n;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = r.ro + 2 * (size_t)i;
    const ulonglong2 uv = rh_ld2(u + o, nt), a = rh_ld2(pk0 + ko + 2 * (size_t)i, false), b = rh_ld2(pk1 + ko + 2 * (size_t)i, false);
    rh_st2(ct0 + o, make_ulonglong2(mred(uv.x, a.x, q, qinv), mred(uv.y, a.y, q, qinv)), nt);
    rh_st2(ct1 + o, make_ulonglong2(mred(uv.x, b.x, q, qinv), mred(uv.y, b.y, q, qinv)), nt);
  }
}

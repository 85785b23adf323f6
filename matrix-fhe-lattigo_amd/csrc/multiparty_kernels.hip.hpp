// multiparty_kernels.hip.hpp -- the kernels of the multiparty protocols (multiparty.hip): row-streaming kernels on the scaffold of
// stream_kernels.hip.hpp, canonical residues in and out.
#pragma once
#include "modarith.hip.hpp"
#include "stream_kernels.hip.hpp"
#include "lc_reduce.hip.hpp"

// ---- rh_mp_aggregate: out = sum over k < nshares of share_k mod q, every share read once -----------------------------------------------------------
// shares: a device table of nshares block addresses, each block (npoly, L, N) dense.  One cred per addend, so the running sum stays canonical
// and equals the chain of pairwise ring.Add calls (multiparty/keygen_evk.go:213-242 and its siblings) word for word, whatever the moduli.
// MP_AGG_WIDTH loads are in flight together.  out may be one of the shares: a lane reads its pair of every share before it writes it.
// grid (npoly * L, chunks)
#define MP_AGG_WIDTH 4
__global__ void __launch_bounds__(256)
mp_aggregate_kernel(const u64* __restrict__ shares, int nshares, u64* out, unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow r(consts, L, n);
  const u64 q = r.c.q;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = r.ro + 2 * (size_t)i;
    ulonglong2 acc = rh_ld2(lc_block(shares[0]) + o, nt);
    int k = 1;
    for (; k + MP_AGG_WIDTH <= nshares; k += MP_AGG_WIDTH) {
      ulonglong2 x[MP_AGG_WIDTH];
#pragma unroll
      for (int w = 0; w < MP_AGG_WIDTH; ++w) x[w] = rh_ld2(lc_block(shares[k + w]) + o, nt);
#pragma unroll
      for (int w = 0; w < MP_AGG_WIDTH; ++w) { acc.x = cred(acc.x + x[w].x, q); acc.y = cred(acc.y + x[w].y, q); }
    }
    for (; k < nshares; ++k) {
      const ulonglong2 x = rh_ld2(lc_block(shares[k]) + o, nt);
      acc.x = cred(acc.x + x.x, q); acc.y = cred(acc.y + x.y, q);
    }
    rh_st2(out + o, acc, nt);
  }
}

// ---- rh_mp_gadget_share: every row of one party's evaluation-key, Galois-key or public-key shares, for one or many keys, in one launch ------------
// Per row r, limb l of Q then P:   h = CRed(CRed(MForm(e) + MRed(skIn, s)) + (q - MRed(crp, skOut[key])))    (the middle term only where s != 0)
// which is MForm, the digit-limb additions of e + skIn P 2^(j pw2) and MulCoeffsMontgomeryThenSub (multiparty/keygen_evk.go:170-202); a
// public-key share (multiparty/keygen_cpk.go:70-83) is the one-row case with s = 0.  skIn is in Montgomery form and s = MForm(P 2^(j pw2)), so
// MRed(skIn, s) is the Montgomery form of skIn P 2^(j pw2): the residue MulScalarBigint and the repeated MulScalar of the reference reach.
// e: the NTT of the lifted error, crp: the common reference rows, h: the share; all (rows, LQ | LP, N).  skOut: (nkeys, LQ | LP, N), skIn:
// (nkeys, LQ, N) or, si_shared, (LQ, N) for every key.  rowtab: rows x (1 + LQ) words, the layout of rh_rlwe_gadget_encrypt's.
// grid (rows * (LQ + LP), chunks)
struct MpShareArgs { const u64* eQ; const u64* eP; const u64* crpQ; const u64* crpP; u64* hQ; u64* hP; const u64* soQ; const u64* soP; const u64* siQ; const u64* rowtab; int si_shared; };

__global__ void __launch_bounds__(256)
mp_gadget_share_kernel(MpShareArgs p, unsigned n, int logN, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP,
                       int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, logN);
  const u64* rt = p.rowtab + (size_t)r.poly * (size_t)(1 + LQ);
  const size_t key = (size_t)rt[0];
  const u64 s = r.inQ ? rt[1 + r.l] : 0;
  const int Lr = r.inQ ? LQ : LP;
  const u64* e = (r.inQ ? p.eQ : p.eP) + r.ro;
  const u64* a = (r.inQ ? p.crpQ : p.crpP) + r.ro;
  u64* h = (r.inQ ? p.hQ : p.hP) + r.ro;
  const u64* so = (r.inQ ? p.soQ : p.soP) + ((key * Lr + r.l) << logN);
  const u64* si = s ? p.siQ + (((p.si_shared ? 0 : key) * LQ + r.l) << logN) : nullptr;
  const LimbConsts c = r.c;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const ulonglong2 ev = rh_ld2(e + 2 * (size_t)i, nt), av = rh_ld2(a + 2 * (size_t)i, nt), sv = rh_ld2(so + 2 * (size_t)i, false);
    ulonglong2 b = make_ulonglong2(mform(ev.x, c.q, c.bred0, c.bred1), mform(ev.y, c.q, c.bred0, c.bred1));
    if (s) {
      const ulonglong2 iv = rh_ld2(si + 2 * (size_t)i, false);
      b.x = cred(b.x + mred(iv.x, s, c.q, c.qinv), c.q);
      b.y = cred(b.y + mred(iv.y, s, c.q, c.qinv), c.q);
    }
    b.x = cred(b.x + (c.q - mred(av.x, sv.x, c.q, c.qinv)), c.q);
    b.y = cred(b.y + (c.q - mred(av.y, sv.y, c.q, c.qinv)), c.q);
    rh_st2(h + 2 * (size_t)i, b, nt);
  }
}

// ---- rh_mp_relin_round_one: both components of every row of a party's round-one share, the CRP read once (multiparty/keygen_relin.go:130-222) -------
//   h0 = CRed(CRed(NTT(e0) + MRed(skI, s)) + (q - MRed(u, a)))    (the middle term on the row's digit limbs, s != 0)
//   h1 = CRed(NTT(e1) + MRed(sk, a))
// The errors are NOT taken to Montgomery form here and the CRP a is read as plain residues, as the reference has it: u and sk are in Montgomery
// form, so MRed(u, a) = u a and MRed(sk, a) = sk a are plain.  skI = IMForm(sk), plain, and s = MForm(P 2^(j pw2)), the gadget table's scalar, so
// MRed(skI, s) = skI s 2^64 2^-64 = sk P 2^(j pw2): the residue of IMForm(MulScalarBigint(sk, P)) after j MulScalar by 2^pw2 (:145-151, :220).
// e0, e1, a: (rows, LQ | LP, N); h: (rows, 2, LQ | LP, N); u, sk: (LQ | LP, N); skI: (LQ, N).  rowtab: rows x (1 + LQ) words, word 0 unused.
// grid (rows * (LQ + LP), chunks)
struct MpRelinOneArgs { RhQPc e0e1; const u64* crpQ; const u64* crpP; u64* hQ; u64* hP; const u64* uQ; const u64* uP; const u64* skQ; const u64* skP; const u64* skIQ; const u64* rowtab; };

__global__ void __launch_bounds__(256)
mp_relin_round_one_kernel(MpRelinOneArgs p, unsigned n, int logN, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP,
                          int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, logN);
  const u64 s = r.inQ ? p.rowtab[(size_t)r.poly * (size_t)(1 + LQ) + 1 + r.l] : 0;
  const int Lr = r.inQ ? LQ : LP;
  const u64* e0 = r.of(p.e0e1, 0);
  const u64* e1 = r.of(p.e0e1, 1);
  const u64* a = (r.inQ ? p.crpQ : p.crpP) + r.ro;
  u64* h0 = (r.inQ ? p.hQ : p.hP) + (((size_t)r.poly * 2 * Lr + r.l) << logN);
  u64* h1 = h0 + ((size_t)Lr << logN);
  const u64* u = (r.inQ ? p.uQ : p.uP) + r.po;
  const u64* sk = (r.inQ ? p.skQ : p.skP) + r.po;
  const u64* ski = s ? p.skIQ + r.po : nullptr;
  const LimbConsts c = r.c;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t w = 2 * (size_t)i;
    const ulonglong2 av = rh_ld2(a + w, nt), uv = rh_ld2(u + w, false), sv = rh_ld2(sk + w, false);
    ulonglong2 b0 = rh_ld2(e0 + w, nt), b1 = rh_ld2(e1 + w, nt);
    if (s) {
      const ulonglong2 iv = rh_ld2(ski + w, false);
      b0.x = cred(b0.x + mred(iv.x, s, c.q, c.qinv), c.q);
      b0.y = cred(b0.y + mred(iv.y, s, c.q, c.qinv), c.q);
    }
    b0.x = cred(b0.x + (c.q - mred(uv.x, av.x, c.q, c.qinv)), c.q);
    b0.y = cred(b0.y + (c.q - mred(uv.y, av.y, c.q, c.qinv)), c.q);
    b1.x = cred(b1.x + mred(sv.x, av.x, c.q, c.qinv), c.q);
    b1.y = cred(b1.y + mred(sv.y, av.y, c.q, c.qinv), c.q);
    rh_st2(h0 + w, b0, nt);
    rh_st2(h1 + w, b1, nt);
  }
}

// ---- rh_mp_relin_round_two: out = MRed(r1[0], sk) + NTT(e) + MRed(u - sk, r1[1]) per row (multiparty/keygen_relin.go:231-270) ---------------------------
// Both components of the aggregated round-one share are read once; u - sk = CRed(u + (q - sk)), ringQP.Sub's value (:241), is formed in registers.
// u and sk are in Montgomery form and r1 holds plain residues, so both products are plain, like e.
// r1: (rows, 2, LQ | LP, N); e, out: (rows, LQ | LP, N); u, sk: (LQ | LP, N).  grid (rows * (LQ + LP), chunks)
struct MpRelinTwoArgs { const u64* eQ; const u64* eP; const u64* r1Q; const u64* r1P; u64* outQ; u64* outP; const u64* uQ; const u64* uP; const u64* skQ; const u64* skP; };

__global__ void __launch_bounds__(256)
mp_relin_round_two_kernel(MpRelinTwoArgs p, unsigned n, int logN, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP,
                          int LQ, int LP, int nt) {
  const StreamRowQP r(blockIdx.x, constsQ, constsP, LQ, LP, logN);
  const int Lr = r.inQ ? LQ : LP;
  const u64* e = (r.inQ ? p.eQ : p.eP) + r.ro;
  const u64* x0 = (r.inQ ? p.r1Q : p.r1P) + (((size_t)r.poly * 2 * Lr + r.l) << logN);
  const u64* x1 = x0 + ((size_t)Lr << logN);
  u64* out = (r.inQ ? p.outQ : p.outP) + r.ro;
  const u64* u = (r.inQ ? p.uQ : p.uP) + r.po;
  const u64* sk = (r.inQ ? p.skQ : p.skP) + r.po;
  const u64 q = r.c.q, qinv = r.c.qinv;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t w = 2 * (size_t)i;
    const ulonglong2 a = rh_ld2(x0 + w, nt), b = rh_ld2(x1 + w, nt), ev = rh_ld2(e + w, nt), uv = rh_ld2(u + w, false), sv = rh_ld2(sk + w, false);
    const u64 dx = cred(uv.x + (q - sv.x), q), dy = cred(uv.y + (q - sv.y), q);
    ulonglong2 v;
    v.x = cred(cred(mred(a.x, sv.x, q, qinv) + ev.x, q) + mred(dx, b.x, q, qinv), q);
    v.y = cred(cred(mred(a.y, sv.y, q, qinv) + ev.y, q) + mred(dy, b.y, q, qinv), q);
    rh_st2(out + w, v, nt);
  }
}

// ---- rh_mp_keyswitch_share: out = [acc +] MRed(c1, skA [- skB]) [+ e] on a batch --------------------------------------------------------------------
// The collective key switch's share (multiparty/keyswitch_sk.go:118-149): Sub(skIn, skOut), MulCoeffsMontgomery, Add of the NTT of the error;
// with acc and without skB the secret-key term of the public key switch (multiparty/keyswitch_pk.go); without e the product step of the
// coefficient-domain paths.  skA, skB: (L, N) NTT domain, Montgomery form, shared by the batch; the difference is formed in registers as
// CRed(skA + (q - skB)), ring.Sub's value.  c1: rows (poly, limb) at (poly * c1_rows + limb) * n (a ciphertext above the share's level);
// acc, e, out: dense (npoly, L, N).  out may be acc or e.  grid (npoly * L, chunks)
template <bool SUB, bool ACC, bool ERR>
__global__ void __launch_bounds__(256)
mp_keyswitch_share_kernel(const u64* c1, int c1_rows, const u64* __restrict__ skA, const u64* __restrict__ skB, const u64* acc, const u64* e, u64* out,
                          unsigned n, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamRow r(consts, L, n);
  const size_t ko = (size_t)r.limb * n, co = r.at(c1_rows, n);
  const u64 q = r.c.q, qinv = r.c.qinv;
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = r.ro + 2 * (size_t)i;
    const ulonglong2 cv = rh_ld2(c1 + co + 2 * (size_t)i, nt);
    ulonglong2 d = rh_ld2(skA + ko + 2 * (size_t)i, false);
    if (SUB) {
      const ulonglong2 b = rh_ld2(skB + ko + 2 * (size_t)i, false);
      d.x = cred(d.x + (q - b.x), q); d.y = cred(d.y + (q - b.y), q);
    }
    ulonglong2 v = make_ulonglong2(mred(cv.x, d.x, q, qinv), mred(cv.y, d.y, q, qinv));
    if (ACC) { const ulonglong2 a = rh_ld2(acc + o, nt); v.x = cred(a.x + v.x, q); v.y = cred(a.y + v.y, q); }
    if (ERR) { const ulonglong2 ev = rh_ld2(e + o, nt); v.x = cred(v.x + ev.x, q); v.y = cred(v.y + ev.y, q); }
    rh_st2(out + o, v, nt);
  }
}

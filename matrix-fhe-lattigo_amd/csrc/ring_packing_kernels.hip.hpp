// ring_packing_kernels.hip.hpp -- the element-wise passes of core/rlwe/ring_packing.go around its key switches, fused: one level of Expand
// (:555-575), the two halves of one level of Pack (:726-769, :786-787), and the coefficient maps between the rings of degree N and N / gap that
// Split and Merge are built on (core/rlwe/element.go:250-312, ring/operations.go:380-392).  All on the scaffold of stream_kernels.hip.hpp: one
// (poly, limb) row per blockIdx.x, the row's pairs over blockIdx.y, 16-byte moves.  The gathered operand (the un-permuted output of the key
// switch) is read through rh_galois_index_even / rh_gather2 (paired_gather.hip.hpp): index(2i + 1) = index(2i) ^ 1 holds for EVERY odd element,
// N / n + 1 and 2N - 1 included, because the proof there only uses that gen is odd.
//
// Every intermediate of the reference's sequences is a canonical residue (Add, Sub and MulCoeffsMontgomery end in CRed), so the values below
// are the reference's bits.
#pragma once
#include "paired_gather.hip.hpp"

// One level of Expand for the live prefix ct[0 .. cnt) of a batch of at least 2 cnt polys (ring_packing.go:555-575): with t = tmp[p][index(j)],
//   ct[p][j]       = CRed(c + t)                        c0 + phi(c0)            (:564-565)
//   ct[cnt + p][j] = MRed(CRed(c + q - t), x[l][j])     (c0 - phi(c0)) X^(-2^i)  (:568-573)
// x: the row table X^(-2^i), one row of N words per limb, NTT domain, Montgomery form.   grid: (2 * cnt * L, chunks)
__global__ void __launch_bounds__(256)
expand_step_kernel(u64* ct0, u64* ct1, const u64* tmp0, const u64* tmp1, const u64* __restrict__ x, int logN, u32 gen,
                   const LimbConsts* __restrict__ consts, int L, int cnt, int nt) {
  const u32 per = (u32)cnt * (u32)L;
  const StreamComp sc(per);
  const u32 l = sc.row % (u32)L;
  const LimbConsts c = consts[l];
  const size_t ro = (size_t)sc.row << logN;
  u64* lo = (sc.comp ? ct1 : ct0) + ro;
  u64* hi = lo + ((size_t)per << logN);
  const u64* tmp = (sc.comp ? tmp1 : tmp0) + ro;
  const u64* xr = x + ((size_t)l << logN);
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const ulonglong2 t = rh_gather2(tmp, rh_galois_index_even(i, logN, gen));
    const ulonglong2 v = rh_ld2(lo + 2 * (size_t)i, nt);
    const ulonglong2 w = rh_ld2(xr + 2 * (size_t)i, false);         // the table is read by every poly: default policy
    ulonglong2 a, d;
    a.x = cred(v.x + t.x, c.q); a.y = cred(v.y + t.y, c.q);
    d.x = mred(cred(v.x + c.q - t.x, c.q), w.x, c.q, c.qinv); d.y = mred(cred(v.y + c.q - t.y, c.q), w.y, c.q, c.qinv);
    rh_st2(lo + 2 * (size_t)i, a, nt);
    rh_st2(hi + 2 * (size_t)i, d, nt);
  }
}

// The plan of one level of Pack: entry k = (mode, slot_a, slot_b) names the operands of key switch k among the `nslots` polys of the batch
enum { RP_MODE_A = 0, RP_MODE_B = 1, RP_MODE_AB = 2 };
struct RpEntry { int mode, a, b; };
RH_DEV bool rp_entry_ok(const RpEntry& e, int nslots) {
  return (unsigned)e.mode <= (unsigned)RP_MODE_AB && (unsigned)e.a < (unsigned)nslots && (unsigned)e.b < (unsigned)nslots;
}

// Before the key switch of one level of Pack (ring_packing.go:726-745), with bx = MRed(b, x):
//   AB:  u[k] = CRed(a + q - bx),  a = CRed(a + bx) in place     (:726-737)
//   B:   b = bx in place,  u[k] = bx                             (:726-727, :741, :781)
//   A:   u[k] = a                                                (:762)
// An entry out of range is skipped (the entry refuses such a table before the launch; the kernel never leaves the batch).  grid: (2 * K * L, chunks)
__global__ void __launch_bounds__(256)
pack_combine_kernel(u64* ct0, u64* ct1, u64* u0, u64* u1, const u64* __restrict__ x, const RpEntry* __restrict__ table, int logN,
                    const LimbConsts* __restrict__ consts, int L, int K, int nslots, int nt) {
  const StreamComp sc((u32)K * (u32)L);
  const u32 k = sc.row / (u32)L, l = sc.row % (u32)L;
  const RpEntry e = table[k];
  if (!rp_entry_ok(e, nslots)) return;
  const LimbConsts c = consts[l];
  u64* base = sc.comp ? ct1 : ct0;
  u64* a = base + (((size_t)e.a * L + l) << logN);
  u64* b = base + (((size_t)e.b * L + l) << logN);
  u64* u = (sc.comp ? u1 : u0) + ((size_t)sc.row << logN);
  const u64* xr = x + ((size_t)l << logN);
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const size_t o = 2 * (size_t)i;
    if (e.mode == RP_MODE_A) { rh_st2(u + o, rh_ld2(a + o, nt), nt); continue; }
    const ulonglong2 w = rh_ld2(xr + o, false);
    ulonglong2 bx = rh_ld2(b + o, nt);
    bx.x = mred(bx.x, w.x, c.q, c.qinv); bx.y = mred(bx.y, w.y, c.q, c.qinv);
    if (e.mode == RP_MODE_B) { rh_st2(b + o, bx, nt); rh_st2(u + o, bx, nt); continue; }
    const ulonglong2 v = rh_ld2(a + o, nt);
    ulonglong2 s, d;
    d.x = cred(v.x + c.q - bx.x, c.q); d.y = cred(v.y + c.q - bx.y, c.q);
    s.x = cred(v.x + bx.x, c.q); s.y = cred(v.y + bx.y, c.q);
    rh_st2(u + o, d, nt);
    rh_st2(a + o, s, nt);
  }
}

// After the key switch of one level of Pack: slot[out_k][j] = CRed(slot[out_k][j] +- tmp[k][index(j)]), out_k = slot_b and minus for mode B
// (:786-787), slot_a and plus otherwise (:768-769).   grid: (2 * K * L, chunks)
__global__ void __launch_bounds__(256)
rotate_addsub_q_kernel(u64* ct0, u64* ct1, const u64* tmp0, const u64* tmp1, const RpEntry* __restrict__ table, int logN, u32 gen,
                       const LimbConsts* __restrict__ consts, int L, int K, int nslots, int nt) {
  const StreamComp sc((u32)K * (u32)L);
  const u32 k = sc.row / (u32)L, l = sc.row % (u32)L;
  const RpEntry e = table[k];
  if (!rp_entry_ok(e, nslots)) return;
  const u64 q = consts[l].q;
  const bool minus = e.mode == RP_MODE_B;
  u64* ct = (sc.comp ? ct1 : ct0) + (((size_t)(minus ? e.b : e.a) * L + l) << logN);
  const u64* tmp = (sc.comp ? tmp1 : tmp0) + ((size_t)sc.row << logN);
  RH_FOR_EACH_PAIR(i, 0, 1u << (logN - 1)) {
    const ulonglong2 t = rh_gather2(tmp, rh_galois_index_even(i, logN, gen));
    ulonglong2 v = rh_ld2(ct + 2 * (size_t)i, nt);
    v.x = cred(minus ? v.x + q - t.x : v.x + t.x, q); v.y = cred(minus ? v.y + q - t.y : v.y + t.y, q);
    rh_st2(ct + 2 * (size_t)i, v, nt);
  }
}

// X -> Y = X^gap on coefficient-domain rows of the degree-N ring (element.go:256-268, :302-308): even[i] = in[i gap] and, when odd is given,
// odd[i] = in[i gap + 1] as rows of the degree-N/gap ring, both components in one pass.  With gap = 2 these are the two halves of Split; the
// reference gets the odd half by a multiplication with X^-1 in the NTT domain and a second inverse transform (ring_packing.go:239-241), which
// yields the same canonical residues: (c X^-1)[2i] = c[2i + 1], no wrap.   grid: (2 * npoly * L, chunks); logM = log2(N / gap) >= 1
__global__ void __launch_bounds__(256)
ring_split_kernel(const u64* in0, const u64* in1, u64* even0, u64* even1, u64* odd0, u64* odd1, int logN, int logM, int nt) {
  const StreamComp sc(gridDim.x / 2);
  const u64* in = (sc.comp ? in1 : in0) + ((size_t)sc.row << logN);
  u64* ev = (sc.comp ? even1 : even0) + ((size_t)sc.row << logM);
  u64* od = sc.comp ? odd1 : odd0;
  if (od) od += (size_t)sc.row << logM;
  const int lg = logN - logM;
  RH_FOR_EACH_PAIR(i, 0, 1u << (logM - 1)) {
    ulonglong2 e, o;
    if (lg == 1) {                                                   // words 4i .. 4i+3: two 16-byte loads
      const ulonglong2 a = rh_ld2(in + 4 * (size_t)i, nt), b = rh_ld2(in + 4 * (size_t)i + 2, nt);
      e = make_ulonglong2(a.x, b.x); o = make_ulonglong2(a.y, b.y);
    } else {                                                         // gap >= 4: the pairs (i gap, i gap + 1) are aligned 16-byte words
      const ulonglong2 a = rh_ld2(in + ((2 * (size_t)i) << lg), nt), b = rh_ld2(in + ((2 * (size_t)i + 1) << lg), nt);
      e = make_ulonglong2(a.x, b.x); o = make_ulonglong2(a.y, b.y);
    }
    rh_st2(ev + 2 * (size_t)i, e, nt);
    if (od) rh_st2(od + 2 * (size_t)i, o, nt);
  }
}

// Y = X^gap -> X in the NTT domain (MapSmallDimensionToLargerDimensionNTT, ring/operations.go:380-392), and Merge's sum (ring_packing.go:429-434):
//   out[i gap + w] = even[i]                                        without odd
//   out[i gap + w] = CRed(even[i] + MRed(odd[i], x[l][i gap + w]))  with odd (MulCoeffsMontgomeryThenAdd); x: the row table X^1 of the large ring
// grid: (2 * npoly * L, chunks) over the pairs of the SMALL rows; logM = log2(N / gap) >= 1
__global__ void __launch_bounds__(256)
ring_merge_kernel(const u64* even0, const u64* even1, const u64* odd0, const u64* odd1, const u64* __restrict__ x, u64* out0, u64* out1,
                  int logN, int logM, const LimbConsts* __restrict__ consts, int L, int nt) {
  const StreamComp sc(gridDim.x / 2);
  const u32 l = sc.row % (u32)L;
  const LimbConsts c = consts[l];
  const u64* ev = (sc.comp ? even1 : even0) + ((size_t)sc.row << logM);
  const u64* od = sc.comp ? odd1 : odd0;
  if (od) od += (size_t)sc.row << logM;
  u64* out = (sc.comp ? out1 : out0) + ((size_t)sc.row << logN);
  const u64* xr = x ? x + ((size_t)l << logN) : nullptr;
  const int lg = logN - logM;
  const u32 half = 1u << (lg - 1);                                   // 16-byte words per replicated coefficient
  RH_FOR_EACH_PAIR(i, 0, 1u << (logM - 1)) {
    const ulonglong2 e = rh_ld2(ev + 2 * (size_t)i, nt);
    ulonglong2 o = make_ulonglong2(0, 0);
    if (od) o = rh_ld2(od + 2 * (size_t)i, nt);
    for (u32 s = 0; s < 2; ++s) {
      const u64 ee = s ? e.y : e.x, oo = s ? o.y : o.x;
      const size_t base = (2 * (size_t)i + s) << lg;
      for (u32 w = 0; w < half; ++w) {
        ulonglong2 v = make_ulonglong2(ee, ee);
        if (od) {
          const ulonglong2 xx = rh_ld2(xr + base + 2 * w, false);
          v.x = cred(ee + mred(oo, xx.x, c.q, c.qinv), c.q); v.y = cred(ee + mred(oo, xx.y, c.q, c.qinv), c.q);
        }
        rh_st2(out + base + 2 * w, v, nt);
      }
    }
  }
}

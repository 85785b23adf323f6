// stream_kernels.hip.hpp -- the scaffold of the element-wise "row-streaming" kernels (engine.hip, bfv.hip, bgv.hip, ckks.hip, keyswitch.hip, and
// through paired_gather.hip.hpp inner_sum.hip, ring_packing.hip, lintrans.hip):
// one (poly, limb) row per blockIdx.x so the per-limb constants are wave-uniform, the row's coefficient PAIRS split over blockIdx.y by a
// grid-stride loop, 16-byte loads and stores, non-temporal when the launch's `nt` says so.  The host half -- which grid, which `nt` -- is
// rh_stream_grid (engine_internal.hpp).
#pragma once
#include "ring_types.hip.hpp"

// 16 bytes at p (16-byte aligned); nt: non-temporal (the launch streams past the Infinity Cache), else the default policy
typedef u64 rh_u64x2_t __attribute__((ext_vector_type(2)));
RH_DEV ulonglong2 rh_ld2(const u64* p, bool nt) {
  if (!nt) return *reinterpret_cast<const ulonglong2*>(p);
  const rh_u64x2_t v = __builtin_nontemporal_load(reinterpret_cast<const rh_u64x2_t*>(p));
  return make_ulonglong2(v.x, v.y);
}
RH_DEV void rh_st2(u64* p, const ulonglong2& w, bool nt) {
  if (nt) { rh_u64x2_t v; v.x = w.x; v.y = w.y; __builtin_nontemporal_store(v, reinterpret_cast<rh_u64x2_t*>(p)); }
  else *reinterpret_cast<ulonglong2*>(p) = w;
}

// The row of this workgroup in a launch of (npoly * L, chunks) workgroups over blocks of L limbs per poly
struct StreamRow {
  u32 row, limb, poly;
  LimbConsts c;
  size_t ro;                       // word offset of the row in a dense (npoly, L, n) block
  RH_DEV StreamRow(const LimbConsts* __restrict__ consts, int L, unsigned n)
      : row(blockIdx.x), limb(row % (u32)L), poly(row / (u32)L), c(consts[limb]), ro((size_t)row * n) {}
  // ... in a block with `rows` >= L limbs per poly (a ring.AtLevel view)
  RH_DEV size_t at(int rows, unsigned n) const { return ((size_t)poly * rows + limb) * n; }
};

// Two-component launches, grid (2 * per, chunks): component 0's `per` rows, then component 1's; `row` is the row within the component
struct StreamComp {
  u32 comp, row;
  RH_DEV explicit StreamComp(u32 per) : comp(blockIdx.x / per), row(blockIdx.x % per) {}
};

// QP launches: a poly is LQ rows of Q followed by LP rows of P.  Two components modulo Q and two modulo P, written (RhQP) or read (RhQPc)
struct RhQP { u64* q[2]; u64* p[2]; };
struct RhQPc { const u64* q[2]; const u64* p[2]; };
// Row `row` of npoly * (LQ + LP): blockIdx.x of a one-component launch, StreamComp::row of a two-component one
struct StreamRowQP {
  u32 poly, l;                     // l: the limb within its ring
  bool inQ;
  LimbConsts c;
  size_t ro, po;                   // word offset of the row in a dense (npoly, LQ or LP, N) block; in ONE poly (a row shared by the batch: a diagonal)
  RH_DEV StreamRowQP(u32 row, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP, int LQ, int LP, int logN) {
    const u32 LT_ = (u32)(LQ + LP);
    poly = row / LT_; l = row % LT_;
    inQ = l < (u32)LQ;
    if (!inQ) l -= (u32)LQ;
    c = inQ ? constsQ[l] : constsP[l];
    po = (size_t)l << logN;
    ro = ((size_t)poly * (inQ ? LQ : LP) + l) << logN;
  }
  // ... on rows of `len.n` words, for rings whose degree is no power of two (3N rings: logN is rounded up there).  The offsets are products of
  // wave-uniform values (blockIdx.x and kernel arguments), formed once per workgroup before the pair loop.
  struct RowLen { unsigned n; };
  RH_DEV StreamRowQP(u32 row, const LimbConsts* __restrict__ constsQ, const LimbConsts* __restrict__ constsP, int LQ, int LP, RowLen len) {
    const u32 LT_ = (u32)(LQ + LP);
    poly = row / LT_; l = row % LT_;
    inQ = l < (u32)LQ;
    if (!inQ) l -= (u32)LQ;
    c = inQ ? constsQ[l] : constsP[l];
    po = (size_t)l * len.n;
    ro = ((size_t)poly * (inQ ? LQ : LP) + l) * len.n;
  }
  // this row of component `comp` of a pack
  RH_DEV u64* of(const RhQP& a, u32 comp) const { return (inQ ? a.q[comp] : a.p[comp]) + ro; }
  RH_DEV const u64* of(const RhQPc& a, u32 comp) const { return (inQ ? a.q[comp] : a.p[comp]) + ro; }
};

// acc[pair i] = [first ? 0 : acc[pair i]] + t mod q, canonical: the tail of the rotate-accumulate kernels
RH_DEV void rh_accumulate2(u64* acc, unsigned i, const ulonglong2& t, u64 q, int first, bool nt) {
  ulonglong2 v = first ? make_ulonglong2(0, 0) : rh_ld2(acc + 2 * (size_t)i, nt);
  v.x = cred(v.x + t.x, q); v.y = cred(v.y + t.y, q);
  rh_st2(acc + 2 * (size_t)i, v, nt);
}

// The loop head over this thread's share of the pairs [pair0, pair1) of its row; pair i is the words 2 i, 2 i + 1
#define RH_FOR_EACH_PAIR(i, pair0, pair1) \
  for (unsigned i = (pair0) + blockIdx.y * blockDim.x + threadIdx.x; i < (pair1); i += gridDim.y * blockDim.x)

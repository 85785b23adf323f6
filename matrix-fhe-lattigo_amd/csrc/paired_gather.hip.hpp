// paired_gather.hip.hpp -- the NTT-domain index map of an automorphism read as aligned 16-byte pairs (the derivation: inner_sum_kernels.hip.hpp).
// Shared by the kernels that fuse the map with what follows it: inner_sum_kernels.hip.hpp, ring_packing_kernels.hip.hpp, lintrans_kernels.hip.hpp.
#pragma once
#include "stream_kernels.hip.hpp"

// index(2 i) of the automorphism `gen` on a standard ring of degree 2^logN >= 4 (every entry refuses N < 4)
RH_DEV u32 rh_galois_index_even(u32 i, int logN, u32 gen) {
  __builtin_assume(logN >= 2);
  const u32 mask = (2u << logN) - 1;
  const u32 t1 = 2 * rh_brev(2 * i, logN) + 1;
  return rh_brev((((gen * t1) & mask) - 1) >> 1, logN);
}
// the words index(2 i), index(2 i) ^ 1 of the row at `row`
RH_DEV ulonglong2 rh_gather2(const u64* row, u32 idx) {
  const ulonglong2 w = *reinterpret_cast<const ulonglong2*>(row + (idx & ~1u));
  return (idx & 1) ? make_ulonglong2(w.y, w.x) : w;
}

struct RhPmodQ { u64 s[RH_MAX_LIMBS_K]; };      // MForm(P mod q_i) per limb of Q

// lc_reduce.hip.hpp -- the 128-bit accumulate-then-reduce of the sums of Montgomery products (ckks.hip: ckks_linear_combination_kernel;
// lintrans_kernels.hip.hpp: diag_mac_qp_kernel).
//
// Every step of the reference's sequences ends in a reduction of acc + MRed(x, y): the result is the canonical residue of sum_k x_k y_k 2^-64,
// whatever the order of the reductions.  Here T = sum x_k y_k is kept in 128 bits and reduced by one Montgomery step,
// (T - (T_lo qinv mod 2^64) q) / 2^64 = T_hi - H with H < q, and one Barrett step on the 64-bit word T_hi - H + q.
// The chunk bound: q < 2^61 and operands below q give x y <= (q - 1)^2 < 2^122, so after C terms T < C 2^122 (no carry out of 128 bits for
// C <= 64) and T_hi - H + q <= T_hi + q < C 2^58 + 2^61 = (C + 8) 2^58, which stays a 64-bit word for C <= 56.
#pragma once
#include "modarith.hip.hpp"
#include "ring_types.hip.hpp"

#define LC_CHUNK 56            // terms summed between two reductions
#define LC_WIDTH 4             // terms whose loads are in flight together
#define LC_MODULUS_BITS 61     // the bound holds for q < 2^61 (checked per call: rh_moduli_below)
static_assert(LC_CHUNK <= 64 && (unsigned __int128)(LC_CHUNK + 8) << (2 * LC_MODULUS_BITS - 64) <= (unsigned __int128)1 << 64, "LC_CHUNK terms of q < 2^61 pass 64 bits after the Montgomery step");
static_assert(LC_CHUNK % LC_WIDTH == 0, "a chunk is a whole number of load groups");

RH_DEV u64 lc_reduce(u128 t, const LimbConsts& c) {
  const u64 lo = (u64)t, hi = (u64)(t >> 64);
  return bred_add(hi - mulhi64(lo * c.qinv, c.q) + c.q, c.q, c.bred0);
}

// a block address out of a device table: global memory, which the compiler cannot know of a word it loaded (it would emit flat loads)
RH_DEV const u64* lc_block(u64 addr) { return (const u64*)reinterpret_cast<const __attribute__((address_space(1))) u64*>(addr); }

// qp_rows_host.hpp -- host-side argument helpers of the entry points whose kernels stream the Q and the P rows of both ciphertext components in one
// launch with the NTT-domain index map of a Galois element (inner_sum.hip, lintrans.hip).
#pragma once
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "paired_gather.hip.hpp"

static inline int is_rings(rh_bext* be, int levelQ, int levelP, const char* who, rh_ring** RQ, rh_ring** RP) {
  if (!be) return rh_fail(RH_ERR_ARG, "%s: null basis extender", who);
  *RQ = rh_bext_ringQ(be); *RP = rh_bext_ringP(be);
  if (!*RP) return rh_fail(RH_ERR_ARG, "%s: basis extender has no P ring", who);
  if ((*RQ)->kind != RH_RING_STANDARD || (*RP)->kind != RH_RING_STANDARD)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
  if (levelQ < 0 || levelQ >= (*RQ)->L || levelP < 0 || levelP >= (*RP)->L)
    return rh_fail(RH_ERR_ARG, "%s: need 0 <= levelQ < %d and 0 <= levelP < %d", who, (*RQ)->L, (*RP)->L);
  if (levelQ + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: at most %d limbs", who, RH_MAX_LIMBS);
  if ((*RQ)->N < 4) return rh_fail(RH_ERR_ARG, "%s: N < 4", who);
  return RH_OK;
}
static inline int is_gen(const rh_ring* r, uint64_t gen, const char* who, u32* out) {
  if ((gen & 1) == 0) return rh_fail(RH_ERR_ARG, "%s: the Galois element must be odd", who);
  *out = (u32)(gen & (2 * (u64)r->N - 1));
  return RH_OK;
}

// ringP.ModulusAtLevel[levelP] mod q_i in Montgomery form, per limb of Q (the scalar of MulScalarBigint: core/rlwe/evaluator_automorphism.go:138-142, lintrans_evaluator.go:170)
static inline RhPmodQ is_pmodq(const rh_ring* RQ, const rh_ring* RP, int LQ, int LP) {
  RhPmodQ pq; memset(&pq, 0, sizeof(pq));
  for (int i = 0; i < LQ; ++i) {
    const u64 q = RQ->moduli[i];
    u64 p = 1 % q;
    for (int j = 0; j < LP; ++j) p = rh::mulmod(p, RP->moduli[j] % q, q);
    pq.s[i] = rh::mform(p, q);
  }
  return pq;
}

// qp_rows_host.hpp -- the ring, Galois-element and block argument checks of the entry points whose kernels stream (poly, limb) rows with the
// NTT-domain index map of a Galois element, modulo Q alone or modulo Q and P in one launch (inner_sum.hip, ring_packing.hip, lintrans.hip).
#pragma once
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "paired_gather.hip.hpp"

// A standard ring at `level`, `count` polys of two components in one launch; `negative`: the entry's words for count < 0
static inline int rh_ring_ok(const rh_ring* r, int level, int count, const char* who, const char* negative = "negative count") {
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (r->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, r->L);
  if (level + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: at most %d limbs", who, RH_MAX_LIMBS);
  if (r->N < 4) return rh_fail(RH_ERR_ARG, "%s: N < 4", who);
  if (count < 0) return rh_fail(RH_ERR_ARG, "%s: %s", who, negative);
  if ((size_t)count * 2 * (size_t)(level + 1) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  return RH_OK;
}
// The two rings of a basis extender: the kind and the level of BOTH come first, in the QP entries' own words; what is left is rh_ring_ok on ringQ
static inline int is_rings(rh_bext* be, int levelQ, int levelP, const char* who, rh_ring** RQ, rh_ring** RP) {
  if (!be) return rh_fail(RH_ERR_ARG, "%s: null basis extender", who);
  *RQ = rh_bext_ringQ(be); *RP = rh_bext_ringP(be);
  if (!*RP) return rh_fail(RH_ERR_ARG, "%s: basis extender has no P ring", who);
  if ((*RQ)->kind != RH_RING_STANDARD || (*RP)->kind != RH_RING_STANDARD)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
  if (levelQ < 0 || levelQ >= (*RQ)->L || levelP < 0 || levelP >= (*RP)->L)
    return rh_fail(RH_ERR_ARG, "%s: need 0 <= levelQ < %d and 0 <= levelP < %d", who, (*RQ)->L, (*RP)->L);
  return rh_ring_ok(*RQ, levelQ, 0, who);                                               // at most RH_MAX_LIMBS limbs, N >= 4
}
static inline int is_gen(const rh_ring* r, uint64_t gen, const char* who, u32* out) {
  if ((gen & 1) == 0) return rh_fail(RH_ERR_ARG, "%s: the Galois element must be odd", who);
  *out = (u32)(gen & (2 * (u64)r->N - 1));
  return RH_OK;
}

// The arguments of the rotate-accumulate entries modulo QP: the four accumulators (Q0, Q1, P0, P1) may overlap nothing that is gathered or read
// beside them: the four blocks of `gathered` and the `extra` operands, each sized by its kind once the rings are known.
enum { QP_BATCH_Q, QP_BATCH_P, QP_ROW_Q, QP_ROW_P };      // (npoly, LQ, N), (npoly, LP, N); one poly shared by the batch: (LQ, N), (LP, N)
struct QpExtra { const void* p; int kind; };
static inline int qp_accumulate_args(rh_bext* be, int levelQ, int levelP, uint64_t gen, const char* who, const uint64_t* const* gathered,
                                     const QpExtra* extra, int nextra, uint64_t* const* acc, int npoly, const char* text, rh_ring** RQ,
                                     rh_ring** RP, u32* g) {
  if (int rc = is_rings(be, levelQ, levelP, who, RQ, RP)) return rc;
  for (int j = 0; j < 4; ++j) if (!gathered[j] || !acc[j]) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  for (int j = 0; j < nextra; ++j) if (!extra[j].p) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  const size_t N = npoly ? (size_t)(*RQ)->N : 0;                                      // an empty batch overlaps nothing
  const size_t words[4] = {(size_t)npoly * (levelQ + 1) * N, (size_t)npoly * (levelP + 1) * N, (size_t)(levelQ + 1) * N, (size_t)(levelP + 1) * N};
  const RhBlock wr[4] = {{acc[0], words[QP_BATCH_Q]}, {acc[1], words[QP_BATCH_Q]}, {acc[2], words[QP_BATCH_P]}, {acc[3], words[QP_BATCH_P]}};
  RhBlock rd[8] = {{gathered[0], words[QP_BATCH_Q]}, {gathered[1], words[QP_BATCH_Q]}, {gathered[2], words[QP_BATCH_P]}, {gathered[3], words[QP_BATCH_P]}};
  for (int j = 0; j < nextra; ++j) rd[4 + j] = {extra[j].p, words[extra[j].kind]};
  if (int rc = rh_blocks_ok(wr, 4, rd, 4 + nextra, who, text)) return rc;
  return is_gen(*RQ, gen, who, g);
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

// multiparty.hip -- the hot paths of the multiparty protocols (multiparty/ of the reference; kernels: multiparty_kernels.hip.hpp):
//   rh_mp_aggregate         AggregateShares of every protocol (keygen_cpk.go:86-88, keygen_evk.go:213-242, keyswitch_sk.go:154-161) over MANY
//                           shares at once: every share read once, one write
//   rh_mp_gadget_share      GenShare of the evaluation-key, Galois-key and public-key protocols (keygen_evk.go:115-210, keygen_gal.go:57-78,
//                           keygen_cpk.go:70-83): every row of one party's shares for one or many keys
//   rh_mp_keyswitch_share   GenShare of the collective key switch (keyswitch_sk.go:118-149) on a batch of ciphertexts, and the secret-key
//                           term of the public key switch (keyswitch_pk.go)
// The samplers, the lift, the transforms and the automorphism of the secret are the library's own, driven from the host (multiparty.py).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "qp_rows_host.hpp"
#include "multiparty_kernels.hip.hpp"

#define MP_MAX_SHARES 4096

extern "C" size_t rh_mp_aggregate_table_words(int nshares) { return (size_t)(nshares > 0 ? nshares : 0); }

extern "C" int rh_mp_aggregate(rh_ring* r, int level, const uint64_t* const* shares, int nshares, uint64_t* out, int npoly, uint64_t* table_dev,
                               size_t table_words) {
  const char* who = "rh_mp_aggregate";
  if (int rc = rh_ring_ok(r, level, npoly, who, "npoly < 0")) return rc;
  if (!shares || !out || !table_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (nshares < 1 || nshares > MP_MAX_SHARES) return rh_fail(RH_ERR_ARG, "%s: %d shares, one call takes 1 to %d", who, nshares, MP_MAX_SHARES);
  const size_t words = rh_mp_aggregate_table_words(nshares);
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the address table needs %zu words, the caller's has %zu", who, words, table_words);
  const int L = level + 1;
  const size_t block = (size_t)npoly * L * (size_t)r->N;
  const RhBlock wr[2] = {{out, block}, {table_dev, words}};
  if (int rc = rh_blocks_ok(wr, 2, nullptr, 0, who, "")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 2, who, "the address table overlaps the output")) return rc;
  for (int k = 0; k < nshares; ++k) {
    if (!shares[k]) return rh_fail(RH_ERR_ARG, "%s: null argument (share %d)", who, k);
    const RhBlock s{shares[k], block};
    if ((uintptr_t)s.p & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
    if (rh_overlap(s, wr[1])) return rh_fail(RH_ERR_ARG, "%s: the address table overlaps share %d", who, k);
    if (shares[k] != out && rh_overlap(s, wr[0])) return rh_fail(RH_ERR_ARG, "%s: the output overlaps share %d without being it", who, k);
  }
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, (unsigned)npoly * (unsigned)L * ((unsigned)nshares + 1u));    // every share read, one write
  hipStream_t st = rh_stream(r);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  for (int k = 0; k < nshares; ++k) stage->h[k] = (u64)(uintptr_t)shares[k];
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  mp_aggregate_kernel<<<dim3((unsigned)npoly * (unsigned)L, g.grid.y), 256, 0, st>>>(table_dev, nshares, out, (unsigned)r->N, r->d_consts, L, g.nt);
  return rh_launch_ok("mp_aggregate_kernel");
}

// ringP may be NULL (levelP ignored): the residues under Q alone
static int mp_qp_ok(const rh_ring* rQ, const rh_ring* rP, int levelQ, int levelP, int count, const char* who) {
  if (int rc = rh_ring_ok(rQ, levelQ, count, who)) return rc;
  if (!rP) return RH_OK;
  if (rP->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
  if (rP->N != rQ->N || rP->device != rQ->device) return rh_fail(RH_ERR_ARG, "%s: ringQ and ringP differ in degree or device", who);
  if (levelP < 0 || levelP >= rP->L || levelP + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: levelP %d out of range [0,%d)", who, levelP, rP->L);
  return RH_OK;
}

extern "C" size_t rh_mp_gadget_share_table_words(int levelQ, int rows) { return (size_t)(rows > 0 ? rows : 0) * (size_t)(levelQ + 2); }

extern "C" int rh_mp_gadget_share(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, const uint64_t* crpQ,
                                  const uint64_t* crpP, uint64_t* shareQ, uint64_t* shareP, const uint64_t* skOutQ, const uint64_t* skOutP,
                                  const uint64_t* skInQ, int nkeys, int skin_keys, const uint64_t* rowtab, int rows, uint64_t* table_dev,
                                  size_t table_words) {
  const char* who = "rh_mp_gadget_share";
  if (int rc = mp_qp_ok(rQ, rP, levelQ, levelP, rows, who)) return rc;
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (!eQ || !crpQ || !shareQ || !skOutQ || !skInQ || !rowtab || !table_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((rP != nullptr) != (eP && crpP && shareP && skOutP) || (!rP && (eP || crpP || shareP || skOutP)))
    return rh_fail(RH_ERR_ARG, "%s: eP, crpP, shareP and skOutP go with ringP, all or none", who);
  if (nkeys < 1 || (skin_keys != 1 && skin_keys != nkeys)) return rh_fail(RH_ERR_ARG, "%s: nkeys < 1, or skIn holds neither one key for all nor one per key", who);
  const size_t words = rh_mp_gadget_share_table_words(levelQ, rows);
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the row table needs %zu words, the caller's has %zu", who, words, table_words);
  if ((size_t)rows * (size_t)(LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  for (int r = 0; r < rows; ++r) {
    const u64* t = rowtab + (size_t)r * (size_t)(1 + LQ);
    if (t[0] >= (u64)nkeys) return rh_fail(RH_ERR_ARG, "%s: row %d names key %llu of %d", who, r, (unsigned long long)t[0], nkeys);
    for (int l = 0; l < LQ; ++l)
      if (t[1 + l] >= rQ->moduli[l]) return rh_fail(RH_ERR_ARG, "%s: the scalar of row %d is not a residue of limb %d", who, r, l);
  }
  const size_t N = (size_t)rQ->N, R = (size_t)rows, K = (size_t)nkeys;
  const RhBlock wr[3] = {{shareQ, R * LQ * N}, {shareP, R * LP * N}, {table_dev, words}};
  const RhBlock rd[7] = {{eQ, R * LQ * N}, {eP, R * LP * N}, {crpQ, R * LQ * N}, {crpP, R * LP * N}, {skOutQ, K * LQ * N}, {skOutP, K * LP * N},
                         {skInQ, (size_t)skin_keys * LQ * N}};
  if (int rc = rh_blocks_ok(wr, 3, rd, 7, who, "a share overlaps an input")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 3, who, "two outputs overlap")) return rc;
  if (!rows) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)rows * (unsigned)(LQ + LP) * 3u);     // e and the CRP read, the share written
  hipStream_t st = rh_stream(rQ);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  memcpy(stage->h, rowtab, words * 8);
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  const MpShareArgs p{eQ, eP, crpQ, crpP, shareQ, shareP, skOutQ, skOutP, skInQ, table_dev, skin_keys == 1 && nkeys > 1 ? 1 : 0};
  mp_gadget_share_kernel<<<dim3((unsigned)rows * (unsigned)(LQ + LP), g.grid.y), 256, 0, st>>>(p, (unsigned)N, rQ->logN, rQ->d_consts,
                                                                                                rP ? rP->d_consts : rQ->d_consts, LQ, LP, g.nt);
  return rh_launch_ok("mp_gadget_share_kernel");
}

// one key of (limbs, N) over Q and over P: `blocks` gets its two read ranges
static void mp_key_blocks(const u64* q, const u64* p, size_t wq, size_t wp, RhBlock* blocks) { blocks[0] = {q, wq}; blocks[1] = {p, wp}; }

extern "C" int rh_mp_relin_round_one(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* e0Q, const uint64_t* e0P, const uint64_t* e1Q,
                                     const uint64_t* e1P, const uint64_t* crpQ, const uint64_t* crpP, uint64_t* shareQ, uint64_t* shareP,
                                     const uint64_t* uQ, const uint64_t* uP, const uint64_t* skQ, const uint64_t* skP, const uint64_t* skIQ,
                                     const uint64_t* rowtab, int rows, uint64_t* table_dev, size_t table_words) {
  const char* who = "rh_mp_relin_round_one";
  if (int rc = mp_qp_ok(rQ, rP, levelQ, levelP, rows, who)) return rc;
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (!e0Q || !e1Q || !crpQ || !shareQ || !uQ || !skQ || !skIQ || !rowtab || !table_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((rP != nullptr) != (e0P && e1P && crpP && shareP && uP && skP) || (!rP && (e0P || e1P || crpP || shareP || uP || skP)))
    return rh_fail(RH_ERR_ARG, "%s: e0P, e1P, crpP, shareP, uP and skP go with ringP, all or none", who);
  const size_t words = rh_mp_gadget_share_table_words(levelQ, rows);
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the row table needs %zu words, the caller's has %zu", who, words, table_words);
  if ((size_t)rows * (size_t)(LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  for (int r = 0; r < rows; ++r)
    for (int l = 0; l < LQ; ++l)
      if (rowtab[(size_t)r * (size_t)(1 + LQ) + 1 + l] >= rQ->moduli[l]) return rh_fail(RH_ERR_ARG, "%s: the scalar of row %d is not a residue of limb %d", who, r, l);
  const size_t N = (size_t)rQ->N, R = (size_t)rows, wq = R * LQ * N, wp = R * LP * N;
  const RhBlock wr[3] = {{shareQ, 2 * wq}, {shareP, 2 * wp}, {table_dev, words}};
  RhBlock rd[11] = {{e0Q, wq}, {e0P, wp}, {e1Q, wq}, {e1P, wp}, {crpQ, wq}, {crpP, wp}, {skIQ, (size_t)LQ * N}};
  mp_key_blocks(uQ, uP, (size_t)LQ * N, (size_t)LP * N, rd + 7);
  mp_key_blocks(skQ, skP, (size_t)LQ * N, (size_t)LP * N, rd + 9);
  if (int rc = rh_blocks_ok(wr, 3, rd, 11, who, "a share overlaps an input")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 3, who, "two outputs overlap")) return rc;
  if (!rows) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)rows * (unsigned)(LQ + LP) * 5u);     // e0, e1 and the CRP read, both components written
  hipStream_t st = rh_stream(rQ);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  memcpy(stage->h, rowtab, words * 8);
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  const MpRelinOneArgs p{RhQPc{{e0Q, e1Q}, {e0P, e1P}}, crpQ, crpP, shareQ, shareP, uQ, uP, skQ, skP, skIQ, table_dev};
  mp_relin_round_one_kernel<<<dim3((unsigned)rows * (unsigned)(LQ + LP), g.grid.y), 256, 0, st>>>(p, (unsigned)N, rQ->logN, rQ->d_consts,
                                                                                                   rP ? rP->d_consts : rQ->d_consts, LQ, LP, g.nt);
  return rh_launch_ok("mp_relin_round_one_kernel");
}

extern "C" int rh_mp_relin_round_two(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, const uint64_t* r1Q,
                                     const uint64_t* r1P, uint64_t* outQ, uint64_t* outP, const uint64_t* uQ, const uint64_t* uP, const uint64_t* skQ,
                                     const uint64_t* skP, int rows) {
  const char* who = "rh_mp_relin_round_two";
  if (int rc = mp_qp_ok(rQ, rP, levelQ, levelP, rows, who)) return rc;
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (!eQ || !r1Q || !outQ || !uQ || !skQ) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((rP != nullptr) != (eP && r1P && outP && uP && skP) || (!rP && (eP || r1P || outP || uP || skP)))
    return rh_fail(RH_ERR_ARG, "%s: eP, r1P, outP, uP and skP go with ringP, all or none", who);
  if ((size_t)rows * (size_t)(LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  const size_t N = (size_t)rQ->N, R = (size_t)rows, wq = R * LQ * N, wp = R * LP * N;
  const RhBlock wr[2] = {{outQ, wq}, {outP, wp}};
  RhBlock rd[8] = {{eQ, wq}, {eP, wp}, {r1Q, 2 * wq}, {r1P, 2 * wp}};
  mp_key_blocks(uQ, uP, (size_t)LQ * N, (size_t)LP * N, rd + 4);
  mp_key_blocks(skQ, skP, (size_t)LQ * N, (size_t)LP * N, rd + 6);
  if (int rc = rh_blocks_ok(wr, 2, rd, 8, who, "a share overlaps an input")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 2, who, "the two outputs overlap")) return rc;
  if (!rows) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)rows * (unsigned)(LQ + LP) * 4u);     // e and both round-one components read, the share written
  const MpRelinTwoArgs p{eQ, eP, r1Q, r1P, outQ, outP, uQ, uP, skQ, skP};
  mp_relin_round_two_kernel<<<dim3((unsigned)rows * (unsigned)(LQ + LP), g.grid.y), 256, 0, rh_stream(rQ)>>>(p, (unsigned)N, rQ->logN, rQ->d_consts,
                                                                                                              rP ? rP->d_consts : rQ->d_consts, LQ, LP, g.nt);
  return rh_launch_ok("mp_relin_round_two_kernel");
}

extern "C" int rh_mp_keyswitch_share(rh_ring* r, int level, const uint64_t* c1, int c1_rows, const uint64_t* skA, const uint64_t* skB,
                                     const uint64_t* acc, const uint64_t* e, uint64_t* out, int npoly) {
  const char* who = "rh_mp_keyswitch_share";
  if (int rc = rh_ring_ok(r, level, npoly, who, "npoly < 0")) return rc;
  if (!c1 || !skA || !out) return rh_fail(RH_ERR_ARG, "%s: null argument (skB, acc and e alone may be NULL)", who);
  const int L = level + 1;
  if (c1_rows < L) return rh_fail(RH_ERR_ARG, "%s: c1_rows %d < %d limbs", who, c1_rows, L);
  for (const void* p : {(const void*)c1, (const void*)skA, (const void*)skB, (const void*)acc, (const void*)e})
    if ((uintptr_t)p & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  const size_t N = (size_t)r->N, words = (size_t)npoly * L * N, kw = (size_t)L * N;
  const size_t cw = npoly ? ((size_t)(npoly - 1) * (size_t)c1_rows + L) * N : 0;
  const RhBlock wr[1] = {{out, words}}, rd[3] = {{skA, kw}, {skB, skB ? kw : 0}, {c1, out == c1 && c1_rows == L ? 0 : cw}};
  if (int rc = rh_blocks_ok(wr, 1, rd, 3, who, "the output overlaps a secret key, or the ciphertext without being it")) return rc;
  for (const u64* p : {acc, e})
    if (p && p != out && rh_overlap(RhBlock{p, words}, wr[0])) return rh_fail(RH_ERR_ARG, "%s: the output overlaps acc or e without being it", who);
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, (unsigned)npoly * (unsigned)L * (2u + (acc ? 1u : 0u) + (e ? 1u : 0u)));
  const dim3 grid((unsigned)npoly * (unsigned)L, g.grid.y);
  hipStream_t st = rh_stream(r);
  rh_with_flag(skB != nullptr, [&](auto SUB) {
    rh_with_flag(acc != nullptr, [&](auto ACC) {
      rh_with_flag(e != nullptr, [&](auto ERR) {
        mp_keyswitch_share_kernel<decltype(SUB)::value, decltype(ACC)::value, decltype(ERR)::value>
            <<<grid, 256, 0, st>>>(c1, c1_rows, skA, skB, acc, e, out, (unsigned)N, r->d_consts, L, g.nt);     // cache policy: rh_stream_grid's, by the rows moved
      });
    });
  });
  return rh_launch_ok("mp_keyswitch_share_kernel");
}

// keygen.hip -- what produces keys and ciphertexts on the device (kernels: keygen_kernels.hip.hpp):
//   rh_sample_uniform        UniformSampler.Read, ring/sampler_uniform.go:46-106, on the library's own stream (a keyed BLAKE2b in counter mode)
//   rh_sample_gaussian       GaussianSampler.Read's distribution, ring/sampler_gaussian.go:159-172, from a cumulative table
//   rh_sample_ternary        TernarySampler.Read with a density, ring/sampler_ternary.go
//   rh_small_lift            the residues of small signed coefficients under Q and P: Read + ExtendBasisSmallNormAndCenter, and ReadAndAdd
//   rh_rlwe_gadget_encrypt   every row of one or many gadget ciphertexts: core/rlwe/encryptor.go:432-452 per row and
//                            AddPolyTimesGadgetVectorToGadgetCiphertext, core/rlwe/gadgetciphertext.go:172-241 (keygenerator.go:297-315)
//   rh_rlwe_encrypt_sk       encryptZeroSkFromC1 with addPtToCt, core/rlwe/encryptor.go:398-424, :512-530
//   rh_rlwe_mul_pk           the two products of encryptZeroPk, core/rlwe/encryptor.go:259-260 (and :324-326)
//   rh_rlwe_decrypt          Decryptor.Decrypt's Horner sum, core/rlwe/decryptor.go:51-92
// The transforms, the automorphism of the secret and the ModDown are the library's own, driven from the host (keygen.py).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "qp_rows_host.hpp"
#include "keygen_kernels.hip.hpp"

// The rings of this file: standard rings, and 3N rings whose rows split into groups of eight coefficients (every kernel here addresses row r at
// r * N words), and conjugate-invariant rings: every kernel here is per coefficient or row-wise in the NTT domain, so the ring type does not
// enter (the transforms are the ring's own).  Who may hand such a ring in is decided above this file: the bare Python constructors refuse it,
// ckks.Parameters passes the permit (sampling.rings_ok).  The other checks are those of the row-streaming entries: level, limb and row counts.
static int kg_ring_ok(const rh_ring* r, int level, int count, const char* who, const char* negative = "negative count") {
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (r->kind == RH_RING_3N && (r->N & 7))
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: a 3N ring of degree %d: the samplers serve groups of eight coefficients (N %% 8 must be 0)", who, r->N);
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, r->L);
  if (level + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: at most %d limbs", who, RH_MAX_LIMBS);
  if (r->N < 4) return rh_fail(RH_ERR_ARG, "%s: N < 4", who);
  if (count < 0) return rh_fail(RH_ERR_ARG, "%s: %s", who, negative);
  if ((size_t)count * 2 * (size_t)(level + 1) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  return RH_OK;
}

// the samplers' common checks: rows that split into groups of eight coefficients
static int samp_ok(const rh_ring* r, int level, int npoly, const uint64_t* state, const void* out, const char* who) {
  if (int rc = kg_ring_ok(r, level, npoly, who, "npoly < 0")) return rc;
  if (r->N < 8) return rh_fail(RH_ERR_ARG, "%s: N < 8 (a lane serves a group of eight coefficients)", who);
  if (!state || !out) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((uintptr_t)out & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  return RH_OK;
}
static SampArgs samp_args(const uint64_t* state, uint64_t call, uint64_t poly0, uint64_t row0) {
  SampArgs a;
  memcpy(a.h, state, sizeof(a.h));
  a.call = call; a.poly0 = poly0; a.row0 = row0;
  return a;
}
static unsigned group_chunks(const rh_ring* r) {                        // blockIdx.y extent: 256 groups of eight coefficients per workgroup
  unsigned chunks = ((unsigned)r->N / 8 + 255) / 256;
  return chunks > 64 ? 64 : chunks;
}

extern "C" int rh_sample_uniform(rh_ring* r, int level, const uint64_t* state, uint64_t call, uint64_t poly0, uint64_t row0, uint64_t* out,
                                 int out_rows, int npoly) {
  const char* who = "rh_sample_uniform";
  if (int rc = samp_ok(r, level, npoly, state, out, who)) return rc;
  const int L = level + 1;
  if (out_rows < L) return rh_fail(RH_ERR_ARG, "%s: out_rows %d < %d limbs", who, out_rows, L);
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, (unsigned)npoly * (unsigned)L);
  sample_uniform_kernel<<<dim3((unsigned)npoly * (unsigned)L, group_chunks(r)), 256, 0, rh_stream(r)>>>(samp_args(state, call, poly0, row0), out, out_rows,
                                                                                                     (unsigned)r->N, r->d_consts, L, g.nt);
  return rh_launch_ok("sample_uniform_kernel");
}

extern "C" int rh_sample_gaussian(rh_ring* r, const uint64_t* state, uint64_t call, uint64_t poly0, const uint64_t* table_dev, int table_len,
                                  int32_t* out, int npoly) {
  const char* who = "rh_sample_gaussian";
  if (int rc = samp_ok(r, 0, npoly, state, out, who)) return rc;
  if (!table_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (table_len < 1 || table_len > 1024)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: a cumulative table of %d entries: floor(bound) must be below 1024 (the big-norm sampler is not built)", who, table_len);
  if (!npoly) return RH_OK;
  (void)rh_stream_begin(r, (unsigned)npoly);
  sample_small_kernel<true><<<dim3((unsigned)npoly, group_chunks(r)), 256, 0, rh_stream(r)>>>(samp_args(state, call, poly0, 0), out, (unsigned)r->N,
                                                                                             table_dev, table_len, 0);
  return rh_launch_ok("sample_small_kernel");
}

extern "C" int rh_sample_ternary(rh_ring* r, const uint64_t* state, uint64_t call, uint64_t poly0, uint64_t threshold, int32_t* out, int npoly) {
  const char* who = "rh_sample_ternary";
  if (int rc = samp_ok(r, 0, npoly, state, out, who)) return rc;
  if (threshold >> 63 && threshold != (1ull << 63)) return rh_fail(RH_ERR_ARG, "%s: the threshold is floor(P 2^63) for a density P <= 1", who);
  if (!npoly) return RH_OK;
  (void)rh_stream_begin(r, (unsigned)npoly);
  sample_small_kernel<false><<<dim3((unsigned)npoly, group_chunks(r)), 256, 0, rh_stream(r)>>>(samp_args(state, call, poly0, 0), out, (unsigned)r->N,
                                                                                              nullptr, 0, threshold);
  return rh_launch_ok("sample_small_kernel");
}

// ringP may be NULL (levelP ignored, outP NULL): the residues under Q alone
static int qp_pair_ok(const rh_ring* rQ, const rh_ring* rP, int levelQ, int levelP, int count, const char* who) {
  if (int rc = kg_ring_ok(rQ, levelQ, count, who)) return rc;
  if (!rP) return RH_OK;
  if (rP->kind != rQ->kind) return rh_fail(RH_ERR_UNSUPPORTED, "%s: ringQ and ringP must be of the same kind", who);
  if (rP->N != rQ->N || rP->device != rQ->device) return rh_fail(RH_ERR_ARG, "%s: ringQ and ringP differ in degree or device", who);
  if (levelP < 0 || levelP >= rP->L || levelP + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: levelP %d out of range [0,%d)", who, levelP, rP->L);
  return RH_OK;
}

extern "C" int rh_small_lift(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const int32_t* in, uint64_t* outQ, int q_rows, uint64_t* outP,
                             int p_rows, int npoly, int accumulate) {
  const char* who = "rh_small_lift";
  if (int rc = qp_pair_ok(rQ, rP, levelQ, levelP, npoly, who)) return rc;
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (!in || !outQ || (rP != nullptr) != (outP != nullptr)) return rh_fail(RH_ERR_ARG, "%s: null argument, or outP without ringP", who);
  if (q_rows < LQ || (rP && p_rows < LP)) return rh_fail(RH_ERR_ARG, "%s: fewer rows per poly than limbs", who);
  if (((uintptr_t)in & 7) || ((uintptr_t)outQ & 15) || ((uintptr_t)outP & 15)) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)npoly * (unsigned)(LQ + LP));
  unsigned chunks = ((unsigned)rQ->N / 2 + 255) / 256; if (chunks > 65535) chunks = 65535;      // one coefficient pair per lane
  const dim3 grid((unsigned)npoly, chunks);
  hipStream_t st = rh_stream(rQ);
  const LimbConsts* cP = rP ? rP->d_consts : rQ->d_consts;
  if (accumulate) small_lift_kernel<true><<<grid, 256, 0, st>>>(in, outQ, q_rows, outP, p_rows, (unsigned)rQ->N, rQ->d_consts, cP, LQ, LP, g.nt);
  else small_lift_kernel<false><<<grid, 256, 0, st>>>(in, outQ, q_rows, outP, p_rows, (unsigned)rQ->N, rQ->d_consts, cP, LQ, LP, g.nt);
  return rh_launch_ok("small_lift_kernel");
}

extern "C" size_t rh_rlwe_gadget_encrypt_table_words(int levelQ, int rows) { return (size_t)(rows > 0 ? rows : 0) * (size_t)(levelQ + 2); }

extern "C" int rh_rlwe_gadget_encrypt(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, uint64_t* tabQ,
                                      uint64_t* tabP, const uint64_t* skOutQ, const uint64_t* skOutP, const uint64_t* skInQ, int nkeys,
                                      int skin_keys, const uint64_t* rowtab, int rows, uint64_t* table_dev, size_t table_words) {
  const char* who = "rh_rlwe_gadget_encrypt";
  if (int rc = qp_pair_ok(rQ, rP, levelQ, levelP, rows, who)) return rc;
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (!eQ || !tabQ || !skOutQ || !skInQ || !rowtab || !table_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((rP != nullptr) != (eP && tabP && skOutP) || (!rP && (eP || tabP || skOutP)))
    return rh_fail(RH_ERR_ARG, "%s: eP, tabP and skOutP go with ringP, all or none", who);
  if (nkeys < 1 || (skin_keys != 1 && skin_keys != nkeys)) return rh_fail(RH_ERR_ARG, "%s: nkeys < 1, or skIn holds neither one key for all nor one per key", who);
  const size_t words = rh_rlwe_gadget_encrypt_table_words(levelQ, rows);
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the row table needs %zu words, the caller's has %zu", who, words, table_words);
  if ((size_t)rows * (size_t)(LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  for (int r = 0; r < rows; ++r) {
    const u64* t = rowtab + (size_t)r * (size_t)(1 + LQ);
    if (t[0] >= (u64)nkeys) return rh_fail(RH_ERR_ARG, "%s: row %d names key %llu of %d", who, r, (unsigned long long)t[0], nkeys);
    for (int l = 0; l < LQ; ++l)
      if (t[1 + l] >= rQ->moduli[l]) return rh_fail(RH_ERR_ARG, "%s: the scalar of row %d is not a residue of limb %d", who, r, l);
  }
  const size_t N = (size_t)rQ->N, R = (size_t)rows, K = (size_t)nkeys;
  const RhBlock wr[3] = {{tabQ, R * 2 * LQ * N}, {tabP, R * 2 * LP * N}, {table_dev, words}};
  const RhBlock rd[5] = {{eQ, R * LQ * N}, {eP, R * LP * N}, {skOutQ, K * LQ * N}, {skOutP, K * LP * N}, {skInQ, (size_t)skin_keys * LQ * N}};
  if (int rc = rh_blocks_ok(wr, 3, rd, 5, who, "a key table overlaps an input")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 3, who, "two tables overlap")) return rc;
  if (!rows) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)rows * (unsigned)(LQ + LP) * 3u);     // e and a read, b written
  hipStream_t st = rh_stream(rQ);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  memcpy(stage->h, rowtab, words * 8);
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  const GadgetEncArgs p{eQ, eP, tabQ, tabP, skOutQ, skOutP, skInQ, table_dev, skin_keys == 1 && nkeys > 1 ? 1 : 0};
  rlwe_gadget_encrypt_kernel<<<dim3((unsigned)rows * (unsigned)(LQ + LP), g.grid.y), 256, 0, st>>>(p, (unsigned)N, rQ->d_consts,
                                                                                                    rP ? rP->d_consts : rQ->d_consts, LQ, LP, g.nt);
  return rh_launch_ok("rlwe_gadget_encrypt_kernel");
}

extern "C" size_t rh_rgsw_encrypt_table_words(int levelQ, int rows) { return (size_t)(rows > 0 ? rows : 0) * (size_t)(levelQ + 3); }

extern "C" int rh_rgsw_encrypt(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, uint64_t* tabQ, uint64_t* tabP,
                               const uint64_t* skQ, const uint64_t* skP, const uint64_t* ptQ, int npt, const uint64_t* rowtab, int rows,
                               uint64_t* table_dev, size_t table_words) {
  const char* who = "rh_rgsw_encrypt";
  if (int rc = qp_pair_ok(rQ, rP, levelQ, levelP, rows, who)) return rc;
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (!eQ || !tabQ || !skQ || !rowtab || !table_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((rP != nullptr) != (eP && tabP && skP) || (!rP && (eP || tabP || skP)))
    return rh_fail(RH_ERR_ARG, "%s: eP, tabP and skP go with ringP, all or none", who);
  if (npt < 0 || (npt && !ptQ)) return rh_fail(RH_ERR_ARG, "%s: npt < 0, or plaintexts without their block", who);
  const size_t words = rh_rgsw_encrypt_table_words(levelQ, rows);
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the row table needs %zu words, the caller's has %zu", who, words, table_words);
  if ((size_t)rows * (size_t)(LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  for (int r = 0; r < rows; ++r) {
    const u64* t = rowtab + (size_t)r * (size_t)(2 + LQ);
    bool any = false;
    for (int l = 0; l < LQ; ++l) {
      if (t[2 + l] >= rQ->moduli[l]) return rh_fail(RH_ERR_ARG, "%s: the scalar of row %d is not a residue of limb %d", who, r, l);
      any = any || t[2 + l];
    }
    if (any && t[0] >= (u64)npt) return rh_fail(RH_ERR_ARG, "%s: row %d names plaintext %llu of %d", who, r, (unsigned long long)t[0], npt);
    if (t[1] > 1) return rh_fail(RH_ERR_ARG, "%s: row %d names half %llu of an RGSW ciphertext", who, r, (unsigned long long)t[1]);
  }
  const size_t N = (size_t)rQ->N, R = (size_t)rows;
  const RhBlock wr[3] = {{tabQ, R * 2 * LQ * N}, {tabP, R * 2 * LP * N}, {table_dev, words}};
  const RhBlock rd[5] = {{eQ, R * LQ * N}, {eP, R * LP * N}, {skQ, LQ * N}, {skP, LP * N}, {ptQ, (size_t)npt * LQ * N}};
  if (int rc = rh_blocks_ok(wr, 3, rd, 5, who, "a key table overlaps an input")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 3, who, "two tables overlap")) return rc;
  if (!rows) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)rows * (unsigned)(LQ + LP) * 3u);     // e and a read, b written
  hipStream_t st = rh_stream(rQ);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  memcpy(stage->h, rowtab, (size_t)rows * (size_t)(2 + LQ) * 8);
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  const RgswEncArgs p{eQ, eP, tabQ, tabP, skQ, skP, ptQ, table_dev};
  rgsw_encrypt_kernel<<<dim3((unsigned)rows * (unsigned)(LQ + LP), g.grid.y), 256, 0, st>>>(p, (unsigned)N, rQ->d_consts, rP ? rP->d_consts : rQ->d_consts,
                                                                                             LQ, LP, g.nt);
  return rh_launch_ok("rgsw_encrypt_kernel");
}

// blocks of (npoly, level + 1, N) words each, 16-byte aligned; `out` may be one of the per-poly inputs (every lane reads its words before it writes them)
static int rows_ok(const rh_ring* r, int level, int npoly, const char* who) {
  if (int rc = kg_ring_ok(r, level, npoly, who, "npoly < 0")) return rc;
  return RH_OK;
}
static bool misaligned(std::initializer_list<const void*> ps) {
  for (const void* p : ps) if ((uintptr_t)p & 15) return true;
  return false;
}

extern "C" int rh_rlwe_encrypt_sk(rh_ring* r, int level, const uint64_t* c1, const uint64_t* sk, const uint64_t* e, const uint64_t* pt, uint64_t* c0, int npoly) {
  const char* who = "rh_rlwe_encrypt_sk";
  if (int rc = rows_ok(r, level, npoly, who)) return rc;
  if (!c1 || !sk || !c0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (pt && !e) return rh_fail(RH_ERR_ARG, "%s: a plaintext is added together with the error (NTT-domain ciphertexts) or not here", who);
  if (misaligned({c1, sk, e, pt, c0})) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  const int L = level + 1;
  const size_t words = (size_t)npoly * L * (size_t)r->N;
  const RhBlock wr[1] = {{c0, words}}, rd[1] = {{sk, (size_t)L * (size_t)r->N}};
  if (int rc = rh_blocks_ok(wr, 1, rd, 1, who, "c0 overlaps the secret key")) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, (unsigned)npoly * (unsigned)L * (e ? 3u : 2u));
  const dim3 grid((unsigned)npoly * (unsigned)L, g.grid.y);
  if (e) rlwe_encrypt_sk_kernel<true><<<grid, 256, 0, rh_stream(r)>>>(c1, sk, e, pt, c0, (unsigned)r->N, r->d_consts, L, g.nt);
  else rlwe_encrypt_sk_kernel<false><<<grid, 256, 0, rh_stream(r)>>>(c1, sk, nullptr, nullptr, c0, (unsigned)r->N, r->d_consts, L, g.nt);
  return rh_launch_ok("rlwe_encrypt_sk_kernel");
}

extern "C" int rh_rlwe_mul_pk(rh_ring* r, int level, const uint64_t* u, const uint64_t* pk0, const uint64_t* pk1, uint64_t* ct0, uint64_t* ct1, int npoly) {
  const char* who = "rh_rlwe_mul_pk";
  if (int rc = rows_ok(r, level, npoly, who)) return rc;
  if (!u || !pk0 || !pk1 || !ct0 || !ct1) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (misaligned({u, pk0, pk1, ct0, ct1})) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  const int L = level + 1;
  const size_t words = (size_t)npoly * L * (size_t)r->N, kw = (size_t)L * (size_t)r->N;
  const RhBlock wr[2] = {{ct0, words}, {ct1, words}}, rd[3] = {{u, words}, {pk0, kw}, {pk1, kw}};
  if (int rc = rh_blocks_ok(wr, 2, rd, 3, who, "an output overlaps an input")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 2, who, "the two outputs overlap")) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, (unsigned)npoly * (unsigned)L * 3u);
  rlwe_mul_pk_kernel<<<dim3((unsigned)npoly * (unsigned)L, g.grid.y), 256, 0, rh_stream(r)>>>(u, pk0, pk1, ct0, ct1, (unsigned)r->N, r->d_consts, L, g.nt);
  return rh_launch_ok("rlwe_mul_pk_kernel");
}

extern "C" int rh_rlwe_decrypt(rh_ring* r, int level, const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* sk, uint64_t* out, int npoly) {
  const char* who = "rh_rlwe_decrypt";
  if (int rc = rows_ok(r, level, npoly, who)) return rc;
  if (!c0 || !c1 || !sk || !out) return rh_fail(RH_ERR_ARG, "%s: null argument (degree 1 or 2: c2 alone may be NULL)", who);
  if (misaligned({c0, c1, c2, sk, out})) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  const int L = level + 1;
  const RhBlock wr[1] = {{out, (size_t)npoly * L * (size_t)r->N}}, rd[1] = {{sk, (size_t)L * (size_t)r->N}};
  if (int rc = rh_blocks_ok(wr, 1, rd, 1, who, "the output overlaps the secret key")) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, (unsigned)npoly * (unsigned)L * (c2 ? 4u : 3u));
  const dim3 grid((unsigned)npoly * (unsigned)L, g.grid.y);
  if (c2) rlwe_decrypt_kernel<2><<<grid, 256, 0, rh_stream(r)>>>(c0, c1, c2, sk, out, (unsigned)r->N, r->d_consts, L, g.nt);
  else rlwe_decrypt_kernel<1><<<grid, 256, 0, rh_stream(r)>>>(c0, c1, nullptr, sk, out, (unsigned)r->N, r->d_consts, L, g.nt);
  return rh_launch_ok("rlwe_decrypt_kernel");
}

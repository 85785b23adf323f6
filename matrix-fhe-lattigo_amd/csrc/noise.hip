// noise.hip -- the noise meters (kernels: noise_kernels.hip.hpp):
//   rh_ring_centered_moments   n, sum x, sum x^2, min |x| and max |x| of PolyToBigintCentered(p, gap, .) (ring/ring.go:503-543, ring/ringqp) for
//                              every poly of a coefficient-domain block, over the limbs of Q and optionally of P as one RNS basis: what
//                              Log2OfStandardDeviation (ring/ring.go:647-686) and NormStats (core/rlwe/utils.go:135-183) are computed from
//   rh_rlwe_gadget_phase       NoiseGadgetCiphertext (core/rlwe/utils.go:51-102) up to its INTT, for many keys in one launch; NoisePublicKey
//                              (:13-25) is one row without a plaintext
// The transforms between the two are the library's own, driven from the host (noise.py).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "noise_kernels.hip.hpp"

// ---- moments ------------------------------------------------------------------------------------------------------------------------------------
static size_t noise_pairs(int L) { return (size_t)(L + 2) * (size_t)(L + 3) / 2; }
extern "C" size_t rh_ring_centered_moments_words(int limbs) { return limbs < 1 ? 0 : 3 * noise_pairs(limbs) + 2 * (size_t)limbs; }

static size_t noise_table_words(int L) { return (size_t)L * (sizeof(LimbConsts) / 8) + 2 * (size_t)L + (size_t)L * L + noise_pairs(L); }

// the ring's scratch, grown under the ring's lock (the free waits for the work that still reads it)
static int noise_scratch(rh_ring* r, size_t words, const char* who) {
  if (r->noise_words >= words) return RH_OK;
  if (r->d_noise) (void)hipFree(r->d_noise);
  r->d_noise = nullptr; r->noise_words = 0;
  if (hipMalloc((void**)&r->d_noise, words * 8) != hipSuccess) { (void)hipGetLastError(); return rh_fail(RH_ERR_NOMEM, "%s: hipMalloc(%zu words of scratch) failed", who, words); }
  r->noise_words = words;
  return RH_OK;
}

// consts | garner | rmod | half | pairs for the basis m = q_0 .. q_levelQ, p_0 .. p_levelP, into h
static int noise_tables(const rh_ring* rQ, int LQ, const rh_ring* rP, int LP, u64* h, const char* who) {
  const int L = LQ + LP;
  std::vector<u64> m((size_t)L);
  LimbConsts* hc = reinterpret_cast<LimbConsts*>(h);
  for (int j = 0; j < L; ++j) {
    hc[j] = j < LQ ? rQ->hconsts[j] : rP->hconsts[j - LQ];
    m[j] = hc[j].q;
  }
  u64* garner = h + (size_t)L * (sizeof(LimbConsts) / 8); u64* rmod = garner + L; u64* half = rmod + (size_t)L * L; u64* pairs = half + L;
  for (int j = 0; j < L; ++j) {
    u64 prod = 1 % m[j];
    for (int i = 0; i < L; ++i) rmod[(size_t)j * L + i] = 0;
    for (int i = 0; i < j; ++i) {
      rmod[(size_t)j * L + i] = rh::mform(prod, m[j]);                                  // R_i mod m_j
      if (m[i] % m[j] == 0) return rh_fail(RH_ERR_ARG, "%s: the moduli of the basis are not pairwise distinct (%llu twice)", who, (unsigned long long)m[j]);
      prod = rh::mulmod(prod, m[i] % m[j], m[j]);
    }
    garner[j] = rh::mform(rh::invmod_prime(prod, m[j]), m[j]);
  }
  // floor(M / 2) in mixed radix: M - 1 has the digits m_i - 1 and is even (M is odd), so halve that digit vector from the top:
  // a remainder of 1 at digit i carries m_{i-1} into digit i - 1
  u64 rem = 0;
  for (int i = L - 1; i >= 0; --i) {
    const u128 v = (u128)rem * m[i] + (m[i] - 1);
    half[i] = (u64)(v >> 1); rem = (u64)(v & 1);
  }
  size_t k = 0;
  for (int i = 0; i < L + 2; ++i) for (int j = i; j < L + 2; ++j) pairs[k++] = (u64)i | ((u64)j << 8);
  return RH_OK;
}

extern "C" int rh_ring_centered_moments(rh_ring* rQ, int levelQ, const uint64_t* q, int q_rows, rh_ring* rP, int levelP, const uint64_t* p, int p_rows,
                                        int gap, int npoly, uint64_t* out) {
  const char* who = "rh_ring_centered_moments";
  if (!rQ) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (levelQ < 0 || levelQ >= rQ->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, levelQ, rQ->L);
  if (rP) {
    if (rP->N != rQ->N || rP->device != rQ->device) return rh_fail(RH_ERR_ARG, "%s: ringQ and ringP differ in degree or device", who);
    if (levelP < 0 || levelP >= rP->L) return rh_fail(RH_ERR_ARG, "%s: levelP %d out of range [0,%d)", who, levelP, rP->L);
    if (rh_stream(rQ) != rh_stream(rP)) return rh_fail(RH_ERR_ARG, "%s: the two ring handles are on different streams (rh_ring_set_stream)", who);
  }
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0, L = LQ + LP;
  if (L > RH_MAX_LIMBS) return rh_fail(RH_ERR_UNSUPPORTED, "%s: more than %d moduli (%d of Q and %d of P)", who, RH_MAX_LIMBS, LQ, LP);
  if (gap < 1 || rQ->N % gap) return rh_fail(RH_ERR_ARG, "%s: gap %d does not divide N = %d", who, gap, rQ->N);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  if (!q || !out || (rP != nullptr) != (p != nullptr)) return rh_fail(RH_ERR_ARG, "%s: null argument, or p without ringP", who);
  if (q_rows < LQ || (rP && p_rows < LP)) return rh_fail(RH_ERR_ARG, "%s: fewer rows per poly than limbs", who);
  if (((uintptr_t)q & 7) || ((uintptr_t)p & 7) || ((uintptr_t)out & 7)) return rh_fail(RH_ERR_ARG, "%s: every block must be 8-byte aligned", who);
  if (int rc = rh_moduli_below(rQ, LQ, LC_MODULUS_BITS, LC_CHUNK, who, rP ? " of Q" : "")) return rc;
  if (rP) if (int rc = rh_moduli_below(rP, LP, LC_MODULUS_BITS, LC_CHUNK, who, " of P")) return rc;
  if (!npoly) return RH_OK;

  // lanes per chunk: the digit image of a chunk, (L + 2) rows of C + 1 words, the two extreme vectors and the tournament fit 64 KiB
  const unsigned n = (unsigned)(rQ->N / gap);
  unsigned C = 256;
  auto lds_bytes = [&](unsigned c) { return ((size_t)(L + 2) * (c + 1) + 2 * (size_t)L) * 8 + (2 * (size_t)c + 4) * 4; };
  while (C > 32 && (lds_bytes(C) > 65536 || C / 2 >= n)) C >>= 1;
  const unsigned nchunks = (n + C - 1) / C;
  const size_t NP = noise_pairs(L), W = rh_ring_centered_moments_words(L), tw = noise_table_words(L);
  const int PPT = (int)((NP + 255) / 256);
  // workgroups per poly: enough of them to fill the device, few enough that the partials stay small; polys per launch under 256 MiB of partials
  unsigned G = 2048u / (unsigned)(npoly < 2048 ? npoly : 2048); if (G < 1) G = 1; if (G > nchunks) G = nchunks;
  size_t per_launch = ((size_t)32 << 20) / ((size_t)G * W); if (per_launch < 1) per_launch = 1; if (per_launch > (size_t)npoly) per_launch = (size_t)npoly;
  if (per_launch > 65535) per_launch = 65535;

  std::lock_guard<std::recursive_mutex> lk(rQ->mu);
  (void)rh_stream_begin(rQ, (unsigned)npoly);
  hipStream_t st = rh_stream(rQ);
  if (int rc = noise_scratch(rQ, tw + per_launch * G * W, who)) return rc;
  RhStage* stage;
  if (int rc = rh_stage_slot(tw, &stage, who)) return rc;
  if (int rc = noise_tables(rQ, LQ, rP, LP, stage->h, who)) return rc;
  if (int rc = rh_stage_upload(stage, rQ->d_noise, tw, st, who)) return rc;
  NoiseTables tb;
  tb.c = reinterpret_cast<const LimbConsts*>(rQ->d_noise);
  tb.garner = rQ->d_noise + (size_t)L * (sizeof(LimbConsts) / 8); tb.rmod = tb.garner + L; tb.half = tb.rmod + (size_t)L * L; tb.pairs = tb.half + L;
  NoiseMomArgs a;
  a.q_rows = q_rows; a.p_rows = p_rows; a.LQ = LQ; a.L = L;
  a.N = (unsigned)rQ->N; a.n = n; a.gap = (unsigned)gap; a.C = C; a.CS = C + 1; a.nchunks = nchunks; a.NP = (unsigned)NP; a.W = (unsigned)W;
  a.part = rQ->d_noise + tw;
  for (size_t p0 = 0; p0 < (size_t)npoly; p0 += per_launch) {
    const unsigned pc = (unsigned)((size_t)npoly - p0 < per_launch ? (size_t)npoly - p0 : per_launch);
    a.q = q + p0 * (size_t)q_rows * a.N; a.p = p ? p + p0 * (size_t)p_rows * a.N : nullptr;
    const dim3 grid(G, pc);
    if (!rh_with_s1<1, NOISE_MAX_PPT>(PPT, [&](auto S) { noise_moments_kernel<decltype(S)::value><<<grid, 256, lds_bytes(C), st>>>(a, tb); }))
      return rh_fail(RH_ERR_UNSUPPORTED, "%s: %zu pair sums exceed the %d per thread the kernel is built for", who, NP, NOISE_MAX_PPT);
    if (int rc = rh_launch_ok("noise_moments_kernel")) return rc;
    noise_moments_reduce_kernel<<<pc, 256, 0, st>>>(a.part, out + p0 * W, G, (unsigned)NP, (unsigned)W, L);
    if (int rc = rh_launch_ok("noise_moments_reduce_kernel")) return rc;
  }
  return RH_OK;
}

// ---- the phase of gadget ciphertexts ---------------------------------------------------------------------------------------------------------------
extern "C" size_t rh_rlwe_gadget_phase_table_words(int levelQ, int outs, int max_terms) {
  if (levelQ < 0 || outs < 0 || max_terms < 0) return 0;
  return (size_t)outs * (size_t)(NOISE_PHASE_HEAD + max_terms + levelQ + 1);
}

extern "C" int rh_rlwe_gadget_phase(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* skQ, const uint64_t* skP, int nsk, const uint64_t* ptQ,
                                    int npt, uint64_t* outQ, uint64_t* outP, const uint64_t* rowtab, int outs, int max_terms, uint64_t* table_dev,
                                    size_t table_words) {
  const char* who = "rh_rlwe_gadget_phase";
  if (!rQ) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (rQ->kind == RH_RING_CI) return rh_fail(RH_ERR_UNSUPPORTED, "%s: conjugate-invariant rings are not supported", who);
  if (rQ->N < 4 || (rQ->N & 1)) return rh_fail(RH_ERR_ARG, "%s: N < 4, or odd", who);
  if (levelQ < 0 || levelQ >= rQ->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, levelQ, rQ->L);
  if (rP) {
    if (rP->kind != rQ->kind) return rh_fail(RH_ERR_UNSUPPORTED, "%s: ringQ and ringP must be of the same kind", who);
    if (rP->N != rQ->N || rP->device != rQ->device) return rh_fail(RH_ERR_ARG, "%s: ringQ and ringP differ in degree or device", who);
    if (levelP < 0 || levelP >= rP->L) return rh_fail(RH_ERR_ARG, "%s: levelP %d out of range [0,%d)", who, levelP, rP->L);
  }
  const int LQ = levelQ + 1, LP = rP ? levelP + 1 : 0;
  if (outs < 0 || max_terms < 1 || nsk < 1 || npt < 0) return rh_fail(RH_ERR_ARG, "%s: outs < 0, max_terms < 1, nsk < 1 or npt < 0", who);
  if (!skQ || !outQ || !rowtab || !table_dev || (npt && !ptQ)) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((rP != nullptr) != (skP && outP) || (!rP && (skP || outP))) return rh_fail(RH_ERR_ARG, "%s: skP and outP go with ringP, both or none", who);
  if (int rc = rh_moduli_below(rQ, LQ, LC_MODULUS_BITS, LC_CHUNK, who, rP ? " of Q" : "")) return rc;
  if (rP) if (int rc = rh_moduli_below(rP, LP, LC_MODULUS_BITS, LC_CHUNK, who, " of P")) return rc;
  const size_t stride = (size_t)(NOISE_PHASE_HEAD + max_terms + LQ), words = (size_t)outs * stride;
  if (table_words < words) return rh_fail(RH_ERR_ARG, "%s: the row table needs %zu words, the caller's has %zu", who, words, table_words);
  if ((size_t)outs * (size_t)(LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  const size_t N = (size_t)rQ->N, O = (size_t)outs;
  RhBlock wr[3] = {{outQ, O * LQ * N}, {outP, O * LP * N}, {table_dev, words}};
  size_t key_rows = 0;
  for (int o = 0; o < outs; ++o) {
    const u64* t = rowtab + (size_t)o * stride;
    if (!t[0] || (t[0] & 15) || (rP && (!t[1] || (t[1] & 15)))) return rh_fail(RH_ERR_ARG, "%s: output %d names a null or misaligned key table", who, o);
    if (t[3] >= (u64)nsk) return rh_fail(RH_ERR_ARG, "%s: output %d names secret %llu of %d", who, o, (unsigned long long)t[3], nsk);
    if (t[4] != NOISE_NO_PT && t[4] >= (u64)npt) return rh_fail(RH_ERR_ARG, "%s: output %d names plaintext %llu of %d", who, o, (unsigned long long)t[4], npt);
    if (t[5] < 1 || t[5] > (u64)max_terms) return rh_fail(RH_ERR_ARG, "%s: output %d sums %llu rows, 1 to max_terms = %d expected", who, o, (unsigned long long)t[5], max_terms);
    if (t[2] > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: output %d: a key of %llu rows", who, o, (unsigned long long)t[2]);
    for (u64 k = 0; k < t[5]; ++k)
      if (t[NOISE_PHASE_HEAD + k] >= t[2]) return rh_fail(RH_ERR_ARG, "%s: output %d names row %llu of a key of %llu", who, o, (unsigned long long)t[NOISE_PHASE_HEAD + k], (unsigned long long)t[2]);
    for (int l = 0; l < LQ; ++l)
      if (t[NOISE_PHASE_HEAD + max_terms + l] >= rQ->moduli[l]) return rh_fail(RH_ERR_ARG, "%s: the scalar of output %d is not a residue of limb %d", who, o, l);
    const RhBlock rd[2] = {{(const void*)(uintptr_t)t[0], (size_t)t[2] * 2 * LQ * N}, {(const void*)(uintptr_t)t[1], rP ? (size_t)t[2] * 2 * LP * N : 0}};
    if (int rc = rh_blocks_ok(wr, 3, rd, 2, who, "an output overlaps a key table")) return rc;
    key_rows += (size_t)t[5];
  }
  const RhBlock rd[3] = {{skQ, (size_t)nsk * LQ * N}, {skP, (size_t)nsk * LP * N}, {ptQ, (size_t)npt * LQ * N}};
  if (int rc = rh_blocks_ok(wr, 3, rd, 3, who, "an output overlaps a secret or a plaintext")) return rc;
  if (int rc = rh_blocks_disjoint(wr, 3, who, "two outputs overlap")) return rc;
  if (!outs) return RH_OK;
  const size_t rows_moved = 2 * key_rows * (size_t)(LQ + LP) + O * (size_t)(LQ + LP);        // both components of every row read, the phase written
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)(rows_moved > 0x7fffffffu ? 0x7fffffffu : rows_moved));
  hipStream_t st = rh_stream(rQ);
  RhStage* stage;
  if (int rc = rh_stage_slot(words, &stage, who)) return rc;
  memcpy(stage->h, rowtab, words * 8);
  if (int rc = rh_stage_upload(stage, table_dev, words, st, who)) return rc;
  const GadgetPhaseArgs a{skQ, skP, ptQ, outQ, outP, table_dev, (unsigned)stride, (unsigned)max_terms};
  rlwe_gadget_phase_kernel<<<dim3((unsigned)outs * (unsigned)(LQ + LP), g.grid.y), 256, 0, st>>>(a, (unsigned)N, rQ->d_consts, rP ? rP->d_consts : rQ->d_consts, LQ, LP, g.nt);
  return rh_launch_ok("rlwe_gadget_phase_kernel");
}

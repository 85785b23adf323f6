// ring_packing.hip -- core/rlwe/ring_packing.go on device batches: the entries of the five kernels of ring_packing_kernels.hip.hpp (one level of
// Expand, the two halves of one level of Pack, the coefficient maps of Split and Merge) and Expand (:475-594) as one C-ABI call.
//
// The key switches are the library's own (rh_bext_gadget_product_then_add); what is here is everything the reference does around them.  A level
// of Expand or Pack is ONE launch sequence over all its ciphertexts: they share the Galois element.  Scratch: the extender's buffer 10 (the
// un-permuted output of the key switch), grown on demand.
#include <hip/hip_runtime.h>
#include <cstring>
#include <vector>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "ring_packing_kernels.hip.hpp"
#include "qp_rows_host.hpp"

static_assert(sizeof(RpEntry) == 3 * sizeof(int32_t), "the plan of a Pack level is a table of int32 triples");

// The plan of a Pack level as the host holds it: every entry in range, and no slot written twice (a written slot is `a` of AB, `b` of B, and the
// slot the finishing kernel adds to: `a` of A and AB, `b` of B) or read by another entry
static int rp_table(const int32_t* table_host, int K, int nslots, const char* who) {
  if (!table_host) return rh_fail(RH_ERR_ARG, "%s: the host copy of the table is needed to check it", who);
  std::vector<char> seen((size_t)nslots, 0);
  for (int k = 0; k < K; ++k) {
    const int mode = table_host[3 * k], a = table_host[3 * k + 1], b = table_host[3 * k + 2];
    if (mode < RP_MODE_A || mode > RP_MODE_AB || a < 0 || a >= nslots || b < 0 || b >= nslots)
      return rh_fail(RH_ERR_ARG, "%s: entry %d (%d, %d, %d) is out of range for %d slots", who, k, mode, a, b, nslots);
    const int used[2] = {mode == RP_MODE_B ? b : a, mode == RP_MODE_AB ? b : -1};
    for (int s : used) {
      if (s < 0) continue;
      if (seen[s]) return rh_fail(RH_ERR_ARG, "%s: slot %d is named by two entries", who, s);
      seen[s] = 1;
    }
  }
  return RH_OK;
}

// One level of Expand (ring_packing.go:555-575); see ringhip.h
extern "C" int rh_rlwe_expand_step(rh_ring* r, int level, uint64_t gen, const uint64_t* tmp0, const uint64_t* tmp1, uint64_t* ct0, uint64_t* ct1,
                                   const uint64_t* xpow, int cnt) {
  const char* who = "expand_step";
  if (int rc = rh_ring_ok(r, level, cnt, who)) return rc;
  if (!tmp0 || !tmp1 || !ct0 || !ct1 || !xpow) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const size_t w = (size_t)cnt * (level + 1) * r->N;
  {
    const RhBlock wr[2] = {{ct0, 2 * w}, {ct1, 2 * w}}, rd[3] = {{tmp0, w}, {tmp1, w}, {xpow, (size_t)(level + 1) * r->N}};
    if (int rc = rh_blocks_ok(wr, 2, rd, 3, who, "the permuted operand and the table cannot overlap the batch")) return rc;
    if (int rc = rh_blocks_disjoint(wr, 2, who, "the two components of the batch overlap")) return rc;
  }
  u32 g; if (int rc = is_gen(r, gen, who, &g)) return rc;
  if (!cnt) return RH_OK;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * (unsigned)cnt * (unsigned)(level + 1));
  expand_step_kernel<<<sg.grid, 256, 0, rh_stream(r)>>>(ct0, ct1, tmp0, tmp1, xpow, r->logN, g, r->d_consts, level + 1, cnt, sg.nt);
  return rh_launch_ok("expand_step_kernel");
}

// Before the key switch of one level of Pack (ring_packing.go:726-745); see ringhip.h
extern "C" int rh_rlwe_pack_combine(rh_ring* r, int level, uint64_t* ct0, uint64_t* ct1, int nslots, const int32_t* table_dev, const int32_t* table_host,
                                    int K, const uint64_t* xpow, uint64_t* u0, uint64_t* u1) {
  const char* who = "pack_combine";
  if (int rc = rh_ring_ok(r, level, K, who)) return rc;
  if (!ct0 || !ct1 || !u0 || !u1 || !xpow || !table_dev || nslots <= 0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (int rc = rp_table(table_host, K, nslots, who)) return rc;
  const size_t row = (size_t)(level + 1) * r->N;
  {
    const RhBlock wr[4] = {{ct0, nslots * row}, {ct1, nslots * row}, {u0, K * row}, {u1, K * row}}, rd[1] = {{xpow, row}};
    if (int rc = rh_blocks_ok(wr, 4, rd, 1, who, "the table of powers of X cannot overlap a written block")) return rc;
    if (int rc = rh_blocks_disjoint(wr, 4, who, "the batch and the key-switch operand overlap")) return rc;
  }
  if (!K) return RH_OK;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * (unsigned)K * (unsigned)(level + 1));
  pack_combine_kernel<<<sg.grid, 256, 0, rh_stream(r)>>>(ct0, ct1, u0, u1, xpow, reinterpret_cast<const RpEntry*>(table_dev), r->logN, r->d_consts,
                                                        level + 1, K, nslots, sg.nt);
  return rh_launch_ok("pack_combine_kernel");
}

// After the key switch of one level of Pack (ring_packing.go:768-769, :786-787); see ringhip.h
extern "C" int rh_rlwe_rotate_addsub_q(rh_ring* r, int level, uint64_t gen, const uint64_t* tmp0, const uint64_t* tmp1, uint64_t* ct0, uint64_t* ct1,
                                       int nslots, const int32_t* table_dev, const int32_t* table_host, int K) {
  const char* who = "rotate_addsub_q";
  if (int rc = rh_ring_ok(r, level, K, who)) return rc;
  if (!tmp0 || !tmp1 || !ct0 || !ct1 || !table_dev || nslots <= 0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (int rc = rp_table(table_host, K, nslots, who)) return rc;
  const size_t row = (size_t)(level + 1) * r->N;
  {
    const RhBlock wr[2] = {{ct0, nslots * row}, {ct1, nslots * row}}, rd[2] = {{tmp0, K * row}, {tmp1, K * row}};
    if (int rc = rh_blocks_ok(wr, 2, rd, 2, who, "the permuted operand cannot overlap the batch it is added to")) return rc;
    if (int rc = rh_blocks_disjoint(wr, 2, who, "the two components of the batch overlap")) return rc;
  }
  u32 g; if (int rc = is_gen(r, gen, who, &g)) return rc;
  if (!K) return RH_OK;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * (unsigned)K * (unsigned)(level + 1));
  rotate_addsub_q_kernel<<<sg.grid, 256, 0, rh_stream(r)>>>(ct0, ct1, tmp0, tmp1, reinterpret_cast<const RpEntry*>(table_dev), r->logN, g, r->d_consts,
                                                           level + 1, K, nslots, sg.nt);
  return rh_launch_ok("rotate_addsub_q_kernel");
}

static int rp_gap(const rh_ring* r, int logGap, const char* who) {
  if (logGap < 1 || logGap > r->logN - 1) return rh_fail(RH_ERR_ARG, "%s: need 1 <= logGap <= logN - 1 (a small ring of degree >= 2)", who);
  return RH_OK;
}

// X -> Y = X^gap on coefficient-domain rows (element.go:256-268, :302-308) and Split's odd half (ring_packing.go:239-241); see ringhip.h
extern "C" int rh_rlwe_ring_split(rh_ring* r, int level, const uint64_t* in0, const uint64_t* in1, uint64_t* even0, uint64_t* even1, uint64_t* odd0,
                                  uint64_t* odd1, int logGap, int npoly) {
  const char* who = "ring_split";
  if (int rc = rh_ring_ok(r, level, npoly, who)) return rc;
  if (int rc = rp_gap(r, logGap, who)) return rc;
  if (!in0 || !in1 || !even0 || !even1 || (odd0 == nullptr) != (odd1 == nullptr)) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const size_t w = (size_t)npoly * (level + 1) * r->N, ws = w >> logGap;
  {
    const RhBlock wr[4] = {{even0, ws}, {even1, ws}, {odd0, ws}, {odd1, ws}}, rd[2] = {{in0, w}, {in1, w}};
    const int nw = odd0 ? 4 : 2;
    if (int rc = rh_blocks_ok(wr, nw, rd, 2, who, "an output cannot overlap the input")) return rc;
    if (int rc = rh_blocks_disjoint(wr, nw, who, "two outputs overlap")) return rc;
  }
  if (!npoly) return RH_OK;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * (unsigned)npoly * (unsigned)(level + 1));
  ring_split_kernel<<<sg.grid, 256, 0, rh_stream(r)>>>(in0, in1, even0, even1, odd0, odd1, r->logN, r->logN - logGap, sg.nt);
  return rh_launch_ok("ring_split_kernel");
}

// Y = X^gap -> X in the NTT domain (ring/operations.go:380-392) and Merge's sum (ring_packing.go:429-434); see ringhip.h
extern "C" int rh_rlwe_ring_merge(rh_ring* r, int level, const uint64_t* even0, const uint64_t* even1, const uint64_t* odd0, const uint64_t* odd1,
                                  const uint64_t* xpow, uint64_t* out0, uint64_t* out1, int logGap, int npoly) {
  const char* who = "ring_merge";
  if (int rc = rh_ring_ok(r, level, npoly, who)) return rc;
  if (int rc = rp_gap(r, logGap, who)) return rc;
  if (!even0 || !even1 || !out0 || !out1 || (odd0 == nullptr) != (odd1 == nullptr)) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (odd0 && !xpow) return rh_fail(RH_ERR_ARG, "%s: an odd operand needs the table of X", who);
  const size_t w = (size_t)npoly * (level + 1) * r->N, ws = w >> logGap;
  {
    const RhBlock wr[2] = {{out0, w}, {out1, w}};
    const RhBlock rd[5] = {{even0, ws}, {even1, ws}, {odd0, ws}, {odd1, ws}, {xpow, (size_t)(level + 1) * r->N}};
    if (int rc = rh_blocks_ok(wr, 2, rd, odd0 ? 5 : 2, who, "the output cannot overlap an input")) return rc;
    if (int rc = rh_blocks_disjoint(wr, 2, who, "the two outputs overlap")) return rc;
  }
  if (!npoly) return RH_OK;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * (unsigned)npoly * (unsigned)(level + 1));
  ring_merge_kernel<<<sg.grid, 256, 0, rh_stream(r)>>>(even0, even1, odd0, odd1, odd0 ? xpow : nullptr, out0, out1, r->logN, r->logN - logGap, r->d_consts,
                                                      level + 1, sg.nt);
  return rh_launch_ok("ring_merge_kernel");
}

// ---- Expand (ring_packing.go:475-594) -----------------------------------------------------------------------------------------------------
extern "C" int rh_rlwe_expand(rh_bext* be, int levelQ, int levelP, uint64_t* ct0, uint64_t* ct1, int nin, int logGap, const uint64_t* xinvpow,
                              int xrows, const rh_galois_key* keys, int nkeys) {
  const char* who = "expand";
  if (!be) return rh_fail(RH_ERR_ARG, "%s: null basis extender", who);
  rh_ring *RQ = rh_bext_ringQ(be), *RP = rh_bext_ringP(be);
  if (!RP) return rh_fail(RH_ERR_ARG, "%s: basis extender has no P ring", who);
  if (RQ->kind != RH_RING_STANDARD || RP->kind != RH_RING_STANDARD)
    return rh_fail(RH_ERR_UNSUPPORTED, "method is only supported for ring.Type = ring.Standard (X^{-2^{i}} does not exist in the sub-ring Z[X + X^{-1}])");
  if (levelP < 1 || levelP >= RP->L) return rh_fail(RH_ERR_UNSUPPORTED, "%s: need 1 <= levelP < %d (keys with one P modulus are not supported by this call)", who, RP->L);
  const int logN = RQ->logN, N = RQ->N;
  if (logGap < 0 || logGap > logN) return rh_fail(RH_ERR_ARG, "%s: need 0 <= logGap <= logN", who);
  const size_t nout = (size_t)nin << (logN - logGap);
  if (nin < 0 || nout > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: bad ciphertext count", who);
  if (int rc = rh_ring_ok(RQ, levelQ, (int)nout, who)) return rc;
  if (!ct0 || !ct1 || !xinvpow || (nkeys > 0 && !keys) || nkeys < 0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (xrows < levelQ + 1) return rh_fail(RH_ERR_ARG, "%s: the table of X^(-2^i) has %d limbs, the level needs %d", who, xrows, levelQ + 1);
  const int LQ = levelQ + 1, beta = (levelQ + levelP + 1) / (levelP + 1);
  std::vector<const rh_galois_key*> key((size_t)logN, nullptr);
  for (int i = 0; i < logN; ++i) {                      // every key before the first launch
    const u64 gen = (u64)(N >> i) + 1;
    for (int k = 0; k < nkeys && !key[i]; ++k) if (keys[k].galois_element == gen) key[i] = &keys[k];
    if (!key[i]) return rh_fail(RH_ERR_ARG, "%s: GaloisKey[%llu] is missing", who, (unsigned long long)gen);
    if (!key[i]->evkQ_dev || !key[i]->evkP_dev) return rh_fail(RH_ERR_ARG, "%s: GaloisKey[%llu] has a null part", who, (unsigned long long)gen);
    if (key[i]->digits < beta) return rh_fail(RH_ERR_ARG, "%s: GaloisKey[%llu] has %d digits, level needs %d", who, (unsigned long long)gen, key[i]->digits, beta);
  }
  if (!nin) return RH_OK;
  RhBextGuard guard(be);
  (void)hipSetDevice(RQ->device);
  const size_t row = (size_t)LQ * N, half = nout > (size_t)nin ? nout / 2 : (size_t)nin;      // the largest live prefix a key switch reads
  u64* tmp;
  if (int rc = rh_bext_scratch(be, 10, 2 * half * row, &tmp)) return rc;
  u64 *tmp0 = tmp, *tmp1 = tmp + half * row;
  {                                                     // times 2^-logN mod Q (:523-528)
    u64 s[RH_MAX_LIMBS];
    for (int i = 0; i < LQ; ++i) {
      const u64 q = RQ->moduli[i];
      s[i] = rh::mform(rh::powmod(((u64)1 << logN) % q, q - 2, q), q);
    }
    if (int rc = rh_ring_vec_op(RQ, RH_OP_MUL_SCALAR_MONT, ct0, nullptr, ct0, nin, levelQ, s, nullptr)) return rc;
    if (int rc = rh_ring_vec_op(RQ, RH_OP_MUL_SCALAR_MONT, ct1, nullptr, ct1, nin, levelQ, s, nullptr)) return rc;
  }
  const int gap = 1 << logGap;
  for (int i = 0; i < logN; ++i) {
    const int n = 1 << i;
    const u64 gen = (u64)(N >> i) + 1;
    const int cnt = n >= gap ? (n / gap) * nin : nin;   // the live prefix: slot-major, it doubles with every level that has a second output
    if (int rc = rh_bext_gadget_product_then_add(be, levelQ, levelP, ct1, key[i]->evkQ_dev, key[i]->evkP_dev, key[i]->digits, ct0, nullptr, tmp0, tmp1, cnt)) return rc;
    if (n >= gap) { if (int rc = rh_rlwe_expand_step(RQ, levelQ, gen, tmp0, tmp1, ct0, ct1, xinvpow + (size_t)i * xrows * N, cnt)) return rc; }
    else if (int rc = rh_rlwe_rotate_add_q(RQ, levelQ, gen, tmp0, tmp1, ct0, ct1, cnt)) return rc;
  }
  return RH_OK;
}

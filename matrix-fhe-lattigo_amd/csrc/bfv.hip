// bfv.hip -- the BFV ciphertext multiply (scale-invariant tensoring) on device-resident (poly, limb, coefficient) blocks.
//
// Replaces schemes/bgv/evaluator.go: newEvaluatorPrecomp (:46-78), tensorScaleInvariant (:975-1014), modUpAndNTT (:1053-1060),
// tensorLowDeg (:1062-1102) and quantize (:1104-1124).  The transforms, ModUpQtoP and the relinearisation's gadget product are the
// existing entry points; two kernels are new:
//
//   bfv_tensor_kernel     tensorLowDeg for BOTH rings in one launch: the level+1 limbs of Q and the levelQMul+1 limbs of QMul are rows
//                         of one grid, each block with its own ring's constants and row stride.  MForm of operand 0 folded in,
//                         c0 = MRed(c00, b0), c2 = MRed(c01, b1), c1 = MRed(c00, b1) + MRed(c01, b0) NOT reduced (in [0, 2q), as
//                         MulCoeffsMontgomeryThenAddLazy leaves it); squaring: two inputs per ring, c1 = 2 * MRed(c00, a1) (AddLazy).
//                         Traffic: 8 * 7 bytes per coefficient and limb (8 * 5 when squaring) instead of the 8 * 17 of the eight ring calls.
//   bfv_quantize_kernel   the middle of quantize, one thread per coefficient: ModDownQPtoP (ring/basis_extension.go:264-278) then
//                         ModUpPtoQ (:205-217) then MulScalar by T (ring/operations.go:201-205: MRed by MForm(T)), with the
//                         levelQMul+1 words between the two extensions in registers.  Traffic: 8 * (2 (level+1) + (levelQMul+1)) bytes
//                         per coefficient instead of the 8 * (4 (level+1) + 3 (levelQMul+1)) of the three launches.
//                         Both extensions are the functions of bext_kernels.hip.hpp on the extender's own plans: the two float sums
//                         of reconstructRNS are computed exactly as bext_kernel computes them, one after the other.
//
// Which quantize a shape gets:  by default EVERY shape takes the composed sequence rh_bext_moddown_qp_to_p, rh_bext_modup_p_to_q, MulScalar on
// the handle's scratch: measured at N = 2^15, 8 + 7 limbs, batch 64, the fused kernel's gain on a whole quantize (a few percent) was inside the
// run-to-run spread of the timing windows (profiles/bfv_ops.json).  The tuning key "fused_quantize" = 1 selects
// bfv_quantize_kernel for level+1 <= 8 and levelQMul+1 <= 8 (instantiated per pair of limb counts, every y_i and every intermediate word in
// registers, at most 92 VGPRs: 5 waves per SIMD); larger shapes, up to the 32 source limbs of basis_extension.go:285, take the composed
// sequence whatever the key says.  Same values either way; rh_bfv_quantize_path tells which one a level takes.
#include <hip/hip_runtime.h>
#include <vector>
#include <cstring>
#include <utility>
#include "engine_internal.hpp"
#include "bext_internal.hpp"
#include "bext_kernels.hip.hpp"
#include "stream_kernels.hip.hpp"
#include "hostmath.hpp"

// ---------------------------------------------------------------------------------------------------------------
// tensorLowDeg, both rings
// ---------------------------------------------------------------------------------------------------------------
struct BfvTensorSide {
  const u64 *a0, *a1, *b0, *b1;
  u64 *c0, *c1, *c2;
  const LimbConsts* consts;
  int rows;                        // limbs per poly of this ring's blocks
};

// grid: (npoly * (rowsQ + rowsM), chunks); row u of a poly is limb u of Q (u < rowsQ) or limb u - rowsQ of QMul: a row mapping of its own,
// so of the scaffold (stream_kernels.hip.hpp) it takes the pair loop and the load / store pair, not StreamRow.
// Outputs may alias inputs element-wise.
template <bool SQUARE>
__global__ void __launch_bounds__(256)
bfv_tensor_kernel(BfvTensorSide sq, BfvTensorSide sm, unsigned n, int nt) {
  const u32 per = (u32)(sq.rows + sm.rows);
  const u32 poly = blockIdx.x / per, u = blockIdx.x % per;
  const bool inQ = u < (u32)sq.rows;
  const BfvTensorSide& s = inQ ? sq : sm;
  const u32 limb = inQ ? u : u - (u32)sq.rows;
  const LimbConsts c = s.consts[limb];
  const size_t ro = ((size_t)poly * s.rows + limb) * n;
  auto one = [&](u64 x0, u64 x1, u64 y0, u64 y1, u64& r0, u64& r1, u64& r2) {
    const u64 m0 = mform(x0, c.q, c.bred0, c.bred1), m1 = mform(x1, c.q, c.bred0, c.bred1);
    if (SQUARE) {
      r0 = mred(m0, x0, c.q, c.qinv); r2 = mred(m1, x1, c.q, c.qinv);
      const u64 t = mred(m0, x1, c.q, c.qinv);
      r1 = t + t;
    } else {
      r0 = mred(m0, y0, c.q, c.qinv); r2 = mred(m1, y1, c.q, c.qinv);
      r1 = mred(m0, y1, c.q, c.qinv) + mred(m1, y0, c.q, c.qinv);
    }
  };
  RH_FOR_EACH_PAIR(i, 0, n >> 1) {
    const size_t o = ro + 2 * (size_t)i;
    const ulonglong2 x0 = rh_ld2(s.a0 + o, nt), x1 = rh_ld2(s.a1 + o, nt);
    ulonglong2 y0 = make_ulonglong2(0, 0), y1 = y0;
    if (!SQUARE) { y0 = rh_ld2(s.b0 + o, nt); y1 = rh_ld2(s.b1 + o, nt); }
    u64 lo0, lo1, lo2, hi0, hi1, hi2;
    one(x0.x, x1.x, y0.x, y1.x, lo0, lo1, lo2);
    one(x0.y, x1.y, y0.y, y1.y, hi0, hi1, hi2);
    rh_st2(s.c0 + o, make_ulonglong2(lo0, hi0), nt); rh_st2(s.c1 + o, make_ulonglong2(lo1, hi1), nt); rh_st2(s.c2 + o, make_ulonglong2(lo2, hi2), nt);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// quantize: ModDownQPtoP -> ModUpPtoQ -> MulScalar(T), one thread per coefficient
// ---------------------------------------------------------------------------------------------------------------
struct BfvQuantArgs {
  // stage 1: the extender's plan {ModUp + ModDown, Q -> QMul} at (level, levelQMul); stage 2: its plan {ModUp, QMul -> Q} at (levelQMul, level)
  const BextSource* S1; const BextTarget* T1; const u64* coef1; const u64* vt1;
  const BextSource* S2; const BextTarget* T2; const u64* coef2; const u64* vt2;
  const u64* tmont;                // MForm(T) per limb of Q
};

// NQ = level+1 words of Q, NM = levelQMul+1 words of QMul, both canonical and in the coefficient domain; dense blocks (npoly, NQ, N) and
// (npoly, NM, N); out: (npoly, NQ, N), may be inQ (a thread holds all its words before it writes one).
// dynamic LDS: vt of stage 1 [NM][NQ+1], then vt of stage 2 [NQ][NM+1] (no global loads between the stores: bext.hip on the vt table).
template <int NQ, int NM>
__global__ void __launch_bounds__(256)
bfv_quantize_kernel(const u64* inQ, const u64* inM, u64* out, BfvQuantArgs a, int N) {
  extern __shared__ u64 dyn_lds[];
  const int tid = threadIdx.x;
  constexpr int W1 = NM * (NQ + 1), W2 = NQ * (NM + 1);
  u64* const vt1 = dyn_lds;
  u64* const vt2 = dyn_lds + W1;
  for (int i = tid; i < W1; i += 256) vt1[i] = a.vt1[i];
  for (int i = tid; i < W2; i += 256) vt2[i] = a.vt2[i];
  __syncthreads();
  const int k = blockIdx.x * 256 + tid;
  const int poly = blockIdx.y;
  const bool live = k < N;
  // ---- ModDownQPtoP: reconstructRNS over the Q words, then per QMul word multSum, centred subtraction, (other - ext) * Q^-1
  u64 y[NQ];
  double vi = 0.0;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const u64 x = live ? inQ[((size_t)poly * NQ + i) * N + k] : 0;
    y[i] = bext_source(x, a.S1[i], BEXT_ADD_CRED, vi);
  }
  const int v = (int)(u64)vi;
  u64 z[NM];
#pragma unroll
  for (int j = 0; j < NM; ++j) {
    const BextTarget t = a.T1[j];
    u64 rlo, rhi;
    bext_mult_sum<NQ, true>(y, NQ, a.coef1 + (size_t)j * NQ, rlo, rhi);
    u64 r = bext_post_center(bext_close(rlo, rhi, t, vt1[j * (NQ + 1) + v]), t);
    const u64 other = live ? inM[((size_t)poly * NM + j) * N + k] : 0;
    z[j] = bext_post_moddown(r, other, t);                                 // canonical
  }
  // ---- ModUpPtoQ on those words, then MulScalar: MRed by MForm(T)
  double vi2 = 0.0;
#pragma unroll
  for (int j = 0; j < NM; ++j) z[j] = bext_source(z[j], a.S2[j], BEXT_ADD_CRED, vi2);
  const int v2 = (int)(u64)vi2;
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const BextTarget t = a.T2[i];
    u64 rlo, rhi;
    bext_mult_sum<NM, true>(z, NM, a.coef2 + (size_t)i * NM, rlo, rhi);
    u64 r = bext_post_center(bext_close(rlo, rhi, t, vt2[i * (NM + 1) + v2]), t);
    r = mred(r, a.tmont[i], t.p, t.pinv);                                  // mulscalarmontgomeryvec
    if (live) out[((size_t)poly * NQ + i) * N + k] = r;
  }
}

typedef void (*bfv_quant_fn)(const u64*, const u64*, u64*, BfvQuantArgs, int);
template <int... I>
static const bfv_quant_fn* bfv_quant_table(std::integer_sequence<int, I...>) {
  static const bfv_quant_fn t[] = {bfv_quantize_kernel<I / 8 + 1, I % 8 + 1>...};
  return t;
}

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
struct rh_bfv {
  rh_ring* Q = nullptr; rh_ring* M = nullptr;
  u64 t = 0;
  rh_bext* be = nullptr;                              // NewBasisExtender(ringQ, ringQMul) (:66)
  std::vector<int> level_qmul;                        // :51-56
  std::vector<u64> tmont;                             // MForm(T, q_i): the scalar MulScalar multiplies by
  u64* d_tmont = nullptr;
  u64* buf[2] = {nullptr, nullptr}; size_t buf_words[2] = {0, 0};     // 0: Q scratch (4 blocks), 1: QMul scratch (4 blocks)
  int fused_quantize = 0;                             // see the header: composed by default, the fused kernel on request
  std::recursive_mutex mu;
};

// bit length of q_0 * ... * q_i for every i
static std::vector<int> product_bitlens(const std::vector<u64>& mods) {
  std::vector<u64> acc{1};
  std::vector<int> out;
  for (u64 q : mods) {
    u64 carry = 0;
    for (u64& w : acc) { const rh::u128 p = (rh::u128)w * q + carry; w = (u64)p; carry = (u64)(p >> 64); }
    if (carry) acc.push_back(carry);
    out.push_back(64 * (int)(acc.size() - 1) + 64 - __builtin_clzll(acc.back()));
  }
  return out;
}

extern "C" int rh_bfv_create(rh_bfv** out, rh_ring* ringQ, rh_ring* ringQMul, uint64_t t) {
  if (!out || !ringQ || !ringQMul) return rh_fail(RH_ERR_ARG, "rh_bfv_create: null argument");
  if (ringQ->kind != RH_RING_STANDARD || ringQMul->kind != RH_RING_STANDARD)
    return rh_fail(RH_ERR_ARG, "rh_bfv_create: scale-invariant tensoring needs standard rings (3N and conjugate-invariant rings are not supported)");
  if (ringQ->N != ringQMul->N || ringQ->device != ringQMul->device) return rh_fail(RH_ERR_ARG, "rh_bfv_create: ringQ and ringQMul differ in N or device (%d, %d)", ringQ->N, ringQMul->N);
  if (ringQ->N < 16) return rh_fail(RH_ERR_ARG, "rh_bfv_create: N = %d < 16 (INTTLazy is not canonical below 16, ring/ntt.go:197-202)", ringQ->N);
  if (t == 0) return rh_fail(RH_ERR_ARG, "rh_bfv_create: plaintext modulus is zero");
  if (t > ringQ->moduli[0]) return rh_fail(RH_ERR_ARG, "rh_bfv_create: plaintext modulus %llu exceeds q_0 = %llu", (unsigned long long)t, (unsigned long long)ringQ->moduli[0]);
  for (u64 q : ringQ->moduli) {
    if (q == t) return rh_fail(RH_ERR_ARG, "rh_bfv_create: plaintext modulus %llu is a modulus of Q", (unsigned long long)t);
    for (u64 p : ringQMul->moduli) if (p == q) return rh_fail(RH_ERR_ARG, "rh_bfv_create: Q and QMul share the modulus %llu", (unsigned long long)q);
  }
  rh_bfv* b = new rh_bfv();
  b->Q = ringQ; b->M = ringQMul; b->t = t;
  const std::vector<int> bits = product_bitlens(ringQ->moduli);
  for (int i = 0; i < ringQ->L; ++i) b->level_qmul.push_back((bits[i] + ringQ->logN + 60) / 61 - 1);   // ceil((bitlen + logN) / 61) - 1
  for (u64 q : ringQ->moduli) b->tmont.push_back(rh::mform(t, q));
  (void)hipSetDevice(ringQ->device);
  int rc = rh_bext_create(&b->be, ringQ, ringQMul);
  if (!rc && hipMalloc((void**)&b->d_tmont, b->tmont.size() * 8) != hipSuccess) rc = rh_fail(RH_ERR_NOMEM, "hipMalloc failed");
  if (!rc && hipMemcpy(b->d_tmont, b->tmont.data(), b->tmont.size() * 8, hipMemcpyHostToDevice) != hipSuccess) rc = rh_fail(RH_ERR_DEVICE, "hipMemcpy failed");
  if (rc) { rh_bfv_destroy(b); return rc; }
  *out = b;
  return RH_OK;
}
extern "C" void rh_bfv_destroy(rh_bfv* b) {
  if (!b) return;
  if (b->be) rh_bext_destroy(b->be);
  if (b->d_tmont) (void)hipFree(b->d_tmont);
  for (u64* p : b->buf) if (p) (void)hipFree(p);
  delete b;
}
extern "C" int rh_bfv_level_qmul(const rh_bfv* b, int level) {
  if (!b) return rh_fail(RH_ERR_ARG, "null bfv handle");
  if (level < 0 || level >= b->Q->L) return rh_fail(RH_ERR_ARG, "rh_bfv_level_qmul: level %d out of range [0,%d)", level, b->Q->L);
  return b->level_qmul[level];
}
extern "C" int rh_bfv_set_tuning(rh_bfv* b, const char* key, long value) {
  if (!b || !key) return rh_fail(RH_ERR_ARG, "rh_bfv_set_tuning: null argument");
  if (!strcmp(key, "fused_quantize")) { b->fused_quantize = value != 0; return RH_OK; }
  return rh_fail(RH_ERR_ARG, "rh_bfv_set_tuning: unknown key '%s'", key);
}

static bool quantize_is_fused(const rh_bfv* b, int level) {
  return b->fused_quantize && level + 1 <= 8 && b->level_qmul[level] + 1 <= 8;
}
extern "C" int rh_bfv_quantize_path(const rh_bfv* b, int level) {
  if (!b) return rh_fail(RH_ERR_ARG, "null bfv handle");
  if (level < 0 || level >= b->Q->L) return rh_fail(RH_ERR_ARG, "rh_bfv_quantize_path: level %d out of range [0,%d)", level, b->Q->L);
  return quantize_is_fused(b, level) ? 1 : 0;
}

static int ensure_scratch(rh_bfv* b, int which, size_t words) {
  if (b->buf_words[which] >= words) return 0;
  if (b->buf[which]) (void)hipFree(b->buf[which]);
  b->buf[which] = nullptr; b->buf_words[which] = 0;
  if (hipMalloc((void**)&b->buf[which], words * 8) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(bfv scratch) failed");
  b->buf_words[which] = words;
  return 0;
}
// Pre-sizes the scratch for multiplies of up to npoly ciphertexts at the top level: four blocks per ring
extern "C" int rh_bfv_reserve(rh_bfv* b, int npoly) {
  if (!b || npoly < 0) return rh_fail(RH_ERR_ARG, "rh_bfv_reserve: bad argument");
  std::lock_guard<std::recursive_mutex> lk(b->mu);
  (void)hipSetDevice(b->Q->device);
  const size_t N = b->Q->N;
  int lm = b->level_qmul[b->Q->L - 1] + 1;
  if (lm > b->M->L) lm = b->M->L;
  if (int rc = ensure_scratch(b, 0, 4 * (size_t)npoly * b->Q->L * N)) return rc;
  return ensure_scratch(b, 1, 4 * (size_t)npoly * lm * N);
}

// level checks shared by the entry points; *lq = levelQMul[level]
static int bfv_levels(rh_bfv* b, int level, int npoly, int* lq, const char* who) {
  if (!b) return rh_fail(RH_ERR_ARG, "%s: null bfv handle", who);
  if (level < 0 || level >= b->Q->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, b->Q->L);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  *lq = b->level_qmul[level];
  if (*lq >= b->M->L) return rh_fail(RH_ERR_ARG, "%s: level %d needs levelQMul = %d but ringQMul has %d moduli", who, level, *lq, b->M->L);
  if (level + 1 > 32 || *lq + 1 > 32) return rh_fail(RH_ERR_ARG, "%s: basis extension supports at most 32 source limbs (ring/basis_extension.go:285)", who);
  (void)hipSetDevice(b->Q->device);
  return 0;
}

static int tensor_launch(rh_bfv* b, int level, int lq, const BfvTensorSide& sq, const BfvTensorSide& sm, int npoly, bool square) {
  const unsigned rows = (unsigned)npoly * (unsigned)(level + 1 + lq + 1), n = (unsigned)b->Q->N;
  if (rows == 0) return RH_OK;
  const RhStreamGrid g = rh_stream_grid(b->Q, rows);                 // both rings have Q's N; the rows of both count towards the working set
  hipStream_t st = rh_stream(b->Q);
  (void)hipGetLastError();
  if (square) bfv_tensor_kernel<true><<<g.grid, 256, 0, st>>>(sq, sm, n, g.nt);
  else bfv_tensor_kernel<false><<<g.grid, 256, 0, st>>>(sq, sm, n, g.nt);
  return rh_launch_ok("bfv_tensor_kernel");
}

extern "C" int rh_bfv_tensor_lazy(rh_bfv* b, int level, const uint64_t* a0Q, const uint64_t* a1Q, const uint64_t* b0Q, const uint64_t* b1Q,
                                  const uint64_t* a0M, const uint64_t* a1M, const uint64_t* b0M, const uint64_t* b1M,
                                  uint64_t* c0Q, uint64_t* c1Q, uint64_t* c2Q, uint64_t* c0M, uint64_t* c1M, uint64_t* c2M, int npoly, int square) {
  int lq;
  if (int rc = bfv_levels(b, level, npoly, &lq, "rh_bfv_tensor_lazy")) return rc;
  if (!a0Q || !a1Q || !a0M || !a1M || !c0Q || !c1Q || !c2Q || !c0M || !c1M || !c2M) return rh_fail(RH_ERR_ARG, "rh_bfv_tensor_lazy: null argument");
  if (!square && (!b0Q || !b1Q || !b0M || !b1M)) return rh_fail(RH_ERR_ARG, "rh_bfv_tensor_lazy: null second operand without square");
  RhCallScope sc(rh_stream(b->Q));
  const BfvTensorSide sq{a0Q, a1Q, b0Q, b1Q, c0Q, c1Q, c2Q, b->Q->d_consts, level + 1};
  const BfvTensorSide sm{a0M, a1M, b0M, b1M, c0M, c1M, c2M, b->M->d_consts, lq + 1};
  return tensor_launch(b, level, lq, sq, sm, npoly, square != 0);
}

// the middle of quantize on coefficient-domain, canonical blocks: bq (npoly, level+1, N) is overwritten with the result, bm (npoly, lq+1, N) is consumed
static int quantize_core(rh_bfv* b, int level, int lq, u64* bq, u64* bm, int npoly) {
  if (npoly <= 0) return RH_OK;
  if (!quantize_is_fused(b, level)) {
    if (int rc = rh_bext_moddown_qp_to_p(b->be, level, lq, bq, bm, bm, npoly)) return rc;         // (:1115) in place: a thread reads its word of p1P before it writes it
    if (int rc = rh_bext_modup_p_to_q(b->be, lq, level, bm, bq, npoly)) return rc;                // (:1118)
    return rh_vec_launch(b->Q, RH_OP_MUL_SCALAR_MONT, bq, nullptr, bq, npoly, level + 1, 0, b->tmont.data(), nullptr);   // (:1121)
  }
  static const bfv_quant_fn* table = bfv_quant_table(std::make_integer_sequence<int, 64>());
  RhBextGuard guard(b->be);
  const BextPlan *p1, *p2;
  if (int rc = rh_bext_modup_plan(b->be, 1, 0, level, lq, &p1)) return rc;
  if (int rc = rh_bext_modup_plan(b->be, 0, 1, lq, level, &p2)) return rc;
  const int NQ = level + 1, NM = lq + 1, N = b->Q->N;
  const BfvQuantArgs a{p1->d_S, p1->d_T, p1->d_coef, p1->d_vt, p2->d_S, p2->d_T, p2->d_coef, p2->d_vt, b->d_tmont};
  const size_t lds = (size_t)(NM * (NQ + 1) + NQ * (NM + 1)) * 8;                                  // at most 2 * 72 words
  (void)hipGetLastError();
  hipLaunchKernelGGL(table[(NQ - 1) * 8 + (NM - 1)], dim3((N + 255) / 256, npoly), dim3(256), lds, rh_stream(b->Q), bq, bm, bq, a, N);
  return rh_launch_ok("bfv_quantize_kernel");
}

extern "C" int rh_bfv_quantize(rh_bfv* b, int level, const uint64_t* cQ, const uint64_t* cM, uint64_t* outQ, int npoly) {
  int lq;
  if (int rc = bfv_levels(b, level, npoly, &lq, "rh_bfv_quantize")) return rc;
  if (!cQ || !cM || !outQ) return rh_fail(RH_ERR_ARG, "rh_bfv_quantize: null argument");
  if (npoly == 0) return RH_OK;
  std::lock_guard<std::recursive_mutex> lk(b->mu);
  RhCallScope sc(rh_stream(b->Q));
  const size_t N = b->Q->N;
  if (int rc = ensure_scratch(b, 0, (size_t)npoly * (level + 1) * N)) return rc;
  if (int rc = ensure_scratch(b, 1, (size_t)npoly * (lq + 1) * N)) return rc;
  if (int rc = rh_ring_intt(b->Q, cQ, b->buf[0], npoly, level, 1)) return rc;                      // ringQ.INTTLazy (:1111)
  if (int rc = rh_ring_intt(b->M, cM, b->buf[1], npoly, lq, 1)) return rc;                         // ringQMul.INTTLazy (:1112)
  if (int rc = quantize_core(b, level, lq, b->buf[0], b->buf[1], npoly)) return rc;
  return rh_ring_ntt(b->Q, b->buf[0], outQ, npoly, level, 0);                                      // ringQ.NTT (:1123)
}

// tensorScaleInvariant :975-1014 (without the relin branch: the caller's GadgetProduct + two Adds).  Nothing is written to c0, c1, c2
// before every input has been read, so they may be any of the inputs.
extern "C" int rh_bfv_mul_scale_invariant(rh_bfv* b, int level, const uint64_t* a0, const uint64_t* a1, const uint64_t* b0, const uint64_t* b1,
                                          uint64_t* c0, uint64_t* c1, uint64_t* c2, int npoly) {
  int lq;
  if (int rc = bfv_levels(b, level, npoly, &lq, "rh_bfv_mul_scale_invariant")) return rc;
  if (!a0 || !a1 || !c0 || !c1 || !c2 || ((b0 == nullptr) != (b1 == nullptr))) return rh_fail(RH_ERR_ARG, "rh_bfv_mul_scale_invariant: null argument");
  if (npoly == 0) return RH_OK;
  const bool square = !b0 || (b0 == a0 && b1 == a1);               // ct0 == ct1 (:995, :1079): the same values with half the lifting
  const int nops = square ? 2 : 4;
  std::lock_guard<std::recursive_mutex> lk(b->mu);
  RhCallScope sc(rh_stream(b->Q));
  const size_t N = b->Q->N, wq = (size_t)npoly * (level + 1) * N, wm = (size_t)npoly * (lq + 1) * N;
  if (int rc = ensure_scratch(b, 0, 4 * wq)) return rc;
  if (int rc = ensure_scratch(b, 1, 4 * wm)) return rc;
  u64* bq = b->buf[0]; u64* bm = b->buf[1];
  // modUpAndNTT (:1053-1060) of every operand component as one batch: INTT -> ModUpQtoP -> NTT on QMul (the reference's NTTLazy there;
  // MForm / MRed take any representative, so the canonical transform gives the same tensor)
  const u64* ops[4] = {a0, a1, b0, b1};
  for (int i = 0; i < nops; ++i) if (int rc = rh_ring_intt(b->Q, ops[i], bq + i * wq, npoly, level, 0)) return rc;
  if (int rc = rh_bext_modup_q_to_p(b->be, level, lq, bq, bm, nops * npoly)) return rc;
  if (int rc = rh_ring_ntt(b->M, bm, bm, nops * npoly, lq, 0)) return rc;
  // tensorLowDeg (:1062-1102): the Q products go to the scratch (the operands' INTTs there are spent), the QMul products over their inputs
  const BfvTensorSide sq{a0, a1, b0, b1, bq, bq + wq, bq + 2 * wq, b->Q->d_consts, level + 1};
  const BfvTensorSide sm{bm, bm + wm, bm + 2 * wm, bm + 3 * wm, bm, bm + wm, bm + 2 * wm, b->M->d_consts, lq + 1};
  if (int rc = tensor_launch(b, level, lq, sq, sm, npoly, square)) return rc;
  // quantize (:1104-1124) of c0, c1, c2 as one batch of 3 * npoly polys; c1 enters INTTLazy in [0, 2q), as in the reference
  if (int rc = rh_ring_intt(b->Q, bq, bq, 3 * npoly, level, 1)) return rc;
  if (int rc = rh_ring_intt(b->M, bm, bm, 3 * npoly, lq, 1)) return rc;
  if (int rc = quantize_core(b, level, lq, bq, bm, 3 * npoly)) return rc;
  u64* outs[3] = {c0, c1, c2};
  for (int i = 0; i < 3; ++i) if (int rc = rh_ring_ntt(b->Q, bq + i * wq, outs[i], npoly, level, 0)) return rc;
  return RH_OK;
}

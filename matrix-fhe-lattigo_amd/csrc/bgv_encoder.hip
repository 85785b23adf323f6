// bgv_encoder.hip -- schemes/bgv/encoder.go on device batches of nvec vectors, standard rings.
//
//   Encode  = slots (permuteMatrix :98-121 on store, the value rules of :197-233) [-> ringT.INTT when batched] -> lift (MulScalar(scale) +
//             RingT2Q :357-386 + MForm) [-> Ring.NTT]
//   Decode  = [Ring.INTT ->] Q to T (RingQ2T :391-439 with the MulScalar by scale^-1 of :325 / :457 folded in) [-> ringT.NTT when batched]
//             -> slots (:330-347, :459-479)
//
// ringT is a ring handle the caller makes (one modulus T, degree n = min(N, order(T) / 2), bgv/params.go:110-121); its transform is the
// ring's own entry point.  Tuning "fused" = 0 issues the reference's own sequence of ring and basis-extension calls in place of
// bgv_lift_kernel and bgv_q2t_kernel, 1 the kernels, -1 whichever the measurement favours for each (the default; "fused_lift" and "fused_q2t"
// set one of the two) -- the same bits; the exact-CRT branch (level > 0, gap > 1), which the reference takes through math/big, has the one
// device form.
//
// The handle owns its scratch (one (nvec, n) block modulo T, one (nvec, L, N) poly block, the rotation table of rh_bgv_embed_qp); rh_bgv_encoder_reserve sizes it so that no later
// call allocates.  Calls are asynchronous on ringQ's stream -- ringT and the ring of rh_bgv_encode are pinned to it for the call -- and lock
// the handle for the enqueue only: the scratch is reused in stream order.
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "bext_internal.hpp"
#include "hostmath.hpp"
#include "bgv_encoder_kernels.hip.hpp"

// Defaults of the "fused" forms, decided by measurement (profiles/bgv_encoder.json; one kernel against the reference's
// sequence of calls in the same process, fused only where it wins by more than the spread of the composed windows):
#define BGV_ENC_FUSED_LIFT 1         // one pass over the block against three: about four times faster
#define BGV_ENC_FUSED_Q2T_LEVEL0 1   // one launch against five: about four times faster
#define BGV_ENC_FUSED_Q2T_MODUP 1    // 24 limbs, bgv_q2t_kernel<32, false>: about twice as fast as MulScalar + bext_kernel<32, false>

struct rh_bgv_encoder {
  rh_ring* Q = nullptr; rh_ring* T = nullptr;
  unsigned n = 0; int logn = 0, loggap = 0;
  u64 t = 0;
  BgvModT m{};
  unsigned* d_perm = nullptr;          // indexMatrix (:98-121) and its inverse, n entries each
  unsigned* d_inv = nullptr;
  u64* d_tables = nullptr;             // tmont | garner | qmodt | Qmodt | qmod | qhalf
  BgvQ2TTables tb{};
  std::vector<u64> tmont;              // MForm(T) modulo q_i (host copy for the call-by-call form)
  std::vector<u64> tinv_mont;          // MForm(T^-1 mod q_i): (T^-1 mod Q_level) mod q_i, whatever the level
  std::vector<BextPlan> plans;         // per level >= 1, gap = 1: GenModUpConstants(Q[:level + 1], {T}) (:61-65)
  std::vector<u64> half_t;             // ... and floor(Q_level / 2) mod T, the scalar of SubScalarBigint (:411)
  void* buf[3] = {nullptr, nullptr, nullptr}; size_t buf_bytes[3] = {0, 0, 0};   // (nvec, n) modulo T | (nvec, L, N) | one rotation per vector
  int fused_lift = BGV_ENC_FUSED_LIFT, fused_level0 = BGV_ENC_FUSED_Q2T_LEVEL0, fused_modup = BGV_ENC_FUSED_Q2T_MODUP;
  std::recursive_mutex mu;
};

extern "C" void rh_bgv_encoder_destroy(rh_bgv_encoder* e) {
  if (!e) return;
  if (e->d_perm) (void)hipFree(e->d_perm);
  if (e->d_inv) (void)hipFree(e->d_inv);
  if (e->d_tables) (void)hipFree(e->d_tables);
  for (BextPlan& p : e->plans) rh_bext_free_plan(p);
  for (void* p : e->buf) if (p) (void)hipFree(p);
  delete e;
}

extern "C" int rh_bgv_encoder_create(rh_bgv_encoder** out, rh_ring* ringQ, rh_ring* ringT) {
  if (!out || !ringQ || !ringT) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: null argument");
  if (ringQ->kind == RH_RING_CI || ringT->kind == RH_RING_CI)
    return rh_fail(RH_ERR_UNSUPPORTED, "rh_bgv_encoder_create: conjugate-invariant rings are not supported (their one-row encoder stays with the reference)");
  if (ringQ->kind != RH_RING_STANDARD || ringT->kind != RH_RING_STANDARD)
    return rh_fail(RH_ERR_UNSUPPORTED, "rh_bgv_encoder_create: 3N rings are not supported (the BGV encoder is defined on power-of-two cyclotomics)");
  if (ringT->L != 1) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: ringT must have one modulus, the plaintext modulus T (it has %d)", ringT->L);
  if (ringT->device != ringQ->device) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: ringQ and ringT live on different devices");
  if (ringQ->L > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: %d limbs, at most %d", ringQ->L, RH_MAX_LIMBS);
  const u64 t = ringT->moduli[0];
  if (ringT->N > ringQ->N || ringQ->N % ringT->N)
    return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: the degree of ringT (%d) must divide the degree of ringQ (%d)", ringT->N, ringQ->N);
  for (u64 q : ringQ->moduli)
    if (q == t) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: insecure parameters: t|Q (T = %llu is a modulus of Q)", (unsigned long long)t);
  for (u64 q : ringQ->moduli)
    if (rh::gcd(t, q) != 1) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: gcd(T, Q) != 1 (T = %llu, q = %llu): T has no inverse modulo Q", (unsigned long long)t, (unsigned long long)q);
  u64 order = 0;                                                          // the largest cyclotomic order enabled by T (bgv/params.go:110-113)
  { int len = 0; while (len < 64 && (t >> len)) ++len; for (order = len < 64 ? (u64)1 << len : 0; order != 0 && (t & (order - 1)) != 1; order >>= 1) {} }
  if (order < 16) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: provided plaintext modulus t has cyclotomic order < 16 (ring degree of minimum 8 is required by the backend)");
  if ((u64)ringT->N > (order >> 1)) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_create: the degree of ringT (%d) exceeds order(T) / 2 = %llu", ringT->N, (unsigned long long)(order >> 1));
  rh_bgv_encoder* e = new rh_bgv_encoder();
  e->Q = ringQ; e->T = ringT; e->t = t; e->n = (unsigned)ringT->N; e->logn = ringT->logN; e->loggap = ringQ->logN - ringT->logN;
  e->m = BgvModT{t, ringT->mred[0], ringT->bred[0], ringT->bred[1]};
  const int L = ringQ->L;
  const std::vector<u64>& q = ringQ->moduli;
  // permuteMatrix(logn): two rows of n / 2 slots; position of slot i of the first row is bitrev((5^i mod 2n) >> 1), the second row mirrors it
  const unsigned n = e->n;
  std::vector<unsigned> perm(n), inv(n);
  { u64 pow = 1; const u64 mask = 2 * (u64)n - 1;
    for (unsigned i = 0, j = n >> 1; i < (n >> 1); ++i, ++j) {
      const unsigned pos = (unsigned)rh::bitrev(pow >> 1, e->logn);
      perm[i] = pos; perm[j] = n - pos - 1;
      pow = (pow * 5) & mask;
    }
    for (unsigned i = 0; i < n; ++i) inv[perm[i]] = i; }
  // tmont | garner | qmodt | Qmodt | qmod | qhalf
  std::vector<u64> tab(4 * (size_t)L + 2 * (size_t)L * L, 0);
  u64* tmont = tab.data(); u64* garner = tmont + L; u64* qmodt = garner + L; u64* Qmodt = qmodt + L; u64* qmod = Qmodt + L; u64* qhalf = qmod + (size_t)L * L;
  e->tmont.resize(L); e->tinv_mont.resize(L);
  for (int j = 0; j < L; ++j) {
    tmont[j] = e->tmont[j] = rh::mform(t, q[j]);
    e->tinv_mont[j] = rh::mform(rh::invmod_prime(t % q[j], q[j]), q[j]);                // the moduli of Q are primes
    u64 prod = 1 % q[j];
    for (int i = 0; i < L; ++i) qmod[(size_t)j * L + i] = q[i] % q[j];
    for (int i = 0; i < j; ++i) prod = rh::mulmod(prod, q[i] % q[j], q[j]);
    garner[j] = rh::invmod_prime(prod, q[j]);
    qmodt[j] = q[j] % t;
    Qmodt[j] = rh::mulmod(j ? Qmodt[j - 1] : 1 % t, q[j] % t, t);
  }
  { std::vector<u64> acc((size_t)L, 0), h((size_t)L);                                   // Q_level as words, then the digits of Q_level >> 1
    acc[0] = 1;
    for (int lv = 0; lv < L; ++lv) {
      u64 carry = 0;
      for (int w = 0; w < L; ++w) { const rh::u128 p = (rh::u128)acc[w] * q[lv] + carry; acc[w] = (u64)p; carry = (u64)(p >> 64); }
      for (int w = 0; w < L; ++w) h[w] = (acc[w] >> 1) | (w + 1 < L ? acc[w + 1] << 63 : 0);
      for (int j = 0; j <= lv; ++j) {                                                   // digit j = h mod q_j, h /= q_j
        u64 rem = 0;
        for (int w = L - 1; w >= 0; --w) { const rh::u128 cur = ((rh::u128)rem << 64) | h[w]; h[w] = (u64)(cur / q[j]); rem = (u64)(cur % q[j]); }
        qhalf[(size_t)lv * L + j] = rem;
      }
    } }
  (void)hipSetDevice(ringQ->device);
  int rc = RH_OK;
  if (hipMalloc((void**)&e->d_perm, n * sizeof(unsigned)) != hipSuccess || hipMalloc((void**)&e->d_inv, n * sizeof(unsigned)) != hipSuccess ||
      hipMalloc((void**)&e->d_tables, tab.size() * 8) != hipSuccess)
    rc = rh_fail(RH_ERR_NOMEM, "rh_bgv_encoder_create: hipMalloc failed");
  if (!rc && (hipMemcpy(e->d_perm, perm.data(), n * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(e->d_inv, inv.data(), n * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(e->d_tables, tab.data(), tab.size() * 8, hipMemcpyHostToDevice) != hipSuccess))
    rc = rh_fail(RH_ERR_DEVICE, "rh_bgv_encoder_create: hipMemcpy failed");
  e->plans.resize(L); e->half_t.assign(L, 0);
  for (int lv = 1; !rc && lv < L && e->loggap == 0 && lv + 1 <= 32; ++lv) {              // the plan of ModUpQtoP onto {T}, centred (post 1)
    std::vector<u64> Qs(q.begin(), q.begin() + lv + 1), tg{t}, qsi, coef, vt;
    rh_gen_modup(Qs, tg, qsi, coef, vt);
    std::vector<BextSource> S(Qs.size());
    for (size_t i = 0; i < Qs.size(); ++i) S[i] = BextSource{Qs[i], ringQ->mred[i], qsi[i], rh_half_product_mod(Qs, Qs[i])};
    BextTarget tt{};
    tt.p = t; tt.pinv = ringT->mred[0]; tt.half = e->half_t[lv] = rh_half_product_mod(Qs, t); tt.buf = 0; tt.limb = 0; tt.post = 1; tt.skip = 0;
    rc = rh_bext_upload_plan(e->plans[lv], S, std::vector<BextTarget>{tt}, coef, vt);
  }
  if (rc) { rh_bgv_encoder_destroy(e); return rc; }
  e->tb.tmont = e->d_tables; e->tb.garner = e->tb.tmont + L; e->tb.qmodt = e->tb.garner + L; e->tb.Qmodt = e->tb.qmodt + L;
  e->tb.qmod = e->tb.Qmodt + L; e->tb.qhalf = e->tb.qmod + (size_t)L * L; e->tb.Lmax = L;
  *out = e;
  return RH_OK;
}

extern "C" int rh_bgv_encoder_set_tuning(rh_bgv_encoder* e, const char* key, long value) {
  if (!e || !key) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_set_tuning: null argument");
  const bool all = !strcmp(key, "fused"), lift = !strcmp(key, "fused_lift"), q2t = !strcmp(key, "fused_q2t");
  if (all || lift || q2t) {
    if (value < -1 || value > 1)
      return rh_fail(RH_ERR_ARG, "%s must be 0 (the reference's sequence of ring calls), 1 (one kernel each for the lift and Q to T) or -1 (the measured defaults)", key);
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    if (all || lift) e->fused_lift = value < 0 ? BGV_ENC_FUSED_LIFT : (int)value;
    if (all || q2t) {
      e->fused_level0 = value < 0 ? BGV_ENC_FUSED_Q2T_LEVEL0 : (int)value;
      e->fused_modup = value < 0 ? BGV_ENC_FUSED_Q2T_MODUP : (int)value;
    }
    return RH_OK;
  }
  return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_set_tuning: unknown key '%s'", key);
}

static int benc_scratch(rh_bgv_encoder* e, int which, size_t bytes) {
  if (e->buf_bytes[which] >= bytes) return RH_OK;
  if (e->buf[which]) (void)hipFree(e->buf[which]);                      // waits for the work that still reads it
  e->buf[which] = nullptr; e->buf_bytes[which] = 0;
  if (hipMalloc(&e->buf[which], bytes ? bytes : 8) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(bgv encoder scratch) failed");
  e->buf_bytes[which] = bytes;
  return RH_OK;
}

extern "C" int rh_bgv_encoder_reserve(rh_bgv_encoder* e, int nvec) {
  if (!e || nvec < 0) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder_reserve: bad argument");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  (void)hipSetDevice(e->Q->device);
  if (int rc = benc_scratch(e, 0, (size_t)nvec * e->n * 8)) return rc;
  if (int rc = benc_scratch(e, 2, (size_t)nvec * 8)) return rc;
  return benc_scratch(e, 1, (size_t)nvec * e->Q->L * e->Q->N * 8);
}

// the host half of every entry point: the handle locked, both rings on ringQ's stream, ringQ's device current, stale errors dropped
struct BencCall {
  std::lock_guard<std::recursive_mutex> lk; RhCallScope sc; hipStream_t st;
  explicit BencCall(rh_bgv_encoder* e) : lk(e->mu), sc(rh_stream(e->Q)), st(rh_stream(e->Q)) { (void)hipSetDevice(e->Q->device); (void)hipGetLastError(); }
};

static int benc_nvec(const rh_bgv_encoder* e, int nvec, const char* who) {
  if (!e) return rh_fail(RH_ERR_ARG, "%s: null encoder handle", who);
  if (nvec < 0 || nvec > 65535) return rh_fail(RH_ERR_ARG, "%s: nvec = %d out of range [0, 65535]", who, nvec);
  return RH_OK;
}
static int benc_level(const rh_ring* r, int level, const char* who) {
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, r->L);
  return RH_OK;
}
static dim3 benc_grid(unsigned words, int nvec) { return dim3((words + 255) / 256, (unsigned)nvec); }

static int benc_slots(rh_bgv_encoder* e, bool encode, const u64* src, u64* dst, unsigned nvals, int nvec, int batched, int is_signed, hipStream_t st) {
  if (encode) bgv_slots_kernel<true><<<benc_grid(e->n, nvec), 256, 0, st>>>(src, dst, batched ? e->d_inv : nullptr, e->n, nvals, e->m, is_signed);
  else if (nvals) bgv_slots_kernel<false><<<benc_grid(nvals, nvec), 256, 0, st>>>(src, dst, batched ? e->d_perm : nullptr, e->n, nvals, e->m, is_signed);
  return rh_launch_ok("bgv_slots_kernel");
}

static int benc_mul_scalar_t(rh_bgv_encoder* e, const u64* in, u64* out, int nvec, u64 s_mont) {
  return rh_vec_launch(e->T, RH_OP_MUL_SCALAR_MONT, in, nullptr, out, nvec, 1, 0, &s_mont, nullptr);
}

// MulScalar(scale) [has_scale] + RingT2Q + MForm [mont]; canonical: a transform or MForm follows.  ring: ringQ or another ring of degree N.
static int benc_lift(rh_bgv_encoder* e, rh_ring* ring, int level, const u64* pT, u64* out, int nvec, u64 scale, int has_scale, int scale_up,
                     int canonical, int mont, hipStream_t st) {
  const int L = level + 1;
  const unsigned N = (unsigned)ring->N, rows = (unsigned)nvec * (unsigned)L;
  const u64 s_mont = has_scale ? rh::mform(scale, e->t) : 0;
  if (e->fused_lift) {
    RhScalars k; memset(&k, 0, sizeof k);
    if (scale_up) memcpy(k.a, e->tinv_mont.data(), (size_t)L * 8);
    const RhStreamGrid g = rh_stream_grid(ring, rows);
    bgv_lift_kernel<<<g.grid, 256, 0, st>>>(pT, out, e->n, N, e->loggap, ring->d_consts, L, k, e->m, s_mont, has_scale, scale_up, canonical, mont, g.nt);
    return rh_launch_ok("bgv_lift_kernel");
  }
  const u64* src = pT;
  if (has_scale) {                                                       // ringT.MulScalar(pT, scale, pT) into the handle's block (:175, :243)
    if (int rc = benc_scratch(e, 0, (size_t)nvec * e->n * 8)) return rc;
    if (int rc = benc_mul_scalar_t(e, pT, (u64*)e->buf[0], nvec, s_mont)) return rc;
    src = (const u64*)e->buf[0];
  }
  bgv_spread_kernel<<<dim3(rows, (N + 255) / 256), 256, 0, st>>>(src, out, e->n, N, e->loggap, L);     // (:364-381)
  if (int rc = rh_launch_ok("bgv_spread_kernel")) return rc;
  if (scale_up)                                                          // MulScalarBigint(pQ, tInvModQ[level], pQ) (:384)
    if (int rc = rh_vec_launch(ring, RH_OP_MUL_SCALAR_MONT, out, nullptr, out, nvec, L, 0, e->tinv_mont.data(), nullptr)) return rc;
  if (canonical && !scale_up)                                            // raw words up to T - 1: the residue the reference's transform sees
    if (int rc = rh_vec_launch(ring, RH_OP_REDUCE, out, nullptr, out, nvec, L, 0, nullptr, nullptr)) return rc;
  return RH_OK;
}

// RingQ2T(level, scaleDown = true) of (nvec, level + 1, N) -> (nvec, n), then MulScalar by scale^-1 when has_sinv.  in may be the handle's block 1.
static int benc_q2t(rh_bgv_encoder* e, int level, const u64* in, u64* pT, int nvec, u64 sinv, int has_sinv, hipStream_t st) {
  const int L = level + 1;
  const unsigned N = (unsigned)e->Q->N;
  const int mode = level == 0 ? BGV_Q2T_LEVEL0 : e->loggap == 0 ? BGV_Q2T_MODUP : BGV_Q2T_EXACT;
  if (mode == BGV_Q2T_MODUP && L > 32) return rh_fail(RH_ERR_ARG, "basis extension supports at most 32 source limbs (ring/basis_extension.go:285)");
  const u64 sinv_mont = has_sinv ? rh::mform(sinv, e->t) : 0;
  if (mode == BGV_Q2T_EXACT || (mode == BGV_Q2T_MODUP ? e->fused_modup : e->fused_level0)) {
    const BextPlan& p = e->plans[level];
    BextTarget tgt{};
    tgt.p = e->t; tgt.pinv = e->m.tinv;
    tgt.half = e->half_t[level];
    const dim3 g = benc_grid(e->n, nvec);
#define BGV_Q2T(NQ, EX) bgv_q2t_kernel<NQ, EX><<<g, 256, 0, st>>>(in, pT, e->n, N, e->loggap, L, mode, e->Q->d_consts, e->tb, e->m, p.d_S, tgt, p.d_coef, p.d_vt, sinv_mont, has_sinv)
    switch (L) {
      case 1: BGV_Q2T(1, true); break; case 2: BGV_Q2T(2, true); break; case 3: BGV_Q2T(3, true); break; case 4: BGV_Q2T(4, true); break;
      case 5: BGV_Q2T(5, true); break; case 6: BGV_Q2T(6, true); break; case 7: BGV_Q2T(7, true); break; case 8: BGV_Q2T(8, true); break;
      default: if (L <= 16) BGV_Q2T(16, false); else if (L <= 32) BGV_Q2T(32, false); else BGV_Q2T(0, false); break;
    }
#undef BGV_Q2T
    return rh_launch_ok("bgv_q2t_kernel");
  }
  if (int rc = benc_scratch(e, 1, (size_t)nvec * L * N * 8)) return rc;
  u64* bufQ = (u64*)e->buf[1];
  if (int rc = rh_vec_launch(e->Q, RH_OP_MUL_SCALAR_MONT, in, nullptr, bufQ, nvec, L, 0, e->tmont.data(), nullptr)) return rc;       // (:398)
  if (mode == BGV_Q2T_MODUP) {                                           // AddScalarBigint + ModUpExact + SubScalarBigint (:409-411) = ModUpQtoP onto {T}
    if (int rc = rh_bext_launch_raw(st, (int)N, e->plans[level], bufQ, L, 0, pT, 1, nullptr, 0, nullptr, 0, nvec, BEXT_ADD_CRED)) return rc;
  } else {                                                               // level 0 (:417-437); the gather commutes with the element-wise AddScalar
    const u64 half = e->Q->moduli[0] >> 1, halft = half % e->t;
    if (int rc = rh_vec_launch(e->Q, RH_OP_ADD_SCALAR, bufQ, nullptr, bufQ, nvec, 1, 0, &half, nullptr)) return rc;
    bgv_gather_kernel<<<benc_grid(e->n, nvec), 256, 0, st>>>(bufQ, pT, e->n, N, e->loggap, 1);
    if (int rc = rh_launch_ok("bgv_gather_kernel")) return rc;
    if (int rc = rh_vec_launch(e->T, RH_OP_REDUCE, pT, nullptr, pT, nvec, 1, 0, nullptr, nullptr)) return rc;
    if (int rc = rh_vec_launch(e->T, RH_OP_SUB_SCALAR, pT, nullptr, pT, nvec, 1, 0, &halft, nullptr)) return rc;
  }
  if (has_sinv) return benc_mul_scalar_t(e, pT, pT, nvec, sinv_mont);
  return RH_OK;
}

static int benc_values(const rh_bgv_encoder* e, int nvals, int batched, bool encode) {
  if (nvals < 0) return rh_fail(RH_ERR_ARG, "rh_bgv_encoder: nvals < 0");
  if ((unsigned)nvals <= e->n) return RH_OK;
  if (!encode) return rh_fail(RH_ERR_ARG, "cannot Decode: len(values)=%d > slots=%u", nvals, e->n);
  return batched ? rh_fail(RH_ERR_ARG, "cannot EncodeRingT (FrequencyDomain): len(values)=%d > slots=%u", nvals, e->n)
                 : rh_fail(RH_ERR_ARG, "cannot Encode (TimeDomain): len(values)=%d > N=%u", nvals, e->n);
}

static int benc_sinv(const rh_bgv_encoder* e, u64 scale, u64* sinv, const char* who) {
  if (scale % e->t == 0 || rh::gcd(scale % e->t, e->t) != 1)
    return rh_fail(RH_ERR_ARG, "%s: the scale %llu is zero or not invertible modulo T = %llu", who, (unsigned long long)scale, (unsigned long long)e->t);
  *sinv = rh::powmod(scale, e->t - 2, e->t);                             // ring.ModExp(scale, T - 2, T) (:325, :457)
  return RH_OK;
}

extern "C" int rh_bgv_encode_ring_t(rh_bgv_encoder* e, uint64_t scale, const uint64_t* values_dev, int nvals, int is_signed, int nvec, uint64_t* pT_dev) {
  if (int rc = benc_nvec(e, nvec, "rh_bgv_encode_ring_t")) return rc;
  if (!values_dev || !pT_dev) return rh_fail(RH_ERR_ARG, "rh_bgv_encode_ring_t: null argument");
  if (int rc = benc_values(e, nvals, 1, true)) return rc;
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  if (int rc = benc_slots(e, true, values_dev, pT_dev, (unsigned)nvals, nvec, 1, is_signed, call.st)) return rc;
  if (int rc = rh_ring_ntt_any(e->T, pT_dev, pT_dev, nvec, 1, 0, true)) return rc;                     // INTT on Y = X^(N/n) (:242)
  return benc_mul_scalar_t(e, pT_dev, pT_dev, nvec, rh::mform(scale, e->t));                           // (:243)
}

extern "C" int rh_bgv_decode_ring_t(rh_bgv_encoder* e, uint64_t scale, const uint64_t* pT_dev, int nvec, uint64_t* values_dev, int nvals, int is_signed) {
  if (int rc = benc_nvec(e, nvec, "rh_bgv_decode_ring_t")) return rc;
  if (!values_dev || !pT_dev) return rh_fail(RH_ERR_ARG, "rh_bgv_decode_ring_t: null argument");
  if (int rc = benc_values(e, nvals, 1, false)) return rc;
  u64 sinv; if (int rc = benc_sinv(e, scale, &sinv, "rh_bgv_decode_ring_t")) return rc;
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  if (int rc = benc_scratch(e, 0, (size_t)nvec * e->n * 8)) return rc;
  u64* bufT = (u64*)e->buf[0];
  if (int rc = benc_mul_scalar_t(e, pT_dev, bufT, nvec, rh::mform(sinv, e->t))) return rc;             // (:325)
  if (int rc = rh_ring_ntt_any(e->T, bufT, bufT, nvec, 1, 0, false)) return rc;                        // (:326)
  return benc_slots(e, false, bufT, values_dev, (unsigned)nvals, nvec, 1, is_signed, call.st);
}

static int benc_ring(const rh_bgv_encoder* e, const rh_ring* ring, int scale_up, const char* who) {
  if (!ring) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (ring->kind != RH_RING_STANDARD || ring->N != e->Q->N || ring->device != e->Q->device)
    return rh_fail(RH_ERR_ARG, "%s: the ring must be ringQ or another standard ring of degree %d on the same device", who, e->Q->N);
  if (scale_up && ring != e->Q)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: scale_up into a ring other than ringQ is refused: the reference multiplies the limbs of P by T^-1 mod Q_levelP "
                                       "under the moduli of Q (bgv/encoder.go:282, :384)", who);
  return RH_OK;
}

extern "C" int rh_bgv_ring_t2q(rh_bgv_encoder* e, rh_ring* ring, int level, int scale_up, const uint64_t* pT_dev, uint64_t* out_dev, int nvec) {
  if (int rc = benc_nvec(e, nvec, "rh_bgv_ring_t2q")) return rc;
  if (int rc = benc_ring(e, ring, scale_up, "rh_bgv_ring_t2q")) return rc;
  if (int rc = benc_level(ring, level, "rh_bgv_ring_t2q")) return rc;
  if (!pT_dev || !out_dev) return rh_fail(RH_ERR_ARG, "rh_bgv_ring_t2q: null argument");
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  return benc_lift(e, ring, level, pT_dev, out_dev, nvec, 0, 0, scale_up ? 1 : 0, 0, 0, call.st);
}

extern "C" int rh_bgv_ring_q2t(rh_bgv_encoder* e, int level, const uint64_t* in_dev, uint64_t* pT_dev, int nvec) {
  if (int rc = benc_nvec(e, nvec, "rh_bgv_ring_q2t")) return rc;
  if (int rc = benc_level(e->Q, level, "rh_bgv_ring_q2t")) return rc;
  if (!pT_dev || !in_dev) return rh_fail(RH_ERR_ARG, "rh_bgv_ring_q2t: null argument");
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  return benc_q2t(e, level, in_dev, pT_dev, nvec, 0, 0, call.st);
}

extern "C" int rh_bgv_encode(rh_bgv_encoder* e, rh_ring* ring, int level, uint64_t scale, const uint64_t* values_dev, int nvals, int is_signed, int nvec,
                             uint64_t* out_dev, int batched, int scale_up, int is_ntt, int is_montgomery) {
  if (int rc = benc_nvec(e, nvec, "rh_bgv_encode")) return rc;
  if (int rc = benc_ring(e, ring, scale_up, "rh_bgv_encode")) return rc;
  if (int rc = benc_level(ring, level, "rh_bgv_encode")) return rc;
  if (!values_dev || !out_dev) return rh_fail(RH_ERR_ARG, "rh_bgv_encode: null argument");
  if (int rc = benc_values(e, nvals, batched, true)) return rc;
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  if (int rc = benc_scratch(e, 0, (size_t)nvec * e->n * 8)) return rc;
  u64* bufT = (u64*)e->buf[0];
  if (int rc = benc_slots(e, true, values_dev, bufT, (unsigned)nvals, nvec, batched, is_signed, call.st)) return rc;
  if (batched) if (int rc = rh_ring_ntt_any(e->T, bufT, bufT, nvec, 1, 0, true)) return rc;
  const int canonical = (is_ntt || is_montgomery) ? 1 : 0;
  if (int rc = benc_lift(e, ring, level, bufT, out_dev, nvec, scale, 1, scale_up ? 1 : 0, canonical, e->fused_lift && is_montgomery ? 1 : 0, call.st)) return rc;
  if (is_ntt) if (int rc = rh_ring_ntt_any(ring, out_dev, out_dev, nvec, level + 1, 0, false)) return rc;
  if (!e->fused_lift && is_montgomery) return rh_vec_launch(ring, RH_OP_MFORM, out_dev, nullptr, out_dev, nvec, level + 1, 0, nullptr, nullptr);   // (:274-276)
  return RH_OK;
}

extern "C" int rh_bgv_decode(rh_bgv_encoder* e, int level, uint64_t scale, const uint64_t* in_dev, int nvec, uint64_t* values_dev, int nvals, int is_signed,
                             int batched, int is_ntt) {
  if (int rc = benc_nvec(e, nvec, "rh_bgv_decode")) return rc;
  if (int rc = benc_level(e->Q, level, "rh_bgv_decode")) return rc;
  if (!values_dev || !in_dev) return rh_fail(RH_ERR_ARG, "rh_bgv_decode: null argument");
  if (int rc = benc_values(e, nvals, batched, false)) return rc;
  u64 sinv; if (int rc = benc_sinv(e, scale, &sinv, "rh_bgv_decode")) return rc;
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  const int L = level + 1;
  if (int rc = benc_scratch(e, 0, (size_t)nvec * e->n * 8)) return rc;
  const u64* src = in_dev;
  if (is_ntt) {                                                          // INTT into the encoder's buffer (:446-448)
    if (int rc = benc_scratch(e, 1, (size_t)nvec * L * e->Q->N * 8)) return rc;
    if (int rc = rh_ring_ntt_any(e->Q, in_dev, (u64*)e->buf[1], nvec, L, 0, true)) return rc;
    src = (const u64*)e->buf[1];
  }
  u64* bufT = (u64*)e->buf[0];
  if (int rc = benc_q2t(e, level, src, bufT, nvec, sinv, 1, call.st)) return rc;
  if (batched) if (int rc = rh_ring_ntt_any(e->T, bufT, bufT, nvec, 1, 0, false)) return rc;
  return benc_slots(e, false, bufT, values_dev, (unsigned)nvals, nvec, batched, is_signed, call.st);
}

// A whole linear transformation: rotateAndEncodeDiagonal (circuits/common/lintrans/lintrans.go:271-292) for nvec diagonals at once, Embed into
// the (Q, P) pair; see ringhip.h.  One gather (row rotation + slot permutation), ONE inverse transform over T, one lift onto the rows of
// both rings, the forward transforms.  "fused" = 0: the rotation as a pass of its own, then the composition rh_bgv_encode issues, per ring.
extern "C" int rh_bgv_embed_qp(rh_bgv_encoder* e, rh_ring* ringP, int levelQ, int levelP, uint64_t scale, const uint64_t* values_dev, int nvals,
                               int is_signed, int nvec, const int* rot, int cols, uint64_t* outQ_dev, uint64_t* outP_dev, int is_ntt,
                               int is_montgomery) {
  const char* who = "rh_bgv_embed_qp";
  if (int rc = benc_nvec(e, nvec, who)) return rc;
  if (int rc = benc_ring(e, ringP, 0, who)) return rc;
  if (int rc = benc_level(e->Q, levelQ, who)) return rc;
  if (int rc = benc_level(ringP, levelP, who)) return rc;
  if (!values_dev || !outQ_dev || !outP_dev) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (int rc = benc_values(e, nvals, 1, true)) return rc;
  if (rot) {
    if (cols <= 0 || (cols & (cols - 1))) return rh_fail(RH_ERR_ARG, "%s: cols = %d is not a power of two", who, cols);
    if ((unsigned)nvals != e->n || 2 * (long long)cols != (long long)nvals)
      return rh_fail(RH_ERR_ARG, "%s: a rotation needs the encoder's own dimensions, nvals = n = 2 * cols (nvals = %d, n = %u, cols = %d); rows of another "
                                 "length are rotated by the caller", who, nvals, e->n, cols);
  }
  const int LQ = levelQ + 1, LP = levelP + 1;
  const size_t N = (size_t)e->Q->N;
  { const RhBlock w[2] = {{outQ_dev, (size_t)nvec * LQ * N}, {outP_dev, (size_t)nvec * LP * N}}, r[1] = {{values_dev, (size_t)nvec * (size_t)nvals}};
    if (int rc = rh_blocks_ok(w, 2, r, nvals ? 1 : 0, who, "an output overlaps the values")) return rc;
    if (int rc = rh_blocks_disjoint(w, 2, who, "outQ and outP overlap")) return rc; }
  if (nvec == 0) return RH_OK;
  BencCall call(e);
  if (int rc = benc_scratch(e, 0, (size_t)nvec * e->n * 8)) return rc;
  u64* bufT = (u64*)e->buf[0];
  const u64* d_rot = nullptr;
  if (rot) {                                                             // rot & (cols - 1) per vector (:276), one word each, through the thread's staging slots
    if (int rc = benc_scratch(e, 2, (size_t)nvec * 8)) return rc;
    RhStage* stage;
    if (int rc = rh_stage_slot((size_t)nvec, &stage, who)) return rc;
    for (int k = 0; k < nvec; ++k) stage->h[k] = (u64)((unsigned)rot[k] & (unsigned)(cols - 1));
    if (int rc = rh_stage_upload(stage, (u64*)e->buf[2], (size_t)nvec, call.st, who)) return rc;
    d_rot = (const u64*)e->buf[2];
  }
  const int canonical = (is_ntt || is_montgomery) ? 1 : 0;
  const u64 s_mont = rh::mform(scale, e->t);
  if (e->fused_lift) {
    bgv_embed_gather_kernel<<<benc_grid(e->n, nvec), 256, 0, call.st>>>(values_dev, bufT, e->d_inv, d_rot, e->n, (unsigned)nvals, (unsigned)cols, e->m, is_signed);
    if (int rc = rh_launch_ok("bgv_embed_gather_kernel")) return rc;
    if (int rc = rh_ring_ntt_any(e->T, bufT, bufT, nvec, 1, 0, true)) return rc;
    const RhStreamGrid g = rh_stream_grid(e->Q, (unsigned)nvec * (unsigned)(LQ + LP));
    bgv_lift_qp_kernel<<<g.grid, 256, 0, call.st>>>(bufT, outQ_dev, outP_dev, e->n, e->Q->logN, e->loggap, e->Q->d_consts, ringP->d_consts, LQ, LP, e->m,
                                                     s_mont, canonical, is_montgomery ? 1 : 0, g.nt);
    if (int rc = rh_launch_ok("bgv_lift_qp_kernel")) return rc;
    if (is_ntt) {
      if (int rc = rh_ring_ntt_any(e->Q, outQ_dev, outQ_dev, nvec, LQ, 0, false)) return rc;
      if (int rc = rh_ring_ntt_any(ringP, outP_dev, outP_dev, nvec, LP, 0, false)) return rc;
    }
    return RH_OK;
  }
  const u64* src = values_dev;
  if (d_rot) {                                                           // the rotated rows in the handle's poly block (nvec * n <= nvec * L * N words)
    if (int rc = benc_scratch(e, 1, (size_t)nvec * e->Q->L * N * 8)) return rc;
    bgv_rotate_rows_kernel<<<benc_grid(e->n, nvec), 256, 0, call.st>>>(values_dev, (u64*)e->buf[1], d_rot, (unsigned)cols);
    if (int rc = rh_launch_ok("bgv_rotate_rows_kernel")) return rc;
    src = (const u64*)e->buf[1];
  }
  if (int rc = benc_slots(e, true, src, bufT, (unsigned)nvals, nvec, 1, is_signed, call.st)) return rc;
  if (int rc = rh_ring_ntt_any(e->T, bufT, bufT, nvec, 1, 0, true)) return rc;
  if (int rc = benc_mul_scalar_t(e, bufT, bufT, nvec, s_mont)) return rc;              // once: both rings lift the same scaled block
  rh_ring* rings[2] = {e->Q, ringP}; u64* outs[2] = {outQ_dev, outP_dev}; const int lv[2] = {levelQ, levelP};
  for (int k = 0; k < 2; ++k) {
    if (int rc = benc_lift(e, rings[k], lv[k], bufT, outs[k], nvec, 0, 0, 0, canonical, 0, call.st)) return rc;
    if (is_ntt) if (int rc = rh_ring_ntt_any(rings[k], outs[k], outs[k], nvec, lv[k] + 1, 0, false)) return rc;
    if (is_montgomery) if (int rc = rh_vec_launch(rings[k], RH_OP_MFORM, outs[k], nullptr, outs[k], nvec, lv[k] + 1, 0, nullptr, nullptr)) return rc;
  }
  return RH_OK;
}

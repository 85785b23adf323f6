// engine.hip -- C-ABI implementation (include/ringhip.h): ring construction, twiddle-table layout, kernel launches.
//
// Host logic here replaces, for device-resident data, the per-limb dispatch loops of the reference
// (Ring.NTT ring/ntt.go:127-152, SubRing ops ring/subring_ops.go, Ring ops ring/operations.go) with one batched
// launch over (poly, limb) -- limbs and polys are independent, so the batch IS the parallelism.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <vector>
#include <new>
#include "../../include/ringhip.h"
#include "hostmath.hpp"
#include "ntt_kernels.hip.hpp"
#include "vec_kernels.hip.hpp"
#include "stream_kernels.hip.hpp"
#include "ntt_kernels_asm.hip.hpp"
#include "ntt3n_kernels_asm.hip.hpp"
#include "engine_internal.hpp"

// ------------------------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";
int rh_fail(int code, const char* fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}
extern "C" const char* rh_last_error(void) { return g_err; }

// ------------------------------------------------------------------------------------------------ per-call context
static thread_local hipStream_t tl_stream = nullptr;
static thread_local bool tl_has_stream = false;
static thread_local u64* tl_ws = nullptr;
static thread_local size_t tl_ws_words = 0;
static thread_local int tl_layout3n = -1;          // -1: the handle's tuning value; 0 / 1: the layout the running entry point was told
int rh_layout3n(const rh_ring* r) { return tl_layout3n >= 0 ? tl_layout3n : r->block_order3n; }
RhLayoutScope::RhLayoutScope(int layout) : prev(tl_layout3n) { tl_layout3n = layout; }
RhLayoutScope::~RhLayoutScope() { tl_layout3n = prev; }
hipStream_t rh_stream(const rh_ring* r) { return tl_has_stream ? tl_stream : r->stream; }
u64* rh_ws_override(size_t words) { return (tl_ws && tl_ws_words >= words) ? tl_ws : nullptr; }
RhCallScope::RhCallScope(hipStream_t st, u64* ws, size_t ws_words) : prev_st(tl_stream), prev_has(tl_has_stream), prev_ws(tl_ws), prev_words(tl_ws_words) {
  tl_stream = st; tl_has_stream = true;
  if (ws) { tl_ws = ws; tl_ws_words = ws_words; }
}
RhCallScope::~RhCallScope() { tl_stream = prev_st; tl_has_stream = prev_has; tl_ws = prev_ws; tl_ws_words = prev_words; }
extern "C" int rh_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

// ------------------------------------------------------------------------------------------------ table layout
// natural order -> the order ntt_fwd_tile / ntt_inv_tile read (ntt_kernels.hip.hpp): per 4096-tile T
//   [slot]                 round A, slot = (2^u - 1) + g          <- nat[2^(S1+u)   + T*2^u     + g]
//   [16 + slot*16 + hi4]   round B                                <- nat[2^(S1+4+u) + T*2^(4+u) + (hi4<<u) + g]
//   [256 + slot*256 + tid] round C                                <- nat[2^(S1+8+u) + T*2^(8+u) + (tid<<u) + g]
template <class T>
static void build_kernel_order(const T* nat, T* out, int logN) {
  const int S1 = logN - LT;
  const size_t ntiles = (size_t)1 << S1;
  for (size_t t = 0; t < ntiles; ++t) {
    T* o = out + (t << LT);
    memset(o, 0, sizeof(T) * TILE);
    for (int u = 0; u < 4; ++u)
      for (int g = 0; g < (1 << u); ++g) {
        const int slot = (1 << u) - 1 + g;
        o[slot] = nat[((size_t)1 << (S1 + u)) + (t << u) + g];
        for (int h = 0; h < 16; ++h) o[16 + slot * 16 + h] = nat[((size_t)1 << (S1 + 4 + u)) + (t << (4 + u)) + ((size_t)h << u) + g];
        for (int i = 0; i < 256; ++i) o[256 + slot * 256 + i] = nat[((size_t)1 << (S1 + 8 + u)) + (t << (8 + u)) + ((size_t)i << u) + g];
      }
  }
}

template <class T>
static int upload(T** dptr, const std::vector<T>& h) {
  if (hipMalloc((void**)dptr, h.size() * sizeof(T)) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(%zu) failed", h.size() * sizeof(T));
  if (hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "hipMemcpy H2D failed");
  return 0;
}

// uploads natural-order Shoup tables (+ optional Montgomery forward table) and, for N >= 4096, their kernel-order copies
int rh_std_upload_tables(rh_ring* r, const std::vector<tw2>& fs, const std::vector<tw2>& is, const std::vector<u64>* mont,
                         const std::vector<tw2>& lastw) {
  const int L = r->L, N = r->N, logN = r->logN;
  int rc = 0;
  if (!rc) rc = upload(&r->d_tw_fwd, fs);
  if (!rc) rc = upload(&r->d_tw_inv, is);
  if (!rc && mont) rc = upload(&r->d_tw_fwd_mont, *mont);
  if (!rc) rc = upload(&r->d_lastw, lastw);
  if (!rc && logN >= LT) {
    std::vector<tw2> kf((size_t)L * N), ki((size_t)L * N);
    for (int i = 0; i < L; ++i) {
      build_kernel_order(fs.data() + (size_t)i * N, kf.data() + (size_t)i * N, logN);
      build_kernel_order(is.data() + (size_t)i * N, ki.data() + (size_t)i * N, logN);
    }
    if (!rc) rc = upload(&r->d_twk_fwd, kf);
    if (!rc) rc = upload(&r->d_twk_inv, ki);
    if (!rc && mont) {
      std::vector<u64> km((size_t)L * N);
      for (int i = 0; i < L; ++i) build_kernel_order(mont->data() + (size_t)i * N, km.data() + (size_t)i * N, logN);
      rc = upload(&r->d_twk_fwd_mont, km);
    }
  }
  return rc;
}
int rh_upload_consts(rh_ring* r, const std::vector<LimbConsts>& hc) { return upload(&r->d_consts, hc); }

// ------------------------------------------------------------------------------------------------ ring construction
static int validate_degree(int kind, int N) {
  if (kind == RH_RING_STANDARD || kind == RH_RING_CI) {
    // MinimumRingDegreeForLoopUnrolledOperations = 8 (ring/ring.go:21-23, :318)
    if (N < 8 || (N & (N - 1)) != 0 || N > (1 << 17)) return rh_fail(RH_ERR_ARG, "invalid ring degree: must be a power of 2 greater than 8 (and at most 2^17), got N=%d", N);
    return 0;
  }
  if (kind == RH_RING_3N) {
    int m = N; int a = 0, b = 0;
    while (m % 2 == 0) { m /= 2; ++a; }
    while (m % 3 == 0) { m /= 3; ++b; }
    if (m != 1 || a < 1 || b < 1) return rh_fail(RH_ERR_ARG, "invalid 3N ring degree: N=%d must be 2^a*3^b with a,b>=1", N);
    return 0;
  }
  return rh_fail(RH_ERR_ARG, "unknown ring kind %d", kind);
}

static bool one_pass_ok(rh_ring* r);
extern "C" int rh_ring_create(rh_ring** out, int device, int kind, int N, int L, const uint64_t* moduli, const uint64_t* mred,
                              const uint64_t* bred, const uint64_t* ninv, const uint64_t* roots_fwd, const uint64_t* roots_bwd,
                              const uint64_t* omega3n) {
  if (!out || !moduli || !mred || !bred || L < 1 || L > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "rh_ring_create: bad arguments (L=%d)", L);
  if (int e = validate_degree(kind, N)) return e;
  for (int i = 0; i < L; ++i) {
    if (moduli[i] >= ((u64)1 << 61) || (moduli[i] & 1) == 0) return rh_fail(RH_ERR_MODULUS, "modulus %d (%llu) must be odd and < 2^61", i, (unsigned long long)moduli[i]);
    for (int j = 0; j < i; ++j) if (moduli[i] == moduli[j]) return rh_fail(RH_ERR_MODULUS, "invalid moduli: duplicate modulus %llu", (unsigned long long)moduli[i]);
  }
  if (hipSetDevice(device) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "hipSetDevice(%d) failed", device);
  rh_ring* r = new (std::nothrow) rh_ring();
  if (!r) return rh_fail(RH_ERR_NOMEM, "out of host memory");
  r->device = device; r->kind = kind; r->N = N; r->L = L;
  r->moduli.assign(moduli, moduli + L); r->mred.assign(mred, mred + L); r->bred.assign(bred, bred + 2 * L);
  int rc = 0;
  std::vector<LimbConsts> hc(L);
  for (int i = 0; i < L; ++i) {
    LimbConsts& c = hc[i];
    c.q = moduli[i]; c.qinv = mred[i]; c.bred0 = bred[2 * i]; c.bred1 = bred[2 * i + 1]; c.nq = (u64)0 - moduli[i];
    c.ninv_mont = 0; c.ninv_w = 0; c.ninv_wp = 0;
  }
  if (kind == RH_RING_STANDARD || kind == RH_RING_CI) {
    if (!ninv || !roots_fwd || !roots_bwd) { delete r; return rh_fail(RH_ERR_ARG, "rh_ring_create: ring needs ninv and root tables"); }
    int logN = 0; while ((1 << logN) < N) ++logN;
    r->logN = logN;
    // table length handed over: NthRoot/2 = N (standard, 2N-th root) or 2N (conjugate invariant, 4N-th root)
    const size_t TN = kind == RH_RING_CI ? (size_t)2 * N : (size_t)N;
    r->ninv.assign(ninv, ninv + L);
    r->roots_fwd.assign(roots_fwd, roots_fwd + (size_t)L * TN);
    r->roots_bwd.assign(roots_bwd, roots_bwd + (size_t)L * TN);
    std::vector<tw2> fs((size_t)L * N), is((size_t)L * N), lastw(L);
    std::vector<u64> mont((size_t)L * N);
    std::vector<CiFold> fold(L);
    for (int i = 0; i < L; ++i) {
      const u64 q = moduli[i];
      LimbConsts& c = hc[i];
      c.ninv_mont = ninv[i];
      c.ninv_w = rh::imform(ninv[i], q); c.ninv_wp = rh::shoup_quotient(c.ninv_w, q);
      // one modular inverse of 2^64 per limb, then a multiply per root
      const u64 rinv = rh::imform(1, q);
      const u64* rf = roots_fwd + (size_t)i * TN; const u64* rb = roots_bwd + (size_t)i * TN;
      for (int j = 0; j < N; ++j) {
        // standard: stage with m blocks uses roots[m+i] (ring/ntt.go:240-255).  Conjugate invariant: the same stage
        // uses roots[2m+i] of the 4N-th-root table (:768-781, :1119-1147), i.e. entry j = m+i reads 2m+i = j + 2^floor(log2 j)
        size_t src = (size_t)j;
        if (kind == RH_RING_CI && j > 0) { int hb = 31 - __builtin_clz((unsigned)j); src = (size_t)j + ((size_t)1 << hb); }
        u64 wf = rh::mulmod(rf[src] % q, rinv, q), wb = rh::mulmod(rb[src] % q, rinv, q);
        fs[(size_t)i * N + j] = tw2{wf, rh::shoup_quotient(wf, q)};
        is[(size_t)i * N + j] = tw2{wb, rh::shoup_quotient(wb, q)};
        mont[(size_t)i * N + j] = rf[src];
      }
      u64 lw = rh::mulmod(is[(size_t)i * N + 1].w, c.ninv_w, q);
      lastw[i] = tw2{lw, rh::shoup_quotient(lw, q)};
      if (kind == RH_RING_CI) {
        const u64 ff = rh::mulmod(rf[1] % q, rinv, q), fb = rh::mulmod(rb[1] % q, rinv, q);
        fold[i] = CiFold{tw2{ff, rh::shoup_quotient(ff, q)}, tw2{fb, rh::shoup_quotient(fb, q)}};
      }
    }
    if (!rc) rc = rh_std_upload_tables(r, fs, is, &mont, lastw);
    if (!rc && kind == RH_RING_STANDARD) {          // N^-1 * 2^64 = NInv as handed over (Montgomery form): constants of rh_ring_intt_mul
      std::vector<LimbConsts> hr(hc); std::vector<tw2> lr(L);
      for (int i = 0; i < L; ++i) {
        const u64 q = moduli[i], nr = ninv[i] % q;
        hr[i].ninv_w = nr; hr[i].ninv_wp = rh::shoup_quotient(nr, q);
        const u64 lw = rh::mulmod(is[(size_t)i * N + 1].w, nr, q);
        lr[i] = tw2{lw, rh::shoup_quotient(lw, q)};
      }
      rc = upload(&r->d_consts_r, hr);
      if (!rc) rc = upload(&r->d_lastw_r, lr);
    }
    if (!rc && N < 16) {
      std::vector<u64> bm((size_t)L * N);
      for (int i = 0; i < L; ++i) for (int j = 0; j < N; ++j) {
        size_t src = (size_t)j;
        if (kind == RH_RING_CI && j > 0) { int hb = 31 - __builtin_clz((unsigned)j); src = (size_t)j + ((size_t)1 << hb); }
        bm[(size_t)i * N + j] = roots_bwd[(size_t)i * TN + src];
      }
      rc = upload(&r->d_tw_inv_mont, bm);
    }
    if (!rc && kind == RH_RING_CI) rc = upload(&r->d_cifold, fold);
  } else {
    if (!omega3n) { delete r; return rh_fail(RH_ERR_ARG, "rh_ring_create: 3N ring needs omega3n"); }
    r->omega3n.assign(omega3n, omega3n + L);
    rc = rh_ring3n_setup(r, hc);
  }
  if (!rc) rc = upload(&r->d_consts, hc);
  if (rc) { rh_ring_destroy(r); return rc; }
  r->hconsts = hc;
  (void)one_pass_ok(r);          // N = 2^13 / 2^14: raise the one-pass kernels' dynamic-LDS limit now, while one thread owns the handle
  *out = r;
  return RH_OK;
}

extern "C" int rh_ring_create_auto(rh_ring** out, int device, int kind, int N, int L, const uint64_t* moduli, const uint64_t* omega3n) {
  if (!out || !moduli || L < 1 || L > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "rh_ring_create_auto: bad arguments");
  if (int e = validate_degree(kind, N)) return e;
  std::vector<u64> mred(L), bred(2 * L), ninv(L), rf, rb, om;
  const bool pow2 = kind == RH_RING_STANDARD || kind == RH_RING_CI;
  const u64 nthroot = kind == RH_RING_STANDARD ? (u64)2 * N : (kind == RH_RING_CI ? (u64)4 * N : (u64)3 * N);
  const size_t TN = (size_t)(nthroot >> 1);
  if (pow2) { rf.resize((size_t)L * TN); rb.resize((size_t)L * TN); }
  else om.resize(L);
  for (int i = 0; i < L; ++i) {
    const u64 q = moduli[i];
    if (!rh::is_prime(q)) return rh_fail(RH_ERR_MODULUS, "invalid modulus: %llu is not prime)", (unsigned long long)q);
    if (q % nthroot != 1) return rh_fail(RH_ERR_MODULUS, "invalid modulus: %llu != 1 mod NthRoot)", (unsigned long long)q);
    mred[i] = rh::gen_mred_constant(q);
    rh::gen_bred_constant(q, &bred[2 * i]);
    if (pow2) {
      if (rh::gen_ntt_tables(q, nthroot, &rf[(size_t)i * TN], &rb[(size_t)i * TN], &ninv[i])) return rh_fail(RH_ERR_MODULUS, "table generation failed for modulus %llu", (unsigned long long)q);
    } else {
      ninv[i] = rh::mform(rh::invmod_prime((u64)N % q, q), q);
      om[i] = omega3n ? omega3n[i] : rh::powmod(rh::primitive_root(q), (q - 1) / nthroot, q);
    }
  }
  return rh_ring_create(out, device, kind, N, L, moduli, mred.data(), bred.data(), ninv.data(),
                        pow2 ? rf.data() : nullptr, pow2 ? rb.data() : nullptr, kind == RH_RING_3N ? om.data() : nullptr);
}

void rh_poly_slots_teardown(rh_ring* r);
extern "C" void rh_ring_destroy(rh_ring* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  void* ptrs[] = {r->d_cifold, r->d_consts, r->d_tw_fwd, r->d_tw_inv, r->d_tw_fwd_mont, r->d_twk_fwd, r->d_twk_inv, r->d_twk_fwd_mont, r->d_lastw, r->d_tw_inv_mont, r->d_consts_r, r->d_lastw_r};
  for (void* p : ptrs) if (p) (void)hipFree(p);
  for (RhHostSlot* sl : r->all_slots) {
    if (sl->buf) (void)hipFree(sl->buf);
    if (sl->stream) (void)hipStreamDestroy(sl->stream);
    delete sl;
  }
  rh_poly_slots_teardown(r);
  rh_rescale_teardown(r);
  for (int i = 0; i < 2; ++i) if (r->d_rs[i]) (void)hipFree(r->d_rs[i]);
  if (r->d_rows) (void)hipFree(r->d_rows);
  if (r->d_noise) (void)hipFree(r->d_noise);
  rh_ring3n_teardown(r);
  delete r;
}
extern "C" int rh_ring_n(const rh_ring* r) { return r ? r->N : 0; }
extern "C" int rh_ring_limbs(const rh_ring* r) { return r ? r->L : 0; }
extern "C" int rh_ring_get_constants(const rh_ring* r, uint64_t* moduli, uint64_t* mred, uint64_t* bred, uint64_t* ninv,
                                     uint64_t* roots_fwd, uint64_t* roots_bwd, uint64_t* omega3n) {
  if (!r) return rh_fail(RH_ERR_ARG, "null ring");
  if (moduli) memcpy(moduli, r->moduli.data(), r->moduli.size() * 8);
  if (mred) memcpy(mred, r->mred.data(), r->mred.size() * 8);
  if (bred) memcpy(bred, r->bred.data(), r->bred.size() * 8);
  if (ninv && !r->ninv.empty()) memcpy(ninv, r->ninv.data(), r->ninv.size() * 8);
  if (roots_fwd && !r->roots_fwd.empty()) memcpy(roots_fwd, r->roots_fwd.data(), r->roots_fwd.size() * 8);
  if (roots_bwd && !r->roots_bwd.empty()) memcpy(roots_bwd, r->roots_bwd.data(), r->roots_bwd.size() * 8);
  if (omega3n && !r->omega3n.empty()) memcpy(omega3n, r->omega3n.data(), r->omega3n.size() * 8);
  return RH_OK;
}
extern "C" int rh_ring_set_stream(rh_ring* r, void* s) { if (!r) return rh_fail(RH_ERR_ARG, "null ring"); r->stream = (hipStream_t)s; return RH_OK; }
extern "C" int rh_ring_sync(rh_ring* r) {
  if (!r) return rh_fail(RH_ERR_ARG, "null ring");
  hipError_t e = hipStreamSynchronize(rh_stream(r));
  if (e != hipSuccess) return rh_fail(RH_ERR_DEVICE, "hipStreamSynchronize: %s", hipGetErrorString(e));
  return RH_OK;
}

// ------------------------------------------------------------------------------------------------ device memory
extern "C" int rh_dev_alloc(rh_ring* r, size_t words, uint64_t** dptr) {
  if (!r || !dptr) return rh_fail(RH_ERR_ARG, "rh_dev_alloc: null argument");
  (void)hipSetDevice(r->device);
  if (hipMalloc((void**)dptr, words * 8) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(%zu words) failed", words);
  return RH_OK;
}
extern "C" int rh_dev_free(rh_ring* /*r: unused, may already be destroyed*/, uint64_t* dptr) { if (dptr) (void)hipFree(dptr); return RH_OK; }
extern "C" int rh_dev_upload(rh_ring* r, uint64_t* dst, const uint64_t* src, size_t words) {
  if (!r || !dst || !src) return rh_fail(RH_ERR_ARG, "rh_dev_upload: null argument");
  hipError_t e = hipMemcpyAsync(dst, src, words * 8, hipMemcpyHostToDevice, rh_stream(r));
  if (e == hipSuccess) e = hipStreamSynchronize(rh_stream(r));
  if (e != hipSuccess) return rh_fail(RH_ERR_DEVICE, "upload: %s", hipGetErrorString(e));
  return RH_OK;
}
// Poly.CopyLvl on device blocks (ring/poly.go): limbs 0..level of every poly of src (src_rows limbs per poly) into dst (dst_rows limbs per
// poly), asynchronous on the ring's stream
extern "C" int rh_ring_copy_rows(rh_ring* r, uint64_t* dst, int dst_rows, const uint64_t* src, int src_rows, int npoly, int level) {
  if (!r || !dst || !src) return rh_fail(RH_ERR_ARG, "rh_ring_copy_rows: null argument");
  if (level < 0 || level >= r->L || dst_rows < level + 1 || src_rows < level + 1 || npoly < 0) return rh_fail(RH_ERR_ARG, "rh_ring_copy_rows: bad level / rows / npoly");
  if (npoly == 0) return RH_OK;
  (void)hipSetDevice(r->device);
  const size_t N = (size_t)r->N;
  hipError_t e = hipMemcpy2DAsync(dst, (size_t)dst_rows * N * 8, src, (size_t)src_rows * N * 8, (size_t)(level + 1) * N * 8, (size_t)npoly,
                                  hipMemcpyDeviceToDevice, rh_stream(r));
  if (e != hipSuccess) return rh_fail(RH_ERR_DEVICE, "rh_ring_copy_rows: %s", hipGetErrorString(e));
  return RH_OK;
}
extern "C" int rh_dev_download(rh_ring* r, uint64_t* dst, const uint64_t* src, size_t words) {
  if (!r || !dst || !src) return rh_fail(RH_ERR_ARG, "rh_dev_download: null argument");
  hipError_t e = hipMemcpyAsync(dst, src, words * 8, hipMemcpyDeviceToHost, rh_stream(r));
  if (e == hipSuccess) e = hipStreamSynchronize(rh_stream(r));
  if (e != hipSuccess) return rh_fail(RH_ERR_DEVICE, "download: %s", hipGetErrorString(e));
  return RH_OK;
}

// ------------------------------------------------------------------------------------------------ launch plumbing (engine_internal.hpp)
int rh_launch_ok(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return rh_fail(RH_ERR_DEVICE, "%s launch failed: %s", what, hipGetErrorString(e));
  return RH_OK;
}
unsigned rh_stream_chunks(const rh_ring* r) {
  unsigned chunks = ((unsigned)r->N / 2 + 1023) / 1024; if (chunks < 1) chunks = 1; if (chunks > 64) chunks = 64;
  return chunks;
}
RhStreamGrid rh_stream_grid(const rh_ring* r, unsigned rows) {
  return {dim3(rows, rh_stream_chunks(r)), rh_nt_policy(r->nt_streams, (size_t)rows * (size_t)r->N * 8, (size_t)512 << 20) ? 1 : 0};
}
int rh_stage_slot(size_t words, RhStage** out, const char* who) {
  static thread_local RhStage slots[4];
  static thread_local unsigned next = 0;
  RhStage& s = slots[next++ % 4];
  if (s.done && hipEventSynchronize(s.done) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "%s: waiting for an earlier table copy failed", who);
  if (!s.done && hipEventCreateWithFlags(&s.done, hipEventDisableTiming) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "%s: hipEventCreate failed", who);
  if (s.words < words) {
    if (s.h) (void)hipHostFree(s.h);
    s.h = nullptr; s.words = 0;
    if (hipHostMalloc((void**)&s.h, words * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return rh_fail(RH_ERR_NOMEM, "%s: hipHostMalloc(%zu words) failed", who, words); }
    s.words = words;
  }
  *out = &s;
  return RH_OK;
}
int rh_stage_upload(RhStage* s, u64* table_dev, size_t words, hipStream_t st, const char* who) {
  if (hipMemcpyAsync(table_dev, s->h, words * 8, hipMemcpyHostToDevice, st) != hipSuccess || hipEventRecord(s->done, st) != hipSuccess)
    return rh_fail(RH_ERR_DEVICE, "%s: table copy failed", who);
  return RH_OK;
}
int rh_scheme_args(const rh_ring* r, int level, int npoly, unsigned kinds, int n_multiple, const char* who) {
  if (!r) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (!(kinds >> r->kind & 1))
    return kinds >> RH_RING_CI & 1 ? rh_fail(RH_ERR_ARG, "%s: the CKKS evaluator needs a standard or conjugate-invariant power-of-two ring (3N rings are not supported)", who)
                                   : rh_fail(RH_ERR_ARG, "%s: BGV tensoring needs a standard ring (3N and conjugate-invariant rings are not supported)", who);
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, r->L);
  if (level + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: at most %d limbs", who, RH_MAX_LIMBS);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  if (r->N < n_multiple || r->N % n_multiple) return rh_fail(RH_ERR_ARG, n_multiple == 2 ? "%s: N must be even" : "%s: N must be a multiple of %d", who, n_multiple);
  return 0;
}
int rh_comps3(const void* in0, const void* in1, const void* in2, const void* out0, const void* out1, const void* out2, const char* who) {
  if (!in0 || !out0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((in2 && !in1) || (in1 != nullptr) != (out1 != nullptr) || (in2 != nullptr) != (out2 != nullptr))
    return rh_fail(RH_ERR_ARG, "%s: components 1 and 2 need an input and an output each, and component 2 needs component 1", who);
  return 0;
}
int rh_pack_scalars(const rh_ring* r, int level, const u64* a, const u64* b, bool mont, RhScalars* s, const char* who, const char* noun) {
  memset(s, 0, sizeof(*s));
  for (int i = 0; i <= level; ++i) {
    const u64 q = r->moduli[i];
    if ((a && a[i] >= q) || (b && b[i] >= q)) return rh_fail(RH_ERR_ARG, "%s: %s of limb %d is not below its modulus", who, noun, i);
    if (a) s->a[i] = mont ? rh::mform(a[i], q) : a[i];
    if (b) s->b[i] = mont ? rh::mform(b[i], q) : b[i];
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------ NTT launches
// The launchers below take what they cannot decide themselves -- rows, strides, tables, body, cache policy, scale -- from the site that calls them
// (the sites' cache policies differ: engine_internal.hpp, rh_nt_rows and the lines after it).

// Tables and per-limb constants of limbs [limb0, ...).  mont_product: N^-1 * 2^64 in the last inverse stage (rh_ring_intt_mul, rh_ring_polymul)
struct NttTabs {
  const tw2 *tw_fwd, *twk_fwd, *tw_inv, *twk_inv, *lastw;
  const u64 *tw_fwd_mont, *twk_fwd_mont, *tw_inv_mont;
  const LimbConsts* c;
};
static NttTabs ntt_tabs(const rh_ring* r, int limb0, bool mont_product = false) {
  const size_t toff = (size_t)limb0 * r->N;
  auto at = [](auto* p, size_t off) { return p ? p + off : nullptr; };
  return {at(r->d_tw_fwd, toff), at(r->d_twk_fwd, toff), at(r->d_tw_inv, toff), at(r->d_twk_inv, toff), at(mont_product ? r->d_lastw_r : r->d_lastw, limb0),
          at(r->d_tw_fwd_mont, toff), at(r->d_twk_fwd_mont, toff), at(r->d_tw_inv_mont, toff), at(mont_product ? r->d_consts_r : r->d_consts, limb0)};
}
// The rows of one launch: npoly polys of Lrows limbs; Ls / Lso: rows per poly of the input / output block (0: dense, Lrows)
struct NttRows {
  const u64* in; u64* out; int npoly, Lrows, Ls, Lso;
  unsigned rows() const { return (unsigned)npoly * (unsigned)Lrows; }
};
enum NttBody { BODY_CPP, BODY_ASM, BODY_MONT };   // compiled Shoup body; hand-scheduled body; compiled Montgomery body (the forward lazy form keeps the reference's representatives)

// forward column stages, in -> out (N >= 8192; the hand-scheduled body exists for N = 2^14 .. 2^16, other degrees get the compiled one)
static void launch_fwd_cols(const NttTabs& t, hipStream_t st, int logN, const NttRows& x, NttBody body, bool nt) {
  const int S1 = logN - LT;
  const dim3 g(x.rows() * 16);
  if (body == BODY_ASM && rh_with_s1<2, 4>(S1, [&](auto S) { rh_with_flag(nt, [&](auto NT) {
        ntt_fwd_cols_asm<S(), NT()><<<g, 256, 0, st>>>(x.in, x.out, t.tw_fwd, t.c, x.Lrows, x.Ls, x.Lso); }); })) return;
  rh_with_s1<1, 5>(S1, [&](auto S) {
    if (body == BODY_MONT) ntt_fwd_cols<MontPolicy, S()><<<g, 256, 0, st>>>(x.in, x.out, t.tw_fwd_mont, t.c, x.Lrows, logN, x.Ls, x.Lso);
    else ntt_fwd_cols<ShoupPolicy, S()><<<g, 256, 0, st>>>(x.in, x.out, t.tw_fwd, t.c, x.Lrows, logN, x.Ls, x.Lso);
  });
}
// forward tile stages, in -> out
static void launch_fwd_tile(const NttTabs& t, hipStream_t st, int logN, const NttRows& x, NttBody body, bool nt) {
  const unsigned tiles = x.rows() << (logN - LT);
  if (body == BODY_MONT) ntt_fwd_tile<MontPolicy><<<tiles, 256, 0, st>>>(x.in, x.out, t.twk_fwd_mont, t.c, x.Lrows, logN, 0, x.npoly, x.Ls, x.Lso);
  else if (body == BODY_ASM) rh_with_flag(nt, [&](auto NT) { ntt_fwd_tile_asm<NT()><<<tiles, 256, 0, st>>>(x.in, x.out, t.twk_fwd, t.c, x.Lrows, logN, x.npoly, x.Ls, x.Lso); });
  else ntt_fwd_tile<ShoupPolicy><<<tiles, 256, 0, st>>>(x.in, x.out, t.twk_fwd, t.c, x.Lrows, logN, 1, x.npoly, x.Ls, x.Lso);
}
// inverse tile stages, in -> out.  The hand-scheduled body leaves values < 4q unscaled; scale: the compiled body of N = 4096 multiplies by N^-1
static void launch_inv_tile(const NttTabs& t, hipStream_t st, int logN, const NttRows& x, NttBody body, bool nt, int scale) {
  const unsigned tiles = x.rows() << (logN - LT);
  if (body == BODY_ASM) rh_with_flag(nt, [&](auto NT) { ntt_inv_tile_asm<NT()><<<tiles, 256, 0, st>>>(x.in, x.out, t.twk_inv, t.c, x.Lrows, logN, x.npoly, x.Ls, x.Lso); });
  else ntt_inv_tile<<<tiles, 256, 0, st>>>(x.in, x.out, t.twk_inv, t.c, x.Lrows, logN, scale, x.npoly, x.Ls, x.Lso);
}
// inverse column stages, in place on x.out (N >= 8192).  The hand-scheduled body (N = 2^14 .. 2^16) always scales by the table's N^-1
static void launch_inv_cols(const NttTabs& t, hipStream_t st, int logN, const NttRows& x, NttBody body, bool nt, int scale) {
  const int S1 = logN - LT;
  const dim3 g(x.rows() * 16);
  if (body == BODY_ASM && rh_with_s1<2, 4>(S1, [&](auto S) { rh_with_flag(nt, [&](auto NT) {
        ntt_inv_cols_asm<S(), NT()><<<g, 256, 0, st>>>(x.out, t.tw_inv, t.lastw, t.c, x.Lrows, x.Lso); }); })) return;
  rh_with_s1<1, 5>(S1, [&](auto S) { ntt_inv_cols<S()><<<g, 256, 0, st>>>(x.out, t.tw_inv, t.lastw, t.c, x.Lrows, logN, scale, x.Lso); });
}

// One-pass launches (N = 2^13, 2^14; ntt_kernels_asm.hip.hpp): 68 / 136 KiB of dynamic LDS per workgroup, beyond the 64 KiB default limit.
static bool one_pass_ok(rh_ring* r) {
  const int S1 = r->logN - LT;
  if (!(r->one_pass && r->asm_tile && S1 >= 1 && S1 <= 2)) return false;
  if (!r->one_pass_ready) {
    const int b1 = 2 * LDS_WORDS * 8, b2 = 4 * LDS_WORDS * 8;
    hipError_t e = hipSuccess;
    auto raise = [&](const void* f, int bytes) { if (e == hipSuccess) e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); };
    raise((const void*)ntt_fwd_onepass_asm<1, false>, b1); raise((const void*)ntt_fwd_onepass_asm<1, true>, b1);
    raise((const void*)ntt_fwd_onepass_asm<2, false>, b2); raise((const void*)ntt_fwd_onepass_asm<2, true>, b2);
    raise((const void*)ntt_inv_onepass_asm<1, false>, b1); raise((const void*)ntt_inv_onepass_asm<1, true>, b1);
    raise((const void*)ntt_inv_onepass_asm<2, false>, b2); raise((const void*)ntt_inv_onepass_asm<2, true>, b2);
    if (e != hipSuccess) { (void)hipGetLastError(); r->one_pass = false; return false; }     // (a device without that much LDS: the two-pass launches)
    r->one_pass_ready = true;
  }
  return true;
}
// the whole transform of a limb row in one workgroup: N = 2^13, 2^14, and the inverse of N = 4096 (the tile body, then N^-1 out of LDS)
static void launch_onepass(const NttTabs& t, hipStream_t st, int S1, const NttRows& x, bool inverse, bool nt, int scale) {
  const size_t lds = ((size_t)LDS_WORDS * 8) << S1;
  const dim3 wg(256u << S1);
  if (!inverse) rh_with_s1<1, 2>(S1, [&](auto S) { rh_with_flag(nt, [&](auto NT) {
      ntt_fwd_onepass_asm<S(), NT()><<<x.rows(), wg, lds, st>>>(x.in, x.out, t.tw_fwd, t.twk_fwd, t.c, x.Lrows, x.Ls, x.Lso); }); });
  else rh_with_s1<0, 2>(S1, [&](auto S) { rh_with_flag(nt, [&](auto NT) {
      ntt_inv_onepass_asm<S(), NT()><<<x.rows(), wg, lds, st>>>(x.in, x.out, t.twk_inv, t.tw_inv, t.lastw, t.c, x.Lrows, x.Ls, x.Lso, scale); }); });
}
// rings below N = 4096: one launch.  mont_inv: the non-canonical BackwardLazy of N = 8 on the Montgomery table
static int launch_small(const NttTabs& t, hipStream_t st, int logN, const NttRows& x, bool inverse, bool lazy, bool mont_inv, int scale) {
  if (!inverse) {
    if (lazy) ntt_fwd_small<MontPolicy><<<x.rows(), 256, 0, st>>>(x.in, x.out, t.tw_fwd_mont, t.c, x.Lrows, logN, 0, x.Ls, x.Lso);
    else      ntt_fwd_small<ShoupPolicy><<<x.rows(), 256, 0, st>>>(x.in, x.out, t.tw_fwd, t.c, x.Lrows, logN, 1, x.Ls, x.Lso);
  } else if (mont_inv) {
    if (x.Ls || x.Lso) return rh_fail(RH_ERR_UNSUPPORTED, "strided non-canonical BackwardLazy of N = 8");          // (ntt_rows compacts this one shape)
    ntt_inv_small_lazy_mont<<<x.rows(), 64, 0, st>>>(x.in, x.out, t.tw_inv_mont, t.c, x.Lrows, logN);   // N = 8: BackwardLazy is not canonical
  } else {
    ntt_inv_small<<<x.rows(), 256, 0, st>>>(x.in, x.out, t.tw_inv, t.c, x.Lrows, logN, scale, x.Ls, x.Lso);
  }
  return rh_launch_ok("ntt_small");
}

// The stages of a two-pass span transform as the ring's tuning picks their bodies, with the span's cache policy (rh_nt_rows).
static void span_fwd_cols(rh_ring* r, const NttRows& x, int limb0, bool lazy) {
  launch_fwd_cols(ntt_tabs(r, limb0), rh_stream(r), r->logN, x, lazy ? BODY_MONT : (r->asm_cols && r->asm_tile ? BODY_ASM : BODY_CPP), rh_nt_rows(r, x.rows()));
}
// x.in: where the column stages wrote (the OUTPUT block, its stride on both sides) or, without column stages (N = 4096), the input block
static void span_fwd_tile(rh_ring* r, const NttRows& x, int limb0, bool lazy) {
  const int lso = x.Lso ? x.Lso : (x.Ls ? x.Ls : x.Lrows);
  const int ls = (x.in == x.out) ? lso : (x.Ls ? x.Ls : x.Lrows);
  launch_fwd_tile(ntt_tabs(r, limb0), rh_stream(r), r->logN, NttRows{x.in, x.out, x.npoly, x.Lrows, ls, lso},
                  lazy ? BODY_MONT : (r->asm_tile ? BODY_ASM : BODY_CPP), rh_nt_rows(r, x.rows()));
}
// the hand-scheduled body leaves values < 4q unscaled: right whenever column stages follow, and for N = 4096 sub-rings of the 3N transform
// (inv_scale = false), which scale in their own last layer
static void span_inv_tile(rh_ring* r, const NttRows& x, int limb0) {
  const bool n4096 = r->logN == LT;
  launch_inv_tile(ntt_tabs(r, limb0), rh_stream(r), r->logN, x, r->asm_tile && (!n4096 || !r->inv_scale) ? BODY_ASM : BODY_CPP, rh_nt_rows(r, x.rows()),
                  (n4096 && r->inv_scale) ? 1 : 0);
}
static void span_inv_cols(rh_ring* r, const NttRows& x, int limb0) {
  launch_inv_cols(ntt_tabs(r, limb0), rh_stream(r), r->logN, x, r->asm_cols && r->asm_tile && r->inv_scale ? BODY_ASM : BODY_CPP, rh_nt_rows(r, x.rows()),
                  r->inv_scale ? 1 : 0);
}

// limb0: first limb of the table set to use (host-pointer single-limb path); rows = npoly * Lrows.
static int std_ntt_launch_span(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse, bool lazy,
                               int Ls = 0, int Lso = 0) {   // Ls / Lso: rows per poly of the input / output block when > Lrows (0: Lrows / Ls): AtLevel views
  (void)hipGetLastError();                       // drop any stale error of an unrelated earlier call
  if (Ls && !Lso) Lso = Ls;                      // one stride given: both sides
  if (Lso && !Ls) Ls = Lrows;
  const NttRows x{in, out, npoly, Lrows, Ls, Lso};
  if (x.rows() == 0) return RH_OK;
  const int logN = r->logN, sc = r->inv_scale ? 1 : 0;
  const NttTabs t = ntt_tabs(r, limb0);
  if (logN < LT) return launch_small(t, rh_stream(r), logN, x, inverse, lazy, lazy && logN < 4 && r->d_tw_inv_mont && r->kind == RH_RING_STANDARD, sc);
  const bool nt = rh_nt_rows(r, x.rows());      // non-temporal data streams beyond the Infinity Cache
  if (!(lazy && !inverse) && one_pass_ok(r)) {          // (the forward lazy form keeps the reference's representatives: Montgomery bodies, two passes)
    launch_onepass(t, rh_stream(r), logN - LT, x, inverse, nt, sc);
    return rh_launch_ok("ntt (one pass)");
  }
  if (!inverse) {
    span_fwd_cols(r, x, limb0, lazy);
    span_fwd_tile(r, NttRows{logN > LT ? out : in, out, npoly, Lrows, Ls, Lso}, limb0, lazy);
  } else {
    if (r->asm_tile && logN == LT && r->inv_scale && r->one_pass) {          // N = 4096 WITH scaling: the tile body, then N^-1 out of LDS
      launch_onepass(t, rh_stream(r), 0, x, true, nt, 1);
      return rh_launch_ok("ntt (N = 4096, inverse)");
    }
    span_inv_tile(r, x, limb0);
    span_inv_cols(r, x, limb0);
  }
  return rh_launch_ok("ntt");
}
// One stage of the two-pass transform (rh_ring_ntt_phase's profiling aid; bext.hip and ntt3n.hip, whose own kernels do the other stage):
// 1 = column stages only (forward in -> out, inverse in place on out), 2 = tile stages only, in -> out.  Rings below N = 4096 have no stages:
// the whole transform
static int std_ntt_launch_stage(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse, int phase) {
  if (r->logN < LT) return std_ntt_launch_span(r, in, out, npoly, Lrows, limb0, inverse, false);
  (void)hipGetLastError();
  const NttRows x{in, out, npoly, Lrows, 0, 0};
  if (x.rows() == 0) return RH_OK;
  if (phase == 1) inverse ? span_inv_cols(r, x, limb0) : span_fwd_cols(r, x, limb0, false);
  else            inverse ? span_inv_tile(r, x, limb0) : span_fwd_tile(r, x, limb0, false);
  return rh_launch_ok("ntt");
}

// ---- software pipelines over spans of polys in ONE stream: launch j works on span j and on span j-1 (and j-2)
// Span size for a batch of npoly polys of Lrows limbs, 0 = no pipeline.  chunk_polys < 0 (auto): batches of more than ~auto_span_rows limb rows go in
// spans of ~auto_span_rows rows (128 polys at 16 limbs; measured optimum: 64..128); > 0: that many polys per span; 0: never
static int rh_span_polys(const rh_ring* r, int Lrows, long npoly) {
  int chunk = r->chunk_polys;
  if (chunk < 0) { chunk = r->auto_span_rows / (Lrows > 0 ? Lrows : 1); if (chunk < 1) chunk = 1; }
  return chunk > 0 && npoly > chunk ? chunk : 0;
}
// The spans of one or several blocks (a block's last span may be shorter); outside [0, count()): 0 polys at the head of block 0, which is what launch j
// asks for when span j or j-1 does not exist
struct Span { int block, p0, polys; };
struct SpanWalk {
  std::vector<Span> spans;
  void add(int block, int npoly, int chunk) { for (int p = 0; p < npoly; p += chunk) spans.push_back(Span{block, p, npoly - p < chunk ? npoly - p : chunk}); }
  SpanWalk() {}
  SpanWalk(int npoly, int chunk) { add(0, npoly, chunk); }
  int count() const { return (int)spans.size(); }
  Span operator()(int j) const { return j >= 0 && j < count() ? spans[j] : Span{0, 0, 0}; }
};

// Forward canonical transform of a large batch: launch j runs the column stages of span j fused with the tile stages of span j-1 (ntt_fwd_fused).
// The spans may come from several blocks (rh_ring_ntt_many): the pipeline runs through the block boundaries, so only the first launch of the first
// block and the last launch of the last block are not fused.
struct NttSeg { const u64* in; u64* out; int npoly; };
static int std_ntt_fwd_pipelined_segs(rh_ring* r, const NttSeg* segs, int nseg, int Lrows, int limb0, int chunk) {
  (void)hipGetLastError();
  const int logN = r->logN, S1 = logN - LT;
  const size_t stride = (size_t)Lrows * r->N;
  const NttTabs t = ntt_tabs(r, limb0);
  hipStream_t st = rh_stream(r);
  SpanWalk w;
  for (int k = 0; k < nseg; ++k) w.add(k, segs[k].npoly, chunk);
  for (int j = 0; j <= w.count(); ++j) {
    const Span s1 = w(j), s2 = w(j - 1);
    const unsigned n1 = (unsigned)s1.polys * Lrows * 16, n2 = ((unsigned)s2.polys * Lrows) << S1, grid = n1 > n2 ? n1 : n2;
    const u64* in1 = segs[s1.block].in + (size_t)s1.p0 * stride; u64* out1 = segs[s1.block].out + (size_t)s1.p0 * stride;
    u64* data2 = segs[s2.block].out + (size_t)s2.p0 * stride;
    const int npoly2 = s2.polys;
    if (r->asm_tile && r->asm_cols && rh_with_s1<2, 4>(S1, [&](auto S) { rh_with_flag(rh_nt_key(r), [&](auto NT) {
          ntt_fwd_fused_asm<S(), true, NT()><<<grid, 256, 0, st>>>(in1, out1, n1, data2, n2, npoly2, t.tw_fwd, t.twk_fwd, t.c, Lrows, logN); }); })) continue;
    rh_with_s1<1, 5>(S1, [&](auto S) {
      if (r->asm_tile) ntt_fwd_fused_asm<S(), false, RH_NT_FUSED_DEFAULT><<<grid, 256, 0, st>>>(in1, out1, n1, data2, n2, npoly2, t.tw_fwd, t.twk_fwd, t.c, Lrows, logN);
      else ntt_fwd_fused<ShoupPolicy, S()><<<grid, 256, 0, st>>>(in1, out1, n1, data2, n2, npoly2, t.tw_fwd, t.twk_fwd, t.c, Lrows, logN, 1);
    });
  }
  return rh_launch_ok("ntt_fwd_fused");
}

// Inverse transform of a large batch (hand-scheduled tile body): launch j = tile stages of span j fused with column stages (+ N^-1) of span j-1.
// in_b: rh_ring_intt_mul: the product a . b on load, 2^64-scaled N^-1 constants
static int std_ntt_inv_pipelined(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, int chunk, const u64* in_b = nullptr) {
  (void)hipGetLastError();
  const int logN = r->logN, S1 = logN - LT;
  const size_t stride = (size_t)Lrows * r->N;
  const NttTabs t = ntt_tabs(r, limb0, in_b != nullptr);
  hipStream_t st = rh_stream(r);
  const SpanWalk w(npoly, chunk);
  for (int j = 0; j <= w.count(); ++j) {
    const Span s1 = w(j), s2 = w(j - 1);
    const unsigned n1 = ((unsigned)s1.polys * Lrows) << S1, n2 = (unsigned)s2.polys * Lrows * 16, grid = n1 > n2 ? n1 : n2;
    const u64* in1 = in + (size_t)s1.p0 * stride; u64* out1 = out + (size_t)s1.p0 * stride; u64* data2 = out + (size_t)s2.p0 * stride;
    const u64* in1b = in_b ? in_b + (size_t)s1.p0 * stride : nullptr;
    const int npoly1 = s1.polys;
    rh_with_flag(in_b != nullptr, [&](auto MUL) {
      if (r->asm_cols && rh_with_s1<2, 4>(S1, [&](auto S) {
            if constexpr (MUL()) ntt_inv_fused_asm<S(), true, true, RH_NT_FUSED_DEFAULT><<<grid, 256, 0, st>>>(in1, in1b, out1, n1, npoly1, data2, n2, t.twk_inv, t.tw_inv, t.lastw, t.c, Lrows, logN);
            else rh_with_flag(rh_nt_key(r), [&](auto NT) {
              ntt_inv_fused_asm<S(), true, false, NT()><<<grid, 256, 0, st>>>(in1, in1b, out1, n1, npoly1, data2, n2, t.twk_inv, t.tw_inv, t.lastw, t.c, Lrows, logN); });
          })) return;
      rh_with_s1<1, 5>(S1, [&](auto S) {
        ntt_inv_fused_asm<S(), false, MUL(), RH_NT_FUSED_DEFAULT><<<grid, 256, 0, st>>>(in1, in1b, out1, n1, npoly1, data2, n2, t.twk_inv, t.tw_inv, t.lastw, t.c, Lrows, logN); });
    });
  }
  return rh_launch_ok("ntt_inv_fused_asm");
}

// phase: 0 = whole transform; 1 / 2: std_ntt_launch_stage, the one place that reads it
int rh_std_ntt_launch(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse, bool lazy, int phase) {
  if (phase) return std_ntt_launch_stage(r, in, out, npoly, Lrows, limb0, inverse, phase);
  const int chunk = rh_span_polys(r, Lrows, npoly);
  const bool two_pass = r->logN > LT && !one_pass_ok(r);
  if (chunk && two_pass && !inverse && !lazy) {
    const NttSeg seg{in, out, npoly};
    return std_ntt_fwd_pipelined_segs(r, &seg, 1, Lrows, limb0, chunk);
  }
  if (chunk && two_pass && inverse && r->asm_tile && r->inv_scale) return std_ntt_inv_pipelined(r, in, out, npoly, Lrows, limb0, chunk);
  return std_ntt_launch_span(r, in, out, npoly, Lrows, limb0, inverse, lazy);
}

// Forward canonical transform, in place, of limbs [limb0, limb0 + Lrows) of each poly of a block that has Ls >= Lrows
// rows per poly (`data` points at row limb0 of poly 0): lets a caller skip rows it will overwrite anyway (the digit's own
// limbs in DecomposeSingleNTT).  N >= 4096 standard rings; the pipelined launches are not involved.
int rh_std_ntt_fwd_strided(rh_ring* r, u64* data, int npoly, int Lrows, int limb0, int Ls) {
  if (r->logN < LT || Ls < Lrows) return rh_fail(RH_ERR_ARG, "strided transform needs N >= 4096 and a row stride >= the row count");
  if (Lrows <= 0 || npoly <= 0) return RH_OK;
  return std_ntt_launch_span(r, data, data, npoly, Lrows, limb0, false, false, Ls);
}

// Forward canonical transform, in place, of the non-digit limbs of every digit block of a hybrid decomposition
// (DecomposeSingleNTT, core/rlwe/evaluator_gadget_product.go:455-478, for all digits at once): block j holds npoly polys
// of LQ rows and its limbs [j*LP, min((j+1)*LP, LQ)) are left alone.  One software-pipelined stream of launches instead of
// two strided transforms (before / after the digit's limbs) per digit.  Needs the hand-scheduled bodies (N = 2^14 .. 2^16).
// lazy_out: the outputs stay < 8q, not canonical (for a consumer that reduces anyway, never for a caller-visible block).
bool rh_can_ntt_digits(const rh_ring* r) {
  const int S1 = r->logN - LT;
  return r->kind == RH_RING_STANDARD && r->asm_tile && r->asm_cols && r->digit_pipeline && S1 >= 2 && S1 <= 4;
}
// Small batches: every block of ring r -- and, when r2 is given, every (gap-free) block of a second ring of the same degree: the P blocks of a key switch
// beside its Q blocks -- in ONE launch of the column stages and one of the tile stages (blockIdx.y = block).  At most 8 blocks per ring.
int rh_std_ntt_fwd_blocks_small(rh_ring* r, u64* data, size_t block_stride, int nblocks, int Ls, const int* gap0, const int* gap_len,
                                rh_ring* r2, u64* data2, size_t block_stride2, int nblocks2, int Ls2, int npoly, bool lazy_out) {
  if (!rh_can_ntt_digits(r) || (r2 && (!rh_can_ntt_digits(r2) || r2->logN != r->logN)) || nblocks > 8 || nblocks2 > 8)
    return rh_fail(RH_ERR_UNSUPPORTED, "small-batch block transform: hand-scheduled bodies, one ring degree, at most 8 blocks per ring");
  if (npoly <= 0 || nblocks <= 0) return RH_OK;
  (void)hipGetLastError();
  const int S1 = r->logN - LT;
  hipStream_t st = rh_stream(r);
  unsigned n1 = 0, n2 = 0;
  auto fill = [&](BlockSet& bs, rh_ring* R, u64* d, size_t stride, int nb, int rows, const int* g0, const int* gl, bool cols) {
    memset(&bs, 0, sizeof bs);
    if (!R) return;
    bs.data = d; bs.stride = stride; bs.tw = cols ? R->d_tw_fwd : R->d_twk_fwd; bs.consts = R->d_consts; bs.nblocks = nb; bs.g.Ls = rows;
    for (int j = 0; j < nb; ++j) {
      const int gl_j = gl ? gl[j] : 0;
      bs.g.L[j] = rows - gl_j; bs.g.gap0[j] = (u32)(g0 ? g0[j] : 0); bs.g.gap_len[j] = (u32)gl_j;
      const unsigned a = (unsigned)npoly * bs.g.L[j] * 16, b = ((unsigned)npoly * bs.g.L[j]) << S1;
      if (a > n1) n1 = a;
      if (b > n2) n2 = b;
    }
  };
  BlockSet ca, cb, ta, tb;
  fill(ca, r, data, block_stride, nblocks, Ls, gap0, gap_len, true); fill(cb, r2, data2, block_stride2, nblocks2, Ls2, nullptr, nullptr, true);
  fill(ta, r, data, block_stride, nblocks, Ls, gap0, gap_len, false); fill(tb, r2, data2, block_stride2, nblocks2, Ls2, nullptr, nullptr, false);
  if (!n1) return RH_OK;
  const unsigned ny = (unsigned)(nblocks + (r2 ? nblocks2 : 0));
  rh_with_s1<2, 4>(S1, [&](auto S) {             // (cache policy: RH_NT_NEVER, the kernels have no other form)
    ntt_fwd_cols_blocks_asm<S()><<<dim3(n1, ny), 256, 0, st>>>(ca, cb, npoly);
    rh_with_flag(lazy_out, [&](auto LAZY) { ntt_fwd_tile_blocks_asm<S(), LAZY()><<<dim3(n2, ny), 256, 0, st>>>(ta, tb, npoly); });
  });
  return rh_launch_ok("ntt_fwd_blocks (small batch)");
}
int rh_std_ntt_fwd_blocks(rh_ring* r, u64* data, size_t block_stride, int npoly, int nblocks, int Ls, const int* gap0, const int* gap_len,
                          bool lazy_out, int small) {       // small: 1 / 0 = every block in one launch pair / the pipelined stream; -1 = by the ring's ks_small_rows                  // block j: npoly polys of Ls rows, rows [gap0[j], gap0[j] + gap_len[j]) left alone
  if (!rh_can_ntt_digits(r)) return rh_fail(RH_ERR_UNSUPPORTED, "digit-block transform needs the hand-scheduled bodies (2^14 <= N <= 2^16)");
  if (npoly <= 0 || nblocks <= 0) return RH_OK;
  (void)hipGetLastError();
  const int S1 = r->logN - LT;
  hipStream_t st = rh_stream(r);
  auto rows = [&](int j) {                          // block j: its transformed rows
    GapRows g; g.Ls = Ls; g.gap0 = (u32)gap0[j]; g.gap_len = (u32)gap_len[j]; g.L = Ls - gap_len[j];
    return g;
  };
  if (small < 0) small = r->ks_small_rows > 0 && (long)npoly * Ls <= r->ks_small_rows;
  if (small && nblocks <= 8) return rh_std_ntt_fwd_blocks_small(r, data, block_stride, nblocks, Ls, gap0, gap_len, nullptr, nullptr, 0, 0, 0, npoly, lazy_out);
  // non-temporal data streams once a block is too large to be re-read from the Infinity Cache by the next launch's tile stages
  const bool nt = rh_nt_gap(r, npoly, Ls);          // 256 MiB, not rh_stream_grid's 512: see above
  for (int j = 0; j <= nblocks; ++j) {               // (every block is one span: launch j = column stages of block j, tile stages of block j-1)
    GapRows g1 = j < nblocks ? rows(j) : GapRows{1, 1, 0, 0}, g2 = j >= 1 ? rows(j - 1) : GapRows{1, 1, 0, 0};
    const unsigned n1 = j < nblocks ? (unsigned)npoly * g1.L * 16 : 0, n2 = j >= 1 ? ((unsigned)npoly * g2.L) << S1 : 0;
    const unsigned grid = n1 > n2 ? n1 : n2;
    if (!grid) continue;
    if (!g1.L) g1.L = 1;
    if (!g2.L) g2.L = 1;
    u64* d1 = data + (size_t)(j < nblocks ? j : 0) * block_stride; u64* d2 = data + (size_t)(j >= 1 ? j - 1 : 0) * block_stride;
    rh_with_s1<2, 4>(S1, [&](auto S) { rh_with_flag(lazy_out, [&](auto LAZY) { rh_with_flag(nt, [&](auto NT) {
      ntt_fwd_fused_gap_asm<S(), LAZY(), NT()><<<grid, 256, 0, st>>>(d1, n1, g1, d2, n2, npoly, g2, r->d_tw_fwd, r->d_twk_fwd, r->d_consts); }); }); });
  }
  return rh_launch_ok("ntt_fwd_fused_gap_asm");
}
int rh_std_ntt_fwd_digits(rh_ring* r, u64* data, size_t digit_stride, int npoly, int beta, int LQ, int LP, bool lazy_out, int small) {
  if (beta <= 0) return RH_OK;
  std::vector<int> g0(beta), gl(beta);
  for (int j = 0; j < beta; ++j) {                  // digit j skips its own limbs [j LP, min((j+1) LP, LQ))
    int n = LQ - j * LP; if (n > LP) n = LP; if (n < 0) n = 0;
    g0[j] = j * LP; gl[j] = n;
  }
  return rh_std_ntt_fwd_blocks(r, data, digit_stride, npoly, beta, LQ, g0.data(), gl.data(), lazy_out, small);
}

// Inverse canonical transform of ONE limb of every poly of a block with in_rows limbs per poly into a dense block of npoly rows
// (the last limb of a rescale step): the tile kernel reads the limb where it lies -- no gather copy.  Hand-scheduled bodies only.
bool rh_can_intt_limb_strided(const rh_ring* r) {
  const int S1 = r->logN - LT;
  return r->kind == RH_RING_STANDARD && r->asm_tile && r->asm_cols && r->inv_scale && S1 >= 2 && S1 <= 4;
}
int rh_std_intt_limb_strided(rh_ring* r, const u64* in, int in_rows, int limb, u64* out, int npoly) {
  if (!rh_can_intt_limb_strided(r)) return rh_fail(RH_ERR_UNSUPPORTED, "strided single-limb inverse transform needs the hand-scheduled bodies");
  if (npoly <= 0) return RH_OK;
  (void)hipGetLastError();
  const NttTabs t = ntt_tabs(r, limb);
  const NttRows x{in + (size_t)limb * r->N, out, npoly, 1, in_rows, 0};
  launch_inv_tile(t, rh_stream(r), r->logN, x, BODY_ASM, RH_NT_NEVER, 0);
  launch_inv_cols(t, rh_stream(r), r->logN, x, BODY_ASM, RH_NT_NEVER, 1);
  return rh_launch_ok("strided single-limb inverse transform");
}

// Inverse canonical transform of limbs 0..Lrows-1 of every poly of a block with in_rows limbs per poly into a block with out_rows limbs per
// poly (ring.AtLevel views of larger polys): one batched launch pair.  Hand-scheduled bodies only (N = 2^14 .. 2^16).
int rh_std_intt_rows(rh_ring* r, const u64* in, int in_rows, u64* out, int out_rows, int npoly, int Lrows) {
  if (!rh_can_intt_limb_strided(r)) return rh_fail(RH_ERR_UNSUPPORTED, "strided inverse transform needs the hand-scheduled bodies");
  if (npoly <= 0 || Lrows <= 0) return RH_OK;
  (void)hipGetLastError();
  const NttTabs t = ntt_tabs(r, 0);
  const NttRows x{in, out, npoly, Lrows, in_rows, out_rows};
  launch_inv_tile(t, rh_stream(r), r->logN, x, BODY_ASM, RH_NT_NEVER, 0);
  launch_inv_cols(t, rh_stream(r), r->logN, x, BODY_ASM, RH_NT_NEVER, 1);
  return rh_launch_ok("strided inverse transform");
}

// ---- 3N transform (ntt3n.hip), b = 1: the hand-scheduled layer kernels live in this translation unit with the tile bodies they fuse with
void rh_3n_launch_layer(bool inverse, int S1, unsigned nblocks, hipStream_t st, const u64* in, u64* out, const N3Layer& a, int nt_streams) {
  // a unit moves 6 * 2^S1 coefficients per thread: nblocks * 256 * 6 * 2^S1 * 8 bytes per direction; non-temporal streams beyond 512 MiB
  // (rh_stream_grid's threshold on this launch's own byte count: its work comes in blocks, not in rows of N)
  const bool nt = rh_nt_policy(nt_streams, (size_t)nblocks * 256 * 6 * ((size_t)8 << S1), (size_t)512 << 20);   // tuning nt_streams = 0: default policy everywhere, 2: non-temporal at every size
  rh_with_s1<1, 3>(S1, [&](auto S) { rh_with_flag(inverse, [&](auto INV) { rh_with_flag(nt, [&](auto NT) {
    ntt3n_layer_asm<S(), INV(), NT()><<<nblocks, 256, 0, st>>>(in, out, a); }); }); });
}
bool rh_can_fuse_submul(const rh_ring* r) { return r->kind == RH_RING_STANDARD && r->logN >= LT && r->fuse_submul; }

// rescale: column stages of limbs 0..Lrows-1 fed by the re-expansion of the coefficient-domain last limb `tmp` (N >= 8192)
int rh_std_ntt_expand_cols_launch(rh_ring* r, const u64* tmp, u64* buf, int npoly, int Lrows, const void* table_dev, int mode, u64 qL) {
  const int S1 = r->logN - LT;
  if (S1 < 1 || S1 > 5) return rh_fail(RH_ERR_UNSUPPORTED, "expand + column stages need 8192 <= N <= 2^17");
  const unsigned rows = (unsigned)npoly * (unsigned)Lrows;
  if (rows == 0) return RH_OK;
  (void)hipGetLastError();
  const RescaleLimb* T = (const RescaleLimb*)table_dev;
  const dim3 g(rows * 16);
  hipStream_t st = rh_stream(r);
  bool lazy_ok = r->asm_tile && r->asm_cols;             // hand-scheduled body (N = 2^14 .. 2^16): needs qL + q <= 8q for every limb
  for (int i = 0; i < Lrows && lazy_ok; ++i) lazy_ok = qL / 7 <= r->moduli[i] && qL - 1 < 7 * r->moduli[i];
  const bool nt = rh_nt_rows(r, rows);                   // non-temporal data streams for working sets far beyond the Infinity Cache
  if (lazy_ok && rh_with_s1<2, 4>(S1, [&](auto S) { rh_with_flag(nt, [&](auto NT) {
        ntt_fwd_cols_expand_asm<S(), NT()><<<g, 256, 0, st>>>(tmp, buf, r->d_tw_fwd, r->d_consts, T, Lrows, mode, qL); }); }))
    return rh_launch_ok("ntt_fwd_cols_expand_asm");
  rh_with_s1<1, 5>(S1, [&](auto S) { ntt_fwd_cols_expand<S()><<<g, 256, 0, st>>>(tmp, buf, r->d_tw_fwd, r->d_consts, T, Lrows, r->logN, mode, qL); });
  return rh_launch_ok("ntt_fwd_cols_expand");
}

// Forward canonical transform of `buf` (in place up to its tile stages) fused with out = MRed(2q - y + NTT(buf), s_limb):
// column stages as usual, then ntt_fwd_tile_submul.  y / out: (poly, limb) blocks with y_rows / out_rows limbs per poly.
// MRed by a limb's scalar = Shoup multiply by s * 2^-64 mod q: the by-value pack of limbs [limb0, limb0 + Lrows)
static LimbShoup limb_shoup_pack(const rh_ring* r, int limb0, int Lrows, const u64* scalars_host) {
  LimbShoup sh; memset(&sh, 0, sizeof(sh));
  for (int i = 0; i < Lrows; ++i) {
    const u64 q = r->moduli[limb0 + i];
    sh.w[i] = rh::imform(scalars_host[i] % q, q); sh.wp[i] = rh::shoup_quotient(sh.w[i], q);
  }
  return sh;
}
// Both components of a ModDown in ONE launch: buf holds 2 * npoly polys (component 0 then component 1, column stages done), component c goes with
// (y_c, out_c, z_c); z0 and z1 are both given or both null.  Hand-scheduled bodies only (the caller checks rh_can_fuse_submul and asm_tile).
int rh_std_ntt_submul_launch_pair(rh_ring* r, u64* buf, int npoly, int Lrows, const u64* y0, const u64* y1, int y_rows, u64* out0, u64* out1, int out_rows,
                                  const u64* scalars_host, const u64* z0, const u64* z1, int z_rows) {
  if (!rh_can_fuse_submul(r) || !r->asm_tile || (z0 == nullptr) != (z1 == nullptr)) return rh_fail(RH_ERR_UNSUPPORTED, "paired subtract-multiply: hand-scheduled bodies, both addends or none");
  const unsigned rows = 2u * (unsigned)npoly * (unsigned)Lrows;
  if (rows == 0) return RH_OK;
  const int S1 = r->logN - LT;
  (void)hipGetLastError();
  const LimbShoup sh = limb_shoup_pack(r, 0, Lrows, scalars_host);
  const bool nt = rh_nt_rows(r, rows / 2);              // (the policy of one component's launch, as before the two were paired)
  hipStream_t st = rh_stream(r);
  rh_with_flag(z0 != nullptr, [&](auto ADD) { rh_with_flag(nt, [&](auto NT) {
    ntt_fwd_tile_submul_asm<ADD(), NT()><<<rows << S1, 256, 0, st>>>(buf, r->d_twk_fwd, r->d_consts, Lrows, r->logN, 2 * npoly, y0, y_rows, out0, out_rows, sh, z0, z_rows, npoly, y1, out1, z1); }); });
  return rh_launch_ok("ntt_fwd_tile_submul_asm (pair)");
}
int rh_std_ntt_submul_launch(rh_ring* r, u64* buf, int npoly, int Lrows, int limb0, const u64* y, int y_rows, u64* out, int out_rows,
                             const u64* scalars_host, bool cols_done, const u64* z, int z_rows) {
  static_assert(RH_MAX_LIMBS_K == RH_MAX_LIMBS, "limb bound mismatch");
  if (!rh_can_fuse_submul(r)) return rh_fail(RH_ERR_UNSUPPORTED, "fused subtract-multiply needs a standard ring with N >= 4096");
  const unsigned rows = (unsigned)npoly * (unsigned)Lrows;
  if (rows == 0) return RH_OK;
  const int S1 = r->logN - LT;
  (void)hipGetLastError();
  if (S1 > 0 && !cols_done) {
    span_fwd_cols(r, NttRows{buf, buf, npoly, Lrows, 0, 0}, limb0, false);
    if (int rc = rh_launch_ok("ntt")) return rc;
  }
  const NttTabs t = ntt_tabs(r, limb0);
  hipStream_t st = rh_stream(r);
  if (r->asm_tile) {
    const LimbShoup sh = limb_shoup_pack(r, limb0, Lrows, scalars_host);
    rh_with_flag(z != nullptr, [&](auto ADD) { rh_with_flag(rh_nt_rows(r, rows), [&](auto NT) {
      ntt_fwd_tile_submul_asm<ADD(), NT()><<<rows << S1, 256, 0, st>>>(buf, t.twk_fwd, t.c, Lrows, r->logN, npoly, y, y_rows, out, out_rows, sh, z, ADD() ? z_rows : 0); }); });
    return rh_launch_ok("ntt_fwd_tile_submul_asm");
  }
  LimbScalars sc; memset(&sc, 0, sizeof(sc)); memcpy(sc.s, scalars_host, (size_t)Lrows * 8);
  ntt_fwd_tile_submul<<<rows << S1, 256, 0, st>>>(buf, t.twk_fwd, t.c, Lrows, r->logN, npoly, y, y_rows, out, out_rows, sc, z, z_rows);
  return rh_launch_ok("ntt_fwd_tile_submul");
}

// ---- conjugate-invariant ring Z[X+X^-1]/(X^2N+1) (ring/ntt.go:716-1311): the negacyclic kernels on the re-indexed
// 4N-th-root table, plus the fold with F = roots[1] before (forward :761-768) / after (inverse :1149-1156) them.
__global__ void __launch_bounds__(256)
ci_fold_kernel(const u64* in, u64* out, int logN, const CiFold* __restrict__ fold, const LimbConsts* __restrict__ consts, int L, int inverse) {
  const u32 N = 1u << logN;
  const u32 limb = blockIdx.x % (u32)L;
  const LimbConsts c = consts[limb];
  const tw2 F = inverse ? fold[limb].b : fold[limb].f;
  const u64 q4 = 4 * c.q;
  const size_t base = (size_t)blockIdx.x << logN;
  for (u32 jx = blockIdx.y * blockDim.x + threadIdx.x; jx <= (N >> 1); jx += gridDim.y * blockDim.x) {
    if (jx == 0) {
      const u64 x = in[base];
      out[base] = inverse ? cred(2 * csub(csub(x, 2 * c.q), c.q), c.q) : x;          // p2[0] = CRed(p2[0] << 1) (:1157) / p1[0] (:770)
    } else if (jx == (N >> 1)) {
      const u64 x = csub(in[base + jx], q4);
      const u64 v = x + q4 - shoup_mul(x, F.w, F.wp, c.nq);
      out[base + jx] = inverse ? canon8(v, c.q) : v;
    } else {
      const u32 jy = N - jx;
      const u64 a = csub(in[base + jx], q4), b = csub(in[base + jy], q4);
      const u64 va = a + q4 - shoup_mul(b, F.w, F.wp, c.nq), vb = b + q4 - shoup_mul(a, F.w, F.wp, c.nq);
      out[base + jx] = inverse ? canon8(va, c.q) : va;
      out[base + jy] = inverse ? canon8(vb, c.q) : vb;
    }
  }
}
static int ci_ntt_launch(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse) {
  const unsigned rows = (unsigned)npoly * Lrows;
  if (!rows) return RH_OK;
  unsigned chunks = ((unsigned)r->N / 2 + 256) / 256; if (chunks > 64) chunks = 64;   // ci_fold_kernel: the N/2 + 1 index pairs (j, N - j), one per thread and chunk; not rh_stream_grid's four adjacent pairs
  (void)hipGetLastError();
  const int S1 = r->logN - LT;
  if (r->asm_tile && r->asm_cols && r->fuse_ci && S1 >= 2 && S1 <= 4) {
    // the fold rides in the column stages (a thread owns the column pair (c, 4096 - c) the fold couples; column 0 apart): no pass of its own
    hipStream_t st = rh_stream(r);
    const NttTabs t = ntt_tabs(r, limb0);
    const CiFoldTw* cf = reinterpret_cast<const CiFoldTw*>(r->d_cifold + limb0);
    // large batches: the software pipeline of the standard ring's fused launches (spans of ~2048 rows): forward launch j = fold + column stages of
    // span j with the tile stages of span j-1; inverse launch j = tile stages of span j with the column stages + fold of span j-1 (round 3)
    if (const int chunk = rh_span_polys(r, Lrows, npoly); chunk && r->inv_scale) {
      const SpanWalk w(npoly, chunk);
      const size_t stride = (size_t)Lrows * r->N;
      for (int j = 0; j <= w.count(); ++j) {
        const Span s1 = w(j), s2 = w(j - 1);
        const size_t o1 = (size_t)s1.p0 * stride, o2 = (size_t)s2.p0 * stride;
        const unsigned rows1 = (unsigned)s1.polys * Lrows, rows2 = (unsigned)s2.polys * Lrows;
        rh_with_s1<2, 4>(S1, [&](auto S) { rh_with_flag(rh_nt_key(r), [&](auto NT) {
          if (!inverse) {
            const unsigned n1 = rows1 * 8, n2 = rows2 << S1, grid = n1 > n2 ? n1 : n2;
            if (rows1) ci_col0_kernel<S(), false><<<(rows1 + 63) / 64, 64, 0, st>>>(in + o1, out + o1, t.tw_fwd, nullptr, cf, t.c, Lrows, rows1);
            ntt_ci_fwd_fused_asm<S(), NT()><<<grid, 256, 0, st>>>(in + o1, out + o1, n1, out + o2, n2, s2.polys, t.tw_fwd, t.twk_fwd, cf, t.c, Lrows);
          } else {
            const unsigned n1 = rows1 << S1, n2 = rows2 * 8, grid = n1 > n2 ? n1 : n2;
            ntt_ci_inv_fused_asm<S(), NT()><<<grid, 256, 0, st>>>(in + o1, out + o1, n1, s1.polys, out + o2, n2, t.twk_inv, t.tw_inv, t.lastw, cf, t.c, Lrows);
            if (rows2) ci_col0_kernel<S(), true><<<(rows2 + 63) / 64, 64, 0, st>>>(out + o2, out + o2, t.tw_inv, t.lastw, cf, t.c, Lrows, rows2);
          }
        }); });
      }
      return rh_launch_ok("conjugate-invariant transform (pipelined)");
    }
    const NttRows x{inverse ? in : out, out, npoly, Lrows, 0, 0};          // the tile stages: forward in place after the column stages, inverse in -> out before them
    auto cols = [&](auto INV, const u64* src, const tw2* tw, const tw2* lw) {
      rh_with_s1<2, 4>(S1, [&](auto S) {
        ntt_cols_ci_asm<S(), INV()><<<rows * 8, 256, 0, st>>>(src, out, tw, lw, cf, t.c, Lrows);
        ci_col0_kernel<S(), INV()><<<(rows + 63) / 64, 64, 0, st>>>(src, out, tw, lw, cf, t.c, Lrows, rows);
      });
      return rh_launch_ok("ntt_cols_ci_asm");
    };
    if (!inverse) {
      if (int rc = cols(std::false_type{}, in, t.tw_fwd, nullptr)) return rc;
      span_fwd_tile(r, x, limb0, false);
      return rh_launch_ok("ntt");
    }
    span_inv_tile(r, x, limb0);
    if (int rc = rh_launch_ok("ntt")) return rc;
    return cols(std::true_type{}, out, t.tw_inv, t.lastw);
  }
  if (!inverse) {
    ci_fold_kernel<<<dim3(rows, chunks), 256, 0, rh_stream(r)>>>(in, out, r->logN, r->d_cifold + limb0, r->d_consts + limb0, Lrows, 0);
    return rh_std_ntt_launch(r, out, out, npoly, Lrows, limb0, false, false, 0);
  }
  if (int rc = rh_std_ntt_launch(r, in, out, npoly, Lrows, limb0, true, false, 0)) return rc;
  ci_fold_kernel<<<dim3(rows, chunks), 256, 0, rh_stream(r)>>>(out, out, r->logN, r->d_cifold + limb0, r->d_consts + limb0, Lrows, 1);
  return rh_launch_ok("ci_fold_kernel");
}

// canonical transform of limbs [limb0, limb0 + Lrows) of a dense block, for a ring of any type (rescale.hip)
int rh_ring_ntt_any(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse) {
  if (r->kind == RH_RING_3N) {
    std::lock_guard<std::recursive_mutex> lk(r->mu);
    return rh_ring3n_ntt_launch(r, in, out, npoly, Lrows, limb0, inverse, rh_layout3n(r) != 0);
  }
  if (r->kind == RH_RING_CI) return ci_ntt_launch(r, in, out, npoly, Lrows, limb0, inverse);
  return rh_std_ntt_launch(r, in, out, npoly, Lrows, limb0, inverse, false, 0);
}

static int ntt_batch(rh_ring* r, const uint64_t* in, uint64_t* out, int npoly, int level, bool inverse, bool lazy, int phase = 0) {   // phase: rh_ring_ntt_phase's way to rh_std_ntt_launch, nothing else
  if (!r || !in || !out) return rh_fail(RH_ERR_ARG, "ntt: null argument");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "ntt: level %d out of range [0,%d)", level, r->L);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "ntt: npoly < 0");
  (void)hipSetDevice(r->device);
  if (r->kind == RH_RING_3N) {
    std::lock_guard<std::recursive_mutex> lk(r->mu);          // the 3N workspace is shared and grows lazily
    return rh_ring3n_ntt_launch(r, in, out, npoly, level + 1, 0, inverse, rh_layout3n(r) != 0);
  }
  if (r->kind == RH_RING_CI) return ci_ntt_launch(r, in, out, npoly, level + 1, 0, inverse);
  return rh_std_ntt_launch(r, in, out, npoly, level + 1, 0, inverse, lazy, phase);
}
extern "C" int rh_ring_ntt(rh_ring* r, const uint64_t* in, uint64_t* out, int npoly, int level, int lazy) { return ntt_batch(r, in, out, npoly, level, false, lazy != 0); }
extern "C" int rh_ring_intt(rh_ring* r, const uint64_t* in, uint64_t* out, int npoly, int level, int lazy) { return ntt_batch(r, in, out, npoly, level, true, lazy != 0); }
// Ring.NTT on several blocks in one call (device-API extension; e.g. both operands of a product): for two-pass standard rings the
// software pipeline of the fused launches runs through all the blocks; otherwise the blocks are transformed one after the other.
extern "C" int rh_ring_ntt_many(rh_ring* r, const uint64_t* const* in, uint64_t* const* out, const int* npoly, int nblocks, int level) {
  if (!r || !in || !out || !npoly || nblocks < 0) return rh_fail(RH_ERR_ARG, "ntt_many: bad argument");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "ntt_many: level %d out of range [0,%d)", level, r->L);
  long total = 0;
  for (int k = 0; k < nblocks; ++k) {
    if (!in[k] || !out[k] || npoly[k] < 0) return rh_fail(RH_ERR_ARG, "ntt_many: block %d: null pointer or npoly < 0", k);
    total += npoly[k];
  }
  (void)hipSetDevice(r->device);
  const int Lrows = level + 1;
  const int chunk = rh_span_polys(r, Lrows, total);          // (the blocks' polys together: the pipeline runs through the block boundaries)
  if (r->kind == RH_RING_STANDARD && r->logN > LT && !one_pass_ok(r) && chunk) {
    std::vector<NttSeg> segs;
    for (int k = 0; k < nblocks; ++k) if (npoly[k] > 0) segs.push_back(NttSeg{in[k], out[k], npoly[k]});
    return std_ntt_fwd_pipelined_segs(r, segs.data(), (int)segs.size(), Lrows, 0, chunk);
  }
  for (int k = 0; k < nblocks; ++k)
    if (int rc = ntt_batch(r, in[k], out[k], npoly[k], level, false, false)) return rc;
  return RH_OK;
}
// ---- views at a lower level of blocks allocated with MORE limbs per poly (ring.AtLevel(level) on max-level polys and buffers,
// ring/ring.go:192-213: the idiomatic use inside the reference's evaluators).  Forward transforms with one row stride on both sides
// (N >= 4096) and inverse transforms through the hand-scheduled bodies (N = 2^14 .. 2^16) are batched (row strides inside the
// kernels); the remaining shapes run poly by poly (correct, not the throughput path).
static int ntt_rows(rh_ring* r, const uint64_t* in, int in_rows, uint64_t* out, int out_rows, int npoly, int level, bool inverse, bool lazy) {
  if (!r) return rh_fail(RH_ERR_ARG, "ntt: null argument");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "ntt: level %d out of range [0,%d)", level, r->L);
  if (in_rows < level + 1 || out_rows < level + 1) return rh_fail(RH_ERR_ARG, "ntt: blocks with %d / %d limbs per poly used at level %d", in_rows, out_rows, level);
  if (in_rows == level + 1 && out_rows == level + 1) return ntt_batch(r, in, out, npoly, level, inverse, lazy);
  if (!in || !out) return rh_fail(RH_ERR_ARG, "ntt: null argument");
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "ntt: npoly < 0");
  (void)hipSetDevice(r->device);
  // standard rings: the row strides of the two blocks go into the kernels (every N, forward and inverse, exact-lazy forward included); the one
  // exception is the non-canonical BackwardLazy of N = 8, which compacts like the other ring types
  if (r->kind == RH_RING_STANDARD && !(inverse && lazy && r->logN < 4)) {
    ++r->stats_rows_direct;
    return std_ntt_launch_span(r, in, out, npoly, level + 1, 0, inverse, lazy, in_rows, out_rows);
  }
  // conjugate-invariant and 3N rings: still ONE batched transform -- the leading limbs are compacted with a strided copy on the way in and / or
  // expanded on the way out (round 3; these shapes ran poly by poly before)
  if (npoly == 0) return RH_OK;
  ++r->stats_rows_compacted;
  const size_t N = (size_t)r->N, Lr = (size_t)(level + 1);
  hipStream_t st = rh_stream(r);
  auto copy2d = [&](u64* dst, size_t drows, const u64* src, size_t srows) {
    return hipMemcpy2DAsync(dst, drows * N * 8, src, srows * N * 8, Lr * N * 8, (size_t)npoly, hipMemcpyDeviceToDevice, st) == hipSuccess
               ? RH_OK : rh_fail(RH_ERR_DEVICE, "ntt: strided copy of the leading limbs failed");
  };
  if ((size_t)out_rows == Lr) {                       // dense destination: gather into it, transform in place
    if (int rc = copy2d(out, Lr, in, (size_t)in_rows)) return rc;
    return ntt_batch(r, out, out, npoly, level, inverse, lazy);
  }
  std::lock_guard<std::recursive_mutex> lk(r->mu);   // the dense scratch is shared and grows lazily; its use is stream-ordered
  const size_t words = (size_t)npoly * Lr * N;
  if (r->rows_words < words) {
    if (r->d_rows) (void)hipFree(r->d_rows);
    r->d_rows = nullptr; r->rows_words = 0;
    if (hipMalloc((void**)&r->d_rows, words * 8) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(AtLevel scratch, %zu words) failed", words);
    r->rows_words = words;
  }
  const u64* src = in;
  if ((size_t)in_rows != Lr) { if (int rc = copy2d(r->d_rows, Lr, in, (size_t)in_rows)) return rc; src = r->d_rows; }
  if (int rc = ntt_batch(r, src, r->d_rows, npoly, level, inverse, lazy)) return rc;
  return copy2d(out, (size_t)out_rows, r->d_rows, Lr);
}
extern "C" int rh_ring_stats(const rh_ring* r, const char* key, long* value) {
  if (!r || !key || !value) return rh_fail(RH_ERR_ARG, "rh_ring_stats: null argument");
  if (!strcmp(key, "rows_direct")) { *value = r->stats_rows_direct; return RH_OK; }
  if (!strcmp(key, "rows_compacted")) { *value = r->stats_rows_compacted; return RH_OK; }
  if (!strcmp(key, "rows_poly_by_poly")) { *value = 0; return RH_OK; }   // no entry point loops over polys any more (kept so a regression has a name)
  return rh_fail(RH_ERR_ARG, "rh_ring_stats: unknown key %s", key);
}
extern "C" int rh_ring_ntt_rows(rh_ring* r, const uint64_t* in, int in_rows, uint64_t* out, int out_rows, int npoly, int level, int lazy) {
  return ntt_rows(r, in, in_rows, out, out_rows, npoly, level, false, lazy != 0);
}
extern "C" int rh_ring_intt_rows(rh_ring* r, const uint64_t* in, int in_rows, uint64_t* out, int out_rows, int npoly, int level, int lazy) {
  return ntt_rows(r, in, in_rows, out, out_rows, npoly, level, true, lazy != 0);
}
// Explicit-layout forms for 3N rings (hosts that TAG their device polys with the NTT-domain layout instead of switching the whole handle with
// the tuning key): block_order 1 = the NTT side of this call is in block order, 0 = the reference's ascending-totative order.  The layout is a
// per-call argument (thread-local inside the call), so concurrent callers of one handle may use different layouts.  Other ring kinds: ignored.
extern "C" int rh_ring_ntt3n_block_order_supported(const rh_ring* r) {
  return r && r->kind == RH_RING_3N && rh_ring3n_block_order_ok(r) ? 1 : 0;
}
extern "C" int rh_ring_ntt_layout(rh_ring* r, const uint64_t* in, int in_rows, uint64_t* out, int out_rows, int npoly, int level, int inverse, int block_order) {
  if (!r) return rh_fail(RH_ERR_ARG, "ntt: null argument");
  if (block_order && !rh_ring_ntt3n_block_order_supported(r)) return rh_fail(RH_ERR_UNSUPPORTED, "block order needs a 3N ring with N = 3 * 2^k, k >= 13");
  RhLayoutScope ls(r->kind == RH_RING_3N ? (block_order ? 1 : 0) : -1);
  return ntt_rows(r, in, in_rows, out, out_rows, npoly, level, inverse != 0, false);
}
extern "C" int rh_ring_ntt_phase(rh_ring* r, const uint64_t* in, uint64_t* out, int npoly, int level, int inverse, int phase) {
  if (phase < 0 || phase > 2) return rh_fail(RH_ERR_ARG, "phase must be 0, 1 or 2");
  return ntt_batch(r, in, out, npoly, level, inverse != 0, false, phase);
}

// INTT(a . b) for NTT-domain blocks a, b (canonical or lazy < 2q): the values ring.MForm(a) -> ring.MulCoeffsMontgomery(., b) ->
// ring.INTT produce (schemes/ckks/evaluator.go:821-834 + :INTT; BASELINE config 3), with the product formed on load by the inverse
// tile kernel (MRedLazy) and the factor 2^64 restored by the N^-1 constants of the last inverse stage.  Outputs are canonical
// residues of a*b*N^-1-transform, hence bit-identical to the three-call sequence.  out may alias a or b.
static int std_intt_mul_launch(rh_ring* r, const u64* a, const u64* b, u64* out, int npoly, int Lrows) {
  const int logN = r->logN;
  const unsigned rows = (unsigned)npoly * (unsigned)Lrows;
  if (rows == 0) return RH_OK;
  hipStream_t st = rh_stream(r);
  if (logN < LT) {                                   // small rings: the three calls as they are (not a throughput path)
    if (int rc = rh_vec_launch(r, RH_OP_MFORM, a, nullptr, out, npoly, Lrows, 0, nullptr, nullptr)) return rc;
    if (int rc = rh_vec_launch(r, RH_OP_MUL_MONT, out, b, out, npoly, Lrows, 0, nullptr, nullptr)) return rc;
    return rh_std_ntt_launch(r, out, out, npoly, Lrows, 0, true, false, 0);
  }
  (void)hipGetLastError();
  const int S1 = logN - LT;
  if (S1 > 0 && r->asm_tile) {
    // large batches: the software pipeline of std_ntt_inv_pipelined (tile stages of span j with the column stages of span j-1).
    // The output may alias an input: a span's tiles read (a, b) of that span only, before its column stages write them.
    if (const int chunk = rh_span_polys(r, Lrows, npoly)) return std_ntt_inv_pipelined(r, a, out, npoly, Lrows, 0, chunk, b);
    ntt_inv_tile_mul_asm<<<rows << S1, 256, 0, st>>>(a, b, out, r->d_twk_inv, r->d_consts_r, Lrows, logN, npoly);
  } else
  ntt_inv_tile_mul<<<rows << S1, 256, 0, st>>>(a, b, out, r->d_twk_inv, r->d_consts_r, Lrows, logN, logN == LT ? 1 : 0, npoly);
  launch_inv_cols(ntt_tabs(r, 0, true), st, logN, NttRows{out, out, npoly, Lrows, 0, 0}, r->asm_cols && r->asm_tile ? BODY_ASM : BODY_CPP, RH_NT_NEVER, 1);
  return rh_launch_ok("intt_mul");
}
extern "C" int rh_ring_intt_mul(rh_ring* r, const uint64_t* a, const uint64_t* b, uint64_t* out, int npoly, int level) {
  if (!r || !a || !b || !out) return rh_fail(RH_ERR_ARG, "intt_mul: null argument");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "intt_mul: level %d out of range [0,%d)", level, r->L);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "intt_mul: npoly < 0");
  (void)hipSetDevice(r->device);
  if (r->kind != RH_RING_STANDARD) {                 // 3N / conjugate-invariant rings: the three calls as they are, through the ring's own transform
    if (int rc = rh_vec_launch(r, RH_OP_MFORM, a, nullptr, out, npoly, level + 1, 0, nullptr, nullptr)) return rc;
    if (int rc = rh_vec_launch(r, RH_OP_MUL_MONT, out, b, out, npoly, level + 1, 0, nullptr, nullptr)) return rc;
    return rh_ring_ntt_any(r, out, out, npoly, level + 1, 0, true);
  }
  return std_intt_mul_launch(r, a, b, out, npoly, level + 1);
}

// c = INTT(NTT(a) . NTT(b)) with a and b given in the COEFFICIENT domain (BASELINE config 3: ring.NTT(a), ring.NTT(b), ring.MForm,
// ring.MulCoeffsMontgomery, ring.INTT -- schemes/ckks/evaluator.go:821-834 around a fresh product): forward column stages of a and of b in
// place, then ONE kernel for the forward tile stages of both, their product and the inverse tile stages (ntt_polymul_tile_asm), then the inverse
// column stages.  Same canonical values as the five ring calls; a and b are CONSUMED (they hold their column-stage intermediates afterwards,
// not NTT(a) / NTT(b)); out may alias either.  Standard rings, 2^13 <= N <= 2^17, hand-scheduled tile bodies; other shapes: RH_ERR_UNSUPPORTED
// (the caller falls back to rh_ring_ntt_many + rh_ring_intt_mul).
extern "C" int rh_ring_polymul(rh_ring* r, uint64_t* a, uint64_t* b, uint64_t* out, int npoly, int level) {
  if (!r || !a || !b || !out) return rh_fail(RH_ERR_ARG, "polymul: null argument");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "polymul: level %d out of range [0,%d)", level, r->L);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "polymul: npoly < 0");
  if (a == b) return rh_fail(RH_ERR_ARG, "polymul: a and b must be different blocks (both are transformed in place)");
  const int S1 = r->logN - LT;
  if (r->kind != RH_RING_STANDARD || S1 < 1 || S1 > 5 || !r->asm_tile) return rh_fail(RH_ERR_UNSUPPORTED, "polymul: standard rings with 2^13 <= N <= 2^17 and the hand-scheduled tile bodies");
  const int Lrows = level + 1;
  const unsigned rows = (unsigned)npoly * (unsigned)Lrows;
  if (rows == 0) return RH_OK;
  (void)hipSetDevice(r->device);
  hipStream_t st = rh_stream(r);
  const NttTabs t = ntt_tabs(r, 0, true);
  (void)hipGetLastError();
  if (const int chunk = rh_span_polys(r, Lrows, npoly)) {
    // large batches: ONE stream of launches, launch j = column stages of span j + tile middle of span j-1 + inverse column stages of span j-2
    const SpanWalk w(npoly, chunk);
    const size_t stride = (size_t)Lrows * r->N;
    for (int j = 0; j < w.count() + 2; ++j) {
      const Span s1 = w(j), s2 = w(j - 1), s3 = w(j - 2);
      const size_t o1 = (size_t)s1.p0 * stride, o2 = (size_t)s2.p0 * stride, o3 = (size_t)s3.p0 * stride;
      const unsigned n1 = (unsigned)s1.polys * Lrows * 16, n2 = ((unsigned)s2.polys * Lrows) << S1, n3 = (unsigned)s3.polys * Lrows * 16;
      const unsigned grid = n1 > n2 ? (n1 > n3 ? n1 : n3) : (n2 > n3 ? n2 : n3);
      if (!grid) continue;
      rh_with_s1<1, 5>(S1, [&](auto S) { rh_with_flag(rh_nt_key(r), [&](auto NT) {     // (three blocks of >= 2048 rows)
        ntt_polymul_fused_asm<S(), NT()><<<grid, 256, 0, st>>>(a + o1, b + o1, n1, a + o2, b + o2, out + o2, n2, s2.polys, out + o3, n3, t.tw_fwd, t.twk_fwd,
                                                               t.twk_inv, t.tw_inv, t.lastw, t.c, Lrows, r->logN); }); });
    }
    return rh_launch_ok("polymul (pipelined)");
  }
  for (u64* p : {a, b}) {                               // forward column stages, in place
    span_fwd_cols(r, NttRows{p, p, npoly, Lrows, 0, 0}, 0, false);
    if (int rc = rh_launch_ok("ntt")) return rc;
  }
  const bool nt = rh_nt_rows(r, rows);
  rh_with_flag(nt, [&](auto NT) { ntt_polymul_tile_asm<NT()><<<rows << S1, 256, 0, st>>>(a, b, out, t.twk_fwd, t.twk_inv, t.c, Lrows, r->logN, npoly); });
  launch_inv_cols(t, st, r->logN, NttRows{out, out, npoly, Lrows, 0, 0}, r->asm_cols ? BODY_ASM : BODY_CPP, nt, 1);
  return rh_launch_ok("polymul");
}

extern "C" int rh_ring_ntt3n_reorder(rh_ring* r, const uint64_t* in, uint64_t* out, int npoly, int level, int to_reference) {
  if (!r || !in || !out) return rh_fail(RH_ERR_ARG, "ntt3n_reorder: null argument");
  if (r->kind != RH_RING_3N) return rh_fail(RH_ERR_ARG, "ntt3n_reorder: not a 3N ring");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "ntt3n_reorder: level %d out of range [0,%d)", level, r->L);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "ntt3n_reorder: npoly < 0");
  (void)hipSetDevice(r->device);
  return rh_ring3n_reorder_launch(r, in, out, npoly, level + 1, to_reference != 0);
}

// Pre-sizes every lazily grown scratch of the ring for batches of up to npoly polys (all limbs): afterwards no entry point of
// the ring allocates.  Optional: without it scratch grows on first use.
extern "C" int rh_ring_reserve(rh_ring* r, int npoly) {
  if (!r || npoly < 0) return rh_fail(RH_ERR_ARG, "rh_ring_reserve: bad argument");
  (void)hipSetDevice(r->device);
  std::lock_guard<std::recursive_mutex> lk(r->mu);
  if (r->kind == RH_RING_3N) if (int rc = rh_ring3n_reserve(r, npoly)) return rc;
  const size_t words = (size_t)npoly * r->L * r->N;            // the rows-per-poly transforms' dense scratch
  if (r->rows_words < words) {
    if (r->d_rows) (void)hipFree(r->d_rows);
    r->d_rows = nullptr; r->rows_words = 0;
    if (hipMalloc((void**)&r->d_rows, (words ? words : 1) * 8) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(AtLevel scratch) failed");
    r->rows_words = words;
  }
  return rh_rescale_reserve(r, npoly);
}

extern "C" int rh_ring_set_tuning(rh_ring* r, const char* key, long value) {
  if (!r || !key) return rh_fail(RH_ERR_ARG, "set_tuning: null argument");
  if (!strcmp(key, "chunk_polys")) { r->chunk_polys = (int)value; return RH_OK; }
  if (!strcmp(key, "asm_tile")) { r->asm_tile = value != 0; return RH_OK; }
  if (!strcmp(key, "auto_span_rows")) { if (value < 1) return rh_fail(RH_ERR_ARG, "auto_span_rows must be >= 1"); r->auto_span_rows = (int)value; return RH_OK; }
  if (!strcmp(key, "fuse_submul")) { r->fuse_submul = (int)value; return RH_OK; }
  if (!strcmp(key, "digit_pipeline")) { r->digit_pipeline = (int)value; return RH_OK; }
  if (!strcmp(key, "fuse_ci")) { r->fuse_ci = (int)value; return RH_OK; }
  if (!strcmp(key, "perm_inv_shape")) { r->perm_inv_shape = (int)value; return RH_OK; }
  if (!strcmp(key, "perm_fwd_shape")) { r->perm_fwd_shape = (int)value; return RH_OK; }
  if (!strcmp(key, "fuse3n")) { r->fuse3n = (int)value; return RH_OK; }
  if (!strcmp(key, "ntt3n_block_order")) {
    if (r->kind != RH_RING_3N) return rh_fail(RH_ERR_ARG, "ntt3n_block_order: not a 3N ring");
    r->block_order3n = value != 0;
    return RH_OK;
  }
  if (!strcmp(key, "asm_cols")) { r->asm_cols = (int)value; return RH_OK; }
  if (!strcmp(key, "ks_small_rows")) { if (value < 0) return rh_fail(RH_ERR_ARG, "ks_small_rows must be >= 0"); r->ks_small_rows = (int)value; return RH_OK; }
  if (!strcmp(key, "pair_submul")) { r->pair_submul = value != 0; return RH_OK; }
  if (!strcmp(key, "one_pass")) { r->one_pass = value != 0; return RH_OK; }
  if (!strcmp(key, "nt_streams")) {     // 0: default cache policy everywhere (A/B runs: bench.py --tune nt_streams=0), 1: by working set, 2: non-temporal at every size
    if (value < 0 || value > 2) return rh_fail(RH_ERR_ARG, "nt_streams must be 0, 1 or 2 (got %ld)", value);
    r->nt_streams = (int)value; if (r->kind == RH_RING_3N) rh_ring3n_set_nt_streams(r, (int)value); return RH_OK;
  }
  return rh_fail(RH_ERR_ARG, "set_tuning: unknown key %s", key);
}

// ---- one limb, host pointers: the NumberTheoreticTransformer interface -----------------------------------------------
// Every call takes a (stream, scratch) slot of its own from the ring's pool, so any number of OS threads may call
// Forward / Backward on one handle at once (ring/ring.go:192-194; goroutines migrate between threads).  A slot is created
// the first time a caller finds the pool empty; steady state allocates nothing.
static int slot_acquire(rh_ring* r, RhHostSlot** out) {
  {
    std::lock_guard<std::mutex> lk(r->slot_mu);
    if (!r->free_slots.empty()) { *out = r->free_slots.back(); r->free_slots.pop_back(); return RH_OK; }
  }
  RhHostSlot* sl = new (std::nothrow) RhHostSlot();
  if (!sl) return rh_fail(RH_ERR_NOMEM, "out of host memory");
  sl->words = (size_t)r->N * (r->kind == RH_RING_3N ? 2 : 1);                    // the limb + the 3N transform's workspace for one row
  if (hipStreamCreateWithFlags(&sl->stream, hipStreamNonBlocking) != hipSuccess) { delete sl; return rh_fail(RH_ERR_DEVICE, "hipStreamCreate failed"); }
  if (hipMalloc((void**)&sl->buf, sl->words * 8) != hipSuccess) { (void)hipStreamDestroy(sl->stream); delete sl; return rh_fail(RH_ERR_NOMEM, "hipMalloc(host-limb scratch) failed"); }
  std::lock_guard<std::mutex> lk(r->slot_mu);
  r->all_slots.push_back(sl);
  *out = sl;
  return RH_OK;
}
static void slot_release(rh_ring* r, RhHostSlot* sl) {
  std::lock_guard<std::mutex> lk(r->slot_mu);
  r->free_slots.push_back(sl);
}
static int ntt_host_limb(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2, bool inverse, bool lazy) {
  if (!r) return rh_fail(RH_ERR_ARG, "null ring");
  if (!p1 || !p2) return rh_fail(RH_ERR_ARG, "cannot NTT: nil slice (len(p1), len(p2) must be >= N=%d)", r->N);
  if (limb < 0 || limb >= r->L) return rh_fail(RH_ERR_ARG, "limb %d out of range [0,%d)", limb, r->L);
  (void)hipSetDevice(r->device);
  RhHostSlot* sl;
  if (int rc = slot_acquire(r, &sl)) return rc;
  int rc = RH_OK;
  {
    RhCallScope scope(sl->stream, r->kind == RH_RING_3N ? sl->buf + r->N : nullptr, (size_t)r->N);
    const size_t bytes = (size_t)r->N * 8;
    hipError_t e = hipMemcpyAsync(sl->buf, p1, bytes, hipMemcpyHostToDevice, sl->stream);
    if (e != hipSuccess) rc = rh_fail(RH_ERR_DEVICE, "H2D: %s", hipGetErrorString(e));
    if (!rc) rc = (r->kind == RH_RING_3N) ? rh_ring3n_ntt_launch(r, sl->buf, sl->buf, 1, 1, limb, inverse)
                : (r->kind == RH_RING_CI) ? ci_ntt_launch(r, sl->buf, sl->buf, 1, 1, limb, inverse)
                                          : rh_std_ntt_launch(r, sl->buf, sl->buf, 1, 1, limb, inverse, lazy, 0);
    if (!rc) {
      e = hipMemcpyAsync(p2, sl->buf, bytes, hipMemcpyDeviceToHost, sl->stream);
      if (e == hipSuccess) e = hipStreamSynchronize(sl->stream);
      if (e != hipSuccess) rc = rh_fail(RH_ERR_DEVICE, "D2H: %s", hipGetErrorString(e));
    } else (void)hipStreamSynchronize(sl->stream);
  }
  slot_release(r, sl);
  return rc;
}
extern "C" int rh_ntt_forward(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2) { return ntt_host_limb(r, limb, p1, p2, false, false); }
extern "C" int rh_ntt_forward_lazy(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2) { return ntt_host_limb(r, limb, p1, p2, false, true); }
extern "C" int rh_ntt_backward(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2) { return ntt_host_limb(r, limb, p1, p2, true, false); }
extern "C" int rh_ntt_backward_lazy(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2) { return ntt_host_limb(r, limb, p1, p2, true, true); }

// ---- a whole Poly, host pointers: Ring.NTT / NTTLazy / INTT / INTTLazy (ring/ntt.go:127-152) as ONE call -------------------------------
// The reference loops `for i, s := range r.SubRings[:r.level+1] { s.NTT(p1.Coeffs[i], p2.Coeffs[i]) }` over Poly.Coeffs [][]uint64
// (ring/poly.go:13-24); through rh_ntt_forward that is level+1 synchronous H2D -> kernel -> D2H -> synchronise round trips.  Here the
// level+1 limb pointers arrive together: the limbs are cut into up to four groups that alternate between two streams, so group g's
// upload runs under group g-1's transform and download (PCIe is full duplex), every group is ONE batched launch pair over its limbs, and
// the host synchronises once.  Page-locked limbs (rh_host_alloc / rh_host_register) are DMA'd where they lie; pageable limbs are staged
// through the slot's page-locked buffers (the CPU copy of group g overlaps the DMA of group g-1).
struct RhPolySlot {
  hipStream_t st[2] = {nullptr, nullptr};
  hipEvent_t done[4] = {nullptr, nullptr, nullptr, nullptr};
  u64* dbuf = nullptr; size_t dwords = 0;                 // device: the limbs (+ the 3N transform's workspace)
  u64* hin = nullptr; u64* hout = nullptr; size_t hwords = 0;   // page-locked staging, allocated when a pageable limb is first seen
};
static void poly_slot_free(RhPolySlot* sl) {
  if (sl->dbuf) (void)hipFree(sl->dbuf);
  if (sl->hin) (void)hipHostFree(sl->hin);
  if (sl->hout) (void)hipHostFree(sl->hout);
  for (hipStream_t s : sl->st) if (s) (void)hipStreamDestroy(s);
  for (hipEvent_t e : sl->done) if (e) (void)hipEventDestroy(e);
  delete sl;
}
void rh_poly_slots_teardown(rh_ring* r) { for (RhPolySlot* sl : r->all_poly_slots) poly_slot_free(sl); r->all_poly_slots.clear(); r->free_poly_slots.clear(); }
static int poly_slot_acquire(rh_ring* r, RhPolySlot** out) {
  {
    std::lock_guard<std::mutex> lk(r->slot_mu);
    if (!r->free_poly_slots.empty()) { *out = r->free_poly_slots.back(); r->free_poly_slots.pop_back(); return RH_OK; }
  }
  RhPolySlot* sl = new (std::nothrow) RhPolySlot();
  if (!sl) return rh_fail(RH_ERR_NOMEM, "out of host memory");
  sl->dwords = (size_t)r->N * r->L * (r->kind == RH_RING_3N ? 2 : 1);
  bool ok = hipMalloc((void**)&sl->dbuf, sl->dwords * 8) == hipSuccess;
  for (int k = 0; k < 2 && ok; ++k) ok = hipStreamCreateWithFlags(&sl->st[k], hipStreamNonBlocking) == hipSuccess;
  for (int k = 0; k < 4 && ok; ++k) ok = hipEventCreateWithFlags(&sl->done[k], hipEventDisableTiming) == hipSuccess;
  if (!ok) { poly_slot_free(sl); return rh_fail(RH_ERR_NOMEM, "whole-poly host path: device buffer / stream / event creation failed"); }
  std::lock_guard<std::mutex> lk(r->slot_mu);
  r->all_poly_slots.push_back(sl);
  *out = sl;
  return RH_OK;
}
static void poly_slot_release(rh_ring* r, RhPolySlot* sl) { std::lock_guard<std::mutex> lk(r->slot_mu); r->free_poly_slots.push_back(sl); }
// 1: page-locked host memory (DMA'd where it lies), 0: ordinary pageable memory (staged), -1: device memory (a caller's mistake: this is the HOST entry)
static int host_ptr_kind(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return 0; }   // an ordinary (pageable) pointer is "invalid value" to the runtime
  if (a.type == hipMemoryTypeHost) return 1;
  return (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) ? -1 : 0;
}
static int ntt_host_poly(rh_ring* r, int level, const uint64_t* const* p1, uint64_t* const* p2, bool inverse, bool lazy) {
  if (!r) return rh_fail(RH_ERR_ARG, "null ring");
  if (!p1 || !p2) return rh_fail(RH_ERR_ARG, "cannot NTT: nil Poly.Coeffs");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "ntt: level %d out of range [0,%d)", level, r->L);
  const int Lr = level + 1, N = r->N;
  for (int i = 0; i < Lr; ++i) if (!p1[i] || !p2[i]) return rh_fail(RH_ERR_ARG, "cannot NTT: nil slice at limb %d (len(p1[i]), len(p2[i]) must be >= N=%d)", i, N);
  (void)hipSetDevice(r->device);
  RhPolySlot* sl;
  if (int rc = poly_slot_acquire(r, &sl)) return rc;
  const size_t bytes = (size_t)N * 8;
  bool pin_in[RH_MAX_LIMBS], pin_out[RH_MAX_LIMBS], staged = false;
  int rc = RH_OK;
  for (int i = 0; i < Lr; ++i) {
    const int ki = host_ptr_kind(p1[i]), ko = host_ptr_kind(p2[i]);
    if (ki < 0 || ko < 0) { rc = rh_fail(RH_ERR_ARG, "cannot NTT: limb %d is a device pointer; device-resident polys go through rh_ring_ntt / rh_ring_intt", i); break; }
    pin_in[i] = ki == 1; pin_out[i] = ko == 1; staged |= !pin_in[i] || !pin_out[i];
  }
  if (rc) { poly_slot_release(r, sl); return rc; }
  if (staged && !sl->hin) {
    sl->hwords = (size_t)N * r->L;
    if (hipHostMalloc((void**)&sl->hin, sl->hwords * 8, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void**)&sl->hout, sl->hwords * 8, hipHostMallocDefault) != hipSuccess) {
      if (sl->hin) { (void)hipHostFree(sl->hin); sl->hin = nullptr; }
      rc = rh_fail(RH_ERR_NOMEM, "hipHostMalloc(page-locked staging) failed");
    }
  }
  // groups: enough bytes per group to amortise a launch pair (>= 256 KiB), at most 4
  int G = (int)(((size_t)Lr * bytes) / ((size_t)256 << 10)); if (G > 4) G = 4; if (G > Lr) G = Lr; if (G < 1) G = 1;
  // the host side of every limb: the caller's slice when it is page-locked, else its place in the staging blocks.  Limbs that are adjacent in
  // host memory move as ONE copy (a copy costs ~10 us to issue and start whatever its size): always the case for staged limbs, and for a
  // Poly whose limbs were carved from one page-locked allocation
  const u64* hsrc[RH_MAX_LIMBS]; u64* hdst[RH_MAX_LIMBS];
  for (int i = 0; i < Lr; ++i) { hsrc[i] = pin_in[i] ? p1[i] : sl->hin + (size_t)i * N; hdst[i] = pin_out[i] ? p2[i] : sl->hout + (size_t)i * N; }
  for (int g = 0; g < G && !rc; ++g) {
    const int g0 = (int)((long)Lr * g / G), g1 = (int)((long)Lr * (g + 1) / G);
    hipStream_t st = sl->st[g & 1];
    hipError_t e = hipSuccess;
    for (int i = g0; i < g1; ++i) if (!pin_in[i]) memcpy(sl->hin + (size_t)i * N, p1[i], bytes);
    for (int i = g0, j; i < g1 && e == hipSuccess; i = j) {
      for (j = i + 1; j < g1 && hsrc[j] == hsrc[j - 1] + N; ++j) {}
      e = hipMemcpyAsync(sl->dbuf + (size_t)i * N, hsrc[i], (size_t)(j - i) * bytes, hipMemcpyHostToDevice, st);
    }
    if (e != hipSuccess) { rc = rh_fail(RH_ERR_DEVICE, "H2D: %s", hipGetErrorString(e)); break; }
    {
      u64* d = sl->dbuf + (size_t)g0 * N;
      RhCallScope scope(st, r->kind == RH_RING_3N ? sl->dbuf + (size_t)(r->L + g0) * N : nullptr, (size_t)(g1 - g0) * N);
      rc = (r->kind == RH_RING_3N) ? rh_ring3n_ntt_launch(r, d, d, 1, g1 - g0, g0, inverse)
         : (r->kind == RH_RING_CI) ? ci_ntt_launch(r, d, d, 1, g1 - g0, g0, inverse)
                                   : rh_std_ntt_launch(r, d, d, 1, g1 - g0, g0, inverse, lazy, 0);
    }
    for (int i = g0, j; i < g1 && !rc; i = j) {
      for (j = i + 1; j < g1 && hdst[j] == hdst[j - 1] + N; ++j) {}
      e = hipMemcpyAsync(hdst[i], sl->dbuf + (size_t)i * N, (size_t)(j - i) * bytes, hipMemcpyDeviceToHost, st);
      if (e != hipSuccess) rc = rh_fail(RH_ERR_DEVICE, "D2H: %s", hipGetErrorString(e));
    }
    if (!rc && hipEventRecord(sl->done[g], st) != hipSuccess) rc = rh_fail(RH_ERR_DEVICE, "hipEventRecord failed");
  }
  if (rc) { (void)hipStreamSynchronize(sl->st[0]); (void)hipStreamSynchronize(sl->st[1]); poly_slot_release(r, sl); return rc; }
  for (int g = 0; g < G; ++g) {                         // staged outputs leave as soon as their group has landed
    const int g0 = (int)((long)Lr * g / G), g1 = (int)((long)Lr * (g + 1) / G);
    hipError_t e = hipEventSynchronize(sl->done[g]);
    if (e != hipSuccess) { rc = rh_fail(RH_ERR_DEVICE, "whole-poly host path: %s", hipGetErrorString(e)); (void)hipStreamSynchronize(sl->st[0]); (void)hipStreamSynchronize(sl->st[1]); break; }
    for (int i = g0; i < g1; ++i) if (!pin_out[i]) memcpy(p2[i], sl->hout + (size_t)i * N, bytes);
  }
  poly_slot_release(r, sl);
  return rc;
}
extern "C" int rh_ntt_poly_forward(rh_ring* r, int level, const uint64_t* const* p1, uint64_t* const* p2, int lazy) { return ntt_host_poly(r, level, p1, p2, false, lazy != 0); }
extern "C" int rh_ntt_poly_backward(rh_ring* r, int level, const uint64_t* const* p1, uint64_t* const* p2, int lazy) { return ntt_host_poly(r, level, p1, p2, true, lazy != 0); }
// page-locked host memory for Poly.Coeffs backing arrays: limbs that live here are DMA'd directly by rh_ntt_* / rh_ntt_poly_*
extern "C" int rh_host_alloc(size_t words, uint64_t** hptr) {
  if (!hptr) return rh_fail(RH_ERR_ARG, "rh_host_alloc: null argument");
  if (hipHostMalloc((void**)hptr, (words ? words : 1) * 8, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return rh_fail(RH_ERR_NOMEM, "hipHostMalloc(%zu words) failed", words); }
  return RH_OK;
}
extern "C" int rh_host_free(uint64_t* hptr) { if (hptr) (void)hipHostFree(hptr); return RH_OK; }
extern "C" int rh_host_register(uint64_t* hptr, size_t words) {
  if (!hptr || !words) return rh_fail(RH_ERR_ARG, "rh_host_register: null argument");
  // whole pages only: the runtime pins and GPU-maps every page the range touches, and a page shared with unrelated heap objects would be dragged along
  if (((uintptr_t)hptr & 4095u) || ((words * 8) & 4095u)) return rh_fail(RH_ERR_ARG, "rh_host_register: register whole 4 KiB pages (pointer %p, %zu bytes)", (void*)hptr, words * 8);
  hipError_t e = hipHostRegister(hptr, words * 8, hipHostRegisterDefault);
  if (e != hipSuccess) { (void)hipGetLastError(); return rh_fail(RH_ERR_DEVICE, "hipHostRegister: %s", hipGetErrorString(e)); }
  return RH_OK;
}
extern "C" int rh_host_unregister(uint64_t* hptr) {
  if (!hptr) return RH_OK;
  hipError_t e = hipHostUnregister(hptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return rh_fail(RH_ERR_DEVICE, "hipHostUnregister: %s", hipGetErrorString(e)); }
  return RH_OK;
}

// ------------------------------------------------------------------------------------------------ element-wise
struct ScalarPack { u64 s[RH_MAX_LIMBS]; };

struct RowStrides { int r1, r2, r3; unsigned pair0, pair1; int nt; };   // nt: non-temporal loads / stores (operands beyond the Infinity Cache; a broadcast row stays cached)   // limbs per poly of the three operand blocks (>= L: ring.AtLevel views; r2 < 0: p2 is ONE
                                                                 // row used for every (poly, limb)); the range of coefficient pairs processed
template <int OP>
__global__ void __launch_bounds__(256)
vec_op_packed(const u64* p1, const u64* p2, u64* p3, unsigned n, ScalarPack s0, ScalarPack s1,
              const LimbConsts* __restrict__ consts, int L, RowStrides rs) {
  const StreamRow row(consts, L, n);
  const LimbConsts& c = row.c;
  const u64 a0 = s0.s[row.limb], a1 = s1.s[row.limb];
  const size_t o1 = row.at(rs.r1, n), o2 = rs.r2 < 0 ? 0 : row.at(rs.r2, n), o3 = row.at(rs.r3, n);
  RH_FOR_EACH_PAIR(i, rs.pair0, rs.pair1) {
    const size_t e = 2 * (size_t)i;
    ulonglong2 x = make_ulonglong2(0, 0), y = x, z = x;
    if (op_reads_x(OP)) x = rh_ld2(p1 + o1 + e, rs.nt);
    if (op_reads_y(OP)) y = rh_ld2(p2 + o2 + e, rs.nt && rs.r2 >= 0);       // a broadcast row is re-read by every workgroup: default policy
    if (op_reads_z(OP)) z = rh_ld2(p3 + o3 + e, rs.nt);
    ulonglong2 w;
    w.x = vec_apply<OP>(x.x, y.x, z.x, a0, a1, c);
    w.y = vec_apply<OP>(x.y, y.y, z.y, a0, a1, c);
    rh_st2(p3 + o3 + e, w, rs.nt);
  }
}

typedef void (*vec_fn)(const u64*, const u64*, u64*, unsigned, ScalarPack, ScalarPack, const LimbConsts*, int, RowStrides);
template <int... I>
static const vec_fn* vec_table(std::integer_sequence<int, I...>) {
  static const vec_fn t[] = {vec_op_packed<I>...};
  return t;
}

int rh_vec_launch(rh_ring* r, int opcode, const u64* p1, const u64* p2, u64* p3, int npoly, int Lrows, int limb0,
                  const u64* s0, const u64* s1, int rows1, int rows2, int rows3, int half) {   // rows_k: limbs per poly of operand k (0: Lrows; rows2 < 0: one broadcast row); half: 0 all coefficients, 1 / 2 the first / second N/2
  static const vec_fn* table = vec_table(std::make_integer_sequence<int, RH_OP_COUNT>());
  (void)hipGetLastError();
  ScalarPack a, b;
  memset(&a, 0, sizeof(a)); memset(&b, 0, sizeof(b));
  if (s0) memcpy(a.s, s0, (size_t)Lrows * 8);
  if (s1) memcpy(b.s, s1, (size_t)Lrows * 8);
  const unsigned rows = (unsigned)npoly * (unsigned)Lrows;
  if (rows == 0) return RH_OK;
  const unsigned n = (unsigned)r->N, npairs = n >> 1;
  const RhStreamGrid g = rh_stream_grid(r, rows);
  const RowStrides rs{rows1 ? rows1 : Lrows, rows2 ? rows2 : Lrows, rows3 ? rows3 : Lrows, half == 2 ? npairs / 2 : 0u, half == 1 ? npairs / 2 : npairs, g.nt};
  hipLaunchKernelGGL(table[opcode], g.grid, dim3(256), 0, rh_stream(r), p1, p2, p3, n, a, b, r->d_consts + limb0, Lrows, rs);
  return rh_launch_ok("vec_op");
}

// p2 = ONE row of N words used for every (poly, limb): MulByVectorMontgomery(ThenAddLazy) (ring/operations.go:366-377) with the
// MUL_MONT / MUL_MONT_THEN_ADD_LAZY opcodes (any two-operand opcode works)
extern "C" int rh_ring_vec_op_bcast(rh_ring* r, int opcode, const uint64_t* p1, int rows1, const uint64_t* vector, uint64_t* p3, int rows3,
                                    int npoly, int level) {
  if (!r || !p1 || !vector || !p3) return rh_fail(RH_ERR_ARG, "vec_op_bcast: null argument");
  if (opcode < 0 || opcode >= RH_OP_COUNT || !op_reads_y(opcode)) return rh_fail(RH_ERR_ARG, "vec_op_bcast: opcode %d has no second operand", opcode);
  if (level < 0 || level >= r->L || rows1 < level + 1 || rows3 < level + 1 || npoly < 0) return rh_fail(RH_ERR_ARG, "vec_op_bcast: bad level / rows / npoly");
  (void)hipSetDevice(r->device);
  return rh_vec_launch(r, opcode, p1, vector, p3, npoly, level + 1, 0, nullptr, nullptr, rows1, -1, rows3);
}
// one-operand scalar opcodes with one RNS scalar for coefficients [0, N/2) and another for [N/2, N): Add / Sub / MulDoubleRNSScalar(ThenAdd)
// (ring/operations.go:167-184, 250-266); s_lo / s_hi: level+1 words each on the host, in the form the opcode takes them
extern "C" int rh_ring_vec_op_halves(rh_ring* r, int opcode, const uint64_t* p1, uint64_t* p3, int npoly, int level, const uint64_t* s_lo,
                                     const uint64_t* s_hi) {
  if (!r || !p1 || !p3 || !s_lo || !s_hi) return rh_fail(RH_ERR_ARG, "vec_op_halves: null argument");
  if (opcode < 0 || opcode >= RH_OP_COUNT || op_reads_y(opcode)) return rh_fail(RH_ERR_ARG, "vec_op_halves: opcode %d is not a one-operand scalar opcode", opcode);
  if (level < 0 || level >= r->L || npoly < 0) return rh_fail(RH_ERR_ARG, "vec_op_halves: bad level / npoly");
  if (r->N % 4) return rh_fail(RH_ERR_ARG, "vec_op_halves: N must be a multiple of 4");
  (void)hipSetDevice(r->device);
  if (int rc = rh_vec_launch(r, opcode, p1, nullptr, p3, npoly, level + 1, 0, s_lo, nullptr, 0, 0, 0, 1)) return rc;
  return rh_vec_launch(r, opcode, p1, nullptr, p3, npoly, level + 1, 0, s_hi, nullptr, 0, 0, 0, 2);
}

extern "C" int rh_ring_vec_op(rh_ring* r, int opcode, const uint64_t* p1, const uint64_t* p2, uint64_t* p3, int npoly, int level,
                              const uint64_t* s0, const uint64_t* s1) {
  if (!r || !p3) return rh_fail(RH_ERR_ARG, "vec_op: null argument");
  if (opcode < 0 || opcode >= RH_OP_COUNT) return rh_fail(RH_ERR_ARG, "vec_op: unknown opcode %d", opcode);
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "vec_op: level %d out of range [0,%d)", level, r->L);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "vec_op: npoly < 0");
  if (op_reads_x(opcode) && !p1) return rh_fail(RH_ERR_ARG, "vec_op %d: p1 is null", opcode);
  if (op_reads_y(opcode) && !p2) return rh_fail(RH_ERR_ARG, "vec_op %d: p2 is null", opcode);
  (void)hipSetDevice(r->device);
  return rh_vec_launch(r, opcode, p1, p2, p3, npoly, level + 1, 0, s0, s1);
}
extern "C" int rh_ring_vec_op_rows(rh_ring* r, int opcode, const uint64_t* p1, int rows1, const uint64_t* p2, int rows2, uint64_t* p3, int rows3,
                                   int npoly, int level, const uint64_t* s0, const uint64_t* s1) {
  if (!r) return rh_fail(RH_ERR_ARG, "vec_op: null argument");
  if (level < 0 || level >= r->L) return rh_fail(RH_ERR_ARG, "vec_op: level %d out of range [0,%d)", level, r->L);
  const int need = level + 1;
  if ((p1 && rows1 < need) || (p2 && rows2 < need) || rows3 < need) return rh_fail(RH_ERR_ARG, "vec_op: a block has fewer than level+1 = %d limbs per poly", need);
  if ((!p1 || rows1 == need) && (!p2 || rows2 == need) && rows3 == need) return rh_ring_vec_op(r, opcode, p1, p2, p3, npoly, level, s0, s1);
  if (!p3) return rh_fail(RH_ERR_ARG, "vec_op: null argument");
  if (opcode < 0 || opcode >= RH_OP_COUNT) return rh_fail(RH_ERR_ARG, "vec_op: unknown opcode %d", opcode);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "vec_op: npoly < 0");
  if (op_reads_x(opcode) && !p1) return rh_fail(RH_ERR_ARG, "vec_op %d: p1 is null", opcode);
  if (op_reads_y(opcode) && !p2) return rh_fail(RH_ERR_ARG, "vec_op %d: p2 is null", opcode);
  (void)hipSetDevice(r->device);
  return rh_vec_launch(r, opcode, p1, p2, p3, npoly, need, 0, s0, s1, p1 ? rows1 : need, p2 ? rows2 : need, rows3);   // one launch, per-operand row strides
}

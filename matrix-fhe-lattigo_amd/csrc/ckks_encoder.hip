// ckks_encoder.hip -- schemes/ckks/encoder.go (float64 path, prec <= 53) on device batches of nvec vectors: standard rings
// (rh_ckks_encoder_create) and the real-only embedding of conjugate-invariant rings (rh_ckks_encoder_create_real).
//
//   Encode  = copy -> special IFFT (ckks_vector_ops.go:18-47) -> quantize with the stride-gap spread (utils.go:130-234,
//             core/rlwe/utils.go:187-245) [-> MForm inside the quantizer] [-> Ring.NTT]
//   Decode  = [Ring.INTT ->] exact CRT reconstruction to the nearest double / scale (encoder.go:796-1003) -> special FFT (:49-76) [-> rounding
//             to logprec bits]
//
// The sparse case of NTTSparseAndMontgomery transforms in dimension n with the roots of N and repeats every value gap times; that is the
// full transform of the polynomial in X^gap, so the spread followed by the ring's own NTT gives the same canonical words, and MForm before
// or after a transform whose outputs are canonical commutes with it.  The transforms' stage grouping is in ckks_encoder_kernels.hip.hpp.
//
// Conjugate-invariant ring of degree n (e->real): m = NthRoot = 4n, rotGroup of n entries, up to n slots (one FFT size above a standard ring
// of the same degree: the same stage kernels, one more stage).  Encode drops the imaginary parts on the way into the scratch block
// (encoder.go:225-228), quantizes the real parts alone at stride n / slots (utils.go:145-147) and transforms with the ring's own
// conjugate-invariant NTT; Decode reads the first `slots` strided coefficients and sets imag[i] = 0 - real[slots - i] (the `isreal` arms,
// encoder.go:825-831, :938-944) before the special FFT.
//
// The handle owns its scratch (two complex blocks and one poly block); rh_ckks_encoder_reserve sizes it so that no later call allocates.
// Calls are asynchronous on the ring's stream and lock the handle for the enqueue only: the scratch is reused in stream order.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstring>
#include "engine_internal.hpp"
#include "ckks_encoder_kernels.hip.hpp"

struct rh_ckks_encoder {
  rh_ring* Q = nullptr;
  int logN = 0, logm = 0;
  bool real = false;                   // conjugate-invariant ring: the real-only embedding
  int max_log_slots = 0;               // LogMaxDimensions().Cols: logN - 1, or logN when real
  EncCplx* d_roots = nullptr;          // m + 1 roots as the caller computed them (GetRootsComplex128, utils.go:53-77)
  unsigned* d_rot = nullptr;           // rotGroup: 5^j mod m, j < m / 4 (encoder.go:77-83)
  u64* d_tables = nullptr;             // garner | qmod | Q | Q >> 1
  EncCrtTables tb{};
  void* buf[3] = {nullptr, nullptr, nullptr}; size_t buf_bytes[3] = {0, 0, 0};   // 0, 1: (nvec, slots) complex; 2: (nvec, L, N) words
  int fft_lds_log = 12;                // largest log2 block whose stages run in one workgroup's LDS (16 << 12 = 64 KiB)
  std::recursive_mutex mu;
};

typedef unsigned __int128 enc_u128;
static u64 enc_mulmod(u64 a, u64 b, u64 q) { return (u64)((enc_u128)a * b % q); }
static u64 enc_powmod(u64 b, u64 e, u64 q) { u64 r = 1 % q; b %= q; for (; e; e >>= 1, b = enc_mulmod(b, b, q)) if (e & 1) r = enc_mulmod(r, b, q); return r; }

extern "C" void rh_ckks_encoder_destroy(rh_ckks_encoder* e) {
  if (!e) return;
  if (e->d_roots) (void)hipFree(e->d_roots);
  if (e->d_rot) (void)hipFree(e->d_rot);
  if (e->d_tables) (void)hipFree(e->d_tables);
  for (void* p : e->buf) if (p) (void)hipFree(p);
  delete e;
}

static int enc_create(rh_ckks_encoder** out, rh_ring* ring, const double* roots, size_t nroots, unsigned prec, bool real, const char* who) {
  if (prec > 53) return rh_fail(RH_ERR_UNSUPPORTED, "%s: prec = %u > 53 needs the *big.Float / *bignum.Complex encoder, which stays with the reference", who, prec);
  const size_t m = (real ? 4 : 2) * (size_t)ring->N;
  if (nroots != m + 1) return rh_fail(RH_ERR_ARG, "%s: %zu roots given, NthRoot + 1 = %zu expected", who, nroots, m + 1);
  if (ring->L > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: %d limbs, at most %d", who, ring->L, RH_MAX_LIMBS);
  rh_ckks_encoder* e = new rh_ckks_encoder();
  e->Q = ring; e->logN = ring->logN; e->logm = ring->logN + (real ? 2 : 1);
  e->real = real; e->max_log_slots = real ? ring->logN : ring->logN - 1;
  const int L = ring->L;
  std::vector<unsigned> rot(m >> 2);
  unsigned five = 1;
  for (size_t i = 0; i < rot.size(); ++i) { rot[i] = five; five = (unsigned)(((u64)five * 5) & (m - 1)); }
  // garner | qmod | Q | Q >> 1
  std::vector<u64> t((size_t)L + 3 * (size_t)L * L, 0);
  u64* garner = t.data(); u64* qmod = garner + L; u64* Qw = qmod + (size_t)L * L; u64* Qh = Qw + (size_t)L * L;
  const std::vector<u64>& q = ring->moduli;
  for (int j = 0; j < L; ++j) {
    u64 prod = 1 % q[j];
    for (int i = 0; i < L; ++i) qmod[(size_t)j * L + i] = q[i] % q[j];
    for (int i = 0; i < j; ++i) prod = enc_mulmod(prod, q[i] % q[j], q[j]);
    garner[j] = enc_powmod(prod, q[j] - 2, q[j]);                       // the moduli are distinct primes
  }
  std::vector<u64> acc((size_t)L, 0);
  acc[0] = 1;
  for (int lv = 0; lv < L; ++lv) {
    u64 carry = 0;
    for (int w = 0; w < L; ++w) { const enc_u128 p = (enc_u128)acc[w] * q[lv] + carry; acc[w] = (u64)p; carry = (u64)(p >> 64); }
    for (int w = 0; w < L; ++w) {
      Qw[(size_t)lv * L + w] = acc[w];
      Qh[(size_t)lv * L + w] = (acc[w] >> 1) | (w + 1 < L ? acc[w + 1] << 63 : 0);
    }
  }
  (void)hipSetDevice(ring->device);
  int rc = RH_OK;
  if (hipMalloc((void**)&e->d_roots, (m + 1) * sizeof(EncCplx)) != hipSuccess || hipMalloc((void**)&e->d_rot, rot.size() * sizeof(unsigned)) != hipSuccess ||
      hipMalloc((void**)&e->d_tables, t.size() * 8) != hipSuccess)
    rc = rh_fail(RH_ERR_NOMEM, "rh_ckks_encoder_create: hipMalloc failed");
  if (!rc && (hipMemcpy(e->d_roots, roots, (m + 1) * sizeof(EncCplx), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(e->d_rot, rot.data(), rot.size() * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess ||
              hipMemcpy(e->d_tables, t.data(), t.size() * 8, hipMemcpyHostToDevice) != hipSuccess))
    rc = rh_fail(RH_ERR_DEVICE, "rh_ckks_encoder_create: hipMemcpy failed");
  if (rc) { rh_ckks_encoder_destroy(e); return rc; }
  e->tb.garner = e->d_tables; e->tb.qmod = e->d_tables + L; e->tb.Q = e->tb.qmod + (size_t)L * L; e->tb.Qhalf = e->tb.Q + (size_t)L * L; e->tb.Lmax = L;
  *out = e;
  return RH_OK;
}

extern "C" int rh_ckks_encoder_create(rh_ckks_encoder** out, rh_ring* ring, const double* roots, size_t nroots, unsigned prec) {
  if (!out || !ring || !roots) return rh_fail(RH_ERR_ARG, "rh_ckks_encoder_create: null argument");
  if (ring->kind == RH_RING_CI) return rh_fail(RH_ERR_UNSUPPORTED, "rh_ckks_encoder_create: conjugate-invariant rings are not supported (the real-only embedding stays with the reference)");
  if (ring->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "rh_ckks_encoder_create: 3N rings are not supported (the CKKS encoder is defined on power-of-two cyclotomics)");
  return enc_create(out, ring, roots, nroots, prec, false, "rh_ckks_encoder_create");
}

// the real-only encoder of a conjugate-invariant ring: roots of 4N + 1 entries
extern "C" int rh_ckks_encoder_create_real(rh_ckks_encoder** out, rh_ring* ring, const double* roots, size_t nroots, unsigned prec) {
  if (!out || !ring || !roots) return rh_fail(RH_ERR_ARG, "rh_ckks_encoder_create_real: null argument");
  if (ring->kind != RH_RING_CI) return rh_fail(RH_ERR_UNSUPPORTED, "rh_ckks_encoder_create_real: a conjugate-invariant ring is expected (standard rings: rh_ckks_encoder_create)");
  return enc_create(out, ring, roots, nroots, prec, true, "rh_ckks_encoder_create_real");
}

extern "C" int rh_ckks_encoder_set_tuning(rh_ckks_encoder* e, const char* key, long value) {
  if (!e || !key) return rh_fail(RH_ERR_ARG, "rh_ckks_encoder_set_tuning: null argument");
  if (!strcmp(key, "ckks_fft_lds_log")) {
    if (value < 1 || value > 12) return rh_fail(RH_ERR_ARG, "ckks_fft_lds_log must be in [1, 12] (16 << 12 bytes = 64 KiB of LDS)");
    std::lock_guard<std::recursive_mutex> lk(e->mu);
    e->fft_lds_log = (int)value;
    return RH_OK;
  }
  return rh_fail(RH_ERR_ARG, "rh_ckks_encoder_set_tuning: unknown key '%s'", key);
}

static int enc_scratch(rh_ckks_encoder* e, int which, size_t bytes) {
  if (e->buf_bytes[which] >= bytes) return RH_OK;
  if (e->buf[which]) (void)hipFree(e->buf[which]);                      // waits for the work that still reads it
  e->buf[which] = nullptr; e->buf_bytes[which] = 0;
  if (hipMalloc(&e->buf[which], bytes ? bytes : 8) != hipSuccess) return rh_fail(RH_ERR_NOMEM, "hipMalloc(ckks encoder scratch) failed");
  e->buf_bytes[which] = bytes;
  return RH_OK;
}

extern "C" int rh_ckks_encoder_reserve(rh_ckks_encoder* e, int nvec) {
  if (!e || nvec < 0) return rh_fail(RH_ERR_ARG, "rh_ckks_encoder_reserve: bad argument");
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  (void)hipSetDevice(e->Q->device);
  const size_t N = (size_t)e->Q->N, cb = ((size_t)nvec << e->max_log_slots) * sizeof(EncCplx);
  if (int rc = enc_scratch(e, 0, cb)) return rc;
  if (int rc = enc_scratch(e, 1, cb)) return rc;
  return enc_scratch(e, 2, (size_t)nvec * e->Q->L * N * 8);
}

// The transform of nvec vectors of 1 << logn values, data -> data.  tmp: a second block of the same size, used when the vector is longer
// than the LDS block (the first launch moves the data there, the last one back: the bit reversal cannot run in place across workgroups).
static int enc_fft(rh_ckks_encoder* e, EncCplx* data, EncCplx* tmp, int logn, int nvec, bool inverse, hipStream_t st) {
  if (logn == 0 && !inverse) return RH_OK;                              // SpecialFFTDouble of one value: no stage, no division
  const int logb = logn < e->fft_lds_log ? logn : e->fft_lds_log, logm = e->logm;
  const dim3 gl(1u << (logn - logb), (unsigned)nvec), gs(((1u << logn) / 2 + 255) / 256, (unsigned)nvec);
  const size_t lds = (size_t)16 << logb;
  if (logb == logn) {
    if (inverse) ckks_fft_lds_kernel<true><<<gl, 256, lds, st>>>(data, data, logn, logb, logm, e->d_roots, e->d_rot);
    else ckks_fft_lds_kernel<false><<<gl, 256, lds, st>>>(data, data, logn, logb, logm, e->d_roots, e->d_rot);
    return rh_launch_ok("ckks_fft_lds_kernel");
  }
  if (inverse) {                                                        // len = n .. 2^(logb+1) in global memory, the rest in LDS
    for (int ll = logn; ll > logb; --ll)
      ckks_fft_stage_kernel<true><<<gs, 256, 0, st>>>(ll == logn ? data : tmp, tmp, logn, ll, logm, e->d_roots, e->d_rot);
    ckks_fft_lds_kernel<true><<<gl, 256, lds, st>>>(tmp, data, logn, logb, logm, e->d_roots, e->d_rot);
  } else {                                                              // bit reversal + len = 2 .. 2^logb in LDS, the rest in global memory
    ckks_fft_lds_kernel<false><<<gl, 256, lds, st>>>(data, tmp, logn, logb, logm, e->d_roots, e->d_rot);
    for (int ll = logb + 1; ll <= logn; ++ll)
      ckks_fft_stage_kernel<false><<<gs, 256, 0, st>>>(tmp, ll == logn ? data : tmp, logn, ll, logm, e->d_roots, e->d_rot);
  }
  return rh_launch_ok("ckks_fft_stage_kernel");
}

static int enc_args(rh_ckks_encoder* e, int log_slots, int nvec, const char* who) {
  if (!e) return rh_fail(RH_ERR_ARG, "%s: null encoder handle", who);
  if (log_slots < 0 || log_slots > e->max_log_slots)
    return rh_fail(RH_ERR_ARG, "%s: logSlots (%d) must be greater or equal to 0 and smaller than %d", who, log_slots, e->max_log_slots + 1);
  if (nvec < 0 || nvec > 65535) return rh_fail(RH_ERR_ARG, "%s: nvec = %d out of range [0, 65535]", who, nvec);
  return RH_OK;
}

static int enc_transform(rh_ckks_encoder* e, double* values, int log_slots, int nvec, bool inverse, const char* who) {
  if (int rc = enc_args(e, log_slots, nvec, who)) return rc;
  if (!values) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (nvec == 0) return RH_OK;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  RhCallScope sc(rh_stream(e->Q));
  (void)hipSetDevice(e->Q->device);
  (void)hipGetLastError();
  if (log_slots > e->fft_lds_log)
    if (int rc = enc_scratch(e, 1, ((size_t)nvec << log_slots) * sizeof(EncCplx))) return rc;
  return enc_fft(e, (EncCplx*)values, (EncCplx*)e->buf[1], log_slots, nvec, inverse, rh_stream(e->Q));
}
extern "C" int rh_ckks_special_ifft(rh_ckks_encoder* e, double* values_dev, int log_slots, int nvec) {
  return enc_transform(e, values_dev, log_slots, nvec, true, "rh_ckks_special_ifft");
}
extern "C" int rh_ckks_special_fft(rh_ckks_encoder* e, double* values_dev, int log_slots, int nvec) {
  return enc_transform(e, values_dev, log_slots, nvec, false, "rh_ckks_special_fft");
}

static int enc_level(rh_ckks_encoder* e, int level, const char* who) {
  if (level < 0 || level >= e->Q->L) return rh_fail(RH_ERR_ARG, "%s: level %d out of range [0,%d)", who, level, e->Q->L);
  return RH_OK;
}

static int enc_quantize(rh_ckks_encoder* e, int level, const double* vals, u64* out, int nvec, double scale, int batched, unsigned slots,
                        unsigned nvals, int loggap, int is_ntt, int mont, hipStream_t st) {
  const unsigned n = (unsigned)e->Q->N;
  const dim3 g((n + 255) / 256, (unsigned)nvec);
  ckks_quantize_kernel<<<g, 256, 0, st>>>(vals, out, n, level + 1, e->Q->d_consts, scale, batched, slots, nvals, loggap,
                                          (is_ntt || mont) ? 1 : 0, mont ? 1 : 0, batched && e->real ? 1 : 0);
  if (int rc = rh_launch_ok("ckks_quantize_kernel")) return rc;
  if (is_ntt) return rh_ring_ntt_any(e->Q, out, out, nvec, level + 1, 0, false);
  return RH_OK;
}

extern "C" int rh_ckks_encode(rh_ckks_encoder* e, int level, int log_slots, double scale, const double* values_dev, int nvec, uint64_t* out_dev,
                              int is_ntt, int is_montgomery) {
  if (int rc = enc_args(e, log_slots, nvec, "rh_ckks_encode")) return rc;
  if (int rc = enc_level(e, level, "rh_ckks_encode")) return rc;
  if (!values_dev || !out_dev) return rh_fail(RH_ERR_ARG, "rh_ckks_encode: null argument");
  if (nvec == 0) return RH_OK;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  RhCallScope sc(rh_stream(e->Q));
  hipStream_t st = rh_stream(e->Q);
  (void)hipSetDevice(e->Q->device);
  (void)hipGetLastError();
  const size_t cb = ((size_t)nvec << log_slots) * sizeof(EncCplx);
  if (int rc = enc_scratch(e, 0, cb)) return rc;
  if (log_slots > e->fft_lds_log) if (int rc = enc_scratch(e, 1, cb)) return rc;
  if (e->real) {                                                        // buffCmplx[i] = complex(real(values[i]), 0) (:225-228)
    const size_t count = (size_t)nvec << log_slots;
    ckks_copy_real_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(values_dev, (double*)e->buf[0], count);
    if (int rc = rh_launch_ok("ckks_copy_real_kernel")) return rc;
  } else if (hipMemcpyAsync(e->buf[0], values_dev, cb, hipMemcpyDeviceToDevice, st) != hipSuccess) return rh_fail(RH_ERR_DEVICE, "rh_ckks_encode: copy failed");
  if (int rc = enc_fft(e, (EncCplx*)e->buf[0], (EncCplx*)e->buf[1], log_slots, nvec, true, st)) return rc;
  return enc_quantize(e, level, (const double*)e->buf[0], out_dev, nvec, scale, 1, 1u << log_slots, 0, e->max_log_slots - log_slots, is_ntt,
                      is_montgomery, st);
}

extern "C" int rh_ckks_encode_coeffs(rh_ckks_encoder* e, int level, double scale, const double* values_dev, int nvals, int nvec, uint64_t* out_dev,
                                     int is_ntt) {
  if (int rc = enc_args(e, 0, nvec, "rh_ckks_encode_coeffs")) return rc;
  if (int rc = enc_level(e, level, "rh_ckks_encode_coeffs")) return rc;
  if (!values_dev || !out_dev) return rh_fail(RH_ERR_ARG, "rh_ckks_encode_coeffs: null argument");
  if (nvals < 0 || nvals > e->Q->N) return rh_fail(RH_ERR_ARG, "cannot Encode: maximum number of values is %d but len(values) is %d", e->Q->N, nvals);
  if (nvec == 0) return RH_OK;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  RhCallScope sc(rh_stream(e->Q));
  (void)hipSetDevice(e->Q->device);
  (void)hipGetLastError();
  return enc_quantize(e, level, values_dev, out_dev, nvec, scale, 0, 0, (unsigned)nvals, 0, is_ntt, 0, rh_stream(e->Q));
}

extern "C" int rh_ckks_decode(rh_ckks_encoder* e, int level, int log_slots, double scale, double logprec, int is_ntt, int batched, int real_only,
                              const uint64_t* poly_dev, int nvec, double* values_dev) {
  if (int rc = enc_args(e, log_slots, nvec, "rh_ckks_decode")) return rc;
  if (int rc = enc_level(e, level, "rh_ckks_decode")) return rc;
  if (!poly_dev || !values_dev) return rh_fail(RH_ERR_ARG, "rh_ckks_decode: null argument");
  if (!batched && level != 0 && level != e->Q->L - 1)
    return rh_fail(RH_ERR_UNSUPPORTED, "rh_ckks_decode: IsBatched = false at level %d of %d is not supported: polyToFloatCRT (encoder.go:1022) reconstructs over the "
                                       "encoder's full ring, so between level 0 and the top level its result depends on stale limbs of the encoder's buffer, not on "
                                       "the plaintext", level, e->Q->L - 1);
  if (!(scale > 0)) return rh_fail(RH_ERR_ARG, "rh_ckks_decode: the scale must be positive");
  if (nvec == 0) return RH_OK;
  std::lock_guard<std::recursive_mutex> lk(e->mu);
  RhCallScope sc(rh_stream(e->Q));
  hipStream_t st = rh_stream(e->Q);
  (void)hipSetDevice(e->Q->device);
  (void)hipGetLastError();
  const unsigned n = (unsigned)e->Q->N, slots = 1u << log_slots;
  const int L = level + 1;
  const u64* src = poly_dev;
  if (is_ntt) {
    if (int rc = enc_scratch(e, 2, (size_t)nvec * L * n * 8)) return rc;
    if (int rc = rh_ring_ntt_any(e->Q, poly_dev, (u64*)e->buf[2], nvec, L, 0, true)) return rc;      // INTT into the encoder's buffer (:485-486)
    src = (const u64*)e->buf[2];
  }
  if (!batched) {                                                       // plaintextToFloat (:467-472): every coefficient, no FFT, logprec unused (:731)
    ckks_crt_to_double_kernel<<<dim3((n + 255) / 256, (unsigned)nvec), 256, 0, st>>>(src, values_dev, n, L, e->Q->d_consts, e->tb, scale, 0, 0, 1);
    return rh_launch_ok("ckks_crt_to_double_kernel");
  }
  if (log_slots > e->fft_lds_log) if (int rc = enc_scratch(e, 1, ((size_t)nvec << log_slots) * sizeof(EncCplx))) return rc;
  const dim3 g(((e->real ? 1 : 2) * slots + 255) / 256, (unsigned)nvec);
  ckks_crt_to_double_kernel<<<g, 256, 0, st>>>(src, values_dev, n, L, e->Q->d_consts, e->tb, scale, slots, e->max_log_slots - log_slots, e->real ? 2 : 0);
  if (int rc = rh_launch_ok("ckks_crt_to_double_kernel")) return rc;
  if (int rc = enc_fft(e, (EncCplx*)values_dev, (EncCplx*)e->buf[1], log_slots, nvec, false, st)) return rc;
  if (logprec != 0 || real_only) {
    const size_t count = (size_t)nvec << log_slots;
    ckks_round_prec_kernel<<<(unsigned)((count + 255) / 256), 256, 0, st>>>(values_dev, count, exp2(logprec), logprec != 0 ? 1 : 0, real_only ? 1 : 0);
    return rh_launch_ok("ckks_round_prec_kernel");
  }
  return RH_OK;
}

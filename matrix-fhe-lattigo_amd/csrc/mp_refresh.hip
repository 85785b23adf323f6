// mp_refresh.hip -- the share conversion of the collective refresh (multiparty/mpckks/{sharing,transform,refresh}.go; kernels:
// mp_refresh_kernels.hip.hpp): multiword integers per coefficient that never leave the device.
//   rh_mp_big_sample      the mask law of mpckks/sharing.go:120-129 on the samplers' stream
//   rh_mp_big_to_rns      SetCoefficientsBigint (ring/ring.go:433-447) with the spread of NTTSparseAndMontgomery (core/rlwe/utils.go:187-245)
//   rh_mp_big_from_rns    PolyToBigintCentered (ring/ring.go:503-543)
//   rh_mp_big_muldiv      the scale change of applyTransformAndScale (mpckks/transform.go:363-376)
//   rh_mp_refresh_recode  the three in one kernel, no big-integer block in memory between them
// The four conversions are instantiations of ONE kernel (source, optional scale change, destination), so the fused form computes the bits of
// the three separate calls by construction.  The transforms are the library's own, driven from the host (multiparty.py).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "qp_rows_host.hpp"
#include "mp_refresh_kernels.hip.hpp"

// n values per poly: a power of two, at least 2 (n = 2 slots, one slot at the least), at most the ring's degree where a ring is given
static int mpb_shape_ok(int n, int W, int npoly, const char* who) {
  if (W < 1 || W > MPB_MAX_W) return rh_fail(RH_ERR_ARG, "%s: %d words per value, a block has 1 to %d", who, W, MPB_MAX_W);
  if (n < 2 || (n & (n - 1))) return rh_fail(RH_ERR_ARG, "%s: %d values per poly: a power of two, at least 2", who, n);
  if (npoly < 0) return rh_fail(RH_ERR_ARG, "%s: npoly < 0", who);
  return RH_OK;
}
static int mpb_log2(unsigned x) { int l = 0; while ((1u << l) < x) ++l; return l; }
static dim3 mpb_grid(int npoly, unsigned lanes) {
  unsigned chunks = (lanes + 255) / 256;
  if (chunks > 1024) chunks = 1024;
  return dim3((unsigned)npoly, chunks ? chunks : 1);
}

extern "C" int rh_mp_big_sample(rh_ring* r, const uint64_t* state, uint64_t call, uint64_t poly0, int logBound, uint64_t* blk, int n, int W, int npoly) {
  const char* who = "rh_mp_big_sample";
  if (int rc = rh_ring_ok(r, 0, 0, who)) return rc;
  if (int rc = mpb_shape_ok(n, W, npoly, who)) return rc;
  if (!state || !blk) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if ((uintptr_t)blk & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  if (logBound < 1 || logBound > 64 * W - 1) return rh_fail(RH_ERR_ARG, "%s: logBound %d out of range [1, %d] for %d words", who, logBound, 64 * W - 1, W);
  if (!npoly) return RH_OK;
  (void)rh_stream_begin(r, (unsigned)npoly);
  SampArgs a;
  memcpy(a.h, state, sizeof(a.h));
  a.call = call; a.poly0 = poly0; a.row0 = 0;
  const dim3 grid = mpb_grid(npoly, ((unsigned)n + 7) / 8);
  hipStream_t st = rh_stream(r);
  rh_with_s1<1, MPB_MAX_W>(W, [&](auto Wc) { mp_big_sample_kernel<decltype(Wc)::value><<<grid, 256, 0, st>>>(a, blk, (unsigned)n, logBound); });
  return rh_launch_ok("mp_big_sample_kernel");
}

// ---- host multiword integers for the tables: little-endian words, as many as the value needs -------------------------------------------------------
typedef std::vector<u64> MpbInt;
static void mpb_mul_word(MpbInt& a, u64 m) {
  u64 carry = 0;
  for (auto& w : a) { const u128 p = (u128)w * m + carry; w = (u64)p; carry = (u64)(p >> 64); }
  if (carry) a.push_back(carry);
}
static int mpb_bits(const MpbInt& a) {
  for (int w = (int)a.size() - 1; w >= 0; --w)
    if (a[w]) return 64 * w + 64 - __builtin_clzll(a[w]);
  return 0;
}

// Q = q_0 .. q_level of the ring, its half, Q / q_k and (Q / q_k)^-1 mod q_k; qbits: Len(Q)
static int mpb_crt(const rh_ring* r, int level, MpbCrt* t, int* qbits, const char* who) {
  const int L = level + 1;
  if (L > MPB_MAX_LIMBS) return rh_fail(RH_ERR_UNSUPPORTED, "%s: %d source limbs, a share is reconstructed from at most %d", who, L, MPB_MAX_LIMBS);
  memset(t, 0, sizeof(*t));
  MpbInt Q{1};
  for (int k = 0; k < L; ++k) mpb_mul_word(Q, r->moduli[k]);
  *qbits = mpb_bits(Q);
  if (*qbits > 64 * MPB_MAX_W - 1)
    return rh_fail(RH_ERR_UNSUPPORTED, "%s: Q at level %d has %d bits, a centred value needs more than the %d words of a block (Q >= 2^%d)", who, level, *qbits,
                   MPB_MAX_W, 64 * MPB_MAX_W - 1);
  for (size_t w = 0; w < Q.size(); ++w) { t->Q[w] = Q[w]; t->half[w] = (Q[w] >> 1) | (w + 1 < Q.size() ? Q[w + 1] << 63 : 0); }
  for (int k = 0; k < L; ++k) {
    const u64 q = r->moduli[k];
    MpbInt h{1};
    u64 prod = 1 % q;
    for (int j = 0; j < L; ++j)
      if (j != k) { mpb_mul_word(h, r->moduli[j]); prod = rh::mulmod(prod, r->moduli[j] % q, q); }
    for (size_t w = 0; w < h.size(); ++w) t->qhat[k][w] = h[w];
    t->yinv[k] = rh::invmod_prime(prod, q);
  }
  return RH_OK;
}

// source / destination of one recode launch
struct MpbEnd { rh_ring* ring; int level; const u64* poly; int rows; const u64* blk; };

// the one launch behind the four conversions.  in.ring: from-RNS source (in.poly at in.rows rows per poly), else in.blk; out.ring: to-RNS
// destination (out.poly dense), else out.blk.  m NULL: no scale change.
// lead: the ring whose device and stream the launch takes.
static int mpb_recode(const char* who, rh_ring* lead, const MpbEnd& in, const MpbEnd& out, int n, int W, int npoly, const u64* m, int mwords, const u64* d,
                      int dwords, int accumulate) {
  if (int rc = rh_ring_ok(lead, 0, 0, who)) return rc;
  if (int rc = mpb_shape_ok(n, W, npoly, who)) return rc;
  MpbArgs a; memset(&a, 0, sizeof(a));
  static MpbCrt zero_crt;
  MpbCrt crt_local;
  const MpbCrt* crt = &zero_crt;
  a.n = (unsigned)n; a.acc = accumulate;
  size_t blk_words = (size_t)npoly * W * (size_t)n;
  RhBlock wr[1], rd[1];
  if (in.ring) {
    if (int rc = rh_ring_ok(in.ring, in.level, npoly, who, "npoly < 0")) return rc;
    if (!in.poly) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
    if (n > in.ring->N) return rh_fail(RH_ERR_ARG, "%s: %d values per poly exceed the source ring's degree %d", who, n, in.ring->N);
    if (in.rows < in.level + 1) return rh_fail(RH_ERR_ARG, "%s: in_rows %d < %d limbs", who, in.rows, in.level + 1);
    int qbits;
    if (int rc = mpb_crt(in.ring, in.level, &crt_local, &qbits, who)) return rc;
    if (qbits > 64 * W - 1) return rh_fail(RH_ERR_ARG, "%s: Q at level %d has %d bits, a centred value does not fit %d words", who, in.level, qbits, W);
    crt = &crt_local;
    a.src = in.poly; a.in_rows = in.rows; a.Lin = in.level + 1; a.Nin = (unsigned)in.ring->N; a.log_gap_in = mpb_log2((unsigned)in.ring->N / (unsigned)n);
    rd[0] = {in.poly, npoly ? ((size_t)(npoly - 1) * in.rows + a.Lin) * (size_t)in.ring->N : 0};
  } else {
    if (!in.blk) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
    a.src = in.blk;
    rd[0] = {in.blk, blk_words};
  }
  if (out.ring) {
    if (int rc = rh_ring_ok(out.ring, out.level, npoly, who, "npoly < 0")) return rc;
    if (!out.poly) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
    if (n > out.ring->N) return rh_fail(RH_ERR_ARG, "%s: n > N_out: %d values per poly exceed the target ring's degree %d", who, n, out.ring->N);
    if (in.ring && in.ring->device != out.ring->device) return rh_fail(RH_ERR_ARG, "%s: the two rings are on different devices", who);
    if (accumulate < -1 || accumulate > 1) return rh_fail(RH_ERR_ARG, "%s: accumulate is 0, +1 or -1", who);
    a.dst = const_cast<u64*>(out.poly); a.Lout = out.level + 1; a.Nout = (unsigned)out.ring->N; a.log_gap_out = mpb_log2((unsigned)out.ring->N / (unsigned)n);
    wr[0] = {out.poly, (size_t)npoly * a.Lout * (size_t)out.ring->N};
  } else {
    if (!out.blk) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
    a.dst = const_cast<u64*>(out.blk);
    wr[0] = {out.blk, blk_words};
  }
  // a lane reads its own value whole before it writes it, so a block may be converted in place; anything else may not overlap
  if (wr[0].p == rd[0].p && !in.ring && !out.ring) rd[0].words = 0;
  if (int rc = rh_blocks_ok(wr, 1, rd, 1, who, "the output overlaps the input")) return rc;
  if (m) {
    if (!d || mwords < 1 || mwords > 2 || dwords < 1 || dwords > 4) return rh_fail(RH_ERR_ARG, "%s: the multiplier has 1 or 2 words and the divisor 1 to 4", who);
    for (int w = 0; w < mwords; ++w) a.m[w] = m[w];
    for (int w = 0; w < dwords; ++w) a.d[w] = d[w];
    if (!(a.d[0] | a.d[1] | a.d[2] | a.d[3])) return rh_fail(RH_ERR_ARG, "%s: the divisor is zero", who);
  }
  if (!npoly) return RH_OK;
  (void)rh_stream_begin(lead, (unsigned)npoly);
  const dim3 grid = mpb_grid(npoly, (unsigned)n);
  hipStream_t st = rh_stream(lead);
  const LimbConsts* ci = in.ring ? in.ring->d_consts : nullptr;
  const LimbConsts* co = out.ring ? out.ring->d_consts : nullptr;
  rh_with_s1<1, MPB_MAX_W>(W, [&](auto Wc) {
    rh_with_flag(in.ring != nullptr, [&](auto SRC) {
      rh_with_flag(m != nullptr, [&](auto MD) {
        rh_with_flag(out.ring != nullptr, [&](auto DST) {
          constexpr bool src = decltype(SRC)::value, md = decltype(MD)::value, dst = decltype(DST)::value;
          if constexpr (src || md || dst)                       // (a block copied to a block is no entry)
            mp_big_recode_kernel<decltype(Wc)::value, src, md, dst><<<grid, 256, 0, st>>>(a, *crt, ci, co);
        });
      });
    });
  });
  return rh_launch_ok("mp_big_recode_kernel");
}

extern "C" int rh_mp_big_to_rns(rh_ring* r, int level, const uint64_t* blk, int n, int W, uint64_t* out, int npoly, int accumulate) {
  return mpb_recode("rh_mp_big_to_rns", r, MpbEnd{nullptr, 0, nullptr, 0, blk}, MpbEnd{r, level, out, 0, nullptr}, n, W, npoly, nullptr, 0, nullptr, 0, accumulate);
}

extern "C" int rh_mp_big_from_rns(rh_ring* r, int level, const uint64_t* in, int in_rows, uint64_t* blk, int n, int W, int npoly, int accumulate) {
  return mpb_recode("rh_mp_big_from_rns", r, MpbEnd{r, level, in, in_rows, nullptr}, MpbEnd{nullptr, 0, nullptr, 0, blk}, n, W, npoly, nullptr, 0, nullptr, 0,
                    accumulate ? 1 : 0);
}

extern "C" int rh_mp_big_muldiv(rh_ring* r, const uint64_t* blk, uint64_t* out, int n, int W, int npoly, const uint64_t* m, int mwords, const uint64_t* d,
                                int dwords) {
  const char* who = "rh_mp_big_muldiv";
  if (!m || !d) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  return mpb_recode(who, r, MpbEnd{nullptr, 0, nullptr, 0, blk}, MpbEnd{nullptr, 0, nullptr, 0, out}, n, W, npoly, m, mwords, d, dwords, 0);   // r: device and stream alone
}

extern "C" int rh_mp_refresh_recode(rh_ring* ringIn, int levelIn, const uint64_t* in, int in_rows, const uint64_t* blk, int n, int W, rh_ring* ringOut,
                                    int levelOut, uint64_t* out, int npoly, const uint64_t* m, int mwords, const uint64_t* d, int dwords, int accumulate) {
  const char* who = "rh_mp_refresh_recode";
  if ((in != nullptr) == (blk != nullptr)) return rh_fail(RH_ERR_ARG, "%s: the source is a poly (with ringIn) or a block, one of them", who);
  if (in && !ringIn) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (!ringOut) return rh_fail(RH_ERR_ARG, "%s: null ring handle", who);
  if (!m || !d) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  return mpb_recode(who, ringOut, in ? MpbEnd{ringIn, levelIn, in, in_rows, nullptr} : MpbEnd{nullptr, 0, nullptr, 0, blk}, MpbEnd{ringOut, levelOut, out, 0, nullptr}, n, W,
                    npoly, m, mwords, d, dwords, accumulate);
}

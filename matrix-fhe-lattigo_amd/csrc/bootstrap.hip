// bootstrap.hip -- the passes of CKKS bootstrapping that no other entry point covers (kernels: bootstrap_kernels.hip.hpp):
//   rh_ckks_bootstrap_pack / _unpack  BootstrapMany's pack and unpack of sparse ciphertexts, :1035-1058 and :985-1001, every tree level of up to
//                            16 ciphertexts in ONE launch over both components
//   rh_ckks_bootstrap_modup  Evaluator.ModUp's lift from q0 to Q (and P), circuits/ckks/bootstrapping/evaluator.go:678-696, :703-722, :762-775,
//                            with the message scaling of :735-750 / :781-789 folded in; both components of a batch in ONE launch
//   rh_ckks_double_angle     Add(res, res, res) and Add(res, -sqrt2pi, res) of a double-angle round, circuits/ckks/mod1/mod1_evaluator.go:108-114
// Everything else of the circuit is the library's own (the key switch, the transforms, Trace, the DFT, the polynomial evaluator), driven from
// the host (bootstrapping.py, mod1.py).
#include <hip/hip_runtime.h>
#include <cstring>
#include "engine_internal.hpp"
#include "hostmath.hpp"
#include "qp_rows_host.hpp"
#include "bootstrap_kernels.hip.hpp"

// residues of the message scalar per limb -> MForm, as MulScalar takes its scalar (ring/operations.go: MForm(BRedAdd(scalar)))
static int modup_scalars(const rh_ring* r, int L, const u64* in, u64* out, const char* who, const char* of) {
  for (int i = 0; i < L; ++i) {
    if (in[i] >= r->moduli[i]) return rh_fail(RH_ERR_ARG, "%s: scalar %d%s is not a residue of its limb", who, i, of);
    out[i] = rh::mform(in[i], r->moduli[i]);
  }
  return RH_OK;
}

extern "C" int rh_ckks_bootstrap_modup(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* in0, const uint64_t* in1, int in_rows,
                                       uint64_t* out0, uint64_t* out1, uint64_t* c1Q, uint64_t* c1P, int npoly, const uint64_t* scalarQ,
                                       const uint64_t* scalarP) {
  const char* who = "rh_ckks_bootstrap_modup";
  if (int rc = rh_ring_ok(rQ, levelQ, npoly, who, "npoly < 0")) return rc;
  const bool encap = rP != nullptr;
  if (encap) {
    if (rP->kind != RH_RING_STANDARD) return rh_fail(RH_ERR_UNSUPPORTED, "%s: standard rings only (3N and conjugate-invariant rings are not supported)", who);
    if (rP->N != rQ->N || rP->device != rQ->device) return rh_fail(RH_ERR_ARG, "%s: ringQ and ringP differ in degree or device", who);
    if (levelP < 0 || levelP >= rP->L || levelP + 1 > RH_MAX_LIMBS) return rh_fail(RH_ERR_ARG, "%s: levelP %d out of range [0,%d)", who, levelP, rP->L);
    if (!c1Q || !c1P || out1) return rh_fail(RH_ERR_ARG, "%s: with ringP component 1 goes to c1Q and c1P, and out1 must be NULL", who);
    if ((scalarQ == nullptr) != (scalarP == nullptr)) return rh_fail(RH_ERR_ARG, "%s: the scalar needs its residues modulo Q and modulo P, or neither", who);
  } else if (c1Q || c1P || scalarP || !out1) {
    return rh_fail(RH_ERR_ARG, "%s: without ringP component 1 goes to out1, and c1Q, c1P and scalarP must be NULL", who);
  }
  if (!in0 || !in1 || !out0) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  if (in_rows < 1) return rh_fail(RH_ERR_ARG, "%s: in_rows < 1", who);
  const int LQ = levelQ + 1, LP = encap ? levelP + 1 : 0;
  const size_t N = (size_t)rQ->N, wq = (size_t)npoly * LQ * N, wp = (size_t)npoly * LP * N, wi = (size_t)npoly * (size_t)in_rows * N;
  if ((size_t)npoly * (size_t)(2 * LQ + LP) > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  // the lift is out of place: a lane reads limb 0 of its input and writes every limb of its outputs
  const RhBlock rd[2] = {{in0, wi}, {in1, wi}};
  const RhBlock wr[3] = {{out0, wq}, {encap ? c1Q : out1, wq}, {c1P, wp}};
  const int nw = encap ? 3 : 2;
  if (int rc = rh_blocks_ok(wr, nw, rd, 2, who, "an output overlaps an input: the lift is not computed in place")) return rc;
  if (int rc = rh_blocks_disjoint(wr, nw, who, "two outputs overlap")) return rc;
  RhScalars s; memset(&s, 0, sizeof(s));
  if (scalarQ) if (int rc = modup_scalars(rQ, LQ, scalarQ, s.a, who, " of Q")) return rc;
  if (scalarP) if (int rc = modup_scalars(rP, LP, scalarP, s.b, who, " of P")) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(rQ, (unsigned)npoly * (unsigned)(2 * LQ + LP));   // cache policy by the bytes WRITTEN; the grid is this kernel's own
  unsigned chunks = ((unsigned)N / 2 + 255) / 256; if (chunks > 65535) chunks = 65535;      // one coefficient pair per lane
  const dim3 grid(2u * (unsigned)npoly, chunks);
  hipStream_t st = rh_stream(rQ);
  const ModUpArgs p{{in0, in1}, {out0, out1}, c1Q, c1P};
  const unsigned n = (unsigned)N;
  const LimbConsts* cP = encap ? rP->d_consts : rQ->d_consts;
#define BTS_MODUP(E, S) bootstrap_modup_kernel<E, S><<<grid, 256, 0, st>>>(p, n, in_rows, rQ->d_consts, cP, LQ, LP, npoly, s, g.nt)
  if (encap) { if (scalarQ) BTS_MODUP(true, true); else BTS_MODUP(true, false); }
  else { if (scalarQ) BTS_MODUP(false, true); else BTS_MODUP(false, false); }
#undef BTS_MODUP
  return rh_launch_ok("bootstrap_modup_kernel");
}

// ---- pack / unpack of BootstrapMany: ceil(g / 4) launches of up to four tree levels each, the levels [0, 4), [4, 8), ... bottom up for the pack and
// top down for the unpack; between two launches the ceil(n / 2^lo) intermediate ciphertexts live in the caller's scratch, dense (L rows per poly) ----
static unsigned bts_ceil_shift(unsigned n, int s) { return s >= 31 ? (n ? 1u : 0u) : (unsigned)(((size_t)n + ((size_t)1 << s) - 1) >> s); }

extern "C" size_t rh_ckks_bootstrap_pack_scratch_words(int N, int L, int n, int g) {
  if (N <= 0 || L <= 0 || n <= 0 || g <= 0) return 0;
  size_t words = 0;
  for (int lo = 4; lo < g; lo += 4) words += 2 * (size_t)bts_ceil_shift((unsigned)n, lo) * (size_t)L * (size_t)N;
  return words;
}

static int bts_pack_args(rh_ring* r, int level, int n, int g, const uint64_t* in0, const uint64_t* in1, int in_rows, uint64_t* out0, uint64_t* out1,
                         int out_rows, const uint64_t* tbl, int tbl_rows, uint64_t* scratch, size_t scratch_words, unsigned cnt_in, unsigned cnt_out,
                         const char* who) {
  if (int rc = rh_scheme_args(r, level, n, 1u << RH_RING_STANDARD | 1u << RH_RING_CI, 2, who)) return rc;
  if (g < 1 || g > 16) return rh_fail(RH_ERR_ARG, "%s: %d tree levels out of range [1,16]", who, g);
  if (!in0 || !in1 || !out0 || !out1 || !tbl) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const int L = level + 1;
  if (in_rows < L || out_rows < L || tbl_rows < L)
    return rh_fail(RH_ERR_ARG, "%s: the blocks hold %d, %d and the table %d limbs per poly, the level needs %d", who, in_rows, out_rows, tbl_rows, L);
  if ((size_t)n * 2 * (size_t)L > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  const size_t N = (size_t)r->N, need = rh_ckks_bootstrap_pack_scratch_words((int)N, L, n, g);
  if (need && (!scratch || scratch_words < need)) return rh_fail(RH_ERR_ARG, "%s: the scratch holds %zu words, %d levels of %d ciphertexts need %zu", who, scratch_words, g, n, need);
  const size_t wi = (size_t)cnt_in * (size_t)in_rows * N, wo = (size_t)cnt_out * (size_t)out_rows * N;
  const RhBlock rd[3] = {{in0, wi}, {in1, wi}, {tbl, (size_t)g * (size_t)tbl_rows * N}};
  const RhBlock wr[3] = {{out0, wo}, {out1, wo}, {scratch, need}};
  const int nw = need ? 3 : 2;
  if (int rc = rh_blocks_ok(wr, nw, rd, 3, who, "an output overlaps an input or the table: the passes are not computed in place")) return rc;
  return rh_blocks_disjoint(wr, nw, who, "two outputs overlap");
}

template <bool UNPACK>
static void bts_pack_launch(int T, dim3 grid, hipStream_t st, const PackArgs& p, rh_ring* r, int L, int in_rows, int out_rows, unsigned wide,
                            unsigned narrow, const u64* tbl, int tbl_rows, int nt) {
#define BTS_PACK(T_) do { if (UNPACK) bootstrap_unpack_kernel<T_><<<grid, 256, 0, st>>>(p, (unsigned)r->N, r->d_consts, L, in_rows, out_rows, wide, narrow, tbl, tbl_rows, nt); \
                          else bootstrap_pack_kernel<T_><<<grid, 256, 0, st>>>(p, (unsigned)r->N, r->d_consts, L, in_rows, out_rows, wide, narrow, tbl, tbl_rows, nt); } while (0)
  switch (T) { case 1: BTS_PACK(1); break; case 2: BTS_PACK(2); break; case 3: BTS_PACK(3); break; default: BTS_PACK(4); break; }
#undef BTS_PACK
}

extern "C" int rh_ckks_bootstrap_pack(rh_ring* r, int level, int n, int g, const uint64_t* in0, const uint64_t* in1, int in_rows, uint64_t* out0,
                                      uint64_t* out1, int out_rows, const uint64_t* xp, int xp_rows, uint64_t* scratch, size_t scratch_words) {
  const char* who = "rh_ckks_bootstrap_pack";
  const unsigned cnt_out = n > 0 && g >= 1 && g <= 16 ? bts_ceil_shift((unsigned)n, g) : 0;
  if (int rc = bts_pack_args(r, level, n, g, in0, in1, in_rows, out0, out1, out_rows, xp, xp_rows, scratch, scratch_words, (unsigned)(n > 0 ? n : 0), cnt_out, who)) return rc;
  if (!n) return RH_OK;
  const int L = level + 1;
  const size_t N = (size_t)r->N;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * ((unsigned)n + cnt_out) * (unsigned)L);            // cache policy by the rows moved; the grid is each launch's own
  hipStream_t st = rh_stream(r);
  PackArgs p{{in0, in1}, {nullptr, nullptr}};
  int rows = in_rows;
  unsigned cnt = (unsigned)n;
  u64* sc = scratch;
  for (int lo = 0; lo < g; lo += 4) {
    const int T = g - lo < 4 ? g - lo : 4;
    const unsigned narrow = bts_ceil_shift(cnt, T);
    const bool last = lo + T == g;
    const int orows = last ? out_rows : L;
    if (last) { p.out[0] = out0; p.out[1] = out1; }
    else { p.out[0] = sc; p.out[1] = sc + (size_t)narrow * L * N; sc += 2 * (size_t)narrow * L * N; }
    bts_pack_launch<false>(T, dim3(2u * narrow * (unsigned)L, sg.grid.y), st, p, r, L, rows, orows, cnt, narrow, xp + (size_t)lo * xp_rows * N, xp_rows, sg.nt);
    p.in[0] = p.out[0]; p.in[1] = p.out[1]; rows = orows; cnt = narrow;
  }
  return rh_launch_ok("bootstrap_pack_kernel");
}

extern "C" int rh_ckks_bootstrap_unpack(rh_ring* r, int level, int n, int g, const uint64_t* in0, const uint64_t* in1, int in_rows, uint64_t* out0,
                                        uint64_t* out1, int out_rows, const uint64_t* xinv, int xinv_rows, uint64_t* scratch, size_t scratch_words) {
  const char* who = "rh_ckks_bootstrap_unpack";
  const unsigned cnt_in = n > 0 && g >= 1 && g <= 16 ? bts_ceil_shift((unsigned)n, g) : 0;
  if (int rc = bts_pack_args(r, level, n, g, in0, in1, in_rows, out0, out1, out_rows, xinv, xinv_rows, scratch, scratch_words, cnt_in, (unsigned)(n > 0 ? n : 0), who)) return rc;
  if (!n) return RH_OK;
  const int L = level + 1;
  const size_t N = (size_t)r->N;
  const RhStreamGrid sg = rh_stream_begin(r, 2u * ((unsigned)n + cnt_in) * (unsigned)L);
  hipStream_t st = rh_stream(r);
  PackArgs p{{in0, in1}, {nullptr, nullptr}};
  int rows = in_rows;
  u64* sc = scratch;
  const int top = (g - 1) / 4 * 4;                                                                   // the highest segment first
  for (int lo = top; lo >= 0; lo -= 4) {
    const int T = g - lo < 4 ? g - lo : 4;
    const unsigned narrow = bts_ceil_shift((unsigned)n, lo + T), wide = bts_ceil_shift((unsigned)n, lo);
    const bool last = lo == 0;
    const int orows = last ? out_rows : L;
    if (last) { p.out[0] = out0; p.out[1] = out1; }
    else { p.out[0] = sc; p.out[1] = sc + (size_t)wide * L * N; sc += 2 * (size_t)wide * L * N; }
    bts_pack_launch<true>(T, dim3(2u * narrow * (unsigned)L, sg.grid.y), st, p, r, L, rows, orows, wide, narrow, xinv + (size_t)lo * xinv_rows * N, xinv_rows, sg.nt);
    p.in[0] = p.out[0]; p.in[1] = p.out[1]; rows = orows;
  }
  return rh_launch_ok("bootstrap_unpack_kernel");
}

extern "C" int rh_ckks_double_angle(rh_ring* r, int level, uint64_t* c0, uint64_t* c1, int npoly, const uint64_t* s0, const uint64_t* s1) {
  const char* who = "rh_ckks_double_angle";
  if (int rc = rh_scheme_args(r, level, npoly, 1u << RH_RING_STANDARD | 1u << RH_RING_CI, 4, who)) return rc;
  if (!c0 || !c1 || !s0 || !s1) return rh_fail(RH_ERR_ARG, "%s: null argument", who);
  const int L = level + 1;
  if ((size_t)npoly * 2 * (size_t)L > 0x7fffffffu) return rh_fail(RH_ERR_ARG, "%s: too many rows for one launch", who);
  const size_t words = (size_t)npoly * L * (size_t)r->N;
  const RhBlock wr[2] = {{c0, words}, {c1, words}};
  if (((uintptr_t)c0 | (uintptr_t)c1) & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  if (int rc = rh_blocks_disjoint(wr, 2, who, "the two components overlap")) return rc;
  RhScalars s;                                                          // Add of a scalar (:82-101): the residues as they are
  if (int rc = rh_pack_scalars(r, level, s0, s1, false, &s, who)) return rc;
  if (!npoly) return RH_OK;
  const RhStreamGrid g = rh_stream_begin(r, 2u * (unsigned)npoly * (unsigned)L);
  ckks_double_angle_kernel<<<g.grid, 256, 0, rh_stream(r)>>>(c0, c1, (unsigned)r->N, r->d_consts, L, npoly, s, g.nt);
  return rh_launch_ok("ckks_double_angle_kernel");
}

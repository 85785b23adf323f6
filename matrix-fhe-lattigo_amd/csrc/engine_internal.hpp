// engine_internal.hpp -- shared between the translation units of libringhip (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include <mutex>
#include <atomic>
#include <cstdint>
#include <type_traits>
#include "../../include/ringhip.h"
#include "ring_types.hip.hpp"

#define RH_MAX_LIMBS 64

int rh_fail(int code, const char* fmt, ...);

// The one cache-policy decision of every launch site (tuning nt_streams: 0 never, 1 by working set, 2 always): non-temporal data streams
// once the bytes a launch moves reach the site's threshold.
inline bool rh_nt_policy(int nt_streams, size_t bytes, size_t threshold) { return nt_streams == 2 || (nt_streams == 1 && bytes >= threshold); }
// (each launch site's rule by name: rh_nt_rows and the lines after it, below rh_stream_grid)

// A run-time value as a template argument: f(std::integral_constant<int, S1>{}) for Lo <= S1 <= Hi, else false -- nothing is instantiated outside
// [Lo, Hi], so a range names exactly the kernels that exist -- and f(std::true_type{}) / f(std::false_type{}).  Inside f: kernel<S(), NT()><<<...>>>(...).
template <int Lo, int Hi, class F> inline bool rh_with_s1(int S1, F&& f) {
  if constexpr (Lo > Hi) return false;
  else {
    if (S1 == Lo) { f(std::integral_constant<int, Lo>{}); return true; }
    return rh_with_s1<Lo + 1, Hi>(S1, f);
  }
}
template <class F> inline void rh_with_flag(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }

struct rh_ring3n_state;   // ntt3n.hip
struct CiFold { tw2 f, b; };   // conjugate-invariant fold twiddles roots_fwd[1], roots_bwd[1] (Shoup pairs)

struct rh_ring {
  int device = 0, kind = 0, N = 0, logN = 0, L = 0;
  hipStream_t stream = nullptr;
  // host copies of what the Go side handed over (SubRing fields)
  std::vector<uint64_t> moduli, mred, bred, ninv, roots_fwd, roots_bwd, omega3n;
  std::vector<LimbConsts> hconsts;
  // device tables
  LimbConsts* d_consts = nullptr;
  tw2* d_tw_fwd = nullptr;        // natural order, Shoup pairs of RootsForward (standard form)
  tw2* d_tw_inv = nullptr;        // natural order, Shoup pairs of RootsBackward
  u64* d_tw_fwd_mont = nullptr;   // natural order, RootsForward as given (Montgomery form)
  tw2* d_twk_fwd = nullptr;       // kernel order (logN >= 12)
  tw2* d_twk_inv = nullptr;
  u64* d_twk_fwd_mont = nullptr;
  u64* d_tw_inv_mont = nullptr;   // N < 16 only: RootsBackward as given, for the non-canonical BackwardLazy of tiny rings
  CiFold* d_cifold = nullptr;     // conjugate-invariant rings only
  tw2* d_lastw = nullptr;         // psi_bwd[1] * N^-1 per limb
  LimbConsts* d_consts_r = nullptr;   // standard rings: d_consts with N^-1 replaced by N^-1 * 2^64 (rh_ring_intt_mul: the inverse
  tw2* d_lastw_r = nullptr;           //   transform of a Montgomery product restores the factor in its last stage), and lastw likewise
  // host-pointer single-limb path (rh_ntt_*): a pool of (stream, scratch) slots, one per concurrent caller
  std::mutex slot_mu;
  std::vector<struct RhHostSlot*> free_slots, all_slots;
  std::vector<struct RhPolySlot*> free_poly_slots, all_poly_slots;   // whole-Poly host path (rh_ntt_poly_*): two streams + staging per concurrent caller
  // serialises the HOST side of the entry points that touch lazily built shared state (rescale tables / scratch, the 3N
  // transform's scratch); device work stays stream-ordered.  Tables, twiddles and tuning are read-only after creation.
  std::recursive_mutex mu;
  rh_ring3n_state* s3n = nullptr;
  std::vector<void*> rescale_tables;      // per level, rescale.hip
  u64* d_rs[2] = {nullptr, nullptr}; size_t rs_words[2] = {0, 0};
  u64* d_rows = nullptr; size_t rows_words = 0;   // dense scratch of the rows-per-poly transforms that compact / expand (engine.hip: ntt_rows)
  u64* d_noise = nullptr; size_t noise_words = 0; // tables and per-workgroup partials of rh_ring_centered_moments (noise.hip)
  std::atomic<long> stats_rows_direct{0}, stats_rows_compacted{0};   // rh_ring_stats: how the rows-per-poly calls were served
  int fuse_submul = 1;            // ModDown / rescale: subtract-multiply fused into the forward tile kernel's epilogue
  int fuse_ci = 1;                // conjugate-invariant ring: the fold inside the column stages (N = 2^14 .. 2^16)
  int digit_pipeline = 1;         // key switch: all digit blocks transformed by one pipelined stream of launches (N = 2^14 .. 2^16)
  int perm_fwd_shape = 44;        // 3N permutation tiles as 10*A + B: block-order runs of 2^A words, rank-order runs of nb * 2^B words
  int perm_inv_shape = 44;        // (4, 4) measured best on MI355X for both directions (12 KiB tiles, 13 workgroups per CU): 1.06 -> 0.91 ms at the config 4 ring
  int fuse3n = 1;                 // 3N rings, b = 1: split + radix-3 layer fused with the sub-transforms' column stages
  int block_order3n = 0;          // 3N rings: device-batched NTT domain kept in block order (ntt3n.hip), no permutation pass
  int asm_cols = 1;               // N = 2^16: hand-scheduled column stages (fwd_cols16_asm_body) in place of the C++ body
  bool asm_tile = true;           // forward tile kernel: hand-scheduled body (ntt_kernels_asm.hip.hpp) vs the C++ one
  bool inv_scale = true;          // false: inverse leaves values < 4q without the N^-1 factor (3N sub-transform)
  int auto_span_rows = 2048;      // chunk_polys = -1: span size of the fused pipeline in (poly, limb) rows
  int ks_small_rows = 512;        // key switch (keyswitch.hip): blocks of at most this many (poly, limb) rows (a few ciphertexts) take the small-batch launches: every digit
                                  // in ONE extension launch and one launch pair of the transforms instead of a chain of ~10 dependent launches (0: never)
  bool pair_submul = true;        // ModDown of a ciphertext: both components' transform + subtract-multiply in ONE launch (false: one launch per component; A/B runs)
  bool one_pass = true;           // N = 2^13 / 2^14: whole limb row in one workgroup's LDS (ntt_fwd_onepass_asm / ntt_inv_onepass_asm); false: the two-pass launches
  bool one_pass_ready = false;    // ... their dynamic-LDS limit has been raised on this ring's device
  int nt_streams = 1;             // cache policy of the data streams: 1 non-temporal (the generated _NT bodies, the nt template arms) for launches beyond the
                                  // Infinity Cache, by working set; 0 default policy everywhere; 2 non-temporal at every size (tests run every variant at small shapes)
  int chunk_polys = -1;           // -1 = auto (128-poly spans for batches >= 256), 0 = whole batch in two launches, >0 = polys per span
};

// ---- launch plumbing shared by every translation unit (engine.hip) ----
int rh_launch_ok(const char* what);                          // RH_OK, or "<what> launch failed: <the runtime's error string>"
// The launch shape of the row-streaming kernels (stream_kernels.hip.hpp): one row per blockIdx.x, 1024 coefficient pairs (four per thread)
// per chunk on blockIdx.y, at most 64 chunks; nt: non-temporal streams once the rows move 512 MiB, twice the 256 MiB Infinity Cache
// (smaller working sets are re-read from the caches and run 3-6 % slower with nt).
struct RhStreamGrid { dim3 grid; int nt; };
unsigned rh_stream_chunks(const rh_ring* r);                 // blockIdx.y extent alone (a launch with rows of its own: gadget_mac_all_kernel)
RhStreamGrid rh_stream_grid(const rh_ring* r, unsigned rows);
// ---- cache policy of the NTT launch sites (engine.hip, ntt3n.hip): non-temporal data streams when ...
// span transforms (every stage, one-pass), expand + column stages, subtract-multiply, the unpipelined polymul: the rows' bytes reach 512 MiB
inline bool rh_nt_rows(const rh_ring* r, unsigned rows) { return rh_stream_grid(r, rows).nt != 0; }
// pipelined launches with hand-scheduled columns (forward / inverse fused, conjugate-invariant pair, polymul fused): the key alone -- a pipelined
// batch (several spans of ~2048 rows) is always far beyond the Infinity Cache
inline bool rh_nt_key(const rh_ring* r) { return r->nt_streams != 0; }
// pipelined launches with the compiled column stages (ntt_fwd_fused_asm<S, false>, ntt_inv_fused_asm<S, false, ...>) and the product-on-load inverse
// (MUL) arms: the kernels' template default, whatever the key says (nt_streams = 0 does not reach their default-policy form)
constexpr bool RH_NT_FUSED_DEFAULT = true;
// digit blocks (rh_std_ntt_fwd_blocks): a block's bytes reach 256 MiB, the Infinity Cache itself -- the next launch's tile stages re-read the block
inline bool rh_nt_gap(const rh_ring* r, int npoly, int Ls) { return rh_nt_policy(r->nt_streams, (size_t)npoly * (size_t)Ls * (size_t)r->N * 8, (size_t)256 << 20); }
// small-batch blocks, the strided inverse transforms (limb, rows) and rh_ring_intt_mul's unpipelined launches: default policy always (nt_streams = 2
// does not reach the non-temporal forms that exist for their tile and column kernels)
constexpr bool RH_NT_NEVER = false;
// (the 3N layer counts its own bytes: rh_3n_launch_layer)
inline RhStreamGrid rh_stream_begin(const rh_ring* r, unsigned rows) {   // ... on the ring's device, any stale error of an earlier call dropped
  (void)hipSetDevice(r->device);
  (void)hipGetLastError();
  return rh_stream_grid(r, rows);
}
// Blocks [p, p + words) as byte ranges: no written block may overlap a permuted (gathered) one, and every block moves as 16-byte pairs
struct RhBlock { const void* p; size_t words; };
inline bool rh_overlap(const RhBlock& a, const RhBlock& b) {
  const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
  return a0 < b0 + b.words * 8 && b0 < a0 + a.words * 8;
}
inline int rh_blocks_ok(const RhBlock* written, int nw, const RhBlock* read, int nr, const char* who, const char* text) {
  for (int i = 0; i < nw; ++i) {
    if ((uintptr_t)written[i].p & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
    for (int j = 0; j < nr; ++j) if (rh_overlap(written[i], read[j])) return rh_fail(RH_ERR_ARG, "%s: %s", who, text);
  }
  for (int j = 0; j < nr; ++j) if ((uintptr_t)read[j].p & 15) return rh_fail(RH_ERR_ARG, "%s: every block must be 16-byte aligned", who);
  return RH_OK;
}
// ... and no two written blocks may overlap each other
inline int rh_blocks_disjoint(const RhBlock* written, int nw, const char* who, const char* text) {
  for (int i = 0; i < nw; ++i) for (int j = i + 1; j < nw; ++j)
    if (rh_overlap(written[i], written[j])) return rh_fail(RH_ERR_ARG, "%s: %s", who, text);
  return RH_OK;
}
// Limbs 0 .. L-1 of a ring below 2^bits, the bound the `chunk`-term 128-bit sums of lc_reduce.hip.hpp are sized for (LC_MODULUS_BITS, LC_CHUNK);
// `of`: " of Q" or " of P" where the entry has both rings
inline int rh_moduli_below(const rh_ring* r, int L, int bits, int chunk, const char* who, const char* of = "") {
  for (int i = 0; i < L; ++i)
    if (r->moduli[i] >> bits) return rh_fail(RH_ERR_ARG, "%s: modulus %d%s is not below 2^%d, the bound the %d-term chunks are sized for", who, i, of, bits, chunk);
  return RH_OK;
}
// Page-locked staging of a host-built table on its way to the device (rh_ckks_linear_combination, rh_rlwe_diag_mac_qp): ONE ring of four slots
// per calling thread, each reused once the copy that read it has run (its event).  Nothing of a call lives in a handle; the slots stay with
// their thread.
struct RhStage { u64* h = nullptr; size_t words = 0; hipEvent_t done = nullptr; };
int rh_stage_slot(size_t words, RhStage** out, const char* who);                                  // the next slot, grown to at least `words` words
int rh_stage_upload(RhStage* s, u64* table_dev, size_t words, hipStream_t st, const char* who);   // h[0 .. words) -> table_dev on st; records the slot's event
// Argument checks of the scheme-level entry points (bgv.hip, ckks.hip): kinds: a mask of 1 << RH_RING_* admitted (the refusal names the scheme
// the mask belongs to); N a multiple of n_multiple
int rh_scheme_args(const rh_ring* r, int level, int npoly, unsigned kinds, int n_multiple, const char* who);
// 1, 2 or 3 components, each with an input and an output; trailing NULLs mean fewer
int rh_comps3(const void* in0, const void* in1, const void* in2, const void* out0, const void* out1, const void* out2, const char* who);
// Two per-limb host scalars -> the by-value pack (1 KiB of kernel arguments); a / b may be null (zeros).  Every scalar must be a residue of
// its limb (the refusal calls it a `noun`); mont: each is taken to Montgomery form.
struct RhScalars { u64 a[RH_MAX_LIMBS]; u64 b[RH_MAX_LIMBS]; };
int rh_pack_scalars(const rh_ring* r, int level, const u64* a, const u64* b, bool mont, RhScalars* s, const char* who, const char* noun = "scalar");

// ---- per-call context of the calling thread -----------------------------------------------------------------------
// A handle is shared by concurrent callers (ring/ring.go:192-194: transformers immutable, AtLevel views concurrency-safe), so
// nothing a call needs may live in the handle as mutable state.  The stream a launch goes to and the 3N transform's workspace
// are resolved through thread-local overrides: the host-limb path installs its slot's stream + scratch, a basis extender
// pins both of its rings to ringQ's stream for the duration of the call.
struct RhHostSlot { hipStream_t stream = nullptr; u64* buf = nullptr; size_t words = 0; };
hipStream_t rh_stream(const rh_ring* r);                     // the calling thread's override, else the ring's stream
u64* rh_ws_override(size_t words);                           // workspace of the calling thread's slot (nullptr: none installed)
struct RhCallScope {                                         // installs (stream [, workspace]) for the calling thread; restores on exit
  RhCallScope(hipStream_t st, u64* ws = nullptr, size_t ws_words = 0);
  ~RhCallScope();
  RhCallScope(const RhCallScope&) = delete;
  RhCallScope& operator=(const RhCallScope&) = delete;
 private:
  hipStream_t prev_st; bool prev_has; u64* prev_ws; size_t prev_words;
};

int rh_layout3n(const rh_ring* r);                          // 3N rings: the calling entry point's NTT-domain layout (1 block order, 0 reference), else the tuning value
struct RhLayoutScope { explicit RhLayoutScope(int layout); ~RhLayoutScope(); RhLayoutScope(const RhLayoutScope&) = delete; RhLayoutScope& operator=(const RhLayoutScope&) = delete; private: int prev; };
bool rh_ring3n_block_order_ok(const rh_ring* r);
int rh_std_ntt_launch(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse, bool lazy, int phase = 0);
int rh_ring_ntt_any(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse);
int rh_std_ntt_fwd_strided(rh_ring* r, u64* data, int npoly, int Lrows, int limb0, int Ls);
bool rh_can_ntt_digits(const rh_ring* r);
int rh_std_ntt_fwd_digits(rh_ring* r, u64* data, size_t digit_stride, int npoly, int beta, int LQ, int LP, bool lazy_out = false, int small = -1);
int rh_std_ntt_fwd_blocks(rh_ring* r, u64* data, size_t block_stride, int npoly, int nblocks, int Ls, const int* gap0, const int* gap_len,
                          bool lazy_out = false, int small = -1);
int rh_std_ntt_fwd_blocks_small(rh_ring* r, u64* data, size_t block_stride, int nblocks, int Ls, const int* gap0, const int* gap_len,
                                rh_ring* r2, u64* data2, size_t block_stride2, int nblocks2, int Ls2, int npoly, bool lazy_out);
bool rh_can_intt_limb_strided(const rh_ring* r);
int rh_std_intt_limb_strided(rh_ring* r, const u64* in, int in_rows, int limb, u64* out, int npoly);
bool rh_can_fuse_submul(const rh_ring* r);
int rh_std_ntt_submul_launch(rh_ring* r, u64* buf, int npoly, int Lrows, int limb0, const u64* y, int y_rows, u64* out, int out_rows,
                             const u64* scalars_host, bool cols_done = false, const u64* z = nullptr, int z_rows = 0);
int rh_std_ntt_submul_launch_pair(rh_ring* r, u64* buf, int npoly, int Lrows, const u64* y0, const u64* y1, int y_rows, u64* out0, u64* out1, int out_rows,
                                  const u64* scalars_host, const u64* z0, const u64* z1, int z_rows);
int rh_std_ntt_expand_cols_launch(rh_ring* r, const u64* tmp, u64* buf, int npoly, int Lrows, const void* table_dev, int mode, u64 qL);
int rh_vec_launch(rh_ring* r, int opcode, const u64* p1, const u64* p2, u64* p3, int npoly, int Lrows, int limb0,
                  const u64* s0, const u64* s1, int rows1 = 0, int rows2 = 0, int rows3 = 0, int half = 0);
int rh_std_intt_rows(rh_ring* r, const u64* in, int in_rows, u64* out, int out_rows, int npoly, int Lrows);
int rh_std_upload_tables(rh_ring* r, const std::vector<tw2>& fs, const std::vector<tw2>& is, const std::vector<u64>* mont,
                         const std::vector<tw2>& lastw);
int rh_upload_consts(rh_ring* r, const std::vector<LimbConsts>& hc);
void rh_rescale_teardown(rh_ring* r);
int rh_rescale_reserve(rh_ring* r, int npoly);
int rh_ring3n_reserve(rh_ring* r, int npoly);
void rh_3n_launch_layer(bool inverse, int S1, unsigned nblocks, hipStream_t st, const u64* in, u64* out, const N3Layer& a, int nt_streams);
// 3N-cyclotomic transform (ntt3n.hip)
int rh_ring3n_setup(rh_ring* r, std::vector<LimbConsts>& hc);
void rh_ring3n_teardown(rh_ring* r);
void rh_ring3n_set_nt_streams(rh_ring* r, int policy);
int rh_ring3n_ntt_launch(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, int limb0, bool inverse, bool block_order = false);
int rh_ring3n_reorder_launch(rh_ring* r, const u64* in, u64* out, int npoly, int Lrows, bool to_reference);

// basis extender internals shared with keyswitch.hip
struct rh_bext;
rh_ring* rh_bext_ringQ(rh_bext* be);
rh_ring* rh_bext_ringP(rh_bext* be);
int rh_bext_scratch(rh_bext* be, int which, size_t words, u64** out);
std::recursive_mutex& rh_bext_mutex(rh_bext* be);
// A basis extender carries scratch and lazily built plans, like the reference's (ring/basis_extension.go:166-183: one ShallowCopy
// per goroutine); its entry points still serialise their host side on the object, and pin both rings to ringQ's stream.
struct RhBextGuard {
  std::unique_lock<std::recursive_mutex> lk; RhCallScope sc;
  explicit RhBextGuard(rh_bext* be) : lk(rh_bext_mutex(be)), sc(rh_stream(rh_bext_ringQ(be))) {}
};
// ModDownQPtoQNTT with an optional addend: p2Q = [addend +] (p1Q - ext(p1P)) / P   (addend: the ring.Add that follows a key switch)
int rh_bext_moddown_ntt_add(rh_bext* be, int levelQ, int levelP, const u64* p1Q, const u64* p1P, u64* p2Q, int npoly, const u64* addend);
int rh_bext_moddown_ntt_pair(rh_bext* be, int levelQ, int levelP, const u64* q0, const u64* q1, const u64* p1P, u64* out0, u64* out1,
                             int npoly, const u64* add0, const u64* add1);

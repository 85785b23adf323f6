/*
 * ringhip.h -- C ABI of the MI355X-native full-RNS polynomial-ring engine.
 *
 * Drop-in boundary for the `ring` hot path of swanhong/matrix-fhe-lattigo (paths below are relative to the reference
 * root).  Plain pointers and sizes only; no C++/torch types.  Every entry point returns 0 on success or a negative
 * rh_status; rh_last_error() returns a thread-local message.  Nothing aborts or throws across this boundary: the Go
 * wrapper turns a non-zero status into the same panic/error the reference raises (ring/ntt.go:212-214,
 * ring/ring.go:321-331).  The cgo binding a maintainer adds is shown in INTEGRATION.md.
 *
 * Data model.  A "limb" is N uint64 residues; device polynomials are (poly, limb, coefficient) contiguous blocks:
 * word index ((poly*L)+limb)*N + j, with L = level+1 limbs per poly for the level a call names (the *_rows entry points take
 * blocks with more limbs per poly: views at a lower level of max-level polys).  This replaces Poly.Coeffs [][]uint64 (ring/poly.go:13-24) for device-resident
 * data; host-pointer entry points take one limb at a time exactly like the NumberTheoreticTransformer interface.
 */
#ifndef RINGHIP_H
#define RINGHIP_H
#include <stddef.h>
#include <stdint.h>
#include "ringhip_ops.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef enum rh_status {
  RH_OK = 0,
  RH_ERR_ARG = -1,        /* bad argument (short slice / bad level / N not supported) -> Go side panics like ntt.go:212 */
  RH_ERR_MODULUS = -2,    /* modulus not prime / not 1 mod NthRoot (ring/subring.go:139-145)                          */
  RH_ERR_DEVICE = -3,     /* HIP runtime error                                                                        */
  RH_ERR_NOMEM = -4,
  RH_ERR_UNSUPPORTED = -5
} rh_status;

typedef enum rh_ring_kind {
  RH_RING_STANDARD = 0,   /* Z_q[X]/(X^N+1), NumberTheoreticTransformerStandard (ring/ntt.go:31-78); N = 2^k, 8 <= N <=
                             2^17 (MinimumRingDegreeForLoopUnrolledOperations = 8, ring/ring.go:21-23, :318); for N < 16
                             BackwardLazy returns the reference's non-canonical values in [0, 2q) (ring/ntt.go:197-202) */
  RH_RING_CI = 1,         /* Z_q[X+X^-1]/(X^2N+1), NumberTheoreticTransformerConjugateInvariant (ring/ntt.go:80-124,
                             716-1311); NthRoot = 4N: root tables have 2N entries per limb; ForwardLazy returns the
                             canonical residues (inside the documented range, congruent)                             */
  RH_RING_3N = 2          /* Z_q[X]/(X^N-X^(N/2)+1), NumberTheoreticTransformer3N (ring/ntt_3n.go:21-156)             */
} rh_ring_kind;

typedef struct rh_ring rh_ring;   /* replaces ring.Ring + its SubRings' NTT state (ring/ring.go:76-89, subring.go:35-55) */

const char* rh_last_error(void);
int rh_device_count(void);

/* ---- ring construction -------------------------------------------------------------------------------------------
 * rh_ring_create: the constants handoff of NewRingWithCustomNTT / NewSubRingWithCustomNTT (ring/ring.go:314-356,
 * ring/subring.go:74-111, generateNTTConstants :129-214).  The engine never re-derives roots: it receives what the Go
 * side generated, so it is bit-identical to that Ring, including the random omega of a 3N ring.
 *   moduli[L], mred[L] (MRedConstant), bred[2L] (BRedConstant hi,lo), ninv[L] (NTTTable.NInv, Montgomery form),
 *   roots_fwd/roots_bwd: L tables of N words (NTTTable.RootsForward/RootsBackward), STANDARD rings only,
 *   omega3n[L]: primitive 3N-th root per limb (NumberTheoreticTransformer3N.psi3N), 3N rings only.            */
int rh_ring_create(rh_ring** out, int device, int kind, int N, int L, const uint64_t* moduli, const uint64_t* mred,
                   const uint64_t* bred, const uint64_t* ninv, const uint64_t* roots_fwd, const uint64_t* roots_bwd,
                   const uint64_t* omega3n);
/* rh_ring_create_auto: NewRing(N, moduli) (ring/ring.go:264-272): generates every constant on the host with the
 * reference's rules (smallest primitive root g >= 3, psi = g^((q-1)/2N), bit-reversed Montgomery tables).  For a 3N
 * ring omega = g^((q-1)/3N) (Find3NPrimitiveRoot, ring/subring.go:255-290) unless omega3n != NULL.               */
int rh_ring_create_auto(rh_ring** out, int device, int kind, int N, int L, const uint64_t* moduli,
                        const uint64_t* omega3n);
void rh_ring_destroy(rh_ring* r);
int rh_ring_n(const rh_ring* r);
int rh_ring_limbs(const rh_ring* r);
/* copies the per-limb constants back (any pointer may be NULL): what SubRing exposes (Modulus, MRedConstant,
 * BRedConstant, NInv, RootsForward, RootsBackward / omega) */
int rh_ring_get_constants(const rh_ring* r, uint64_t* moduli, uint64_t* mred, uint64_t* bred, uint64_t* ninv,
                          uint64_t* roots_fwd, uint64_t* roots_bwd, uint64_t* omega3n);
/* all device work of this ring is enqueued on `hip_stream` (a hipStream_t; NULL = the null stream) */
int rh_ring_set_stream(rh_ring* r, void* hip_stream);
int rh_ring_sync(rh_ring* r);
/* Optional: pre-sizes every lazily grown scratch of the ring (rescale, 3N transform) for batches of up to npoly polys of all
 * limbs, so that no later call allocates (hipMalloc / hipFree synchronise the device and cannot be captured in a HIP graph). */
int rh_ring_reserve(rh_ring* r, int npoly);

/* ---- concurrency (ring/ring.go:192-194: transformers are immutable, AtLevel views are concurrency-safe) ------------------
 * A ring handle may be used by any number of OS threads at once (goroutines migrate between threads):
 *   - rh_ntt_forward/_lazy/backward/_lazy: every call runs on a (stream, scratch) slot of its own taken from a pool in the
 *     handle; calls on the same or different limbs proceed in parallel and never share device memory;
 *   - the device-batched entry points only ENQUEUE on the ring's stream: concurrent callers are serialised in stream order;
 *     the few that use lazily built shared state (rescale, the 3N transform's workspace) take a lock for the enqueue;
 *   - tables and twiddles are read-only after creation; rh_ring_set_stream / rh_ring_set_tuning configure the handle and are
 *     not meant to race with calls.
 * rh_bext / rh_kshard objects carry scratch and plans like the reference's BasisExtender (one ShallowCopy per goroutine,
 * ring/basis_extension.go:166-183): one object per thread is the intended use; their entry points still lock the object,
 * so sharing one is safe, merely serial.  Several such objects may share the same rings.
 * rh_last_error() is thread-local: read it on the thread that got the status (the cgo wrapper locks the OS thread). */

/* ---- device memory (plain hipMalloc'd words; any device pointer from another allocator, e.g. torch, is accepted) */
int rh_dev_alloc(rh_ring* r, size_t words, uint64_t** dptr);
int rh_dev_free(rh_ring* r, uint64_t* dptr);
int rh_dev_upload(rh_ring* r, uint64_t* dst_dev, const uint64_t* src_host, size_t words);
int rh_dev_download(rh_ring* r, uint64_t* dst_host, const uint64_t* src_dev, size_t words);
/* Poly.CopyLvl (ring/poly.go) on device blocks: limbs 0..level of every poly, blocks with src_rows / dst_rows >= level+1 limbs per poly;
 * asynchronous on the ring's stream */
int rh_ring_copy_rows(rh_ring* r, uint64_t* dst_dev, int dst_rows, const uint64_t* src_dev, int src_rows, int npoly, int level);

/* ---- NumberTheoreticTransformer interface, one limb, host pointers (ring/ntt.go:17-22; SubRing.NTT/NTTLazy/INTT/
 * INTTLazy ring/subring_ops.go:235-252).  p1 and p2 hold N words each and may alias.  Synchronous.
 *   Forward      -> canonical [0,q)                       (NTTStandard, ntt.go:174-177 / 3N Forward ntt_3n.go:82-109)
 *   ForwardLazy  -> exactly the reference's lazy representatives in [0,6q-2] (NTTStandardLazy :180-182)
 *   Backward, BackwardLazy -> canonical [0,q)             (INTTStandard :185-194, INTTStandardLazy :197-206, N>=16) */
int rh_ntt_forward(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2);
int rh_ntt_forward_lazy(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2);
int rh_ntt_backward(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2);
int rh_ntt_backward_lazy(rh_ring* r, int limb, const uint64_t* p1, uint64_t* p2);

/* ---- Ring.NTT / NTTLazy / INTT / INTTLazy on a whole host Poly in ONE call (ring/ntt.go:127-152: the loop over
 * r.SubRings[:level+1] calling s.NTT(p1.Coeffs[i], p2.Coeffs[i]); Poly.Coeffs is [][]uint64, ring/poly.go:13-24).
 * p1 / p2: host arrays of level+1 limb pointers (N words each; p2[i] may alias p1[i]); limb i uses modulus i.  Same results as level+1
 * calls of rh_ntt_forward / _lazy / backward / _lazy, but pipelined: up to four limb groups alternate between two streams (upload of
 * group g under the transform and download of group g-1), one batched launch pair per group, one host synchronisation.  Limbs in
 * page-locked memory (rh_host_alloc / rh_host_register) are DMA'd where they lie; pageable limbs are staged through page-locked buffers
 * owned by the handle.  Synchronous; any number of OS threads may call it on one handle (each call takes a slot of its own).
 * The cgo wrapper pins the Go slices for the call (runtime.Pinner) and passes a C array of their data pointers. */
int rh_ntt_poly_forward(rh_ring* r, int level, const uint64_t* const* p1, uint64_t* const* p2, int lazy);
int rh_ntt_poly_backward(rh_ring* r, int level, const uint64_t* const* p1, uint64_t* const* p2, int lazy);
/* Page-locked host memory for Poly.Coeffs backing arrays (a Go slice over it: unsafe.Slice): such limbs skip the staging copy.
 * rh_host_register page-locks memory the caller already owns (it must stay allocated and unmoved until rh_host_unregister).  WHOLE 4 KiB PAGES only
 * (pointer and byte count multiples of 4096, else RH_ERR_ARG), pages
 * the caller owns exclusively (a page-aligned mapping or allocation: a Go slice of a megabyte or more sits in spans of its own): the runtime pins and
 * maps every page the range touches, and a page shared with unrelated heap objects drags those into the GPU mapping for the registration's lifetime. */
int rh_host_alloc(size_t words, uint64_t** hptr);
int rh_host_free(uint64_t* hptr);
int rh_host_register(uint64_t* hptr, size_t words);
int rh_host_unregister(uint64_t* hptr);

/* ---- Ring.NTT / NTTLazy / INTT / INTTLazy on device-resident batches (ring/ntt.go:127-152).
 * in/out: npoly polys of (level+1) limbs each, limbs 0..level of the ring (Ring.AtLevel view); may alias.
 * Asynchronous on the ring's stream. */
int rh_ring_ntt(rh_ring* r, const uint64_t* in_dev, uint64_t* out_dev, int npoly, int level, int lazy);
int rh_ring_intt(rh_ring* r, const uint64_t* in_dev, uint64_t* out_dev, int npoly, int level, int lazy);

/* Ring.NTT on several blocks in one call (device-API extension: e.g. both operands of a product, schemes/ckks/evaluator.go:821-834
 * after the two NTTs).  in[k] / out[k]: block k, npoly[k] polys of (level+1) limbs; each pair may alias.  Same results as nblocks
 * rh_ring_ntt calls; for two-pass standard rings (N >= 8192) the software pipeline of the fused launches runs through the block
 * boundaries.  The pointer arrays are host arrays of device pointers, read before the call returns. */
int rh_ring_ntt_many(rh_ring* r, const uint64_t* const* in_dev, uint64_t* const* out_dev, const int* npoly, int nblocks, int level);

/* The same on blocks that carry MORE limbs per poly than the level they are used at (in_rows / out_rows limbs per poly, each
 * >= level+1): ring.AtLevel(level) on max-level polys and buffers (ring/ring.go:192-213), the idiomatic use inside the reference's
 * evaluators.  Limbs 0..level of every poly are transformed, the others are untouched.  With rows == level+1 this IS rh_ring_ntt /
 * rh_ring_intt. */
/* (round 3: every shape is ONE batched transform.  Standard rings take both row strides inside the kernels (every N, forward and inverse);
 * conjugate-invariant and 3N rings compact the leading limbs with one strided device copy on the way in and / or out.  rh_ring_stats(ring, "rows_direct" | "rows_compacted" |
 * "rows_poly_by_poly", &n) counts how the calls of a handle were served.) */
int rh_ring_stats(const rh_ring* r, const char* key, long* value);
int rh_ring_ntt_rows(rh_ring* r, const uint64_t* in_dev, int in_rows, uint64_t* out_dev, int out_rows, int npoly, int level, int lazy);
int rh_ring_intt_rows(rh_ring* r, const uint64_t* in_dev, int in_rows, uint64_t* out_dev, int out_rows, int npoly, int level, int lazy);

/* INTT of a pointwise product, NTT-domain inputs: out = INTT(a . b), the values of ring.MForm(a, t); ring.MulCoeffsMontgomery(t, b, c);
 * ring.INTT(c, c) (the degree-0 part of ckks mulRelin, schemes/ckks/evaluator.go:821-834, and BASELINE config 3) -- canonical, hence
 * bit-identical -- with the product formed on load by the inverse transform's first kernel: 24 bytes per coefficient less traffic
 * than the three calls.  a, b: npoly polys of level+1 limbs, canonical or lazy (< 2q); out may alias either.  Standard rings. */
int rh_ring_intt_mul(rh_ring* r, const uint64_t* a_dev, const uint64_t* b_dev, uint64_t* out_dev, int npoly, int level);

/* The whole of BASELINE config 3 from COEFFICIENT-domain operands: out = INTT(NTT(a) . NTT(b)), the values of ring.NTT(a); ring.NTT(b);
 * ring.MForm; ring.MulCoeffsMontgomery; ring.INTT (schemes/ckks/evaluator.go:821-834 around a fresh product) -- canonical, hence bit-identical.
 * The forward tile stages of both operands, their product and the inverse tile stages run as ONE kernel per 4096-coefficient tile: NTT(a), NTT(b)
 * and the product never reach memory (72 instead of 104 bytes per coefficient).  a and b are CONSUMED: they are transformed in place as far as
 * their column stages and do not hold NTT(a) / NTT(b) afterwards (a caller that needs those keeps rh_ring_ntt_many + rh_ring_intt_mul).  out may
 * alias a or b; a != b.  Standard rings, 2^13 <= N <= 2^17 (otherwise RH_ERR_UNSUPPORTED). */
int rh_ring_polymul(rh_ring* r, uint64_t* a_dev, uint64_t* b_dev, uint64_t* out_dev, int npoly, int level);

/* 3N rings: NTT-domain blocks between the reference's ascending-totative order and block order (see ntt3n_block_order):
 * to_reference = 1: block order -> reference order, 0: the reverse.  Out of place (in != out). */
int rh_ring_ntt3n_reorder(rh_ring* r, const uint64_t* in_dev, uint64_t* out_dev, int npoly, int level, int to_reference);

/* 3N rings, for hosts that TAG their device polys with the NTT-domain layout (matrix-fhe-lattigo_amd/ringhip.py DevicePoly.layout, the Go
 * wrapper's DevicePoly.BlockOrder) instead of switching the whole handle with the tuning key: the layout of the NTT side of the call is an
 * argument (block_order 1: block order, 0: the reference's order), so concurrent callers of one handle may differ.  rows as rh_ring_ntt_rows;
 * canonical outputs.  rh_ring_ntt3n_block_order_supported: 1 for 3N rings with N = 3 * 2^k, k >= 13.  Other ring kinds ignore the argument. */
int rh_ring_ntt3n_block_order_supported(const rh_ring* r);
int rh_ring_ntt_layout(rh_ring* r, const uint64_t* in_dev, int in_rows, uint64_t* out_dev, int out_rows, int npoly, int level, int inverse, int block_order);
int rh_ring_div_by_last_modulus_many_ntt_layout(rh_ring* r, int round, int level, int nb, const uint64_t* p0_dev, uint64_t* p1_dev, int p1_rows, int npoly,
                                                int block_order);

/* profiling aid: phase 0 = whole transform, 1 = column kernel only, 2 = tile kernel only (N >= 8192) */
int rh_ring_ntt_phase(rh_ring* r, const uint64_t* in_dev, uint64_t* out_dev, int npoly, int level, int inverse, int phase);
/* Tuning knobs: performance only, never results (each non-default setting is covered by a parity test).  Unknown keys
 * return RH_ERR_ARG.  Defaults are the measured optimum on MI355X.  Set them before the handle is
 * shared between threads: they are plain fields read by every call.
 *   chunk_polys     polys per span of the fused (column + tile) pipeline: -1 auto (auto_span_rows), 0 = two launches per batch
 *   auto_span_rows  span size of the auto rule in (poly, limb) rows (2048)
 *   asm_tile / asm_cols   1: generated hand-scheduled bodies (default), 0: the C++ kernels
 *   fuse_submul     1: ModDown / rescale subtract-multiply in the forward tile kernel's epilogue (default)
 *   ks_small_rows   n: key switches whose blocks have at most n (poly, limb) rows (up to ~20 ciphertexts at 24 limbs) run every digit of the decomposition in ONE
 *                   basis-extension launch and the transforms of all digit blocks of BOTH rings in one launch pair instead of digit by digit (default 512; 0: never).
 *                   One ciphertext at N = 2^16, 24 + 6 limbs: 0.38 -> 0.24 ms; eight: 1.26 -> 1.15 ms; from ~24 ciphertexts on the pipelined stream of launches
 *                   is as fast or faster (set on ringQ)
 *   one_pass        1: N = 2^13 / 2^14 (and the inverse at N = 4096) keep the whole limb row in one workgroup's LDS between the column and the tile
 *                   stages: one HBM pass per transform instead of two (default); 0: the two-pass launches
 *   fuse_ci         1: conjugate-invariant rings fold inside the column stages instead of in a pass of their own (default; N = 2^14..2^16)
 *   digit_pipeline  1: key switch transforms all digit blocks with one software-pipelined stream of launches (default; N = 2^14..2^16)
 *   fuse3n          1: 3N rings, split + radix-3 layer fused with the sub-transforms' column stages (default)
 *   perm_fwd_shape / perm_inv_shape  3N permutation tile as 10*A + B: block-order runs of 2^A words, rank-order runs of nb * 2^B words
 *   nt_streams      cache policy of the data streams (a hint: every value gives the same bits).  1: non-temporal once a launch's working set
 *                   passes its threshold (512 MiB; 256 MiB for the key switch's digit pipeline), and in the pipelined launches, which only exist for
 *                   batches far beyond the Infinity Cache (default); 0: default policy everywhere (A/B runs: bench.py --tune nt_streams=0);
 *                   2: non-temporal at every size (tests/test_gpu_cache_policy.py runs every variant at test sizes).  Other values: RH_ERR_ARG.
 *                   3N rings hand the value on to their radix-2 sub-ring
 * One key changes a LAYOUT, not a value (3N rings, N = 3*2^k >= 24576, default 0):
 *   ntt3n_block_order  1: rh_ring_ntt / rh_ring_intt keep the NTT domain in "block order" (slot j of block c of the radix-2
 *                   sub-transforms at word c*N/6 + j) instead of the Go transformer's ascending-totative order
 *                   (ring/ntt_3n.go:82-109, :235-243).  Every NTT-domain operation of a ring is coefficient-wise, so NTT ->
 *                   pointwise -> INTT chains (matrix_ckks.Evaluator.Mul) give the same coefficient-domain bits with one pass less
 *                   per transform; NTT-domain data that crosses the host boundary is converted with rh_ring_ntt3n_reorder.  The
 *                   per-limb host interface (rh_ntt_*) always speaks the reference order. */
int rh_ring_set_tuning(rh_ring* r, const char* key, long value);

/* ---- element-wise family (ring/vec_ops.go via ring/operations.go loops): p3 = op(p1, p2 [, p3]) on npoly polys of
 * (level+1) limbs.  s0/s1: per-limb scalar arrays of level+1 words on the HOST (NULL = unused), e.g. the RNSScalar of
 * MulRNSScalarMontgomery (ring/operations.go).  Asynchronous. */
int rh_ring_vec_op(rh_ring* r, int opcode, const uint64_t* p1_dev, const uint64_t* p2_dev, uint64_t* p3_dev, int npoly,
                   int level, const uint64_t* s0_host, const uint64_t* s1_host);

/* rows-per-poly form (see rh_ring_ntt_rows): every operand block with its own limb count >= level+1; one launch, the three row
 * strides inside the kernel */
int rh_ring_vec_op_rows(rh_ring* r, int opcode, const uint64_t* p1_dev, int rows1, const uint64_t* p2_dev, int rows2, uint64_t* p3_dev,
                        int rows3, int npoly, int level, const uint64_t* s0_host, const uint64_t* s1_host);

/* p2 = ONE row of N words on the device used for every (poly, limb): Ring.MulByVectorMontgomery / ...ThenAddLazy (ring/operations.go:366-377)
 * with RH_OP_MUL_MONT / RH_OP_MUL_MONT_THEN_ADD_LAZY (any opcode with a second operand) */
int rh_ring_vec_op_bcast(rh_ring* r, int opcode, const uint64_t* p1_dev, int rows1, const uint64_t* vector_dev, uint64_t* p3_dev, int rows3,
                         int npoly, int level);
/* a one-operand scalar opcode with one RNS scalar for coefficients [0, N/2) and another for [N/2, N): Ring.AddDoubleRNSScalar,
 * SubDoubleRNSScalar, MulDoubleRNSScalar(ThenAdd) (ring/operations.go:167-184, 250-266); scalars as the opcode takes them */
int rh_ring_vec_op_halves(rh_ring* r, int opcode, const uint64_t* p1_dev, uint64_t* p3_dev, int npoly, int level,
                          const uint64_t* s_lo_host, const uint64_t* s_hi_host);
/* Ring.Shift (:278-282): p2[j] = p1[(j + k) mod N]; Ring.MultByMonomial (:306-363): p2 = p1 * X^k with the reference's representatives
 * (q - 0 is written as q).  Every limb 0..level of dense blocks; out of place. */
int rh_ring_shift(rh_ring* r, int level, const uint64_t* in_dev, uint64_t* out_dev, int k, int npoly);
int rh_ring_mult_by_monomial(rh_ring* r, int level, const uint64_t* in_dev, uint64_t* out_dev, int k, int npoly);
/* Ring.AutomorphismNTTWithIndex / AutomorphismNTTWithIndexThenAddLazy (ring/automorphism.go:50-117): out[j] (=|+=) in[index[j]] on every limb
 * 0..level; index_dev: the caller's lookup table of N words ON THE DEVICE (e.g. AutomorphismNTTIndex, :12-34); out of place */
int rh_ring_automorphism_ntt_index(rh_ring* r, int level, const uint64_t* in_dev, const uint64_t* index_dev, uint64_t* out_dev, int npoly,
                                   int add_lazy);
/* Standard <-> conjugate-invariant bridges (ring/conjugate_invariant.go; callers: schemes/ckks/bridge.go:82-83, 116-117,
 * core/rlwe/keygenerator.go:213).  Dense blocks, every limb 0..level, out of place; n = the SMALLER of the two degrees.
 *   rh_ring_unfold_ci_to_standard (:8-26)   r: the standard ring of degree 2n.  ci: rows of n words, std: rows of 2n words;
 *                                           std[j] = ci[j], std[n + k] = ci[n - 1 - k]
 *   rh_ring_fold_standard_to_ci (:31-49)    r: the conjugate-invariant ring of degree n.  std: rows of 2n words, ci: rows of n words,
 *                                           index_dev: n words on the device with values < 2n (AutomorphismNTTIndex of the standard ring);
 *                                           ci[j] = CRed(std[index[j]] + std[j])
 *   rh_ring_pad_default_to_ci (:52-80)      r: a ring of degree n (level and moduli).  std: rows of n words, ci: rows of 2n words of which only
 *                                           the first n are written, with the reference's in-place loop reproduced: is_ntt: ci[k] = std[k],
 *                                           ci[n-1-k] = std[k] for k < n/2;  else ci[0] = 0, ci[k] = std[k] (1 <= k < n/2),
 *                                           ci[n/2] = q - std[n/2], ci[n-k] = q - std[k] (1 <= k < n/2; q - 0 is written as q) */
int rh_ring_unfold_ci_to_standard(rh_ring* r, int level, const uint64_t* ci_dev, uint64_t* std_dev, int npoly);
int rh_ring_fold_standard_to_ci(rh_ring* r, int level, const uint64_t* std_dev, const uint64_t* index_dev, uint64_t* ci_dev, int npoly);
int rh_ring_pad_default_to_ci(rh_ring* r, int level, const uint64_t* std_dev, int is_ntt, uint64_t* ci_dev, int npoly);

/* The tail of DomainSwitcher.ComplexToReal (schemes/ckks/bridge.go:79-83) as one launch over both components of a batch: the Add of the
 * gadget product's first output g0 with c0 over rows of 2n words and the two FoldStandardToConjugateInvariant calls,
 *   out0[j] = CRed(CRed(g0[index[j]] + c0[index[j]]) + CRed(g0[j] + c0[j])),  out1[j] = CRed(g1[index[j]] + g1[j]),  j < n.
 * r: a ring of degree n with the level's moduli (the conjugate-invariant ring); g0, g1, c0: (npoly, level+1, 2n) canonical words; out0, out1:
 * (npoly, level+1, n), disjoint from the inputs; index_dev as for rh_ring_fold_standard_to_ci.  The words of the composed calls. */
int rh_ckks_bridge_fold_tail(rh_ring* r, int level, const uint64_t* g0_dev, const uint64_t* g1_dev, const uint64_t* c0_dev,
                             const uint64_t* index_dev, uint64_t* out0_dev, uint64_t* out1_dev, int npoly);

/* ---- RNS rescale (ring/scaling.go): divide by the last modulus, `nb` times.  round = 0: floored, 1: rounded.
 * p0: npoly polys of level+1 limbs; p1: npoly polys of p1_rows >= level+1-nb limbs (limbs 0..level-nb are written).
 *   rh_ring_div_by_last_modulus_many      coefficient domain: DivFloorByLastModulus(:21-28) / DivRoundByLastModulus
 *                                          (:112-126) and their Many forms (:56-88, :160-192); p0 is modified in
 *                                          place exactly as the reference modifies its input / buffer
 *   rh_ring_div_by_last_modulus_many_ntt  NTT domain: DivFloorByLastModulusManyNTT(:32-52), DivRoundByLastModulusNTT
 *                                          (:92-108), DivRoundByLastModulusManyNTT(:130-156); p0 is not modified
 * All three ring types (the 3N ring is what schemes/matrix_ckks/evaluator.go:235 rescales on); the fused kernels are the standard ring's. */
int rh_ring_div_by_last_modulus_many(rh_ring* r, int round, int level, int nb, uint64_t* p0_dev, uint64_t* p1_dev, int p1_rows, int npoly);
int rh_ring_div_by_last_modulus_many_ntt(rh_ring* r, int round, int level, int nb, const uint64_t* p0_dev, uint64_t* p1_dev, int p1_rows, int npoly);

/* Degree-1 x degree-1 tensoring in one pass.  mform_first = 1: ckks mulRelin (schemes/ckks/evaluator.go:821-834),
 * c0 = MRed(MForm(a0), b0), c1 = CRed(MRed(MForm(a0), b1) + MRed(MForm(a1), b0)), c2 = MRed(MForm(a1), b1) -- the values the six
 * ring calls of the reference produce.  mform_first = 0: matrix_ckks.Evaluator.Mul (schemes/matrix_ckks/evaluator.go:166-173),
 * the same without the MForm (its four ring calls).  All blocks: npoly polys of level+1 limbs, NTT domain; any ring kind. */
int rh_ring_tensor_degree1(rh_ring* r, const uint64_t* a0_dev, const uint64_t* a1_dev, const uint64_t* b0_dev, const uint64_t* b1_dev,
                           uint64_t* c0_dev, uint64_t* c1_dev, uint64_t* c2_dev, int npoly, int level, int mform_first);

/* ---- Galois automorphisms X -> X^gen (ring/automorphism.go), standard and conjugate-invariant rings, never in place.
 *   conjugate-invariant rings: the NTT-domain table is built over NthRoot = 4N (gen must be 1 mod 4, else the reference's look-up
 *   runs out of range); the coefficient-domain form is the Z[X+X^-1] branch (:131-156)
 *   rh_ring_automorphism_ntt: AutomorphismNTT (:39-47) / AutomorphismNTTWithIndex (:52-81); add_lazy != 0:
 *                             AutomorphismNTTWithIndexThenAddLazy (:86-117) (out += permuted in, wrapping)
 *   rh_ring_automorphism:     Automorphism (:121-176, standard ring branch), coefficient domain with sign flips   */
int rh_ring_automorphism_ntt(rh_ring* r, int level, const uint64_t* in_dev, uint64_t gen, uint64_t* out_dev, int npoly, int add_lazy);
int rh_ring_automorphism(rh_ring* r, int level, const uint64_t* in_dev, uint64_t gen, uint64_t* out_dev, int npoly);

/* ---- RNS basis extension (ring/basis_extension.go).  A basis extender pairs a Q ring and a P ring
 * (NewBasisExtender :52-79).  All polys device-resident, limbs 0..levelQ / 0..levelP, npoly polys.  Asynchronous. */
typedef struct rh_bext rh_bext;
int rh_bext_create(rh_bext** out, rh_ring* ringQ, rh_ring* ringP);
void rh_bext_destroy(rh_bext* be);
/* Optional: pre-sizes the extender's scratch for key switches / ModDowns of up to npoly polys at the rings' top levels. */
int rh_bext_reserve(rh_bext* be, int npoly);
int rh_bext_modup_q_to_p(rh_bext* be, int levelQ, int levelP, const uint64_t* polQ, uint64_t* polP, int npoly);   /* :188-200 */
int rh_bext_modup_p_to_q(rh_bext* be, int levelP, int levelQ, const uint64_t* polP, uint64_t* polQ, int npoly);   /* :205-217 */
int rh_bext_moddown_qp_to_q(rh_bext* be, int levelQ, int levelP, const uint64_t* p1Q, const uint64_t* p1P,
                            uint64_t* p2Q, int npoly);                                                            /* :223-234 */
int rh_bext_moddown_qp_to_q_ntt(rh_bext* be, int levelQ, int levelP, const uint64_t* p1Q, const uint64_t* p1P,
                                uint64_t* p2Q, int npoly);                                                        /* :241-258 */
int rh_bext_moddown_qp_to_p(rh_bext* be, int levelQ, int levelP, const uint64_t* p1Q, const uint64_t* p1P,
                            uint64_t* p2P, int npoly);                                                            /* :264-278 */
/* Decomposer.DecomposeAndSplit (:381-502): digit `digit` of p0Q -> p1Q (levelQ+1 limbs), p1P (levelP+1 limbs) */
int rh_bext_decompose_and_split(rh_bext* be, int levelQ, int levelP, int nbPi, int digit, const uint64_t* p0Q,
                                uint64_t* p1Q, uint64_t* p1P, int npoly);


/* ---- hybrid key-switch gadget product: rlwe.Evaluator.GadgetProduct.  This entry: NTT-domain ciphertext, levelP >= 1
 * (core/rlwe/evaluator_gadget_product.go:16-30) = gadgetProductMultiplePLazy (:122-188) + ModDown NTT->NTT (:33-46).
 * cx: npoly polys of levelQ+1 limbs (NTT domain).  evkQ / evkP: GadgetCiphertext.Value[i][0][c].Q / .P
 * (core/rlwe/gadgetciphertext.go:17-45) laid out [digit i < beta_key][component c < 2][all limbs of the ring][N], NTT
 * domain, Montgomery form, shared by every poly of the batch.  ct0/ct1: npoly polys of levelQ+1 limbs (NTT domain). */
int rh_bext_gadget_product(rh_bext* be, int levelQ, int levelP, const uint64_t* cx_dev, const uint64_t* evkQ_dev,
                           const uint64_t* evkP_dev, int beta_key, uint64_t* ct0_dev, uint64_t* ct1_dev, int npoly);

/* The same with the ring.Add that follows it in Relinearize (core/rlwe/evaluator_evaluationkey.go:144-146), mulRelin
 * (schemes/ckks/evaluator.go:850-852), applyEvaluationKey (:105-112) and Automorphism (evaluator_automorphism.go:42-44):
 * ct_c = add_c + product_c, canonical.  add0 / add1 may be NULL and may alias ct0 / ct1. */
int rh_bext_gadget_product_then_add(rh_bext* be, int levelQ, int levelP, const uint64_t* cx_dev, const uint64_t* evkQ_dev,
                                    const uint64_t* evkP_dev, int beta_key, const uint64_t* add0_dev, const uint64_t* add1_dev,
                                    uint64_t* ct0_dev, uint64_t* ct1_dev, int npoly);

/* The same for a COEFFICIENT-domain ciphertext (ct.IsNTT == false; :114-118, :139-143 and ModDown INTT -> INTT :62-66): cx, ct0, ct1 in
 * the coefficient domain, levelP >= 1. */
int rh_bext_gadget_product_coeff(rh_bext* be, int levelQ, int levelP, const uint64_t* cx_dev, const uint64_t* evkQ_dev,
                                 const uint64_t* evkP_dev, int beta_key, uint64_t* ct0_dev, uint64_t* ct1_dev, int npoly);

/* Gadget ciphertexts with at most ONE P modulus, optionally with a power-of-two decomposition on top of the RNS one:
 * gadgetProductSinglePAndBitDecompLazy (core/rlwe/evaluator_gadget_product.go:190-324) + ModDown (:33-98).
 *   levelP = 0: one P modulus (be has a P ring);  levelP = -1: none (be created with ringP = NULL, evkP = NULL, needs pw2 > 0)
 *   pw2 = GadgetCiphertext.BaseTwoDecomposition (0: RNS digits only); digits_per_limb[i] = len(Value[i]) for i <= levelQ (host array,
 *   NULL when pw2 = 0); key rows: row e = (sum of digits_per_limb before limb i) + j holds Value[i][j]: evkQ / evkP are
 *   [row][component < 2][all limbs of the ring][N] like rh_bext_gadget_product, key_rows = number of rows supplied
 *   cx_is_ntt: the ciphertext's domain (cx, ct0 and ct1 alike), as ct.IsNTT in the reference. */
int rh_bext_gadget_product_single_p(rh_bext* be, int levelQ, int levelP, const uint64_t* cx_dev, int cx_is_ntt, int pw2,
                                    const int* digits_per_limb, const uint64_t* evkQ_dev, const uint64_t* evkP_dev, int key_rows,
                                    uint64_t* ct0_dev, uint64_t* ct1_dev, int npoly);
/* The same WITHOUT the closing ModDown / CopyLvl (the accumulators after the closing Reduce: canonical residues modulo Q in ctQ0 / ctQ1 and,
 * for levelP = 0, modulo P in ctP0 / ctP1; NTT domain), for callers that sum several products under one ModDown: rgsw's external product.
 * raw_limb_digits != 0: the digit form of externalProductInPlaceSinglePAndBitDecomp (core/rgsw/evaluator.go:119-186) -- MaskVec of limb i
 * under every modulus even when pw2 = 0 (mask = all ones), where rlwe's routine calls DecomposeAndSplit. */
int rh_bext_gadget_product_single_p_lazy(rh_bext* be, int levelQ, int levelP, const uint64_t* cx_dev, int cx_is_ntt, int pw2,
                                         const int* digits_per_limb, const uint64_t* evkQ_dev, const uint64_t* evkP_dev, int key_rows,
                                         int raw_limb_digits, uint64_t* ctQ0_dev, uint64_t* ctQ1_dev, uint64_t* ctP0_dev, uint64_t* ctP1_dev, int npoly);

/* Hoisted form (rotations of one ciphertext share the decomposition).  Evaluator.DecomposeNTT
 * (core/rlwe/evaluator_gadget_product.go:431-453): c2 (levelQ+1 limbs, NTT or coefficient domain per c2_is_ntt) ->
 * decompQ [beta][npoly][levelQ+1][N], decompP [beta][npoly][levelP+1][N], NTT domain, beta = BaseRNSDecompositionVectorSize. */
int rh_bext_decompose_ntt(rh_bext* be, int levelQ, int levelP, const uint64_t* c2_dev, int c2_is_ntt, uint64_t* decompQ_dev,
                          uint64_t* decompP_dev, int npoly);
/* Evaluator.GadgetProductHoisted (:326-349, :373-429) on such a decomposition; key and outputs as rh_bext_gadget_product */
int rh_bext_gadget_product_hoisted(rh_bext* be, int levelQ, int levelP, const uint64_t* decompQ_dev, const uint64_t* decompP_dev,
                                   const uint64_t* evkQ_dev, const uint64_t* evkP_dev, int beta_key, uint64_t* ct0_dev,
                                   uint64_t* ct1_dev, int npoly);

/* Evaluator.GadgetProductHoistedLazy (core/rlwe/evaluator_gadget_product.go:351-429): the product WITHOUT the ModDown -- accumulators
 * modulo Q (ctQ0 / ctQ1, levelQ+1 limbs) and modulo P (ctP0 / ctP1, levelP+1 limbs), canonical, NTT domain, still scaled by P: what
 * AutomorphismHoistedLazy and the linear transformations accumulate before ONE ModDown.
 * rh_bext_moddown_qp_to_q_ntt_pair: Evaluator.ModDown (:33-46) NTT -> NTT on both components (ct_c may alias ctQ_c). */
int rh_bext_gadget_product_hoisted_lazy(rh_bext* be, int levelQ, int levelP, const uint64_t* decompQ_dev, const uint64_t* decompP_dev,
                                        const uint64_t* evkQ_dev, const uint64_t* evkP_dev, int beta_key, uint64_t* ctQ0_dev,
                                        uint64_t* ctQ1_dev, uint64_t* ctP0_dev, uint64_t* ctP1_dev, int npoly);
int rh_bext_moddown_qp_to_q_ntt_pair(rh_bext* be, int levelQ, int levelP, const uint64_t* ctQ0_dev, const uint64_t* ctQ1_dev,
                                     const uint64_t* ctP0_dev, const uint64_t* ctP1_dev, uint64_t* ct0_dev, uint64_t* ct1_dev, int npoly);

/* the same with the ring.Add of AutomorphismHoisted (core/rlwe/evaluator_automorphism.go:88-89): ct_c = add_c + product_c */
int rh_bext_gadget_product_hoisted_then_add(rh_bext* be, int levelQ, int levelP, const uint64_t* decompQ_dev, const uint64_t* decompP_dev,
                                            const uint64_t* evkQ_dev, const uint64_t* evkP_dev, int beta_key, const uint64_t* add0_dev,
                                            const uint64_t* add1_dev, uint64_t* ct0_dev, uint64_t* ct1_dev, int npoly);

/* ---- sums of rotations (core/rlwe/inner_sum.go).  Standard rings (RH_ERR_UNSUPPORTED for 3N and conjugate-invariant rings), NTT domain, dense
 * blocks of npoly polys with levelQ+1 / levelP+1 limbs, canonical residues in and out; the Galois element is any odd number, taken modulo 2N,
 * and the NTT-domain index map (ring/automorphism.go:12-35) is computed in the kernel.
 *   rh_rlwe_rotate_accumulate_qp  the tail of AutomorphismHoistedLazy (core/rlwe/evaluator_automorphism.go:107-160: MulScalarBigint, Add and the four
 *                                 AutomorphismNTTWithIndex passes over the Q and P parts) and the ringQP.Add that follows it in PartialTracesSum
 *                                 (inner_sum.go:245-246), ONE launch over both components, the Q and the P rows and every poly:
 *                                   acc_c[j] = [first ? 0 : acc_c[j]] + tmp_c[index(j)] + [c == 0, Q rows] (P mod q_i) * ct0[index(j)]
 *                                 tmp: the output of rh_bext_gadget_product_hoisted_lazy; ct0: ctIn.Value[0]; first != 0: acc is written, not read
 *                                 (the `copy` flag, inner_sum.go:236-240).  levelP >= 0.  No acc block may overlap a tmp block or ct0, and every block is
 *                                 16-byte aligned (RH_ERR_ARG otherwise: the kernels move 16-byte pairs).
 *   rh_rlwe_rotate_add_q          the two AutomorphismNTTWithIndex calls that end AutomorphismHoisted (evaluator_automorphism.go:90-95) and the
 *                                 ringQ.Add pair that follows them (inner_sum.go:279-280; Trace :94-95), one launch: ct_c[j] = ct_c[j] + tmp_c[index(j)]
 *                                 mod q_i, in place on ct; tmp may not overlap ct; 16-byte aligned blocks.
 *   rh_rlwe_partial_traces_sum    the whole of Evaluator.PartialTracesSum (inner_sum.go:152-291): out = sum_{i < n} phi_{5^(i offset)}(in), by the
 *                                 reference's binary reading of n -- log2(n) hoisted rotations, HW(n) - 1 lazy ones under one ModDown.  in / out:
 *                                 both components in the domain is_ntt names (a coefficient-domain input is transformed on entry and the result
 *                                 transformed back, :180-182, :285-288); out may be in (both components) and is otherwise another ciphertext.
 *                                 keys: the caller's table of Galois keys, each laid out as rh_bext_gadget_product takes evkQ / evkP, `digits` rows;
 *                                 every element the call needs is looked up BEFORE the first launch, a missing one is RH_ERR_ARG naming it.
 *                                 levelP >= 1 (the hoisted product's own limit), n >= 1, offset != 0 (the reference's "partialtrace: invalid
 *                                 parameter" otherwise).  fused != 0: the two kernels above; 0: the reference's own passes (rh_ring_automorphism_ntt,
 *                                 rh_ring_vec_op) -- the same bits.  Scratch is the extender's (rh_bext_reserve); asynchronous. */
typedef struct rh_galois_key { uint64_t galois_element; const uint64_t* evkQ_dev; const uint64_t* evkP_dev; int digits; } rh_galois_key;
int rh_rlwe_rotate_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* ct0_dev, const uint64_t* tmpQ0_dev,
                                 const uint64_t* tmpQ1_dev, const uint64_t* tmpP0_dev, const uint64_t* tmpP1_dev, uint64_t* accQ0_dev,
                                 uint64_t* accQ1_dev, uint64_t* accP0_dev, uint64_t* accP1_dev, int npoly, int first);
int rh_rlwe_rotate_add_q(rh_ring* r, int level, uint64_t gen, const uint64_t* tmp0_dev, const uint64_t* tmp1_dev, uint64_t* ct0_dev,
                         uint64_t* ct1_dev, int npoly);
int rh_rlwe_partial_traces_sum(rh_bext* be, int levelQ, int levelP, const uint64_t* in0_dev, const uint64_t* in1_dev, int is_ntt, int offset,
                               int n, const rh_galois_key* keys, int nkeys, uint64_t* out0_dev, uint64_t* out1_dev, int npoly, int fused);

/* ---- linear transformations (circuits/common/lintrans/lintrans_evaluator.go): the three streaming passes of the diagonal matrix x ciphertext
 * product.  Standard rings (RH_ERR_UNSUPPORTED otherwise), NTT domain, dense blocks of npoly polys with levelQ+1 / levelP+1 limbs, canonical
 * residues in and out; ONE launch over both components, the Q and the P rows and every poly.  A diagonal is ONE PolyQP (ptQ: at least levelQ+1
 * rows, ptP: at least levelP+1 rows of N words, Montgomery form, NTT domain) shared by every poly of the batch.  The reference's lazy sums all
 * end in Reduce before anything reads them (:220-239, :349-357, :419-427), so every output word is the canonical residue of the exact sum.
 * Every block is 16-byte aligned and no written block may overlap a read one (RH_ERR_ARG).
 *   rh_rlwe_diag_mac_qp               the inner loop of MultiplyByDiagMatrixBSGS for one giant step (:311-357: MulCoeffsMontgomeryLazy(ThenAddLazy)
 *                                     modulo QP over the baby steps and the Reduce that closes them):
 *                                       tmp_c[j] = (sum_k pt_k[j] * x_{k,c}[j]) * 2^-64 mod q,   c = 0, 1
 *                                     x: four device blocks per term, { xQ0, xQ1, xP0, xP1 }: a pre-rotated ciphertext modulo QP, or with
 *                                     xP0 = xP1 = NULL the baby step 0 term (P ct0, P ct1) modulo Q (:316-325), which adds nothing on the P rows; P
 *                                     rows without another term are written as zero (:320-321).  The products are summed in 128 bits and reduced
 *                                     once per rh_ckks_linear_combination_chunk() = 56 terms, which needs every modulus of Q and P below 2^61
 *                                     (checked per call) and operands below q.  table: the caller's device scratch of at least
 *                                     rh_rlwe_diag_mac_qp_table_words(nterms, levelQ, levelP) words, which carries the terms to the kernel: the
 *                                     call keeps no state in the handle.  No output may overlap a term or the table.
 *   rh_rlwe_rotate_sum_accumulate_qp  the giant-step tail of MultiplyByDiagMatrixBSGS (:384-393: ringQP.Add(cQP[0], tmp0QP) and the two
 *                                     AutomorphismNTTWithIndex(ThenAddLazy) passes modulo QP):
 *                                       acc_c[j] = [first ? 0 : acc_c[j]] + (c_c + [c == 0] tmp0)[index(j)]
 *                                     c: the output of the lazy gadget product; acc may overlap neither c nor tmp0.
 *   rh_rlwe_rotate_mul_accumulate_qp  one diagonal of MultiplyByDiagMatrix (:200-218: ringQ.Add of ct0TimesP, the two AutomorphismNTTWithIndex
 *                                     passes modulo QP, MulCoeffsMontgomery(ThenAdd) by the diagonal):
 *                                       acc_c[j] = [first ? 0 : acc_c[j]] + pt[j] * (c_c + [c == 0, Q rows] (P mod q_i) * ct0)[index(j)] * 2^-64
 *                                     c: the output of rh_bext_gadget_product_hoisted_lazy; ct0: ctIn.Value[0]; acc may overlap none of them. */
size_t rh_rlwe_diag_mac_qp_table_words(int nterms, int levelQ, int levelP);
int rh_rlwe_diag_mac_qp(rh_bext* be, int levelQ, int levelP, int nterms, const uint64_t* const* ptQ_dev, const uint64_t* const* ptP_dev,
                        const uint64_t* const* x_dev, uint64_t* tmpQ0_dev, uint64_t* tmpQ1_dev, uint64_t* tmpP0_dev, uint64_t* tmpP1_dev, int npoly,
                        uint64_t* table_dev, size_t table_words);
int rh_rlwe_rotate_sum_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* cQ0_dev, const uint64_t* cQ1_dev,
                                     const uint64_t* cP0_dev, const uint64_t* cP1_dev, const uint64_t* tmpQ0_dev, const uint64_t* tmpP0_dev,
                                     uint64_t* accQ0_dev, uint64_t* accQ1_dev, uint64_t* accP0_dev, uint64_t* accP1_dev, int npoly, int first);
int rh_rlwe_rotate_mul_accumulate_qp(rh_bext* be, int levelQ, int levelP, uint64_t gen, const uint64_t* ptQ_dev, const uint64_t* ptP_dev,
                                     const uint64_t* ct0_dev, const uint64_t* cQ0_dev, const uint64_t* cQ1_dev, const uint64_t* cP0_dev,
                                     const uint64_t* cP1_dev, uint64_t* accQ0_dev, uint64_t* accQ1_dev, uint64_t* accP0_dev, uint64_t* accP1_dev,
                                     int npoly, int first);

/* ---- blind rotation (core/rgsw/blindrot/evaluator.go): BlindRotateCore (:134-186) and evaluateFromDiscreteLogSets (:189-229) for a batch of
 * accumulators in ONE launch, one workgroup per accumulator, resident for the accumulator's whole chain.  It replaces the calls of
 * rgsw.Evaluator.ExternalProduct (core/rgsw/evaluator.go:42-186: the 32-bit branch :82-117 and the Montgomery branch :119-186, which give the same
 * canonical residues) and of rlwe.Evaluator.Automorphism (core/rlwe/evaluator_automorphism.go:14-60) that the reference issues per accumulator.
 * Standard ring (RH_ERR_UNSUPPORTED otherwise) of degree 2^6 .. 2^11 (RH_ERR_UNSUPPORTED otherwise), its modulus 0 alone (levelQ = 0), keys
 * without P and with a power-of-two decomposition: pw2 = BaseTwoDecomposition >= 1, `digits` rows per gadget ciphertext.
 *   rgsw_dev         [key][k < 2][digit][component < 2][N]: Value[k] of BlindRotationKeys[key], NTT domain, Montgomery form; nkeys keys
 *   galois_dev       [slot][digit][component < 2][N]: the automorphism keys; galois_elements: their Galois elements (HOST array, odd, taken
 *                    modulo 2N), ngalois <= 16 slots
 *   prog_offsets_dev nacc + 1 int32 on the device: accumulator b runs prog_ops_dev[prog_offsets[b] .. prog_offsets[b + 1]), in order
 *   prog_ops_dev     nops int32 on the device.  op >= 0: acc = acc x rgsw[op] (ExternalProduct in place); op < 0: acc = Automorphism(acc) with
 *                    key slot -op - 1.  An op that names a key outside the tables, or an offset outside [0, nops], is skipped by the kernel
 *   c0_dev, c1_dev   the accumulators, nacc polys each, NTT domain, canonical residues in and out, updated in place
 * Asynchronous on the ring's stream; keeps no state in the handle. */
int rh_blindrot_core(rh_ring* r, int pw2, int digits, const uint64_t* rgsw_dev, int nkeys, const uint64_t* galois_dev,
                     const uint64_t* galois_elements, int ngalois, const int32_t* prog_offsets_dev, const int32_t* prog_ops_dev, int nops,
                     uint64_t* c0_dev, uint64_t* c1_dev, int nacc);

/* ---- the front end of blindrot.Evaluator.Evaluate (evaluator.go:46-132) on the device: from the sample ciphertexts to the programs and the X^b
 * rows that rh_blindrot_core and the calls around it read.  No coefficient and no program crosses to the host.  Standard rings (RH_ERR_UNSUPPORTED
 * otherwise), blind rotation ring of degree N = 2^6 .. 2^11; every count and pointer is checked on the host, every index read from device
 * memory is range-checked in the kernel.  Asynchronous on the stream of the ring each entry takes; no state is kept in a handle.
 *   rh_blindrot_mod_switch     modSwitchRLWETo2NLvl (:284-307) at level 0 of the LWE ring for ncts sample ciphertexts: x_dev [ct][component < 2][N_LWE],
 *                              coefficient domain, modulus 0 (below 2^63; the inverse transform before it is rh_ring_intt) ->
 *                              a2n_dev int32 [ct][component][N_LWE] = round(x 2N / q) mod 2N, half rounding up, 2N = 2^(logN_br + 1).  The quotient
 *                              is taken exactly, as logN_br + 1 steps of a binary long division in 64-bit integers (never floating point); an even
 *                              non-zero value of component 1 is made odd with ^ 1 (:301-303).  With njobs > 0 it also gathers b (:95):
 *                              b_dev[j] = a2n[ct_j][0][index_j] for the jobs (ct, index) of jobs_dev (int32 pairs).
 *   rh_blindrot_program_stride ops per job that rh_blindrot_program reserves: N_LWE external products, at most min(N_LWE, N - 1) + (N - 2) / 10 + 2
 *                              automorphisms, one spare
 *   rh_blindrot_program        one workgroup per job: the job's vector a (:62-103: the reversal a_0, -a_{n-1}, .., -a_1 of component 1, then
 *                              mulBySmallMonomialMod2N up to X^index) read through its index map, getDiscreteLogSets (:258-280) with indices in
 *                              ascending order inside a set, and the steps of BlindRotateCore (:134-186) / evaluateFromDiscreteLogSets (:189-229):
 *                              the counter carried from the first half-loop into the second, the dropped look-up of set 2N, k == 1 in the second
 *                              half only.  dlog_pos_dev: 2N int32, the step of the walk at which the set of each value of Z_2N is visited
 *                              (getGaloisElementInverseMap :231-255, 0 and 2N - 1 in set 0), negative for an even non-zero value; slots: HOST
 *                              array of 11 key slots, of GaloisGen^1 .. GaloisGen^10 and of 2N - GaloisGen, in rh_blindrot_core's galois table.
 *                              Layout: a FIXED STRIDE per job, stride >= rh_blindrot_program_stride: offsets_dev[j] = j * stride (njobs + 1 int32),
 *                              job j's ops from ops_dev[j * stride], the tail filled with 0x7fffffff, an external product with a key that no table
 *                              holds, which rh_blindrot_core skips.  *flag_dev |= 1: an even non-zero a (the reference panics), |= 2: a program
 *                              longer than stride, |= 4: a dlog_pos entry outside the walk; the caller zeroes it.
 *   rh_blindrot_monomials      MForm(X^b) (:108, ring.NewMonomialXi) for every job: out_dev (njobs, level + 1, N), zero but for +-2^64 mod q_u at
 *                              b mod N, minus for b mod 2N >= N.  The transform, the product with the test polynomial and the first
 *                              automorphism (:109-112) stay rh_ring_ntt, the vec ops and rh_ring_automorphism_ntt. */
int rh_blindrot_mod_switch(rh_ring* rlwe, int logN_br, const uint64_t* x_dev, int ncts, int32_t* a2n_dev, const int32_t* jobs_dev, int njobs,
                           int32_t* b_dev);
int rh_blindrot_program_stride(int n_br, int n_lwe);
int rh_blindrot_program(rh_ring* rbr, int n_lwe, const int32_t* a2n_dev, int ncts, const int32_t* jobs_dev, int njobs, const int32_t* dlog_pos_dev,
                        const int32_t* slots, int stride, int32_t* offsets_dev, int32_t* ops_dev, int32_t* flag_dev);
int rh_blindrot_monomials(rh_ring* rbr, int level, const int32_t* b_dev, int njobs, uint64_t* out_dev);

/* ---- ring packing (core/rlwe/ring_packing.go).  Standard rings (RH_ERR_UNSUPPORTED otherwise), dense blocks of level+1 limbs per poly, canonical
 * residues in and out, both components of a batch of ciphertexts in one launch; the NTT-domain index map of the Galois element (any odd number,
 * taken modulo 2N) is computed in the kernel.  Every block is 16-byte aligned and no written block may overlap a read one (RH_ERR_ARG).
 *   rh_rlwe_expand_step      one level of Expand for the live prefix ct[0 .. cnt) of a batch of at least 2 cnt polys (ring_packing.go:555-575: the two
 *                            AutomorphismNTT that end Automorphism, the CopyNew, and the Add, Sub and MulCoeffsMontgomery pairs):
 *                              ct[p][j] = ct[p][j] + t,  ct[cnt + p][j] = (ct[p][j] - t) * xpow[l][j],  t = tmp[p][index(j)]
 *                            tmp: the un-permuted output of the key switch (cnt polys per component); xpow: X^(-2^i), one poly, NTT domain,
 *                            Montgomery form.  Levels without a second output are rh_rlwe_rotate_add_q.
 *   rh_rlwe_pack_combine     one level of Pack before its key switch (ring_packing.go:726-745, :762, :781).  The level's plan is a table of K int32
 *                            triples (mode, slot_a, slot_b) over the nslots polys of the batch, on the device for the kernel and on the host for the
 *                            check (out of range, or a slot named twice: RH_ERR_ARG).  With bx = b * xpow:
 *                              mode 2 (a and b): u[k] = a - bx, a = a + bx in place;  mode 1 (b alone): b = bx in place, u[k] = bx;  mode 0 (a alone): u[k] = a
 *                            u: the contiguous batch of K polys per component that the level's one key switch reads.
 *   rh_rlwe_rotate_addsub_q  one level of Pack after its key switch (ring_packing.go:768-769, :786-787), same table:
 *                              slot[j] = slot[j] +- tmp[k][index(j)],  slot = slot_b and minus for mode 1, slot_a and plus otherwise
 *   rh_rlwe_ring_split       X -> Y = X^gap on COEFFICIENT-domain rows, gap = 2^logGap (SwitchCiphertextRingDegree, core/rlwe/element.go:293-312, and the
 *                            middle of SwitchCiphertextRingDegreeNTT, :256-268): even[i] = in[i gap] and, when odd0 / odd1 are given, odd[i] = in[i gap + 1],
 *                            as rows of the ring of degree N / gap.  With gap = 2 the two halves of Split; the odd half replaces the multiplication
 *                            by X^-1 and the second inverse transform of ring_packing.go:239-241 (the same canonical residues).
 *   rh_rlwe_ring_merge       Y = X^gap -> X in the NTT domain (MapSmallDimensionToLargerDimensionNTT, ring/operations.go:380-392) and, with odd0 / odd1 and
 *                            the table xpow = X^1 of the large ring, Merge's sum (ring_packing.go:429-434): out[i gap + w] = even[i] + odd[i] * xpow[l][i gap + w]
 *   rh_rlwe_expand           the whole of Expand (ring_packing.go:475-594) on NTT-domain inputs: ct0 / ct1 hold nin << (logN - logGap) polys, the nin inputs
 *                            first; on return the ciphertext of coefficient m 2^logGap of input b is poly m nin + b.  xinvpow: logN polys of xrows limbs,
 *                            X^(-2^i) (GenXPow2NTT, :795-833).  keys: the caller's table, every element N / 2^i + 1 looked up BEFORE the first launch
 *                            (a missing one is RH_ERR_ARG naming it).  levelP >= 1.  Scratch is the extender's; asynchronous. */
int rh_rlwe_expand_step(rh_ring* r, int level, uint64_t gen, const uint64_t* tmp0_dev, const uint64_t* tmp1_dev, uint64_t* ct0_dev, uint64_t* ct1_dev,
                        const uint64_t* xpow_dev, int cnt);
int rh_rlwe_pack_combine(rh_ring* r, int level, uint64_t* ct0_dev, uint64_t* ct1_dev, int nslots, const int32_t* table_dev, const int32_t* table_host,
                         int K, const uint64_t* xpow_dev, uint64_t* u0_dev, uint64_t* u1_dev);
int rh_rlwe_rotate_addsub_q(rh_ring* r, int level, uint64_t gen, const uint64_t* tmp0_dev, const uint64_t* tmp1_dev, uint64_t* ct0_dev, uint64_t* ct1_dev,
                            int nslots, const int32_t* table_dev, const int32_t* table_host, int K);
int rh_rlwe_ring_split(rh_ring* r, int level, const uint64_t* in0_dev, const uint64_t* in1_dev, uint64_t* even0_dev, uint64_t* even1_dev,
                       uint64_t* odd0_dev, uint64_t* odd1_dev, int logGap, int npoly);
int rh_rlwe_ring_merge(rh_ring* r, int level, const uint64_t* even0_dev, const uint64_t* even1_dev, const uint64_t* odd0_dev, const uint64_t* odd1_dev,
                       const uint64_t* xpow_dev, uint64_t* out0_dev, uint64_t* out1_dev, int logGap, int npoly);
int rh_rlwe_expand(rh_bext* be, int levelQ, int levelP, uint64_t* ct0_dev, uint64_t* ct1_dev, int nin, int logGap, const uint64_t* xinvpow_dev,
                   int xrows, const rh_galois_key* keys, int nkeys);

/* ---- BFV ciphertext multiply: scale-invariant tensoring (schemes/bgv/evaluator.go, the scheme of schemes/bfv) ----------------------
 * rh_bfv pairs ringQ with ringQMul (bgv/params.go:98-108: ceil((bitlen(Q_max) + logN) / 61) NTT-friendly 61-bit primes, none shared
 * with Q) and a plaintext modulus T: newEvaluatorPrecomp (:46-78).  Standard rings of the same degree N >= 16.  RH_ERR_ARG for T = 0,
 * T > q_0, T equal to a modulus of Q, rings of different N or of another kind, a modulus in both chains; a call at a level whose
 * levelQMul ringQMul does not have is refused where it is made.
 * All blocks are device-resident, dense (npoly, level+1, N) for Q and (npoly, levelQMul+1, N) for QMul, NTT domain on entry and exit;
 * calls are asynchronous on ringQ's stream (both rings' work goes there).  Scratch belongs to the handle and grows with the largest
 * shape seen; rh_bfv_reserve sizes it up front (multiplies of npoly ciphertexts at the top level).  One handle per thread, like rh_bext;
 * sharing one is safe and serial.
 *   rh_bfv_level_qmul          levelQMul[level] = ceil((bitlen(q_0 .. q_level) + logN) / 61) - 1 (:51-56), negative status for a bad level
 *   rh_bfv_tensor_lazy         tensorLowDeg (:1062-1102) in both rings with ONE launch: c0 = MRed(MForm(a0), b0), c2 = MRed(MForm(a1), b1),
 *                              c1 = MRed(MForm(a0), b1) + MRed(MForm(a1), b0) left in [0, 2q) (MulCoeffsMontgomeryThenAddLazy); square != 0:
 *                              the squaring case (:1079-1088), b* unused (NULL), c1 = 2 * MRed(MForm(a0), a1).  Any representative of
 *                              the operands is accepted; outputs may alias inputs.
 *   rh_bfv_quantize            quantize (:1104-1124) of npoly polys: INTTLazy in both rings, ModDownQPtoP, ModUpPtoQ, MulScalar by T
 *                              (ring/operations.go:201-205), NTT.  cQ, cM: canonical or in [0, 2q), not modified; outQ may alias cQ.
 *                              The middle runs as the three existing launches (rh_bext_moddown_qp_to_p, rh_bext_modup_p_to_q, MulScalar) on
 *                              the handle's scratch, or -- on request, for level+1 <= 8 and levelQMul+1 <= 8 -- as ONE kernel with the QMul
 *                              words in registers.  Same values.
 *   rh_bfv_set_tuning          "fused_quantize" 0 (default: the fused kernel's measured gain was inside the run-to-run spread) / 1:
 *                              shapes of at most 8 limbs a side take the fused kernel; larger ones (up to 32 a side) stay composed.
 *                              Performance only.
 *   rh_bfv_quantize_path       1: that level takes the fused kernel under the current tuning, 0: the composed sequence
 *   rh_bfv_mul_scale_invariant tensorScaleInvariant (:975-1014) without relinearisation: (a0, a1) x (b0, b1) -> (c0, c1, c2) * T / Q.
 *                              b0 = b1 = NULL (or b == a): the squaring case.  c0, c1, c2 may alias any input (ct0 == opOut, ct1 == opOut).
 *                              Relinearisation (:1016-1035) is rh_bext_gadget_product_then_add on c2. */
typedef struct rh_bfv rh_bfv;
int rh_bfv_create(rh_bfv** out, rh_ring* ringQ, rh_ring* ringQMul, uint64_t t);
void rh_bfv_destroy(rh_bfv* b);
int rh_bfv_level_qmul(const rh_bfv* b, int level);
int rh_bfv_reserve(rh_bfv* b, int npoly);
int rh_bfv_set_tuning(rh_bfv* b, const char* key, long value);
int rh_bfv_quantize_path(const rh_bfv* b, int level);
int rh_bfv_tensor_lazy(rh_bfv* b, int level, const uint64_t* a0Q_dev, const uint64_t* a1Q_dev, const uint64_t* b0Q_dev, const uint64_t* b1Q_dev,
                       const uint64_t* a0M_dev, const uint64_t* a1M_dev, const uint64_t* b0M_dev, const uint64_t* b1M_dev,
                       uint64_t* c0Q_dev, uint64_t* c1Q_dev, uint64_t* c2Q_dev, uint64_t* c0M_dev, uint64_t* c1M_dev, uint64_t* c2M_dev,
                       int npoly, int square);
int rh_bfv_quantize(rh_bfv* b, int level, const uint64_t* cQ_dev, const uint64_t* cM_dev, uint64_t* outQ_dev, int npoly);
int rh_bfv_mul_scale_invariant(rh_bfv* b, int level, const uint64_t* a0_dev, const uint64_t* a1_dev, const uint64_t* b0_dev,
                               const uint64_t* b1_dev, uint64_t* c0_dev, uint64_t* c1_dev, uint64_t* c2_dev, int npoly);

/* ---- BGV: standard tensoring and scale matching (schemes/bgv/evaluator.go) ------------------------------------------------------------
 * Entry points on a STANDARD ring handle (RH_ERR_ARG for a 3N or conjugate-invariant ring, a null handle, a level out of range, a scalar
 * that is not below its modulus).  Blocks are device-resident, dense (npoly, level+1, N), NTT domain, residues in [0, q_i) in and out;
 * per-limb scalars are host arrays of level+1 words.  Asynchronous on the ring's stream.  Every thread reads all its operands before it
 * writes: outputs may be any of the inputs (opOut is op0 / op1).
 *   rh_bgv_tensor     tensorStandard, ct x ct (:665-734), and the ct x ct branch of mulRelinThenAdd (:1299-1367) in ONE launch:
 *                     c0 (+)= a0 b0 K, c1 (+)= (a0 b1 + a1 b0) K, c2 (+)= a1 b1 K with K = T * r0.  k[i] = T * r0 * 2^128 mod q_i (r0 = 1:
 *                     tMontgomery of :46-78, one Montgomery factor per MRed).  b0 = b1 = NULL (or b == a): the squaring case (:704-708).
 *                     accumulate 0: outputs written; 1: c0, c1, c2 read and added to (no relinearisation: opOut has degree 2);
 *                     2: c0, c1 read and added to, c2 written (the relin form :1353: c2 is scratch for the gadget product).
 *                     r1 (NULL or MForm(r1) per limb): every accumulator is multiplied by r1 before the add (:1324-1326).
 *   rh_bgv_mul_plain  the plaintext branches (:737-748, :1370-1400): out_j (+)= ct_j * pt * K for the 1, 2 or 3 components given
 *                     (ct1 / ct2 NULL with out1 / out2: fewer components); k, r1, accumulate (0 / 1) as above.
 *   rh_bgv_axpby      matchScaleThenEvaluateInPlace (:288-305): out = r0 a + r1 b (sub != 0: - r1 b) with r0[i] = MForm(r0), r1[i] = MForm(r1);
 *                     b = r1 = NULL: out = r0 a; a = r0 = NULL: out = +- r1 b (a component the other operand does not have).
 *   rh_bgv_plain_combination  a baby step of the BGV polynomial evaluator over a PolynomialVector with a mapping
 *                     (circuits/common/polynomial/polynomial_evaluator.go:281-319): the Add of the encoded constant vector and one MulThenAdd
 *                     by an encoded vector per power (:235-262, :1202-1239, :1370-1400) in ONE launch,
 *                         out_j = [j == 0] c c_scalar + sum_k X_k,j (.) m_k  mod q_i, the canonical residue, for the 1, 2 or 3 outputs given.
 *                     x_dev[3 k + j]: component j of term k, a block of x_rows[k] >= level + 1 limbs per poly (a power kept at a higher level
 *                     is read as its AtLevel view).  m_dev[k] and c_dev (NULL: no constant): ONE poly of level + 1 limbs each, shared by every
 *                     poly of the batch, NTT domain, Montgomery form: the plain lift of the vector (Embed without scale-up).  The T^-1 of
 *                     Encode's scale-up and the T of tMontgomery cancel in a term; the constant keeps its T^-1 as c_scalar[i] = T^-1 mod q_i
 *                     (host, level + 1 residues, given exactly when c_dev is).  table_dev: device scratch of the caller of at least
 *                     rh_bgv_plain_combination_table_words(nterms) words (NULL with nterms = 0), which carries the terms to the kernel: the
 *                     call keeps nothing in the handle.  An output may overlap no term, plaintext, other output or the table (RH_ERR_ARG).
 *                     Products are summed in 128 bits and reduced once per rh_ckks_linear_combination_chunk() terms, which needs every
 *                     modulus up to `level` below 2^61 (RH_ERR_ARG otherwise, checked per call). */
int rh_bgv_tensor(rh_ring* r, int level, const uint64_t* a0_dev, const uint64_t* a1_dev, const uint64_t* b0_dev, const uint64_t* b1_dev,
                  uint64_t* c0_dev, uint64_t* c1_dev, uint64_t* c2_dev, int npoly, const uint64_t* k, const uint64_t* r1, int accumulate);
int rh_bgv_mul_plain(rh_ring* r, int level, const uint64_t* ct0_dev, const uint64_t* ct1_dev, const uint64_t* ct2_dev, const uint64_t* pt_dev,
                     uint64_t* out0_dev, uint64_t* out1_dev, uint64_t* out2_dev, int npoly, const uint64_t* k, const uint64_t* r1, int accumulate);
int rh_bgv_axpby(rh_ring* r, int level, const uint64_t* a_dev, const uint64_t* b_dev, uint64_t* out_dev, int npoly, const uint64_t* r0,
                 const uint64_t* r1, int sub);
int rh_bgv_plain_combination(rh_ring* r, int level, int nterms, const uint64_t* const* x_dev, const int* x_rows, const uint64_t* const* m_dev,
                             const uint64_t* c_dev, const uint64_t* c_scalar, uint64_t* out0_dev, uint64_t* out1_dev, uint64_t* out2_dev, int npoly,
                             uint64_t* table_dev, size_t table_words);
size_t rh_bgv_plain_combination_table_words(int nterms);

/* ---- CKKS: the evaluator's element-wise sequences, one launch each (schemes/ckks/evaluator.go) -----------------------------------------
 * Entry points on a STANDARD or conjugate-invariant power-of-two ring handle (RH_ERR_ARG for a 3N ring, a null handle, a level out of
 * range, a scalar that is not below its modulus).  Blocks are device-resident, dense (npoly, level+1, N), NTT domain, residues in [0, q_i)
 * in and out; per-limb scalars are host arrays of level+1 words.  Asynchronous on the ring's stream.  Every thread reads all its operands
 * before it writes: any output may be any input.  x' = MForm(x) below.
 *   rh_ckks_tensor          the ct x ct branch of mulRelin (:821-835) and of mulRelinThenAdd (:1135-1162) in ONE launch.
 *                           accumulate 0: c0 = MRed(a0', b0), c2 = MRed(a1', b1), c1 = CRed(MRed(a0', b1) + MRed(a1', b0)) -- the bits of
 *                           rh_ring_tensor_degree1; square != 0 (accumulate 0 only; b NULL or b == a): c1 = CRed(2 MRed(a0', a1)) (:825-828);
 *                           1: c0 = CRed(c0 + MRed(a0', b0)), c1 = CRed(CRed(c1 + MRed(a0', b1)) + MRed(a1', b0)), c2 = CRed(c2 + MRed(a1', b1))
 *                           (:1138-1140, :1161); 2: c0, c1 as for 1, c2 WRITTEN (the relin form :1150: c2 is scratch for the gadget product).
 *   rh_ckks_mul_plain       the plaintext branches (:856-878, :1165-1175): out_j (+)= MRed(pt', ct_j) for the 1, 2 or 3 components given
 *                           (trailing NULLs: fewer components); accumulate 0 / 1.
 *   rh_ckks_scalar          evaluateWithScalar (:433-447) on every component given: Ring.AddDoubleRNSScalar / Sub... / Mul... / Mul...ThenAdd
 *                           (ring/operations.go:167-184, :250-266) with the RNS scalar s0 on coefficients [0, N/2) and s1 on [N/2, N), the
 *                           scalars as those calls take them (not in Montgomery form).
 *   rh_ckks_scale_then_add  the scale-matching Add / Sub of evaluateInPlace (:246-431): the operand with the smaller scale (b if scaled_is_b,
 *                           else a) times ratio[i] = ratioInt mod q_i as Mul(ct, ratioInt, tmp) does it (ratio NULL: equal scales, nothing is
 *                           scaled), Add (sub != 0: Sub) on the components both operands have, the components only one has copied (:422-430)
 *                           and, for b's under Sub, negated with ring.Neg (:173-177: q_i - x, so 0 gives q_i as in the reference).  out has
 *                           the components of the larger operand.
 *   rh_ckks_linear_combination  a baby step of the polynomial evaluator (circuits/common/polynomial/polynomial_evaluator.go:342-355), Add of a
 *                           constant and nterms calls of MulThenAdd(X[k], c_k, res), in ONE launch: for the components j the outputs name,
 *                           out_j = [j == 0] c + sum_k s_k X_k,j mod q_i, the canonical residue -- the bits of the sequence, whose every step
 *                           ends in CRed(acc + MRed(x, MForm(s))).  x: a HOST array of 3 nterms device blocks (term k's component j at
 *                           x[3 k + j]; entries past the last output's component are not read), x_rows[k] >= level + 1 the limbs per poly of
 *                           term k's blocks (a power at a higher level is read as its AtLevel view); s0 / s1: host scalars, nterms rows of
 *                           level + 1 words, as rh_ckks_scalar takes them; c0 / c1: the constant's (both NULL: none; nterms = 0 with a
 *                           constant is allowed).  table_dev: device scratch of the CALLER, at least
 *                           rh_ckks_linear_combination_table_words(nterms, level) words, which carries the terms to the kernel: the call keeps
 *                           nothing in the handle, and concurrent callers bring a table each.  The table may be reused by the next call on
 *                           the same stream.  Unlike its neighbours this entry is NOT in place: an output that overlaps a term (or the
 *                           table) is refused.  Moduli must be below 2^61: the products are summed in 128 bits and reduced once per
 *                           rh_ckks_linear_combination_chunk() = 56 terms, the most that bound allows (csrc/ckks.hip derives it);
 *                           rh_ckks_linear_combination_width() terms have their loads in flight together.
 *   rh_ckks_axpby           out_j = ra[i] x_j - rb[i] t_j - [j == 0] s mod q_i, the canonical residue, in ONE launch: the step that follows
 *                           every product of the Chebyshev power basis (circuits/common/polynomial/power_basis.go:148-176: Add(X, X, X), then
 *                           Add(X, -1, X) or the scale-matching Sub(X, T_c, X)) and, with ra = q_i - 1 and no t, the 2 - x, 1 - x and 1 - z^2 of
 *                           the inverse circuits.  Every step of those sequences ends in CRed or MRed of exact values, so these are their
 *                           bits -- except where t has MORE components than x (ring.Neg writes q_i for 0 there), which this entry refuses.
 *                           ra / rb: host arrays of level + 1 residues (rb with t, NULL without); s0 / s1: the constant on coefficients
 *                           [0, N/2) / [N/2, N) as rh_ckks_scalar takes it, or both NULL.  x has 1 to 3 components, t none or components
 *                           0 .. k <= those of x; x_rows / t_rows >= level + 1 are the limbs per poly of the blocks x / t live in (a block at a
 *                           higher level is read as its AtLevel view); outputs are dense at level + 1.  An output may BE an input block whose
 *                           rows equal level + 1; any other overlap of an output with an input or another output is refused. */
enum rh_ckks_scalar_op { RH_CKKS_ADD_SCALAR = 0, RH_CKKS_SUB_SCALAR = 1, RH_CKKS_MUL_SCALAR = 2, RH_CKKS_MUL_SCALAR_THEN_ADD = 3 };
int rh_ckks_tensor(rh_ring* r, int level, const uint64_t* a0_dev, const uint64_t* a1_dev, const uint64_t* b0_dev, const uint64_t* b1_dev,
                   uint64_t* c0_dev, uint64_t* c1_dev, uint64_t* c2_dev, int npoly, int accumulate, int square);
int rh_ckks_mul_plain(rh_ring* r, int level, const uint64_t* ct0_dev, const uint64_t* ct1_dev, const uint64_t* ct2_dev, const uint64_t* pt_dev,
                      uint64_t* out0_dev, uint64_t* out1_dev, uint64_t* out2_dev, int npoly, int accumulate);
int rh_ckks_scalar(rh_ring* r, int level, int op, const uint64_t* in0_dev, const uint64_t* in1_dev, const uint64_t* in2_dev,
                   uint64_t* out0_dev, uint64_t* out1_dev, uint64_t* out2_dev, int npoly, const uint64_t* s0, const uint64_t* s1);
int rh_ckks_scale_then_add(rh_ring* r, int level, const uint64_t* a0_dev, const uint64_t* a1_dev, const uint64_t* a2_dev, const uint64_t* b0_dev,
                           const uint64_t* b1_dev, const uint64_t* b2_dev, uint64_t* out0_dev, uint64_t* out1_dev, uint64_t* out2_dev, int npoly,
                           const uint64_t* ratio, int sub, int scaled_is_b);
int rh_ckks_linear_combination(rh_ring* r, int level, int nterms, const uint64_t* const* x_dev, const int* x_rows, const uint64_t* s0,
                               const uint64_t* s1, const uint64_t* c0, const uint64_t* c1, uint64_t* out0_dev, uint64_t* out1_dev,
                               uint64_t* out2_dev, int npoly, uint64_t* table_dev, size_t table_words);
int rh_ckks_axpby(rh_ring* r, int level, const uint64_t* x0_dev, const uint64_t* x1_dev, const uint64_t* x2_dev, int x_rows,
                  const uint64_t* t0_dev, const uint64_t* t1_dev, const uint64_t* t2_dev, int t_rows, uint64_t* out0_dev, uint64_t* out1_dev,
                  uint64_t* out2_dev, int npoly, const uint64_t* ra, const uint64_t* rb, const uint64_t* s0, const uint64_t* s1);
size_t rh_ckks_linear_combination_table_words(int nterms, int level);
int rh_ckks_linear_combination_chunk(void);
int rh_ckks_linear_combination_width(void);

/* ---- homomorphic DFT (circuits/ckks/dft/dft.go) ---------------------------------------------------------------------------------------
 * The real / imaginary split after CoeffsToSlots and the merge before SlotsToCoeffs, each ONE launch over both components of a batch
 * (standard rings; blocks (npoly, level + 1, N), NTT domain; z, zc, re, im, out: HOST arrays of the two components' device blocks):
 *   rh_ckks_split_real_imag  re = zc + z, im = (z - zc) (-i): Sub, Mul(-1i), Add of dft.go:267-278 (zc = Conjugate(z))
 *   rh_ckks_merge_real_imag  out = im i + re: Mul(1i), Add of :324-330
 * s0 / s1: the double RNS scalar of -i / i as rh_ckks_scalar takes it.  An output may BE an input block (out = im, out = re, re = zc ...);
 * partial overlaps are refused.
 * GenMatrices (:644-773) on the device, float64: values are complex128 (re, im interleaved); a factor is one (ndiag, dslots) block with
 * dslots = slots or 2 slots (sparse RepackImagAsReal).  The ring handle gives the device and the stream.
 *   rh_ckks_dft_level_vectors  abc_dev (3, dslots) = a, b, c of fftPlainVec (decode != 0) / ifftPlainVec at fft_level in [1, log_slots]
 *                            (a[logSlots - fftLevel] of :362-490), the second copy for dslots = 2 slots, every block of `slots` values
 *                            bit-reversed when bit_reversed.  roots_dev: the 4 slots + 1 complex doubles of GetRootsComplex128(4 slots);
 *                            pow5_dev: 5^j mod 4 slots as 64-bit words, at least slots / 2 of them.
 *   rh_ckks_dft_merge_level  out_dev (nout, dslots): per output diagonal d the sum of up to three contributions, FIRST COPIED, THEN ADDED IN
 *                            THE ORDER GIVEN.  program: HOST array of nout * 3 (source, kind) int pairs; source -2: none, -1: the level's
 *                            vector itself (genFFTDiagMatrix :775-804), else row `source` of vec_dev (nin, dslots) times the vector
 *                            (multiplyFFTMatrixWithNextFFTLevel :831-862); kind 0: a and the source as it is, 1: b and the source rotated by
 *                            rot, 2: c and the source rotated by -rot, modulo dslots.  A complex product is four rounded products, one
 *                            rounded difference and one rounded sum.  table_dev: device scratch of the caller, 3 nout words.
 *   rh_ckks_dft_finish       out[d][x] = in[d][(x + rots[d]) mod dslots] * scaling on both parts (rots: HOST array or NULL: no rotation, and
 *                            out_dev may be in_dev), slots [dslots / 2, dslots) of the source taken as zero when zero_upper (:733-740).
 *                            table_dev: device scratch of ndiag words when rots is given. */
int rh_ckks_split_real_imag(rh_ring* r, int level, const uint64_t* const* z_dev, const uint64_t* const* zc_dev, uint64_t* const* re_dev,
                            uint64_t* const* im_dev, int npoly, const uint64_t* s0, const uint64_t* s1);
int rh_ckks_merge_real_imag(rh_ring* r, int level, const uint64_t* const* re_dev, const uint64_t* const* im_dev, uint64_t* const* out_dev,
                            int npoly, const uint64_t* s0, const uint64_t* s1);
int rh_ckks_dft_level_vectors(rh_ring* r, int decode, int log_slots, unsigned dslots, int fft_level, int bit_reversed, const double* roots_dev,
                              size_t nroots, const uint64_t* pow5_dev, size_t npow5, double* abc_dev);
int rh_ckks_dft_merge_level(rh_ring* r, unsigned dslots, int rot, const double* abc_dev, const double* vec_dev, int nin, const int* program,
                            int nout, double* out_dev, uint64_t* table_dev, size_t table_words);
int rh_ckks_dft_finish(rh_ring* r, unsigned dslots, int ndiag, const double* in_dev, double* out_dev, double scaling, int zero_upper,
                       const int* rots, uint64_t* table_dev, size_t table_words);

/* ---- CKKS bootstrapping (circuits/ckks/bootstrapping/evaluator.go, circuits/ckks/mod1/mod1_evaluator.go) ------------------------------
 *   rh_ckks_bootstrap_modup  Evaluator.ModUp's lift of the level-0 residues, centred around q0, to every limb of Q (:678-696, :762-775) and,
 *                            with ringP (sparse-secret encapsulation, :703-722), of component 1 to every limb of Q and of P; ONE launch over
 *                            both components of a batch.  in0 / in1: limb 0 in the COEFFICIENT domain, blocks of in_rows limbs per poly of
 *                            which row 0 is read.  out0 (and out1 without ringP): blocks (npoly, levelQ + 1, N); with ringP component 1 goes
 *                            to c1Q (npoly, levelQ + 1, N) and c1P (npoly, levelP + 1, N) and out1 is NULL.  Every limb of the outputs is
 *                            written; an output that overlaps an input is refused (the lift is not computed in place).  The comparison is coeff >= q0 >> 1, and
 *                            coeff > q0 >> 1 for the encapsulated component 1, as the reference writes them.  Where a modulus divides
 *                            |coeff| of a negative coefficient the canonical 0 is written (the reference's (Q[i] - tmp) * neg gives Q[i]).
 *                            scalarQ / scalarP: HOST residues per limb of uint64(round(scale)) (:735-750, :781-789) or NULL: every limb
 *                            written, limb 0 included, is multiplied by it -- the bits of MulScalar after the NTT.
 *   rh_ckks_double_angle     c0 <- (c0 + c0) + k, c1 <- c1 + c1 (mod1_evaluator.go:108-114: Add(res, res, res), Add(res, -sqrt2pi, res)), in
 *                            place, one launch; k: the double RNS scalar as rh_ckks_scalar takes it (s0 on coefficients [0, N/2), s1 above). */
int rh_ckks_bootstrap_modup(rh_ring* rQ, rh_ring* rP, int levelQ, int levelP, const uint64_t* in0_dev, const uint64_t* in1_dev, int in_rows,
                            uint64_t* out0_dev, uint64_t* out1_dev, uint64_t* c1Q_dev, uint64_t* c1P_dev, int npoly, const uint64_t* scalarQ,
                            const uint64_t* scalarP);
int rh_ckks_double_angle(rh_ring* r, int level, uint64_t* c0_dev, uint64_t* c1_dev, int npoly, const uint64_t* s0, const uint64_t* s1);
/*   rh_ckks_bootstrap_pack   BootstrapMany's pack (evaluator.go:1035-1058): n ciphertexts -> ceil(n / 2^g), g tree levels of
 *                            eve += odd * xPow2[logGap - i]; group j of the output is the sum over the inputs j 2^g + k that exist of
 *                            in times the rows of the set bits of k (a ciphertext without a partner moves up as it is, :1052-1057).
 *                            in0 / in1: blocks (n, in_rows, N), out0 / out1: blocks (ceil(n / 2^g), out_rows, N), NTT domain; xp: the block
 *                            (g, xp_rows, N) with row i = xPow2[logGap - i], NTT domain, Montgomery form; every *_rows >= level + 1.
 *   rh_ckks_bootstrap_unpack its inverse (:985-1001): ceil(n / 2^g) ciphertexts -> n, out[j 2^g + k] = in[j] times the rows xinv[i] =
 *                            xPow2Inv[logGap - i] of the set bits of k, out[j 2^g] a copy; a new block.
 *                            Both: ceil(g / 4) launches over both components, up to four levels each; for g > 4 the intermediates go
 *                            through `scratch` (rh_ckks_bootstrap_pack_scratch_words(N, level + 1, n, g) words, 0 for g <= 4).  1 <= g <= 16.
 *                            Outputs are canonical for canonical inputs; the inputs are left as they were; an output or the scratch that
 *                            overlaps an input, the table or another output is refused.  Standard and conjugate-invariant rings. */
size_t rh_ckks_bootstrap_pack_scratch_words(int N, int L, int n, int g);
int rh_ckks_bootstrap_pack(rh_ring* r, int level, int n, int g, const uint64_t* in0_dev, const uint64_t* in1_dev, int in_rows, uint64_t* out0_dev,
                           uint64_t* out1_dev, int out_rows, const uint64_t* xp_dev, int xp_rows, uint64_t* scratch_dev, size_t scratch_words);
int rh_ckks_bootstrap_unpack(rh_ring* r, int level, int n, int g, const uint64_t* in0_dev, const uint64_t* in1_dev, int in_rows, uint64_t* out0_dev,
                             uint64_t* out1_dev, int out_rows, const uint64_t* xinv_dev, int xinv_rows, uint64_t* scratch_dev, size_t scratch_words);

/* ---- CKKS encoder: the float64 path of schemes/ckks/encoder.go on device batches of nvec vectors ------------------------------------
 * A handle on a STANDARD ring.  Refused by name (RH_ERR_UNSUPPORTED): conjugate-invariant rings, 3N rings, prec > 53 (the *big.Float /
 * *bignum.Complex encoder), rh_ckks_decode with batched = 0 at a level that is neither 0 nor the ring's top level.  Values are IEEE doubles, complex values interleaved (re, im); a block of
 * values is (nvec, 2^log_slots) complex, a plaintext block (nvec, level+1, N) words.  Calls are asynchronous on the ring's stream and lock
 * the handle for the enqueue only; the scratch (two value blocks, one poly block) belongs to the handle and grows with the largest shape
 * seen -- after rh_ckks_encoder_reserve(nvec) no call on up to nvec vectors allocates.  Finite inputs are assumed.
 *   rh_ckks_encoder_create   NewEncoder (encoder.go:72-120).  roots: the NthRoot + 1 = 2N + 1 complex doubles of GetRootsComplex128 (utils.go:53-77),
 *                            RECEIVED like every constant of this engine: results are bit-exact for the table given (Go's math.Cos is not
 *                            libm's cos).  rotGroup (5^j mod 2N) and the CRT tables of the decoder are computed here.
 *   rh_ckks_encoder_set_tuning  "ckks_fft_lds_log": the largest log2 block of a transform kept in one workgroup's LDS, 1 .. 12 (default 12:
 *                            64 KiB); longer vectors run their leading (IFFT) / trailing (FFT) stages as global-memory launches.  Same bits.
 *   rh_ckks_special_ifft / _fft  SpecialIFFTDouble / SpecialFFTDouble (ckks_vector_ops.go:18-76; the unrolled-8 variants compute the same
 *                            butterflies), in place; the IFFT's division by n is Go's complex128 division by complex(n, 0).
 *   rh_ckks_encode           embedDouble (encoder.go:204-320) from a FULL block of values (a caller with fewer values pads with zeros,
 *                            :292-295): copy, IFFT, Complex128ToFixedPointCRT (utils.go:130-234) with the stride-N/(2 slots) spread of
 *                            NTTSparseAndMontgomery (core/rlwe/utils.go:187-245), MForm if is_montgomery, Ring.NTT if is_ntt.  With neither
 *                            flag the words are the reference's own (positive values unreduced up to 2^61 - 1, the word q for a negative
 *                            multiple of q); with either they are the canonical residues the reference's transform / MForm gives.
 *                            values_dev is not modified.
 *   rh_ckks_encode_coeffs    Encode with IsBatched = false (:147-170): Float64ToFixedPointCRT of (nvec, nvals) doubles, nvals <= N, NTT if is_ntt
 *   rh_ckks_decode           decodePublic with IsBatched (:476-575): INTT if is_ntt, polyToComplexNoCRT / polyToComplexCRT (:796-1003) with the
 *                            integer rebuilt exactly and rounded to nearest even (scaleDown, scaling.go:46-52), the FFT, and for
 *                            logprec != 0 math.Round(x * 2^logprec) / 2^logprec on both parts -- on the real part alone, the imaginary one
 *                            zeroed, with real_only (the []float64 output; zeroed whatever logprec is).  values_dev: (nvec, 2^log_slots)
 *                            complex, written whole; poly_dev is not modified.
 *                            batched = 0: plaintextToFloat (:467-472, polyToFloatNoCRT / polyToFloatCRT :1006-1185), the inverse of
 *                            rh_ckks_encode_coeffs: INTT if is_ntt, then every coefficient as its centred integer / scale; values_dev is
 *                            (nvec, N) DOUBLES, log_slots, logprec and real_only are not used (the reference ignores logprec there, :731).
 *                            Level 0 and the ring's top level only: polyToFloatCRT reconstructs over the encoder's FULL ring, so at a
 *                            level in between the reference's result depends on stale limbs of its buffer -- RH_ERR_UNSUPPORTED. */
typedef struct rh_ckks_encoder rh_ckks_encoder;
/* Conjugate-invariant rings: rh_ckks_encoder_create keeps refusing them, in the words it always had; the real-only encoder is the entry
 * of its own below (the Python constructor ckks.Encoder refuses such a ring with the same text unless ckks.NewEncoder(params) passes the
 * permit).  rh_ckks_encoder_create_real: ring of degree n and kind RH_RING_CI, roots: the NthRoot + 1 = 4n + 1 entries; rotGroup is
 * 5^j mod 4n for j < n and log_slots runs up to log2 n (n real slots).  Every other entry takes the handle as it takes a standard one:
 * rh_ckks_encode reads the real parts alone (encoder.go:225-228; utils.go:145-147) and spreads at stride n / slots before the ring's own
 * transform; rh_ckks_decode gathers `slots` coefficients and sets imag[i] = 0 - real[slots - i] before the special FFT (the `isreal`
 * arms of polyToComplexNoCRT / polyToComplexCRT). */
int rh_ckks_encoder_create(rh_ckks_encoder** out, rh_ring* ring, const double* roots, size_t nroots, unsigned prec);
int rh_ckks_encoder_create_real(rh_ckks_encoder** out, rh_ring* ring, const double* roots, size_t nroots, unsigned prec);
void rh_ckks_encoder_destroy(rh_ckks_encoder* e);
int rh_ckks_encoder_reserve(rh_ckks_encoder* e, int nvec);
int rh_ckks_encoder_set_tuning(rh_ckks_encoder* e, const char* key, long value);
int rh_ckks_special_ifft(rh_ckks_encoder* e, double* values_dev, int log_slots, int nvec);
int rh_ckks_special_fft(rh_ckks_encoder* e, double* values_dev, int log_slots, int nvec);
int rh_ckks_encode(rh_ckks_encoder* e, int level, int log_slots, double scale, const double* values_dev, int nvec, uint64_t* out_dev,
                   int is_ntt, int is_montgomery);
int rh_ckks_encode_coeffs(rh_ckks_encoder* e, int level, double scale, const double* values_dev, int nvals, int nvec, uint64_t* out_dev, int is_ntt);
int rh_ckks_decode(rh_ckks_encoder* e, int level, int log_slots, double scale, double logprec, int is_ntt, int batched, int real_only,
                   const uint64_t* poly_dev, int nvec, double* values_dev);

/* ---- BGV encoder: schemes/bgv/encoder.go on device batches of nvec vectors -----------------------------------------------------------
 * A handle on a STANDARD ringQ and the plaintext ring ringT the caller makes: one modulus T, degree n = min(N, order(T) / 2) with order(T)
 * the largest power of two dividing T - 1 (bgv/params.go:110-121).  Values are uint64 words -- []uint64, or []int64 in two's complement
 * with is_signed -- in blocks of (nvec, nvals), nvals <= n; a block modulo T is (nvec, n) words, a plaintext block (nvec, level+1, N).
 * Calls are asynchronous on ringQ's stream (ringT and the target ring are pinned to it for the call) and lock the handle for the enqueue
 * only; the scratch belongs to the handle -- after rh_bgv_encoder_reserve(nvec) no call on up to nvec vectors allocates.
 *   rh_bgv_encoder_create    NewEncoder (:49-96).  Refused by name: a degree of ringT that does not divide N, T a modulus of Q,
 *                            gcd(T, Q) != 1, order(T) < 16; conjugate-invariant and 3N rings (RH_ERR_UNSUPPORTED).  indexMatrix
 *                            (permuteMatrix :98-121) and its inverse, T^-1 mod q_i, the ModUp constants onto {T} per level (:61-65) and the
 *                            mixed-radix tables of the exact branch are computed here.
 *   rh_bgv_encoder_set_tuning  "fused": 1 the lift and Q to T as one kernel each; 0 the reference's own sequence of ring and basis-extension
 *                            calls; -1 (the state at create) whichever the measurement favours for each -- the kernel, for all of
 *                            them, in profiles/bgv_encoder.json.  "fused_lift" / "fused_q2t" set one of the two.  Same bits.  (The
 *                            branch the reference takes through math/big has one form.)
 *   rh_bgv_encode_ring_t     EncodeRingT (:187-246): pT[indexMatrix[i]] = values[i] modulo T, zero past nvals, ringT.INTT, MulScalar(scale)
 *   rh_bgv_decode_ring_t     DecodeRingT (:323-353): MulScalar(scale^-1), ringT.NTT, values[i] = pT[indexMatrix[i]], the signed form minus T
 *                            from T >> 1 on.  pT_dev is not modified.  A scale that is zero or not invertible modulo T is refused.
 *   rh_bgv_ring_t2q          RingT2Q (:357-386): every limb takes pT UNREDUCED at stride N / n and zero elsewhere; scale_up multiplies by
 *                            T^-1 mod Q_level.  ring: ringQ, or another standard ring of degree N (the key-switch ring P, for Embed into a
 *                            ringqp.Poly) WITHOUT scale_up: the reference multiplies the limbs of P under the moduli of Q there (:282, :384).
 *   rh_bgv_ring_q2t          RingQ2T (:391-439) with scaleDown = true, all four branches (level 0 / level > 0, gap 1 / gap > 1)
 *   rh_bgv_encode            Encode (:130-184) / EmbedScale (:252-316): batched: EncodeRingT, RingT2Q, Ring.NTT if is_ntt, MForm if
 *                            is_montgomery; batched = 0: the values at coefficients 0 .. nvals-1, MulScalar(scale), RingT2Q, NTT.  Without
 *                            scale_up, is_ntt and is_montgomery the words are the raw residues modulo T the reference leaves.
 *   rh_bgv_decode            Decode (:442-487): Ring.INTT if is_ntt, RingQ2T, then DecodeRingT (batched) or MulScalar(scale^-1) and the
 *                            values in coefficient order.  in_dev is not modified.
 *   rh_bgv_embed_qp          a whole linear transformation in one pass (circuits/common/lintrans/lintrans.go:271-292 over Embed into a
 *                            ringqp.Poly): for each of the nvec vectors, limbs 0 .. levelQ of outQ (nvec, levelQ + 1, N) and 0 .. levelP of outP
 *                            (nvec, levelP + 1, N) are exactly the words of: each row of cols values rotated to the left by rot[k] & (cols - 1)
 *                            on the host, rh_bgv_encode(ringQ, scale_up = 0), rh_bgv_encode(ringP).  rot: a HOST array of nvec rotations, or
 *                            NULL (no rotation, cols ignored).  One gather (rotation + slot permutation), one inverse transform over T, one
 *                            lift onto the rows of both rings, the forward transforms; "fused" = 0 issues the rotation as a pass of its own
 *                            and then the composition of rh_bgv_encode per ring -- the same bits.  Refused by name: null pointers, levels out
 *                            of range, a ringP that is no standard ring of degree N on ringQ's device, nvals > n; with rot: cols no power of
 *                            two, or not nvals = n = 2 * cols (a BGV plaintext has the encoder's dimensions; shorter rows are the caller's to
 *                            rotate); outputs that overlap the values or each other. */
typedef struct rh_bgv_encoder rh_bgv_encoder;
int rh_bgv_encoder_create(rh_bgv_encoder** out, rh_ring* ringQ, rh_ring* ringT);
void rh_bgv_encoder_destroy(rh_bgv_encoder* e);
int rh_bgv_encoder_reserve(rh_bgv_encoder* e, int nvec);
int rh_bgv_encoder_set_tuning(rh_bgv_encoder* e, const char* key, long value);
int rh_bgv_encode(rh_bgv_encoder* e, rh_ring* ring, int level, uint64_t scale, const uint64_t* values_dev, int nvals, int is_signed, int nvec,
                  uint64_t* out_dev, int batched, int scale_up, int is_ntt, int is_montgomery);
int rh_bgv_decode(rh_bgv_encoder* e, int level, uint64_t scale, const uint64_t* in_dev, int nvec, uint64_t* values_dev, int nvals, int is_signed,
                  int batched, int is_ntt);
int rh_bgv_encode_ring_t(rh_bgv_encoder* e, uint64_t scale, const uint64_t* values_dev, int nvals, int is_signed, int nvec, uint64_t* pT_dev);
int rh_bgv_decode_ring_t(rh_bgv_encoder* e, uint64_t scale, const uint64_t* pT_dev, int nvec, uint64_t* values_dev, int nvals, int is_signed);
int rh_bgv_ring_t2q(rh_bgv_encoder* e, rh_ring* ring, int level, int scale_up, const uint64_t* pT_dev, uint64_t* out_dev, int nvec);
int rh_bgv_ring_q2t(rh_bgv_encoder* e, int level, const uint64_t* in_dev, uint64_t* pT_dev, int nvec);
int rh_bgv_embed_qp(rh_bgv_encoder* e, rh_ring* ringP, int levelQ, int levelP, uint64_t scale, const uint64_t* values_dev, int nvals, int is_signed,
                    int nvec, const int* rot, int cols, uint64_t* outQ_dev, uint64_t* outP_dev, int is_ntt, int is_montgomery);

/* ---- limb-sharded hybrid key switch (BASELINE config 5): one process per GPU owns a subset of the limbs
 * of Q and P and the matching slice of the evaluation key.  Same arithmetic as rh_bext_gadget_product, cut where
 * reconstructRNS (ring/basis_extension.go:550-594) needs limbs of other owners; the exchange (an all-gather of the
 * digit's source limbs, and of the P part before ModDown) is the caller's -- RCCL through torch.distributed in
 * matrix-fhe-lattigo_amd/sharding.py -- and this library never communicates.
 * ringQ_loc / ringP_loc: rings over the OWNED moduli only, ascending global order (ringP_loc NULL iff nownP == 0);
 * allQ / allP: moduli 0..levelQ / 0..levelP of the full chain; ownQ / ownP: global indices of the owned limbs.
 * Local blocks are (poly, owned limb, N); gathered source blocks are (poly, source limb in global order, N). */
typedef struct rh_kshard rh_kshard;
int rh_kshard_create(rh_kshard** out, rh_ring* ringQ_loc, rh_ring* ringP_loc, const uint64_t* allQ, int levelQ,
                     const uint64_t* allP, int levelP, const int* ownQ, int nownQ, const int* ownP, int nownP);
void rh_kshard_destroy(rh_kshard* ks);
int rh_kshard_num_digits(const rh_kshard* ks);                             /* core/rlwe/params.go:635-642 */
int rh_kshard_digit_range(const rh_kshard* ks, int digit, int* st, int* ed); /* global limbs [st, ed) of the digit */
/* one digit of gadgetProductMultiplePLazy (core/rlwe/evaluator_gadget_product.go:154-187, DecomposeSingleNTT :455-478)
 * for the owned limbs.  src_dev: limbs [st, ed) of INTT(cx) gathered from their owners; cx_loc: owned limbs of the
 * NTT-domain input; evkQ_loc / evkP_loc: [digit][component < 2][owned limb][N].  Feed digits 0 .. beta-1 in order. */
int rh_kshard_digit(rh_kshard* ks, int digit, const uint64_t* src_dev, const uint64_t* cx_loc, const uint64_t* evkQ_loc,
                    const uint64_t* evkP_loc, uint64_t* ct0_loc, uint64_t* ct1_loc, uint64_t* accP0_loc, uint64_t* accP1_loc,
                    int npoly);

/* All digits in one call: src_all_dev = EVERY limb of INTT(cx), (npoly, levelQ + 1, N) in chain order (ONE all-gather of the owners'
 * limbs instead of one per digit); the other arguments as for rh_kshard_digit.  Same results as the beta rh_kshard_digit calls, with
 * the structure of the single-GPU product: one pipelined transform of all digit blocks, one multiply-accumulate over all digits. */
int rh_kshard_product(rh_kshard* ks, const uint64_t* src_all_dev, const uint64_t* cx_loc, const uint64_t* evkQ_loc,
                      const uint64_t* evkP_loc, uint64_t* ct0_loc, uint64_t* ct1_loc, uint64_t* accP0_loc, uint64_t* accP1_loc, int npoly);
/* ModDownQPtoQNTT (ring/basis_extension.go:241-258) for the owned Q limbs.  srcP_dev: (npoly, levelP+1, N), the
 * INTTLazy of the P part gathered from its owners. */
int rh_kshard_moddown(rh_kshard* ks, const uint64_t* srcP_dev, const uint64_t* ctQ_in_loc, uint64_t* ctQ_out_loc, int npoly);


/* The WHOLE limb-sharded product in one call, orchestration included: ringQ.INTT(cx) -> exchange of every limb of INTT(cx) ->
 * gadgetProductMultiplePLazy on the owned limbs -> INTTLazy of the owned P limbs -> exchange of the P part of both accumulators ->
 * ModDownQPtoQNTT on the owned Q limbs (core/rlwe/evaluator_gadget_product.go:16-30, 33-46, 122-188, 455-478).  The library still never
 * communicates: both exchanges are calls of `allgather`, which the HOST supplies -- ncclAllGather on the node's RCCL communicator from a cgo
 * host, torch.distributed from Python (sharding.LimbShardedKeySwitch).
 *   rh_allgather_fn(ctx, send_dev, recv_dev, send_words, hip_stream): every rank contributes send_words uint64 at send_dev and receives
 *       world * send_words at recv_dev, rank-major (the semantics of ncclAllGather), ENQUEUED on hip_stream; 0 on success.  All ranks make
 *       the same sequence of calls (two per chunk), so the collectives match up.
 *   rh_kshard_set_world: the owner of every limb of Q ++ P (owner[i], i <= levelQ: Q limb i; owner[levelQ+1+j]: P limb j); the entries equal
 *       to `rank` must be exactly the owned limbs the handle was created with.  A handle that owns every limb needs no map (world = 1).
 *   chunks: the batch is cut into this many chunks alternating between two side streams, so that one chunk's exchange runs under the other's
 *       arithmetic (<= 0: auto = 4 for npoly >= 4 on more than one rank, else 1).  The call returns with everything enqueued; the ring's
 *       stream (rh_ring_set_stream of the local Q ring) waits for the side streams, so the caller synchronises as for any other entry.
 *   rh_kshard_exchange_words / rh_kshard_set_exchange: optional.  The exchange blocks are carved from memory the library allocates, unless
 *       the host registers an arena of at least rh_kshard_exchange_words(...) words (a host whose all-gather must map the pointers it is
 *       handed back to its own buffer objects, e.g. torch tensors).
 * cx_loc, ct0_loc, ct1_loc: (npoly, owned Q limbs, N); evkQ_loc / evkP_loc: [digit][component < 2][owned limb][N].  Outputs stay limb-sharded,
 * every owned limb bit-identical to the same limb of rh_bext_gadget_product. */
typedef int (*rh_allgather_fn)(void* ctx, const uint64_t* send_dev, uint64_t* recv_dev, size_t send_words, void* hip_stream);
int rh_kshard_set_world(rh_kshard* ks, int world, int rank, const int* owner);
int rh_kshard_exchange_words(const rh_kshard* ks, int npoly, int chunks, size_t* words);
int rh_kshard_set_exchange(rh_kshard* ks, uint64_t* arena_dev, size_t words);
int rh_kshard_gadget_product(rh_kshard* ks, const uint64_t* cx_loc, const uint64_t* evkQ_loc, const uint64_t* evkP_loc,
                             uint64_t* ct0_loc, uint64_t* ct1_loc, int npoly, rh_allgather_fn allgather, void* ctx, int chunks);

/* ---- keys and ciphertexts made on the device (csrc/keygen.hip) -------------------------------------------------------------------------
 * The samplers' stream.  Block t of substream (call, poly, row, group) is the 64-byte BLAKE2b digest, keyed with the PRNG's key and
 * personalised with "ringhip-sampler\0", of the five little-endian words (call, poly, row, group, t), read as eight little-endian words;
 * coefficient i uses word i % 8 of blocks t = 0, 1, ... of group i / 8.  `state`: the eight chaining words after the padded key block
 * (the host computes them once per key), so a block costs one compression.  call: the PRNG's read counter; poly0: the index of the first
 * poly written (a batch sampled in sub-blocks gives the same polys); row: row0 + limb for uniform polys (Q limbs first, then P), 0 for
 * the small-norm samplers.  Everything is enqueued on the ring's stream.
 *   rh_sample_uniform   UniformSampler.Read (ring/sampler_uniform.go:46-106): candidate = word & Mask, accepted when < q.  Limbs 0..level of
 *                       npoly polys; row (poly, limb) goes to out + (poly * out_rows + limb) * N (out_rows >= level + 1: a write at a row
 *                       stride into a larger block, e.g. component 1 of a key table).
 *   rh_sample_gaussian  the distribution of GaussianSampler.Read (ring/sampler_gaussian.go:159-172) from the cumulative table
 *                       table_dev[k] = floor(P(|x| <= k) 2^63), k < table_len <= 1024, table[table_len - 1] = 2^63 (the host builds it up to the largest magnitude the law reaches): |x| = #{k: table[k] <= word & (2^63 - 1)}, negative when
 *                       bit 63 is set.  out: int32 (npoly, N).  Zero is the canonical 0 (the reference writes q for a zero of sign 0).
 *   rh_sample_ternary   TernarySampler.Read with a density P (ring/sampler_ternary.go): non-zero when (word >> 1) < threshold = floor(P 2^63),
 *                       negative when bit 0 is set.  out: int32 (npoly, N).
 *   rh_small_lift       int32 (npoly, N) -> residues under limbs 0..levelQ of ringQ and 0..levelP of ringP (NULL: Q alone): x >= 0 ? x : q - |x|,
 *                       what Read + ExtendBasisSmallNormAndCenter produce; accumulate: ReadAndAdd, out = CRed(out + lift).  q_rows / p_rows:
 *                       limbs per poly of the output blocks. */
int rh_sample_uniform(rh_ring* r, int level, const uint64_t* state, uint64_t call, uint64_t poly0, uint64_t row0, uint64_t* out_dev, int out_rows, int npoly);
int rh_sample_gaussian(rh_ring* r, const uint64_t* state, uint64_t call, uint64_t poly0, const uint64_t* table_dev, int table_len, int32_t* out_dev, int npoly);
int rh_sample_ternary(rh_ring* r, const uint64_t* state, uint64_t call, uint64_t poly0, uint64_t threshold, int32_t* out_dev, int npoly);
int rh_small_lift(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const int32_t* in_dev, uint64_t* outQ_dev, int q_rows, uint64_t* outP_dev, int p_rows,
                  int npoly, int accumulate);
/* Every row of one or many gadget ciphertexts in one launch (per row: MForm, MulCoeffsMontgomeryThenSub, core/rlwe/encryptor.go:449-452, and the
 * MulScalarMontgomery + Add per digit limb of AddPolyTimesGadgetVectorToGadgetCiphertext, core/rlwe/gadgetciphertext.go:172-241, as
 * genEvaluationKey sequences them, core/rlwe/keygenerator.go:297-315):
 *   tab[r][0] = MForm(e_r) - tab[r][1] * skOut[key_r] [+ skIn[key_r] * s_r on the Q limbs where s_r != 0]
 * eQ / eP: the NTT of the lifted errors, (rows, limbs, N); tabQ / tabP: (rows, 2, limbs, N), component 1 already holding the uniform a;
 * skOutQ / skOutP: (nkeys, limbs, N) and skInQ: (skin_keys, levelQ + 1, N), skin_keys = nkeys or 1 (one input key for all), NTT domain, Montgomery form.  rowtab (HOST): rows x (levelQ + 2) words:
 * key_r, then s_r per limb of Q -- P 2^(j pw2) in Montgomery form on the limbs of the row's digit, 0 elsewhere.  table_dev: device scratch of
 * at least rh_rlwe_gadget_encrypt_table_words(levelQ, rows) words the row table is staged into.  ringP NULL: no P (eP, tabP, skOutP NULL). */
size_t rh_rlwe_gadget_encrypt_table_words(int levelQ, int rows);
int rh_rlwe_gadget_encrypt(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, uint64_t* tabQ, uint64_t* tabP,
                           const uint64_t* skOutQ, const uint64_t* skOutP, const uint64_t* skInQ, int nkeys, int skin_keys, const uint64_t* rowtab, int rows,
                           uint64_t* table_dev, size_t table_words);
/* Every row of many RGSW ciphertexts under one secret key in one launch (rgsw.Encryptor.EncryptZero and Encrypt, core/rgsw/encryptor.go:25-118: per
 * row the encryption of zero of core/rlwe/encryptor.go:449-452, then AddPolyTimesGadgetVectorToGadgetCiphertext, core/rlwe/gadgetciphertext.go:172-241,
 * on component 0 of Value[0] and component 1 of Value[1]):
 *   tab[r][0] = MForm(e_r) - tab[r][1] * sk          with tab[r][1] as sampled, then on the Q limbs where s_r != 0
 *   half_r == 0: tab[r][0] += pt[p_r] * s_r;          half_r == 1: tab[r][1] += pt[p_r] * s_r
 * eQ / eP, tabQ / tabP: as rh_rlwe_gadget_encrypt's; skQ / skP: (limbs, N), one secret; ptQ: (npt, levelQ + 1, N) plaintexts, NTT domain, Montgomery
 * form, named by the rows (the keys of a blind rotation set share three: X^-1, X^0, X^1).  rowtab (HOST): rows x (levelQ + 3) words: p_r, half_r,
 * then s_r per limb of Q; table_dev: device scratch of rh_rgsw_encrypt_table_words(levelQ, rows) words.  ringP NULL: no P. */
size_t rh_rgsw_encrypt_table_words(int levelQ, int rows);
int rh_rgsw_encrypt(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, uint64_t* tabQ, uint64_t* tabP,
                    const uint64_t* skQ, const uint64_t* skP, const uint64_t* ptQ, int npt, const uint64_t* rowtab, int rows, uint64_t* table_dev,
                    size_t table_words);
/* encryptZeroSkFromC1 with addPtToCt folded in (core/rlwe/encryptor.go:398-424, :512-530), NTT domain: c0 = -c1 sk + e [+ pt], canonical.
 * sk: (level + 1, N), NTT domain, Montgomery form; e: the NTT of the lifted error; pt: NULL or an NTT-domain plaintext batch.  e NULL: only
 * -c1 sk (a coefficient-domain ciphertext adds its error and plaintext after the inverse transform, :415-420). */
int rh_rlwe_encrypt_sk(rh_ring* r, int level, const uint64_t* c1, const uint64_t* sk, const uint64_t* e, const uint64_t* pt, uint64_t* c0, int npoly);
/* ct0 = u * pk0, ct1 = u * pk1 (MulCoeffsMontgomery, core/rlwe/encryptor.go:259-260, :324-326) in one launch that reads u once.
 * u: (npoly, level + 1, N); pk0, pk1: (level + 1, N) shared by the batch. */
int rh_rlwe_mul_pk(rh_ring* r, int level, const uint64_t* u, const uint64_t* pk0, const uint64_t* pk1, uint64_t* ct0, uint64_t* ct1, int npoly);
/* Decryptor.Decrypt's Horner sum c0 + s (c1 + s c2) (core/rlwe/decryptor.go:51-92), NTT domain, canonical, every component read once.
 * c2 NULL: degree 1.  out may be c0. */
int rh_rlwe_decrypt(rh_ring* r, int level, const uint64_t* c0, const uint64_t* c1, const uint64_t* c2, const uint64_t* sk, uint64_t* out, int npoly);
/* The entries of this section take standard rings and 3N rings whose degree is a multiple of 8 (a sampler lane serves a group of eight
 * coefficients); ringQ and ringP of the same kind; every kernel addresses row r at r * N words.  Conjugate-invariant rings are refused. */

/* ---- the Matrix CKKS encoder (csrc/matrix_ckks.hip; schemes/matrix_ckks/encoder.go) --------------------------------------------------------
 * 3N rings.  Values are (nvec, nvals) blocks on the device: vtype 0 = uint64, 1 = float64, 2 = complex128 (interleaved; real parts only,
 * encoder.go:237-241).  nvals > N: "too many values: %d > %d" (:182-184).  Enqueued on the ring's stream.
 *   rh_matrix_ckks_encode  Encode (:163-257) through SingleFloat64ToFixedPointCRT (:384-426) into a dense (nvec, level + 1, N) block, coefficient
 *                          domain, coefficients i >= nvals zero: uint64 through float64(val); the sign onto the scale; the product truncated;
 *                          from 2^64 on the low 64 bits of the integer the float is, no sign applied; below, a negative value gives -c modulo
 *                          2^64.  The reference stores CRed(word, q_i) (it can stay >= q_i); this entry stores that word's canonical residue.
 *                          negatives_signed != 0: a negative value stores q_i - (|c| mod q_i) instead, which Decode gives back.
 *   rh_matrix_ckks_decode  polyToFloatNoCRT (:430-445) on limb 0 of a coefficient-domain block with pt_rows limbs per poly:
 *                          c >= q_0 >> 1 ? -float64(q_0 - c) / scale : float64(c) / scale, the first nvals coefficients, into float64, complex128
 *                          (imaginary part 0) or uint64 (truncated, :299-302; a negative value's word is not defined there: 0). */
int rh_matrix_ckks_encode(rh_ring* r, int level, double scale, const void* values_dev, int vtype, int nvals, int nvec, int negatives_signed, uint64_t* pt_dev);
int rh_matrix_ckks_decode(rh_ring* r, double scale, const uint64_t* pt_dev, int pt_rows, int nvec, int nvals, int vtype, void* values_dev);

/* ---- the multiparty protocols' hot paths (csrc/multiparty.hip; multiparty/ of the reference) ---------------------------------------------
 * Standard rings, canonical residues in and out, everything enqueued on the ring's stream.
 *   rh_mp_aggregate        out = sum over k < nshares of shares[k] mod q on blocks of (npoly, level + 1, N): AggregateShares of every protocol
 *                          (keygen_cpk.go:86-88, keygen_evk.go:213-242, keyswitch_sk.go:154-161) over many shares at once.  Every share is read
 *                          once and the sum written once; one conditional subtraction per addend, so the result is that of the pairwise ring.Add
 *                          calls, word for word.  shares (HOST): nshares device block addresses, staged into table_dev (device scratch of at
 *                          least rh_mp_aggregate_table_words(nshares) words).  out may be one of the shares; it may overlap none otherwise.
 *   rh_mp_gadget_share     every row of one party's evaluation-key, Galois-key or public-key shares for one or many keys in one launch
 *                          (keygen_evk.go:115-210, keygen_gal.go:57-78, keygen_cpk.go:70-83):
 *                            share[r] = MForm(e_r) + skIn[key_r] * s_r (on the Q limbs where s_r != 0) - crp[r] * skOut[key_r]
 *                          eQ / eP: the NTT of the lifted errors; crpQ / crpP: the common reference rows; shareQ / shareP: the output; all
 *                          (rows, limbs, N).  skOutQ / skOutP: (nkeys, limbs, N), skInQ: (skin_keys, levelQ + 1, N), skin_keys = nkeys or 1, NTT
 *                          domain, Montgomery form.  rowtab (HOST) and table_dev: as rh_rlwe_gadget_encrypt's (rh_mp_gadget_share_table_words).
 *                          A public-key share is one row whose scalars are all 0.  ringP NULL: no P (eP, crpP, shareP, skOutP NULL).
 *   rh_mp_relin_round_one  both components of every row of a party's round-one relinearisation share, the CRP read once (keygen_relin.go:130-222):
 *                            share[r][0] = e0_r + skI * s_r (on the Q limbs where s_r != 0) - u * crp[r],   share[r][1] = e1_r + sk * crp[r]
 *                          e0, e1: the NTT of the lifted errors, NOT in Montgomery form; crp: (rows, limbs, N); share: (rows, 2, limbs, N); u, sk:
 *                          (limbs, N), NTT domain, Montgomery form; skIQ = IMForm(sk) on Q.  s_r = MForm(P 2^(j pw2)), so skI * s_r is the plain
 *                          residue of P 2^(j pw2) sk.  rowtab / table_dev: as rh_mp_gadget_share's (the key index is not read).
 *   rh_mp_relin_round_two  out[r] = r1[r][0] * sk + e_r + (u - sk) * r1[r][1] (keygen_relin.go:231-270): r1 the aggregated round-one share
 *                          (rows, 2, limbs, N), both components read once; e and out: (rows, limbs, N).
 *   rh_mp_keyswitch_share  out = [acc +] c1 * (skA [- skB]) [+ e] on a batch of npoly ciphertexts (keyswitch_sk.go:118-149; with acc and
 *                          without skB the secret-key term of keyswitch_pk.go).  c1: row (poly, limb) at (poly * c1_rows + limb) * N, c1_rows >=
 *                          level + 1 (a ciphertext above the share's level); skA, skB: (level + 1, N), NTT domain, Montgomery form; acc, e, out:
 *                          (npoly, level + 1, N), e the NTT of the lifted error.  skB, acc and e may be NULL; out may be acc or e. */
size_t rh_mp_aggregate_table_words(int nshares);
int rh_mp_aggregate(rh_ring* r, int level, const uint64_t* const* shares, int nshares, uint64_t* out, int npoly, uint64_t* table_dev, size_t table_words);
size_t rh_mp_gadget_share_table_words(int levelQ, int rows);
int rh_mp_gadget_share(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, const uint64_t* crpQ, const uint64_t* crpP,
                       uint64_t* shareQ, uint64_t* shareP, const uint64_t* skOutQ, const uint64_t* skOutP, const uint64_t* skInQ, int nkeys, int skin_keys,
                       const uint64_t* rowtab, int rows, uint64_t* table_dev, size_t table_words);
int rh_mp_relin_round_one(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const uint64_t* e0Q, const uint64_t* e0P, const uint64_t* e1Q, const uint64_t* e1P,
                          const uint64_t* crpQ, const uint64_t* crpP, uint64_t* shareQ, uint64_t* shareP, const uint64_t* uQ, const uint64_t* uP,
                          const uint64_t* skQ, const uint64_t* skP, const uint64_t* skIQ, const uint64_t* rowtab, int rows, uint64_t* table_dev, size_t table_words);
int rh_mp_relin_round_two(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const uint64_t* eQ, const uint64_t* eP, const uint64_t* r1Q, const uint64_t* r1P,
                          uint64_t* outQ, uint64_t* outP, const uint64_t* uQ, const uint64_t* uP, const uint64_t* skQ, const uint64_t* skP, int rows);
int rh_mp_keyswitch_share(rh_ring* r, int level, const uint64_t* c1, int c1_rows, const uint64_t* skA, const uint64_t* skB, const uint64_t* acc,
                          const uint64_t* e, uint64_t* out, int npoly);

/* ---- the share conversion of the collective refresh (csrc/mp_refresh.hip; multiparty/mpckks of the reference) ------------------------------
 * Multiword integers per coefficient on the device, where the reference walks []*big.Int on the host.  A big-integer BLOCK holds npoly * n
 * values of W 64-bit words each (1 <= W <= 8), little-endian, two's complement, word-major in memory: word w of value i of poly p is at
 * blk[(p * W + w) * n + i].  n: a power of two, 2 <= n <= N (n = 2 * slots on a standard ring); value i belongs to coefficient i * gap,
 * gap = N / n.  Standard rings; polys are COEFFICIENT-domain, canonical residues; everything is enqueued on the ring's stream (the target
 * ring's for rh_mp_refresh_recode).  The reference's non-NTT sparse branch (core/rlwe/utils.go:235-240) is not reproduced.
 *   rh_mp_big_sample      the mask law of mpckks/sharing.go:120-129: RandInt(prng, 2^logBound), then - 2^logBound when >= 2^(logBound - 1),
 *                         which is logBound uniform bits sign-extended from bit logBound - 1; no rejection.  Word w of value i of poly p is word
 *                         i % 8 of block t = 0 of substream (call, poly0 + p, row = w, group = i / 8) of the samplers' stream (above);
 *                         1 <= logBound <= 64 W - 1.  The ring gives the device and the stream alone.
 *   rh_mp_big_to_rns      SetCoefficientsBigint (ring/ring.go:433-447) with the spread of NTTSparseAndMontgomery (core/rlwe/utils.go:187-245):
 *                         limb k <= level of coefficient i * gap is value_i mod q_k, Euclidean and canonical as big.Int.Mod gives, zero
 *                         elsewhere.  out: dense (npoly, level + 1, N).  accumulate = +1 / -1: added to / subtracted from what is there instead
 *                         (the Sub of mpckks/sharing.go:140 and the Add of :259), the coefficients between left as they are.
 *   rh_mp_big_from_rns    PolyToBigintCentered(p, gap, .) (ring/ring.go:503-543): v = CRT(limbs 0..level of coefficient i * gap) in [0, Q),
 *                         value_i = v - Q when v >= floor(Q / 2) (note the >=), else v.  in: row (poly, limb) at (poly * in_rows + limb) * N.
 *                         accumulate != 0: added to the value that is there (the Add of mpckks/sharing.go:172-178), modulo 2^(64 W).
 *                         RH_ERR_UNSUPPORTED when Q_level >= 2^511, the most eight words centre, or the level has more than 16 limbs;
 *                         RH_ERR_ARG when the caller's W is too small for Q_level.
 *   rh_mp_big_muldiv      out = Quo(x * m, d) per value, truncated TOWARD ZERO like big.Int.Quo (mpckks/transform.go:363-376).  m: mwords <= 2
 *                         words, d > 0: dwords <= 4 words (HOST, little-endian).  The product is held in W + 2 words; a quotient that does
 *                         not fit W words is the caller's error.  out may be blk.  The ring gives the device and the stream alone.
 *   rh_mp_refresh_recode  from-RNS at levelIn of ringIn, muldiv, to-RNS at levelOut of ringOut in ONE kernel, no block in memory: the bits of
 *                         the three calls.  Source: `in` (with ringIn, in_rows; blk NULL), the Transform of mpckks/transform.go:300-376, or
 *                         `blk` (in and ringIn NULL), the second half of its GenShare.  W: the words a value is held in, enough for the
 *                         centred source and for the quotient.  ringOut may have another degree, n <= N_out.  The launch goes to ringOut's
 *                         stream and orders nothing against ringIn's: two handles must be on ONE stream (rh_ring_set_stream), as every
 *                         protocol of multiparty_refresh.py that takes two rings requires of its caller. */
int rh_mp_big_sample(rh_ring* r, const uint64_t* state, uint64_t call, uint64_t poly0, int logBound, uint64_t* blk_dev, int n, int W, int npoly);
int rh_mp_big_to_rns(rh_ring* r, int level, const uint64_t* blk_dev, int n, int W, uint64_t* out_dev, int npoly, int accumulate);
int rh_mp_big_from_rns(rh_ring* r, int level, const uint64_t* in_dev, int in_rows, uint64_t* blk_dev, int n, int W, int npoly, int accumulate);
int rh_mp_big_muldiv(rh_ring* r, const uint64_t* blk_dev, uint64_t* out_dev, int n, int W, int npoly, const uint64_t* m, int mwords, const uint64_t* d, int dwords);
int rh_mp_refresh_recode(rh_ring* ringIn, int levelIn, const uint64_t* in_dev, int in_rows, const uint64_t* blk_dev, int n, int W, rh_ring* ringOut,
                         int levelOut, uint64_t* out_dev, int npoly, const uint64_t* m, int mwords, const uint64_t* d, int dwords, int accumulate);

/* ---- the noise meters (csrc/noise.hip; ring.Log2OfStandardDeviation, core/rlwe/utils.go of the reference) ------------------------------------
 *   rh_ring_centered_moments  the exact integers PolyToBigintCentered(p, gap, .) (ring/ring.go:503-543, ring/ringqp) would give, summed: for every
 *                          poly of a COEFFICIENT-domain block, over limbs 0..levelQ of ringQ and, with ringP, limbs 0..levelP of ringP as one RNS
 *                          basis m_0 .. m_{L-1} (Q first) of product M: v = CRT(residues of coefficient i gap) in [0, M), x = v - M when
 *                          v >= floor(M / 2) (note the >=), for the n = N / gap coefficients 0, gap, 2 gap ...  Any residues: words >= m_i are
 *                          reduced first.  Every ring kind; N need not be a power of two.  q: row (poly, limb) at (poly * q_rows + limb) * N
 *                          words, p likewise; ringP NULL: Q alone (p NULL, levelP and p_rows not read).
 *                          out: rh_ring_centered_moments_words(L) words per poly, L = levelQ + 1 [+ levelP + 1], all integers, no float anywhere.
 *                          With the mixed-radix digits d_0 .. d_{L-1} of v (v = sum_i R_i d_i, R_i = m_0 ... m_{i-1}, 0 <= d_i < m_i) and two
 *                          more rows d_L = 1, d_{L+1} = c (1 on the lanes where M was subtracted), the block holds
 *                            P_ij = sum over the n lanes of d_i d_j, 0 <= i <= j <= L + 1, three little-endian words each (192 bits), pair (i, j)
 *                                   at 3 (i (L + 2) - i (i - 1) / 2 + j - i): the upper triangle, row-major;
 *                            then the L digits of the smallest |x| and the L digits of the largest |x| (|x| = sum_i R_i digit_i).
 *                          So  sum c = P_{L,L+1},  sum v = sum_i R_i P_{i,L},  sum x = sum v - M sum c,
 *                              sum x^2 = sum_{i <= j < L} (2 - [i = j]) R_i R_j P_ij - 2 M sum_i R_i P_{i,L+1} + M^2 sum c.
 *                          (P_{L,L} counts the lanes of whole chunks, not n.)  The sums are exact whatever the launch geometry.
 *                          Scratch (tables, per-workgroup partials) belongs to ringQ's handle, as the rescale and AtLevel scratch does, and
 *                          every call rewrites it in stream order: calls on one handle must go to ONE stream.  Two host threads that drive
 *                          the same handle on different streams would overwrite each other's tables under a running kernel; give each such
 *                          thread a handle of its own.  The handle's lock serialises the host side alone.  Enqueued on ringQ's stream.
 *                          RH_ERR_UNSUPPORTED: more than 64 moduli over Q and P together.  RH_ERR_ARG: gap does not divide N; the two handles
 *                          are on different streams (rh_ring_set_stream); a modulus of 2^61 or more; the moduli are not pairwise distinct.
 *   rh_rlwe_gadget_phase   NoiseGadgetCiphertext (core/rlwe/utils.go:51-102) up to its INTT for many gadget ciphertexts in one launch that reads
 *                          every row once.  Output poly o names one key and one power-of-two index j < min_i len(Value[i]):
 *                            out[o] = sum over the key's RNS digits i of (Value[i][j][0] + Value[i][j][1] * sk[sk_o])  on the limbs of Q and of P,
 *                                     - pt[pt_o] * s_o  on the limbs of Q,  s_o = MForm(P 2^(j pw2)) per limb (MForm(2^(j pw2)) without P)
 *                          NTT domain, Montgomery form in and out, canonical residues: the words the reference's MulCoeffsMontgomeryThenAdd,
 *                          Add, MulScalarBigint, MulScalar and Sub leave in Value[0][j][0].  The digit sum is kept lazily and reduced once per
 *                          row.  A public key (NoisePublicKey, :13-25) is one row without a plaintext.
 *                          Key tables: (rows, 2, limbs, N) as rh_rlwe_gadget_encrypt writes them, one for Q and one for P, anywhere on the
 *                          device.  sk: (nsk, limbs, N) for Q and for P; pt: (npt, levelQ + 1, N).  out: (outs, limbs, N) for Q and for P.
 *                          rowtab (HOST): outs x (6 + max_terms + levelQ + 1) words: the address of the key's Q table, of its P table (0
 *                          without P), the rows the key has, sk_o, pt_o (all ones: no plaintext), the term count m_o <= max_terms, max_terms row
 *                          numbers (the first m_o are read: the rows of Value[i][j], i = 0 ..), then s_o per limb of Q.  table_dev: device scratch
 *                          of rh_rlwe_gadget_phase_table_words(levelQ, outs, max_terms) words.  ringP NULL: no P (skP, outP NULL).
 *                          Standard rings and 3N rings; conjugate-invariant rings are refused. */
size_t rh_ring_centered_moments_words(int limbs);
int rh_ring_centered_moments(rh_ring* ringQ, int levelQ, const uint64_t* q_dev, int q_rows, rh_ring* ringP, int levelP, const uint64_t* p_dev, int p_rows,
                             int gap, int npoly, uint64_t* out_dev);
size_t rh_rlwe_gadget_phase_table_words(int levelQ, int outs, int max_terms);
int rh_rlwe_gadget_phase(rh_ring* ringQ, rh_ring* ringP, int levelQ, int levelP, const uint64_t* skQ, const uint64_t* skP, int nsk, const uint64_t* ptQ, int npt,
                         uint64_t* outQ, uint64_t* outP, const uint64_t* rowtab, int outs, int max_terms, uint64_t* table_dev, size_t table_words);

#ifdef __cplusplus
}
#endif
#endif

// ringhip.hpp -- C++ host-side mirror of the reference's `ring` interface over the C ABI (ringhip.h).
//
// The reference is compiled Go; this image has no Go toolchain, so the compiled-language host side is C++ (the Go/cgo
// binding is go/ringhip/).  Names, argument order and error behaviour follow the reference: methods that panic in Go
// throw ringhip::Panic here (ring/ntt.go:212-214), constructors that return `error` throw ringhip::Error
// (ring/ring.go:321-331).  Header-only; link with -lringhip.
#pragma once
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "ringhip.h"

namespace ringhip {

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };   // Go `error`
struct Panic : std::logic_error { using std::logic_error::logic_error; };         // Go `panic`

inline void check(int rc) {
  if (rc == RH_OK) return;
  const std::string msg = rh_last_error();
  if (rc == RH_ERR_ARG) throw Panic(msg);
  throw Error(msg);
}

enum class Type { Standard = RH_RING_STANDARD, ConjugateInvariant = RH_RING_CI, Matrix = RH_RING_3N };   // ring.Type

class Ring;

// Device-resident block of `npoly` polynomials with `limbs` limbs: the device form of ring.Poly (ring/poly.go:13-24)
class Poly {
 public:
  Poly(const Ring& r, int npoly, int limbs);
  ~Poly();
  Poly(const Poly&) = delete;
  Poly& operator=(const Poly&) = delete;
  Poly(Poly&& o) noexcept : ring_(o.ring_), ptr_(o.ptr_), npoly_(o.npoly_), limbs_(o.limbs_) { o.ptr_ = nullptr; }
  uint64_t* data() const { return ptr_; }
  int npoly() const { return npoly_; }
  int limbs() const { return limbs_; }
  size_t words() const;
  void upload(const std::vector<uint64_t>& host);          // host layout: [poly][limb][coeff]
  std::vector<uint64_t> download() const;
 private:
  const Ring* ring_; uint64_t* ptr_ = nullptr; int npoly_, limbs_;
};

// one modulus of a Ring: the NumberTheoreticTransformer seam (ring/ntt.go:17-22), host slices, one limb per call
class SubRing {
 public:
  SubRing(rh_ring* h, int idx, int n, uint64_t q) : N(n), Modulus(q), h_(h), idx_(idx) {}
  const int N; const uint64_t Modulus;
  void NTT(const std::vector<uint64_t>& p1, std::vector<uint64_t>& p2) const { call(rh_ntt_forward, p1, p2); }
  void NTTLazy(const std::vector<uint64_t>& p1, std::vector<uint64_t>& p2) const { call(rh_ntt_forward_lazy, p1, p2); }
  void INTT(const std::vector<uint64_t>& p1, std::vector<uint64_t>& p2) const { call(rh_ntt_backward, p1, p2); }
  void INTTLazy(const std::vector<uint64_t>& p1, std::vector<uint64_t>& p2) const { call(rh_ntt_backward_lazy, p1, p2); }
 private:
  template <class F> void call(F f, const std::vector<uint64_t>& p1, std::vector<uint64_t>& p2) const {
    if ((int)p1.size() < N || (int)p2.size() < N)
      throw Panic("cannot NTT: ensure that len(p1)=" + std::to_string(p1.size()) + ", len(p2)=" + std::to_string(p2.size()) + " >= N=" + std::to_string(N));
    check(f(h_, idx_, p1.data(), p2.data()));
  }
  rh_ring* h_; int idx_;
};

// what a SubRing holds per modulus (ring/subring.go:35-55, NTTTable ring/ntt.go:38-44), concatenated over the limbs:
// roots_* have N words per limb (Standard) or 2N (ConjugateInvariant, NthRoot = 4N); omega3n is the 3N transformer's psi3N
struct Constants { std::vector<uint64_t> mred, bred, ninv, roots_fwd, roots_bwd, omega3n; };

class Ring {
 public:
  // NewRing / NewRingConjugateInvariant / NewRingFromType(.., Matrix) (ring/ring.go:264-308): constants generated with the
  // reference's rules.  Type::Matrix: omega3n (one primitive 3N-th root per modulus) may be given, as the Go transformer draws
  // its own at random (ring/ntt_3n.go:39, primes_3n.go:127-149); default g^((q-1)/3N).
  Ring(int N, const std::vector<uint64_t>& moduli, Type type = Type::Standard, int device = 0, const std::vector<uint64_t>* omega3n = nullptr)
      : N_(N), type_(type), moduli_(moduli), level_((int)moduli.size() - 1) {
    rh_ring* h = nullptr;
    check(rh_ring_create_auto(&h, device, (int)type, N, (int)moduli.size(), moduli.data(), omega3n ? omega3n->data() : nullptr));
    adopt(h);
  }
  // NewRingWithCustomNTT (ring/ring.go:314-356): the constants handoff -- the engine receives what the host side generated and
  // never re-derives a root (this is the constructor the cgo factories Factory / FactoryCI / Factory3N use, go/ringhip)
  Ring(int N, const std::vector<uint64_t>& moduli, Type type, const Constants& c, int device = 0)
      : N_(N), type_(type), moduli_(moduli), level_((int)moduli.size() - 1) {
    rh_ring* h = nullptr;
    auto ptr = [](const std::vector<uint64_t>& v) { return v.empty() ? nullptr : v.data(); };
    check(rh_ring_create(&h, device, (int)type, N, (int)moduli.size(), moduli.data(), ptr(c.mred), ptr(c.bred), ptr(c.ninv), ptr(c.roots_fwd),
                         ptr(c.roots_bwd), ptr(c.omega3n)));
    adopt(h);
  }
  Type GetType() const { return type_; }
  Constants GetConstants() const {
    const size_t L = moduli_.size(), TN = type_ == Type::ConjugateInvariant ? (size_t)2 * N_ : (size_t)N_;
    Constants c;
    c.mred.resize(L); c.bred.resize(2 * L); c.ninv.resize(L);
    if (type_ == Type::Matrix) {
      c.omega3n.resize(L);
      check(rh_ring_get_constants(h_.get(), nullptr, c.mred.data(), c.bred.data(), nullptr, nullptr, nullptr, c.omega3n.data()));
    } else {
      c.roots_fwd.resize(L * TN); c.roots_bwd.resize(L * TN);
      check(rh_ring_get_constants(h_.get(), nullptr, c.mred.data(), c.bred.data(), c.ninv.data(), c.roots_fwd.data(), c.roots_bwd.data(), nullptr));
    }
    return c;
  }
  void Reserve(int npoly) const { check(rh_ring_reserve(h_.get(), npoly)); }
  int N() const { return N_; }
  int Level() const { return level_; }
  int ModuliChainLength() const { return (int)moduli_.size(); }
  const std::vector<uint64_t>& ModuliChain() const { return moduli_; }
  rh_ring* handle() const { return h_.get(); }
  // view restricted to limbs 0..level (ring/ring.go:194-213); shares the engine handle
  Ring AtLevel(int level) const {
    if (level < 0 || level >= (int)moduli_.size()) throw Panic("level out of range");
    Ring v(*this); v.level_ = level; return v;
  }
  Poly NewPoly(int npoly = 1) const { return Poly(*this, npoly, level_ + 1); }
  void Sync() const { check(rh_ring_sync(h_.get())); }

  // polys may carry more limbs than the view's level (AtLevel on max-level polys, ring/ring.go:192-213): the *_rows entry points
  void NTT(const Poly& p1, Poly& p2) const { check(rh_ring_ntt_rows(h_.get(), p1.data(), p1.limbs(), p2.data(), p2.limbs(), p1.npoly(), level_, 0)); }
  void NTTLazy(const Poly& p1, Poly& p2) const { check(rh_ring_ntt_rows(h_.get(), p1.data(), p1.limbs(), p2.data(), p2.limbs(), p1.npoly(), level_, 1)); }
  void INTT(const Poly& p1, Poly& p2) const { check(rh_ring_intt_rows(h_.get(), p1.data(), p1.limbs(), p2.data(), p2.limbs(), p1.npoly(), level_, 0)); }
  void INTTLazy(const Poly& p1, Poly& p2) const { check(rh_ring_intt_rows(h_.get(), p1.data(), p1.limbs(), p2.data(), p2.limbs(), p1.npoly(), level_, 1)); }
  // Ring.NTT / NTTLazy / INTT / INTTLazy on a whole HOST poly in one call (ring/ntt.go:127-152: the loop over Poly.Coeffs [][]uint64):
  // coeffs[i] = limb i's slice (>= N words; pageable, or page-locked memory from rh_host_alloc / rh_host_register), limbs 0..level of this view
  void NTT(const std::vector<const uint64_t*>& p1, const std::vector<uint64_t*>& p2) const { hostPoly(rh_ntt_poly_forward, p1, p2, 0); }
  void NTTLazy(const std::vector<const uint64_t*>& p1, const std::vector<uint64_t*>& p2) const { hostPoly(rh_ntt_poly_forward, p1, p2, 1); }
  void INTT(const std::vector<const uint64_t*>& p1, const std::vector<uint64_t*>& p2) const { hostPoly(rh_ntt_poly_backward, p1, p2, 0); }
  void INTTLazy(const std::vector<const uint64_t*>& p1, const std::vector<uint64_t*>& p2) const { hostPoly(rh_ntt_poly_backward, p1, p2, 1); }
  // 3N rings: the NTT-domain layout as an argument of the call (the host tags its blocks: DevicePoly.layout in Python, DevPoly.BlockOrder in Go)
  bool BlockOrderSupported() const { return rh_ring_ntt3n_block_order_supported(h_.get()) != 0; }
  void NTTLayout(const Poly& p1, Poly& p2, bool blockOrder) const {
    check(rh_ring_ntt_layout(h_.get(), p1.data(), p1.limbs(), p2.data(), p2.limbs(), p1.npoly(), level_, 0, blockOrder ? 1 : 0));
  }
  void INTTLayout(const Poly& p1, Poly& p2, bool blockOrder) const {
    check(rh_ring_ntt_layout(h_.get(), p1.data(), p1.limbs(), p2.data(), p2.limbs(), p1.npoly(), level_, 1, blockOrder ? 1 : 0));
  }
  void NTT3NReorder(const Poly& p1, Poly& p2, bool toReference) const { check(rh_ring_ntt3n_reorder(h_.get(), p1.data(), p2.data(), p1.npoly(), level_, toReference ? 1 : 0)); }
  long Stats(const char* key) const { long v = 0; check(rh_ring_stats(h_.get(), key, &v)); return v; }
  // c = INTT(NTT(a) . NTT(b)) from coefficient-domain operands (BASELINE config 3) with the tile stages of all three transforms as one kernel;
  // a and b are consumed (rh_ring_polymul)
  void PolyMul(Poly& a, Poly& b, Poly& c) const { check(rh_ring_polymul(h_.get(), a.data(), b.data(), c.data(), a.npoly(), level_)); }
  // Ring.NTT on several blocks in one call (rh_ring_ntt_many): every poly of a block at this view's level (limbs() == level + 1)
  void NTTMany(const std::vector<std::pair<const Poly*, Poly*>>& blocks) const {
    std::vector<const uint64_t*> in; std::vector<uint64_t*> out; std::vector<int> cnt;
    for (const auto& b : blocks) {
      if (b.first->limbs() != level_ + 1 || b.second->limbs() != level_ + 1) throw std::invalid_argument("NTTMany: blocks must hold level+1 limbs per poly");
      in.push_back(b.first->data()); out.push_back(b.second->data()); cnt.push_back(b.first->npoly());
    }
    check(rh_ring_ntt_many(h_.get(), in.data(), out.data(), cnt.data(), (int)in.size(), level_));
  }

  // ring/operations.go -> ring/vec_ops.go
  void VecOp(int op, const Poly* p1, const Poly* p2, Poly& p3, const uint64_t* s0 = nullptr, const uint64_t* s1 = nullptr) const {
    check(rh_ring_vec_op_rows(h_.get(), op, p1 ? p1->data() : nullptr, p1 ? p1->limbs() : 0, p2 ? p2->data() : nullptr, p2 ? p2->limbs() : 0,
                              p3.data(), p3.limbs(), p3.npoly(), level_, s0, s1));
  }
  void Add(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_ADD, &a, &b, c); }
  void Sub(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_SUB, &a, &b, c); }
  void Neg(const Poly& a, Poly& c) const { VecOp(RH_OP_NEG, &a, nullptr, c); }
  void Reduce(const Poly& a, Poly& c) const { VecOp(RH_OP_REDUCE, &a, nullptr, c); }
  void MForm(const Poly& a, Poly& c) const { VecOp(RH_OP_MFORM, &a, nullptr, c); }
  void IMForm(const Poly& a, Poly& c) const { VecOp(RH_OP_IMFORM, &a, nullptr, c); }
  void MulCoeffsBarrett(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_MUL_BARRETT, &a, &b, c); }
  void MulCoeffsMontgomery(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_MUL_MONT, &a, &b, c); }
  void MulCoeffsMontgomeryThenAdd(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_MUL_MONT_THEN_ADD, &a, &b, c); }
  void MulCoeffsMontgomeryLazy(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_MUL_MONT_LAZY, &a, &b, c); }
  void MulCoeffsMontgomeryLazyThenAddLazy(const Poly& a, const Poly& b, Poly& c) const { VecOp(RH_OP_MUL_MONT_LAZY_THEN_ADD_LAZY, &a, &b, c); }
  // ring/scaling.go
  void DivRoundByLastModulusManyNTT(int nb, const Poly& p0, Poly& p1) const {
    check(rh_ring_div_by_last_modulus_many_ntt(h_.get(), 1, level_, nb, p0.data(), p1.data(), p1.limbs(), p0.npoly()));
  }
  void DivFloorByLastModulusManyNTT(int nb, const Poly& p0, Poly& p1) const {
    check(rh_ring_div_by_last_modulus_many_ntt(h_.get(), 0, level_, nb, p0.data(), p1.data(), p1.limbs(), p0.npoly()));
  }
  // ring/automorphism.go
  // ckks mulRelin's degree-1 x degree-1 tensoring as one kernel (schemes/ckks/evaluator.go:821-834)
  void TensorDegree1(const Poly& a0, const Poly& a1, const Poly& b0, const Poly& b1, Poly& c0, Poly& c1, Poly& c2, bool mformFirst = true) const {
    check(rh_ring_tensor_degree1(h_.get(), a0.data(), a1.data(), b0.data(), b1.data(), c0.data(), c1.data(), c2.data(), a0.npoly(), level_, mformFirst ? 1 : 0));
  }
  // CKKS: a baby step of the polynomial evaluator as one kernel (rh_ckks_linear_combination): out_j = [j == 0] c + sum_k s_k X_k,j.  terms[k]: the
  // components of X_k (each term as many as `out`), s0 / s1: terms.size() rows of level + 1 scalars, c0 / c1: the constant's or null; table: device
  // scratch of the caller of at least LinearCombinationTableWords(terms.size()) words
  size_t LinearCombinationTableWords(size_t nterms) const { return rh_ckks_linear_combination_table_words((int)nterms, level_); }
  void LinearCombination(const std::vector<std::vector<const Poly*>>& terms, const uint64_t* s0, const uint64_t* s1, const uint64_t* c0, const uint64_t* c1,
                         const std::vector<Poly*>& out, uint64_t* table, size_t tableWords) const {
    if (out.empty() || out.size() > 3) throw std::invalid_argument("LinearCombination: one to three output components");
    std::vector<const uint64_t*> x(3 * terms.size(), nullptr); std::vector<int> rows(terms.size(), 0);
    for (size_t k = 0; k < terms.size(); ++k) {
      if (terms[k].size() != out.size()) throw std::invalid_argument("LinearCombination: every term has the output's components");
      for (size_t j = 0; j < out.size(); ++j) x[3 * k + j] = terms[k][j]->data();
      rows[k] = terms[k][0]->limbs();
    }
    check(rh_ckks_linear_combination(h_.get(), level_, (int)terms.size(), x.data(), rows.data(), s0, s1, c0, c1, out[0]->data(), out.size() > 1 ? out[1]->data() : nullptr,
                                     out.size() > 2 ? out[2]->data() : nullptr, out[0]->npoly(), table, tableWords));
  }
  // BGV (schemes/bgv/evaluator.go): tensorStandard / mulRelinThenAdd ct x ct as one kernel, k[i] = T r0 2^128 mod q_i; b0 / b1 null: squaring;
  // accumulate 0 / 1 / 2 and r1 (null or MForm(r1) per limb) as rh_bgv_tensor takes them.  BgvAxpby: out = r0 a +- r1 b (an operand and its scalar may be null)
  void BgvTensor(const Poly& a0, const Poly& a1, const Poly* b0, const Poly* b1, Poly& c0, Poly& c1, Poly& c2, const uint64_t* k, const uint64_t* r1 = nullptr,
                 int accumulate = 0) const {
    check(rh_bgv_tensor(h_.get(), level_, a0.data(), a1.data(), b0 ? b0->data() : nullptr, b1 ? b1->data() : nullptr, c0.data(), c1.data(), c2.data(), a0.npoly(), k, r1, accumulate));
  }
  void BgvMulPlain(const Poly& ct0, const Poly* ct1, const Poly* ct2, const Poly& pt, Poly& out0, Poly* out1, Poly* out2, const uint64_t* k, const uint64_t* r1 = nullptr,
                   int accumulate = 0) const {
    check(rh_bgv_mul_plain(h_.get(), level_, ct0.data(), ct1 ? ct1->data() : nullptr, ct2 ? ct2->data() : nullptr, pt.data(), out0.data(), out1 ? out1->data() : nullptr,
                           out2 ? out2->data() : nullptr, ct0.npoly(), k, r1, accumulate));
  }
  void BgvAxpby(const Poly* a, const Poly* b, Poly& out, const uint64_t* r0, const uint64_t* r1, bool sub = false) const {
    check(rh_bgv_axpby(h_.get(), level_, a ? a->data() : nullptr, b ? b->data() : nullptr, out.data(), out.npoly(), r0, r1, sub ? 1 : 0));
  }
  // BGV: a baby step of the polynomial evaluator over a mapping as one kernel (rh_bgv_plain_combination): out_j = [j == 0] c cScalar + sum_k X_k,j (.) m_k.
  // terms[k]: the components of X_k (each term as many as `out`); m[k] and c (null: no constant, then cScalar null too): one shared poly each, NTT domain,
  // Montgomery form; table: device scratch of the caller of at least PlainCombinationTableWords(terms.size()) words
  static size_t PlainCombinationTableWords(size_t nterms) { return rh_bgv_plain_combination_table_words((int)nterms); }
  void BgvPlainCombination(const std::vector<std::vector<const Poly*>>& terms, const std::vector<const Poly*>& m, const Poly* c, const uint64_t* cScalar,
                           const std::vector<Poly*>& out, uint64_t* table, size_t tableWords) const {
    if (out.empty() || out.size() > 3) throw std::invalid_argument("BgvPlainCombination: one to three output components");
    if (m.size() != terms.size()) throw std::invalid_argument("BgvPlainCombination: one plaintext per term");
    std::vector<const uint64_t*> x(3 * terms.size(), nullptr), pm(terms.size(), nullptr); std::vector<int> rows(terms.size(), 0);
    for (size_t k = 0; k < terms.size(); ++k) {
      if (terms[k].size() != out.size()) throw std::invalid_argument("BgvPlainCombination: every term has the output's components");
      for (size_t j = 0; j < out.size(); ++j) x[3 * k + j] = terms[k][j]->data();
      rows[k] = terms[k][0]->limbs();
      pm[k] = m[k]->data();
    }
    check(rh_bgv_plain_combination(h_.get(), level_, (int)terms.size(), x.data(), rows.data(), pm.data(), c ? c->data() : nullptr, cScalar, out[0]->data(),
                                   out.size() > 1 ? out[1]->data() : nullptr, out.size() > 2 ? out[2]->data() : nullptr, out[0]->npoly(), table, tableWords));
  }
  void AutomorphismNTT(const Poly& in, uint64_t gen, Poly& out) const { check(rh_ring_automorphism_ntt(h_.get(), level_, in.data(), gen, out.data(), in.npoly(), 0)); }
  void Automorphism(const Poly& in, uint64_t gen, Poly& out) const { check(rh_ring_automorphism(h_.get(), level_, in.data(), gen, out.data(), in.npoly())); }
  // ct_c += phi_gen(tmp_c) modulo Q, both components in one launch: the end of AutomorphismHoisted + ringQ.Add (core/rlwe/inner_sum.go:279-280)
  void RotateAddQ(uint64_t gen, const Poly& tmp0, const Poly& tmp1, Poly& ct0, Poly& ct1) const {
    check(rh_rlwe_rotate_add_q(h_.get(), level_, gen, tmp0.data(), tmp1.data(), ct0.data(), ct1.data(), ct0.npoly()));
  }
  // core/rlwe/ring_packing.go, one level at a time over a batch (see ringhip.h): ExpandStep (:555-575), PackCombine / RotateAddSubQ (:726-787) with the
  // level's table of (mode, slot_a, slot_b) on the device and on the host, RingSplit / RingMerge (element.go:250-312, ring/operations.go:380-392)
  void ExpandStep(uint64_t gen, const Poly& tmp0, const Poly& tmp1, Poly& ct0, Poly& ct1, const Poly& xpow, int cnt) const {
    check(rh_rlwe_expand_step(h_.get(), level_, gen, tmp0.data(), tmp1.data(), ct0.data(), ct1.data(), xpow.data(), cnt));
  }
  void PackCombine(Poly& ct0, Poly& ct1, const int32_t* table_dev, const std::vector<int32_t>& table, const Poly& xpow, Poly& u0, Poly& u1) const {
    check(rh_rlwe_pack_combine(h_.get(), level_, ct0.data(), ct1.data(), ct0.npoly(), table_dev, table.data(), (int)(table.size() / 3), xpow.data(), u0.data(), u1.data()));
  }
  void RotateAddSubQ(uint64_t gen, const Poly& tmp0, const Poly& tmp1, Poly& ct0, Poly& ct1, const int32_t* table_dev, const std::vector<int32_t>& table) const {
    check(rh_rlwe_rotate_addsub_q(h_.get(), level_, gen, tmp0.data(), tmp1.data(), ct0.data(), ct1.data(), ct0.npoly(), table_dev, table.data(), (int)(table.size() / 3)));
  }
  void RingSplit(const Poly& in0, const Poly& in1, Poly& even0, Poly& even1, Poly* odd0, Poly* odd1, int logGap = 1) const {
    check(rh_rlwe_ring_split(h_.get(), level_, in0.data(), in1.data(), even0.data(), even1.data(), odd0 ? odd0->data() : nullptr, odd1 ? odd1->data() : nullptr, logGap, in0.npoly()));
  }
  void RingMerge(const Poly& even0, const Poly& even1, const Poly* odd0, const Poly* odd1, const Poly* xpow, Poly& out0, Poly& out1, int logGap = 1) const {
    check(rh_rlwe_ring_merge(h_.get(), level_, even0.data(), even1.data(), odd0 ? odd0->data() : nullptr, odd1 ? odd1->data() : nullptr, xpow ? xpow->data() : nullptr,
                             out0.data(), out1.data(), logGap, out0.npoly()));
  }
  // AutomorphismNTTWithIndex / ...ThenAddLazy (ring/automorphism.go:50-117): `index` = a 1-poly, 1-limb device block holding the lookup table
  void AutomorphismNTTWithIndex(const Poly& in, const Poly& index, Poly& out, bool thenAddLazy = false) const {
    check(rh_ring_automorphism_ntt_index(h_.get(), level_, in.data(), index.data(), out.data(), in.npoly(), thenAddLazy ? 1 : 0));
  }
  // ring/operations.go: Poly.CopyLvl, Shift (:278-282), MultByMonomial (:306-363), MulByVectorMontgomery(ThenAddLazy) (:366-377); out of place
  void CopyLvl(const Poly& p1, Poly& p2) const { check(rh_ring_copy_rows(h_.get(), p2.data(), p2.limbs(), p1.data(), p1.limbs(), p1.npoly(), level_)); }
  // ring/conjugate_invariant.go: UnfoldConjugateInvariantToStandard (:8-26, receiver: standard ring of degree 2n), FoldStandardToConjugateInvariant
  // (:31-49, receiver: conjugate-invariant ring of degree n; index: device table of n words < 2n), PadDefaultRingToConjugateInvariant (:52-80)
  void UnfoldConjugateInvariantToStandard(const Poly& ci, Poly& std_) const { check(rh_ring_unfold_ci_to_standard(h_.get(), level_, ci.data(), std_.data(), std_.npoly())); }
  void FoldStandardToConjugateInvariant(const Poly& std_, const Poly& index, Poly& ci) const {
    check(rh_ring_fold_standard_to_ci(h_.get(), level_, std_.data(), index.data(), ci.data(), std_.npoly()));
  }
  void PadDefaultRingToConjugateInvariant(const Poly& std_, bool isNTT, Poly& ci) const {
    check(rh_ring_pad_default_to_ci(h_.get(), level_, std_.data(), isNTT ? 1 : 0, ci.data(), std_.npoly()));
  }
  // the tail of ckks.DomainSwitcher.ComplexToReal (schemes/ckks/bridge.go:79-83) in one launch; receiver: the conjugate-invariant ring of degree n
  void BridgeFoldTail(const Poly& g0, const Poly& g1, const Poly& c0, const Poly& index, Poly& out0, Poly& out1) const {
    check(rh_ckks_bridge_fold_tail(h_.get(), level_, g0.data(), g1.data(), c0.data(), index.data(), out0.data(), out1.data(), g0.npoly()));
  }
  void Shift(const Poly& p1, int k, Poly& p2) const { check(rh_ring_shift(h_.get(), level_, p1.data(), p2.data(), k, p1.npoly())); }
  void MultByMonomial(const Poly& p1, int k, Poly& p2) const { check(rh_ring_mult_by_monomial(h_.get(), level_, p1.data(), p2.data(), k, p1.npoly())); }
  void MulByVectorMontgomery(const Poly& p1, const Poly& vector, Poly& p2, bool thenAddLazy = false) const {
    check(rh_ring_vec_op_bcast(h_.get(), thenAddLazy ? RH_OP_MUL_MONT_THEN_ADD_LAZY : RH_OP_MUL_MONT, p1.data(), p1.limbs(), vector.data(), p2.data(),
                               p2.limbs(), p1.npoly(), level_));
  }
  // MForm + MulCoeffsMontgomery + INTT as one call (schemes/ckks/evaluator.go:821-834 + INTT)
  void INTTMul(const Poly& a, const Poly& b, Poly& out) const { check(rh_ring_intt_mul(h_.get(), a.data(), b.data(), out.data(), a.npoly(), level_)); }

  // The exact sums behind Log2OfStandardDeviation (ring/ring.go:647-686) of every poly of a coefficient-domain block, modulo Q (this ring) or, with
  // ringP, modulo QP: rh_ring_centered_moments_words(limbs) words per poly into `out` (device), laid out as ringhip.h documents
  void CenteredMoments(const Poly& q, uint64_t* out, int gap = 1, const Ring* ringP = nullptr, const Poly* p = nullptr) const {
    check(rh_ring_centered_moments(h_.get(), level_, q.data(), q.limbs(), ringP ? ringP->handle() : nullptr, ringP ? ringP->level_ : 0,
                                   p ? p->data() : nullptr, p ? p->limbs() : 0, gap, q.npoly(), out));
  }

  std::vector<SubRing> SubRings;
 private:
  template <class F> void hostPoly(F f, const std::vector<const uint64_t*>& p1, const std::vector<uint64_t*>& p2, int lazy) const {
    if ((int)p1.size() < level_ + 1 || (int)p2.size() < level_ + 1)
      throw Panic("cannot NTT: poly has " + std::to_string(p1.size()) + " / " + std::to_string(p2.size()) + " limbs, ring level needs " + std::to_string(level_ + 1));
    check(f(h_.get(), level_, p1.data(), p2.data(), lazy));
  }
  void adopt(rh_ring* h) {
    h_.reset(h, rh_ring_destroy);
    for (int i = 0; i < (int)moduli_.size(); ++i) SubRings.emplace_back(h, i, N_, moduli_[i]);
  }
  int N_; Type type_; std::vector<uint64_t> moduli_; int level_;
  std::shared_ptr<rh_ring> h_;
};

inline Poly::Poly(const Ring& r, int npoly, int limbs) : ring_(&r), npoly_(npoly), limbs_(limbs) {
  check(rh_dev_alloc(r.handle(), words() ? words() : 1, &ptr_));
}
inline Poly::~Poly() { if (ptr_) rh_dev_free(nullptr, ptr_); }
inline size_t Poly::words() const { return (size_t)npoly_ * limbs_ * ring_->N(); }
inline void Poly::upload(const std::vector<uint64_t>& host) {
  if (host.size() < words()) throw Panic("upload: host vector too short");
  check(rh_dev_upload(ring_->handle(), ptr_, host.data(), words()));
}
inline std::vector<uint64_t> Poly::download() const {
  std::vector<uint64_t> out(words());
  check(rh_dev_download(ring_->handle(), out.data(), ptr_, words()));
  return out;
}

// ring.BasisExtender (ring/basis_extension.go:13-79) + the key-switch gadget product built on it
class BasisExtender {
 public:
  BasisExtender(const Ring& q, const Ring& p) { rh_bext* h = nullptr; check(rh_bext_create(&h, q.handle(), p.handle())); h_.reset(h, rh_bext_destroy); }
  void Reserve(int npoly) const { check(rh_bext_reserve(h_.get(), npoly)); }
  void ModUpQtoP(int lq, int lp, const Poly& polQ, Poly& polP) const { check(rh_bext_modup_q_to_p(h_.get(), lq, lp, polQ.data(), polP.data(), polQ.npoly())); }
  void ModUpPtoQ(int lp, int lq, const Poly& polP, Poly& polQ) const { check(rh_bext_modup_p_to_q(h_.get(), lp, lq, polP.data(), polQ.data(), polP.npoly())); }
  void ModDownQPtoQ(int lq, int lp, const Poly& q1, const Poly& p1, Poly& q2) const { check(rh_bext_moddown_qp_to_q(h_.get(), lq, lp, q1.data(), p1.data(), q2.data(), q1.npoly())); }
  void ModDownQPtoQNTT(int lq, int lp, const Poly& q1, const Poly& p1, Poly& q2) const { check(rh_bext_moddown_qp_to_q_ntt(h_.get(), lq, lp, q1.data(), p1.data(), q2.data(), q1.npoly())); }
  void ModDownQPtoP(int lq, int lp, const Poly& q1, const Poly& p1, Poly& p2) const { check(rh_bext_moddown_qp_to_p(h_.get(), lq, lp, q1.data(), p1.data(), p2.data(), q1.npoly())); }
  void DecomposeAndSplit(int lq, int lp, int nbPi, int digit, const Poly& p0Q, Poly& p1Q, Poly& p1P) const {
    check(rh_bext_decompose_and_split(h_.get(), lq, lp, nbPi, digit, p0Q.data(), p1Q.data(), p1P.data(), p0Q.npoly()));
  }
  void GadgetProduct(int lq, int lp, const Poly& cx, const Poly& evkQ, const Poly& evkP, int beta, Poly& ct0, Poly& ct1) const {
    check(rh_bext_gadget_product(h_.get(), lq, lp, cx.data(), evkQ.data(), evkP.data(), beta, ct0.data(), ct1.data(), cx.npoly()));
  }
  // ct_c = add_c + GadgetProduct(cx)_c: the ring.Add that follows the product in Relinearize / mulRelin / Automorphism,
  // folded into ModDown's epilogue (add0 / add1 may be null and may alias ct0 / ct1)
  void GadgetProductThenAdd(int lq, int lp, const Poly& cx, const Poly& evkQ, const Poly& evkP, int beta, const Poly* add0, const Poly* add1,
                            Poly& ct0, Poly& ct1) const {
    check(rh_bext_gadget_product_then_add(h_.get(), lq, lp, cx.data(), evkQ.data(), evkP.data(), beta, add0 ? add0->data() : nullptr,
                                          add1 ? add1->data() : nullptr, ct0.data(), ct1.data(), cx.npoly()));
  }
  // Evaluator.DecomposeNTT / GadgetProductHoisted (core/rlwe/evaluator_gadget_product.go:431-453, 326-429): decompQ / decompP
  // hold beta * npoly polys (digit i of poly k = poly i*npoly + k)
  void DecomposeNTT(int lq, int lp, const Poly& c2, bool c2IsNTT, Poly& decompQ, Poly& decompP) const {
    check(rh_bext_decompose_ntt(h_.get(), lq, lp, c2.data(), c2IsNTT ? 1 : 0, decompQ.data(), decompP.data(), c2.npoly()));
  }
  void GadgetProductHoisted(int lq, int lp, const Poly& decompQ, const Poly& decompP, const Poly& evkQ, const Poly& evkP, int beta,
                            Poly& ct0, Poly& ct1) const {
    check(rh_bext_gadget_product_hoisted(h_.get(), lq, lp, decompQ.data(), decompP.data(), evkQ.data(), evkP.data(), beta, ct0.data(),
                                         ct1.data(), ct0.npoly()));
  }
  // GadgetProductHoistedLazy (:351-371): the accumulators modulo Q and modulo P, no ModDown; ModDownPair: Evaluator.ModDown (:33-46) NTT -> NTT
  void GadgetProductHoistedLazy(int lq, int lp, const Poly& decompQ, const Poly& decompP, const Poly& evkQ, const Poly& evkP, int beta,
                                Poly& ctQ0, Poly& ctQ1, Poly& ctP0, Poly& ctP1) const {
    check(rh_bext_gadget_product_hoisted_lazy(h_.get(), lq, lp, decompQ.data(), decompP.data(), evkQ.data(), evkP.data(), beta, ctQ0.data(),
                                              ctQ1.data(), ctP0.data(), ctP1.data(), ctQ0.npoly()));
  }
  void ModDownPair(int lq, int lp, const Poly& ctQ0, const Poly& ctQ1, const Poly& ctP0, const Poly& ctP1, Poly& ct0, Poly& ct1) const {
    check(rh_bext_moddown_qp_to_q_ntt_pair(h_.get(), lq, lp, ctQ0.data(), ctQ1.data(), ctP0.data(), ctP1.data(), ct0.data(), ct1.data(), ct0.npoly()));
  }
  // Evaluator.PartialTracesSum (core/rlwe/inner_sum.go:152-291) as one call: out = sum_{i < n} phi_{5^(i offset)}(in); keys: the caller's table of
  // Galois keys (element, evkQ, evkP, digits); out may be in.  RotateAccumulateQP: the tail of AutomorphismHoistedLazy + ringQP.Add (:245-246)
  void PartialTracesSum(int lq, int lp, const Poly& in0, const Poly& in1, bool isNTT, int offset, int n, const std::vector<rh_galois_key>& keys,
                        Poly& out0, Poly& out1, bool fused = true) const {
    check(rh_rlwe_partial_traces_sum(h_.get(), lq, lp, in0.data(), in1.data(), isNTT ? 1 : 0, offset, n, keys.data(), (int)keys.size(), out0.data(),
                                     out1.data(), in0.npoly(), fused ? 1 : 0));
  }
  // RingPackingEvaluator.Expand (core/rlwe/ring_packing.go:475-594) as one call: ct0 / ct1 hold nin << (logN - logGap) polys, the nin inputs first
  void Expand(int lq, int lp, Poly& ct0, Poly& ct1, int nin, int logGap, const Poly& xinvpow, const std::vector<rh_galois_key>& keys) const {
    check(rh_rlwe_expand(h_.get(), lq, lp, ct0.data(), ct1.data(), nin, logGap, xinvpow.data(), xinvpow.limbs(), keys.data(), (int)keys.size()));
  }
  void RotateAccumulateQP(int lq, int lp, uint64_t galEl, const Poly& ct0, const Poly& tmpQ0, const Poly& tmpQ1, const Poly& tmpP0, const Poly& tmpP1,
                          Poly& accQ0, Poly& accQ1, Poly& accP0, Poly& accP1, bool first) const {
    check(rh_rlwe_rotate_accumulate_qp(h_.get(), lq, lp, galEl, ct0.data(), tmpQ0.data(), tmpQ1.data(), tmpP0.data(), tmpP1.data(), accQ0.data(),
                                       accQ1.data(), accP0.data(), accP1.data(), ct0.npoly(), first ? 1 : 0));
  }
  // The three streaming passes of the diagonal matrix x ciphertext product (circuits/common/lintrans/lintrans_evaluator.go): the inner loop of
  // MultiplyByDiagMatrixBSGS for one giant step (:311-357), its giant-step tail (:384-393), one diagonal of MultiplyByDiagMatrix (:200-218).
  // DiagMacQP: per term one diagonal (ptQ, ptP: one poly each) and four blocks {xQ0, xQ1, xP0, xP1} (xP0 = xP1 = nullptr: the baby step 0 term);
  // table: the caller's device scratch of DiagMacTableWords(nterms, lq, lp) words
  static size_t DiagMacTableWords(size_t nterms, int lq, int lp) { return rh_rlwe_diag_mac_qp_table_words((int)nterms, lq, lp); }
  void DiagMacQP(int lq, int lp, const std::vector<const uint64_t*>& ptQ, const std::vector<const uint64_t*>& ptP, const std::vector<const uint64_t*>& x,
                 Poly& tmpQ0, Poly& tmpQ1, Poly& tmpP0, Poly& tmpP1, Poly& table) const {
    check(rh_rlwe_diag_mac_qp(h_.get(), lq, lp, (int)ptQ.size(), ptQ.data(), ptP.data(), x.data(), tmpQ0.data(), tmpQ1.data(), tmpP0.data(), tmpP1.data(),
                              tmpQ0.npoly(), table.data(), table.words()));
  }
  void RotateSumAccumulateQP(int lq, int lp, uint64_t galEl, const Poly& cQ0, const Poly& cQ1, const Poly& cP0, const Poly& cP1, const Poly& tmpQ0,
                             const Poly& tmpP0, Poly& accQ0, Poly& accQ1, Poly& accP0, Poly& accP1, bool first) const {
    check(rh_rlwe_rotate_sum_accumulate_qp(h_.get(), lq, lp, galEl, cQ0.data(), cQ1.data(), cP0.data(), cP1.data(), tmpQ0.data(), tmpP0.data(), accQ0.data(),
                                           accQ1.data(), accP0.data(), accP1.data(), accQ0.npoly(), first ? 1 : 0));
  }
  void RotateMulAccumulateQP(int lq, int lp, uint64_t galEl, const Poly& ptQ, const Poly& ptP, const Poly& ct0, const Poly& cQ0, const Poly& cQ1,
                             const Poly& cP0, const Poly& cP1, Poly& accQ0, Poly& accQ1, Poly& accP0, Poly& accP1, bool first) const {
    check(rh_rlwe_rotate_mul_accumulate_qp(h_.get(), lq, lp, galEl, ptQ.data(), ptP.data(), ct0.data(), cQ0.data(), cQ1.data(), cP0.data(), cP1.data(),
                                           accQ0.data(), accQ1.data(), accP0.data(), accP1.data(), accQ0.npoly(), first ? 1 : 0));
  }
 private:
  std::shared_ptr<rh_bext> h_;
};

// bgv.Evaluator's scale-invariant (BFV) multiply (schemes/bgv/evaluator.go:975-1124): ringQ, ringQMul and the plaintext modulus
class BfvEvaluator {
 public:
  BfvEvaluator(const Ring& q, const Ring& qmul, uint64_t t) { rh_bfv* h = nullptr; check(rh_bfv_create(&h, q.handle(), qmul.handle(), t)); h_.reset(h, rh_bfv_destroy); }
  int LevelQMul(int level) const { int v = rh_bfv_level_qmul(h_.get(), level); if (v < 0) check(v); return v; }
  void Reserve(int npoly) const { check(rh_bfv_reserve(h_.get(), npoly)); }
  void SetTuning(const char* key, long value) const { check(rh_bfv_set_tuning(h_.get(), key, value)); }
  bool QuantizeIsFused(int level) const { int v = rh_bfv_quantize_path(h_.get(), level); if (v < 0) check(v); return v != 0; }
  // tensorLowDeg in both rings; b*: null pointers when squaring
  void TensorLowDeg(int level, const Poly& a0Q, const Poly& a1Q, const Poly* b0Q, const Poly* b1Q, const Poly& a0M, const Poly& a1M, const Poly* b0M,
                    const Poly* b1M, Poly& c0Q, Poly& c1Q, Poly& c2Q, Poly& c0M, Poly& c1M, Poly& c2M) const {
    const bool sq = !b0Q;
    check(rh_bfv_tensor_lazy(h_.get(), level, a0Q.data(), a1Q.data(), sq ? nullptr : b0Q->data(), sq ? nullptr : b1Q->data(), a0M.data(), a1M.data(),
                             sq ? nullptr : b0M->data(), sq ? nullptr : b1M->data(), c0Q.data(), c1Q.data(), c2Q.data(), c0M.data(), c1M.data(),
                             c2M.data(), a0Q.npoly(), sq ? 1 : 0));
  }
  void Quantize(int level, const Poly& cQ, const Poly& cM, Poly& outQ) const { check(rh_bfv_quantize(h_.get(), level, cQ.data(), cM.data(), outQ.data(), cQ.npoly())); }
  // tensorScaleInvariant without relinearisation; b0 / b1 null: squaring; outputs may be the operands' blocks
  void MulScaleInvariant(int level, const Poly& a0, const Poly& a1, const Poly* b0, const Poly* b1, Poly& c0, Poly& c1, Poly& c2) const {
    check(rh_bfv_mul_scale_invariant(h_.get(), level, a0.data(), a1.data(), b0 ? b0->data() : nullptr, b1 ? b1->data() : nullptr, c0.data(), c1.data(),
                                     c2.data(), a0.npoly()));
  }
 private:
  std::shared_ptr<rh_bfv> h_;
};

// bgv.Encoder's state on the device (schemes/bgv/encoder.go:49-96) and the one-pass encoding of a linear transformation
class BgvEncoder {
 public:
  BgvEncoder(const Ring& q, const Ring& t) { rh_bgv_encoder* h = nullptr; check(rh_bgv_encoder_create(&h, q.handle(), t.handle())); h_.reset(h, rh_bgv_encoder_destroy); }
  void Reserve(int nvec) const { check(rh_bgv_encoder_reserve(h_.get(), nvec)); }
  void SetTuning(const char* key, long value) const { check(rh_bgv_encoder_set_tuning(h_.get(), key, value)); }
  // rotateAndEncodeDiagonal (circuits/common/lintrans/lintrans.go:271-292) for outQ.npoly() vectors at once (rh_bgv_embed_qp): values is a device
  // block of nvals words per vector; rot (host, one rotation per vector) may be null
  void EmbedQP(const Ring& p, uint64_t scale, const uint64_t* values, int nvals, bool isSigned, const int* rot, int cols, Poly& outQ, Poly& outP,
               bool isNTT = true, bool isMontgomery = true) const {
    check(rh_bgv_embed_qp(h_.get(), p.handle(), outQ.limbs() - 1, outP.limbs() - 1, scale, values, nvals, isSigned ? 1 : 0, outQ.npoly(), rot, cols,
                          outQ.data(), outP.data(), isNTT ? 1 : 0, isMontgomery ? 1 : 0));
  }
 private:
  std::shared_ptr<rh_bgv_encoder> h_;
};

// limb-sharded key switch (rh_kshard_*): this rank's limbs of the gadget product; the caller moves the
// gathered source limbs (RCCL all-gather) between Digit / ModDown calls
class KeySwitchShard {
 public:
  KeySwitchShard(const Ring& qLoc, const Ring* pLoc, const std::vector<uint64_t>& allQ, const std::vector<uint64_t>& allP,
                 const std::vector<int>& ownQ, const std::vector<int>& ownP) {
    rh_kshard* h = nullptr;
    check(rh_kshard_create(&h, qLoc.handle(), pLoc ? pLoc->handle() : nullptr, allQ.data(), (int)allQ.size() - 1, allP.data(),
                           (int)allP.size() - 1, ownQ.data(), (int)ownQ.size(), ownP.empty() ? ownQ.data() : ownP.data(), (int)ownP.size()));
    h_.reset(h, rh_kshard_destroy);
  }
  int NumDigits() const { return rh_kshard_num_digits(h_.get()); }
  std::pair<int, int> DigitRange(int digit) const { int st = 0, ed = 0; check(rh_kshard_digit_range(h_.get(), digit, &st, &ed)); return {st, ed}; }
  void Digit(int digit, const uint64_t* srcGathered, const Poly& cxLoc, const uint64_t* evkQLoc, const uint64_t* evkPLoc, Poly& ct0, Poly& ct1,
             uint64_t* accP0, uint64_t* accP1) const {
    check(rh_kshard_digit(h_.get(), digit, srcGathered, cxLoc.data(), evkQLoc, evkPLoc, ct0.data(), ct1.data(), accP0, accP1, cxLoc.npoly()));
  }
  // all digits in one call: srcAll = every limb of INTT(cx) in chain order (one all-gather per product)
  void Product(const uint64_t* srcAll, const Poly& cxLoc, const uint64_t* evkQLoc, const uint64_t* evkPLoc, Poly& ct0, Poly& ct1,
               uint64_t* accP0, uint64_t* accP1) const {
    check(rh_kshard_product(h_.get(), srcAll, cxLoc.data(), evkQLoc, evkPLoc, ct0.data(), ct1.data(), accP0, accP1, cxLoc.npoly()));
  }
  void ModDown(const uint64_t* srcPGathered, const Poly& ctIn, Poly& ctOut) const {
    check(rh_kshard_moddown(h_.get(), srcPGathered, ctIn.data(), ctOut.data(), ctIn.npoly()));
  }
  // the whole product in one call (rlwe.Evaluator.GadgetProduct on the owned limbs): the host supplies the all-gather -- ncclAllGather on a node
  // (tests/cpp/test_sharded_host.cpp runs it with threads as ranks).  owner[i]: the rank of limb i of Q ++ P.
  void SetWorld(int world, int rank, const std::vector<int>& owner) const { check(rh_kshard_set_world(h_.get(), world, rank, owner.data())); }
  void GadgetProduct(const Poly& cxLoc, const uint64_t* evkQLoc, const uint64_t* evkPLoc, Poly& ct0, Poly& ct1, rh_allgather_fn allgather, void* ctx,
                     int chunks = 0) const {
    check(rh_kshard_gadget_product(h_.get(), cxLoc.data(), evkQLoc, evkPLoc, ct0.data(), ct1.data(), cxLoc.npoly(), allgather, ctx, chunks));
  }
 private:
  std::shared_ptr<rh_kshard> h_;
};

}  // namespace ringhip

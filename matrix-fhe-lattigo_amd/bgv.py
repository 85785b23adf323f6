"""Host-side mirror of bgv.Evaluator, schemes/bgv/evaluator.go, on device-resident batches in the NTT domain: the scale-invariant (BFV)
multiply and the BGV half -- standard tensoring, multiply-accumulate, Add / Sub with scale matching, scalar operands, Rescale -- and of
bgv.Encoder, schemes/bgv/encoder.go, on device batches of vectors.  Call sequences and the scale bookkeeping (Python ints modulo T) only: the
arithmetic is the HIP library's (csrc/bfv.hip, csrc/bgv.hip, csrc/bgv_encoder.hip); key generation stays with the reference.  An evaluator
built with encoder= takes slice operands ([]uint64 / []int64) the way the reference does: encoded into its buffer at the scale the method
sets, then the plaintext branch.  Without one they are refused by name.

  newEvaluatorPrecomp      :46-78        MulScaleInvariant(New)       :771-857     MulRelinScaleInvariant(New)  :877-972
  tensorScaleInvariant     :975-1040     MulScaleInvariant (scale)    :1045-1051   quantize                     :1104-1124
  Add(New) / Sub(New)      :173-432      evaluateInPlace              :270-286     matchScaleThenEvaluateInPlace :288-305
  Mul(New) / MulRelin(New) :458-663      tensorStandard               :665-751     MulThenAdd / MulRelinThenAdd :1142-1287
  mulRelinThenAdd          :1289-1403    Rescale                      :1415-1445   MatchScalesAndLevel          :1593-1614
  matchScalesBinary        :1620-1659
  encoder.go: NewEncoder :49-96, permuteMatrix :98-121, Encode :130-184, EncodeRingT :187-246, EmbedScale / Embed :252-320,
  DecodeRingT :323-353, RingT2Q :357-386, RingQ2T :391-439, Decode :442-487

A batch of B ciphertexts is one Ciphertext whose polys have npoly = B; all operands of a call sit at the same level (dense
(npoly, level+1, N) blocks), which may be lower than the ring's top: a mismatch raises.  A degree-0 Ciphertext plays the role of a plaintext.
Scales are Python ints modulo T in the attribute Scale (1 when a ciphertext carries none).  In this scheme a ciphertext of scale s has the
phase c0 + c1 s = (m s) T^-1 + e modulo Q: T times the phase is m s + T e."""
import ctypes as C
import math
import threading

import numpy as np

from .ringhip import ConjugateInvariant, DevicePoly, Ring, RingHipError, Standard, _check, _p, _u64, lib
from .schemes import Ciphertext
from . import rlwe


def MulScaleInvariant(t, Q_level, a, b):
    """:1045-1051: the scale after the invariant tensoring, c = a * b / (T - (Q_level mod T)) in rlwe.Scale arithmetic modulo T
    (core/rlwe/scale.go:77-119: the product reduced modulo T, then times the modular inverse of the divisor).  Python ints in and out."""
    t, Q_level = int(t), int(Q_level)
    c = (int(a) * int(b)) % t
    q_mod_t_neg = t - Q_level % t
    try:
        inv = pow(q_mod_t_neg, -1, t)
    except ValueError:
        raise RingHipError("MulScaleInvariant: T - (Q mod T) = %d has no inverse modulo T = %d" % (q_mod_t_neg, t))
    return (c * inv) % t


def center(x, thalf, t):
    """:1661-1666"""
    return t - x if x >= thalf else x


def matchScalesBinary(t, scale0, scale1):
    """:1620-1659: (r0, r1, e) with r0 * scale0 = r1 * scale1 modulo t, gcd(r0, t) = 1 and e = center(r0) + center(r1) the smallest the
    extended Euclid sequence of (t, scale0^-1 * scale1) offers.  scale0^-1 is ModExp(scale0, t - 2, t), as in the reference (t prime)."""
    t, scale0, scale1 = int(t), int(scale0), int(scale1)
    thalf = t >> 1
    if math.gcd(scale0, t) != 1:
        raise RingHipError("cannot matchScalesBinary: invalid ciphertext scale: gcd(scale, t) != 1")
    a, b = t, 0
    A, B = pow(scale0, t - 2, t) * scale1 % t, 1
    r0, r1 = A, B
    e = center(A, thalf, t) + 1
    while A != 0:
        q = a // A
        a, A = A, a % A
        b, B = B, (t + b - B * q % t) % t
        if A != 0 and math.gcd(A, t) == 1:
            tmp = center(A, thalf, t) + center(B, thalf, t)
            if tmp < e:
                e = tmp
                r0, r1 = A, B
    return r0, r1, e


def _is_slice(op):
    return isinstance(op, (list, tuple, np.ndarray))


def _is_values(op):
    return _is_slice(op) or isinstance(op, DeviceValues)


def _is_int(op):
    return isinstance(op, (int, np.integer)) and not isinstance(op, bool)


class Evaluator(rlwe.Evaluator):
    """bgv.Evaluator.  ringQMul: bgv/params.go:98-108 (ceil((bitlen(Q) + logN) / 61) NTT-friendly 61-bit primes disjoint from Q), needed by the
    scale-invariant methods only: None builds a pure BGV evaluator, whose scale-invariant methods raise.  ringP / rlk: the key-switch ring and the
    relinearisation key (rlwe.GadgetCiphertext) for the Relin forms.  scaleInvariant: NewEvaluator's flag (:125-134): Mul / MulRelin dispatch
    to the scale-invariant forms (:460-465, :604-606) and Rescale does nothing (:1417).  fused: the BGV hot paths as one kernel each
    (rh_bgv_tensor, rh_bgv_mul_plain, rh_bgv_axpby); False issues the reference's own sequence of Ring calls -- the same bits.  encoder: a
    bgv.Encoder over the same ringQ and t; with it Add, Sub, Mul, MulRelin, MulThenAdd and MulRelinThenAdd take []uint64 / []int64 operands."""

    def __init__(self, ringQ, ringQMul=None, t=None, ringP=None, rlk=None, scaleInvariant=False, fused=True, encoder=None):
        if t is None:
            raise RingHipError("bgv.Evaluator: the plaintext modulus t is missing")
        if encoder is not None and (encoder.t != int(t) or encoder.ringQ._h.value != ringQ._h.value):
            raise RingHipError("bgv.Evaluator: the encoder was built for another ringQ or plaintext modulus")
        super().__init__(ringQ, ringP, galois_keys={"rlk": rlk} if rlk is not None else None)
        self.encoder = encoder             # bgv.Encoder: with one, slice operands take the reference's slice branches; without, they are refused
        self.ringQMul, self.t = ringQMul, int(t)
        self.ScaleInvariant, self.fused = bool(scaleInvariant), bool(fused)
        self._bfv, self.levelQMul = None, None
        if ringQMul is None:
            if self.t <= 0 or self.t in [int(q) for q in ringQ.moduli]:
                raise RingHipError("bgv.Evaluator: plaintext modulus %d is zero or a modulus of Q" % self.t)
            return
        h = C.c_void_p()
        _check(lib().rh_bfv_create(C.byref(h), ringQ._h, ringQMul._h, self.t))
        self._bfv = h
        self.levelQMul = [lib().rh_bfv_level_qmul(h, i) for i in range(ringQ.L)]          # :51-56

    def close(self):
        if getattr(self, "_bfv", None):
            lib().rh_bfv_destroy(self._bfv)
            self._bfv = None
        super().close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _need_qmul(self, who):
        if self._bfv is None:
            raise RingHipError("cannot %s: the evaluator was built without ringQMul, which scale-invariant tensoring needs" % who)

    def reserve(self, npoly):
        """pre-size the handle's scratch for multiplies of npoly ciphertexts at the top level: no allocation afterwards"""
        self._need_qmul("reserve")
        _check(lib().rh_bfv_reserve(self._bfv, int(npoly)))

    def set_tuning(self, key, value):
        self._need_qmul("set_tuning")
        _check(lib().rh_bfv_set_tuning(self._bfv, key.encode(), int(value)))

    def QuantizePath(self, level):
        """"fused": quantize's two basis extensions and the scalar multiply run as one kernel at this level; "composed": three launches"""
        self._need_qmul("QuantizePath")
        rc = lib().rh_bfv_quantize_path(self._bfv, int(level))
        if rc < 0:
            _check(rc)
        return "fused" if rc else "composed"

    # ---- the two kernels on their own (tensorLowDeg :1062-1102, quantize :1104-1124) ----------------------------------------------
    def TensorLowDeg(self, level, ct0Q, ct1Q, ct2Q, ct0M, ct1M, ct2M):
        """ct0*, ct1*: two-component lists of blocks in Q / QMul (ct1* None: the squaring case); ct2*: three-component output lists.
        c1 is left in [0, 2q) as MulCoeffsMontgomeryThenAddLazy / AddLazy leave it."""
        self._need_qmul("TensorLowDeg")
        sq = ct1Q is None
        b = [None, None] if sq else list(ct1Q)
        bm = [None, None] if sq else list(ct1M)
        self._rows(level, *ct0Q, *ct2Q, *[p for p in b if p is not None])
        self._rows(self.levelQMul[level], *ct0M, *ct2M, *[p for p in bm if p is not None])
        ptr = lambda p: p.ptr if p is not None else None
        _check(lib().rh_bfv_tensor_lazy(self._bfv, level, ct0Q[0].ptr, ct0Q[1].ptr, ptr(b[0]), ptr(b[1]), ct0M[0].ptr, ct0M[1].ptr, ptr(bm[0]), ptr(bm[1]),
                                        ct2Q[0].ptr, ct2Q[1].ptr, ct2Q[2].ptr, ct2M[0].ptr, ct2M[1].ptr, ct2M[2].ptr, ct0Q[0].npoly, 1 if sq else 0))

    def Quantize(self, level, c2Q1, c2Q2, out=None):
        """NTT-domain c (Q) and c (QMul) -> NTT-domain round(c / Q) * T in Q; out defaults to c2Q1 (the reference works in place)"""
        self._need_qmul("Quantize")
        out = c2Q1 if out is None else out
        self._rows(level, c2Q1, out)
        self._rows(self.levelQMul[level], c2Q2)
        _check(lib().rh_bfv_quantize(self._bfv, level, c2Q1.ptr, c2Q2.ptr, out.ptr, c2Q1.npoly))

    # ---- :771-972 -----------------------------------------------------------------------------------------------------------------
    def _operands(self, op0, op1, opOut, relin, who):
        if not isinstance(op1, Ciphertext):
            raise RingHipError("cannot %s: op1 of type %s goes to tensorStandard / Mul (BGV scale matching), which the device path does not build"
                               % (who, type(op1).__name__))
        if op1.Degree() == 0:
            raise RingHipError("cannot %s: a degree-0 operand goes to tensorStandard (BGV scale matching), which the device path does not build" % who)
        if op0.Degree() != 1 or op1.Degree() != 1:
            raise RingHipError("cannot %s: input degrees must be 1, got %d and %d" % (who, op0.Degree(), op1.Degree()))
        if opOut.Degree() != (1 if relin else 2):
            raise RingHipError("cannot %s: opOut must have degree %d" % (who, 1 if relin else 2))
        if not (op0.IsNTT and op1.IsNTT):
            raise RingHipError("cannot %s: operands must be in the NTT domain" % who)
        lv = {op0.Level(), op1.Level(), opOut.Level()}
        if len(lv) != 1:
            raise RingHipError("cannot %s: operands must sit at the same level, got %s" % (who, sorted(lv)))
        return lv.pop()

    def tensorScaleInvariant(self, ct0, ct1, relin, opOut):
        """:975-1040"""
        level = opOut.Level()
        npoly = ct0.Value[0].npoly
        ringQ = self.ringQ.AtLevel(level)
        tmp0, tmp1 = (ct1, ct0) if ct1 is opOut else (ct0, ct1)                 # avoid overwriting if the second input is the output (:982-987)
        c2 = self.buffer("bfv_c2", ringQ, npoly, level + 1) if relin else opOut.Value[2]
        self._rows(level, *tmp0.Value, *tmp1.Value, opOut.Value[0], opOut.Value[1], c2)
        sq = tmp0 is tmp1
        _check(lib().rh_bfv_mul_scale_invariant(self._bfv, level, tmp0.Value[0].ptr, tmp0.Value[1].ptr, None if sq else tmp1.Value[0].ptr,
                                                None if sq else tmp1.Value[1].ptr, opOut.Value[0].ptr, opOut.Value[1].ptr, c2.ptr, npoly))
        if relin:
            rlk = self.galois_keys.get("rlk")
            if rlk is None:
                raise RingHipError("cannot TensorInvariant: relinearization key is missing")
            tmpCt = Ciphertext([self.buffer("bfv_ks0", ringQ, npoly, level + 1), self.buffer("bfv_ks1", ringQ, npoly, level + 1)], is_ntt=True)
            self.GadgetProduct(level, c2, rlk, tmpCt)                            # (:1029)
            ringQ.Add(opOut.Value[0], tmpCt.Value[0], opOut.Value[0])            # (:1033-1034)
            ringQ.Add(opOut.Value[1], tmpCt.Value[1], opOut.Value[1])
        Q = 1
        for q in self.ringQ.moduli[:level + 1]:
            Q *= int(q)
        opOut.Scale = MulScaleInvariant(self.t, Q, getattr(ct0, "Scale", 1), getattr(tmp1, "Scale", 1))   # (:1037)
        opOut.IsNTT = True

    def MulScaleInvariant(self, op0, op1, opOut):
        """:771-830, ciphertext branch: opOut (degree 2) = op0 x op1 * T / Q.  A slice (with encoder=) is encoded at scale 1 and goes to
        tensorStandard (:794-821)"""
        if self.encoder is not None and _is_values(op1):
            return self.tensorStandard(op0, self._slice_pt(op0, op1, 1), False, opOut, "MulInvariant")
        self._need_qmul("MulScaleInvariant")
        self._operands(op0, op1, opOut, False, "MulInvariant")
        self.tensorScaleInvariant(op0, op1, False, opOut)

    def MulRelinScaleInvariant(self, op0, op1, opOut):
        """:877-941, ciphertext branch: the same, relinearised to degree 1.  A slice (with encoder=): as above (:901-930)"""
        if self.encoder is not None and _is_values(op1):
            return self.tensorStandard(op0, self._slice_pt(op0, op1, 1), True, opOut, "MulRelinInvariant")
        self._need_qmul("MulRelinScaleInvariant")
        self._operands(op0, op1, opOut, True, "MulRelinInvariant")
        self.tensorScaleInvariant(op0, op1, True, opOut)

    def _new(self, degree, like):
        level, npoly = like.Level(), like.Value[0].npoly
        ringQ = self.ringQ.AtLevel(level)
        return Ciphertext([ringQ.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)

    def MulScaleInvariantNew(self, op0, op1):
        """:849-857"""
        opOut = self._new(op0.Degree() if self.encoder is not None and _is_values(op1) else 2, op0)
        self.MulScaleInvariant(op0, op1, opOut)
        return opOut

    def MulRelinScaleInvariantNew(self, op0, op1):
        """:960-972"""
        opOut = self._new(op0.Degree() if self.encoder is not None and _is_values(op1) else 1, op0)
        self.MulRelinScaleInvariant(op0, op1, opOut)
        return opOut

    # ---- the BGV half: scales, operand checks ----------------------------------------------------------------------------------------
    @staticmethod
    def _scale(ct):
        return int(getattr(ct, "Scale", 1))

    def _refuse_slice(self, op1, who):
        if _is_slice(op1):
            raise RingHipError("cannot %s: op1 of type %s (a slice, []uint64 / []int64) needs the BGV encoder, which the device path does not build"
                               % (who, type(op1).__name__))
        if not (_is_int(op1) or isinstance(op1, Ciphertext)):
            raise RingHipError("cannot %s: invalid op1 of type %s, expected a Ciphertext or an int" % (who, type(op1).__name__))

    def _slice_pt(self, op0, op1, scale):
        """the plaintext of a slice operand: op0's metadata with the scale the method sets, encoded into the evaluator's buffer
        (:245-259, :519-534, :804-818, :1213-1235)"""
        level, npoly = op0.Level(), op0.Value[0].npoly
        pt = Plaintext(self.buffer("bgv_pt", self.ringQ.AtLevel(level), npoly, level + 1), scale, is_ntt=op0.IsNTT,
                       is_montgomery=getattr(op0, "IsMontgomery", False), is_batched=getattr(op0, "IsBatched", True))
        self.encoder.Encode(op1, pt)
        return pt

    def _same_level(self, who, *cts):
        for ct in cts:
            if not ct.IsNTT:
                raise RingHipError("cannot %s: operands must be in the NTT domain" % who)
        lv = {ct.Level() for ct in cts}
        if len(lv) != 1:
            raise RingHipError("cannot %s: operands must sit at the same level, got %s" % (who, sorted(lv)))
        level = lv.pop()
        for ct in cts:
            self._rows(level, *ct.Value)
        if len({p.npoly for ct in cts for p in ct.Value}) != 1:
            raise RingHipError("cannot %s: every poly block of a call holds the same number of polys" % who)
        return level

    def _qs(self, level):
        return [int(q) for q in self.ringQ.moduli[:level + 1]]

    def _k(self, level, r0=1):
        """T * r0 * 2^128 mod q_i: tMontgomery (:68-70) with the scale-matching factor folded in"""
        return _u64([((self.t * int(r0)) << 128) % q for q in self._qs(level)])

    def _mont(self, level, r):
        """MForm(r) per limb (ring/operations.go:201-205)"""
        return _u64([(int(r) << 64) % q for q in self._qs(level)])

    def _center_t(self, v):
        """v mod T, minus T above T/2 (:494-499)"""
        v = int(v) % self.t
        return v - self.t if v > (self.t >> 1) else v

    def _rlk(self, who):
        rlk = self.galois_keys.get("rlk")
        if rlk is None:
            raise RingHipError("cannot %s: cannot Relinearize: relinearization key is missing" % who)
        return rlk

    def _relin_add(self, level, ringQ, c2, rlk, opOut):
        """:719-733 / :1355-1363: GadgetProduct of c2 into the evaluator's buffers, then the two Adds"""
        npoly = c2.npoly
        tmpCt = Ciphertext([self.buffer("bgv_ks0", ringQ, npoly, level + 1), self.buffer("bgv_ks1", ringQ, npoly, level + 1)], is_ntt=True)
        self.GadgetProduct(level, c2, rlk, tmpCt)
        ringQ.Add(opOut.Value[0], tmpCt.Value[0], opOut.Value[0])
        ringQ.Add(opOut.Value[1], tmpCt.Value[1], opOut.Value[1])

    def _axpby(self, level, a, b, out, r0, r1, sub):
        _check(lib().rh_bgv_axpby(self.ringQ._h, level, a.ptr if a is not None else None, b.ptr if b is not None else None, out.ptr, out.npoly,
                                  _p(self._mont(level, r0)) if a is not None else None, _p(self._mont(level, r1)) if b is not None else None,
                                  1 if sub else 0))

    # ---- Add / Sub :173-432 ------------------------------------------------------------------------------------------------------------
    def _add_sub(self, op0, op1, opOut, sub):
        who = "Sub" if sub else "Add"
        if self.encoder is not None and _is_values(op1):
            op1 = self._slice_pt(op0, op1, self._scale(op0))                         # the plaintext takes op0's metadata, scale included (:254)
        self._refuse_slice(op1, who)
        if _is_int(op1):                                                           # *big.Int (:197-227, :368-369: Sub adds the negation)
            level = self._same_level(who, op0, opOut)
            if opOut.Degree() != op0.Degree():
                raise RingHipError("cannot %s: opOut must have degree %d" % (who, op0.Degree()))
            ringQ = self.ringQ.AtLevel(level)
            v = self._center_t((-int(op1) if sub else int(op1)) * self._scale(op0))   # op1 at op0's scale, centred (:209-216)
            v *= pow(self.t, -1, math.prod(self._qs(level)))                       # T^-1 mod Q_level (:219, bgv/encoder.go:67-71)
            ringQ.AddScalarBigint(op0.Value[0], v, opOut.Value[0])                 # (:221)
            if op0 is not opOut:
                for i in range(1, op0.Degree() + 1):
                    ringQ.CopyLvl(op0.Value[i], opOut.Value[i])                    # (:223-227)
            opOut.Scale, opOut.IsNTT = self._scale(op0), True
            return
        level = self._same_level(who, op0, op1, opOut)
        d0, d1 = op0.Degree(), op1.Degree()
        if opOut.Degree() != max(d0, d1):
            raise RingHipError("cannot %s: opOut must have degree %d" % (who, max(d0, d1)))
        ringQ = self.ringQ.AtLevel(level)
        s0, s1 = self._scale(op0), self._scale(op1)
        if s0 == s1:                                                               # evaluateInPlace (:270-286)
            f = ringQ.Sub if sub else ringQ.Add
            for i in range(min(d0, d1) + 1):
                f(op0.Value[i], op1.Value[i], opOut.Value[i])
            largest = op0 if d0 > d1 else op1 if d1 > d0 else None
            if largest is not None and largest is not opOut:
                for i in range(min(d0, d1) + 1, max(d0, d1) + 1):                  # copied, under Sub too (:281-285)
                    ringQ.CopyLvl(largest.Value[i], opOut.Value[i])
            opOut.Scale, opOut.IsNTT = max(s0, s1), True
            return
        # matchScaleThenEvaluateInPlace (:288-305)
        if op1 is opOut:
            raise RingHipError("cannot %s: opOut is op1 and the scales differ: the reference's sequence overwrites op1 before it reads it" % who)
        r0, r1, _ = matchScalesBinary(self.t, s0, s1)
        if self.fused:
            for i in range(opOut.Degree() + 1):                                    # r0 a +- r1 b, r0 a alone, +- r1 b into a zeroed component
                self._axpby(level, op0.Value[i] if i <= d0 else None, op1.Value[i] if i <= d1 else None, opOut.Value[i], r0, r1, sub)
        else:
            for i in range(d0 + 1):
                ringQ.MulScalar(op0.Value[i], r0, opOut.Value[i])                  # (:292-294)
            for i in range(d0 + 1, opOut.Degree() + 1):
                ringQ.vec_op("ZERO", None, None, opOut.Value[i])                   # (:296-298)
            f = ringQ.MulScalarThenSub if sub else ringQ.MulScalarThenAdd
            for i in range(d1 + 1):
                f(op1.Value[i], r1, opOut.Value[i])                                # (:300-302)
        opOut.Scale, opOut.IsNTT = s0 * r0 % self.t, True                          # (:304)

    def Add(self, op0, op1, opOut):
        """:173-268: op1 a Ciphertext (any degrees up to 2; scales that differ are matched first, :194) or an int"""
        self._add_sub(op0, op1, opOut, False)

    def Sub(self, op0, op1, opOut):
        """:348-409"""
        self._add_sub(op0, op1, opOut, True)

    def _new_binary(self, op0, op1, degree=None):
        if degree is None:
            degree = max(op0.Degree(), op1.Degree()) if isinstance(op1, Ciphertext) else op0.Degree()
        return self._new(degree, op0)

    def AddNew(self, op0, op1):
        """:323-333"""
        opOut = self._new_binary(op0, op1)
        self.Add(op0, op1, opOut)
        return opOut

    def SubNew(self, op0, op1):
        """:423-432"""
        opOut = self._new_binary(op0, op1)
        self.Sub(op0, op1, opOut)
        return opOut

    # ---- Mul / MulRelin :458-663, tensorStandard :665-751 -----------------------------------------------------------------------------
    def _tensor_degrees(self, op0, op1, who):
        d0, d1 = op0.Degree(), op1.Degree()
        if d0 > 2 or d1 > 1 or (d1 == 1 and d0 != 1):
            raise RingHipError("cannot %s: degrees %d and %d: the device path builds degree 1 x degree 1 and degree <= 2 x degree 0 (a plaintext)"
                               % (who, d0, d1))
        return d0, d1

    def tensorStandard(self, op0, op1, relin, opOut, who="Mul"):
        """:665-751"""
        level = self._same_level(who, op0, op1, opOut)
        d0, d1 = self._tensor_degrees(op0, op1, who)
        scale = self._scale(op0) * self._scale(op1) % self.t                       # (:669)
        ringQ = self.ringQ.AtLevel(level)
        npoly = op0.Value[0].npoly
        tMontgomery = self._k(level)
        if d0 == 1 and d1 == 1:
            if opOut.Degree() != (1 if relin else 2):
                raise RingHipError("cannot %s: opOut must have degree %d" % (who, 1 if relin else 2))
            rlk = self._rlk(who) if relin else None
            c0, c1 = opOut.Value[0], opOut.Value[1]
            c2 = self.buffer("bgv_c2", ringQ, npoly, level + 1) if relin else opOut.Value[2]
            tmp0, tmp1 = (op1, op0) if op1 is opOut else (op0, op1)                # avoid overwriting if the second input is the output (:693-698)
            sq = op0 is op1
            if self.fused:
                _check(lib().rh_bgv_tensor(self.ringQ._h, level, tmp0.Value[0].ptr, tmp0.Value[1].ptr, None if sq else tmp1.Value[0].ptr,
                                           None if sq else tmp1.Value[1].ptr, c0.ptr, c1.ptr, c2.ptr, npoly, _p(tMontgomery), None, 0))
            else:
                c00, c01 = self.buffer("bgv_c00", ringQ, npoly, level + 1), self.buffer("bgv_c01", ringQ, npoly, level + 1)
                ringQ.MulRNSScalarMontgomery(tmp0.Value[0], tMontgomery, c00)      # (:701-702)
                ringQ.MulRNSScalarMontgomery(tmp0.Value[1], tMontgomery, c01)
                ringQ.MulCoeffsMontgomery(c00, tmp1.Value[0], c0)                  # (:705 / :711)
                ringQ.MulCoeffsMontgomery(c01, tmp1.Value[1], c2)                  # (:706 / :712)
                ringQ.MulCoeffsMontgomery(c00, tmp1.Value[1], c1)                  # (:707 / :713)
                if sq:
                    ringQ.Add(c1, c1, c1)                                          # (:708)
                else:
                    ringQ.MulCoeffsMontgomeryThenAdd(c01, tmp1.Value[0], c1)       # (:714)
            if relin:
                self._relin_add(level, ringQ, c2, rlk, opOut)                      # (:717-734)
        else:                                                                      # plaintext x ciphertext (:737-748)
            if opOut.Degree() != d0:
                raise RingHipError("cannot %s: opOut must have degree %d" % (who, d0))
            if self.fused:
                ins = [v.ptr for v in op0.Value] + [None] * (2 - d0)
                outs = [v.ptr for v in opOut.Value] + [None] * (2 - d0)
                _check(lib().rh_bgv_mul_plain(self.ringQ._h, level, *ins, op1.Value[0].ptr, *outs, npoly, _p(tMontgomery), None, 0))
            else:
                c00 = self.buffer("bgv_c00", ringQ, npoly, level + 1)
                ringQ.MulRNSScalarMontgomery(op1.Value[0], tMontgomery, c00)       # (:744)
                for i in range(d0 + 1):
                    ringQ.MulCoeffsMontgomery(op0.Value[i], c00, opOut.Value[i])   # (:745-747)
        opOut.Scale, opOut.IsNTT = scale, True

    def _mul_scalar(self, op0, op1, opOut, who):
        """the *big.Int branch (:481-503)"""
        level = self._same_level(who, op0, opOut)
        if opOut.Degree() != op0.Degree():
            raise RingHipError("cannot %s: opOut must have degree %d" % (who, op0.Degree()))
        ringQ = self.ringQ.AtLevel(level)
        v = self._center_t(op1)
        for i in range(op0.Degree() + 1):
            ringQ.MulScalarBigint(op0.Value[i], v, opOut.Value[i])
        opOut.Scale, opOut.IsNTT = self._scale(op0), True

    def Mul(self, op0, op1, opOut):
        """:458-544: opOut (degree op0.Degree() + op1.Degree()) = op0 x op1 * T, scale op0.Scale * op1.Scale; op1 an int: every component
        times the scalar centred modulo T.  A scale-invariant evaluator sends ciphertexts and slices to MulScaleInvariant (:460-465)."""
        if self.encoder is not None and _is_values(op1):                           # (:511-538; the scale-invariant form comes here too, :794-821)
            return self.tensorStandard(op0, self._slice_pt(op0, op1, 1), False, opOut, "Mul")
        if self.ScaleInvariant and (isinstance(op1, Ciphertext) or _is_slice(op1)):
            return self.MulScaleInvariant(op0, op1, opOut)
        self._refuse_slice(op1, "Mul")
        if _is_int(op1):
            return self._mul_scalar(op0, op1, opOut, "Mul")
        self.tensorStandard(op0, op1, False, opOut, "Mul")

    def MulRelin(self, op0, op1, opOut):
        """:602-629: the same, relinearised to degree 1"""
        if self.encoder is not None and _is_values(op1):                           # (:901-930)
            return self.tensorStandard(op0, self._slice_pt(op0, op1, 1), True, opOut, "MulRelin")
        if self.ScaleInvariant:
            return self.MulRelinScaleInvariant(op0, op1, opOut)
        self._refuse_slice(op1, "MulRelin")
        if _is_int(op1):
            return self._mul_scalar(op0, op1, opOut, "MulRelin")
        self.tensorStandard(op0, op1, True, opOut, "MulRelin")

    def MulNew(self, op0, op1):
        """:564-581"""
        if self.encoder is not None and _is_values(op1):
            opOut = self._new(op0.Degree(), op0)
            self.Mul(op0, op1, opOut)
            return opOut
        if self.ScaleInvariant and (isinstance(op1, Ciphertext) or _is_slice(op1)):
            return self.MulScaleInvariantNew(op0, op1)
        self._refuse_slice(op1, "Mul")
        opOut = self._new_binary(op0, op1, op0.Degree() + op1.Degree() if isinstance(op1, Ciphertext) else None)
        self.Mul(op0, op1, opOut)
        return opOut

    def MulRelinNew(self, op0, op1):
        """:649-663"""
        if self.encoder is not None and _is_values(op1):
            opOut = self._new(op0.Degree(), op0)
            self.MulRelin(op0, op1, opOut)
            return opOut
        if self.ScaleInvariant:
            return self.MulRelinScaleInvariantNew(op0, op1)
        self._refuse_slice(op1, "MulRelin")
        opOut = self._new_binary(op0, op1, max(1, op0.Degree()) if isinstance(op1, Ciphertext) else None)
        self.MulRelin(op0, op1, opOut)
        return opOut

    # ---- MulThenAdd / MulRelinThenAdd :1142-1287, mulRelinThenAdd :1289-1403 -----------------------------------------------------------
    def mulRelinThenAdd(self, op0, op1, relin, opOut, who="MulThenAdd"):
        """:1289-1403"""
        level = self._same_level(who, op0, op1, opOut)
        d0, d1 = self._tensor_degrees(op0, op1, who)
        if op0 is opOut or op1 is opOut:
            raise RingHipError("cannot %s: opOut must be different from op0 and op1" % who)      # (:1152-1154)
        ringQ = self.ringQ.AtLevel(level)
        npoly = op0.Value[0].npoly
        ct = d0 == 1 and d1 == 1
        if ct and (opOut.Degree() != 2 if not relin else opOut.Degree() not in (1, 2)):
            raise RingHipError("cannot %s: opOut must have degree %s" % (who, "1 or 2" if relin else "2"))
        if not ct and not d0 <= opOut.Degree() <= 2:
            raise RingHipError("cannot %s: opOut must have a degree from %d to 2" % (who, d0))
        rlk = self._rlk(who) if ct and relin else None
        # if op0.Scale * op1.Scale != opOut.Scale, both sides are brought to a common scale (:1317-1329, :1379-1391)
        r0, r1 = 1, None
        targetScale = self._scale(op0) * self._scale(op1) % self.t
        if self._scale(opOut) != targetScale:
            r0, r1, _ = matchScalesBinary(self.t, targetScale, self._scale(opOut))
        # components of opOut the fused kernel does not visit; call by call, every component (:1324-1326, :1386-1388)
        nacc = (2 if relin else 3) if ct else d0 + 1
        if r1 is not None:
            for i in range(nacc if self.fused else 0, opOut.Degree() + 1):
                ringQ.MulScalar(opOut.Value[i], r1, opOut.Value[i])
            opOut.Scale = self._scale(opOut) * r1 % self.t                         # (:1328, :1390)
        tMontgomery = self._k(level)
        if ct:
            c0, c1 = opOut.Value[0], opOut.Value[1]
            c2 = self.buffer("bgv_c2", ringQ, npoly, level + 1) if relin else opOut.Value[2]
            if self.fused:
                sq = op0 is op1
                _check(lib().rh_bgv_tensor(self.ringQ._h, level, op0.Value[0].ptr, op0.Value[1].ptr, None if sq else op1.Value[0].ptr,
                                           None if sq else op1.Value[1].ptr, c0.ptr, c1.ptr, c2.ptr, npoly, _p(self._k(level, r0)),
                                           _p(self._mont(level, r1)) if r1 not in (None, 1) else None, 2 if relin else 1))
            else:
                c00, c01 = self.buffer("bgv_c00", ringQ, npoly, level + 1), self.buffer("bgv_c01", ringQ, npoly, level + 1)
                ringQ.MulRNSScalarMontgomery(op0.Value[0], tMontgomery, c00)       # (:1332-1333)
                ringQ.MulRNSScalarMontgomery(op0.Value[1], tMontgomery, c01)
                if r0 != 1:
                    ringQ.MulScalar(c00, r0, c00)                                  # (:1336-1339)
                    ringQ.MulScalar(c01, r0, c01)
                ringQ.MulCoeffsMontgomeryThenAdd(c00, op1.Value[0], c0)            # (:1341-1343)
                ringQ.MulCoeffsMontgomeryThenAdd(c00, op1.Value[1], c1)
                ringQ.MulCoeffsMontgomeryThenAdd(c01, op1.Value[0], c1)
                if relin:
                    ringQ.MulCoeffsMontgomery(c01, op1.Value[1], c2)               # (:1353)
                else:
                    ringQ.MulCoeffsMontgomeryThenAdd(c01, op1.Value[1], c2)        # (:1366)
            if relin:
                self._relin_add(level, ringQ, c2, rlk, opOut)                      # (:1355-1363)
        else:                                                                      # plaintext x ciphertext (:1370-1400)
            if self.fused:
                ins = [v.ptr for v in op0.Value] + [None] * (2 - d0)
                outs = [v.ptr for v in opOut.Value[:d0 + 1]] + [None] * (2 - d0)
                _check(lib().rh_bgv_mul_plain(self.ringQ._h, level, *ins, op1.Value[0].ptr, *outs, npoly, _p(self._k(level, r0)),
                                              _p(self._mont(level, r1)) if r1 not in (None, 1) else None, 1))
            else:
                c00 = self.buffer("bgv_c00", ringQ, npoly, level + 1)
                ringQ.MulRNSScalarMontgomery(op1.Value[0], tMontgomery, c00)       # (:1377)
                if r0 != 1:
                    ringQ.MulScalar(c00, r0, c00)                                  # (:1393-1395)
                for i in range(d0 + 1):
                    ringQ.MulCoeffsMontgomeryThenAdd(op0.Value[i], c00, opOut.Value[i])   # (:1397-1399)
        opOut.Scale, opOut.IsNTT = self._scale(opOut), True

    def MulThenAdd(self, op0, op1, opOut):
        """:1142-1246: opOut += op0 x op1 * T without relinearisation (opOut of degree 2 for two degree-1 operands); an opOut whose scale is
        not op0.Scale * op1.Scale has both sides matched first.  op1 an int: opOut += op0 * (op1 * opOut.Scale / op0.Scale)."""
        if self.encoder is not None and _is_values(op1):                           # (:1202-1239): encoded at opOut.Scale / op0.Scale, or 1
            s0, so = self._scale(op0), self._scale(opOut)
            op1 = self._slice_pt(op0, op1, pow(s0, self.t - 2, self.t) * so % self.t if s0 != so else 1)
        self._refuse_slice(op1, "MulThenAdd")
        if _is_int(op1):                                                           # (:1162-1194)
            level = self._same_level("MulThenAdd", op0, opOut)
            if opOut.Degree() < op0.Degree():
                raise RingHipError("cannot MulThenAdd: opOut must have at least degree %d" % op0.Degree())
            ringQ = self.ringQ.AtLevel(level)
            v = int(op1)
            if self._scale(op0) != self._scale(opOut):                             # op1 *= opOut.Scale / op0.Scale (:1177-1181)
                v *= pow(self._scale(op0), self.t - 2, self.t) * self._scale(opOut) % self.t
            v = self._center_t(v)
            for i in range(op0.Degree() + 1):
                ringQ.MulScalarBigintThenAdd(op0.Value[i], v, opOut.Value[i])      # (:1192-1194)
            opOut.Scale = self._scale(opOut)
            return
        self.mulRelinThenAdd(op0, op1, False, opOut, "MulThenAdd")

    def MulRelinThenAdd(self, op0, op1, opOut):
        """:1264-1287: the same with the degree-2 term relinearised before it is added (opOut of degree 1)"""
        if isinstance(op1, Ciphertext) and op1.Degree() != 0:
            return self.mulRelinThenAdd(op0, op1, True, opOut, "MulRelinThenAdd")
        self.MulThenAdd(op0, op1, opOut)

    # ---- Rescale :1415-1445, MatchScalesAndLevel :1593-1614 -----------------------------------------------------------------------------
    def Rescale(self, op0, opOut):
        """:1415-1445: DivRoundByLastModulusNTT on every component; the scale is divided by the consumed prime modulo T.  opOut's polys are
        allocated at op0's level or one below; limbs 0 .. level-1 hold the result.  Nothing happens on a scale-invariant evaluator (:1417)."""
        if self.ScaleInvariant:
            return
        level = op0.Level()
        if level == 0:
            raise RingHipError("cannot rescale: op0 already at level 0")
        if opOut.Level() < level - 1:
            raise RingHipError("cannot rescale: opOut.Level() < op0.Level()-1")
        if opOut.Degree() != op0.Degree() or not op0.IsNTT:
            raise RingHipError("cannot rescale: opOut must have op0's degree and op0 must be in the NTT domain")
        self._rows(level, *op0.Value)
        for p in opOut.Value:
            if p.limbs not in (level, level + 1) or p.npoly != op0.Value[0].npoly:
                raise RingHipError("cannot rescale: opOut must be allocated at level %d or %d, with op0's number of polys" % (level - 1, level))
        ringQ = self.ringQ.AtLevel(level)
        for a, b in zip(op0.Value, opOut.Value):
            ringQ.DivRoundByLastModulusNTT(a, b)                                   # (:1436-1438)
        qL = int(self.ringQ.moduli[level])
        opOut.Scale, opOut.IsNTT = self._scale(op0) * pow(qL % self.t, -1, self.t) % self.t, True      # (:1443)

    def RescaleNew(self, op0):
        """opOut allocated one level down"""
        if self.ScaleInvariant:
            return op0
        if op0.Level() == 0:
            raise RingHipError("cannot rescale: op0 already at level 0")
        ringQ = self.ringQ.AtLevel(op0.Level() - 1)
        opOut = Ciphertext([ringQ.NewPoly(op0.Value[0].npoly) for _ in op0.Value], is_ntt=True)
        self.Rescale(op0, opOut)
        return opOut

    def MatchScalesAndLevel(self, ct0, opOut):
        """:1593-1614: both ciphertexts multiplied in place by the factors of matchScalesBinary, so that their scales agree"""
        level = self._same_level("MatchScalesAndLevel", ct0, opOut)
        r0, r1, _ = matchScalesBinary(self.t, self._scale(ct0), self._scale(opOut))
        ringQ = self.ringQ.AtLevel(level)
        for ct, r in ((ct0, r0), (opOut, r1)):
            for el in ct.Value:
                if self.fused:
                    self._axpby(level, el, None, el, r, None, False)
                else:
                    ringQ.MulScalar(el, r, el)                                     # (:1601-1603, :1608-1610)
            ct.Scale = self._scale(ct) * r % self.t                                # (:1606, :1613)

    # ---- rotations :1465-1506, InnerSum / RotateAndAdd :1527-1586 (Replicate and Trace: rlwe.Evaluator's) -------------------------------
    def GaloisElement(self, k):
        """Parameters.GaloisElement: 5^k mod 2N"""
        return rlwe.GaloisElement(self.ringQ.N, k)

    def GaloisElementForRowRotation(self):
        """GaloisElementOrderTwoOrthogonalSubgroup (core/rlwe/params.go:683-689): 2N - 1"""
        return 2 * self.ringQ.N - 1

    def _rotate(self, op0, galEl, opOut):
        self.Automorphism(op0, galEl, opOut)
        self._copy_metadata(op0, opOut)

    def RotateColumns(self, op0, k, opOut):
        """:1473-1475: both rows of the 2 x N/2 plaintext matrix rotated by k columns to the left"""
        self._rotate(op0, self.GaloisElement(k), opOut)

    def RotateColumnsNew(self, op0, k):
        opOut = self._new(op0.Degree(), op0)
        self.RotateColumns(op0, k, opOut)
        return opOut

    def RotateRows(self, op0, opOut):
        """:1488-1490: the two rows swapped"""
        self._rotate(op0, self.GaloisElementForRowRotation(), opOut)

    def RotateRowsNew(self, op0):
        opOut = self._new(op0.Degree(), op0)
        self.RotateRows(op0, opOut)
        return opOut

    def RotateHoistedLazyNew(self, level, rotations, op0, c2DecompQP):
        """:1494-1506: a dict rotation -> rlwe.ElementQP (modulo QP, not yet divided by P) for every rotation other than 0"""
        if self.ringP is None:
            raise RingHipError("cannot RotateHoistedLazyNew: the evaluator was built without ringP, which the key switch needs")
        opOut = {}
        for i in rotations:
            if i != 0:
                opOut[i] = rlwe.ElementQP.alloc(self.ringQ, self.ringP, op0.Value[0].npoly, level, self.ringP.L - 1)
                self.AutomorphismHoistedLazy(level, op0, c2DecompQP, self.GaloisElement(i), opOut[i])
        return opOut

    def InnerSum(self, ctIn, batchSize, n, opOut, fused=None):
        """:1527-1566: the sub-vectors of batchSize slots of each row added together in groups of n.  n batchSize = N sums over BOTH rows:
        PartialTracesSum with n / 2, RotateRows, Add (:1541-1562).  fused: as rlwe.Evaluator.PartialTracesSum."""
        N, l = self.ringQ.N, int(n) * int(batchSize)                                  # ctIn.Slots(): a 2 x N/2 matrix
        if n <= 0 or batchSize <= 0:
            raise RingHipError("innersum: invalid parameter (n <= 0 or batchSize <= 0)")
        if l > N:
            raise RingHipError("innersum: invalid parameters (n*batchSize=%d > #slots=%d)" % (l, N))
        if l & (l - 1) != 0:
            raise RingHipError("innersum: invalid parameters (n*batchSize=%d does not divide #slots=%d)" % (l, N))
        if l != N:
            return self.PartialTracesSum(ctIn, batchSize, n, opOut, fused=fused)
        if n == 1:
            if opOut is not ctIn:
                ringQ = self.ringQ.AtLevel(self._sum_operands(ctIn, opOut, "InnerSum"))
                for a, b in zip(ctIn.Value, opOut.Value):
                    ringQ.CopyLvl(a, b)
                self._copy_metadata(ctIn, opOut)
            return
        g = self.GaloisElementForRowRotation()
        self._sum_keys([g], "InnerSum")                                               # before the first launch, like the keys of the partial sum
        self.PartialTracesSum(ctIn, batchSize, n // 2, opOut, fused=fused)
        level, npoly = opOut.Level(), opOut.Value[0].npoly
        ringQ = self.ringQ.AtLevel(level)
        ctTmp = Ciphertext([self.buffer("rowsQ%d" % c, ringQ, npoly, level + 1) for c in (0, 1)], is_ntt=True)
        self.RotateRows(opOut, ctTmp)
        self.Add(opOut, ctTmp, opOut)

    def RotateAndAdd(self, ctIn, batchSize, n, opOut, fused=None):
        """:1583-1586"""
        self.PartialTracesSum(ctIn, batchSize, n, opOut, fused=fused)


# ---- bgv.Encoder, schemes/bgv/encoder.go, on standard rings -------------------------------------------------------------------------------
def PlaintextRingDegree(N, t):
    """bgv/params.go:110-121: min(N, order / 2) with order the largest power of two such that t = 1 modulo it"""
    t = int(t)
    order = 1 << t.bit_length()
    while order and t & (order - 1) != 1:
        order >>= 1
    if order < 16:
        raise RingHipError("provided plaintext modulus t has cyclotomic order < 16 (ring degree of minimum 8 is required by the backend)")
    return min(int(N), order >> 1)


def permuteMatrix(logN):
    """encoder.go:98-121: slot i of the first row sits at bitrev((5^i mod 2N) >> 1), slot i of the second row mirrors it"""
    N = 1 << logN
    perm = np.zeros(N, dtype=np.uint64)
    pow5, mask = 1, 2 * N - 1
    for i in range(N >> 1):
        pos = int(format(pow5 >> 1, "0%db" % logN)[::-1], 2)
        perm[i], perm[i + (N >> 1)] = pos, N - pos - 1
        pow5 = pow5 * 5 & mask
    return perm


class DeviceValues:
    """(nvec, n) uint64 -- or int64 with signed=True -- on the device: the []uint64 / []int64 of a batch of vectors"""

    def __init__(self, ring, nvec, n, signed=False):
        self.ring, self.nvec, self.n, self.signed = ring, int(nvec), int(n), bool(signed)
        self.words = self.nvec * self.n
        p = C.c_void_p()
        _check(lib().rh_dev_alloc(ring._h, max(self.words, 1), C.byref(p)))
        self.ptr = int(p.value)

    @classmethod
    def from_numpy(cls, ring, arr):
        arr = np.asarray(arr)
        if arr.dtype not in (np.uint64, np.int64):
            raise RingHipError("bgv.DeviceValues: values must be uint64 or int64, but are %s" % arr.dtype)
        arr = np.ascontiguousarray(arr[None] if arr.ndim == 1 else arr)
        assert arr.ndim == 2, arr.shape
        v = cls(ring, arr.shape[0], arr.shape[1], arr.dtype == np.int64)
        v.upload(arr)
        return v

    def upload(self, arr):
        if self.words:
            _check(lib().rh_dev_upload(self.ring._h, self.ptr, _p(np.ascontiguousarray(arr).view(np.uint64).reshape(-1)), self.words))

    def numpy(self):
        out = np.empty(self.words, dtype=np.uint64)
        if self.words:
            _check(lib().rh_dev_download(self.ring._h, _p(out), self.ptr, self.words))
        return out.view(np.int64 if self.signed else np.uint64).reshape(self.nvec, self.n)

    def free(self):
        if self.ptr:
            lib().rh_dev_free(None, self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Plaintext(Ciphertext):
    """rlwe.Plaintext: one poly block (npoly vectors) with the MetaData the BGV encoder reads -- Scale (an int modulo T), IsNTT, IsBatched,
    IsMontgomery.  A degree-0 Ciphertext to the evaluator."""

    def __init__(self, poly, scale=1, is_ntt=True, is_montgomery=False, is_batched=True):
        Ciphertext.__init__(self, [poly], is_ntt=is_ntt)
        self.Scale = int(scale)
        self.IsMontgomery, self.IsBatched = bool(is_montgomery), bool(is_batched)


class Encoder:
    """bgv.Encoder on device batches: Encode / Decode / EncodeRingT / DecodeRingT / Embed / EmbedScale / RingT2Q / RingQ2T of nvec vectors at
    once (csrc/bgv_encoder.hip).  ringT is built here by the rule of bgv/params.go:110-121.  Refused by name: conjugate-invariant and 3N
    rings, more values than slots, value types other than uint64 / int64, a scale that is zero or not invertible modulo T in Decode, and
    EmbedScale(scaleUp=True) into a (Q, P) pair: the reference multiplies the limbs of P by T^-1 mod Q_levelP under the moduli of Q there
    (:282, :384), which is a finding about the reference, not a behaviour to reproduce."""

    def __init__(self, ringQ, t, ringP=None):
        self.ringQ, self.ringP, self.t = ringQ, ringP, int(t)
        self._h, self.ringT = None, None
        for r in (ringQ, ringP):
            if r is not None and r.kind == ConjugateInvariant:
                raise RingHipError("cannot NewEncoder: conjugate-invariant rings are not supported (their one-row encoder stays with the reference)")
            if r is not None and r.kind != Standard:
                raise RingHipError("cannot NewEncoder: 3N rings are not supported (the BGV encoder is defined on power-of-two cyclotomics)")
        if self.t <= 0:
            raise RingHipError("invalid parameters: t = 0")
        n = PlaintextRingDegree(ringQ.N, self.t)
        try:
            self.ringT = Ring(n, [self.t], device=ringQ.device)
        except RingHipError as e:
            raise RingHipError("provided plaintext modulus t is invalid: %s" % e) from None
        h = C.c_void_p()
        _check(lib().rh_bgv_encoder_create(C.byref(h), ringQ._h, self.ringT._h))
        self._h = h
        self.indexMatrix = permuteMatrix(n.bit_length() - 1)
        self._tls = threading.local()      # per host thread: the blocks host values go through, kept so that no call frees device memory

    def close(self):
        if self._h:
            lib().rh_bgv_encoder_destroy(self._h)
            self._h = None
        if self.ringT is not None:
            self.ringT.close()
            self.ringT = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def RingT(self):
        return self.ringT

    def MaxSlots(self):
        """params.go:189-192: Rows * Cols = 2 * (n / 2)"""
        return self.ringT.N

    def LogMaxDimensions(self):
        """params.go:176-185 on a standard ring: (Rows, Cols) = (1, log2(n) - 1) -- two rows of n / 2 slots"""
        return (1, self.ringT.N.bit_length() - 2)

    def reserve(self, nvec):
        _check(lib().rh_bgv_encoder_reserve(self._h, int(nvec)))

    def set_tuning(self, key, value):
        _check(lib().rh_bgv_encoder_set_tuning(self._h, key.encode(), int(value)))

    def NewPlaintext(self, level, scale=1, nvec=1, is_ntt=True, is_batched=True):
        return Plaintext(self.ringQ.AtLevel(level).NewPoly(nvec), scale, is_ntt, False, is_batched)

    # ---- values on their way to and from the device --------------------------------------------------------------------------------------
    def _pooled(self, nvec, n, signed):
        pool = self._tls.__dict__.setdefault("blocks", {})
        dv = pool.get((nvec, n, signed))
        if dv is None:
            dv = pool[(nvec, n, signed)] = DeviceValues(self.ringQ, nvec, n, signed)
        return dv

    def _block(self, values, nvec, text):
        """(nvec, nvals) block on the device from a slice (one vector, shared by the batch), a (nvec, nvals) array or a DeviceValues; text: the
        reference's refusal of too many values, with %d for their number"""
        slots = self.ringT.N
        if isinstance(values, DeviceValues):
            if values.nvec != nvec:
                raise RingHipError("a device block of %d vectors given for a block of %d polys" % (values.nvec, nvec))
            if values.n > slots:
                raise RingHipError(text % values.n)
            return values
        a = np.asarray(values)
        if a.dtype not in (np.uint64, np.int64) and not (isinstance(values, (list, tuple)) and a.size == 0):
            raise RingHipError("cannot EncodeRingT: values.(type) must be either []uint64 or []int64 but is %s"
                               % (a.dtype if isinstance(values, np.ndarray) else "%s of %s" % (type(values).__name__, a.dtype)))
        if a.size == 0:
            a = np.zeros((0,), dtype=np.uint64)
        if a.ndim == 1:
            a = np.broadcast_to(a, (nvec, a.shape[0]))
        if a.ndim != 2 or a.shape[0] != nvec:
            raise RingHipError("%d vectors given for a block of %d polys" % (a.shape[0] if a.ndim == 2 else -1, nvec))
        if a.shape[1] > slots:
            raise RingHipError(text % a.shape[1])
        dv = self._pooled(nvec, a.shape[1], a.dtype == np.int64)
        dv.upload(a)
        return dv

    def _out(self, values, nvec, who):
        """where decoded values go: (device block, host array or None, signed)"""
        if isinstance(values, DeviceValues):
            if values.nvec != nvec or values.n > self.ringT.N:
                raise RingHipError("cannot %s: a device block of values must be (%d, k) with k <= %d" % (who, nvec, self.ringT.N))
            return values, None, values.signed
        if not isinstance(values, np.ndarray) or values.dtype not in (np.uint64, np.int64):
            raise RingHipError("cannot %s: values must be either []uint64 or []int64 but is %s"
                               % (who, values.dtype if isinstance(values, np.ndarray) else type(values).__name__))
        if not (values.ndim == 2 and values.shape[0] == nvec) and not (values.ndim == 1 and nvec == 1):
            raise RingHipError("cannot %s: values of shape %s for a block of %d vectors: give (%d, k)" % (who, values.shape, nvec, nvec))
        if values.shape[-1] > self.ringT.N:
            raise RingHipError("cannot %s: len(values)=%d > slots=%d" % (who, values.shape[-1], self.ringT.N))
        signed = values.dtype == np.int64
        return self._pooled(nvec, values.shape[-1], signed), values, signed

    @staticmethod
    def _back(dv, host):
        if host is None:
            return dv
        np.copyto(host, dv.numpy().reshape(host.shape))        # through the caller's own array, whatever its strides
        return host

    def _ring_of(self, poly, who):
        for r in (self.ringQ, self.ringP):
            if r is not None and poly.ring._h.value == r._h.value:
                return r
        raise RingHipError("cannot %s: the poly belongs to neither ringQ nor ringP of this encoder" % who)

    # ---- Encode / Embed (:130-320) --------------------------------------------------------------------------------------------------------
    def _encode(self, values, scale, batched, scaleUp, is_ntt, mont, poly, text, who):
        ring = self._ring_of(poly, who)
        dv = self._block(values, poly.npoly, text)
        _check(lib().rh_bgv_encode(self._h, ring._h, poly.limbs - 1, int(scale) % (1 << 64), dv.ptr, dv.n, 1 if dv.signed else 0, poly.npoly,
                                   poly.ptr, 1 if batched else 0, 1 if scaleUp else 0, 1 if is_ntt else 0, 1 if mont else 0))

    def Encode(self, values, pt):
        """:130-184: batched through EmbedScale(scaleUp=True); IsBatched = false puts the values on coefficients 0 .. len-1 of the plaintext ring"""
        if pt.IsBatched:
            return self.EmbedScale(values, True, pt, pt.Value[0])
        self._encode(values, pt.Scale, False, True, pt.IsNTT, False, pt.Value[0],
                     "cannot Encode (TimeDomain): len(values)=%%d > N=%d" % self.ringT.N, "Encode")

    def EmbedScale(self, values, scaleUp, metadata, polyOut):
        """:252-316: metadata is anything with Scale, IsNTT and IsMontgomery (a Plaintext, a Ciphertext given them); polyOut a DevicePoly of
        ringQ (or of ringP), or a (Q, P) pair -- a tuple or an rlwe.PolyQP -- whose P may be None"""
        pair = isinstance(polyOut, (tuple, list, rlwe.PolyQP))
        Q, P = ((polyOut.Q, polyOut.P) if isinstance(polyOut, rlwe.PolyQP) else tuple(polyOut)) if pair else (polyOut, None)
        if not isinstance(Q, DevicePoly) or not (P is None or isinstance(P, DevicePoly)):
            raise RingHipError("cannot embed: invalid polyOut.(Type) must be ringqp.Poly or *ring.Poly")
        if pair and scaleUp:
            raise RingHipError("cannot EmbedScale: scaleUp into a ringqp.Poly is refused: the reference multiplies the limbs of P by T^-1 mod Q_levelP "
                               "under the moduli of Q (bgv/encoder.go:282, :384)")
        text = "cannot EncodeRingT (FrequencyDomain): len(values)=%%d > slots=%d" % self.ringT.N
        scale, ntt, mont = getattr(metadata, "Scale", 1), metadata.IsNTT, getattr(metadata, "IsMontgomery", False)
        self._encode(values, scale, True, scaleUp, ntt, mont, Q, text, "Embed")
        if P is not None:
            if self.ringP is None:
                raise RingHipError("cannot embed into a ringqp.Poly: the encoder was built without ringP")
            self._encode(values, scale, True, False, ntt, mont, P, text, "Embed")

    def Embed(self, values, metadata, polyOut):
        """:318-320"""
        return self.EmbedScale(values, False, metadata, polyOut)

    def EmbedRows(self, values, rots, cols, metadata, polyQP):
        """A whole linear transformation in one pass (rh_bgv_embed_qp): vector k of `values` -- a (nvec, 2 * cols) array or DeviceValues -- is
        rotated to the left by rots[k] on each of its two rows (rotateAndEncodeDiagonal, circuits/common/lintrans/lintrans.go:271-292) and
        embedded into poly k of the (Q, P) pair, the words Embed writes for the rotated vector.  rots None: no rotation, any length up to
        the slot count."""
        if not isinstance(polyQP, (tuple, list, rlwe.PolyQP)):
            raise RingHipError("cannot embed: invalid polyOut.(Type) must be ringqp.Poly")
        Q, P = (polyQP.Q, polyQP.P) if isinstance(polyQP, rlwe.PolyQP) else tuple(polyQP)
        if not isinstance(Q, DevicePoly) or not isinstance(P, DevicePoly):
            raise RingHipError("cannot embed: invalid polyOut.(Type) must be ringqp.Poly")
        if self.ringP is None:
            raise RingHipError("cannot embed into a ringqp.Poly: the encoder was built without ringP")
        if self._ring_of(Q, "EmbedRows") is not self.ringQ or self._ring_of(P, "EmbedRows") is not self.ringP or P.npoly != Q.npoly:
            raise RingHipError("cannot EmbedRows: polyQP must pair a block of ringQ with a block of ringP of as many polys")
        dv = self._block(values, Q.npoly, "cannot EncodeRingT (FrequencyDomain): len(values)=%%d > slots=%d" % self.ringT.N)
        rot = None
        if rots is not None:
            if len(rots) != Q.npoly:
                raise RingHipError("cannot EmbedRows: %d rotations given for a block of %d polys" % (len(rots), Q.npoly))
            rot = (C.c_int * max(Q.npoly, 1))(*[int(r) & (int(cols) - 1) for r in rots])
        scale, ntt, mont = getattr(metadata, "Scale", 1), metadata.IsNTT, getattr(metadata, "IsMontgomery", False)
        _check(lib().rh_bgv_embed_qp(self._h, self.ringP._h, Q.limbs - 1, P.limbs - 1, int(scale) % (1 << 64), dv.ptr, dv.n, 1 if dv.signed else 0,
                                     Q.npoly, rot, int(cols), Q.ptr, P.ptr, 1 if ntt else 0, 1 if mont else 0))

    def EncodeRingT(self, values, scale, pT):
        """:187-246; pT: a DevicePoly of RingT(), one limb"""
        dv = self._block(values, pT.npoly, "cannot EncodeRingT (FrequencyDomain): len(values)=%%d > slots=%d" % self.ringT.N)
        self._t_block(pT, "EncodeRingT")
        _check(lib().rh_bgv_encode_ring_t(self._h, int(scale) % (1 << 64), dv.ptr, dv.n, 1 if dv.signed else 0, pT.npoly, pT.ptr))

    # ---- Decode (:323-353, :442-487) --------------------------------------------------------------------------------------------------------
    def _t_block(self, pT, who):
        if pT.ring._h.value != self.ringT._h.value or pT.limbs != 1:
            raise RingHipError("cannot %s: pT must be a one-limb poly block of RingT()" % who)

    def _new_values(self, nvec, signed):
        return np.zeros((nvec, self.ringT.N), dtype=np.int64 if signed else np.uint64)

    def DecodeRingT(self, pT, scale, values=None, signed=False):
        """:323-353: values None (a new (nvec, slots) array, int64 with signed), a numpy array of dtype uint64 or int64 -- (nvec, k), or (k,) for
        a single vector -- or a DeviceValues; filled and returned"""
        self._t_block(pT, "DecodeRingT")
        dv, host, signed = self._out(self._new_values(pT.npoly, signed) if values is None else values, pT.npoly, "DecodeRingT")
        _check(lib().rh_bgv_decode_ring_t(self._h, int(scale) % (1 << 64), pT.ptr, pT.npoly, dv.ptr, dv.n, 1 if signed else 0))
        return self._back(dv, host)

    def Decode(self, pt, values=None, signed=False):
        """:442-487, values as for DecodeRingT; IsBatched = false: the coefficients of the plaintext ring in their order"""
        p = pt.Value[0]
        if self._ring_of(p, "Decode") is not self.ringQ:
            raise RingHipError("cannot Decode: the plaintext must live in ringQ")
        dv, host, signed = self._out(self._new_values(p.npoly, signed) if values is None else values, p.npoly, "Decode")
        _check(lib().rh_bgv_decode(self._h, p.limbs - 1, int(getattr(pt, "Scale", 1)) % (1 << 64), p.ptr, p.npoly, dv.ptr, dv.n, 1 if signed else 0,
                                   1 if getattr(pt, "IsBatched", True) else 0, 1 if pt.IsNTT else 0))
        return self._back(dv, host)

    # ---- the two conversions alone (:357-439) ------------------------------------------------------------------------------------------------
    def RingT2Q(self, level, scaleUp, pT, pQ):
        self._t_block(pT, "RingT2Q")
        ring = self._ring_of(pQ, "RingT2Q")
        if pQ.limbs != level + 1 or pQ.npoly != pT.npoly:
            raise RingHipError("cannot RingT2Q: pQ must be a block of %d polys with level + 1 = %d limbs" % (pT.npoly, level + 1))
        _check(lib().rh_bgv_ring_t2q(self._h, ring._h, int(level), 1 if scaleUp else 0, pT.ptr, pQ.ptr, pT.npoly))

    def RingQ2T(self, level, scaleDown, pQ, pT):
        self._t_block(pT, "RingQ2T")
        if not scaleDown:
            raise RingHipError("cannot RingQ2T: scaleDown = false is not built on the device (the encoder calls it with true only)")
        if self._ring_of(pQ, "RingQ2T") is not self.ringQ or pQ.limbs != level + 1 or pQ.npoly != pT.npoly:
            raise RingHipError("cannot RingQ2T: pQ must be a block of %d polys of ringQ with level + 1 = %d limbs" % (pT.npoly, level + 1))
        _check(lib().rh_bgv_ring_q2t(self._h, int(level), pQ.ptr, pT.ptr, pT.npoly))


# ---- bgv.NewEncryptor / NewDecryptor (schemes/bgv/bgv.go): rlwe's, carrying the Plaintext metadata ---------------------------------------------------
class Encryptor(rlwe.Encryptor):
    """bgv.Encryptor: rlwe.Encryptor on bgv.Plaintext batches; the ciphertext takes the plaintext's Scale and IsBatched"""


class Decryptor(rlwe.Decryptor):
    """bgv.Decryptor: rlwe.Decryptor; DecryptNew returns a bgv.Plaintext with the ciphertext's Scale and IsBatched"""

    def DecryptNew(self, ct, fused=None):
        poly = self.ringQ.AtLevel(ct.Level()).NewPoly(ct.Value[0].npoly)
        pt = Plaintext(poly, getattr(ct, "Scale", 1), ct.IsNTT, getattr(ct, "IsMontgomery", False), getattr(ct, "IsBatched", True))
        self.Decrypt(ct, pt, fused)
        return pt

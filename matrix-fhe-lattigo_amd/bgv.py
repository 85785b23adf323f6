"""Host-side mirror of bgv.Evaluator, schemes/bgv/evaluator.go, on device-resident batches in the NTT domain: the scale-invariant (BFV)
multiply and the BGV half -- standard tensoring, multiply-accumulate, Add / Sub with scale matching, scalar operands, Rescale.  Call sequences
and the scale bookkeeping (Python ints modulo T) only: the arithmetic is the HIP library's (csrc/bfv.hip, csrc/bgv.hip); key generation and the
BGV encoder stay with the reference, so slice operands ([]uint64 / []int64) are refused by name.

  newEvaluatorPrecomp      :46-78        MulScaleInvariant(New)       :771-857     MulRelinScaleInvariant(New)  :877-972
  tensorScaleInvariant     :975-1040     MulScaleInvariant (scale)    :1045-1051   quantize                     :1104-1124
  Add(New) / Sub(New)      :173-432      evaluateInPlace              :270-286     matchScaleThenEvaluateInPlace :288-305
  Mul(New) / MulRelin(New) :458-663      tensorStandard               :665-751     MulThenAdd / MulRelinThenAdd :1142-1287
  mulRelinThenAdd          :1289-1403    Rescale                      :1415-1445   MatchScalesAndLevel          :1593-1614
  matchScalesBinary        :1620-1659

A batch of B ciphertexts is one Ciphertext whose polys have npoly = B; all operands of a call sit at the same level (dense
(npoly, level+1, N) blocks), which may be lower than the ring's top: a mismatch raises.  A degree-0 Ciphertext plays the role of a plaintext.
Scales are Python ints modulo T in the attribute Scale (1 when a ciphertext carries none).  In this scheme a ciphertext of scale s has the
phase c0 + c1 s = (m s) T^-1 + e modulo Q: T times the phase is m s + T e."""
import ctypes as C
import math

import numpy as np

from .ringhip import RingHipError, _check, _p, _u64, lib
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


def _is_int(op):
    return isinstance(op, (int, np.integer)) and not isinstance(op, bool)


class Evaluator(rlwe.Evaluator):
    """bgv.Evaluator.  ringQMul: bgv/params.go:98-108 (ceil((bitlen(Q) + logN) / 61) NTT-friendly 61-bit primes disjoint from Q), needed by the
    scale-invariant methods only: None builds a pure BGV evaluator, whose scale-invariant methods raise.  ringP / rlk: the key-switch ring and the
    relinearisation key (rlwe.GadgetCiphertext) for the Relin forms.  scaleInvariant: NewEvaluator's flag (:125-134): Mul / MulRelin dispatch
    to the scale-invariant forms (:460-465, :604-606) and Rescale does nothing (:1417).  fused: the BGV hot paths as one kernel each
    (rh_bgv_tensor, rh_bgv_mul_plain, rh_bgv_axpby); False issues the reference's own sequence of Ring calls -- the same bits."""

    def __init__(self, ringQ, ringQMul=None, t=None, ringP=None, rlk=None, scaleInvariant=False, fused=True):
        if t is None:
            raise RingHipError("bgv.Evaluator: the plaintext modulus t is missing")
        super().__init__(ringQ, ringP, galois_keys={"rlk": rlk} if rlk is not None else None)
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
        """:771-830, ciphertext branch: opOut (degree 2) = op0 x op1 * T / Q"""
        self._need_qmul("MulScaleInvariant")
        self._operands(op0, op1, opOut, False, "MulInvariant")
        self.tensorScaleInvariant(op0, op1, False, opOut)

    def MulRelinScaleInvariant(self, op0, op1, opOut):
        """:877-941, ciphertext branch: the same, relinearised to degree 1"""
        self._need_qmul("MulRelinScaleInvariant")
        self._operands(op0, op1, opOut, True, "MulRelinInvariant")
        self.tensorScaleInvariant(op0, op1, True, opOut)

    def _new(self, degree, like):
        level, npoly = like.Level(), like.Value[0].npoly
        ringQ = self.ringQ.AtLevel(level)
        return Ciphertext([ringQ.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)

    def MulScaleInvariantNew(self, op0, op1):
        """:849-857"""
        opOut = self._new(2, op0)
        self.MulScaleInvariant(op0, op1, opOut)
        return opOut

    def MulRelinScaleInvariantNew(self, op0, op1):
        """:960-972"""
        opOut = self._new(1, op0)
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
        if self.ScaleInvariant and (isinstance(op1, Ciphertext) or _is_slice(op1)):
            return self.MulScaleInvariant(op0, op1, opOut)
        self._refuse_slice(op1, "Mul")
        if _is_int(op1):
            return self._mul_scalar(op0, op1, opOut, "Mul")
        self.tensorStandard(op0, op1, False, opOut, "Mul")

    def MulRelin(self, op0, op1, opOut):
        """:602-629: the same, relinearised to degree 1"""
        if self.ScaleInvariant:
            return self.MulRelinScaleInvariant(op0, op1, opOut)
        self._refuse_slice(op1, "MulRelin")
        if _is_int(op1):
            return self._mul_scalar(op0, op1, opOut, "MulRelin")
        self.tensorStandard(op0, op1, True, opOut, "MulRelin")

    def MulNew(self, op0, op1):
        """:564-581"""
        if self.ScaleInvariant and (isinstance(op1, Ciphertext) or _is_slice(op1)):
            return self.MulScaleInvariantNew(op0, op1)
        self._refuse_slice(op1, "Mul")
        opOut = self._new_binary(op0, op1, op0.Degree() + op1.Degree() if isinstance(op1, Ciphertext) else None)
        self.Mul(op0, op1, opOut)
        return opOut

    def MulRelinNew(self, op0, op1):
        """:649-663"""
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

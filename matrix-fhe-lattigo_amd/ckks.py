"""Host-side mirror of ckks.Evaluator, schemes/ckks/evaluator.go, on device-resident batches in the NTT domain: call sequences and the scale
bookkeeping only -- the arithmetic is the HIP library's (csrc/ckks.hip and the ring entry points); key generation stays with the reference.
Slice operands ([]complex128 / []float64) are encoded on the device when the evaluator is given an Encoder (the class at the end of this
file, csrc/ckks_encoder.hip) and refused by name when it is not.

  Add(New) / Sub(New)   :59-244      evaluateInPlace   :246-431     evaluateWithScalar  :433-447     ScaleUp / SetScale  :449-478
  DropLevel(New)        :480-492     Rescale           :500-535     RescaleTo           :543-602     Mul(New)            :604-728
  MulRelin(New)         :730-784     mulRelin          :786-881     MulThenAdd          :918-1046    MulRelinThenAdd     :1065-1093
  mulRelinThenAdd       :1095-1178   Rotate / Conjugate / RotateHoisted (New)  :1195-1255            bigComplexToRNSScalar  scaling.go:10-43

A batch of B ciphertexts is one Ciphertext whose polys have npoly = B.  All operands of one call sit at the same level (every poly block has
level+1 limbs): the device layout is (poly, limb, N) contiguous, so a poly cannot be read at a lower level than it was allocated for --
DropLevel copies the leading limbs into blocks of the lower level.  A degree-0 Ciphertext plays the role of a plaintext.  Scales are `Scale`
objects in the attribute Scale; MulRelin and Rescale still serve ciphertexts that carry none, every other method raises on one."""
from fractions import Fraction

import numpy as np

from .ringhip import AutomorphismNTTIndex, ConjugateInvariant, DevicePoly, Ring, RingHipError, Standard, _check, _p, _u64, lib
from .schemes import Ciphertext, MatrixCKKSEvaluator
from . import rlwe

ScalePrecision = 128            # core/rlwe/scale.go:12-15
GaloisGen = 5                   # ring/ring.go
_round = MatrixCKKSEvaluator._round_to_prec

ADD_SCALAR, SUB_SCALAR, MUL_SCALAR, MUL_SCALAR_THEN_ADD = range(4)      # enum rh_ckks_scalar_op


class Scale:
    """rlwe.Scale without a modulus (core/rlwe/scale.go): a big.Float of ScalePrecision = 128 bits.  The value is an exact rational that is
    rounded to 128 significant bits, half to even, when it is set and after every Mul / Div -- Go's new(big.Float).Mul / Quo take the larger
    operand precision (128 on both sides here) and round to nearest even."""
    __slots__ = ("Value",)

    def __init__(self, s):
        if isinstance(s, Scale):
            s = s.Value
        v = Fraction(s)
        if v < 0:
            raise RingHipError("scale cannot be negative, but is %s" % (s,))
        self.Value = _round(v, ScalePrecision)

    def Mul(self, s1):
        return Scale(self.Value * Scale(s1).Value)

    def Div(self, s1):
        return Scale(self.Value / Scale(s1).Value)

    def Cmp(self, s1):
        a, b = self.Value, Scale(s1).Value
        return (a > b) - (a < b)

    def Max(self, s1):
        s1 = Scale(s1)
        return s1 if self.Cmp(s1) < 0 else self

    def Min(self, s1):
        s1 = Scale(s1)
        return s1 if self.Cmp(s1) > 0 else self

    def Equal(self, s1):
        return self.Cmp(s1) == 0

    def Float64(self):
        return float(self.Value)          # int / int true division rounds to nearest even, as big.Float.Float64 does

    def Uint64(self):
        return min(int(self.Value), (1 << 64) - 1)

    def BigInt(self):
        return int(_round(self.Value + Fraction(1, 2), ScalePrecision))

    def __eq__(self, other):
        return isinstance(other, (Scale, int, float, Fraction)) and self.Cmp(other) == 0

    def __hash__(self):
        return hash(self.Value)

    def __repr__(self):
        return "Scale(%s)" % (self.Value,)


def GaloisElement(N, k, NthRoot=None):
    """rlwe.Parameters.GaloisElement (core/rlwe/params.go:671-675): GaloisGen^k mod NthRoot (2N; 4N on a conjugate-invariant ring); a negative k
    is taken modulo NthRoot, a multiple of the order of GaloisGen"""
    NthRoot = 2 * int(N) if NthRoot is None else int(NthRoot)
    return pow(GaloisGen, int(k) % NthRoot, NthRoot)


def GaloisElementOrderTwoOrthogonalSubgroup(N):
    """:683-689: X -> X^-1, the conjugation, 2N - 1"""
    return 2 * int(N) - 1


def _is_slice(op):
    return isinstance(op, (list, tuple, np.ndarray))


class Complex:
    """bignum.Complex (utils/bignum/complex.go:13-16): two big.Floats, held as exact rationals -- the scalar operand type that carries more
    than a complex128 does (the coefficients of a polynomial, polynomial.py)"""
    __slots__ = ("re", "im")

    def __init__(self, re_=0, im_=0):
        self.re, self.im = Fraction(re_), Fraction(im_)

    def __eq__(self, other):
        return isinstance(other, Complex) and (self.re, self.im) == (other.re, other.im)

    def __hash__(self):
        return hash((self.re, self.im))

    def __complex__(self):
        return complex(float(self.re), float(self.im))

    def __repr__(self):
        return "Complex(%s, %s)" % (self.re, self.im)


def _is_scalar(op):
    return isinstance(op, (int, float, complex, Fraction, Complex, np.integer, np.floating, np.complexfloating)) and not isinstance(op, bool)


def to_complex(value, prec):
    """bignum.ToComplex (utils/bignum/complex.go:22-55): both parts as big.Floats of `prec` bits -- ints and big.Floats (Fractions here) are
    ROUNDED to prec bits like floats.  Returns two Fractions."""
    if isinstance(value, Complex):
        re_, im_ = value.re, value.im
    elif isinstance(value, (complex, np.complexfloating)):
        re_, im_ = Fraction(float(value.real)), Fraction(float(value.imag))
    elif isinstance(value, (float, np.floating)):
        re_, im_ = Fraction(float(value)), Fraction(0)
    else:
        re_, im_ = Fraction(int(value) if isinstance(value, (int, np.integer)) else value), Fraction(0)
    return _round(re_, prec), _round(im_, prec)


def scaled_int(x, scale, prec):
    """one part of bigComplexToRNSScalar (schemes/ckks/scaling.go:16-27): new(big.Float).Mul(x, scale) rounded to the larger operand precision,
    plus / minus 0.5 by the sign of x rounded at that same precision, .Int truncating toward zero"""
    prec = max(int(prec), ScalePrecision)
    r = _round(x * scale, prec)
    if x > 0:
        r = _round(r + Fraction(1, 2), prec)
    elif x < 0:
        r = _round(r - Fraction(1, 2), prec)
    return int(r)                         # Fraction -> int truncates toward zero


class Evaluator:
    """ckks.Evaluator.  ringP / rlk / galois_keys: the key-switch ring, the relinearisation key and the Galois keys (a dict Galois element ->
    rlwe.GadgetCiphertext).  fused: True the kernels of csrc/ckks.hip wherever there is one, False the reference's own sequence of Ring calls --
    the same bits; None (default) what FUSED_DEFAULT says per kernel, the measured choice.  encoding_precision:
    Parameters.EncodingPrecision(), max(53, floor(log2 DefaultScale)) (schemes/ckks/params.go:187-195)."""

    # profiles/ckks_ops.json: the scalar kernel is not faster than the four half-row launches; profiles/ckks_polynomial.json: the one-launch baby step
    # (polynomial.py) is 4 to 7 % slower than the composed calls at batch 64 through this layer, whose per-term host work the composed launches overlap
    FUSED_DEFAULT = {"tensor": True, "mul_plain": True, "scalar": False, "scale_then_add": True, "linear_combination": False}

    def __init__(self, ringQ, ringP=None, rlk=None, levels_consumed_per_rescaling=1, galois_keys=None, fused=None, encoding_precision=53, encoder=None):
        self.ringQ, self.ringP, self.rlk = ringQ, ringP, rlk
        self.encoder = encoder             # ckks.Encoder: with one, slice operands take the reference's slice branches; without, they are refused
        self.nb_rescales = int(levels_consumed_per_rescaling)
        self.fused = dict(self.FUSED_DEFAULT) if fused is None else {k: bool(fused) for k in self.FUSED_DEFAULT}
        self.fused_tensor = fused is None or bool(fused)   # regular ct x ct case: rh_ring_tensor_degree1 instead of six element-wise launches (same bits)
        self.encoding_precision = int(encoding_precision)
        self.ks = rlwe.Evaluator(ringQ, ringP, galois_keys=galois_keys) if ringP is not None else None
        self._pool = {}
        self._roots1 = None
        self._scalars = {}                 # _rns_scalar's results by (level, scale, constant): host big-integer work, about a millisecond each at 16 limbs

    def close(self):
        self._pool.clear()
        if self.ks:
            self.ks.close()

    def _buffer(self, tag, ring, npoly, limbs):
        key = (tag, id(ring._h), npoly, limbs)
        p = self._pool.get(key)
        if p is None:
            p = self._pool[key] = DevicePoly(ring, npoly, limbs)
        return p

    def _same_level(self, *cts):
        lv = {c.Level() for c in cts}
        if len(lv) != 1:
            raise RingHipError("operands must sit at the same level, got %s" % sorted(lv))
        return lv.pop()

    # ---- operands, scales, host scalars ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _scale(ct, who):
        s = getattr(ct, "Scale", None)
        if s is None:
            raise RingHipError("cannot %s: a ciphertext carries no Scale" % who)
        return s if isinstance(s, Scale) else Scale(s)

    def _operands(self, who, *cts):
        for ct in cts:
            if not ct.IsNTT:
                raise RingHipError("cannot %s: operands must be in the NTT domain" % who)
        lv = {ct.Level() for ct in cts}
        if len(lv) != 1:
            raise RingHipError("cannot %s: operands must sit at the same level, got %s" % (who, sorted(lv)))
        level = lv.pop()
        for ct in cts:
            rlwe.Evaluator._rows(level, *ct.Value)
        if len({p.npoly for ct in cts for p in ct.Value}) != 1:
            raise RingHipError("cannot %s: every poly block of a call holds the same number of polys" % who)
        return level

    def _refuse(self, op1, who):
        if _is_slice(op1) and self.encoder is not None:
            return
        if _is_slice(op1):
            raise RingHipError("cannot %s: op1 of type %s (a slice, []complex128 / []float64 ...) needs the CKKS encoder, which the device path does not build"
                               % (who, type(op1).__name__))
        if not (_is_scalar(op1) or isinstance(op1, Ciphertext)):
            raise RingHipError("cannot %s: invalid op1.(type): must be a Ciphertext, int, float, complex or Fraction, but is %s" % (who, type(op1).__name__))

    def _encode_slice(self, op0, op1, level, scale):
        """the plaintext of the slice branches (:112-126, :697-718, :1021-1035): eval.buffQ[0] at op0's level with op0's metadata and the scale
        given, the vector encoded into it on the device (one vector shared by the batch, or one per ciphertext)"""
        pt = Plaintext(self._buffer("buffQ0", self.ringQ.AtLevel(level), op0.Value[0].npoly, level + 1), scale,
                       getattr(op0, "LogDimensions", self.encoder.LogMaxSlots), is_ntt=op0.IsNTT, is_montgomery=getattr(op0, "IsMontgomery", False))
        self.encoder.Encode(op1, pt)
        return pt

    def _qs(self, level):
        return [int(q) for q in self.ringQ.moduli[:level + 1]]

    def _rescale_scale(self, level):
        """the scale a non-integer constant is given: q_level ... over levels_consumed_per_rescaling moduli (:665-671, :962-966)"""
        qs = self._qs(level)
        if level - (self.nb_rescales - 1) < 0:
            raise RingHipError("level %d is too low for a constant scaled by %d moduli" % (level, self.nb_rescales))
        scale = Scale(qs[level])
        for i in range(1, self.nb_rescales):
            scale = scale.Mul(Scale(qs[level - i]))
        return scale

    def _rns_scalar(self, level, scale, cmplx):
        """bigComplexToRNSScalar (scaling.go:10-43) followed by the scalar half of evaluateWithScalar (:439-442): the RNS scalars for
        coefficients [0, N/2) and [N/2, N).  cmplx: the two Fractions of to_complex."""
        key = (level, Scale(scale).Value, cmplx[0], cmplx[1])                                  # a circuit asks for the same few scalars call after call
        hit = self._scalars.get(key)
        if hit is not None:
            return hit
        if len(self._scalars) >= 4096:
            self._scalars.clear()
        qs = self._qs(level)
        real = scaled_int(cmplx[0], Scale(scale).Value, self.encoding_precision)
        imag = scaled_int(cmplx[1], Scale(scale).Value, self.encoding_precision)
        s0, s1 = [], []
        if imag != 0 and self._roots1 is None:
            self._roots1 = [int(w) for w in self.ringQ.constants()["roots_fwd"][:, 1]]          # SubRing.RootsForward[1], Montgomery form
        for i, q in enumerate(qs):
            re_, im_ = real % q, imag % q                                                        # NewRNSScalarFromBigint: the non-negative residue
            if im_:
                im_ = im_ * self._roots1[i] * pow(1 << 64, -1, q) % q                            # MRed(RNSImag[i], RootsForward[1]) (:440)
            s0.append((re_ + im_) % q)                                                           # (:441)
            s1.append((re_ + q - im_) % q)
        self._scalars[key] = (tuple(s0), tuple(s1))
        return self._scalars[key]

    def _use(self, kind):
        return self.fused[kind]

    @staticmethod
    def _ptrs(polys, n=3):
        return [p.ptr for p in polys] + [None] * (n - len(polys))

    def _scalar_op(self, level, op, ins, outs, s0, s1):
        """evaluateWithScalar's loop (:444-446) on the components given"""
        rq = self.ringQ.AtLevel(level)
        if self._use("scalar"):
            a, b = _u64(s0), _u64(s1)
            _check(lib().rh_ckks_scalar(self.ringQ._h, level, op, *self._ptrs(ins), *self._ptrs(outs), ins[0].npoly, _p(a), _p(b)))
            return
        f = (rq.AddDoubleRNSScalar, rq.SubDoubleRNSScalar, rq.MulDoubleRNSScalar, rq.MulDoubleRNSScalarThenAdd)[op]
        for x, y in zip(ins, outs):
            f(x, s0, s1, y)

    def _new(self, degree, like):
        level, npoly = like.Level(), like.Value[0].npoly
        rq = self.ringQ.AtLevel(level)
        return Ciphertext([rq.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)

    # ---- Add / Sub :59-244, evaluateInPlace :246-431 -------------------------------------------------------------------------------------
    def _add_sub(self, op0, op1, opOut, sub):
        who = "Sub" if sub else "Add"
        self._refuse(op1, who)
        if _is_scalar(op1):                                                        # (:82-101, :178-197)
            level = self._operands(who, op0, opOut)
            scale0 = self._scale(op0, who)
            if opOut.Degree() != op0.Degree():
                raise RingHipError("cannot %s: opOut must have degree %d" % (who, op0.Degree()))
            s0, s1 = self._rns_scalar(level, scale0, to_complex(op1, self.encoding_precision))
            self._scalar_op(level, SUB_SCALAR if sub else ADD_SCALAR, op0.Value[:1], opOut.Value[:1], s0, s1)
            if op0 is not opOut:
                rq = self.ringQ.AtLevel(level)
                for i in range(1, op0.Degree() + 1):
                    rq.CopyLvl(op0.Value[i], opOut.Value[i])
            opOut.Scale, opOut.IsNTT = scale0, True
            return
        if _is_slice(op1):                                                         # (:103-129, :199-225)
            level = self._operands(who, op0, opOut)
            op1 = self._encode_slice(op0, op1, level, self._scale(op0, who))
        level = self._operands(who, op0, op1, opOut)
        c0Scale, c1Scale = self._scale(op0, who), self._scale(op1, who)
        d0, d1 = op0.Degree(), op1.Degree()
        lo, hi = min(d0, d1), max(d0, d1)
        if opOut.Degree() != hi:
            raise RingHipError("cannot %s: opOut must have degree %d" % (who, hi))
        rq = self.ringQ.AtLevel(level)
        cmp = c0Scale.Cmp(c1Scale)
        ratio = None
        if cmp:
            ratioInt = int((c0Scale.Div(c1Scale) if cmp == 1 else c1Scale.Div(c0Scale)).Value)      # ratioFlo.Int(nil)
            # Mul(ct, ratioInt, tmp) (:282 ...): a *big.Int through bignum.ToComplex, a Gaussian integer, scale 1
            ratio = self._rns_scalar(level, Scale(1), to_complex(ratioInt, self.encoding_precision))
        if self._use("scale_then_add"):
            a, b, o = self._ptrs(op0.Value), self._ptrs(op1.Value), self._ptrs(opOut.Value)
            k = _u64(ratio[0]) if ratio is not None else None
            _check(lib().rh_ckks_scale_then_add(self.ringQ._h, level, *a, *b, *o, op0.Value[0].npoly, _p(k), 1 if sub else 0, 1 if cmp == 1 else 0))
        else:
            npoly = op0.Value[0].npoly
            tmp0, tmp1 = op0, op1
            scaled = op1 if cmp == 1 else op0 if cmp == -1 else None
            if scaled is not None:
                if scaled is opOut:                                                # scaled in place (:295, :319)
                    dst = opOut
                else:                                                              # into eval.BuffCt (:273, :336, :366, :390)
                    dst = Ciphertext([self._buffer("BuffCt%d" % i, rq, npoly, level + 1) for i in range(scaled.Degree() + 1)], is_ntt=True)
                for x, y in zip(scaled.Value, dst.Value):
                    rq.MulDoubleRNSScalar(x, ratio[0], ratio[1], y)
                if cmp == 1:
                    tmp1 = dst
                else:
                    tmp0 = dst
            f = rq.Sub if sub else rq.Add
            for i in range(lo + 1):
                f(tmp0.Value[i], tmp1.Value[i], opOut.Value[i])                    # (:413-415)
            if d0 > d1 and tmp0 is not opOut:
                for i in range(lo + 1, hi + 1):
                    rq.CopyLvl(tmp0.Value[i], opOut.Value[i])                      # (:422-425)
            elif d1 > d0 and tmp1 is not opOut:
                for i in range(lo + 1, hi + 1):
                    rq.CopyLvl(tmp1.Value[i], opOut.Value[i])                      # (:426-430)
            if sub and d0 < d1:
                for i in range(d0 + 1, d1 + 1):
                    rq.Neg(opOut.Value[i], opOut.Value[i])                         # (:173-177)
        opOut.Scale, opOut.IsNTT = c0Scale.Max(c1Scale), True                      # (:417)

    def Add(self, op0, op1, opOut):
        """:66-135: op1 a Ciphertext (degrees up to 2; the operand with the smaller scale is first multiplied by the integer part of the
        ratio of the scales) or a scalar (added to component 0 at op0's scale)"""
        self._add_sub(op0, op1, opOut, False)

    def Sub(self, op0, op1, opOut):
        """:156-232"""
        self._add_sub(op0, op1, opOut, True)

    def _new_binary(self, op0, op1):
        return self._new(max(op0.Degree(), op1.Degree()) if isinstance(op1, Ciphertext) else op0.Degree(), op0)

    def AddNew(self, op0, op1):
        """:144-147 (the reference's Resize lets opOut grow to the larger degree: it is allocated with it here)"""
        self._refuse(op1, "Add")
        opOut = self._new_binary(op0, op1)
        self.Add(op0, op1, opOut)
        return opOut

    def SubNew(self, op0, op1):
        """:241-244"""
        self._refuse(op1, "Sub")
        opOut = self._new_binary(op0, op1)
        self.Sub(op0, op1, opOut)
        return opOut

    # ---- ScaleUp, SetScale, DropLevel :449-492 --------------------------------------------------------------------------------------------
    def ScaleUp(self, op0, scale, opOut):
        """:456-465: op0 times scale.Uint64(), the scale multiplied by `scale`"""
        scale = Scale(scale)
        scale0 = self._scale(op0, "ScaleUp")
        self._mul_scalar(op0, scale.Uint64(), opOut, "ScaleUp")
        opOut.Scale = scale0.Mul(scale)

    def ScaleUpNew(self, op0, scale):
        opOut = self._new(op0.Degree(), op0)
        self.ScaleUp(op0, scale, opOut)
        return opOut

    def SetScale(self, ct, scale):
        """:468-478: ct times scale / ct.Scale (a *big.Float: not an integer, so it is scaled by the moduli one rescaling consumes), RescaleTo
        the target, and the scale set to it"""
        scale = Scale(scale)
        ratioFlo = scale.Div(self._scale(ct, "SetScale")).Value
        self._mul_scalar(ct, ratioFlo, ct, "SetScale")
        self.RescaleTo(ct, scale, ct)
        ct.Scale = scale

    def _resize(self, ct, level):
        """rlwe.Element.Resize to a lower level: device blocks are dense, so the leading limbs are copied into blocks of that level"""
        rq = self.ringQ.AtLevel(level)
        for i, p in enumerate(ct.Value):
            if p.limbs != level + 1:
                q = rq.NewPoly(p.npoly)
                rq.CopyLvl(p, q)
                ct.Value[i] = q

    def DropLevel(self, op0, levels):
        """:490-492: no rescaling"""
        if not 0 <= int(levels) <= op0.Level():
            raise RingHipError("cannot DropLevel: %d levels from level %d" % (levels, op0.Level()))
        self._resize(op0, op0.Level() - int(levels))

    def DropLevelNew(self, op0, levels):
        """:482-486"""
        opOut = Ciphertext(list(op0.Value), is_ntt=op0.IsNTT)
        if hasattr(op0, "Scale"):
            opOut.Scale = op0.Scale
        if int(levels) == 0:
            rq = self.ringQ.AtLevel(op0.Level())
            opOut.Value = [rq.NewPoly(p.npoly) for p in op0.Value]
            for p, q in zip(op0.Value, opOut.Value):
                rq.CopyLvl(p, q)
            return opOut
        self.DropLevel(opOut, levels)
        return opOut

    # ---- Rescale :500-535, RescaleTo :543-602 ---------------------------------------------------------------------------------------------
    def Rescale(self, op0, opOut):
        """Rescale (:500-535): DivRoundByLastModulusManyNTT(nbRescales) on every component.  opOut's polys keep op0's limb count; limbs
        0 .. level-nbRescales hold the result (ring/scaling.go:130-156).  With a Scale on op0 the scale is divided by the consumed moduli."""
        nb = self.nb_rescales
        if op0.Level() <= nb - 1:
            raise RingHipError("cannot Rescale: input Ciphertext level is too low")
        if opOut.Degree() != op0.Degree():
            raise RingHipError("Rescale: degrees differ")
        rq = self.ringQ.AtLevel(op0.Level())
        if getattr(op0, "Scale", None) is not None:
            scale = self._scale(op0, "Rescale")
            for i in range(nb):
                scale = scale.Div(Scale(int(self.ringQ.moduli[op0.Level() - i])))          # (:522-524)
            opOut.Scale = scale
        for a, b in zip(op0.Value, opOut.Value):
            rq.DivRoundByLastModulusManyNTT(nb, a, b)
        opOut.IsNTT = op0.IsNTT

    def RescaleTo(self, op0, minScale, opOut):
        """:543-602: divides by the last moduli, one level each, as long as the scale stays at or above minScale / 2.  opOut's blocks are
        replaced by blocks of the new level (the reference's Resize); with nothing to divide op0 is copied."""
        minScale = Scale(minScale)
        if minScale.Cmp(Scale(0)) != 1:
            raise RingHipError("cannot RescaleTo: minScale is <0")
        minScale = minScale.Div(Scale(2))
        scale = self._scale(op0, "RescaleTo")
        if scale.Cmp(Scale(0)) != 1:
            raise RingHipError("cannot RescaleTo: ciphertext scale is <0")
        level = op0.Level()
        if level == 0:
            raise RingHipError("cannot RescaleTo: input Ciphertext already at level 0")
        if opOut.Degree() != op0.Degree() or not op0.IsNTT:
            raise RingHipError("cannot RescaleTo: opOut must have op0's degree and op0 must be in the NTT domain")
        rlwe.Evaluator._rows(level, *op0.Value)
        newLevel, nbRescales = level, 0
        while newLevel >= 0:                                                       # (:572-584)
            s = scale.Div(Scale(int(self.ringQ.moduli[newLevel])))
            if s.Cmp(minScale) == -1:
                break
            scale = s
            nbRescales += 1
            newLevel -= 1
        if newLevel < 0:
            raise RingHipError("cannot RescaleTo: the scale allows %d divisions, more than the %d levels above level 0" % (nbRescales, level))
        rq = self.ringQ.AtLevel(level)
        if nbRescales > 0:
            outs = [self.ringQ.AtLevel(newLevel).NewPoly(p.npoly) for p in op0.Value]
            for a, b in zip(op0.Value, outs):
                rq.DivRoundByLastModulusManyNTT(nbRescales, a, b)                  # (:590-593)
            opOut.Value = outs
        elif op0 is not opOut:
            for i, p in enumerate(op0.Value):                                      # opOut.Copy(op0) (:596-598)
                if opOut.Value[i].limbs != level + 1 or opOut.Value[i].npoly != p.npoly:
                    opOut.Value[i] = rq.NewPoly(p.npoly)
                rq.CopyLvl(p, opOut.Value[i])
        opOut.Scale, opOut.IsNTT = scale, True

    # ---- Mul / MulRelin :604-881 ----------------------------------------------------------------------------------------------------------
    def _mul_scalar(self, op0, op1, opOut, who):
        """the scalar branch of Mul (:646-683): a Gaussian integer multiplies as it is; any other constant is scaled by the moduli one
        rescaling consumes and the scale grows by that factor"""
        level = self._operands(who, op0, opOut)
        scale0 = self._scale(op0, who)
        if opOut.Degree() != op0.Degree():
            raise RingHipError("cannot %s: opOut must have degree %d" % (who, op0.Degree()))
        cmplx = to_complex(op1, self.encoding_precision)
        scale = Scale(1) if cmplx[0].denominator == 1 and cmplx[1].denominator == 1 else self._rescale_scale(level)
        s0, s1 = self._rns_scalar(level, scale, cmplx)
        self._scalar_op(level, MUL_SCALAR, op0.Value, opOut.Value, s0, s1)
        opOut.Scale, opOut.IsNTT = scale0.Mul(scale), True                        # (:681)

    def Mul(self, op0, op1, opOut):
        """:630-728: without relinearisation; op1 a Ciphertext (opOut of degree op0.Degree() + op1.Degree()) or a scalar"""
        self._refuse(op1, "Mul")
        if _is_scalar(op1):
            return self._mul_scalar(op0, op1, opOut, "Mul")
        if _is_slice(op1):                                                         # (:685-723)
            level = self._operands("Mul", op0, opOut)
            self._scale(op0, "Mul")
            if opOut.Degree() != op0.Degree():
                raise RingHipError("cannot Mul: opOut must have degree %d" % op0.Degree())
            op1 = self._encode_slice(op0, op1, level, self._rescale_scale(level))
        self._scale(op0, "Mul"), self._scale(op1, "Mul")
        self.MulRelin(op0, op1, opOut, relin=False)

    def MulNew(self, op0, op1):
        """:613-616 (opOut allocated with the product's degree)"""
        self._refuse(op1, "Mul")
        opOut = self._new(op0.Degree() + op1.Degree() if isinstance(op1, Ciphertext) else op0.Degree(), op0)
        self.Mul(op0, op1, opOut)
        return opOut

    def MulRelinNew(self, op0, op1):
        """:741-750"""
        self._refuse(op1, "MulRelin")
        ct = isinstance(op1, Ciphertext)
        opOut = self._new((1 if op0.Degree() == 1 and op1.Degree() == 1 else max(op0.Degree(), op1.Degree())) if ct else op0.Degree(), op0)
        if ct:
            self._scale(op0, "MulRelin"), self._scale(op1, "MulRelin")
        self.MulRelin(op0, op1, opOut)
        return opOut

    def MulRelin(self, op0, op1, opOut, relin=True):
        """mulRelin (:786-881).  Degree-1 x degree-1: tensoring (:821-834, squaring case :825-829 when op1 is op0), then
        with relin the gadget product of c2 with the relinearisation key and two Adds (:836-852); opOut has degree 1 with
        relin, 2 without.  Degree-0 x degree-1 (plaintext x ciphertext): MForm + MulCoeffsMontgomery per component (:855-878).
        A scalar op1 goes to Mul (:778-781).  Operands that carry scales give opOut their product (:790)."""
        if not isinstance(op1, Ciphertext):
            self._refuse(op1, "MulRelin")
            if _is_slice(op1):
                return self.Mul(op0, op1, opOut)                                   # (:778-781)
            return self._mul_scalar(op0, op1, opOut, "MulRelin")
        if not (op0.IsNTT and op1.IsNTT):
            raise RingHipError("MulRelin: operands must be in the NTT domain")
        level = self._same_level(op0, op1, opOut)
        rq = self.ringQ.AtLevel(level)
        npoly = op0.Value[0].npoly
        counter = [0]

        def new():                         # eval.buffQ[i]: evaluator-owned, allocated once per shape
            counter[0] += 1
            return self._buffer("buffQ%d" % counter[0], rq, npoly, level + 1)
        d0, d1 = op0.Degree(), op1.Degree()
        if d0 == 1 and d1 == 1:
            need = 1 if relin else 2
            if opOut.Degree() != need:
                raise RingHipError("MulRelin: opOut must have degree %d" % need)
            if relin and (self.rlk is None or self.ks is None):
                raise RingHipError("cannot MulRelin: Relinearize: relinearization key is missing")
            c00, c01 = new(), new()
            c0, c1 = opOut.Value[0], opOut.Value[1]
            c2 = new() if relin else opOut.Value[2]
            tmp0, tmp1 = (op1, op0) if op1 is opOut else (op0, op1)        # avoid overwriting when the second input is the output
            if self._use("tensor") and (op0 is op1 or op1 is opOut):        # squaring, or the swapped operands: one launch
                rlwe.Evaluator._rows(level, *tmp0.Value, *tmp1.Value, c0, c1, c2)
                sq = op0 is op1
                _check(lib().rh_ckks_tensor(self.ringQ._h, level, tmp0.Value[0].ptr, tmp0.Value[1].ptr, None if sq else tmp1.Value[0].ptr,
                                            None if sq else tmp1.Value[1].ptr, c0.ptr, c1.ptr, c2.ptr, npoly, 0, 1 if sq else 0))
            elif self.fused_tensor and op0 is not op1:                      # the same six ring calls as one kernel
                rq.TensorDegree1(tmp0.Value[0], tmp0.Value[1], tmp1.Value[0], tmp1.Value[1], c0, c1, c2)
            else:
                rq.MForm(tmp0.Value[0], c00)
                rq.MForm(tmp0.Value[1], c01)
                rq.MulCoeffsMontgomery(c00, tmp1.Value[0], c0)
                rq.MulCoeffsMontgomery(c01, tmp1.Value[1], c2)
                rq.MulCoeffsMontgomery(c00, tmp1.Value[1], c1)
                if op0 is op1:                                              # squaring
                    rq.Add(c1, c1, c1)
                else:
                    rq.MulCoeffsMontgomeryThenAdd(c01, tmp1.Value[0], c1)
            if relin:
                self.ks.GadgetProductThenAdd(level, c2, self.rlk, c0, c1, opOut)      # GadgetProduct + the two Adds (:850-852)
        elif (d0 == 0 or d1 == 0) and d0 + d1 <= 2:
            pt, ct = (op0, op1) if d0 == 0 else (op1, op0)
            if opOut.Degree() != max(d0, d1):
                raise RingHipError("MulRelin: opOut must have degree %d" % max(d0, d1))
            if self._use("mul_plain"):
                rlwe.Evaluator._rows(level, *pt.Value, *ct.Value, *opOut.Value)
                _check(lib().rh_ckks_mul_plain(self.ringQ._h, level, *self._ptrs(ct.Value), pt.Value[0].ptr, *self._ptrs(opOut.Value), npoly, 0))
            else:
                c0 = new()
                rq.MForm(pt.Value[0], c0)
                for i, v in enumerate(ct.Value):
                    rq.MulCoeffsMontgomery(c0, v, opOut.Value[i])
        else:
            raise RingHipError("MulRelin: unsupported degrees %d, %d" % (d0, d1))
        if getattr(op0, "Scale", None) is not None and getattr(op1, "Scale", None) is not None:
            opOut.Scale = self._scale(op0, "MulRelin").Mul(self._scale(op1, "MulRelin"))   # (:790)
        opOut.IsNTT = True

    # ---- MulThenAdd / MulRelinThenAdd :918-1178 -------------------------------------------------------------------------------------------
    def MulThenAdd(self, op0, op1, opOut):
        """:918-1046: opOut += op0 x op1 without relinearisation.  A scalar op1: opOut and op0 of equal scale and a constant that is not a
        Gaussian integer have opOut multiplied by the moduli one rescaling consumes first; opOut.Scale > op0.Scale scales the constant by
        the quotient; op0.Scale > opOut.Scale is refused."""
        self._refuse(op1, "MulThenAdd")
        if isinstance(op1, Ciphertext):
            if op0 is opOut or op1 is opOut:
                raise RingHipError("cannot MulThenAdd: opOut must be different from op0 and op1")     # (:927-929)
            return self.mulRelinThenAdd(op0, op1, False, opOut)
        who = "MulThenAdd"
        level = self._operands(who, op0, opOut)
        scale0, scaleOut = self._scale(op0, who), self._scale(opOut, who)
        if opOut.Degree() != op0.Degree():
            raise RingHipError("cannot MulThenAdd: opOut must have degree %d" % op0.Degree())
        if _is_slice(op1):                                                         # (:986-1039)
            cmp = scale0.Cmp(scaleOut)
            if cmp == 0:
                scaleRLWE = self._rescale_scale(level)
                self._mul_scalar(opOut, int(scaleRLWE.Value), opOut, who)          # eval.Mul(opOut, scaleInt, opOut)
                opOut.Scale = scaleOut.Mul(scaleRLWE)
            elif cmp == -1:
                scaleRLWE = scaleOut.Div(scale0)
            else:
                raise RingHipError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
            return self.MulThenAdd(op0, self._encode_slice(op0, op1, level, scaleRLWE), opOut)
        cmplx = to_complex(op1, self.encoding_precision)
        cmp = scale0.Cmp(scaleOut)
        if cmp == 0:                                                               # (:957-974)
            if cmplx[0].denominator == 1 and cmplx[1].denominator == 1:
                scaleRLWE = Scale(1)
            else:
                scaleRLWE = self._rescale_scale(level)
                self._mul_scalar(opOut, int(scaleRLWE.Value), opOut, who)          # eval.Mul(opOut, scaleInt, opOut)
                opOut.Scale = scaleOut.Mul(scaleRLWE)
        elif cmp == -1:
            scaleRLWE = scaleOut.Div(scale0)                                       # (:976-977)
        else:
            raise RingHipError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
        s0, s1 = self._rns_scalar(level, scaleRLWE, cmplx)                         # (:982)
        self._scalar_op(level, MUL_SCALAR_THEN_ADD, op0.Value, opOut.Value, s0, s1)
        opOut.IsNTT = True

    def MulRelinThenAdd(self, op0, op1, opOut):
        """:1065-1093: the same with the degree-2 term relinearised before it is added (opOut of degree 1 or 2)"""
        if isinstance(op1, Ciphertext) and op1.Degree() != 0:
            if op0 is opOut or op1 is opOut:
                raise RingHipError("cannot MulThenAdd: opOut must be different from op0 and op1")     # (:1078-1080)
            return self.mulRelinThenAdd(op0, op1, True, opOut)
        self.MulThenAdd(op0, op1, opOut)

    def mulRelinThenAdd(self, op0, op1, relin, opOut):
        """:1095-1178"""
        who = "MulRelinThenAdd" if relin else "MulThenAdd"
        level = self._operands(who, op0, op1, opOut)
        d0, d1 = op0.Degree(), op1.Degree()
        if d0 + d1 > 2 or d1 > 1 or d0 > 2:
            raise RingHipError("cannot %s: degrees %d and %d: the sum of the degrees is at most 2" % (who, d0, d1))
        ct = d0 == 1 and d1 == 1
        if not ct and d1 != 0:
            raise RingHipError("cannot %s: a degree-0 op0 with a degree-1 op1: give the plaintext as op1" % who)
        if ct and (opOut.Degree() != 2 if not relin else opOut.Degree() not in (1, 2)):
            raise RingHipError("cannot %s: opOut must have degree %s" % (who, "1 or 2" if relin else "2"))
        if not ct and opOut.Degree() < d0:
            raise RingHipError("cannot %s: opOut must have at least degree %d" % (who, d0))
        if ct and relin and (self.rlk is None or self.ks is None):
            raise RingHipError("cannot %s: cannot relinearize: relinearization key is missing" % who)
        resScale = self._scale(op0, who).Mul(self._scale(op1, who))               # (:1099)
        scaleOut = self._scale(opOut, who)
        if scaleOut.Cmp(resScale) == -1:
            ratio = resScale.Div(scaleOut)
            if ratio.Float64() >= 2.0:                                             # only scales up if int(ratio) >= 2 (:1103-1109)
                self._mul_scalar(opOut, ratio.Value, opOut, who)                   # eval.Mul(opOut, &ratio.Value, opOut): a *big.Float
                opOut.Scale = resScale
        rq = self.ringQ.AtLevel(level)
        npoly = op0.Value[0].npoly
        if ct:
            c0, c1 = opOut.Value[0], opOut.Value[1]
            c2 = self._buffer("buffQ3", rq, npoly, level + 1) if relin else opOut.Value[2]
            if self._use("tensor"):
                _check(lib().rh_ckks_tensor(self.ringQ._h, level, op0.Value[0].ptr, op0.Value[1].ptr, op1.Value[0].ptr, op1.Value[1].ptr,
                                            c0.ptr, c1.ptr, c2.ptr, npoly, 2 if relin else 1, 0))
            else:
                c00, c01 = self._buffer("buffQ1", rq, npoly, level + 1), self._buffer("buffQ2", rq, npoly, level + 1)
                rq.MForm(op0.Value[0], c00)                                        # (:1135-1136)
                rq.MForm(op0.Value[1], c01)
                rq.MulCoeffsMontgomeryThenAdd(c00, op1.Value[0], c0)               # (:1138-1140)
                rq.MulCoeffsMontgomeryThenAdd(c00, op1.Value[1], c1)
                rq.MulCoeffsMontgomeryThenAdd(c01, op1.Value[0], c1)
                if relin:
                    rq.MulCoeffsMontgomery(c01, op1.Value[1], c2)                  # (:1150)
                else:
                    rq.MulCoeffsMontgomeryThenAdd(c01, op1.Value[1], c2)           # (:1161)
            if relin:
                self.ks.GadgetProductThenAdd(level, c2, self.rlk, c0, c1, opOut)   # GadgetProduct + the two Adds (:1157-1159)
        else:                                                                      # plaintext x ciphertext (:1165-1175)
            if self._use("mul_plain"):
                _check(lib().rh_ckks_mul_plain(self.ringQ._h, level, *self._ptrs(op0.Value), op1.Value[0].ptr,
                                               *self._ptrs(opOut.Value[:d0 + 1]), npoly, 1))
            else:
                c00 = self._buffer("buffQ1", rq, npoly, level + 1)
                rq.MForm(op1.Value[0], c00)
                for i in range(d0 + 1):
                    rq.MulCoeffsMontgomeryThenAdd(op0.Value[i], c00, opOut.Value[i])
        opOut.IsNTT = True

    # ---- Rotate / Conjugate / RotateHoisted :1195-1255 ------------------------------------------------------------------------------------
    def _nth_root(self):
        return (4 if self.ringQ.kind == ConjugateInvariant else 2) * self.ringQ.N

    def GaloisElement(self, k):
        return GaloisElement(self.ringQ.N, k, self._nth_root())

    def _automorphism(self, op0, galEl, opOut, who):
        if self.ks is None:
            raise RingHipError("cannot %s: the evaluator was built without ringP, which the key switch needs" % who)
        scale = self._scale(op0, who)
        try:
            self.ks.Automorphism(op0, galEl, opOut)
        except RingHipError as e:
            raise RingHipError("cannot %s: %s" % (who, e)) from None
        opOut.Scale = scale

    def Rotate(self, op0, k, opOut):
        """:1202-1207: the slots rotated by k positions to the left"""
        self._automorphism(op0, self.GaloisElement(k), opOut, "Rotate")

    def RotateNew(self, op0, k):
        opOut = self._new(op0.Degree(), op0)
        self.Rotate(op0, k, opOut)
        return opOut

    def Conjugate(self, op0, opOut):
        """:1218-1229"""
        if self.ringQ.kind == ConjugateInvariant:
            raise RingHipError("cannot Conjugate: method is not supported when parameters.RingType() == ring.ConjugateInvariant")
        self._automorphism(op0, GaloisElementOrderTwoOrthogonalSubgroup(self.ringQ.N), opOut, "Conjugate")

    def ConjugateNew(self, op0):
        opOut = self._new(op0.Degree(), op0)
        self.Conjugate(op0, opOut)
        return opOut

    def RotateHoisted(self, ctIn, rotations, opOut):
        """:1245-1255: opOut, a dict rotation -> Ciphertext, filled with the rotations of ctIn, its decomposition shared"""
        if self.ks is None:
            raise RingHipError("cannot RotateHoisted: the evaluator was built without ringP, which the key switch needs")
        scale = self._scale(ctIn, "RotateHoisted")
        levelQ, levelP = ctIn.Level(), self.ringP.L - 1
        beta = self.ks.BaseRNSDecompositionVectorSize(levelQ, levelP)
        npoly = ctIn.Value[1].npoly
        buff = (self.ks.buffer("BuffDecompQ", self.ringQ.AtLevel(levelQ), beta * npoly, levelQ + 1),
                self.ks.buffer("BuffDecompP", self.ringP.AtLevel(levelP), beta * npoly, levelP + 1))
        self.ks.DecomposeNTT(levelQ, levelP, ctIn.Value[1], ctIn.IsNTT, buff)
        for i in rotations:
            try:
                self.ks.AutomorphismHoisted(levelQ, ctIn, buff, self.GaloisElement(i), opOut[i])
            except RingHipError as e:
                raise RingHipError("cannot RotateHoisted: %s" % e) from None
            opOut[i].Scale = scale

    def RotateHoistedNew(self, ctIn, rotations):
        """:1233-1240"""
        opOut = {i: self._new(1, ctIn) for i in rotations}
        self.RotateHoisted(ctIn, rotations, opOut)
        return opOut

    def RotateHoistedLazyNew(self, level, rotations, ct, c2DecompQP):
        """:1257-1269: a dict rotation -> rlwe.ElementQP (modulo QP, scaled by P: not yet divided by it) for every rotation other than 0"""
        ks = self._sum_evaluator("RotateHoistedLazyNew")
        cOut = {}
        for i in rotations:
            if i != 0:
                cOut[i] = rlwe.ElementQP.alloc(self.ringQ, self.ringP, ct.Value[0].npoly, level, self.ringP.L - 1)
                try:
                    ks.AutomorphismHoistedLazy(level, ct, c2DecompQP, self.GaloisElement(i), cOut[i])
                except RingHipError as e:
                    raise RingHipError("cannot RotateHoistedLazyNew: %s" % e) from None
        return cOut

    # ---- InnerSum / RotateAndAdd :1271-1317, Replicate (core/rlwe/inner_sum.go:477-479), Trace / Average (linear_transformation.go:13-52) ------------
    def _sum_evaluator(self, who):
        if self.ks is None:
            raise RingHipError("cannot %s: the evaluator was built without ringP, which the key switch needs" % who)
        return self.ks

    def _slots(self, ct):
        """ct.Slots(): 2^LogDimensions, the ring's N / 2 slots when the ciphertext does not say"""
        return 1 << int(getattr(ct, "LogDimensions", self.ringQ.N.bit_length() - 2))

    def InnerSum(self, ctIn, batchSize, n, opOut, fused=None):
        """:1284-1299: the sub-vectors of batchSize slots added together in groups of n; n batchSize must be a power of two and at most the slot
        count (RotateAndAdd takes any).  The scale is ctIn's.  fused: as rlwe.Evaluator.PartialTracesSum."""
        N, l = self._slots(ctIn), int(n) * int(batchSize)
        if n <= 0 or batchSize <= 0:
            raise RingHipError("innersum: invalid parameter (n <= 0 or batchSize <= 0)")
        if l > N:
            raise RingHipError("innersum: invalid parameters (n*batchSize=%d > #slots=%d)" % (l, N))
        if l & (l - 1) != 0:
            raise RingHipError("innersum: invalid parameters (n*batchSize=%d does not divide #slots=%d)" % (l, N))
        self._sum_evaluator("InnerSum").PartialTracesSum(ctIn, batchSize, n, opOut, fused=fused)

    def RotateAndAdd(self, ctIn, batchSize, n, opOut, fused=None):
        """:1314-1317: the sum of ctIn rotated by i batchSize slots, 0 <= i < n"""
        self._sum_evaluator("RotateAndAdd").PartialTracesSum(ctIn, batchSize, n, opOut, fused=fused)

    def Replicate(self, ctIn, batchSize, n, opOut, fused=None):
        self._sum_evaluator("Replicate").Replicate(ctIn, batchSize, n, opOut, fused=fused)

    def Trace(self, ctIn, logSlots, opOut, fused=None):
        self._sum_evaluator("Trace").Trace(ctIn, logSlots, opOut, fused=fused)

    def TraceNew(self, ctIn, logSlots, fused=None):
        """linear_transformation.go:13-16"""
        opOut = self._new(1, ctIn)
        self.Trace(ctIn, logSlots, opOut, fused=fused)
        return opOut

    def Average(self, ctIn, logBatchSize, opOut, fused=None):
        """linear_transformation.go:24-52: every sub-vector of 2^logBatchSize slots replaced by the average of all of them -- a multiplication by
        n^-1 mod q_i, n = slots / 2^logBatchSize, then InnerSum(2^logBatchSize, n) in place on opOut"""
        if ctIn.Degree() != 1 or opOut.Degree() != 1:
            raise RingHipError("cannot Average: ctIn.Degree() != 1 or opOut.Degree() != 1")
        logSlots = int(getattr(ctIn, "LogDimensions", self.ringQ.N.bit_length() - 2))
        if logBatchSize > logSlots:
            raise RingHipError("cannot Average: batchSize must be smaller or equal to the number of slots")
        level = min(ctIn.Level(), opOut.Level())
        rlwe.Evaluator._rows(level, *ctIn.Value, *opOut.Value)
        rq = self.ringQ.AtLevel(level)
        n = 1 << (logSlots - logBatchSize)
        Q = 1
        for q in self._qs(level):
            Q *= q
        for c in (0, 1):
            rq.MulScalarBigint(ctIn.Value[c], pow(n, -1, Q), opOut.Value[c])      # MulScalarMontgomery by MForm(n^-1 mod q_i) (:41-49)
        rlwe.Evaluator._copy_metadata(ctIn, opOut)
        self.InnerSum(opOut, 1 << logBatchSize, n, opOut, fused=fused)


# ---- ckks.Encoder, schemes/ckks/encoder.go: the float64 path (prec <= 53) on standard rings -------------------------------------------------
def GetRootsComplex128(NthRoot):
    """utils.go:53-77 by its rule: one cosine per entry of the first quarter, the rest by symmetry; (NthRoot + 1, 2) float64 (re, im).  The
    cosine is libm's; Go's math.Cos is pure Go and may differ from it in the last place, so a Go caller hands its own table to
    rh_ckks_encoder_create: the device is bit-exact for a GIVEN table."""
    import math
    m = int(NthRoot)
    quarm = m >> 2
    r = np.zeros((m + 1, 2), dtype=np.float64)
    angle = 2 * 3.141592653589793 / float(m)
    for i in range(quarm):
        r[i, 0] = math.cos(angle * float(i))
    for i in range(quarm):
        r[quarm - i, 1] += r[i, 0]
    for i in range(1, quarm + 1):
        r[i + quarm] = (-r[quarm - i, 0], r[quarm - i, 1])
        r[i + 2 * quarm] = (-r[i, 0], -r[i, 1])
        r[i + 3 * quarm] = (r[quarm - i, 0], -r[quarm - i, 1])
    r[m] = r[0]
    return r


class DeviceValues:
    """(nvec, n) complex128 -- or float64 with complex=False -- on the device: the []complex128 / []float64 of a batch of vectors"""

    def __init__(self, ring, nvec, n, complex=True):
        import ctypes as C
        self.ring, self.nvec, self.n, self.complex = ring, int(nvec), int(n), bool(complex)
        self.words = self.nvec * self.n * (2 if complex else 1)
        p = C.c_void_p()
        _check(lib().rh_dev_alloc(ring._h, max(self.words, 1), C.byref(p)))
        self.ptr = int(p.value)

    @classmethod
    def from_numpy(cls, ring, arr):
        arr = np.asarray(arr)
        cplx = np.iscomplexobj(arr)
        arr = np.ascontiguousarray(arr, dtype=np.complex128 if cplx else np.float64)
        if arr.ndim == 1:
            arr = arr[None]
        assert arr.ndim == 2, arr.shape
        v = cls(ring, arr.shape[0], arr.shape[1], cplx)
        if v.words:
            _check(lib().rh_dev_upload(ring._h, v.ptr, _p(arr.view(np.uint64).reshape(-1)), v.words))
        return v

    def numpy(self):
        out = np.empty(self.words, dtype=np.uint64)
        if self.words:
            _check(lib().rh_dev_download(self.ring._h, _p(out), self.ptr, self.words))
        return out.view(np.complex128 if self.complex else np.float64).reshape(self.nvec, self.n)

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
    """rlwe.Plaintext: one poly block (npoly vectors) with its MetaData -- Scale, LogDimensions (the log2 of the slot count; the reference's
    Rows is always 0 for CKKS), IsNTT, IsMontgomery, IsBatched -- carried the way Ciphertext carries Scale"""

    def __init__(self, poly, scale, log_slots, is_ntt=True, is_montgomery=False, is_batched=True):
        Ciphertext.__init__(self, [poly], is_ntt=is_ntt)
        self.Scale = scale if isinstance(scale, Scale) else Scale(scale)
        self.LogDimensions = int(log_slots)
        self.IsMontgomery, self.IsBatched = bool(is_montgomery), bool(is_batched)


class Encoder:
    """ckks.Encoder on device batches: Encode / Decode / DecodePublic / Embed / FFT / IFFT of nvec vectors at once (csrc/ckks_encoder.hip).
    Refused by name: 3N rings, precision > 53 (the *big.Float / *bignum.Complex path), Decode with IsBatched = false at a level that is
    neither 0 nor the ring's top level.
    Conjugate-invariant rings: the real-only embedding (m = 4N roots, up to N real slots; Embed drops the imaginary parts, Decode returns what
    the reference's `isreal` arms and its FFT leave in them), behind the permit conjugate_invariant=True that ckks.NewEncoder(params) sets
    (sampling.rings_ok says why a permit); without it the constructor refuses such a ring in the words of rh_ckks_encoder_create.  On such
    a ring Embed into a PolyQP (ringP) is refused by name."""

    def __init__(self, ringQ, precision=53, roots=None, ringP=None, conjugate_invariant=False):
        """ringP: the key-switch ring, for Embed into an rlwe.PolyQP (the ringqp.Poly arm of embedDouble, encoder.go:304-311: the diagonals of a
        linear transformation); None (default): a PolyQP is refused by name"""
        import ctypes as C
        self.ringQ, self.ringP, self.prec = ringQ, ringP, int(precision)
        self._h = self._hP = None
        if self.prec < 0:
            raise RingHipError("cannot NewEncoder: negative precision")
        self.real = ringQ.kind == ConjugateInvariant and bool(conjugate_invariant)
        if self.real and ringP is not None:
            raise RingHipError("cannot NewEncoder: Embed into a ringqp.Poly (ringP) is built on standard rings only, not on conjugate-invariant rings")
        self.m = (4 if self.real else 2) * ringQ.N
        r = np.ascontiguousarray(GetRootsComplex128(self.m) if roots is None else roots, dtype=np.float64)
        h = C.c_void_p()
        create = lib().rh_ckks_encoder_create_real if self.real else lib().rh_ckks_encoder_create      # the latter refuses a conjugate-invariant ring
        _check(create(C.byref(h), ringQ._h, r.ctypes.data_as(C.POINTER(C.c_double)), r.size // 2, self.prec))
        self._h = h
        if ringP is not None:                                      # the same quantizer and transform over the P moduli
            if ringP.N != ringQ.N or ringP.kind != ringQ.kind:
                raise RingHipError("cannot NewEncoder: ringP must be a ring of ringQ's degree and type")
            hP = C.c_void_p()
            _check(lib().rh_ckks_encoder_create(C.byref(hP), ringP._h, r.ctypes.data_as(C.POINTER(C.c_double)), r.size // 2, self.prec))
            self._hP = hP
        self.LogMaxSlots = ringQ.N.bit_length() - (1 if self.real else 2)
        import threading
        self._tls = threading.local()      # per host thread: the upload blocks host values go through, kept so that no call frees device memory

    def close(self):
        if self._h:
            lib().rh_ckks_encoder_destroy(self._h)
            self._h = None
        if getattr(self, "_hP", None):
            lib().rh_ckks_encoder_destroy(self._hP)
            self._hP = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Prec(self):
        return self.prec

    def reserve(self, nvec):
        _check(lib().rh_ckks_encoder_reserve(self._h, int(nvec)))

    def set_tuning(self, key, value):
        _check(lib().rh_ckks_encoder_set_tuning(self._h, key.encode(), int(value)))

    def NewPlaintext(self, level, scale, nvec=1, log_slots=None, is_ntt=True, is_montgomery=False, is_batched=True):
        return Plaintext(self.ringQ.AtLevel(level).NewPoly(nvec), scale, self.LogMaxSlots if log_slots is None else log_slots,
                         is_ntt, is_montgomery, is_batched)

    # ---- values on their way to the device -----------------------------------------------------------------------------------------------
    def _block(self, values, nvec, slots, who):
        """(nvec, slots) complex block on the device from a slice (one vector, shared by the batch), a (nvec, n) array or a DeviceValues"""
        if isinstance(values, DeviceValues):
            if not values.complex or values.n != slots or values.nvec != nvec:
                raise RingHipError("cannot %s: a device block of values must be complex128 of shape (%d, %d)" % (who, nvec, slots))
            return values
        a = np.asarray(values)
        if a.dtype == object or not (np.issubdtype(a.dtype, np.number)):
            raise RingHipError("cannot %s: values.(Type) must be []complex128 or []float64 ([]*bignum.Complex and []*big.Float stay with the reference), but is %s"
                               % (who, type(values).__name__))
        if a.ndim == 1:
            a = np.broadcast_to(a, (nvec, a.shape[0]))
        if a.ndim != 2 or a.shape[0] != nvec:
            raise RingHipError("cannot %s: %d vectors given for a block of %d polys" % (who, a.shape[0] if a.ndim == 2 else -1, nvec))
        maxCols = 1 << self.LogMaxSlots
        if a.shape[1] > maxCols or a.shape[1] > slots:
            raise RingHipError("cannot %s: ensure that #values (%d) <= slots (%d) <= maxCols (%d)" % (who, a.shape[1], slots, maxCols))
        full = np.zeros((nvec, slots), dtype=np.complex128)                      # zeroes all other values (:292-295)
        full[:, :a.shape[1]] = a
        return self._upload(full)

    def _upload(self, arr):
        """host values -> this thread's upload block of that shape (allocated once).  The copy is ordered on the ring's stream behind the
        calls that still read the block, and nothing is freed, so a call from host values costs the copy and no device-wide synchronisation."""
        cplx = np.iscomplexobj(arr)
        arr = np.ascontiguousarray(arr, dtype=np.complex128 if cplx else np.float64)
        pool = self._tls.__dict__.setdefault("blocks", {})
        key = (arr.shape, cplx)
        dv = pool.get(key)
        if dv is None:
            dv = pool[key] = DeviceValues(self.ringQ, arr.shape[0], arr.shape[1], cplx)
        if dv.words:
            _check(lib().rh_dev_upload(self.ringQ._h, dv.ptr, _p(arr.view(np.uint64).reshape(-1)), dv.words))
        return dv

    def _log_slots(self, log_slots, who):
        if log_slots < 0 or log_slots > self.LogMaxSlots:
            raise RingHipError("cannot %s: logSlots (%d) must be greater or equal to %d and smaller than %d" % (who, log_slots, 0, self.LogMaxSlots))
        return int(log_slots)

    # ---- Encode / Embed (:141-320) -------------------------------------------------------------------------------------------------------
    def Embed(self, values, metadata, polyOut):
        """embedDouble: metadata is anything with Scale, LogDimensions, IsNTT and IsMontgomery (a Plaintext, a Ciphertext given them);
        polyOut a DevicePoly whose limb count sets the level, or an rlwe.PolyQP (the ringqp.Poly arm, :304-311): its Q part is encoded as a
        DevicePoly is, its P part is the same values quantized modulo the P moduli, each part at the level its limb count sets"""
        logs = self._log_slots(metadata.LogDimensions, "Embed")
        scale = metadata.Scale if isinstance(metadata.Scale, Scale) else Scale(metadata.Scale)
        if isinstance(polyOut, rlwe.PolyQP):
            if self._hP is None:
                raise RingHipError("cannot Embed: polyOut is a ringqp.Poly but the encoder was built without ringP (Encoder(ringQ, ringP=...))")
            if polyOut.Q.npoly != polyOut.P.npoly:
                raise RingHipError("cannot Embed: the Q and P parts of polyOut hold different numbers of polys")
            block = self._block(values, polyOut.Q.npoly, 1 << logs, "Embed")
            ntt, mont = 1 if metadata.IsNTT else 0, 1 if getattr(metadata, "IsMontgomery", False) else 0
            for h, part in ((self._h, polyOut.Q), (self._hP, polyOut.P)):
                _check(lib().rh_ckks_encode(h, part.limbs - 1, logs, scale.Float64(), block.ptr, part.npoly, part.ptr, ntt, mont))
            return
        block = self._block(values, polyOut.npoly, 1 << logs, "Embed")
        _check(lib().rh_ckks_encode(self._h, polyOut.limbs - 1, logs, scale.Float64(), block.ptr, polyOut.npoly, polyOut.ptr,
                                    1 if metadata.IsNTT else 0, 1 if getattr(metadata, "IsMontgomery", False) else 0))

    def Encode(self, values, pt):
        if pt.IsBatched:
            return self.Embed(values, pt, pt.Value[0])
        p = pt.Value[0]
        if isinstance(values, DeviceValues):
            if values.complex or values.nvec != p.npoly:
                raise RingHipError("cannot Encode: supported values.(type) for IsBatched=False is []float64")
            dv = values
        else:
            a = np.asarray(values)
            if np.iscomplexobj(a) or a.dtype == object:
                raise RingHipError("cannot Encode: supported values.(type) for IsBatched=False is []float64 or []*big.Float, but %s was given" % a.dtype)
            if a.ndim == 1:
                a = np.broadcast_to(a, (p.npoly, a.shape[0]))
            if a.shape[-1] > self.ringQ.N:
                raise RingHipError("cannot Encode: maximum number of values is %d but len(values) is %d" % (self.ringQ.N, a.shape[-1]))
            dv = self._upload(np.ascontiguousarray(a, dtype=np.float64).reshape(p.npoly, -1))
        _check(lib().rh_ckks_encode_coeffs(self._h, p.limbs - 1, pt.Scale.Float64(), dv.ptr, dv.n, p.npoly, p.ptr, 1 if pt.IsNTT else 0))

    # ---- Decode (:177-186, :476-575) -------------------------------------------------------------------------------------------------------
    def DecodePublic(self, pt, values=None, logprec=0):
        """values: None (a new (nvec, slots) complex128 array is returned), a numpy array of dtype complex128 or float64 -- (nvec, k), or (k,)
        for a single vector -- filled with up to slots values per vector (the real parts for float64) and returned, or a complex
        DeviceValues of shape (nvec, slots), filled on the device.  IsBatched = false (plaintextToFloat, :467-472): the N coefficients
        over the scale, real; values None (a new (nvec, N) float64 array), a numpy array as above, or a float64 DeviceValues of shape
        (nvec, N); level 0 and the ring's top level only (csrc/ckks_encoder.hip says why), and logprec is not used (:731)."""
        batched = bool(pt.IsBatched)
        logs = self._log_slots(pt.LogDimensions, "Decode")
        p = pt.Value[0]
        cols = 1 << logs if batched else self.ringQ.N
        on_dev = isinstance(values, DeviceValues)
        real = values is not None and not on_dev and not np.iscomplexobj(values)
        if on_dev and (values.complex != batched or values.n != cols or values.nvec != p.npoly):
            raise RingHipError("cannot Decode: a device block of values must be %s of shape (%d, %d)" % ("complex128" if batched else "float64", p.npoly, cols))
        if values is not None and not on_dev:
            if not isinstance(values, np.ndarray) or values.dtype not in (np.float64, np.complex128):
                raise RingHipError("cannot decode: values.(type) accepted are []complex128 and []float64 (numpy arrays), but is %s" % type(values).__name__)
            if not (values.ndim == 2 and values.shape[0] == p.npoly) and not (values.ndim == 1 and p.npoly == 1):
                raise RingHipError("cannot Decode: values of shape %s for a plaintext block of %d vectors: give (%d, k)" % (values.shape, p.npoly, p.npoly))
        dv = values if on_dev else self._tls.__dict__.setdefault("blocks", {}).get(((p.npoly, cols), batched))
        if dv is None:
            dv = self._tls.blocks[((p.npoly, cols), batched)] = DeviceValues(self.ringQ, p.npoly, cols, batched)
        _check(lib().rh_ckks_decode(self._h, p.limbs - 1, logs if batched else 0, pt.Scale.Float64(), float(logprec), 1 if pt.IsNTT else 0,
                                    1 if batched else 0, 1 if real else 0, p.ptr, p.npoly, dv.ptr))
        if on_dev:
            return values
        got = dv.numpy()
        if values is None:
            return got
        k = min(values.shape[-1], cols)
        values.reshape(p.npoly, -1)[:, :k] = (got.real if real or not batched else got)[:, :k]
        return values

    def Decode(self, pt, values=None):
        return self.DecodePublic(pt, values, 0)

    # ---- the transforms alone (:738-793) -----------------------------------------------------------------------------------------------
    def _transform(self, values, logN, fn, who):
        logN = self._log_slots(int(logN), who)
        if isinstance(values, DeviceValues):
            if not values.complex or values.n != 1 << logN:
                raise RingHipError("cannot %s: a device block of values must be complex128 with %d columns" % (who, 1 << logN))
            _check(fn(self._h, values.ptr, logN, values.nvec))
            return values
        a = np.asarray(values, dtype=np.complex128)
        if a.shape[-1] != 1 << logN:
            raise RingHipError("cannot %s: %d values for logN = %d" % (who, a.shape[-1], logN))
        dv = self._upload(a.reshape(-1, a.shape[-1]))
        _check(fn(self._h, dv.ptr, logN, dv.nvec))
        return dv.numpy().reshape(a.shape)

    def IFFT(self, values, logN):
        return self._transform(values, logN, lib().rh_ckks_special_ifft, "IFFT")

    def FFT(self, values, logN):
        return self._transform(values, logN, lib().rh_ckks_special_fft, "FFT")


# ---- ckks.NewEncryptor / NewDecryptor (schemes/ckks/ckks.go): rlwe's, carrying the Plaintext metadata ------------------------------------------------
class Encryptor(rlwe.Encryptor):
    """ckks.Encryptor: rlwe.Encryptor on ckks.Plaintext batches; the ciphertext takes the plaintext's Scale, LogDimensions and IsBatched"""


class Decryptor(rlwe.Decryptor):
    """ckks.Decryptor: rlwe.Decryptor; DecryptNew returns a ckks.Plaintext with the ciphertext's Scale, LogDimensions and IsBatched"""

    def DecryptNew(self, ct, fused=None):
        poly = self.ringQ.AtLevel(ct.Level()).NewPoly(ct.Value[0].npoly)
        pt = Plaintext(poly, ct.Scale, ct.LogDimensions, ct.IsNTT, getattr(ct, "IsMontgomery", False), getattr(ct, "IsBatched", True))
        self.Decrypt(ct, pt, fused)
        return pt


# ---- ckks.Parameters (schemes/ckks/params.go) and the constructors that take them (schemes/ckks/ckks.go) ---------------------------------------
class Parameters:
    """ckks.Parameters with explicit moduli (no prime generation): ringQ / ringP = Ring(2^LogN, ., kind=RingType).  RingType: Standard or
    ConjugateInvariant; Xs: ("P", density) or ("H", weight); Xe: (sigma, bound).  The New* factories below are how a conjugate-invariant ring
    reaches the key layer and the encoder: they pass the permit conjugate_invariant=True (sampling.rings_ok)."""

    def __init__(self, LogN, Q, P, LogDefaultScale, RingType=Standard, Xs=("P", 2 / 3), Xe=(3.2, 19), device=0):
        if RingType not in (Standard, ConjugateInvariant):
            raise RingHipError("cannot NewParameters: RingType must be Standard or ConjugateInvariant")
        self.logN, self.ringType, self.device = int(LogN), RingType, device
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in (P or [])]
        nth = self.NthRoot()
        for q in self.Q + self.P:
            if q % nth != 1:
                raise RingHipError("cannot NewParameters: modulus %d is not 1 mod NthRoot = %d" % (q, nth))
        n = 1 << self.logN
        self.ringQ = Ring(n, self.Q, kind=RingType, device=device)
        self.ringP = Ring(n, self.P, kind=RingType, device=device) if self.P else None
        self.logDefaultScale = int(LogDefaultScale)
        self.scale = Scale(1 << self.logDefaultScale)
        self.xs, self.xe = tuple(Xs), tuple(Xe)

    def N(self): return 1 << self.logN
    def LogN(self): return self.logN
    def MaxLevel(self): return len(self.Q) - 1
    def MaxLevelQ(self): return len(self.Q) - 1
    def MaxLevelP(self): return len(self.P) - 1
    def RingQ(self): return self.ringQ
    def RingP(self): return self.ringP
    def RingType(self): return self.ringType
    def NthRoot(self): return (4 if self.ringType == ConjugateInvariant else 2) << self.logN       # ring/ring.go:178-183
    def DefaultScale(self): return self.scale
    def LogDefaultScale(self): return self.logDefaultScale
    def LogMaxSlots(self): return self.logN if self.ringType == ConjugateInvariant else self.logN - 1
    def MaxSlots(self): return 1 << self.LogMaxSlots()                                # params.go:138-177: Cols = N, or N / 2 on a standard ring
    def LogMaxDimensions(self): return (0, self.LogMaxSlots())                        # ring.Dimensions{Rows, Cols}
    def MaxDimensions(self): return (1, self.MaxSlots())
    def GaloisElement(self, k): return GaloisElement(self.N(), k, self.NthRoot())
    def EncodingPrecision(self): return max(53, self.logDefaultScale)                 # params.go:187-195
    def Xs(self): return self.xs
    def Xe(self): return self.xe
    def _ci(self): return self.ringType == ConjugateInvariant

    def StandardParameters(self, P=None):
        """params.go:103-113 over core/rlwe/params.go StandardParameters: the receiver when it is standard; else the standard parameters of
        twice the degree (the same NthRoot) with the same Q and P.  P=...: other auxiliary moduli for the standard side."""
        if self.ringType == Standard and P is None:
            return self
        logN = self.logN + (1 if self.ringType == ConjugateInvariant else 0)
        return Parameters(logN, self.Q, self.P if P is None else P, self.logDefaultScale, Standard, self.xs, self.xe, self.device)

    def close(self):
        for r in (self.ringQ, self.ringP):
            if r is not None:
                r.close()


def NewKeyGenerator(params, prng=None):
    return rlwe.KeyGenerator(params.RingQ(), params.RingP(), params.Xs(), params.Xe(), prng, conjugate_invariant=params._ci())


def NewEncoder(params, precision=None, roots=None):
    """ckks.NewEncoder: precision None is Parameters.EncodingPrecision()"""
    return Encoder(params.RingQ(), params.EncodingPrecision() if precision is None else precision, roots,
                   None if params._ci() else params.RingP(), conjugate_invariant=params._ci())


def NewEncryptor(params, key, prng=None):
    return Encryptor(params.RingQ(), params.RingP(), key, prng, params.Xs(), params.Xe(), conjugate_invariant=params._ci())


def NewDecryptor(params, sk):
    return Decryptor(params.RingQ(), sk, conjugate_invariant=params._ci())


def NewEvaluator(params, evk=None, **kw):
    """evk: a MemEvaluationKeySet (or None)"""
    gks = dict(evk.GaloisKeys) if evk is not None else None
    return Evaluator(params.RingQ(), params.RingP(), rlk=evk.RelinearizationKey if evk is not None else None, galois_keys=gks,
                     encoding_precision=params.EncodingPrecision(), **kw)


def NewPlaintext(params, level, nvec=1, log_slots=None, is_ntt=True):
    """ckks.NewPlaintext (ckks.go): the default scale and the maximum dimensions"""
    return Plaintext(params.RingQ().AtLevel(level).NewPoly(nvec), params.DefaultScale(), params.LogMaxSlots() if log_slots is None else log_slots, is_ntt)


def NewCiphertext(params, degree, level, nvec=1, is_ntt=True):
    rq = params.RingQ().AtLevel(level)
    ct = Ciphertext([rq.NewPoly(nvec) for _ in range(degree + 1)], is_ntt=is_ntt)
    ct.Scale, ct.LogDimensions, ct.IsBatched, ct.IsMontgomery = params.DefaultScale(), params.LogMaxSlots(), True, False
    return ct


# ---- ckks.DomainSwitcher (schemes/ckks/bridge.go) ---------------------------------------------------------------------------------------------------
# "fold_tail": the tail of ComplexToReal -- rh_ckks_bridge_fold_tail (True) or the reference's Add and two FoldStandardToConjugateInvariant
# calls (False); "unfold_then_add": RealToComplex -- GadgetProductThenAdd with the unfolded c0 as addend (True) or GadgetProduct, Add, CopyLvl
# (False; also what keys with at most one modulus of P and coefficient-domain ciphertexts take).  The same bits.  profiles/ci_ckks.json
# (n = 2^16, 25 + 5 limbs, call rates): the tail alone 1.84x (batch 1) and 1.53x (batch 8) faster in one launch, a whole ComplexToReal 1.9 % and
# 2.3 %, a whole RealToComplex 0.6 % and 4.0 %, each outside the spread of its windows: both default to the fused side.
FUSED_BRIDGE = {"fold_tail": True, "unfold_then_add": True}


class DomainSwitcher:
    """ckks.DomainSwitcher on batches of ciphertexts: ComplexToReal / RealToComplex between the standard ring of degree 2n and the
    conjugate-invariant ring of degree n.  params: parameters of either type (its RingQ's degree and moduli fix both rings); the keys are
    those of KeyGenerator.GenEvaluationKeysForRingSwapNew.  The level is min(ctIn.Level(), opOut.Level()): a ctIn above it is read at that
    level; an opOut above it is refused by name (a device batch cannot be resized)."""

    def __init__(self, params, complexToRealEvk=None, realToComplexEvk=None):
        self.stdToci, self.ciToStd = complexToRealEvk, realToComplexEvk
        rq = params.RingQ()
        ci = params.RingType() == ConjugateInvariant
        n = rq.N if ci else rq.N // 2
        self._own = []
        mods = [int(q) for q in rq.moduli]
        for q in mods:
            if q % (4 * n) != 1:
                raise RingHipError("cannot NewDomainSwitcher because the standard NTT is undefined for params: modulus %d is not 1 mod %d" % (q, 4 * n))
        if ci:
            self.conjugateRingQ = rq
            self.stdRingQ = Ring(2 * n, mods, kind=Standard, device=params.device)
            self._own.append(self.stdRingQ)
        else:
            self.stdRingQ = rq
            self.conjugateRingQ = Ring(n, mods, kind=ConjugateInvariant, device=params.device)
            self._own.append(self.conjugateRingQ)
        N = self.stdRingQ.N
        self.automorphismIndex = AutomorphismNTTIndex(N, 2 * N, 2 * N - 1)
        self._index = DevicePoly.from_numpy(self.conjugateRingQ.AtLevel(0), _u64(self.automorphismIndex).reshape(-1)[:n].reshape(1, 1, n))
        self._pool = {}
        self._ks_own = None

    def close(self):
        self._pool.clear()
        if self._ks_own is not None:
            self._ks_own.close()
            self._ks_own = None
        for r in self._own:
            r.close()
        self._own = []

    def _ks(self, eval, key, who):
        """the key-switch evaluator: the ckks.Evaluator's, or one of the switcher's own over ringQ alone for keys without P.  The device gadget
        product strides a key by the limb counts of the evaluator's rings (rlwe.GadgetCiphertext), so a key made at lower levels is refused."""
        ks = eval.ks
        if ks is None:
            if self._ks_own is None:
                self._ks_own = rlwe.Evaluator(eval.ringQ, None)
            ks = self._ks_own
        have = (ks.ringQ.L - 1, ks.ringP.L - 1 if ks.ringP is not None else -1)
        if (key.LevelQ(), key.LevelP()) != have:
            raise RingHipError("cannot %s: the key is made at levels (Q %d, P %d) but the evaluator's rings hold levels (Q %d, P %d): build the "
                               "evaluator over rings of the key's limb counts" % ((who, key.LevelQ(), key.LevelP()) + have))
        return ks

    def _buf(self, tag, ring, npoly, limbs):
        key = (tag, id(ring._h), npoly, limbs)
        p = self._pool.get(key)
        if p is None:
            p = self._pool[key] = DevicePoly(ring, npoly, limbs)
        return p

    def _at_level(self, tag, ring, p, level):
        """a block read at `level`: itself, a view of a single poly's leading limbs, or a copy of a batch's"""
        if p.limbs == level + 1:
            return p
        if p.npoly == 1:
            return DevicePoly(ring, 1, level + 1, ptr=p.ptr, owner=p)
        out = self._buf(tag, ring, p.npoly, level + 1)
        ring.CopyLvl(p, out)
        return out

    def _enter(self, who, eval, ctIn, opOut):
        if eval.ringQ.kind != Standard:
            raise RingHipError("cannot %s: provided evaluator is not instantiated with RingType ring.Standard" % who)
        to_real = who == "ComplexToReal"
        big, small = (ctIn, opOut) if to_real else (opOut, ctIn)
        if big.Value[0].ring.N != 2 * small.Value[0].ring.N:
            raise RingHipError("cannot %s: %s" % (who, "ctIn ring degree must be twice opOut ring degree" if to_real
                                                  else "opOut ring degree must be twice ctIn ring degree"))
        level = min(ctIn.Level(), opOut.Level())
        if opOut.Level() != level:
            raise RingHipError("cannot %s: opOut is allocated at level %d above the level %d of the switch: a device batch cannot be resized, "
                               "allocate opOut at ctIn's level or below" % (who, opOut.Level(), level))
        if opOut.Degree() != 1 or ctIn.Degree() != 1 or opOut.Value[0].npoly != ctIn.Value[0].npoly:
            raise RingHipError("cannot %s: ciphertexts of degree 1 and the same batch size" % who)
        return level

    @staticmethod
    def _meta(ctIn, opOut, scale):
        for name in ("LogDimensions", "IsBatched", "IsMontgomery"):
            if hasattr(ctIn, name):
                setattr(opOut, name, getattr(ctIn, name))
        opOut.IsNTT, opOut.Scale = ctIn.IsNTT, scale

    def ComplexToReal(self, eval, ctIn, opOut, fused=None):
        """(:55-87): enc(real(m) + i imag(m)) on the standard ring -> enc(2 real(m)) read at twice the scale on the conjugate-invariant ring"""
        who = "ComplexToReal"
        level = self._enter(who, eval, ctIn, opOut)
        if self.stdToci is None:
            raise RingHipError("cannot ComplexToReal: no realToComplexEvk provided to this DomainSwitcher")
        rs, rc = self.stdRingQ.AtLevel(level), self.conjugateRingQ.AtLevel(level)
        npoly = ctIn.Value[0].npoly
        c0, c1 = (self._at_level(("in", c), rs, ctIn.Value[c], level) for c in (0, 1))
        tmp = Ciphertext([self._buf(("g", c), rs, npoly, level + 1) for c in (0, 1)], is_ntt=ctIn.IsNTT)
        self._ks(eval, self.stdToci, who).GadgetProduct(level, c1, self.stdToci, tmp)
        if FUSED_BRIDGE["fold_tail"] if fused is None else fused:
            _check(lib().rh_ckks_bridge_fold_tail(rc._h, level, tmp.Value[0].ptr, tmp.Value[1].ptr, c0.ptr, self._index.ptr,
                                                  opOut.Value[0].ptr, opOut.Value[1].ptr, npoly))
        else:
            rs.Add(tmp.Value[0], c0, tmp.Value[0])
            rc.FoldStandardToConjugateInvariant(tmp.Value[0], self._index, opOut.Value[0])
            rc.FoldStandardToConjugateInvariant(tmp.Value[1], self._index, opOut.Value[1])
        s = ctIn.Scale if isinstance(ctIn.Scale, Scale) else Scale(ctIn.Scale)
        self._meta(ctIn, opOut, s.Mul(Scale(2)))

    def RealToComplex(self, eval, ctIn, opOut, fused=None):
        """(:96-129): enc(real(m)) on the conjugate-invariant ring -> enc(real(m) + 0 i) on the standard ring"""
        who = "RealToComplex"
        level = self._enter(who, eval, ctIn, opOut)
        if self.ciToStd is None:
            raise RingHipError("cannot RealToComplex: no realToComplexEvk provided to this DomainSwitcher")
        rs, rc = self.stdRingQ.AtLevel(level), self.conjugateRingQ.AtLevel(level)
        npoly = ctIn.Value[0].npoly
        c0, c1 = (self._at_level(("in", c), rc, ctIn.Value[c], level) for c in (0, 1))
        key = self.ciToStd
        fuse = FUSED_BRIDGE["unfold_then_add"] if fused is None else fused
        if fuse and key.LevelP() >= 1 and ctIn.IsNTT:
            both = self._buf("u", rs, 2 * npoly, level + 1)                     # one unfold over both components
            if c1.ptr == c0.ptr + c0.words * 8:
                src = DevicePoly(rc, 2 * npoly, level + 1, ptr=c0.ptr, owner=c0)
                rs.UnfoldConjugateInvariantToStandard(src, both)
            else:
                for c, v in enumerate((c0, c1)):
                    rs.UnfoldConjugateInvariantToStandard(v, DevicePoly(rs, npoly, level + 1, ptr=both.ptr + c * npoly * (level + 1) * rs.N * 8, owner=both))
            u0 = DevicePoly(rs, npoly, level + 1, ptr=both.ptr, owner=both)
            u1 = DevicePoly(rs, npoly, level + 1, ptr=both.ptr + npoly * (level + 1) * rs.N * 8, owner=both)
            self._ks(eval, key, who).GadgetProductThenAdd(level, u1, key, u0, None, opOut)
        else:
            rs.UnfoldConjugateInvariantToStandard(c0, opOut.Value[0])
            rs.UnfoldConjugateInvariantToStandard(c1, opOut.Value[1])
            tmp = Ciphertext([self._buf(("g", c), rs, npoly, level + 1) for c in (0, 1)], is_ntt=ctIn.IsNTT)
            self._ks(eval, key, who).GadgetProduct(level, opOut.Value[1], key, tmp)
            rs.Add(opOut.Value[0], tmp.Value[0], opOut.Value[0])
            rs.CopyLvl(tmp.Value[1], opOut.Value[1])
        self._meta(ctIn, opOut, ctIn.Scale if isinstance(ctIn.Scale, Scale) else Scale(ctIn.Scale))

    def ComplexToRealNew(self, eval, ctIn, fused=None):
        rc = self.conjugateRingQ.AtLevel(min(ctIn.Level(), self.stdToci.LevelQ() if self.stdToci is not None else ctIn.Level()))
        out = Ciphertext([rc.NewPoly(ctIn.Value[0].npoly) for _ in (0, 1)], is_ntt=ctIn.IsNTT)
        self.ComplexToReal(eval, ctIn, out, fused)
        return out

    def RealToComplexNew(self, eval, ctIn, fused=None):
        rs = self.stdRingQ.AtLevel(min(ctIn.Level(), self.ciToStd.LevelQ() if self.ciToStd is not None else ctIn.Level()))
        out = Ciphertext([rs.NewPoly(ctIn.Value[0].npoly) for _ in (0, 1)], is_ntt=ctIn.IsNTT)
        self.RealToComplex(eval, ctIn, out, fused)
        return out


def NewDomainSwitcher(params, complexToRealEvk=None, realToComplexEvk=None):
    return DomainSwitcher(params, complexToRealEvk, realToComplexEvk)


# ---- ckks.GetPrecisionStats (schemes/ckks/precision.go): host statistics over the device Decode (precision.py) -------------------------------------------
from .precision import GetPrecisionStats, PrecisionStats, Stats  # noqa: E402,F401

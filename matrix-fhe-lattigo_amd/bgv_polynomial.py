"""Host-side mirror of the reference's polynomial evaluation circuit for BGV / BFV on device-resident batches: the Paterson-Stockmeyer
recursion, the power basis and the scale bookkeeping modulo T; the arithmetic is the device evaluator's (bgv.Evaluator) and, for a baby step,
one launch of rh_ckks_linear_combination (a polynomial: the scalars are the same on both halves of a row) or of rh_bgv_plain_combination
(a PolynomialVector with a mapping; csrc/bgv.hip).

  circuits/bgv/polynomial/polynomial.go                    NewPolynomial :14-16   PolynomialVector, Depth :19-36
  circuits/bgv/polynomial/polynomial_evaluator.go          NewEvaluator :18-29    Evaluate :40-53   EvaluateFromPowerBasis :58-76
                                                           CoefficientGetter :80-106
  circuits/bgv/polynomial/polynomial_evaluator_sim.go      simEvaluator :25-104, both arms (standard and scale-invariant tensoring)
  circuits/common/polynomial/{polynomial,power_basis,polynomial_evaluator,polynomial_evaluator_sim}.go   as polynomial.py lists them

What does not depend on the scheme is polynomial.py's: OptimalSplit, SplitDegree, recursePS with its SimOperand / SimPowerBasis, the
Paterson-Stockmeyer containers, CopyNew, and the call of rh_ckks_linear_combination.  Nothing of the CKKS classes changes.

A batch of npoly ciphertexts is one Ciphertext (schemes.py); all of them share the level and the scale, an int modulo T as bgv.Evaluator carries
it.  Where the reference reads an operand at a lower level than it was allocated for (ring.AtLevel), the device path copies its leading limbs:
the same values.

Refused by name: a basis other than Monomial (the reference's BGV package never builds one, and Chebyshev constants have no meaning modulo T),
polynomials with Lazy = True (the power basis then holds powers of mixed degrees, and the reference's MulThenAdd drops the accumulator's third
component when a relinearised power follows a lazy one: opOut.Resize(op0.Degree(), ...), schemes/bgv/evaluator.go:1170 -- there is nothing sound
to match; PowerBasis.GenPower(lazy=True) itself is supported), a mapping on an evaluator without an encoder, conjugate-invariant and 3N rings.
BGV linear transformations are bgv_lintrans.py."""
import ctypes as C
import math
import types

import numpy as np

from .ckks import ScalePrecision
from .bgv import MulScaleInvariant
from .polynomial import (BabyStep, InDelta, Monomial, OptimalSplit, PatersonStockmeyerPolynomial, PatersonStockmeyerPolynomialVector,  # noqa: F401
                         PolynomialEvaluator, SimOperand, SimPowerBasis, SplitDegree, _copy_new, recursePS)
from .ringhip import DevicePoly, RingHipError, Standard, _check, _p, _u64, lib
from .schemes import Ciphertext

# The baby step as ONE launch (rh_ckks_linear_combination for a polynomial, rh_bgv_plain_combination for a mapping), or as the reference's own
# Add and MulThenAdd calls through bgv.Evaluator: the same bits.  profiles/bgv_polynomial.json (tools/bench_bgv_polynomial.py,
# "fused_bgv_polynomial_default"): an arm is fused by default only if at EVERY shape timed (N = 2^15, 2^16; batches of 1 and 8) the median of a
# whole Evaluate beats the composed one by more than the run-to-run spread.  Neither arm meets that, so both are composed by default.  Scalar:
# fused is 1.12 to 1.51 times faster at every shape (the baby steps alone 2.0 to 3.9 times), but at batch 8 the windows of BOTH sides spread by
# more than the difference (8.4 ms on 24.6 | 32.4 ms at N = 2^15, 44 ms on 50.2 | 76.0 ms at N = 2^16: the first window of a side runs about twice
# as fast as its later ones).  Vector: 1.18 to 1.23 times faster from N = 2^15, batch 8 up (baby steps 1.8 to 2.1 times), but 3 % SLOWER at
# N = 2^15, batch 1 (8.92 | 8.65 ms, beyond the 0.28 ms spread), and the N = 2^16, batch 8 windows spread like the scalar ones.  Evaluator(ev,
# fused=True) takes the kernels where the shapes are known to be large.
FUSED_BGV_POLYNOMIAL = {"scalar": False, "vector": False}

LC_MODULUS_BITS = 61                  # lc_reduce.hip.hpp: the one-launch sums need every modulus below 2^61 (checked per call by both entries)


def _basis(basis):
    if basis != Monomial:
        raise RingHipError("invalid basis type for a BGV polynomial: only `Monomial` is built (the reference's bgv package builds no other, "
                           "and Chebyshev constants have no meaning modulo T), but is %r" % (basis,))


class Polynomial:
    """bgv polynomial.Polynomial (NewPolynomial :14-16): Coeffs are Python ints (None: a nil coefficient, which Factorize may leave), taken
    modulo T where they are used; the Monomial basis.  IsOdd and IsEven are fields, both true from the constructor as in the reference
    (bignum/polynomial.go:104-111), never inferred."""

    def __init__(self, coeffs, basis=Monomial):
        _basis(basis)
        self.Basis = basis
        self.Coeffs = [None if c is None else int(c) for c in coeffs]
        if not self.Coeffs:
            raise RingHipError("cannot NewPolynomial: no coefficients")
        self.IsOdd = self.IsEven = True
        self.MaxDeg, self.Lead, self.Lazy = len(self.Coeffs) - 1, True, False      # polynomial.NewPolynomial :28-35
        self.Level, self.Scale = 0, None

    @classmethod
    def _raw(cls, like, coeffs):
        p = object.__new__(cls)
        p.Basis, p.Coeffs, p.IsOdd, p.IsEven = like.Basis, coeffs, like.IsOdd, like.IsEven
        p.MaxDeg, p.Lead, p.Lazy, p.Level, p.Scale = 0, False, False, 0, None     # the zero value of polynomial.Polynomial
        return p

    def Degree(self):
        return len(self.Coeffs) - 1

    def Depth(self):
        return int(math.ceil(math.log2(float(self.Degree()))))

    def Evaluate(self, x, t):
        """the value at x modulo t (Horner): what a decrypted slot is compared with"""
        y = 0
        for c in reversed(self.Coeffs):
            y = (y * int(x) + (0 if c is None else c)) % int(t)
        return y

    def Factorize(self, n):
        """p = X^n pq + pr: bignum/polynomial.go:258-314 (Monomial) with the fields of polynomial.Polynomial.Factorize :38-58"""
        if n < self.Degree() >> 1:
            raise RingHipError("cannot Factorize: n < p.Degree()/2")
        deg = self.Degree()
        pr = list(self.Coeffs[:n])
        pq = [None] * (deg - n + 1)
        pq[0] = self.Coeffs[n]
        even, odd = self.IsEven, self.IsOdd
        for i in range(n + 1, deg + 1):
            c = self.Coeffs[i]
            if c is not None and (not (even or odd) or (i & 1 == 0 and even) or (i & 1 == 1 and odd)):
                pq[i - n] = c
        q, r = Polynomial._raw(self, pq), Polynomial._raw(self, pr)
        q.MaxDeg = self.MaxDeg
        r.MaxDeg = n - 1 if self.MaxDeg == deg else self.MaxDeg - (deg - n + 1)
        q.Lead = bool(self.Lead)
        return q, r

    def PatersonStockmeyerPolynomial(self, sim, inputLevel, inputScale, outputScale):
        """polynomial.go:74-106; sim: a SimEvaluator.  The recursion is polynomial.py's recursePS: it takes levels and scales from the simulator alone"""
        logDegree = self.Degree().bit_length()
        logSplit = OptimalSplit(logDegree)
        pb = SimPowerBasis()
        pb[1] = SimOperand(inputLevel, int(inputScale) % sim.T)
        pb.GenPower(1 << logDegree, sim)
        for i in range((1 << logSplit) - 1, 2, -1):
            pb.GenPower(i, sim)
        value, _ = recursePS(logSplit, inputLevel - sim.PolynomialDepth(self.Degree()), self, pb, int(outputScale) % sim.T, sim)
        return PatersonStockmeyerPolynomial(self.Degree(), 1 << logSplit, inputLevel, int(outputScale) % sim.T, value)


class PolynomialVector:
    """polynomial.go:159-229 with the BGV wrapper's Depth (circuits/bgv/polynomial/polynomial.go:22-24): polynomials of one degree, and
    mapping[i] = the slots polynomial i is evaluated on; slots no polynomial names evaluate to zero"""

    def __init__(self, polys, mapping=None):
        polys = [p if isinstance(p, Polynomial) else Polynomial(p) for p in polys]
        if not polys:
            raise RingHipError("cannot NewPolynomialVector: no polynomials")
        if len({p.Degree() for p in polys}) > 1:
            raise RingHipError("polynomial degree must all be the same")
        self.Value = polys
        self.Mapping = None if mapping is None else {int(k): [int(j) for j in v] for k, v in mapping.items()}
        self._index = {}                                                           # slots -> the mapping as index arrays: made once, shared by
                                                                                   # the vectors Factorize and the baby steps derive from this one

    @classmethod
    def _derived(cls, polys, mapping, index):
        """the vector of other polynomials over a mapping that has been through the constructor"""
        v = object.__new__(cls)
        v.Value, v.Mapping, v._index = list(polys), mapping, {} if index is None else index
        return v

    def IsEven(self):
        return all(p.IsEven for p in self.Value)

    def IsOdd(self):
        return all(p.IsOdd for p in self.Value)

    def Depth(self):
        return self.Value[0].Depth()

    def Factorize(self, n):
        qs, rs = zip(*[p.Factorize(n) for p in self.Value])
        return PolynomialVector._derived(qs, self.Mapping, self._index), PolynomialVector._derived(rs, self.Mapping, self._index)

    def slot_index(self, slots):
        """polynomial i -> its slots as an index array, every slot inside [0, slots)"""
        if slots not in self._index:
            index = {i: np.asarray(v, dtype=np.int64) for i, v in self.Mapping.items()}
            for i, v in index.items():
                if v.size and (v.min() < 0 or v.max() >= slots):
                    raise RingHipError("cannot GetVectorCoefficient: a mapped slot of polynomial %d is outside [0, %d)" % (i, slots))
            self._index[slots] = index
        return self._index[slots]

    def PatersonStockmeyerPolynomial(self, sim, inputLevel, inputScale, outputScale):
        """polynomial.go:241-251"""
        ps = PatersonStockmeyerPolynomialVector([p.PatersonStockmeyerPolynomial(sim, inputLevel, inputScale, outputScale) for p in self.Value], self.Mapping)
        ps._index = self._index
        return ps


# ---- the simulator: levels and scales alone -------------------------------------------------------------------------------------------------
class SimEvaluator:
    """circuits/bgv/polynomial/polynomial_evaluator_sim.go:25-104.  Q: the moduli chain, T the plaintext modulus; scales are ints modulo T
    (rlwe.Scale with Mod = T: Mul and Div reduce modulo T, Div by the modular inverse, core/rlwe/scale.go:77-119)"""

    def __init__(self, Q, T, InvariantTensoring=False):
        self.Q, self.T, self.InvariantTensoring = [int(q) for q in Q], int(T), bool(InvariantTensoring)

    def _div(self, a, b):
        try:
            return int(a) * pow(int(b) % self.T, -1, self.T) % self.T
        except ValueError:
            raise RingHipError("cannot divide a scale by %d: no inverse modulo T = %d" % (b, self.T)) from None

    def _Qlevel(self, level):
        return math.prod(self.Q[:level + 1])

    def PolynomialDepth(self, degree):
        if self.InvariantTensoring:
            return 0                                                               # (:26-28)
        if degree <= 0:
            raise RingHipError("invalid degree: degree=%d should be greater than zero" % degree)
        return degree.bit_length() - 1                                             # (:34)

    def Rescale(self, op0):
        if not self.InvariantTensoring:                                            # (:38-43)
            op0.Scale = self._div(op0.Scale, self.Q[op0.Level])
            op0.Level -= 1

    def MulNew(self, op0, op1):
        level = min(op0.Level, op1.Level)                                          # (:46-57)
        if self.InvariantTensoring:
            return SimOperand(level, MulScaleInvariant(self.T, self._Qlevel(level), op0.Scale, op1.Scale))
        return SimOperand(level, int(op0.Scale) * int(op1.Scale) % self.T)

    def UpdateLevelAndScaleBabyStep(self, lead, tLevelOld, tScaleOld):
        tScaleNew = int(tScaleOld) % self.T                                        # (:60-67)
        if not self.InvariantTensoring and lead:
            tScaleNew = tScaleNew * self.Q[tLevelOld] % self.T
        return tLevelOld, tScaleNew

    def UpdateLevelAndScaleGiantStep(self, lead, tLevelOld, tScaleOld, xPowScale):
        tScaleNew = self._div(tScaleOld, xPowScale)                                # (:75)
        if not self.InvariantTensoring:
            currentQi = self.Q[tLevelOld] if lead else self.Q[tLevelOld + 1]       # (:80-87)
            return tLevelOld + 1, tScaleNew * currentQi % self.T
        qModTNeg = self.T - self._Qlevel(tLevelOld) % self.T                       # (:91-96)
        return tLevelOld, tScaleNew * qModTNeg % self.T


# ---- the power basis on the device ----------------------------------------------------------------------------------------------------------
def _at_level(ev, ct, level):
    """ct as the reference reads it at a lower level: a copy of the leading limbs (the operand itself at its own level), as polynomial.py's"""
    if ct.Level() == level:
        return ct
    rq = ev.ringQ.AtLevel(level)
    out = Ciphertext([rq.NewPoly(p.npoly) for p in ct.Value], is_ntt=ct.IsNTT)
    for p, q in zip(ct.Value, out.Value):
        rq.CopyLvl(p, q)
    ev._copy_metadata(ct, out)
    return out


def _drop(ev, ct, level):
    """rlwe.Element.Resize to a lower level, in place"""
    if ct.Level() != level:
        ct.Value = _at_level(ev, ct, level).Value


def _rescale(ev, ct):
    """eval.Rescale(ct, ct): the blocks replaced by blocks of the lower level; nothing on a scale-invariant evaluator (evaluator.go:1417)"""
    if ev.ScaleInvariant:
        return
    out = ev.RescaleNew(ct)
    ct.Value, ct.Scale = out.Value, out.Scale


def _relinearize(ev, ct):
    """eval.Relinearize(ct, ct): the gadget product of the third component added to the first two, as bgv.Evaluator relinearises its own
    products (any number of P moduli)"""
    if ct.Degree() != 2:
        raise RingHipError("cannot relinearize: ctIn.Degree() should be 2 but is %d" % ct.Degree())
    level = ct.Level()
    ev._relin_add(level, ev.ringQ.AtLevel(level), ct.Value[2], ev._rlk("Relinearize"), ct)
    ct.Value = ct.Value[:2]


class PowerBasis:
    """power_basis.go:17-182 over a bgv.Evaluator: Value[n] = X^n, Value[1] a copy of the ciphertext given"""

    def __init__(self, ct, basis=Monomial):
        _basis(basis)
        self.Basis, self.Value = basis, {1: _copy_new(ct)}
        self.Value[1].Scale = int(getattr(ct, "Scale", 1))
        for name in ("IsBatched", "IsMontgomery"):
            if hasattr(ct, name):
                setattr(self.Value[1], name, getattr(ct, name))

    def GenPower(self, n, lazy, ev):
        """:57-78.  lazy: X^n is left at degree 2; the powers it is made of are relinearised on the way.  ev: a bgv.Evaluator"""
        if ev is None:
            raise RingHipError("cannot GenPower: EvaluatorInterface is nil")
        if self.Value.get(n) is None:
            if self._gen(n, lazy, True, ev):
                _rescale(ev, self.Value[n])

    def _gen(self, n, lazy, rescale, ev):
        """genPower :80-182 -> whether Value[n] is new and still waits for its rescaling (the rescale-on-use rule)"""
        if self.Value.get(n) is not None:
            return False
        a, b = SplitDegree(n)
        isPow2 = n & (n - 1) == 0
        rescaleA = self._gen(a, lazy and not isPow2, rescale, ev)
        rescaleB = self._gen(b, lazy and not isPow2, rescale, ev)
        X = self.Value
        if lazy:
            for k in (a, b):
                if X[k].Degree() == 2:
                    _relinearize(ev, X[k])                                         # (:101-111)
        if rescaleA:
            _rescale(ev, X[a])                                                     # (:113-117 / :131-135)
        if rescaleB:                                                               # never with b == a: Value[a] was there by then
            _rescale(ev, X[b])
        level = min(X[a].Level(), X[b].Level())
        xa = _at_level(ev, X[a], level)
        xb = xa if b == a else _at_level(ev, X[b], level)
        X[n] = ev.MulNew(xa, xb) if lazy else ev.MulRelinNew(xa, xb)              # (:125 / :143): both dispatch on ScaleInvariant
        scale = X[n].Scale
        ev._copy_metadata(X[1], X[n])
        X[n].Scale = scale
        return True


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------------
class Evaluator:
    """circuits/bgv/polynomial.Evaluator over a bgv.Evaluator, which brings the rings, T, the relinearisation key, ScaleInvariant
    (InvariantTensoring :27) and the encoder of the mapping path.  fused: None what FUSED_BGV_POLYNOMIAL says, else True / False for both arms."""

    def __init__(self, bgv_evaluator, fused=None):
        self.ev = bgv_evaluator
        if bgv_evaluator.ringQ.kind != Standard:
            raise RingHipError("cannot NewEvaluator: the BGV polynomial evaluator needs a standard ring (conjugate-invariant and 3N rings are not supported)")
        self.fused = None if fused is None else bool(fused)
        self.InvariantTensoring = bool(bgv_evaluator.ScaleInvariant)
        self._table = self._pc_table = None                                        # device tables of the two entries: this evaluator's, like the
        self._pc_block = None                                                      # reference's buffers (an evaluator serves one thread)

    def _sim(self):
        return SimEvaluator(self.ev.ringQ.moduli, self.ev.t, self.InvariantTensoring)

    def _use(self, arm):
        return FUSED_BGV_POLYNOMIAL[arm] if self.fused is None else self.fused

    # ---- Evaluate (circuits/bgv :40-76, common :29-91) ---------------------------------------------------------------------------------------------
    def _poly_vector(self, p):
        if isinstance(p, PolynomialVector):
            polyVec = p
        elif isinstance(p, Polynomial):
            polyVec = PolynomialVector([p])
        else:
            raise RingHipError("cannot Polynomial: invalid polynomial type, must be either Polynomial or PolynomialVector, but is %s" % type(p).__name__)
        self._refuse(polyVec)
        return polyVec

    def _refuse(self, polyVec):
        for p in polyVec.Value:
            _basis(p.Basis)
        if any(p.Lazy for p in polyVec.Value):
            raise RingHipError("cannot evaluate a polynomial with Lazy = true: the power basis then holds powers of mixed degrees, and the reference's "
                               "MulThenAdd drops the accumulator's third component when a relinearised power follows a lazy one (opOut.Resize(op0.Degree(), ...)): "
                               "there is nothing sound to match.  PowerBasis.GenPower(lazy=True) itself is supported")
        if polyVec.Mapping is not None and self.ev.encoder is None:
            raise RingHipError("cannot evaluate a PolynomialVector with a mapping: its per-slot coefficients need the BGV encoder: build the evaluator with Evaluator(..., encoder=enc)")

    def Evaluate(self, ct, p, targetScale):
        """:40-53: P(ct); a standard evaluator consumes the levels the simulator says, a scale-invariant one none"""
        polyVec = self._poly_vector(p)
        return self._evaluate(PowerBasis(ct, polyVec.Value[0].Basis), polyVec, targetScale)

    def EvaluateFromPowerBasis(self, pb, p, targetScale):
        """:58-76"""
        polyVec = self._poly_vector(p)
        if pb.Value.get(1) is None:
            raise RingHipError("cannot EvaluateFromPowerBasis: X^{1} is nil")
        return self._evaluate(pb, polyVec, targetScale)

    def _evaluate(self, powerbasis, polyVec, targetScale):
        ev = self.ev
        p0 = polyVec.Value[0]
        if p0.Degree() < 1:
            raise RingHipError("cannot evaluate poly: the degree must be at least 1")
        level, depth = powerbasis.Value[1].Level(), p0.Depth()                     # levelsConsumedPerRescaling = 1 (bgv :52), in both arms
        if level < depth:
            raise RingHipError("%d levels < %d log(d) -> cannot evaluate poly" % (level, depth))
        logDegree = p0.Degree().bit_length()
        logSplit = OptimalSplit(logDegree)
        odd, even = any(p.IsOdd for p in polyVec.Value), any(p.IsEven for p in polyVec.Value)
        powerbasis.GenPower(1 << (logDegree - 1), False, ev)                       # the powers of two, relinearised (:71)
        for i in range((1 << logSplit) - 1, 2, -1):                                # (:76-82)
            if not (even or odd) or (i & 1 == 0 and even) or (i & 1 == 1 and odd):
                powerbasis.GenPower(i, p0.Lazy, ev)
        X1 = powerbasis.Value[1]
        PS = polyVec.PatersonStockmeyerPolynomial(self._sim(), X1.Level(), ev._scale(X1), int(targetScale) % ev.t)
        return self.EvaluatePatersonStockmeyerPolynomialVector(PS, powerbasis)

    # ---- common :101-251 ---------------------------------------------------------------------------------------------------------------------------------
    def EvaluatePatersonStockmeyerPolynomialVector(self, poly, pb):
        split = len(poly.Value[0].Value)
        babySteps = [None] * split
        for i in range(split):
            babySteps[split - i - 1] = self.EvaluateBabyStep(i, poly, pb)
        while len(babySteps) != 1:
            giantsteps = [0] * len(babySteps)
            i = 0
            while i < len(babySteps):                                              # (:121-128)
                if i == len(babySteps) - 1:
                    giantsteps[i] = 2
                elif babySteps[i].Degree == babySteps[i + 1].Degree:
                    giantsteps[i] = 1
                    i += 1
                i += 1
            for i in range(len(babySteps)):
                self.EvaluateGianStep(i, giantsteps, babySteps, pb)
            babySteps = [b for b in babySteps if b is not None]
        res = babySteps[0].Value
        if res.Degree() == 2:
            _relinearize(self.ev, res)
        _rescale(self.ev, res)
        return res

    def EvaluateBabyStep(self, i, poly, pb):
        """:165-189: the inner product of the powers with the coefficients of the i-th baby-step polynomials"""
        polyVec = PolynomialVector._derived([ps.Value[i] for ps in poly.Value], poly.Mapping, getattr(poly, "_index", None))
        first = poly.Value[0].Value[i]
        return BabyStep(first.Degree(), self.EvaluatePolynomialVectorFromPowerBasis(first.Level, polyVec, pb, first.Scale))

    def EvaluateGianStep(self, i, giantSteps, babySteps, pb):
        """:193-223, spelled as in the reference"""
        if giantSteps[i] == 2:
            babySteps[i].Degree = babySteps[i - 1].Degree
        elif giantSteps[i] == 1:
            even, odd = babySteps[i], babySteps[i + 1]
            deg = 1 << babySteps[i].Degree.bit_length()
            self.EvaluateMonomial(even.Value, odd.Value, pb.Value[deg])
            odd.Degree = 2 * deg - 1
            babySteps[i] = None

    def EvaluateMonomial(self, a, b, xpow):
        """:226-251: b <- a + rescale(b) * xpow"""
        ev = self.ev
        if b.Degree() == 2:
            _relinearize(ev, b)
        _rescale(ev, b)
        level = min(b.Level(), xpow.Level())
        prod = ev.MulNew(_at_level(ev, b, level), _at_level(ev, xpow, level))       # eval.Mul(b, xpow, b): b grows to degree 2
        b.Value, b.Scale = prod.Value, prod.Scale
        if not InDelta(ev._scale(a), b.Scale, float(ScalePrecision - 12)):
            raise RingHipError("evalMonomial: scale discrepency: (rescale(b) * X^{n}).Scale = %s != a.Scale = %s" % (b.Scale, ev._scale(a)))
        level = min(a.Level(), b.Level())
        _drop(ev, b, level)
        ev.Add(b, _at_level(ev, a, level), b)

    # ---- EvaluatePolynomialVectorFromPowerBasis :254-359 -----------------------------------------------------------------------------------------------------
    def _zero(self, npoly, degree, level):
        """rlwe.NewCiphertext"""
        rq = self.ev.ringQ.AtLevel(level)
        out = Ciphertext([rq.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)
        for p in out.Value:
            rq.vec_op("ZERO", None, None, p)
        return out

    def EvaluatePolynomialVectorFromPowerBasis(self, targetLevel, pol, pb, targetScale):
        """P(ct) = sum c_i ct^i from the powers at hand, at targetLevel and targetScale.  With the fused path chosen it is ONE launch: every step
        of the reference's sequence ends in a canonical reduction of an exact value, so the canonical residue of the exact sum is its bits.  A
        power below the target level, or a modulus of 2^61 or more, sends the whole sum to the composed sequence of evaluator calls: the same
        bits.  (Below the target level the reference updates the limbs the power has and leaves the rest of the accumulator stale; here the
        accumulator is dropped to that level, as polynomial.py does.)"""
        ev, X = self.ev, pb.Value
        self._refuse(pol)
        targetScale = int(targetScale) % ev.t
        even, odd = pol.IsEven(), pol.IsOdd()
        p0 = pol.Value[0]
        minimumDegreeNonZeroCoefficient = len(p0.Coeffs) - 1
        if even and not odd:
            minimumDegreeNonZeroCoefficient -= 1
        used = lambda key: not (even or odd) or (key & 1 == 0 and even) or (key & 1 == 1 and odd)
        if X.get(1) is None:
            raise RingHipError("cannot EvaluatePolynomialVectorFromPowerBasis: X^{1} is nil")
        if minimumDegreeNonZeroCoefficient == 0:
            keys, degree = [], 1
        else:
            keys = [k for k in range(p0.Degree(), 0, -1) if used(k)]
            degree = max([X[k].Degree() for k in range(p0.Degree(), 0, -1) if X.get(k) is not None] or [0])
            for k in keys:
                if X.get(k) is None:
                    raise RingHipError("cannot EvaluatePolynomialVectorFromPowerBasis: X^{%d} is missing from the power basis" % k)
            if any(X[k].Degree() != degree for k in keys):
                raise RingHipError("cannot EvaluatePolynomialVectorFromPowerBasis: the powers have mixed degrees (a lazy power basis): the reference's MulThenAdd "
                                   "drops the accumulator's third component when a relinearised power follows a lazy one (opOut.Resize(op0.Degree(), ...)): "
                                   "there is nothing sound to match")
        vector = pol.Mapping is not None
        coeff = (lambda k: self.GetVectorCoefficient(pol, k)) if vector else (lambda k: self.GetSingleCoefficient(p0, k))
        npoly = X[1].Value[0].npoly
        res = None
        if self._use("vector" if vector else "scalar") and all(X[k].Level() >= targetLevel for k in keys) \
                and all(q >> LC_MODULUS_BITS == 0 for q in ev._qs(targetLevel)):
            res = Ciphertext([ev.ringQ.AtLevel(targetLevel).NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)
            (self._fused_vector if vector else self._fused_scalar)(targetLevel, targetScale, keys, pol, even, X, res.Value)
        if res is None:
            res = self._zero(npoly, degree, targetLevel)
            res.Scale = targetScale
            if even:
                ev.Add(res, coeff(0), res)                                         # (:293 / :307 / :330 / :343)
            for k in keys:
                level = min(X[k].Level(), res.Level())
                _drop(ev, res, level)
                ev.MulThenAdd(_at_level(ev, X[k], level), coeff(k), res)           # (:315 / :351)
        ev._copy_metadata(X[1], res)                                               # *res.MetaData = *X[1].MetaData; res.Scale = targetScale
        res.Scale, res.IsNTT = targetScale, True
        return res

    def _ratio(self, xScale, targetScale):
        """opOut.Scale / op0.Scale modulo T as MulThenAdd forms it (evaluator.go:1177-1180, :1224-1230): 1 for equal scales"""
        t = self.ev.t
        return 1 if xScale == targetScale else pow(xScale, t - 2, t) * targetScale % t

    # the call of rh_ckks_linear_combination with its device table is scheme-independent: polynomial.py's, on this evaluator's own _table
    linear_combination = PolynomialEvaluator.linear_combination

    def _fused_scalar(self, level, targetScale, keys, pol, even, X, outs):
        """(:321-356) as one launch of rh_ckks_linear_combination with s0 == s1 and c0 == c1: per limb the scalar of MulScalarBigintThenAdd, the
        coefficient times opOut.Scale / op0.Scale centred modulo T (evaluator.go:1177-1194), and of AddScalarBigint, the constant at the
        accumulator's scale, centred, times T^-1 mod Q_level (:209-221)"""
        ev, p0 = self.ev, pol.Value[0]
        qs = ev._qs(level)
        s = [[ev._center_t(self.GetSingleCoefficient(p0, k) * self._ratio(ev._scale(X[k]), targetScale)) % q for q in qs] for k in keys]
        c = None
        if even:
            v = ev._center_t(self.GetSingleCoefficient(p0, 0) * targetScale) * pow(ev.t, -1, math.prod(qs))
            c = [v % q for q in qs]
        self.linear_combination(level, [X[k].Value for k in keys], s, s, c, c, outs)

    def _fused_vector(self, level, targetScale, keys, pol, even, X, outs):
        """(:281-319) as one launch of rh_bgv_plain_combination.  The reference encodes the slot vector of k-th coefficients at the scale
        opOut.Scale / X_k.Scale (evaluator.go:1221-1235), multiplies by tMontgomery and accumulates the Montgomery product on every component
        (:1370-1400): the T^-1 of Encode's scale-up and the T of tMontgomery cancel modulo q_i, so the plaintext of a term is the Montgomery
        form of the plain lift (Embed, no scale-up) of the vector, which ONE call of the batched encoder makes for all terms and the constant,
        the scales multiplied into the values here (EncodeRingT's MulScalar is linear modulo T).  The constant (Encode at res.Scale, :254-262)
        keeps its T^-1 as the entry's per-limb scalar."""
        ev = self.ev
        t, K = ev.t, len(keys)
        nvec = K + (1 if even else 0)
        rq = ev.ringQ.AtLevel(level)
        N, L = ev.ringQ.N, level + 1
        m, c = [], None
        if nvec:
            vals = np.stack([self.GetVectorCoefficient(pol, k, self._ratio(ev._scale(X[k]), targetScale)) for k in keys]
                            + ([self.GetVectorCoefficient(pol, 0, targetScale)] if even else []))
            if self._pc_block is None or (self._pc_block.npoly, self._pc_block.limbs) != (nvec, L):
                self._pc_block = rq.NewPoly(nvec)
            block = self._pc_block
            ev.encoder.Embed(vals, types.SimpleNamespace(Scale=1, IsNTT=True, IsMontgomery=True), block)
            m = [block.ptr + 8 * r * L * N for r in range(K)]
            c = block.ptr + 8 * K * L * N if even else None
        Lb = lib()
        words = Lb.rh_bgv_plain_combination_table_words(K)
        if K and (self._pc_table is None or self._pc_table.words < words):
            self._pc_table = DevicePoly(ev.ringQ, 1, -(-words // N))
        x = (C.c_void_p * max(3 * K, 1))()
        rows = (C.c_int * max(K, 1))()
        mp = (C.c_void_p * max(K, 1))(*m)
        for i, k in enumerate(keys):
            for j, p in enumerate(X[k].Value):
                x[3 * i + j] = p.ptr
            rows[i] = X[k].Value[0].limbs
        ptrs = [p.ptr for p in outs] + [None] * (3 - len(outs))
        cs = _u64([pow(t, -1, q) for q in ev._qs(level)]) if even else None
        _check(Lb.rh_bgv_plain_combination(ev.ringQ._h, level, K, x, rows, mp, c, _p(cs) if even else None, *ptrs, outs[0].npoly,
                                           self._pc_table.ptr if K else None, self._pc_table.words if K else 0))

    # ---- CoefficientGetter (circuits/bgv/polynomial/polynomial_evaluator.go:80-106) -------------------------------------------------------------------------
    def GetSingleCoefficient(self, pol, k):
        c = pol.Coeffs[k]
        if c is None:
            raise RingHipError("cannot GetSingleCoefficient: coefficient %d is nil" % k)
        return c % self.ev.t

    def GetVectorCoefficient(self, pol, k, scale=1):
        """the k-th coefficients over the slots as []uint64, zero where no polynomial is mapped; scale: a factor modulo T multiplied in"""
        slots = self.ev.encoder.MaxSlots()
        values = np.zeros(slots, dtype=np.uint64)
        index = pol.slot_index(slots)
        for i, p in enumerate(pol.Value):
            c = p.Coeffs[k]
            if c is None:
                raise RingHipError("cannot GetVectorCoefficient: coefficient %d of polynomial %d is nil" % (k, i))
            if i in index:
                values[index[i]] = c * int(scale) % self.ev.t
        return values

"""Host-side mirror of the reference's polynomial evaluation circuit for CKKS on device-resident batches: the Paterson-Stockmeyer recursion, the
power basis and the scale bookkeeping; the arithmetic is the device evaluator's (ckks.Evaluator) and, for a baby step, one launch of
rh_ckks_linear_combination (csrc/ckks.hip).

  utils/bignum/polynomial.go                          OptimalSplit :14-23   NewPolynomial :48-113   ChangeOfBasis :119-141   Depth / Degree :144-151
                                                      Evaluate :176-255     Factorize :258-314
  circuits/common/polynomial/polynomial.go            NewPolynomial :28-35  Factorize :38-58        PatersonStockmeyerPolynomial :74-106
                                                      recursePS :109-153    PolynomialVector :159-229
  circuits/common/polynomial/power_basis.go           NewPowerBasis :25-30  SplitDegree :34-52      GenPower :57-78           genPower :80-182
  circuits/common/polynomial/polynomial_evaluator.go  Evaluate :29-91       EvaluatePatersonStockmeyerPolynomialVector :101-161
                                                      EvaluateBabyStep :165-189   EvaluateGianStep :193-223   EvaluateMonomial :226-251
                                                      EvaluatePolynomialVectorFromPowerBasis :254-359
  circuits/common/polynomial/polynomial_evaluator_sim.go   SimOperand, SimPowerBasis.GenPower :25-38
  circuits/ckks/polynomial/{polynomial,polynomial_evaluator,polynomial_evaluator_sim}.go   the CKKS wrappers and the simulator

A batch of npoly ciphertexts is one Ciphertext (ckks.py); all of them share the level and the scale.  Where the reference reads an operand at a
lower level than it was allocated for (ring.AtLevel), the device path copies its leading limbs (DropLevelNew): the same values.

Refused by name: polynomials with Lazy = True (the power basis then holds powers of mixed degrees, and the reference's MulThenAdd drops the
accumulator's third component when a relinearised power follows a lazy one: opOut.Resize(op0.Degree(), ...), schemes/ckks/evaluator.go:945 with
core/rlwe/element.go:170-176 -- there is nothing sound to match; PowerBasis.GenPower(lazy=True) itself is supported), a mapping without an
encoder or with encoding_precision > 53, vector polynomials on conjugate-invariant rings (the encoder is standard-only), 3N rings."""
import copy
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from .ckks import Complex, Scale, ScalePrecision, to_complex, _round
from .ringhip import ConjugateInvariant, DevicePoly, Matrix3N, RingHipError, _check, _p, _u64, lib
from .schemes import Ciphertext

Monomial, Chebyshev = 0, 1            # bignum.Basis (utils/bignum/metadata.go)


def OptimalSplit(logDegree):
    """bignum/polynomial.go:14-23"""
    logSplit = logDegree >> 1
    a = (1 << logSplit) + (1 << (logDegree - logSplit)) + logDegree - logSplit - 3
    b = (1 << (logSplit + 1)) + (1 << (logDegree - logSplit - 1)) + logDegree - logSplit - 4
    return logSplit + 1 if a > b else logSplit


def SplitDegree(n):
    """power_basis.go:34-52: a + b = n with |a - b| smallest, a and / or b odd where possible"""
    if n <= 0:
        raise RingHipError("invalid n: n=%d should be greater than zero" % n)
    if n & (n - 1) == 0:
        return n // 2, n // 2
    k = (n - 1).bit_length() - 1
    return (1 << k) - 1, n + 1 - (1 << k)


def _prec_of(c):
    """the precision new(big.Float).Set... gives a coefficient: 53 bits from a float64, 64 from an integer"""
    return 64 if isinstance(c, (int, np.integer)) and not isinstance(c, bool) else 53


class Polynomial:
    """bignum.Polynomial with the evaluation fields of polynomial.Polynomial.  Coeffs: ckks.Complex values (None: a nil coefficient, which
    Factorize may leave); each carries the precision of the big.Float it stands for in `prec` (Coeffs of one polynomial share it: 53 bits for
    []float64 / []complex128, the default; `prec` for Fractions and ckks.Complex), and every Add / Sub of Factorize rounds to it.
    IsOdd and IsEven are fields, both true from the constructor as in the reference (bignum/polynomial.go:104-111), never inferred."""

    def __init__(self, basis, coeffs, interval=None, prec=None):
        if basis not in (Monomial, Chebyshev):
            raise RingHipError("invalid basis type, allowed types are `Monomial` or `Chebyshev` but is %r" % (basis,))
        self.Basis = basis
        coeffs = list(coeffs)
        self.prec = int(prec) if prec is not None else max([_prec_of(c) for c in coeffs] + [53])
        self.Coeffs = [None if c is None else c if isinstance(c, Complex) else Complex(*to_complex(c, self.prec)) for c in coeffs]
        a, b = (0, 0) if interval is None else interval
        self.A, self.B = _round(Fraction(a), 53), _round(Fraction(b), 53)          # new(big.Float).SetFloat64
        self.IsOdd = self.IsEven = True
        self.MaxDeg, self.Lead, self.Lazy = len(self.Coeffs) - 1, True, False      # polynomial.NewPolynomial :28-35
        self.Level, self.Scale = 0, None

    @classmethod
    def _raw(cls, like, coeffs):
        p = object.__new__(cls)
        p.Basis, p.Coeffs, p.prec, p.A, p.B, p.IsOdd, p.IsEven = like.Basis, coeffs, like.prec, like.A, like.B, like.IsOdd, like.IsEven
        p.MaxDeg, p.Lead, p.Lazy, p.Level, p.Scale = 0, False, False, 0, None     # the zero value of polynomial.Polynomial
        return p

    def Degree(self):
        return len(self.Coeffs) - 1

    def Depth(self):
        return int(math.ceil(math.log2(float(self.Degree()))))

    def ChangeOfBasis(self):
        """:119-141 -> (scalar, constant) as Fractions: 1 and 0, or 2 / (b - a) and (-a - b) / (b - a) with the reference's roundings"""
        if self.Basis == Monomial:
            return Fraction(1), Fraction(0)
        num = _round(self.B - self.A, 53)
        scalar = _round(Fraction(2) / num, 64)                                     # Quo of SetInt64(2), 64 bits, and num
        constant = _round(_round(-self.B - self.A, 53) / num, 53)
        return scalar, constant

    def Evaluate(self, x):
        """:176-255 in exact rationals (the reference rounds every step to the precision of x): the value a decrypted result is compared with.
        The change of basis adds its constant to the real part; the reference adds it to the imaginary part as well (:218-219), which is the
        same for the real x and the symmetric intervals its tests use."""
        x = Complex(*to_complex(x, 64)) if not isinstance(x, Complex) else x
        mul = lambda u, v: (u[0] * v[0] - u[1] * v[1], u[0] * v[1] + u[1] * v[0])
        co = [(0, 0) if c is None else (c.re, c.im) for c in self.Coeffs]
        if self.Basis == Monomial:
            y = co[-1]
            for c in reversed(co[:-1]):
                y = mul(y, (x.re, x.im))
                y = (y[0] + c[0], y[1] + c[1])
            return Complex(*y)
        scalar, constant = self.ChangeOfBasis()
        t = (x.re * scalar + constant, x.im * scalar)                              # (:215-219)
        x2 = (2 * t[0], 2 * t[1])
        prev, y = (Fraction(1), Fraction(0)), co[0]
        for c in co[1:]:
            m = mul(t, c)
            y = (y[0] + m[0], y[1] + m[1])
            nxt = mul(x2, t)
            prev, t = t, (nxt[0] - prev[0], nxt[1] - prev[1])
        return Complex(*y)

    def _add(self, a, b, sign=1):
        return Complex(_round(a.re + sign * b.re, self.prec), _round(a.im + sign * b.im, self.prec))

    def Factorize(self, n):
        """p = X^n pq + pr (T_n pq + pr in the Chebyshev basis): bignum :258-314 with the fields of polynomial.Polynomial.Factorize :38-58"""
        if n < self.Degree() >> 1:
            raise RingHipError("cannot Factorize: n < p.Degree()/2")
        deg = self.Degree()
        pr = list(self.Coeffs[:n])
        pq = [None] * (deg - n + 1)
        pq[0] = self.Coeffs[n]
        even, odd = self.IsEven, self.IsOdd
        for i in range(n + 1, deg + 1):
            c = self.Coeffs[i]
            if c is None or not (not (even or odd) or (i & 1 == 0 and even) or (i & 1 == 1 and odd)):
                continue
            if self.Basis == Monomial:
                pq[i - n] = c
            else:
                j = i - n
                pq[j] = self._add(c, c)                                             # (:295)
                pr[n - j] = self._add(pr[n - j], c, -1) if pr[n - j] is not None else Complex(-c.re, -c.im)   # (:297-303)
        q, r = Polynomial._raw(self, pq), Polynomial._raw(self, pr)
        q.MaxDeg = self.MaxDeg
        r.MaxDeg = n - 1 if self.MaxDeg == deg else self.MaxDeg - (deg - n + 1)
        q.Lead = bool(self.Lead)
        return q, r

    def PatersonStockmeyerPolynomial(self, sim, inputLevel, inputScale, outputScale):
        """polynomial.go:74-106; sim: a SimEvaluator"""
        logDegree = self.Degree().bit_length()
        logSplit = OptimalSplit(logDegree)
        pb = SimPowerBasis()
        pb[1] = SimOperand(inputLevel, Scale(inputScale))
        pb.GenPower(1 << logDegree, sim)
        for i in range((1 << logSplit) - 1, 2, -1):
            pb.GenPower(i, sim)
        value, _ = recursePS(logSplit, inputLevel - sim.PolynomialDepth(self.Degree()), self, pb, Scale(outputScale), sim)
        return PatersonStockmeyerPolynomial(self.Degree(), 1 << logSplit, inputLevel, Scale(outputScale), value)


class PatersonStockmeyerPolynomial:
    """polynomial.go:64-70"""

    def __init__(self, degree, base, level, scale, value):
        self.Degree, self.Base, self.Level, self.Scale, self.Value = degree, base, level, scale, value


class PolynomialVector:
    """polynomial.go:159-229 with the CKKS wrapper's Depth and ChangeOfBasis (circuits/ckks/polynomial/polynomial.go:22-56): polynomials of one
    basis and one degree, and mapping[i] = the slots polynomial i is evaluated on; slots no polynomial names evaluate to zero"""

    def __init__(self, polys, mapping=None):
        polys = list(polys)
        if len({p.Basis for p in polys}) > 1:
            raise RingHipError("polynomial basis must be the same for all polynomials in a polynomial vector")
        if len({p.Degree() for p in polys}) > 1:
            raise RingHipError("polynomial degree must all be the same")
        self.Value = polys
        self.Mapping = None if mapping is None else {int(k): [int(j) for j in v] for k, v in mapping.items()}

    def IsEven(self):
        return all(p.IsEven for p in self.Value)

    def IsOdd(self):
        return all(p.IsOdd for p in self.Value)

    def Depth(self):
        return self.Value[0].Depth()

    def Factorize(self, n):
        qs, rs = zip(*[p.Factorize(n) for p in self.Value])
        return PolynomialVector(qs, self.Mapping), PolynomialVector(rs, self.Mapping)

    def ChangeOfBasis(self, slots):
        scalar, constant = [Fraction(0)] * slots, [Fraction(0)] * slots
        for i, m in (self.Mapping or {}).items():
            s, c = self.Value[i].ChangeOfBasis()
            for j in m:
                scalar[j], constant[j] = s, c
        return scalar, constant

    def PatersonStockmeyerPolynomial(self, sim, inputLevel, inputScale, outputScale):
        """polynomial.go:241-251"""
        return PatersonStockmeyerPolynomialVector([p.PatersonStockmeyerPolynomial(sim, inputLevel, inputScale, outputScale) for p in self.Value], self.Mapping)


class PatersonStockmeyerPolynomialVector:
    def __init__(self, value, mapping):
        self.Value, self.Mapping = value, mapping


# ---- the simulator: levels and scales alone -------------------------------------------------------------------------------------------------
class SimOperand:
    def __init__(self, level, scale):
        self.Level, self.Scale = level, scale


class SimEvaluator:
    """circuits/ckks/polynomial/polynomial_evaluator_sim.go: Q the moduli chain, nb = levels_consumed_per_rescaling"""

    def __init__(self, Q, levels_consumed_per_rescaling=1):
        self.Q, self.nb = [int(q) for q in Q], int(levels_consumed_per_rescaling)

    def PolynomialDepth(self, degree):
        if degree <= 0:
            raise RingHipError("invalid degree: degree=%d should be greater than zero" % degree)
        return self.nb * (degree.bit_length() - 1)                                 # (:26-33)

    def Rescale(self, op0):
        for _ in range(self.nb):                                                   # (:36-41)
            op0.Scale = op0.Scale.Div(Scale(self.Q[op0.Level]))
            op0.Level -= 1

    def MulNew(self, op0, op1):
        return SimOperand(min(op0.Level, op1.Level), op0.Scale.Mul(op1.Scale))     # (:44-49)

    def UpdateLevelAndScaleBabyStep(self, lead, tLevelOld, tScaleOld):
        tScaleNew = Scale(tScaleOld)
        if lead:
            for i in range(self.nb):                                               # (:57-61)
                tScaleNew = tScaleNew.Mul(Scale(self.Q[tLevelOld - i]))
        return tLevelOld, tScaleNew

    def UpdateLevelAndScaleGiantStep(self, lead, tLevelOld, tScaleOld, xPowScale):
        top = tLevelOld if lead else tLevelOld + self.nb                           # (:71-82)
        qi = 1
        for i in range(self.nb):
            qi *= self.Q[top - i]
        return tLevelOld + self.nb, Scale(tScaleOld).Mul(Scale(qi)).Div(xPowScale)  # (:84-86)


class SimPowerBasis(dict):
    def GenPower(self, n, sim):
        """polynomial_evaluator_sim.go:25-38"""
        if n < 2:
            return
        a, b = SplitDegree(n)
        self.GenPower(a, sim)
        self.GenPower(b, sim)
        self[n] = sim.MulNew(self[a], self[b])
        sim.Rescale(self[n])


def Log2Delta(s, s1):
    """rlwe.Scale.Log2Delta (core/rlwe/scale.go:140-149): -log2(|a - b| / max(a, b)); +inf for equal scales"""
    a, b = Scale(s).Value, Scale(s1).Value
    d = abs(a - b) / max(a, b)
    return float("inf") if d == 0 else -(math.log2(d.numerator) - math.log2(d.denominator))


def InDelta(s, s1, log2Delta):
    return Log2Delta(s, s1) >= log2Delta


def recursePS(logSplit, targetLevel, p, pb, outputScale, sim):
    """polynomial.go:109-153 -> (the baby-step polynomials with their Level and Scale set, the SimOperand of their combination)"""
    if p.Degree() < 1 << logSplit:
        if p.Lead and logSplit > 1 and p.MaxDeg > (1 << p.MaxDeg.bit_length()) - (1 << (logSplit - 1)):
            return recursePS(OptimalSplit(p.Degree().bit_length()), targetLevel, p, pb, outputScale, sim)
        p = copy.copy(p)                                                           # the reference's p is a value: the caller's polynomial keeps its fields
        p.Level, p.Scale = sim.UpdateLevelAndScaleBabyStep(p.Lead, targetLevel, outputScale)
        return [p], SimOperand(p.Level, p.Scale)
    nextPower = 1 << logSplit
    while nextPower < (p.Degree() >> 1) + 1:
        nextPower <<= 1
    XPow = pb[nextPower]
    coeffsq, coeffsr = p.Factorize(nextPower)
    tLevelNew, tScaleNew = sim.UpdateLevelAndScaleGiantStep(p.Lead, targetLevel, outputScale, XPow.Scale)
    bsgsQ, res = recursePS(logSplit, tLevelNew, coeffsq, pb, tScaleNew, sim)
    sim.Rescale(res)
    res = sim.MulNew(res, XPow)
    bsgsR, tmp = recursePS(logSplit, targetLevel, coeffsr, pb, res.Scale, sim)
    if not InDelta(tmp.Scale, res.Scale, float(ScalePrecision - 12)):
        raise RingHipError("recursePS: res.Scale != tmp.Scale: %s != %s" % (res.Scale, tmp.Scale))
    return bsgsQ + bsgsR, res


# ---- the power basis on the device ----------------------------------------------------------------------------------------------------------
def _copy_meta(src, dst):
    if hasattr(src, "LogDimensions"):
        dst.LogDimensions = src.LogDimensions


def _copy_new(ct):
    """rlwe.Ciphertext.CopyNew"""
    rq = ct.Value[0].ring.AtLevel(ct.Level())
    out = Ciphertext([rq.NewPoly(p.npoly) for p in ct.Value], is_ntt=ct.IsNTT)
    for p, q in zip(ct.Value, out.Value):
        rq.CopyLvl(p, q)
    if getattr(ct, "Scale", None) is not None:
        out.Scale = ct.Scale
    _copy_meta(ct, out)
    return out


def _at_level(ev, ct, level):
    """ct as the reference reads it at a lower level: a copy of the leading limbs (the operand itself at its own level)"""
    return ct if ct.Level() == level else ev.DropLevelNew(ct, ct.Level() - level)


def _rescale(ev, ct):
    """eval.Rescale(ct, ct): the blocks replaced by blocks of the lower level"""
    low = ev.ringQ.AtLevel(ct.Level() - ev.nb_rescales) if ct.Level() >= ev.nb_rescales else None
    if low is None:
        raise RingHipError("cannot Rescale: input Ciphertext level is too low")
    out = Ciphertext([low.NewPoly(p.npoly) for p in ct.Value], is_ntt=True)
    ev.Rescale(ct, out)
    ct.Value, ct.Scale = out.Value, out.Scale


def _relinearize(ev, ct):
    """eval.Relinearize(ct, ct)"""
    if ev.ks is None or ev.rlk is None:
        raise RingHipError("cannot relinearize: relinearization key is missing")
    ev.ks.Relinearize(ct, ct, rlk=ev.rlk)
    ct.Value = ct.Value[:2]


# The step after every product of a Chebyshev power basis as ONE launch of rh_ckks_axpby, or as the reference's own calls: the same bits.
# profiles/minimax.json (tools/bench_minimax.py, "fused_power_basis_default"): a whole GenPower(31) at N = 2^16, 25 limbs is 1.17 and 1.13
# times faster with the kernel at batches of 1 and 8 (medians; beyond the run-to-run spread at batch 1).
FUSED_POWER_BASIS = {"chebyshev_step": True}


def axpby(ringQ, level, x, t, out, ra, rb=None, s0=None, s1=None):
    """rh_ckks_axpby on lists of DevicePoly: out_j = ra x_j - rb t_j - [j == 0] s on limbs 0 .. level.  x and t (None: no second term) may
    sit at higher levels (they are read as their AtLevel views); out is dense at `level` and may be x where x is."""
    npoly = x[0].npoly
    if any(p.npoly != npoly for p in list(x) + list(t or []) + list(out)) or any(p.limbs != level + 1 for p in out):
        raise RingHipError("cannot axpby: every block holds the same number of polys, and the outputs level + 1 = %d limbs" % (level + 1))
    if len({p.limbs for p in x}) != 1 or (t and len({p.limbs for p in t}) != 1):
        raise RingHipError("cannot axpby: the components of an operand sit at one level")
    ptrs = lambda polys: [p.ptr for p in polys] + [None] * (3 - len(polys))
    _check(lib().rh_ckks_axpby(ringQ._h, level, *ptrs(x), x[0].limbs, *ptrs(t or []), t[0].limbs if t else 0, *ptrs(out), npoly,
                               _p(_u64(ra)), _p(_u64(rb)) if t else None, _p(_u64(s0)) if s0 is not None else None,
                               _p(_u64(s1)) if s1 is not None else None))


def affine_minus(ev, ct, constant, fused, out=None):
    """constant - ct: the reference's Mul(ct, -1, out) and Add(out, constant, out), or with `fused` one launch of rh_ckks_axpby with
    ra = q - 1 and s = -constant.  out: None (a new ciphertext) or ct itself."""
    if out is None:
        out = ev._new(ct.Degree(), ct)
        _copy_meta(ct, out)
    if not fused:
        ev.Mul(ct, -1, out)
        ev.Add(out, constant, out)
        return out
    level, scale = ev._operands("Add", ct, out), ev._scale(ct, "Add")
    qs = ev._qs(level)
    s0, s1 = ev._rns_scalar(level, scale, to_complex(constant, ev.encoding_precision))
    axpby(ev.ringQ, level, ct.Value, None, out.Value, [q - 1 for q in qs], None, [(q - v) % q for v, q in zip(s0, qs)], [(q - v) % q for v, q in zip(s1, qs)])
    out.Scale, out.IsNTT = scale, True
    return out


class PowerBasis:
    """power_basis.go:17-182: Value[n] = X^n (T_n(X) in the Chebyshev basis), Value[1] a copy of the ciphertext given.
    fused: None what FUSED_POWER_BASIS says, else True / False."""

    def __init__(self, ct, basis, fused=None):
        if basis not in (Monomial, Chebyshev):
            raise RingHipError("invalid basis type, allowed types are `Monomial` or `Chebyshev` but is %r" % (basis,))
        self.Basis, self.Value = basis, {1: _copy_new(ct)}
        self.fused = None if fused is None else bool(fused)

    def GenPower(self, n, lazy, ev):
        """:57-78.  lazy: X^n is left at degree 2; the powers it is made of are relinearised on the way.  ev: a ckks.Evaluator"""
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
        X[n] = ev.MulNew(xa, xb) if lazy else ev.MulRelinNew(xa, xb)              # (:125 / :143)
        _copy_meta(X[1], X[n])
        if self.Basis == Chebyshev and not self._chebyshev_step(n, abs(a - b), lazy, ev):      # T_n = 2 T_a T_b - T_|a - b| (:148-176)
            c = abs(a - b)
            ev.Add(X[n], X[n], X[n])
            if c == 0:
                ev.Add(X[n], -1, X[n])
            else:
                self.GenPower(c, lazy, ev)
                level = min(X[n].Level(), X[c].Level())
                if X[n].Level() != level:
                    ev.DropLevel(X[n], X[n].Level() - level)
                xc = _at_level(ev, X[c], level)
                if xc.Degree() > X[n].Degree():                                    # the reference's Resize grows opOut to the larger degree
                    grown = ev.SubNew(X[n], xc)
                    X[n].Value, X[n].Scale = grown.Value, grown.Scale
                else:
                    ev.Sub(X[n], xc, X[n])
        return True

    def _chebyshev_step(self, n, c, lazy, ev):
        """Add(X, X, X), then Add(X, -1, X) or GenPower(c) and the scale-matching Sub(X, T_c, X) (:157-176), as ONE launch of rh_ckks_axpby:
        every step of that sequence ends in CRed or MRed of exact values, so the canonical residue of 2 k0 X - k1 T_c - s is its bits (k0 or
        k1 the integer ratio of the scales as evaluateInPlace multiplies it in, the other 1).  False: the composed calls are to run -- the
        switch is off, or T_c has more components than X (the reference's Sub then negates with ring.Neg, which writes q for 0)."""
        if not (FUSED_POWER_BASIS["chebyshev_step"] if self.fused is None else self.fused):
            return False
        X = self.Value
        xn, prec = X[n], ev.encoding_precision
        scale = ev._scale(xn, "Add")
        if c == 0:
            level = ev._operands("Add", xn)
            qs = ev._qs(level)
            s0, s1 = ev._rns_scalar(level, scale, to_complex(-1, prec))              # what Add(X, -1, X) adds: its negative is subtracted
            axpby(ev.ringQ, level, xn.Value, None, xn.Value, [2] * len(qs), None, [(q - v) % q for v, q in zip(s0, qs)], [(q - v) % q for v, q in zip(s1, qs)])
            return True
        self.GenPower(c, lazy, ev)
        xc = X[c]
        if xc.Degree() > xn.Degree():
            return False
        ev._operands("Sub", xn)
        ev._operands("Sub", xc)
        level = min(xn.Level(), xc.Level())
        qs = ev._qs(level)
        scalec = ev._scale(xc, "Sub")
        cmp = scale.Cmp(scalec)
        k = [1] * len(qs)
        if cmp:                                                                    # Mul(ct, ratioInt, tmp) (evaluator.go:282 ...)
            ratioInt = int((scale.Div(scalec) if cmp == 1 else scalec.Div(scale)).Value)
            k = ev._rns_scalar(level, Scale(1), to_complex(ratioInt, prec))[0]
        ra = [2 * v % q for v, q in zip(k, qs)] if cmp == -1 else [2] * len(qs)
        rb = list(k) if cmp == 1 else [1] * len(qs)
        out = xn.Value if xn.Level() == level else [ev.ringQ.AtLevel(level).NewPoly(p.npoly) for p in xn.Value]
        axpby(ev.ringQ, level, xn.Value, xc.Value, out, ra, rb)
        xn.Value, xn.Scale = out, scale.Max(scalec)
        return True


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------------
class BabyStep:
    def __init__(self, degree, value):
        self.Degree, self.Value = degree, value


class PolynomialEvaluator:
    """circuits/ckks/polynomial.Evaluator over a ckks.Evaluator (which brings the rings, the relinearisation key, levels_consumed_per_rescaling,
    encoding_precision, the encoder for the mapping path, and the fused / composed choice: FUSED_DEFAULT["linear_combination"])"""

    def __init__(self, ckks_evaluator):
        self.ev = ckks_evaluator
        if ckks_evaluator.ringQ.kind == Matrix3N:
            raise RingHipError("cannot NewPolynomialEvaluator: 3N rings are not supported (the CKKS evaluator needs a standard or conjugate-invariant ring)")
        self._table = None

    def _sim(self):
        return SimEvaluator(self.ev.ringQ.moduli, self.ev.nb_rescales)

    # ---- Evaluate :29-91 -------------------------------------------------------------------------------------------------------------------------
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
        if any(p.Lazy for p in polyVec.Value):
            raise RingHipError("cannot evaluate a polynomial with Lazy = true: the power basis then holds powers of mixed degrees, and the reference's "
                               "MulThenAdd drops the accumulator's third component when a relinearised power follows a lazy one (opOut.Resize(op0.Degree(), ...)): "
                               "there is nothing sound to match.  PowerBasis.GenPower(lazy=True) itself is supported")
        if polyVec.Mapping is not None:
            if self.ev.ringQ.kind == ConjugateInvariant:
                raise RingHipError("cannot evaluate a PolynomialVector on a conjugate-invariant ring: the encoder its per-slot coefficients go through is standard-only")
            if self.ev.encoder is None:
                raise RingHipError("cannot evaluate a PolynomialVector with a mapping: its per-slot coefficients need the CKKS encoder: build the evaluator with Evaluator(..., encoder=enc)")
            if self.ev.encoding_precision > 53:
                raise RingHipError("cannot evaluate a PolynomialVector with a mapping at encoding_precision %d > 53: the device encoder is the float64 path" % self.ev.encoding_precision)

    def Evaluate(self, ct, p, targetScale):
        """circuits/ckks/polynomial/polynomial_evaluator.go:42-57: P(ct) in ceil(log2(deg + 1)) levels.  A Chebyshev polynomial expects
        ct' = scalar ct + constant of ChangeOfBasis()."""
        polyVec = self._poly_vector(p)
        return self._evaluate(PowerBasis(ct, polyVec.Value[0].Basis), polyVec, targetScale)

    def EvaluateFromPowerBasis(self, pb, p, targetScale):
        """:62-81"""
        polyVec = self._poly_vector(p)
        if pb.Value.get(1) is None:
            raise RingHipError("cannot EvaluateFromPowerBasis: X^{1} is nil")
        return self._evaluate(pb, polyVec, targetScale)

    def _evaluate(self, powerbasis, polyVec, targetScale):
        ev = self.ev
        p0 = polyVec.Value[0]
        if p0.Degree() < 1:
            raise RingHipError("cannot evaluate poly: the degree must be at least 1")
        level, depth = powerbasis.Value[1].Level(), ev.nb_rescales * p0.Depth()
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
        PS = polyVec.PatersonStockmeyerPolynomial(self._sim(), X1.Level(), ev._scale(X1, "Evaluate"), Scale(targetScale))
        return self.EvaluatePatersonStockmeyerPolynomialVector(PS, powerbasis)

    # ---- :101-251 ------------------------------------------------------------------------------------------------------------------------------------
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
        polyVec = PolynomialVector([ps.Value[i] for ps in poly.Value], poly.Mapping)
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
        if not InDelta(ev._scale(a, "evalMonomial"), b.Scale, float(ScalePrecision - 12)):
            raise RingHipError("evalMonomial: scale discrepency: (rescale(b) * X^{n}).Scale = %s != a.Scale = %s" % (b.Scale, a.Scale))
        level = min(a.Level(), b.Level())
        if b.Level() != level:
            ev.DropLevel(b, b.Level() - level)
        ev.Add(b, _at_level(ev, a, level), b)

    # ---- EvaluatePolynomialVectorFromPowerBasis :254-359 -----------------------------------------------------------------------------------------------------
    def _zero(self, like, degree, level):
        """rlwe.NewCiphertext: x - x on the leading limbs of a block that is there already"""
        rq = self.ev.ringQ.AtLevel(level)
        out = Ciphertext([rq.NewPoly(like.npoly) for _ in range(degree + 1)], is_ntt=True)
        for p in out.Value:
            rq.Sub(like, like, p)
        return out

    def EvaluatePolynomialVectorFromPowerBasis(self, targetLevel, pol, pb, targetScale):
        """P(ct) = sum c_i ct^i from the powers at hand, at targetLevel and targetScale.  Without a mapping and with the fused path chosen it is
        ONE launch of rh_ckks_linear_combination, every term's scalars worked out as MulThenAdd would (:937-984); a term that would rescale the
        accumulator mid-sum (a power at the target scale with a constant that is no Gaussian integer) or a power below the target level sends
        the whole sum to the composed sequence of evaluator calls: the same bits.  (Below the target level the reference updates the limbs the
        power has and leaves the rest of the accumulator stale; here the accumulator is dropped to that level.)"""
        ev, X = self.ev, pb.Value
        self._refuse(pol)
        targetScale = Scale(targetScale)
        even, odd = pol.IsEven(), pol.IsOdd()
        p0 = pol.Value[0]
        minimumDegreeNonZeroCoefficient = len(p0.Coeffs) - 1
        if even and not odd:
            minimumDegreeNonZeroCoefficient -= 1
        used = lambda key: not (even or odd) or (key & 1 == 0 and even) or (key & 1 == 1 and odd)
        if minimumDegreeNonZeroCoefficient == 0:
            keys, degree = [], 1
        else:
            keys = [k for k in range(p0.Degree(), 0, -1) if used(k)]
            degree = max([X[k].Degree() for k in range(p0.Degree(), 0, -1) if X.get(k) is not None] or [0])
            for k in keys:
                if X.get(k) is None:
                    raise RingHipError("cannot EvaluatePolynomialVectorFromPowerBasis: X^{%d} is missing from the power basis" % k)
            if len({X[k].Degree() for k in keys}) > 1 or any(X[k].Degree() != degree for k in keys):
                raise RingHipError("cannot EvaluatePolynomialVectorFromPowerBasis: the powers have mixed degrees (a lazy power basis): the reference's MulThenAdd "
                                   "drops the accumulator's third component when a relinearised power follows a lazy one (opOut.Resize(op0.Degree(), ...)): "
                                   "there is nothing sound to match")
        if pol.Mapping is not None:
            coeff = lambda k: self.GetVectorCoefficient(pol, k)
        else:
            coeff = lambda k: self.GetSingleCoefficient(p0, k)
        res = None
        if pol.Mapping is None and ev._use("linear_combination"):
            res = self._fused(targetLevel, targetScale, keys, degree, coeff, even, X)
        if res is None:
            res = self._zero(X[1].Value[0], degree, targetLevel)
            res.Scale = targetScale
            if even:
                ev.Add(res, coeff(0), res)
            for k in keys:
                level = min(X[k].Level(), res.Level())
                if res.Level() != level:
                    ev.DropLevel(res, res.Level() - level)
                ev.MulThenAdd(_at_level(ev, X[k], level), coeff(k), res)
        _copy_meta(X[1], res)
        return res

    def _fused(self, targetLevel, targetScale, keys, degree, coeff, even, X):
        """the baby step as one launch, or None where it does not fit"""
        ev = self.ev
        prec = ev.encoding_precision
        s0, s1 = [], []
        for k in keys:
            if X[k].Level() < targetLevel:
                return None
            cmplx = to_complex(coeff(k), prec)
            cmp = ev._scale(X[k], "MulThenAdd").Cmp(targetScale)
            if cmp == 0:
                if cmplx[0].denominator != 1 or cmplx[1].denominator != 1:
                    return None
                scaleRLWE = Scale(1)
            elif cmp == -1:
                scaleRLWE = targetScale.Div(X[k].Scale)
            else:
                raise RingHipError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
            a, b = ev._rns_scalar(targetLevel, scaleRLWE, cmplx)
            s0.append(a)
            s1.append(b)
        c0 = c1 = None
        if even:
            c0, c1 = [_u64(v) for v in ev._rns_scalar(targetLevel, targetScale, to_complex(coeff(0), prec))]
        rq = ev.ringQ.AtLevel(targetLevel)
        npoly = X[1].Value[0].npoly
        res = Ciphertext([rq.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)
        res.Scale = targetScale
        self.linear_combination(targetLevel, [X[k].Value for k in keys], s0, s1, c0, c1, res.Value)
        return res

    def linear_combination(self, level, terms, s0, s1, c0, c1, outs):
        """rh_ckks_linear_combination: outs_j = [j == 0] c + sum_k s_k terms[k][j]; the device table is this evaluator's (one per evaluator, like
        the reference's buffers: an evaluator serves one thread)"""
        K, L = len(terms), lib()
        words = L.rh_ckks_linear_combination_table_words(K, level)
        if self._table is None or self._table.words < words:
            self._table = DevicePoly(outs[0].ring, 1, -(-words // outs[0].ring.N))
        x = (C.c_void_p * max(3 * K, 1))()
        rows = (C.c_int * max(K, 1))()
        for k, t in enumerate(terms):
            for j, p in enumerate(t):
                x[3 * k + j] = p.ptr
            rows[k] = t[0].limbs
        a = _u64(s0).reshape(-1) if K else None
        b = _u64(s1).reshape(-1) if K else None
        ptrs = [p.ptr for p in outs] + [None] * (3 - len(outs))
        _check(L.rh_ckks_linear_combination(outs[0].ring._h, level, K, x, rows, _p(a), _p(b), _p(_u64(c0)) if c0 is not None else None,
                                            _p(_u64(c1)) if c1 is not None else None, *ptrs, outs[0].npoly, self._table.ptr, self._table.words))

    # ---- CoefficientGetter (circuits/ckks/polynomial/polynomial_evaluator.go:85-114) ------------------------------------------------------------------------
    def GetSingleCoefficient(self, pol, k):
        return pol.Coeffs[k]

    def GetVectorCoefficient(self, pol, k):
        """the k-th coefficients over the slots as []complex128 (encoder.go:251-256 takes []*bignum.Complex to complex128; nil slots are zero)"""
        values = np.zeros(1 << self.ev.encoder.LogMaxSlots, dtype=np.complex128)
        for i, p in enumerate(pol.Value):
            c = p.Coeffs[k]
            for j in pol.Mapping.get(i, ()):
                values[j] = complex(c) if c is not None else 0
        return values

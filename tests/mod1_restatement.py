"""circuits/ckks/mod1 restated in plain Python over polynomial_restatement.py and ckks_restatement.py.  TEST INFRASTRUCTURE, written from the
reference, not from the package.

  mod1_parameters.go   the float64 half of NewParametersFromLiteral (:117-159: doubleAngle, K, qDiff, scaling, the arcsine series, sqrt2pi),
                       the nil-ing of the even or odd coefficients and the sqrt2pi factor (:171-211), Depth (:57-74)
  mod1_evaluator.go    EvaluateAndScaleNew (:31-144), one ciphertext at a time

The 256-bit Chebyshev coefficients themselves (cosine.ApproximateCos, bignum.ChebyshevApproximation) are GIVENS here: `params` takes them as
exact rationals from the caller, and tests/test_mod1_oracle.py pins the package's to the functions they approximate."""
import math
from fractions import Fraction

import ckks_restatement as cr
import polynomial_restatement as pr

COS_DISCRETE, SIN_CONTINUOUS, COS_CONTINUOUS = 0, 1, 2
PREC = 256                                                               # cosine.EncodingPrecision


class Params:
    pass


def depth(tp, K, degree, double_angle, inv_degree):
    """ParametersLiteral.Depth (:57-74)"""
    d = max(degree, 2 * K - 1).bit_length() if tp == COS_DISCRETE else degree.bit_length()
    if tp != SIN_CONTINUOUS:
        d += double_angle
    return d + inv_degree.bit_length()


def params(Q0, level_q, log_scale, tp, log_message_ratio, K, double_angle, inv_degree, coeffs, scaling=0.0):
    """NewParametersFromLiteral (:112-226) around the given coefficients (the Chebyshev coefficients of the approximation BEFORE the nil-ing and
    the sqrt2pi factor, as Fractions)"""
    e = Params()
    e.double_angle = 0 if tp == SIN_CONTINUOUS else double_angle          # :117-120
    sc_fac = 2.0 ** e.double_angle
    Ks = float(K) / sc_fac                                               # :124
    e.qdiff = float(Q0) / 2.0 ** math.floor(math.log2(float(Q0)) + 0.5)  # :127
    scaling = scaling if scaling != 0 else 1.0                           # :130-132
    e.inv_poly = None
    if inv_degree > 0:                                                   # :134-155
        e.sqrt2pi = 1.0
        co = [0.0] * (inv_degree + 1)
        co[1] = 0.15915494309189535 * (e.qdiff * scaling)
        for i in range(3, inv_degree + 1, 2):
            co[i] = co[i - 2] * (float(i * i - 4 * i + 4) / float(i * i - i))
        e.inv_poly = pr.Poly(pr.MONOMIAL, [None if i & 1 == 0 else (Fraction(c), Fraction(0)) for i, c in enumerate(co)])
        e.inv_poly.is_even = False
    else:
        e.sqrt2pi = math.pow(0.15915494309189535 * e.qdiff * scaling, 1.0 / sc_fac)   # :158
    s = Fraction(e.sqrt2pi)
    keep = 1 if tp == SIN_CONTINUOUS else 0                              # :171-199: the even (sine) or the odd (cosine) coefficients are nil
    co = [(cr.round_bits(Fraction(c) * s, PREC), Fraction(0)) if i & 1 == keep else None for i, c in enumerate(coeffs)]   # :205-211
    e.poly = pr.Poly(pr.CHEBYSHEV, co, (-Ks, Ks), PREC)
    if tp == SIN_CONTINUOUS:
        e.poly.is_even = False
    else:
        e.poly.is_odd = False
    e.interval_prec = PREC if tp != COS_DISCRETE else 53                 # the precision of Mod1Poly.A / B: bignum.Interval at 256 bits, or [2]float64
    e.level_q, e.log_scale, e.type, e.log_message_ratio, e.K = level_q, log_scale, tp, log_message_ratio, float(K)
    return e


def scale_sqrt(s):
    """big.Float.Sqrt on a Scale (mod1_evaluator.go:57): the square root rounded to 128 bits"""
    v = s.v
    t = 2 * cr.PREC + v.denominator.bit_length()
    scaled = v * (1 << (2 * t))
    r = math.isqrt(scaled.numerator // scaled.denominator)
    exact = r * r == scaled
    return cr.Scale(Fraction(2 * r + (0 if exact else 1), 1 << (t + 1)))


def scaled_poly(p, scaling):
    """Clone, then every coefficient times the complex128 `scaling` through bignum.ComplexMultiplier.Mul (:78-88, :124-134)"""
    sr, si = Fraction(scaling.real), Fraction(scaling.imag)
    r = lambda x: cr.round_bits(x, p.prec)
    q = pr.Poly(p.basis, [None if c is None else (r(r(c[0] * sr) - r(c[1] * si)), r(r(c[0] * si) + r(c[1] * sr))) for c in p.coeffs], (p.a, p.b), p.prec)
    q.is_odd, q.is_even = p.is_odd, p.is_even
    return q


def evaluate(P, ct, evm, scaling=1):
    """EvaluateAndScaleNew (:31-144).  P: polynomial_restatement.Params; ct: a polynomial_restatement.Ct at or above evm.level_q"""
    scaling = complex(scaling)
    assert ct.level() >= evm.level_q, "cannot Evaluate: ct.Level() < Mod1Parameters.LevelQ"      # :35-37
    level = evm.level_q                                                  # DropLevel (:39-41)
    res = pr.Ct([x[:level + 1].copy() for x in ct.comps], cr.Scale(2 ** evm.log_scale))         # CopyNew; res.Scale = ScalingFactor() (:43-46)
    target = res.scale
    for i in range(evm.double_angle):                                    # :54-58
        target = scale_sqrt(target.mul(cr.Scale(P.Q[level - evm.poly.depth() - evm.double_angle + i + 1])))
    if evm.type in (COS_DISCRETE, COS_CONTINUOUS):                       # :61-68
        offset = cr.round_bits((evm.poly.b - evm.poly.a) * Fraction(2.0 ** evm.double_angle), evm.interval_prec)
        offset = cr.round_bits(Fraction(-1, 2) / offset, evm.interval_prec)
        pr.add_const(P, res, (offset, Fraction(0)))
    sqrt2pi = complex(evm.sqrt2pi, 0)                                    # :71
    if evm.inv_poly is None:                                             # :74-94
        if scaling != 1:
            scaling = scaling ** complex(1 / 2.0 ** evm.double_angle, 0)   # cmplx.Pow, a given for a non-trivial scaling
        poly = scaled_poly(evm.poly, scaling)
        sqrt2pi *= scaling
    else:
        poly = evm.poly
    res = pr.evaluate(P, res, [poly], None, target)                      # :97
    for _ in range(evm.double_angle):                                    # :101-119
        sqrt2pi *= sqrt2pi
        res = pr.mul_new(P, res, res, True)
        pr.add_sub(P, res, res)
        pr.add_const(P, res, (Fraction(-sqrt2pi.real), Fraction(-sqrt2pi.imag)))
        pr.rescale(P, res)
    if evm.inv_poly is not None:                                         # :122-139
        res = pr.evaluate(P, res, [scaled_poly(evm.inv_poly, scaling)], None, res.scale)
    res.scale = ct.scale                                                 # :142
    return res

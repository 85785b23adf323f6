"""Host-side mirror of circuits/ckks/mod1, homomorphic x mod 1 for CKKS bootstrapping, on device-resident batches: the parameters, the
coefficients of the approximating polynomials (on the host, at 256 bits) and the evaluator's call sequence.  The arithmetic is the device
evaluator's (ckks.Evaluator, polynomial.PolynomialEvaluator) and, for a double-angle round, one launch of rh_ckks_double_angle
(csrc/bootstrap.hip).

  circuits/ckks/mod1/mod1_parameters.go   Type :18-26   ParametersLiteral :32-74   Parameters :77-108   NewParametersFromLiteral :112-226
  circuits/ckks/mod1/mod1_evaluator.go    EvaluateAndScaleNew :31-144   EvaluateNew :160-162
  utils/cosine/cosine_approx.go           ApproximateCos :30-40   genDegrees :81-158   genNodes :160-234   solve :236-377
  utils/bignum/chebyshev_approximation.go ChebyshevApproximation :15-51   chebyshevNodes :53-79   chebyCoeffs :81-148

The coefficients are GIVENS in the sense of DESIGN.md section 5: they are computed here step for step as the reference computes them, every
operation rounded to 256 bits (cosine.EncodingPrecision), but through mpmath's cosine, sine and pi, which may differ from Go's bignum.Sin /
bignum.Cos in the last bits of 256; Sqrt2Pi goes through libm's pow and cmplx.Pow of a non-trivial `scaling` through Python's complex power.
A caller that needs a Go run's bits passes its own: Parameters(Mod1Poly=..., Mod1InvPoly=..., Sqrt2Pi=...).  With scaling = 1 the scaling
step is exact.  A batch of npoly ciphertexts is one Ciphertext; all of them share level and scale."""
import copy
import json
import math
from fractions import Fraction

from .ckks import Complex, Scale, ScalePrecision, to_complex, _round
from .polynomial import Chebyshev, Monomial, Polynomial, _copy_new, _rescale
from .ringhip import RingHipError, _check, _p, _u64, lib

CosDiscrete, SinContinuous, CosContinuous = 0, 1, 2       # mod1.Type (:22-26)
EncodingPrecision = 256                                   # cosine.EncodingPrecision
_INV_2PI = 0.15915494309189535                            # the literal of :140, :158


def _go_float(x):
    """encoding/json's float64: the shortest decimal that round-trips, without exponent for 1e-6 <= |x| < 1e21"""
    x = float(x)
    if x == int(x) and abs(x) < 1e21:
        return "%d" % int(x)
    r = repr(x)
    if "e" in r and 1e-6 <= abs(x) < 1e21:
        r = ("%.17f" % x).rstrip("0")
    return r


class ParametersLiteral:
    """mod1.ParametersLiteral (:32-42)"""
    _FIELDS = ("LevelQ", "LogScale", "Mod1Type", "Scaling", "LogMessageRatio", "K", "Mod1Degree", "DoubleAngle", "Mod1InvDegree")

    def __init__(self, LevelQ=0, LogScale=0, Mod1Type=CosDiscrete, Scaling=0.0, LogMessageRatio=0, K=0, Mod1Degree=0, DoubleAngle=0, Mod1InvDegree=0):
        self.LevelQ, self.LogScale, self.Mod1Type, self.Scaling = int(LevelQ), int(LogScale), int(Mod1Type), float(Scaling)
        self.LogMessageRatio, self.K, self.Mod1Degree = int(LogMessageRatio), int(K), int(Mod1Degree)
        self.DoubleAngle, self.Mod1InvDegree = int(DoubleAngle), int(Mod1InvDegree)

    def __eq__(self, other):
        return isinstance(other, ParametersLiteral) and all(getattr(self, f) == getattr(other, f) for f in self._FIELDS)

    def __repr__(self):
        return "mod1.ParametersLiteral(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in self._FIELDS)

    def Depth(self):
        """:57-74"""
        if self.Mod1Type == CosDiscrete:                                           # this method requires a minimum degree of 2*K-1
            depth = max(self.Mod1Degree, 2 * self.K - 1).bit_length()
        else:
            depth = self.Mod1Degree.bit_length()
        if self.Mod1Type != SinContinuous:
            depth += self.DoubleAngle
        return depth + self.Mod1InvDegree.bit_length()

    def MarshalBinary(self):
        """:46-48: encoding/json of the struct, fields in declaration order"""
        return ("{" + ",".join('"%s":%s' % (f, _go_float(getattr(self, f)) if f == "Scaling" else "%d" % getattr(self, f)) for f in self._FIELDS) + "}").encode()

    def UnmarshalBinary(self, data):
        """:52-54: fields the JSON does not name keep their values"""
        d = json.loads(data.decode() if isinstance(data, (bytes, bytearray)) else data)
        for f in self._FIELDS:
            if f in d:
                setattr(self, f, float(d[f]) if f == "Scaling" else int(d[f]))
        return self


# ---- the coefficients, on the host at 256 bits ----------------------------------------------------------------------------------------------
def _ctx(prec=EncodingPrecision):
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = int(prec)
    return mp


def _frac(x):
    """an mpf as the exact rational it is"""
    sign, man, exp, _ = x._mpf_
    v = Fraction(int(man)) * (Fraction(2) ** int(exp))
    return -v if sign else v


def _go_log2(x):
    """math.Log2 (log10.go): Frexp, exact at powers of two, else Log(frac) * (1 / Ln2) + exp"""
    frac, exp = math.frexp(x)
    if frac == 0.5:
        return float(exp - 1)
    return math.log(frac) * (1 / math.log(2.0)) + float(exp)


def _go_round(x):
    """math.Round: half away from zero"""
    return math.copysign(math.floor(abs(x) + 0.5), x)


def genDegrees(degree, K, dev):
    """cosine_approx.go:81-158, float64 as written: the number of nodes of each interval [i +/- 1/dev], 0 <= i < K, and their total"""
    log2 = _go_log2
    log2TwoPi = log2(2 * math.pi)
    degbdd, totdeg, err = degree + 1, 2 * K - 1, 1.0 / dev
    deg = [1] * K
    temp = 0.0
    for i in range(1, 2 * K):
        temp -= log2(float(i))
    temp += (2 * float(K) - 1) * log2TwoPi
    temp += log2(err)
    bdd = [0.0] * K
    for i in range(K):
        bdd[i] = temp
        for j in range(1, K - 1 - i + 1):
            bdd[i] += log2(float(j) + err)
        for j in range(1, K - 1 + i + 1):
            bdd[i] += log2(float(j) + err)
    for _ in range(200):
        if totdeg >= degbdd:
            break
        maxi = 0                                                                   # maxIndex :67-77: the first of the largest
        for i in range(1, K):
            if bdd[i] > bdd[maxi]:
                maxi = i
        if maxi != 0:
            if totdeg + 2 > degbdd:
                break
            for i in range(K):
                bdd[i] -= log2(float(totdeg + 1))
                bdd[i] -= log2(float(totdeg + 2))
                bdd[i] += 2.0 * log2TwoPi
                if i != maxi:
                    bdd[i] += log2(abs(float(i - maxi)) + err)
                    bdd[i] += log2(float(i + maxi) + err)
                else:
                    bdd[i] += log2(err) - 1.0
                    bdd[i] += log2(2.0 * float(i) + err)
            totdeg += 2
        else:
            bdd[0] -= log2(float(totdeg + 1))
            bdd[0] += log2(err) - 1.0
            bdd[0] += log2TwoPi
            for i in range(1, K):
                bdd[i] -= log2(float(totdeg + 1))
                bdd[i] += log2TwoPi
                bdd[i] += log2(float(i) + err)
            totdeg += 1
        deg[maxi] += 1
    return deg, totdeg


def ApproximateCos(K, degree, dev, scnum):
    """cosine.ApproximateCos (:30-40): the Chebyshev coefficients, on [-K / 2^scnum, K / 2^scnum], of the polynomial that interpolates
    cos(2 pi x) at the images (t - 0.25) / 2^scnum of the Han-Ki nodes t -- the nodes are shifted in place by cos2PiXMinusQuarterOverR
    (:43-57), which is why the evaluator subtracts 0.25 / K first.  Returns exact rationals of 256-bit values."""
    mp = _ctx()
    mpf, pi = mp.mpf, +mp.pi
    deg, totdeg = genDegrees(degree, K, dev)
    # genNodes :160-234
    scfac, intersize = mpf(1 << scnum), mpf(1.0 / dev)
    nodes = [mpf(0)] * totdeg
    cnt = 1 if deg[0] % 2 else 0
    for i in range(K - 1, 0, -1):
        twodegi, iF = mpf(2 * deg[i]), mpf(i)
        for j in range(deg[i]):
            tmp = mp.cos(pi * mpf(2 * j) / twodegi) * intersize
            nodes[cnt] = iF + tmp
            nodes[cnt + 1] = -nodes[cnt]
            cnt += 2
    twodegi = mpf(2 * deg[0])
    for j in range(deg[0] // 2):
        tmp = mp.cos(pi * mpf(2 * j) / twodegi) * intersize
        nodes[cnt] = tmp
        nodes[cnt + 1] = -tmp
        cnt += 2
    twopi = mpf(2) * pi
    y = [None] * totdeg
    for i in range(totdeg):
        nodes[i] = (nodes[i] - mpf(0.25)) / scfac                                  # x.Sub(x, aQuarter); x.Quo(x, r): in place
        y[i] = mp.cos(twopi * nodes[i])
    # solve :236-377: divided differences, then the values at the Chebyshev points of [-K / 2^r, K / 2^r], then the pivoted elimination
    for j in range(1, totdeg):
        for i in range(totdeg - j):
            y[i] = (y[i + 1] - y[i]) / (nodes[i + j] - nodes[i])
    n = totdeg + 1
    Kr = mpf(float(K)) / scfac
    x = [Kr * mp.cos(mpf(i) * pi / mpf(n - 1)) for i in range(n)]
    p = []
    for i in range(n):
        v = y[0]
        for j in range(1, n - 1):
            v = v * (x[i] - nodes[j]) + y[j]
        p.append(v)
    KBig = mpf(K)
    T = [[None] * n for _ in range(n)]
    for i in range(n):
        T[i][0] = mpf(1)
        T[i][1] = x[i] / (KBig / scfac)
        for j in range(2, n):
            T[i][j] = mpf(2) * (x[i] / (KBig / scfac)) * T[i][j - 1] - T[i][j - 2]
    for i in range(n - 1):
        maxabs, maxindex = abs(T[i][i]), i
        for j in range(i + 1, n):
            if abs(T[j][i]) > maxabs:
                maxabs, maxindex = abs(T[j][i]), j
        if i != maxindex:
            T[maxindex][i:], T[i][i:] = T[i][i:], T[maxindex][i:]
            p[maxindex], p[i] = p[i], p[maxindex]
        for j in range(i + 1, n):
            T[i][j] = T[i][j] / T[i][i]
        p[i] = p[i] / T[i][i]
        T[i][i] = mpf(1)
        for j in range(i + 1, n):
            p[j] = p[j] - T[j][i] * p[i]
            for l in range(i + 1, n):
                T[j][l] = T[j][l] - T[j][i] * T[i][l]
            T[j][i] = mpf(0)
    c = [None] * n
    c[n - 1] = p[n - 1]
    for i in range(n - 2, -1, -1):
        c[i] = p[i]
        for j in range(i + 1, n):
            c[i] = c[i] - T[i][j] * c[j]
    return [_frac(v) for v in c[:totdeg]]


def ChebyshevApproximation(name, nodes, K):
    """bignum.ChebyshevApproximation (:15-51) of sin2pi / cos2pi (mod1_parameters.go:228-241) on [-K, K] with Nodes = `nodes`: nodes + 1
    coefficients, exact rationals of 256-bit values"""
    mp = _ctx()
    mpf, pi = mp.mpf, +mp.pi
    f = {"sin2pi": mp.sin, "cos2pi": mp.cos}[name]
    A, B = mpf(-float(K)), mpf(float(K))
    n = nodes + 1
    # chebyshevNodes :53-79
    half = mpf(0.5)
    xm, ym = (A + B) * half, (B - A) * half
    PiOverN = pi / mpf(n)
    xs = [None] * n
    for k in range(1, n + 1):
        xs[n - k] = mp.cos(mpf(float(k) - 0.5) * PiOverN) * ym + xm
    fi = [f(x * mpf(2) * pi) for x in xs]
    # chebyCoeffs :81-148 (real values: the imaginary parts stay zero)
    two, minusab, bminusa = mpf(2), -A - B, B - A
    coeffs = [mpf(0)] * n
    for i in range(n):
        u = (xs[i] * two + minusab) / bminusa
        Tprev, T = mpf(1), u
        for j in range(n):
            coeffs[j] = coeffs[j] + fi[i] * Tprev
            Tnext = (u * T) * two - Tprev
            Tprev, T = T, Tnext
    NHalf = mpf(n)
    coeffs[0] = coeffs[0] / NHalf
    NHalf = NHalf / two
    for i in range(1, n):
        coeffs[i] = coeffs[i] / NHalf
    return [_frac(v) for v in coeffs]


class Parameters:
    """mod1.Parameters (:77-88).  Mod1Poly / Mod1InvPoly: polynomial.Polynomial (prec 256 for Mod1Poly, nil coefficients as None)."""

    def __init__(self, LevelQ, LogDefaultScale, Mod1Type, LogMessageRatio, DoubleAngle, QDiff, Sqrt2Pi, Mod1Poly, Mod1InvPoly=None, K=0.0):
        self.LevelQ, self.LogDefaultScale, self.Mod1Type = int(LevelQ), int(LogDefaultScale), int(Mod1Type)
        self.LogMessageRatio, self.DoubleAngle = int(LogMessageRatio), int(DoubleAngle)
        self.QDiff, self.Sqrt2Pi, self.K = float(QDiff), float(Sqrt2Pi), float(K)
        self.Mod1Poly, self.Mod1InvPoly = Mod1Poly, Mod1InvPoly

    def IntervalShrinkFactor(self):
        return math.ldexp(1.0, self.DoubleAngle)

    def KShrinked(self):
        return self.K / self.IntervalShrinkFactor()

    def ScalingFactor(self):
        return Scale(1 << self.LogDefaultScale) if self.LogDefaultScale >= 0 else Scale(math.ldexp(1.0, self.LogDefaultScale))

    def MessageRatio(self):
        return float(1 << self.LogMessageRatio)


def _drop(poly, parity):
    """the coefficients of the given parity set to nil (:151-155, :171-175 ...)"""
    for i in range(len(poly.Coeffs)):
        if i & 1 == parity:
            poly.Coeffs[i] = None


def NewParametersFromLiteral(Q0, evm):
    """:112-226.  Q0: the first modulus of the chain (params.Q()[0])"""
    if evm.Mod1Type not in (CosDiscrete, SinContinuous, CosContinuous):
        raise RingHipError("invalid Mod1Type")
    doubleAngle = 0 if evm.Mod1Type == SinContinuous else evm.DoubleAngle
    scFac = math.ldexp(1.0, doubleAngle)
    K = float(evm.K) / scFac
    Q = int(Q0)
    qDiff = float(Q) / math.ldexp(1.0, int(_go_round(_go_log2(float(Q)))))
    scaling = evm.Scaling if evm.Scaling != 0 else 1.0
    mod1InvPoly = None
    if evm.Mod1InvDegree > 0:
        sqrt2pi = 1.0
        coeffs = [0j] * (evm.Mod1InvDegree + 1)
        coeffs[1] = complex(_INV_2PI * (qDiff * scaling), 0.0)
        for i in range(3, evm.Mod1InvDegree + 1, 2):
            coeffs[i] = complex(coeffs[i - 2].real * (float(i * i - 4 * i + 4) / float(i * i - i)), 0.0)
        mod1InvPoly = Polynomial(Monomial, coeffs)
        mod1InvPoly.IsEven = False
        _drop(mod1InvPoly, 0)
    else:
        sqrt2pi = math.pow(_INV_2PI * qDiff * scaling, 1.0 / scFac)
    if evm.Mod1Type == SinContinuous:
        mod1Poly = Polynomial(Chebyshev, [Complex(c, 0) for c in ChebyshevApproximation("sin2pi", evm.Mod1Degree, K)], (-K, K), prec=EncodingPrecision)
        mod1Poly.IsEven = False
        _drop(mod1Poly, 0)
    elif evm.Mod1Type == CosDiscrete:
        c = ApproximateCos(evm.K, evm.Mod1Degree, float(1 << evm.LogMessageRatio), doubleAngle)
        mod1Poly = Polynomial(Chebyshev, [Complex(v, 0) for v in c], (-K, K), prec=EncodingPrecision)
        mod1Poly.IsOdd = False
        _drop(mod1Poly, 1)
    else:
        mod1Poly = Polynomial(Chebyshev, [Complex(c, 0) for c in ChebyshevApproximation("cos2pi", evm.Mod1Degree, K)], (-K, K), prec=EncodingPrecision)
        mod1Poly.IsOdd = False
        _drop(mod1Poly, 1)
    s = Fraction(sqrt2pi)                                                            # Coeffs[i][0].Mul(Coeffs[i][0], sqrt2piBig): rounded to the coefficient's 256 bits (:205-211)
    mod1Poly.Coeffs = [None if c is None else Complex(_round(c.re * s, EncodingPrecision), _round(c.im * s, EncodingPrecision)) for c in mod1Poly.Coeffs]
    return Parameters(evm.LevelQ, evm.LogScale, evm.Mod1Type, evm.LogMessageRatio, doubleAngle, qDiff, sqrt2pi, mod1Poly, mod1InvPoly, float(evm.K))


# ---- the evaluator ------------------------------------------------------------------------------------------------------------------------
def ScaleSqrt(scale):
    """big.Float.Sqrt at ScalePrecision bits (:57): the square root of a Scale, correctly rounded, half to even"""
    v = Scale(scale).Value
    t = ScalePrecision + 8 + v.denominator.bit_length()
    num = (v.numerator << (2 * t)) // v.denominator
    R = math.isqrt(num)
    sticky = 0 if R * R == num and (v.numerator << (2 * t)) % v.denominator == 0 else 1
    return Scale(_round(Fraction(2 * R + sticky, 1 << (t + 1)), ScalePrecision))


def _scaled(poly, scaling):
    """poly.Clone() with every coefficient multiplied by the complex128 `scaling` through bignum's ComplexMultiplier (:78-88, :124-134): four
    products, a difference and a sum, each rounded to the coefficient's precision"""
    sr, si = Fraction(scaling.real), Fraction(scaling.imag)
    out = copy.copy(poly)
    r = lambda v: _round(v, poly.prec)
    out.Coeffs = [None if c is None else Complex(r(r(c.re * sr) - r(c.im * si)), r(r(c.re * si) + r(c.im * sr))) for c in poly.Coeffs]
    return out


class Evaluator:
    """mod1.Evaluator over a ckks.Evaluator and a polynomial.PolynomialEvaluator.  fused: None what FUSED_BOOTSTRAP says, else True / False
    for every kernel: the double-angle round as one launch of rh_ckks_double_angle, or as the reference's two Adds -- the same bits."""

    # profiles/bootstrap.json (fused_bootstrap_default): the double-angle kernel is within the run-to-run spread of the two Adds in the whole EvalMod at
    # batch 1 (composed / fused 1.003) and undecided at batch 8 (bimodal windows on both sides); the scalar folded into the ModUp kernel is 1.19x / 1.21x
    # faster than MulScalar after the NTT
    FUSED_BOOTSTRAP = {"double_angle": True, "modup_scale": True}

    def __init__(self, ckks_evaluator, polynomial_evaluator, parameters, fused=None):
        self.ev, self.PolynomialEvaluator, self.Parameters = ckks_evaluator, polynomial_evaluator, parameters
        self.fused = dict(self.FUSED_BOOTSTRAP) if fused is None else {k: bool(fused) for k in self.FUSED_BOOTSTRAP}

    def EvaluateNew(self, ct):
        """:160-162"""
        return self.EvaluateAndScaleNew(ct, 1)

    def _double_angle(self, res, c):
        """Add(res, res, res); Add(res, c, res) (:108-114)"""
        ev = self.ev
        if not self.fused["double_angle"]:
            ev.Add(res, res, res)
            ev.Add(res, c, res)
            return
        level = ev._operands("Add", res)
        if res.Degree() != 1:
            raise RingHipError("cannot Evaluate: the double-angle round needs a ciphertext of degree 1")
        s0, s1 = ev._rns_scalar(level, ev._scale(res, "Add"), to_complex(c, ev.encoding_precision))
        a, b = _u64(s0), _u64(s1)
        _check(lib().rh_ckks_double_angle(ev.ringQ._h, level, res.Value[0].ptr, res.Value[1].ptr, res.Value[0].npoly, _p(a), _p(b)))

    def EvaluateAndScaleNew(self, ct, scaling):
        """:31-144.  As in the reference, a ciphertext above Parameters.LevelQ is itself dropped to it."""
        ev, evm = self.ev, self.Parameters
        scaling = complex(scaling)
        if ct.Level() < evm.LevelQ:
            raise RingHipError("cannot Evaluate: ct.Level() < Mod1Parameters.LevelQ")
        if ct.Level() > evm.LevelQ:
            ev.DropLevel(ct, ct.Level() - evm.LevelQ)
        ctScale = ev._scale(ct, "Evaluate")
        res = _copy_new(ct)
        res.Scale = evm.ScalingFactor()                                            # normalize the modular reduction to mod by 1 (:46)
        Qi = [int(q) for q in ev.ringQ.moduli]
        targetScale = res.Scale                                                    # the scale before the double angle such that after it it is res.Scale (:54-58)
        for i in range(evm.DoubleAngle):
            targetScale = ScaleSqrt(targetScale.Mul(Scale(Qi[ct.Level() - evm.Mod1Poly.Depth() - evm.DoubleAngle + i + 1])))
        if evm.Mod1Type in (CosDiscrete, CosContinuous):                           # division by 1/2^r and change of variable (:61-68)
            p = evm.Mod1Poly.prec if evm.Mod1Type == CosContinuous else 53         # the precision of Mod1Poly.B - Mod1Poly.A: ChebyshevApproximation's interval, or [2]float64
            offset = _round((evm.Mod1Poly.B - evm.Mod1Poly.A) * Fraction(evm.IntervalShrinkFactor()), p)
            offset = _round(Fraction(-1, 2) / offset, p)
            ev.Add(res, offset, res)
        sqrt2pi = complex(evm.Sqrt2Pi, 0)
        if evm.Mod1InvPoly is None:
            scaling = scaling ** complex(1 / evm.IntervalShrinkFactor(), 0) if scaling != 1 else scaling     # cmplx.Pow (:76); exactly 1 for 1
            mod1Poly = _scaled(evm.Mod1Poly, scaling)
            sqrt2pi *= scaling
        else:
            mod1Poly = evm.Mod1Poly
        res = self.PolynomialEvaluator.Evaluate(res, mod1Poly, targetScale)        # Chebyshev evaluation (:97)
        for _ in range(evm.DoubleAngle):                                           # (:101-119)
            sqrt2pi *= sqrt2pi
            ev.MulRelin(res, res, res)
            self._double_angle(res, -sqrt2pi)
            _rescale(ev, res)
        if evm.Mod1InvPoly is not None:                                            # arcsine (:122-139)
            res = self.PolynomialEvaluator.Evaluate(res, _scaled(evm.Mod1InvPoly, scaling), ev._scale(res, "Evaluate"))
        res.Scale = ctScale                                                        # multiplies back by q (:142)
        return res

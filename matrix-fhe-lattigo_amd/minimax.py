"""Host-side mirror of circuits/ckks/minimax, composite minimax polynomials on device-resident batches: the arithmetic is the device
evaluators' (ckks.Evaluator, polynomial.PolynomialEvaluator) and the bootstrapper's.

  minimax_composite_polynomial.go            NewPolynomial :18-38   MaxDepth :40-45   Evaluate :47-55   CoeffsSignX2Cheby / X4Cheby :64, :73
                                             parseCoeffs :244-259
  minimax_composite_polynomial_evaluator.go  NewEvaluator :24-26    Evaluate :29-89

A batch of npoly ciphertexts is one Ciphertext; all of them share the level and the scale.  A bootstrapper is any object with Bootstrap,
MinimumInputLevel, OutputLevel and Depth (bootstrapping.Evaluator, bootstrapping.SecretKeyBootstrapper).  None counts as minimum input
level 0 and raises by name where the reference would call it (the reference dereferences nil there).

Not built: the Remez generator (GenMinimaxCompositePolynomial, GenMinimaxCompositePolynomialForSign, PrettyPrintCoefficients) -- composite
polynomials are given as coefficient tables, as the reference's own default is.  Refused by name: conjugate-invariant and 3N rings."""
import json
from fractions import Fraction

from . import polynomial
from .ckks import Complex, Scale, GaloisElementOrderTwoOrthogonalSubgroup, _round
from .ringhip import RingHipError, Standard
from .schemes import Ciphertext

# What profiles/minimax.json measured decides ("fused_minimax_default": both faster than composed at batches of 1 and 8); every choice gives
# the same bits.
#   affine         constant - x (the 2 - x, 1 - x, 1 - z^2 of the inverse circuits) as one launch of rh_ckks_axpby, or Mul(-1) and Add
#   conjugate_add  res + Conjugate(res) as GadgetProductThenAdd and rh_rlwe_rotate_add_q in place, or ConjugateNew and Add
FUSED_MINIMAX = {"affine": True, "conjugate_add": True}


def _decimal(c):
    """a decimal string as big.Float.SetString reads it -> Fraction"""
    try:
        return Fraction(c.strip())
    except ValueError:
        raise RingHipError("cannot NewPolynomial: %r is not a decimal number" % (c,)) from None


def parseCoeffs(coeffs):
    """:244-259 -> (Fractions, prec): strings are read at round(3.32... x the longest string's length) bits, the reference's rule.  A row of
    floats is taken at 53 bits, a row of mpmath values at the longest mantissa among them (53 at least): both exactly."""
    coeffs = list(coeffs)
    if all(isinstance(c, str) for c in coeffs):
        prec = int(float(max([len(c) for c in coeffs] + [0])) * 3.3219280948873626 + 0.5)
        return [_round(_decimal(c), prec) for c in coeffs], prec
    vals, prec = [], 53
    for c in coeffs:
        if hasattr(c, "_mpf_"):                                                    # mpmath.mpf: (sign, mantissa, exponent, bit count)
            sign, man, exp, bc = c._mpf_
            vals.append((-1 if sign else 1) * Fraction(int(man)) * Fraction(2) ** int(exp))
            prec = max(prec, int(bc))
        elif isinstance(c, (int, float, Fraction)) and not isinstance(c, bool):
            vals.append(Fraction(c))
        else:
            raise RingHipError("cannot NewPolynomial: a row holds str, float or mpmath values, not a mix with %s" % type(c).__name__)
    return [_round(v, prec) for v in vals], prec


class Polynomial(list):
    """minimax.Polynomial: P = p_k o ... o p_1 o p_0, a list of polynomial.Polynomial in the Chebyshev basis on [-1, 1]"""

    def __init__(self, coeffs=()):
        list.__init__(self)
        for row in coeffs:
            if isinstance(row, polynomial.Polynomial):
                self.append(row)
                continue
            vals, prec = parseCoeffs(row)
            self.append(polynomial.Polynomial(polynomial.Chebyshev, [Complex(v, 0) for v in vals], (-1, 1), prec=prec))

    @classmethod
    def from_json(cls, path, append=()):
        """a JSON list of coefficient rows (strings); `append`: further rows, composed after them"""
        with open(path) as f:
            rows = json.load(f)
        return cls(list(rows) + list(append))

    def MaxDepth(self):
        return max([p.Depth() for p in self] + [0])

    def Evaluate(self, x):
        """:47-55 on the host: every polynomial in exact rationals (polynomial.Polynomial.Evaluate), its value rounded to 256 bits before
        the next one takes it (the reference rounds every step to the precision of x; exact composites grow without bound)"""
        y = self[0].Evaluate(x)
        for p in self[1:]:
            y = p.Evaluate(Complex(_round(y.re, 256), _round(y.im, 256)))
        return y


def _chebyshev_of_monomial(mono):
    """the Chebyshev coefficients, as the decimal strings the reference lists, of sum mono[i] x^i on [-1, 1]: Horner in the Chebyshev basis
    (x T_k = (T_k+1 + T_|k-1|) / 2) after the affine map of Polynomial.ChangeOfBasis"""
    scalar, constant = polynomial.Polynomial(polynomial.Chebyshev, [0, 1], (-1, 1)).ChangeOfBasis()      # t = scalar x + constant

    def times_x(c):                                                                # x = (t - constant) / scalar
        out = [Fraction(0)] * (len(c) + 1)
        for k, v in enumerate(c):
            out[k + 1] += v / 2
            out[abs(k - 1)] += v / 2
            out[k] -= constant * v
        return [v / scalar for v in out]
    acc = [Fraction(0)]
    for m in reversed(mono):
        acc = times_x(acc)
        acc[0] += Fraction(m)
    while len(acc) > 1 and acc[-1] == 0:
        acc.pop()
    out = []
    for v in acc:
        digits = 0
        while (v * 10 ** digits).denominator != 1:                                 # dyadic values: the exact decimal expansion
            digits += 1
            if digits > 64:
                raise RingHipError("no finite decimal expansion")
        n = int(abs(v) * 10 ** digits)
        s = "%d" % n if digits == 0 else "%d.%0*d" % (n // 10 ** digits, digits, n % 10 ** digits)
        out.append(("-" if v < 0 else "") + s)
    return out


# 3/2 x - 1/2 x^3 and 35/16 x - 35/16 x^3 + 21/16 x^5 - 5/16 x^7 (https://eprint.iacr.org/2019/1234): composed after a sign polynomial, each
# evaluation about doubles / quadruples the number of correct bits
CoeffsSignX2Cheby = _chebyshev_of_monomial([0, Fraction(3, 2), 0, Fraction(-1, 2)])
CoeffsSignX4Cheby = _chebyshev_of_monomial([0, Fraction(35, 16), 0, Fraction(-35, 16), 0, Fraction(21, 16), 0, Fraction(-5, 16)])


def min_level(btp):
    return 0 if btp is None else btp.MinimumInputLevel()


def bootstrap(btp, ct, who):
    if btp is None:
        raise RingHipError("cannot %s: the ciphertext is at level %d, which needs a bootstrapping, and the bootstrapper is nil" % (who, ct.Level()))
    return btp.Bootstrap(ct)


def at_common_level(ev, a, b):
    """the two operands as the reference reads them at min(a.Level(), b.Level())"""
    level = min(a.Level(), b.Level())
    return polynomial._at_level(ev, a, level), polynomial._at_level(ev, b, level)


class Evaluator:
    """minimax.Evaluator.  ckks_evaluator brings the rings, the keys (the conjugation's among them) and levels_consumed_per_rescaling;
    default_scale is Parameters.DefaultScale().  fused: None what FUSED_MINIMAX says, else True / False for every choice."""

    def __init__(self, ckks_evaluator, bootstrapper, default_scale, fused=None):
        ev = self.ev = ckks_evaluator
        if ev.ringQ.kind != Standard:
            raise RingHipError("cannot NewEvaluator: the minimax circuits are built for standard rings (conjugate-invariant and 3N rings are not supported)")
        self.PolyEval = polynomial.PolynomialEvaluator(ev)
        self.BtsEval = bootstrapper
        self.DefaultScale = Scale(default_scale)
        self.fused = dict(FUSED_MINIMAX) if fused is None else {k: bool(fused) for k in FUSED_MINIMAX}

    def MaxLevel(self):
        return self.ev.ringQ.L - 1

    def Evaluate(self, ct, mcp):
        """:29-89"""
        ev, btp, nb = self.ev, self.BtsEval, self.ev.nb_rescales
        maxDepth = mcp.MaxDepth() * nb
        if self.MaxLevel() < maxDepth + min_level(btp):
            raise RingHipError("parameters do not enable the evaluation of the minimax composite polynomial, required levels is %d but parameters only provide %d levels"
                               % (maxDepth + min_level(btp), self.MaxLevel()))
        res = polynomial._copy_new(ct)
        for poly in mcp:
            if res.Level() < poly.Depth() * nb + min_level(btp):
                res = bootstrap(btp, res, "Evaluate")
            targetScale = self.DefaultScale.Div(Scale(2))                          # so that x + conj(x) has the scale wanted (:56-61)
            try:
                res = self.PolyEval.Evaluate(res, poly, targetScale)
            except RingHipError as e:
                raise RingHipError("evaluate polynomial: %s" % e) from None
            res.Scale = res.Scale.Mul(Scale(2))                                    # (:72)
            self._add_conjugate(res)
        res.Scale = ct.Scale                                                       # avoids float errors (:86)
        return res

    def _add_conjugate(self, res):
        """res += Conjugate(res): cleans the imaginary part (:74-81)"""
        ev = self.ev
        galEl = GaloisElementOrderTwoOrthogonalSubgroup(ev.ringQ.N)
        evk = ev.ks.galois_keys.get(galEl) if ev.ks is not None else None
        # the fused product takes keys with more than one P modulus; a missing key, or one generated below the ciphertext's level, is
        # ConjugateNew's to refuse or to handle, as it does on the composed path
        if not self.fused["conjugate_add"] or evk is None or evk.LevelP() < 1 or evk.LevelQ() < res.Level():
            ev.Add(res, ev.ConjugateNew(res), res)
            return
        level, ks = ev._operands("Conjugate", res), ev.ks
        ev._scale(res, "Conjugate")
        rq, npoly = ev.ringQ.AtLevel(level), res.Value[0].npoly
        tmp = Ciphertext([ks.buffer("auto0", rq, npoly, level + 1), ks.buffer("auto1", rq, npoly, level + 1)], is_ntt=True)
        ks.GadgetProductThenAdd(level, res.Value[1], evk, res.Value[0], None, tmp)
        ks.RotateAddQ(level, galEl, tmp, res)

"""Host-side mirror of circuits/ckks/comparison/comparison.go, homomorphic comparisons on device-resident batches, over minimax.Evaluator:

  NewEvaluator :37-51   Sign :75-77   Step :81-103   Max :111-125   Min :133-147   stepdiff :149-206

The composite sign polynomial is mandatory: the reference's default table is a recorded result of its generator and is kept as a test
fixture (tests/golden/minimax_default_sign.json, read with minimax.Polynomial.from_json), not as program text."""
import copy

from fractions import Fraction

from . import polynomial
from .ckks import Complex, Scale, _round
from .minimax import Polynomial, at_common_level, bootstrap
from .ringhip import RingHipError


class Evaluator:
    """comparison.Evaluator: minimax_evaluator a minimax.Evaluator, sign_poly a minimax.Polynomial approximating the sign on [-1, 1]"""

    def __init__(self, minimax_evaluator, sign_poly):
        if sign_poly is None or len(sign_poly) == 0:
            raise RingHipError("cannot NewEvaluator: the composite sign polynomial is mandatory (the reference's default table is a test fixture: "
                               "minimax.Polynomial.from_json)")
        self.mm, self.MinimaxCompositeSignPolynomial = minimax_evaluator, sign_poly

    def Sign(self, op0):
        """:75-77: 1 if x > 0, -1 if x < 0; sign.Scale = DefaultScale"""
        return self.mm.Evaluate(op0, self.MinimaxCompositeSignPolynomial)

    def StepPolynomial(self):
        """(sign + 1) / 2 (:83-100): the last polynomial's coefficients halved and 1/2 added to coefficient 0, each rounded to the
        coefficients' precision as big.Float.Mul / Add on the coefficient itself round"""
        last = copy.copy(self.MinimaxCompositeSignPolynomial[-1])
        half = Fraction(1, 2)
        co = [None if c is None else Complex(_round(c.re * half, last.prec), c.im) for c in last.Coeffs]
        co[0] = Complex(_round(co[0].re + half, last.prec), co[0].im)
        last.Coeffs = co
        return Polynomial(list(self.MinimaxCompositeSignPolynomial[:-1]) + [last])

    def Step(self, op0):
        """:81-103: 1 if x > 0, 0 if x < 0, 1/2 at 0"""
        return self.mm.Evaluate(op0, self.StepPolynomial())

    def Max(self, op0, op1):
        """:111-125: step(op0 - op1) (op0 - op1) + op1; op0 + op1 in [-1, 1], equal scales"""
        ev = self.mm.ev
        stepdiff = self.stepdiff(op0, op1)
        a, b = at_common_level(ev, stepdiff, op1)
        out = ev.AddNew(a, b)
        polynomial._copy_meta(op0, out)
        return out

    def Min(self, op0, op1):
        """:133-147: op0 - step(op0 - op1) (op0 - op1)"""
        ev = self.mm.ev
        stepdiff = self.stepdiff(op0, op1)
        a, b = at_common_level(ev, op0, stepdiff)
        out = ev.SubNew(a, b)
        polynomial._copy_meta(op0, out)
        return out

    def stepdiff(self, op0, op1):
        """:149-206"""
        mm, ev, btp = self.mm, self.mm.ev, self.mm.BtsEval
        nb = ev.nb_rescales
        diff = ev.SubNew(*at_common_level(ev, op0, op1))
        polynomial._copy_meta(op0, diff)
        if diff.Level() < nb * 2:                                                  # the scale matching before the last multiplication
            diff = bootstrap(btp, diff, "stepdiff")
        step = self.Step(diff)
        if step.Level() < nb:
            step = bootstrap(btp, step, "stepdiff")
        level = min(diff.Level(), step.Level())
        Q = ev.ringQ.moduli
        ratio = Scale(1)
        for i in range(nb):
            ratio = ratio.Mul(Scale(int(Q[level - i])))
        ratio = ratio.Div(ev._scale(diff, "stepdiff"))
        ev.Mul(diff, ratio.Value, diff)                                            # a *big.Float: scaled by the moduli one rescaling consumes
        polynomial._rescale(ev, diff)
        diff.Scale = diff.Scale.Mul(ratio)
        a, b = at_common_level(ev, diff, step)
        out = ev.MulRelinNew(a, b)
        polynomial._copy_meta(op0, out)
        polynomial._rescale(ev, out)
        return out

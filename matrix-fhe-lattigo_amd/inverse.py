"""Host-side mirror of circuits/ckks/inverse/inverse.go, homomorphic 1 / x on device-resident batches, over minimax.Evaluator:

  EvaluateFullDomainNew :45-55   EvaluatePositiveDomainNew :63-65   EvaluateNegativeDomainNew :73-85   evaluateNew :87-198
  GoldschmidtDivisionNew :208-299   IntervalNormalization :312-407

The composite sign polynomial of the full domain is mandatory (see comparison.py).  The float64 constants are computed as the reference
computes them; Python's math.pow and 2.0 ** x stand where Go has math.Pow and math.Exp2."""
import math

from . import polynomial
from .minimax import at_common_level, bootstrap, min_level
from .ringhip import RingHipError


class Evaluator:
    """inverse.Evaluator over a minimax.Evaluator (None: only the refusal of the full domain is left, as in the reference)"""

    def __init__(self, minimax_evaluator):
        self.mm = minimax_evaluator

    def _mm(self, who):
        if self.mm is None:
            raise RingHipError("cannot %s: MinimaxCompositePolynomialEvaluator is nil" % who)
        return self.mm

    def _affine(self, ct, constant, out=None):
        """constant - ct"""
        return polynomial.affine_minus(self.mm.ev, ct, constant, self.mm.fused["affine"], out)

    def _mul_relin_rescale(self, a, b):
        """MulRelin(a, b, a) and Rescale(a, a) at the smaller of the two levels; a new ciphertext"""
        ev = self.mm.ev
        x, y = (a, a) if a is b else at_common_level(ev, a, b)
        out = ev.MulRelinNew(x, y)
        polynomial._copy_meta(a, out)
        polynomial._rescale(ev, out)
        return out

    # ---- :45-85 ----
    def EvaluateFullDomainNew(self, ct, log2min, log2max, signMinimaxPoly=None):
        """1 / x for x in [-2^log2max, -2^log2min] U [2^log2min, 2^log2max]"""
        if self.mm is None:
            raise RingHipError("preprocessing: cannot EvaluateNew: MinimaxCompositePolynomialEvaluator is nil but fulldomain is set to true")
        if signMinimaxPoly is None:
            raise RingHipError("cannot EvaluateFullDomainNew: the composite sign polynomial is mandatory (the reference's default table is a test fixture: "
                               "minimax.Polynomial.from_json)")
        return self.evaluateNew(ct, log2min, log2max, True, signMinimaxPoly)

    def EvaluatePositiveDomainNew(self, ct, log2min, log2max):
        """1 / x for x in [2^log2min, 2^log2max]"""
        self._mm("EvaluatePositiveDomainNew")
        return self.evaluateNew(ct, log2min, log2max, False, None)

    def EvaluateNegativeDomainNew(self, ct, log2min, log2max):
        """1 / x for x in [-2^log2max, -2^log2min]"""
        ev = self._mm("EvaluateNegativeDomainNew").ev
        ctNeg = ev.MulNew(ct, -1)
        polynomial._copy_meta(ct, ctNeg)
        cInv = self.EvaluatePositiveDomainNew(ctNeg, log2min, log2max)
        ev.Mul(cInv, -1, cInv)
        return cInv

    # ---- :87-198 ----
    def evaluateNew(self, ct, log2min, log2max, fulldomain, signMinimaxPoly):
        mm = self.mm
        ev, btp, nb = mm.ev, mm.BtsEval, mm.ev.nb_rescales
        normalizationfactor = None
        if log2max > 0:
            try:
                cInv, normalizationfactor = self.IntervalNormalization(ct, log2max, btp)
            except RingHipError as e:
                raise RingHipError("preprocessing: normalizationfactor: %s" % e) from None
        else:
            cInv = polynomial._copy_new(ct)
        sign = None
        if fulldomain:
            try:
                sign = mm.Evaluate(cInv, signMinimaxPoly)                          # the sign with precision [-1, -2^-a] U [2^-a, 1]
            except RingHipError as e:
                raise RingHipError("preprocessing: fulldomain: true -> sign: %s" % e) from None
            if sign.Level() < min_level(btp) + nb:
                sign = bootstrap(btp, sign, "EvaluateFullDomainNew: preprocessing: fulldomain: true -> sign -> bootstrap(sign)")
            if cInv.Level() < min_level(btp) + nb:
                cInv = bootstrap(btp, cInv, "EvaluateFullDomainNew: preprocessing: fulldomain: true -> sign -> bootstrap(cInv)")
            cInv = self._mul_relin_rescale(cInv, sign)                             # |x| = x sign(x)
        try:
            cInv = self.GoldschmidtDivisionNew(cInv, log2min)
        except RingHipError as e:
            raise RingHipError("division: GoldschmidtDivisionNew: %s" % e) from None
        postprocessdepth = 0
        if normalizationfactor is not None or fulldomain:
            postprocessdepth += nb
        if fulldomain:
            postprocessdepth += nb
        if normalizationfactor is not None:                                        # back through the encrypted normalization factor
            if cInv.Level() < min_level(btp) + postprocessdepth:
                cInv = bootstrap(btp, cInv, "evaluateNew: normalizationfactor: bootstrap(cInv)")
            if normalizationfactor.Level() < min_level(btp) + postprocessdepth:
                normalizationfactor = bootstrap(btp, normalizationfactor, "evaluateNew: normalizationfactor: bootstrap(normalizationfactor)")
            cInv = self._mul_relin_rescale(cInv, normalizationfactor)
        if fulldomain:
            cInv = self._mul_relin_rescale(cInv, sign)                             # back through the encrypted sign
        return cInv

    # ---- :208-299 ----
    def GoldschmidtDivisionNew(self, ct, log2min):
        """1 / x for x in [2^log2min, 2 - 2^log2min]: a <- a (1 + b), b <- b^2 from a = 2 - x, b = 1 - x; the iteration count from the scale"""
        mm = self._mm("GoldschmidtDivisionNew")
        ev, btp, nb = mm.ev, mm.BtsEval, mm.ev.nb_rescales
        prec = float(ev.ringQ.N // 2) / ev._scale(ct, "GoldschmidtDivisionNew").Float64()    # 2^-(prec - LogN + 1)
        start = 1 - 2.0 ** log2min
        iters = 1
        while start >= prec:
            start *= start                                                         # doubles the bit-precision at each iteration
            iters += 1
        iters = max(iters, 3)
        depth = iters * nb
        if btp is None and depth > ct.Level():
            raise RingHipError("cannot GoldschmidtDivisionNew: ct.Level()=%d < depth=%d and rlwe.Bootstrapper is nil" % (ct.Level(), depth))
        if mm.fused["affine"]:
            a, b = self._affine(ct, 2), self._affine(ct, 1)
        else:
            a = ev.MulNew(ct, -1)
            polynomial._copy_meta(ct, a)
            b = polynomial._copy_new(a)
            ev.Add(a, 2, a)
            ev.Add(b, 1, b)
        needs = lambda x: btp is not None and (x.Level() == btp.MinimumInputLevel() or x.Level() == nb - 1)
        for _ in range(1, iters):
            if needs(b):
                b = btp.Bootstrap(b)
            if needs(a):
                a = btp.Bootstrap(a)
            b = self._mul_relin_rescale(b, b)
            if needs(b):
                b = btp.Bootstrap(b)
            tmp = self._mul_relin_rescale(a, b)
            ev.SetScale(a, tmp.Scale)                                              # a is at a higher level than tmp: a level brings it down
            x, y = at_common_level(ev, a, tmp)
            out = ev.AddNew(x, y)
            polynomial._copy_meta(ct, out)
            a = out
        return a

    # ---- :312-407 ----
    def IntervalNormalization(self, ct, log2Max, btp):
        """Algorithm 2 of https://eprint.iacr.org/2022/280, modified to keep the compression factor: -> (ctNorm with values in [-1, 1],
        ctNormFac with ctNorm = ct ctNormFac)"""
        mm = self._mm("IntervalNormalization")
        ev, nb = mm.ev, mm.ev.nb_rescales
        ctNorm, ctNormFac = polynomial._copy_new(ct), None
        L = 2.45                                                                   # compression factor (experimental)
        n = math.ceil(log2Max / math.log2(L))
        for i in range(int(n)):
            if ctNorm.Level() < min_level(btp) + 4 * nb:
                ctNorm = bootstrap(btp, ctNorm, "IntervalNormalization")
            if ctNormFac is not None and (ctNormFac.Level() == min_level(btp) or ctNormFac.Level() == nb - 1):
                ctNormFac = bootstrap(btp, ctNormFac, "IntervalNormalization")
            c = 2.0 / math.sqrt(27 * math.pow(L, 2 * (float(n) - 1 - float(i))))
            z = ev.MulNew(ctNorm, c)                                               # z = 1 - (c y)^2, two levels
            polynomial._copy_meta(ct, z)
            polynomial._rescale(ev, z)
            z = self._mul_relin_rescale(z, z)
            self._affine(z, 1, z)
            if z.Level() < min_level(btp) + nb:
                z = bootstrap(btp, z, "IntervalNormalization")
            ctNormFac = z if ctNormFac is None else self._mul_relin_rescale(ctNormFac, z)
            ctNorm = self._mul_relin_rescale(ctNorm, z)
        return ctNorm, ctNormFac

"""Host-side mirror of circuits/ckks/bootstrapping/evaluator.go, CKKS bootstrapping, on device-resident batches: standard rings, the float64
path, ResidualParameters.N == BootstrappingParameters.N, one iteration.  The arithmetic is the device evaluators' (ckks.Evaluator,
rlwe.Evaluator, dft.Evaluator, mod1.Evaluator) and, for ModUp's lift, one launch of rh_ckks_bootstrap_modup (csrc/bootstrap.hip).

  NewEvaluator :48-128   checkKeys :164-185   initialize :187-246   Bootstrap :249-256   Depth / OutputLevel / MinimumInputLevel :317-329
  Evaluate :345-488 (the single-iteration arm)   checkMessageRatio :541-546   bootstrap :548-587   ScaleDown :596-643   ModUp :646-794
  CoeffsToSlots :797-799   EvalMod :802-809   EvalModAndScale :813-820   SlotsToCoeffs :822-824
  parameters.go: Parameters :18-35, GaloisElements :461-484, the depths :379-397      keys.go: EvaluationKeys :33-41
  sk_bootstrapper.go: SecretKeyBootstrapper :11-69

A batch of npoly ciphertexts is one Ciphertext; all of them share level and scale.  This package takes rings, not parameter literals, so
Parameters is built from explicit pieces.  Where the reference works in place on its input (ScaleDown, ModUp), the device path writes new
blocks and leaves the caller's ciphertext as it was.

Refused by name: IterationsParameters (META-BTS) and PREC128, conjugate-invariant residual rings (EvaluateConjugateInvariant), N1 != N2 (the
ring-degree switch), ciphertexts whose LogDimensions differ from the bootstrapping LogSlots (the pack / unpack of BootstrapMany), the
DecodeThenModUp and Custom circuit orders, and the reference's own refusals (SinContinuous with a double angle, CosDiscrete below degree
2 (K - 1), inconsistent levels, missing keys)."""
import math
from fractions import Fraction

from . import dft, mod1, polynomial, rlwe
from .ckks import Decryptor, DeviceValues, Encoder, Encryptor, Evaluator as CkksEvaluator, Scale, _round
from .ringhip import ConjugateInvariant, RingHipError, Standard, _check, _p, _u64, lib
from .schemes import Ciphertext

ModUpThenEncode, DecodeThenModUp, Custom = 0, 1, 2       # CircuitOrder (parameters_literal.go:144-150)
PREC64, PREC128 = 0, 1                                   # ckks.PrecisionMode


def modup_lift(ringQ, ringP, levelQ, levelP, in0, in1, out0, out1=None, c1Q=None, c1P=None, scalar=None):
    """The lift of ModUp (:678-696, :703-722, :762-775), one launch over both components of a batch.
    in0 / in1: the two components at level 0 or above in the COEFFICIENT domain (limb 0 of every poly is read).  Without ringP both are
    lifted to limbs 0 .. levelQ of out0 / out1, which overlap neither input.  With ringP (sparse-secret
    encapsulation) component 1 goes to c1Q (limbs 0 .. levelQ of Q) and c1P (limbs 0 .. levelP of P) with the comparison coeff > q0 >> 1.
    scalar: uint64(round(scale)) of the message scaling (:735-750, :781-789), or None; every limb written is multiplied by it."""
    if in0.limbs != in1.limbs or in0.npoly != in1.npoly:
        raise RingHipError("cannot ModUp: the two components differ in shape")
    outs = [out0] + ([out1] if ringP is None else [c1Q])
    if any(o is None or o.limbs != levelQ + 1 or o.npoly != in0.npoly for o in outs):
        raise RingHipError("cannot ModUp: every output modulo Q holds levelQ + 1 = %d limbs and the input's %d polys" % (levelQ + 1, in0.npoly))
    if ringP is not None and (c1P is None or c1P.limbs != levelP + 1 or c1P.npoly != in0.npoly):
        raise RingHipError("cannot ModUp: the output modulo P holds levelP + 1 = %d limbs and the input's %d polys" % (levelP + 1, in0.npoly))
    sq = sp = None
    if scalar is not None:
        sq = _u64([int(scalar) % int(q) for q in ringQ.moduli[:levelQ + 1]])
        if ringP is not None:
            sp = _u64([int(scalar) % int(p) for p in ringP.moduli[:levelP + 1]])
    _check(lib().rh_ckks_bootstrap_modup(ringQ._h, ringP._h if ringP is not None else None, levelQ, levelP if ringP is not None else 0,
                                         in0.ptr, in1.ptr, in0.limbs, out0.ptr, out1.ptr if out1 is not None else None,
                                         c1Q.ptr if c1Q is not None else None, c1P.ptr if c1P is not None else None, in0.npoly, _p(sq), _p(sp)))


class Parameters:
    """bootstrapping.Parameters (parameters.go:18-35) from explicit pieces.  ringQ / ringP: the rings of BootstrappingParameters, whose first
    ResidualMaxLevel + 1 moduli are ResidualParameters.Q; ResidualDefaultScale / BootstrappingDefaultScale: the two DefaultScale();
    the three literals as the reference holds them; EphemeralSecretWeight: 0 without sparse-secret encapsulation."""

    def __init__(self, ringQ, ringP, ResidualMaxLevel, ResidualDefaultScale, SlotsToCoeffsParameters, Mod1ParametersLiteral, CoeffsToSlotsParameters,
                 EphemeralSecretWeight=32, BootstrappingDefaultScale=None, CircuitOrder=ModUpThenEncode, IterationsParameters=None,
                 ResidualRingType=Standard, ResidualN=None, PrecisionMode=PREC64):
        self.ringQ, self.ringP, self.ResidualMaxLevel = ringQ, ringP, int(ResidualMaxLevel)
        self.ResidualDefaultScale = Scale(ResidualDefaultScale)
        self.BootstrappingDefaultScale = Scale(ResidualDefaultScale if BootstrappingDefaultScale is None else BootstrappingDefaultScale)
        self.SlotsToCoeffsParameters, self.Mod1ParametersLiteral, self.CoeffsToSlotsParameters = SlotsToCoeffsParameters, Mod1ParametersLiteral, CoeffsToSlotsParameters
        self.EphemeralSecretWeight, self.CircuitOrder, self.IterationsParameters = int(EphemeralSecretWeight), CircuitOrder, IterationsParameters
        self.ResidualRingType, self.ResidualN, self.PrecisionMode = ResidualRingType, ringQ.N if ResidualN is None else int(ResidualN), PrecisionMode

    def LogMaxSlots(self):
        return self.SlotsToCoeffsParameters.LogSlots                          # :369-376

    def DepthCoeffsToSlots(self):
        return self.SlotsToCoeffsParameters.Depth(True)                       # :379-381, as written: the SlotsToCoeffs literal

    def DepthEvalMod(self):
        return self.Mod1ParametersLiteral.Depth()

    def DepthSlotsToCoeffs(self):
        return self.CoeffsToSlotsParameters.Depth(True)                       # :389-391, as written: the CoeffsToSlots literal

    def Depth(self):
        return self.DepthCoeffsToSlots() + self.DepthEvalMod() + self.DepthSlotsToCoeffs()

    def GaloisElements(self):
        """:461-484: the SubSum rotations X -> Y^slots, the two DFTs', the conjugation; sorted"""
        N = self.ringQ.N
        logN = N.bit_length() - 1
        keys = {rlwe.GaloisElement(N, 1 << i) for i in range(self.LogMaxSlots(), logN - 1)}
        keys |= set(self.CoeffsToSlotsParameters.GaloisElements(N)) | set(self.SlotsToCoeffsParameters.GaloisElements(N))
        keys.add(2 * N - 1)
        return sorted(keys)


class EvaluationKeys:
    """bootstrapping.EvaluationKeys (keys.go:33-41) as far as this path reads them: the relinearisation key and the Galois keys
    (rlwe.GadgetCiphertext over ringQ, ringP) and the two encapsulation keys -- EvkDenseToSparse over the one-limb rings of Q[:1] and P[:1]
    (keys.go:131-141), EvkSparseToDense over ringQ, ringP"""

    def __init__(self, rlk=None, galois_keys=None, EvkDenseToSparse=None, EvkSparseToDense=None):
        self.rlk, self.galois_keys = rlk, dict(galois_keys or {})
        self.EvkDenseToSparse, self.EvkSparseToDense = EvkDenseToSparse, EvkSparseToDense


def _with_scaling(lit, scaling):
    """the literal with `scaling` multiplied into its Scaling (:223-233)"""
    s = scaling if lit.Scaling is None else float(Fraction(lit.Scaling) * Fraction(scaling))
    return dft.MatrixLiteral(lit.Type, lit.LogSlots, lit.LevelQ, lit.LevelP, lit.Levels, lit.Format, s, lit.BitReversed, lit.LogBSGSRatio)


class Evaluator:
    """bootstrapping.Evaluator.  fused: None what mod1.Evaluator.FUSED_BOOTSTRAP says, else True / False for every choice:
      modup_scale   the message scalar multiplied inside the ModUp kernel, or as MulScalar after the NTT (:735-750, :781-789)
      double_angle  rh_ckks_double_angle, or the two Adds (mod1.py)
    -- the same bits either way."""

    def __init__(self, parameters, keys, fused=None):
        p = self.Parameters = parameters
        who = "cannot NewBootstrapper"
        if p.ResidualRingType == ConjugateInvariant:
            raise RingHipError("%s: conjugate-invariant residual parameters (EvaluateConjugateInvariant, the domain switch) are not built on the device path" % who)
        if p.ResidualRingType != Standard or p.ringQ.kind != Standard:
            raise RingHipError("%s: standard rings only" % who)
        if p.ResidualN != p.ringQ.N:
            raise RingHipError("%s: ResidualParameters.N = %d != BootstrappingParameters.N = %d: the ring-degree switch (EvkN1ToN2, EvkN2ToN1) is not built on the device path"
                               % (who, p.ResidualN, p.ringQ.N))
        if p.IterationsParameters is not None:
            raise RingHipError("%s: IterationsParameters (META-BTS iterations, the reserved prime) are not built on the device path" % who)
        if p.PrecisionMode != PREC64:
            raise RingHipError("%s: PREC128 residual parameters are not built on the device path" % who)
        m1 = p.Mod1ParametersLiteral
        if m1.Mod1Type == mod1.SinContinuous and m1.DoubleAngle != 0:                                  # :83-85
            raise RingHipError("cannot use double angle formula for Mod1Type = Sin -> must use Mod1Type = Cos")
        if m1.Mod1Type == mod1.CosDiscrete and m1.Mod1Degree < 2 * (m1.K - 1):                         # :87-89
            raise RingHipError("Mod1Type 'mod1.CosDiscrete' uses a minimum degree of 2*(K-1) but EvalMod degree is smaller")
        c2s, s2c = p.CoeffsToSlotsParameters, p.SlotsToCoeffsParameters
        if p.CircuitOrder == ModUpThenEncode:                                                          # :91-107
            if c2s.LevelQ - c2s.Depth(True) != m1.LevelQ:
                raise RingHipError("starting level and depth of CoeffsToSlotsParameters inconsistent starting level of Mod1ParametersLiteral")
            if m1.LevelQ - m1.Depth() != s2c.LevelQ:
                raise RingHipError("starting level and depth of Mod1ParametersLiteral inconsistent starting level of CoeffsToSlotsParameters")
        elif p.CircuitOrder in (DecodeThenModUp, Custom):
            raise RingHipError("%s: CircuitOrder %s is not built on the device path: ModUpThenEncode only"
                               % (who, "DecodeThenModUp" if p.CircuitOrder == DecodeThenModUp else "Custom"))
        else:
            raise RingHipError("invalid CircuitOrder value")
        if c2s.LogSlots != s2c.LogSlots:
            raise RingHipError("%s: CoeffsToSlotsParameters.LogSlots = %d != SlotsToCoeffsParameters.LogSlots = %d" % (who, c2s.LogSlots, s2c.LogSlots))
        self.fused = dict(mod1.Evaluator.FUSED_BOOTSTRAP) if fused is None else {k: bool(fused) for k in mod1.Evaluator.FUSED_BOOTSTRAP}
        self._check_keys(keys)
        self.EvaluationKeys = keys
        self.EvkDenseToSparse, self.EvkSparseToDense = keys.EvkDenseToSparse, keys.EvkSparseToDense
        self._initialize()
        self.Evaluator = CkksEvaluator(p.ringQ, p.ringP, rlk=keys.rlk, galois_keys=keys.galois_keys)
        self.DFTEvaluator = dft.Evaluator(self.Evaluator)
        self.Mod1Evaluator = mod1.Evaluator(self.Evaluator, polynomial.PolynomialEvaluator(self.Evaluator), self.Mod1Parameters, fused=fused)
        self._sparse = None
        if self.EvkDenseToSparse is not None:
            q0, p0 = self.EvkDenseToSparse.Q.ring, self.EvkDenseToSparse.P.ring if self.EvkDenseToSparse.P is not None else None
            if p0 is None or q0.L != 1 or p0.L != 1 or int(q0.moduli[0]) != int(p.ringQ.moduli[0]):
                raise RingHipError("%s: EvkDenseToSparse lives over the one-limb rings of Q[:1] and P[:1]" % who)
            self._sparse = rlwe.Evaluator(q0, p0)

    def close(self):
        self.Evaluator.close()
        if self._sparse is not None:
            self._sparse.close()

    # ---- checkKeys :164-185 ----
    def _check_keys(self, evk):
        if evk.rlk is None:
            raise RingHipError("RelinearizationKey is nil")
        for g in self.Parameters.GaloisElements():
            if g != 1 and evk.galois_keys.get(g) is None:
                raise RingHipError("GaloisKey[%d] is nil" % g)
        if evk.EvkDenseToSparse is None and self.Parameters.EphemeralSecretWeight != 0:
            raise RingHipError("rlwe.EvaluationKey key dense to sparse is nil")
        if evk.EvkSparseToDense is None and self.Parameters.EphemeralSecretWeight != 0:
            raise RingHipError("rlwe.EvaluationKey key sparse to dense is nil")

    # ---- initialize :187-246 ----
    def _initialize(self):
        p = self.Parameters
        Q0 = int(p.ringQ.moduli[0])
        self.Mod1Parameters = evm = mod1.NewParametersFromLiteral(Q0, p.Mod1ParametersLiteral)
        K, qDiff = evm.K, evm.QDiff
        qDiv = evm.ScalingFactor().Float64() / math.ldexp(1.0, int(mod1._go_round(mod1._go_log2(float(Q0)))))      # :205
        if qDiv > 1:
            qDiv = 1.0
        scale = p.BootstrappingDefaultScale.Float64()
        offset = evm.ScalingFactor().Float64() / evm.MessageRatio()
        self.CoeffsToSlotsParameters = _with_scaling(p.CoeffsToSlotsParameters, qDiv / (K * qDiff))                 # :220-227
        self.SlotsToCoeffsParameters = _with_scaling(p.SlotsToCoeffsParameters, scale / offset)                     # :221-233
        encoder = Encoder(p.ringQ, ringP=p.ringP)
        try:
            self.C2SDFTMatrix = dft.NewMatrixFromLiteral(p.ringQ, p.ringP, self.CoeffsToSlotsParameters, encoder)
            self.S2CDFTMatrix = dft.NewMatrixFromLiteral(p.ringQ, p.ringP, self.SlotsToCoeffsParameters, encoder)
        finally:
            encoder.close()

    # ---- :317-329 ----
    def Depth(self):
        return self.Parameters.ringQ.L - 1 - self.Parameters.ResidualMaxLevel

    def OutputLevel(self):
        return self.Parameters.ResidualMaxLevel

    def MinimumInputLevel(self):
        return self.Evaluator.nb_rescales

    # ---- Bootstrap :249-314, Evaluate :345-488 ----
    def _check_in(self, ct, who):
        ls = getattr(ct, "LogDimensions", None)
        if ls is None:
            raise RingHipError("cannot %s: a ciphertext carries no LogDimensions" % who)
        if ls != self.Parameters.LogMaxSlots():
            raise RingHipError("cannot %s: the ciphertext has LogSlots = %d, the bootstrapping %d: the pack / unpack of sparse ciphertexts (BootstrapMany) is not built on the device path"
                               % (who, ls, self.Parameters.LogMaxSlots()))

    def Bootstrap(self, ct):
        """:249-256 with the scale of BootstrapMany (:309-311)"""
        self._check_in(ct, "Bootstrap")
        out = self.Evaluate(ct)
        out.Scale = self.Parameters.ResidualDefaultScale
        return out

    def Evaluate(self, ctIn):
        """the single-iteration arm (:347-350)"""
        self._check_in(ctIn, "Evaluate")
        return self.bootstrap(ctIn)[0]

    def EvaluateConjugateInvariant(self, ctLeftN1Q0, ctRightN1Q0=None):
        raise RingHipError("cannot EvaluateConjugateInvariant: conjugate-invariant residual parameters (the domain switch) are not built on the device path")

    def bootstrap(self, ctIn):
        """:548-587 -> (ctOut, errScale)"""
        ctOut, errScale = self.ScaleDown(ctIn)
        ctOut = self.ModUp(ctOut)
        ctReal, ctImag = self.CoeffsToSlots(ctOut)
        if ctImag is None:
            ctReal = self.EvalMod(ctReal)
        else:
            ctReal, ctImag = self._eval_mod_pair(ctReal, ctImag)
        return self.SlotsToCoeffs(ctReal, ctImag), errScale

    # ---- ScaleDown :596-643 ----
    def _check_message_ratio(self, level, scale):
        """:541-546"""
        Q = [int(q) for q in self.Parameters.ringQ.moduli]
        cur = Scale(math.prod(Q[:level + 1])).Div(scale)
        return cur.Cmp(Scale(Q[level]).Mul(Scale(self.Mod1Parameters.MessageRatio()))) > -1

    def ScaleDown(self, ctIn):
        """-> (ct at level 0 and scale ~ Q[0] / MessageRatio, errScale).  ctIn is left as it was."""
        ev = self.Evaluator
        Q = [int(q) for q in self.Parameters.ringQ.moduli]
        scale = ev._scale(ctIn, "ScaleDown")
        level = ctIn.Level()
        while level != 0 and self._check_message_ratio(level, scale):                 # removes unnecessary primes (:603-605)
            level -= 1
        ct = ev.DropLevelNew(ctIn, ctIn.Level() - level)
        ct.LogDimensions = getattr(ctIn, "LogDimensions", None)
        currentMessageRatio = Scale(math.prod(Q[:level + 1])).Div(scale)
        targetMessageRatio = Scale(self.Mod1Parameters.MessageRatio())
        scaleUp = currentMessageRatio.Div(targetMessageRatio)
        if scaleUp.Cmp(Scale(0.5)) == -1:
            raise RingHipError("initial Q/Scale = %f < 0.5*Q[0]/MessageRatio = %f" % (currentMessageRatio.Float64(), targetMessageRatio.Float64()))
        scaleUpBigint = scaleUp.BigInt()
        ev.Mul(ct, scaleUpBigint, ct)                                                 # :623
        ct.Scale = ct.Scale.Mul(Scale(scaleUpBigint))                                 # :627
        targetScale = Scale(_round(Fraction(Q[0]) / Fraction(self.Mod1Parameters.MessageRatio()), 256))      # :630-631
        if ct.Level() != 0:
            ev.RescaleTo(ct, targetScale, ct)                                         # :633-637
        return ct, ct.Scale.Div(targetScale)                                          # :640

    # ---- ModUp :646-794 ----
    def ModUp(self, ctIn):
        """a level-0 ciphertext -> the top level: the switch to the sparse key, INTT, the lift (one launch), NTT, the switch back through the
        hoisted gadget product fed the lifted c1 as every digit's decomposition (or the dense arm), the message scaling, Trace.  ctIn is
        left as it was."""
        p, ev = self.Parameters, self.Evaluator
        if ctIn.Level() != 0 or ctIn.Degree() != 1 or not ctIn.IsNTT:
            raise RingHipError("cannot ModUp: the input must be a degree-1 ciphertext at level 0 in the NTT domain")
        rq0 = p.ringQ.AtLevel(0)
        npoly = ctIn.Value[0].npoly
        scale = ev._scale(ctIn, "ModUp")
        c0, c1 = rq0.NewPoly(npoly), rq0.NewPoly(npoly)
        if self.EvkDenseToSparse is not None:                                          # switch to the sparse key (:649-653): GadgetProduct + Add
            tmp = Ciphertext([rq0.NewPoly(npoly), c1], is_ntt=True)
            self._sparse.GadgetProduct(0, ctIn.Value[1], self.EvkDenseToSparse, tmp)
            rq0.Add(ctIn.Value[0], tmp.Value[0], c0)
            rq0.INTT(c0, c0)
            rq0.INTT(c1, c1)
        else:
            rq0.INTT(ctIn.Value[0], c0)                                                # :660-662
            rq0.INTT(ctIn.Value[1], c1)
        levelQ, levelP = p.ringQ.L - 1, p.ringP.L - 1
        rq, rp = p.ringQ.AtLevel(levelQ), p.ringP.AtLevel(levelP)
        s = (self.Mod1Parameters.ScalingFactor().Float64() / self.Mod1Parameters.MessageRatio()) / scale.Float64()     # :735 / :781
        scalar = int(mod1._go_round(s)) if s > 1 else None
        fold = scalar if self.fused["modup_scale"] else None
        out0 = rq.NewPoly(npoly)
        if self.EvkSparseToDense is not None:
            ks = ev.ks
            beta = ks.BaseRNSDecompositionVectorSize(levelQ, levelP)
            dq = ks.buffer("BuffDecompQ", rq, beta * npoly, levelQ + 1)
            dp = ks.buffer("BuffDecompP", rp, beta * npoly, levelP + 1)
            digit = lambda i: (rlwe._view(dq, i * npoly, npoly), rlwe._view(dp, i * npoly, npoly))
            c1Q, c1P = digit(0)                                                        # ks.BuffDecompQP[0] (:714-720)
            modup_lift(p.ringQ, p.ringP, levelQ, levelP, c0, c1, out0, c1Q=c1Q, c1P=c1P, scalar=fold)
            rq.NTT(c1Q, c1Q)                                                           # transformed ONCE, then copied into every digit (:724-730)
            rp.NTT(c1P, c1P)
            rq.NTT(out0, out0)                                                         # :732
            if scalar is not None and fold is None:                                    # :735-750
                rq.MulScalar(c1Q, scalar, c1Q)
                rp.MulScalar(c1P, scalar, c1P)
                rq.MulScalar(out0, scalar, out0)
            for i in range(1, beta):
                dQ, dP = digit(i)
                rq.CopyLvl(c1Q, dQ)
                rp.CopyLvl(c1P, dP)
            ctTmp = Ciphertext([ks.buffer("BuffQP1Q", rq, npoly, levelQ + 1), rq.NewPoly(npoly)], is_ntt=True)      # (ks.BuffQP[1].Q, ctIn.Value[1]) (:752-754)
            ks.GadgetProductHoisted(levelQ, (dq, dp), self.EvkSparseToDense, ctTmp)   # switch back to the dense key (:757)
            rq.Add(out0, ctTmp.Value[0], out0)                                         # :758
            out = Ciphertext([out0, ctTmp.Value[1]], is_ntt=True)
        else:
            out1 = rq.NewPoly(npoly)
            modup_lift(p.ringQ, None, levelQ, 0, c0, c1, out0, out1, scalar=fold)      # :762-775
            rq.NTT(out0, out0)
            rq.NTT(out1, out1)
            if scalar is not None and fold is None:                                    # :781-789
                rq.MulScalar(out0, scalar, out0)
                rq.MulScalar(out1, scalar, out1)
            out = Ciphertext([out0, out1], is_ntt=True)
        out.Scale = scale.Mul(Scale(s)) if scalar is not None else scale
        out.LogDimensions = getattr(ctIn, "LogDimensions", None)
        ev.Trace(out, self.CoeffsToSlotsParameters.LogSlots, out)                      # SubSum X -> (N / dslots) Y^dslots (:793)
        return out

    # ---- :797-824 ----
    def CoeffsToSlots(self, ctIn):
        return self.DFTEvaluator.CoeffsToSlotsNew(ctIn, self.C2SDFTMatrix)

    def EvalMod(self, ctIn):
        return self.EvalModAndScale(ctIn, 1)

    def EvalModAndScale(self, ctIn, scaling):
        ctOut = self.Mod1Evaluator.EvaluateAndScaleNew(ctIn, scaling)
        ctOut.Scale = self.Parameters.BootstrappingDefaultScale
        ctOut.LogDimensions = getattr(ctIn, "LogDimensions", None)
        return ctOut

    def SlotsToCoeffs(self, ctReal, ctImag):
        return self.DFTEvaluator.SlotsToCoeffsNew(ctReal, ctImag, self.S2CDFTMatrix)

    def _eval_mod_pair(self, ctReal, ctImag):
        """EvalMod on ctReal and on ctImag (:570-579) as ONE batch of 2 npoly ciphertexts: they leave CoeffsToSlots at the same level and scale and
        every operation is per ciphertext, so the bits are those of two calls and the launches are half"""
        ev = self.Evaluator
        if ctReal.Level() != ctImag.Level() or ev._scale(ctReal, "EvalMod").Cmp(ev._scale(ctImag, "EvalMod")) != 0:
            return self.EvalMod(ctReal), self.EvalMod(ctImag)
        level, npoly = ctReal.Level(), ctReal.Value[0].npoly
        rq = self.Parameters.ringQ.AtLevel(level)
        both = Ciphertext([rq.NewPoly(2 * npoly) for _ in (0, 1)], is_ntt=True)
        for c in (0, 1):
            rq.CopyLvl(ctReal.Value[c], rlwe._view(both.Value[c], 0, npoly))
            rq.CopyLvl(ctImag.Value[c], rlwe._view(both.Value[c], npoly, npoly))
        both.Scale, both.LogDimensions = ctReal.Scale, ctReal.LogDimensions
        out = self.EvalMod(both)
        halves = []
        for first in (0, npoly):
            h = Ciphertext([rlwe._view(v, first, npoly) for v in out.Value], is_ntt=True)
            h.Scale, h.LogDimensions = out.Scale, out.LogDimensions
            halves.append(h)
        return halves[0], halves[1]


class SecretKeyBootstrapper:
    """bootstrapping.SecretKeyBootstrapper (sk_bootstrapper.go:11-69): the Bootstrapper that decrypts and re-encrypts under the secret key --
    decrypt, decode, encode at the top level and at default_scale, encrypt, in place on the ciphertext it returns; the stand-in the
    reference's comparison and inverse tests run their circuits with.  encoder: a ckks.Encoder over ringQ.  The device encoder is the
    float64 path, where the reference decodes to []*bignum.Complex at the parameters' precision: the refresh is meaningful up to 53 bits.
    Counter records the number of bootstrappings; MinLevel is what MinimumInputLevel returns.  samples=: as Encryptor.Encrypt takes them."""

    def __init__(self, ringQ, sk, encoder, default_scale, prng=None):
        if ringQ.kind != Standard:
            raise RingHipError("cannot NewSecretKeyBootstrapper: standard rings only (the encoder is standard-only)")
        self.ringQ, self.sk, self.Encoder = ringQ, sk, encoder
        self.DefaultScale = Scale(default_scale)
        self.Decryptor = Decryptor(ringQ, sk)
        self.Encryptor = Encryptor(ringQ, None, sk, prng)
        self.Counter, self.MinLevel = 0, 0
        self._values = {}

    def MaxLevel(self):
        return self.ringQ.L - 1

    def Bootstrap(self, ct, samples=None):
        """:32-46"""
        logSlots = getattr(ct, "LogDimensions", None)
        if logSlots is None:
            raise RingHipError("cannot Bootstrap: a ciphertext carries no LogDimensions")
        npoly = ct.Value[0].npoly
        key = (npoly, 1 << logSlots)
        values = self._values.get(key)
        if values is None:
            values = self._values[key] = DeviceValues(self.ringQ, npoly, 1 << logSlots)
        self.Encoder.Decode(self.Decryptor.DecryptNew(ct), values)
        pt = self.Encoder.NewPlaintext(self.MaxLevel(), self.DefaultScale, nvec=npoly, log_slots=logSlots, is_ntt=ct.IsNTT)
        self.Encoder.Encode(values, pt)
        rq = self.ringQ.AtLevel(self.MaxLevel())
        ct.Value = [rq.NewPoly(npoly), rq.NewPoly(npoly)]                              # ct.Resize(1, MaxLevel)
        self.Counter += 1
        self.Encryptor.Encrypt(pt, ct, samples)
        return ct

    def BootstrapMany(self, cts):
        return [self.Bootstrap(ct) for ct in cts]

    def Depth(self):
        return 0

    def MinimumInputLevel(self):
        return self.MinLevel

    def OutputLevel(self):
        return self.MaxLevel()

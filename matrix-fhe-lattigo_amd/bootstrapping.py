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

Refused by name by Evaluator: IterationsParameters (META-BTS) and PREC128, conjugate-invariant residual rings (EvaluateConjugateInvariant),
N1 != N2 (the ring-degree switch), ciphertexts whose LogDimensions differ from the bootstrapping LogSlots (the pack / unpack of BootstrapMany), the
DecodeThenModUp and Custom circuit orders, and the reference's own refusals (SinContinuous with a double angle, CosDiscrete below degree
2 (K - 1), inconsistent levels, missing keys).

Bootstrapper (the interface of bootstrapper.go) is BootstrapMany :259-314 around one inner Evaluator: PackAndSwitchN1ToN2 :880-911,
UnpackAndSwitchN2ToN1 :915-961, pack :1008-1065 and unpack :965-1004 (rh_ckks_bootstrap_pack / _unpack, csrc/bootstrap.hip),
EvaluateConjugateInvariant :493-538, ComplexToRealNew / RealToComplexNew :848-868; Parameters.GenEvaluationKeys is keys.go:69-144.  It takes the
three arms Evaluator refuses; iterations, PREC128 and the other circuit orders stay refused."""
import math
from fractions import Fraction

import numpy as np

from . import dft, mod1, polynomial, rlwe
from .ckks import Decryptor, DeviceValues, DomainSwitcher, Encoder, Encryptor, Evaluator as CkksEvaluator, Scale, _round
from .ringhip import ConjugateInvariant, DevicePoly, RingHipError, Standard, _check, _p, _u64, lib
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


# which passes of BootstrapMany run as rh_ckks_bootstrap_pack / rh_ckks_bootstrap_unpack (True) or as the reference's ring calls (False):
# MulCoeffsMontgomeryThenAdd per pair and level (pack), CopyNew + MulCoeffsMontgomery (unpack), Mul(ct, +-1j) + Add (the conjugate-invariant
# pair fold and unfold).  The same bits either way.
FUSED_BOOTSTRAP_MANY = {"pack": True, "unpack": True, "pair_fold": True, "pair_unfold": True}


def pack_table(ring, xPow2, logGap, g):
    """rows i = xPow2[logGap - i], 0 <= i < g, of GenXPow2NTT's list as ONE block (g, level + 1, N): the table rh_ckks_bootstrap_pack / _unpack take"""
    if g < 1 or logGap - (g - 1) < 0 or logGap >= len(xPow2):
        raise RingHipError("cannot build the pack table: rows %d .. %d of %d powers" % (logGap - (g - 1), logGap, len(xPow2)))
    block = ring.NewPoly(g)
    for i in range(g):
        ring.CopyLvl(xPow2[logGap - i], rlwe._view(block, i, 1))
    return block


def _pack_shapes(ring, n, g, ins, outs, table, who):
    L = ring.level + 1
    if len(ins) != 2 or len(outs) != 2:
        raise RingHipError("cannot %s: two components in and two out" % who)
    if any(p.limbs < L for p in (*ins, *outs, table)):
        raise RingHipError("cannot %s: every block and the table hold at least level + 1 = %d limbs" % (who, L))
    if ins[0].limbs != ins[1].limbs or outs[0].limbs != outs[1].limbs:
        raise RingHipError("cannot %s: the two components differ in limbs" % who)
    if table.npoly != g:
        raise RingHipError("cannot %s: the table holds %d rows per limb, %d tree levels need %d" % (who, table.npoly, g, g))
    words = lib().rh_ckks_bootstrap_pack_scratch_words(ring.N, L, n, g)
    return _Scratch(ring, words) if words else None


class _Scratch:
    """device words for the intermediates of a tree deeper than four levels"""

    def __init__(self, ring, words):
        self.words = int(words)
        self._p = DevicePoly(ring, (self.words + ring.N - 1) // ring.N, 1)
        self.ptr = self._p.ptr


def bootstrap_pack(ring, g, ins, outs, xp):
    """pack (evaluator.go:1035-1058) as rh_ckks_bootstrap_pack: ins = (c0, c1), batches of n polys; outs: batches of ceil(n / 2^g); xp: pack_table.
    The inputs are left as they were."""
    n = ins[0].npoly
    if ins[1].npoly != n or any(o.npoly != -(-n >> g) for o in outs):
        raise RingHipError("cannot pack: %d ciphertexts over %d tree levels give %d, the components hold %s and %s polys"
                           % (n, g, -(-n >> g), [p.npoly for p in ins], [p.npoly for p in outs]))
    sc = _pack_shapes(ring, n, g, ins, outs, xp, "pack")
    words = getattr(sc, "words", 0)
    _check(lib().rh_ckks_bootstrap_pack(ring._h, ring.level, n, g, ins[0].ptr, ins[1].ptr, ins[0].limbs, outs[0].ptr, outs[1].ptr, outs[0].limbs,
                                        xp.ptr, xp.limbs, sc.ptr if words else None, words))


def bootstrap_unpack(ring, g, n, ins, outs, xinv):
    """unpack (:985-1001) as rh_ckks_bootstrap_unpack: ins: batches of ceil(n / 2^g) polys; outs: NEW batches of n polys; xinv: pack_table of xPow2Inv"""
    if any(p.npoly != -(-n >> g) for p in ins) or any(o.npoly != n for o in outs):
        raise RingHipError("cannot unpack: %d ciphertexts over %d tree levels come from %d, the components hold %s and %s polys"
                           % (n, g, -(-n >> g), [p.npoly for p in ins], [p.npoly for p in outs]))
    sc = _pack_shapes(ring, n, g, ins, outs, xinv, "unpack")
    words = getattr(sc, "words", 0)
    _check(lib().rh_ckks_bootstrap_unpack(ring._h, ring.level, n, g, ins[0].ptr, ins[1].ptr, ins[0].limbs, outs[0].ptr, outs[1].ptr, outs[0].limbs,
                                          xinv.ptr, xinv.limbs, sc.ptr if words else None, words))


def pack_composed(ring, g, ins, outs, xp, work=None):
    """the reference's tree as written (:1035-1058) on a copy of the inputs: MulCoeffsMontgomeryThenAdd(odd, xPow2[logGap - i], eve) per pair
    and level, the odd one out moving up as it is (:1052-1057).  work: two blocks for the copies (allocated here without)"""
    n = ins[0].npoly
    for c in (0, 1):
        copy = ring.NewPoly(n) if work is None else work[c]
        ring.CopyLvl(ins[c], copy)
        cts = [rlwe._view(copy, k, 1) for k in range(n)]
        for i in range(g):
            t = rlwe._view(xp, i, 1)
            for j in range(len(cts) >> 1):
                ring.MulCoeffsMontgomeryThenAdd(cts[2 * j + 1], t, cts[2 * j])
                cts[j] = cts[2 * j]
            if len(cts) & 1:
                cts[len(cts) >> 1] = cts[-1]
                cts = cts[:(len(cts) >> 1) + 1]
            else:
                cts = cts[:len(cts) >> 1]
        for j, v in enumerate(cts):
            ring.CopyLvl(v, rlwe._view(outs[c], j, 1))


def unpack_composed(ring, g, n, ins, outs, xinv):
    """the reference's loops as written (:968-1001) per packed ciphertext: CopyNew, then MulCoeffsMontgomery by xPow2Inv[logGap - i] in place"""
    G = 1 << g
    for c in (0, 1):
        for j in range(ins[c].npoly):
            nj = min(n - j * G, G)                                                   # n = min(NbPackedCTs, 2^logPackCTs) (:973)
            cts = [rlwe._view(outs[c], j * G + k, 1) for k in range(nj)]
            for v in cts:
                ring.CopyLvl(rlwe._view(ins[c], j, 1), v)
            for i in range(min((nj - 1).bit_length(), g)):                           # :985
                step = 1 << (i + 1)
                t = rlwe._view(xinv, i, 1)
                for j0 in range(0, nj, step):
                    for k in range(step >> 1, step):
                        if j0 + k >= nj:
                            break
                        ring.MulCoeffsMontgomery(cts[j0 + k], t, cts[j0 + k])


class Parameters:
    """bootstrapping.Parameters (parameters.go:18-35) from explicit pieces.  ringQ / ringP: the rings of BootstrappingParameters, whose first
    ResidualMaxLevel + 1 moduli are ResidualParameters.Q; ResidualDefaultScale / BootstrappingDefaultScale: the two DefaultScale();
    the three literals as the reference holds them; EphemeralSecretWeight: 0 without sparse-secret encapsulation."""

    def __init__(self, ringQ, ringP, ResidualMaxLevel, ResidualDefaultScale, SlotsToCoeffsParameters, Mod1ParametersLiteral, CoeffsToSlotsParameters,
                 EphemeralSecretWeight=32, BootstrappingDefaultScale=None, CircuitOrder=ModUpThenEncode, IterationsParameters=None,
                 ResidualRingType=Standard, ResidualN=None, PrecisionMode=PREC64, ResidualRingQ=None, BootstrappingSecretWeight=None):
        """ResidualRingQ: the ring handle of ResidualParameters (degree N1, Standard or ConjugateInvariant) when it is not the bootstrapping ring
        itself: its moduli are Q[:ResidualMaxLevel + 1], and ResidualN / ResidualRingType follow from it (Bootstrapper reads it).
        BootstrappingSecretWeight: the Hamming weight of the ephemeral secret GenEvaluationKeys samples when N1 != N2; None: the ternary law."""
        self.ringQ, self.ringP, self.ResidualMaxLevel = ringQ, ringP, int(ResidualMaxLevel)
        self.ResidualRingQ, self.BootstrappingSecretWeight = ResidualRingQ, BootstrappingSecretWeight
        if ResidualRingQ is not None:
            if [int(q) for q in ResidualRingQ.moduli] != [int(q) for q in ringQ.moduli[:self.ResidualMaxLevel + 1]]:
                raise RingHipError("cannot NewParameters: the moduli of ResidualRingQ are not Q[:ResidualMaxLevel + 1] of the bootstrapping parameters")
            if ResidualRingQ.kind not in (Standard, ConjugateInvariant):
                raise RingHipError("cannot NewParameters: ResidualRingQ must be a standard or a conjugate-invariant ring")
            ResidualRingType, ResidualN = ResidualRingQ.kind, ResidualRingQ.N
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

    def GenEvaluationKeys(self, skN1, prng=None, samples=None, xe=(3.2, 19)):
        """keys.go:69-144 -> (EvaluationKeys, skN2), every key made on the device by the key layer's own calls, in the reference's order: the
        ephemeral secret and the keys between the rings (N1 != N2), or skN1 extended to all of Q and P (N1 == N2:
        ExtendBasisSmallNormAndCenterNTTMontgomery, here the small coefficients -- the key's own, or INTT / IMForm of limb 0 centred -- lifted
        under QP); the two encapsulation keys; the relinearisation key; the Galois keys of GaloisElements() (the conjugation among them) in one
        launch sequence.  samples: {name: what that key-layer call takes as samples} for any of "skN2", "EvkN1ToN2", "EvkN2ToN1", "RingSwap"
        (a pair), "skSparse", "EvkDenseToSparse", "EvkSparseToDense", "rlk", "galois"."""
        from .keygen import centred_coeffs
        from .ringhip import Ring
        from .sampling import SmallPoly
        samples = samples or {}
        rq, rp = self.ringQ, self.ringP
        kgen = rlwe.KeyGenerator(rq, rp, xe=xe, prng=prng)
        prng = kgen.prng
        N1to2 = N2to1 = RtoC = CtoR = None
        if self.ResidualN != rq.N:
            if "skN2" in samples or self.BootstrappingSecretWeight is None:
                skN2 = kgen.GenSecretKeyNew(samples.get("skN2"))
            else:
                skN2 = kgen.GenSecretKeyWithHammingWeightNew(self.BootstrappingSecretWeight)
            if self.ResidualRingType == ConjugateInvariant:
                CtoR, RtoC = kgen.GenEvaluationKeysForRingSwapNew(skN2, skN1, samples=samples.get("RingSwap"))
            else:
                N1to2 = kgen.GenEvaluationKeyNew(skN1, skN2, samples=samples.get("EvkN1ToN2"))
                N2to1 = kgen.GenEvaluationKeyNew(skN2, skN1, samples=samples.get("EvkN2ToN1"))
        else:
            if skN1.Value.Q.ring.N != rq.N or skN1.Value.Q.ring.kind != Standard:
                raise RingHipError("cannot GenEvaluationKeys: skN1 is not a secret of the standard ring of degree %d" % rq.N)
            c = centred_coeffs(skN1)
            skN2 = kgen._secret_from(SmallPoly.from_numpy(rq, np.asarray(c, dtype=np.int32).reshape(1, -1)))
        d2s = s2d = None
        if self.EphemeralSecretWeight != 0:                                                           # genEncapsulationEvaluationKeysNew (:123-144)
            q0 = Ring(rq.N, [int(rq.moduli[0])], device=rq.device)
            p0 = Ring(rq.N, [int(rp.moduli[0])], device=rq.device)
            kgenSparse = rlwe.KeyGenerator(q0, p0, xe=xe, prng=prng)
            if "skSparse" in samples:
                skSparse = kgenSparse.GenSecretKeyNew(samples["skSparse"])
            else:
                skSparse = kgenSparse.GenSecretKeyWithHammingWeightNew(self.EphemeralSecretWeight)
            small = SmallPoly.from_numpy(rq, np.asarray(centred_coeffs(skSparse), dtype=np.int32).reshape(1, -1))
            d2s = kgenSparse.GenEvaluationKeyNew(skN2, skSparse, samples=samples.get("EvkDenseToSparse"))       # limb 0 of skN2 is read
            s2d = kgen.GenEvaluationKeyNew(kgen._secret_from(small), skN2, samples=samples.get("EvkSparseToDense"))
        rlk = kgen.GenRelinearizationKeyNew(skN2, samples=samples.get("rlk"))
        galEls = [g for g in self.GaloisElements() if g != 1]
        gks = kgen.GenGaloisKeysNew(galEls, skN2, samples=samples.get("galois"))
        return EvaluationKeys(rlk, dict(zip(galEls, gks)), d2s, s2d, N1to2, N2to1, RtoC, CtoR), skN2


class EvaluationKeys:
    """bootstrapping.EvaluationKeys (keys.go:33-41) as far as this path reads them: the relinearisation key and the Galois keys
    (rlwe.GadgetCiphertext over ringQ, ringP) and the two encapsulation keys -- EvkDenseToSparse over the one-limb rings of Q[:1] and P[:1]
    (keys.go:131-141), EvkSparseToDense over ringQ, ringP"""

    def __init__(self, rlk=None, galois_keys=None, EvkDenseToSparse=None, EvkSparseToDense=None, EvkN1ToN2=None, EvkN2ToN1=None,
                 EvkRealToCmplx=None, EvkCmplxToReal=None):
        self.rlk, self.galois_keys = rlk, dict(galois_keys or {})
        self.EvkDenseToSparse, self.EvkSparseToDense = EvkDenseToSparse, EvkSparseToDense
        self.EvkN1ToN2, self.EvkN2ToN1 = EvkN1ToN2, EvkN2ToN1                     # Bootstrapper: the ring-degree switch (keys.go:33-41)
        self.EvkRealToCmplx, self.EvkCmplxToReal = EvkRealToCmplx, EvkCmplxToReal # Bootstrapper: the ring-type switch


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


class _PackingContext:
    """packingContext (:871-876): the ring packed in and its LogMaxSlots, the dimension packed up to, the ciphertexts' own, their number"""

    def __init__(self, ring, ParamsLogMaxSlots, LogMaxDimensions, LogSlots, NbPackedCTs):
        self.ring, self.ParamsLogMaxSlots, self.LogMaxDimensions, self.LogSlots, self.NbPackedCTs = ring, ParamsLogMaxSlots, LogMaxDimensions, LogSlots, NbPackedCTs


class _SwitcherParameters:
    """what ckks.DomainSwitcher reads of its parameters"""

    def __init__(self, ring):
        self.ring, self.device = ring, ring.device

    def RingQ(self):
        return self.ring

    def RingType(self):
        return self.ring.kind


class Bootstrapper:
    """The Bootstrapper interface (bootstrapper.go) over bootstrapping.Evaluator: BootstrapMany (evaluator.go:259-314) with the arms Evaluator
    refuses -- ciphertexts packed more sparsely than the bootstrapping (pack / unpack, :965-1065), ResidualParameters.N != BootstrappingParameters.N
    (PackAndSwitchN1ToN2 / UnpackAndSwitchN2ToN1, :880-961) and conjugate-invariant residual parameters (EvaluateConjugateInvariant, :493-538).
    It owns one inner Evaluator over the standard ring of degree N2 (the same parameters with ResidualRingType = Standard, ResidualN = N2 and,
    for a conjugate-invariant residual ring, SlotsToCoeffsParameters.Scaling = 0.5, :71): every core step is that evaluator's.

    A batch of n ciphertexts is one Ciphertext with npoly = n; all share level, scale and LogDimensions (the per-pair min(level) of :1042 is
    moot).  BootstrapMany returns a batch of n at OutputLevel() with Scale = ResidualDefaultScale and leaves its input as it was; the packed
    ciphertexts go through Evaluate as ONE batch.  On a conjugate-invariant residual ring the whole batch is switched by one RealToComplex,
    pairs (2 j, 2 j + 1) are folded into c_2j + i c_2j+1 (the last one alone when n is odd: the nil arm), bootstrapped, unfolded to
    [x_j, -i x_j] and switched back by one ComplexToReal.

    The pack tables are made at the residual ring's full level and read at the input's level (the reference makes them at level 0 only, :77,
    :80, so its pack serves level-0 inputs; at level 0 the words are the reference's).

    fused: None what FUSED_BOOTSTRAP_MANY (and, for the inner evaluator, mod1.Evaluator.FUSED_BOOTSTRAP) says, else True / False for every choice:
      pack, unpack             rh_ckks_bootstrap_pack / _unpack, or MulCoeffsMontgomeryThenAdd per pair and level / CopyLvl + MulCoeffsMontgomery
      pair_fold, pair_unfold   the same kernels with a group of 2 and the one row NTT(X^(N/2)) (its negation), or Mul(ct, +-1i) and Add
    -- the same bits either way.

    Refused by name: IterationsParameters (META-BTS) and PREC128, the DecodeThenModUp and Custom orders, missing switch keys (the reference's
    text), and what the inner evaluator refuses."""

    def __init__(self, parameters, keys, fused=None):
        p = self.Parameters = parameters
        who = "cannot NewBootstrapper"
        if p.IterationsParameters is not None:
            raise RingHipError("%s: IterationsParameters (META-BTS iterations, the reserved prime) are not built on the device path" % who)
        if p.PrecisionMode != PREC64:
            raise RingHipError("%s: PREC128 residual parameters are not built on the device path" % who)
        self.N2, self.N1, self.ci = p.ringQ.N, p.ResidualN, p.ResidualRingType == ConjugateInvariant
        if p.ResidualRingType not in (Standard, ConjugateInvariant) or p.ringQ.kind != Standard:
            raise RingHipError("%s: a standard bootstrapping ring and a standard or conjugate-invariant residual ring" % who)
        missing = "%s: evk.(BootstrappingKeys) is missing EvkN1ToN2 and EvkN2ToN1" % who                  # :55-63, both arms with this text
        if self.ci:
            if keys.EvkCmplxToReal is None or keys.EvkRealToCmplx is None:
                raise RingHipError(missing)
            if 2 * self.N1 != self.N2:
                raise RingHipError("%s: a conjugate-invariant residual ring has degree N2 / 2 = %d, not %d" % (who, self.N2 // 2, self.N1))
        elif self.N1 != self.N2 and (keys.EvkN1ToN2 is None or keys.EvkN2ToN1 is None):
            raise RingHipError(missing)
        if self.N1 != self.N2 and p.ResidualRingQ is None:
            raise RingHipError("%s: ResidualParameters.N = %d != BootstrappingParameters.N = %d needs Parameters.ResidualRingQ, the ring of degree N1"
                               % (who, self.N1, self.N2))
        if self.N1 > self.N2:
            raise RingHipError("%s: ResidualParameters.N = %d > BootstrappingParameters.N = %d" % (who, self.N1, self.N2))
        self.fused = dict(FUSED_BOOTSTRAP_MANY) if fused is None else {k: bool(fused) for k in FUSED_BOOTSTRAP_MANY}
        s2c = p.SlotsToCoeffsParameters
        if self.ci:                                                                                       # the switch to the conjugate-invariant ring doubles the scale (:70-71)
            s2c = dft.MatrixLiteral(s2c.Type, s2c.LogSlots, s2c.LevelQ, s2c.LevelP, s2c.Levels, s2c.Format, 0.5, s2c.BitReversed, s2c.LogBSGSRatio)
        inner = Parameters(p.ringQ, p.ringP, p.ResidualMaxLevel, p.ResidualDefaultScale, s2c, p.Mod1ParametersLiteral, p.CoeffsToSlotsParameters,
                           EphemeralSecretWeight=p.EphemeralSecretWeight, BootstrappingDefaultScale=p.BootstrappingDefaultScale, CircuitOrder=p.CircuitOrder)
        self.Evaluator = Evaluator(inner, keys, fused=fused)
        self.EvaluationKeys = keys
        res = p.ResidualMaxLevel
        self.ringN2 = p.ringQ.AtLevel(res)
        self.ringN1 = p.ResidualRingQ if self.N1 != self.N2 else None
        logN2 = self.N2.bit_length() - 1
        self.xPow2N2, self.xPow2InvN2 = rlwe.GenXPow2NTT(self.ringN2, logN2, False), rlwe.GenXPow2NTT(self.ringN2, logN2, True)
        self.xPow2N1 = self.xPow2InvN1 = None
        if self.ringN1 is not None and not self.ci:
            logN1 = self.N1.bit_length() - 1
            self.xPow2N1, self.xPow2InvN1 = rlwe.GenXPow2NTT(self.ringN1, logN1, False), rlwe.GenXPow2NTT(self.ringN1, logN1, True)
        self._tables = {}
        self.DomainSwitcher = self._switch_eval = self._switch_ring = None
        if self.ci:
            # the ring-swap keys are made at the secrets' common level, the residual one: the switch runs on an evaluator over Q[:ResidualMaxLevel + 1]
            from .ringhip import Ring
            self._switch_ring = Ring(self.N2, [int(q) for q in p.ringQ.moduli[:res + 1]], device=p.ringQ.device)
            self._switch_eval = CkksEvaluator(self._switch_ring, p.ringP)
            self.DomainSwitcher = DomainSwitcher(_SwitcherParameters(self._switch_ring), keys.EvkCmplxToReal, keys.EvkRealToCmplx)
            self._i = pack_table(self.ringN2, self.xPow2N2, logN2 - 1, 1)                               # NTT(X^(N/2)), Montgomery form: i
            self._minus_i = self.ringN2.NewPoly(1)
            self.ringN2.Neg(self._i, self._minus_i)

    def close(self):
        self.Evaluator.close()
        if self.DomainSwitcher is not None:
            self.DomainSwitcher.close()
            self._switch_eval.close()
            self._switch_ring.close()

    def Depth(self):
        return self.Evaluator.Depth()

    def OutputLevel(self):
        return self.Evaluator.OutputLevel()

    def MinimumInputLevel(self):
        return self.Evaluator.MinimumInputLevel()

    # ---- Bootstrap :249-256, BootstrapMany :259-314 ----
    def Bootstrap(self, ct):
        return self.BootstrapMany(ct)

    def BootstrapMany(self, cts):
        who = "cannot BootstrapMany"
        if getattr(cts, "LogDimensions", None) is None:
            raise RingHipError("%s: a ciphertext carries no LogDimensions" % who)
        try:
            if self.ci:
                out = self.EvaluateConjugateInvariant(cts)
            else:
                packed, ctxt1, ctxt2 = self.PackAndSwitchN1ToN2(cts)
                out = self.UnpackAndSwitchN2ToN1(self.Evaluator.Evaluate(packed), ctxt1, ctxt2)
        except RingHipError as e:
            if str(e).startswith(who):
                raise
            raise RingHipError("%s: %s" % (who, e)) from e
        out.Scale = self.Parameters.ResidualDefaultScale
        return out

    # ---- the tables ----
    def _table(self, ring, powers, logGap, g, tag):
        key = (tag, logGap, g)
        if key not in self._tables:
            self._tables[key] = pack_table(ring, powers, logGap, g)
        return self._tables[key]

    @staticmethod
    def _like(ct, value):
        out = Ciphertext(value, is_ntt=ct.IsNTT)
        out.Scale, out.LogDimensions = ct.Scale if isinstance(ct.Scale, Scale) else Scale(ct.Scale), getattr(ct, "LogDimensions", None)
        for name in ("IsBatched", "IsMontgomery"):
            if hasattr(ct, name):
                setattr(out, name, getattr(ct, name))
        return out

    # ---- pack :1008-1065, unpack :965-1004 on a batch ----
    def pack(self, cts, ctxt, powers, tag):
        logSlots, logMaxSlots = ctxt.LogSlots, ctxt.LogMaxDimensions
        if logSlots > logMaxSlots:
            raise RingHipError("cannot Pack: cts[0].LogSlots()=%d > logMaxSlots=%d" % (logSlots, logMaxSlots))
        if cts.Value[0].ring.N != ctxt.ring.N:
            raise RingHipError("cannot Pack: cts[0].Value[0].N()=%d != params.N()=%d" % (cts.Value[0].ring.N, ctxt.ring.N))
        g = logMaxSlots - logSlots
        if g == 0:
            return cts
        if not cts.IsNTT or cts.Degree() != 1:
            raise RingHipError("cannot Pack: degree-1 ciphertexts in the NTT domain")
        logGap = ctxt.ParamsLogMaxSlots - logSlots - 1
        n, level = cts.Value[0].npoly, cts.Level()
        if level > ctxt.ring.level:
            raise RingHipError("cannot Pack: the ciphertexts are at level %d, above the residual level %d" % (level, ctxt.ring.level))
        ring = ctxt.ring.AtLevel(level)
        xp = self._table(ctxt.ring, powers, logGap, g, tag)
        outs = [ring.NewPoly(-(-n >> g)) for _ in (0, 1)]
        (bootstrap_pack if self.fused["pack"] else pack_composed)(ring, g, cts.Value, outs, xp)
        out = self._like(cts, outs)
        out.LogDimensions = logMaxSlots                                                                # :1060-1062
        return out

    def unpack(self, cts, ctxt, powers, tag):
        """every packed ciphertext of the batch (:922-931): NbPackedCTs ciphertexts come out, min(what is left, 2^logPackCTs) of each"""
        g = ctxt.LogMaxDimensions - ctxt.LogSlots
        if g == 0:
            ctxt.NbPackedCTs -= cts.Value[0].npoly
            return cts
        n, level = ctxt.NbPackedCTs, cts.Level()
        if cts.Value[0].npoly != -(-n >> g):
            raise RingHipError("cannot Unpack: %d ciphertexts of 2^%d each do not hold %d" % (cts.Value[0].npoly, g, n))
        logGap = ctxt.ParamsLogMaxSlots - ctxt.LogSlots - 1
        ring = ctxt.ring.AtLevel(level)
        xinv = self._table(ctxt.ring, powers, logGap, g, tag)
        outs = [ring.NewPoly(n) for _ in (0, 1)]
        if self.fused["unpack"]:
            bootstrap_unpack(ring, g, n, cts.Value, outs, xinv)
        else:
            unpack_composed(ring, g, n, cts.Value, outs, xinv)
        ctxt.NbPackedCTs -= n
        return self._like(cts, outs)

    # ---- :826-846 ----
    def _switch_degree(self, ct, evk, ring):
        out = self._like(ct, [ring.AtLevel(ct.Level()).NewPoly(ct.Value[0].npoly) for _ in (0, 1)])
        self.Evaluator.Evaluator.ks.ApplyEvaluationKey(ct, evk, out)
        out.Scale, out.LogDimensions = ct.Scale, ct.LogDimensions
        return out

    # ---- PackAndSwitchN1ToN2 :880-911, UnpackAndSwitchN2ToN1 :915-961 ----
    def PackAndSwitchN1ToN2(self, cts):
        p = self.Parameters
        packN1 = None
        n = cts.Value[0].npoly
        if self.N1 != self.N2:
            logMaxN1 = self.N1.bit_length() - 2
            packN1 = _PackingContext(self.ringN1, logMaxN1, min(logMaxN1, p.LogMaxSlots()), cts.LogDimensions, n)
            try:
                cts = self.pack(cts, packN1, self.xPow2N1, "N1")
            except RingHipError as e:
                raise RingHipError("cannot PackAndSwitchN1ToN2: PackN1: %s" % e) from e
            cts = self._switch_degree(cts, self.EvaluationKeys.EvkN1ToN2, p.ringQ)
        packN2 = _PackingContext(self.ringN2, self.N2.bit_length() - 2, p.LogMaxSlots(), cts.LogDimensions, cts.Value[0].npoly)
        try:
            cts = self.pack(cts, packN2, self.xPow2N2, "N2")
        except RingHipError as e:
            raise RingHipError("cannot PackAndSwitchN1ToN2: PackN1: %s" % e) from e                     # the reference's text, as written (:907)
        return cts, packN1, packN2

    def UnpackAndSwitchN2ToN1(self, cts, ctxtN1, ctxtN2):
        logSlots = ctxtN2.LogSlots
        out = self.unpack(cts, ctxtN2, self.xPow2InvN2, "N2inv")
        if ctxtN1 is not None:
            logSlots = ctxtN1.LogSlots
            out = self._switch_degree(out, self.EvaluationKeys.EvkN2ToN1, self.ringN1)
            out = self.unpack(out, ctxtN1, self.xPow2InvN1, "N1inv")
        if out is cts:
            out = self._like(cts, cts.Value)
        out.LogDimensions = logSlots                                                                   # :956-958
        return out

    # ---- :848-868 ----
    def _rewrap(self, ct, ring):
        """the same device blocks as polys of `ring` (the switcher works over its own handles of the same degree and moduli)"""
        out = self._like(ct, [DevicePoly(ring.AtLevel(v.limbs - 1), v.npoly, v.limbs, ptr=v.ptr, owner=v) for v in ct.Value])
        return out

    def RealToComplexNew(self, ctReal):
        if self.DomainSwitcher is None:
            raise RingHipError("cannot RealToComplex: the residual parameters are not conjugate-invariant")
        out = self.DomainSwitcher.RealToComplexNew(self._switch_eval, ctReal)
        return self._rewrap(out, self.Parameters.ringQ)

    def ComplexToRealNew(self, ctCmplx):
        if self.DomainSwitcher is None:
            raise RingHipError("cannot ComplexToReal: the residual parameters are not conjugate-invariant")
        out = self.DomainSwitcher.ComplexToRealNew(self._switch_eval, self._rewrap(ctCmplx, self._switch_ring))
        return self._rewrap(out, self.Parameters.ResidualRingQ)

    # ---- EvaluateConjugateInvariant :493-538 on a batch: pairs (2 j, 2 j + 1) ----
    def _views(self, ct, first, count=1):
        return self._like(ct, [rlwe._view(v, first, count) for v in ct.Value])

    def pair_fold(self, std):
        """:502-514 for every pair of the batch: c_2j + i c_2j+1; the last one alone when the batch is odd"""
        n, level = std.Value[0].npoly, std.Level()
        ring = self.Parameters.ringQ.AtLevel(level)
        outs = [ring.NewPoly((n + 1) >> 1) for _ in (0, 1)]
        out = self._like(std, outs)
        if self.fused["pair_fold"]:
            bootstrap_pack(ring, 1, std.Value, outs, self._i)
            return out
        ev = self.Evaluator.Evaluator
        for j in range(n >> 1):
            right = ev.MulNew(self._views(std, 2 * j + 1), 1j)
            ev.Add(self._views(std, 2 * j), right, self._views(out, j))
        if n & 1:
            for c in (0, 1):
                ring.CopyLvl(rlwe._view(std.Value[c], n - 1, 1), rlwe._view(outs[c], n >> 1, 1))
        return out

    def pair_unfold(self, std, n):
        """:527-535: [x_j, -i x_j] for every bootstrapped pair, the absent last right-hand one dropped"""
        level = std.Level()
        ring = self.Parameters.ringQ.AtLevel(level)
        outs = [ring.NewPoly(n) for _ in (0, 1)]
        out = self._like(std, outs)
        if self.fused["pair_unfold"]:
            bootstrap_unpack(ring, 1, n, std.Value, outs, self._minus_i)
            return out
        ev = self.Evaluator.Evaluator
        for j in range(std.Value[0].npoly):
            for c in (0, 1):
                ring.CopyLvl(rlwe._view(std.Value[c], j, 1), rlwe._view(outs[c], 2 * j, 1))
            if 2 * j + 1 < n:
                ev.Mul(self._views(std, j), -1j, self._views(out, 2 * j + 1))
        return out

    def EvaluateConjugateInvariant(self, cts):
        """a batch over the conjugate-invariant ring of degree N2 / 2 -> the batch bootstrapped, at OutputLevel()"""
        if cts is None:
            raise RingHipError("ctLeftN1Q0 cannot be nil")
        if not self.ci:
            raise RingHipError("cannot EvaluateConjugateInvariant: the residual parameters are not conjugate-invariant")
        if cts.Value[0].ring.N != self.N1:
            raise RingHipError("cannot EvaluateConjugateInvariant: the ciphertexts have ring degree %d, the residual parameters %d" % (cts.Value[0].ring.N, self.N1))
        n = cts.Value[0].npoly
        std = self.RealToComplexNew(cts)
        std.LogDimensions = cts.LogDimensions
        both = self.Evaluator.Evaluate(self.pair_fold(std))
        both.Scale = both.Scale.Mul(Scale(Fraction(1, 2)))                                              # :524
        out = self.ComplexToRealNew(self.pair_unfold(both, n))
        out.LogDimensions = cts.LogDimensions
        return out


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

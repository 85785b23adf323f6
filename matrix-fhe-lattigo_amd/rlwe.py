"""Host-side mirror of the key-switch callers in core/rlwe: the evaluator methods that
sequence the ring hot path for rotations and relinearisation, on device-resident batches.  Every step is a call into
the HIP library.  Key generation, encryption and decryption: keygen.py and sampling.py, re-exported at the end of this module.

  GadgetProduct          core/rlwe/evaluator_gadget_product.go:16-30
  DecomposeNTT           :431-453        GadgetProductHoisted   :326-349
  Automorphism           core/rlwe/evaluator_automorphism.go:14-60      AutomorphismHoisted  :62-105
  ApplyEvaluationKey     core/rlwe/evaluator_evaluationkey.go:37-123 (also between ring degrees)   Relinearize  :125-153

GadgetProduct covers both branches of GadgetProductLazy (:102-121): gadgetProductMultiplePLazy (levelP >= 1) and
gadgetProductSinglePAndBitDecompLazy (levelP <= 0, optional BaseTwoDecomposition), for NTT- and coefficient-domain ciphertexts.
The hoisted forms and the automorphism / relinearisation callers take NTT-domain ciphertexts and levelP >= 1; Automorphism alone also takes
keys of levelP <= 0 (single P, or no P with a power-of-two decomposition) through GadgetProduct, ringQ.Add and AutomorphismNTT.

  PartialTracesSum       core/rlwe/inner_sum.go:152-291     Trace  :36-121     InnerFunction  :316-440     Replicate  :477-479
  GaloisElementsForInnerSum  :444-468     GaloisElementsForReplicate  :483-485     GaloisElementsForTrace  :125-146

The sums of rotations take NTT- and coefficient-domain ciphertexts on standard rings, keys with levelP >= 1 and no power-of-two decomposition.

  RingPackingEvaluator   core/rlwe/ring_packing.go: Expand :475-594, Pack :623-793, Split :193-258, Merge :396-464, Extract :70-189, Repack :260-392
  GenXPow2NTT  :795-833     GaloisElementsForExpand / ForPack  core/rlwe/ring_packing_keys.go:143-180
  SwitchCiphertextRingDegreeNTT  core/rlwe/element.go:250-287     SwitchCiphertextRingDegree  :293-312 (to the smaller degree)

Ring packing takes standard rings and every key GadgetProduct takes; Expand and Pack take NTT- and coefficient-domain ciphertexts, Split and Merge
NTT-domain ones."""
import numpy as np

from .ringhip import BasisExtender, DevicePoly, GaloisKeyEntry, RingHipError, Standard, U64P, _check, lib
from .schemes import Ciphertext

GaloisGen = 5                                                          # ring.GaloisGen (ring/ring.go:17-19)
METADATA = ("Scale", "LogDimensions", "IsMontgomery", "IsBatched")     # what the scheme layers hang on a Ciphertext besides IsNTT


def GaloisElement(N, k, NthRoot=None):
    """Parameters.GaloisElement (core/rlwe/params.go:671-675): GaloisGen^k mod NthRoot (2N on a standard ring), a negative k taken modulo NthRoot"""
    NthRoot = 2 * int(N) if NthRoot is None else int(NthRoot)
    return pow(GaloisGen, int(k) % NthRoot, NthRoot)


def GaloisElementsForInnerSum(N, batch, n):
    """(:444-468): the Galois elements of the rotations i batch and (n - (n & (2i - 1))) batch for i = 1, 2, 4 ... < n, sorted.  A superset of what
    PartialTracesSum(batch, n) applies: the reference lists the rotation by 0 (element 1) when it occurs and the last power of two too."""
    rot = set()
    i = 1
    while i < n:
        rot.add(i * batch)
        rot.add((n - (n & ((i << 1) - 1))) * batch)
        i <<= 1
    return sorted({GaloisElement(N, k) for k in rot})


def GaloisElementsForReplicate(N, batch, n):
    """(:483-485)"""
    return GaloisElementsForInnerSum(N, -batch, n)


def GaloisElementsForTrace(N, logN, kind=Standard):
    """(:125-146): 5^(2^i) for logN <= i < log2(N) - 1, and 2N - 1 for the full trace (logN = 0) of a standard ring"""
    if kind != Standard:
        raise RingHipError("cannot GaloisElementsForTrace: standard rings only on the device path")
    top = int(N).bit_length() - 1
    out = [GaloisElement(N, 1 << i) for i in range(logN, top - 1)]
    if logN == 0:
        out.append(2 * int(N) - 1)                                    # GaloisElementOrderTwoOrthogonalSubgroup
    return out


LAZY, CLOSE, DOUBLE = "lazy", "close", "double"


def partial_traces_plan(N, offset, n):
    """The binary reading of n in PartialTracesSum (:216-282) as a list of steps (kind, Galois element, decompose):
    LAZY accQP (+)= AutomorphismHoistedLazy(ctInNTT, g); CLOSE opOut = ModDown(accQP) + ctInNTT, or ctInNTT when n is a power of two;
    DOUBLE ctInNTT += AutomorphismHoisted(ctInNTT, g).  decompose: the step is the first of its iteration to read DecomposeNTT(ctInNTT[1]) --
    the reference decomposes at the top of EVERY iteration, the last one for nothing (nothing reads it after CLOSE)."""
    plan, state, i, j = [], False, 0, n
    while j > 0:
        fresh = True
        if j & 1:
            k = (n - (n & ((2 << i) - 1))) * offset
            if k != 0:
                plan.append((LAZY, GaloisElement(N, k), fresh))
                fresh = False
            else:
                state = True
                plan.append((CLOSE, 0, False))
        if not state:
            plan.append((DOUBLE, GaloisElement(N, (1 << i) * offset), fresh))
        i, j = i + 1, j >> 1
    return plan


class GadgetCiphertext:
    """rlwe.GadgetCiphertext (core/rlwe/gadgetciphertext.go:17-45) in the layout the kernels read:
    Q part [digit][component < 2][limb of ringQ][N], P part [digit][component][limb of ringP][N], NTT domain, Montgomery
    form, shared by every ciphertext of a batch."""

    def __init__(self, ringQ, ringP, valueQ, valueP, BaseTwoDecomposition=0, digits_per_limb=None):
        """valueQ / valueP: (rows, 2, limbs, N).  rows = RNS digits; with a power-of-two decomposition (BaseTwoDecomposition > 0,
        at most one P modulus) row sum(digits_per_limb[:i]) + j holds Value[i][j] and digits_per_limb[i] = len(Value[i]).
        ringP / valueP may be None: a gadget ciphertext without P (LevelP() == -1)."""
        valueQ = np.asarray(valueQ, dtype=np.uint64)
        if valueQ.ndim != 4 or valueQ.shape[1] != 2 or valueQ.shape[2] != ringQ.L:
            raise RingHipError("GadgetCiphertext: expected a (rows, 2, limbs of ringQ, N) array for Q")
        self.digits = valueQ.shape[0]
        self.Q = DevicePoly.from_numpy(ringQ, valueQ.reshape(self.digits * 2, ringQ.L, ringQ.N))
        self.P = None
        if ringP is not None:
            valueP = np.asarray(valueP, dtype=np.uint64)
            if valueP.ndim != 4 or valueP.shape[:2] != valueQ.shape[:2] or valueP.shape[2] != ringP.L:
                raise RingHipError("GadgetCiphertext: expected a (rows, 2, limbs of ringP, N) array for P")
            self.P = DevicePoly.from_numpy(ringP, valueP.reshape(self.digits * 2, ringP.L, ringP.N))
        self.levelQ, self.levelP = ringQ.L - 1, (ringP.L - 1 if ringP is not None else -1)
        self.BaseTwoDecomposition = int(BaseTwoDecomposition)
        self.digits_per_limb = list(digits_per_limb) if digits_per_limb is not None else None
        if self.BaseTwoDecomposition and (self.levelP > 0 or self.digits_per_limb is None or sum(self.digits_per_limb) != self.digits):
            raise RingHipError("GadgetCiphertext: BaseTwoDecomposition needs at most one P modulus and digits_per_limb summing to the row count")

    @classmethod
    def from_device(cls, ringQ, ringP, Q, P, BaseTwoDecomposition=0, digits_per_limb=None):
        """a gadget ciphertext over tables that are already on the device (keygen.KeyGenerator): Q a DevicePoly of (rows * 2, limbs of ringQ, N),
        P likewise under ringP or None; nothing is copied"""
        if Q.npoly % 2 or Q.limbs != ringQ.level + 1:
            raise RingHipError("GadgetCiphertext: expected a (rows * 2, limbs of ringQ, N) device block for Q")
        if (ringP is None) != (P is None) or (P is not None and (P.npoly != Q.npoly or P.limbs != ringP.level + 1)):
            raise RingHipError("GadgetCiphertext: expected a (rows * 2, limbs of ringP, N) device block for P")
        self = object.__new__(cls)
        self.digits, self.Q, self.P = Q.npoly // 2, Q, P
        self.levelQ, self.levelP = Q.limbs - 1, (P.limbs - 1 if P is not None else -1)
        self.BaseTwoDecomposition = int(BaseTwoDecomposition)
        self.digits_per_limb = list(digits_per_limb) if digits_per_limb is not None else None
        if self.BaseTwoDecomposition and (self.levelP > 0 or self.digits_per_limb is None or sum(self.digits_per_limb) != self.digits):
            raise RingHipError("GadgetCiphertext: BaseTwoDecomposition needs at most one P modulus and digits_per_limb summing to the row count")
        return self

    def LevelQ(self):
        return self.levelQ

    def LevelP(self):
        return self.levelP


class PolyQP:
    """ringqp.Poly: the Q part and the P part of one polynomial of the extended ring (ring/ringqp/poly.go)"""

    def __init__(self, Q, P):
        self.Q, self.P = Q, P


class ElementQP:
    """Element[ringqp.Poly] as the lazy key-switch routines use it: Value[0..1] of PolyQP batches and the NTT flag"""

    def __init__(self, value, is_ntt=True):
        self.Value = list(value)
        self.IsNTT = bool(is_ntt)

    @classmethod
    def alloc(cls, ringQ, ringP, npoly, levelQ, levelP):
        mk = lambda: PolyQP(DevicePoly(ringQ.AtLevel(levelQ), npoly, levelQ + 1), DevicePoly(ringP.AtLevel(levelP), npoly, levelP + 1))
        return cls([mk(), mk()], True)

    def LevelP(self):
        return self.Value[0].P.limbs - 1

    def LevelQ(self):
        return self.Value[0].Q.limbs - 1


class Evaluator:
    """rlwe.Evaluator restricted to the key-switch path; `galois_keys` maps a Galois element to its GadgetCiphertext."""

    def __init__(self, ringQ, ringP=None, galois_keys=None):
        self.ringQ, self.ringP = ringQ, ringP
        self.be = BasisExtender(ringQ, ringP)
        self.galois_keys = dict(galois_keys or {})
        self._pool = {}

    def close(self):
        self._pool.clear()
        self.be.close()

    def buffer(self, tag, ring, npoly, limbs):
        """evaluator-owned scratch poly (the reference's eval.BuffQP / BuffCt): allocated once per shape, reused by every call --
        no hipMalloc / hipFree (and their implicit synchronisation) on the hot path.  Not thread-safe, like the reference's
        buffers (use one Evaluator per thread: Evaluator.ShallowCopy in the reference)."""
        key = (tag, id(ring._h), npoly, limbs)
        p = self._pool.get(key)
        if p is None:
            p = self._pool[key] = DevicePoly(ring, npoly, limbs)
        return p

    @staticmethod
    def _rows(level, *polys):
        """device blocks are strided by level+1 rows per poly (ringhip.h): a batch allocated with more limbs than the level
        it is used at would be read with the wrong stride -- refuse it (a single poly's leading limbs are contiguous)"""
        for p in polys:
            if p is None:
                continue
            if getattr(p, "layout", None) == "block":      # 3N rings: the key-switch kernels and the keys speak the reference's order
                p.ring.ToReferenceOrder(p)
            if p.limbs < level + 1 or (p.limbs != level + 1 and p.npoly > 1):
                raise RingHipError("batch of %d polys with %d limbs used at level %d: allocate it at that level" % (p.npoly, p.limbs, level))

    # ---- core/rlwe/evaluator_gadget_product.go ---------------------------------------------------------------
    def GadgetProduct(self, levelQ, cx, gadgetCt, ct):
        """ct = (<decomp(cx), gadget[0]>, <decomp(cx), gadget[1]>) / P mod Q (:16-30).  ct.IsNTT tells the domain of cx and of the
        result (:14); gadgetCt.LevelP() >= 1 takes gadgetProductMultiplePLazy, <= 0 the single-P / bit-decomposition branch (:109-113)"""
        import ctypes as C
        levelQ = min(levelQ, gadgetCt.LevelQ())
        self._rows(levelQ, cx, ct.Value[0], ct.Value[1])
        L, lp = lib(), gadgetCt.LevelP()
        pP = gadgetCt.P.ptr if gadgetCt.P is not None else None
        if lp >= 1 and ct.IsNTT:
            _check(L.rh_bext_gadget_product(self.be._h, levelQ, lp, cx.ptr, gadgetCt.Q.ptr, pP, gadgetCt.digits, ct.Value[0].ptr, ct.Value[1].ptr, cx.npoly))
        elif lp >= 1:
            _check(L.rh_bext_gadget_product_coeff(self.be._h, levelQ, lp, cx.ptr, gadgetCt.Q.ptr, pP, gadgetCt.digits, ct.Value[0].ptr, ct.Value[1].ptr, cx.npoly))
        else:
            dpl = gadgetCt.digits_per_limb
            arr = (C.c_int * len(dpl))(*dpl) if dpl is not None else None
            _check(L.rh_bext_gadget_product_single_p(self.be._h, levelQ, lp, cx.ptr, 1 if ct.IsNTT else 0, gadgetCt.BaseTwoDecomposition, arr,
                                                     gadgetCt.Q.ptr, pP, gadgetCt.digits, ct.Value[0].ptr, ct.Value[1].ptr, cx.npoly))

    def GadgetProductThenAdd(self, levelQ, cx, gadgetCt, add0, add1, ct):
        """ct[c] = add_c + GadgetProduct(cx)[c] (ring.Add, canonical) -- the Add the callers below issue right after the
        product, folded into ModDown's tile epilogue.  add0 / add1: DevicePoly or None; they may be ct.Value[c] themselves."""
        levelQ = min(levelQ, gadgetCt.LevelQ())
        self._rows(levelQ, cx, add0, add1, ct.Value[0], ct.Value[1])
        _check(lib().rh_bext_gadget_product_then_add(self.be._h, levelQ, gadgetCt.LevelP(), cx.ptr, gadgetCt.Q.ptr, gadgetCt.P.ptr,
                                                     gadgetCt.digits, add0.ptr if add0 is not None else None,
                                                     add1.ptr if add1 is not None else None, ct.Value[0].ptr, ct.Value[1].ptr, cx.npoly))

    def BaseRNSDecompositionVectorSize(self, levelQ, levelP):
        return (levelQ + levelP + 1) // (levelP + 1)                  # core/rlwe/params.go:635-642

    def DecomposeNTT(self, levelQ, levelP, c2, c2IsNTT, decompQP=None):
        """(:431-453) -> (decompQ, decompP): digit i of poly k is row i*npoly + k of each block.  `decompQP` is the
        caller's buffer pair, as in the reference (its BuffDecompQP argument); without it the blocks are allocated here."""
        beta = self.BaseRNSDecompositionVectorSize(levelQ, levelP)
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        self._rows(levelQ, c2)
        if decompQP is None:
            decompQP = (DevicePoly(rq, beta * c2.npoly, levelQ + 1), DevicePoly(rp, beta * c2.npoly, levelP + 1))
        dq, dp = decompQP
        if (dq.npoly, dq.limbs, dp.npoly, dp.limbs) != (beta * c2.npoly, levelQ + 1, beta * c2.npoly, levelP + 1):
            raise RingHipError("DecomposeNTT: decompQP must hold %d polys of %d and %d limbs" % (beta * c2.npoly, levelQ + 1, levelP + 1))
        _check(lib().rh_bext_decompose_ntt(self.be._h, levelQ, levelP, c2.ptr, 1 if c2IsNTT else 0, dq.ptr, dp.ptr, c2.npoly))
        return dq, dp

    def GadgetProductHoisted(self, levelQ, decompQP, gadgetCt, ct):
        """(:326-349) on the output of DecomposeNTT"""
        dq, dp = decompQP
        npoly = ct.Value[0].npoly
        self._rows(levelQ, dq, ct.Value[0], ct.Value[1])
        _check(lib().rh_bext_gadget_product_hoisted(self.be._h, levelQ, gadgetCt.LevelP(), dq.ptr, dp.ptr, gadgetCt.Q.ptr,
                                                    gadgetCt.P.ptr, gadgetCt.digits, ct.Value[0].ptr, ct.Value[1].ptr, npoly))

    def GadgetProductHoistedLazy(self, levelQ, decompQP, gadgetCt, ctQP):
        """(:351-371): the hoisted product WITHOUT the ModDown -- ctQP receives the accumulators modulo Q and modulo P (canonical, NTT
        domain, still scaled by P).  For sums of rotations that share one ModDown (AutomorphismHoistedLazy, linear transformations)."""
        dq, dp = decompQP
        q0, q1, p0, p1 = ctQP.Value[0].Q, ctQP.Value[1].Q, ctQP.Value[0].P, ctQP.Value[1].P
        levelP = gadgetCt.LevelP()
        if ctQP.LevelP() < levelP:
            raise RingHipError("ctQP.LevelP()=%d < gadgetCt.LevelP()=%d" % (ctQP.LevelP(), levelP))
        self._rows(levelQ, dq, q0, q1)
        self._rows(levelP, dp, p0, p1)          # the P accumulators are strided by levelP+1 rows per poly too
        _check(lib().rh_bext_gadget_product_hoisted_lazy(self.be._h, levelQ, levelP, dq.ptr, dp.ptr, gadgetCt.Q.ptr, gadgetCt.P.ptr,
                                                         gadgetCt.digits, q0.ptr, q1.ptr, p0.ptr, p1.ptr, q0.npoly))
        ctQP.IsNTT = True

    def GadgetProductLazy(self, levelQ, cx, gadgetCt, ctQP, cxIsNTT=True):
        """(:100-120) for gadget ciphertexts with more than one P modulus: the product without the ModDown.  The accumulators are the
        canonical residues the hoisted form leaves (gadgetProductMultiplePLazy and ...Hoisted differ in WHEN the digits are formed, not
        in what is summed), so this is DecomposeNTT into the evaluator's buffer + GadgetProductHoistedLazy."""
        levelP = gadgetCt.LevelP()
        dec = (self.buffer("lazydecQ", self.ringQ.AtLevel(levelQ), self.BaseRNSDecompositionVectorSize(levelQ, levelP) * cx.npoly, levelQ + 1),
               self.buffer("lazydecP", self.ringP.AtLevel(levelP), self.BaseRNSDecompositionVectorSize(levelQ, levelP) * cx.npoly, levelP + 1))
        self.DecomposeNTT(levelQ, levelP, cx, cxIsNTT, dec)
        self.GadgetProductHoistedLazy(levelQ, dec, gadgetCt, ctQP)

    def DecomposeSingleNTT(self, levelQ, levelP, nbPi, decompRNS, c2NTT, c2InvNTT, c2QiQ, c2QiP):
        """(:455-478): digit `decompRNS` of the decomposition -- DecomposeAndSplit of the coefficient-domain c2InvNTT, the digit's own limbs
        copied from the NTT-domain c2NTT, the others transformed (the reference's NTTLazy there; canonical here, same residues)"""
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        self.be.DecomposeAndSplit(levelQ, levelP, nbPi, decompRNS, c2InvNTT, c2QiQ, c2QiP)
        rq.NTT(c2QiQ, c2QiQ)
        rp.NTT(c2QiP, c2QiP)
        st = decompRNS * nbPi
        ed = min(st + nbPi, levelQ + 1)
        N = rq.N
        for k in range(c2NTT.npoly):                   # limbs [st, ed) of every poly from the NTT-domain input (:467-468)
            off = (k * (levelQ + 1) + st) * N * 8
            src = DevicePoly(rq.AtLevel(ed - st - 1), 1, ed - st, ptr=c2NTT.ptr + off, owner=c2NTT)
            dst = DevicePoly(rq.AtLevel(ed - st - 1), 1, ed - st, ptr=c2QiQ.ptr + off, owner=c2QiQ)
            rq.AtLevel(ed - st - 1).CopyLvl(src, dst)

    def ModDown(self, levelQ, levelP, ctQP, ct):
        """(:33-98), NTT -> NTT and coefficient -> coefficient: ct_c = ModDownQPtoQ(NTT)(ctQP_c.Q, ctQP_c.P)"""
        if ctQP.IsNTT != ct.IsNTT:
            raise RingHipError("ModDown: the mixed-domain forms are not built on the device path")
        if ctQP.IsNTT:
            self._rows(levelQ, ct.Value[0], ct.Value[1], ctQP.Value[0].Q, ctQP.Value[1].Q)
            self._rows(levelP, ctQP.Value[0].P, ctQP.Value[1].P)
            _check(lib().rh_bext_moddown_qp_to_q_ntt_pair(self.be._h, levelQ, levelP, ctQP.Value[0].Q.ptr, ctQP.Value[1].Q.ptr,
                                                          ctQP.Value[0].P.ptr, ctQP.Value[1].P.ptr, ct.Value[0].ptr, ct.Value[1].ptr,
                                                          ct.Value[0].npoly))
        else:
            for c in (0, 1):
                self.be.ModDownQPtoQ(levelQ, levelP, ctQP.Value[c].Q, ctQP.Value[c].P, ct.Value[c])

    def ALlocateDecompositionBuffer(self, levelQ, levelP, npoly):
        """(:480-494), spelled as in the reference: the (decompQ, decompP) pair DecomposeNTT fills"""
        beta = self.BaseRNSDecompositionVectorSize(levelQ, levelP)
        return (DevicePoly(self.ringQ.AtLevel(levelQ), beta * npoly, levelQ + 1), DevicePoly(self.ringP.AtLevel(levelP), beta * npoly, levelP + 1))

    # ---- core/rlwe/evaluator_evaluationkey.go ---------------------------------------------------------------
    def ApplyEvaluationKey(self, ctIn, evk, opOut):
        """(:37-123): opOut = (ctIn[0] + KS(ctIn[1])_0, KS(ctIn[1])_1) (applyEvaluationKey :105-112).  With operands of different ring degrees
        (:50-93) the evaluator is the larger ring's and evk a key between the degrees (KeyGenerator.GenEvaluationKeyNew): to a larger degree the
        input is first mapped to Y = X^(N/n) (SwitchCiphertextRingDegreeNTT), to a smaller one the key switch runs in the larger ring and its
        output is mapped down.  NTT-domain operands."""
        if ctIn.Degree() != 1 or opOut.Degree() != 1:
            raise RingHipError("cannot ApplyEvaluationKey: input and output Ciphertext must be of degree 1")
        if not ctIn.IsNTT:
            raise RingHipError("ApplyEvaluationKey: coefficient-domain ciphertexts are not supported by the device path")
        level = min(ctIn.Level(), opOut.Level())
        ringQ = self.ringQ.AtLevel(level)
        npoly = ctIn.Value[1].npoly
        NIn, NOut = ctIn.Value[0].ring.N, opOut.Value[0].ring.N
        if NIn == NOut:
            self.GadgetProductThenAdd(level, ctIn.Value[1], evk, ctIn.Value[0], None, opOut)   # (:108-111) with the Add in the epilogue
            opOut.IsNTT = True
            return
        if (NOut if NIn < NOut else NIn) != ringQ.N:
            raise RingHipError("cannot ApplyEvaluationKey: %s ring degree does not match evaluator params ring degree" % ("opOut" if NIn < NOut else "ctIn"))
        tmp = Ciphertext([ringQ.NewPoly(npoly), ringQ.NewPoly(npoly)], is_ntt=True)
        if NIn < NOut:
            SwitchCiphertextRingDegreeNTT(ctIn, self.ringQ, tmp)       # Y = X^(N/n) -> X (:65-69)
            self._switch_key(level, ringQ, tmp, evk, opOut)            # (:72)
        else:
            self._switch_key(level, ringQ, ctIn, evk, tmp)             # (:95)
            SwitchCiphertextRingDegreeNTT(tmp, self.ringQ, opOut)      # X -> Y = X^(N/n) (:98-102)
        self._copy_metadata(ctIn, opOut)                               # (:116)
        opOut.IsNTT = True

    def _switch_key(self, level, ringQ, ctIn, evk, opOut):
        """applyEvaluationKey (:105-112) with either branch of GadgetProduct, by the key's LevelP (as Automorphism below)"""
        if evk.LevelP() >= 1:
            self.GadgetProductThenAdd(level, ctIn.Value[1], evk, ctIn.Value[0], None, opOut)
        else:
            opOut.IsNTT = True
            self.GadgetProduct(level, ctIn.Value[1], evk, opOut)
            ringQ.Add(opOut.Value[0], ctIn.Value[0], opOut.Value[0])

    def Relinearize(self, ctIn, opOut, rlk=None):
        """(:125-153): degree 2 -> degree 1 with the relinearisation key (galois_keys["rlk"] or the argument)"""
        if ctIn.Degree() != 2:
            raise RingHipError("cannot relinearize: ctIn.Degree() should be 2 but is %d" % ctIn.Degree())
        rlk = rlk or self.galois_keys.get("rlk")
        if rlk is None:
            raise RingHipError("cannot relinearize: relinearization key is missing")
        if not ctIn.IsNTT:
            raise RingHipError("Relinearize: coefficient-domain ciphertexts are not supported by the device path")
        level = min(ctIn.Level(), opOut.Level())
        ringQ = self.ringQ.AtLevel(level)
        npoly = ctIn.Value[2].npoly
        self.GadgetProductThenAdd(level, ctIn.Value[2], rlk, ctIn.Value[0], ctIn.Value[1], opOut)   # (:144-146)
        opOut.IsNTT = True

    # ---- core/rlwe/evaluator_automorphism.go -----------------------------------------------------------------
    def _galois_key(self, galEl):
        if galEl not in self.galois_keys:                             # CheckAndGetGaloisKey
            raise RingHipError("cannot apply Automorphism: GaloisKey[%d] is missing" % galEl)
        return self.galois_keys[galEl]

    def _check_degree1_ntt(self, ctIn, opOut, who):
        if ctIn.Degree() != 1 or opOut.Degree() != 1:
            raise RingHipError("cannot apply %s: input and output Ciphertext must be of degree 1" % who)
        if not ctIn.IsNTT:
            raise RingHipError("%s: coefficient-domain ciphertexts are not supported by the device path" % who)

    def Automorphism(self, ctIn, galEl, opOut):
        """(:14-60): opOut = phi_galEl(ctIn[0] + KS(ctIn[1])_0, KS(ctIn[1])_1)"""
        self._check_degree1_ntt(ctIn, opOut, "Automorphism")
        level = min(ctIn.Level(), opOut.Level())
        ringQ = self.ringQ.AtLevel(level)
        if galEl == 1:
            if opOut is not ctIn:
                for a, b in zip(ctIn.Value, opOut.Value):
                    ringQ.vec_op("ADD_SCALAR_LAZY", a, None, b, s0=[0] * (level + 1))    # opOut.Copy(ctIn): x + 0, no reduction
            opOut.IsNTT = ctIn.IsNTT
            return
        evk = self._galois_key(galEl)
        npoly = ctIn.Value[1].npoly
        tmp = Ciphertext([self.buffer("auto0", ringQ, npoly, level + 1), self.buffer("auto1", ringQ, npoly, level + 1)], is_ntt=True)
        if evk.LevelP() >= 1:
            self.GadgetProductThenAdd(level, ctIn.Value[1], evk, ctIn.Value[0], None, tmp)     # product + ringQ.Add (:42-44)
        else:                                                         # single P, or no P with a power-of-two decomposition: the other branch of GadgetProduct
            self.GadgetProduct(level, ctIn.Value[1], evk, tmp)
            ringQ.Add(tmp.Value[0], ctIn.Value[0], tmp.Value[0])
        ringQ.AutomorphismNTT(tmp.Value[0], galEl, opOut.Value[0])   # AutomorphismNTTWithIndex (ring/automorphism.go:52-73)
        ringQ.AutomorphismNTT(tmp.Value[1], galEl, opOut.Value[1])
        opOut.IsNTT = ctIn.IsNTT

    def AutomorphismHoisted(self, level, ctIn, c1DecompQP, galEl, opOut):
        """(:62-105): as Automorphism with the decomposition of ctIn[1] shared between rotations"""
        self._check_degree1_ntt(ctIn, opOut, "AutomorphismHoisted")
        ringQ = self.ringQ.AtLevel(level)
        if galEl == 1:
            return self.Automorphism(ctIn, 1, opOut)
        evk = self._galois_key(galEl)
        npoly = ctIn.Value[1].npoly
        tmp = Ciphertext([self.buffer("auto0", ringQ, npoly, level + 1), self.buffer("auto1", ringQ, npoly, level + 1)], is_ntt=True)
        dq, dp = c1DecompQP
        self._rows(level, dq, ctIn.Value[0], opOut.Value[0], opOut.Value[1])
        _check(lib().rh_bext_gadget_product_hoisted_then_add(self.be._h, level, evk.LevelP(), dq.ptr, dp.ptr, evk.Q.ptr, evk.P.ptr, evk.digits,
                                                             ctIn.Value[0].ptr, None, tmp.Value[0].ptr, tmp.Value[1].ptr, npoly))   # product + Add (:88-89)
        ringQ.AutomorphismNTT(tmp.Value[0], galEl, opOut.Value[0])
        ringQ.AutomorphismNTT(tmp.Value[1], galEl, opOut.Value[1])
        opOut.IsNTT = ctIn.IsNTT

    def AutomorphismHoistedLazy(self, levelQ, ctIn, c1DecompQP, galEl, ctQP):
        """(:103-160), NTT-domain ctQP: the rotated ciphertext modulo QP and scaled by P --
        ctQP[1] = phi(KS_1), ctQP[0] = phi(KS_0 + P * ctIn[0]) on the Q part, phi(KS_0) on the P part (P * ctIn[0] vanishes modulo P)"""
        evk = self._galois_key(galEl)
        levelP = evk.LevelP()
        if ctQP.LevelP() < levelP:
            raise RingHipError("ctQP.LevelP()=%d < GaloisKey[%d].LevelP()=%d" % (ctQP.LevelP(), galEl, levelP))
        if not ctIn.IsNTT:
            raise RingHipError("AutomorphismHoistedLazy: coefficient-domain ciphertexts are not supported by the device path")
        ringQ, ringP = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        npoly = ctIn.Value[0].npoly
        tmp = ElementQP([PolyQP(self.buffer("lazyQ0", ringQ, npoly, levelQ + 1), self.buffer("lazyP0", ringP, npoly, levelP + 1)),
                         PolyQP(self.buffer("lazyQ1", ringQ, npoly, levelQ + 1), self.buffer("lazyP1", ringP, npoly, levelP + 1))])
        self.GadgetProductHoistedLazy(levelQ, c1DecompQP, evk, tmp)
        # "Result NTT domain is returned according to the NTT flag of ctQP" (:105): the flag only selects which index map is applied
        # (:134-157) -- ringQP.AutomorphismNTTWithIndex or the coefficient-domain ringQP.Automorphism -- and is left as the caller set it
        autQ, autP = (ringQ.AutomorphismNTT, ringP.AutomorphismNTT) if ctQP.IsNTT else (ringQ.Automorphism, ringP.Automorphism)
        autQ(tmp.Value[1].Q, galEl, ctQP.Value[1].Q)                                      # ringQP.Automorphism(NTTWithIndex) (:136 / :147)
        autP(tmp.Value[1].P, galEl, ctQP.Value[1].P)
        P = 1
        for p in self.ringP.moduli[:levelP + 1]:
            P *= int(p)
        ringQ.MulScalarBigintThenAdd(ctIn.Value[0], P, tmp.Value[0].Q)                    # + ctIn[0] * P (:138-142 as one pass: same canonical values)
        autQ(tmp.Value[0].Q, galEl, ctQP.Value[0].Q)                                      # (:144 / :155)
        autP(tmp.Value[0].P, galEl, ctQP.Value[0].P)

    # ---- core/rlwe/inner_sum.go ------------------------------------------------------------------------------------------------------
    # Which of the two fused kernels (csrc/inner_sum_kernels.hip.hpp) a call uses when it is not told (fused=None): the measured choice -- a kernel is
    # the default where the run shows it no slower than its composed form, alone and in the whole call (profiles/inner_sum.json).
    # fused=True / False selects both / neither; the bits are the same.
    FUSED_INNER_SUM = {"accumulate": True, "rotate_add": True}

    def _fused_inner_sum(self, fused):
        return dict(self.FUSED_INNER_SUM) if fused is None else {k: bool(fused) for k in self.FUSED_INNER_SUM}

    def RotateAccumulateQP(self, levelQ, galEl, ct0, tmpQP, accQP, first):
        """accQP (=|+=) phi_galEl(tmpQP + (P ct0, 0)) modulo QP in one launch: the tail of AutomorphismHoistedLazy (evaluator_automorphism.go:107-160)
        and ringQP.Add (inner_sum.go:245-246).  tmpQP: the output of GadgetProductHoistedLazy; first: accQP is written, not added to."""
        levelP = tmpQP.LevelP()
        q, p = [v.Q for v in tmpQP.Value + accQP.Value], [v.P for v in tmpQP.Value + accQP.Value]
        self._rows(levelQ, ct0, *q)
        self._rows(levelP, *p)
        _check(lib().rh_rlwe_rotate_accumulate_qp(self.be._h, levelQ, levelP, int(galEl), ct0.ptr, q[0].ptr, q[1].ptr, p[0].ptr, p[1].ptr,
                                                  q[2].ptr, q[3].ptr, p[2].ptr, p[3].ptr, ct0.npoly, 1 if first else 0))

    def RotateAddQ(self, level, galEl, tmp, ct):
        """ct += phi_galEl(tmp) modulo Q, both components in one launch, in place on ct: the AutomorphismNTT pair that ends AutomorphismHoisted
        (evaluator_automorphism.go:90-95) and the ringQ.Add pair that follows it (inner_sum.go:279-280)"""
        self._rows(level, *tmp.Value, *ct.Value)
        _check(lib().rh_rlwe_rotate_add_q(self.ringQ._h, level, int(galEl), tmp.Value[0].ptr, tmp.Value[1].ptr, ct.Value[0].ptr, ct.Value[1].ptr,
                                          ct.Value[0].npoly))

    def _sum_operands(self, ctIn, opOut, who):
        if ctIn.Degree() != 1 or opOut.Degree() != 1:
            raise RingHipError("cannot %s: ctIn.Degree() != 1 or opOut.Degree() != 1" % who)
        if self.ringQ.kind != Standard:
            raise RingHipError("cannot %s: 3N and conjugate-invariant rings are not supported by the device path" % who)
        if self.ringP is None:
            raise RingHipError("cannot %s: the evaluator was built without ringP, which the key switch needs" % who)
        level = ctIn.Level()
        self._rows(level, *ctIn.Value, *opOut.Value)
        if opOut.Value[0].npoly != ctIn.Value[0].npoly:
            raise RingHipError("cannot %s: ctIn and opOut hold different numbers of ciphertexts" % who)
        return level

    def _sum_keys(self, galEls, who):
        """every key a sum of rotations needs, looked up before the first launch (CheckAndGetGaloisKey for each element)"""
        keys = {}
        for g in galEls:
            if g not in self.galois_keys:
                raise RingHipError("cannot apply %s: GaloisKey[%d] is missing" % (who, g))
            evk = keys[g] = self.galois_keys[g]
            if evk.BaseTwoDecomposition != 0:
                raise RingHipError("cannot apply %s: method is unsupported for BaseTwoDecomposition != 0" % who)   # gadgetProductMultiplePLazyHoisted's own text
            if evk.LevelP() < 1:
                raise RingHipError("cannot apply %s: GaloisKey[%d] has one P modulus, which the hoisted product of the device path does not take (levelP >= 1)" % (who, g))
        return keys

    @staticmethod
    def _copy_metadata(ctIn, opOut):
        for name in METADATA:                                            # *opOut.MetaData = *ctIn.MetaData
            if hasattr(ctIn, name):
                setattr(opOut, name, getattr(ctIn, name))
        opOut.IsNTT = ctIn.IsNTT

    def _sum_buffers(self, levelQ, levelP, npoly):
        """ctInNTT (BuffCt), accQP (BuffQP[2:4]), cQP (BuffQP[4:6]) and BuffDecompQP, evaluator-owned"""
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        beta = self.BaseRNSDecompositionVectorSize(levelQ, levelP)
        qp = lambda t: ElementQP([PolyQP(self.buffer(t + "Q%d" % c, rq, npoly, levelQ + 1), self.buffer(t + "P%d" % c, rp, npoly, levelP + 1)) for c in (0, 1)])
        ct = Ciphertext([self.buffer("BuffCt%d" % c, rq, npoly, levelQ + 1) for c in (0, 1)], is_ntt=True)
        dec = (self.buffer("BuffDecompQ", rq, beta * npoly, levelQ + 1), self.buffer("BuffDecompP", rp, beta * npoly, levelP + 1))
        return ct, qp("sumAcc"), qp("sumC"), dec

    def PartialTracesSum(self, ctIn, offset, n, opOut, fused=None):
        """(:152-291): opOut = sum_{i < n} phi_{5^(i offset)}(ctIn) with log2(n) hoisted and HW(n) - 1 lazy rotations under one ModDown, by the
        reference's binary reading of n.  opOut may be ctIn.  A coefficient-domain ctIn is transformed on entry and the result transformed back
        (:180-182, :285-288 -- for n = 1 too, where the reference copies and then applies INTT to the copy: kept).  The keys are used at
        ctIn.Level(); every one is looked up before the first launch.  fused: the kernels of csrc/inner_sum.hip (True), the composition of
        DecomposeNTT / AutomorphismHoisted(Lazy) / Add / ModDown (False), FUSED_INNER_SUM per kernel (None) -- the same bits."""
        n, offset = int(n), int(offset)
        if n <= 0 or offset == 0:
            raise RingHipError("partialtrace: invalid parameter (n = 0 or batchSize = 0)")
        levelQ = self._sum_operands(ctIn, opOut, "PartialTracesSum")
        levelP = self.ringP.L - 1
        use = self._fused_inner_sum(fused)
        plan = partial_traces_plan(self.ringQ.N, offset, n) if n > 1 else []
        keys = self._sum_keys([g for kind, g, _ in plan if kind == LAZY or (kind == DOUBLE and g != 1)], "PartialTracesSum")
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        npoly = ctIn.Value[0].npoly
        ct, acc, cqp, dec = self._sum_buffers(levelQ, levelP, npoly)
        cq = Ciphertext([cqp.Value[0].Q, cqp.Value[1].Q], is_ntt=True)
        in_ntt = ctIn.IsNTT
        for c in (0, 1):                                                 # ctInNTT (:180-186)
            (rq.CopyLvl if in_ntt else rq.NTT)(ctIn.Value[c], ct.Value[c])
        if n == 1 and opOut is not ctIn:                                 # (:188-192)
            for c in (0, 1):
                rq.CopyLvl(ctIn.Value[c], opOut.Value[c])
        add_q = lambda a, b: [rq.vec_op("ADD", a.Value[c], b.Value[c], a.Value[c]) for c in (0, 1)]
        first = True
        for kind, g, decompose in plan:
            if decompose:
                self.DecomposeNTT(levelQ, levelP, ct.Value[1], True, dec)                        # (:222)
            if kind == LAZY and use["accumulate"]:                                               # (:236-247), the tail in one launch
                self.GadgetProductHoistedLazy(levelQ, dec, keys[g], cqp)
                self.RotateAccumulateQP(levelQ, g, ct.Value[0], cqp, acc, first)
                first = False
            elif kind == LAZY:
                self.AutomorphismHoistedLazy(levelQ, ct, dec, g, acc if first else cqp)
                if not first:
                    for c in (0, 1):
                        rq.vec_op("ADD", acc.Value[c].Q, cqp.Value[c].Q, acc.Value[c].Q)        # ringQP.Add (:245-246)
                        rp.vec_op("ADD", acc.Value[c].P, cqp.Value[c].P, acc.Value[c].P)
                first = False
            elif kind == CLOSE and n & (n - 1):                                                  # opOut = accQP / P + ctInNTT (:258-262)
                view = Ciphertext(opOut.Value, is_ntt=True)                                      # opOut's flag is the caller's until the call has succeeded
                self.ModDown(levelQ, levelP, acc, view)
                add_q(opOut, ct)
            elif kind == CLOSE:                                                                  # (:265-266)
                for c in (0, 1):
                    rq.CopyLvl(ct.Value[c], opOut.Value[c])
            elif g == 1:                                                                         # AutomorphismHoisted of the identity copies (:68-73)
                add_q(ct, ct)
            elif use["rotate_add"]:                                                              # (:276-280), the tail in one launch
                evk = keys[g]
                _check(lib().rh_bext_gadget_product_hoisted_then_add(self.be._h, levelQ, evk.LevelP(), dec[0].ptr, dec[1].ptr, evk.Q.ptr, evk.P.ptr, evk.digits,
                                                                     ct.Value[0].ptr, None, cq.Value[0].ptr, cq.Value[1].ptr, npoly))
                self.RotateAddQ(levelQ, g, cq, ct)
            else:
                self.AutomorphismHoisted(levelQ, ct, dec, g, cq)
                add_q(ct, cq)
        if not in_ntt:                                                   # (:285-288)
            for c in (0, 1):
                rq.INTT(opOut.Value[c], opOut.Value[c])
        self._copy_metadata(ctIn, opOut)

    def PartialTracesSumC(self, ctIn, offset, n, opOut, fused=None):
        """PartialTracesSum as ONE call into the library (rh_rlwe_partial_traces_sum): what a compiled host uses.  fused: both kernels or neither."""
        n, offset = int(n), int(offset)
        if n <= 0 or offset == 0:
            raise RingHipError("partialtrace: invalid parameter (n = 0 or batchSize = 0)")
        levelQ = self._sum_operands(ctIn, opOut, "PartialTracesSum")
        plan = partial_traces_plan(self.ringQ.N, offset, n) if n > 1 else []
        keys = self._sum_keys([g for kind, g, _ in plan if kind == LAZY or (kind == DOUBLE and g != 1)], "PartialTracesSum")
        table = (GaloisKeyEntry * max(len(keys), 1))()
        for i, (g, evk) in enumerate(keys.items()):
            table[i] = GaloisKeyEntry(g, evk.Q.ptr, evk.P.ptr, evk.digits)
        use = self._fused_inner_sum(fused)
        _check(lib().rh_rlwe_partial_traces_sum(self.be._h, levelQ, self.ringP.L - 1, ctIn.Value[0].ptr, ctIn.Value[1].ptr, 1 if ctIn.IsNTT else 0, offset, n,
                                                table, len(keys), opOut.Value[0].ptr, opOut.Value[1].ptr, ctIn.Value[0].npoly,
                                                1 if all(use.values()) else 0))
        self._copy_metadata(ctIn, opOut)

    def Replicate(self, ctIn, batchSize, n, opOut, fused=None):
        """(:477-479): the inverse of an inner sum, PartialTracesSum by -batchSize"""
        self.PartialTracesSum(ctIn, -int(batchSize), n, opOut, fused=fused)

    def Trace(self, ctIn, logN, opOut, fused=None):
        """(:36-121): X -> sum of the automorphisms 5^(2^i), logN <= i < log2(N) - 1 (and 2N - 1 when logN = 0), pre-multiplied by (N / 2^logN)^-1:
        monomials X^k with N / 2^logN not dividing k vanish, the others are kept.  opOut may be ctIn."""
        level = self._sum_operands(ctIn, opOut, "Trace")
        N, top = self.ringQ.N, self.ringQ.N.bit_length() - 1
        gap = 1 << (top - logN - 1)
        if logN == 0:
            gap <<= 1
        rq = self.ringQ.AtLevel(level)
        if gap <= 1:
            if opOut is not ctIn:
                for c in (0, 1):
                    rq.CopyLvl(ctIn.Value[c], opOut.Value[c])
            self._copy_metadata(ctIn, opOut)
            return
        galEls = GaloisElementsForTrace(N, logN)
        keys = self._sum_keys(galEls, "Trace")
        use = self._fused_inner_sum(fused)
        in_ntt = ctIn.IsNTT
        Q = 1
        for q in self.ringQ.moduli[:level + 1]:
            Q *= int(q)
        NInv = pow(gap, -1, Q)
        npoly = ctIn.Value[0].npoly
        buff = Ciphertext([self.buffer("traceQ%d" % c, rq, npoly, level + 1) for c in (0, 1)], is_ntt=True)
        for c in (0, 1):
            rq.MulScalarBigint(ctIn.Value[c], NInv, opOut.Value[c])      # pre-multiplication by (N/n)^-1 (:69-70)
            if not in_ntt:
                rq.NTT(opOut.Value[c], opOut.Value[c])
        view = Ciphertext(opOut.Value, is_ntt=True)                      # opOut's flag is the caller's until the call has succeeded
        for g in galEls:                                                 # (:88-106)
            if use["rotate_add"]:                                        # Automorphism's product + Add (:42-44), then its index maps and the Adds in one launch
                self.GadgetProductThenAdd(level, opOut.Value[1], keys[g], opOut.Value[0], None, buff)
                self.RotateAddQ(level, g, buff, opOut)
            else:
                self.Automorphism(view, g, buff)
                for c in (0, 1):
                    rq.vec_op("ADD", opOut.Value[c], buff.Value[c], opOut.Value[c])
        if not in_ntt:
            for c in (0, 1):
                rq.INTT(opOut.Value[c], opOut.Value[c])
        self._copy_metadata(ctIn, opOut)

    def InnerFunction(self, ctIn, batchSize, n, f, opOut):
        """(:316-440): the tree of PartialTracesSum with a caller's f(a, b, c) -- a Python callable on device ciphertexts, c = f(a, b) -- in place
        of the additions, and plain (not hoisted) automorphisms.  f = Add gives the inner sum."""
        n, batchSize = int(n), int(batchSize)
        levelQ = self._sum_operands(ctIn, opOut, "InnerFunction")
        rq = self.ringQ.AtLevel(levelQ)
        npoly = ctIn.Value[0].npoly
        plan = partial_traces_plan(self.ringQ.N, batchSize, n) if n > 1 else []
        self._sum_keys([g for kind, g, _ in plan if kind != CLOSE and g != 1], "InnerFunction")
        new = lambda: Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=True)
        ct, accQ, cQ = new(), new(), new()
        for x in (ct, accQ, cQ):
            self._copy_metadata(ctIn, x)
            x.IsNTT = True
        in_ntt = ctIn.IsNTT
        copy = lambda a, b: [rq.CopyLvl(a.Value[c], b.Value[c]) for c in (0, 1)]
        for c in (0, 1):
            (rq.CopyLvl if in_ntt else rq.NTT)(ctIn.Value[c], ct.Value[c])
        if n == 1 and opOut is not ctIn:
            copy(ctIn, opOut)
        self._copy_metadata(ctIn, opOut)
        opOut.IsNTT = True                                               # f sees NTT-domain operands; the caller's flag comes back whatever happens
        try:
            first = True
            for kind, g, _ in plan:
                if kind == LAZY:
                    self.Automorphism(ct, g, accQ if first else cQ)
                    if not first:
                        f(accQ, cQ, accQ)
                    first = False
                elif kind == CLOSE and n & (n - 1):
                    copy(accQ, opOut)
                    f(opOut, ct, opOut)
                elif kind == CLOSE:
                    copy(ct, opOut)
                else:
                    self.Automorphism(ct, g, cQ)
                    f(ct, cQ, ct)
            if not in_ntt:
                for c in (0, 1):
                    rq.INTT(opOut.Value[c], opOut.Value[c])
        finally:
            opOut.IsNTT = in_ntt


# ---- core/rlwe/ring_packing.go, ring_packing_keys.go ----------------------------------------------------------------------------------------
def GaloisElementsForExpand(N, logN):
    """(ring_packing_keys.go:143-153): NthRoot / 2^(i+1) + 1 = N / 2^i + 1 for 0 <= i < logN"""
    return [2 * int(N) // (2 << i) + 1 for i in range(logN)]


def GaloisElementsForPack(N, logGap):
    """(ring_packing_keys.go:156-180), standard rings: 5^(2^i) for 0 <= i < logGap, and 2N - 1 when logGap = logN"""
    logN = int(N).bit_length() - 1
    if logGap > logN or logGap < 0:
        raise RingHipError("cannot GaloisElementsForPack: logGap > logN || logGap < 0")
    out = [GaloisElement(N, 1 << i) for i in range(logGap)]
    if logGap == logN:
        out.append(2 * int(N) - 1)
    return out


def _view(p, first, count, ring=None):
    """polys [first, first + count) of a batch as a batch of their own"""
    ring = p.ring if ring is None else ring
    return DevicePoly(ring, count, p.limbs, ptr=p.ptr + first * p.limbs * p.ring.N * 8, owner=p)


def GenXPow2NTT(ring, logN, div):
    """(ring_packing.go:795-833): [X^(+-2^i) for 0 <= i < logN] in the NTT domain and in Montgomery form, at the level of `ring`, built on the device with
    the ring's own calls: MForm(1) at coefficient 1 (N - 1 for div) transformed, then squared logN - 1 times; for div the first entry is negated
    (X^(N-1) = -X^-1).  Returns views of ONE block of logN polys (what rh_rlwe_expand takes as its table)."""
    L, N = ring.level + 1, ring.N
    first = np.zeros((1, L, N), dtype=np.uint64)
    first[0, :, N - 1 if div else 1] = [(1 << 64) % int(q) for q in ring.moduli[:L]]
    block = DevicePoly(ring, max(logN, 1), L)
    x = [_view(block, i, 1) for i in range(logN)]
    if logN:
        _check(lib().rh_dev_upload(ring._h, block.ptr, first.ctypes.data_as(U64P), first.size))
        ring.NTT(x[0], x[0])
        for i in range(1, logN):
            ring.MulCoeffsMontgomery(x[i - 1], x[i - 1], x[i])
        if div:
            ring.Neg(x[0], x[0])
    return x


def _log_n(ct):
    return ct.Value[0].ring.N.bit_length() - 1


def _small_ntt(ring, p):
    # The reference transforms the rows of the small ring with ring.NTTStandard and the LARGE ring's table of roots (core/rlwe/element.go:273):
    # entry i < N/2 of that table is psi_N^bitrev(i, logN) = (psi_N^2)^bitrev(i, logN - 1).  Both rings derive psi from the same smallest
    # primitive root g of q, psi_N = g^((q-1)/2N), so psi_(N/2) = g^((q-1)/N) = psi_N^2: the small ring's own transform is that very transform.
    ring.NTT(p, p)


def SwitchCiphertextRingDegreeNTT(ctIn, ringQLargeDim, opOut):
    """(core/rlwe/element.go:250-287): Y^(N/n) -> X^N or back, NTT domain in and out; ringQLargeDim: the ring of the larger degree (its level is not
    read: the ciphertexts' is).  Down: an inverse transform at the large degree, every gap-th coefficient, the small ring's transform.  Up: every
    NTT coefficient gap times (ring.MapSmallDimensionToLargerDimensionNTT, ring/operations.go:380-392).  ctIn is left alone."""
    NIn, NOut = ctIn.Value[0].ring.N, opOut.Value[0].ring.N
    level = min(ctIn.Level(), opOut.Level())
    npoly = ctIn.Value[0].npoly
    if ringQLargeDim.N != max(NIn, NOut) or NIn == NOut:
        raise RingHipError("SwitchCiphertextRingDegreeNTT: ringQLargeDim must be the ring of the larger of two different degrees")
    big = ringQLargeDim.AtLevel(level)
    lg = abs(NIn.bit_length() - NOut.bit_length())
    Evaluator._rows(level, *ctIn.Value, *opOut.Value)
    if NIn > NOut:
        buff = [DevicePoly(big, npoly, level + 1) for _ in (0, 1)]
        for c in (0, 1):
            big.INTT(ctIn.Value[c], buff[c])
        _check(lib().rh_rlwe_ring_split(big._h, level, buff[0].ptr, buff[1].ptr, opOut.Value[0].ptr, opOut.Value[1].ptr, None, None, lg, npoly))
        for c in (0, 1):
            _small_ntt(opOut.Value[c].ring.AtLevel(level), opOut.Value[c])
    else:
        _check(lib().rh_rlwe_ring_merge(big._h, level, ctIn.Value[0].ptr, ctIn.Value[1].ptr, None, None, None, opOut.Value[0].ptr, opOut.Value[1].ptr, lg, npoly))
    Evaluator._copy_metadata(ctIn, opOut)


def SwitchCiphertextRingDegree(ctIn, opOut):
    """(core/rlwe/element.go:293-312), to the SMALLER degree: opOut[w] = ctIn[w gap], whatever the domain flag says (the reference does not read it).
    The other direction writes every gap-th word of opOut and leaves the rest: not built on the device path."""
    NIn, NOut = ctIn.Value[0].ring.N, opOut.Value[0].ring.N
    if NIn <= NOut:
        raise RingHipError("SwitchCiphertextRingDegree: only the map to a smaller ring degree is built on the device path")
    level = min(ctIn.Level(), opOut.Level())
    Evaluator._rows(level, *ctIn.Value, *opOut.Value)
    big = ctIn.Value[0].ring
    _check(lib().rh_rlwe_ring_split(big._h, level, ctIn.Value[0].ptr, ctIn.Value[1].ptr, opOut.Value[0].ptr, opOut.Value[1].ptr, None, None,
                                    NIn.bit_length() - NOut.bit_length(), ctIn.Value[0].npoly))
    Evaluator._copy_metadata(ctIn, opOut)


def getMinimumGap(keys):
    """(ring_packing.go:835-868) -> (gap, logGap): the odd part and the 2-adic valuation of the smallest difference of a sorted list"""
    gap, logGap = 0x7fffffffffffffff, 0
    for a, b in zip(keys, keys[1:]):
        if a > b:
            raise RingHipError("getMinimumGap: invalid index list: element must be sorted from smallest to largest")
        if a == b:
            raise RingHipError("getMinimumGap: invalid index list: contains duplicated elements")
        gap = min(gap, b - a)
        if gap == 1:
            break
    while gap & 1 == 0:
        logGap += 1
        gap >>= 1
    return gap, logGap


MODE_A, MODE_B, MODE_AB = 0, 1, 2


def pack_plan(N, keys, inputLogGap, zeroGarbageSlots):
    """The loops of Pack (ring_packing.go:660-790) on the sorted index list alone -> (logStart, logEnd, levels, slot): `levels` holds, per level that
    has work, (Galois element, position of X^(N/2^(i+1)) in XPow2NTT, [(mode, slot_a, slot_b)]), a slot being the position of a ciphertext in
    `keys`; `slot` is where cts[0] ends (None: the reference returns a nil ciphertext).  MODE_AB: both halves of a pair are there, MODE_B: only the
    upper one (it takes the lower one's place in the map, not in memory), MODE_A: only the lower one."""
    N = int(N)
    logN = N.bit_length() - 1
    if len(keys) > 1:
        gap, logGap = getMinimumGap(keys)
    else:
        gap, logGap = N, logN
    logStart, logEnd = logN - inputLogGap, logN
    if not zeroGarbageSlots and gap > 0:
        logEnd -= logGap
    if logStart >= logEnd:
        raise RingHipError("gaps between ciphertexts is smaller than inputLogGap > N")
    pos = {k: s for s, k in enumerate(keys)}
    levels = []
    for i in range(logStart, logEnd):
        t = 1 << (logN - 1 - i)
        entries = []
        for jx in sorted({k % t for k in pos if 0 <= k < 2 * t}):
            a, b = pos.get(jx), pos.get(jx + t)
            if b is not None:
                entries.append((MODE_AB, a, b) if a is not None else (MODE_B, b, b))
                if a is None:
                    pos[jx] = b
                del pos[jx + t]
            else:
                entries.append((MODE_A, a, a))
        if entries:
            galEl = 2 * N - 1 if i == 0 else GaloisElement(N, 1 << (i - 1))
            levels.append((galEl, logN - i - 1, entries))
    return logStart, logEnd, levels, pos.get(0)


class RingPackingEvaluator:
    """rlwe.RingPackingEvaluator (core/rlwe/ring_packing.go) on device batches.  parameters: {logN: (ringQ, ringP)}, rings over the same moduli;
    RingSwitchingKeys[logNIn][logNOut], RepackKeys[logN][galEl], ExtractKeys[logN][galEl]: GadgetCiphertexts (RingPackingEvaluationKey,
    ring_packing_keys.go:14-32), every key setting GadgetProduct takes.  Standard rings, NTT-friendly chains.

    Where the reference walks maps of single ciphertexts and issues one key switch per ciphertext, a level of Expand or Pack is here ONE launch
    sequence over all the ciphertexts of the level: they share the Galois element."""

    # Which fused kernels (csrc/ring_packing_kernels.hip.hpp) a call uses when it is not told (fused=None): the measured choice, a kernel being the
    # default where the run shows it no slower than its composed form, alone and in the whole call (profiles/ring_packing.json).
    # fused=True / False selects all / none; the bits are the same.
    FUSED_RING_PACKING = {"expand_step": True, "rotate_add": True, "pack_combine": True, "pack_finish": True}

    def __init__(self, parameters, RingSwitchingKeys=None, RepackKeys=None, ExtractKeys=None):
        self.parameters = dict(parameters)
        if not self.parameters:
            raise RingHipError("RingPackingEvaluator: no parameters")
        self.RingSwitchingKeys, self.RepackKeys, self.ExtractKeys = RingSwitchingKeys, RepackKeys, ExtractKeys
        levelQ = self.parameters[self.MinLogN()][0].L - 1                # (:35)
        self.Evaluators, self.XPow2NTT, self.XInvPow2NTT = {}, {}, {}
        for logN, (ringQ, ringP) in self.parameters.items():
            if ringQ.N != 1 << logN:
                raise RingHipError("RingPackingEvaluator: parameters[%d] has a ring of degree %d" % (logN, ringQ.N))
            self.Evaluators[logN] = Evaluator(ringQ, ringP)
            if ringQ.kind == Standard:
                self.XPow2NTT[logN] = GenXPow2NTT(ringQ.AtLevel(levelQ), logN, False)
                self.XInvPow2NTT[logN] = GenXPow2NTT(ringQ.AtLevel(levelQ), logN, True)
        self._xrep = {}

    def close(self):
        for ev in self.Evaluators.values():
            ev.close()

    def MinLogN(self):
        return min(self.parameters)

    def MaxLogN(self):
        return max(self.parameters)

    def _use(self, fused):
        return dict(self.FUSED_RING_PACKING) if fused is None else {k: bool(fused) for k in self.FUSED_RING_PACKING}

    @staticmethod
    def _key_switch(ev, level, c0, c1, evk, out0, out1):
        """(c0 + KS(c1)_0, KS(c1)_1) (applyEvaluationKey, evaluator_evaluationkey.go:105-112) into out0 / out1, other buffers than c0 / c1"""
        out = Ciphertext([out0, out1], is_ntt=True)
        if evk.LevelP() >= 1:
            ev.GadgetProductThenAdd(level, c1, evk, c0, None, out)
        else:
            ev.GadgetProduct(level, c1, evk, out)
            ev.ringQ.AtLevel(level).vec_op("ADD", out0, c0, out0)

    def _galois_keys(self, keyset, galEls):
        """CheckAndGetGaloisKey for every element, before the first launch"""
        for g in galEls:
            if g not in keyset:
                raise RingHipError("cannot apply Automorphism: GaloisKey[%d] is missing" % g)
        return {g: keyset[g] for g in galEls}

    def _replicated(self, x, cnt, rq, level):
        """the composed forms multiply a batch by a table poly: the table `cnt` times, built once per (table, level, cnt)"""
        key = (x.ptr, level, cnt)
        rep = self._xrep.get(key)
        if rep is None:
            rep = self._xrep[key] = DevicePoly(rq, cnt, level + 1)
            for p in range(cnt):
                rq.CopyLvl(x, _view(rep, p, 1))
        return rep

    # ---- Expand (:475-594) ----------------------------------------------------------------------------------------------------------------
    def _expand_checks(self, ct, logGap):
        if ct.Degree() != 1:
            raise RingHipError("ct.Degree() != 1")                                                      # (:477-479)
        logN = _log_n(ct)
        if logN not in self.parameters:
            raise RingHipError("eval.Parameters[%d] is nil" % logN)                                     # (:485-486)
        if self.ExtractKeys is None:
            raise RingHipError("eval.ExtractKeys is nil")                                               # (:491-493)
        if logN not in self.ExtractKeys:
            raise RingHipError("eval.ExtractKeys[%d] is nil" % logN)                                    # (:496-497)
        ev = self.Evaluators[logN]
        if ev.ringQ.kind != Standard:                                                                   # (:509-511)
            raise RingHipError("method is only supported for ring.Type = ring.Standard (X^{-2^{i}} does not exist in the sub-ring Z[X + X^{-1}])")
        if not 0 <= logGap <= logN:
            raise RingHipError("Expand: need 0 <= logGap <= logN")
        N = 1 << logN
        keys = self._galois_keys(self.ExtractKeys[logN], [N // (1 << i) + 1 for i in range(logN)])
        return logN, ev, keys

    def _expand_head(self, ct, logN, logGap, ev, scale=True):
        """the output batch with the NTT-domain inputs, scaled by 2^-logN, in its first B polys (:513-528)"""
        level, B = ct.Level(), ct.Value[0].npoly
        ev._rows(level, *ct.Value)
        rq = ev.ringQ.AtLevel(level)
        out = Ciphertext([DevicePoly(rq, B << (logN - logGap), level + 1) for _ in (0, 1)], is_ntt=True)
        Q = 1
        for q in ev.ringQ.moduli[:level + 1]:
            Q *= int(q)
        NInv = pow(1 << logN, -1, Q)
        for c in (0, 1):
            head = _view(out.Value[c], 0, B)
            (rq.CopyLvl if ct.IsNTT else rq.NTT)(ct.Value[c], head)
            if scale:
                rq.MulScalarBigint(head, NInv, head)
        return out, rq, level, B

    def _expand_done(self, ct, out, logN, logGap):
        Evaluator._copy_metadata(ct, out)
        out.IsNTT = True                       # (:517-521): the flag is set on entry, so the closing INTT loop (:586-592) never fires
        out.LogDimensions = 0                  # (:515): Rows = Cols = 0; every output descends from cts[0]
        return out, [m << logGap for m in range(1 << (logN - logGap))]

    def Expand(self, ct, logGap, fused=None):
        """(:475-594) on a batch of B ciphertexts -> (one batch of B N / 2^logGap ciphertexts, the index list): the ciphertext of coefficient
        m 2^logGap of input b is poly m B + b, so the live set of every level is a contiguous prefix, which doubles with every level that has a
        second output.  The outputs are in the NTT domain with IsNTT set, whatever the input's domain (:517-521, :586-592).  ct is left alone."""
        logN, ev, keys = self._expand_checks(ct, logGap)
        use = self._use(fused)
        out, rq, level, B = self._expand_head(ct, logN, logGap, ev)
        N, gap = 1 << logN, 1 << logGap
        half = max(B, (B << (logN - logGap)) // 2)
        tmp = [ev.buffer("rpTmp%d" % c, rq, half, level + 1) for c in (0, 1)]
        xinv = self.XInvPow2NTT[logN]
        for i in range(logN):
            n = 1 << i
            galEl = N // n + 1
            cnt = (n // gap) * B if n >= gap else B
            c = [_view(out.Value[k], 0, cnt) for k in (0, 1)]
            t = [_view(tmp[k], 0, cnt) for k in (0, 1)]
            self._key_switch(ev, level, c[0], c[1], keys[galEl], t[0], t[1])                               # Automorphism's product + Add (:555)
            if n >= gap and use["expand_step"]:                                                           # (:555-575) in one launch
                _check(lib().rh_rlwe_expand_step(rq._h, level, galEl, t[0].ptr, t[1].ptr, out.Value[0].ptr, out.Value[1].ptr, xinv[i].ptr, cnt))
            elif n >= gap:
                rot = ev.buffer("rpRot", rq, half, level + 1)
                x = self._replicated(xinv[i], cnt, rq, level)
                for k in (0, 1):
                    r, hi = _view(rot, 0, cnt), _view(out.Value[k], cnt, cnt)
                    rq.AutomorphismNTT(t[k], galEl, r)
                    rq.Sub(c[k], r, hi)
                    rq.Add(c[k], r, c[k])
                    rq.MulCoeffsMontgomery(hi, x, hi)
            elif use["rotate_add"]:                                                                       # (:580-581)
                ev.RotateAddQ(level, galEl, Ciphertext(t, is_ntt=True), Ciphertext(c, is_ntt=True))
            else:
                rot = ev.buffer("rpRot", rq, half, level + 1)
                for k in (0, 1):
                    r = _view(rot, 0, cnt)
                    rq.AutomorphismNTT(t[k], galEl, r)
                    rq.Add(c[k], r, c[k])
        return self._expand_done(ct, out, logN, logGap)

    def ExpandC(self, ct, logGap):
        """Expand as ONE call into the library (rh_rlwe_expand): what a compiled host uses.  Keys with more than one P modulus."""
        logN, ev, keys = self._expand_checks(ct, logGap)
        for g, evk in keys.items():
            if evk.LevelP() < 1 or evk.BaseTwoDecomposition:
                raise RingHipError("ExpandC: GaloisKey[%d] must have more than one P modulus and no power-of-two decomposition" % g)
        out, rq, level, B = self._expand_head(ct, logN, logGap, ev, scale=False)       # the call scales by 2^-logN itself
        table = (GaloisKeyEntry * max(len(keys), 1))()
        for i, (g, evk) in enumerate(keys.items()):
            table[i] = GaloisKeyEntry(g, evk.Q.ptr, evk.P.ptr, evk.digits)
        x = self.XInvPow2NTT[logN]
        _check(lib().rh_rlwe_expand(ev.be._h, level, ev.ringP.L - 1, out.Value[0].ptr, out.Value[1].ptr, B, logGap, x[0].ptr, x[0].limbs, table, len(keys)))
        return self._expand_done(ct, out, logN, logGap)

    # ---- Pack (:623-793) ------------------------------------------------------------------------------------------------------------------
    def Pack(self, cts, keys, inputLogGap, zeroGarbageSlots, fused=None):
        """(:623-793): cts is ONE batch, keys the sorted index of each of its ciphertexts.  A host plan (pack_plan) lists per level the Galois
        element and the (mode, slot_a, slot_b) entries; it is uploaded once, and sparse and dense index sets take the same path: one key switch
        per level over all its pairs.  Returns the ciphertext where index 0 ends, a view into cts (None where the reference returns nil).
        cts is CONSUMED, as in the reference: transformed to the NTT domain on entry (:699-703), scaled by 2^-(logEnd - logStart) (:705-706),
        and b X^k written over b (:726-727)."""
        keys = [int(k) for k in keys]
        if len(keys) == 0:
            raise RingHipError("len(cts) = 0")                                                          # (:625-627)
        if cts.Value[0].npoly != len(keys):
            raise RingHipError("Pack: the batch holds %d ciphertexts for %d keys" % (cts.Value[0].npoly, len(keys)))
        getMinimumGap(keys)
        logN = _log_n(cts)
        if logN not in self.parameters:
            raise RingHipError("eval.Parameters[%d] is nil" % logN)                                     # (:635-636)
        if self.RepackKeys is None:
            raise RingHipError("eval.RepackKeys is nil")                                                # (:641-643)
        if logN not in self.RepackKeys:
            raise RingHipError("eval.RepackKeys[%d] is nil" % logN)                                     # (:646-647)
        ev = self.Evaluators[logN]
        if ev.ringQ.kind != Standard:                                                                   # (:656-658)
            raise RingHipError("procedure is only supported for ring.Type = ring.Standard (X^{2^{i}} does not exist in the sub-ring Z[X + X^{-1}])")
        N = 1 << logN
        logStart, logEnd, levels, slot = pack_plan(N, keys, inputLogGap, zeroGarbageSlots)              # (:684-686)
        if cts.Degree() != 1:
            raise RingHipError("cts[%d].Degree() != 1" % keys[0])                                       # (:695-697)
        gk = self._galois_keys(self.RepackKeys[logN], [g for g, _, _ in levels])
        use = self._use(fused)
        level, nslots = cts.Level(), len(keys)
        ev._rows(level, *cts.Value)
        rq = ev.ringQ.AtLevel(level)
        Q = 1
        for q in ev.ringQ.moduli[:level + 1]:
            Q *= int(q)
        NInv = pow(1 << (logEnd - logStart), -1, Q)
        for c in (0, 1):
            if not cts.IsNTT:
                rq.NTT(cts.Value[c], cts.Value[c])
            rq.MulScalarBigint(cts.Value[c], NInv, cts.Value[c])
        cts.IsNTT = True
        Kmax = max([len(e) for _, _, e in levels] + [1])
        u = [ev.buffer("rpU%d" % c, rq, Kmax, level + 1) for c in (0, 1)]
        tmp = [ev.buffer("rpTmp%d" % c, rq, Kmax, level + 1) for c in (0, 1)]
        # the whole plan as one table of int32 triples, every level's part starting on an 8-byte word; uploaded once
        import ctypes as C
        host, offs = [], []
        for _, _, entries in levels:
            offs.append(len(host))
            host += [v for e in entries for v in e]
            host += [0] * (len(host) & 1)
        arr = np.ascontiguousarray(np.array(host + [0, 0], dtype=np.int32))
        dev = DevicePoly(rq, (arr.size // 2 + rq.N - 1) // rq.N, 1)
        _check(lib().rh_dev_upload(rq._h, dev.ptr, arr.view(np.uint64).ctypes.data_as(U64P), arr.size // 2))
        xpow = self.XPow2NTT[logN]
        for (galEl, xi, entries), off in zip(levels, offs):
            K = len(entries)
            tdev = dev.ptr + 4 * off
            thost = arr[off:off + 3 * K].ctypes.data_as(C.POINTER(C.c_int32))
            uk, tk = [_view(u[c], 0, K) for c in (0, 1)], [_view(tmp[c], 0, K) for c in (0, 1)]
            if use["pack_combine"]:                                                                     # (:726-745) over the level
                _check(lib().rh_rlwe_pack_combine(rq._h, level, cts.Value[0].ptr, cts.Value[1].ptr, nslots, tdev, thost, K, xpow[xi].ptr, uk[0].ptr, uk[1].ptr))
            else:
                for k, (mode, sa, sb) in enumerate(entries):
                    for c in (0, 1):
                        a, b, uu = _view(cts.Value[c], sa, 1), _view(cts.Value[c], sb, 1), _view(u[c], k, 1)
                        if mode == MODE_A:
                            rq.CopyLvl(a, uu)
                            continue
                        rq.MulCoeffsMontgomery(b, xpow[xi], b)
                        if mode == MODE_B:
                            rq.CopyLvl(b, uu)
                        else:
                            rq.Sub(a, b, uu)
                            rq.Add(a, b, a)
            self._key_switch(ev, level, uk[0], uk[1], gk[galEl], tk[0], tk[1])                           # the level's ONE key switch (:758-763, :781)
            if use["pack_finish"]:                                                                      # (:768-769, :786-787) over the level
                _check(lib().rh_rlwe_rotate_addsub_q(rq._h, level, galEl, tk[0].ptr, tk[1].ptr, cts.Value[0].ptr, cts.Value[1].ptr, nslots, tdev, thost, K))
            else:
                for c in (0, 1):
                    rq.AutomorphismNTT(tk[c], galEl, uk[c])
                    for k, (mode, sa, sb) in enumerate(entries):
                        dst, r = _view(cts.Value[c], sb if mode == MODE_B else sa, 1), _view(u[c], k, 1)
                        (rq.Sub if mode == MODE_B else rq.Add)(dst, r, dst)
        rq.sync()                                                        # the plan's device copy is released with this frame
        if slot is None:
            return None
        res = Ciphertext([_view(cts.Value[c], slot, 1) for c in (0, 1)], is_ntt=True)
        Evaluator._copy_metadata(cts, res)
        return res

    # ---- Split (:193-258), Merge (:396-464) -----------------------------------------------------------------------------------------------
    def _two_degrees(self):
        if self.MinLogN() == self.MaxLogN():
            raise RingHipError("method is not supported when eval.MinLogN() == eval.MaxLogN()")         # (:195-197, :251-253, :398-400, :450-452)

    def _switching_key(self, a, b):
        try:
            return self.RingSwitchingKeys[a][b]
        except (KeyError, TypeError):
            raise RingHipError("eval.RingSwitchingKeys[%d][%d] is nil" % (a, b))

    def Split(self, ctN, ctEvenNHalf, ctOddNHalf):
        """(:193-246): ctN[X] = ctEvenNHalf[Y] + X ctOddNHalf[Y], Y = X^2: ONE key switch to the small secret, one inverse transform pair at N, the
        split kernel for both halves, the small ring's transform.  ctOddNHalf may be None.  The metadata is ctN's with LogDimensions one less
        (:227-229, :238-242).  NTT domain only: the device ApplyEvaluationKey takes no coefficient-domain ciphertext."""
        self._two_degrees()
        LogN = _log_n(ctN)
        if LogN <= self.MinLogN():
            raise RingHipError("ctN.Log() must be greater than eval.MinLogN()")                         # (:199-201)
        if ctEvenNHalf is None:
            raise RingHipError("ctEvenNHalf cannot be nil")                                             # (:203-205)
        if _log_n(ctEvenNHalf) != LogN - 1:
            raise RingHipError("ctEvenNHalf.LogN() must be equal to ctN.LogN()-1")                      # (:207-209)
        if ctOddNHalf is not None and _log_n(ctOddNHalf) != LogN - 1:
            raise RingHipError("ctOddNHalf.LogN() must be equal to ctN.LogN()-1")                       # (:234-236)
        if not ctN.IsNTT:
            raise RingHipError("Split: coefficient-domain ciphertexts are not supported by the device path")
        ev, evk = self.Evaluators[LogN], self._switching_key(LogN, LogN - 1)
        level, npoly = ctN.Level(), ctN.Value[0].npoly
        outs = [ctEvenNHalf] + ([ctOddNHalf] if ctOddNHalf is not None else [])
        ev._rows(level, *ctN.Value)
        for o in outs:
            ev._rows(level, *o.Value)
            if o.Value[0].npoly != npoly:
                raise RingHipError("Split: the halves hold another number of ciphertexts than ctN")
        rq = ev.ringQ.AtLevel(level)
        tmp = [ev.buffer("rpSw%d" % c, rq, npoly, level + 1) for c in (0, 1)]
        self._key_switch(ev, level, ctN.Value[0], ctN.Value[1], evk, tmp[0], tmp[1])                   # SkN -> SkNHalf (:219)
        for c in (0, 1):
            rq.INTT(tmp[c], tmp[c])
        odd = ctOddNHalf.Value if ctOddNHalf is not None else (None, None)
        _check(lib().rh_rlwe_ring_split(rq._h, level, tmp[0].ptr, tmp[1].ptr, ctEvenNHalf.Value[0].ptr, ctEvenNHalf.Value[1].ptr,
                                        odd[0].ptr if odd[0] is not None else None, odd[1].ptr if odd[1] is not None else None, 1, npoly))
        for o in outs:
            for c in (0, 1):
                _small_ntt(o.Value[c].ring.AtLevel(level), o.Value[c])
            Evaluator._copy_metadata(ctN, o)
            if hasattr(o, "LogDimensions"):
                o.LogDimensions -= 1

    def _new(self, logN, level, npoly):
        rq = self.parameters[logN][0].AtLevel(level)
        return Ciphertext([DevicePoly(rq, npoly, level + 1) for _ in (0, 1)], is_ntt=True)

    def SplitNew(self, ctN):
        """(:250-258)"""
        self._two_degrees()
        LogN = _log_n(ctN)
        if LogN - 1 not in self.parameters:
            raise RingHipError("ctN.Log() must be greater than eval.MinLogN()")
        even, odd = self._new(LogN - 1, ctN.Level(), ctN.Value[0].npoly), self._new(LogN - 1, ctN.Level(), ctN.Value[0].npoly)
        self.Split(ctN, even, odd)
        return even, odd

    def Merge(self, ctEvenNHalf, ctOddNHalf, ctN):
        """(:396-444): ctN[X] = ctEvenNHalf[Y] + X ctOddNHalf[Y]: the merge kernel (replication, and the product with X and the sum when there is an
        odd half), then ONE key switch to the large secret.  The metadata is ctEvenNHalf's with LogDimensions one more (:428, :442).  NTT domain only."""
        self._two_degrees()
        if ctEvenNHalf is None:
            raise RingHipError("ctEvenNHalf cannot be nil")                                             # (:402-404)
        if _log_n(ctEvenNHalf) >= self.MaxLogN():
            raise RingHipError("ctEvenNHalf.LogN() must be smaller than eval.MaxLogN()")                # (:406-408)
        if _log_n(ctN) != _log_n(ctEvenNHalf) + 1:
            raise RingHipError("ctN.LogN() must be equal to ctEvenNHalf.LogN()+1")                      # (:410-412)
        if ctOddNHalf is not None and _log_n(ctEvenNHalf) != _log_n(ctOddNHalf):
            raise RingHipError("ctEvenNHalf.LogN() and ctOddNHalf.LogN() must be equal")                # (:414-418)
        if not ctEvenNHalf.IsNTT or (ctOddNHalf is not None and not ctOddNHalf.IsNTT):
            raise RingHipError("Merge: coefficient-domain ciphertexts are not supported by the device path")
        LogN = _log_n(ctN)
        ev, evk = self.Evaluators[LogN], self._switching_key(LogN - 1, LogN)
        level, npoly = ctN.Level(), ctN.Value[0].npoly
        ev._rows(level, *ctN.Value, *ctEvenNHalf.Value, *(ctOddNHalf.Value if ctOddNHalf is not None else ()))
        if ctEvenNHalf.Value[0].npoly != npoly or (ctOddNHalf is not None and ctOddNHalf.Value[0].npoly != npoly):
            raise RingHipError("Merge: the halves hold another number of ciphertexts than ctN")
        rq = ev.ringQ.AtLevel(level)
        tmp = [ev.buffer("rpSw%d" % c, rq, npoly, level + 1) for c in (0, 1)]
        odd = ctOddNHalf.Value if ctOddNHalf is not None else (None, None)
        _check(lib().rh_rlwe_ring_merge(rq._h, level, ctEvenNHalf.Value[0].ptr, ctEvenNHalf.Value[1].ptr, odd[0].ptr if odd[0] is not None else None,
                                        odd[1].ptr if odd[1] is not None else None, self.XPow2NTT[LogN][0].ptr, tmp[0].ptr, tmp[1].ptr, 1, npoly))
        self._key_switch(ev, level, tmp[0], tmp[1], evk, ctN.Value[0], ctN.Value[1])                   # SkNHalf -> SkN (:438)
        Evaluator._copy_metadata(ctEvenNHalf, ctN)
        ctN.IsNTT = True
        if hasattr(ctN, "LogDimensions"):
            ctN.LogDimensions += 1

    def MergeNew(self, ctEvenNHalf, ctOddNHalf):
        """(:448-464)"""
        self._two_degrees()
        if ctEvenNHalf is None:
            raise RingHipError("ctEvenNHalf cannot be nil")
        if _log_n(ctEvenNHalf) >= self.MaxLogN():
            raise RingHipError("ctEvenNHalf.LogN() must be smaller than eval.MaxLogN()")
        ctN = self._new(_log_n(ctEvenNHalf) + 1, ctEvenNHalf.Level(), ctEvenNHalf.Value[0].npoly)
        self.Merge(ctEvenNHalf, ctOddNHalf, ctN)
        return ctN

    # ---- Extract (:70-189), Repack (:260-392) ---------------------------------------------------------------------------------------------
    def Extract(self, ct, idx):
        return self._extract(ct, idx, False)

    def ExtractNaive(self, ct, idx):
        return self._extract(ct, idx, True)

    def _extract(self, ct, idx, naive):
        """extract (:90-189) on ONE ciphertext -> {index: ciphertext of degree 2^MinLogN}, views into one batch per bucket.  With one index
        getMinimumGap returns logGap = 0 (:101), so everything is expanded."""
        if ct.Value[0].npoly != 1:
            raise RingHipError("Extract: one ciphertext at a time (Expand takes batches)")
        logNMax, logNMin, level = _log_n(ct), self.MinLogN(), ct.Level()
        logNFactor = logNMax - logNMin
        NFactor = 1 << logNFactor
        keys = sorted(int(i) for i in idx)
        _, logGap = getMinimumGap(keys)
        tmpCts = {0: ct}
        for i in range(logNFactor):
            t = 1 << i
            logGap = max(0, logGap - 1)
            for j in range(t):
                if tmpCts.get(j) is not None:
                    tmpCts[j], tmpCts[j + t] = self.SplitNew(tmpCts[j])
        buckets = {}
        for i in keys:
            buckets.setdefault(i & (NFactor - 1), []).append(i // NFactor)
        out = {}
        for i, want in buckets.items():
            src = tmpCts[i]
            if naive:
                rq = self.parameters[logNMin][0].AtLevel(level)
                xinv = self.XInvPow2NTT[logNMin]
                batch = self._new(logNMin, level, len(want))
                for s, j in enumerate(want):
                    for c in (0, 1):
                        dst = _view(batch.Value[c], s, 1)
                        rq.CopyLvl(src.Value[c], dst)
                        for b in range(logNMin):
                            if (j >> b) & 1:
                                rq.MulCoeffsMontgomery(dst, xinv[b], dst)                              # (:162-170)
                where = {j: s for s, j in enumerate(want)}
            else:
                batch, index = self.Expand(src, logGap)
                where = {j: s for s, j in enumerate(index)}
            for j in want:
                if j not in where:
                    raise RingHipError("invalid ciphertexts map: index i+j*(NFactor*gap)=%d is nil" % (i + j * (NFactor << logGap)))
                one = Ciphertext([_view(batch.Value[c], where[j], 1) for c in (0, 1)], is_ntt=True)
                Evaluator._copy_metadata(src if naive else batch, one)
                one.IsNTT = True
                out[i + j * NFactor] = one
        return out

    def Repack(self, cts):
        return self._repack(cts, False)

    def RepackNaive(self, cts):
        return self._repack(cts, True)

    def _repack(self, cts, naive):
        """repack (:291-392) on {index: ciphertext}: the ciphertexts of a bucket are gathered into one batch and packed by ONE Pack; the buckets are
        merged in the reference's tree.  Its merge loop tests ctsLargeN[j+1], not ctsLargeN[j+t] (:377): a node without an even half therefore
        fails with Merge's "ctEvenNHalf cannot be nil" or, when [j+1] is empty too, is dropped -- kept."""
        keys = sorted(cts)
        first = cts[keys[0]]
        logNMin, logNMax, level = _log_n(first), self.MaxLogN(), first.Level()
        logNFactor = logNMax - logNMin
        NFactor = 1 << logNFactor
        rq = self.parameters[logNMin][0].AtLevel(level)
        small = [dict() for _ in range(NFactor)]
        for i in keys:
            small[i & (NFactor - 1)][i // NFactor] = cts[i]
        large = {}
        for i in range(NFactor):
            ks = sorted(small[i])
            if not ks:
                if naive:
                    large[i] = None
                continue
            batch = self._new(logNMin, level, len(ks))
            for s, k in enumerate(ks):
                for c in (0, 1):
                    rq.CopyLvl(small[i][k].Value[c], _view(batch.Value[c], s, 1))
            Evaluator._copy_metadata(small[i][ks[0]], batch)
            batch.IsNTT = small[i][ks[0]].IsNTT
            if naive:
                large[i] = self._pack_naive(batch, ks, logNMin, rq)
            else:
                large[i] = self.Pack(batch, ks, logNMin, True)
        for i in range(logNFactor - 1, -1, -1):
            t = 1 << i
            for j in range(t):
                if large.get(j) is not None or large.get(j + 1) is not None:
                    large[j] = self.MergeNew(large.get(j), large.get(j + t))
                    large[j + t] = None
        return large.get(0)

    def _pack_naive(self, batch, keys, logN, rq):
        """the naive branch of repack (:322-360): b X^(N/2^(l+1)) added to a, no key switch, no zeroing"""
        xpow = self.XPow2NTT[logN]
        pos = {k: s for s, k in enumerate(keys)}
        for l in range(logN):
            t = 1 << (logN - 1 - l)
            for jx in range(t):
                a, b = pos.get(jx), pos.get(jx + t)
                if b is None:
                    continue
                for c in (0, 1):
                    vb = _view(batch.Value[c], b, 1)
                    rq.MulCoeffsMontgomery(vb, xpow[len(xpow) - l - 1], vb)
                    if a is not None:
                        va = _view(batch.Value[c], a, 1)
                        rq.Add(va, vb, va)
                if a is None:
                    pos[jx] = b
                del pos[jx + t]
        slot = pos.get(0)
        if slot is None:
            return None
        res = Ciphertext([_view(batch.Value[c], slot, 1) for c in (0, 1)], is_ntt=True)
        Evaluator._copy_metadata(batch, res)
        return res


# ---- keys and ciphertexts made on the device: the samplers (sampling.py) and core/rlwe/keygenerator.go, encryptor.go, decryptor.go (keygen.py) --------
from .sampling import (  # noqa: E402,F401
    KeyedPRNG, NewPRNG, UniformSampler, GaussianSampler, TernarySampler, SmallPoly, lift_small, gaussian_table,
)
from .keygen import (  # noqa: E402,F401
    SecretKey, PublicKey, EvaluationKey, RelinearizationKey, GaloisKey, MemEvaluationKeySet, KeyGenerator, Encryptor, Decryptor, Plaintext,
)
# ---- the noise meters: ring.Log2OfStandardDeviation and core/rlwe/utils.go:13-183 (noise.py) ----------------------------------------------------------
from .noise import (  # noqa: E402,F401
    FUSED_NOISE, NoisePublicKey, NoiseRelinearizationKey, NoiseGaloisKey, NoiseGaloisKeys, NoiseGadgetCiphertext, NoiseEvaluationKey, Norm, NormStats,
    CenteredMomentsQP, Log2OfStandardDeviationQP,
)

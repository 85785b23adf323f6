"""Host-side mirror of the key-switch callers in core/rlwe: the evaluator methods that
sequence the ring hot path for rotations and relinearisation, on device-resident batches.  Every step is a call into
the HIP library; no key generation, no encoders (those stay with the reference).

  GadgetProduct          core/rlwe/evaluator_gadget_product.go:16-30
  DecomposeNTT           :431-453        GadgetProductHoisted   :326-349
  Automorphism           core/rlwe/evaluator_automorphism.go:14-60      AutomorphismHoisted  :62-105
  ApplyEvaluationKey     core/rlwe/evaluator_evaluationkey.go:37-123 (same ring degree)   Relinearize  :125-153

GadgetProduct covers both branches of GadgetProductLazy (:102-121): gadgetProductMultiplePLazy (levelP >= 1) and
gadgetProductSinglePAndBitDecompLazy (levelP <= 0, optional BaseTwoDecomposition), for NTT- and coefficient-domain ciphertexts.
The hoisted forms and the automorphism / relinearisation callers take NTT-domain ciphertexts and levelP >= 1.

  PartialTracesSum       core/rlwe/inner_sum.go:152-291     Trace  :36-121     InnerFunction  :316-440     Replicate  :477-479
  GaloisElementsForInnerSum  :444-468     GaloisElementsForReplicate  :483-485     GaloisElementsForTrace  :125-146

The sums of rotations take NTT- and coefficient-domain ciphertexts on standard rings, keys with levelP >= 1 and no power-of-two decomposition."""
import numpy as np

from .ringhip import BasisExtender, DevicePoly, GaloisKeyEntry, RingHipError, Standard, _check, lib
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
        """(:37-123), same ring degree on both sides (:97-99 -> applyEvaluationKey :105-112):
        opOut = (ctIn[0] + KS(ctIn[1])_0, KS(ctIn[1])_1).  The ring-degree switching branches are not built."""
        if ctIn.Degree() != 1 or opOut.Degree() != 1:
            raise RingHipError("cannot ApplyEvaluationKey: input and output Ciphertext must be of degree 1")
        if not ctIn.IsNTT:
            raise RingHipError("ApplyEvaluationKey: coefficient-domain ciphertexts are not supported by the device path")
        level = min(ctIn.Level(), opOut.Level())
        ringQ = self.ringQ.AtLevel(level)
        npoly = ctIn.Value[1].npoly
        self.GadgetProductThenAdd(level, ctIn.Value[1], evk, ctIn.Value[0], None, opOut)   # (:108-111) with the Add in the epilogue
        opOut.IsNTT = True

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
        self.GadgetProductThenAdd(level, ctIn.Value[1], evk, ctIn.Value[0], None, tmp)         # product + ringQ.Add (:42-44)
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

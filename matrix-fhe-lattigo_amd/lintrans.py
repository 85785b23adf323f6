"""Homomorphic linear transformations (diagonal matrix x ciphertext) for CKKS on device batches: circuits/common/lintrans/lintrans.go,
circuits/common/lintrans/lintrans_evaluator.go and circuits/ckks/lintrans/lintrans.go.

  Parameters, Diagonals (At :97-122, Evaluate ckks/lintrans:24-56), Permutation / PermutationMapping (GetDiagonals ckks/lintrans:78-100)
  BSGSIndex :344-367     FindBestBSGSRatio :321-341     GaloisElements :297-318
  LinearTransformation, NewTransformation :148-201     Encode :205-292     (NewTransformationFromBlock: both for a whole device block, dft.py)
  Evaluator: EvaluateMany lintrans_evaluator.go:18-68, PreRotatedCiphertextForDiagonalMatrixMultiplication :71-99, EvaluateSequential :102-124,
             MultiplyByDiagMatrix :131-250, MultiplyByDiagMatrixBSGS :256-433

A diagonal is ONE rlwe.PolyQP (npoly = 1) shared by every ciphertext of a batch.  The three streaming passes the circuits spend their time in are
kernels of csrc/lintrans.hip (rh_rlwe_diag_mac_qp, rh_rlwe_rotate_sum_accumulate_qp, rh_rlwe_rotate_mul_accumulate_qp); the composed paths issue
the reference's own ring calls through the existing entries and give the same bits.

The reference's lazy sums (MulCoeffsMontgomeryLazy(ThenAddLazy), AddLazy, AutomorphismNTTWithIndexThenAddLazy) all end in Reduce before anything
reads them (:220-239, :349-357, :419-427), so every value that leaves a loop is the canonical residue of the exact sum, whatever the schedule of the
QiOverF / PiOverF reductions; both paths here keep canonical residues throughout.

BGV linear transformations (circuits/bgv/lintrans) are bgv_lintrans.py: its Evaluator is the one below with the scheme's points overridden -- the
scale of the input, the scale of the output, the rescale of EvaluateSequential and the slot count (the hooks _ks_of, _scale_in, _scale_out, _rescale
and LinearTransformation.Slots).

Not built: conjugate-invariant and 3N rings, the big-float encoding path."""
import ctypes as C
import math

import numpy as np

from . import rlwe
from .ckks import Scale
from .ringhip import DevicePoly, RingHipError, Standard, _check, lib
from .schemes import Ciphertext


# ---- index arithmetic (lintrans.go) ----------------------------------------------------------------------------------------------------------
def BSGSIndex(nonZeroDiags, slots, N1):
    """(:344-367) -> (index, rotN1, rotN2): index maps a giant step to its sorted baby steps; rotN1 the sorted giant steps, rotN2 the sorted
    baby steps"""
    index, rotN1, rotN2 = {}, set(), set()
    for rot in nonZeroDiags:
        rot &= slots - 1
        idxN1 = ((rot // N1) * N1) & (slots - 1)
        idxN2 = rot & (N1 - 1)
        index.setdefault(idxN1, []).append(idxN2)
        rotN1.add(idxN1)
        rotN2.add(idxN2)
    for k in index:
        index[k].sort()
    return index, sorted(rotN1), sorted(rotN2)


def _go_div(a, b):
    """float64(a) / float64(b) as Go evaluates it: +-Inf or NaN where Python raises"""
    if b == 0:
        return math.nan if a == 0 else math.copysign(math.inf, a)
    return float(a) / float(b)


def FindBestBSGSRatio(nonZeroDiags, maxN, logMaxRatio):
    """(:321-341): the first N1 = 1, 2, 4 ... < maxN whose (#baby steps - 1) / (#giant steps - 1) reaches 2^logMaxRatio, halved when it passes it"""
    maxRatio = float(1 << logMaxRatio)
    N1 = 1
    while N1 < maxN:
        _, rotN1, rotN2 = BSGSIndex(nonZeroDiags, maxN, N1)
        nbN1, nbN2 = len(rotN1) - 1, len(rotN2) - 1
        r = _go_div(nbN2, nbN1)
        if r == maxRatio:
            return N1
        if r > maxRatio:
            return N1 // 2
        N1 <<= 1
    return 1


def GaloisElements(N, diags, slots, logBabyStepGianStepRatio):
    """(:297-318) on a standard ring of degree N: the Galois elements of every rotation the evaluation applies (the rotation by 0 included, as
    the reference lists it).  With BSGS the reference returns the distinct rotations in map order; here they are sorted."""
    if logBabyStepGianStepRatio < 0:
        _, _, rotN2 = BSGSIndex(diags, slots, slots)
        return [rlwe.GaloisElement(N, r) for r in rotN2]
    N1 = FindBestBSGSRatio(diags, slots, logBabyStepGianStepRatio)
    _, rotN1, rotN2 = BSGSIndex(diags, slots, N1)
    return [rlwe.GaloisElement(N, r) for r in sorted(set(rotN1) | set(rotN2))]


class Parameters:
    """lintrans.Parameters (:51-81).  LogDimensions: the log2 of the slot count (Cols; Rows is 0, as ckks.Plaintext carries it)"""

    def __init__(self, DiagonalsIndexList, LevelQ, LevelP, Scale, LogDimensions, LogBabyStepGiantStepRatio=0):
        self.DiagonalsIndexList = [int(i) for i in DiagonalsIndexList]
        self.LevelQ, self.LevelP = int(LevelQ), int(LevelP)
        self.Scale = Scale
        self.LogDimensions = int(LogDimensions)
        self.LogBabyStepGiantStepRatio = int(LogBabyStepGiantStepRatio)

    def GaloisElements(self, N):
        """ckks/lintrans GaloisElements(params, lt) (:127-129)"""
        return GaloisElements(N, self.DiagonalsIndexList, 1 << self.LogDimensions, self.LogBabyStepGiantStepRatio)


class Diagonals(dict):
    """lintrans.Diagonals: diagonal index -> the vector of its `slots` values"""

    def DiagonalsIndexList(self):
        return list(self.keys())

    def At(self, i, slots):
        """(:97-122) as written: a missing positive index i falls back to i - slots; for a missing index i <= 0 the reference's second arm tests
        its own zero-initialised j, never holds, and the call fails with "cannot At[0]" """
        if i in self:
            return self[i]
        if i > 0:
            j = i - slots
        else:
            raise RingHipError("cannot At[0]: diagonal does not exist")
        if j not in self:
            raise RingHipError("cannot At[%d or %d]: diagonal does not exist" % (i, j))
        return self[j]

    def Evaluate(self, vector, newVec=None, add=None, muladd=None):
        """(ckks/lintrans:24-56): the transformation on a plain vector, by the BSGS schedule of ratio 1.  Without the callbacks: exact Python arithmetic on
        whatever the entries are (ints, Fractions, complex)"""
        slots = len(vector)
        newVec = newVec or (lambda size: [0] * size)
        if add is None:
            def add(a, b, c):
                c[:] = [x + y for x, y in zip(a, b)]
        if muladd is None:
            def muladd(a, b, c):
                c[:] = [z + x * y for x, y, z in zip(a, b, c)]
        rotate = lambda v, k: [v[(i + k) % len(v)] for i in range(len(v))]                # utils.RotateSlice: to the left
        keys = list(self.keys())
        N1 = FindBestBSGSRatio(keys, slots, 1)
        index, _, _ = BSGSIndex(keys, slots, N1)
        res = newVec(slots)
        for j in index:
            rot = -j & (slots - 1)
            tmp = newVec(slots)
            for i in index[j]:
                v = self[j + i] if j + i in self else self[j + i - slots]
                muladd(rotate(list(vector), i), rotate(list(v), rot), tmp)
            add(res, rotate(tmp, j), res)
        return res


class PermutationMapping:
    """(ckks/lintrans:60-64)"""

    def __init__(self, From, To, Scaling):
        self.From, self.To, self.Scaling = int(From), int(To), Scaling


class Permutation(list):
    """(ckks/lintrans:73): a list of PermutationMapping"""

    def GetDiagonals(self, logSlots):
        """(:78-100)"""
        slots = 1 << logSlots
        diagonals = Diagonals()
        for pm in self:
            diagIndex = (slots + pm.From - pm.To) & (slots - 1)
            if diagIndex not in diagonals:
                diagonals[diagIndex] = [0] * slots
            diagonals[diagIndex][pm.To] = pm.Scaling
        return diagonals


class LinearTransformation:
    """lintrans.LinearTransformation (:127-134) with its embedded MetaData: Vec maps a diagonal index to an rlwe.PolyQP of ONE poly (NTT domain,
    Montgomery form) shared by every ciphertext of a batch"""

    def __init__(self, LogBabyStepGiantStepRatio, N1, LevelQ, LevelP, Vec, Scale, LogDimensions):
        self.LogBabyStepGiantStepRatio, self.N1, self.LevelQ, self.LevelP, self.Vec = LogBabyStepGiantStepRatio, N1, LevelQ, LevelP, Vec
        self.Scale, self.LogDimensions = Scale, LogDimensions
        self.IsBatched, self.IsNTT, self.IsMontgomery = True, True, True                   # (:181-191)

    def Slots(self):
        """1 << LogDimensions.Cols: the length of a row, which the rotations act on"""
        return 1 << self.LogDimensions

    def BSGSIndex(self):
        return BSGSIndex(list(self.Vec.keys()), self.Slots(), self.N1)

    def GaloisElements(self, N):
        return GaloisElements(N, list(self.Vec.keys()), self.Slots(), self.LogBabyStepGiantStepRatio)


def _rings_at(ringQ, ringP, levelQ, levelP):
    """ringQP.AtLevel(levelQ, levelP) (:157) as the pair of level views"""
    if ringP is None:
        raise RingHipError("cannot NewTransformation: a linear transformation is encoded modulo QP and needs ringP")
    if not (0 <= levelQ < ringQ.L and 0 <= levelP < ringP.L):
        raise RingHipError("cannot NewTransformation: LevelQ = %d, LevelP = %d out of range" % (levelQ, levelP))
    return ringQ.AtLevel(levelQ), ringP.AtLevel(levelP)


def _vec_keys(diagslist, cols, logBabyStepGiantStepRatio):
    """(:161-179) -> (N1, the keys of Vec in the order the reference allocates them)"""
    keys = []
    if logBabyStepGiantStepRatio < 0:
        N1 = 0
        for i in diagslist:
            keys.append(i + cols if i < 0 else i)
    else:
        N1 = FindBestBSGSRatio(diagslist, cols, logBabyStepGiantStepRatio)
        index, _, _ = BSGSIndex(diagslist, cols, N1)
        for j in index:
            for i in index[j]:
                keys.append(j + i)
    return N1, keys


def NewTransformation(ringQ, ringP, ltparams):
    """NewLinearTransformation (:148-201): the diagonals allocated (not zeroed: Encode writes every one it is given) at (LevelQ, LevelP)"""
    cols = 1 << ltparams.LogDimensions
    levelQ, levelP = ltparams.LevelQ, ltparams.LevelP
    rq, rp = _rings_at(ringQ, ringP, levelQ, levelP)
    N1, keys = _vec_keys(ltparams.DiagonalsIndexList, cols, ltparams.LogBabyStepGiantStepRatio)
    vec = {k: rlwe.PolyQP(DevicePoly(rq, 1, levelQ + 1), DevicePoly(rp, 1, levelP + 1)) for k in keys}
    scale = ltparams.Scale if isinstance(ltparams.Scale, Scale) else Scale(ltparams.Scale)
    return LinearTransformation(ltparams.LogBabyStepGiantStepRatio, N1, levelQ, levelP, vec, scale, ltparams.LogDimensions)


def _rotate_and_encode_diagonal(v, encoder, rot, metaData, poly):
    """rotateAndEncodeDiagonal (:271-292), Rows = 0: the values rotated to the left by rot, then embedded"""
    cols = 1 << metaData.LogDimensions
    rot &= cols - 1
    v = list(v)
    values = v[rot:] + v[:rot] if rot else v
    encoder.Embed(np.asarray(values), metaData, poly)


def Encode(encoder, diagonals, allocated):
    """(:205-292): every diagonal of `diagonals` onto the allocated transformation; with BSGS the values of giant step j are rotated by -j first
    (:246-262)"""
    if encoder.Prec() > 53:
        raise RingHipError("cannot Encode: encoder precision %d > 53 needs the *big.Float / *bignum.Complex encoder, which stays with the reference" % encoder.Prec())
    for v, rot, idx in _encode_walk(diagonals, allocated):
        _rotate_and_encode_diagonal(v, encoder, rot, allocated, allocated.Vec[idx])


def _encode_walk(diagonals, allocated):
    """the loops of Encode (:221-266) with its refusals: (values, rotation, key of Vec) per diagonal, in the reference's order"""
    cols = allocated.Slots()
    N1 = allocated.N1
    if N1 == 0:
        for i in diagonals.DiagonalsIndexList():
            idx = i + cols if i < 0 else i
            if idx not in allocated.Vec:
                raise RingHipError("cannot Encode: error encoding on LinearTransformation: plaintext diagonal [%d] does not exist" % idx)
            try:
                v = diagonals.At(i, cols)
            except RingHipError as e:
                raise RingHipError("cannot Encode: %s" % e) from None
            yield v, 0, idx
    else:
        index, _, _ = allocated.BSGSIndex()
        for j in index:
            rot = -j & (cols - 1)
            for i in index[j]:
                if i + j not in allocated.Vec:
                    raise RingHipError("cannot Encode: error encoding on LinearTransformation BSGS: input does not match the same non-zero diagonals")
                try:
                    v = diagonals.At(i + j, cols)
                except RingHipError as e:
                    raise RingHipError("cannot Encode: %s" % e) from None
                yield v, rot, i + j


def _view(p, k):
    """poly k of a batch as a batch of its own"""
    return DevicePoly(p.ring, 1, p.limbs, ptr=p.ptr + k * p.limbs * p.ring.N * 8, owner=p)


def NewTransformationFromBlock(ringQ, ringP, ltparams, encoder, index, block):
    """NewTransformation and Encode in the block form (dft.NewMatrixFromLiteral): `block`, a ckks.DeviceValues of shape (len(index), cols) whose
    row k holds diagonal index[k] of ltparams.DiagonalsIndexList ALREADY rotated as Encode rotates it (:246-262), goes through ONE Encoder.Embed
    into ONE contiguous rlwe.PolyQP of len(index) polys; the entries of Vec are one-poly views that keep the block alive."""
    if encoder.Prec() > 53:
        raise RingHipError("cannot Encode: encoder precision %d > 53 needs the *big.Float / *bignum.Complex encoder, which stays with the reference" % encoder.Prec())
    cols = 1 << ltparams.LogDimensions
    levelQ, levelP = ltparams.LevelQ, ltparams.LevelP
    rq, rp = _rings_at(ringQ, ringP, levelQ, levelP)
    index = [int(i) for i in index]
    if sorted(i & (cols - 1) for i in ltparams.DiagonalsIndexList) != sorted(index) or len(set(index)) != len(index):
        raise RingHipError("cannot NewTransformation: the block's rows are not the diagonals of DiagonalsIndexList")
    if block.nvec != len(index) or block.n != cols or not block.complex:
        raise RingHipError("cannot NewTransformation: the block must be complex128 of shape (%d, %d)" % (len(index), cols))
    N1 = 0 if ltparams.LogBabyStepGiantStepRatio < 0 else FindBestBSGSRatio(index, cols, ltparams.LogBabyStepGiantStepRatio)
    scale = ltparams.Scale if isinstance(ltparams.Scale, Scale) else Scale(ltparams.Scale)
    qp = rlwe.PolyQP(DevicePoly(rq, len(index), levelQ + 1), DevicePoly(rp, len(index), levelP + 1))
    lt = LinearTransformation(ltparams.LogBabyStepGiantStepRatio, N1, levelQ, levelP, {}, scale, ltparams.LogDimensions)
    encoder.Embed(block, lt, qp)
    lt.Vec = {k: rlwe.PolyQP(_view(qp.Q, row), _view(qp.P, row)) for row, k in enumerate(index)}
    return lt


class Evaluator:
    """lintrans.Evaluator over a ckks.Evaluator (NewEvaluator, ckks/lintrans:139-145), on batches of ciphertexts that share the transformation.

    fused (per call, or FUSED_LINTRANS when None): the kernels of csrc/lintrans.hip (True) or the reference's own ring calls (False), per pass:
      diag_mac    the inner loop of MultiplyByDiagMatrixBSGS, one launch per giant step (rh_rlwe_diag_mac_qp)
      giant_tail  its giant-step tail, ringQP.Add and the two automorphisms modulo QP (rh_rlwe_rotate_sum_accumulate_qp)
      naive_step  one diagonal of MultiplyByDiagMatrix (rh_rlwe_rotate_mul_accumulate_qp)
    The bits are the same."""

    # A kernel is the default where the measurement shows it no slower than the calls it replaces, alone and in the whole Evaluate, at batches of
    # 1 and 8 (tools/bench_ops.py lintrans -> profiles/lintrans.json, "fused_lintrans_default"): all three are.
    FUSED_LINTRANS = {"diag_mac": True, "giant_tail": True, "naive_step": True}

    def __init__(self, eval):
        self.eval = eval
        self.ringQ, self.ringP = eval.ringQ, eval.ringP
        if self.ringQ.kind != Standard:
            raise RingHipError("cannot NewEvaluator: linear transformations on conjugate-invariant and 3N rings are not supported by the device path")
        self.ks = self._ks_of(eval)
        if self.ks is None:
            raise RingHipError("cannot NewEvaluator: the evaluator was built without ringP, which the key switch needs")

    # ---- the scheme's points (bgv_lintrans.Evaluator overrides them) ----------------------------------------------------------------------------
    @staticmethod
    def _ks_of(eval):
        """the rlwe.Evaluator that holds the Galois keys and the key-switch buffers, None without ringP"""
        return eval.ks

    def _scale_in(self, ctIn):
        return self.eval._scale(ctIn, "EvaluateMany")

    @staticmethod
    def _scale_out(scaleIn, lt):
        """opOut.Scale = opOut.Scale.Mul(matrix.Scale)"""
        return scaleIn.Mul(lt.Scale)

    def _use(self, fused):
        """fused: None (FUSED_LINTRANS), True / False (every kernel / none), or a dict kernel -> bool over FUSED_LINTRANS (measurements)"""
        if fused is None:
            return dict(self.FUSED_LINTRANS)
        if isinstance(fused, dict):
            return {k: bool(fused.get(k, v)) for k, v in self.FUSED_LINTRANS.items()}
        return {k: bool(fused) for k in self.FUSED_LINTRANS}

    # ---- buffers (eval.BuffQP / BuffCt / BuffDecompQP of the reference) -------------------------------------------------------------------------
    def _qp(self, tag, levelQ, levelP, npoly):
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        return rlwe.ElementQP([rlwe.PolyQP(self.ks.buffer("%sQ%d" % (tag, c), rq, npoly, levelQ + 1), self.ks.buffer("%sP%d" % (tag, c), rp, npoly, levelP + 1))
                               for c in (0, 1)])

    def _ct(self, tag, levelQ, npoly):
        rq = self.ringQ.AtLevel(levelQ)
        return Ciphertext([self.ks.buffer("%s%d" % (tag, c), rq, npoly, levelQ + 1) for c in (0, 1)], is_ntt=True)

    def _dec(self, levelQ, levelP, npoly):
        beta = self.ks.BaseRNSDecompositionVectorSize(levelQ, levelP)
        return (self.ks.buffer("BuffDecompQ", self.ringQ.AtLevel(levelQ), beta * npoly, levelQ + 1),
                self.ks.buffer("BuffDecompP", self.ringP.AtLevel(levelP), beta * npoly, levelP + 1))

    def _P(self, levelP):
        P = 1
        for p in self.ringP.moduli[:levelP + 1]:
            P *= int(p)
        return P

    def _key(self, galEl, levelP, who):
        """CheckAndGetGaloisKey and the LevelP check of :194-196 / :373-375, plus what the hoisted products of the device path ask of a key"""
        if galEl not in self.ks.galois_keys:
            raise RingHipError("cannot %s: CheckAndGetGaloisKey: GaloisKey[%d] is missing" % (who, galEl))
        evk = self.ks.galois_keys[galEl]
        if evk.BaseTwoDecomposition != 0:
            raise RingHipError("cannot %s: method is unsupported for BaseTwoDecomposition != 0" % who)
        if evk.LevelP() < 1:
            raise RingHipError("cannot %s: GaloisKey[%d] has one P modulus, which the hoisted product of the device path does not take (levelP >= 1)" % (who, galEl))
        if evk.LevelP() != levelP:
            raise RingHipError("LinearTransformation.LevelP = %d != GaloiKey[%d].LevelP() = %d: ensure that the levelP of the linear transformation is the same "
                               "as the levelP of the GaloisKeys" % (levelP, galEl, evk.LevelP()))
        return evk

    def _keys_of(self, lt, levelP):
        """every key a transformation needs, looked up before the first launch"""
        N = self.ringQ.N
        slots = lt.Slots()
        if lt.N1 == 0:
            rots, who = [k & (slots - 1) for k in sorted(lt.Vec) if k != 0], "MultiplyByDiagMatrix"
        else:
            _, rotN1, rotN2 = lt.BSGSIndex()
            rots, who = [r for r in rotN1 + rotN2 if r != 0], "MultiplyByDiagMatrixBSGS"
        for r in rots:
            self._key(rlwe.GaloisElement(N, r), levelP, who)

    # ---- Evaluate* (ckks/lintrans:147-194) ------------------------------------------------------------------------------------------------------
    def _new_out(self, ctIn, level):
        rq = self.ringQ.AtLevel(level)
        return Ciphertext([rq.NewPoly(ctIn.Value[0].npoly) for _ in (0, 1)], is_ntt=True)

    def Evaluate(self, ctIn, linearTransformation, opOut, fused=None):
        self.EvaluateMany(ctIn, [linearTransformation], [opOut], fused=fused)

    def EvaluateNew(self, ctIn, linearTransformation, fused=None):
        return self.EvaluateManyNew(ctIn, [linearTransformation], fused=fused)[0]

    def EvaluateManyNew(self, ctIn, linearTransformations, fused=None):
        opOut = [self._new_out(ctIn, lt.LevelQ) for lt in linearTransformations]
        self.EvaluateMany(ctIn, linearTransformations, opOut, fused=fused)
        return opOut

    def EvaluateSequentialNew(self, ctIn, linearTransformations, fused=None):
        opOut = self._new_out(ctIn, linearTransformations[0].LevelQ)
        self.EvaluateSequential(ctIn, linearTransformations, opOut, fused=fused)
        return opOut

    def EvaluateSequential(self, ctIn, linearTransformations, opOut, fused=None):
        """(:102-124): ... M2(M1(M0(ctIn))), a Rescale after each"""
        self.EvaluateMany(ctIn, linearTransformations[:1], [opOut], fused=fused)
        self._rescale(opOut)
        for lt in linearTransformations[1:]:
            self.EvaluateMany(opOut, [lt], [opOut], fused=fused)
            self._rescale(opOut)

    def _rescale(self, ct):
        """eval.Rescale(opOut, opOut) and the Resize it ends in: the blocks of the lower level"""
        nb = self.eval.nb_rescales
        self.eval.Rescale(ct, ct)
        self.eval._resize(ct, ct.Level() - nb)

    def EvaluateMany(self, ctIn, linearTransformations, opOut, fused=None):
        """(:18-68): opOut[i] = M_i(ctIn), the decomposition of ctIn[1] and the pre-rotated ciphertexts shared between the transformations.
        opOut[i] may be ctIn (the input is first brought to the evaluator's BuffCt, the reference's own CopyLvl, :165 / :281)."""
        lts = list(linearTransformations)
        if len(opOut) < len(lts):
            raise RingHipError("output *rlwe.Ciphertext slice is too small")
        for i in range(len(lts)):
            if opOut[i] is None:
                raise RingHipError("output slice contains unallocated ciphertext")
        if not lts:
            return
        levelQ, levelP = 0, lts[0].LevelP
        for lt in lts:
            levelQ = max(levelQ, lt.LevelQ)
            if levelP != lt.LevelP:
                raise RingHipError("all linearTransformations must have the same levelP")
        levelQ = min(levelQ, ctIn.Level())
        if ctIn.Degree() != 1:
            raise RingHipError("cannot EvaluateMany: ctIn.Degree() != 1")
        if not ctIn.IsNTT:
            raise RingHipError("cannot EvaluateMany: coefficient-domain ciphertexts are not supported by the device path")
        if not 0 <= levelP < self.ringP.L:
            raise RingHipError("cannot EvaluateMany: LevelP = %d out of range" % levelP)
        npoly = ctIn.Value[0].npoly
        self.ks._rows(ctIn.Level(), *ctIn.Value)
        for i, lt in enumerate(lts):
            out = opOut[i]
            if out.Degree() != 1 or out.Value[0].npoly != npoly or out.Value[1].npoly != npoly:
                raise RingHipError("cannot EvaluateMany: ctIn and opOut[%d] hold different numbers of ciphertexts" % i)
            if min(out.Level(), ctIn.Level(), lt.LevelQ) != levelQ:
                # the reference would read a decomposition made at levelQ at the lower level of this product (:141 / :266 against :39-43)
                raise RingHipError("cannot EvaluateMany: opOut[%d] and its transformation meet at level %d but the shared decomposition is made at level %d: "
                                   "evaluate transformations of different levels in calls of their own" % (i, min(out.Level(), ctIn.Level(), lt.LevelQ), levelQ))
            self._keys_of(lt, levelP)
        use = self._use(fused)
        rq = self.ringQ.AtLevel(levelQ)
        # ctIn at levelQ in BuffCt: device blocks are strided by level + 1 rows per poly, so everything below reads this dense copy
        ct = self._ct("BuffCt", levelQ, npoly)
        for c in (0, 1):
            rq.CopyLvl(ctIn.Value[c], ct.Value[c])
        meta = {name: getattr(ctIn, name) for name in rlwe.METADATA if hasattr(ctIn, name)}
        scaleIn = self._scale_in(ctIn)
        dec = self._dec(levelQ, levelP, npoly)
        self.ks.DecomposeNTT(levelQ, levelP, ct.Value[1], True, dec)                                   # (:43)
        ctPreRot = {}
        state = {"pct": None}
        for i, lt in enumerate(lts):
            out = opOut[i]
            for c in (0, 1):                                                                           # opOut.Resize(opOut.Degree(), levelQ)
                if out.Value[c].limbs != levelQ + 1:
                    out.Value[c] = rq.NewPoly(npoly)
            if lt.N1 == 0:
                self.MultiplyByDiagMatrix(ct, lt, dec, out, use=use)
            else:
                _, _, rotN2 = lt.BSGSIndex()
                self.PreRotatedCiphertextForDiagonalMatrixMultiplication(levelQ, levelP, ct, dec, rotN2, ctPreRot)
                self.MultiplyByDiagMatrixBSGS(ct, lt, ctPreRot, out, use=use, state=state)
            for name, v in meta.items():                                                               # *opOut.MetaData = *ctIn.MetaData
                setattr(out, name, v)
            out.IsNTT = True
            out.Scale = self._scale_out(scaleIn, lt)

    def PreRotatedCiphertextForDiagonalMatrixMultiplication(self, levelQ, levelP, ctIn, BuffDecompQP, rots, ctPreRot):
        """(:71-99): ctPreRot[i] = AutomorphismHoistedLazy(ctIn, 5^i) for every i of rots that is not there yet (0 excepted); entries that are not
        in rots are dropped.  The blocks are the evaluator's, one set per rotation: nothing is allocated after the first call of a shape."""
        npoly = ctIn.Value[0].npoly
        for i in [k for k in ctPreRot if k not in set(rots)]:
            del ctPreRot[i]
        for i in rots:
            if i != 0 and i not in ctPreRot:
                galEl = rlwe.GaloisElement(self.ringQ.N, i)
                evk = self._key(galEl, levelP, "PreRotatedCiphertextForDiagonalMatrixMultiplication")
                pre = self._qp("ltPre%d" % i, levelQ, levelP, npoly)
                try:
                    if self.ks.FUSED_INNER_SUM["accumulate"]:      # the tail of AutomorphismHoistedLazy in one launch (rh_rlwe_rotate_accumulate_qp, written: first)
                        tmp = self._qp("lazy", levelQ, levelP, npoly)
                        self.ks.GadgetProductHoistedLazy(levelQ, BuffDecompQP, evk, tmp)
                        self.ks.RotateAccumulateQP(levelQ, galEl, ctIn.Value[0], tmp, pre, True)
                    else:
                        self.ks.AutomorphismHoistedLazy(levelQ, ctIn, BuffDecompQP, galEl, pre)
                except RingHipError as e:
                    raise RingHipError("eval.AutomorphismHoistedLazy: %s" % e) from None
                ctPreRot[i] = pre

    # ---- MultiplyByDiagMatrix (:131-250) --------------------------------------------------------------------------------------------------------
    def MultiplyByDiagMatrix(self, ctIn, matrix, BuffDecompQP, opOut, use=None):
        """The naive form: one hoisted rotation and one multiplication per diagonal, one ModDown.  ctIn: a dense NTT-domain batch at the level of
        the product (EvaluateMany's BuffCt), opOut at that level too and not ctIn."""
        use = self._use(None) if use is None else use
        levelQ, levelP = ctIn.Level(), matrix.LevelP
        npoly = ctIn.Value[0].npoly
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        N = self.ringQ.N
        slots = matrix.Slots()
        keys = sorted(matrix.Vec)
        state = bool(keys) and keys[0] == 0
        if state:
            keys = keys[1:]
        acc = rlwe.ElementQP([rlwe.PolyQP(opOut.Value[c], self.ks.buffer("ltOutP%d" % c, rp, npoly, levelP + 1)) for c in (0, 1)])   # c0OutQP, c1OutQP
        cqp = self._qp("ltC", levelQ, levelP, npoly)
        L = lib()
        if keys and not use["naive_step"]:
            tmp = self._qp("ltTmp", levelQ, levelP, npoly)
            ct0P = self.ks.buffer("ltCt0P", rq, npoly, levelQ + 1)
            rq.MulScalarBigint(ctIn.Value[0], self._P(levelP), ct0P)                                   # P * c0 (:170)
        for i, k in enumerate(keys):
            galEl = rlwe.GaloisElement(N, k & (slots - 1))
            evk = self._key(galEl, levelP, "MultiplyByDiagMatrix")
            pt = matrix.Vec[k]
            self.ks.GadgetProductHoistedLazy(levelQ, BuffDecompQP, evk, cqp)                            # (:200)
            if use["naive_step"]:                                                                      # (:204-218) in one launch
                _check(L.rh_rlwe_rotate_mul_accumulate_qp(self.ks.be._h, levelQ, levelP, galEl, pt.Q.ptr, pt.P.ptr, ctIn.Value[0].ptr,
                                                          cqp.Value[0].Q.ptr, cqp.Value[1].Q.ptr, cqp.Value[0].P.ptr, cqp.Value[1].P.ptr,
                                                          acc.Value[0].Q.ptr, acc.Value[1].Q.ptr, acc.Value[0].P.ptr, acc.Value[1].P.ptr, npoly, 1 if i == 0 else 0))
                continue
            rq.Add(cqp.Value[0].Q, ct0P, cqp.Value[0].Q)                                                # (:204)
            for c in (0, 1):
                rq.AutomorphismNTT(cqp.Value[c].Q, galEl, tmp.Value[c].Q)                               # (:205-206)
                rp.AutomorphismNTT(cqp.Value[c].P, galEl, tmp.Value[c].P)
                self._mul_diag(rq, pt.Q, tmp.Value[c].Q, acc.Value[c].Q, i == 0)                        # (:210-218), canonical: the Reduce of :220-239
                self._mul_diag(rp, pt.P, tmp.Value[c].P, acc.Value[c].P, i == 0)
        if keys:
            self.ks.ModDown(levelQ, levelP, acc, Ciphertext(opOut.Value, is_ntt=True))                  # (:241-242)
        if state:                                                                                      # the rotation by zero (:244-247)
            for c in (0, 1):
                self._mul_diag(rq, matrix.Vec[0].Q, ctIn.Value[c], opOut.Value[c], not keys)

    @staticmethod
    def _mul_diag(ring, pt, x, out, first):
        """out (=|+=) pt * x * 2^-64 canonical, the one-poly diagonal against every poly of the batch: MulCoeffsMontgomery(ThenAdd) per poly"""
        for k in range(x.npoly):
            xa, oa = (x, out) if x.npoly == 1 else (_view(x, k), _view(out, k))
            (ring.MulCoeffsMontgomery if first else ring.MulCoeffsMontgomeryThenAdd)(pt, xa, oa)

    # ---- MultiplyByDiagMatrixBSGS (:256-433) ----------------------------------------------------------------------------------------------------
    def MultiplyByDiagMatrixBSGS(self, ctIn, matrix, ctInPreRot, opOut, use=None, state=None):
        """Double hoisting: per giant step the baby-step products summed modulo QP, one ModDown of component 1, a lazy key switch and a rotation
        modulo QP; one ModDown pair at the end.  ctIn / opOut as MultiplyByDiagMatrix takes them."""
        use = self._use(None) if use is None else use
        levelQ, levelP = ctIn.Level(), matrix.LevelP
        npoly = ctIn.Value[0].npoly
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        N = self.ringQ.N
        index, _, _ = matrix.BSGSIndex()
        state = {"pct": None} if state is None else state
        if state["pct"] is None:                                                                       # P * c0, P * c1 (:300-301), once per EvaluateMany
            pct = self._ct("ltPct", levelQ, npoly)
            for c in (0, 1):
                rq.MulScalarBigint(ctIn.Value[c], self._P(levelP), pct.Value[c])
            state["pct"] = pct
        pct = state["pct"]
        tmp = self._qp("ltTmp", levelQ, levelP, npoly)                                                 # tmp0QP, tmp1QP
        cqp = self._qp("ltC", levelQ, levelP, npoly)
        acc = rlwe.ElementQP([rlwe.PolyQP(opOut.Value[c], self.ks.buffer("ltOutP%d" % c, rp, npoly, levelP + 1)) for c in (0, 1)])   # c0OutQP, c1OutQP
        down = self.ks.buffer("ltDown", rq, npoly, levelQ + 1)
        L = lib()
        for cnt0, j in enumerate(sorted(index)):
            terms = [(matrix.Vec[j + i], None if i == 0 else ctInPreRot[i]) for i in index[j]]
            if use["diag_mac"]:
                self._diag_mac(levelQ, levelP, terms, pct, tmp, npoly)
            else:
                self._diag_mac_composed(rq, rp, terms, pct, tmp)
            if j != 0:
                self.ks.be.ModDownQPtoQNTT(levelQ, levelP, tmp.Value[1].Q, tmp.Value[1].P, down)        # (:363)
                galEl = rlwe.GaloisElement(N, j)
                evk = self._key(galEl, levelP, "MultiplyByDiagMatrixBSGS")
                self.ks.GadgetProductLazy(levelQ, down, evk, cqp)                                       # (:380)
                if use["giant_tail"]:                                                                  # (:384-393) in one launch
                    _check(L.rh_rlwe_rotate_sum_accumulate_qp(self.ks.be._h, levelQ, levelP, galEl, cqp.Value[0].Q.ptr, cqp.Value[1].Q.ptr,
                                                              cqp.Value[0].P.ptr, cqp.Value[1].P.ptr, tmp.Value[0].Q.ptr, tmp.Value[0].P.ptr,
                                                              acc.Value[0].Q.ptr, acc.Value[1].Q.ptr, acc.Value[0].P.ptr, acc.Value[1].P.ptr, npoly, 1 if cnt0 == 0 else 0))
                    continue
                rq.Add(cqp.Value[0].Q, tmp.Value[0].Q, cqp.Value[0].Q)                                  # ringQP.Add (:384)
                rp.Add(cqp.Value[0].P, tmp.Value[0].P, cqp.Value[0].P)
                for c in (0, 1):
                    if cnt0 == 0:                                                                      # (:387-389)
                        rq.AutomorphismNTT(cqp.Value[c].Q, galEl, acc.Value[c].Q)
                        rp.AutomorphismNTT(cqp.Value[c].P, galEl, acc.Value[c].P)
                    else:                                                                              # (:391-392) and the Reduce of :406-427
                        rq.AutomorphismNTT(cqp.Value[c].Q, galEl, tmp.Value[c].Q)
                        rp.AutomorphismNTT(cqp.Value[c].P, galEl, tmp.Value[c].P)
                        rq.Add(acc.Value[c].Q, tmp.Value[c].Q, acc.Value[c].Q)
                        rp.Add(acc.Value[c].P, tmp.Value[c].P, acc.Value[c].P)
            else:
                for c in (0, 1):
                    if cnt0 == 0:                                                                      # (:398-399)
                        rq.CopyLvl(tmp.Value[c].Q, acc.Value[c].Q)
                        rp.CopyLvl(tmp.Value[c].P, acc.Value[c].P)
                    else:                                                                              # (:401-402) and the Reduce of :406-427
                        rq.Add(acc.Value[c].Q, tmp.Value[c].Q, acc.Value[c].Q)
                        rp.Add(acc.Value[c].P, tmp.Value[c].P, acc.Value[c].P)
        self.ks.ModDown(levelQ, levelP, acc, Ciphertext(opOut.Value, is_ntt=True))                      # (:429-430)

    def _diag_mac(self, levelQ, levelP, terms, pct, tmp, npoly):
        """rh_rlwe_diag_mac_qp: the baby-step sum of one giant step in one launch; the term table is the evaluator's device scratch"""
        L = lib()
        K = len(terms)
        words = L.rh_rlwe_diag_mac_qp_table_words(K, levelQ, levelP)
        N = self.ringQ.N
        table = self.ks.buffer("ltTable", self.ringQ.AtLevel(0), max(1, -(-words // N)), 1)
        ptQ = (C.c_void_p * K)(*[pt.Q.ptr for pt, _ in terms])
        ptP = (C.c_void_p * K)(*[pt.P.ptr for pt, _ in terms])
        xs = []
        for _, x in terms:
            xs += [pct.Value[0].ptr, pct.Value[1].ptr, None, None] if x is None else [x.Value[0].Q.ptr, x.Value[1].Q.ptr, x.Value[0].P.ptr, x.Value[1].P.ptr]
        x = (C.c_void_p * (4 * K))(*xs)
        _check(L.rh_rlwe_diag_mac_qp(self.ks.be._h, levelQ, levelP, K, ptQ, ptP, x, tmp.Value[0].Q.ptr, tmp.Value[1].Q.ptr, tmp.Value[0].P.ptr,
                                     tmp.Value[1].P.ptr, npoly, table.ptr, table.words))

    def _diag_mac_composed(self, rq, rp, terms, pct, tmp):
        """(:311-357) through the ring's own calls, canonical at every step (the Reduce of :349-357)"""
        zero = [0] * (rp.level + 1)
        for cnt1, (pt, x) in enumerate(terms):
            for c in (0, 1):
                if x is None:                                                                          # the baby step 0 term lives modulo Q (:316-325)
                    self._mul_diag(rq, pt.Q, pct.Value[c], tmp.Value[c].Q, cnt1 == 0)
                    if cnt1 == 0:
                        rp.vec_op("MUL_SCALAR_MONT", tmp.Value[c].P, None, tmp.Value[c].P, s0=zero)    # tmpQP.P.Zero() (:320-321)
                else:
                    self._mul_diag(rq, pt.Q, x.Value[c].Q, tmp.Value[c].Q, cnt1 == 0)
                    self._mul_diag(rp, pt.P, x.Value[c].P, tmp.Value[c].P, cnt1 == 0)

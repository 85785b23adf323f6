"""Homomorphic linear transformations for BFV / BGV on device batches: circuits/bgv/lintrans/lintrans.go over circuits/common/lintrans.

  Diagonals: DiagonalsIndexList :17-19, At (common/lintrans :97-122), Evaluate :24-58       PermutationMapping :62-66, Permutation :75,
  GetDiagonals :80-107        Parameters :110       LinearTransformation :113, GaloisElements :116-118       NewLinearTransformation :121-123
  Encode :126-131 (common/lintrans Encode :205-292 with rows = 2)       Evaluator, NewEvaluator :135-147, Evaluate* :150-196

A BGV plaintext is a 2 x n/2 matrix of slots modulo T whose rows rotate independently (RotateColumns): LogDimensions is (Rows, Cols) = (1,
log2(n) - 1) as bgv.Encoder.LogMaxDimensions() returns it, a diagonal holds 2 * cols values -- row 0 then row 1 -- and every rotation acts on
each row of cols values.  Scales are integers modulo T.

What does not depend on the scheme is lintrans.py's and is used from there, not copied: BSGSIndex, FindBestBSGSRatio, GaloisElements, the keys
of Vec and the walk of Encode with its refusals, and the whole Evaluator -- EvaluateMany, the hoisted pre-rotations, MultiplyByDiagMatrix(BSGS)
with their three kernels and the same `fused` selection per pass.  The Evaluator below overrides the scheme's points only: the scale of the
input, opOut.Scale = ctIn.Scale * lt.Scale mod T, the rescale of EvaluateSequential (bgv.Evaluator.Rescale into blocks of the lower level), and
through LinearTransformation.Slots the row length 1 << Cols.

The encoding of a transformation is ONE pass over all its diagonals (bgv.Encoder.EmbedRows, rh_bgv_embed_qp: the row rotation folded into the
slot gather, one inverse transform over T, one lift onto the rows of Q and of P) or, with FUSED_BGV_LINTRANS["encode"] False, the reference's
per-diagonal rotate-then-Embed.  The bits are the same.

Refused by name, as the CKKS evaluator refuses them: conjugate-invariant and 3N rings, coefficient-domain ciphertexts, an evaluator without
ringP, keys with BaseTwoDecomposition != 0 or a single P modulus, differing batch sizes, transformations of different LevelP in one call."""
import numpy as np

from . import bgv, lintrans as _lt, rlwe
from .lintrans import BSGSIndex, FindBestBSGSRatio, GaloisElements, _rings_at, _vec_keys, _view  # noqa: F401
from .ringhip import DevicePoly, RingHipError

# The encoding of a transformation as one EmbedRows (True) or as the reference's per-diagonal rotate-then-Embed (False): the same bits.  The
# default is the one the measurement supports (tools/bench_bgv_lintrans.py -> profiles/bgv_lintrans.json, "fused_bgv_lintrans_default";
# DESIGN.md): fused only if at EVERY shape timed the windows of the fused encode lie below the windows of the per-diagonal one.  They do: 9 and
# 64 diagonals at N = 2^13 and 2^15, BSGS and naive, from host arrays, 6.6 to 28 times faster (0.11 | 1.03 ms to 0.27 | 7.34 ms at N = 2^13,
# 0.16 | 1.09 ms to 0.89 | 7.77 ms at N = 2^15), no window of one side within the other's.
FUSED_BGV_LINTRANS = {"encode": True}


def _fused_encode(fused):
    if fused is None:
        return bool(FUSED_BGV_LINTRANS["encode"])
    if isinstance(fused, dict):
        return bool(fused.get("encode", FUSED_BGV_LINTRANS["encode"]))
    return bool(fused)


def _rotate_rows(v, rot, cols):
    """utils.RotateSliceAllocFree on each row of cols values (common/lintrans :283-285): to the left by rot"""
    rot &= cols - 1
    if isinstance(v, np.ndarray):
        return v if rot == 0 else np.roll(v.reshape(-1, cols), -rot, axis=1).reshape(-1)
    v = list(v)
    if rot == 0:
        return v
    return [v[r * cols + ((c + rot) & (cols - 1))] for r in range(len(v) // cols) for c in range(cols)]


class Diagonals(_lt.Diagonals):
    """bgv lintrans.Diagonals (:13): diagonal index -> 2 * cols values, row 0 then row 1.  DiagonalsIndexList and At are the common ones."""

    def Evaluate(self, vector, newVec=None, add=None, muladd=None, t=None):
        """(:24-58): the transformation on a plain vector of 2 * slots values, the BSGS schedule of ratio 1 on each half separately.  Without
        the callbacks: exact Python integers, reduced modulo t when one is given"""
        slots = len(vector) >> 1                                                          # 2 x n/2 matrix (:26)
        newVec = newVec or (lambda size: [0] * size)
        red = (lambda x: x % t) if t else (lambda x: x)
        if add is None:
            def add(a, b, c):
                return [red(x + y) for x, y in zip(a, b)]
        if muladd is None:
            def muladd(a, b, c):
                return [red(z + x * y) for x, y, z in zip(a, b, c)]
        rotate = lambda v, k: [v[(i + k) % len(v)] for i in range(len(v))]                # utils.RotateSlice: to the left
        vector = list(vector)
        keys = list(self.keys())
        N1 = FindBestBSGSRatio(keys, slots, 1)
        index, _, _ = BSGSIndex(keys, slots, N1)
        res = list(newVec(2 * slots))
        halves = (slice(0, slots), slice(slots, 2 * slots))
        for j in index:
            rot = -j & (slots - 1)
            tmp = list(newVec(2 * slots))
            for i in index[j]:
                v = list(self[j + i] if j + i in self else self[j + i - slots])
                for h in halves:                                                          # (:49-50)
                    out = tmp[h]
                    r = muladd(rotate(vector[h], i), rotate(v[h], rot), out)
                    tmp[h] = out if r is None else r
            for h in halves:                                                              # (:53-54)
                out = res[h]
                r = add(res[h], rotate(tmp[h], j), out)
                res[h] = out if r is None else r
        return res


class PermutationMapping:
    """(:62-66)"""

    def __init__(self, From, To, Scaling):
        self.From, self.To, self.Scaling = int(From), int(To), Scaling


class Permutation(list):
    """(:75): [2][]PermutationMapping, one list per row of the 2 x n/2 matrix, each row permuted on its own"""

    def __init__(self, rows=((), ())):
        rows = [list(r) for r in rows]
        if len(rows) != 2:
            raise RingHipError("a BGV Permutation is a pair of lists of PermutationMapping, one per row, but has %d" % len(rows))
        list.__init__(self, rows)

    def GetDiagonals(self, logSlots):
        """(:80-107)"""
        slots = 1 << (logSlots - 1)                                                       # matrix of 2 x 2^{logSlots - 1}
        diagonals = Diagonals()
        for i, row in enumerate(self):
            offset = i * slots
            for pm in row:
                diagIndex = (slots + pm.From - pm.To) & (slots - 1)
                if diagIndex not in diagonals:
                    diagonals[diagIndex] = [0] * (2 * slots)
                diagonals[diagIndex][pm.To + offset] = pm.Scaling
        return diagonals


class Parameters:
    """bgv lintrans.Parameters (:110, common/lintrans :51-81).  LogDimensions: (Rows, Cols) as bgv.Encoder.LogMaxDimensions() returns it;
    Scale: an integer modulo T"""

    def __init__(self, DiagonalsIndexList, LevelQ, LevelP, Scale, LogDimensions, LogBabyStepGiantStepRatio=0):
        self.DiagonalsIndexList = [int(i) for i in DiagonalsIndexList]
        self.LevelQ, self.LevelP = int(LevelQ), int(LevelP)
        self.Scale = int(Scale)
        self.LogDimensions = _dims(LogDimensions)
        self.LogBabyStepGiantStepRatio = int(LogBabyStepGiantStepRatio)

    def GaloisElements(self, N):
        """GaloisElements(params, lt) on the parameters (common/lintrans :84-86)"""
        return GaloisElements(N, self.DiagonalsIndexList, 1 << self.LogDimensions[1], self.LogBabyStepGiantStepRatio)


def _dims(LogDimensions):
    try:
        rows, cols = LogDimensions
    except TypeError:
        raise RingHipError("LogDimensions of a BGV linear transformation is (Rows, Cols), as bgv.Encoder.LogMaxDimensions() returns it, but is %r"
                           % (LogDimensions,)) from None
    if int(rows) != 1:
        raise RingHipError("LogDimensions.Rows = %d: a BGV plaintext on a standard ring has two rows (LogDimensions.Rows = 1)" % int(rows))
    return (1, int(cols))


class LinearTransformation(_lt.LinearTransformation):
    """bgv lintrans.LinearTransformation (:113): the common one with LogDimensions = (Rows, Cols) and an integer Scale.  Vec maps a diagonal
    index to a one-poly rlwe.PolyQP view of Block, ONE contiguous rlwe.PolyQP whose poly k is the diagonal Keys[k]."""

    def __init__(self, LogBabyStepGiantStepRatio, N1, LevelQ, LevelP, Block, Keys, Scale, LogDimensions):
        vec = {k: rlwe.PolyQP(_view(Block.Q, row), _view(Block.P, row)) for row, k in enumerate(Keys)}
        _lt.LinearTransformation.__init__(self, LogBabyStepGiantStepRatio, N1, LevelQ, LevelP, vec, int(Scale), _dims(LogDimensions))
        self.Block, self.Keys = Block, list(Keys)

    def Slots(self):
        return 1 << self.LogDimensions[1]

    def GaloisElements(self, N):
        """(:116-118)"""
        return _lt.LinearTransformation.GaloisElements(self, N)


def _allocate(ringQ, ringP, ltparams, keys, N1):
    levelQ, levelP = ltparams.LevelQ, ltparams.LevelP
    rq, rp = _rings_at(ringQ, ringP, levelQ, levelP)
    keys = list(dict.fromkeys(keys))
    block = rlwe.PolyQP(DevicePoly(rq, len(keys), levelQ + 1), DevicePoly(rp, len(keys), levelP + 1))
    return LinearTransformation(ltparams.LogBabyStepGiantStepRatio, N1, levelQ, levelP, block, keys, ltparams.Scale, ltparams.LogDimensions)


def NewLinearTransformation(ringQ, ringP, ltparams):
    """(:121-123, common/lintrans :148-201): the diagonals allocated (not zeroed: Encode writes every one it is given) at (LevelQ, LevelP), as
    one contiguous block"""
    N1, keys = _vec_keys(ltparams.DiagonalsIndexList, 1 << ltparams.LogDimensions[1], ltparams.LogBabyStepGiantStepRatio)
    return _allocate(ringQ, ringP, ltparams, keys, N1)


def _values(encoder, rows):
    """the diagonals as ONE (D, n) array of uint64 or int64; mixed or wider integer types are brought to their residues modulo T on the host,
    which is the word both value rules of the encoder produce"""
    arrs = [np.asarray(r) for r in rows]
    kinds = {a.dtype for a in arrs}
    if len(kinds) == 1 and arrs[0].dtype in (np.uint64, np.int64):
        return np.stack(arrs)
    return np.array([[int(x) % encoder.t for x in r] for r in rows], dtype=np.uint64).reshape(len(rows), -1)


def _one(encoder, v):
    a = np.asarray(v)
    return a if a.dtype in (np.uint64, np.int64) else np.array([int(x) % encoder.t for x in v], dtype=np.uint64)


def _encode_rows(encoder, lt, keys, rows, rots, fused):
    """rows[k] (host values, 2 * cols each) rotated by rots[k] onto lt.Vec[keys[k]]"""
    cols = lt.Slots()
    for r in rows:
        if len(r) != 2 * cols:
            raise RingHipError("cannot Encode: a diagonal of a BGV linear transformation holds 2 * cols = %d values, but has %d" % (2 * cols, len(r)))
    if not _fused_encode(fused):                                                          # rotateAndEncodeDiagonal (common/lintrans :271-292), rows = 2
        for k, v, rot in zip(keys, rows, rots):
            encoder.Embed(_one(encoder, _rotate_rows(v, rot, cols)), lt, lt.Vec[k])
        return
    if list(keys) == lt.Keys:                                                             # the whole transformation: one pass over its block
        encoder.EmbedRows(_values(encoder, rows), rots, cols, lt, lt.Block)
        return
    for k, v, rot in zip(keys, rows, rots):                                               # some of its diagonals: one pass each
        encoder.EmbedRows(_values(encoder, [v]), [rot], cols, lt, lt.Vec[k])


def Encode(encoder, diagonals, allocated, fused=None):
    """(:126-131, common/lintrans :205-292 with rows = 2): every diagonal of `diagonals` onto the allocated transformation; with BSGS each row
    of the values of giant step j is rotated by -j first (:246-262, :283-285).  metaData.Scale is the transformation's (:217)."""
    walk = list(_lt._encode_walk(diagonals, allocated))
    by_key = {idx: (v, rot) for v, rot, idx in walk}
    keys = [k for k in allocated.Keys if k in by_key] if len(by_key) == len(allocated.Keys) else [idx for _, _, idx in walk]
    _encode_rows(encoder, allocated, keys, [by_key[k][0] for k in keys], [by_key[k][1] for k in keys], fused)


def NewTransformationFromBlock(ringQ, ringP, ltparams, encoder, index, block, fused=None):
    """NewLinearTransformation and Encode in the block form: row k of `block` -- a (len(index), 2 * cols) array of uint64 / int64 or a
    bgv.DeviceValues -- holds diagonal index[k] of ltparams.DiagonalsIndexList, NOT rotated: the rotations of Encode (:246-262) are applied by
    the encoder."""
    cols = 1 << ltparams.LogDimensions[1]
    index = [int(i) for i in index]
    if sorted(i & (cols - 1) for i in ltparams.DiagonalsIndexList) != sorted(index) or len(set(index)) != len(index):
        raise RingHipError("cannot NewTransformation: the block's rows are not the diagonals of DiagonalsIndexList")
    shape = (block.nvec, block.n) if isinstance(block, bgv.DeviceValues) else np.asarray(block).shape
    if tuple(shape) != (len(index), 2 * cols):
        raise RingHipError("cannot NewTransformation: the block must be uint64 or int64 of shape (%d, %d)" % (len(index), 2 * cols))
    N1 = 0 if ltparams.LogBabyStepGiantStepRatio < 0 else FindBestBSGSRatio(index, cols, ltparams.LogBabyStepGiantStepRatio)
    lt = _allocate(ringQ, ringP, ltparams, index, N1)
    rots = [0 if N1 == 0 else -(((k // N1) * N1) & (cols - 1)) & (cols - 1) for k in index]          # rot = -j of the giant step j (BSGSIndex :351)
    if _fused_encode(fused):
        encoder.EmbedRows(block, rots, cols, lt, lt.Block)
    else:
        host = block.numpy() if isinstance(block, bgv.DeviceValues) else np.asarray(block)
        _encode_rows(encoder, lt, index, [host[k] for k in range(len(index))], rots, False)
    return lt


class Evaluator(_lt.Evaluator):
    """bgv lintrans.Evaluator over a bgv.Evaluator (NewEvaluator :141-147), on batches of ciphertexts that share the transformation: the
    methods, passes and `fused` selection of lintrans.Evaluator, with BGV's scales and rescale"""

    @staticmethod
    def _ks_of(eval):
        return eval if eval.ringP is not None else None

    def _scale_in(self, ctIn):
        return int(getattr(ctIn, "Scale", 1)) % self.eval.t

    def _scale_out(self, scaleIn, lt):
        """opOut.Scale = opOut.Scale.Mul(matrix.Scale) (common/lintrans_evaluator.go:137, :264) on bgv scales: the product modulo T"""
        return scaleIn * (int(lt.Scale) % self.eval.t) % self.eval.t

    def _rescale(self, ct):
        """eval.Rescale(opOut, opOut) (:113, :120): bgv.Evaluator.Rescale and the resize to the blocks of the lower level"""
        if self.eval.ScaleInvariant:
            return
        out = self.eval.RescaleNew(ct)
        ct.Value, ct.Scale = out.Value, out.Scale

"""Homomorphic DFT for CKKS on device batches: circuits/ckks/dft/dft.go.

  MatrixLiteral :73-85     Depth :90-99     GaloisElements :102-127     MarshalBinary / UnmarshalBinary :131-139
  NewMatrixFromLiteral :159-215     CoeffsToSlots(New) :222-300     SlotsToCoeffs(New) :306-342     dft :345-360
  fftPlainVec / ifftPlainVec :362-490     addMatrixRotToList :492-527     computeBootstrappingDFTIndexMap :529-597
  genWfftIndexMap, genWfftRepackIndexMap, nextLevelfftIndexMap :599-642     GenMatrices :644-773
  genFFTDiagMatrix, genRepackMatrix, multiplyFFTMatrixWithNextFFTLevel :775-862

The float64 path on standard rings.  GenMatrices builds every factor's diagonals in HBM as one (ndiag, dslots) complex128 block (csrc/dft.hip:
rh_ckks_dft_level_vectors, rh_ckks_dft_merge_level, rh_ckks_dft_finish), NewMatrixFromLiteral encodes a whole factor with ONE Encoder.Embed into
one contiguous rlwe.PolyQP whose polys the LinearTransformation's diagonals are views of, and the real / imaginary split and merge around the
transformations are one launch each (csrc/ckks.hip: rh_ckks_split_real_imag, rh_ckks_merge_real_imag) or the reference's Sub / Mul / Add calls.

Three things are GIVEN rather than computed as a Go run computes them:
  the roots table   GetRootsComplex128(4 slots), libm's cosine; a Go caller passes its own (roots=)
  scaling           (Scaling or 1) / (2 slots or slots), to the power 1 / Depth(false): float64 pow here, bignum.Pow at 53 bits there
  addition order    the reference adds the contributions to a diagonal in the order of a Go map; here: ascending source diagonal, and per source
                    a, b, c.  A diagonal with more than two contributions may differ from a Go run in its last bit.

Not built: mod1 and the bootstrapping evaluator, the *big.Float / *bignum.Complex path (encoder precision above 53), PREC128
(LevelsConsumedPerRescaling = 2), conjugate-invariant and 3N rings."""
import ctypes as C
import json
import math
from fractions import Fraction

import numpy as np

from . import lintrans
from .ckks import DeviceValues, GaloisElement, GetRootsComplex128, Scale, ScalePrecision, _round
from .ringhip import RingHipError, Standard as _StandardRing, _check, _p, _u64, lib
from .schemes import Ciphertext

# Type
HomomorphicEncode, HomomorphicDecode = 0, 1
# Format
Standard, SplitRealAndImag, RepackImagAsReal = 0, 1, 2


# ---- index maps (:492-642) ---------------------------------------------------------------------------------------------------------------------
def _by_level_rot(logL, level, ltType, bitreversed):
    """the rotation of one FFT level: 2^(level-1) for an encode in natural order or a decode in bit-reversed order, else 2^(logL-level)"""
    if (ltType == HomomorphicEncode and not bitreversed) or (ltType == HomomorphicDecode and bitreversed):
        return 1 << (level - 1)
    return 1 << (logL - level)


def genWfftIndexMap(logL, level, ltType, bitreversed):
    rot = _by_level_rot(logL, level, ltType, bitreversed)
    return {0: True, rot: True, (1 << logL) - rot: True}


def genWfftRepackIndexMap(logL, level):
    return {0: True, 1 << logL: True}


def nextLevelfftIndexMap(vec, logL, N, nextLevel, ltType, bitreversed):
    rot = _by_level_rot(logL, nextLevel, ltType, bitreversed) & (N - 1)
    newVec = {}
    for i in vec:
        newVec[i] = True
        newVec[(i + rot) & (N - 1)] = True
        newVec[(i - rot) & (N - 1)] = True
    return newVec


def addMatrixRotToList(pVec, rotations, N1, slots, repack):
    if len(pVec) < 3:
        for j in pVec:
            if j not in rotations:
                rotations.append(j)
    else:
        for j in pVec:
            index = (j // N1) * N1
            index &= (2 * slots - 1) if repack else (slots - 1)
            if index != 0 and index not in rotations:
                rotations.append(index)
            index = j & (N1 - 1)
            if index != 0 and index not in rotations:
                rotations.append(index)
    return rotations


def _iroot(n, k):
    """floor of the k-th root of the integer n >= 0"""
    if n < 2:
        return n
    x = 1 << -(-n.bit_length() // k)
    while True:
        y = ((k - 1) * x + n // x ** (k - 1)) // k
        if y >= x:
            return x
        x = y


def ScaleRoot(scale, k):
    """The k-th root of a Scale whose value is an integer (a modulus), correctly rounded to ScalePrecision bits, half to even.  The reference
    takes it with bignum.Pow at 128 bits, which is not specified to the last bit: the last bit of the 128-bit Scale may differ from a Go run;
    Scale.Float64(), what the encoder sees, does not."""
    v = Scale(scale).Value
    if v.denominator != 1:
        raise RingHipError("cannot ScaleRoot: the scale %s is not an integer" % v)
    n, k = int(v), int(k)
    if k == 1:
        return Scale(n)
    t = ScalePrecision + 2                                               # R = floor(root * 2^t) has more than ScalePrecision + 2 bits
    R = _iroot(n << (k * t), k)
    sticky = 0 if R ** k == n << (k * t) else 1
    return Scale(_round(Fraction(2 * R + sticky, 1 << (t + 1)), ScalePrecision))


class MatrixLiteral:
    """dft.MatrixLiteral (:73-85).  Scaling: None (1.0), or a number (a *big.Float of the reference; a decimal string in the JSON form)"""

    def __init__(self, Type, LogSlots, LevelQ, LevelP, Levels, Format=Standard, Scaling=None, BitReversed=False, LogBSGSRatio=0):
        self.Type, self.LogSlots, self.LevelQ, self.LevelP = int(Type), int(LogSlots), int(LevelQ), int(LevelP)
        self.Levels = [int(x) for x in Levels]
        self.Format, self.Scaling, self.BitReversed, self.LogBSGSRatio = int(Format), Scaling, bool(BitReversed), int(LogBSGSRatio)

    def Depth(self, actual):
        return len(self.Levels) if actual else sum(self.Levels)

    # ---- :529-597 ----
    def _merge(self):
        """how many FFT levels each factor collapses (:547-560 / :684-697)"""
        maxDepth = self.Depth(False)
        level = self.LogSlots
        merge = [0] * maxDepth
        for i in range(maxDepth):
            depth = int(math.ceil(float(level) / float(maxDepth - i)))
            if self.Type == HomomorphicEncode:
                merge[i] = depth
            else:
                merge[len(merge) - i - 1] = depth
            level -= depth
        return merge

    def computeBootstrappingDFTIndexMap(self, logN):
        logSlots, ltType, bitreversed = self.LogSlots, self.Type, self.BitReversed
        repacki2r = self.Format == RepackImagAsReal
        maxDepth = self.Depth(False)
        merge = self._merge()
        rotationMap = [None] * maxDepth
        level = logSlots
        for i in range(maxDepth):
            if logSlots < logN - 1 and ltType == HomomorphicDecode and i == 0 and repacki2r:
                m = genWfftRepackIndexMap(logSlots, level)
                m = nextLevelfftIndexMap(m, logSlots, 2 << logSlots, level, ltType, bitreversed)
                nextLevel = level - 1
                for _ in range(merge[i] - 1):
                    m = nextLevelfftIndexMap(m, logSlots, 2 << logSlots, nextLevel, ltType, bitreversed)
                    nextLevel -= 1
            else:
                m = genWfftIndexMap(logSlots, level, ltType, bitreversed)
                nextLevel = level - 1
                for _ in range(merge[i] - 1):
                    m = nextLevelfftIndexMap(m, logSlots, 1 << logSlots, nextLevel, ltType, bitreversed)
                    nextLevel -= 1
            rotationMap[i] = m
            level -= merge[i]
        return rotationMap

    def GaloisElements(self, N):
        """(:102-127) on a standard ring of degree N; the reference's order is that of Go maps, here: sorted index maps"""
        logN = int(N).bit_length() - 1
        rotations = []
        imgRepack = self.Format == RepackImagAsReal
        logSlots = self.LogSlots
        slots = 1 << logSlots
        dslots = slots
        if logSlots < logN - 1 and imgRepack:
            dslots <<= 1
            if self.Type == HomomorphicEncode:
                rotations.append(slots)
        for i, pVec in enumerate(self.computeBootstrappingDFTIndexMap(logN)):
            keys = sorted(pVec)
            N1 = lintrans.FindBestBSGSRatio(keys, dslots, self.LogBSGSRatio)
            rotations = addMatrixRotToList(keys, rotations, N1, slots, self.Type == HomomorphicDecode and logSlots < logN - 1 and i == 0 and imgRepack)
        return [GaloisElement(N, r) for r in rotations]

    # ---- :131-139 ----
    def MarshalBinary(self):
        """json.Marshal of the struct: the fields in declaration order, Scaling null or a *big.Float's text (a JSON string)"""
        d = {"Type": self.Type, "LogSlots": self.LogSlots, "LevelQ": self.LevelQ, "LevelP": self.LevelP, "Levels": self.Levels, "Format": self.Format,
             "Scaling": None if self.Scaling is None else _float_text(self.Scaling), "BitReversed": self.BitReversed, "LogBSGSRatio": self.LogBSGSRatio}
        return json.dumps(d, separators=(",", ":")).encode()

    @classmethod
    def UnmarshalBinary(cls, data):
        d = json.loads(data.decode() if isinstance(data, (bytes, bytearray)) else data)
        s = d.get("Scaling")
        return cls(d["Type"], d["LogSlots"], d["LevelQ"], d["LevelP"], d["Levels"] or [], d.get("Format", 0), None if s is None else float(s),
                   d.get("BitReversed", False), d.get("LogBSGSRatio", 0))

    def __eq__(self, other):
        return isinstance(other, MatrixLiteral) and self.__dict__ == other.__dict__

    __hash__ = None

    # ---- GenMatrices (:644-773) ----
    def _scaling(self):
        """the real factor every diagonal is multiplied by: float64 arithmetic and pow (the reference: bignum.Pow at the encoder's precision)"""
        slots = 1 << self.LogSlots
        scaling = 1.0 if self.Scaling is None else float(self.Scaling)
        if self.Type == HomomorphicEncode:
            scaling = scaling / (float(2 * slots) if self.Format in (RepackImagAsReal, SplitRealAndImag) else float(slots))
        return math.pow(scaling, 1.0 / float(self.Depth(False)))

    def _plan(self, LogN):
        """The factors as a list of merge steps: per factor (steps, zero_upper); a step is (fft_level, rot, program, out_index, first) where program
        lists per output diagonal its contributions (source ROW or -1, kind) in the order they are added: ascending source diagonal, then a, b, c;
        first: 'repack' (the source is genRepackMatrix), 'level' (genFFTDiagMatrix: no source) or None (the factor so far)."""
        logSlots, ltType, bitreversed = self.LogSlots, self.Type, self.BitReversed
        slots = 1 << logSlots
        maxDepth = self.Depth(False)
        logdSlots = logSlots + 1 if logSlots < LogN - 1 and self.Format == RepackImagAsReal else logSlots
        merge = self._merge()
        factors = []
        fftLevel = logSlots
        for i in range(maxDepth):
            steps = []
            if logSlots != logdSlots and ltType == HomomorphicDecode and i == 0:
                index, Nmod, todo, first = [0, slots], 2 * slots, [fftLevel] + [fftLevel - 1 - j for j in range(merge[i] - 1)], "repack"
            else:
                rot = _by_level_rot(logSlots, fftLevel, ltType, bitreversed)
                prog = {}
                for d, kind in ((0, 0), (rot, 1), (slots - rot, 2)):                     # addToDiagMatrix in the order of :799-801
                    prog.setdefault(d, []).append((-1, kind))
                index = sorted(prog)
                steps.append((fftLevel, 0, [prog[d] for d in index], index, "level"))
                Nmod, todo, first = slots, [fftLevel - 1 - j for j in range(merge[i] - 1)], None
            for lvl in todo:
                rot = _by_level_rot(logSlots, lvl, ltType, bitreversed) & (Nmod - 1)
                prog = {}
                for row, s in enumerate(index):                                        # ascending source diagonal; per source a, b, c
                    for d, kind in ((s, 0), ((s + rot) & (Nmod - 1), 1), ((s - rot) & (Nmod - 1), 2)):
                        prog.setdefault(d, []).append((row, kind))
                index = sorted(prog)
                steps.append((lvl, rot, [prog[d] for d in index], index, first))
                first = None
            factors.append((steps, False))
            fftLevel -= merge[i]
        if logSlots != logdSlots and ltType == HomomorphicEncode:
            factors[-1] = (factors[-1][0], True)
        return factors, logdSlots

    def _tables(self, roots):
        slots = 1 << self.LogSlots
        roots = GetRootsComplex128(slots << 2) if roots is None else np.ascontiguousarray(roots, dtype=np.float64).reshape(-1, 2)
        if roots.shape[0] != 4 * slots + 1:
            raise RingHipError("cannot GenMatrices: %d roots given, 4 slots + 1 = %d expected" % (roots.shape[0], 4 * slots + 1))
        pow5 = np.ones((slots << 1) + 1, dtype=np.uint64)
        for i in range(1, pow5.size):
            pow5[i] = (int(pow5[i - 1]) * 5) & ((slots << 2) - 1)
        return roots, pow5

    def GenMatrices(self, LogN, roots=None, ring=None, device=None):
        """The factors in order, each a lintrans.Diagonals (device=False: numpy rows, the same rules on the host) or a DeviceDiagonals
        (device=True, the default when a ring is given: one (ndiag, dslots) complex128 block in HBM).  roots: GetRootsComplex128(4 slots) or
        the caller's own table."""
        self._check(LogN)
        device = ring is not None if device is None else bool(device)
        if device:
            if ring is None:
                raise RingHipError("cannot GenMatrices: device=True needs a ring (its device and stream)")
            return _gen_device(self, LogN, roots, ring, None)
        return _gen_host(self, LogN, roots)

    def _check(self, LogN):
        if not 1 <= self.LogSlots <= LogN - 1:
            raise RingHipError("cannot GenMatrices: LogSlots = %d outside [1, LogN - 1 = %d]" % (self.LogSlots, LogN - 1))
        if not self.Levels or min(self.Levels) < 1:
            raise RingHipError("cannot GenMatrices: Levels must be a non-empty list of positive depths, got %s" % (self.Levels,))
        if self.Depth(False) > self.LogSlots:
            raise RingHipError("cannot GenMatrices: Depth(false) = %d exceeds the %d FFT levels of LogSlots" % (self.Depth(False), self.LogSlots))
        if self.Type not in (HomomorphicEncode, HomomorphicDecode) or self.Format not in (Standard, SplitRealAndImag, RepackImagAsReal):
            raise RingHipError("cannot GenMatrices: unknown Type %d or Format %d" % (self.Type, self.Format))


def _float_text(x):
    """big.Float.MarshalText of a float64-valued *big.Float: the shortest decimal that reads back to it ('g' format, as Go writes it)"""
    from decimal import Decimal
    x = float(x)
    if x == 0:
        return "0"
    sign, digits, exp = Decimal(repr(x)).as_tuple()
    digits = "".join(map(str, digits)).rstrip("0") or "0"
    dp = len(Decimal(repr(x)).as_tuple().digits) + exp                   # the decimal point sits after dp digits
    e = dp - 1
    if e < -4 or e >= 6:                                                 # %e: the shortest form's eprec is 6 (math/big/ftoa.go)
        body = digits[0] + ("." + digits[1:] if len(digits) > 1 else "") + "e%s%02d" % ("-" if e < 0 else "+", abs(e))
    elif dp <= 0:
        body = "0." + "0" * -dp + digits
    else:
        body = digits[:dp].ljust(dp, "0") + ("." + digits[dp:] if len(digits) > dp else "")
    return ("-" if sign else "") + body


# ---- GenMatrices on the host: the rules of the kernels in numpy, real and imaginary parts as separate float64 arrays ----------------------------
def _level_vectors_host(d, logdSlots, fft_level, roots, pow5):
    logSlots = d.LogSlots
    slots, dslots = 1 << logSlots, 1 << logdSlots
    decode = d.Type == HomomorphicDecode
    logm = logSlots - fft_level + 1 if decode else fft_level
    m, tt = 1 << logm, 1 << (logm - 1)
    x = np.arange(dslots)
    p = x & (slots - 1)
    if d.BitReversed:
        p = np.array([int(format(int(v), "0%db" % logSlots)[::-1], 2) for v in p])
    jj = p & (m - 1)
    j = jj & (tt - 1)
    r = pow5[j].astype(np.int64) & ((m << 2) - 1)
    k = (r if decode else (m << 2) - r) * (slots >> logm)
    w = roots[k]
    upper = (jj < tt)[:, None]
    one, zero = np.broadcast_to(roots[0], w.shape), np.zeros_like(w)
    a = np.where(upper, one, -w)
    b = np.where(upper, w if decode else one, zero)
    c = np.where(upper, zero, one if decode else w)
    return a, b, c                                                       # each (dslots, 2): re, im


def _gen_host(d, LogN, roots):
    roots, pow5 = d._tables(roots)
    factors, logdSlots = d._plan(LogN)
    dslots = 1 << logdSlots
    slots = 1 << d.LogSlots
    scaling = d._scaling()
    out = []
    for steps, zero_upper in factors:
        cur = None
        for lvl, rot, prog, index, first in steps:
            abc = _level_vectors_host(d, logdSlots, lvl, roots, pow5)
            if first == "repack":
                cur = _repack_host(slots)
            new = np.empty((len(index), dslots, 2))
            x = np.arange(dslots)
            for row, terms in enumerate(prog):
                acc = None
                for src, kind in terms:
                    v = abc[kind]
                    if src >= 0:
                        s = cur[src][(x + (0, rot, -rot)[kind]) & (dslots - 1)]
                        v = np.stack([v[:, 0] * s[:, 0] - v[:, 1] * s[:, 1], v[:, 0] * s[:, 1] + v[:, 1] * s[:, 0]], axis=1)
                    acc = v.copy() if acc is None else acc + v
                new[row] = acc
            cur = new
        if zero_upper:
            cur[:, slots:] = 0.0
        cur = cur * scaling
        out.append(lintrans.Diagonals({k: np.ascontiguousarray(cur[row]).view(np.complex128).reshape(-1) for row, k in enumerate(index)}))
    return out


def _repack_host(slots):
    """genRepackMatrix (:806-829): diagonal 0 = [1] * slots + [i] * slots, diagonal slots = [i] * slots + [1] * slots"""
    a = np.zeros((2, 2 * slots, 2))
    a[0, :slots, 0] = 1.0
    a[0, slots:, 1] = 1.0
    a[1, :slots, 1] = 1.0
    a[1, slots:, 0] = 1.0
    return a


# ---- GenMatrices on the device ----------------------------------------------------------------------------------------------------------------
class DeviceDiagonals:
    """One factor on the device: Index, the sorted diagonal indices, and Block, a DeviceValues of shape (len(Index), dslots) whose row k holds
    diagonal Index[k]"""

    def __init__(self, Index, Block):
        self.Index, self.Block = list(Index), Block

    def DiagonalsIndexList(self):
        return list(self.Index)

    def host(self):
        """the factor as a lintrans.Diagonals of numpy rows"""
        a = self.Block.numpy()
        return lintrans.Diagonals({k: a[row].copy() for row, k in enumerate(self.Index)})


def _words(ring, n):
    return DeviceValues(ring, 1, max(int(n), 1), complex=False)


def _gen_device(d, LogN, roots, ring, rots_of):
    """rots_of: None, or a function (factor number, index list) -> the left rotation of every diagonal (the BSGS pre-rotation of lintrans.Encode)"""
    L = lib()
    roots, pow5 = d._tables(roots)
    factors, logdSlots = d._plan(LogN)
    dslots, slots = 1 << logdSlots, 1 << d.LogSlots
    scaling = d._scaling()
    droots = DeviceValues.from_numpy(ring, roots.view(np.complex128).reshape(1, -1))
    dpow5 = _words(ring, pow5.size)
    _check(L.rh_dev_upload(ring._h, dpow5.ptr, _p(pow5), pow5.size))
    abc = DeviceValues(ring, 3, dslots)
    nmax = max(len(step[3]) for steps, _ in factors for step in steps)
    table = _words(ring, 3 * nmax)
    out, keep = [], []                                                   # keep: the intermediate blocks live until the stream has drained
    for f, (steps, zero_upper) in enumerate(factors):
        cur = None
        for lvl, rot, prog, index, first in steps:
            keep.append(cur)
            _check(L.rh_ckks_dft_level_vectors(ring._h, 1 if d.Type == HomomorphicDecode else 0, d.LogSlots, dslots, lvl, 1 if d.BitReversed else 0,
                                               droots.ptr, roots.shape[0], dpow5.ptr, pow5.size, abc.ptr))
            if first == "repack":
                cur = DeviceValues.from_numpy(ring, _repack_host(slots).reshape(2, -1).view(np.complex128))
            flat = []
            for terms in prog:
                terms = list(terms) + [(-2, 0)] * (3 - len(terms))
                for src, kind in terms:
                    flat += [src, kind]
            program = (C.c_int * len(flat))(*flat)
            new = DeviceValues(ring, len(index), dslots)
            _check(L.rh_ckks_dft_merge_level(ring._h, dslots, rot, abc.ptr, None if cur is None else cur.ptr, 0 if cur is None else cur.nvec, program,
                                             len(index), new.ptr, table.ptr, table.words))
            cur = new
        rots = None if rots_of is None else rots_of(f, index)
        if rots is None:
            _check(L.rh_ckks_dft_finish(ring._h, dslots, len(index), cur.ptr, cur.ptr, scaling, 1 if zero_upper else 0, None, None, 0))
            fin = cur
        else:
            keep.append(cur)
            fin = DeviceValues(ring, len(index), dslots)
            _check(L.rh_ckks_dft_finish(ring._h, dslots, len(index), cur.ptr, fin.ptr, scaling, 1 if zero_upper else 0, (C.c_int * len(rots))(*rots),
                                        table.ptr, table.words))
        out.append(DeviceDiagonals(index, fin))
    _check(L.rh_ring_sync(ring._h))                                      # the scratch blocks above are freed on return
    return out


def _bsgs_rotations(index, cols, log_ratio):
    """lintrans.Encode (:231-241): the diagonals of giant step j go to the encoder rotated to the left by -j"""
    N1 = 0 if log_ratio < 0 else lintrans.FindBestBSGSRatio(index, cols, log_ratio)
    return [0 if N1 == 0 else -(((k // N1) * N1) & (cols - 1)) & (cols - 1) for k in index]


# ---- NewMatrixFromLiteral (:159-215) -------------------------------------------------------------------------------------------------------------
class Matrix:
    """dft.Matrix: the literal and its factors, a list of lintrans.LinearTransformation; the literal's fields read through"""

    def __init__(self, MatrixLiteral, Matrices):
        self.MatrixLiteral, self.Matrices = MatrixLiteral, list(Matrices)

    def __getattr__(self, name):
        return getattr(self.__dict__["MatrixLiteral"], name)


def NewMatrixFromLiteral(ringQ, ringP, d, encoder, levels_consumed_per_rescaling=1, roots=None):
    """As written, with its quirks: every factor is allocated at d.LevelQ, whatever level its turn comes at; the scale of group i is Q[level],
    level going down by one per entry of Levels, and for Levels[i] > 1 its Levels[i]-th root (ScaleRoot).  Each factor is generated on the
    device, pre-rotated for its BSGS schedule, and encoded by ONE Encoder.Embed into one rlwe.PolyQP block of ndiag polys; the entries of
    LinearTransformation.Vec are one-poly views that keep the block alive."""
    who = "cannot NewDFTMatrixFromLiteral"
    if ringQ.kind != _StandardRing:
        raise RingHipError("%s: conjugate-invariant and 3N rings are not supported by the device path" % who)
    if encoder.Prec() > 53:
        raise RingHipError("%s: encoder precision %d > 53 needs the *big.Float / *bignum.Complex encoder, which stays with the reference" % (who, encoder.Prec()))
    if ringP is None or getattr(encoder, "ringP", None) is None:
        raise RingHipError("%s: a linear transformation is encoded modulo QP: NewMatrixFromLiteral and its encoder need ringP" % who)
    if int(levels_consumed_per_rescaling) != 1:
        raise RingHipError("%s: LevelsConsumedPerRescaling = %d: the PREC128 path is not built" % (who, levels_consumed_per_rescaling))
    N = ringQ.N
    LogN = N.bit_length() - 1
    if not 1 <= d.LogSlots <= LogN - 1:
        raise RingHipError("%s: LogSlots = %d outside [1, LogN - 1 = %d]" % (who, d.LogSlots, LogN - 1))
    d._check(LogN)
    if not (0 <= d.LevelQ < ringQ.L and 0 <= d.LevelP < ringP.L):
        raise RingHipError("%s: LevelQ = %d, LevelP = %d out of range" % (who, d.LevelQ, d.LevelP))
    if d.LevelQ - d.Depth(False) < 0:                                    # EvaluateSequential rescales after every factor
        raise RingHipError("%s: %d levels are consumed below LevelQ = %d: the chain needs sum(Levels) + 1 = %d moduli up to LevelQ"
                           % (who, d.Depth(False), d.LevelQ, d.Depth(False) + 1))
    logdSlots = d.LogSlots + 1 if d.LogSlots < LogN - 1 and d.Format == RepackImagAsReal else d.LogSlots
    cols = 1 << logdSlots
    Q = [int(q) for q in ringQ.moduli]

    blocks = _gen_device(d, LogN, roots, ringQ, lambda f, index: _bsgs_rotations(index, cols, d.LogBSGSRatio))
    matrices = []
    level, idx = d.LevelQ, 0
    for i in range(len(d.Levels)):
        scale = Scale(Q[level])
        if d.Levels[i] > 1:
            scale = ScaleRoot(scale, d.Levels[i])
        for _ in range(d.Levels[i]):
            blk = blocks[idx]
            ltparams = lintrans.Parameters(blk.Index, d.LevelQ, d.LevelP, scale, logdSlots, d.LogBSGSRatio)
            matrices.append(lintrans.NewTransformationFromBlock(ringQ, ringP, ltparams, encoder, blk.Index, blk.Block))
            idx += 1
        level -= 1
    return Matrix(d, matrices)


# ---- Evaluator (:143-360) -----------------------------------------------------------------------------------------------------------------------
class Evaluator:
    """dft.Evaluator over a ckks.Evaluator (NewEvaluator :150-156), on batches of ciphertexts that share the matrices.

    fused (per call, or FUSED_DFT when None; True / False / a dict): the kernels of csrc/ckks.hip (True) or the reference's own calls (False):
      split  Sub, Mul(-1i), Add after the transformations of CoeffsToSlots (rh_ckks_split_real_imag)
      merge  Mul(1i), Add before those of SlotsToCoeffs (rh_ckks_merge_real_imag)
    The bits are the same."""

    # A kernel is the default where the measurement shows it no slower than the calls it replaces, alone and in the whole circuit, at batches of
    # 1 and 8 (tools/bench_ops.py dft -> profiles/dft.json, "fused_dft_default"): both are.
    FUSED_DFT = {"split": True, "merge": True}

    def __init__(self, eval):
        self.eval = eval
        try:
            self.LTEvaluator = lintrans.Evaluator(eval)
        except RingHipError as e:
            raise RingHipError(str(e).replace("cannot NewEvaluator", "cannot NewEvaluator (dft)")) from None
        self.ringQ = eval.ringQ
        self.LogMaxSlots = self.ringQ.N.bit_length() - 2
        self._iscalars = {}                # _i_scalar's results by (level, sign)

    def _use(self, fused):
        if fused is None:
            return dict(self.FUSED_DFT)
        if isinstance(fused, dict):
            return {k: bool(fused.get(k, v)) for k, v in self.FUSED_DFT.items()}
        return {k: bool(fused) for k in self.FUSED_DFT}

    def _fit(self, ct, level, npoly):
        """opOut.Resize(degree, level): device blocks are dense, so blocks of another shape are replaced"""
        rq = self.ringQ.AtLevel(level)
        for c in (0, 1):
            if ct.Value[c].limbs != level + 1 or ct.Value[c].npoly != npoly:
                ct.Value[c] = rq.NewPoly(npoly)

    def _new(self, level, npoly):
        rq = self.ringQ.AtLevel(level)
        return Ciphertext([rq.NewPoly(npoly) for _ in (0, 1)], is_ntt=True)

    @staticmethod
    def _pp(polys):
        return (C.c_void_p * 2)(*[p.ptr for p in polys])

    def _i_scalar(self, level, sign):
        """the double RNS scalar of +-i as Mul(ct, +-1i, ct) forms it: a Gaussian integer, scale 1"""
        hit = self._iscalars.get((level, sign))
        if hit is None:
            s0, s1 = self.eval._rns_scalar(level, Scale(1), (Fraction(0), Fraction(sign)))
            hit = self._iscalars[(level, sign)] = (_u64(s0), _u64(s1))
        return hit

    def _check_in(self, ct, who):
        if not ct.IsNTT:
            raise RingHipError("cannot %s: coefficient-domain ciphertexts are not supported by the device path" % who)
        if ct.Degree() != 1:
            raise RingHipError("cannot %s: the input must be of degree 1" % who)
        if getattr(ct, "LogDimensions", None) is None:
            raise RingHipError("cannot %s: a ciphertext carries no LogDimensions" % who)

    def _split(self, zV, ctReal, tmp, fused):
        """ctReal holds Conjugate(zV) on entry: tmp = (zV - ctReal) (-i), ctReal = ctReal + zV (:267-278), one launch or the three calls"""
        ev = self.eval
        if fused:
            level, npoly = zV.Level(), zV.Value[0].npoly
            s0, s1 = self._i_scalar(level, -1)
            _check(lib().rh_ckks_split_real_imag(self.ringQ._h, level, self._pp(zV.Value), self._pp(ctReal.Value), self._pp(ctReal.Value),
                                                 self._pp(tmp.Value), npoly, _p(s0), _p(s1)))
            tmp.Scale, tmp.IsNTT = ev._scale(zV, "CoeffsToSlots"), True
            return
        ev.Sub(zV, ctReal, tmp)                                                                   # the imaginary part (:267-273)
        ev.Mul(tmp, -1j, tmp)
        ev.Add(ctReal, zV, ctReal)                                                                # the real part (:276)

    def _merge_parts(self, ctReal, ctImag, opOut, fused):
        """opOut = ctImag i + ctReal (:324-330), one launch -- when the two scales are equal, so that Add scales neither -- or the two calls"""
        ev = self.eval
        if fused and ev._scale(ctImag, "SlotsToCoeffs").Cmp(ev._scale(ctReal, "SlotsToCoeffs")) == 0:
            level, npoly = ctImag.Level(), ctImag.Value[0].npoly
            s0, s1 = self._i_scalar(level, 1)
            _check(lib().rh_ckks_merge_real_imag(self.ringQ._h, level, self._pp(ctReal.Value), self._pp(ctImag.Value), self._pp(opOut.Value), npoly,
                                                 _p(s0), _p(s1)))
            opOut.Scale, opOut.IsNTT = ev._scale(ctImag, "SlotsToCoeffs"), True
            return
        ev.Mul(ctImag, 1j, opOut)                                                                 # (:324)
        ev.Add(opOut, ctReal, opOut)                                                              # (:328)

    # ---- dft (:345-360) ----
    def dft(self, ctIn, matrices, opOut):
        inputLogSlots = ctIn.LogDimensions
        self.LTEvaluator.EvaluateSequential(ctIn, matrices, opOut)
        opOut.LogDimensions = inputLogSlots                              # a `fractal' transformation: the plaintext polynomial Y = X^{N/n} stays

    # ---- CoeffsToSlots (:222-300) ----
    def CoeffsToSlotsNew(self, ctIn, ctsMatrices, fused=None):
        npoly = ctIn.Value[0].npoly
        ctReal = self._new(ctsMatrices.LevelQ, npoly)
        ctImag = self._new(ctsMatrices.LevelQ, npoly) if ctsMatrices.LogSlots == self.LogMaxSlots else None
        self.CoeffsToSlots(ctIn, ctsMatrices, ctReal, ctImag, fused=fused)
        return ctReal, ctImag

    def CoeffsToSlots(self, ctIn, ctsMatrices, ctReal, ctImag, fused=None):
        """ctReal = Ecd(vReal || vImag) and ctImag = None for a sparse packing (n < N/2); ctReal = Ecd(vReal), ctImag = Ecd(vImag) for a full one"""
        who = "CoeffsToSlots"
        self._check_in(ctIn, who)
        ev = self.eval
        try:
            if ctsMatrices.Format not in (RepackImagAsReal, SplitRealAndImag):
                return self.dft(ctIn, ctsMatrices.Matrices, ctReal)
            use = self._use(fused)
            npoly = ctIn.Value[0].npoly
            zV = self._new(min(ctIn.Level(), ctsMatrices.LevelQ), npoly)                          # ctIn.CopyNew(): every word is written by dft
            self.dft(ctIn, ctsMatrices.Matrices, zV)
            level = zV.Level()
            self._fit(ctReal, level, npoly)
            ev.Conjugate(zV, ctReal)                                                              # (:246)
            ctReal.LogDimensions = zV.LogDimensions
            if ctImag is not None:
                tmp = ctImag
                self._fit(tmp, level, npoly)
            else:                                                                                 # eval.GetBuffCt() (:254)
                tmp = Ciphertext([ev._buffer("dftTmp%d" % c, self.ringQ.AtLevel(level), npoly, level + 1) for c in (0, 1)], is_ntt=True)
            self._split(zV, ctReal, tmp, use["split"])
            tmp.LogDimensions = zV.LogDimensions
            if ctsMatrices.Format == RepackImagAsReal and ctsMatrices.LogSlots < self.LogMaxSlots:   # the right n/2 slots of both are zero (:281-289)
                rot = Ciphertext([ev._buffer("dftRot%d" % c, self.ringQ.AtLevel(level), npoly, level + 1) for c in (0, 1)], is_ntt=True)
                ev.Rotate(tmp, 1 << ctIn.LogDimensions, rot)
                ev.Add(ctReal, rot, ctReal)
        except RingHipError as e:
            raise RingHipError("cannot CoeffsToSlots: %s" % e) from None

    # ---- SlotsToCoeffs (:306-342) ----
    def SlotsToCoeffsNew(self, ctReal, ctImag, stcMatrices, fused=None):
        if ctReal.Level() < stcMatrices.LevelQ or (ctImag is not None and ctImag.Level() < stcMatrices.LevelQ):
            raise RingHipError("ctReal.Level() or ctImag.Level() < DFTMatrix.LevelQ")
        opOut = self._new(stcMatrices.LevelQ, ctReal.Value[0].npoly)
        self.SlotsToCoeffs(ctReal, ctImag, stcMatrices, opOut, fused=fused)
        return opOut

    def SlotsToCoeffs(self, ctReal, ctImag, stcMatrices, opOut, fused=None):
        who = "SlotsToCoeffs"
        self._check_in(ctReal, who)
        ev = self.eval
        try:
            if ctImag is None:
                return self.dft(ctReal, stcMatrices.Matrices, opOut)
            self._check_in(ctImag, who)
            use = self._use(fused)
            npoly = ctReal.Value[0].npoly
            level = ev._operands(who, ctReal, ctImag)
            self._fit(opOut, level, npoly)
            self._merge_parts(ctReal, ctImag, opOut, use["merge"])
            opOut.LogDimensions = ctImag.LogDimensions
            self.dft(opOut, stcMatrices.Matrices, opOut)
        except RingHipError as e:
            raise RingHipError("cannot SlotsToCoeffs: %s" % e) from None

"""schemes/matrix_ckks on the device: parameters, plaintexts and ciphertexts, the encoder, keys, encryption and decryption on the 3N ring
Z_Q[X]/(X^N - X^(N/2) + 1), N = 2^order2 3^order3.

  Parameters                       rlwe.Parameters3N as far as the scheme reads it (core/rlwe/params_3n.go): moduli given explicitly
  NewPlaintext, NewCiphertext      matrix_ckks.go:29-68 (IsBatched = true, Scale = DefaultScale, LogDimensions = LogMaxDimensions)
  NewEncoder -> Encoder            encoder.go:108-445, on batches of nvec vectors (csrc/matrix_ckks.hip)
  NewKeyGenerator, NewEncryptor, NewDecryptor     matrix_ckks.go:77-100: the rlwe classes (keygen.py) on the 3N rings, carrying the metadata
  NewEvaluator                     MatrixCKKSEvaluator (schemes.py), unchanged
  MatrixEncryptor, MatrixDecryptor encryptor.go:48-86, decryptor.go:31-74, as written
  computeInputPermutation, computeInversePermutation, factorN3N, pow3       encoder.go:25-106, host functions

Givens and deviations of the encoder.  Encode follows SingleFloat64ToFixedPointCRT (encoder.go:384-426) as written: a uint64 value goes through
float64(val); the sign goes onto the scale; the product is TRUNCATED (uint64(value)), not rounded; from 1.8446744073709552e+19 on the word is the
LOW 64 bits of the integer m 2^e the float is (big.Int.Uint64), with no sign applied; below, a negative value gives c = -c modulo 2^64.  The
reference then applies ONE conditional subtraction (ring.CRed), so the word it stores can be >= q; the device stores the canonical residue in
[0, q) of that word (the deviation the CKKS encoder documents too).
  negatives="as_written" (default): a negative value encodes (2^64 - |c|) mod q, NOT -|c| mod q: Decode does not give it back (the reference's
      tests use positive values only).
  negatives="signed": a negative value encodes q - (|c| mod q) (0 when q divides c), on the big path q - (m 2^e mod q): what polyToFloatNoCRT's
      centring decodes.
The two differ on negative values alone (and there on every limb, since 2^64 mod q != 0).
Decode restates polyToFloatNoCRT (:430-445) on limb 0 alone; an NTT-domain plaintext's limb 0 is inverse-transformed into a buffer first
(:314-317; the plaintext is not modified, a block-order tag is honoured).  The uint64 output truncates non-negative values; Go leaves the
conversion of a negative float64 to uint64 implementation-defined (0 here, untested).

Refused by name: conjugate-invariant rings, 3N degrees with N % 8 != 0 (the samplers serve groups of eight coefficients), Galois keys on 3N
rings (ring/automorphism.go:14-20), encoder precision above 53.  Follow-ups: moduli from LogQ / LogP (GenModuli3N), Parameters3N
marshalling, multiparty protocols on 3N rings, a slot encoder, a relinearising Mul inside the evaluator."""
import ctypes as C

import numpy as np

from .ckks import DeviceValues, Scale
from .keygen import Decryptor as _Decryptor
from .keygen import Encryptor as _Encryptor
from .keygen import KeyGenerator, _pt_poly, error_sampler
from .ringhip import DevicePoly, Matrix3N, Ring, RingHipError, _check, _p, lib
from .sampling import NewPRNG, SmallPoly, lift_small, rings_ok
from .schemes import Ciphertext as _Ciphertext
from .schemes import MatrixCKKSEvaluator

U64, F64, C128 = 0, 1, 2          # the vtype of rh_matrix_ckks_encode / _decode


# ---- encoder.go:25-106: the coefficient order of the mixed-radix transform, host functions ---------------------------------------------------------
def pow3(b):
    return 3 ** int(b)


def factorN3N(n):
    """n = 2^a 3^b -> (a, b) (:82-97)"""
    n = int(n)
    if n < 1:
        raise RingHipError("n must be of form 2^a * 3^b, but has other factors: %d" % n)
    a = b = 0
    while n % 2 == 0:
        a, n = a + 1, n // 2
    while n % 3 == 0:
        b, n = b + 1, n // 3
    if n != 1:
        raise RingHipError("n must be of form 2^a * 3^b, but has other factors: %d" % n)
    return a, b


def computeInputPermutation(n):
    """(:25-70): one radix-2 layer, the radix-3 layers, the remaining radix-2 layers"""
    a, b = factorN3N(n)
    if a < 1:
        raise RingHipError("n must be even, got n = %d" % n)
    index = [0]
    shift = n >> 1
    index += [x + shift for x in index]
    for _ in range(b):
        shift //= 3
        base = list(index)
        index += [x + shift for x in base] + [x + 2 * shift for x in base]
    for _ in range(a - 1):
        shift //= 2
        index += [x + shift for x in list(index)]
    return index


def computeInversePermutation(perm):
    """(:73-79)"""
    inv = [0] * len(perm)
    for i, p in enumerate(perm):
        inv[p] = i
    return inv


# ---- parameters, plaintexts, ciphertexts -----------------------------------------------------------------------------------------------------------
class Parameters:
    """rlwe.Parameters3N with explicit moduli: ringQ / ringP are Ring(N, ., kind=Matrix3N), N = 2^order2 3^order3.  xs: ("P", density) or
    ("H", weight); xe: (sigma, bound) or a ternary law likewise.  omega3n: (omegas of Q, omegas of P) as the Go side holds them, or None."""

    def __init__(self, order2, order3, Q, P, default_scale, xs=("P", 2 / 3), xe=(3.2, 19), device=0, omega3n=None):
        self.order2, self.order3 = int(order2), int(order3)
        if self.order2 < 1 or self.order3 < 1:
            raise RingHipError("Parameters: a 3N ring has N = 2^order2 * 3^order3 with order2, order3 >= 1")
        n = (1 << self.order2) * pow3(self.order3)
        if n % 8:
            raise RingHipError("cannot Parameters: a 3N ring of degree %d: the samplers serve groups of eight coefficients (N %% 8 must be 0)" % n)
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in (P or [])]
        omQ, omP = omega3n if omega3n is not None else (None, None)
        self.ringQ = Ring(n, self.Q, kind=Matrix3N, device=device, omega3n=omQ)
        self.ringP = Ring(n, self.P, kind=Matrix3N, device=device, omega3n=omP) if self.P else None
        self.scale = Scale(default_scale)
        self.xs, self.xe = tuple(xs), tuple(xe)

    def N(self): return self.ringQ.N
    def MaxLevel(self): return len(self.Q) - 1
    def MaxLevelQ(self): return len(self.Q) - 1
    def MaxLevelP(self): return len(self.P) - 1
    def RingQ(self): return self.ringQ
    def RingP(self): return self.ringP
    def DefaultScale(self): return self.scale
    def MaxSlots(self): return self.N() // 2                                  # params_3n.go:378-382
    def LogMaxDimensions(self): return (self.order2 - 1, self.order3)         # ring.Dimensions{Rows, Cols}, params_3n.go:372-376
    def EncodingPrecision(self): return 53
    def Xs(self): return self.xs
    def Xe(self): return self.xe

    def close(self):
        for r in (self.ringQ, self.ringP):
            if r is not None:
                r.close()


class Plaintext(_Ciphertext):
    """rlwe.Plaintext of the scheme: one poly block (npoly vectors) and the MetaData"""

    def __init__(self, poly, scale, log_dimensions, is_ntt=False, is_batched=True):
        _Ciphertext.__init__(self, [poly], is_ntt=is_ntt)
        self.Scale, self.LogDimensions, self.IsBatched, self.IsMontgomery = Scale(scale), tuple(log_dimensions), bool(is_batched), False


def NewPlaintext(params, level, npoly=1):
    """matrix_ckks.go:29-42"""
    return Plaintext(params.RingQ().AtLevel(level).NewPoly(npoly), params.DefaultScale(), params.LogMaxDimensions())


def NewCiphertext(params, degree, level, npoly=1):
    """matrix_ckks.go:52-68"""
    rq = params.RingQ().AtLevel(level)
    ct = _Ciphertext([rq.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=False)
    ct.Scale, ct.LogDimensions, ct.IsBatched, ct.IsMontgomery = params.DefaultScale(), params.LogMaxDimensions(), True, False
    return ct


# ---- the encoder -----------------------------------------------------------------------------------------------------------------------------------
class DeviceWords:
    """(nvec, n) uint64 on the device: the []uint64 of a batch of vectors"""

    def __init__(self, ring, nvec, n):
        self.ring, self.nvec, self.n, self.words = ring, int(nvec), int(n), int(nvec) * int(n)
        self._block = DevicePoly(ring.AtLevel(0), (self.words + ring.N - 1) // ring.N or 1, 1)
        self.ptr = self._block.ptr

    @classmethod
    def from_numpy(cls, ring, arr):
        arr = np.ascontiguousarray(np.asarray(arr, dtype=np.uint64))
        arr = arr[None] if arr.ndim == 1 else arr
        v = cls(ring, arr.shape[0], arr.shape[1])
        if v.words:
            _check(lib().rh_dev_upload(ring._h, v.ptr, _p(arr.reshape(-1)), v.words))
        return v

    def numpy(self):
        out = np.empty(self.words, dtype=np.uint64)
        if self.words:
            _check(lib().rh_dev_download(self.ring._h, _p(out), self.ptr, self.words))
        return out.reshape(self.nvec, self.n)


def _vtype(v):
    if isinstance(v, DeviceWords):
        return U64
    if isinstance(v, DeviceValues):
        return C128 if v.complex else F64
    return None


class Encoder:
    """matrix_ckks.Encoder on device batches: Encode / Decode of nvec vectors in one launch each.  negatives: "as_written" or "signed" (the
    module docstring says where they differ)."""

    def __init__(self, params, precision=0, negatives="as_written"):
        self.parameters, self.prec = params, int(precision) or 53
        if self.prec > 53:
            raise RingHipError("cannot NewEncoder: precision %d > 53 (the *big.Float path) is not built on the device path" % self.prec)
        if negatives not in ("as_written", "signed"):
            raise RingHipError("cannot NewEncoder: negatives must be \"as_written\" or \"signed\"")
        self.negatives, self.n = negatives, params.N()

    def Prec(self): return self.prec
    def GetParameters(self): return self.parameters

    def _values(self, values, nvec):
        """a device block of (nvec, nvals) values and its vtype, from a host array (one vector or a batch) or a device block"""
        ring = self.parameters.RingQ()
        vt = _vtype(values)
        if vt is None:
            arr = np.asarray(values)
            arr = arr[None] if arr.ndim == 1 else arr
            if arr.ndim != 2:
                raise RingHipError("cannot Encode: values are one vector or an (nvec, nvals) array")
            if arr.shape[1] > self.n:
                raise RingHipError("too many values: %d > %d" % (arr.shape[1], self.n))
            if arr.dtype == np.uint64:
                values = DeviceWords.from_numpy(ring, arr)
            elif np.iscomplexobj(arr) or arr.dtype == np.float64:
                values = DeviceValues.from_numpy(ring, arr)
            else:
                raise RingHipError("cannot Encode: supported types are []uint64, []float64, or []complex128, but %s was given" % arr.dtype)
            vt = _vtype(values)
        if values.n > self.n:
            raise RingHipError("too many values: %d > %d" % (values.n, self.n))
        if values.nvec != nvec:
            raise RingHipError("cannot Encode: %d vectors for a plaintext batch of %d" % (values.nvec, nvec))
        return values, vt

    def Encode(self, values, pt):
        """(:163-257): (nvec, nvals) values -> the coefficients of pt, coefficient domain (pt.IsNTT = False)"""
        p = _pt_poly(pt)
        dv, vt = self._values(values, p.npoly)
        _check(lib().rh_matrix_ckks_encode(self.parameters.RingQ()._h, p.limbs - 1, pt.Scale.Float64(), dv.ptr, vt, dv.n, p.npoly,
                                           1 if self.negatives == "signed" else 0, p.ptr))
        p.layout = None
        pt.IsNTT = False

    def Decode(self, pt, values=None, nvals=None, dtype=np.float64):
        """(:260-351): the first nvals coefficients of limb 0 over the scale.  values: a DeviceWords / DeviceValues block of (nvec, nvals) that is
        filled on the device, or None: a new host array of `dtype` (uint64, float64 or complex128) with nvals columns (default N)."""
        p = _pt_poly(pt)
        ring = self.parameters.RingQ()
        on_dev = _vtype(values) is not None
        if on_dev:
            dv, vt = values, _vtype(values)
            if dv.nvec != p.npoly:
                raise RingHipError("cannot Decode: %d vectors for a plaintext batch of %d" % (dv.nvec, p.npoly))
        else:
            if values is not None:
                raise RingHipError("cannot Decode: values is a device block or None")
            nvals = self.n if nvals is None else int(nvals)
            dt = np.dtype(dtype)
            if dt not in (np.dtype(np.uint64), np.dtype(np.float64), np.dtype(np.complex128)):
                raise RingHipError("cannot Decode: supported types are *[]uint64, *[]float64, or *[]complex128, but %s was given" % dt)
            if nvals > self.n:
                raise RingHipError("too many values: %d > %d" % (nvals, self.n))
            dv = DeviceWords(ring, p.npoly, nvals) if dt == np.uint64 else DeviceValues(ring, p.npoly, nvals, dt == np.complex128)
            vt = _vtype(dv)
        if dv.n > self.n:
            raise RingHipError("too many values: %d > %d" % (dv.n, self.n))
        src, rows = p, p.limbs
        if pt.IsNTT:                                                        # (:314-317): INTT into the encoder's buffer; limb 0 is all that is read
            r0 = ring.AtLevel(0)
            src, rows = r0.NewPoly(p.npoly), 1
            r0.CopyLvl(p, src)
            r0.INTT(src, src)
        _check(lib().rh_matrix_ckks_decode(ring._h, pt.Scale.Float64(), src.ptr, rows, p.npoly, dv.n, vt, dv.ptr))
        return dv if on_dev else dv.numpy()


def NewEncoder(params, precision=0, negatives="as_written"):
    return Encoder(params, precision, negatives)


# ---- keys, encryption, decryption: rlwe's on the 3N rings (matrix_ckks.go:77-100) ----------------------------------------------------------------------
def NewKeyGenerator(params, prng=None):
    return KeyGenerator(params.RingQ(), params.RingP(), params.Xs(), params.Xe(), prng)


class Encryptor(_Encryptor):
    """rlwe.Encryptor on the scheme's plaintext batches; the ciphertext takes the plaintext's Scale, LogDimensions and IsBatched"""


class Decryptor(_Decryptor):
    """rlwe.Decryptor; DecryptNew returns a Plaintext of the scheme with the ciphertext's metadata"""

    def DecryptNew(self, ct, fused=None):
        poly = self.ringQ.AtLevel(ct.Level()).NewPoly(ct.Value[0].npoly)
        pt = Plaintext(poly, getattr(ct, "Scale", 1), getattr(ct, "LogDimensions", (0, 0)), ct.IsNTT, getattr(ct, "IsBatched", True))
        self.Decrypt(ct, pt, fused)
        return pt


def NewEncryptor(params, key, prng=None):
    return Encryptor(params.RingQ(), params.RingP(), key, prng, params.Xs(), params.Xe())


def NewDecryptor(params, sk):
    return Decryptor(params.RingQ(), sk)


def NewEvaluator(params, block_order=True):
    return MatrixCKKSEvaluator(params.RingQ(), block_order)


# ---- encryptor.go / decryptor.go of the scheme, as written ----------------------------------------------------------------------------------------
def _meta(src, dst):
    for name in ("Scale", "LogDimensions", "IsBatched", "IsMontgomery"):
        if hasattr(src, name):
            setattr(dst, name, getattr(src, name))
    dst.IsNTT = src.IsNTT


class MatrixEncryptor:
    """encryptor.go:48-86 as written: ct = (pt + e - MRed(a, sk.Value.Q), a) with a AND e read from the ERROR sampler, the product
    coefficient-wise whatever the domain, no transform, IsNTT copied.  This is a MASK under the stored form of the secret, not an RLWE
    encryption: a is small and a . s is not a ring product.  One rh_rlwe_encrypt_sk call.  samples: {"a": (npoly, N), "e": (npoly, N)} int32."""

    def __init__(self, params, sk, prng=None):
        rings_ok("MatrixEncryptor", params.RingQ())
        self.params, self.ringQ, self.sk = params, params.RingQ(), sk
        self.prng = NewPRNG() if prng is None else prng
        self.xe = error_sampler(self.prng, self.ringQ, params.Xe())

    def _small(self, npoly, given):
        if given is not None:
            return SmallPoly.from_numpy(self.ringQ, np.asarray(given, dtype=np.int32).reshape(npoly, self.ringQ.N))
        return self.xe.ReadNew(npoly)

    def Encrypt(self, pt, ct, samples=None):
        samples = samples or {}
        level, p = pt.Level(), _pt_poly(pt)
        if ct.Degree() != 1 or ct.Level() != level or ct.Value[0].npoly != p.npoly:
            raise RingHipError("cannot Encrypt: allocate the ciphertext with degree 1 at the plaintext's level and batch size")
        if self.sk.LevelQ() < level:
            raise RingHipError("the secret key has fewer limbs than the ciphertext's level")
        rq = self.ringQ.AtLevel(level)
        if pt.IsNTT:
            rq.ToReferenceOrder(p)                                          # the secret is held in the reference's order
        c0, c1 = ct.Value
        e = rq.NewPoly(p.npoly)
        lift_small(rq, None, self._small(p.npoly, samples.get("a")), c1)
        lift_small(rq, None, self._small(p.npoly, samples.get("e")), e)
        sk = DevicePoly(rq, 1, level + 1, ptr=self.sk.Value.Q.ptr, owner=self.sk.Value.Q)
        _check(lib().rh_rlwe_encrypt_sk(rq._h, level, c1.ptr, sk.ptr, e.ptr, p.ptr, c0.ptr, p.npoly))
        c0.layout = c1.layout = None
        _meta(pt, ct)

    def EncryptNew(self, pt, samples=None):
        ct = NewCiphertext(self.params, 1, pt.Level(), _pt_poly(pt).npoly)
        self.Encrypt(pt, ct, samples)
        return ct


class MatrixDecryptor:
    """decryptor.go:31-74 as written: pt = ct[0] + MRed(sk.Value.Q, ct[1]), coefficient-wise, reduced; no transform, IsNTT copied.
    One rh_rlwe_decrypt call."""

    def __init__(self, params, sk):
        rings_ok("MatrixDecryptor", params.RingQ())
        self.params, self.ringQ, self.sk = params, params.RingQ(), sk

    def Decrypt(self, ct, pt):
        level, out = min(ct.Level(), pt.Level()), _pt_poly(pt)
        if ct.Degree() != 1 or ct.Level() != level or out.limbs != level + 1 or out.npoly != ct.Value[0].npoly:
            raise RingHipError("cannot Decrypt: a ciphertext of degree 1 and a plaintext at its level and batch size")
        rq = self.ringQ.AtLevel(level)
        for v in ct.Value:
            rq.ToReferenceOrder(v)
        sk = DevicePoly(rq, 1, level + 1, ptr=self.sk.Value.Q.ptr, owner=self.sk.Value.Q)
        _check(lib().rh_rlwe_decrypt(rq._h, level, ct.Value[0].ptr, ct.Value[1].ptr, None, sk.ptr, out.ptr, out.npoly))
        out.layout = None
        _meta(ct, pt)

    def DecryptNew(self, ct):
        pt = NewPlaintext(self.params, ct.Level(), ct.Value[0].npoly)
        self.Decrypt(ct, pt)
        return pt

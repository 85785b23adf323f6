"""Host-side mirror of the BGV evaluator's scale-invariant (BFV) multiply, schemes/bgv/evaluator.go, on device-resident batches in the
NTT domain.  Call sequences only: the arithmetic is the HIP library's (csrc/bfv.hip); encoders, key generation and BGV's scale-matching
paths stay with the reference.

  newEvaluatorPrecomp      :46-78        MulScaleInvariant(New)       :771-857     MulRelinScaleInvariant(New)  :877-972
  tensorScaleInvariant     :975-1040     MulScaleInvariant (scale)    :1045-1051   quantize                     :1104-1124

Only the ciphertext x ciphertext branch (op1.Degree() == 1) is built.  A degree-0 operand, slices and scalars take tensorStandard / Mul in
the reference (BGV's scale matching): they are refused by name.  A batch of B ciphertexts is one Ciphertext whose polys have npoly = B; all
operands of a call sit at the same level (dense (npoly, level+1, N) blocks), which may be lower than the ring's top."""
import ctypes as C

from .ringhip import RingHipError, _check, lib
from .schemes import Ciphertext
from . import rlwe


def MulScaleInvariant(t, Q_level, a, b):
    """:1045-1051: the scale after the invariant tensoring, c = a * b / (T - (Q_level mod T)) in rlwe.Scale arithmetic modulo T
    (core/rlwe/scale.go:77-119: the product reduced modulo T, then times the modular inverse of the divisor).  Python ints in and out."""
    t, Q_level = int(t), int(Q_level)
    c = (int(a) * int(b)) % t
    q_mod_t_neg = t - Q_level % t
    try:
        inv = pow(q_mod_t_neg, -1, t)
    except ValueError:
        raise RingHipError("MulScaleInvariant: T - (Q mod T) = %d has no inverse modulo T = %d" % (q_mod_t_neg, t))
    return (c * inv) % t


class Evaluator(rlwe.Evaluator):
    """bgv.Evaluator restricted to the scale-invariant multiply.  ringQMul: bgv/params.go:98-108 (ceil((bitlen(Q) + logN) / 61) NTT-friendly
    61-bit primes disjoint from Q); ringP / rlk: the key-switch ring and the relinearisation key (rlwe.GadgetCiphertext) for the Relin forms."""

    def __init__(self, ringQ, ringQMul, t, ringP=None, rlk=None):
        super().__init__(ringQ, ringP, galois_keys={"rlk": rlk} if rlk is not None else None)
        self.ringQMul, self.t = ringQMul, int(t)
        h = C.c_void_p()
        _check(lib().rh_bfv_create(C.byref(h), ringQ._h, ringQMul._h, self.t))
        self._bfv = h
        self.levelQMul = [lib().rh_bfv_level_qmul(h, i) for i in range(ringQ.L)]          # :51-56

    def close(self):
        if getattr(self, "_bfv", None):
            lib().rh_bfv_destroy(self._bfv)
            self._bfv = None
        super().close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, npoly):
        """pre-size the handle's scratch for multiplies of npoly ciphertexts at the top level: no allocation afterwards"""
        _check(lib().rh_bfv_reserve(self._bfv, int(npoly)))

    def set_tuning(self, key, value):
        _check(lib().rh_bfv_set_tuning(self._bfv, key.encode(), int(value)))

    def QuantizePath(self, level):
        """"fused": quantize's two basis extensions and the scalar multiply run as one kernel at this level; "composed": three launches"""
        rc = lib().rh_bfv_quantize_path(self._bfv, int(level))
        if rc < 0:
            _check(rc)
        return "fused" if rc else "composed"

    # ---- the two kernels on their own (tensorLowDeg :1062-1102, quantize :1104-1124) ----------------------------------------------
    def TensorLowDeg(self, level, ct0Q, ct1Q, ct2Q, ct0M, ct1M, ct2M):
        """ct0*, ct1*: two-component lists of blocks in Q / QMul (ct1* None: the squaring case); ct2*: three-component output lists.
        c1 is left in [0, 2q) as MulCoeffsMontgomeryThenAddLazy / AddLazy leave it."""
        sq = ct1Q is None
        b = [None, None] if sq else list(ct1Q)
        bm = [None, None] if sq else list(ct1M)
        self._rows(level, *ct0Q, *ct2Q, *[p for p in b if p is not None])
        self._rows(self.levelQMul[level], *ct0M, *ct2M, *[p for p in bm if p is not None])
        ptr = lambda p: p.ptr if p is not None else None
        _check(lib().rh_bfv_tensor_lazy(self._bfv, level, ct0Q[0].ptr, ct0Q[1].ptr, ptr(b[0]), ptr(b[1]), ct0M[0].ptr, ct0M[1].ptr, ptr(bm[0]), ptr(bm[1]),
                                        ct2Q[0].ptr, ct2Q[1].ptr, ct2Q[2].ptr, ct2M[0].ptr, ct2M[1].ptr, ct2M[2].ptr, ct0Q[0].npoly, 1 if sq else 0))

    def Quantize(self, level, c2Q1, c2Q2, out=None):
        """NTT-domain c (Q) and c (QMul) -> NTT-domain round(c / Q) * T in Q; out defaults to c2Q1 (the reference works in place)"""
        out = c2Q1 if out is None else out
        self._rows(level, c2Q1, out)
        self._rows(self.levelQMul[level], c2Q2)
        _check(lib().rh_bfv_quantize(self._bfv, level, c2Q1.ptr, c2Q2.ptr, out.ptr, c2Q1.npoly))

    # ---- :771-972 -----------------------------------------------------------------------------------------------------------------
    def _operands(self, op0, op1, opOut, relin, who):
        if not isinstance(op1, Ciphertext):
            raise RingHipError("cannot %s: op1 of type %s goes to tensorStandard / Mul (BGV scale matching), which the device path does not build"
                               % (who, type(op1).__name__))
        if op1.Degree() == 0:
            raise RingHipError("cannot %s: a degree-0 operand goes to tensorStandard (BGV scale matching), which the device path does not build" % who)
        if op0.Degree() != 1 or op1.Degree() != 1:
            raise RingHipError("cannot %s: input degrees must be 1, got %d and %d" % (who, op0.Degree(), op1.Degree()))
        if opOut.Degree() != (1 if relin else 2):
            raise RingHipError("cannot %s: opOut must have degree %d" % (who, 1 if relin else 2))
        if not (op0.IsNTT and op1.IsNTT):
            raise RingHipError("cannot %s: operands must be in the NTT domain" % who)
        lv = {op0.Level(), op1.Level(), opOut.Level()}
        if len(lv) != 1:
            raise RingHipError("cannot %s: operands must sit at the same level, got %s" % (who, sorted(lv)))
        return lv.pop()

    def tensorScaleInvariant(self, ct0, ct1, relin, opOut):
        """:975-1040"""
        level = opOut.Level()
        npoly = ct0.Value[0].npoly
        ringQ = self.ringQ.AtLevel(level)
        tmp0, tmp1 = (ct1, ct0) if ct1 is opOut else (ct0, ct1)                 # avoid overwriting if the second input is the output (:982-987)
        c2 = self.buffer("bfv_c2", ringQ, npoly, level + 1) if relin else opOut.Value[2]
        self._rows(level, *tmp0.Value, *tmp1.Value, opOut.Value[0], opOut.Value[1], c2)
        sq = tmp0 is tmp1
        _check(lib().rh_bfv_mul_scale_invariant(self._bfv, level, tmp0.Value[0].ptr, tmp0.Value[1].ptr, None if sq else tmp1.Value[0].ptr,
                                                None if sq else tmp1.Value[1].ptr, opOut.Value[0].ptr, opOut.Value[1].ptr, c2.ptr, npoly))
        if relin:
            rlk = self.galois_keys.get("rlk")
            if rlk is None:
                raise RingHipError("cannot TensorInvariant: relinearization key is missing")
            tmpCt = Ciphertext([self.buffer("bfv_ks0", ringQ, npoly, level + 1), self.buffer("bfv_ks1", ringQ, npoly, level + 1)], is_ntt=True)
            self.GadgetProduct(level, c2, rlk, tmpCt)                            # (:1029)
            ringQ.Add(opOut.Value[0], tmpCt.Value[0], opOut.Value[0])            # (:1033-1034)
            ringQ.Add(opOut.Value[1], tmpCt.Value[1], opOut.Value[1])
        Q = 1
        for q in self.ringQ.moduli[:level + 1]:
            Q *= int(q)
        opOut.Scale = MulScaleInvariant(self.t, Q, getattr(ct0, "Scale", 1), getattr(tmp1, "Scale", 1))   # (:1037)
        opOut.IsNTT = True

    def MulScaleInvariant(self, op0, op1, opOut):
        """:771-830, ciphertext branch: opOut (degree 2) = op0 x op1 * T / Q"""
        self._operands(op0, op1, opOut, False, "MulInvariant")
        self.tensorScaleInvariant(op0, op1, False, opOut)

    def MulRelinScaleInvariant(self, op0, op1, opOut):
        """:877-941, ciphertext branch: the same, relinearised to degree 1"""
        self._operands(op0, op1, opOut, True, "MulRelinInvariant")
        self.tensorScaleInvariant(op0, op1, True, opOut)

    def _new(self, degree, like):
        level, npoly = like.Level(), like.Value[0].npoly
        ringQ = self.ringQ.AtLevel(level)
        return Ciphertext([ringQ.NewPoly(npoly) for _ in range(degree + 1)], is_ntt=True)

    def MulScaleInvariantNew(self, op0, op1):
        """:849-857"""
        opOut = self._new(2, op0)
        self.MulScaleInvariant(op0, op1, opOut)
        return opOut

    def MulRelinScaleInvariantNew(self, op0, op1):
        """:960-972"""
        opOut = self._new(1, op0)
        self.MulRelinScaleInvariant(op0, op1, opOut)
        return opOut

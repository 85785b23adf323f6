"""Host-side mirror of core/rgsw's external product on device batches (a caller of the key-switch path, SURVEY 8(b) "Callers").

  Ciphertext               core/rgsw/elements.go:15-25   (two gadget ciphertexts: Value[0], Value[1])
  Evaluator.ExternalProduct   core/rgsw/evaluator.go:42-80, externalProductInPlaceMultipleP :188-257 (LevelP >= 1)
  NewCiphertext, Encryptor    core/rgsw/elements.go:27-40, encryptor.go:12-118 (secret key; every row of many ciphertexts in one launch: rh_rgsw_encrypt)

RLWE (c0, c1) x RGSW = (<decomp(c0), RGSW[0]> + <decomp(c1), RGSW[1]>) / P: two gadget products summed modulo QP BEFORE the one ModDown.
The reference accumulates both products in one pair of lazy accumulators with a running Reduce counter and closes with a Reduce; every
Reduce is the canonical residue, so the accumulators after the loop are the canonical residues of the sum whatever the schedule -- here
the two lazy products (rlwe.Evaluator.GadgetProductLazy: canonical residues modulo Q and modulo P) are added with ring.Add and handed to
ModDown: the same bits (tests/test_gpu_rgsw.py checks it against the reference's loop restated over the oracle pieces).  LevelP <= 0 takes
externalProductInPlaceSinglePAndBitDecomp (:119-186) the same way, and so does the 32-bit branch (:82-117, one modulus below 2^29 without P):
its wrapping 64-bit sum of NTTLazy digits times Montgomery-form key rows never overflows (:57) and IMForm closes it, so it is the canonical residue
of the same sum (tests/test_blindrot_oracle.py restates the literal loop against the Montgomery branch)."""
from .ringhip import RingHipError
from .rlwe import ElementQP, Evaluator as RLWEEvaluator, GadgetCiphertext
from .noise import NoiseRGSWCiphertext  # noqa: F401  (core/rgsw/utils.go)


class Ciphertext:
    """rgsw.Ciphertext: Value[0] encrypts (P*w*m, 0)-gadget of the message against c0, Value[1] against c1 (core/rgsw/elements.go:15-25)"""

    def __init__(self, value0, value1):
        if not isinstance(value0, GadgetCiphertext) or not isinstance(value1, GadgetCiphertext):
            raise RingHipError("rgsw.Ciphertext: two rlwe.GadgetCiphertext values")
        if (value0.LevelQ(), value0.LevelP()) != (value1.LevelQ(), value1.LevelP()):
            raise RingHipError("rgsw.Ciphertext: the two gadget ciphertexts must share their levels")
        self.Value = [value0, value1]

    def LevelQ(self):
        return self.Value[0].LevelQ()

    def LevelP(self):
        return self.Value[0].LevelP()


class Evaluator(RLWEEvaluator):
    """rgsw.Evaluator (core/rgsw/evaluator.go:12-35): an rlwe.Evaluator plus the external product"""

    def ExternalProduct(self, op0, op1, opOut):
        """opOut = op0 x op1 (:42-80).  op0, opOut: degree-1 rlwe ciphertexts (batches), NTT or coefficient domain like the reference
        (:208-216: the decomposition is taken from whichever domain op0 is in); op1: rgsw.Ciphertext with LevelP >= 1.  The product runs
        at op1's levels (:44); opOut may be op0."""
        levelQ, levelP = op1.LevelQ(), op1.LevelP()
        if levelP < 1:
            return self._external_product_single_p(op0, op1, opOut, levelQ, levelP)
        if len(op0.Value) != 2 or len(opOut.Value) != 2:
            raise RingHipError("ExternalProduct: degree-1 ciphertexts")
        if opOut.IsNTT is not True:
            raise RingHipError("ExternalProduct: the result is in the NTT domain (ModDownQPtoQNTT, :75-76)")
        self._rows(levelQ, op0.Value[0], op0.Value[1], opOut.Value[0], opOut.Value[1])
        npoly = op0.Value[0].npoly
        acc = [ElementQP.alloc(self.ringQ, self.ringP, npoly, levelQ, levelP) for _ in (0, 1)]
        for k in (0, 1):
            self.GadgetProductLazy(levelQ, op0.Value[k], op1.Value[k], acc[k], cxIsNTT=op0.IsNTT)
        rq, rp = self.ringQ.AtLevel(levelQ), self.ringP.AtLevel(levelP)
        for c in (0, 1):
            rq.Add(acc[0].Value[c].Q, acc[1].Value[c].Q, acc[0].Value[c].Q)
            rp.Add(acc[0].Value[c].P, acc[1].Value[c].P, acc[0].Value[c].P)
        self.ModDown(levelQ, levelP, acc[0], opOut)

    def _external_product_single_p(self, op0, op1, opOut, levelQ, levelP):
        """LevelP <= 0 (:55-70): externalProductInPlaceSinglePAndBitDecomp (:119-186) -- every digit is MaskVec of a limb of INTT(c_k) under
        every modulus (mask = all ones without a power-of-two decomposition), the products accumulated with the canonical
        MulCoeffsMontgomery(ThenAdd) over both components k -- then ModDownQPtoQNTT (LevelP = 0) or CopyLvl (no P).  Each component's sum is
        rh_bext_gadget_product_single_p_lazy in its rgsw digit form; the two canonical sums are added with ring.Add.  The reference's 32-bit
        branch (:54-57, :82-117: one modulus below 2^29, plain wrapping products closed by IMForm) gives the same canonical residues and runs
        through the same calls."""
        import ctypes as C
        from .ringhip import _check, lib, DevicePoly
        if levelQ == 0 and levelP == -1 and (int(self.ringQ.moduli[0]) >> 29) == 0 and op1.Value[0].BaseTwoDecomposition == 0:
            raise RingHipError("ExternalProduct: the 32-bit branch (core/rgsw/evaluator.go:82-117) without a power-of-two decomposition masks "
                               "every digit with (1 << 0) - 1 = 0 in the reference; that zero product is not built")
        if not op0.IsNTT or opOut.IsNTT is not True:
            raise RingHipError("ExternalProduct (LevelP <= 0): NTT-domain ciphertexts (the reference takes INTT of op0.Value[k], :148)")
        self._rows(levelQ, op0.Value[0], op0.Value[1], opOut.Value[0], opOut.Value[1])
        npoly = op0.Value[0].npoly
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        accQ = [[DevicePoly(rq, npoly, levelQ + 1) for _ in (0, 1)] for _ in (0, 1)]
        accP = [[DevicePoly(rp, npoly, levelP + 1) for _ in (0, 1)] for _ in (0, 1)] if rp is not None else None
        for k in (0, 1):
            g = op1.Value[k]
            dpl = g.digits_per_limb
            arr = (C.c_int * len(dpl))(*dpl) if dpl is not None else None
            _check(lib().rh_bext_gadget_product_single_p_lazy(
                self.be._h, levelQ, levelP, op0.Value[k].ptr, 1, g.BaseTwoDecomposition, arr, g.Q.ptr, g.P.ptr if g.P is not None else None,
                g.digits, 1, accQ[k][0].ptr, accQ[k][1].ptr, accP[k][0].ptr if accP else None, accP[k][1].ptr if accP else None, npoly))
        for c in (0, 1):
            rq.Add(accQ[0][c], accQ[1][c], accQ[0][c])
            if rp is not None:
                rp.Add(accP[0][c], accP[1][c], accP[0][c])
        if rp is not None:
            _check(lib().rh_bext_moddown_qp_to_q_ntt_pair(self.be._h, levelQ, levelP, accQ[0][0].ptr, accQ[0][1].ptr, accP[0][0].ptr, accP[0][1].ptr,
                                                          opOut.Value[0].ptr, opOut.Value[1].ptr, npoly))
        else:
            for c in (0, 1):
                rq.CopyLvl(accQ[0][c], opOut.Value[c])


# ---- core/rgsw/elements.go:27-40, encryptor.go ----------------------------------------------------------------------------------------------------------
def _ciphertexts(ringQ, ringP, tabQ, tabP, n, rows, levelQ, levelP, pw2, dpl):
    """n rgsw.Ciphertext over one table of n * 2 gadget ciphertexts (gadget 2 k: Value[0] of ciphertext k, gadget 2 k + 1: its Value[1])"""
    from .keygen import _view
    rq = ringQ.AtLevel(levelQ)
    rp = ringP.AtLevel(levelP) if levelP >= 0 else None
    g = lambda i: GadgetCiphertext.from_device(rq, rp, _view(tabQ, rq, 2 * i * rows, 2 * rows), _view(tabP, rp, 2 * i * rows, 2 * rows) if rp is not None else None,
                                               BaseTwoDecomposition=pw2, digits_per_limb=dpl if pw2 else None)
    return [Ciphertext(g(2 * k), g(2 * k + 1)) for k in range(n)]


def NewCiphertext(ringQ, ringP, levelQ, levelP, BaseTwoDecomposition=0, n=1):
    """rgsw.NewCiphertext (core/rgsw/elements.go:27-40): a zero RGSW ciphertext at (levelQ, levelP); n > 1: a list of n over one device table"""
    from .ringhip import DevicePoly
    from .keygen import digits_per_limb
    if ringQ.kind != 0 or (ringP is not None and ringP.kind != 0):
        raise RingHipError("rgsw.NewCiphertext: standard rings only (3N and conjugate-invariant rings are not supported)")
    pw2 = int(BaseTwoDecomposition)
    if not 0 <= levelQ < ringQ.L or not -1 <= levelP < (ringP.L if ringP is not None else 0):
        raise RingHipError("rgsw.NewCiphertext: levelQ %d or levelP %d out of range" % (levelQ, levelP))
    dpl = digits_per_limb([int(q) for q in ringQ.moduli], levelQ, levelP, pw2)
    rows = sum(dpl)
    rq = ringQ.AtLevel(levelQ)
    rp = ringP.AtLevel(levelP) if levelP >= 0 else None
    tabQ = DevicePoly(rq, 4 * n * rows, levelQ + 1)
    rq.vec_op("ZERO", None, None, tabQ)
    tabP = None
    if rp is not None:
        tabP = DevicePoly(rp, 4 * n * rows, levelP + 1)
        rp.vec_op("ZERO", None, None, tabP)
    out = _ciphertexts(ringQ, ringP, tabQ, tabP, n, rows, levelQ, levelP, pw2, dpl)
    return out[0] if n == 1 else out


class Encryptor:
    """rgsw.Encryptor (core/rgsw/encryptor.go:12-23), built like rlwe.Encryptor; secret-key encryption only, as in the reference.  Every row of both
    gadget ciphertexts is an encryption of zero (EncryptZero :72-118); Encrypt (:25-70) then adds pt w to component 0 of Value[0] and to component
    1 of Value[1] (AddPolyTimesGadgetVectorToGadgetCiphertext), the plaintext brought to the NTT domain and to Montgomery form first (:44-57).
    All rows of a call -- of one ciphertext or of a list -- are one launch sequence (KeyGenerator.gadget_rows with rh_rgsw_encrypt, or the
    composed ring calls: FUSED_KEYGEN["rgsw_encrypt"], fused=).  samples: {"a": (aQ, aP or None), "e"}: per ciphertext the rows of Value[0], then
    those of Value[1]."""

    def __init__(self, ringQ, ringP=None, key=None, prng=None, xs=("P", 2 / 3), xe=(3.2, 19)):
        from .keygen import KeyGenerator, PublicKey, SecretKey
        if isinstance(key, PublicKey):
            raise RingHipError("rgsw.Encryptor: public-key encryption is not supported (core/rgsw/encryptor.go:18-19: only secret-key encryption)")
        if key is not None and not isinstance(key, SecretKey):
            raise RingHipError("rgsw.Encryptor: invalid key type, want SecretKey or None")
        if ringQ.kind != 0 or (ringP is not None and ringP.kind != 0):
            raise RingHipError("rgsw.Encryptor: standard rings only (3N and conjugate-invariant rings are not supported)")
        self.ringQ, self.ringP, self.key = ringQ, ringP, key
        self.kg = KeyGenerator(ringQ, ringP, xs, xe, prng)

    def EncryptZero(self, ct, samples=None, fused=None):
        self.Encrypt(None, ct, samples, fused)

    def rows(self, ptQ, index, levelQ, levelP, pw2, samples=None, fused=None):
        """len(index) fresh RGSW ciphertexts of the plaintexts ptQ[index[k]] (negative: zero) as one launch sequence -> list of rgsw.Ciphertext"""
        if self.key is None:
            raise RingHipError("cannot encrypt: Encryptor has no encryption key")
        sq, sp = self.kg._sk_rows(self.key, levelQ, levelP)
        tabQ, tabP, rows, dpl = self.kg.gadget_rows(None, sq, sp, levelQ, levelP, pw2, 2 * len(index), samples=samples, fused=fused, rgsw=(ptQ, list(index)))
        return _ciphertexts(self.ringQ, self.ringP, tabQ, tabP, len(index), rows, levelQ, levelP, pw2, dpl)

    def Encrypt(self, pt, ct, samples=None, fused=None):
        """ct: an rgsw.Ciphertext, or a list of them with a plaintext batch of as many polys (or of one, for all)"""
        from .keygen import _pt_poly
        cts = list(ct) if isinstance(ct, (list, tuple)) else [ct]
        for c in cts:
            if not isinstance(c, Ciphertext):
                raise RingHipError("rgsw.Encryptor: an rgsw.Ciphertext (rlwe ciphertexts go to rlwe.Encryptor)")
        g0 = cts[0].Value[0]
        levelQ, levelP, pw2 = g0.LevelQ(), g0.LevelP(), g0.BaseTwoDecomposition
        if any((c.LevelQ(), c.LevelP(), c.Value[0].BaseTwoDecomposition, c.Value[0].digits) != (levelQ, levelP, pw2, g0.digits) for c in cts):
            raise RingHipError("rgsw.Encryptor: the ciphertexts of a call share their levels and decomposition")
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        ptQ, index = None, [-1] * len(cts)
        if pt is not None:
            src = _pt_poly(pt)
            if src.limbs < levelQ + 1 or src.npoly not in (1, len(cts)):
                raise RingHipError("rgsw.Encryptor: the plaintext has fewer limbs than the ciphertext's level, or a batch of another size")
            ptQ = rq.NewPoly(src.npoly)
            if not pt.IsNTT:                                           # (:44-57)
                rq.NTT(src, ptQ)
                if not getattr(pt, "IsMontgomery", False):
                    rq.MForm(ptQ, ptQ)
            elif not getattr(pt, "IsMontgomery", False):
                rq.MForm(src, ptQ)
            else:
                rq.CopyLvl(src, ptQ)
            index = [k if src.npoly > 1 else 0 for k in range(len(cts))]
        new = self.rows(ptQ, index, levelQ, levelP, pw2, samples, fused)
        for c, n in zip(cts, new):
            for k in (0, 1):
                rq.CopyLvl(n.Value[k].Q, c.Value[k].Q)
                if rp is not None:
                    rp.CopyLvl(n.Value[k].P, c.Value[k].P)

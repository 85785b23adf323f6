"""Keys and ciphertexts made on the device: core/rlwe/keygenerator.go, encryptor.go and decryptor.go over the samplers of sampling.py.

  SecretKey, PublicKey, EvaluationKey, RelinearizationKey, GaloisKey, MemEvaluationKeySet     core/rlwe/keys.go
  KeyGenerator    GenSecretKey(New) :39-72, GenSecretKeyWithHammingWeight(New) :43-58, GenPublicKey(New) :74-90, GenKeyPairNew :92-98,
                  GenEvaluationKey(New) :230-274 (also between ring degrees), GenRelinearizationKey(New) :100-120, GenGaloisKey(New) :122-174,
                  GenGaloisKeys(New) :176-205 -- all keys of a call in one launch sequence
  Encryptor       Encrypt(New), EncryptZero(New), WithKey, WithPRNG: encryptor.go:148-216; secret key :355-460, public key :218-350
  Decryptor       Decrypt(New): decryptor.go:42-90

Every arithmetic entry takes `samples=` in place of the PRNG: the uniform block(s) and the int32 error / ternary rows as host arrays; that is
how it is pinned bit for bit (tests/keygen_restatement.py).  FUSED_KEYGEN selects the kernels of csrc/keygen.hip (rh_rlwe_gadget_encrypt,
rh_rlwe_encrypt_sk, rh_rlwe_mul_pk, rh_rlwe_decrypt) or the composed ring calls of the reference: the same bits either way.
gadget_rows also serves rgsw.Encryptor: the rows of many RGSW ciphertexts under one secret, rh_rgsw_encrypt or the composed calls
(FUSED_KEYGEN["rgsw_encrypt"]).

Rings: standard rings, and 3N rings (kind Matrix3N) whose degree is a multiple of 8; ringQ and ringP of the same kind.  On a 3N ring every
NTT-domain block this module stores or hands out -- SecretKey.Value, public and evaluation keys, the ciphertexts Encrypt writes -- is in the
REFERENCE's order (ring/ntt_3n.go:82-109), which is what the key-switch kernels read, whatever Ring.ntt3n_layout says: the transforms of this
module run with the ring's layout switched to the reference's order (reference_order below), a block-order plaintext or ciphertext that comes in
is converted with Ring.ToReferenceOrder first, and every block written carries the tag of what it holds (DevicePoly.layout = None).

The error law: xe = (sigma, bound), the discrete Gaussian, or ("P", density) / ("H", weight), a ternary law through TernarySampler (the
reference's Matrix CKKS test parameters use Xe = ring.Ternary{H: 1}; ring.NewSampler takes any law).

Conjugate-invariant rings: behind the permit conjugate_invariant=True (sampling.rings_ok), which ckks.Parameters' factories set; the Galois
elements are then taken modulo NthRoot = 4N.  GenEvaluationKeysForRingSwapNew (:207-228) is called on the standard ring's generator.

Not built, refused by name: compressed (seeded) keys, conjugate-invariant rings without the permit, 3N degrees that are no multiple of 8, Galois keys on 3N rings, the big-norm Gaussian, a plaintext and a ciphertext in
different domains or allocated at different levels."""
import functools

import numpy as np

from .ringhip import BasisExtender, ConjugateInvariant, DevicePoly, Matrix3N, RingHipError, Standard, U64P, _check, lib
from .rlwe import ElementQP, GadgetCiphertext, PolyQP
from .sampling import GaussianSampler, NewPRNG, SmallPoly, TernarySampler, UniformSampler, lift_small, rings_ok
from .schemes import Ciphertext

class _KeygenSwitches(dict):
    """FUSED_KEYGEN: its truth value is the switch of the kernels of csrc/keygen.hip that every entry of this module reads ("kernels");
    ["rgsw_encrypt"]: rh_rgsw_encrypt (True) or the composed ring calls (False) for the rows of RGSW ciphertexts"""

    def __bool__(self):
        return bool(self["kernels"])


# the kernels of csrc/keygen.hip (True) or the composed ring calls (False); the measured choice: profiles/keygen.json.  rgsw_encrypt: one launch for
# every row against three ring calls per row and limb set; not measured on its own yet, it follows the choice of rh_rlwe_gadget_encrypt, whose
# row sequence it shares
FUSED_KEYGEN = _KeygenSwitches(kernels=True, rgsw_encrypt=True)
SCRATCH_CAP = 1 << 30        # bytes of error scratch (int32 samples + their residues under Q and P) one chunk of a batched key generation may hold


def _fused(fused):
    return bool(FUSED_KEYGEN) if fused is None else bool(fused)


def _fused_rgsw(fused):
    if fused is not None:
        return bool(fused)
    return bool(FUSED_KEYGEN["rgsw_encrypt"]) if isinstance(FUSED_KEYGEN, dict) else bool(FUSED_KEYGEN)


def centred_coeffs(sk):
    """the small coefficients of a secret key as int64: its int32 row when it carries one, else INTT and IMForm of limb 0 centred at q_0 >> 1
    (`coeff > QHalf` is negative, core/rlwe/utils.go:266-275): one N-word download"""
    ring = sk.Value.Q.ring
    if sk.coeffs is not None:
        return np.asarray(sk.coeffs.numpy(), dtype=np.int64).reshape(-1)[:ring.N]
    r0 = ring.AtLevel(0)
    t = r0.NewPoly(1)
    r0.INTT(DevicePoly(r0, 1, 1, ptr=sk.Value.Q.ptr, owner=sk.Value.Q), t)
    r0.IMForm(t, t)
    x = t.numpy()[0, 0]
    q0 = int(ring.moduli[0])
    return np.where(x > np.uint64(q0 >> 1), x.astype(np.int64) - np.int64(q0), x.astype(np.int64))


def _view(p, ring, first, count, limbs=None):
    """polys [first, first + count) of a block as a block of their own"""
    limbs = p.limbs if limbs is None else limbs
    return DevicePoly(ring, count, limbs, ptr=p.ptr + first * p.limbs * ring.N * 8, owner=p)


def _standard(*rings):
    for r in rings:
        if r is not None and r.kind != Standard:
            raise RingHipError("keygen: standard rings only (3N and conjugate-invariant rings are not supported)")


def reference_order(method):
    """3N rings: run `method` of an object with ringQ (and ringP) with Ring.NTT writing the reference's order, and put the rings' layout back"""
    @functools.wraps(method)
    def run(self, *args, **kw):
        rings = [r for r in (self.ringQ, getattr(self, "ringP", None)) if r is not None and r.kind == Matrix3N and r.ntt3n_layout is not None]
        saved = [r.ntt3n_layout for r in rings]
        for r in rings:
            r.ntt3n_layout = None
        try:
            return method(self, *args, **kw)
        finally:
            for r, lay in zip(rings, saved):
                r.ntt3n_layout = lay
    return run


def error_sampler(prng, ring, xe, conjugate_invariant=False):
    """the sampler of the error law xe: (sigma, bound), or ("P", density) / ("H", weight)"""
    if isinstance(xe[0], str):
        if xe[0] not in ("P", "H") or len(xe) != 2:
            raise RingHipError("the error law is (sigma, bound), (\"P\", density) or (\"H\", weight)")
        return TernarySampler(prng, ring, conjugate_invariant=conjugate_invariant, **{xe[0]: xe[1]})
    return GaussianSampler(prng, ring, *xe, conjugate_invariant=conjugate_invariant)


class Plaintext:
    """rlwe.Plaintext as far as encryption reads it: Value (a DevicePoly batch), IsNTT and the scheme metadata"""

    def __init__(self, value, is_ntt=True, **meta):
        self.Value, self.IsNTT = value, bool(is_ntt)
        for k, v in meta.items():
            setattr(self, k, v)

    def Level(self):
        return self.Value.limbs - 1

    def Degree(self):
        return 0


def _pt_poly(pt):
    """the poly block of a plaintext: rlwe.Plaintext holds it as Value, the scheme packages' plaintexts as Value[0]"""
    return pt.Value[0] if isinstance(pt.Value, (list, tuple)) else pt.Value


class SecretKey:
    """rlwe.SecretKey: the int32 coefficients (coeffs, a SmallPoly of one poly) and Value = PolyQP(Q, P), the residues under every limb of Q and
    of P in the NTT domain and in Montgomery form (keygenerator.go:60-72)"""

    def __init__(self, coeffs, Q, P):
        self.coeffs, self.Value = coeffs, PolyQP(Q, P)

    def LevelQ(self):
        return self.Value.Q.limbs - 1

    def LevelP(self):
        return self.Value.P.limbs - 1 if self.Value.P is not None else -1


class PublicKey:
    """rlwe.PublicKey: Value[0] = -a s + e, Value[1] = a modulo QP, NTT domain, Montgomery form.  Held as one gadget row, (1, 2, limbs, N)."""

    def __init__(self, ringQ, ringP, Q, P):
        self.Q, self.P = Q, P
        self.Value = [PolyQP(_view(Q, ringQ, c, 1), _view(P, ringP, c, 1) if P is not None else None) for c in (0, 1)]

    def LevelQ(self):
        return self.Q.limbs - 1

    def LevelP(self):
        return self.P.limbs - 1 if self.P is not None else -1


class EvaluationKey(GadgetCiphertext):
    """rlwe.EvaluationKey: a GadgetCiphertext built from device tables (GadgetCiphertext.from_device); every evaluator takes it as it is"""


class RelinearizationKey(EvaluationKey):
    pass


class GaloisKey(EvaluationKey):
    GaloisElement, NthRoot = 0, 0


class MemEvaluationKeySet:
    """rlwe.MemEvaluationKeySet: the relinearisation key and the Galois keys; `galois_keys` is the dict the evaluators take"""

    def __init__(self, rlk=None, galois_keys=()):
        self.RelinearizationKey = rlk
        self.GaloisKeys = {int(k.GaloisElement): k for k in galois_keys}

    @property
    def galois_keys(self):
        out = dict(self.GaloisKeys)
        if self.RelinearizationKey is not None:
            out["rlk"] = self.RelinearizationKey
        return out

    def GetGaloisKey(self, galEl):
        if galEl not in self.GaloisKeys:
            raise RingHipError("GaloisKey[%d] is nil" % galEl)
        return self.GaloisKeys[galEl]

    def GetRelinearizationKey(self):
        if self.RelinearizationKey is None:
            raise RingHipError("RelinearizationKey is nil")
        return self.RelinearizationKey

    def GetGaloisKeysList(self):
        return sorted(self.GaloisKeys)


def digits_per_limb(Q, levelQ, levelP, pw2):
    """Parameters.BaseTwoDecompositionVectorSize (core/rlwe/params.go:613-632) over the RNS digits (:634-642)"""
    n = levelQ + 1 if levelP == -1 else (levelQ + levelP + 1) // (levelP + 1)
    if pw2 == 0 or levelP > 0:
        return [1] * n
    import math
    return [(int(round(math.log2(float(int(q))))) + pw2 - 1) // pw2 for q in Q[:n]]


def gadget_row_table(Q, P, levelQ, levelP, pw2, dpl, key=0):
    """the per-(row, limb) scalars of AddPolyTimesGadgetVectorToGadgetCiphertext (core/rlwe/gadgetciphertext.go:172-241) as rows of
    rh_rlwe_gadget_encrypt's table: [key, s_0 .. s_levelQ], s = MForm(P 2^(j pw2)) on the limbs i (levelP + 1) + k of digit i that exist at
    levelQ (the `index >= levelQ + 1` break where #P does not divide #Q), 0 elsewhere; without P the factor is 1 and a digit is one limb."""
    Pb = 1
    for p in P[:levelP + 1]:
        Pb *= int(p)
    width = max(levelP, 0) + 1
    rows = []
    for i in range(len(dpl)):
        for j in range(dpl[i]):
            f = Pb << (j * pw2)
            row = [key] + [0] * (levelQ + 1)
            for k in range(width):
                index = i * width + k
                if index >= levelQ + 1:
                    break
                row[1 + index] = (f << 64) % int(Q[index])
            rows.append(row)
    return rows


class KeyGenerator:
    """rlwe.KeyGenerator over (ringQ, ringP): ringP None for parameters without P.  xs: ("P", density) or ("H", weight); xe: (sigma, bound)."""

    def __init__(self, ringQ, ringP=None, xs=("P", 2 / 3), xe=(3.2, 19), prng=None, conjugate_invariant=False):
        rings_ok("KeyGenerator", ringQ, ringP, conjugate_invariant)
        self._ci = bool(conjugate_invariant)
        if ringP is not None and ringP.N != ringQ.N:
            raise RingHipError("KeyGenerator: ringQ and ringP differ in degree")
        self.ringQ, self.ringP = ringQ, ringP
        self.prng = NewPRNG() if prng is None else prng
        self.xs, self.xe = tuple(xs), tuple(xe)
        self.uniform = UniformSampler(self.prng, ringQ, ringP, conjugate_invariant=self._ci)
        self.gauss = error_sampler(self.prng, ringQ, self.xe, self._ci)
        self.Q, self.P = [int(q) for q in ringQ.moduli], [int(p) for p in ringP.moduli] if ringP is not None else []

    # ---- secret keys ------------------------------------------------------------------------------------------------------------------------
    @reference_order
    def _secret_from(self, small):
        """genSecretKeyFromSampler (:60-72): lift under QP, NTT, MForm"""
        rq, rp = self.ringQ, self.ringP
        q = rq.NewPoly(1)
        p = rp.NewPoly(1) if rp is not None else None
        lift_small(rq, rp, small, q, p)
        rq.NTT(q, q); rq.MForm(q, q)
        if p is not None:
            rp.NTT(p, p); rp.MForm(p, p)
        return SecretKey(small, q, p)

    def GenSecretKeyNew(self, samples=None):
        """samples: the N int32 coefficients"""
        if samples is not None:
            return self._secret_from(SmallPoly.from_numpy(self.ringQ, np.asarray(samples, dtype=np.int32).reshape(1, -1)))
        kind, v = self.xs
        return self._secret_from(TernarySampler(self.prng, self.ringQ, conjugate_invariant=self._ci, **{kind: v}).ReadNew(1))

    def GenSecretKeyWithHammingWeightNew(self, hw):
        return self._secret_from(TernarySampler(self.prng, self.ringQ, H=int(hw), conjugate_invariant=self._ci).ReadNew(1))

    def GenSecretKey(self, sk, samples=None):
        new = self.GenSecretKeyNew(samples)
        sk.coeffs, sk.Value = new.coeffs, new.Value

    def GenSecretKeyWithHammingWeight(self, hw, sk):
        new = self.GenSecretKeyWithHammingWeightNew(hw)
        sk.coeffs, sk.Value = new.coeffs, new.Value

    # ---- the rows of gadget ciphertexts ----------------------------------------------------------------------------------------------------
    def _levels(self, levelQ, levelP, BaseTwoDecomposition, compressed):
        """ResolveEvaluationKeyParameters (core/rlwe/keys.go): the parameters' maxima unless told"""
        if compressed:
            raise RingHipError("compressed (seeded) evaluation keys are not built on the device path")
        levelQ = self.ringQ.L - 1 if levelQ is None else int(levelQ)
        levelP = (self.ringP.L - 1 if self.ringP is not None else -1) if levelP is None else int(levelP)
        if not 0 <= levelQ < self.ringQ.L or not -1 <= levelP < (self.ringP.L if self.ringP is not None else 0):
            raise RingHipError("evaluation key parameters: levelQ %d or levelP %d out of range" % (levelQ, levelP))
        return levelQ, levelP, int(BaseTwoDecomposition)

    @reference_order
    def gadget_rows(self, skIn, skOutQ, skOutP, levelQ, levelP, pw2, nkeys, plaintext=True, samples=None, fused=None, dpl=None, rgsw=None):
        """`nkeys` gadget ciphertexts at (levelQ, levelP) in one launch sequence (genEvaluationKey :276-316 for each): one uniform Read for every a,
        written straight into component 1 of the tables; one Gaussian Read, one lift and one NTT over every error row; one rh_rlwe_gadget_encrypt
        with the per-row key index.  skIn: (1 or nkeys, levelQ + 1, N) -- one input key for all (Galois keys) or one per key; skOutQ / skOutP:
        (nkeys, limbs, N); all NTT domain, Montgomery form.  plaintext=False: encryptions of zero (a public key is one such row).
        Chunked over keys so that the error scratch stays under SCRATCH_CAP.  samples: {"a": (aQ, aP or None), "e": int32} with aQ
        (nkeys * rows, levelQ + 1, N), aP (nkeys * rows, levelP + 1, N), e (nkeys * rows, N), key-major.
        rgsw=(ptQ, index): the gadget ciphertexts are the halves of nkeys / 2 RGSW ciphertexts under the ONE secret skOutQ / skOutP (gadget 2 k is
        Value[0] of ciphertext k, gadget 2 k + 1 its Value[1]); ptQ: (npt, levelQ + 1, N) plaintexts, NTT domain, Montgomery form; index[k]: the
        plaintext of ciphertext k, negative for an encryption of zero; skIn is not read (rh_rgsw_encrypt, or the composed calls).
        Returns (tabQ, tabP, rows, dpl): tables of (nkeys * rows * 2, limbs, N)."""
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        LQ, LP, N = levelQ + 1, levelP + 1, rq.N
        dpl = digits_per_limb(self.Q, levelQ, levelP, pw2) if dpl is None else dpl
        rows = sum(dpl)
        R = nkeys * rows
        tabQ = DevicePoly(rq, 2 * R, LQ)
        tabP = DevicePoly(rp, 2 * R, LP) if rp is not None else None
        one = gadget_row_table(self.Q, self.P, levelQ, levelP, pw2, dpl) if plaintext else [[0] * (LQ + 1) for _ in range(rows)]
        if samples is None:
            call_a, call_e = self.prng.next_call(), self.prng.next_call()
        else:
            aQ, aP = samples["a"]
            full = np.zeros((R, 2, LQ, N), dtype=np.uint64)
            full[:, 1] = np.asarray(aQ, dtype=np.uint64).reshape(R, LQ, N)
            _check(lib().rh_dev_upload(rq._h, tabQ.ptr, full.ctypes.data_as(U64P), full.size))
            if rp is not None:
                full = np.zeros((R, 2, LP, N), dtype=np.uint64)
                full[:, 1] = np.asarray(aP, dtype=np.uint64).reshape(R, LP, N)
                _check(lib().rh_dev_upload(rp._h, tabP.ptr, full.ctypes.data_as(U64P), full.size))
            e_all = np.asarray(samples["e"], dtype=np.int32).reshape(R, N)
        per_key = rows * N * (4 + 8 * (LQ + LP))
        step = max(1, min(nkeys, SCRATCH_CAP // per_key))
        scratch = None
        for k0 in range(0, nkeys, step):
            kc = min(step, nkeys - k0)
            r0, rc = k0 * rows, kc * rows
            tq = _view(tabQ, rq, 2 * r0, 2 * rc)
            tp = _view(tabP, rp, 2 * r0, 2 * rc) if rp is not None else None
            if scratch is None or scratch[0].npoly != rc:
                scratch = (SmallPoly(rq, rc), DevicePoly(rq, rc, LQ), DevicePoly(rp, rc, LP) if rp is not None else None,
                           DevicePoly(rq.AtLevel(0), (rc * (LQ + 2) + N - 1) // N + 1, 1))
            small, eQ, eP, table = scratch
            if samples is None:
                self.uniform.read_rows(rq, tq.ptr + LQ * N * 8, 2 * LQ, rc, call_a, poly0=r0, row0=0)
                if rp is not None:
                    self.uniform.read_rows(rp, tp.ptr + LP * N * 8, 2 * LP, rc, call_a, poly0=r0, row0=LQ)
                self.gauss.Read(small, call=call_e, poly0=r0)
            else:
                small.upload(e_all[r0:r0 + rc])
            lift_small(rq, rp, small, eQ, eP)
            rq.NTT(eQ, eQ)
            if rp is not None:
                rp.NTT(eP, eP)
            if rgsw is not None:
                ptQ, index = rgsw
                if _fused_rgsw(fused):
                    rt = np.array([[max(index[k // 2], 0), k & 1] + (row[1:] if index[k // 2] >= 0 else [0] * LQ) for k in range(k0, k0 + kc) for row in one],
                                  dtype=np.uint64)
                    _check(lib().rh_rgsw_encrypt(rq._h, rp._h if rp is not None else None, levelQ, levelP, eQ.ptr, eP.ptr if eP is not None else None,
                                                 tq.ptr, tp.ptr if tp is not None else None, skOutQ.ptr, skOutP.ptr if skOutP is not None else None,
                                                 ptQ.ptr if ptQ is not None else None, ptQ.npoly if ptQ is not None else 0,
                                                 rt.ctypes.data_as(U64P), rc, table.ptr, table.words))
                else:
                    self._rows_composed_rgsw(rq, rp, tq, tp, eQ, eP, skOutQ, skOutP, ptQ, index, k0, kc, rows, one)
            elif _fused(fused):
                rt = np.array([[k] + row[1:] for k in range(k0, k0 + kc) for row in one], dtype=np.uint64)
                _check(lib().rh_rlwe_gadget_encrypt(rq._h, rp._h if rp is not None else None, levelQ, levelP, eQ.ptr, eP.ptr if eP is not None else None,
                                                    tq.ptr, tp.ptr if tp is not None else None, skOutQ.ptr, skOutP.ptr if skOutP is not None else None,
                                                    skIn.ptr, nkeys, skIn.npoly, rt.ctypes.data_as(U64P), rc, table.ptr, table.words))
            else:
                self._rows_composed(rq, rp, tq, tp, eQ, eP, skIn, skOutQ, skOutP, k0, kc, rows, one)
        return tabQ, tabP, rows, dpl

    def _rows_composed(self, rq, rp, tq, tp, eQ, eP, skIn, skOutQ, skOutP, k0, kc, rows, one):
        """the reference's calls per row: MForm, MulCoeffsMontgomeryThenSub (encryptor.go:449-452), MulScalarMontgomeryThenAdd on the digit limbs
        (gadgetciphertext.go:225-230; a zero scalar adds nothing)"""
        LQ = rq.level + 1
        for r in range(kc * rows):
            k = k0 + r // rows
            for ring, tab, e, so in ((rq, tq, eQ, skOutQ), (rp, tp, eP, skOutP)):
                if ring is None:
                    continue
                b, a, er, s = _view(tab, ring, 2 * r, 1), _view(tab, ring, 2 * r + 1, 1), _view(e, ring, r, 1), _view(so, ring, k, 1)
                ring.MForm(er, b)
                ring.MulCoeffsMontgomeryThenSub(a, s, b)
            scal = one[r % rows][1:]
            if any(scal):
                si = _view(skIn, rq, k if skIn.npoly > 1 else 0, 1, LQ)
                rq.vec_op("MUL_SCALAR_MONT_THEN_ADD", si, None, _view(tq, rq, 2 * r, 1), s0=scal)

    def _rows_composed_rgsw(self, rq, rp, tq, tp, eQ, eP, skQ, skP, ptQ, index, k0, kc, rows, one):
        """rgsw.Encryptor's calls per row (core/rgsw/encryptor.go:25-118): the encryption of zero as in _rows_composed, then
        MulScalarMontgomeryThenAdd of the plaintext onto component 0 of a Value[0] row and component 1 of a Value[1] row"""
        LQ = rq.level + 1
        for r in range(kc * rows):
            k = k0 + r // rows
            for ring, tab, e, s in ((rq, tq, eQ, skQ), (rp, tp, eP, skP)):
                if ring is None:
                    continue
                b, a, er = _view(tab, ring, 2 * r, 1), _view(tab, ring, 2 * r + 1, 1), _view(e, ring, r, 1)
                ring.MForm(er, b)
                ring.MulCoeffsMontgomeryThenSub(a, s, b)
            scal = one[r % rows][1:]
            if index[k // 2] >= 0 and any(scal):
                rq.vec_op("MUL_SCALAR_MONT_THEN_ADD", _view(ptQ, rq, index[k // 2], 1, LQ), None, _view(tq, rq, 2 * r + (k & 1), 1), s0=scal)

    def _sk_rows(self, sk, levelQ, levelP):
        """views of sk's leading limbs (a single poly's leading limbs are contiguous)"""
        if sk.LevelQ() < levelQ or sk.LevelP() < levelP:
            raise RingHipError("the secret key has fewer limbs than the key's level")
        q = DevicePoly(self.ringQ.AtLevel(levelQ), 1, levelQ + 1, ptr=sk.Value.Q.ptr, owner=sk.Value.Q)
        p = DevicePoly(self.ringP.AtLevel(levelP), 1, levelP + 1, ptr=sk.Value.P.ptr, owner=sk.Value.P) if levelP >= 0 else None
        return q, p

    @reference_order
    def _mapped_secret(self, sk, levelQ, levelP):
        """The secret of a ring of smaller degree n as (Q rows, P rows) of this generator's ring, NTT domain, Montgomery form (:262-272):
        ring.MapSmallDimensionToLargerDimensionNTT (Y = X^(N/n)) and ExtendBasisSmallNormAndCenterNTTMontgomery (core/rlwe/utils.go:250-284) restated
        on the small coefficients: INTT and IMForm of limb 0, centred around q_0 / 2 (the key's int32 coefficients when it carries them: the same
        numbers), placed at every (N/n)-th coefficient, lifted under limbs 0..levelQ of Q and 0..levelP of P (rh_small_lift), NTT, MForm.  The
        canonical residues of s(X^(N/n)) under every limb: for the limbs of Q the small key holds, the repetition of its NTT rows gives the same
        words, because both rings take psi from the same generator of q (rlwe._small_ntt).  The small ring's own P is never read; its moduli
        must be a prefix of this ring's Q."""
        small = sk.Value.Q.ring
        _standard(self.ringQ, self.ringP, small)
        n, N = small.N, self.ringQ.N
        if n >= N:
            raise RingHipError("cannot GenEvaluationKey: evaluation keys between ring degrees (N != n) are made by the key generator of the larger degree")
        mods = [int(q) for q in small.moduli]
        if mods != self.Q[:len(mods)]:
            raise RingHipError("cannot GenEvaluationKey: the moduli of the ring of smaller degree must be a prefix of the moduli Q of the larger ring")
        c = centred_coeffs(sk)
        big = np.zeros((1, N), dtype=np.int32)
        big[0, ::N // n] = c
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        q = rq.NewPoly(1)
        p = rp.NewPoly(1) if rp is not None else None
        lift_small(rq, rp, SmallPoly.from_numpy(self.ringQ, big), q, p)
        rq.NTT(q, q); rq.MForm(q, q)
        if rp is not None:
            rp.NTT(p, p); rp.MForm(p, p)
        return q, p

    def _key(self, cls, tabQ, tabP, first, rows, levelQ, levelP, pw2, dpl):
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        return cls.from_device(rq, rp, _view(tabQ, rq, 2 * first, 2 * rows), _view(tabP, rp, 2 * first, 2 * rows) if rp is not None else None,
                               BaseTwoDecomposition=pw2, digits_per_limb=dpl if pw2 else None)

    # ---- public and evaluation keys -------------------------------------------------------------------------------------------------------
    def GenPublicKeyNew(self, sk, samples=None, fused=None):
        """(:74-90): one encryption of zero modulo QP, NTT domain, Montgomery form.  samples: {"a": (aQ (1, LQ, N), aP), "e": (1, N)}"""
        levelQ, levelP = self.ringQ.L - 1, self.ringP.L - 1 if self.ringP is not None else -1
        sq, sp = self._sk_rows(sk, levelQ, levelP)
        tabQ, tabP, _, _ = self._zero_rows(sq, sp, levelQ, levelP, samples, fused)
        return PublicKey(self.ringQ, self.ringP, tabQ, tabP)

    def _zero_rows(self, sq, sp, levelQ, levelP, samples, fused):
        """one row (-a s + e, a), whatever the digit count of the level"""
        return self.gadget_rows(sq, sq, sp, levelQ, levelP, 0, 1, plaintext=False, samples=samples, fused=fused, dpl=[1])

    def GenPublicKey(self, sk, pk, samples=None, fused=None):
        new = self.GenPublicKeyNew(sk, samples, fused)
        pk.Q, pk.P, pk.Value = new.Q, new.P, new.Value

    def GenKeyPairNew(self):
        sk = self.GenSecretKeyNew()
        return sk, self.GenPublicKeyNew(sk)

    def GenEvaluationKeyNew(self, skInput, skOutput, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False, samples=None, fused=None, cls=EvaluationKey):
        """(:230-274): rows (-a skOut + e + w P skIn, a).  One of the two keys may belong to a ring of smaller degree n: the key is then generated
        in this generator's degree N, with the smaller key mapped to Y = X^(N/n) and extended to this generator's Q and P (_mapped_secret)."""
        levelQ, levelP, pw2 = self._levels(levelQ, levelP, BaseTwoDecomposition, compressed)
        NIn, NOut = skInput.Value.Q.ring.N, skOutput.Value.Q.ring.N
        if max(NIn, NOut) != self.ringQ.N:
            raise RingHipError("cannot GenEvaluationKey: evaluation keys between ring degrees (N != n) are made by the key generator of the larger "
                               "degree (generator: %d, skInput: %d, skOutput: %d)" % (self.ringQ.N, NIn, NOut))
        si = self._mapped_secret(skInput, levelQ, -1)[0] if NIn != self.ringQ.N else self._sk_rows(skInput, levelQ, -1)[0]
        oq, op = self._mapped_secret(skOutput, levelQ, levelP) if NOut != self.ringQ.N else self._sk_rows(skOutput, levelQ, levelP)
        tabQ, tabP, rows, dpl = self.gadget_rows(si, oq, op, levelQ, levelP, pw2, 1, samples=samples, fused=fused)
        return self._key(cls, tabQ, tabP, 0, rows, levelQ, levelP, pw2, dpl)

    def GenEvaluationKey(self, skInput, skOutput, evk, samples=None, fused=None):
        new = self.GenEvaluationKeyNew(skInput, skOutput, evk.levelQ, evk.levelP, evk.BaseTwoDecomposition, samples=samples, fused=fused)
        evk.__dict__.update(new.__dict__)

    def GenRelinearizationKeyNew(self, sk, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False, samples=None, fused=None):
        """(:100-120): skIn = sk^2 (MulCoeffsMontgomery on the rows of Q), skOut = sk"""
        levelQ, levelP, pw2 = self._levels(levelQ, levelP, BaseTwoDecomposition, compressed)
        sq, sp = self._sk_rows(sk, levelQ, levelP)
        rq = self.ringQ.AtLevel(levelQ)
        sk2 = rq.NewPoly(1)
        rq.MulCoeffsMontgomery(sq, sq, sk2)
        tabQ, tabP, rows, dpl = self.gadget_rows(sk2, sq, sp, levelQ, levelP, pw2, 1, samples=samples, fused=fused)
        return self._key(RelinearizationKey, tabQ, tabP, 0, rows, levelQ, levelP, pw2, dpl)

    def GenRelinearizationKey(self, sk, rlk, samples=None, fused=None):
        new = self.GenRelinearizationKeyNew(sk, rlk.levelQ, rlk.levelP, rlk.BaseTwoDecomposition, samples=samples, fused=fused)
        rlk.__dict__.update(new.__dict__)

    def GenGaloisKeysNew(self, galEls, sk, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False, samples=None, fused=None):
        """(:195-205) as ONE launch sequence over all keys: skOut_k = the NTT automorphism of ModInvGaloisElement(g_k) on sk (:150-170), skIn = sk"""
        galEls = [int(g) for g in galEls]
        if self.ringQ.kind == Matrix3N:
            raise RingHipError("cannot GenGaloisKey: 3N rings have no automorphism (ring/automorphism.go:14-20: N must be a power of two)")
        levelQ, levelP, pw2 = self._levels(levelQ, levelP, BaseTwoDecomposition, compressed)
        if not galEls:
            return []
        sq, sp = self._sk_rows(sk, levelQ, levelP)
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        n, N = len(galEls), rq.N
        NthRoot = (4 if rq.kind == ConjugateInvariant else 2) * N          # ring.NthRoot (ring/ring.go:178-183)
        outQ = DevicePoly(rq, n, levelQ + 1)
        outP = DevicePoly(rp, n, levelP + 1) if rp is not None else None
        for k, g in enumerate(galEls):
            if g & 1 == 0:
                raise RingHipError("cannot GenGaloisKey: the Galois element must be odd")
            inv = pow(g, NthRoot - 1, NthRoot)                          # Parameters.ModInvGaloisElement (core/rlwe/params.go:677-681)
            rq.AutomorphismNTT(sq, inv, _view(outQ, rq, k, 1))
            if rp is not None:
                rp.AutomorphismNTT(sp, inv, _view(outP, rp, k, 1))
        tabQ, tabP, rows, dpl = self.gadget_rows(sq, outQ, outP, levelQ, levelP, pw2, n, samples=samples, fused=fused)
        keys = []
        for k, g in enumerate(galEls):
            gk = self._key(GaloisKey, tabQ, tabP, k * rows, rows, levelQ, levelP, pw2, dpl)
            gk.GaloisElement, gk.NthRoot = g, NthRoot
            keys.append(gk)
        return keys

    def GenGaloisKeyNew(self, galEl, sk, **kw):
        return self.GenGaloisKeysNew([galEl], sk, **kw)[0]

    def GenGaloisKey(self, galEl, sk, gk, samples=None, fused=None):
        new = self.GenGaloisKeyNew(galEl, sk, levelQ=gk.levelQ, levelP=gk.levelP, BaseTwoDecomposition=gk.BaseTwoDecomposition, samples=samples, fused=fused)
        gk.__dict__.update(new.__dict__)

    def GenGaloisKeys(self, galEls, sk, gks, samples=None, fused=None):
        if len(galEls) != len(gks):
            raise RingHipError("galEls and gks must have the same length")
        kw = {} if gks[0] is None else dict(levelQ=gks[0].levelQ, levelP=gks[0].levelP, BaseTwoDecomposition=gks[0].BaseTwoDecomposition)
        for i, new in enumerate(self.GenGaloisKeysNew(galEls, sk, samples=samples, fused=fused, **kw)):
            if gks[i] is None:
                gks[i] = new
            else:
                gks[i].__dict__.update(new.__dict__)

    def ring_swap_secret(self, skConjugateInvariant):
        """The conjugate-invariant secret of degree n as a secret of this generator's standard ring of degree 2n (:212-217), from its small
        coefficients s: m[0] = s_0, m[i] = s_i and m[2n - i] = -s_i for 1 <= i < n, m[n] = 0 -- the element s(X + X^-1) of Z[X]/(X^2n + 1) --
        lifted under this ring's Q and P, NTT, MForm.  Its Q rows are UnfoldConjugateInvariantToStandard of the secret's own rows (what the
        reference computes); its P rows are made here because the two parameter sets need not share P."""
        who = "GenEvaluationKeysForRingSwapNew"
        small = skConjugateInvariant.Value.Q.ring
        n = small.N
        if self.ringQ.kind != Standard or small.kind != ConjugateInvariant or self.ringQ.N != 2 * n:
            raise RingHipError("%s: the generator's ring must be the standard ring of degree 2n of a conjugate-invariant secret of degree n "
                               "(generator: degree %d, skConjugateInvariant: degree %d)" % (who, self.ringQ.N, n))
        c = centred_coeffs(skConjugateInvariant)
        m = np.zeros((1, 2 * n), dtype=np.int32)
        m[0, :n] = c
        m[0, n + 1:] = -c[:0:-1]
        return self._secret_from(SmallPoly.from_numpy(self.ringQ, m))

    def GenEvaluationKeysForRingSwapNew(self, skStd, skConjugateInvariant, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False,
                                        samples=None, fused=None):
        """(:207-228), on the standard ring's generator: (stdToci, ciToStd), the keys from skStd to the mapped conjugate-invariant secret
        (ring_swap_secret) and back, both through GenEvaluationKeyNew.  samples: a pair, one entry per key."""
        who = "GenEvaluationKeysForRingSwapNew"
        rs, rc = skStd.Value.Q.ring, skConjugateInvariant.Value.Q.ring
        if rs.kind != Standard or rc.kind != ConjugateInvariant or rs.N != 2 * rc.N or rs.N != self.ringQ.N:
            raise RingHipError("%s: skStd must belong to the generator's standard ring of degree 2n and skConjugateInvariant to a conjugate-invariant "
                               "ring of degree n (generator: %d, skStd: %d, skConjugateInvariant: %d)" % (who, self.ringQ.N, rs.N, rc.N))
        k = min(skStd.LevelQ(), skConjugateInvariant.LevelQ()) + 1
        if [int(q) for q in rc.moduli][:k] != self.Q[:k]:
            raise RingHipError("%s: the two secrets must share the moduli Q" % who)
        if levelQ is None:
            levelQ = k - 1
        if levelQ > k - 1:
            raise RingHipError("%s: levelQ %d above the secrets' common level %d" % (who, levelQ, k - 1))
        mapped = self.ring_swap_secret(skConjugateInvariant)
        sa, sb = samples if samples is not None else (None, None)
        kw = dict(levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=BaseTwoDecomposition, compressed=compressed, fused=fused)
        return self.GenEvaluationKeyNew(skStd, mapped, samples=sa, **kw), self.GenEvaluationKeyNew(mapped, skStd, samples=sb, **kw)


class Encryptor:
    """rlwe.Encryptor: `key` a SecretKey or a PublicKey.  Ciphertexts are batches (one Ciphertext whose polys hold npoly ciphertexts): one sampler
    Read per batch, the ciphertext's index within the batch in the substream id."""

    def __init__(self, ringQ, ringP=None, key=None, prng=None, xs=("P", 2 / 3), xe=(3.2, 19), conjugate_invariant=False):
        rings_ok("Encryptor", ringQ, ringP, conjugate_invariant)
        self._ci = bool(conjugate_invariant)
        self.ringQ, self.ringP, self.key = ringQ, ringP, key
        self.xs, self.xe = tuple(xs), tuple(xe)
        self._set_prng(NewPRNG() if prng is None else prng)
        self.be = BasisExtender(ringQ, ringP) if ringP is not None else None

    def _set_prng(self, prng):
        self.prng = prng
        self.uniform = UniformSampler(prng, self.ringQ, self.ringP, conjugate_invariant=self._ci)
        self.gauss = error_sampler(prng, self.ringQ, self.xe, self._ci)
        self.ternary = TernarySampler(prng, self.ringQ, conjugate_invariant=self._ci, **{self.xs[0]: self.xs[1]})

    def _copy(self):
        new = object.__new__(type(self))                                   # a ckks.Encryptor stays one
        new.__dict__.update(self.__dict__)
        return new

    def WithKey(self, key):
        if key is not None and not isinstance(key, (SecretKey, PublicKey)):
            raise RingHipError("invalid key type, want SecretKey, PublicKey or None")
        new = self._copy()
        if key is not None:
            new.key = key
        return new

    def WithPRNG(self, prng):
        new = self._copy()
        new._set_prng(prng)
        return new

    # ---- the sampled rows --------------------------------------------------------------------------------------------------------------------
    def _small(self, sampler, npoly, given):
        if given is not None:
            return SmallPoly.from_numpy(self.ringQ, np.asarray(given, dtype=np.int32).reshape(npoly, self.ringQ.N))
        return sampler.ReadNew(npoly)

    def _error_ntt(self, rq, npoly, given):
        """NTT of the lifted error under Q (:410-412)"""
        e = rq.NewPoly(npoly)
        lift_small(rq, None, self._small(self.gauss, npoly, given), e)
        rq.NTT(e, e)
        return e

    # ---- Encrypt / EncryptZero ------------------------------------------------------------------------------------------------------------
    def EncryptZero(self, ct, samples=None, fused=None):
        self._encrypt(None, ct, samples, fused)

    def EncryptZeroNew(self, level, npoly=1, is_ntt=True, samples=None, fused=None):
        rq = self.ringQ.AtLevel(level)
        ct = Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=is_ntt)
        self._encrypt(None, ct, samples, fused)
        return ct

    def Encrypt(self, pt, ct, samples=None, fused=None):
        """(:148-166): the ciphertext takes the plaintext's metadata.  The reference works at the minimum of the two levels and resizes the ciphertext;
        a device batch is strided by its limb count, so the ciphertext must be allocated at the plaintext's level (refused by name otherwise)"""
        if pt is None:
            return self.EncryptZero(ct, samples, fused)
        for name in ("Scale", "LogDimensions", "IsBatched", "IsMontgomery"):
            if hasattr(pt, name):
                setattr(ct, name, getattr(pt, name))
        ct.IsNTT = pt.IsNTT                                                # *ct.MetaData = *pt.MetaData
        self._encrypt(pt, ct, samples, fused)

    def EncryptNew(self, pt, samples=None, fused=None):
        rq = self.ringQ.AtLevel(pt.Level())
        npoly = _pt_poly(pt).npoly
        ct = Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=pt.IsNTT)
        self.Encrypt(pt, ct, samples, fused)
        return ct

    @reference_order
    def _encrypt(self, pt, ct, samples, fused):
        if self.key is None:
            raise RingHipError("cannot encrypt: Encryptor has no encryption key")
        if isinstance(ct, ElementQP):
            return self._zero_qp(ct, samples, fused)
        if self.ringQ.kind == Matrix3N:
            for v in ct.Value:
                v.layout = None                                            # written whole below, in the reference's order: a stale tag must not steer an INTT
            if pt is not None and pt.IsNTT:
                self.ringQ.ToReferenceOrder(_pt_poly(pt))
        if ct.Degree() != 1:
            raise RingHipError("cannot encrypt: the device path takes ciphertexts of degree 1")
        level = ct.Level()
        if pt is not None and (pt.Level() != level or _pt_poly(pt).npoly != ct.Value[0].npoly):
            raise RingHipError("cannot Encrypt: allocate the ciphertext at the plaintext's level and batch size")
        if pt is not None and pt.IsNTT != ct.IsNTT:
            raise RingHipError("cannot Encrypt: plaintext and ciphertext in different domains are not supported by the device path")
        if isinstance(self.key, SecretKey):
            self._sk(pt, ct, level, samples or {}, _fused(fused))
        elif self.ringP is not None:
            self._pk(pt, ct, level, samples or {}, _fused(fused))
        else:
            self._pk_no_p(pt, ct, level, samples or {}, _fused(fused))

    def _sk(self, pt, ct, level, samples, fused):
        """encryptZeroSk (:355-424) + addPtToCt (:512-530).  samples: {"c1": (npoly, level + 1, N), "e": (npoly, N)}"""
        rq = self.ringQ.AtLevel(level)
        c0, c1 = ct.Value
        npoly, L = c0.npoly, level + 1
        if self.key.LevelQ() < level:
            raise RingHipError("the secret key has fewer limbs than the ciphertext's level")
        sk = DevicePoly(rq, 1, L, ptr=self.key.Value.Q.ptr, owner=self.key.Value.Q)
        if "c1" in samples:
            a = np.ascontiguousarray(np.asarray(samples["c1"], dtype=np.uint64).reshape(npoly, L, rq.N))
            _check(lib().rh_dev_upload(rq._h, c1.ptr, a.ctypes.data_as(U64P), a.size))
        else:
            self.uniform.Read(c1)
        if ct.IsNTT:
            e = self._error_ntt(rq, npoly, samples.get("e"))
            if fused:
                _check(lib().rh_rlwe_encrypt_sk(rq._h, level, c1.ptr, sk.ptr, e.ptr, _pt_poly(pt).ptr if pt is not None else None, c0.ptr, npoly))
            else:
                for k in range(npoly):
                    v = _view(c0, rq, k, 1)
                    rq.MulCoeffsMontgomery(_view(c1, rq, k, 1), sk, v)
                    rq.Neg(v, v)
                rq.Add(c0, e, c0)
                if pt is not None:
                    rq.Add(c0, _pt_poly(pt), c0)
            return
        rq.NTT(c1, c1)                                                     # (:369-371)
        if fused:
            _check(lib().rh_rlwe_encrypt_sk(rq._h, level, c1.ptr, sk.ptr, None, None, c0.ptr, npoly))
        else:
            for k in range(npoly):
                v = _view(c0, rq, k, 1)
                rq.MulCoeffsMontgomery(_view(c1, rq, k, 1), sk, v)
                rq.Neg(v, v)
        rq.INTT(c0, c0)                                                    # (:415-420)
        rq.INTT(c1, c1)
        lift_small(rq, None, self._small(self.gauss, npoly, samples.get("e")), c0, accumulate=True)
        if pt is not None:
            rq.Add(c0, _pt_poly(pt), c0)

    def _pk(self, pt, ct, level, samples, fused):
        """encryptZeroPk (:218-308) for a ciphertext: levelP = 0 (:231).  samples: {"u", "e0", "e1"}: (npoly, N) each"""
        pk = self.key
        rq, rp = self.ringQ.AtLevel(level), self.ringP.AtLevel(0)
        if pk.LevelQ() < level or pk.LevelP() < 0:
            raise RingHipError("the public key has fewer limbs than the ciphertext's level")
        npoly, L = ct.Value[0].npoly, level + 1
        uQ, uP = rq.NewPoly(npoly), rp.NewPoly(npoly)
        lift_small(rq, rp, self._small(self.ternary, npoly, samples.get("u")), uQ, uP)
        rq.NTT(uQ, uQ); rp.NTT(uP, uP)
        cQ, cP = [rq.NewPoly(npoly), rq.NewPoly(npoly)], [rp.NewPoly(npoly), rp.NewPoly(npoly)]
        self._mul_pk(rq, level, uQ, pk.Value[0].Q, pk.Value[1].Q, cQ, fused)
        self._mul_pk(rp, 0, uP, pk.Value[0].P, pk.Value[1].P, cP, fused)
        for c, name in ((0, "e0"), (1, "e1")):
            rq.INTT(cQ[c], cQ[c]); rp.INTT(cP[c], cP[c])
            lift_small(rq, rp, self._small(self.gauss, npoly, samples.get(name)), cQ[c], cP[c], accumulate=True)
            self.be.ModDownQPtoQ(level, 0, cQ[c], cP[c], ct.Value[c])
            if ct.IsNTT:
                rq.NTT(ct.Value[c], ct.Value[c])
        self._add_pt(rq, pt, ct)

    def _pk_no_p(self, pt, ct, level, samples, fused):
        """encryptZeroPkNoP (:310-350)"""
        pk = self.key
        rq = self.ringQ.AtLevel(level)
        npoly = ct.Value[0].npoly
        u = rq.NewPoly(npoly)
        lift_small(rq, None, self._small(self.ternary, npoly, samples.get("u")), u)
        rq.NTT(u, u)
        self._mul_pk(rq, level, u, pk.Value[0].Q, pk.Value[1].Q, ct.Value, fused)
        for c, name in ((0, "e0"), (1, "e1")):
            if ct.IsNTT:
                rq.Add(ct.Value[c], self._error_ntt(rq, npoly, samples.get(name)), ct.Value[c])
            else:
                rq.INTT(ct.Value[c], ct.Value[c])
                lift_small(rq, None, self._small(self.gauss, npoly, samples.get(name)), ct.Value[c], accumulate=True)
        self._add_pt(rq, pt, ct)

    @staticmethod
    def _mul_pk(ring, level, u, pk0, pk1, out, fused):
        """out[c] = u pk_c (:259-260, :324-326): one launch that reads u once, or the reference's two MulCoeffsMontgomery per ciphertext of the batch"""
        if fused:
            _check(lib().rh_rlwe_mul_pk(ring._h, level, u.ptr, pk0.ptr, pk1.ptr, out[0].ptr, out[1].ptr, u.npoly))
            return
        keys = [DevicePoly(ring, 1, level + 1, ptr=k.ptr, owner=k) for k in (pk0, pk1)]
        for k in range(u.npoly):
            for c in (0, 1):
                ring.MulCoeffsMontgomery(_view(u, ring, k, 1), keys[c], _view(out[c], ring, k, 1))

    @staticmethod
    def _add_pt(rq, pt, ct):
        if pt is not None:
            rq.Add(ct.Value[0], _pt_poly(pt), ct.Value[0])

    def _zero_qp(self, ct, samples, fused):
        """Element[ringqp.Poly] targets, NTT domain and Montgomery form (what the key generator asks for, :432-460): one poly per component"""
        if not isinstance(self.key, SecretKey):
            raise RingHipError("cannot EncryptZero: ringqp elements are encrypted under a secret key on the device path")
        if not ct.IsNTT or ct.Value[0].Q.npoly != 1:
            raise RingHipError("cannot EncryptZero: ringqp elements are taken one at a time, in the NTT domain and in Montgomery form")
        kg = KeyGenerator(self.ringQ, self.ringP, self.xs, self.xe, self.prng, conjugate_invariant=self._ci)
        levelQ, levelP = ct.LevelQ(), ct.LevelP()
        sq, sp = kg._sk_rows(self.key, levelQ, levelP)
        tabQ, tabP, _, _ = kg._zero_rows(sq, sp, levelQ, levelP, samples, fused)
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        for c in (0, 1):
            rq.CopyLvl(_view(tabQ, rq, c, 1), ct.Value[c].Q)
            if rp is not None:
                rp.CopyLvl(_view(tabP, rp, c, 1), ct.Value[c].P)


class Decryptor:
    """rlwe.Decryptor (decryptor.go:42-90): pt = c0 + s (c1 + s c2), degree <= 2, in the ciphertext's domain"""

    def __init__(self, ringQ, sk, conjugate_invariant=False):
        rings_ok("Decryptor", ringQ, None, conjugate_invariant)
        self.ringQ, self.sk = ringQ, sk

    @reference_order
    def Decrypt(self, ct, pt, fused=None):
        level = min(ct.Level(), pt.Level())
        out = _pt_poly(pt)
        if self.ringQ.kind == Matrix3N:
            for v in ct.Value:                                             # the secret is held in the reference's order
                if ct.IsNTT:
                    self.ringQ.ToReferenceOrder(v)
                else:
                    v.layout = None
            out.layout = None
        if ct.Degree() not in (1, 2):
            raise RingHipError("cannot Decrypt: the device path takes ciphertexts of degree 1 or 2")
        if out.limbs != level + 1 or ct.Level() != level or out.npoly != ct.Value[0].npoly:
            raise RingHipError("cannot Decrypt: allocate the plaintext at the ciphertext's level and batch size")
        rq = self.ringQ.AtLevel(level)
        npoly = out.npoly
        sk = DevicePoly(rq, 1, level + 1, ptr=self.sk.Value.Q.ptr, owner=self.sk.Value.Q)
        vals = ct.Value
        if not ct.IsNTT:                                                   # NTTLazy of every component (:64, :72): the same residues
            vals = [rq.NewPoly(npoly) for _ in ct.Value]
            for a, b in zip(ct.Value, vals):
                rq.NTT(a, b)
        if _fused(fused):
            _check(lib().rh_rlwe_decrypt(rq._h, level, vals[0].ptr, vals[1].ptr, vals[2].ptr if len(vals) == 3 else None, sk.ptr, out.ptr, npoly))
        else:
            acc = rq.NewPoly(npoly)
            rq.CopyLvl(vals[-1], acc)
            for v in reversed(vals[:-1]):
                for k in range(npoly):
                    rq.MulCoeffsMontgomery(_view(acc, rq, k, 1), sk, _view(acc, rq, k, 1))
                rq.Add(acc, v, acc)
            rq.CopyLvl(acc, out)
        if not ct.IsNTT:
            rq.INTT(out, out)
        for name in ("Scale", "LogDimensions", "IsBatched", "IsMontgomery"):
            if hasattr(ct, name):
                setattr(pt, name, getattr(ct, name))
        pt.IsNTT = ct.IsNTT

    def DecryptNew(self, ct, fused=None):
        pt = Plaintext(self.ringQ.AtLevel(ct.Level()).NewPoly(ct.Value[0].npoly), is_ntt=ct.IsNTT)
        self.Decrypt(ct, pt, fused)
        return pt

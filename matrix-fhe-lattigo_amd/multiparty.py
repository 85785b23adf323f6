"""The multiparty protocols of the reference's multiparty/ package on the device, over the samplers of sampling.py and the keys of keygen.py.

  CRS                          crs.go: a KeyedPRNG.  Two CRS objects made from the same key and used in the same order give identical CRPs: a CRP
                               is ONE uniform Read under the next call counter, poly index = the flat row of the gadget table
  PublicKeyGenProtocol         keygen_cpk.go: SampleCRP :59-63, AllocateShare :53-55, GenShare :70-83, AggregateShares :86-88, GenPublicKey :91-94
  EvaluationKeyGenProtocol     keygen_evk.go: AllocateShare :77-84, SampleCRP :88-112, GenShare :115-210, AggregateShares :213-242, GenEvaluationKey :245-268
  GaloisKeyGenProtocol         keygen_gal.go: GenShare :57-78, AggregateShares :81-90, GenGaloisKey :93-100; GenSharesNew / GenGaloisKeysNew: the
                               shares (keys) of many Galois elements in ONE launch sequence, chunked under keygen.SCRATCH_CAP
  KeySwitchProtocol            keyswitch_sk.go: the error law :78-84, AllocateShare :101-103, SampleCRP :107-112, GenShare :118-149,
                               AggregateShares :154-161, KeySwitch :164-178, on batches of ciphertexts in both domains
  PublicKeySwitchProtocol      keyswitch_pk.go: AllocateShare :65-67, GenShare :73-108, AggregateShares :114-122, KeySwitch :125-137
  RelinearizationKeyGenProtocol keygen_relin.go: SampleCRP :103-123, AllocateShare :316-326, GenShareRoundOne :130-222, GenShareRoundTwo :231-270,
                               AggregateShares :273-290, GenRelinearizationKey :297-312
  Thresholdizer, Combiner      threshold.go: GenShamirPolynomial :81-93, GenShamirSecretShare :102-104, AggregateShares :107-113, NewCombiner
                               :117-144, GenAdditiveShare :148-167, lagrange_coefficient :169-179; over the existing ring calls, no kernel
  NoiseRelinearizationKey, NoiseEvaluationKey, NoiseGaloisKey, NoiseKeySwitch, NoisePublicKeySwitch      utils.go:10-56

Keys, shares, CRPs and ciphertexts are device blocks.  A share or a CRP of a gadget protocol is a degree-0 gadget table: Q (rows, levelQ + 1, N)
and P (rows, levelP + 1, N), flat row sum(dpl[:i]) + j for Value[i][j].  They travel between parties as numpy() / from_numpy arrays.

Every AggregateShares takes the reference's (share1, share2, shareOut) and also (list_of_shares, shareOut): the list form is one
rh_mp_aggregate call per ring that reads every share once; shareOut may be one of the inputs.  KeySwitch takes a list of shares too and then
puts ctIn.Value[0] through the same call as one more addend.

Every arithmetic entry takes `samples=` in place of its PRNG (the exact keys are in each docstring), which pins it bit for bit to
tests/multiparty_restatement.py.  FUSED_MULTIPARTY selects, per family, the kernels of csrc/multiparty.hip or the composed ring calls of the
reference: the same bits either way; `fused=` overrides per call.

The collective refresh of multiparty/mpckks -- big-integer shares on the device, EncToShare, ShareToEnc, the masked transform and Refresh -- is
multiparty_refresh.py, imported below: rh.multiparty.mpckks and the names beside it; multiparty/mpbgv, composed from existing calls, is there too.

Not built, refused by name or absent: a non-nil CKKS transform function, binary serialisation of shares, ShallowCopy (nothing here is
shared mutable state), compressed shares, conjugate-invariant and 3N rings, a flooding law that is not a discrete Gaussian, a flooding bound
with floor(bound) >= 1024."""
import ctypes as C
import math

import numpy as np

from . import keygen as _kg
from .keygen import Encryptor, EvaluationKey, GaloisKey, KeyGenerator, PublicKey, RelinearizationKey, SecretKey, _standard, _view, digits_per_limb, gadget_row_table
from .ringhip import DevicePoly, RingHipError, U64P, _check, lib
from .rlwe import PolyQP
from .sampling import GaussianSampler, KeyedPRNG, NewPRNG, SmallPoly, TernarySampler, UniformSampler, lift_small
from .schemes import Ciphertext

# the kernels of csrc/multiparty.hip (True) or the composed ring calls (False), per family; the measured choice: profiles/multiparty.json
FUSED_MULTIPARTY = {"aggregate": True, "gadget_share": True, "relin_rounds": True, "keyswitch_share": True}


def _fused(family, fused):
    return FUSED_MULTIPARTY[family] if fused is None else bool(fused)


def CRS(key):
    """multiparty.CRS (crs.go): a keyed PRNG every party builds from the same key"""
    return KeyedPRNG(key)


# ---- utils.go ------------------------------------------------------------------------------------------------------------------------------
def NoiseRelinearizationKey(hamming_weight, nbParties, sigma=3.2):
    """(:10-26): sqrt(2 e (H + 1)), H = nbParties * XsHammingWeight, e = nbParties * NoiseFreshSK^2"""
    H = float(nbParties * hamming_weight)
    e = float(nbParties) * sigma * sigma
    return math.sqrt(2 * e * (H + 1))


def NoiseEvaluationKey(nbParties, sigma=3.2):
    """(:29-31): sqrt(nbParties) * NoiseFreshSK"""
    return math.sqrt(float(nbParties)) * sigma


def NoiseGaloisKey(nbParties, sigma=3.2):
    """(:34-36)"""
    return NoiseEvaluationKey(nbParties, sigma)


def _noise_decrypt_with_smudging(nbParties, noisect, noisefresh, noiseflood):
    """(:49-56)"""
    std = noisefresh * noisefresh + noiseflood * noiseflood
    return math.sqrt(std * float(nbParties) + noisect * noisect)


def NoiseKeySwitch(nbParties, noisect, noiseflood, sigma=3.2):
    """(:39-42): NoiseFreshSK = sigma"""
    return _noise_decrypt_with_smudging(nbParties, noisect, sigma, noiseflood)


def NoisePublicKeySwitch(nbParties, noisect, noiseflood, noise_fresh_pk):
    """(:44-47): noise_fresh_pk = Parameters.NoiseFreshPK of the parameters"""
    return _noise_decrypt_with_smudging(nbParties, noisect, noise_fresh_pk, noiseflood)


# ---- aggregation ---------------------------------------------------------------------------------------------------------------------------
_AGG_TABLES = {}


def aggregate(ring, polys, out, fused=None):
    """out = the sum of `polys` (DevicePoly blocks of out's shape) modulo the ring's limbs, canonical.  fused: ONE rh_mp_aggregate launch that
    reads every block once (P + 1 block-sized passes for P blocks); composed: the reference's P - 1 pairwise ring.Add calls (3 (P - 1) passes).
    Two blocks are the same three passes either way and the one Add is the faster (profiles/multiparty.json), so the default takes the
    kernel from three blocks on; fused=True forces it.  out may be one of the blocks."""
    polys = list(polys)
    if fused is None and len(polys) <= 2:
        fused = False
    if not polys:
        raise RingHipError("cannot AggregateShares: no shares")
    for p in polys:
        if p.npoly != out.npoly or p.limbs != out.limbs:
            raise RingHipError("cannot AggregateShares: shares levels do not match")
    rl = ring.AtLevel(out.limbs - 1)
    if _fused("aggregate", fused):
        n = len(polys)
        table = _AGG_TABLES.get(ring._h.value)
        if table is None or table.words < n:
            table = _AGG_TABLES[ring._h.value] = DevicePoly(ring.AtLevel(0), (max(n, 64) + ring.N - 1) // ring.N, 1)
        ptrs = (C.c_void_p * n)(*[p.ptr for p in polys])
        _check(lib().rh_mp_aggregate(ring._h, out.limbs - 1, ptrs, n, out.ptr, out.npoly, table.ptr, table.words))
        return
    for k, p in enumerate(polys):                                          # an output that is also an addend is read first
        if p.ptr == out.ptr:
            polys.insert(0, polys.pop(k))
            break
    if len(polys) == 1:
        if polys[0].ptr != out.ptr:
            rl.CopyLvl(polys[0], out)
        return
    rl.Add(polys[0], polys[1], out)
    for p in polys[2:]:
        rl.Add(out, p, out)


def _share_list(args):
    """(share1, share2, shareOut) or (list_of_shares, shareOut) -> (shares, shareOut)"""
    if len(args) == 2 and isinstance(args[0], (list, tuple)):
        return list(args[0]), args[1]
    if len(args) == 3:
        return [args[0], args[1]], args[2]
    raise RingHipError("AggregateShares takes (share1, share2, shareOut) or (list_of_shares, shareOut)")


# ---- the collective public key ----------------------------------------------------------------------------------------------------------------
class PublicKeyGenShare:
    """multiparty.PublicKeyGenShare: Value = PolyQP of one poly modulo QP, NTT domain, Montgomery form (also the type of PublicKeyGenCRP)"""

    def __init__(self, Q, P):
        self.Value = PolyQP(Q, P)

    def numpy(self):
        return self.Value.Q.numpy(), (self.Value.P.numpy() if self.Value.P is not None else None)


PublicKeyGenCRP = PublicKeyGenShare


class _Protocol:
    """what the key protocols share: the rings, the parameters' error law and a key generator's samplers and level checks"""

    def __init__(self, ringQ, ringP=None, xe=(3.2, 19), prng=None):
        _standard(ringQ, ringP)
        self.ringQ, self.ringP = ringQ, ringP
        self.kg = KeyGenerator(ringQ, ringP, xe=xe, prng=prng)
        self.prng = self.kg.prng
        self.Q, self.P = self.kg.Q, self.kg.P

    def _crp_rows(self, crs, levelQ, levelP, rows, call=None):
        """`rows` uniform polys modulo QP at (levelQ, levelP) from ONE call counter value of the CRS: poly index = row, limbs of Q then of P"""
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        q = DevicePoly(rq, rows, levelQ + 1)
        p = DevicePoly(rp, rows, levelP + 1) if rp is not None else None
        self._crp_fill(crs, q, p, 0, rows, crs.next_call() if call is None else call)
        return q, p

    def _crp_fill(self, crs, q, p, first, rows, call):
        us = UniformSampler(crs, self.ringQ, self.ringP)
        rq = self.ringQ.AtLevel(q.limbs - 1)
        N = rq.N
        us.read_rows(rq, q.ptr + first * q.limbs * N * 8, q.limbs, rows, call, 0, 0)
        if p is not None:
            us.read_rows(self.ringP.AtLevel(p.limbs - 1), p.ptr + first * p.limbs * N * 8, p.limbs, rows, call, 0, q.limbs)

    def _share_rows(self, skIn, skOutQ, skOutP, crpQ, crpP, hQ, hP, levelQ, levelP, pw2, nkeys, dpl, plaintext=True, samples=None, fused=None):
        """the rows of `nkeys` shares at (levelQ, levelP) in one launch sequence: one Gaussian Read, one lift and one NTT over every error row, one
        rh_mp_gadget_share with the per-row key index (keygen_evk.go:161-207 for each key).  skIn: (1 or nkeys, levelQ + 1, N); skOutQ / skOutP:
        (nkeys, limbs, N); crp and h: (nkeys * rows, limbs, N), key-major.  Chunked over keys so that the error scratch stays under
        keygen.SCRATCH_CAP.  samples: {"e": int32 (nkeys * rows, N)}."""
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        LQ, LP, N = levelQ + 1, levelP + 1, rq.N
        rows = sum(dpl)
        R = nkeys * rows
        one = gadget_row_table(self.Q, self.P, levelQ, levelP, pw2, dpl) if plaintext else [[0] * (LQ + 1) for _ in range(rows)]
        if samples is None:
            call_e = self.prng.next_call()
        else:
            e_all = np.asarray(samples["e"], dtype=np.int32).reshape(R, N)
        per_key = rows * N * (4 + 8 * (LQ + LP))
        step = max(1, min(nkeys, _kg.SCRATCH_CAP // per_key))
        scratch = None
        for k0 in range(0, nkeys, step):
            kc = min(step, nkeys - k0)
            r0, rc = k0 * rows, kc * rows
            cq, hq = _view(crpQ, rq, r0, rc), _view(hQ, rq, r0, rc)
            cp, hp = (_view(crpP, rp, r0, rc), _view(hP, rp, r0, rc)) if rp is not None else (None, None)
            if scratch is None or scratch[0].npoly != rc:
                scratch = (SmallPoly(rq, rc), DevicePoly(rq, rc, LQ), DevicePoly(rp, rc, LP) if rp is not None else None,
                           DevicePoly(rq.AtLevel(0), (rc * (LQ + 1) + N - 1) // N + 1, 1))
            small, eQ, eP, table = scratch
            if samples is None:
                self.kg.gauss.Read(small, call=call_e, poly0=r0)
            else:
                small.upload(e_all[r0:r0 + rc])
            lift_small(rq, rp, small, eQ, eP)
            rq.NTT(eQ, eQ)
            if rp is not None:
                rp.NTT(eP, eP)
            self._rows_apply(rq, rp, eQ, eP, cq, cp, hq, hp, skIn, skOutQ, skOutP, nkeys, k0, kc, rows, one, table, _fused("gadget_share", fused))

    @staticmethod
    def _rows_apply(rq, rp, eQ, eP, cq, cp, hq, hp, skIn, skOutQ, skOutP, nkeys, k0, kc, rows, one, table, fused):
        """the rows of keys [k0, k0 + kc) from their prepared errors (the NTT of the lift): rh_mp_gadget_share, or the reference's calls per row"""
        levelQ, levelP = rq.level, rp.level if rp is not None else -1
        rc = kc * rows
        if fused:
            rt = np.array([[k] + row[1:] for k in range(k0, k0 + kc) for row in one], dtype=np.uint64)
            _check(lib().rh_mp_gadget_share(rq._h, rp._h if rp is not None else None, levelQ, levelP, eQ.ptr, eP.ptr if eP is not None else None,
                                            cq.ptr, cp.ptr if cp is not None else None, hq.ptr, hp.ptr if hp is not None else None,
                                            skOutQ.ptr, skOutP.ptr if skOutP is not None else None, skIn.ptr, nkeys, skIn.npoly,
                                            rt.ctypes.data_as(U64P), rc, table.ptr, table.words))
            return
        for r in range(rc):                                                # (keygen_evk.go:170-202)
            k = k0 + r // rows
            for ring, e, h in ((rq, eQ, hq), (rp, eP, hp)):
                if ring is not None:
                    ring.MForm(_view(e, ring, r, 1), _view(h, ring, r, 1))
            scal = one[r % rows][1:]
            if any(scal):
                si = _view(skIn, rq, k if skIn.npoly > 1 else 0, 1, levelQ + 1)
                rq.vec_op("MUL_SCALAR_MONT_THEN_ADD", si, None, _view(hq, rq, r, 1), s0=scal)
            for ring, c, h, so in ((rq, cq, hq, skOutQ), (rp, cp, hp, skOutP)):
                if ring is not None:
                    ring.MulCoeffsMontgomeryThenSub(_view(c, ring, r, 1), _view(so, ring, k, 1), _view(h, ring, r, 1))


class PublicKeyGenProtocol(_Protocol):
    """multiparty.PublicKeyGenProtocol over (ringQ, ringP), at the parameters' top levels"""

    def _levels(self):
        return self.ringQ.L - 1, self.ringP.L - 1 if self.ringP is not None else -1

    def AllocateShare(self):
        """(:53-55)"""
        lq, lp = self._levels()
        return PublicKeyGenShare(self.ringQ.NewPoly(1), self.ringP.NewPoly(1) if lp >= 0 else None)

    def SampleCRP(self, crs):
        """(:59-63): one uniform poly modulo QP"""
        lq, lp = self._levels()
        return PublicKeyGenCRP(*self._crp_rows(crs, lq, lp, 1))

    def GenShare(self, sk, crp, shareOut, samples=None, fused=None):
        """(:70-83): share = MForm(NTT(e)) - crp * sk.  samples: {"e": int32 (1, N)}"""
        lq, lp = self._levels()
        sq, sp = self.kg._sk_rows(sk, lq, lp)
        self._share_rows(sq, sq, sp, crp.Value.Q, crp.Value.P, shareOut.Value.Q, shareOut.Value.P, lq, lp, 0, 1, [1], plaintext=False,
                         samples=samples, fused=fused)

    def AggregateShares(self, *args, fused=None):
        """(:86-88), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        aggregate(self.ringQ, [s.Value.Q for s in shares], out.Value.Q, fused)
        if self.ringP is not None:
            aggregate(self.ringP, [s.Value.P for s in shares], out.Value.P, fused)

    def GenPublicKey(self, roundShare, crp, pubkey=None):
        """(:91-94): Value[0] = the aggregated share, Value[1] = the CRP"""
        lq, lp = self._levels()
        Q = self.ringQ.NewPoly(2)
        P = self.ringP.NewPoly(2) if lp >= 0 else None
        for c, src in ((0, roundShare), (1, crp)):
            self.ringQ.CopyLvl(src.Value.Q, _view(Q, self.ringQ, c, 1))
            if P is not None:
                self.ringP.CopyLvl(src.Value.P, _view(P, self.ringP, c, 1))
        new = PublicKey(self.ringQ, self.ringP, Q, P)
        if pubkey is None:
            return new
        pubkey.Q, pubkey.P, pubkey.Value = new.Q, new.P, new.Value
        return pubkey


# ---- collective evaluation and Galois keys -----------------------------------------------------------------------------------------------------
class EvaluationKeyGenShare:
    """multiparty.EvaluationKeyGenShare, a degree-0 gadget table: Q (rows, levelQ + 1, N), P (rows, levelP + 1, N) or None, NTT domain, Montgomery
    form; flat row sum(dpl[:i]) + j holds Value[i][j][0].  EvaluationKeyGenCRP has the same shape."""
    GaloisElement = 0

    def __init__(self, Q, P, levelQ, levelP, BaseTwoDecomposition, dpl):
        self.Q, self.P, self.levelQ, self.levelP = Q, P, levelQ, levelP
        self.BaseTwoDecomposition, self.dpl = int(BaseTwoDecomposition), list(dpl)

    def LevelQ(self):
        return self.levelQ

    def LevelP(self):
        return self.levelP

    def BaseRNSDecompositionVectorSize(self):
        return len(self.dpl)

    def BaseTwoDecompositionVectorSize(self):
        return list(self.dpl)

    def numpy(self):
        return self.Q.numpy(), (self.P.numpy() if self.P is not None else None)


EvaluationKeyGenCRP = GaloisKeyGenShare = GaloisKeyGenCRP = EvaluationKeyGenShare


class EvaluationKeyGenProtocol(_Protocol):
    """multiparty.EvaluationKeyGenProtocol.  levelQ / levelP / BaseTwoDecomposition: rlwe.EvaluationKeyParameters, the parameters' maxima unless told"""

    def _blocks(self, levelQ, levelP, pw2, compressed, n=1):
        levelQ, levelP, pw2 = self.kg._levels(levelQ, levelP, pw2, compressed)
        dpl = digits_per_limb(self.Q, levelQ, levelP, pw2)
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        rows = sum(dpl)
        return levelQ, levelP, pw2, dpl, DevicePoly(rq, n * rows, levelQ + 1), DevicePoly(rp, n * rows, levelP + 1) if rp is not None else None

    def _split(self, q, p, n, levelQ, levelP, pw2, dpl):
        """n shares (CRPs) as views of one block each of Q and P, key-major"""
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        rows = sum(dpl)
        return [EvaluationKeyGenShare(_view(q, rq, k * rows, rows), _view(p, rp, k * rows, rows) if p is not None else None, levelQ, levelP, pw2, dpl)
                for k in range(n)]

    def AllocateShare(self, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False):
        """(:77-84)"""
        return self.AllocateShares(1, levelQ, levelP, BaseTwoDecomposition, compressed)[0]

    def AllocateShares(self, n, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False):
        """n shares in one block each of Q and P, the layout GenSharesNew writes in one launch"""
        levelQ, levelP, pw2, dpl, q, p = self._blocks(levelQ, levelP, BaseTwoDecomposition, compressed, n)
        return self._split(q, p, n, levelQ, levelP, pw2, dpl)

    def SampleCRP(self, crs, levelQ=None, levelP=None, BaseTwoDecomposition=0):
        """(:88-112): every row a uniform poly modulo QP; one call counter value of the CRS, poly index = flat row"""
        return self.SampleCRPs(crs, 1, levelQ, levelP, BaseTwoDecomposition)[0]

    def SampleCRPs(self, crs, n, levelQ=None, levelP=None, BaseTwoDecomposition=0):
        """n SampleCRP calls -- the same polys, one call counter value each -- into one block each of Q and P"""
        levelQ, levelP, pw2, dpl, q, p = self._blocks(levelQ, levelP, BaseTwoDecomposition, False, n)
        rows = sum(dpl)
        for k in range(n):
            self._crp_fill(crs, q, p, k * rows, rows, crs.next_call())
        return self._split(q, p, n, levelQ, levelP, pw2, dpl)

    def _check_crp(self, crp, shareOut):
        if shareOut.BaseRNSDecompositionVectorSize() != crp.BaseRNSDecompositionVectorSize():
            raise RingHipError("cannot GenShare: crp.BaseRNSDecompositionVectorSize() != shareOut.BaseRNSDecompositionVectorSize()")
        if shareOut.BaseTwoDecompositionVectorSize() != crp.BaseTwoDecompositionVectorSize():
            raise RingHipError("cannot GenShare: crp.BaseTwoDecompositionVectorSize() != shareOut.BaseTwoDecompositionVectorSize()")
        if crp.LevelQ() != shareOut.LevelQ() or crp.LevelP() != shareOut.LevelP():
            raise RingHipError("cannot GenShare: crp and shareOut are at different levels")

    def GenShare(self, skIn, skOut, crp, shareOut, samples=None, fused=None):
        """(:115-210): per row e + skIn P 2^(j pw2) on the digit limbs - crp skOut.  samples: {"e": int32 (rows, N)}"""
        levelQ, levelP = shareOut.LevelQ(), shareOut.LevelP()
        if levelQ > min(skIn.LevelQ(), skOut.LevelQ()):
            raise RingHipError("cannot GenShare: min(skIn, skOut) LevelQ < shareOut LevelQ")
        if skOut.LevelP() < levelP:
            raise RingHipError("cannot GenShare: min(skIn, skOut) LevelP != shareOut LevelP")
        self._check_crp(crp, shareOut)
        si, _ = self.kg._sk_rows(skIn, levelQ, -1)
        oq, op = self.kg._sk_rows(skOut, levelQ, levelP)
        self._share_rows(si, oq, op, crp.Q, crp.P, shareOut.Q, shareOut.P, levelQ, levelP, shareOut.BaseTwoDecomposition, 1, shareOut.dpl,
                         samples=samples, fused=fused)

    def _check_levels(self, shares, out):
        for s in shares:
            if s.LevelQ() != out.LevelQ():
                raise RingHipError("cannot AggregateShares: share LevelQ do not match")
            if s.LevelP() != out.LevelP():
                raise RingHipError("cannot AggregateShares: share LevelP do not match")
            if s.dpl != out.dpl:
                raise RingHipError("cannot AggregateShares: share BaseTwoDecompositionVectorSize do not match")

    def AggregateShares(self, *args, fused=None):
        """(:213-242), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        self._check_levels(shares, out)
        aggregate(self.ringQ, [s.Q for s in shares], out.Q, fused)
        if out.P is not None:
            aggregate(self.ringP, [s.P for s in shares], out.P, fused)

    def _tables(self, shareQ, shareP, crpQ, crpP, levelQ, levelP, R):
        """R rows of share and CRP interleaved into gadget tables of (R * 2, limbs, N): component 0 the share, component 1 the CRP"""
        out = []
        for ring, level, s, c in ((self.ringQ, levelQ, shareQ, crpQ), (self.ringP, levelP, shareP, crpP)):
            if s is None:
                out.append(None)
                continue
            rl, L = ring.AtLevel(level), level + 1
            tab = DevicePoly(rl, 2 * R, L)
            _check(lib().rh_ring_copy_rows(rl._h, tab.ptr, 2 * L, s.ptr, L, R, level))
            _check(lib().rh_ring_copy_rows(rl._h, tab.ptr + L * rl.N * 8, 2 * L, c.ptr, L, R, level))
            out.append(tab)
        return out

    def _key(self, cls, tabQ, tabP, first, share):
        return self.kg._key(cls, tabQ, tabP, first, sum(share.dpl), share.levelQ, share.levelP, share.BaseTwoDecomposition, share.dpl)

    def GenEvaluationKey(self, share, crp, evk=None, cls=EvaluationKey):
        """(:245-268): Value[i][j] = (share, crp)"""
        if evk is not None and share.LevelQ() != evk.LevelQ():
            raise RingHipError("cannot GenEvaluationKey: share LevelQ != evk LevelQ")
        if evk is not None and share.LevelP() != evk.LevelP():
            raise RingHipError("cannot GenEvaluationKey: share LevelP != evk LevelP")
        self._check_crp(crp, share)
        tabQ, tabP = self._tables(share.Q, share.P, crp.Q, crp.P, share.levelQ, share.levelP, sum(share.dpl))
        new = self._key(cls, tabQ, tabP, 0, share)
        if evk is None:
            return new
        evk.__dict__.update(new.__dict__)
        return evk


def _contiguous(blocks):
    """the blocks (views of equal shape) lie one after another in memory"""
    step = blocks[0].words * 8
    return all(b.ptr == blocks[0].ptr + k * step for k, b in enumerate(blocks))


class GaloisKeyGenProtocol(EvaluationKeyGenProtocol):
    """multiparty.GaloisKeyGenProtocol"""

    def _sk_out(self, sk, galEls, levelQ, levelP):
        """skOut_k = the NTT automorphism of g_k^-1 on sk (:65-74), (n, limbs, N) over Q and P"""
        sq, sp = self.kg._sk_rows(sk, levelQ, levelP)
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None
        n, N = len(galEls), rq.N
        outQ = DevicePoly(rq, n, levelQ + 1)
        outP = DevicePoly(rp, n, levelP + 1) if rp is not None else None
        for k, g in enumerate(galEls):
            if g & 1 == 0:
                raise RingHipError("cannot GenShare: the Galois element must be odd")
            inv = pow(g, 2 * N - 1, 2 * N)
            rq.AutomorphismNTT(sq, inv, _view(outQ, rq, k, 1))
            if rp is not None:
                rp.AutomorphismNTT(sp, inv, _view(outP, rp, k, 1))
        return sq, outQ, outP

    def GenShare(self, sk, galEl, crp, shareOut, samples=None, fused=None):
        """(:57-78).  samples: {"e": int32 (rows, N)}"""
        self._gen([int(galEl)], sk, [crp], [shareOut], samples, fused)

    def GenSharesNew(self, sk, galEls, crps, samples=None, fused=None):
        """one party's shares for every element of galEls as ONE launch sequence: one Gaussian read, one lift, one NTT, one rh_mp_gadget_share with
        the per-row key index (CRPs that do not lie in one block, as SampleCRPs lays them, are gathered into one first).
        samples: {"e": int32 (len(galEls) * rows, N)}, key-major"""
        galEls = [int(g) for g in galEls]
        if len(galEls) != len(crps):
            raise RingHipError("cannot GenSharesNew: galEls and crps must have the same length")
        if not galEls:
            return []
        c = crps[0]
        shares = self.AllocateShares(len(galEls), c.levelQ, c.levelP, c.BaseTwoDecomposition)
        self._gen(galEls, sk, list(crps), shares, samples, fused)
        return shares

    def _gen(self, galEls, sk, crps, shares, samples, fused):
        s0 = shares[0]
        levelQ, levelP = s0.LevelQ(), s0.LevelP()
        if levelQ > sk.LevelQ():
            raise RingHipError("cannot GenShare: min(skIn, skOut) LevelQ < shareOut LevelQ")
        if sk.LevelP() < levelP:
            raise RingHipError("cannot GenShare: min(skIn, skOut) LevelP != shareOut LevelP")
        for crp, sh in zip(crps, shares):
            self._check_crp(crp, sh)
        sq, outQ, outP = self._sk_out(sk, galEls, levelQ, levelP)
        n, rows = len(galEls), sum(s0.dpl)
        rq = self.ringQ.AtLevel(levelQ)
        rp = self.ringP.AtLevel(levelP) if levelP >= 0 else None

        def block(items, part, ring, gather):
            """the items' Q (or P) parts as one (n * rows, limbs, N) block"""
            bs = [getattr(x, part) for x in items]
            if _contiguous(bs):
                return DevicePoly(ring, n * rows, bs[0].limbs, ptr=bs[0].ptr, owner=bs[0]), None
            whole = DevicePoly(ring, n * rows, bs[0].limbs)
            if gather:
                for k, b in enumerate(bs):
                    ring.CopyLvl(b, _view(whole, ring, k * rows, rows))
            return whole, bs
        cq, _ = block(crps, "Q", rq, True)
        hq, back_q = block(shares, "Q", rq, False)
        cp = hp = back_p = None
        if rp is not None:
            cp, _ = block(crps, "P", rp, True)
            hp, back_p = block(shares, "P", rp, False)
        self._share_rows(sq, outQ, outP, cq, cp, hq, hp, levelQ, levelP, s0.BaseTwoDecomposition, n, s0.dpl, samples=samples, fused=fused)
        for ring, whole, back in ((rq, hq, back_q), (rp, hp, back_p)):
            if back is not None:
                for k, b in enumerate(back):
                    ring.CopyLvl(_view(whole, ring, k * rows, rows), b)
        for g, sh in zip(galEls, shares):
            sh.GaloisElement = g                                           # "Important" (:68)

    def AggregateShares(self, *args, fused=None):
        """(:81-90), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        for s in shares[1:]:
            if s.GaloisElement != shares[0].GaloisElement:
                raise RingHipError("cannot aggregate: GaloisKeyGenShares do not share the same GaloisElement: %d != %d"
                                   % (shares[0].GaloisElement, s.GaloisElement))
        out.GaloisElement = shares[0].GaloisElement
        EvaluationKeyGenProtocol.AggregateShares(self, shares, out, fused=fused)

    def GenGaloisKey(self, share, crp, gk=None):
        """(:93-100)"""
        new = self.GenEvaluationKey(share, crp, gk, cls=GaloisKey)
        new.GaloisElement, new.NthRoot = share.GaloisElement, 2 * self.ringQ.N
        return new

    def GenGaloisKeysNew(self, shares, crps):
        """the Galois keys of many aggregated shares: two strided copies over all keys when the shares and the CRPs each lie in one block"""
        if len(shares) != len(crps):
            raise RingHipError("cannot GenGaloisKeysNew: shares and crps must have the same length")
        if not shares:
            return []
        s0 = shares[0]
        rq = self.ringQ.AtLevel(s0.levelQ)
        rp = self.ringP.AtLevel(s0.levelP) if s0.levelP >= 0 else None
        parts = [[x.Q for x in shares], [x.Q for x in crps]] + ([[x.P for x in shares], [x.P for x in crps]] if rp is not None else [])
        if not all(_contiguous(b) for b in parts):
            return [self.GenGaloisKey(s, c) for s, c in zip(shares, crps)]
        for s, c in zip(shares, crps):
            self._check_crp(c, s)
        n, rows = len(shares), sum(s0.dpl)
        whole = lambda bs, ring: DevicePoly(ring, n * rows, bs[0].limbs, ptr=bs[0].ptr, owner=bs[0])
        tabQ, tabP = self._tables(whole(parts[0], rq), whole(parts[2], rp) if rp is not None else None, whole(parts[1], rq),
                                  whole(parts[3], rp) if rp is not None else None, s0.levelQ, s0.levelP, n * rows)
        keys = []
        for k, s in enumerate(shares):
            gk = self._key(GaloisKey, tabQ, tabP, k * rows, s)
            gk.GaloisElement, gk.NthRoot = s.GaloisElement, 2 * self.ringQ.N
            keys.append(gk)
        return keys


# ---- collective key switching -------------------------------------------------------------------------------------------------------------------
def _flooding(noise_flooding):
    """ring.DiscreteGaussian as a sigma (Bound = 6 sigma) or a (sigma, bound) pair; any other law is refused (keyswitch_sk.go:78-86, keyswitch_pk.go:48-52)"""
    if isinstance(noise_flooding, (int, float)) and not isinstance(noise_flooding, bool):
        return float(noise_flooding), 6.0 * float(noise_flooding)
    if isinstance(noise_flooding, (tuple, list)) and len(noise_flooding) == 2 and all(isinstance(x, (int, float)) for x in noise_flooding):
        return float(noise_flooding[0]), float(noise_flooding[1])
    raise RingHipError("invalid distribution type, expected DiscreteGaussian (a sigma, or (sigma, bound)) but got %r" % (noise_flooding,))


class KeySwitchShare:
    """multiparty.KeySwitchShare: Value a DevicePoly batch (npoly, level + 1, N), in the domain of the ciphertexts it was made for"""

    def __init__(self, value):
        self.Value = value

    def Level(self):
        return self.Value.limbs - 1

    def _resize(self, ring, level):
        """Poly.Resize to a lower level: the batch dense at that level, in the same memory"""
        if level != self.Level():
            v = self.Value
            self.Value = DevicePoly(ring.AtLevel(level), v.npoly, level + 1, ptr=v.ptr, owner=v)


def _share_product(rl, c1, skA, skB, acc, e, out, fused):
    """out = [acc +] c1 (skA [- skB]) [+ e]: rh_mp_keyswitch_share, or the reference's Sub, MulCoeffsMontgomery and Adds.  c1 may carry more limbs
    per poly than the ring view's level."""
    L, N = rl.level + 1, rl.N
    if fused:
        _check(lib().rh_mp_keyswitch_share(rl._h, rl.level, c1.ptr, c1.limbs, skA.ptr, skB.ptr if skB is not None else None,
                                           acc.ptr if acc is not None else None, e.ptr if e is not None else None, out.ptr, out.npoly))
        return
    delta = skA
    if skB is not None:
        delta = rl.NewPoly(1)
        rl.Sub(skA, skB, delta)
    prod = out if acc is None or acc.ptr != out.ptr else rl.NewPoly(out.npoly)
    for k in range(out.npoly):
        ck = DevicePoly(rl, 1, L, ptr=c1.ptr + k * c1.limbs * N * 8, owner=c1)
        rl.MulCoeffsMontgomery(ck, delta, _view(prod, rl, k, 1))
    if acc is not None:
        rl.Add(acc, prod, out)
    if e is not None:
        rl.Add(out, e, out)


class _Switch:
    def _level(self, ct, shareOut):
        c1 = ct.Value[1]
        npoly = shareOut.Value[0].npoly if isinstance(shareOut.Value, list) else shareOut.Value.npoly
        if c1.npoly != npoly:
            raise RingHipError("cannot GenShare: the share and the ciphertext batch hold different numbers of polys")
        return min(shareOut.Level(), c1.limbs - 1)

    def _sk(self, sk, rl):
        if sk.LevelQ() < rl.level:
            raise RingHipError("the secret key has fewer limbs than the share's level")
        return DevicePoly(rl, 1, rl.level + 1, ptr=sk.Value.Q.ptr, owner=sk.Value.Q)

    def _flood(self, rl, npoly, samples):
        """the flooding error of a batch as int32 coefficients"""
        if samples is not None:
            return SmallPoly.from_numpy(self.ringQ, np.asarray(samples["e"], dtype=np.int32).reshape(npoly, rl.N))
        return self.noise.ReadNew(npoly)

    def _term(self, rl, ct, skA, skB, acc, out, samples, fused):
        """out = [acc +] ct[1] (skA [- skB]) + e in the ciphertext's domain (keyswitch_sk.go:126-148, keyswitch_pk.go:96-107)"""
        npoly, c1 = out.npoly, ct.Value[1]
        small = self._flood(rl, npoly, samples)
        if ct.IsNTT:
            e = rl.NewPoly(npoly)
            lift_small(rl, None, small, e)
            rl.NTT(e, e)
            _share_product(rl, c1, skA, skB, acc, e, out, fused)
            return
        buf = rl.NewPoly(npoly)
        rl.NTT(c1, buf)
        tgt = out if acc is None else buf
        _share_product(rl, buf, skA, skB, None, None, tgt, fused)
        rl.INTT(tgt, tgt)
        lift_small(rl, None, small, tgt, accumulate=True)
        if acc is not None:
            rl.Add(acc, tgt, out)

    @staticmethod
    def _meta(ctIn, opOut):
        for name in ("Scale", "LogDimensions", "IsBatched", "IsMontgomery"):
            if hasattr(ctIn, name):
                setattr(opOut, name, getattr(ctIn, name))
        opOut.IsNTT = ctIn.IsNTT

    def _add_c0(self, ctIn, values, opOut, fused):
        """opOut[0] = ctIn[0] + the combined share, or + every share of a list in one call"""
        level = ctIn.Level()
        for v in values:
            if v.limbs != level + 1 or v.npoly != ctIn.Value[0].npoly or opOut.Value[0].limbs != level + 1:
                raise RingHipError("cannot KeySwitch: the shares and opOut must be at the ciphertext's level and batch size")
        aggregate(self.ringQ, [ctIn.Value[0]] + values, opOut.Value[0], fused)


class KeySwitchProtocol(_Switch):
    """multiparty.KeySwitchProtocol(params, noiseFlooding) over ringQ.  The protocol's error law (:78-84): sigma = sqrt(NoiseFreshSK^2 +
    flooding^2), bound = 6 sigma, from the cumulative table (floor(bound) >= 1024 is refused by the sampler, by name)"""

    def __init__(self, ringQ, noise_flooding, xe_sigma=3.2, prng=None):
        _standard(ringQ)
        self.ringQ = ringQ
        flood, _ = _flooding(noise_flooding)
        self.sigma = math.sqrt(xe_sigma * xe_sigma + flood * flood)
        self.bound = 6 * self.sigma
        self.prng = NewPRNG() if prng is None else prng
        self.noise = GaussianSampler(self.prng, ringQ, self.sigma, self.bound)

    def AllocateShare(self, level, npoly=1):
        """(:101-103), for a batch of npoly ciphertexts"""
        return KeySwitchShare(self.ringQ.AtLevel(level).NewPoly(npoly))

    def SampleCRP(self, level, crs):
        """(:107-112)"""
        p = self.ringQ.AtLevel(level).NewPoly(1)
        UniformSampler(crs, self.ringQ).Read(p)
        return p

    def GenShare(self, skInput, skOutput, ct, shareOut, samples=None, fused=None):
        """(:118-149): share = ct[1] (skInput - skOutput) + e at min(share level, ct level), in ct's domain; ct.Value[0] is not read.
        samples: {"e": int32 (npoly, N)}, drawn from the protocol's law"""
        level = self._level(ct, shareOut)
        shareOut._resize(self.ringQ, level)
        rl = self.ringQ.AtLevel(level)
        self._term(rl, ct, self._sk(skInput, rl), self._sk(skOutput, rl), None, shareOut.Value, samples, _fused("keyswitch_share", fused))

    def AggregateShares(self, *args, fused=None):
        """(:154-161), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        aggregate(self.ringQ, [s.Value for s in shares], out.Value, fused)

    def KeySwitch(self, ctIn, combined, opOut, fused=None):
        """(:164-178): opOut = (ctIn[0] + combined, ctIn[1]).  combined: the aggregated share, or a list of shares summed with ctIn[0] in one call"""
        level = ctIn.Level()
        if ctIn is not opOut:
            self.ringQ.AtLevel(level).CopyLvl(ctIn.Value[1], opOut.Value[1])
            self._meta(ctIn, opOut)
        self._add_c0(ctIn, [s.Value for s in combined] if isinstance(combined, (list, tuple)) else [combined.Value], opOut, fused)


class PublicKeySwitchShare:
    """multiparty.PublicKeySwitchShare: Value[0..1], DevicePoly batches (npoly, level + 1, N)"""

    def __init__(self, value):
        self.Value = list(value)

    def Level(self):
        return self.Value[0].limbs - 1

    def _resize(self, ring, level):
        if level != self.Level():
            self.Value = [DevicePoly(ring.AtLevel(level), v.npoly, level + 1, ptr=v.ptr, owner=v) for v in self.Value]


class PublicKeySwitchProtocol(_Switch):
    """multiparty.PublicKeySwitchProtocol(params, noiseFlooding) over (ringQ, ringP): noise_flooding a sigma (Bound = 6 sigma) or (sigma, bound)"""

    def __init__(self, ringQ, ringP, noise_flooding, xs=("P", 2 / 3), xe=(3.2, 19), prng=None):
        _standard(ringQ, ringP)
        self.ringQ, self.ringP = ringQ, ringP
        self.sigma, self.bound = _flooding(noise_flooding)
        self.prng = NewPRNG() if prng is None else prng
        self.noise = GaussianSampler(self.prng, ringQ, self.sigma, self.bound)
        self.Encryptor = Encryptor(ringQ, ringP, None, prng=self.prng, xs=xs, xe=xe)

    def AllocateShare(self, levelQ, npoly=1):
        """(:65-67)"""
        rl = self.ringQ.AtLevel(levelQ)
        return PublicKeySwitchShare([rl.NewPoly(npoly), rl.NewPoly(npoly)])

    def GenShare(self, sk, pk, ct, shareOut, samples=None, fused=None):
        """(:73-108): Encryptor.WithKey(pk).EncryptZero into the share, then share[0] += ct[1] sk + e, in ct's domain.
        samples: {"u", "e0", "e1"}: int32 (npoly, N) of the zero encryption, {"e"}: int32 (npoly, N) of the flooding law"""
        level = self._level(ct, shareOut)
        shareOut._resize(self.ringQ, level)
        rl = self.ringQ.AtLevel(level)
        zero = Ciphertext(shareOut.Value, is_ntt=ct.IsNTT)
        enc = None if samples is None else {k: samples[k] for k in ("u", "e0", "e1")}
        self.Encryptor.WithKey(pk).EncryptZero(zero, samples=enc, fused=fused)
        self._term(rl, ct, self._sk(sk, rl), None, shareOut.Value[0], shareOut.Value[0], samples, _fused("keyswitch_share", fused))

    def AggregateShares(self, *args, fused=None):
        """(:114-122), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        if any(s.Value[0].limbs != s.Value[1].limbs for s in shares):
            raise RingHipError("cannot AggregateShares: the two shares are at different levelQ")
        for c in (0, 1):
            aggregate(self.ringQ, [s.Value[c] for s in shares], out.Value[c], fused)

    def KeySwitch(self, ctIn, combined, opOut, fused=None):
        """(:125-137): opOut = (ctIn[0] + combined[0], combined[1]).  combined: the aggregated share or a list of shares"""
        level = ctIn.Level()
        many = isinstance(combined, (list, tuple))
        shares = list(combined) if many else [combined]
        if ctIn is not opOut:
            self._meta(ctIn, opOut)
        self._add_c0(ctIn, [s.Value[0] for s in shares], opOut, fused)
        if many:
            aggregate(self.ringQ, [s.Value[1] for s in shares], opOut.Value[1], fused)
        else:
            self.ringQ.AtLevel(level).CopyLvl(combined.Value[1], opOut.Value[1])


# ---- the collective relinearisation key -----------------------------------------------------------------------------------------------------------
class RelinearizationKeyGenShare(EvaluationKeyGenShare):
    """multiparty.RelinearizationKeyGenShare: a gadget table of degree 1 (round one: Q (rows * 2, limbs, N), row r's components at polys 2 r and
    2 r + 1) or of degree 0 (round two: Q (rows, limbs, N)).  PLAIN residues in the NTT domain: the final key takes MForm of both components."""

    def __init__(self, Q, P, levelQ, levelP, BaseTwoDecomposition, dpl, degree):
        EvaluationKeyGenShare.__init__(self, Q, P, levelQ, levelP, BaseTwoDecomposition, dpl)
        self.degree = int(degree)

    def Degree(self):
        return self.degree


class RelinearizationKeyGenProtocol(EvaluationKeyGenProtocol):
    """multiparty.RelinearizationKeyGenProtocol.  xs: the ephemeral secret's law, ("P", density) or ("H", weight).  SampleCRP is the evaluation-key
    protocol's (:103-123)."""

    def __init__(self, ringQ, ringP=None, xs=("P", 2 / 3), xe=(3.2, 19), prng=None):
        EvaluationKeyGenProtocol.__init__(self, ringQ, ringP, xe, prng)
        self.xs = tuple(xs)

    def AllocateShare(self, levelQ=None, levelP=None, BaseTwoDecomposition=0, compressed=False):
        """(:316-326): the ephemeral secret, a degree-1 round-one share and a degree-0 round-two share"""
        if compressed:
            raise RingHipError("cannot AllocateShare: relinearization key shares cannot be allocated in the compressed format")
        levelQ, levelP, pw2, dpl, q1, p1 = self._blocks(levelQ, levelP, BaseTwoDecomposition, False, 2)
        _, _, _, _, q2, p2 = self._blocks(levelQ, levelP, pw2, False, 1)
        eph = SecretKey(None, self.ringQ.NewPoly(1), self.ringP.NewPoly(1) if self.ringP is not None else None)
        return (eph, RelinearizationKeyGenShare(q1, p1, levelQ, levelP, pw2, dpl, 1), RelinearizationKeyGenShare(q2, p2, levelQ, levelP, pw2, dpl, 0))

    def _errors(self, rq, rp, rows, given, call):
        """the NTT of `rows` lifted error polys modulo QP, not in Montgomery form (:176-182)"""
        small = SmallPoly.from_numpy(rq, np.asarray(given, dtype=np.int32).reshape(rows, rq.N)) if given is not None else None
        if small is None:
            small = SmallPoly(rq, rows)
            self.kg.gauss.Read(small, call=call)
        eQ = rq.NewPoly(rows)
        eP = rp.NewPoly(rows) if rp is not None else None
        lift_small(rq, rp, small, eQ, eP)
        rq.NTT(eQ, eQ)
        if rp is not None:
            rp.NTT(eP, eP)
        return eQ, eP

    def _rings(self, share):
        rq = self.ringQ.AtLevel(share.levelQ)
        return rq, self.ringP.AtLevel(share.levelP) if share.levelP >= 0 else None

    def GenShareRoundOne(self, sk, crp, ephSkOut, shareOut, samples=None, fused=None):
        """(:130-222): round1[r] = (-u crp[r] + sk P 2^(j pw2) on the digit limbs + e0_r, sk crp[r] + e1_r); the ephemeral secret u goes to ephSkOut.
        samples: {"u": int32 (N,), "e0": int32 (rows, N), "e1": int32 (rows, N)}"""
        if shareOut.Degree() != 1:
            raise RingHipError("cannot GenShareRoundOne: the round-one share has degree 1")
        self._check_crp(crp, shareOut)
        levelQ, levelP, pw2, dpl = shareOut.levelQ, shareOut.levelP, shareOut.BaseTwoDecomposition, shareOut.dpl
        rq, rp = self._rings(shareOut)
        LQ, N, rows = levelQ + 1, rq.N, sum(dpl)
        samples = samples or {}
        if "u" in samples:
            u = self.kg._secret_from(SmallPoly.from_numpy(self.ringQ, np.asarray(samples["u"], dtype=np.int32).reshape(1, -1)))
        else:
            u = self.kg._secret_from(TernarySampler(self.prng, self.ringQ, **{self.xs[0]: self.xs[1]}).ReadNew(1))
        ephSkOut.coeffs, ephSkOut.Value = u.coeffs, u.Value
        call0, call1 = (None, None) if "e0" in samples else (self.prng.next_call(), self.prng.next_call())
        e0Q, e0P = self._errors(rq, rp, rows, samples.get("e0"), call0)
        e1Q, e1P = self._errors(rq, rp, rows, samples.get("e1"), call1)
        sq, sp = self.kg._sk_rows(sk, levelQ, levelP)
        uq, up = self.kg._sk_rows(u, levelQ, levelP)
        skI = rq.NewPoly(1)
        rq.IMForm(sq, skI)                                                 # IMForm(P sk) = P IMForm(sk): the factor P 2^(j pw2) is the row's scalar
        one = gadget_row_table(self.Q, self.P, levelQ, levelP, pw2, dpl)
        ptr = lambda x: x.ptr if x is not None else None
        if _fused("relin_rounds", fused):
            rt = np.array(one, dtype=np.uint64)
            table = DevicePoly(rq.AtLevel(0), (rows * (LQ + 1) + N - 1) // N + 1, 1)
            _check(lib().rh_mp_relin_round_one(rq._h, rp._h if rp is not None else None, levelQ, levelP, e0Q.ptr, ptr(e0P), e1Q.ptr, ptr(e1P), crp.Q.ptr, ptr(crp.P),
                                               shareOut.Q.ptr, ptr(shareOut.P), uq.ptr, ptr(up), sq.ptr, ptr(sp), skI.ptr,
                                               rt.ctypes.data_as(U64P), rows, table.ptr, table.words))
            return
        for r in range(rows):
            for ring, e0, e1, c, h, uu, ss in ((rq, e0Q, e1Q, crp.Q, shareOut.Q, uq, sq), (rp, e0P, e1P, crp.P, shareOut.P, up, sp)):
                if ring is None:
                    continue
                h0, h1, a = _view(h, ring, 2 * r, 1), _view(h, ring, 2 * r + 1, 1), _view(c, ring, r, 1)
                ring.CopyLvl(_view(e0, ring, r, 1), h0)
                if ring is rq and any(one[r][1:]):
                    rq.vec_op("MUL_SCALAR_MONT_THEN_ADD", skI, None, h0, s0=one[r][1:])
                ring.MulCoeffsMontgomeryThenSub(uu, a, h0)
                ring.CopyLvl(_view(e1, ring, r, 1), h1)
                ring.MulCoeffsMontgomeryThenAdd(ss, a, h1)

    def GenShareRoundTwo(self, ephSk, sk, round1, shareOut, samples=None, fused=None):
        """(:231-270): round2[r] = sk round1[r][0] + (u - sk) round1[r][1] + e_r.  samples: {"e": int32 (rows, N)}"""
        if round1.Degree() != 1 or shareOut.Degree() != 0:
            raise RingHipError("cannot GenShareRoundTwo: round1 has degree 1 and the round-two share degree 0")
        self._check_levels([round1], shareOut)
        levelQ, levelP = shareOut.levelQ, shareOut.levelP
        rq, rp = self._rings(shareOut)
        rows = sum(shareOut.dpl)
        given = samples["e"] if samples is not None else None
        eQ, eP = self._errors(rq, rp, rows, given, None if given is not None else self.prng.next_call())
        sq, sp = self.kg._sk_rows(sk, levelQ, levelP)
        uq, up = self.kg._sk_rows(ephSk, levelQ, levelP)
        ptr = lambda x: x.ptr if x is not None else None
        if _fused("relin_rounds", fused):
            _check(lib().rh_mp_relin_round_two(rq._h, rp._h if rp is not None else None, levelQ, levelP, eQ.ptr, ptr(eP), round1.Q.ptr, ptr(round1.P), shareOut.Q.ptr,
                                               ptr(shareOut.P), uq.ptr, ptr(up), sq.ptr, ptr(sp), rows))
            return
        for ring, e, x, h, uu, ss in ((rq, eQ, round1.Q, shareOut.Q, uq, sq), (rp, eP, round1.P, shareOut.P, up, sp)):
            if ring is None:
                continue
            delta = ring.NewPoly(1)
            ring.Sub(uu, ss, delta)
            for r in range(rows):
                out = _view(h, ring, r, 1)
                ring.MulCoeffsMontgomery(_view(x, ring, 2 * r, 1), ss, out)
                ring.Add(out, _view(e, ring, r, 1), out)
                ring.MulCoeffsMontgomeryThenAdd(delta, _view(x, ring, 2 * r + 1, 1), out)

    def AggregateShares(self, *args, fused=None):
        """(:273-290), or (list_of_shares, shareOut): round-one shares with round-one shares, round-two with round-two"""
        shares, out = _share_list(args)
        if any(s.Degree() != out.Degree() for s in shares):
            raise RingHipError("cannot AggregateShares: shares of different rounds")
        EvaluationKeyGenProtocol.AggregateShares(self, shares, out, fused=fused)

    def GenRelinearizationKey(self, round1, round2, evalKeyOut=None):
        """(:297-312): Value[r] = (MForm(round2[r]), MForm(round1[r][1]))"""
        if round1.Degree() != 1 or round2.Degree() != 0:
            raise RingHipError("cannot GenRelinearizationKey: round1 has degree 1 and round2 degree 0")
        self._check_levels([round1], round2)
        rows = sum(round1.dpl)
        tabs = []
        for ring, r1, r2 in zip(self._rings(round1), (round1.Q, round1.P), (round2.Q, round2.P)):
            if ring is None:
                tabs.append(None)
                continue
            L, N = ring.level + 1, ring.N
            tab = DevicePoly(ring, 2 * rows, L)
            wide = lambda p, off: DevicePoly(ring, rows, 2 * L, ptr=p.ptr + off * L * N * 8, owner=p)    # one component of every row, at the row stride
            ring.MForm(r2, wide(tab, 0))
            ring.MForm(wide(r1, 1), wide(tab, 1))
            tabs.append(tab)
        new = self._key(RelinearizationKey, tabs[0], tabs[1], 0, round1)
        if evalKeyOut is None:
            return new
        evalKeyOut.__dict__.update(new.__dict__)
        return evalKeyOut


# ---- t-out-of-N threshold secret sharing ----------------------------------------------------------------------------------------------------------
def lagrange_coefficient(moduli, this, that):
    """Combiner.lagrangeCoeff (threshold.go:169-179) as residues: that (that - this)^-1 mod q for every modulus"""
    out = []
    for q in moduli:
        q = int(q)
        d = (int(that) - int(this)) % q
        if d == 0:
            raise RingHipError("lagrange_coefficient: the two points are equal modulo %d" % q)
        out.append(int(that) % q * pow(d, -1, q) % q)
    return out


class ShamirPolynomial:
    """multiparty.ShamirPolynomial: Value a list of PolyQP, the constant term first"""

    def __init__(self, value):
        self.Value = list(value)


class ShamirSecretShare(PolyQP):
    """multiparty.ShamirSecretShare: one poly modulo QP"""


class Thresholdizer:
    """multiparty.Thresholdizer over (ringQ, ringP).  A ShamirPublicPoint is a non-zero integer."""

    def __init__(self, ringQ, ringP=None, prng=None):
        _standard(ringQ, ringP)
        self.ringQ, self.ringP = ringQ, ringP
        self.prng = NewPRNG() if prng is None else prng
        self.usampler = UniformSampler(self.prng, ringQ, ringP)

    def _new(self):
        return self.ringQ.NewPoly(1), self.ringP.NewPoly(1) if self.ringP is not None else None

    def GenShamirPolynomial(self, threshold, secret, samples=None):
        """(:81-93): degree threshold - 1, constant term the secret's Value, the rest uniform.  samples: {"a": [(aQ (LQ, N), aP or None)] * (threshold - 1)}"""
        if threshold < 1:
            raise RingHipError("threshold should be >= 1")
        q, p = self._new()
        self.ringQ.CopyLvl(secret.Value.Q, q)
        if p is not None:
            self.ringP.CopyLvl(secret.Value.P, p)
        gen = [PolyQP(q, p)]
        for i in range(1, threshold):
            if samples is not None:
                aQ, aP = samples["a"][i - 1]
                q = DevicePoly.from_numpy(self.ringQ, np.asarray(aQ, dtype=np.uint64)[None])
                p = DevicePoly.from_numpy(self.ringP, np.asarray(aP, dtype=np.uint64)[None]) if self.ringP is not None else None
            else:
                q, p = self._new()
                self.usampler.Read(q, p)
            gen.append(PolyQP(q, p))
        return ShamirPolynomial(gen)

    def AllocateThresholdSecretShare(self):
        """(:96-98)"""
        return ShamirSecretShare(*self._new())

    def GenShamirSecretShare(self, recipient, secretPoly, shareOut):
        """(:102-104): the polynomial at the recipient's point, by Ring.EvalPolyScalar"""
        self.ringQ.EvalPolyScalar([c.Q for c in secretPoly.Value], int(recipient), shareOut.Q)
        if self.ringP is not None:
            self.ringP.EvalPolyScalar([c.P for c in secretPoly.Value], int(recipient), shareOut.P)

    def AggregateShares(self, *args, fused=None):
        """(:107-113), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        aggregate(self.ringQ, [s.Q for s in shares], out.Q, fused)
        if self.ringP is not None:
            aggregate(self.ringP, [s.P for s in shares], out.P, fused)


class Combiner:
    """multiparty.Combiner (NewCombiner :117-144): the Lagrange factors of `own` against every other point, computed on the host"""

    def __init__(self, ringQ, ringP, own, others, threshold):
        _standard(ringQ, ringP)
        self.ringQ, self.ringP, self.own, self.threshold = ringQ, ringP, int(own), int(threshold)
        self.moduli = [int(q) for q in ringQ.moduli] + ([int(p) for p in ringP.moduli] if ringP is not None else [])
        self.lagrangeCoeffs = {int(o): lagrange_coefficient(self.moduli, own, o) for o in others if int(o) != int(own)}

    def GenAdditiveShare(self, activesPoints, ownPoint, ownShare, skOut):
        """(:148-167): skOut.Value = ownShare times the product of the Lagrange factors of the first `threshold` active points, taken to Montgomery
        form (`one` = MForm(1) starts the product) for MulRNSScalarMontgomery.  skOut has no small coefficients afterwards (coeffs = None)."""
        if len(activesPoints) < self.threshold:
            raise RingHipError("cannot GenAdditiveShare: Not enough active players to combine threshold shares")
        prod = [1] * len(self.moduli)
        for active in activesPoints[:self.threshold]:
            if int(active) != int(ownPoint):
                prod = [a * b % q for a, b, q in zip(prod, self.lagrangeCoeffs[int(active)], self.moduli)]
        scal = [(x << 64) % q for x, q in zip(prod, self.moduli)]
        LQ = self.ringQ.L
        self.ringQ.MulRNSScalarMontgomery(ownShare.Q, scal[:LQ], skOut.Value.Q)
        if self.ringP is not None:
            self.ringP.MulRNSScalarMontgomery(ownShare.P, scal[LQ:], skOut.Value.P)
        skOut.coeffs = None


# ---- the collective refresh (multiparty_refresh.py; at the end: it builds on the classes above) ---------------------------------------------------
from .multiparty_refresh import (FUSED_REFRESH, AdditiveShare, AdditiveShareBigint, GetMinimumLevelForRefresh, NewAdditiveShare, NewAdditiveShareBigint,  # noqa: E402,F401
                                 MaskedTransformFunc, RefreshShare, big_from_rns, big_muldiv, big_sample, big_to_rns, mpbgv, mpckks, refresh_recode)

"""The collective refresh of the reference's multiparty/mpckks package on the device (imported into multiparty.py).

  AdditiveShareBigint          additive_shares.go: a big-integer block on the device (below)
  RefreshShare                 refresh.go: {EncToShareShare, ShareToEncShare, MetaData}
  GetMinimumLevelForRefresh    mpckks/utils.go:16-39, floats included
  mpckks.EncToShareProtocol    mpckks/sharing.go: GenShare :90-143, GetShare :150-186
  mpckks.ShareToEncProtocol    mpckks/sharing.go: GenShare :234-262, GetEncryption :266-283
  mpckks.MaskedLinearTransformationProtocol   mpckks/transform.go: GenShare :153-199, AggregateShares :202-216, Transform :220-300,
                               applyTransformAndScale :302-379 with transform = nil
  mpckks.RefreshProtocol       mpckks/refresh.go

The reference walks []*big.Int on the host, one coefficient at a time (SetCoefficientsBigint, PolyToBigintCentered, Mul / Quo).  Here a share
is a BLOCK of multiword integers that never leaves the device (csrc/mp_refresh.hip): npoly * n values of W 64-bit words, little-endian, two's
complement, word-major in memory; numpy() hands out (npoly, n, W).  n = 2 * slots; value i belongs to coefficient i * (N / n).

  big_sample      the mask law of sharing.go:120-129: logBound uniform bits sign-extended from bit logBound - 1.  Word w of value i of poly p is
                  the stream's word for (call, poly0 + p, row = w, i), block t = 0; no rejection
  big_to_rns      SetCoefficientsBigint + the spread of NTTSparseAndMontgomery: Euclidean residues, coefficient domain; the transform is Ring.NTT
                  of the spread poly, which equals the reference's sub-ring shortcut
  big_from_rns    PolyToBigintCentered: v - Q when v >= floor(Q / 2) -- note the >=
  big_muldiv      Quo(x * m, d), truncated toward zero
  refresh_recode  the three in one kernel (FUSED_REFRESH["refresh_recode"]) or composed from them: the same bits

Two rings (the masked transform with other output parameters) must be on ONE stream: the recode is enqueued on the output ring's stream and
the calls around it on each ring's own, and nothing orders two streams against each other.

The scale change of a refresh is x * int(scale_out) / ceil(scale_in): defaultScale is a truncation (transform.go:119) and inputScaleInt is .Int
plus one when that truncated (:364-370), which is a ceiling for a non-integer, whatever the comment there says.

Every arithmetic entry takes `samples=` in place of its PRNGs: {"e": int32 (npoly, N), "mask": a list of npoly lists of ints, or a block}; the
masked transform's GenShare draws two errors, so its "e" is the pair (decryption share's, re-encryption share's).

Refused by name: a non-nil MaskedLinearTransformationFunc (the reference runs a big-float FFT at prec >= logBound on the masked values; that
stays with the reference, like the big-float encoder), every coefficient-domain ciphertext (the reference's non-NTT sparse branch,
core/rlwe/utils.go:235-240, shadows its loop variable and zeroes the wrong coefficients, and at full slots its GetShare still applies INTT,
sharing.go:160: wider than the sparse case alone, on purpose), 2^logBound > Q_level, n > N_out, conjugate-invariant and 3N
rings, a modulus at the share's level of 2^511 or more.  Not built: binary serialisation of RefreshShare, the Go binding.

mpbgv (mpbgv/{sharing,transform,refresh}.go) is composed from calls that exist: KeySwitchProtocol's share with the zero key, UniformSampler on
ringT, bgv.Encoder's RingT2Q / RingQ2T / EncodeRingT / DecodeRingT, Ring.NTT, Add and Sub; its additive shares are ringT polys (AdditiveShare)."""
import math
import types

import numpy as np

from .keygen import _standard, _view
from .multiparty import KeySwitchProtocol, KeySwitchShare, _fused, _share_list, aggregate
from .ringhip import DevicePoly, RingHipError, U64P, _check, lib
from .sampling import UniformSampler

MAX_WORDS = 8
# the one-kernel share conversion of csrc/mp_refresh.hip (True) or its three calls (False); the measured choice: profiles/refresh.json.  The other
# families of a refresh (its key-switch shares, its aggregation) follow FUSED_MULTIPARTY; `fused=` overrides both per call.
FUSED_REFRESH = {"refresh_recode": True}


def words_for_bits(bits):
    """the words a signed value of magnitude below 2^bits is held in"""
    return max(1, (bits + 1 + 63) // 64)


def _host_words(x, count, who):
    x = int(x)
    if x < 0 or x >> (64 * count):
        raise RingHipError("%s: expected a non-negative integer of at most %d words" % (who, count))
    n = max(1, (x.bit_length() + 63) // 64)
    return np.array([(x >> (64 * w)) & ((1 << 64) - 1) for w in range(n)], dtype=np.uint64), n


class AdditiveShareBigint:
    """multiparty.AdditiveShareBigint for a batch of npoly ciphertexts: npoly * n integers of W words on the device.  bits: a bound on the
    magnitudes' bit length when the maker knows one (the host's check that a scale change fits reads it)."""

    def __init__(self, ring, n, W, npoly=1, bits=None):
        _standard(ring)
        n, W = int(n), int(W)
        if not 1 <= W <= MAX_WORDS:
            raise RingHipError("AdditiveShareBigint: %d words per value, a block has 1 to %d" % (W, MAX_WORDS))
        if n < 2 or n & (n - 1):
            raise RingHipError("AdditiveShareBigint: %d values per poly: a power of two, at least 2" % n)
        self.ring, self.n, self.W, self.npoly, self.bits = ring, n, W, int(npoly), bits
        self.words = self.npoly * W * n
        self._block = DevicePoly(ring.AtLevel(0), (self.words + ring.N - 1) // ring.N, 1)
        self.ptr = self._block.ptr

    def numpy(self):
        """(npoly, n, W) uint64 words, little-endian, two's complement"""
        rows = self._block.numpy().reshape(-1)[:self.words]
        return np.ascontiguousarray(rows.reshape(self.npoly, self.W, self.n).transpose(0, 2, 1))

    def upload(self, arr):
        arr = np.asarray(arr, dtype=np.uint64)
        if arr.shape != (self.npoly, self.n, self.W):
            raise RingHipError("AdditiveShareBigint: expected words of shape (%d, %d, %d)" % (self.npoly, self.n, self.W))
        buf = np.zeros(self._block.words, dtype=np.uint64)
        buf[:self.words] = arr.transpose(0, 2, 1).reshape(-1)
        _check(lib().rh_dev_upload(self.ring._h, self.ptr, buf.ctypes.data_as(U64P), buf.size))

    def to_ints(self):
        """npoly lists of n Python ints"""
        a, W = self.numpy(), self.W
        out = []
        for p in range(self.npoly):
            vals = []
            for i in range(self.n):
                v = sum(int(a[p, i, w]) << (64 * w) for w in range(W))
                vals.append(v - (1 << (64 * W)) if v >> (64 * W - 1) else v)
            out.append(vals)
        return out

    @classmethod
    def from_ints(cls, ring, values, W=None):
        """values: npoly lists of n ints (or one list); W: the words per value, by default what the largest magnitude needs"""
        if values and not isinstance(values[0], (list, tuple, np.ndarray)):
            values = [values]
        bits = max([int(v).bit_length() for row in values for v in row] + [1])
        W = words_for_bits(bits) if W is None else W
        s = cls(ring, len(values[0]), W, len(values), bits=bits)
        if bits > 64 * W - 1:
            raise RingHipError("AdditiveShareBigint: a value of %d bits does not fit %d words" % (bits, W))
        mask = (1 << 64) - 1
        s.upload(np.array([[[(int(v) >> (64 * w)) & mask for w in range(W)] for v in row] for row in values], dtype=np.uint64))
        return s

    def copy_to(self, other):
        if (other.n, other.W, other.npoly) != (self.n, self.W, self.npoly):
            raise RingHipError("AdditiveShareBigint: the shares differ in shape")
        if other.ptr != self.ptr:
            self.ring.AtLevel(0).CopyLvl(self._block, other._block)
        other.bits = self.bits


class AdditiveShare:
    """multiparty.AdditiveShare: Value a ringT DevicePoly batch"""

    def __init__(self, value):
        self.Value = value


def NewAdditiveShare(ringT, npoly=1):
    return AdditiveShare(ringT.NewPoly(npoly))


def NewAdditiveShareBigint(ring, n, W, npoly=1):
    return AdditiveShareBigint(ring, n, W, npoly)


class RefreshShare:
    """multiparty.RefreshShare (refresh.go)"""

    def __init__(self, e2s, s2e, metadata=None):
        self.EncToShareShare, self.ShareToEncShare, self.MetaData = e2s, s2e, metadata


def GetMinimumLevelForRefresh(lam, scale, nParties, moduli):
    """(mpckks/utils.go:16-39) -> (minLevel, logBound, ok), with the reference's float64 arithmetic"""
    scale = scale.Float64() if hasattr(scale, "Float64") else float(scale)
    logBound = lam + int(math.ceil(math.log2(scale)))
    maxBound = math.ceil(float(logBound) + math.log2(float(nParties)))
    minLevel, logQ, i = -1, 0.0, 0
    while logQ < maxBound:
        if i >= len(moduli):
            return 0, 0, False
        logQ += math.log2(float(int(moduli[i])))
        minLevel += 1
        i += 1
    if len(moduli) < minLevel:
        return 0, 0, False
    return minLevel, logBound, True


# ---- the kernels of csrc/mp_refresh.hip ---------------------------------------------------------------------------------------------------------
def big_sample(prng, share, logBound, call=None, poly0=0):
    """fills `share` with the masks of sharing.go:120-129 from the next call counter value of prng"""
    if not 1 <= logBound <= 64 * share.W - 1:
        raise RingHipError("big_sample: logBound %d out of range [1, %d] for %d words" % (logBound, 64 * share.W - 1, share.W))
    call = prng.next_call() if call is None else call
    _check(lib().rh_mp_big_sample(share.ring._h, prng._state, call, poly0, logBound, share.ptr, share.n, share.W, share.npoly))
    share.bits = logBound - 1
    return call


def _gap_ok(rl, share, out_npoly, who):
    if share.n > rl.N:
        raise RingHipError("%s: n > N_out: %d values per poly exceed the ring's degree %d" % (who, share.n, rl.N))
    if share.npoly != out_npoly:
        raise RingHipError("%s: the share and the poly batch hold different numbers of polys" % who)


def big_to_rns(rl, share, out, accumulate=0):
    """out (coefficient domain, dense at rl's level) = / += / -= the residues of the share's values at stride N / n"""
    _gap_ok(rl, share, out.npoly, "big_to_rns")
    if out.limbs != rl.level + 1:
        raise RingHipError("big_to_rns: the output is not at the ring view's level")
    _check(lib().rh_mp_big_to_rns(rl._h, rl.level, share.ptr, share.n, share.W, out.ptr, out.npoly, int(accumulate)))


def big_from_rns(rl, poly, share, accumulate=False):
    """share = / += the centred integers of limbs 0..rl.level of `poly` (coefficient domain, possibly with more limbs per poly) at stride N / n"""
    _gap_ok(rl, share, poly.npoly, "big_from_rns")
    _check(lib().rh_mp_big_from_rns(rl._h, rl.level, poly.ptr, poly.limbs, share.ptr, share.n, share.W, share.npoly, 1 if accumulate else 0))
    share.bits = None


def _quotient_bits(bits, m, d):
    """a bound on the bit length of Quo(x m, d) for |x| < 2^bits"""
    return max(bits + int(m).bit_length() - int(d).bit_length() + 1, 1)


def big_muldiv(share, m, d, out=None):
    """out = Quo(share * m, d), truncated toward zero (out: by default the share itself)"""
    out = share if out is None else out
    if (out.n, out.W, out.npoly) != (share.n, share.W, share.npoly):
        raise RingHipError("big_muldiv: the shares differ in shape")
    if int(d) <= 0:
        raise RingHipError("big_muldiv: the divisor must be positive")
    if share.bits is not None and _quotient_bits(share.bits, m, d) > 64 * share.W - 1:
        raise RingHipError("big_muldiv: the quotient may need %d bits and does not fit %d words" % (_quotient_bits(share.bits, m, d), share.W))
    mw, mn = _host_words(m, 2, "big_muldiv: the multiplier")
    dw, dn = _host_words(d, 4, "big_muldiv: the divisor")
    _check(lib().rh_mp_big_muldiv(share.ring._h, share.ptr, out.ptr, share.n, share.W, share.npoly, mw.ctypes.data_as(U64P), mn, dw.ctypes.data_as(U64P), dn))
    out.bits = None if share.bits is None else _quotient_bits(share.bits, m, d)


def recode_words(rl_in, m, d):
    """the words a value is held in on its way from rl_in's level through Quo(x m, d)"""
    qbits = math.prod(int(q) for q in rl_in.moduli[:rl_in.level + 1]).bit_length()
    W = words_for_bits(max(qbits, _quotient_bits(qbits, m, d)))
    if W > MAX_WORDS:
        raise RingHipError("refresh_recode: a value of %d bits needs more than the %d words of a block" % (max(qbits, _quotient_bits(qbits, m, d)), MAX_WORDS))
    return W


def refresh_recode(rl_out, out, m, d, n, src_poly=None, rl_in=None, src_share=None, accumulate=0, fused=None, scratch=None):
    """out (coefficient domain at rl_out's level) = / += / -= the residues of Quo(x m, d), x the centred integers of src_poly at rl_in's level
    (Transform) or the values of src_share (GenShare's second half).  fused: ONE kernel, no block in memory; composed: the three calls, through
    the block `scratch` (n values of at least the needed words per poly) or one allocated here"""
    if (src_poly is None) == (src_share is None):
        raise RingHipError("refresh_recode: the source is a poly (with rl_in) or a share, one of them")
    if n > rl_out.N:
        raise RingHipError("refresh_recode: n > N_out: %d values per poly exceed the target ring's degree %d" % (n, rl_out.N))
    if int(d) <= 0:
        raise RingHipError("refresh_recode: the divisor must be positive")
    mw, mn = _host_words(m, 2, "refresh_recode: the multiplier")
    dw, dn = _host_words(d, 4, "refresh_recode: the divisor")
    if src_poly is not None:
        W = recode_words(rl_in, m, d)
    else:
        W = src_share.W
        if src_share.bits is not None and _quotient_bits(src_share.bits, m, d) > 64 * W - 1:
            raise RingHipError("refresh_recode: the quotient may need %d bits and does not fit %d words" % (_quotient_bits(src_share.bits, m, d), W))
    if FUSED_REFRESH["refresh_recode"] if fused is None else bool(fused):
        _check(lib().rh_mp_refresh_recode(rl_in._h if src_poly is not None else None, rl_in.level if src_poly is not None else 0,
                                          src_poly.ptr if src_poly is not None else None, src_poly.limbs if src_poly is not None else 0,
                                          src_share.ptr if src_share is not None else None, n, W, rl_out._h, rl_out.level, out.ptr, out.npoly,
                                          mw.ctypes.data_as(U64P), mn, dw.ctypes.data_as(U64P), dn, int(accumulate)))
        return
    tmp = scratch
    if tmp is None:
        tmp = AdditiveShareBigint(rl_out, n, W, out.npoly)
    elif (tmp.n, tmp.W, tmp.npoly) != (n, W, out.npoly):
        raise RingHipError("refresh_recode: the scratch block must hold %d polys of %d values of %d words" % (out.npoly, n, W))
    if src_poly is not None:
        big_from_rns(rl_in, src_poly, tmp)
        big_muldiv(tmp, m, d)
    else:
        big_muldiv(src_share, m, d, tmp)
    big_to_rns(rl_out, tmp, out, accumulate)


# ---- mpckks ---------------------------------------------------------------------------------------------------------------------------------------
def _dslots(ring, ct):
    """2 * ct.Slots() on a standard ring"""
    return 2 << int(getattr(ct, "LogDimensions", ring.N.bit_length() - 2))


def _ntt_only(ct, who):
    """CKKS and BGV ciphertexts here are NTT-domain.  A coefficient-domain ciphertext is refused at EVERY gap, for two reasons that both lie in
    the reference: with gap > 1 its non-NTT sparse branch (core/rlwe/utils.go:235-240) shadows its loop variable and zeroes the wrong
    coefficients, and at any gap GetShare runs INTT on the sum whatever the ciphertext's domain (mpckks/sharing.go:160, mpbgv/sharing.go:110),
    so Transform is wrong for such an input there too."""
    if not ct.IsNTT:
        raise RingHipError("cannot %s: the ciphertext is not in the NTT domain: the reference's non-NTT sparse branch (core/rlwe/utils.go:235-240) "
                           "zeroes the wrong coefficients and its GetShare applies INTT whatever the domain (sharing.go:160); neither is "
                           "reproduced, at any gap" % who)


def _mask_share(ring, samples, n, npoly, W, logBound, prng):
    """the masks of one GenShare as a block of W words"""
    if samples is not None:
        m = samples["mask"]
        if isinstance(m, AdditiveShareBigint):
            if m.W == W:
                return m
            m = m.to_ints()
        s = AdditiveShareBigint.from_ints(ring, m, W)
        if (s.n, s.npoly) != (n, npoly):
            raise RingHipError("samples: the mask has another shape than the ciphertext batch's slots")
        s.bits = max(s.bits, logBound - 1)
        return s
    s = AdditiveShareBigint(ring, n, W, npoly)
    big_sample(prng, s, logBound)
    return s


class _CKKSSwitch(KeySwitchProtocol):
    """the KeySwitchProtocol both share protocols embed, with the zero key on either side"""

    def _zero_term(self, rl, ct, sk, negate, out, samples, fused):
        """out = ct[1] sk + e (E2S: GenShare(sk, zero)), or ct[1] (0 - sk) + e (S2E: GenShare(zero, sk))"""
        key = self._sk(sk, rl)
        if not negate:
            self._term(rl, ct, key, None, None, out, samples, _fused("keyswitch_share", fused))       # skB = None: the zero key costs nothing
            return
        if getattr(self, "_zero", None) is None or self._zero.limbs < rl.level + 1:
            self._zero = self.ringQ.NewPoly(1)
            self.ringQ.Sub(self._zero, self._zero, self._zero)
        zero = DevicePoly(rl, 1, rl.level + 1, ptr=self._zero.ptr, owner=self._zero)
        self._term(rl, ct, zero, key, None, out, samples, _fused("keyswitch_share", fused))


class EncToShareProtocol(_CKKSSwitch):
    """mpckks.EncToShareProtocol (sharing.go:21-186) over ringQ"""

    def GenShare(self, sk, logBound, ct, secretShareOut, publicShareOut, samples=None, fused=None):
        """(:90-143): secretShareOut = the party's masks M, publicShareOut = ct[1] sk + e - NTT(spread(M)) at min(ct level, share level).
        samples: {"e": int32 (npoly, N), "mask": ints or a block}"""
        _ntt_only(ct, "GenShare")
        level = self._level(ct, publicShareOut)
        rl = self.ringQ.AtLevel(level)
        if (1 << logBound) > math.prod(int(q) for q in self.ringQ.moduli[:level + 1]):
            raise RingHipError("cannot GenShare: ciphertext level is not large enough for refresh correctness")
        n = _dslots(self.ringQ, ct)
        if secretShareOut.n != n or secretShareOut.npoly != ct.Value[1].npoly:
            raise RingHipError("cannot GenShare: the secret share's shape is not the ciphertext batch's (2 * slots values per ciphertext)")
        if logBound > 64 * secretShareOut.W - 1:
            raise RingHipError("cannot GenShare: masks of %d bits do not fit the share's %d words" % (logBound, secretShareOut.W))
        mask = _mask_share(self.ringQ, samples, n, secretShareOut.npoly, secretShareOut.W, logBound, self.prng)
        mask.copy_to(secretShareOut)
        publicShareOut._resize(self.ringQ, level)
        self._zero_term(rl, ct, sk, False, publicShareOut.Value, samples, fused)
        buf = rl.NewPoly(secretShareOut.npoly)
        big_to_rns(rl, secretShareOut, buf)
        rl.NTT(buf, buf)
        rl.Sub(publicShareOut.Value, buf, publicShareOut.Value)

    def GetShare(self, secretShare, aggregatePublicShare, ct, secretShareOut):
        """(:150-186): secretShareOut = [secretShare +] centred(INTT(aggregate + ct[0])) at stride N / (2 slots)"""
        _ntt_only(ct, "GetShare")
        level = min(ct.Level(), aggregatePublicShare.Level())
        rl = self.ringQ.AtLevel(level)
        buf = self._masked(rl, ct, aggregatePublicShare)
        if secretShare is not None:
            secretShare.copy_to(secretShareOut)
        big_from_rns(rl, buf, secretShareOut, accumulate=secretShare is not None)

    def _masked(self, rl, ct, agg):
        """INTT(agg + ct[0]) at rl's level, dense"""
        c0, npoly, L = ct.Value[0], ct.Value[0].npoly, rl.level + 1
        buf = rl.NewPoly(npoly)
        row = lambda p, k: DevicePoly(rl, 1, L, ptr=p.ptr + k * p.limbs * rl.N * 8, owner=p)      # limbs 0..level of poly k, whatever p's level
        for k in range(npoly):
            rl.Add(row(agg.Value, k), row(c0, k), _view(buf, rl, k, 1))
        rl.INTT(buf, buf)
        return buf


class ShareToEncProtocol(_CKKSSwitch):
    """mpckks.ShareToEncProtocol (sharing.go:190-283) over ringQ"""

    def GenShare(self, sk, crs, metadata, secretShare, c0ShareOut, samples=None, fused=None):
        """(:234-262): c0ShareOut = -crs sk + e + NTT(spread(secretShare)).  crs: the CRP (a DevicePoly of one poly, shared by the batch);
        metadata: anything with LogDimensions.  samples: {"e": int32 (npoly, N)}"""
        if crs.limbs - 1 != c0ShareOut.Level():
            raise RingHipError("cannot GenShare: crs and c0ShareOut level must be equal")
        rl = self.ringQ.AtLevel(crs.limbs - 1)
        self._crp_term(rl, sk, crs, c0ShareOut.Value, samples, fused)
        buf = rl.NewPoly(secretShare.npoly)
        big_to_rns(rl, secretShare, buf)
        rl.NTT(buf, buf)
        rl.Add(c0ShareOut.Value, buf, c0ShareOut.Value)

    def _crp_term(self, rl, sk, crs, out, samples, fused):
        """out = -crs sk + e for every poly of the batch"""
        npoly = out.npoly
        c1 = crs
        if npoly > 1:                                      # the one CRP under every ciphertext of the batch
            c1 = rl.NewPoly(npoly)
            for k in range(npoly):
                rl.CopyLvl(crs, _view(c1, rl, k, 1))
        ct = types.SimpleNamespace(Value=[None, c1], IsNTT=True)
        self._zero_term(rl, ct, sk, True, out, samples, fused)

    def GetEncryption(self, c0Agg, crs, opOut):
        """(:266-283)"""
        if opOut.Degree() != 1:
            raise RingHipError("cannot GetEncryption: opOut must have degree 1")
        if c0Agg.Level() != crs.limbs - 1:
            raise RingHipError("cannot GetEncryption: c0Agg level must be equal to crs level")
        if opOut.Level() != crs.limbs - 1:
            raise RingHipError("cannot GetEncryption: opOut level must be equal to crs level")
        rl = self.ringQ.AtLevel(crs.limbs - 1)
        if c0Agg.Value.ptr != opOut.Value[0].ptr:
            rl.CopyLvl(c0Agg.Value, opOut.Value[0])
        for k in range(opOut.Value[1].npoly):
            rl.CopyLvl(crs, _view(opOut.Value[1], rl, k, 1))


_META = ("Scale", "LogDimensions", "IsBatched", "IsMontgomery", "IsNTT")


def _metadata(ct):
    return {k: getattr(ct, k) for k in _META if hasattr(ct, k)}


class MaskedLinearTransformationProtocol:
    """mpckks.MaskedLinearTransformationProtocol (transform.go) with transform = nil: ringQ_in / ringQ_out the rings of the input and output
    parameters (they may differ in degree), scale_out the output parameters' default scale"""

    def __init__(self, ringQ_in, ringQ_out, scale_out, noise_flooding, xe_sigma=3.2, prng=None):
        _standard(ringQ_in, ringQ_out)
        self.e2s = EncToShareProtocol(ringQ_in, noise_flooding, xe_sigma, prng)
        self.s2e = ShareToEncProtocol(ringQ_out, noise_flooding, xe_sigma, self.e2s.prng)
        self.prng = self.e2s.prng
        self.scale_out = scale_out
        value = scale_out.Value if hasattr(scale_out, "Value") else scale_out
        self.defaultScale = int(value)                    # the truncation of transform.go:119

    @staticmethod
    def inputScaleInt(scale):
        """.Int plus the Below correction (:364-370): a ceiling"""
        return math.ceil(scale.Value if hasattr(scale, "Value") else scale)

    def AllocateShare(self, levelDecrypt, levelRecrypt, npoly=1):
        """(:132-134)"""
        return RefreshShare(self.e2s.AllocateShare(levelDecrypt, npoly), self.s2e.AllocateShare(levelRecrypt, npoly))

    def SampleCRP(self, level, crs):
        """(:138-140): NTT domain"""
        return self.s2e.SampleCRP(level, crs)

    @staticmethod
    def _no_transform(transform, who):
        if transform is not None:
            raise RingHipError("cannot %s: a MaskedLinearTransformationFunc is not supported: the reference applies it in a big-float FFT at the mask's "
                               "precision, which stays with the reference (transform = None only)" % who)

    def GenShare(self, skIn, skOut, logBound, ct, crs, transform, shareOut, samples=None, fused=None):
        """(:153-199).  samples: {"e": (decryption share's, re-encryption share's), "mask": ...}"""
        self._no_transform(transform, "GenShare")
        if ct.Value[1].limbs - 1 < shareOut.EncToShareShare.Level():
            raise RingHipError("cannot GenShare: ct[1] level must be at least equal to EncToShareShare level")
        if crs.limbs - 1 != shareOut.ShareToEncShare.Level():
            raise RingHipError("cannot GenShare: crs level must be equal to ShareToEncShare")
        rin, rout = self.e2s.ringQ, self.s2e.ringQ
        n, npoly = _dslots(rin, ct), ct.Value[1].npoly
        if n > rout.N:
            raise RingHipError("cannot GenShare: n > N_out: %d values per ciphertext exceed the output ring's degree %d" % (n, rout.N))
        m, d = self.defaultScale, self.inputScaleInt(ct.Scale)
        W = words_for_bits(max(logBound, _quotient_bits(logBound, m, d)))
        if W > MAX_WORDS:
            raise RingHipError("cannot GenShare: masks of %d bits and their rescaled values need more than %d words" % (logBound, MAX_WORDS))
        mask = AdditiveShareBigint(rin, n, W, npoly)
        s1 = None if samples is None else {"e": samples["e"][0], "mask": samples["mask"]}
        s2 = None if samples is None else {"e": samples["e"][1]}
        self.e2s.GenShare(skIn, logBound, ct, mask, shareOut.EncToShareShare, samples=s1, fused=fused)
        shareOut.MetaData = _metadata(ct)
        rl = rout.AtLevel(crs.limbs - 1)
        out = shareOut.ShareToEncShare.Value
        self.s2e._crp_term(rl, skOut, crs, out, s2, fused)
        buf = rl.NewPoly(npoly)
        refresh_recode(rl, buf, m, d, n, src_share=mask, fused=fused)
        rl.NTT(buf, buf)
        rl.Add(out, buf, out)

    def AggregateShares(self, *args, fused=None):
        """(:202-216), or (list_of_shares, shareOut)"""
        shares, out = _share_list(args)
        for s in shares:
            if s.EncToShareShare.Level() != out.EncToShareShare.Level():
                raise RingHipError("cannot AggregateShares: all e2s shares must be at the same level")
            if s.ShareToEncShare.Level() != out.ShareToEncShare.Level():
                raise RingHipError("cannot AggregateShares: all s2e shares must be at the same level")
        aggregate(self.e2s.ringQ, [s.EncToShareShare.Value for s in shares], out.EncToShareShare.Value, fused)
        aggregate(self.s2e.ringQ, [s.ShareToEncShare.Value for s in shares], out.ShareToEncShare.Value, fused)
        out.MetaData = shares[0].MetaData

    def Transform(self, ct, transform, crs, share, ciphertextOut, fused=None):
        """(:220-300): ciphertextOut = (NTT(spread(Quo(x defaultScale, inputScaleInt))) + s2e share, crs), x = centred(INTT(e2s share + ct[0]))"""
        self._no_transform(transform, "Transform")
        _ntt_only(ct, "Transform")
        if ct.Level() < share.EncToShareShare.Level():
            raise RingHipError("cannot Transform: input ciphertext level must be at least equal to e2s level")
        if _metadata(ct) != share.MetaData:
            raise RingHipError("cannot Transform: input ciphertext MetaData is not equal to share.MetaData")
        maxLevel = crs.limbs - 1
        if maxLevel != share.ShareToEncShare.Level():
            raise RingHipError("cannot Transform: crs level and s2e level must be the same")
        rin, rout = self.e2s.ringQ, self.s2e.ringQ
        n = _dslots(rin, ct)
        if n > rout.N:
            raise RingHipError("cannot Transform: n > N_out: %d values per ciphertext exceed the output ring's degree %d" % (n, rout.N))
        if ciphertextOut.Level() != maxLevel or ciphertextOut.Value[0].npoly != ct.Value[0].npoly:
            raise RingHipError("cannot Transform: ciphertextOut must be at the crs level, with the input's batch size")
        rli = rin.AtLevel(min(ct.Level(), share.EncToShareShare.Level()))
        rlo = rout.AtLevel(maxLevel)
        x = self.e2s._masked(rli, ct, share.EncToShareShare)
        c0 = ciphertextOut.Value[0]
        refresh_recode(rlo, c0, self.defaultScale, self.inputScaleInt(ct.Scale), n, src_poly=x, rl_in=rli, fused=fused)
        rlo.NTT(c0, c0)
        rlo.Add(c0, share.ShareToEncShare.Value, c0)
        self.s2e.GetEncryption(KeySwitchShare(c0), crs, ciphertextOut)
        for k, v in share.MetaData.items():
            setattr(ciphertextOut, k, v)
        ciphertextOut.Scale = self.scale_out


class RefreshProtocol(MaskedLinearTransformationProtocol):
    """mpckks.RefreshProtocol (refresh.go): the masked transform with one set of parameters and no transform"""

    def __init__(self, ringQ, scale, noise_flooding, xe_sigma=3.2, prng=None):
        super().__init__(ringQ, ringQ, scale, noise_flooding, xe_sigma, prng)

    def GenShare(self, sk, logBound, ct, crs, shareOut, samples=None, fused=None):
        """(:46-48)"""
        super().GenShare(sk, sk, logBound, ct, crs, None, shareOut, samples=samples, fused=fused)

    def Finalize(self, ctIn, crs, share, opOut, fused=None):
        """(:57-59)"""
        self.Transform(ctIn, None, crs, share, opOut, fused=fused)


# ---- mpbgv: composed from calls that exist -------------------------------------------------------------------------------------------------------------
class _BGVSwitch(_CKKSSwitch):
    """the KeySwitchProtocol of the BGV share protocols: encoder is a bgv.Encoder over ringQ and T (its ringT holds the additive shares)"""

    def __init__(self, encoder, noise_flooding, xe_sigma=3.2, prng=None):
        super().__init__(encoder.ringQ, noise_flooding, xe_sigma, prng)
        self.encoder, self.ringT = encoder, encoder.ringT

    def _lift(self, rl, pT):
        """NTT(RingT2Q(level, true, pT)) at rl's level"""
        buf = rl.NewPoly(pT.npoly)
        self.encoder.RingT2Q(rl.level, True, pT, buf)
        rl.NTT(buf, buf)
        return buf


class BGVEncToShareProtocol(_BGVSwitch):
    """mpbgv.EncToShareProtocol (mpbgv/sharing.go:22-117)"""

    def GenShare(self, sk, ct, secretShareOut, publicShareOut, samples=None, fused=None):
        """(:91-99): secretShareOut = a uniform mask modulo T, publicShareOut = ct[1] sk + e - NTT(RingT2Q(mask)).
        samples: {"e": int32 (npoly, N), "mask": uint64 (npoly, n) modulo T}"""
        _ntt_only(ct, "GenShare")
        level = self._level(ct, publicShareOut)
        rl = self.ringQ.AtLevel(level)
        publicShareOut._resize(self.ringQ, level)
        self._zero_term(rl, ct, sk, False, publicShareOut.Value, samples, fused)
        pT = secretShareOut.Value
        if samples is not None:
            _check(lib().rh_dev_upload(self.ringT._h, pT.ptr, np.ascontiguousarray(np.asarray(samples["mask"], dtype=np.uint64)).ctypes.data_as(U64P), pT.words))
        else:
            UniformSampler(self.prng, self.ringT).Read(pT)
        rl.Sub(publicShareOut.Value, self._lift(rl, pT), publicShareOut.Value)

    def GetShare(self, secretShare, aggregatePublicShare, ct, secretShareOut):
        """(:106-117): secretShareOut = [secretShare +] RingQ2T(INTT(aggregate + ct[0]))"""
        _ntt_only(ct, "GetShare")
        level = min(ct.Level(), aggregatePublicShare.Level())
        rl = self.ringQ.AtLevel(level)
        buf = EncToShareProtocol._masked(self, rl, ct, aggregatePublicShare)
        if secretShare is None:
            self.encoder.RingQ2T(level, True, buf, secretShareOut.Value)
            return
        tmp = self.ringT.NewPoly(buf.npoly)
        self.encoder.RingQ2T(level, True, buf, tmp)
        self.ringT.Add(secretShare.Value, tmp, secretShareOut.Value)


class BGVShareToEncProtocol(_BGVSwitch):
    """mpbgv.ShareToEncProtocol (mpbgv/sharing.go:121-195)"""

    def GenShare(self, sk, crp, secretShare, c0ShareOut, samples=None, fused=None):
        """(:168-184): c0ShareOut = -crp sk + e + NTT(RingT2Q(secretShare)).  samples: {"e": int32 (npoly, N)}"""
        if crp.limbs - 1 != c0ShareOut.Level():
            raise RingHipError("cannot GenShare: crp and c0ShareOut level must be equal")
        rl = self.ringQ.AtLevel(crp.limbs - 1)
        ShareToEncProtocol._crp_term(self, rl, sk, crp, c0ShareOut.Value, samples, fused)
        rl.Add(c0ShareOut.Value, self._lift(rl, secretShare.Value), c0ShareOut.Value)

    def GetEncryption(self, c0Agg, crp, opOut):
        """(:188-195)"""
        if opOut.Degree() != 1:
            raise RingHipError("cannot GetEncryption: opOut must have degree 1")
        rl = self.ringQ.AtLevel(crp.limbs - 1)
        if c0Agg.Value.ptr != opOut.Value[0].ptr:
            rl.CopyLvl(c0Agg.Value, opOut.Value[0])
        for k in range(opOut.Value[1].npoly):
            rl.CopyLvl(crp, _view(opOut.Value[1], rl, k, 1))


class MaskedTransformFunc:
    """mpbgv.MaskedTransformFunc (mpbgv/transform.go:31-43): Func is a Python callable that receives the device value block the BGV encoder
    uses (bgv.DeviceValues, (npoly, n) uint64) and changes it in place"""

    def __init__(self, Decode, Func, Encode):
        self.Decode, self.Func, self.Encode = bool(Decode), Func, bool(Encode)


class MaskedTransformProtocol:
    """mpbgv.MaskedTransformProtocol (mpbgv/transform.go): encoder_in / encoder_out: bgv.Encoder of the input and output parameters"""

    def __init__(self, encoder_in, encoder_out, noise_flooding, xe_sigma=3.2, prng=None):
        if encoder_in.ringT.N != encoder_out.ringT.N or encoder_in.t != encoder_out.t:
            raise RingHipError("cannot NewMaskedTransformProtocol: the two parameter sets differ in plaintext ring")
        self.e2s = BGVEncToShareProtocol(encoder_in, noise_flooding, xe_sigma, prng)
        self.s2e = BGVShareToEncProtocol(encoder_out, noise_flooding, xe_sigma, self.e2s.prng)
        self.prng = self.e2s.prng

    def SampleCRP(self, level, crs):
        """(:78-80)"""
        return self.s2e.SampleCRP(level, crs)

    def AllocateShare(self, levelDecrypt, levelRecrypt, npoly=1):
        """(:83-85)"""
        return RefreshShare(self.e2s.AllocateShare(levelDecrypt, npoly), self.s2e.AllocateShare(levelRecrypt, npoly))

    def _apply(self, transform, mask, scale):
        """Decode, Func, Encode on a ringT batch (:101-123, :167-189): the mask itself when transform is None"""
        if transform is None:
            return mask
        from .bgv import DeviceValues
        ringT, n = self.e2s.ringT, self.e2s.ringT.N
        vals = DeviceValues(self.e2s.ringQ, mask.npoly, n)
        as_poly = DevicePoly(ringT, mask.npoly, 1, ptr=vals.ptr, owner=vals)       # the value block seen as ringT polys: copies stay on the device
        if transform.Decode:
            self.e2s.encoder.DecodeRingT(mask, scale, vals)
        else:
            ringT.CopyLvl(mask, as_poly)
        transform.Func(vals)
        out = ringT.NewPoly(mask.npoly)
        if transform.Encode:
            self.s2e.encoder.EncodeRingT(vals, scale, out)
        else:
            ringT.CopyLvl(as_poly, out)
        return out

    def GenShare(self, skIn, skOut, ct, crs, transform, shareOut, samples=None, fused=None):
        """(:89-129); Decode / Encode at ct.Scale (:105, :115).  samples: {"e": (decryption share's, re-encryption share's), "mask": ...}"""
        if ct.Level() < shareOut.EncToShareShare.Level():
            raise RingHipError("cannot GenShare: ct[1] level must be at least equal to EncToShareShare level")
        if crs.limbs - 1 != shareOut.ShareToEncShare.Level():
            raise RingHipError("cannot GenShare: crs level must be equal to ShareToEncShare")
        mask = AdditiveShare(self.e2s.ringT.NewPoly(ct.Value[1].npoly))
        s1 = None if samples is None else {"e": samples["e"][0], "mask": samples["mask"]}
        s2 = None if samples is None else {"e": samples["e"][1]}
        self.e2s.GenShare(skIn, ct, mask, shareOut.EncToShareShare, samples=s1, fused=fused)
        shareOut.MetaData = _metadata(ct)
        self.s2e.GenShare(skOut, crs, AdditiveShare(self._apply(transform, mask.Value, ct.Scale)), shareOut.ShareToEncShare, samples=s2, fused=fused)

    AggregateShares = MaskedLinearTransformationProtocol.AggregateShares

    def Transform(self, ct, transform, crs, share, ciphertextOut, fused=None):
        """(:149-198); Decode / Encode at ciphertextOut.Scale (:171, :181), the reference's asymmetry kept"""
        if _metadata(ct) != share.MetaData:
            raise RingHipError("cannot Transform: input ct.MetaData != share.MetaData")
        if ct.Level() < share.EncToShareShare.Level():
            raise RingHipError("cannot Transform: input ciphertext level must be at least equal to e2s level")
        maxLevel = crs.limbs - 1
        if maxLevel != share.ShareToEncShare.Level():
            raise RingHipError("cannot Transform: crs level and s2e level must be the same")
        if ciphertextOut.Level() != maxLevel or ciphertextOut.Value[0].npoly != ct.Value[0].npoly:
            raise RingHipError("cannot Transform: ciphertextOut must be at the crs level, with the input's batch size")
        mask = AdditiveShare(self.e2s.ringT.NewPoly(ct.Value[0].npoly))
        self.e2s.GetShare(None, share.EncToShareShare, ct, mask)
        pT = self._apply(transform, mask.Value, getattr(ciphertextOut, "Scale", 1))
        rlo = self.s2e.ringQ.AtLevel(maxLevel)
        rlo.Add(self.s2e._lift(rlo, pT), share.ShareToEncShare.Value, ciphertextOut.Value[0])
        self.s2e.GetEncryption(KeySwitchShare(ciphertextOut.Value[0]), crs, ciphertextOut)


class BGVRefreshProtocol(MaskedTransformProtocol):
    """mpbgv.RefreshProtocol (mpbgv/refresh.go)"""

    def __init__(self, encoder, noise_flooding, xe_sigma=3.2, prng=None):
        super().__init__(encoder, encoder, noise_flooding, xe_sigma, prng)

    def GenShare(self, sk, ct, crp, shareOut, samples=None, fused=None):
        super().GenShare(sk, sk, ct, crp, None, shareOut, samples=samples, fused=fused)

    def Finalize(self, ctIn, crp, share, opOut, fused=None):
        self.Transform(ctIn, None, crp, share, opOut, fused=fused)


mpbgv = types.SimpleNamespace(EncToShareProtocol=BGVEncToShareProtocol, ShareToEncProtocol=BGVShareToEncProtocol, MaskedTransformFunc=MaskedTransformFunc,
                              MaskedTransformProtocol=MaskedTransformProtocol, RefreshProtocol=BGVRefreshProtocol, NewAdditiveShare=NewAdditiveShare)
mpckks = types.SimpleNamespace(EncToShareProtocol=EncToShareProtocol, ShareToEncProtocol=ShareToEncProtocol,
                               MaskedLinearTransformationProtocol=MaskedLinearTransformationProtocol, RefreshProtocol=RefreshProtocol,
                               GetMinimumLevelForRefresh=GetMinimumLevelForRefresh, NewAdditiveShare=NewAdditiveShareBigint)

"""core/rlwe/ring_packing.go restated over the pinned oracle pieces and tests/rlwe_restatement.py: Expand (:475-594), Pack (:623-793), Split (:193-246),
Merge (:396-444), extract (:90-189), repack (:291-392), GenXPow2NTT (:795-833), getMinimumGap (:835-868); SwitchCiphertextRingDegreeNTT
(core/rlwe/element.go:250-287) and ring.MapSmallDimensionToLargerDimensionNTT (ring/operations.go:380-392); GaloisElementsForExpand / ...ForPack and
GenRingSwitchingKeys (core/rlwe/ring_packing_keys.go:106-109, :143-180).
TEST INFRASTRUCTURE ONLY: what the device path (rlwe.RingPackingEvaluator) is compared with bit for bit, itself pinned to decryption by
tests/test_ring_packing_oracle.py.

The loops are the reference's, line by line and one ciphertext at a time -- NOT the batched levels and plans of the device path.  Split forms its
odd half as the reference does: a multiplication by X^-1 in the NTT domain and a second inverse transform, and transforms the small rows with
the LARGE ring's table of roots (element.go:273).  Ciphertexts are lists [c0, c1] of (limbs, N) uint64 arrays in the NTT domain; maps of
ciphertexts are dicts; Galois keys: {element: rr.GadgetKey}."""
import numpy as np

import rlwe_restatement as rr
from oracle import ring_oracle as orc


class NoCiphertext(ValueError):
    """the reference's error returns"""


def _mul_scalar(x, s, mods):
    """MulScalarBigint (ring/operations.go:231-237): canonical x * s mod q_i"""
    return np.stack([((x[i].astype(object) * (int(s) % int(q))) % int(q)).astype(np.uint64) for i, q in enumerate(mods)])


def _mul(a, b, mods):
    return rr._vec("MUL_MONT", np.asarray(a, dtype=np.uint64), np.asarray(b[:len(mods)], dtype=np.uint64), mods)


def _sub(a, b, mods):
    return rr._vec("SUB", np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64), mods)


def gen_xpow2_ntt(N, mods, logN, div):
    """GenXPow2NTT (:795-833): X^(+-2^i), 0 <= i < logN, NTT domain, Montgomery form"""
    mods = [int(q) for q in mods]
    out = []
    for i in range(logN):
        idx = 1 << i
        if div:
            idx = N - idx
        if i == 0:
            p = np.zeros((len(mods), N), dtype=np.uint64)
            for j, q in enumerate(mods):
                p[j, idx] = (1 << 64) % q                                # MForm(1)
            out.append(rr.ntt(p, N, mods))
        else:
            out.append(_mul(out[i - 1], out[i - 1], mods))
    if div:
        out[0] = rr._vec("NEG", out[0], None, mods)
    return out


def get_minimum_gap(keys):
    """getMinimumGap (:835-868) -> (gap, logGap); the returned gap is the odd part the loop leaves"""
    gap, logGap = 0x7fffffffffffffff, 0
    for a, b in zip(keys, keys[1:]):
        if a > b:
            raise NoCiphertext("invalid index list: element must be sorted from smallest to largest")
        if a == b:
            raise NoCiphertext("invalid index list: contains duplicated elements")
        gap = min(gap, b - a)
        if gap == 1:
            break
    while gap & 1 == 0:
        logGap += 1
        gap >>= 1
    return gap, logGap


def galois_elements_for_expand(N, logN):
    """(ring_packing_keys.go:143-153)"""
    return [2 * N // (2 << i) + 1 for i in range(logN)]


def galois_elements_for_pack(N, logGap):
    """(ring_packing_keys.go:156-180), standard ring"""
    logN = N.bit_length() - 1
    if logGap > logN or logGap < 0:
        raise ValueError("cannot GaloisElementsForPack: logGap > logN || logGap < 0")
    out = [pow(5, 1 << i, 2 * N) for i in range(logGap)]
    if logGap == logN:
        out.append(2 * N - 1)
    return out


def expand(N, Q, P, ct, logGap, keys, xinv=None):
    """Expand (:475-594) on an NTT-domain ciphertext -> {index: ciphertext}.  xinv: the table in the place of XInvPow2NTT (the negative control)"""
    logN = N.bit_length() - 1
    level = ct[0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    xpow2 = gen_xpow2_ntt(N, mods, logN, True) if xinv is None else xinv
    ninv = pow(1 << logN, -1, rr.prod(mods))
    cts = {0: [_mul_scalar(np.asarray(c, dtype=np.uint64), ninv, mods) for c in ct]}
    gap = 1 << logGap
    for i in range(logN):
        n = 1 << i
        galEl = N // n + 1
        for j in range(0, n, gap):
            c0 = cts[j]
            tmp = rr.automorphism(N, Q, P, c0, keys[galEl], galEl)
            if j + n // gap > 0:
                c1 = [x.copy() for x in c0]
                c0[:] = [rr._add(c0[c], tmp[c], mods) for c in (0, 1)]
                c1 = [_sub(c1[c], tmp[c], mods) for c in (0, 1)]
                cts[j + n] = [_mul(c1[c], xpow2[i], mods) for c in (0, 1)]
            else:
                c0[:] = [rr._add(c0[c], tmp[c], mods) for c in (0, 1)]
    return cts


def pack(N, Q, P, cts, inputLogGap, zeroGarbageSlots, keys, xpow=None):
    """Pack (:623-793) on NTT-domain ciphertexts.  `cts` is CONSUMED as in the reference: its ciphertexts are scaled and combined in place and its
    entries move and vanish.  Returns cts[0] (None when the reference returns a nil ciphertext)."""
    if len(cts) == 0:
        raise NoCiphertext("len(cts) = 0")
    logN = N.bit_length() - 1
    ks = sorted(cts)
    level = cts[ks[0]][0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    xpow2 = gen_xpow2_ntt(N, mods, logN, False) if xpow is None else xpow
    if len(ks) > 1:
        gap, logGap = get_minimum_gap(ks)
    else:
        gap, logGap = N, logN
    logStart, logEnd = logN - inputLogGap, logN
    if not zeroGarbageSlots and gap > 0:
        logEnd -= logGap
    if logStart >= logEnd:
        raise NoCiphertext("gaps between ciphertexts is smaller than inputLogGap > N")
    ninv = pow(1 << (logEnd - logStart), -1, rr.prod(mods))
    for k in ks:
        ct = cts[k]
        ct[:] = [_mul_scalar(np.asarray(c, dtype=np.uint64), ninv, mods) for c in ct]
    for i in range(logStart, logEnd):
        t = 1 << (logN - 1 - i)
        x = xpow2[len(xpow2) - i - 1]
        galEl = 2 * N - 1 if i == 0 else pow(5, 1 << (i - 1), 2 * N)
        for jx in range(t):
            jy = jx + t
            a, b = cts.get(jx), cts.get(jy)
            tmpa = None
            if b is not None:
                b[:] = [_mul(b[c], x, mods) for c in (0, 1)]
                if a is not None:
                    tmpa = [_sub(a[c], b[c], mods) for c in (0, 1)]
                    a[:] = [rr._add(a[c], b[c], mods) for c in (0, 1)]
                else:
                    cts[jx] = cts[jy]
                del cts[jy]
            if a is not None:
                tmpa = rr.automorphism(N, Q, P, tmpa if b is not None else a, keys[galEl], galEl)
                a[:] = [rr._add(a[c], tmpa[c], mods) for c in (0, 1)]
            elif b is not None:
                tmpa = rr.automorphism(N, Q, P, b, keys[galEl], galEl)
                b[:] = [_sub(b[c], tmpa[c], mods) for c in (0, 1)]
    return cts.get(0)


class _LargeRoots:
    """the constants ring.NTTStandard gets at element.go:273: the small degree with the LARGE ring's RootsForward"""

    def __init__(self, sr, NOut):
        self.N, self.q, self.mred, self.bred, self.roots_fwd = NOut, sr.q, sr.mred, sr.bred, sr.roots_fwd


def switch_ring_degree_ntt(x, NOut, mods):
    """SwitchCiphertextRingDegreeNTT (element.go:250-287) on one (limbs, NIn) poly"""
    NIn = x.shape[1]
    if NIn > NOut:
        gap = NIn // NOut
        rows = []
        for j, q in enumerate(mods):
            sr = rr.subring(NIn, q)
            buff = orc.intt(x[j], sr)
            rows.append(orc.ntt(np.ascontiguousarray(buff[::gap]), _LargeRoots(sr, NOut)))
        return np.stack(rows)
    return np.repeat(np.asarray(x, dtype=np.uint64), NOut // NIn, axis=1)      # MapSmallDimensionToLargerDimensionNTT


def switch_ring_degree(x, NOut):
    """SwitchCiphertextRingDegree (element.go:293-312) on one (limbs, NIn) poly; the positions it does not write are left zero here"""
    NIn = x.shape[1]
    if NIn > NOut:
        return np.ascontiguousarray(x[:, ::NIn // NOut])
    out = np.zeros((x.shape[0], NOut), dtype=np.uint64)
    out[:, ::NOut // NIn] = x
    return out


def split(N, Q, P, ct, key, odd=True):
    """Split (:193-246): (ctEvenNHalf, ctOddNHalf) of degree N / 2; key: RingSwitchingKeys[logN][logN - 1]"""
    level = ct[0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    tmp = rr.apply_evaluation_key(N, Q, P, ct, key)
    even = [switch_ring_degree_ntt(c, N // 2, mods) for c in tmp]
    if not odd:
        return even, None
    xinv = gen_xpow2_ntt(N, mods, N.bit_length() - 1, True)[0]
    tmp = [_mul(c, xinv, mods) for c in tmp]
    return even, [switch_ring_degree_ntt(c, N // 2, mods) for c in tmp]


def merge(N, Q, P, even, odd, key):
    """Merge (:396-444) into degree N; key: RingSwitchingKeys[logN - 1][logN]"""
    if even is None:
        raise NoCiphertext("ctEvenNHalf cannot be nil")
    level = even[0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    ctN = [switch_ring_degree_ntt(c, N, mods) for c in even]
    if odd is not None:
        x = gen_xpow2_ntt(N, mods, N.bit_length() - 1, False)[0]
        tmp = [switch_ring_degree_ntt(c, N, mods) for c in odd]
        ctN = [rr._add(ctN[c], _mul(tmp[c], x, mods), mods) for c in (0, 1)]      # MulCoeffsMontgomeryThenAdd
    return rr.apply_evaluation_key(N, Q, P, ctN, key)


class Keys:
    """RingPackingEvaluationKey: P per use, RingSwitchingKeys[logNIn][logNOut], RepackKeys[logN] / ExtractKeys[logN] = {element: key}"""

    def __init__(self, Q, P, min_logN, max_logN, switching=None, repack=None, extract=None):
        self.Q, self.P, self.min_logN, self.max_logN = Q, P, min_logN, max_logN
        self.switching, self.repack, self.extract = switching or {}, repack or {}, extract or {}


def extract(keys, ct, idx, naive):
    """extract (:90-189) -> {index: ciphertext of degree 2^min_logN}"""
    Q, P = keys.Q, keys.P
    NMax = ct[0].shape[1]
    logNMax, logNMin = NMax.bit_length() - 1, keys.min_logN
    level = ct[0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    logNFactor = logNMax - logNMin
    NFactor = 1 << logNFactor
    ks = sorted(idx)
    _, logGap = get_minimum_gap(ks)
    tmp = {0: [np.array(c, dtype=np.uint64) for c in ct]}
    for i in range(logNFactor):
        t = 1 << i
        logGap = max(0, logGap - 1)
        for j in range(t):
            if tmp.get(j) is not None:
                n = NMax >> i
                tmp[j], tmp[j + t] = split(n, Q, P, tmp[j], keys.switching[(logNMax - i, logNMax - i - 1)])
    NMin = 1 << logNMin
    buckets = {}
    for i in ks:
        buckets.setdefault(i & (NFactor - 1), []).append(i // NFactor)
    out = {}
    for i in buckets:
        if naive:
            cts = {j: [x.copy() for x in tmp[i]] for j in buckets[i]}
            xinv = gen_xpow2_ntt(NMin, mods, logNMin, True)
            for b in range(logNMin):
                for j in cts:
                    if (j >> b) & 1:
                        cts[j] = [_mul(c, xinv[b], mods) for c in cts[j]]
        else:
            cts = expand(NMin, Q, P, tmp[i], logGap, keys.extract[logNMin])
        for j in buckets[i]:
            if j not in cts:
                raise NoCiphertext("invalid ciphertexts map: index i+j*(NFactor*gap)=%d is nil" % (i + j * (NFactor << logGap)))
            out[i + j * NFactor] = cts[j]
    return out


def repack(keys, cts, naive):
    """repack (:291-392) -> one ciphertext of degree 2^max_logN; `cts` is consumed.  The merge loop tests ctsLargeN[j + 1], not [j + t] (:377), as
    the reference does: a node with no even half fails with Merge's own text, or is dropped when [j + 1] is empty too."""
    Q, P = keys.Q, keys.P
    ks = sorted(cts)
    NMin = cts[ks[0]][0].shape[1]
    logNMin, logNMax = NMin.bit_length() - 1, keys.max_logN
    level = cts[ks[0]][0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    logNFactor = logNMax - logNMin
    NFactor = 1 << logNFactor
    small = [dict() for _ in range(NFactor)]
    for i in ks:
        small[i & (NFactor - 1)][i // NFactor] = cts[i]
    large = {}
    for i in range(NFactor):
        if naive:
            tmp = small[i]
            xpow = gen_xpow2_ntt(NMin, mods, logNMin, False)
            for l in range(logNMin):
                t = 1 << (logNMin - 1 - l)
                for jx in range(t):
                    jy = jx + t
                    a, b = tmp.get(jx), tmp.get(jy)
                    if b is not None:
                        b[:] = [_mul(b[c], xpow[len(xpow) - l - 1], mods) for c in (0, 1)]
                        if a is not None:
                            a[:] = [rr._add(a[c], b[c], mods) for c in (0, 1)]
                        else:
                            tmp[jx] = tmp[jy]
                        del tmp[jy]
            large[i] = tmp.get(0)
        elif len(small[i]) != 0:
            large[i] = pack(NMin, Q, P, small[i], logNMin, True, keys.repack[logNMin])
    for i in range(logNFactor - 1, -1, -1):
        t = 1 << i
        for j in range(t):
            if large.get(j) is not None or large.get(j + 1) is not None:
                n = 1 << (logNMax - i)
                large[j] = merge(n, Q, P, large.get(j), large.get(j + t), keys.switching[(logNMax - i - 1, logNMax - i)])
                large[j + t] = None
    return large.get(0)

"""The noise meters on the device: ring.Log2OfStandardDeviation and everything the reference measures through it.

  CenteredMoments, Log2OfStandardDeviation          ring/ring.go:503-543, :647-686; the PolyQP forms: ring/ringqp/ring.go:136-175
  NoisePublicKey, NoiseRelinearizationKey, NoiseGaloisKey(s), NoiseGadgetCiphertext, NoiseEvaluationKey     core/rlwe/utils.go:13-108
  NoiseRGSWCiphertext                                core/rgsw/utils.go
  Norm, NormStats                                    core/rlwe/utils.go:111-183

The moments of a poly are (n, S1 = sum x, S2 = sum x^2, min |x|, max |x|) over the centred coefficients x, as Python integers: exact, so
every float this module returns comes out of ONE finishing function on the same integers whichever way they were obtained.
FUSED_NOISE selects the kernels of csrc/noise.hip -- "moments": rh_ring_centered_moments, "gadget_phase": rh_rlwe_gadget_phase -- or the
reference's own sequence: the ring calls (MulCoeffsMontgomeryThenAdd, Add, MulScalarBigint, Sub, MulScalar) and a download with Python
integers.  `fused=` per call: a bool for both, or a dict with either key.

The finishing functions: var = (S2 - S1^2 / n) / (n - 1) as an exact rational (divisor n in NormStats), sqrt and log2 at 256 bits, one rounding
to float64.  The reference keeps running sums of 128-bit floats (ring.go) or of floats at the integers' own precision (NormStats) and rounds the
standard deviation to float64 before math.Log2; its results differ from these by that rounding alone.

Rings: the moments take every ring kind; the key-noise functions take what the key layer makes (standard rings, 3N rings with N % 8 == 0;
Galois keys on 3N rings stay refused)."""
import math
from fractions import Fraction

import numpy as np

from .ringhip import DevicePoly, Matrix3N, RingHipError, U64P, _check, lib

FUSED_NOISE = {"gadget_phase": True, "moments": True}
SCRATCH_CAP = 1 << 30        # bytes of phase output (outs x (Q + P rows)) one launch of a batched key measurement may hold
NO_PT = (1 << 64) - 1


def _use(fused, key):
    if fused is None:
        return bool(FUSED_NOISE[key])
    if isinstance(fused, dict):
        return bool(fused.get(key, FUSED_NOISE[key]))
    return bool(fused)


# ---- the finishing functions (host) -----------------------------------------------------------------------------------------------------------------
def _log2_exact(x):
    """log2 of a non-negative rational at 256 bits, rounded once to float64; -inf at 0"""
    import mpmath
    if x == 0:
        return -math.inf
    with mpmath.workprec(256):
        x = Fraction(x)
        return float(mpmath.log(mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator), 2))


def log2_std(n, S1, S2, divisor=None):
    """log2 sqrt((S2 - S1^2 / n) / divisor) from exact integers; divisor: n - 1 (Log2OfStandardDeviation, the default) or n (NormStats).
    A zero divisor (one coefficient) is the reference's 0 / 0: nan."""
    n, S1, S2 = int(n), int(S1), int(S2)
    divisor = n - 1 if divisor is None else int(divisor)
    if n == 0 or divisor == 0:
        return math.nan
    var = Fraction(n * S2 - S1 * S1, n * divisor)
    import mpmath
    if var == 0:
        return -math.inf
    with mpmath.workprec(256):
        v = mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator)
        return float(mpmath.log(mpmath.sqrt(v), 2))


def moments_of(values):
    """(n, S1, S2, min |x|, max |x|) of a list of integers"""
    xs = [int(v) for v in values]
    ab = [abs(v) for v in xs]
    return len(xs), sum(xs), sum(v * v for v in xs), min(ab), max(ab)


def NormStats(vec):
    """(:135-183): (log2 of the standard deviation with divisor N, log2 min |x|, log2 max |x|) of a list of integers; -inf where a value is 0"""
    n, S1, S2, lo, hi = moments_of(vec)
    return log2_std(n, S1, S2, divisor=n), _log2_exact(lo), _log2_exact(hi)


# ---- moments ----------------------------------------------------------------------------------------------------------------------------------------
def moments_words(L):
    return 3 * ((L + 2) * (L + 3) // 2) + 2 * L


def assemble_moments(words, mods, n):
    """(n, S1, S2, min |x|, max |x|) from one poly's output block of rh_ring_centered_moments (include/ringhip.h): the pair sums P_ij of the
    mixed-radix digits times R_i R_j, R_i = m_0 ... m_{i-1}"""
    L = len(mods)
    w = [int(v) for v in words]
    R = [1]
    for m in mods:
        R.append(R[-1] * int(m))
    M = R.pop()
    NP = (L + 2) * (L + 3) // 2

    def P(i, j):
        k = 3 * (i * (L + 2) - i * (i - 1) // 2 + j - i)
        return w[k] | (w[k + 1] << 64) | (w[k + 2] << 128)

    cnt = P(L, L + 1)
    Sv = sum(R[i] * P(i, L) for i in range(L))
    Sc = sum(R[i] * P(i, L + 1) for i in range(L))
    Svv = sum((1 if i == j else 2) * R[i] * R[j] * P(i, j) for i in range(L) for j in range(i, L))
    lo = sum(R[i] * w[3 * NP + i] for i in range(L))
    hi = sum(R[i] * w[3 * NP + L + i] for i in range(L))
    return int(n), Sv - M * cnt, Svv - 2 * M * Sc + M * M * cnt, lo, hi


def _basis(ringQ, ringP):
    mods = [int(q) for q in ringQ.moduli[:ringQ.level + 1]]
    if ringP is not None:
        mods += [int(p) for p in ringP.moduli[:ringP.level + 1]]
    return mods


def _check_polys(ringQ, q, ringP, p, gap):
    if q.limbs < ringQ.level + 1:
        raise RingHipError("poly has %d limbs, ring level needs %d" % (q.limbs, ringQ.level + 1))
    if (ringP is None) != (p is None):
        raise RingHipError("CenteredMoments: the P part goes with ringP")
    if ringP is not None:
        if ringP.N != ringQ.N:
            raise RingHipError("CenteredMoments: ringQ and ringP differ in degree")
        if p.limbs < ringP.level + 1 or p.npoly != q.npoly:
            raise RingHipError("CenteredMoments: the P part has fewer limbs than ringP's level, or another batch size")
    gap = int(gap)
    if gap < 1 or ringQ.N % gap:
        raise RingHipError("CenteredMoments: gap %d does not divide N = %d" % (gap, ringQ.N))
    return gap


def centered_moments(ringQ, q, ringP=None, p=None, gap=1, fused=None):
    """per poly of the coefficient-domain batch q (and p under ringP: one basis QP): (n, S1, S2, min |x|, max |x|) of the centred coefficients
    0, gap, 2 gap ...: x = CRT(residues) - M where that is >= floor(M / 2).  Blocks wider than the rings' levels (AtLevel views) are read at
    their own row stride."""
    gap = _check_polys(ringQ, q, ringP, p, gap)
    mods = _basis(ringQ, ringP)
    n = ringQ.N // gap
    if not _use(fused, "moments"):
        M = 1
        for m in mods:
            M *= m
        crt = [(M // m) * pow(M // m, -1, m) for m in mods]
        half = M >> 1
        hq = q.numpy()[:, :ringQ.level + 1]
        host = hq if p is None else np.concatenate([hq, p.numpy()[:, :ringP.level + 1]], axis=1)
        out = []
        for k in range(q.npoly):
            vs = [sum(int(host[k, i, j]) % mods[i] * crt[i] for i in range(len(mods))) % M for j in range(0, ringQ.N, gap)]
            out.append(moments_of([v - M if v >= half else v for v in vs]))
        return out
    W = moments_words(len(mods))
    r0 = ringQ.AtLevel(0)
    blk = DevicePoly(r0, (q.npoly * W + ringQ.N - 1) // ringQ.N + 1, 1)
    _check(lib().rh_ring_centered_moments(ringQ._h, ringQ.level, q.ptr, q.limbs, ringP._h if ringP is not None else None,
                                          ringP.level if ringP is not None else 0, p.ptr if p is not None else None, p.limbs if p is not None else 0,
                                          gap, q.npoly, blk.ptr))
    host = np.empty(blk.words, dtype=np.uint64)
    _check(lib().rh_dev_download(ringQ._h, host.ctypes.data_as(U64P), blk.ptr, host.size))
    return [assemble_moments(host[k * W:(k + 1) * W], mods, n) for k in range(q.npoly)]


def log2_of_standard_deviation(ringQ, q, ringP=None, p=None, fused=None):
    """ring.Log2OfStandardDeviation / ringqp's (divisor N - 1): one float per poly of the batch"""
    return [log2_std(n, S1, S2) for n, S1, S2, _, _ in centered_moments(ringQ, q, ringP, p, 1, fused)]


def CenteredMomentsQP(ringQ, ringP, poly, gap=1, fused=None):
    """the moments of a ringqp poly (rlwe.PolyQP of coefficient-domain batches) modulo QP; ringP / poly.P None: modulo Q"""
    return centered_moments(ringQ, poly.Q, ringP, poly.P if ringP is not None else None, gap, fused)


def Log2OfStandardDeviationQP(ringQ, ringP, poly, fused=None):
    """ringqp.Ring.Log2OfStandardDeviation (ring/ringqp/ring.go:136-175), one float per poly of the batch"""
    return log2_of_standard_deviation(ringQ, poly.Q, ringP, poly.P if ringP is not None else None, fused)


# ---- the phase of gadget ciphertexts ----------------------------------------------------------------------------------------------------------------
def _view(p, ring, first, count, limbs=None):
    limbs = p.limbs if limbs is None else limbs
    return DevicePoly(ring, count, limbs, ptr=p.ptr + first * p.limbs * ring.N * 8, owner=p)


def _lead(p, ring):
    """the leading limbs of a single poly as a block at the ring's level"""
    if p.limbs < ring.level + 1:
        raise RingHipError("a secret key or plaintext has fewer limbs than the key's level")
    return DevicePoly(ring, 1, ring.level + 1, ptr=p.ptr, owner=p)


def _rows_of(gct):
    """the rows of Value[i][j]: dpl[i] = len(Value[i]); J = min_i dpl[i] (utils.go:58); rows(j) = [row of Value[i][j] for every i]"""
    dpl = gct.digits_per_limb if gct.digits_per_limb is not None else [1] * gct.digits
    J = min(dpl)
    first = [sum(dpl[:i]) for i in range(len(dpl))]
    return J, [[f + j for f in first] for j in range(J)]


def _stack(ring, polys):
    out = DevicePoly(ring, len(polys), ring.level + 1)
    for k, p in enumerate(polys):
        ring.CopyLvl(_lead(p, ring), _view(out, ring, k, 1))
    return out


def _rings_of(gct):
    rq = gct.Q.ring.AtLevel(gct.LevelQ())
    rp = gct.P.ring.AtLevel(gct.LevelP()) if gct.P is not None else None
    return rq, rp


def gadget_phases(items, sks, pts, fused=None):
    """The phases behind every Noise* function, over many gadget ciphertexts in one launch sequence.  items: (gct, sk index, pt index or None)
    per key, all at the same levels of the same rings; sks: single secrets (SecretKey, or (Q, P) blocks); pts: single plaintext polys modulo Q;
    all NTT domain, Montgomery form.  Yields (outQ, outP or None) blocks of phases, key after key and within a key j = 0 .. J - 1,
    J = min_i len(Value[i]): sum_i (Value[i][j][0] + Value[i][j][1] sk) - pt P 2^(j pw2) on Q, NTT domain, Montgomery form (utils.go:62-88)."""
    if not items:
        return
    g0 = items[0][0]
    rq, rp = _rings_of(g0)
    for r in (rq, rp):
        if r is not None and r.kind == Matrix3N and r.ntt3n_layout is not None:
            raise RingHipError("noise: keys are held in the reference's order; measure them with Ring.ntt3n_layout = None")
    LQ, LP, N = rq.level + 1, (rp.level + 1 if rp is not None else 0), rq.N
    for g, _, _ in items:
        if (g.LevelQ(), g.LevelP()) != (g0.LevelQ(), g0.LevelP()) or g.Q.ring._h is not g0.Q.ring._h:
            raise RingHipError("noise: the gadget ciphertexts of one call share their rings and levels")
    Pb = 1
    if rp is not None:
        for m in rp.moduli[:LP]:
            Pb *= int(m)
    plans = [_rows_of(g) for g, _, _ in items]
    skQ = [s.Value.Q if hasattr(s, "Value") else s[0] for s in sks]
    skP = [s.Value.P if hasattr(s, "Value") else s[1] for s in sks]
    if not _use(fused, "gadget_phase"):
        for (g, si, pi), (J, rows) in zip(items, plans):
            yield _composed_phase(g, rq, rp, _lead(skQ[si], rq), _lead(skP[si], rp) if rp is not None else None,
                                  _lead(pts[pi], rq) if pi is not None else None, Pb, J, rows)
        return
    sq = _stack(rq, skQ)
    sp = _stack(rp, skP) if rp is not None else None
    pq = _stack(rq, pts) if pts else None
    mmax = max(len(rows[0]) for _, rows in plans)
    table = []
    for (g, si, pi), (J, rows) in zip(items, plans):
        pw2 = g.BaseTwoDecomposition
        for j in range(J):
            f = Pb << (j * pw2)
            scal = [(f << 64) % int(q) for q in rq.moduli[:LQ]] if pi is not None else [0] * LQ
            table.append([g.Q.ptr, g.P.ptr if g.P is not None else 0, g.digits, si, pi if pi is not None else NO_PT, len(rows[j])]
                         + rows[j] + [0] * (mmax - len(rows[j])) + scal)
    step = max(1, SCRATCH_CAP // ((LQ + LP) * N * 8))
    for o0 in range(0, len(table), step):
        rt = np.array(table[o0:o0 + step], dtype=np.uint64)
        oc = rt.shape[0]
        outQ = DevicePoly(rq, oc, LQ)
        outP = DevicePoly(rp, oc, LP) if rp is not None else None
        tdev = DevicePoly(rq.AtLevel(0), (rt.size + N - 1) // N + 1, 1)
        _check(lib().rh_rlwe_gadget_phase(rq._h, rp._h if rp is not None else None, rq.level, rp.level if rp is not None else 0,
                                          sq.ptr, sp.ptr if sp is not None else None, sq.npoly, pq.ptr if pq is not None else None,
                                          pq.npoly if pq is not None else 0, outQ.ptr, outP.ptr if outP is not None else None,
                                          rt.ctypes.data_as(U64P), oc, mmax, tdev.ptr, tdev.words))
        yield outQ, outP


def gadget_noise(items, sks, pts, fused=None):
    """per key the list over j < min_i len(Value[i]) of log2 of the standard deviation modulo QP of the key's phases (gadget_phases): INTT,
    IMForm and Log2OfStandardDeviation (utils.go:90-93) over every block"""
    if not items:
        return []
    rq, rp = _rings_of(items[0][0])
    stds = []
    for outQ, outP in gadget_phases(items, sks, pts, fused):
        outQ.layout = None
        rq.INTT(outQ, outQ); rq.IMForm(outQ, outQ)
        if rp is not None:
            outP.layout = None
            rp.INTT(outP, outP); rp.IMForm(outP, outP)
        stds += log2_of_standard_deviation(rq, outQ, rp, outP, fused)
    out, at = [], 0
    for g, _, _ in items:
        J = _rows_of(g)[0]
        out.append(stds[at:at + J])
        at += J
    return out


def _composed_phase(g, rq, rp, skQ, skP, pt, Pb, J, rows):
    """the reference's sequence on a copy of the key (utils.go:62-99): MulCoeffsMontgomeryThenAdd per row, Add over the RNS digits,
    MulScalarBigint(pt, P), then per j: Sub on Q and MulScalar(pt, 2^pw2)"""
    accQ = DevicePoly(rq, J, rq.level + 1)
    accP = DevicePoly(rp, J, rp.level + 1) if rp is not None else None
    for ring, tab, acc, sk in ((rq, g.Q, accQ, skQ), (rp, g.P, accP, skP)):
        if ring is None:
            continue
        tmp = ring.NewPoly(1)
        for j in range(J):
            a = _view(acc, ring, j, 1)
            for i, r in enumerate(rows[j]):
                ring.CopyLvl(_view(tab, ring, 2 * r, 1), tmp)
                ring.MulCoeffsMontgomeryThenAdd(_view(tab, ring, 2 * r + 1, 1), sk, tmp)
                if i == 0:
                    ring.CopyLvl(tmp, a)
                else:
                    ring.Add(a, tmp, a)
    if pt is not None:
        p = rq.NewPoly(1)
        rq.CopyLvl(pt, p)
        if rp is not None:
            rq.MulScalarBigint(p, Pb, p)
        for j in range(J):
            aq = _view(accQ, rq, j, 1)
            rq.Sub(aq, p, aq)
            rq.MulScalar(p, 1 << g.BaseTwoDecomposition, p)
    return accQ, accP


def _max_from_zero(stds):
    """the running maximum that starts at 0 (utils.go:83, :95): a noise below one reports 0"""
    m = 0.0
    for s in stds:
        m = max(m, s)
    return m


# ---- the reference's functions ----------------------------------------------------------------------------------------------------------------------
def NoisePublicKey(pk, sk, fused=None):
    """(:13-25): Log2OfStandardDeviation of Value[0] + Value[1] sk modulo QP: one gadget row without a plaintext"""
    from .rlwe import GadgetCiphertext
    row = GadgetCiphertext.from_device(pk.Q.ring, pk.P.ring if pk.P is not None else None, pk.Q, pk.P)
    return gadget_noise([(row, 0, None)], [sk], [], fused)[0][0]


def NoiseGadgetCiphertext(gct, pt, sk, fused=None):
    """(:51-102); pt: a poly modulo Q, NTT domain, Montgomery form"""
    return _max_from_zero(gadget_noise([(gct, 0, 0)], [sk], [pt], fused)[0])


def NoiseEvaluationKey(evk, skIn, skOut, fused=None):
    """(:105-108)"""
    return NoiseGadgetCiphertext(evk, skIn.Value.Q, skOut, fused)


def NoiseRelinearizationKey(rlk, sk, fused=None):
    """(:28-32): skIn = sk^2 by MulCoeffsMontgomery"""
    rq, _ = _rings_of(rlk)
    s = _lead(sk.Value.Q, rq)
    sk2 = rq.NewPoly(1)
    rq.MulCoeffsMontgomery(s, s, sk2)
    return NoiseGadgetCiphertext(rlk, sk2, sk, fused)


def NoiseGaloisKeys(keys, sk, fused=None):
    """{galEl: noise} for a list of Galois keys or a MemEvaluationKeySet, as ONE launch sequence over all keys: skOut_k = AutomorphismNTT(sk,
    galEl_k^-1 mod NthRoot) (:35-48), skIn = sk"""
    if hasattr(keys, "GaloisKeys"):
        keys = [keys.GaloisKeys[g] for g in sorted(keys.GaloisKeys)]
    keys = list(keys)
    if not keys:
        return {}
    rq, rp = _rings_of(keys[0])
    if rq.kind == Matrix3N:
        raise RingHipError("cannot NoiseGaloisKey: 3N rings have no automorphism (ring/automorphism.go:14-20: N must be a power of two)")
    sq = _lead(sk.Value.Q, rq)
    sp = _lead(sk.Value.P, rp) if rp is not None else None
    outQ = DevicePoly(rq, len(keys), rq.level + 1)
    outP = DevicePoly(rp, len(keys), rp.level + 1) if rp is not None else None
    sks = []
    for k, gk in enumerate(keys):
        nth = int(gk.NthRoot) or 2 * rq.N
        inv = pow(int(gk.GaloisElement), nth - 1, nth)
        rq.AutomorphismNTT(sq, inv, _view(outQ, rq, k, 1))
        if rp is not None:
            rp.AutomorphismNTT(sp, inv, _view(outP, rp, k, 1))
        sks.append((_view(outQ, rq, k, 1), _view(outP, rp, k, 1) if rp is not None else None))
    res = gadget_noise([(gk, k, 0) for k, gk in enumerate(keys)], sks, [sq], fused)
    return {int(gk.GaloisElement): _max_from_zero(r) for gk, r in zip(keys, res)}


def NoiseGaloisKey(gk, sk, fused=None):
    """(:35-48)"""
    return NoiseGaloisKeys([gk], sk, fused)[int(gk.GaloisElement)]


def NoiseRGSWCiphertext(ct, pt, sk, fused=None):
    """core/rgsw/utils.go: (noise of Value[0] against pt, of Value[1] against pt sk), both gadget ciphertexts in one launch"""
    rq, _ = _rings_of(ct.Value[0])
    p = _lead(pt, rq)
    ptsk = rq.NewPoly(1)
    rq.MulCoeffsMontgomery(p, _lead(sk.Value.Q, rq), ptsk)
    a, b = gadget_noise([(ct.Value[0], 0, 0), (ct.Value[1], 0, 1)], [sk], [p, ptsk], fused)
    return _max_from_zero(a), _max_from_zero(b)


def Norm(ct, dec, fused=None):
    """(:111-133): per ciphertext of the batch (log2 of the standard deviation with divisor N, log2 min |x|, log2 max |x|) of the decrypted
    plaintext's centred coefficients: Decryptor.Decrypt, INTT when IsNTT, the moments modulo Q at the ciphertext's level"""
    pt = dec.DecryptNew(ct)
    rq = dec.ringQ.AtLevel(ct.Level())
    v = pt.Value
    if pt.IsNTT:
        rq.INTT(v, v)
    return [(log2_std(n, S1, S2, divisor=n), _log2_exact(lo), _log2_exact(hi)) for n, S1, S2, lo, hi in centered_moments(rq, v, fused=fused)]

"""The reference's circuits/ckks/{minimax,comparison,inverse} and bootstrapping.SecretKeyBootstrapper restated over polynomial_restatement.py,
ckks_restatement.py and the key-layer restatements.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the device path against it bit for bit
(with the float64 bootstrapper, the device encoder's path), tests/test_minimax_oracle.py pins it to decryption in the reference's own test
set-up (with the bootstrapper and the encoder at big-float precision, as the reference runs them).

  minimax_composite_polynomial.go            parseCoeffs :244-259   NewPolynomial :18-38   MaxDepth :40-45   Evaluate :47-55
  minimax_composite_polynomial_evaluator.go  Evaluate :29-89
  comparison.go                              Sign :75-77   Step :81-103   Max :111-125   Min :133-147   stepdiff :149-206
  inverse.go                                 evaluateNew :87-198   GoldschmidtDivisionNew :208-299   IntervalNormalization :312-407
  bootstrapping/sk_bootstrapper.go           Bootstrap :32-46

One ciphertext at a time (a pr.Ct): a batch is a loop of the caller."""
import math
from fractions import Fraction

import numpy as np

import ckks_encoder_restatement as ce
import ckks_restatement as cr
import keygen_restatement as kr
import polynomial_restatement as pr
import rlwe_restatement as rr

S = cr.Scale


# ---- minimax_composite_polynomial.go ---------------------------------------------------------------------------------------------------------------
def parse_coeffs(row):
    """parseCoeffs (:244-259): big.Floats of round(3.32... x the longest string) bits"""
    prec = int(float(max(len(c) for c in row)) * 3.3219280948873626 + 0.5)
    return [cr.round_bits(Fraction(c), prec) for c in row], prec


def new_polynomial(rows):
    """NewPolynomial (:18-38): Chebyshev basis on [-1, 1]"""
    out = []
    for row in rows:
        co, prec = parse_coeffs(row)
        out.append(pr.Poly(pr.CHEBYSHEV, [(c, Fraction(0)) for c in co], (-1, 1), prec))
    return out


def max_depth(mcp):
    return max(p.depth() for p in mcp)


def chebyshev_row(mono):
    """sum mono[i] x^i on [-1, 1] -> its Chebyshev coefficients as exact decimal strings (dyadic rationals), from
    x^m = 2^(1 - m) sum' binom(m, (m - k) / 2) T_k over k = m, m - 2, ... >= 0 (the T_0 term halved)"""
    co = [Fraction(0)] * len(mono)
    for m, c in enumerate(mono):
        for k in range(m, -1, -2):
            co[k] += Fraction(c) * math.comb(m, (m - k) // 2) * Fraction(2 if k else 1, 2 ** m)
    out = []
    for v in co:
        digits = v.denominator.bit_length() - 1                                       # n / 2^d = n 5^d / 10^d
        assert v.denominator == 1 << digits
        n = abs(v.numerator) * 5 ** digits
        s = str(n) if digits == 0 else "%d.%0*d" % (n // 10 ** digits, digits, n % 10 ** digits)
        out.append(("-" if v < 0 else "") + s)
    return out


# CoeffsSignX2Cheby and CoeffsSignX4Cheby (:64, :73) from their monomial forms, 3/2 x - 1/2 x^3 and 35/16 x - 35/16 x^3 + 21/16 x^5 - 5/16 x^7
MONO_X2 = [0, Fraction(3, 2), 0, Fraction(-1, 2)]
MONO_X4 = [0, Fraction(35, 16), 0, Fraction(-35, 16), 0, Fraction(21, 16), 0, Fraction(-5, 16)]
X2, X4 = chebyshev_row(MONO_X2), chebyshev_row(MONO_X4)


def evaluate_exact(mcp, x):
    """Polynomial.Evaluate (:47-55) at the real rational x: each polynomial exactly, its value rounded to 256 bits for the next"""
    y = (Fraction(x), Fraction(0))
    for p in mcp:
        y = pr.evaluate_exact(p, (cr.round_bits(y[0], 256), cr.round_bits(y[1], 256)))
    return y


# ---- parameters and bootstrappers -------------------------------------------------------------------------------------------------------------------
class Params(pr.Params):
    """pr.Params with DefaultScale, the Galois key of the conjugation (an rlwe_restatement.GadgetKey) and the bootstrapper (or None)"""

    def __init__(self, N, Q, P, rlk, conj, default_scale, btp=None, nb=1, prec=53):
        pr.Params.__init__(self, N, Q, P, rlk, nb, prec)
        self.conj, self.default_scale, self.btp = conj, S(default_scale), btp

    def max_level(self):
        return len(self.Q) - 1


class SkBootstrapper:
    """SecretKeyBootstrapper on the float64 encoder (what the device runs): decrypt, decode, encode at the top level and DefaultScale, encrypt
    with the samples handed in.  samples: an iterator of (c1 (L, N) uniform, e (N,) ints), one pair per call."""

    def __init__(self, N, Q, sk, default_scale, samples, min_level=0):
        self.N, self.Q, self.sk, self.default_scale, self.samples = N, [int(q) for q in Q], sk, S(default_scale), iter(samples)
        self.counter, self.min_level = 0, min_level

    def values(self, ct):
        mods = self.Q[:ct.level() + 1]
        re_, im_ = ce.decode(kr.decrypt(ct.comps, self.sk, self.Q), self.N.bit_length() - 2, ct.scale.float64(), self.N, mods)
        return re_ + 1j * im_

    def plaintext(self, values):
        return ce.embed(values, self.N.bit_length() - 2, self.default_scale.float64(), self.N, self.Q)

    def bootstrap(self, ct):
        pt = self.plaintext(self.values(ct))
        c1, e = next(self.samples)
        self.counter += 1
        return pr.Ct(kr.encrypt_sk(self.sk, self.Q, len(self.Q) - 1, c1, e, pt), self.default_scale)


# ---- the encoder at big-float precision (encoder.go: the *bignum.Complex arm), for decryption checks beyond 53 bits -----------------------------------------
def _mp():
    import mpmath
    return mpmath


BIG_PREC = 256


def big_tables(m):
    """the m + 1 roots exp(2 pi i k / m) as two object arrays of mpf, and the rotation group"""
    mp = _mp()
    with mp.workprec(BIG_PREC):
        ang = [2 * mp.pi * k / m for k in range(m + 1)]
        return np.array([mp.cos(a) for a in ang], dtype=object), np.array([mp.sin(a) for a in ang], dtype=object), ce.rot_group(m)


_tables = {}


def _big_tables(m):
    if m not in _tables:
        _tables[m] = big_tables(m)
    return _tables[m]


def special_fft_big(re, im, m, inverse=False):
    """ce.special_fft / special_ifft on object arrays of mpf"""
    mp = _mp()
    rr_, ri_, rot = _big_tables(m)
    with mp.workprec(BIG_PREC):
        re, im = np.array(re, dtype=object), np.array(im, dtype=object)
        n = len(re)
        logn, logm = n.bit_length() - 1, m.bit_length() - 1
        cmul = lambda ar, ai, br, bi: (ar * br - ai * bi, ar * bi + ai * br)
        if not inverse:
            re, im = ce.bit_reverse(re, n), ce.bit_reverse(im, n)
            for loglen in range(1, logn + 1):
                ln, lenh, lenq = 1 << loglen, 1 << (loglen - 1), 4 << loglen
                idx = (rot[:lenh] & (lenq - 1)) << (logm - 2 - loglen)
                xr, xi = re.reshape(n // ln, ln), im.reshape(n // ln, ln)
                ur, ui = xr[:, :lenh], xi[:, :lenh]
                vr, vi = cmul(xr[:, lenh:], xi[:, lenh:], rr_[idx], ri_[idx])
                re, im = np.concatenate([ur + vr, ur - vr], axis=-1).reshape(n), np.concatenate([ui + vi, ui - vi], axis=-1).reshape(n)
            return re, im
        for loglen in range(logn, 0, -1):
            ln, lenh, lenq = 1 << loglen, 1 << (loglen - 1), 4 << loglen
            idx = (lenq - (rot[:lenh] & (lenq - 1))) << (logm - 2 - loglen)
            xr, xi = re.reshape(n // ln, ln), im.reshape(n // ln, ln)
            ur, ui, vr, vi = xr[:, :lenh], xi[:, :lenh], xr[:, lenh:], xi[:, lenh:]
            pr_, pi_ = cmul(ur - vr, ui - vi, rr_[idx], ri_[idx])
            re, im = np.concatenate([ur + vr, pr_], axis=-1).reshape(n), np.concatenate([ui + vi, pi_], axis=-1).reshape(n)
        return ce.bit_reverse(re / n, n), ce.bit_reverse(im / n, n)


def encode_big(re, im, scale, N, mods):
    """N / 2 slots (mpf, or anything mpf takes) -> (L, N) NTT-domain words: the canonical embedding inverted, times `scale` (a Fraction),
    rounded to the nearest integer"""
    mp = _mp()
    slots = N // 2
    with mp.workprec(BIG_PREC):
        re, im = special_fft_big([mp.mpf(v) for v in re], [mp.mpf(v) for v in im], 2 * N, inverse=True)
        sc = mp.mpf(scale.numerator) / mp.mpf(scale.denominator)
        ints = [int(mp.nint(v * sc)) for v in list(re) + list(im)]
    assert len(ints) == 2 * slots == N
    return rr.ntt(rr.rns(ints, mods), N, mods)


def decode_big(poly, scale, N, mods):
    """(L, N) NTT-domain words -> (re, im) object arrays of mpf"""
    mp = _mp()
    ints = rr.crt_centered(rr.intt(np.asarray(poly, dtype=np.uint64), N, mods), mods)
    with mp.workprec(BIG_PREC):
        sc = mp.mpf(scale.numerator) / mp.mpf(scale.denominator)
        vals = [mp.mpf(v) / sc for v in ints]
        return special_fft_big(vals[:N // 2], vals[N // 2:], 2 * N)


class SkBootstrapperBig:
    """SecretKeyBootstrapper as the reference runs it: values decoded to and encoded from big floats; samples from `rnd` (a random.Random)"""

    def __init__(self, N, Q, sk, default_scale, rnd, min_level=0):
        self.N, self.Q, self.sk, self.default_scale, self.rnd = N, [int(q) for q in Q], sk, S(default_scale), rnd
        self.counter, self.min_level = 0, min_level

    def encrypt(self, re, im, scale=None):
        scale = self.default_scale if scale is None else S(scale)
        pt = encode_big(re, im, scale.v, self.N, self.Q)
        c1, e = rr.uniform_poly(self.rnd, self.N, self.Q), rr.gaussian_coeffs(self.rnd, self.N)
        return pr.Ct(kr.encrypt_sk(self.sk, self.Q, len(self.Q) - 1, c1, e, pt), scale)

    def decrypt(self, ct):
        return decode_big(kr.decrypt(ct.comps, self.sk, self.Q), ct.scale.v, self.N, self.Q[:ct.level() + 1])

    def bootstrap(self, ct):
        self.counter += 1
        return self.encrypt(*self.decrypt(ct))


def _min_level(btp):
    return 0 if btp is None else btp.min_level


def _bootstrap(btp, ct):
    if btp is None:
        raise ValueError("the bootstrapper is nil")
    return btp.bootstrap(ct)


# ---- evaluator calls the circuits make --------------------------------------------------------------------------------------------------------------------
def copy_new(ct):
    return pr.Ct([x.copy() for x in ct.comps], ct.scale)


def conjugate_new(P, ct):
    """ConjugateNew (evaluator.go:1218-1229)"""
    return pr.Ct(rr.automorphism(P.N, P.Q, P.P, [np.ascontiguousarray(x) for x in ct.comps], P.conj, 2 * P.N - 1), ct.scale)


def add_sub_new(P, a, b, sub=False):
    level = min(a.level(), b.level())
    comps, scale = cr.add_sub(P.N, P.mods(level), a.at(level), a.scale, b.at(level), b.scale, sub, prec=P.prec)
    return pr.Ct(comps, scale)


def mul_const(P, ct, const):
    """Mul(ct, const, ct) (:646-683)"""
    ct.comps, ct.scale = cr.mul_scalar(P.N, P.mods(ct.level()), ct.comps, ct.scale, const, P.prec, P.nb)


def add_const(P, ct, const):
    """Add(ct, const, ct) (:82-101)"""
    ct.comps, ct.scale = cr.add_sub_scalar(P.N, P.mods(ct.level()), ct.comps, ct.scale, const, False, P.prec)


def mul_relin_rescale(P, a, b):
    out = pr.mul_new(P, a, b, True)
    pr.rescale(P, out)
    return out


def set_scale(P, ct, scale):
    """SetScale (:468-478)"""
    mul_const(P, ct, scale.div(ct.scale).v)
    ct.comps, _ = cr.rescale_to(P.N, P.mods(ct.level()), ct.comps, ct.scale, scale)
    ct.scale = scale


# ---- minimax_composite_polynomial_evaluator.go -----------------------------------------------------------------------------------------------------------
def evaluate(P, ct, mcp):
    """Evaluate (:29-89)"""
    btp, nb = P.btp, P.nb
    depth = max_depth(mcp) * nb
    if P.max_level() < depth + _min_level(btp):
        raise ValueError("parameters do not enable the evaluation of the minimax composite polynomial, required levels is %d but parameters only provide %d levels"
                         % (depth + _min_level(btp), P.max_level()))
    res = copy_new(ct)
    for poly in mcp:
        if res.level() < poly.depth() * nb + _min_level(btp):
            res = _bootstrap(btp, res)
        res = pr.evaluate(P, res, [poly], None, P.default_scale.div(S(2)))           # :56-66
        res.scale = res.scale.mul(S(2))                                              # :72
        pr.add_sub(P, res, conjugate_new(P, res))                                    # :74-81
    res.scale = ct.scale                                                             # :86
    return res


# ---- comparison.go ----------------------------------------------------------------------------------------------------------------------------------------
def step_polynomial(mcp):
    """:83-100"""
    last = mcp[-1]
    half = Fraction(1, 2)
    co = [None if c is None else (cr.round_bits(c[0] * half, last.prec), c[1]) for c in last.coeffs]
    co[0] = (cr.round_bits(co[0][0] + half, last.prec), co[0][1])
    return list(mcp[:-1]) + [pr.Poly(pr.CHEBYSHEV, co, (last.a, last.b), last.prec)]


def sign(P, ct, mcp):
    return evaluate(P, ct, mcp)


def step(P, ct, mcp):
    return evaluate(P, ct, step_polynomial(mcp))


def stepdiff(P, op0, op1, mcp):
    """:149-206"""
    btp, nb = P.btp, P.nb
    diff = add_sub_new(P, op0, op1, sub=True)
    if diff.level() < nb * 2:
        diff = _bootstrap(btp, diff)
    st = step(P, diff, mcp)
    if st.level() < nb:
        st = _bootstrap(btp, st)
    level = min(diff.level(), st.level())
    ratio = S(1)
    for i in range(nb):
        ratio = ratio.mul(S(P.Q[level - i]))
    ratio = ratio.div(diff.scale)
    mul_const(P, diff, ratio.v)                                                      # :187
    pr.rescale(P, diff)
    diff.scale = diff.scale.mul(ratio)                                               # :194
    return mul_relin_rescale(P, diff, st)


def maximum(P, op0, op1, mcp):
    return add_sub_new(P, stepdiff(P, op0, op1, mcp), op1)                           # :120


def minimum(P, op0, op1, mcp):
    return add_sub_new(P, op0, stepdiff(P, op0, op1, mcp), sub=True)                 # :142


# ---- inverse.go -------------------------------------------------------------------------------------------------------------------------------------------
def goldschmidt_iterations(N, scale, log2min):
    """:214-227"""
    prec = float(N // 2) / scale.float64()
    start, iters = 1 - 2.0 ** log2min, 1
    while start >= prec:
        start *= start
        iters += 1
    return max(iters, 3)


def goldschmidt_division(P, ct, log2min):
    """GoldschmidtDivisionNew (:208-299)"""
    btp, nb = P.btp, P.nb
    iters = goldschmidt_iterations(P.N, ct.scale, log2min)
    if btp is None and iters * nb > ct.level():
        raise ValueError("cannot GoldschmidtDivisionNew: ct.Level()=%d < depth=%d and rlwe.Bootstrapper is nil" % (ct.level(), iters * nb))
    a = copy_new(ct)
    mul_const(P, a, -1)
    b = copy_new(a)
    add_const(P, a, 2)
    add_const(P, b, 1)
    needs = lambda x: btp is not None and (x.level() == btp.min_level or x.level() == nb - 1)
    for _ in range(1, iters):
        if needs(b):
            b = btp.bootstrap(b)
        if needs(a):
            a = btp.bootstrap(a)
        b = mul_relin_rescale(P, b, b)
        if needs(b):
            b = btp.bootstrap(b)
        tmp = mul_relin_rescale(P, a, b)
        set_scale(P, a, tmp.scale)                                                   # :289
        a = add_sub_new(P, a, tmp)                                                   # :293
    return a


def normalization_constants(log2max):
    """:318-338 -> the c of every iteration, in float64"""
    L = 2.45
    n = math.ceil(log2max / math.log2(L))
    return [2.0 / math.sqrt(27 * math.pow(L, 2 * (float(n) - 1 - float(i)))) for i in range(int(n))]


def interval_normalization(P, ct, log2max):
    """IntervalNormalization (:312-407) -> (ctNorm, ctNormFac)"""
    btp, nb = P.btp, P.nb
    norm, fac = copy_new(ct), None
    for c in normalization_constants(log2max):
        if norm.level() < _min_level(btp) + 4 * nb:
            norm = _bootstrap(btp, norm)
        if fac is not None and (fac.level() == _min_level(btp) or fac.level() == nb - 1):
            fac = _bootstrap(btp, fac)
        z = copy_new(norm)
        mul_const(P, z, c)                                                           # :346
        pr.rescale(P, z)
        z = mul_relin_rescale(P, z, z)                                               # :356-362
        mul_const(P, z, -1)
        add_const(P, z, 1)                                                           # :365-372
        if z.level() < _min_level(btp) + nb:
            z = _bootstrap(btp, z)
        fac = z if fac is None else mul_relin_rescale(P, fac, z)
        norm = mul_relin_rescale(P, norm, z)
    return norm, fac


def inverse(P, ct, log2min, log2max, fulldomain=False, mcp=None):
    """evaluateNew (:87-198)"""
    btp, nb = P.btp, P.nb
    fac = None
    if log2max > 0:
        cinv, fac = interval_normalization(P, ct, log2max)
    else:
        cinv = copy_new(ct)
    sgn = None
    if fulldomain:
        sgn = evaluate(P, cinv, mcp)
        if sgn.level() < _min_level(btp) + nb:
            sgn = _bootstrap(btp, sgn)
        if cinv.level() < _min_level(btp) + nb:
            cinv = _bootstrap(btp, cinv)
        cinv = mul_relin_rescale(P, cinv, sgn)
    cinv = goldschmidt_division(P, cinv, log2min)
    post = (nb if fac is not None or fulldomain else 0) + (nb if fulldomain else 0)
    if fac is not None:
        if cinv.level() < _min_level(btp) + post:
            cinv = _bootstrap(btp, cinv)
        if fac.level() < _min_level(btp) + post:
            fac = _bootstrap(btp, fac)
        cinv = mul_relin_rescale(P, cinv, fac)
    if fulldomain:
        cinv = mul_relin_rescale(P, cinv, sgn)
    return cinv


def inverse_negative(P, ct, log2min, log2max):
    """EvaluateNegativeDomainNew (:73-85)"""
    neg = copy_new(ct)
    mul_const(P, neg, -1)
    out = inverse(P, neg, log2min, log2max)
    mul_const(P, out, -1)
    return out

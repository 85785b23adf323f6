"""CPU: circuits/ckks/mod1.  The package's 256-bit coefficients (mod1.py: ApproximateCos, ChebyshevApproximation) pinned to the functions they
approximate, within bounds derived below; tests/mod1_restatement.py (what the GPU tests compare the device evaluator with) pinned to
decryption under a real key at the reference's own setting and bound; the literal's JSON and Depth; the host-side half of the package held to
the restatement.

The approximation bounds.  There is no Go bit pattern to compare with, so each set of coefficients is held to a bound its construction gives:

  Chebyshev interpolation (SinContinuous, CosContinuous).  On [-K', K'] with t = x / K' and z = 2 pi K' the Jacobi-Anger expansions are
  cos(z t) = J_0(z) + 2 sum_k (-1)^k J_2k(z) T_2k(t) and sin(z t) = 2 sum_k (-1)^k J_2k+1(z) T_2k+1(t): the Chebyshev coefficients are
  a_k = 2 J_k(z) in absolute value.  The interpolant at the n + 1 Chebyshev nodes differs from f by at most 2 sum_{k > n} |a_k| (truncation
  plus aliasing), so  max |p - f| <= 4 sum_{k > n} |J_k(2 pi K')|  on the whole interval.

  Han-Ki interpolation (CosDiscrete).  p interpolates g(u) = cos(2 pi u) at the n shifted nodes u_i = (t_i - 1/4) / 2^r, so for every u
  |p(u) - g(u)| <= max |g^(n)| / n! prod |u - u_i| <= (2 pi)^n / n! prod_i |u - u_i|, evaluated here at every sample of the nodes'
  intervals [i - 1/dev, i + 1/dev], |i| < K.

Both are evaluated at 256 bits; 2^-150 is allowed on top for the roundings of the construction itself (the elimination of `solve` loses a few
dozen of its 256 bits)."""
import functools
import math
import random
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_restatement as ce
import ckks_restatement as cr
import mod1_restatement as mr
import polynomial_restatement as pr
import rlwe_restatement as rr
from oracle import primes

S = cr.Scale
LOGN, LOGQ, LOGP, H, LOGSCALE = 10, [55] + [60] * 12 + [53], [61] * 5, 192, 45          # mod1_evaluator_test.go:25-31
# mod1_evaluator_test.go:83-125, and the default of bootstrapping/default_parameters.go (K = 16, degree 30, r = 3)
LITERALS = {
    "SineContinuousWithArcSine": dict(LevelQ=12, Mod1Type=mr.SIN_CONTINUOUS, LogMessageRatio=8, K=14, Mod1Degree=127, Mod1InvDegree=7, LogScale=60),
    "CosDiscrete": dict(LevelQ=12, Mod1Type=mr.COS_DISCRETE, LogMessageRatio=8, K=12, Mod1Degree=30, DoubleAngle=3, LogScale=60),
    "CosContinuous": dict(LevelQ=12, Mod1Type=mr.COS_CONTINUOUS, LogMessageRatio=4, K=325, Mod1Degree=177, DoubleAngle=4, LogScale=60),
    "Default": dict(LevelQ=12, Mod1Type=mr.COS_DISCRETE, LogMessageRatio=8, K=16, Mod1Degree=30, DoubleAngle=3, LogScale=60),
}
SLACK = Fraction(1, 1 << 150)


def mp256():
    import mpmath
    mp = mpmath.mp.clone()
    mp.prec = 256
    return mp


@functools.lru_cache(maxsize=None)
def raw_coefficients(name):
    """the package's coefficients before the nil-ing and the sqrt2pi factor, as Fractions"""
    import matrix_fhe_lattigo_amd as rh
    lit = LITERALS[name]
    r = lit.get("DoubleAngle", 0)
    if lit["Mod1Type"] == mr.COS_DISCRETE:
        return tuple(rh.mod1.ApproximateCos(lit["K"], lit["Mod1Degree"], float(1 << lit["LogMessageRatio"]), r))
    f = "sin2pi" if lit["Mod1Type"] == mr.SIN_CONTINUOUS else "cos2pi"
    return tuple(rh.mod1.ChebyshevApproximation(f, lit["Mod1Degree"], float(lit["K"]) / 2.0 ** r))


def clenshaw(mp, coeffs, t):
    b1 = b2 = mp.mpf(0)
    for c in reversed(coeffs[1:]):
        b1, b2 = 2 * t * b1 - b2 + c, b1
    return t * b1 - b2 + coeffs[0]


@pytest.mark.parametrize("name", ["SineContinuousWithArcSine", "CosContinuous"])
def test_chebyshev_coefficients_within_the_bessel_tail_bound(name):
    mp = mp256()
    lit = LITERALS[name]
    n, Ks = lit["Mod1Degree"], mp.mpf(lit["K"]) / 2 ** lit.get("DoubleAngle", 0)
    co = [mp.mpf(c.numerator) / c.denominator for c in raw_coefficients(name)]
    assert len(co) == n + 1
    z = 2 * mp.pi * Ks
    bound = 4 * sum(abs(mp.besselj(k, z)) for k in range(n + 1, n + 400))
    f = mp.sin if lit["Mod1Type"] == mr.SIN_CONTINUOUS else mp.cos
    rng = random.Random(name)
    ts = [mp.mpf(-1), mp.mpf(1), mp.mpf(0)] + [mp.mpf(rng.uniform(-1, 1)) for _ in range(300)]
    worst = max(abs(clenshaw(mp, co, t) - f(z * t)) for t in ts)
    print("%s: max |p - f| = 2^%.2f, bound 4 sum |J_k(2 pi K')| = 2^%.2f" % (name, float(mp.log(worst, 2)), float(mp.log(bound, 2))))
    assert worst <= bound + mp.mpf(SLACK.numerator) / SLACK.denominator
    assert bound < mp.mpf(2) ** -30                                                     # the literals are chosen so that the approximation is not the limit


def han_ki_nodes(mp, K, degree, dev, r):
    """the shifted nodes of cosine.genNodes (:160-234) from the package's genDegrees: t = i +- cos(pi j / deg_i) / dev, u = (t - 1/4) / 2^r"""
    import matrix_fhe_lattigo_amd as rh
    deg, totdeg = rh.mod1.genDegrees(degree, K, dev)
    assert deg[0] + 2 * sum(deg[1:]) == totdeg and totdeg <= degree + 1 and all(d >= 1 for d in deg)      # an interval i > 0 stands for +-i
    t = [mp.mpf(0)] if deg[0] % 2 else []
    for i in range(K - 1, 0, -1):
        for j in range(deg[i]):
            w = mp.cos(mp.pi * j / deg[i]) / dev
            t += [i + w, -i - w]
    for j in range(deg[0] // 2):
        w = mp.cos(mp.pi * j / deg[0]) / dev
        t += [w, -w]
    assert len(t) == totdeg
    return [(x - mp.mpf(0.25)) / 2 ** r for x in t]


@pytest.mark.parametrize("name", ["CosDiscrete", "Default"])
def test_han_ki_coefficients_within_the_interpolation_bound(name):
    mp = mp256()
    lit = LITERALS[name]
    K, r, dev = lit["K"], lit["DoubleAngle"], float(1 << lit["LogMessageRatio"])
    co = [mp.mpf(c.numerator) / c.denominator for c in raw_coefficients(name)]
    nodes = han_ki_nodes(mp, K, lit["Mod1Degree"], dev, r)
    n = len(nodes)
    assert len(co) == n
    lead = (2 * mp.pi) ** n / mp.factorial(n)
    Ks = mp.mpf(K) / 2 ** r
    rng = random.Random(name)
    worst = worst_bound = mp.mpf(0)
    for i in range(-K + 1, K):
        for e in [-1.0, 1.0, 0.0] + [rng.uniform(-1, 1) for _ in range(6)]:
            u = (mp.mpf(i) + mp.mpf(e) / dev - mp.mpf(0.25)) / 2 ** r
            err = abs(clenshaw(mp, co, u / Ks) - mp.cos(2 * mp.pi * u))
            bound = lead * abs(mp.fprod(u - v for v in nodes))
            assert err <= bound + mp.mpf(SLACK.numerator) / SLACK.denominator, (i, e)
            worst, worst_bound = max(worst, err), max(worst_bound, bound)
    for v in nodes[::3]:                                                                # it IS the interpolant: exact at the nodes
        assert abs(clenshaw(mp, co, v / Ks) - mp.cos(2 * mp.pi * v)) < mp.mpf(2) ** -150
    print("%s: %d nodes, max |p - f| = 2^%.2f, max bound = 2^%.2f" % (name, n, float(mp.log(worst, 2)), float(mp.log(worst_bound, 2))))


def test_parameters_follow_the_reference_and_the_restatement(rh):
    Q0 = primes.gen_moduli(LOGN + 1, LOGQ, LOGP)[0][0]
    for name, lit in LITERALS.items():
        L = rh.mod1.ParametersLiteral(**lit)
        p = rh.mod1.NewParametersFromLiteral(Q0, L)
        e = mr.params(Q0, L.LevelQ, L.LogScale, L.Mod1Type, L.LogMessageRatio, L.K, L.DoubleAngle, L.Mod1InvDegree, raw_coefficients(name))
        assert (p.QDiff, p.Sqrt2Pi, p.DoubleAngle, p.K) == (e.qdiff, e.sqrt2pi, e.double_angle, e.K)
        assert [None if c is None else (c.re, c.im) for c in p.Mod1Poly.Coeffs] == e.poly.coeffs
        assert (p.Mod1Poly.IsOdd, p.Mod1Poly.IsEven, p.Mod1Poly.A, p.Mod1Poly.B, p.Mod1Poly.prec) == (e.poly.is_odd, e.poly.is_even, e.poly.a, e.poly.b, 256)
        assert (p.Mod1InvPoly is None) == (e.inv_poly is None)
        if e.inv_poly is not None:
            assert [None if c is None else (c.re, c.im) for c in p.Mod1InvPoly.Coeffs] == e.inv_poly.coeffs and not p.Mod1InvPoly.IsEven
        assert L.Depth() == mr.depth(L.Mod1Type, L.K, L.Mod1Degree, L.DoubleAngle, L.Mod1InvDegree)
        assert p.MessageRatio() == 2.0 ** L.LogMessageRatio and p.ScalingFactor().Value == 2 ** 60
        assert p.IntervalShrinkFactor() == 2.0 ** p.DoubleAngle and p.KShrinked() == L.K / 2.0 ** p.DoubleAngle
    assert [rh.mod1.ParametersLiteral(**LITERALS[k]).Depth() for k in LITERALS] == [10, 8, 12, 8]     # 7 + 3; 5 + 3; 8 + 4; 5 + 3
    rng = random.Random(9)
    for _ in range(50):                                                                 # the 128-bit square root of the targetScale loop
        v = Fraction(rng.getrandbits(120) + 1, 1 << rng.randrange(0, 70))
        assert rh.mod1.ScaleSqrt(v).Value == mr.scale_sqrt(S(v)).v
    assert rh.mod1.ScaleSqrt(1 << 120).Value == 1 << 60 and mr.scale_sqrt(S(Fraction(9, 4))).v == Fraction(3, 2)
    a = mr.scale_sqrt(S(2)).v
    assert abs(a * a - 2) < Fraction(1, 1 << 126) and a == cr.round_bits(a, 128)
    with pytest.raises(rh.RingHipError, match="invalid Mod1Type"):
        rh.mod1.NewParametersFromLiteral(Q0, rh.mod1.ParametersLiteral(Mod1Type=3, K=2, Mod1Degree=3))


def test_literal_json_round_trip(rh):
    """mod1_evaluator_test.go:48-70, and the bytes encoding/json writes for that literal"""
    L = rh.mod1.ParametersLiteral(**LITERALS["SineContinuousWithArcSine"])
    data = L.MarshalBinary()
    assert data == b'{"LevelQ":12,"LogScale":60,"Mod1Type":1,"Scaling":0,"LogMessageRatio":8,"K":14,"Mod1Degree":127,"DoubleAngle":0,"Mod1InvDegree":7}'
    assert rh.mod1.ParametersLiteral().UnmarshalBinary(data) == L
    M = rh.mod1.ParametersLiteral(Scaling=0.5, **LITERALS["CosContinuous"])
    assert b'"Scaling":0.5,' in M.MarshalBinary() and rh.mod1.ParametersLiteral().UnmarshalBinary(M.MarshalBinary()) == M and M != L


# ---- the three subtests of mod1_evaluator_test.go through the restatement, decrypted ----------------------------------------------------------
class Keyed:
    """the reference's test ring: LogN 10, LogQ 55, 12 x 60, 53, five 61-bit P, a ternary secret of Hamming weight 192, scale 2^45"""
    _one = None

    def __new__(cls):
        if cls._one is None:
            self = object.__new__(cls)
            Q, Pk = primes.gen_moduli(LOGN + 1, LOGQ, LOGP)
            self.N, self.Q, self.Pk = 1 << LOGN, [int(q) for q in Q], [int(p) for p in Pk]
            self.rnd = random.Random(2024)
            co = [0] * self.N
            for i in self.rnd.sample(range(self.N), H):
                co[i] = self.rnd.choice((-1, 1))
            self.sk = rr.Secret(self.N, co)
            self.rlk = rr.relin_key(self.rnd, self.sk, self.Q, self.Pk, len(self.Q) - 1, len(self.Pk) - 1)
            self.P = pr.Params(self.N, self.Q, self.Pk, self.rlk)
            cls._one = self
        return cls._one

    def encrypt(self, values, scale, tag):
        words = ce.embed_coeffs(np.asarray(values) + 0j, LOGN - 1, float(scale), self.N, self.Q)
        comps, _ = rr.encrypt(random.Random("enc %s" % tag), self.sk, rr.crt_centered(words, self.Q), self.Q, len(self.Q) - 1)
        return pr.Ct(comps, S(scale))

    def decrypt(self, ct):
        mods = self.Q[:ct.level() + 1]
        acc = rr._vec("ADD", rr._vec("MUL_MONT", np.asarray(ct.comps[1], dtype=np.uint64), self.sk.rows(mods), mods), np.asarray(ct.comps[0], dtype=np.uint64), mods)
        re_, im_ = ce.decode(acc, LOGN - 1, ct.scale.float64(), self.N, mods)
        return re_ + 1j * im_


@functools.lru_cache(maxsize=None)
def restated_parameters(name):
    lit = LITERALS[name]
    return mr.params(Keyed().Q[0], lit["LevelQ"], lit["LogScale"], lit["Mod1Type"], lit["LogMessageRatio"], lit["K"], lit.get("DoubleAngle", 0),
                     lit.get("Mod1InvDegree", 0), raw_coefficients(name))


def test_vector(evm, seed):
    """newTestVectorsMod1 (:180-204)"""
    rng = np.random.default_rng(seed)
    K, Qd = evm.K - 1, evm.qdiff * 2.0 ** evm.log_message_ratio
    values = np.round(rng.uniform(-K, K, 1 << (LOGN - 1))) * Qd + rng.uniform(-1, 1, 1 << (LOGN - 1))
    values[0] = K * Qd + 0.5
    return values


test_vector.__test__ = False


def scale_up(k, ct, s):
    """ScaleUp (schemes/ckks/evaluator.go:456-465)"""
    ct.comps, _ = cr.mul_scalar(k.N, k.Q[:ct.level() + 1], ct.comps, ct.scale, min(int(s.v), (1 << 64) - 1))
    ct.scale = ct.scale.mul(s)


def normalised(k, evm, values, tag):
    """evaluateMod1 up to the call of the mod1 evaluator (:140-152): the input of EvaluateNew, at level 12"""
    ct = k.encrypt(values, 2 ** LOGSCALE, tag)
    ratio = 2.0 ** evm.log_message_ratio
    scale = S(2.0 ** math.floor(math.log2(float(k.Q[0]) / ratio) + 0.5)).div(ct.scale)
    scale_up(k, ct, S(float(math.floor(scale.float64() + 0.5))))
    scale = S(2 ** evm.log_scale).div(ct.scale).div(S(ratio))
    scale_up(k, ct, S(float(math.floor(scale.float64() + 0.5))))
    ct.comps, ct.scale = cr.mul_scalar(k.N, k.Q[:ct.level() + 1], ct.comps, ct.scale, 1 / (evm.K * evm.qdiff))
    pr.rescale(k.P, ct)
    return ct


def plaintext_circuit(evm, values, arcsine):
    """:158-175"""
    ratio = 2.0 ** evm.log_message_ratio
    x = np.sin(6.28318530717958 * (values / ratio / evm.qdiff))
    if arcsine:
        x = np.arcsin(x)
    return x * ratio * evm.qdiff / 6.28318530717958


def avg_log2_prec(want, have):
    """getPrecisionStats (schemes/ckks/precision.go:106-204), as tests/test_polynomial_oracle.py applies it"""
    out = []
    for part in (np.real, np.imag):
        err = np.abs(part(np.asarray(have)) - part(np.asarray(want)))
        out.append(float(np.mean([LOGSCALE if e == 0 else -math.log2(e) for e in err])))
    return out


@pytest.mark.parametrize("name", ["SineContinuousWithArcSine", "CosDiscrete", "CosContinuous"])
def test_reference_subtests_decrypt_to_the_reference_bound(name):
    """VerifyTestVectors with LogDefaultScale: average precision of both parts >= LogDefaultScale - (LogN + 2) = 33 bits (precision.go:92-103)"""
    k, evm = Keyed(), restated_parameters(name)
    values = test_vector(evm, 17)
    ct = normalised(k, evm, values, name)
    assert ct.level() == evm.level_q
    out = mr.evaluate(k.P, ct, evm)
    depth = mr.depth(evm.type, int(evm.K), evm.poly.degree(), evm.double_angle, 0 if evm.inv_poly is None else evm.inv_poly.degree())
    assert out.level() == evm.level_q - depth and out.scale.v == ct.scale.v
    re_, im_ = avg_log2_prec(plaintext_circuit(evm, values, evm.inv_poly is not None) + 0j, k.decrypt(out))
    print("%s: avg log2 precision: real %.2f imag %.2f" % (name, re_, im_))
    assert min(re_, im_) >= LOGSCALE - (LOGN + 2)

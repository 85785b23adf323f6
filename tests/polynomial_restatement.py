"""The reference's polynomial evaluation for CKKS restated over ckks_restatement.py and the oracle: utils/bignum/polynomial.go,
circuits/common/polynomial/{polynomial,power_basis,polynomial_evaluator,polynomial_evaluator_sim}.go and
circuits/ckks/polynomial/{polynomial,polynomial_evaluator,polynomial_evaluator_sim}.go.
TEST INFRASTRUCTURE ONLY: the GPU tests compare the device path against it bit for bit, tests/test_polynomial_oracle.py pins it to exact
rational arithmetic and to decryption under a real key.

A coefficient is a pair of Fractions (re, im) or None (nil); a polynomial is a Poly below; a ciphertext is a Ct: a list of (limbs, N) uint64
arrays in the NTT domain with its Scale.  One ciphertext at a time: a batch is a loop of the caller.

big.Float rule (see ckks_restatement.py): z.Add / z.Sub on a z that has a precision round to it, which is what Factorize's in-place Add and Sub
do with the precision of the coefficient (53 bits for a float64)."""
import math
from fractions import Fraction

import numpy as np

import ckks_encoder_restatement as ce
import ckks_restatement as cr
import rlwe_restatement as rr

MONOMIAL, CHEBYSHEV = 0, 1
DELTA = float(cr.PREC - 12)                                              # rlwe.ScalePrecision - 12 (polynomial.go:148, polynomial_evaluator.go:242)


# ---- utils/bignum/polynomial.go -------------------------------------------------------------------------------------------------------------
def optimal_split(log_degree):
    """OptimalSplit (:14-23)"""
    s = log_degree >> 1
    a = (1 << s) + (1 << (log_degree - s)) + log_degree - s - 3
    b = (1 << (s + 1)) + (1 << (log_degree - s - 1)) + log_degree - s - 4
    return s + 1 if a > b else s


def split_degree(n):
    """SplitDegree (power_basis.go:34-52)"""
    assert n > 0
    if n & (n - 1) == 0:
        return n // 2, n // 2
    k = (n - 1).bit_length() - 1
    return (1 << k) - 1, n + 1 - (1 << k)


class Poly:
    """bignum.Polynomial (:25-28, :104-111) with polynomial.Polynomial's fields (polynomial.go:17-35)"""

    def __init__(self, basis, coeffs, interval=(0, 0), prec=53):
        self.basis, self.prec, self.a, self.b = basis, prec, Fraction(interval[0]), Fraction(interval[1])
        self.coeffs = [None if c is None else c if isinstance(c, tuple) else (Fraction(complex(c).real), Fraction(complex(c).imag)) for c in coeffs]
        self.is_odd = self.is_even = True                                # :108-109
        self.max_deg, self.lead, self.lazy = len(self.coeffs) - 1, True, False    # polynomial.go:28-35
        self.level, self.scale = 0, None

    def degree(self):
        return len(self.coeffs) - 1                                      # :149-151

    def depth(self):
        return int(math.ceil(math.log2(float(self.degree()))))          # :144-146

    def keeps(self, i):
        return not (self.is_even or self.is_odd) or (i & 1 == 0 and self.is_even) or (i & 1 == 1 and self.is_odd)

    def change_of_basis(self):
        """ChangeOfBasis (:119-141): big.Float precisions 53 (SetFloat64) and 64 (SetInt64)"""
        if self.basis == MONOMIAL:
            return Fraction(1), Fraction(0)
        num = cr.round_bits(self.b - self.a, 53)                         # :126
        return cr.round_bits(2 / num, 64), cr.round_bits(cr.round_bits(-self.b - self.a, 53) / num, 53)   # :129, :132-135


def factorize(p, n):
    """bignum Factorize (:258-314) inside polynomial.Polynomial.Factorize (polynomial.go:38-58): p = X^n pq + pr, T_n pq + pr for Chebyshev"""
    assert n >= p.degree() >> 1
    rnd = lambda c: (cr.round_bits(c[0], p.prec), cr.round_bits(c[1], p.prec))
    pr = list(p.coeffs[:n])                                              # :266-271
    pq = [None] * (p.degree() - n + 1)
    pq[0] = p.coeffs[n]                                                  # :276-278
    for i in range(n + 1, p.degree() + 1):
        c = p.coeffs[i]
        if c is None or not p.keeps(i):
            continue
        if p.basis == MONOMIAL:
            pq[i - n] = c                                                # :287
        else:
            j = i - n
            pq[j] = rnd((c[0] + c[0], c[1] + c[1]))                      # :294-295
            pr[n - j] = rnd((pr[n - j][0] - c[0], pr[n - j][1] - c[1])) if pr[n - j] is not None else (-c[0], -c[1])   # :297-303
    out = []
    for co in (pq, pr):
        q = Poly(p.basis, co, (p.a, p.b), p.prec)
        q.is_odd, q.is_even, q.lead, q.lazy, q.max_deg = p.is_odd, p.is_even, False, False, 0     # :308-311; the zero value of the wrapper
        out.append(q)
    out[0].max_deg = p.max_deg                                           # polynomial.go:45
    out[1].max_deg = n - 1 if p.max_deg == p.degree() else p.max_deg - (p.degree() - n + 1)       # :47-51
    out[0].lead = p.lead                                                 # :53-55
    return out


def evaluate_exact(p, x):
    """the value of p at the complex rational x = (re, im), exactly; Chebyshev after the affine map of change_of_basis"""
    mul = lambda u, v: (u[0] * v[0] - u[1] * v[1], u[0] * v[1] + u[1] * v[0])
    co = [(Fraction(0), Fraction(0)) if c is None else c for c in p.coeffs]
    if p.basis == MONOMIAL:
        y = co[-1]
        for c in reversed(co[:-1]):
            y = mul(y, x)
            y = (y[0] + c[0], y[1] + c[1])
        return y
    s, k = p.change_of_basis()
    t, prev, y = (x[0] * s + k, x[1] * s), (Fraction(1), Fraction(0)), co[0]
    two_x = (2 * t[0], 2 * t[1])
    for c in co[1:]:
        m = mul(t, c)
        y = (y[0] + m[0], y[1] + m[1])
        nxt = mul(two_x, t)
        prev, t = t, (nxt[0] - prev[0], nxt[1] - prev[1])
    return y


# ---- the simulator (polynomial_evaluator_sim.go of both packages) ---------------------------------------------------------------------------
class Sim:
    def __init__(self, Q, nb=1):
        self.Q, self.nb = [int(q) for q in Q], nb

    def depth(self, degree):
        return self.nb * (degree.bit_length() - 1)                       # PolynomialDepth (ckks sim :26-33)

    def rescale(self, op):
        level, scale = op
        for _ in range(self.nb):                                         # :36-41
            scale = scale.div(cr.Scale(self.Q[level]))
            level -= 1
        return level, scale

    def mul(self, a, b):
        return min(a[0], b[0]), a[1].mul(b[1])                           # :44-49

    def baby_step(self, lead, level, scale):
        if lead:
            for i in range(self.nb):                                     # :57-61
                scale = scale.mul(cr.Scale(self.Q[level - i]))
        return level, scale

    def giant_step(self, lead, level, scale, xpow_scale):
        top = level if lead else level + self.nb                         # :71-82
        qi = 1
        for i in range(self.nb):
            qi *= self.Q[top - i]
        return level + self.nb, scale.mul(cr.Scale(qi)).div(xpow_scale)  # :84-86

    def gen_power(self, pb, n):
        """SimPowerBasis.GenPower (common sim :25-38); pb: dict power -> (level, scale)"""
        if n < 2:
            return
        a, b = split_degree(n)
        self.gen_power(pb, a)
        self.gen_power(pb, b)
        pb[n] = self.rescale(self.mul(pb[a], pb[b]))


def log2_delta(s, t):
    """Scale.Log2Delta (core/rlwe/scale.go:140-149)"""
    d = abs(s.v - t.v) / max(s.v, t.v)
    return float("inf") if d == 0 else -(math.log2(d.numerator) - math.log2(d.denominator))


def recurse_ps(sim, log_split, target_level, p, pb, out_scale, fired=None):
    """recursePS (polynomial.go:109-153) -> (baby-step polynomials with level and scale, (level, scale) of the combination).  fired: a list
    that collects the scale pairs which miss the delta check (:148-150) instead of raising"""
    if p.degree() < 1 << log_split:
        if p.lead and log_split > 1 and p.max_deg > (1 << p.max_deg.bit_length()) - (1 << (log_split - 1)):       # :114
            return recurse_ps(sim, optimal_split(p.degree().bit_length()), target_level, p, pb, out_scale, fired)
        q = Poly(p.basis, p.coeffs, (p.a, p.b), p.prec)
        q.is_odd, q.is_even, q.lead, q.lazy, q.max_deg = p.is_odd, p.is_even, p.lead, p.lazy, p.max_deg
        q.level, q.scale = sim.baby_step(p.lead, target_level, out_scale)                                        # :123
        return [q], (q.level, q.scale)
    nxt = 1 << log_split
    while nxt < (p.degree() >> 1) + 1:                                   # :128-131
        nxt <<= 1
    pq, pr = factorize(p, nxt)
    lvl, scl = sim.giant_step(p.lead, target_level, out_scale, pb[nxt][1])                                      # :137
    bq, res = recurse_ps(sim, log_split, lvl, pq, pb, scl, fired)
    res = sim.mul(sim.rescale(res), pb[nxt])                             # :141-142
    br, tmp = recurse_ps(sim, log_split, target_level, pr, pb, res[1], fired)
    if log2_delta(tmp[1], res[1]) < DELTA:                               # :148
        if fired is None:
            raise ValueError("recursePS: res.Scale != tmp.Scale")
        fired.append((tmp[1], res[1]))
    return bq + br, res


def paterson_stockmeyer(sim, p, in_level, in_scale, out_scale, fired=None):
    """Polynomial.PatersonStockmeyerPolynomial (polynomial.go:74-106) -> the baby-step polynomials"""
    log_degree = p.degree().bit_length()
    log_split = optimal_split(log_degree)
    pb = {1: (in_level, in_scale)}
    sim.gen_power(pb, 1 << log_degree)                                   # :91
    for i in range((1 << log_split) - 1, 2, -1):
        sim.gen_power(pb, i)
    return recurse_ps(sim, log_split, in_level - sim.depth(p.degree()), p, pb, out_scale, fired)[0]


# ---- ciphertexts and the evaluator calls the circuit makes ------------------------------------------------------------------------------------
class Ct:
    def __init__(self, comps, scale):
        self.comps, self.scale = list(comps), scale

    def level(self):
        return self.comps[0].shape[0] - 1

    def at(self, level):
        return [x[:level + 1] for x in self.comps]


class Params:
    """N, the chains Q and P, the relinearisation key (an rlwe_restatement.GadgetKey), LevelsConsumedPerRescaling, EncodingPrecision"""

    def __init__(self, N, Q, P, rlk, nb=1, prec=53):
        self.N, self.Q, self.P, self.rlk, self.nb, self.prec = N, [int(q) for q in Q], [int(p) for p in P], rlk, nb, prec

    def mods(self, level):
        return self.Q[:level + 1]


def relinearize(P, ct):
    ct.comps = rr.relinearize(P.N, P.Q, P.P, [np.ascontiguousarray(x) for x in ct.comps], P.rlk)


def rescale(P, ct):
    ct.comps, ct.scale = cr.rescale(P.N, P.mods(ct.level()), ct.comps, ct.scale, P.nb)


def mul_new(P, a, b, relin):
    """MulNew / MulRelinNew of two ciphertexts at the smaller of their levels (evaluator.go:613-616, :741-750)"""
    level = min(a.level(), b.level())
    comps, scale = cr.mul_relin(P.mods(level), a.at(level), a.scale, b.at(level), b.scale, square=a is b)
    out = Ct(comps, scale)
    if relin:
        relinearize(P, out)
    return out


def add_sub(P, a, b, sub=False):
    """Add / Sub into a (evaluateInPlace): a is lowered to the smaller level"""
    level = min(a.level(), b.level())
    a.comps, a.scale = cr.add_sub(P.N, P.mods(level), a.at(level), a.scale, b.at(level), b.scale, sub, prec=P.prec)


def rounded(P, c):
    return cr.round_bits(c[0], P.prec), cr.round_bits(c[1], P.prec)     # bignum.ToComplex of a *bignum.Complex


def add_const(P, ct, c):
    """Add of a scalar (evaluator.go:82-101)"""
    _, _, s0, s1 = cr.rns_scalar(P.N, P.mods(ct.level()), ct.scale, rounded(P, c), P.prec)
    ct.comps = [cr.add_double(ct.comps[0], s0, s1, P.mods(ct.level()))] + ct.comps[1:]


def mul_then_add_const(P, x, c, res):
    """MulThenAdd with a scalar (evaluator.go:937-984) at the smaller level; res is lowered to it (see polynomial.py on the limbs above)"""
    level = min(x.level(), res.level())
    mods = P.mods(level)
    c = rounded(P, c)
    out, sout = res.at(level), res.scale
    cmp = x.scale.cmp(sout)
    if cmp == 0:
        if cr.is_int(c):
            s = cr.Scale(1)
        else:
            s = cr.rescale_scale(mods, P.nb)                             # :962-966
            out, _ = cr.mul_scalar(P.N, mods, out, sout, int(s.v), P.prec, P.nb)      # :968-972
            sout = sout.mul(s)
    elif cmp == -1:
        s = sout.div(x.scale)                                            # :977
    else:
        raise ValueError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
    _, _, s0, s1 = cr.rns_scalar(P.N, mods, s, c, P.prec)                # :982
    res.comps, res.scale = [cr.mul_double_then_add(a, s0, s1, o, mods) for a, o in zip(x.at(level), out)], sout   # :984


def plaintext(P, values, level, scale):
    """the plaintext of the slice branches: the vector embedded at `scale` (a float64 on its way to the encoder), all slots"""
    return ce.embed(values, P.N.bit_length() - 2, scale.float64(), P.N, P.mods(level))


def mul_then_add_vector(P, x, values, res):
    """MulThenAdd with a slice (evaluator.go:986-1039)"""
    level = min(x.level(), res.level())
    mods = P.mods(level)
    out, sout = res.at(level), res.scale
    cmp = x.scale.cmp(sout)
    if cmp == 0:
        s = cr.rescale_scale(mods, P.nb)
        out, _ = cr.mul_scalar(P.N, mods, out, sout, int(s.v), P.prec, P.nb)
        sout = sout.mul(s)
    elif cmp == -1:
        s = sout.div(x.scale)
    else:
        raise ValueError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
    res.comps, res.scale, _ = cr.mul_relin_then_add(P.N, mods, x.at(level), x.scale, [plaintext(P, values, level, s)], s, out, sout, False, P.prec, P.nb)


# ---- power_basis.go ------------------------------------------------------------------------------------------------------------------------------
def gen_power(P, pb, basis, n, lazy):
    """GenPower (:57-78); pb: dict power -> Ct"""
    if n not in pb and _gen(P, pb, basis, n, lazy):
        rescale(P, pb[n])


def _gen(P, pb, basis, n, lazy):
    """genPower (:80-182)"""
    if n in pb:
        return False
    a, b = split_degree(n)
    pow2 = n & (n - 1) == 0
    ra = _gen(P, pb, basis, a, lazy and not pow2)                        # :91
    rb = _gen(P, pb, basis, b, lazy and not pow2)                        # :94
    if lazy:
        for k in (a, b):
            if len(pb[k].comps) == 3:
                relinearize(P, pb[k])                                    # :101-111
    if ra:
        rescale(P, pb[a])                                                # :113-117, :131-135
    if rb:
        rescale(P, pb[b])
    pb[n] = mul_new(P, pb[a], pb[b], not lazy)                           # :125, :143
    if basis == CHEBYSHEV:
        c = abs(a - b)
        add_sub(P, pb[n], pb[n])                                         # :157
        if c == 0:
            add_const(P, pb[n], (Fraction(-1), Fraction(0)))             # :163
        else:
            gen_power(P, pb, basis, c, lazy)                             # :168
            add_sub(P, pb[n], pb[c], sub=True)                           # :172
    return True


# ---- polynomial_evaluator.go ---------------------------------------------------------------------------------------------------------------------
def vector_coefficient(P, polys, mapping, k):
    """GetVectorCoefficient (ckks polynomial_evaluator.go:92-109) taken to complex128 (encoder.go:251-256)"""
    values = np.zeros(P.N // 2, dtype=np.complex128)
    for i, p in enumerate(polys):
        for j in mapping.get(i, ()):
            c = p.coeffs[k]
            values[j] = complex(float(c[0]), float(c[1])) if c is not None else 0
    return values


def evaluate_from_power_basis(P, target_level, polys, mapping, pb, target_scale, trace=None):
    """EvaluatePolynomialVectorFromPowerBasis (:254-359)"""
    p0 = polys[0]
    even, odd = all(p.is_even for p in polys), all(p.is_odd for p in polys)
    lowest = len(p0.coeffs) - 1 - (1 if even and not odd else 0)         # :266-269
    zero = lambda d: Ct([np.zeros((target_level + 1, P.N), dtype=np.uint64) for _ in range(d + 1)], target_scale)
    coeff = (lambda k: vector_coefficient(P, polys, mapping, k)) if mapping is not None else (lambda k: p0.coeffs[k])
    first = (lambda res: add_sub(P, res, Ct([plaintext(P, coeff(0), target_level, res.scale)], res.scale))) if mapping is not None else \
        (lambda res: add_const(P, res, coeff(0)))
    if lowest == 0:
        res = zero(1)                                                    # :287, :325
        if even:
            first(res)
        return res
    res = zero(max([len(pb[i].comps) - 1 for i in range(p0.degree(), 0, -1) if i in pb] + [0]))    # :273-278
    if even:
        first(res)                                                       # :307, :343
    for key in range(p0.degree(), 0, -1):
        if p0.keeps(key):
            (mul_then_add_vector if mapping is not None else mul_then_add_const)(P, pb[key], coeff(key), res)   # :315, :351
    if trace is not None:
        trace.append((res.level(), res.scale))
    return res


def evaluate_monomial(P, a, b, xpow):
    """EvaluateMonomial (:226-251): b <- a + rescale(b) xpow"""
    if len(b.comps) == 3:
        relinearize(P, b)
    rescale(P, b)
    prod = mul_new(P, b, xpow, False)                                    # :238
    b.comps, b.scale = prod.comps, prod.scale
    assert log2_delta(a.scale, b.scale) >= DELTA, "evalMonomial: scale discrepency"   # :242
    add_sub(P, b, a)                                                     # :246


def evaluate(P, ct, polys, mapping, target_scale, pb=None, trace=None):
    """Evaluate (:29-91) and EvaluatePatersonStockmeyerPolynomialVector (:101-161).  polys: the Polys of the vector (one for a single
    polynomial, mapping None).  trace: collects (sim level, sim scale, reached level, reached scale) of every baby step."""
    p0 = polys[0]
    basis = p0.basis
    pb = {1: Ct([x.copy() for x in ct.comps], ct.scale)} if pb is None else pb
    assert pb[1].level() >= P.nb * p0.depth()                            # :56-58
    log_degree = p0.degree().bit_length()
    log_split = optimal_split(log_degree)
    odd, even = any(p.is_odd for p in polys), any(p.is_even for p in polys)
    gen_power(P, pb, basis, 1 << (log_degree - 1), False)                # :71
    for i in range((1 << log_split) - 1, 2, -1):
        if not (even or odd) or (i & 1 == 0 and even) or (i & 1 == 1 and odd):
            gen_power(P, pb, basis, i, p0.lazy)                          # :78
    sim = Sim(P.Q, P.nb)
    PS = [paterson_stockmeyer(sim, p, pb[1].level(), pb[1].scale, target_scale) for p in polys]   # :84
    split = len(PS[0])
    steps = [None] * split
    for i in range(split):                                               # :108-114, EvaluateBabyStep :165-189
        first = PS[0][i]
        reached = []
        val = evaluate_from_power_basis(P, first.level, [ps[i] for ps in PS], mapping, pb, first.scale, reached)
        if trace is not None and reached:
            trace.append((first.level, first.scale) + reached[0])
        steps[split - i - 1] = [first.degree(), val]
    while len(steps) != 1:
        giant = [0] * len(steps)
        i = 0
        while i < len(steps):                                            # :121-128
            if i == len(steps) - 1:
                giant[i] = 2
            elif steps[i][0] == steps[i + 1][0]:
                giant[i] = 1
                i += 1
            i += 1
        for i in range(len(steps)):                                      # EvaluateGianStep :193-223
            if giant[i] == 2:
                steps[i][0] = steps[i - 1][0]
            elif giant[i] == 1:
                deg = 1 << steps[i][0].bit_length()
                evaluate_monomial(P, steps[i][1], steps[i + 1][1], pb[deg])
                steps[i + 1][0] = 2 * deg - 1
                steps[i] = None
        steps = [s for s in steps if s is not None]
    res = steps[0][1]
    if len(res.comps) == 3:
        relinearize(P, res)                                              # :150-154
    rescale(P, res)                                                      # :156
    return res

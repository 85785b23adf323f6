"""The reference's polynomial evaluation for BGV / BFV restated over bgv_restatement.py, bfv_restatement.py, bgv_encoder_restatement.py,
rlwe_restatement.py and the oracle: circuits/bgv/polynomial/{polynomial,polynomial_evaluator,polynomial_evaluator_sim}.go and the generic
circuits/common/polynomial/{polynomial,power_basis,polynomial_evaluator,polynomial_evaluator_sim}.go as the BGV wrappers instantiate them.
TEST INFRASTRUCTURE ONLY: the GPU tests compare the device path against it bit for bit, tests/test_bgv_polynomial_oracle.py pins it to Python
integers and to decryption under a real key.

A coefficient is a Python int or None (nil); a polynomial is a Poly below; a ciphertext is a Ct: a list of (limbs, N) uint64 arrays in the NTT
domain with its scale, an int modulo T.  One ciphertext at a time: a batch is a loop of the caller."""
import math

import numpy as np

import bfv_restatement as fr
import bgv_encoder_restatement as be
import bgv_restatement as br
import rlwe_restatement as rr
from polynomial_restatement import optimal_split, split_degree

DELTA = 128.0 - 12                                                       # rlwe.ScalePrecision - 12 (polynomial.go:148, polynomial_evaluator.go:242)


class Poly:
    """bgv polynomial.NewPolynomial (:14-16): bignum.NewPolynomial(Monomial, coeffs, nil) (IsOdd = IsEven = true, :104-111) inside
    polynomial.NewPolynomial (MaxDeg = degree, Lead = true, Lazy = false, polynomial.go:28-35)"""

    def __init__(self, coeffs):
        self.coeffs = [None if c is None else int(c) for c in coeffs]
        self.is_odd = self.is_even = True
        self.max_deg, self.lead, self.lazy = len(self.coeffs) - 1, True, False
        self.level, self.scale = 0, None

    def degree(self):
        return len(self.coeffs) - 1

    def depth(self):
        return int(math.ceil(math.log2(float(self.degree()))))          # bignum :144-146

    def keeps(self, i):
        return not (self.is_even or self.is_odd) or (i & 1 == 0 and self.is_even) or (i & 1 == 1 and self.is_odd)


def factorize(p, n):
    """bignum Factorize (:258-314), Monomial branch, inside polynomial.Polynomial.Factorize (polynomial.go:38-58): p = X^n pq + pr"""
    assert n >= p.degree() >> 1
    pr = list(p.coeffs[:n])                                              # :266-271
    pq = [None] * (p.degree() - n + 1)
    pq[0] = p.coeffs[n]                                                  # :276-278
    for i in range(n + 1, p.degree() + 1):
        if p.coeffs[i] is not None and p.keeps(i):
            pq[i - n] = p.coeffs[i]                                      # :287
    out = []
    for co in (pq, pr):
        q = Poly(co)
        q.is_odd, q.is_even, q.lead, q.lazy, q.max_deg = p.is_odd, p.is_even, False, False, 0
        out.append(q)
    out[0].max_deg = p.max_deg                                           # polynomial.go:45
    out[1].max_deg = n - 1 if p.max_deg == p.degree() else p.max_deg - (p.degree() - n + 1)       # :47-51
    out[0].lead = p.lead                                                 # :53-55
    return out


def evaluate_exact(p, x, t):
    """sum c_i x^i modulo t, term by term"""
    return sum((0 if c is None else c) * pow(int(x), i, t) for i, c in enumerate(p.coeffs)) % t


# ---- the simulator (circuits/bgv/polynomial/polynomial_evaluator_sim.go; rlwe.Scale modulo T, core/rlwe/scale.go:77-119) ------------------------
class Sim:
    def __init__(self, Q, t, invariant):
        self.Q, self.t, self.invariant = [int(q) for q in Q], int(t), bool(invariant)

    def div(self, a, b):
        return a * pow(b % self.t, -1, self.t) % self.t                  # Scale.Div: ModInverse, Mul, Mod

    def depth(self, degree):
        return 0 if self.invariant else degree.bit_length() - 1          # PolynomialDepth (:25-35)

    def rescale(self, op):
        level, scale = op
        if self.invariant:                                               # :38-43
            return level, scale
        return level - 1, self.div(scale, self.Q[level])

    def mul(self, a, b):
        level = min(a[0], b[0])                                          # :46-57
        if self.invariant:
            return level, fr.scale_invariant(self.t, br.prod(self.Q[:level + 1]), a[1], b[1])
        return level, a[1] * b[1] % self.t

    def baby_step(self, lead, level, scale):
        if not self.invariant and lead:                                  # :60-67
            scale = scale * self.Q[level] % self.t
        return level, scale

    def giant_step(self, lead, level, scale, xpow_scale):
        scale = self.div(scale, xpow_scale)                              # :75
        if not self.invariant:
            qi = self.Q[level] if lead else self.Q[level + 1]            # :80-87
            return level + 1, scale * qi % self.t                        # :99-101
        return level, scale * (self.t - br.prod(self.Q[:level + 1]) % self.t) % self.t     # :91-96

    def gen_power(self, pb, n):
        """SimPowerBasis.GenPower (common sim :25-38); pb: dict power -> (level, scale)"""
        if n < 2:
            return
        a, b = split_degree(n)
        self.gen_power(pb, a)
        self.gen_power(pb, b)
        pb[n] = self.rescale(self.mul(pb[a], pb[b]))


def log2_delta(s, t):
    """Scale.Log2Delta (core/rlwe/scale.go:140-149) on the values"""
    if s == t:
        return float("inf")
    return -math.log2(abs(s - t) / max(s, t))


def recurse_ps(sim, log_split, target_level, p, pb, out_scale):
    """recursePS (polynomial.go:109-153) -> (baby-step polynomials with level and scale, (level, scale) of the combination)"""
    if p.degree() < 1 << log_split:
        if p.lead and log_split > 1 and p.max_deg > (1 << p.max_deg.bit_length()) - (1 << (log_split - 1)):       # :114
            return recurse_ps(sim, optimal_split(p.degree().bit_length()), target_level, p, pb, out_scale)
        q = Poly(p.coeffs)
        q.is_odd, q.is_even, q.lead, q.lazy, q.max_deg = p.is_odd, p.is_even, p.lead, p.lazy, p.max_deg
        q.level, q.scale = sim.baby_step(p.lead, target_level, out_scale)                                        # :123
        return [q], (q.level, q.scale)
    nxt = 1 << log_split
    while nxt < (p.degree() >> 1) + 1:                                   # :128-131
        nxt <<= 1
    pq, pr = factorize(p, nxt)
    lvl, scl = sim.giant_step(p.lead, target_level, out_scale, pb[nxt][1])                                      # :137
    bq, res = recurse_ps(sim, log_split, lvl, pq, pb, scl)
    res = sim.mul(sim.rescale(res), pb[nxt])                             # :141-142
    br_, tmp = recurse_ps(sim, log_split, target_level, pr, pb, res[1])
    assert log2_delta(tmp[1], res[1]) >= DELTA, "recursePS: res.Scale != tmp.Scale"                              # :148
    return bq + br_, res


def paterson_stockmeyer(sim, p, in_level, in_scale, out_scale):
    """Polynomial.PatersonStockmeyerPolynomial (polynomial.go:74-106) -> the baby-step polynomials"""
    log_degree = p.degree().bit_length()
    log_split = optimal_split(log_degree)
    pb = {1: (in_level, in_scale)}
    sim.gen_power(pb, 1 << log_degree)                                   # :91
    for i in range((1 << log_split) - 1, 2, -1):
        sim.gen_power(pb, i)
    return recurse_ps(sim, log_split, in_level - sim.depth(p.degree()), p, pb, out_scale)[0]


# ---- ciphertexts and the evaluator calls the circuit makes ------------------------------------------------------------------------------------
class Ct:
    def __init__(self, comps, scale):
        self.comps, self.scale = list(comps), int(scale)

    def level(self):
        return self.comps[0].shape[0] - 1

    def at(self, level):
        return [np.ascontiguousarray(x[:level + 1]) for x in self.comps]


class Params:
    """N, the chains Q and P, T, the relinearisation key (an rlwe_restatement.GadgetKey), the evaluator's ScaleInvariant flag with the moduli
    of ringQMul it needs, and the encoder's tables"""

    def __init__(self, N, Q, Pk, t, rlk, invariant=False, QMul=None):
        self.N, self.Q, self.Pk, self.t, self.rlk, self.invariant = N, [int(q) for q in Q], [int(p) for p in Pk], int(t), rlk, bool(invariant)
        self.bfv = fr.Params(N, self.Q, QMul, t) if invariant else None
        self.enc = be.Params(N, self.Q, t)

    def mods(self, level):
        return self.Q[:level + 1]

    def sim(self):
        return Sim(self.Q, self.t, self.invariant)


def relinearize(P, ct):
    ct.comps = rr.relinearize(P.N, P.Q, P.Pk, [np.ascontiguousarray(x) for x in ct.comps], P.rlk)


def rescale(P, ct):
    """bgv Rescale (:1415-1445): nothing on a scale-invariant evaluator (:1417)"""
    if not P.invariant:
        ct.comps, ct.scale = br.rescale(P.N, P.mods(ct.level()), P.t, ct.comps, ct.scale)


def mul_new(P, a, b, relin):
    """MulNew / MulRelinNew of two ciphertexts at the smaller of their levels: tensorStandard (:665-751), or on a scale-invariant evaluator
    tensorScaleInvariant (:975-1040) with the scale of MulScaleInvariant (:1045-1051)"""
    level = min(a.level(), b.level())
    mods = P.mods(level)
    x = a.at(level)
    y = x if a is b else b.at(level)
    if P.invariant:
        out = Ct(fr.tensor_scale_invariant(P.bfv, level, x, y), fr.scale_invariant(P.t, br.prod(mods), a.scale, b.scale))
    else:
        out = Ct(*br.tensor_standard(mods, P.t, x, a.scale, y, b.scale, square=a is b))
    if relin:
        relinearize(P, out)
    return out


def add(P, a, b):
    """Add(a, b, a) of two ciphertexts (:181-195): a is lowered to the smaller level"""
    level = min(a.level(), b.level())
    a.comps, a.scale = br.add_sub(P.mods(level), P.t, a.at(level), a.scale, b.at(level), b.scale, False)


def add_const(P, ct, c):
    """Add of a uint64 (:229-230 -> :197-227)"""
    ct.comps, ct.scale = br.add_scalar(P.mods(ct.level()), P.t, ct.comps, ct.scale, c)


def add_vector(P, ct, values):
    """Add of a []uint64 (:235-262): encoded with the ciphertext's metadata (its scale), then evaluateInPlace"""
    pt = be.encode(P.enc, ct.level(), values, ct.scale)
    ct.comps, ct.scale = br.add_sub(P.mods(ct.level()), P.t, ct.comps, ct.scale, [pt], ct.scale, False)


def ratio(P, x_scale, out_scale):
    """opOut.Scale / op0.Scale (:1177-1180, :1224-1230)"""
    return 1 if x_scale == out_scale else pow(x_scale, P.t - 2, P.t) * out_scale % P.t


def mul_then_add_const(P, x, c, res):
    """MulThenAdd with a uint64 (:1200-1201 -> :1162-1194) at the smaller level; res is lowered to it (see bgv_polynomial.py on the limbs above)"""
    level = min(x.level(), res.level())
    mods = P.mods(level)
    v = int(c)
    if x.scale != res.scale:
        v *= ratio(P, x.scale, res.scale)                                # :1177-1181
    v = br.center_t(v, P.t)                                              # :1185-1190
    res.comps = [br.mul_scalar_then_add(a, v, o, mods) for a, o in zip(x.at(level), res.at(level))]   # MulScalarBigintThenAdd (:1192-1194)


def mul_then_add_vector(P, x, values, res):
    """MulThenAdd with a []uint64 (:1202-1239): encoded at opOut.Scale / op0.Scale (1 for equal scales), then the plaintext branch of
    mulRelinThenAdd (:1370-1400)"""
    level = min(x.level(), res.level())
    mods = P.mods(level)
    s = ratio(P, x.scale, res.scale)
    pt = be.encode(P.enc, level, values, s)
    res.comps, res.scale, _ = br.mul_relin_then_add(mods, P.t, x.at(level), x.scale, [pt], s, res.at(level), res.scale, False)


# ---- power_basis.go ------------------------------------------------------------------------------------------------------------------------------
def gen_power(P, pb, n, lazy):
    """GenPower (:57-78); pb: dict power -> Ct"""
    if n not in pb and _gen(P, pb, n, lazy):
        rescale(P, pb[n])


def _gen(P, pb, n, lazy):
    """genPower (:80-182), Monomial basis"""
    if n in pb:
        return False
    a, b = split_degree(n)
    pow2 = n & (n - 1) == 0
    ra = _gen(P, pb, a, lazy and not pow2)                               # :91
    rb = _gen(P, pb, b, lazy and not pow2)                               # :94
    if lazy:
        for k in (a, b):
            if len(pb[k].comps) == 3:
                relinearize(P, pb[k])                                    # :101-111
    if ra:
        rescale(P, pb[a])                                                # :113-117, :131-135
    if rb:
        rescale(P, pb[b])
    pb[n] = mul_new(P, pb[a], pb[b], not lazy)                           # :125, :143
    return True


# ---- polynomial_evaluator.go ---------------------------------------------------------------------------------------------------------------------
def vector_coefficient(P, polys, mapping, k):
    """GetVectorCoefficient (bgv polynomial_evaluator.go:87-102): MaxSlots uint64, zero where nothing is mapped"""
    values = np.zeros(P.enc.n, dtype=np.uint64)
    for i, p in enumerate(polys):
        for j in mapping.get(i, ()):
            values[j] = p.coeffs[k] % (1 << 64)
    return values


def evaluate_from_power_basis(P, target_level, polys, mapping, pb, target_scale):
    """EvaluatePolynomialVectorFromPowerBasis (:254-359)"""
    p0 = polys[0]
    even, odd = all(p.is_even for p in polys), all(p.is_odd for p in polys)
    lowest = len(p0.coeffs) - 1 - (1 if even and not odd else 0)         # :266-269
    zero = lambda d: Ct([np.zeros((target_level + 1, P.N), dtype=np.uint64) for _ in range(d + 1)], target_scale)
    if mapping is not None:
        first = lambda res: add_vector(P, res, vector_coefficient(P, polys, mapping, 0))
        term = lambda key, res: mul_then_add_vector(P, pb[key], vector_coefficient(P, polys, mapping, key), res)
    else:
        first = lambda res: add_const(P, res, p0.coeffs[0])
        term = lambda key, res: mul_then_add_const(P, pb[key], p0.coeffs[key], res)
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
            term(key, res)                                               # :315, :351
    return res


def evaluate_monomial(P, a, b, xpow):
    """EvaluateMonomial (:226-251): b <- a + rescale(b) xpow"""
    if len(b.comps) == 3:
        relinearize(P, b)
    rescale(P, b)
    prod = mul_new(P, b, xpow, False)                                    # :238
    b.comps, b.scale = prod.comps, prod.scale
    assert log2_delta(a.scale, b.scale) >= DELTA, "evalMonomial: scale discrepency"   # :242
    add(P, b, a)                                                         # :246


def evaluate(P, ct, polys, mapping, target_scale, pb=None, trace=None):
    """Evaluate (:29-91) and EvaluatePatersonStockmeyerPolynomialVector (:101-161).  polys: the Polys of the vector (one for a single
    polynomial, mapping None).  trace: collects (sim level, sim scale, reached level, reached scale) of every baby step."""
    p0 = polys[0]
    pb = {1: Ct([x.copy() for x in ct.comps], ct.scale)} if pb is None else pb
    assert pb[1].level() >= p0.depth(), "%d levels < %d log(d) -> cannot evaluate poly" % (pb[1].level(), p0.depth())      # :56-58
    log_degree = p0.degree().bit_length()
    log_split = optimal_split(log_degree)
    odd, even = any(p.is_odd for p in polys), any(p.is_even for p in polys)
    gen_power(P, pb, 1 << (log_degree - 1), False)                       # :71
    for i in range((1 << log_split) - 1, 2, -1):
        if not (even or odd) or (i & 1 == 0 and even) or (i & 1 == 1 and odd):
            gen_power(P, pb, i, p0.lazy)                                 # :78
    sim = P.sim()
    PS = [paterson_stockmeyer(sim, p, pb[1].level(), pb[1].scale, target_scale % P.t) for p in polys]   # :84
    split = len(PS[0])
    steps = [None] * split
    for i in range(split):                                               # :108-114, EvaluateBabyStep :165-189
        first = PS[0][i]
        val = evaluate_from_power_basis(P, first.level, [ps[i] for ps in PS], mapping, pb, first.scale)
        if trace is not None:
            trace.append((first.level, first.scale, val.level(), val.scale))
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


# ---- rh_bgv_plain_combination: the reference's sequence for one baby step over a mapping, on given plaintexts ------------------------------------------
def plain_combination(mods, t, terms, pts, const):
    """res = [0 .. 0]; Add of the constant plaintext `const` (or None) on component 0 (evaluateInPlace, :270-286); per term the plaintext
    branch of mulRelinThenAdd with matching scales (:1377, :1397-1399): c00 = MRed(pt, tMontgomery), res_j = CRed(res_j + MRed(X_j, c00)).
    terms: K lists of (limbs, N) arrays (rows beyond len(mods) are not read), pts: K (len(mods), N) arrays as Encode leaves them."""
    L = len(mods)
    nc = len(terms[0]) if terms else 1
    z = np.zeros((L, pts[0].shape[1] if pts else const.shape[1]), dtype=np.uint64)
    res = [z.copy() for _ in range(nc)]
    if const is not None:
        res[0] = br._vec("ADD", res[0], const, z, None, mods)
    tm = br.t_montgomery(t, mods)
    for x, pt in zip(terms, pts):
        c00 = br._vec("MUL_SCALAR_MONT", pt, None, z, tm, mods)
        res = [br._vec("MUL_MONT_THEN_ADD", np.ascontiguousarray(x[j][:L]), c00, res[j], None, mods) for j in range(nc)]
    return res

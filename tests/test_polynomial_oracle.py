"""CPU: tests/polynomial_restatement.py (the restated polynomial evaluation the GPU tests compare against) pinned to ground truth that does not
depend on the composition -- Factorize to exact rational polynomial identities, the split tables to their formulas, the simulator to the
levels and scales the evaluation reaches, the whole circuit to decryption under a real secret key at the reference's own test parameters and
its own precision bound -- and the new C entry point's declaration.  The host-side half of the package (polynomial.py) is held to the same
restatement where it needs no device."""
import math
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_restatement as ce
import ckks_restatement as cr
import polynomial_restatement as pr
import rlwe_restatement as rr
from oracle import primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = cr.Scale
EXP7 = [Fraction(1, math.factorial(k)) for k in range(8)]               # polynomial_evaluator_test.go:87-96: 1 / k! rounded to prec bits
LOGQ, LOGP, LOGSCALE = (55, 45, 45, 45, 45, 45, 45), (60,), 45           # testInsecurePrec45 (:162-167)


def exp7():
    return pr.Poly(pr.MONOMIAL, [(cr.round_bits(c, 53), Fraction(0)) for c in EXP7])


def cheb_expand(coeffs, n):
    """the Chebyshev coefficients of T_n * sum_j c_j T_j: T_n T_j = (T_{n+j} + T_|n-j|) / 2"""
    out = [(Fraction(0), Fraction(0))] * (n + len(coeffs))
    add = lambda k, c: out.__setitem__(k, (out[k][0] + c[0] / 2, out[k][1] + c[1] / 2))
    for j, c in enumerate(coeffs):
        if c is not None:
            add(n + j, c)
            add(abs(n - j), c)
    return out


@pytest.mark.parametrize("basis", [pr.MONOMIAL, pr.CHEBYSHEV])
@pytest.mark.parametrize("deg,n", [(7, 4), (31, 16), (15, 8), (20, 16), (12, 8), (5, 4)])
def test_factorize_is_an_exact_identity_and_rounds_at_prec(basis, deg, n):
    rng = random.Random(deg * 100 + n)
    # coefficients of 24 bits: every Add and Sub at 53 bits is exact, so X^n pq + pr == p holds as polynomials
    small = [(Fraction(rng.randrange(-2 ** 23, 2 ** 23), 2 ** 20), Fraction(rng.randrange(-2 ** 23, 2 ** 23), 2 ** 20)) for _ in range(deg + 1)]
    p = pr.Poly(basis, small)
    pq, prem = pr.factorize(p, n)
    assert pq.degree() == deg - n and prem.degree() == n - 1
    z = (Fraction(0), Fraction(0))
    if basis == pr.MONOMIAL:
        back = [c or z for c in prem.coeffs] + [c or z for c in pq.coeffs]
    else:
        back = cheb_expand(pq.coeffs, n)
        for k, c in enumerate(prem.coeffs):
            back[k] = (back[k][0] + (c or z)[0], back[k][1] + (c or z)[1])
    assert back[:deg + 1] == small and all(c == z for c in back[deg + 1:])
    # full 53-bit coefficients: each coefficient is the exact one rounded once to 53 bits
    full = [(Fraction(rng.uniform(-1, 1)), Fraction(rng.uniform(-1, 1))) for _ in range(deg + 1)]
    p = pr.Poly(basis, full)
    pq, prem = pr.factorize(p, n)
    for j in range(1, deg - n + 1):
        c = full[n + j]
        if basis == pr.MONOMIAL:
            assert pq.coeffs[j] == c
        else:
            assert pq.coeffs[j] == (2 * c[0], 2 * c[1])
            assert prem.coeffs[n - j] == (cr.round_bits(full[n - j][0] - c[0], 53), cr.round_bits(full[n - j][1] - c[1], 53))
    assert pq.coeffs[0] == full[n] and (pq.max_deg, pq.lead, prem.max_deg, prem.lead) == (deg, True, n - 1, False)
    q2, r2 = pr.factorize(prem, n // 2)                                  # a remainder: MaxDeg < Degree is carried on (polynomial.go:47-51)
    assert (q2.max_deg, r2.max_deg, q2.lead) == (n - 1, n // 2 - 1, False)


def test_split_tables_follow_their_formulas():
    assert pr.split_degree(1) == (0, 0)                                  # n = 1 counts as a power of two (:40-41); GenPower never asks for it
    for n in range(2, 65):
        a, b = pr.split_degree(n)
        assert a + b == n
        if n & (n - 1) == 0:
            assert a == b == n // 2
        else:
            assert a == 2 ** int(math.floor(math.log2(n))) - 1 and a % 2 == 1 and b == n - a
    # OptimalSplit: the cheaper of logDegree // 2 and logDegree // 2 + 1 under the multiplication count 2^s + 2^(logDegree - s) + logDegree - s - 3
    cost = lambda ld, s: (1 << s) + (1 << (ld - s)) + ld - s - 3
    table = {ld: pr.optimal_split(ld) for ld in range(1, 8)}           # degrees up to 127; logDegree 0 shifts by -1 in the reference too
    assert table == {1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 6: 3, 7: 4}
    for ld, got in table.items():
        s = ld >> 1
        assert got == (s + 1 if cost(ld, s) > cost(ld, s + 1) else s)


def test_package_host_side_matches_the_restatement(rh):
    P = rh.polynomial
    assert [P.SplitDegree(n) for n in range(1, 65)] == [pr.split_degree(n) for n in range(1, 65)]
    assert [P.OptimalSplit(k) for k in range(1, 8)] == [pr.optimal_split(k) for k in range(1, 8)]
    rng = random.Random(5)
    Q = [int(q) for q in primes.gen_moduli(11, list(LOGQ), list(LOGP))[0]]
    for basis, pbasis, deg in ((P.Monomial, pr.MONOMIAL, 7), (P.Chebyshev, pr.CHEBYSHEV, 31), (P.Chebyshev, pr.CHEBYSHEV, 5), (P.Monomial, pr.MONOMIAL, 20)):
        co = [complex(rng.uniform(-1, 1), rng.uniform(-1, 1)) for _ in range(deg + 1)]
        a, b = P.Polynomial(basis, co, (-3, 5)), pr.Poly(pbasis, co, (-3, 5))
        assert (a.IsOdd, a.IsEven, a.Lead, a.Lazy, a.MaxDeg, a.Depth()) == (True, True, True, False, deg, b.depth())
        assert a.ChangeOfBasis() == b.change_of_basis()
        n = 1 << (deg.bit_length() - 1)
        for x, y in zip(a.Factorize(n), pr.factorize(b, n)):
            assert [None if c is None else (c.re, c.im) for c in x.Coeffs] == y.coeffs and (x.MaxDeg, x.Lead) == (y.max_deg, y.lead)
        ps = a.PatersonStockmeyerPolynomial(P.SimEvaluator(Q), 6, 2 ** 45, 2 ** 45)
        want = pr.paterson_stockmeyer(pr.Sim(Q), b, 6, S(2 ** 45), S(2 ** 45))
        assert [(v.Degree(), v.Level, v.Scale.Value, v.Lead, v.MaxDeg) for v in ps.Value] == [(w.degree(), w.level, w.scale.v, w.lead, w.max_deg) for w in want]
        assert [[None if c is None else (c.re, c.im) for c in v.Coeffs] for v in ps.Value] == [w.coeffs for w in want]
        x = complex(0.25, -0.5)
        got, exact = a.Evaluate(x), pr.evaluate_exact(b, (Fraction(0.25), Fraction(-0.5)))
        assert (got.re, got.im) == exact
    vec = P.PolynomialVector([P.Polynomial(P.Chebyshev, [1, 2, 3], (-3, 5))], {0: [0, 2]})
    assert vec.ChangeOfBasis(4)[0] == [Fraction(1, 4), 0, Fraction(1, 4), 0] and vec.Depth() == 1
    with pytest.raises(rh.RingHipError, match="degree must all be the same"):
        P.PolynomialVector([P.Polynomial(P.Monomial, [1, 2]), P.Polynomial(P.Monomial, [1, 2, 3])], {})


# ---- the simulator against the evaluation, and the circuit against decryption ---------------------------------------------------------------
class Keyed:
    """a ring with a real secret key and relinearisation key (LogP (60): one P modulus, the single-P gadget product)"""
    _cache = {}

    def __new__(cls, logN):
        if logN not in cls._cache:
            self = object.__new__(cls)
            Q, Pk = primes.gen_moduli(logN + 1, list(LOGQ), list(LOGP))
            self.N, self.Q, self.Pk = 1 << logN, [int(q) for q in Q], [int(p) for p in Pk]
            self.rnd = random.Random(1000 + logN)
            self.sk = rr.Secret.sample(self.rnd, self.N)
            rlk = rr.relin_key(self.rnd, self.sk, self.Q, self.Pk, len(self.Q) - 1, 0)
            self.P = pr.Params(self.N, self.Q, self.Pk, rlk)
            cls._cache[logN] = self
        return cls._cache[logN]

    def encrypt(self, values, scale):
        level = len(self.Q) - 1
        words = ce.embed_coeffs(values, self.N.bit_length() - 2, float(scale), self.N, self.Q)
        m = rr.crt_centered(words, self.Q)
        comps, _ = rr.encrypt(self.rnd, self.sk, m, self.Q, level)
        return pr.Ct(comps, S(scale))

    def decrypt(self, ct):
        mods = self.Q[:ct.level() + 1]
        s = self.sk.rows(mods)
        acc = np.asarray(ct.comps[-1], dtype=np.uint64)
        for c in reversed(ct.comps[:-1]):                                # Decryptor.Decrypt (core/rlwe/decryptor.go:51-92): Horner in s
            acc = rr._vec("ADD", rr._vec("MUL_MONT", acc, s, mods), np.asarray(c, dtype=np.uint64), mods)
        re_, im_ = ce.decode(acc, self.N.bit_length() - 2, ct.scale.float64(), self.N, mods)
        return re_ + 1j * im_


def avg_log2_prec(want, have):
    """getPrecisionStats (schemes/ckks/precision.go:106-204): the averages of -log2 |error| of the real and of the imaginary parts; an error of
    zero counts as Log2Scale (:146-152)"""
    out = []
    for part in (np.real, np.imag):
        err = np.abs(part(np.asarray(have)) - part(np.asarray(want)))
        out.append(float(np.mean([LOGSCALE if e == 0 else -math.log2(e) for e in err])))
    return out


@pytest.mark.parametrize("case", ["monomial7", "chebyshev31"])
def test_simulator_predicts_every_baby_step(case):
    k = Keyed(5)
    rng = np.random.default_rng(3)
    if case == "monomial7":
        p = exp7()
    else:
        p = pr.Poly(pr.CHEBYSHEV, [complex(a, b) for a, b in rng.uniform(-1, 1, (32, 2))], (-1, 1))
    ct = k.encrypt(rng.uniform(-1, 1, k.N // 2) + 1j * rng.uniform(-1, 1, k.N // 2), 2 ** LOGSCALE)
    fired, trace = [], []
    steps = pr.paterson_stockmeyer(pr.Sim(k.Q), p, ct.level(), ct.scale, ct.scale, fired)
    assert fired == [] and sum(s.degree() + 1 for s in steps) >= p.degree() + 1
    out = pr.evaluate(k.P, ct, [p], None, ct.scale, trace=trace)
    assert len(trace) == len(steps)
    for sim_level, sim_scale, level, scale in trace:
        assert sim_level == level and sim_scale.v == scale.v
    assert out.level() == ct.level() - p.depth() and pr.log2_delta(out.scale, ct.scale) >= pr.DELTA


@pytest.fixture(scope="module")
def vector():
    k = Keyed(10)                                                        # LogN 10, LogQ (55, 45 x 6), LogP (60), scale 2^45 (:162-167)
    rng = np.random.default_rng(45)
    values = rng.uniform(-1, 1, k.N // 2) + 1j * rng.uniform(-1, 1, k.N // 2)      # NewTestVector(-1, 1)
    return k, values, k.encrypt(values, 2 ** LOGSCALE)


def exact(p, values):
    return np.array([complex(*[float(v) for v in pr.evaluate_exact(p, (Fraction(z.real), Fraction(z.imag)))]) for z in values])


def test_exp_taylor_decrypts_to_the_reference_bound(vector):
    """polynomial_evaluator_test.go:77-109: average precision of both parts >= LogDefaultScale - (LogN + 2) = 33 bits (precision.go:92-103)"""
    k, values, ct = vector
    p = exp7()
    out = pr.evaluate(k.P, ct, [p], None, ct.scale)
    re_, im_ = avg_log2_prec(exact(p, values), k.decrypt(out))
    print("avg log2 precision: real %.2f imag %.2f" % (re_, im_))
    assert out.level() == ct.level() - 3 and min(re_, im_) >= LOGSCALE - (10 + 2)


def test_exp_taylor_vector_case_decrypts_to_the_reference_bound(vector):
    """:111-157: the even slots mapped to the polynomial, the odd slots zero"""
    k, values, ct = vector
    p = exp7()
    idx = list(range(0, k.N // 2, 2))
    out = pr.evaluate(k.P, ct, [p], {0: idx}, ct.scale)
    want = np.zeros(k.N // 2, dtype=np.complex128)
    want[idx] = exact(p, values[idx])
    re_, im_ = avg_log2_prec(want, k.decrypt(out))
    print("avg log2 precision: real %.2f imag %.2f" % (re_, im_))
    assert min(re_, im_) >= LOGSCALE - (10 + 2)


def test_chebyshev_on_another_interval_decrypts_to_the_reference_bound():
    """a degree-15 Chebyshev interpolant of a sigmoid on [-4, 4], values in the interval, after the affine map of ChangeOfBasis: the
    ciphertext of scalar x + constant is what the evaluation is given"""
    k = Keyed(10)
    rng = np.random.default_rng(46)
    a, b = -4.0, 4.0
    nodes = np.cos(np.pi * (np.arange(16) + 0.5) / 16)
    f = 1 / (1 + np.exp(-(nodes * (b - a) / 2 + (b + a) / 2)))
    co = [float(2 / 16 * np.sum(f * np.cos(j * np.pi * (np.arange(16) + 0.5) / 16))) for j in range(16)]
    co[0] /= 2
    p = pr.Poly(pr.CHEBYSHEV, co, (a, b))
    values = rng.uniform(a, b, k.N // 2) + 0j
    s, c = p.change_of_basis()
    assert (s, c) == (Fraction(1, 4), 0)
    ct = k.encrypt(values * float(s) + float(c), 2 ** LOGSCALE)
    out = pr.evaluate(k.P, ct, [p], None, ct.scale)
    re_, im_ = avg_log2_prec(exact(p, values), k.decrypt(out))
    print("avg log2 precision: real %.2f imag %.2f" % (re_, im_))
    assert out.level() == ct.level() - 4 and min(re_, im_) >= LOGSCALE - (10 + 2)


def test_linear_combination_is_declared_exported_and_checks_its_arguments(rh):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ringhip.h")).read(), flags=re.S)
    name = "rh_ckks_linear_combination"
    assert re.search(r"\bint %s\s*\(rh_ring\* r, int level," % name, txt), "%s is not declared in include/ringhip.h" % name
    L = rh.lib()
    for n in (name, name + "_table_words", name + "_chunk", name + "_width"):
        assert hasattr(L, n), "libringhip.so does not export %s" % n
    assert L.rh_ckks_linear_combination(None, 0, 0, None, None, None, None, None, None, None, None, None, 1, None, 0) == -1
    assert b"rh_ckks_linear_combination: null ring handle" in L.rh_last_error()
    # the chunk bound: C products below 2^122 and one Montgomery step stay inside 64 bits iff (C + 8) 2^58 <= 2^64 (csrc/ckks.hip)
    chunk, width = L.rh_ckks_linear_combination_chunk(), L.rh_ckks_linear_combination_width()
    assert chunk == 56 and (chunk + 8) << 58 <= 1 << 64 < (chunk + 9) << 58 and chunk % width == 0
    assert L.rh_ckks_linear_combination_table_words(7, 15) == 2 * 16 + 7 * (4 + 2 * 16)
    assert "linear_combination" in rh.ckks.Evaluator.FUSED_DEFAULT

"""tests/bgv_polynomial_restatement.py pinned to ground truth with Python integers: the simulator's levels and scales against the recursion
evaluated by hand with the evaluator's own rules, baby steps against big-integer sums, and whole evaluations against decryption under a real key
(encrypt with the restated key layer, evaluate, decrypt, decode: the polynomial slot by slot modulo T).  It also holds the condition under which
tests/test_gpu_bgv_polynomial.py is meaningful: for every (chain, T, polynomial) used there, the restatement decrypts exactly with the noise at
least MARGIN_BITS below Q_level / (2T).  CPU only."""
import functools
import math
import os
import random
import re

import numpy as np
import pytest

import bfv_restatement as fr
import bgv_encoder_restatement as be
import bgv_polynomial_restatement as bp
import bgv_restatement as br
import keygen_restatement as kr
import rlwe_restatement as rr
from oracle import primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN_BITS = 10                                                         # a safety margin on the choice of inputs, not a measurement

# ---- what the GPU file evaluates: (logN, logQ, T) and the polynomials --------------------------------------------------------------------------------
LOGQ = (55, 45, 45, 45, 45, 45, 45)                                      # degree 31 ends at level 1 in the standard arm (4 + 1 levels of 6)
SETTINGS = {"n7": (7, LOGQ, 257), "n10": (10, LOGQ, 65537)}
_rnd = random.Random("bgv polynomial coefficients")
POLYS = {
    "square": [0, 0, 1],                                                 # the reference's own (polynomial_evaluator_test.go)
    "dense7": [_rnd.randrange(1, 257) for _ in range(8)],
    "pow2_8": [_rnd.randrange(1, 257) for _ in range(9)],                # a power of two: the split changes
    "odd7": [0 if i % 2 == 0 else _rnd.randrange(1, 257) for i in range(8)],
    "even6": [0 if i % 2 == 1 else _rnd.randrange(1, 257) for i in range(7)],
    "dense31": [_rnd.randrange(1, 65537) for _ in range(32)],
    "gap7": [_rnd.randrange(1, 257) for _ in range(6)] + [0, 5],         # a zero leading-but-one coefficient
}
VECTOR = ([_rnd.randrange(1, 257) for _ in range(8)], [_rnd.randrange(1, 257) for _ in range(8)])      # two polynomials of degree 7
POLYS["odd7_only"], POLYS["even6_only"] = POLYS["odd7"], POLYS["even6"]     # the same coefficients with IsEven / IsOdd cleared: the zero powers are never built
FLAGS = {"odd7_only": (True, False), "even6_only": (False, True)}        # name -> (IsOdd, IsEven); both true from the constructor otherwise
GPU_CASES = [("n7", name) for name in POLYS] + [("n7", "vector"), ("n10", "dense7"), ("n10", "dense31"), ("n10", "vector")]


def mapping(slots):
    """polynomial 0 on the slots = 0 mod 3, polynomial 1 on the slots = 1 mod 3, over both rows of the 2 x slots/2 matrix; the rest unmapped"""
    return {0: list(range(0, slots, 3)), 1: list(range(1, slots, 3))}


@functools.lru_cache(maxsize=None)
def chain(logN, logQ):
    """Q, one 61-bit P for the relinearisation key and the moduli of ringQMul (bgv/params.go:98-108), from ONE GenModuli call"""
    nb = -(-(sum(logQ) + logN) // 61)
    Q, M = primes.gen_moduli(logN + 1, list(logQ), [61] * (nb + 1))
    Q, M = [int(q) for q in Q], [int(p) for p in M]
    assert fr.nb_qi_mul(Q, logN) <= nb
    return Q, M[:1], M[1:]


class Keyed:
    """a secret key and its relinearisation key from the restated key layer, both arms' parameters, and encrypt / decrypt with the noise"""
    _cache = {}

    def __new__(cls, logN, logQ, t):
        key = (logN, tuple(logQ), t)
        if key not in cls._cache:
            self = object.__new__(cls)
            self.N, self.t = 1 << logN, t
            self.Q, self.Pk, self.QMul = chain(logN, tuple(logQ))
            self.rnd = random.Random("bgv polynomial keys %d %d" % (logN, t))
            self.sk = rr.Secret.sample(self.rnd, self.N)
            self.rlk = rr.relin_key(self.rnd, self.sk, self.Q, self.Pk, len(self.Q) - 1, 0)
            self.P = {inv: bp.Params(self.N, self.Q, self.Pk, t, self.rlk, inv, self.QMul) for inv in (False, True)}
            self.enc = self.P[False].enc
            cls._cache[key] = self
        return cls._cache[key]

    def encrypt(self, values, level=None, scale=1):
        level = len(self.Q) - 1 if level is None else level
        mods = self.Q[:level + 1]
        pt = be.encode(self.enc, level, np.asarray(values, dtype=np.uint64), scale)
        c1 = rr.uniform_poly(self.rnd, self.N, mods)
        return bp.Ct(kr.encrypt_sk(self.sk, self.Q, level, c1, rr.gaussian_coeffs(self.rnd, self.N), pt), scale)

    def decrypt(self, ct):
        """(the decoded slots, log2 of the infinity norm of the noise, log2(Q_level / (2T))): T * phase = M + T e with M centred modulo T"""
        level = ct.level()
        vals = be.decode(self.enc, level, kr.decrypt([np.ascontiguousarray(x) for x in ct.comps], self.sk, self.Q), ct.scale)
        Qb, t = br.prod(self.Q[:level + 1]), self.t
        worst = 0
        for x in rr.phase(ct.comps, self.sk, self.Q):
            v = t * x % Qb
            v = v - Qb if 2 * v > Qb else v
            m = v % t
            m = m - t if 2 * m > t else m
            worst = max(worst, abs((v - m) // t))
        return [int(v) for v in vals], math.log2(max(worst, 1)), math.log2(Qb) - 1 - math.log2(t)


def values_of(k, seed):
    return np.array([random.Random(seed + i).randrange(k.t) for i in range(k.enc.n)], dtype=np.uint64)


# ---- the simulator against the recursion evaluated by hand ------------------------------------------------------------------------------------------
def by_hand(Q, t, invariant, steps, degree, L, s_in):
    """the circuit on (level, scale) pairs alone, with the EVALUATOR's rules (Mul: the product of the scales, or MulScaleInvariant; Rescale: divide
    by the prime consumed; Add: equal scales) and none of the simulator's update formulas: the power basis, then the baby steps the simulator
    placed, combined as EvaluatePatersonStockmeyerPolynomialVector combines them -> (level, scale) of the result"""
    inv = lambda a: pow(a % t, -1, t)
    resc = (lambda a: a) if invariant else (lambda a: (a[0] - 1, a[1] * inv(Q[a[0]]) % t))

    def mul(a, b):
        lv = min(a[0], b[0])
        if invariant:
            return lv, a[1] * b[1] % t * inv(t - math.prod(Q[:lv + 1]) % t) % t
        return lv, a[1] * b[1] % t
    pb = {1: (L, s_in)}

    def gen(n):
        if n not in pb:
            a, b = (n // 2, n // 2) if n & (n - 1) == 0 else ((1 << ((n - 1).bit_length() - 1)) - 1, n + 1 - (1 << ((n - 1).bit_length() - 1)))
            gen(a)
            gen(b)
            pb[n] = resc(mul(pb[a], pb[b]))
    todo = [[p.degree(), (p.level, p.scale)] for p in reversed(steps)]
    for p in steps:
        for k in range(1, p.degree() + 1):
            gen(k)
            assert pb[k][0] >= p.level, "a power below the baby step's level"
    while len(todo) > 1:
        nxt, i = [], 0
        while i < len(todo):
            if i + 1 < len(todo) and todo[i][0] == todo[i + 1][0]:
                deg = 1 << todo[i][0].bit_length()
                gen(deg)
                b = mul(resc(todo[i + 1][1]), pb[deg])
                a = todo[i][1]
                assert a[1] == b[1], "Add of unequal scales in a giant step"
                nxt.append([2 * deg - 1, (min(a[0], b[0]), b[1])])
                i += 2
            else:
                nxt.append([nxt[-1][0] if i == len(todo) - 1 and nxt else todo[i][0], todo[i][1]])   # the last one takes its neighbour's degree (:200-201)
                i += 1
        todo = nxt
    return resc(todo[0][1])


@pytest.mark.parametrize("invariant", [False, True], ids=["standard", "invariant"])
@pytest.mark.parametrize("degree", [2, 7, 8, 31, 33])
def test_simulator_against_the_recursion_by_hand(degree, invariant):
    Q, t = chain(5, (55,) + (45,) * 8)[0], 65537
    L, s_in, target = len(Q) - 1, 3, 11
    sim = bp.Sim(Q, t, invariant)
    assert sim.depth(degree) == (0 if invariant else degree.bit_length() - 1)
    steps = bp.paterson_stockmeyer(sim, bp.Poly(list(range(1, degree + 2))), L, s_in, target)
    assert sum(s.degree() + 1 for s in steps) == degree + 1 and all(0 <= s.scale < t for s in steps)
    if invariant:
        assert all(s.level == L for s in steps)
    else:
        assert L - sim.depth(degree) == min(s.level for s in steps) and steps[0].lead and not any(s.lead for s in steps[1:])
    level, scale = by_hand(Q, t, invariant, steps, degree, L, s_in)
    assert scale == target and level == (L if invariant else L - sim.depth(degree) - 1)


def test_simulator_rescale_and_updates_are_scale_arithmetic_modulo_t():
    Q, t = [1000003, 999983], 257                                        # any integers coprime to t: the rules are arithmetic modulo t
    for q in Q:
        assert math.gcd(q, t) == 1
    std, inv = bp.Sim(Q, t, False), bp.Sim(Q, t, True)
    assert std.rescale((1, 5)) == (0, 5 * pow(Q[1] % t, -1, t) % t) and inv.rescale((1, 5)) == (1, 5)
    assert std.mul((1, 5), (0, 7)) == (0, 35) and inv.mul((1, 5), (0, 7)) == (0, 35 * pow(t - Q[0] % t, -1, t) % t)
    assert std.baby_step(True, 1, 5) == (1, 5 * Q[1] % t) and std.baby_step(False, 1, 5) == (1, 5) and inv.baby_step(True, 1, 5) == (1, 5)
    assert std.giant_step(True, 0, 5, 7) == (1, 5 * pow(7, -1, t) * Q[0] % t) and std.giant_step(False, 0, 5, 7) == (1, 5 * pow(7, -1, t) * Q[1] % t)
    assert inv.giant_step(True, 1, 5, 7) == (1, 5 * pow(7, -1, t) * (t - Q[0] * Q[1] % t) % t)


# ---- baby steps against big-integer sums -------------------------------------------------------------------------------------------------------------
def ntt_rows(k, level, rows):
    mods = k.Q[:level + 1]
    return rr.ntt(np.stack([np.array([int(v) % q for v in rows], dtype=np.uint64) for q in mods]), k.N, mods)


@pytest.mark.parametrize("scales", [(3, 3), (3, 5)], ids=["equal", "ratio"])
def test_baby_steps_against_big_integer_sums(scales):
    """a polynomial and a mapping over synthetic powers (uniform rows, two and three components, one power at a higher level): every word of
    the restated Add / MulThenAdd sequence is the canonical residue of the exact sum"""
    k = Keyed(5, (61, 61), 257)
    P, t, level = k.P[False], k.t, 0
    mods = k.Q[:level + 1]
    rng = np.random.default_rng(5)
    xs, out_scale = scales
    for nc in (2, 3):
        pb = {i: bp.Ct([np.stack([rng.integers(0, q, k.N, dtype=np.uint64) for q in k.Q[:level + 1 + (i % 2)]]) for _ in range(nc)], xs) for i in (1, 2, 3)}
        p = bp.Poly([7, 200, 0, 129])
        r = bp.ratio(P, xs, out_scale)
        got = bp.evaluate_from_power_basis(P, level, [p], None, pb, out_scale)
        tinv = pow(t, -1, br.prod(mods))
        for j in range(nc):
            for i, q in enumerate(mods):
                want = sum(pb[e].comps[j][i].astype(object) * br.center_t(p.coeffs[e] * r, t) for e in (1, 2, 3))
                want = (want + (br.center_t(p.coeffs[0] * out_scale, t) * tinv if j == 0 else 0)) % q
                assert np.array_equal(got.comps[j][i].astype(object), want), (nc, j, i)
        pv = [bp.Poly([1, 2, 3, 4]), bp.Poly([250, 0, 9, 256])]
        mp = mapping(k.enc.n)
        got = bp.evaluate_from_power_basis(P, level, pv, mp, pb, out_scale)
        lift = lambda e, s: ntt_rows(k, level, [int(v) * s % t for v in np.asarray(be.encode_ring_t(k.enc, bp.vector_coefficient(P, pv, mp, e), 1))])
        for j in range(nc):
            for i, q in enumerate(mods):
                want = sum(pb[e].comps[j][i].astype(object) * lift(e, r)[i].astype(object) for e in (1, 2, 3))
                want = (want + (lift(0, out_scale)[i].astype(object) * tinv if j == 0 else 0)) % q
                assert np.array_equal(got.comps[j][i].astype(object), want), ("vector", nc, j, i)
        # the sequence rh_bgv_plain_combination is compared with, on the same plaintexts
        pts = [be.encode(k.enc, level, bp.vector_coefficient(P, pv, mp, e), r) for e in (3, 2, 1)]
        const = be.encode(k.enc, level, bp.vector_coefficient(P, pv, mp, 0), out_scale)
        seq = bp.plain_combination(mods, t, [pb[e].comps for e in (3, 2, 1)], pts, const)
        for j in range(nc):
            assert np.array_equal(seq[j], got.comps[j])


# ---- end to end ------------------------------------------------------------------------------------------------------------------------------------------
def run(setting, name, invariant, target=None, seed=0):
    """-> (the result Ct, expected slots, decoded slots, noise bits, bound bits, input level)"""
    logN, logQ, t = SETTINGS[setting]
    k = Keyed(logN, logQ, t)
    x = values_of(k, seed)
    ct = k.encrypt(x)
    if name == "vector":
        polys, mp = [bp.Poly(c) for c in VECTOR], mapping(k.enc.n)
        want = [0] * k.enc.n
        for i, idx in mp.items():
            for j in idx:
                want[j] = bp.evaluate_exact(polys[i], x[j], t)
    else:
        polys, mp = [bp.Poly(POLYS[name])], None
        polys[0].is_odd, polys[0].is_even = FLAGS.get(name, (True, True))
        want = [bp.evaluate_exact(polys[0], v, t) for v in x]
    out = bp.evaluate(k.P[invariant], ct, polys, mp, ct.scale if target is None else target)
    got, noise, bound = k.decrypt(out)
    return out, want, got, noise, bound, ct.level()


@pytest.mark.parametrize("invariant", [False, True], ids=["standard", "invariant"])
@pytest.mark.parametrize("setting,name", GPU_CASES, ids=lambda v: str(v))
def test_every_gpu_case_decrypts_exactly_with_the_noise_margin(setting, name, invariant):
    """the condition under which the GPU file's exact comparison of decrypted slots is meaningful"""
    out, want, got, noise, bound, top = run(setting, name, invariant)
    degree = len(VECTOR[0]) - 1 if name == "vector" else len(POLYS[name]) - 1
    print("MEASURED %s %s %s: noise 2^%.1f, Q_level / 2T = 2^%.1f, output level %d" % (setting, name, "invariant" if invariant else "standard", noise, bound, out.level()))
    assert out.scale == 1 and out.level() == (top if invariant else top - (degree.bit_length() - 1) - 1)
    assert out.level() >= 1 or invariant
    assert got == want
    assert noise + MARGIN_BITS <= bound


@pytest.mark.parametrize("invariant", [False, True], ids=["standard", "invariant"])
def test_another_target_scale_and_a_prebuilt_power_basis(invariant):
    out, want, got, noise, bound, _ = run("n7", "dense7", invariant, target=77)
    assert out.scale == 77 and got == want and noise + MARGIN_BITS <= bound
    logN, logQ, t = SETTINGS["n7"]
    k = Keyed(logN, logQ, t)
    x = values_of(k, 9)
    ct = k.encrypt(x)
    pb = {1: bp.Ct([c.copy() for c in ct.comps], ct.scale)}
    for n in (2, 3):
        bp.gen_power(k.P[invariant], pb, n, False)
    p = bp.Poly(POLYS["gap7"])
    out = bp.evaluate(k.P[invariant], ct, [p], None, 1, pb=pb)
    assert k.decrypt(out)[0] == [bp.evaluate_exact(p, v, t) for v in x]


def test_degree_33_decrypts_on_the_small_ring():
    """the largest degree of the simulator's list, end to end where it is cheap: N = 32, T = 257, nine primes"""
    k = Keyed(5, (55,) + (45,) * 8, 257)
    x = values_of(k, 33)
    p = bp.Poly([random.Random(i).randrange(257) for i in range(34)])
    for invariant in (False, True):
        out = bp.evaluate(k.P[invariant], k.encrypt(x), [p], None, 1)
        got, noise, bound = k.decrypt(out)
        assert got == [bp.evaluate_exact(p, v, 257) for v in x] and noise + MARGIN_BITS <= bound


# ---- the entry, without a device ----------------------------------------------------------------------------------------------------------------------------
def test_plain_combination_is_declared_exported_and_checks_its_arguments(rh):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ringhip.h")).read(), flags=re.S)
    name = "rh_bgv_plain_combination"
    assert re.search(r"\bint %s\s*\(rh_ring\* r, int level, int nterms," % name, txt), "%s is not declared in include/ringhip.h" % name
    assert re.search(r"\bsize_t %s_table_words\s*\(int nterms\)" % name, txt)
    for path in ("include/ringhip.hpp", "go/ringhip/ringhip.go", "matrix-fhe-lattigo_amd/ringhip.py"):
        assert name in open(os.path.join(ROOT, path)).read(), "%s does not mirror %s" % (path, name)
    L = rh.lib()
    assert hasattr(L, name) and hasattr(L, name + "_table_words"), "libringhip.so does not export %s" % name
    assert L.rh_bgv_plain_combination(None, 0, 0, None, None, None, None, None, None, None, None, 1, None, 0) == -1
    assert b"rh_bgv_plain_combination: null ring handle" in L.rh_last_error()
    assert L.rh_bgv_plain_combination_table_words(7) == 7 * 5 and L.rh_bgv_plain_combination_table_words(-1) == 0
    assert set(rh.bgv_polynomial.FUSED_BGV_POLYNOMIAL) == {"scalar", "vector"}


def test_host_types_and_refusals_without_a_device(rh):
    bpm = rh.bgv_polynomial
    p = bpm.Polynomial([1, 2, 3, 4, 5, 6, 7, 8, 9])
    assert (p.Degree(), p.Depth(), p.IsEven, p.IsOdd, p.Lead, p.MaxDeg) == (8, 3, True, True, True, 8)
    q, r = p.Factorize(4)
    assert (q.Coeffs, r.Coeffs, q.Lead, r.Lead, q.MaxDeg, r.MaxDeg) == ([5, 6, 7, 8, 9], [1, 2, 3, 4], True, False, 8, 3)
    assert p.Evaluate(3, 257) == sum(c * 3 ** i for i, c in enumerate(p.Coeffs)) % 257
    with pytest.raises(rh.RingHipError, match="only `Monomial` is built"):
        bpm.Polynomial([1, 2], basis=rh.polynomial.Chebyshev)
    with pytest.raises(rh.RingHipError, match="polynomial degree must all be the same"):
        bpm.PolynomialVector([[1, 2], [1, 2, 3]])
    v = bpm.PolynomialVector([[1, 2, 3], [4, 5, 6]], {0: [0], 1: [1]})
    assert v.Depth() == 1 and v.IsEven() and v.IsOdd()
    # the device simulator against the restated one, both arms
    Q, t = chain(5, (55,) + (45,) * 8)[0], 65537
    for invariant in (False, True):
        for degree in (2, 7, 8, 31, 33):
            co = list(range(1, degree + 2))
            want = bp.paterson_stockmeyer(bp.Sim(Q, t, invariant), bp.Poly(co), len(Q) - 1, 3, 11)
            have = bpm.Polynomial(co).PatersonStockmeyerPolynomial(bpm.SimEvaluator(Q, t, invariant), len(Q) - 1, 3, 11).Value
            assert [(h.Coeffs, h.Level, h.Scale, h.Lead, h.MaxDeg) for h in have] == [(w.coeffs, w.level, w.scale, w.lead, w.max_deg) for w in want]

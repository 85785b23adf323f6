"""CPU: tests/minimax_restatement.py (what the GPU tests compare the minimax, comparison and inverse circuits against) pinned to decryption under
a real key in the reference's own test set-up, testInsecurePrec90 (comparison_test.go:164-170, inverse_test.go:178-184): LogN 10, LogQ {55, 55,
45 x 10}, LogP {60, 60}, scale 2^90, two levels per rescaling, the encoder and the secret-key bootstrapper at big-float precision, the
reference's inputs and its bounds log2MinPrec - (LogN + 2) on the average precision (ckks.VerifyTestVectors); and the host-side half of the
package (minimax.py, comparison.py) held to the same restatement where it needs no device."""
import json
import math
import os
import random
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import ckks_restatement as cr
import minimax_restatement as mr
import polynomial_restatement as pr
import rlwe_restatement as rr
from oracle import primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "minimax_default_sign.json")
LOGN = 10
S = cr.Scale


def default_sign():
    """DefaultCompositePolynomialForSign (comparison.go:61-71): the recorded rows, CoeffsSignX4Cheby appended"""
    with open(FIXTURE) as f:
        return mr.new_polynomial(json.load(f) + [mr.X4])


class Keyed:
    """testInsecurePrec90 / Prec45 with a real secret, relinearisation and conjugation key and the big-float secret-key bootstrapper"""
    _cache = {}

    def __new__(cls, name):
        if name not in cls._cache:
            self = object.__new__(cls)
            logQ, logP, nb, logscale = {"prec90": ([55, 55] + [45] * 10, [60, 60], 2, 90), "prec45": ([55] + [45] * 11, [60, 60], 1, 45)}[name]
            Q, Pk = primes.gen_moduli(LOGN + 1, logQ, logP)
            self.N, self.Q, self.Pk, self.logscale = 1 << LOGN, [int(q) for q in Q], [int(p) for p in Pk], logscale
            self.rnd = random.Random(90 + nb)
            self.sk = rr.Secret.sample(self.rnd, self.N)
            rlk = rr.relin_key(self.rnd, self.sk, self.Q, self.Pk, len(self.Q) - 1, len(self.Pk) - 1)
            conj = rr.galois_key(self.rnd, self.sk, 2 * self.N - 1, self.Q, self.Pk, len(self.Q) - 1, len(self.Pk) - 1)
            self.btp = mr.SkBootstrapperBig(self.N, self.Q, self.sk, 2 ** logscale, self.rnd)
            self.P = mr.Params(self.N, self.Q, self.Pk, rlk, conj, 2 ** logscale, self.btp, nb, max(53, logscale))
            cls._cache[name] = self
        return cls._cache[name]

    def vector(self, lo, hi, seed):
        """NewTestVector(complex(lo, 0), complex(hi, 0)): real values, uniform"""
        rng = random.Random(seed)
        values = [Fraction(rng.uniform(lo, hi)) for _ in range(self.N // 2)]
        return values, self.btp.encrypt([mpmath.mpf(v.numerator) / v.denominator for v in values], [0] * len(values))


def precision(want, have_re, have_im, logscale):
    """getPrecisionStats (schemes/ckks/precision.go:106-204): the average of -log2 |error| of the real and of the imaginary parts"""
    out = []
    with mpmath.workprec(mr.BIG_PREC):
        for w, h in ((want, have_re), ([0] * len(want), have_im)):
            errs = [abs(mpmath.mpf(a.numerator) / a.denominator - b) if isinstance(a, Fraction) else abs(a - b) for a, b in zip(w, h)]
            out.append(float(sum(logscale if e == 0 else -mpmath.log(e, 2) for e in errs) / len(errs)))
    return out


def check(k, name, want, out, log2MinPrec, keep=None):
    re_, im_ = k.btp.decrypt(out)
    if keep is not None:
        want, re_, im_ = [want[i] for i in keep], [re_[i] for i in keep], [im_[i] for i in keep]
    real, imag = precision(want, re_, im_, k.logscale)
    print("%s: avg log2 precision real %.2f imag %.2f (bound %d)" % (name, real, imag, log2MinPrec - (LOGN + 2)))
    assert min(real, imag) >= log2MinPrec - (LOGN + 2), (name, real, imag)
    return real, imag


# ---- comparison_test.go: Sign, Step, Max, Min from 90 bits --------------------------------------------------------------------------------------------------
def test_sign_decrypts_to_the_reference_bound():
    """measured: real 82.1, imag 83.9 bits (bound 78); the other figures are in DESIGN.md"""
    k, mcp = Keyed("prec90"), default_sign()
    values, ct = k.vector(-1, 1, 1)
    out = mr.sign(k.P, ct, mcp)
    assert out.scale.v == 2 ** 90
    check(k, "Sign", [mr.evaluate_exact(mcp, v)[0] for v in values], out, 90)


def test_step_decrypts_to_the_reference_bound():
    k, mcp = Keyed("prec90"), default_sign()
    values, ct = k.vector(-1, 1, 2)
    out = mr.step(k.P, ct, mcp)
    check(k, "Step", [mr.evaluate_exact(mcp, v)[0] / 2 + Fraction(1, 2) for v in values], out, 90)


@pytest.mark.parametrize("what", ["Max", "Min"])
def test_max_min_decrypt_to_the_reference_bound(what):
    k, mcp = Keyed("prec90"), default_sign()
    v0, ct0 = k.vector(-0.5, 0.5, 3)
    v1, ct1 = k.vector(-0.5, 0.5, 4)
    out = (mr.maximum if what == "Max" else mr.minimum)(k.P, ct0, ct1, mcp)
    check(k, what, [(max if what == "Max" else min)(a, b) for a, b in zip(v0, v1)], out, 90)


# ---- inverse_test.go: from 70 bits, logmin = -30, logmax = 10 -------------------------------------------------------------------------------------------------
LOGMIN, LOGMAX = -30.0, 10.0


def test_goldschmidt_division_decrypts_to_the_reference_bound():
    k = Keyed("prec90")
    lo = 2.0 ** LOGMIN
    values, ct = k.vector(lo, 2 - lo, 5)
    out = mr.goldschmidt_division(k.P, ct, LOGMIN)
    check(k, "GoldschmidtDivisionNew", [1 / v for v in values], out, 70)


@pytest.mark.parametrize("domain", ["Positive", "Negative", "Full"])
def test_inverse_domains_decrypt_to_the_reference_bound(domain):
    k = Keyed("prec90")
    hi = 2.0 ** LOGMAX
    lo_, hi_ = {"Positive": (0, hi), "Negative": (-hi, 0), "Full": (-hi, hi)}[domain]
    values, ct = k.vector(lo_, hi_, 6 + len(domain))
    keep = [i for i, v in enumerate(values) if abs(v) >= Fraction(2) ** int(LOGMIN)]
    assert len(keep) == len(values), "the seeded inputs skip no slot"
    if domain == "Positive":
        out = mr.inverse(k.P, ct, LOGMIN, LOGMAX)
    elif domain == "Negative":
        out = mr.inverse_negative(k.P, ct, LOGMIN, LOGMAX)
    else:
        out = mr.inverse(k.P, ct, LOGMIN, LOGMAX, True, default_sign())
    check(k, domain + "Domain", [1 / v for v in values], out, 70, keep)


# ---- Prec45: the sanity bound the GPU end-to-end test uses -------------------------------------------------------------------------------------------------------
def test_sign_at_prec45_meets_the_sanity_bound():
    """every slot with |x| >= 2^-4 within 2^-10 of sign(x) (the polynomial's stated precision is 2^-21)"""
    k, mcp = Keyed("prec45"), default_sign()
    values, ct = k.vector(-1, 1, 9)
    re_, _ = k.btp.decrypt(mr.sign(k.P, ct, mcp))
    errs = [abs(float(h) - (1 if v > 0 else -1)) for v, h in zip(values, re_) if abs(v) >= Fraction(1, 16)]
    print("Sign at Prec45: largest error 2^%.2f over %d slots" % (math.log2(max(errs)), len(errs)))
    assert max(errs) < 2.0 ** -10


# ---- the package's host side against the restatement ----------------------------------------------------------------------------------------------------------------
def test_package_host_side_matches_the_restatement(rh):
    M = rh.minimax
    mcp, want = M.Polynomial.from_json(FIXTURE, [M.CoeffsSignX4Cheby]), default_sign()
    assert M.CoeffsSignX2Cheby == mr.X2 and M.CoeffsSignX4Cheby == mr.X4 and len(mcp) == 9 and mcp.MaxDepth() == mr.max_depth(want) == 5
    for a, b in zip(mcp, want):
        assert (a.prec, a.Basis, a.A, a.B) == (b.prec, pr.CHEBYSHEV, -1, 1) and [(c.re, c.im) for c in a.Coeffs] == b.coeffs
    # the two tables are the Chebyshev forms of their monomials: the identity at rational points, exactly
    for table, mono in ((M.CoeffsSignX2Cheby, mr.MONO_X2), (M.CoeffsSignX4Cheby, mr.MONO_X4)):
        p = M.Polynomial([table])
        for x in (Fraction(-1), Fraction(1, 4), Fraction(7, 8), Fraction(0)):         # dyadic: Evaluate takes x at 64 bits
            assert p.Evaluate(x).re == sum(m * x ** i for i, m in enumerate(mono))
    x = Fraction(-3, 8)
    got = mcp.Evaluate(x)
    assert (got.re, got.im) == mr.evaluate_exact(want, x)
    cmp_ = rh.comparison.Evaluator(None, mcp)
    for a, b in zip(cmp_.StepPolynomial(), mr.step_polynomial(want)):
        assert [(c.re, c.im) for c in a.Coeffs] == b.coeffs
    assert [(c.re, c.im) for c in mcp[-1].Coeffs] == want[-1].coeffs       # Step works on a clone
    with open(os.path.join(ROOT, "profiles", "minimax.json")) as f:               # the defaults are what the measurement found
        profile = json.load(f)
    assert rh.polynomial.FUSED_POWER_BASIS == profile["fused_power_basis_default"] and M.FUSED_MINIMAX == profile["fused_minimax_default"]
    assert "chebyshev_step" not in rh.ckks.Evaluator.FUSED_DEFAULT
    assert hasattr(rh.lib(), "rh_ckks_axpby")

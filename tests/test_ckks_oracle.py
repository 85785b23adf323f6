"""CPU: tests/ckks_restatement.py (the restated schemes/ckks/evaluator.go the GPU tests compare against) pinned to big-integer ground truth
that does not depend on the composition, the 128-bit scale arithmetic on its own, and the new C entry points' declarations."""
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

import ckks_restatement as cr
from bfv_restatement import crt, intt, prod
from oracle import primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGN = 5
N = 1 << LOGN
MODS = [int(q) for q in primes.gen_moduli(LOGN + 1, [61, 61], [])[0]]
QB = prod(MODS)
S = cr.Scale


def uniform(rng, kind="uniform"):
    if kind == "q_minus_1":
        return np.stack([np.full(N, q - 1, dtype=np.uint64) for q in MODS])
    if kind == "zero":
        return np.zeros((len(MODS), N), dtype=np.uint64)
    return np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in MODS])


def big(p):
    """(limbs, N) residues -> N Python ints modulo Q: CRT position by position (a ring isomorphism, so element-wise identities carry over)"""
    return crt(p, MODS)


@pytest.fixture(scope="module")
def polys():
    rng = np.random.default_rng(11)
    out = {k: uniform(rng) for k in ("a0", "a1", "a2", "b0", "b1", "b2", "z0", "z1", "z2", "pt")}
    out["m0"], out["m1"] = uniform(rng, "q_minus_1"), uniform(rng, "zero")
    return out


@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("s0,s1", [(2 ** 40, 2 ** 40), (2 ** 45 * 3, 2 ** 40), (2 ** 40, 5 * 2 ** 41 + 7)])
@pytest.mark.parametrize("d0,d1", [(2, 2), (2, 3), (3, 2), (2, 1)])
def test_add_sub_is_a_times_ratio_plus_minus_b(polys, sub, s0, s1, d0, d1):
    a, b = [polys["a0"], polys["m0"], polys["a2"]][:d0], [polys["b0"], polys["b1"], polys["m1"]][:d1]
    out, scale = cr.add_sub(N, MODS, a, S(s0), b, S(s1), sub)
    ra, rb = (1, Fraction(s0, s1).__floor__()) if s0 > s1 else (Fraction(s1, s0).__floor__(), 1) if s1 > s0 else (1, 1)
    assert scale == max(s0, s1) and len(out) == max(d0, d1)
    sign = -1 if sub else 1
    for j, o in enumerate(out):
        x = big(a[j]) if j < d0 else [0] * N
        y = big(b[j]) if j < d1 else [0] * N
        assert big(o) == [(u * ra + sign * v * rb) % QB for u, v in zip(x, y)], "component %d" % j
    for alias in ("op0", "op1"):                                        # the branch taken never changes a value
        again, sc = cr.add_sub(N, MODS, a, S(s0), b, S(s1), sub, alias=alias)
        assert sc == scale and all(np.array_equal(u, v) for u, v in zip(out, again))


def test_neg_of_zero_is_q_like_the_reference(polys):
    # ring.Neg is q - x (ring/vec_ops.go:103): Sub of a degree-1 and a degree-2 element whose last component is zero leaves q_i there
    out, _ = cr.add_sub(N, MODS, [polys["a0"], polys["a1"]], S(8), [polys["b0"], polys["b1"], polys["m1"]], S(8), True)
    for i, q in enumerate(MODS):
        assert np.all(out[2][i] == q)


@pytest.mark.parametrize("square", [False, True])
def test_tensor_components(polys, square):
    a = [polys["a0"], polys["a1"]]
    b = a if square else [polys["b0"], polys["b1"]]
    (c0, c1, c2), scale = cr.mul_relin(MODS, a, S(2 ** 40), b, S(2 ** 41), square)
    A0, A1, B0, B1 = big(a[0]), big(a[1]), big(b[0]), big(b[1])
    assert scale == 2 ** 81                                              # no 2^-64 left: MForm and MRed cancel
    assert big(c0) == [x * y % QB for x, y in zip(A0, B0)]
    assert big(c1) == [(x * v + y * u) % QB for x, y, u, v in zip(A0, A1, B0, B1)]
    assert big(c2) == [x * y % QB for x, y in zip(A1, B1)]
    z = [polys["z0"], polys["z1"], polys["z2"]]
    Z = [big(p) for p in z]
    out, sc, none = cr.mul_relin_then_add(N, MODS, a, S(2 ** 40), b, S(2 ** 41), z, S(2 ** 81), False)
    assert none is None and sc == 2 ** 81
    assert big(out[0]) == [(w + x * y) % QB for w, x, y in zip(Z[0], A0, B0)]
    assert big(out[1]) == [(w + x * v + y * u) % QB for w, x, y, u, v in zip(Z[1], A0, A1, B0, B1)]
    assert big(out[2]) == [(w + x * y) % QB for w, x, y in zip(Z[2], A1, B1)]
    out, sc, c2r = cr.mul_relin_then_add(N, MODS, a, S(2 ** 40), b, S(2 ** 41), z[:2], S(2 ** 81), True)
    assert big(c2r) == [x * y % QB for x, y in zip(A1, B1)] and big(out[0]) == [(w + x * y) % QB for w, x, y in zip(Z[0], A0, B0)]


def test_plaintext_branches(polys):
    ct = [polys["a0"], polys["m0"], polys["a2"]]
    P = big(polys["pt"])
    for d in (1, 2, 3):
        out, scale = cr.mul_relin(MODS, ct[:d], S(3), [polys["pt"]], S(5))
        assert scale == 15
        for j in range(d):
            assert big(out[j]) == [x * y % QB for x, y in zip(big(ct[j]), P)]
        z = [polys["z0"], polys["z1"], polys["z2"]]
        acc, _, _ = cr.mul_relin_then_add(N, MODS, ct[:d], S(3), [polys["pt"]], S(5), z, S(15), False)
        for j in range(3):
            want = [(w + x * y) % QB for w, x, y in zip(big(z[j]), big(ct[j]), P)] if j < d else big(z[j])
            assert big(acc[j]) == want


def test_scale_up_of_the_accumulator_at_ratio_two(polys):
    a, b = [polys["a0"], polys["a1"]], [polys["b0"], polys["b1"]]
    z = [polys["z0"], polys["z1"], polys["z2"]]
    # ratio 2.0 and 3.00..: scaled by the integer; 2.5: not a Gaussian integer, so Mul scales by round(2.5 q_level) (:662-671); 1.99..: left alone
    for sout, scaled in ((2 ** 80, True), (2 ** 81 // 3, True), (2 ** 82 // 5, True), (2 ** 80 + 2 ** 30, False)):
        out, sc, _ = cr.mul_relin_then_add(N, MODS, a, S(2 ** 40), b, S(2 ** 41), z, S(sout), False)
        ratio = S(2 ** 81).div(S(sout))
        assert (ratio.float64() >= 2.0) == scaled
        assert sc == (2 ** 81 if scaled else sout)
        c = cr.to_complex(ratio.v, 53)                                    # a *big.Float: rounded to EncodingPrecision bits
        k = 1 if not scaled else int(c[0]) if cr.is_int(c) else cr.scaled_part(c[0], S(MODS[-1]), 53)
        assert k in (1, 2, 3) or abs(k - Fraction(5, 2) * MODS[-1]) <= 2 ** 10
        assert big(out[2]) == [(w * k + x * y) % QB for w, x, y in zip(big(z[2]), big(a[1]), big(b[1]))]
    assert S(4).div(S(2)).float64() >= 2.0 and not S(2 ** 81 - 2 ** 29).div(S(2 ** 80)).float64() >= 2.0      # 2.0, and 2 - 2^-51
    assert S(2 ** 81 - 1).div(S(2 ** 80)).float64() == 2.0               # 2 - 2^-80 is below the float64 grid: Float64 rounds it to 2.0


@pytest.mark.parametrize("const", [3, -2, 0.5, 1.25 - 0.75j, 0, 2 ** 60 + 1])
def test_scalars_against_big_integers(polys, const):
    ct = [polys["a0"], polys["m0"]]
    sr = cr.subrings(N, tuple(MODS))
    coeffs = [crt(intt(p, sr), MODS) for p in ct]

    def times(real, imag, v):
        """(real + imag X^(N/2)) * v in Z_Q[X]/(X^N + 1)"""
        rot = [-x for x in v[N // 2:]] + v[:N // 2]
        return [(real * x + imag * y) % QB for x, y in zip(v, rot)]
    c = cr.to_complex(const, 53)
    # Mul: a Gaussian integer as it is, otherwise round(c * q_level), half away from zero
    scale = S(1) if cr.is_int(c) else S(MODS[-1])
    re_, im_ = (int(c[0]), int(c[1])) if cr.is_int(c) else (cr.scaled_part(c[0], scale, 53), cr.scaled_part(c[1], scale, 53))
    if not cr.is_int(c):
        for part, got in ((c[0], re_), (c[1], im_)):
            exact = part * MODS[-1]
            assert abs(got - exact) <= Fraction(1, 2) + Fraction(abs(exact), 2 ** 127)
    elif const == 2 ** 60 + 1:
        assert re_ == 2 ** 60                                            # a *big.Int is rounded to EncodingPrecision bits by bignum.ToComplex
    out, sc = cr.mul_scalar(N, MODS, ct, S(2 ** 40), const)
    assert sc == 2 ** 40 * scale.v
    for j in range(2):
        assert crt(intt(out[j], sr), MODS) == times(re_, im_, coeffs[j])
    # Add / Sub at the ciphertext's scale: component 0 only
    s40 = S(2 ** 40)
    re_, im_ = cr.scaled_part(c[0], s40, 53), cr.scaled_part(c[1], s40, 53)
    one = [1] + [0] * (N - 1)
    for sub in (False, True):
        out, sc = cr.add_sub_scalar(N, MODS, ct, s40, const, sub)
        shift = times(re_, im_, one)
        assert crt(intt(out[0], sr), MODS) == [(x - y if sub else x + y) % QB for x, y in zip(coeffs[0], shift)]
        assert np.array_equal(out[1], ct[1]) and sc == 2 ** 40
    # MulThenAdd: equal scales (opOut scaled by q_level first unless the constant is a Gaussian integer), and opOut.Scale = 4 op0.Scale
    z = [polys["z0"], polys["z1"]]
    zc = [crt(intt(p, sr), MODS) for p in z]
    out, sc = cr.mul_then_add_scalar(N, MODS, ct, s40, const, z, s40)
    k = 1 if cr.is_int(c) else cr.scaled_part(cr.to_complex(MODS[-1], 53)[0], S(1), 53)
    m_re, m_im = (int(c[0]), int(c[1])) if cr.is_int(c) else (cr.scaled_part(c[0], S(MODS[-1]), 53), cr.scaled_part(c[1], S(MODS[-1]), 53))
    assert sc == (2 ** 40 if cr.is_int(c) else S(2 ** 40).mul(S(MODS[-1])).v)
    for j in range(2):
        assert crt(intt(out[j], sr), MODS) == [(k * w + x) % QB for w, x in zip(zc[j], times(m_re, m_im, coeffs[j]))]
    out, sc = cr.mul_then_add_scalar(N, MODS, ct, s40, const, z, S(2 ** 42))
    m_re, m_im = cr.scaled_part(c[0], S(4), 53), cr.scaled_part(c[1], S(4), 53)
    assert sc == 2 ** 42
    for j in range(2):
        assert crt(intt(out[j], sr), MODS) == [(w + x) % QB for w, x in zip(zc[j], times(m_re, m_im, coeffs[j]))]
    with pytest.raises(ValueError, match="op0.Scale > opOut.Scale is not supported"):
        cr.mul_then_add_scalar(N, MODS, ct, S(2 ** 42), const, z, s40)


def test_scale_rounds_to_128_bits_after_every_step():
    q = MODS[-1]
    assert q.bit_length() == 61
    s = S(2 ** 128 - 1)                                                  # 128 significant bits
    down = s.div(S(q))
    exact = Fraction(2 ** 128 - 1, q)
    assert down.v != exact                                               # the quotient is not representable: rounded to 128 bits ...
    n = down.v.numerator
    assert n.bit_length() - (n & -n).bit_length() + 1 <= 128 and abs(down.v - exact) <= exact / 2 ** 128
    back = down.mul(S(q))
    assert back.v == 2 ** 128 != s.v                                     # ... and the product back is one off the start: the rounding is visible
    small = S(2 ** 90 + 1)
    assert small.div(S(q)).mul(S(q)).v == small.v                        # with bits to spare the round trip is exact
    assert cr.round_bits(Fraction(2 ** 128 + 1), 128) == 2 ** 128 and cr.round_bits(Fraction(2 ** 128 + 3), 128) == 2 ** 128 + 4   # ties to even
    assert cr.round_bits(Fraction(2 ** 128 + 2), 128) == 2 ** 128 + 2 and cr.round_bits(Fraction(-(2 ** 128 + 1)), 128) == -(2 ** 128)
    assert S(5).cmp(S(7)) == -1 and S(7).cmp(S(5)) == 1 and S(5).cmp(S(5)) == 0 and S(5).max(S(7)) == 7 and S(7).max(S(5)) == 7
    assert S(0.5).float64() == 0.5 and S(2 ** 200 + 1).float64() == float(2 ** 200)


def test_the_library_scale_agrees_with_the_restated_one(rh):
    rnd = random.Random(5)
    for _ in range(200):
        a, b = rnd.getrandbits(rnd.randrange(1, 140)) + 1, rnd.getrandbits(rnd.randrange(1, 70)) + 1
        x, y = rh.ckks.Scale(a), rh.ckks.Scale(b)
        u, v = S(a), S(b)
        assert x.Mul(y).Value == u.mul(v).v and x.Div(y).Value == u.div(v).v and x.Div(y).Mul(y).Value == u.div(v).mul(v).v
        assert x.Cmp(y) == u.cmp(v) and x.Max(y).Value == u.max(v).v and x.Div(y).Float64() == u.div(v).float64()
    c = rnd.random() * 1000 - 500
    for value in (3, -2, 0.5, 1.25 - 0.75j, 0, c, 2 ** 70 + 12345):
        assert tuple(rh.ckks.to_complex(value, 53)) == tuple(cr.to_complex(value, 53))
        for part in cr.to_complex(value, 53):
            for sc in (1, MODS[-1], Fraction(2 ** 90 + 1, MODS[0])):
                assert rh.ckks.scaled_int(part, rh.ckks.Scale(sc).Value, 53) == cr.scaled_part(part, S(sc), 53)
    for k in (0, 1, 2, -1, -5, N // 2, 1000):
        assert rh.ckks.GaloisElement(N, k) == cr.galois_element(N, k)
        assert rh.ckks.GaloisElement(N, k) * rh.ckks.GaloisElement(N, -k) % (2 * N) == 1
    assert rh.ckks.GaloisElementOrderTwoOrthogonalSubgroup(N) == 2 * N - 1


def test_rescale_to_stops_at_half_the_target():
    q0, q1 = MODS
    # (scale, minScale) -> divisions: the loop divides while the quotient stays >= minScale / 2, down to the last modulus
    s = S(q0).mul(S(q1)).mul(S(2 ** 40))
    assert cr.rescale_to_count(MODS, s, S(2 ** 40))[0] == 2
    assert cr.rescale_to_count(MODS, s, S(2 ** 100))[0] == 1
    assert cr.rescale_to_count(MODS, s, S(2 ** 41))[0] == 2              # 2^40 >= 2^41 / 2: the boundary divides
    assert cr.rescale_to_count(MODS, s, S(2 ** 41 + 2 ** 20))[0] == 1   # just above it does not
    assert cr.rescale_to_count(MODS, S(2 ** 40), S(2 ** 40)) == (0, S(2 ** 40))
    nb, out = cr.rescale_to_count(MODS, s, S(2 ** 40))
    assert out == s.div(S(q1)).div(S(q0)).v


def test_rescale_divides_and_rounds(polys):
    x = polys["a0"]
    down, scale = cr.rescale(N, MODS, [x], S(2 ** 100))
    sr = cr.subrings(N, tuple(MODS))
    q1 = MODS[-1]
    want = [((v + q1 // 2) // q1) % MODS[0] for v in crt(intt(x, sr), MODS)]
    assert [int(v) for v in intt(down[0], sr[:1])[0]] == want and scale == S(2 ** 100).div(S(q1)).v


def test_new_entry_points_are_declared_and_exported(rh):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ringhip.h")).read(), flags=re.S)
    for name in ("rh_ckks_tensor", "rh_ckks_mul_plain", "rh_ckks_scalar", "rh_ckks_scale_then_add"):
        assert re.search(r"\bint %s\s*\(rh_ring\* r, int level," % name, txt), "%s is not declared in include/ringhip.h" % name
        assert hasattr(rh.lib(), name), "libringhip.so does not export %s" % name
    # host-side argument checks that need no device
    L = rh.lib()
    assert L.rh_ckks_tensor(None, 0, *[None] * 7, 1, 0, 0) == -1 and b"null ring handle" in L.rh_last_error()
    assert L.rh_ckks_scalar(None, 0, 0, *[None] * 6, 1, None, None) == -1
    assert L.rh_ckks_mul_plain(None, 0, *[None] * 7, 1, 0) == -1 and L.rh_ckks_scale_then_add(None, 0, *[None] * 9, 1, None, 0, 0) == -1

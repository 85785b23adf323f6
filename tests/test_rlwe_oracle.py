"""CPU: the oracle compositions of the key-switch callers (oracle/compose.py, and the evaluators' call sequences restated in
tests/rlwe_restatement.py and tests/ckks_restatement.py) pinned to DECRYPTION under real keys -- the statement the reference's own tests make
(core/rlwe/rlwe_test.go: testGadgetProduct :690-798, testApplyEvaluationKey :800-914, testAutomorphism :916-1079; core/rgsw/rgsw_test.go:61-113).
With uniformly random keys "kernel == composition" cannot see a misreading both sides share (a key row paired with the wrong digit, the wrong
row order under a power-of-two decomposition, a Galois key applied with the wrong index map, swapped RGSW halves ...); a real key can: the
ciphertext then decrypts to noise of about log2(Q) - 2 bits.  tests/test_gpu_rlwe_decrypt.py runs the same keys through the device path and may
only use shapes that pass here.

Bounds, from the reference and not from this code: log2 of the standard deviation of the decryption error <= logN + BaseTwoDecomposition
(NoiseBound, rlwe_test.go:703, :809), plus log2(level + 1) + 1 for automorphisms under a power-of-two decomposition (:925-929); the external
product decrypts, after DivRound by q_0, to the monomial exactly (rgsw_test.go:98-112).

Chains.  REF: the reference's own (tests/golden/rlwe_test_moduli.json, N = 2^10) with its three settings (pw2, #P) = (0, 2), (16, 1), (2, 0), and
(0, 1), the LevelP = 0 key testGadgetProduct also makes (:705-713).  Q61: gen_moduli 61 x 6 | 61, 61 at N = 2^10 with the same four settings;
Q61N13: the same widths at N = 2^13, both P (the two-pass device shape).  SPLIT3: gen_moduli 55, 45, 45 | 61, 61 at N = 2^10.  TAIL: 7 | 4 61-bit
primes at N = 32 (a last digit of 3 limbs).  RGSW: gen_moduli 35, 20 | 61, 61, the reference's RGSW test.  Keys are made at the top level and used
at the top and two lower levels, one of which changes the number of digits.  (pw2, #P) = (0, 0) -- no P and no power-of-two decomposition --
is not kept: its error is a whole digit times the key's error, about log2(q_i) bits, far above logN; the reference does not test it either.

Measured log2 of the standard deviation of the error, the largest over the cases of each kept shape (bound in brackets):

  chain   pw2 #P   key switch      automorphism    relinearise     rotate k, -k
  REF       0  2    2.92 [10.00]    3.05 [10.00]    3.00 [10.00]    3.46 [11.00]
  REF      16  1    2.96 [26.00]    3.08 [29.32]    2.99 [26.00]         -
  REF       2  0   10.67 [12.00]   10.91 [15.32]   10.71 [12.00]         -
  REF       0  1    2.97 [10.00]    3.08 [10.00]    2.93 [10.00]         -
  Q61       0  2    5.65 [10.00]    5.79 [10.00]    5.70 [10.00]         -
  Q61      16  1    2.93 [26.00]         -               -               -
  Q61       2  0   11.29 [12.00]         -               -               -
  Q61       0  1    6.20 [10.00]         -               -               -
  Q61N13    0  2    7.20 [13.00]    7.21 [13.00]    7.21 [13.00]    7.70 [14.00]
  SPLIT3    0  2    2.91 [10.00]    3.17 [10.00]    2.99 [10.00]         -
  SPLIT3    0  1    2.92 [10.00]    3.07 [10.00]    2.97 [10.00]         -
  TAIL      0  4    2.64 [ 5.00]    2.84 [ 5.00]    2.38 [ 5.00]    2.92 [ 6.00]
  TAIL      0  1    3.78 [ 5.00]    4.06 [ 5.00]    3.42 [ 5.00]         -
  TAIL     16  1    0.48 [21.00]    1.94 [24.81]    0.80 [21.00]         -

The negative controls (swapped key rows, the Galois key of g with the map of g^-1, swapped RGSW halves) must miss the bound by more than 10 bits.
"""
import functools
import json
import math
import os
import random

import numpy as np
import pytest

import ckks_restatement as cr
import rlwe_restatement as rr
from conftest import QI60, PI60
from oracle import compose, primes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def chain(name):
    """(N, Q, P, levels): levels = the top level and two lower ones, one with another digit count under the full P"""
    with open(os.path.join(ROOT, "tests", "golden", "rlwe_test_moduli.json")) as f:
        gold = json.load(f)
    if name == "REF":
        return 1 << gold["rlwe"]["LogN"], tuple(gold["rlwe"]["Q"]), tuple(gold["rlwe"]["P"]), (4, 3, 1)
    if name == "RGSW":
        Q, P = primes.gen_moduli(gold["rgsw"]["LogN"] + 1, gold["rgsw"]["LogQ"], gold["rgsw"]["LogP"])
        return 1 << gold["rgsw"]["LogN"], tuple(Q), tuple(P), (1, 0)
    if name in ("Q61", "Q61N13"):
        logN = 13 if name == "Q61N13" else 10
        Q, P = primes.gen_moduli(logN + 1, [61] * 6, [61, 61])
        return 1 << logN, tuple(Q), tuple(P), (5, 4, 1)
    if name == "SPLIT3":
        Q, P = primes.gen_moduli(11, [55, 45, 45], [61, 61])
        return 1024, tuple(Q), tuple(P), (2, 1, 0)
    if name == "TAIL":
        return 32, tuple(QI60[:7]), tuple(PI60[:4]), (6, 5, 2)
    raise KeyError(name)


def ref_settings():
    with open(os.path.join(ROOT, "tests", "golden", "rlwe_test_moduli.json")) as f:
        return [(s["BaseTwoDecomposition"], s["PCount"]) for s in json.load(f)["rlwe"]["settings"]]


FOUR = [(0, 2), (16, 1), (2, 0), (0, 1)]                                # the reference's three settings (asserted below) and the LevelP = 0 key
assert FOUR[:3] == ref_settings()
SHAPES = [("REF", s) for s in FOUR] + [("Q61", s) for s in FOUR] + [("Q61N13", (0, 2)), ("SPLIT3", (0, 2)), ("SPLIT3", (0, 1)),
                                                                     ("TAIL", (0, 4)), ("TAIL", (0, 1)), ("TAIL", (16, 1))]
_ids = lambda v: "%s-pw%d-p%d" % (v[0], v[1][0], v[1][1]) if isinstance(v, tuple) and isinstance(v[1], tuple) else None


@functools.lru_cache(maxsize=None)
def secrets(name):
    N = chain(name)[0]
    rnd = random.Random("sk " + name)
    return rr.Secret.sample(rnd, N), rr.Secret.sample(rnd, N)


@functools.lru_cache(maxsize=None)
def key(name, setting, kind, g=0):
    """one real key per (chain, setting, kind), made at the top level: "switch" sk -> skOut, "relin", "galois" of g"""
    N, Q, P, levels = chain(name)
    pw2, pc = setting
    sk, sk_out = secrets(name)
    rnd = random.Random("%s %s %s %d" % (name, setting, kind, g))
    args = (Q, P[:pc], levels[0], pc - 1, pw2)
    if kind == "switch":
        return rr.gadget_key(rnd, sk, sk_out, *args)
    if kind == "relin":
        return rr.relin_key(rnd, sk, *args)
    return rr.galois_key(rnd, sk, g, *args)


@functools.lru_cache(maxsize=None)
def rgsw(name, setting, k0):
    N, Q, P, levels = chain(name)
    pw2, pc = setting
    m = [0] * N
    m[k0] = 1
    return rr.rgsw_encrypt(random.Random("rgsw %s %s %d" % (name, setting, k0)), secrets(name)[0], m, Q, P[:pc], levels[0], pc - 1, pw2)


def bound(N, pw2, level=None):
    b = (N.bit_length() - 1) + pw2                                       # NoiseBound (rlwe_test.go:703, :809)
    if level is not None and pw2:
        b += math.log2(level + 1) + 1                                    # automorphisms (:925-929)
    return b


def report(what, name, setting, level, got, bnd):
    print("MEASURED %-12s %-7s pw2=%-2d P=%d level=%d  %6.2f  [%.2f]" % (what, name, setting[0], setting[1], level, got, bnd))


def switch_error(name, setting, level, a, out, is_ntt=True):
    """log2 std of phase_skOut(out) - a sk (rlwe_test.go:733-749)"""
    N, Q, P, _ = chain(name)
    sk, sk_out = secrets(name)
    mods = Q[:level + 1]
    if not is_ntt:
        a, out = rr.ntt(a, N, mods), [rr.ntt(x, N, mods) for x in out]
    got = rr.phase(list(out), sk_out, Q)
    want = rr.phase([np.zeros_like(a), a], sk, Q)
    return rr.log2_std(rr.centered_diff(got, want, rr.prod(mods)))


@functools.lru_cache(maxsize=None)
def switch_case(name, setting, level):
    """(a, oracle gadget product of a with the sk -> skOut key), NTT domain: shared with the GPU tests"""
    N, Q, P, _ = chain(name)
    a = rr.uniform_poly(random.Random("a %s %d" % (name, level)), N, Q[:level + 1])
    return a, rr.gadget_product(N, Q, P[:setting[1]], level, a, key(name, setting, "switch"))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_key_switch_decrypts(oracle, shape):
    """testGadgetProduct (:690-750): GadgetProduct(a, evk(sk -> skOut)) decrypts under skOut to a sk, NTT- and coefficient-domain input, with a
    top-level key at three levels"""
    name, setting = shape
    N, Q, P, levels = chain(name)
    k = key(name, setting, "switch")
    for level in levels:
        a, out = switch_case(name, setting, level)
        got = switch_error(name, setting, level, a, out)
        report("keyswitch", name, setting, level, got, bound(N, setting[0]))
        assert got <= bound(N, setting[0])
        if level != levels[1]:
            ac = rr.intt(a, N, Q[:level + 1])
            got = switch_error(name, setting, level, ac, rr.gadget_product(N, Q, P[:setting[1]], level, ac, k, is_ntt=False), is_ntt=False)
            report("keyswitch/c", name, setting, level, got, bound(N, setting[0]))
            assert got <= bound(N, setting[0])


def message(name, tag, size):
    N = chain(name)[0]
    rnd = random.Random("m %s %s" % (name, tag))
    return [rnd.randrange(-size, size + 1) for _ in range(N)]


@functools.lru_cache(maxsize=None)
def fresh(name, tag, level, size=1 << 30):
    """(m, ct, e): a message with coefficients up to 2^30 (genPlaintext, rlwe_test.go:936) and its encryption under sk"""
    N, Q, P, _ = chain(name)
    m = message(name, tag, size)
    ct, e = rr.encrypt(random.Random("ct %s %s %d" % (name, tag, level)), secrets(name)[0], m, Q, level)
    return m, ct, e


def galois_elements(N):
    return [5, pow(5, -1, 2 * N), pow(5, 3, 2 * N), 2 * N - 1]


def auto_error(name, level, out, m, g):
    N, Q, _, _ = chain(name)
    got = rr.phase(list(out), secrets(name)[0], Q)
    return rr.log2_std(rr.centered_diff(got, rr.automorphism_coeffs(m, g), rr.prod(Q[:level + 1])))


@functools.lru_cache(maxsize=None)
def auto_case(name, setting, level, g):
    N, Q, P, _ = chain(name)
    m, ct, _ = fresh(name, "auto", level)
    return m, ct, rr.automorphism(N, Q, P[:setting[1]], ct, key(name, setting, "galois", g), g)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != "Q61" or s[1] == (0, 2)], ids=_ids)
def test_automorphism_decrypts(oracle, shape):
    """testAutomorphism (:916-974): the key switch with GaloisKey[g] then the index map of g decrypts under sk to sigma_g(m)"""
    name, setting = shape
    N, Q, P, levels = chain(name)
    gs = galois_elements(N) if N <= 1024 else [5, 2 * N - 1]
    for g in gs:
        assert math.gcd(g, 2 * N) == 1
        for level in (levels[:2] if g == 5 else levels[:1]):
            m, ct, out = auto_case(name, setting, level, g)
            got = auto_error(name, level, out, m, g)
            report("automorphism", name, setting, level, got, bound(N, setting[0], level))
            assert got <= bound(N, setting[0], level)


def tensor_case(name, level, size=1 << 20):
    """two encryptions with known errors and their exact tensor: the degree-2 phase is (m0 + e0)(m1 + e1) exactly"""
    N, Q, _, _ = chain(name)
    (m0, ct0, e0), (m1, ct1, e1) = fresh(name, "t0", level, size), fresh(name, "t1", level, size)
    want = rr.negacyclic_mul([x + y for x, y in zip(m0, e0)], [x + y for x, y in zip(m1, e1)])
    c, _ = cr.mul_relin(list(Q[:level + 1]), ct0, cr.Scale(1), ct1, cr.Scale(1))
    return ct0, ct1, c, want


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] != "Q61" or s[1] == (0, 2)], ids=_ids)
def test_relinearize_decrypts(oracle, shape):
    """a degree-2 ciphertext built as an exact tensor decrypts to the product exactly; relinearised with a real key, within the key-switch bound"""
    name, setting = shape
    N, Q, P, levels = chain(name)
    sk = secrets(name)[0]
    for level in levels[:2]:
        Ql = rr.prod(Q[:level + 1])
        if Ql.bit_length() < 60:
            continue                                                     # the product of two 2^20 messages needs room below Q / 2
        _, _, c, want = tensor_case(name, level)
        assert rr.phase(c, sk, Q) == want
        lin = rr.relinearize(N, Q, P[:setting[1]], c, key(name, setting, "relin"))
        got = rr.log2_std(rr.centered_diff(rr.phase(lin, sk, Q), want, Ql))
        report("relinearize", name, setting, level, got, bound(N, setting[0]))
        assert got <= bound(N, setting[0])


# ---- RGSW --------------------------------------------------------------------------------------------------------------------------------------
RGSW_SHAPES = [("RGSW", (0, 2)), ("REF", (0, 2)), ("REF", (16, 1)), ("REF", (0, 1)), ("REF", (16, 0)), ("Q61N13", (0, 2)), ("TAIL", (0, 4)), ("TAIL", (16, 1))]


def external_product(name, setting, ct, value):
    N, Q, P, levels = chain(name)
    pw2, pc = setting
    kq, kp = [v.Q for v in value], [v.P for v in value]
    x = np.stack(ct)
    if pc >= 2:
        return compose.external_product(N, Q, P[:pc], levels[0], pc - 1, x, True, kq, kp)
    return compose.external_product_single_p(N, Q, P[:pc], levels[0], pc - 1, x, pw2, value[0].digits_per_limb, kq, kp if pc else [None, None])


@functools.lru_cache(maxsize=None)
def rgsw_case(name, setting, k0, k1):
    """(RLWE of q0 X^k1, oracle external product with the RGSW of X^k0)"""
    N, Q, P, levels = chain(name)
    m = [0] * N
    m[k1] = int(Q[0])                                                    # Scale * X^k1 (rgsw_test.go:72-75)
    ct, _ = rr.encrypt(random.Random("rlwe %s %d" % (name, k1)), secrets(name)[0], m, Q, levels[0])
    return ct, external_product(name, setting, ct, rgsw(name, setting, k0))


def div_round(x, q):
    return (2 * x + q) // (2 * q)


def decrypt_monomial(name, out):
    N, Q, _, _ = chain(name)
    ph = rr.phase(list(out), secrets(name)[0], Q)
    return [div_round(x, int(Q[0])) for x in ph], ph


@pytest.mark.parametrize("shape", RGSW_SHAPES, ids=_ids)
def test_external_product_decrypts_to_the_monomial(oracle, shape):
    """Evaluator/ExternalProduct (rgsw_test.go:61-113): RGSW(X^k0) x RLWE(q0 X^k1) decrypts, after DivRound by q0, to +-X^(k0 + k1 mod N) on every
    coefficient; (3, N - 2) wraps with a sign"""
    name, setting = shape
    N = chain(name)[0]
    for k0, k1 in ((0, 1), (3, N - 2)):
        _, out = rgsw_case(name, setting, k0, k1)
        mono = [0] * N
        mono[k1] = 1
        assert decrypt_monomial(name, out)[0] == rr.monomial_mul(mono, k0), (k0, k1)
    assert rr.monomial_mul(mono, 3)[1] == -1


# ---- CKKS ---------------------------------------------------------------------------------------------------------------------------------------
CKKS_SHAPES = [("REF", (0, 2)), ("Q61N13", (0, 2)), ("TAIL", (0, 4))]
SA, SB = cr.Scale(1 << 30), cr.Scale((1 << 30) + 12345)


@functools.lru_cache(maxsize=None)
def ckks_mul_case(name, setting):
    """MulRelin -> Rescale over the restated evaluator: (ct0, ct1, want, lin, low, scale)"""
    N, Q, P, levels = chain(name)
    level = levels[0]
    mods = list(Q[:level + 1])
    ct0, ct1, _, want = tensor_case(name, level)
    c, sc = cr.mul_relin(mods, ct0, SA, ct1, SB)
    lin = rr.relinearize(N, Q, P[:setting[1]], c, key(name, setting, "relin"))
    low, sc2 = cr.rescale(N, mods, lin, sc)
    return ct0, ct1, want, lin, low, sc2


def rescale_excess(name, lin, low):
    """twice the max over the coefficients of |q_L phase(out) - phase(in)| centred modulo Q_L, and twice the provable bound q_L (1 + |s|_1) / 2: the rescale step
    obeys q_L out_j = in_j - [in_j]_{q_L} per component, the remainders centred"""
    N, Q, _, _ = chain(name)
    sk = secrets(name)[0]
    L = lin[0].shape[0]
    qL = int(Q[L - 1])
    d = rr.centered_diff([qL * x for x in rr.phase(list(low), sk, Q)], rr.phase(list(lin), sk, Q), rr.prod(Q[:L]))
    return 2 * max(abs(x) for x in d), qL * (1 + sum(abs(x) for x in sk.coeffs))


@pytest.mark.parametrize("shape", CKKS_SHAPES, ids=_ids)
def test_ckks_mul_relin_rescale_decrypts(oracle, shape):
    name, setting = shape
    N, Q, P, levels = chain(name)
    ct0, ct1, want, lin, low, sc2 = ckks_mul_case(name, setting)
    got = rr.log2_std(rr.centered_diff(rr.phase(lin, secrets(name)[0], Q), want, rr.prod(Q[:levels[0] + 1])))
    report("ckks/mulrelin", name, setting, levels[0], got, bound(N, 0))
    assert got <= bound(N, 0)
    assert low[0].shape[0] == levels[0]
    worst, limit = rescale_excess(name, lin, low)
    assert worst <= limit
    assert sc2 == cr.Scale(SA.v * SB.v / int(Q[levels[0]]))              # the tracked scale: SA SB / q_L rounded to 128 bits


ROTATIONS = (1, -1, 3)


@functools.lru_cache(maxsize=None)
def ckks_rotation_case(name, setting, k):
    """Rotate by k (k = None: Conjugate) over the restated evaluator: (m, ct, g, out)"""
    N, Q, P, levels = chain(name)
    g = 2 * N - 1 if k is None else cr.galois_element(N, k)
    m, ct, out = auto_case(name, setting, levels[0], g)
    return m, ct, g, out


@pytest.mark.parametrize("shape", CKKS_SHAPES, ids=_ids)
def test_ckks_rotate_conjugate_decrypt(oracle, shape):
    """Rotate / Conjugate / RotateHoisted (schemes/ckks/evaluator.go:1195-1255) are Automorphism(Hoisted) of 5^k or 2N - 1 with real Galois keys"""
    name, setting = shape
    N, Q, P, levels = chain(name)
    level = levels[0]
    for k in ROTATIONS + (None,):
        m, ct, g, out = ckks_rotation_case(name, setting, k)
        if k is not None:
            assert g == pow(5, k, 2 * N)
        got = auto_error(name, level, out, m, g)
        report("ckks/rotate", name, setting, level, got, bound(N, 0, level))
        assert got <= bound(N, 0, level)
    # by k, then by -k: the message again, two key switches' worth of error (twice the bound on the standard deviation: one bit)
    m, ct, g, out = ckks_rotation_case(name, setting, 1)
    ginv = cr.galois_element(N, -1)
    assert g * ginv % (2 * N) == 1
    back = rr.automorphism(N, Q, P[:setting[1]], out, key(name, setting, "galois", ginv), ginv)
    got = auto_error(name, level, back, m, 1)
    report("ckks/rot+back", name, setting, level, got, bound(N, 0, level) + 1)
    assert got <= bound(N, 0, level) + 1


# ---- negative controls: the misreadings the bound must catch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [("REF", (0, 2)), ("REF", (16, 1)), ("REF", (2, 0)), ("TAIL", (0, 4))], ids=_ids)
def test_control_swapped_key_rows_decrypt_to_noise(oracle, shape):
    name, setting = shape
    N, Q, P, levels = chain(name)
    k = key(name, setting, "switch")
    level = levels[0]
    a, _ = switch_case(name, setting, level)
    rows = list(range(k.Q.shape[0]))
    i, j = (0, 1) if not setting[0] else (1, k.digits_per_limb[0] + 1)   # two RNS digits; under pw2, the same power of two limbs
    rows[i], rows[j] = rows[j], rows[i]
    bad = rr.GadgetKey(k.Q[rows], k.P[rows] if k.P is not None else None, k.levelQ, k.levelP, k.pw2, k.digits_per_limb)
    got = switch_error(name, setting, level, a, rr.gadget_product(N, Q, P[:setting[1]], level, a, bad))
    assert got > bound(N, setting[0]) + 10
    if setting[0]:                                                       # the order WITHIN a limb: powers j and j + 1 exchanged
        rows = list(range(k.Q.shape[0]))
        rows[0], rows[1] = rows[1], rows[0]
        bad = rr.GadgetKey(k.Q[rows], k.P[rows] if k.P is not None else None, k.levelQ, k.levelP, k.pw2, k.digits_per_limb)
        got = switch_error(name, setting, level, a, rr.gadget_product(N, Q, P[:setting[1]], level, a, bad))
        assert got > bound(N, setting[0]) + 10


@pytest.mark.parametrize("shape", [("REF", (0, 2)), ("TAIL", (0, 4))], ids=_ids)
def test_control_galois_key_with_the_inverse_map_decrypts_to_noise(oracle, shape):
    name, setting = shape
    N, Q, P, levels = chain(name)
    level, g = levels[0], 5
    ginv = pow(g, -1, 2 * N)
    m, ct, _ = fresh(name, "auto", level)
    out = rr.automorphism(N, Q, P[:setting[1]], ct, key(name, setting, "galois", g), g, map_g=ginv)
    for h in (g, ginv):
        assert auto_error(name, level, out, m, h) > bound(N, 0, level) + 10


@pytest.mark.parametrize("shape", [("RGSW", (0, 2)), ("REF", (16, 1))], ids=_ids)
def test_control_swapped_rgsw_halves_do_not_decrypt(oracle, shape):
    name, setting = shape
    N, Q, P, levels = chain(name)
    ct, _ = rgsw_case(name, setting, 3, N - 2)
    value = rgsw(name, setting, 3)
    got, ph = decrypt_monomial(name, external_product(name, setting, ct, value[::-1]))
    mono = [0] * N
    mono[N - 2] = 1
    want = rr.monomial_mul(mono, 3)
    assert got != want
    err = rr.centered_diff(ph, [int(Q[0]) * x for x in want], rr.prod(Q[:levels[0] + 1]))
    assert rr.log2_std(err) > 10 + 10                                    # the reference's RGSW noise bound is 10 bits (rgsw_test.go:30)

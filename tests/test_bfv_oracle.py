"""CPU: the restatement of the reference's scale-invariant (BFV) multiply (tests/bfv_restatement.py, schemes/bgv/evaluator.go:975-1124)
pinned to ground truth that does not depend on how it is composed: decryption with exact big integers, the quantize stage against
big-integer rounding, levelQMul against its formula and the scale function against Python ints.  The GPU tests compare the device path
with this restatement bit for bit."""
import random

import numpy as np
import pytest

import bfv_restatement as br
from oracle import primes

T = 65537


def chain(logN, logQ):
    """Q and QMul from ONE GenModuli call (so they never share a prime): bgv/params.go:98-108 sizes QMul from Q's bit length, which is known
    to within a bit per prime before the primes are drawn, so the count is fixed up after the first draw"""
    nb = -(-(sum(logQ) + len(logQ) + logN) // 61)
    Q, M = primes.gen_moduli(logN + 1, logQ, [61] * nb)
    return Q, M[:br.nb_qi_mul(Q, logN)]


@pytest.fixture(scope="module")
def rh():
    import matrix_fhe_lattigo_amd as m          # every test here rests on the feature being present
    assert hasattr(m, "bgv") and hasattr(m.lib(), "rh_bfv_create")
    return m


def test_level_qmul_formula(rh):
    # (:51-56): the restatement's levelQMul at every level of the chains the GPU tests use (the library's table is read back there: an
    # rh_bfv handle needs a device)
    for logN, logQ in ((5, [61, 61]), (10, [55, 45, 45]), (10, [45] * 9), (12, [55, 45, 45]), (15, [61, 61])):
        Q, M = chain(logN, logQ)
        want = br.level_qmul(Q, logN)
        acc = 1
        for i, q in enumerate(Q):
            acc *= q
            bits = len(bin(acc)) - 2
            assert want[i] == (bits + logN + 60) // 61 - 1
        assert len(M) == want[-1] + 1 == br.nb_qi_mul(Q, logN)
    assert br.level_qmul(chain(10, [55, 45, 45])[0], 10) == [1, 1, 2]        # level 0 of the 3-limb chain differs from the top
    assert br.level_qmul(chain(10, [45] * 9)[0], 10)[-1] == 6               # nine 45-bit primes: 7 limbs of QMul
    assert br.level_qmul(chain(5, [61, 61])[0], 5) == [1, 2]


def test_scale_function_against_python_ints(rh):
    rnd = random.Random(5)
    Q, _ = chain(10, [55, 45, 45])
    for level in range(3):
        Qb = br.prod(Q[:level + 1])
        for _ in range(20):
            a, b = rnd.randrange(1, T), rnd.randrange(1, T)
            c = rh.bgv.MulScaleInvariant(T, Qb, a, b)
            assert 0 <= c < T and c == br.scale_invariant(T, Qb, a, b)
            assert (c * (T - Qb % T) - a * b) % T == 0                       # c = a b / (T - Q mod T) modulo T
    assert rh.bgv.MulScaleInvariant(T, Qb, 1, 1) == pow(-Qb, -1, T)
    with pytest.raises(rh.RingHipError):
        rh.bgv.MulScaleInvariant(15, 5 * 7, 1, 1)                           # T - Q mod T = 10 shares a factor with T = 15


@pytest.mark.parametrize("logN,logQ,level", [(5, [55, 45, 45], 2), (10, [55, 45, 45], 2), (10, [55, 45, 45], 0), (5, [61, 61], 1), (10, [45] * 9, 8)])
def test_quantize_is_exact_rounding_then_centred_lift(rh, logN, logQ, level):
    """quantize (:1104-1124) against big integers.  The input is x modulo Q * QMul.  ModDownQPtoP subtracts the CENTRED residue
    xc = ((x + floor(Q/2)) mod Q) - floor(Q/2) and divides exactly, so y = (x - xc) / Q is x / Q rounded to the NEAREST integer (Q is odd: no
    ties), known modulo P = prod(QMul).  ModUpPtoQ lifts the centred representative yc = ((y + floor(P/2)) mod P) - floor(P/2), and the
    output is T * yc modulo Q -- on every coefficient, for inputs whose float sums in reconstructRNS are not within rounding error of an
    integer (|xc| not within Q * 2^-40 of Q/2 and |y| not within P * 2^-40 of P/2, where the reference itself is off by Q or P:
    tests/test_oracle_bext.py; the random inputs here are not, the hand-picked ones sit at xc = 0, +-1)."""
    N = 1 << logN
    Q, M = chain(logN, logQ)
    P = br.Params(N, Q, M, T)
    Ql, Ml, srQ, srM = P.at(level)
    Qb, Pb = br.prod(Ql), br.prod(Ml)
    rnd = random.Random(logN * 100 + level)
    bound = Qb * (Pb >> 1)                                                   # |x / Q| stays below P / 2
    xs = [0, 1, -1, Qb, -Qb, Qb + 1, -Qb - 1, 5 * Qb - 1, T * Qb, (bound // 3 // Qb) * Qb, -(bound // 3 // Qb) * Qb + 1]
    xs += [rnd.randrange(-bound + Qb, bound - Qb) for _ in range(N - len(xs))]
    out = br.quantize(P, level, br.ntt(br.rns(xs, Ql), srQ), br.ntt(br.rns(xs, Ml), srM))
    got = br.crt(br.intt(out, srQ), Ql)
    for x, g in zip(xs, got):
        xc = ((x + (Qb >> 1)) % Qb) - (Qb >> 1)
        y = (x - xc) // Qb
        assert (x - xc) % Qb == 0 and abs(2 * (x - y * Qb)) < Qb               # nearest
        yc = ((y + (Pb >> 1)) % Pb) - (Pb >> 1)
        assert yc == y
        assert g == (T * yc) % Qb


def _messages(rnd, N):
    return [rnd.randrange(T) for _ in range(N)], [rnd.randrange(T) for _ in range(N)]


@pytest.mark.parametrize("logN", [5, 10])
@pytest.mark.parametrize("square", [False, True])
def test_decryption_of_the_product(rh, logN, square):
    """Ground truth that never looks at RNS: with phases m_i T^-1 + e_i (mod Q), scales 1, d = T (c0 + c1 s + c2 s^2) centred modulo Q
    satisfies (d mod t) (T - Q mod T) = m0 * m1 (mod X^N + 1, t) on EVERY coefficient."""
    N = 1 << logN
    Q, M = chain(logN, [55, 45, 45])
    P = br.Params(N, Q, M, T)
    level = 2
    rnd = random.Random(77 + logN)
    s = [rnd.randrange(-1, 2) for _ in range(N)]
    m0, m1 = _messages(rnd, N)
    ct0 = br.encrypt(rnd, P, level, m0, s)
    ct1 = ct0 if square else br.encrypt(rnd, P, level, m1, s)
    if square:
        m1 = m0
    c = br.tensor_scale_invariant(P, level, ct0, ct1)
    d = br.decrypt_product(P, level, c, s)
    Qb = br.prod(Q)
    f = T - Qb % T
    want = br.negacyclic_mul_mod_t(m0, m1, T)
    assert [(x * f) % T for x in d] == want
    assert rh.bgv.MulScaleInvariant(T, Qb, 1, 1) * f % T == 1               # the scale the evaluator records undoes exactly that factor


def test_tensor_c1_is_the_unreduced_sum(rh):
    # tensorLowDeg (:1094-1095, :1082-1083): c1 = MRed + MRed is left in [0, 2q); with every operand q - 1 both terms are (q-1)^2 2^-64 ... mod q
    N = 32
    Q, _ = chain(5, [55, 45, 45])
    a = [np.stack([np.full(N, q - 1, dtype=np.uint64) for q in Q]) for _ in range(2)]
    for ct1 in (a, None):
        c = br.tensor_low_deg(Q, a, ct1)
        for i, q in enumerate(Q):
            one = (q - 1) * (q - 1) % q                                      # = 1: MRed(MForm(q-1), q-1) = (q-1)^2 mod q
            assert np.all(c[0][i] == one) and np.all(c[2][i] == one) and np.all(c[1][i] == 2 * one)
    rng = np.random.default_rng(1)
    u = [np.stack([rng.integers(0, q, size=N, dtype=np.uint64) for q in Q]) for _ in range(4)]
    c = br.tensor_low_deg(Q, u[:2], u[2:])
    for i, q in enumerate(Q):
        t0 = [int(x) * int(y) % q for x, y in zip(u[0][i], u[3][i])]
        t1 = [int(x) * int(y) % q for x, y in zip(u[1][i], u[2][i])]
        assert [int(x) for x in c[1][i]] == [x + y for x, y in zip(t0, t1)]   # the plain sum, values >= q included
        assert any(x + y >= q for x, y in zip(t0, t1))

"""CPU: the restatement of the reference's BGV evaluator paths (tests/bgv_restatement.py, schemes/bgv/evaluator.go:173-751, :1142-1445,
:1593-1659) pinned to ground truth that does not depend on how it is composed: every tensor / accumulate limb against Python big integers,
matchScalesBinary against its defining properties, and mul -> relin -> rescale -> decrypt with a real key against the negacyclic product of
the messages times the tracked scale.  The GPU tests compare the device path with this restatement bit for bit."""
import math
import random

import numpy as np
import pytest

import bfv_restatement as br
import bgv_restatement as gr
import rlwe_restatement as rr
from oracle import primes

T = 65537


@pytest.fixture(scope="module")
def rh():
    import matrix_fhe_lattigo_amd as m          # every test here rests on the feature being present
    assert hasattr(m.lib(), "rh_bgv_tensor") and hasattr(m.bgv.Evaluator, "Mul") and hasattr(m.bgv, "matchScalesBinary")
    return m


def _uniform(rng, mods, N):
    return np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in mods])


def _ints(x):
    return [[int(v) for v in row] for row in x]


@pytest.mark.parametrize("logQ", [[61, 61], [55, 45, 45]])
def test_tensor_and_accumulate_limbs_against_python_ints(rh, logQ):
    """(a) every output limb of tensorStandard is T (...) mod q_i and of mulRelinThenAdd T r0 (...) + r1 acc mod q_i, in Python ints"""
    N = 32
    Q, _ = primes.gen_moduli(6, logQ, [61])
    rng = np.random.default_rng(len(logQ))
    a0, a1, b0, b1, z0, z1, z2, pt = (_uniform(rng, Q, N) for _ in range(8))
    for i, q in enumerate(Q):                                        # coefficient 0: both cross terms q - 1 and the accumulator q - 1
        a0[i, 0] = a1[i, 0] = 1
        b0[i, 0] = b1[i, 0] = z0[i, 0] = z1[i, 0] = z2[i, 0] = q - 1
    A0, A1, B0, B1, Z0, Z1, Z2, PT = (_ints(x) for x in (a0, a1, b0, b1, z0, z1, z2, pt))
    s0, s1 = 3, 5
    for square in (False, True):
        y0, y1, Y0, Y1 = (a0, a1, A0, A1) if square else (b0, b1, B0, B1)
        c, sc = gr.tensor_standard(Q, T, [a0, a1], s0, [y0, y1], s1 if not square else s0, square)
        assert sc == (s0 * s0 if square else s0 * s1) % T
        for i, q in enumerate(Q):
            assert _ints(c[0])[i] == [T * x * y % q for x, y in zip(A0[i], Y0[i])]
            assert _ints(c[1])[i] == [T * (x0 * w1 + x1 * w0) % q for x0, x1, w0, w1 in zip(A0[i], A1[i], Y0[i], Y1[i])]
            assert _ints(c[2])[i] == [T * x * y % q for x, y in zip(A1[i], Y1[i])]
    for d in (1, 2):                                                 # plaintext x degree-1 and x degree-2
        ct = [a0, a1, b0][:d + 1]
        c, sc = gr.tensor_standard(Q, T, ct, s0, [pt], s1)
        for j in range(d + 1):
            for i, q in enumerate(Q):
                assert _ints(c[j])[i] == [T * int(x) * p % q for x, p in zip(ct[j][i], PT[i])]
    # accumulate: scales that match (r0 = r1 = 1) and scales that do not
    for sout in (s0 * s1 % T, 7):
        r0, r1 = (1, 1) if sout == s0 * s1 % T else gr.match_scales_binary(T, s0 * s1 % T, sout)[:2]
        assert (r0, r1) == (1, 1) or (r0 != 1 and r1 != 1)
        for relin in (False, True):
            out, sc, c2 = gr.mul_relin_then_add(Q, T, [a0, a1], s0, [b0, b1], s1, [z0, z1, z2][:2 if relin else 3], sout, relin)
            assert sc == sout * r1 % T == s0 * s1 * r0 % T
            for i, q in enumerate(Q):
                assert _ints(out[0])[i] == [(T * r0 * x * y + r1 * z) % q for x, y, z in zip(A0[i], B0[i], Z0[i])]
                assert _ints(out[1])[i] == [(T * r0 * (x0 * y1 + x1 * y0) + r1 * z) % q
                                            for x0, x1, y0, y1, z in zip(A0[i], A1[i], B0[i], B1[i], Z1[i])]
                if relin:
                    assert _ints(c2)[i] == [T * r0 * x * y % q for x, y in zip(A1[i], B1[i])]
                else:
                    assert _ints(out[2])[i] == [(T * r0 * x * y + r1 * z) % q for x, y, z in zip(A1[i], B1[i], Z2[i])]
        out, sc, _ = gr.mul_relin_then_add(Q, T, [a0, a1, b0], s0, [pt], s1, [z0, z1, z2], sout, False)
        for j, (X, Z) in enumerate(((A0, Z0), (A1, Z1), (B0, Z2))):
            for i, q in enumerate(Q):
                assert _ints(out[j])[i] == [(T * r0 * x * p + r1 * z) % q for x, p, z in zip(X[i], PT[i], Z[i])]
    # Add / Sub with different scales and degrees 1 + 2: r0 a +- r1 b, r0 a alone where b has no component, +- r1 b where a has none
    for sub in (False, True):
        sg = -1 if sub else 1
        for x, y in (([a0, a1], [b0, b1, z2]), ([b0, b1, z2], [a0, a1])):
            r0, r1, _ = gr.match_scales_binary(T, s0, s1)
            out, sc = gr.add_sub(Q, T, x, s0, y, s1, sub)
            assert sc == s0 * r0 % T == s1 * r1 % T and len(out) == 3
            for j in range(3):
                for i, q in enumerate(Q):
                    xa = _ints(x[j])[i] if j < len(x) else [0] * N
                    yb = _ints(y[j])[i] if j < len(y) else [0] * N
                    assert _ints(out[j])[i] == [(r0 * u + sg * r1 * v) % q for u, v in zip(xa, yb)]


def _msb_properties(rh, t, s0, s1):
    r0, r1, e = gr.match_scales_binary(t, s0, s1)
    assert (r0, r1, e) == rh.bgv.matchScalesBinary(t, s0, s1)                        # the evaluator's own copy
    assert r0 * s0 % t == r1 * s1 % t and math.gcd(r0, t) == 1 and 0 < r0 < t and 0 < r1 < t
    half = t >> 1
    cost = gr.center(r0, half, t) + gr.center(r1, half, t)
    start = gr.center(pow(s0, -1, t) * s1 % t, half, t) + 1                          # the pair (s0^-1 s1, 1)
    assert cost <= start and e == min(cost, start)


def test_match_scales_binary_properties(rh):
    """(b) r0 s0 = r1 s1 (mod t), gcd(r0, t) = 1, and a cost no larger than that of the starting pair (s0^-1 s1 mod t, 1)"""
    rnd = random.Random(11)
    for _ in range(300):
        _msb_properties(rh, T, rnd.randrange(1, T), rnd.randrange(1, T))
    for t in (97,):                                                                 # exhaustively at a small prime
        for s0 in range(1, t):
            for s1 in range(1, t):
                _msb_properties(rh, t, s0, s1)
    assert gr.match_scales_binary(T, 5, 5)[:2] == (1, 1)
    with pytest.raises(rh.RingHipError, match="gcd"):
        rh.bgv.matchScalesBinary(15, 5, 1)


@pytest.fixture(scope="module")
def world():
    """N = 32, two 61-bit limbs of Q, one of P, a ternary secret and a real relinearisation key"""
    N = 32
    Q, Pk = primes.gen_moduli(6, [61, 61], [61])
    rnd = random.Random(2025)
    s = [rnd.randrange(-1, 2) for _ in range(N)]
    rlk = rr.relin_key(rnd, rr.Secret(N, s), Q, Pk, len(Q) - 1, 0)     # the one key generator (tests/rlwe_restatement.py), one P modulus
    evkQ, evkP = rlk.Q, rlk.P
    return N, Q, Pk, s, evkQ, evkP, rnd


def _relin(N, Q, Pk, level, c, evkQ, evkP):
    return br.relinearize(N, Q, Pk, level, c, evkQ, evkP)


def test_mul_relin_rescale_decrypts_to_the_product(rh, world):
    """(c) Mul -> relin with a real key -> Rescale -> decrypt = negacyclic product times the tracked scale, on every coefficient"""
    N, Q, Pk, s, evkQ, evkP, rnd = world
    m0, m1 = [rnd.randrange(T) for _ in range(N)], [rnd.randrange(T) for _ in range(N)]
    for square in (False, True):
        ct0 = gr.encrypt(rnd, N, Q, T, m0, s, 3)
        ct1 = ct0 if square else gr.encrypt(rnd, N, Q, T, m1, s, 5)
        ma, mb, sa, sb = (m0, m0, 3, 3) if square else (m0, m1, 3, 5)
        assert gr.decrypt(N, Q, T, ct0, s) == [x * 3 % T for x in m0]                 # decryption returns message * scale
        c, sc = gr.tensor_standard(Q, T, ct0, sa, ct1, sb, square)
        want = br.negacyclic_mul_mod_t(ma, mb, T)
        assert sc == sa * sb % T and gr.decrypt(N, Q, T, c, s) == [x * sc % T for x in want]      # degree 2, before relinearisation
        lin = _relin(N, Q, Pk, 1, c, evkQ, evkP)
        assert gr.decrypt(N, Q, T, lin, s) == [x * sc % T for x in want]
        low, sc2 = gr.rescale(N, Q, T, lin, sc)
        assert sc2 == sc * pow(Q[1], -1, T) % T and low[0].shape == (1, N)
        assert gr.decrypt(N, Q[:1], T, low, s) == [x * sc2 % T for x in want]


def test_mul_relin_then_add_into_an_accumulator_of_another_scale(rh, world):
    N, Q, Pk, s, evkQ, evkP, rnd = world
    m0, m1, m2 = ([rnd.randrange(T) for _ in range(N)] for _ in range(3))
    ct0, ct1 = gr.encrypt(rnd, N, Q, T, m0, s, 3), gr.encrypt(rnd, N, Q, T, m1, s, 5)
    acc = gr.encrypt(rnd, N, Q, T, m2, s, 7)                                         # 7 != 3 * 5
    out, sc, c2 = gr.mul_relin_then_add(Q, T, ct0, 3, ct1, 5, acc, 7, True)
    r0, r1, _ = gr.match_scales_binary(T, 15, 7)
    assert r0 != 1 and sc == 7 * r1 % T == 15 * r0 % T
    lin = _relin(N, Q, Pk, 1, out + [c2], evkQ, evkP)
    want = [(x + y) * sc % T for x, y in zip(br.negacyclic_mul_mod_t(m0, m1, T), m2)]
    assert gr.decrypt(N, Q, T, lin, s) == want
    low, sc2 = gr.rescale(N, Q, T, lin, sc)
    assert gr.decrypt(N, Q[:1], T, low, s) == [(x + y) * sc2 % T for x, y in zip(br.negacyclic_mul_mod_t(m0, m1, T), m2)]
    # without relinearisation, into a degree-2 accumulator (itself a product)
    acc2, sacc = gr.tensor_standard(Q, T, ct1, 5, acc, 7)
    out, sc, none = gr.mul_relin_then_add(Q, T, ct0, 3, ct1, 5, acc2, sacc, False)
    assert none is None and sc == sacc * gr.match_scales_binary(T, 15, sacc)[1] % T
    want = [(x + y) * sc % T for x, y in zip(br.negacyclic_mul_mod_t(m0, m1, T), br.negacyclic_mul_mod_t(m1, m2, T))]
    assert gr.decrypt(N, Q, T, out, s) == want


def test_add_sub_scalars_and_scale_matching_decrypt(rh, world):
    N, Q, Pk, s, evkQ, evkP, rnd = world
    m0, m1 = [rnd.randrange(T) for _ in range(N)], [rnd.randrange(T) for _ in range(N)]
    ct0, ct1 = gr.encrypt(rnd, N, Q, T, m0, s, 3), gr.encrypt(rnd, N, Q, T, m1, s, 5)
    for sub in (False, True):
        out, sc = gr.add_sub(Q, T, ct0, 3, ct1, 5, sub)                                # different scales
        assert sc == 3 * gr.match_scales_binary(T, 3, 5)[0] % T
        assert gr.decrypt(N, Q, T, out, s) == [(x - y if sub else x + y) * sc % T for x, y in zip(m0, m1)]
        same = gr.encrypt(rnd, N, Q, T, m1, s, 3)
        out, sc = gr.add_sub(Q, T, ct0, 3, same, 3, sub)                               # equal scales: plain Add / Sub
        assert sc == 3 and gr.decrypt(N, Q, T, out, s) == [(x - y if sub else x + y) * 3 % T for x, y in zip(m0, m1)]
    a, sa, b, sb = gr.match_scales_and_level(Q, T, ct0, 3, ct1, 5)
    assert sa == sb and gr.decrypt(N, Q, T, a, s) == [x * sa % T for x in m0] and gr.decrypt(N, Q, T, b, s) == [x * sb % T for x in m1]
    for v in (5, T - 2, T // 2 + 1):                                                  # int scalars, positive and above T/2
        out, sc = gr.add_scalar(Q, T, ct0, 3, v)
        assert sc == 3 and gr.decrypt(N, Q, T, out, s) == [((m0[0] + v) if j == 0 else m0[j]) * 3 % T for j in range(N)]
        out, sc = gr.mul_scalar_int(Q, T, ct0, 3, v)
        assert sc == 3 and gr.decrypt(N, Q, T, out, s) == [x * v * 3 % T for x in m0]


def test_host_side_scalars_of_the_evaluator(rh):
    """the constants bgv.Evaluator hands the kernels, without a device: the class is not instantiated, its helpers are read as functions"""
    Q, _ = primes.gen_moduli(6, [61, 61], [61])

    class Shim:
        t = T
        ringQ = type("R", (), {"moduli": np.array(Q, dtype=np.uint64)})()
        _qs = rh.bgv.Evaluator._qs
    sh = Shim()
    assert list(rh.bgv.Evaluator._k(sh, 1)) == gr.t_montgomery(T, Q)
    assert list(rh.bgv.Evaluator._k(sh, 1, 9)) == [(T * 9 << 128) % q for q in Q]
    assert list(rh.bgv.Evaluator._mont(sh, 0, 7)) == gr.mform(7, Q[:1])
    assert rh.bgv.Evaluator._center_t(sh, T - 2) == -2 == gr.center_t(T - 2, T) and rh.bgv.Evaluator._center_t(sh, 5) == 5


def test_null_handles_are_argument_errors(rh):
    L = rh.lib()
    for call, who in ((lambda: L.rh_bgv_tensor(None, 0, *[None] * 7, 1, None, None, 0), b"rh_bgv_tensor"),
                      (lambda: L.rh_bgv_mul_plain(None, 0, *[None] * 7, 1, None, None, 0), b"rh_bgv_mul_plain"),
                      (lambda: L.rh_bgv_axpby(None, 0, None, None, None, 1, None, None, 0), b"rh_bgv_axpby")):
        assert call() == -1 and L.rh_last_error() == who + b": null ring handle"

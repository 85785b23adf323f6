"""CPU: pins tests/matrix_ckks_restatement.py to decryption in the reference's own set-up (schemes/matrix_ckks/matrix_ckks_test.go):
N = 24 (Order2 3, Order3 1), LogQ {55, 45 x 6}, LogP {60}, scale 2^45, Xs = Xe = ring.Ternary{H: 1}, tolerance 0.1 (:63).

The five reference tests with explicit samples (encrypt / decrypt, Add, MulByConst with a real constant, several constants, integer constants;
every constant of the reference's tests is an integer, so MulByConst takes its unscaled branch, evaluator.go:344-347), and a sixth the
reference lacks: Mul of two encryptions, MForm of the three components (Mul leaves 2^-64), NTT, Rescale, degree-2 decryption, Decode at
scale^2 / q_L, against the naive product of the value vectors in Z[X]/(X^N - X^(N/2) + 1).  The encoder's unit cases are stated on Python
integers, independently of the restatement's own arithmetic."""
import random

import numpy as np
import pytest

import matrix_ckks_restatement as mr
import rlwe_restatement as rr
from oracle import primes
from oracle import ring_oracle as orc

N, LOGQ, LOGP, SCALE, TOL = 24, [55] + [45] * 6, [60], float(1 << 45), 0.1
_CACHE = {}


def setup():
    """(Q, P, omegas, samples): the chain and one fixed set of samples, made once"""
    if not _CACHE:
        Q, P = primes.gen_moduli_3n(N, LOGQ, LOGP)
        om = {int(q): mr.omega_for(q, N) for q in list(Q) + list(P)}
        rnd = random.Random(20240611)

        def one_hot():                                                    # ring.Ternary{H: 1}: one coefficient of random sign
            out = [0] * N
            out[rnd.randrange(N)] = rnd.choice((-1, 1))
            return out
        key_mods = list(Q) + list(P)                                      # the relinearisation key lives on the whole of QP, one P
        s = dict(sk=one_hot(), e=[one_hot() for _ in range(4)], c1=[rr.uniform_poly(rnd, N, Q) for _ in range(4)],
                 rlk_a=np.stack([rr.uniform_poly(rnd, N, key_mods) for _ in range(7)]), rlk_e=[one_hot() for _ in range(7)])
        _CACHE.update(Q=[int(q) for q in Q], P=[int(p) for p in P], om=om, s=s)
    return _CACHE["Q"], _CACHE["P"], _CACHE["om"], _CACHE["s"]


def encrypt(values, which, level=6):
    """Encode (coefficient domain) and encrypt under the secret key with sample set `which`"""
    Q, P, om, s = setup()
    mods = Q[:level + 1]
    pt = mr.encode(values, SCALE, mods, N)
    with mr.ring3n(om) as kr:
        sk = kr.secret(s["sk"])
        return kr.encrypt_sk(sk, Q, level, s["c1"][which][:level + 1], s["e"][which], pt, is_ntt=False), sk


def decrypt_decode(ct, sk, scale, nvals, is_ntt=False):
    Q, P, om, s = setup()
    with mr.ring3n(om) as kr:
        pt = kr.decrypt(ct, sk, Q, is_ntt=is_ntt)
        if is_ntt:
            pt = rr.intt(pt, N, Q[:pt.shape[0]])
    return mr.decode(pt[0], Q[0], scale, nvals)


def test_encrypt_decrypt():
    vals = [1.0 + 0j, 2.0 + 0j, 3.0 + 0j, 4.0 + 0j]
    ct, sk = encrypt(vals, 0)
    got = decrypt_decode(ct, sk, SCALE, 4)
    assert np.all(np.abs(got - np.array([v.real for v in vals])) <= TOL), got


def test_addition():
    Q = setup()[0]
    v1, v2 = [1.0, 2.0, 3.0, 4.0], [5.0, 6.0, 7.0, 8.0]
    (a, sk), (b, _) = encrypt(v1, 0), encrypt(v2, 1)
    ct = [rr._vec("ADD", x, y, Q) for x, y in zip(a, b)]
    got = decrypt_decode(ct, sk, SCALE, 4)
    assert np.all(np.abs(got - (np.array(v1) + np.array(v2))) <= TOL), got


@pytest.mark.parametrize("vals,consts", [([1.0, 2.0, 3.0, 4.0], [2.0]), ([1.0, 2.0, 3.0], [2.0, 3.0, 4.0]), ([1.0, 2.0, 3.0, 4.0], [2, 3, 4])],
                         ids=["real", "several", "integer"])
def test_mul_by_const(vals, consts):
    Q = setup()[0]
    ct, sk = encrypt(vals, 2)
    for c in consts:
        assert float(c) == int(c)                                        # IsInt: no scaling (evaluator.go:344-347)
        out = [np.stack([(x[i].astype(object) * int(c) % q).astype(np.uint64) for i, q in enumerate(Q)]) for x in ct]
        got = decrypt_decode(out, sk, SCALE, len(vals))
        assert np.all(np.abs(got - np.array(vals) * float(c)) <= TOL), (c, got)


def mul_rescale(ct0, ct1, level=6):
    """MatrixCKKSEvaluator.Mul (evaluator.go:114-192: NTT, the four MulCoeffsMontgomery without MForm, INTT), then MForm, NTT and
    DivRoundByLastModulusManyNTT once: a degree-2 ciphertext at level - 1 in the NTT domain"""
    Q = setup()[0]
    mods = Q[:level + 1]
    a, b = [rr.ntt(x, N, mods) for x in ct0], [rr.ntt(x, N, mods) for x in ct1]
    mm = lambda x, y: rr._vec("MUL_MONT", x, y, mods)
    o = [mm(a[0], b[0]), rr._vec("ADD", mm(a[0], b[1]), mm(a[1], b[0]), mods), mm(a[1], b[1])]
    o = [rr.intt(x, N, mods) for x in o]                                  # what Mul returns
    o = [rr._vec("MFORM", x, None, mods) for x in o]
    o = [orc.div_by_last_modulus_many(x, mods, 1, True) for x in o]       # the NTT-domain form divides the same coefficients
    return [rr.ntt(x, N, mods[:-1]) for x in o]


def test_mul_is_pinned_to_decryption():
    Q, P, om, s = setup()
    v1, v2 = [1, 2, 3, 4], [5, 6, 7, 8]
    want = np.array(mr.naive_mul(v1 + [0] * (N - 4), v2 + [0] * (N - 4)), dtype=np.float64)
    (a, sk), (b, _) = encrypt([float(x) for x in v1], 0), encrypt([float(x) for x in v2], 1)
    scale = SCALE * SCALE / float(Q[6])
    with mr.ring3n(om) as kr:
        ct = mul_rescale(a, b)
    got = decrypt_decode(ct, sk, scale, N, is_ntt=True)
    assert np.all(np.abs(got - want) <= TOL), np.abs(got - want).max()
    with mr.ring3n(om) as kr:                                             # ... and after Relinearize with a restated key, degree 1
        rlk = kr.relin_key(sk, Q, P, 6, 0, 0, s["rlk_a"], s["rlk_e"])
        d = relinearize(ct, rlk, Q[:6], P)
    got = decrypt_decode(d, sk, scale, N, is_ntt=True)
    assert np.all(np.abs(got - want) <= TOL), np.abs(got - want).max()


def relinearize(ct, rlk, mods, P):
    """rlwe.Evaluator.Relinearize (core/rlwe/evaluator.go:125-153) on a 3N ring, single P: the formulas of oracle.compose.gadget_product_single_p
    with the transforms of the block it is called in (ring3n): the digits of c2, one per limb of Q, by DecomposeAndSplit, times the key rows,
    summed, divided by P, plus (c0, c1)"""
    mp = [int(p) for p in P[:1]]
    allm = list(mods) + mp
    c2 = rr.intt(ct[2], N, mods)
    acc = [np.zeros((len(allm), N), dtype=np.uint64) for _ in range(2)]
    for i, qi in enumerate(mods):
        dq, dp = orc.decompose_and_split(len(mods) - 1, 0, 1, i, c2, list(mods), mp)      # the limb, centred, under every modulus (DecomposeAndSplit)
        digit = rr.ntt(np.concatenate([dq, dp]), N, allm)
        for c in (0, 1):
            key = np.concatenate([rlk.Q[i, c][:len(mods)], rlk.P[i, c]])      # the key's leading limbs: it is used below its own level
            acc[c] = rr._vec("ADD", acc[c], rr._vec("MUL_MONT", digit, key, allm), allm)
    out = []
    for c in (0, 1):
        x = rr.intt(acc[c], N, allm)
        x = orc.moddown_qp_to_q(x[:len(mods)], x[len(mods):], list(mods), mp)
        out.append(rr._vec("ADD", rr.ntt(x, N, list(mods)), ct[c], list(mods)))
    return out


# ---- the encoder's unit cases, on Python integers -----------------------------------------------------------------------------------------------------
def test_encoder_unit_cases():
    Q = setup()[0]
    q = Q[1]                                                              # a 45-bit limb: products in [q, 2q) and [2q, 2^64) exist at scale 2^45
    two64 = 1 << 64
    cases = [
        (0.0, SCALE, 0, 0),                                               # zero
        (1.0 - 2.0 ** -53, SCALE, (1 << 45) - 1, (1 << 45) - 1),           # truncation: 0.999.. * scale is 2^45 - 2^-8, not rounded up
        (float(q + 5) / SCALE, SCALE, None, None),                        # a product in [q, 2q)
        (float(3 * q + 7) / SCALE, SCALE, None, None),                    # a product in [2q, 2^64)
        (3.0 * 2.0 ** 30, SCALE, (3 << 75) & (two64 - 1), None),          # a product >= 2^64: the low 64 bits (0 here: 3 * 2^75)
        (float((1 << 52) + 1) * 2.0 ** 13, 1.0, (((1 << 52) + 1) << 13) & (two64 - 1), None),   # ... with low bits that survive (2^13)
    ]
    for v, sc, word, _ in cases:
        prod = v * sc
        w, signed = mr.reference_word(v, sc)
        if word is None:
            word = int(prod)
        assert w == word, (v, w, word)
        got = mr.encode([v], sc, Q, N)
        assert [int(x) for x in got[:, 0]] == [word % m for m in Q]
        assert not got[:, 1:].any()
    p1, p2 = int(float(q + 5) / SCALE * SCALE), int(float(3 * q + 7) / SCALE * SCALE)
    assert q <= p1 < 2 * q and 2 * q <= p2 < two64
    assert mr.reference_stored(float(3 * q + 7) / SCALE, SCALE, q) >= q     # the reference's single CRed leaves it above q; the device word is canonical
    # a negative value in both forms
    neg = mr.encode([-3.0], SCALE, Q, N, "as_written")
    sgn = mr.encode([-3.0], SCALE, Q, N, "signed")
    c = 3 << 45
    assert [int(x) for x in neg[:, 0]] == [(two64 - c) % m for m in Q]
    assert [int(x) for x in sgn[:, 0]] == [m - c % m for m in Q]
    assert mr.decode(sgn[0], Q[0], SCALE, 1)[0] == -3.0 and mr.decode(neg[0], Q[0], SCALE, 1)[0] != -3.0
    big = mr.encode([-3.0 * 2.0 ** 30], SCALE, Q, N, "signed")
    assert [int(x) for x in big[:, 0]] == [(-(3 << 75)) % m for m in Q]
    # a uint64 above 2^53 goes through float64(val): round to nearest even
    u = (1 << 53) + 1
    assert mr.as_float(np.uint64(u)) == float(1 << 53)
    assert [int(x) for x in mr.encode([np.uint64(u)], 1.0, Q, N)[:, 0]] == [(1 << 53) % m for m in Q]


def test_naive_product_rule():
    x = [0] * N
    x[N // 2] = 1
    assert mr.naive_mul(x, x) == [-1 if i == 0 else (1 if i == N // 2 else 0) for i in range(N)]     # X^N = X^(N/2) - 1


def test_permutations(rh):
    m = rh.matrix_ckks
    assert m.factorN3N(24) == (3, 1) and m.pow3(3) == 27
    p = m.computeInputPermutation(12)
    assert p == [0, 6, 2, 8, 4, 10, 1, 7, 3, 9, 5, 11] and sorted(p) == list(range(12))
    assert [p[i] for i in m.computeInversePermutation(p)] == list(range(12))
    with pytest.raises(rh.RingHipError, match="other factors"):
        m.factorN3N(20)

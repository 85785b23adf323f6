"""CPU: tests/lut_restatement.py pinned to decryption in the reference's own set-up (core/rlwe/rlwe_test.go:837-913): a key between ring degrees
re-encrypts a fresh encryption of zero, in both directions, with noise Log2OfStandardDeviation <= LogN + BaseTwoDecomposition; and the reference's
literal statements (NTT rows repeated, further moduli from limb 0) give the rows of s(X^(N/n))."""
import random

import numpy as np
import pytest

import lut_restatement as lr
import rlwe_restatement as rr
from conftest import QI60, PI60

Q27 = 0x7fff801

SHAPES = [pytest.param((128, 64, QI60[:2], PI60[:1], 0), id="two-limbs-one-P"), pytest.param((128, 64, [Q27], [], 7), id="one-limb-pw2-7"),
          pytest.param((64, 16, QI60[:1], PI60[:2], 0), id="gap-4-two-P")]


@pytest.mark.parametrize("shape", SHAPES)
def test_mapped_secret_is_the_embedded_secret(oracle, shape):
    """repeating the NTT rows of s is the NTT of s(X^(N/n)), and the extension from limb 0 gives its rows under every other modulus"""
    N, n, Q, P, pw2 = shape
    sk = rr.Secret.sample(random.Random(N + n), n)
    levelQ, levelP = len(Q) - 1, len(P) - 1
    want = lr.embed(sk, N)
    for as_input in (True, False):
        got = lr.mapped_secret(sk, N, Q, P, levelQ, levelP, as_input)
        mods = list(Q) + ([] if as_input else list(P))
        assert np.array_equal(got.rows(mods), want.rows(mods))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("level", ["top", 0])
def test_key_switch_between_ring_degrees_decrypts(oracle, shape, level):
    N, n, Q, P, pw2 = shape
    level = len(Q) - 1 if level == "top" else 0
    levelQ, levelP = len(Q) - 1, len(P) - 1
    rnd = random.Random(N * 31 + n + pw2)
    sk_big, sk_small = rr.Secret.sample(rnd, N), rr.Secret.sample(rnd, n)
    bound = (N.bit_length() - 1) + pw2                                 # NoiseBound of rlwe_test.go: LogN + bpw2
    mods = [int(q) for q in Q[:level + 1]]
    # LargeToSmall (:837-878)
    evk = lr.random_degree_key(rnd, sk_big, sk_small, Q, P, levelQ, levelP, pw2)
    b, a, _ = rr.encrypt_zero(rnd, sk_big, mods)
    ct = [rr._vec("IMFORM", b, None, mods), rr._vec("IMFORM", a, None, mods)]        # a ciphertext is not in Montgomery form
    out = lr.apply_evaluation_key(N, n, Q, P, ct, evk)
    assert out[0].shape == (level + 1, n)
    assert rr.log2_std(rr.phase(out, sk_small, Q)) <= bound
    # SmallToLarge (:880-913)
    evk = lr.random_degree_key(rnd, sk_small, sk_big, Q, P, levelQ, levelP, pw2)
    b, a, _ = rr.encrypt_zero(rnd, sk_small, mods)
    ct = [rr._vec("IMFORM", b, None, mods), rr._vec("IMFORM", a, None, mods)]
    out = lr.apply_evaluation_key(n, N, Q, P, ct, evk)
    assert out[0].shape == (level + 1, N)
    noise = rr.phase(out, sk_big, Q)
    assert rr.log2_std(noise) <= bound
    # control: under the wrong key of the large ring the same ciphertext is uniform
    assert rr.log2_std(rr.phase(out, rr.Secret.sample(rnd, N), Q)) > bound + 10


# ---- RGSW encryption (core/rgsw/rgsw_test.go) and the blind rotation key set ----------------------------------------------------------------------------
RGSW_SHAPES = [pytest.param((64, QI60[:2], PI60[:2], 0), id="two-limbs-two-P"), pytest.param((64, [Q27], [], 7), id="one-limb-pw2-7"),
               pytest.param((64, QI60[:2], PI60[:1], 0), id="two-limbs-one-P")]


def _rgsw_samples(rnd, N, Q, P, levelQ, levelP, pw2, count=1):
    import keygen_restatement as kr
    rows = 2 * count * kr.rows_of(Q, levelQ, levelP, pw2)
    mods = [int(q) for q in Q[:levelQ + 1]] + ([int(p) for p in P[:levelP + 1]] if levelP >= 0 else [])
    return np.stack([rr.uniform_poly(rnd, N, mods) for _ in range(rows)]), [rr.gaussian_coeffs(rnd, N) for _ in range(rows)]


@pytest.mark.parametrize("shape", RGSW_SHAPES)
def test_rgsw_encryption_noise(oracle, shape):
    """Encryptor/SK (rgsw_test.go:37-47): a ternary plaintext in Montgomery form, both noise values <= 10.0; a zero encryption likewise"""
    N, Q, P, pw2 = shape
    levelQ, levelP = len(Q) - 1, len(P) - 1
    rnd = random.Random(N + pw2 + len(P))
    sk, m = rr.Secret.sample(rnd, N), rr.Secret.sample(rnd, N)
    pt = m.rows(Q)
    a, e = _rgsw_samples(rnd, N, Q, P, levelQ, levelP, pw2)
    left, right = lr.noise_rgsw(lr.rgsw_encrypt(sk, pt, Q, P, levelQ, levelP, pw2, a, e), pt, sk, Q, P)
    assert left <= 10.0 and right <= 10.0
    zero = np.zeros_like(pt)
    left, right = lr.noise_rgsw(lr.rgsw_encrypt(sk, None, Q, P, levelQ, levelP, pw2, a, e), zero, sk, Q, P)
    assert left <= 10.0 and right <= 10.0
    wrong = lr.noise_rgsw(lr.rgsw_encrypt(sk, pt, Q, P, levelQ, levelP, pw2, a, e), zero, sk, Q, P)        # control: the plaintext is really there
    assert min(wrong) > 20.0


@pytest.mark.parametrize("shape", RGSW_SHAPES)
def test_rgsw_external_product_decodes_exactly(oracle, shape):
    """Evaluator/ExternalProduct (rgsw_test.go:61-113): Scale X^1 times RGSW(X^0) decrypts, after DivRound by Scale = q_0, to exactly X^1"""
    from oracle import compose
    N, Q, P, pw2 = shape
    levelQ, levelP = len(Q) - 1, len(P) - 1
    rnd = random.Random(N * 7 + pw2 + len(P))
    sk = rr.Secret.sample(rnd, N)
    a, e = _rgsw_samples(rnd, N, Q, P, levelQ, levelP, pw2)
    value = lr.rgsw_encrypt(sk, lr.monomial_rows(N, 0, Q), Q, P, levelQ, levelP, pw2, a, e)
    scale = int(Q[0]) if pw2 == 0 else int(Q[0]) >> 10                 # one 27-bit limb: the scale leaves room for the digits' noise
    m = [0] * N
    m[1] = scale
    ct, _ = rr.encrypt(rnd, sk, m, Q, levelQ)
    kq, kp = [v.Q for v in value], [v.P for v in value]
    if levelP >= 1:
        out = compose.external_product(N, Q, P, levelQ, levelP, np.stack(ct), True, kq, kp)
    else:
        out = compose.external_product_single_p(N, Q, P, levelQ, levelP, np.stack(ct), pw2, value[0].digits_per_limb, kq, kp if P else [None, None])
    have = [(2 * x + scale) // (2 * scale) for x in rr.phase(list(out), sk, Q)]
    want = [0] * N
    want[1] = 1
    assert have == want


def test_restated_blind_rotation_keys_rotate(oracle):
    """keys made by the restated GenEvaluationKeyNew pass tests/test_blindrot_oracle.py's rotation check through blindrot_restatement.evaluate"""
    import blindrot_restatement as br
    import keygen_restatement as kr
    NBR, QBR, NLWE, QLWE, pw2 = 64, Q27, 32, 0x3001, 7
    st = br.setting(NBR, QBR, NLWE, QLWE, pw2, 16, 64)
    rnd = random.Random(2022198)
    rows = kr.rows_of([QBR], 0, -1, pw2)
    a_r = np.stack([rr.uniform_poly(rnd, NBR, [QBR]) for _ in range(2 * rows * NLWE)])
    e_r = [rr.gaussian_coeffs(rnd, NBR) for _ in range(2 * rows * NLWE)]
    a_g = np.stack([rr.uniform_poly(rnd, NBR, [QBR]) for _ in range(11 * rows)])
    e_g = [rr.gaussian_coeffs(rnd, NBR) for _ in range(11 * rows)]
    keys = lr.blind_rotation_keys(st.sk_br, st.sk_lwe, NBR, QBR, pw2, a_r, e_r, a_g, e_g)
    indices = [0, 5, 31]
    res = br.evaluate(st.ct, True, NLWE, QLWE, NBR, QBR, {i: st.F for i in indices}, keys)
    ab = br.lwe_samples(st.ct, True, NLWE, QLWE, NBR, indices)
    for i in indices:
        u = br.rotation(ab[i][0], ab[i][1], st.sk_lwe.coeffs, NBR)
        noise = rr.centered_diff(rr.phase(res[i], st.sk_br, [QBR]), br.expected_plaintext(st.Fc, QBR, u, NBR), QBR)
        assert max(abs(x) for x in noise) < QBR // 8 and abs(noise[0]) < QBR // 64, "slot %d" % i

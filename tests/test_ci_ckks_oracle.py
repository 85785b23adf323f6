"""CPU: pins tests/ci_ckks_restatement.py -- the yardstick tests/test_gpu_ci_ckks.py compares the device with -- to things that are not the
restatement: the canonical embedding of Z[X + X^-1]/(X^2n + 1) at zeta = exp(2 pi i / 4n), exact integer arithmetic for the mapped secret, and
the reference's own precision bound on every step of its CKKS tests in the reference's setting testInsecurePrec45 (conjugate-invariant
LogN = 10, LogQ {55, 45 x 6}, LogP {60}, scale 2^45; the standard side of testBridge at LogN = 11 with two other 61-bit P):
AVGLog2Prec >= 45 - (LogN + 3) = 32 bits on the conjugate-invariant side, 45 - (11 + 2) = 32 on the standard side (precision.go:92-103).
The Prec90 set of the reference needs the big-float encoder (prec > 53), which is not built: it is not covered."""
import math
import random

import numpy as np
import pytest

import ci_ckks_restatement as cc
import ckks_encoder_restatement as er
import ckks_restatement as cr
import keygen_restatement as kr
import rlwe_restatement as rr
from oracle import primes
from oracle.compose import unfold_ci_to_standard

LOGN, n, N = 10, 1 << 10, 1 << 11
SCALE = 2.0 ** 45
PSTD = [0x1ffffffff6c80001, 0x1ffffffff6140001]          # testBridge's auxiliary moduli of the standard side (ckks_test.go:764)
MIN_CI, MIN_STD = 45 - (LOGN + 3), 45 - (LOGN + 1 + 2)


def moduli():
    Q, P = primes.gen_moduli(12, [55] + [45] * 6, [60])   # NthRoot = 4n = 2^12
    return [int(q) for q in Q], [int(p) for p in P]


def stats(want, re, im, log2_scale=45):
    from matrix_fhe_lattigo_amd.precision import precision_stats
    return precision_stats(np.asarray(want, dtype=np.complex128), np.asarray(re) + 1j * np.asarray(im), log2_scale)


def meets(want, re, im, bound):
    p = stats(want, re, im).AVGLog2Prec
    print("AVGLog2Prec real %.2f imag %.2f (bound %d)" % (p.Real, p.Imag, bound))
    return p.Real >= bound and p.Imag >= bound


def centred(poly, mods):
    return np.array(rr.crt_centered(poly, mods), dtype=object)


# ---- the encoder against the canonical embedding ---------------------------------------------------------------------------------------------------
def embedding(c, nn, j):
    """the element c_0 + sum_k c_k (X^k + X^-k) of Z[X]/(X^2nn + 1) at zeta^(5^j), zeta = exp(2 pi i / 4nn): c_0 + 2 sum_k c_k cos(2 pi 5^j k / 4nn)"""
    r = pow(5, j, 4 * nn)
    k = np.arange(1, nn)
    return float(c[0]) + 2.0 * float(np.sum(np.asarray(c[1:], dtype=np.float64) * np.cos(2.0 * math.pi * ((r * k) % (4 * nn)) / (4 * nn))))


@pytest.mark.parametrize("nn,log_slots", [(16, 4), (16, 0), (16, 1), (64, 6), (64, 3), (256, 8)])
def test_encoder_is_the_canonical_embedding(nn, log_slots):
    mods = [int(q) for q in primes.gen_moduli(nn.bit_length() + 1, [55, 45], [])[0]]
    rng = np.random.default_rng(nn + log_slots)
    slots = 1 << log_slots
    v = rng.uniform(-1, 1, slots)
    words = cc.embed_coeffs(v + 1j * rng.uniform(-1, 1, slots), log_slots, SCALE, nn, mods)     # the imaginary parts are dropped
    assert np.array_equal(words, cc.embed_coeffs(v, log_slots, SCALE, nn, mods))
    c = centred(words, mods).astype(np.float64) / SCALE
    gap = nn // slots
    assert not np.any(np.delete(c, np.arange(0, nn, gap))), "the sparse spread writes every gap-th coefficient only"
    # each coefficient is rounded to 1 / (2 scale) and enters a slot with weight at most 2; the float64 transform adds about log2(n) 2^-53
    bound = (nn + 1) / SCALE
    for j in range(nn):
        assert abs(embedding(c, nn, j) - v[j % slots]) < bound
    # the NTT-domain words are the conjugate-invariant transform of those coefficients, and Decode inverts Embed
    pt = cc.embed(v, log_slots, SCALE, nn, mods)
    assert np.array_equal(cc.intt(pt, nn, mods), words % np.array(mods, dtype=np.uint64)[:, None])
    re, im = cc.decode(pt, log_slots, SCALE, nn, mods)
    assert np.max(np.abs(re - v)) < bound and np.max(np.abs(im)) < bound


def test_decode_is_the_evaluation_of_the_poly():
    nn = 32
    mods = [int(q) for q in primes.gen_moduli(7, [55, 45], [])[0]]
    rng = np.random.default_rng(5)
    c = rng.integers(-(1 << 40), 1 << 40, nn)
    poly = rr.rns(c, mods)
    re, im = cc.decode(poly, 5, SCALE, nn, mods, is_ntt=False)
    for j in range(nn):
        assert abs(re[j] - embedding(c.astype(np.float64) / SCALE, nn, j)) < 1e-9 * nn and abs(im[j]) < 1e-9 * nn
    for level0 in (mods[:1], mods):                                                  # the NoCRT and the CRT arm read the same coefficients
        r2, i2 = cc.decode(rr.rns(c, level0), 5, SCALE, nn, level0, is_ntt=False)
        assert np.array_equal(r2, re) and np.array_equal(i2, im)


# ---- the mapped secret ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nn", [16, 64])
def test_mapped_secret_is_the_unfolded_secret(nn):
    """GenEvaluationKeysForRingSwapNew relies on it: the rows of s(X + X^-1) under the standard NTT of degree 2nn are
    UnfoldConjugateInvariantToStandard of the conjugate-invariant rows; and the mapped poly is s in Z[X]/(X^2nn + 1) by exact arithmetic"""
    mods = [int(q) for q in primes.gen_moduli(nn.bit_length() + 1, [55, 45, 60], [])[0]]
    rnd = random.Random(nn)
    sk = cc.Secret(nn, [rnd.randrange(-1, 2) for _ in range(nn)])
    m = cc.mapped_secret(sk)
    assert m.coeffs[nn] == 0 and all(m.coeffs[i] == sk.coeffs[i] and m.coeffs[2 * nn - i] == -sk.coeffs[i] for i in range(1, nn))
    got, ci = m.rows(mods), sk.rows(mods)
    for i in range(len(mods)):
        assert np.array_equal(got[i], unfold_ci_to_standard(ci[i]))
    # multiplication commutes with the map: the product of two mapped polys is the mapped product (exact negacyclic arithmetic, then the
    # conjugate-invariant NTT-domain product)
    t = cc.Secret(nn, [rnd.randrange(-3, 4) for _ in range(nn)])
    prod = rr.negacyclic_mul(m.coeffs, cc.mapped_coeffs(t.coeffs))
    assert prod[nn] == 0 and all(prod[2 * nn - i] == -prod[i] for i in range(1, nn))
    rows = cc.ntt(rr.rns(prod[:nn], mods), nn, mods)
    a, b = cc.ntt(rr.rns(sk.coeffs, mods), nn, mods), cc.ntt(rr.rns(t.coeffs, mods), nn, mods)
    want = np.stack([(a[i].astype(object) * b[i].astype(object) % mods[i]).astype(np.uint64) for i in range(len(mods))])
    assert np.array_equal(rows, want)


# ---- the reference's tests in its own setting ----------------------------------------------------------------------------------------------------------
class Setting:
    def __init__(self):
        self.Q, self.P = moduli()
        rnd = self.rnd = random.Random(2024)
        self.sk = cc.Secret(n, [rnd.randrange(-1, 2) for _ in range(n)])
        self.rng = np.random.default_rng(7)
        self.level = len(self.Q) - 1

    def uniform(self, rows, mods, deg=n):
        return np.stack([rr.uniform_poly(self.rnd, deg, mods) for _ in range(rows)])

    def errors(self, rows, deg=n):
        return [rr.gaussian_coeffs(self.rnd, deg) for _ in range(rows)]

    def fresh(self):
        v = self.rng.uniform(-1, 1, n)
        pt = cc.embed(v, LOGN, SCALE, n, self.Q)
        ct = cc.encrypt_sk(self.sk, self.Q, self.level, self.uniform(1, self.Q)[0], self.errors(1)[0], pt)
        return v, ct

    def read(self, ct, scale=SCALE):
        mods = self.Q[:ct[0].shape[0]]
        return cc.decode(cc.decrypt(ct, self.sk, self.Q), LOGN, scale, n, mods)


@pytest.fixture(scope="module")
def S():
    return Setting()


def test_moduli_are_one_mod_4n(S):
    assert all(q % (4 * n) == 1 for q in S.Q + S.P + PSTD)
    assert [round(math.log2(q)) for q in S.Q] == [55] + [45] * 6 and [round(math.log2(p)) for p in S.P] == [60]


def test_encrypt_decrypt_add(S):
    v, ct = S.fresh()
    assert meets(v, *S.read(ct), MIN_CI)
    w, ct2 = S.fresh()
    assert meets(v + w, *S.read([rr._add(a, b, S.Q) for a, b in zip(ct, ct2)]), MIN_CI)


def test_encrypt_pk(S):
    rows = 1
    a, e = S.uniform(rows, S.Q + S.P), S.errors(rows)
    pkQ, pkP = cc.public_key(S.sk, S.Q, S.P, a, e)
    v = S.rng.uniform(-1, 1, n)
    u = [S.rnd.randrange(-1, 2) for _ in range(n)]
    ct = cc.encrypt_pk(pkQ, pkP, S.Q, S.P, S.level, n, u, S.errors(1)[0], S.errors(1)[0], cc.embed(v, LOGN, SCALE, n, S.Q))
    assert meets(v, *S.read(ct), MIN_CI)


def test_mul_relin_rescale(S):
    v, ct = S.fresh()
    w, ct2 = S.fresh()
    rows = kr.rows_of(S.Q, S.level, 0, 0)
    rlk = cc.relin_key(S.sk, S.Q, S.P, S.level, 0, 0, S.uniform(rows, S.Q + S.P), S.errors(rows))
    prod, scale = cr.mul_relin(S.Q, ct, cr.Scale(1 << 45), ct2, cr.Scale(1 << 45))
    out = cc.rescale(n, S.Q, cc.relinearize(n, S.Q, S.P, prod, rlk))
    assert out[0].shape[0] == S.level
    assert meets(v * w, *S.read(out, scale.float64() / S.Q[-1]), MIN_CI)


def test_rotate(S):
    v, ct = S.fresh()
    for k in (1, 3, -2):
        g = cc.galois_element(n, k)
        assert g % 4 == 1
        rows = kr.rows_of(S.Q, S.level, 0, 0)
        gk = cc.galois_keys(S.sk, [g], S.Q, S.P, S.level, 0, 0, S.uniform(rows, S.Q + S.P), S.errors(rows))[0]
        assert meets(np.roll(v, -k), *S.read(cc.rotate(n, S.Q, S.P, ct, gk, g)), MIN_CI)


def test_bridge(S):
    """testBridge (ckks_test.go:747-801): RealToComplex, then ct + i ct and ComplexToReal"""
    rnd = S.rnd
    sk_std = rr.Secret(N, [rnd.randrange(-1, 2) for _ in range(N)])
    rows = kr.rows_of(S.Q, S.level, 1, 0)
    a = [S.uniform(rows, S.Q + PSTD, N) for _ in (0, 1)]
    e = [S.errors(rows, N) for _ in (0, 1)]
    stdToci, ciToStd = cc.ring_swap_keys(sk_std, S.sk, S.Q, PSTD, S.level, 1, 0, a, e)
    v, ct = S.fresh()
    std = cc.real_to_complex(N, S.Q, PSTD, ct, ciToStd)
    re, im = er.decode(kr.decrypt(std, sk_std, S.Q), LOGN, SCALE, N, S.Q)
    assert meets(v, re, im, MIN_STD)
    imag, scale = cr.mul_scalar(N, S.Q, std, cr.Scale(1 << 45), 1j)
    assert scale == cr.Scale(1 << 45)
    std = [rr._add(x, y, S.Q) for x, y in zip(std, imag)]
    re, im = er.decode(kr.decrypt(std, sk_std, S.Q), LOGN, SCALE, N, S.Q)
    assert meets(v + 1j * v, re, im, MIN_STD)
    back = cc.complex_to_real(N, S.Q, PSTD, std, stdToci)
    assert back[0].shape == (S.level + 1, n)
    assert meets(v, *S.read(back, 2 * SCALE), MIN_CI)

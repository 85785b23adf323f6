"""Pins tests/bgv_encoder_restatement.py -- the reference's BGV encoder restated over the CPU oracle -- to facts that do not depend on it:
the round trip, the meaning of a plaintext (T times it is the coefficient vector times the scale, modulo T), the ring product of two
encodings (slot-wise product), and the Galois action on the slots, which pins permuteMatrix without running Go.  One negative control per
fact.  CPU only."""
import random

import numpy as np
import pytest

import bgv_encoder_restatement as er
from oracle import ring_oracle as orc

Q61 = [0x1fffffffffe00001, 0x1fffffffffc80001]
# (logN, Q, T): gap 2 on the smallest ring; gap 1
SHAPES = {"n16_gap2": (5, Q61, 97), "n64_gap1": (6, Q61, 257)}


@pytest.fixture(scope="module", params=sorted(SHAPES))
def P(request):
    logN, Q, t = SHAPES[request.param]
    return er.Params(1 << logN, Q, t)


def _values(P, seed, signed):
    rnd = random.Random(seed)
    if signed:
        v = [rnd.randrange(-((P.t + 1) >> 1), P.t >> 1) for _ in range(P.n)]      # the signed form's range: T >> 1 and up come back negative (>=)
        v[:4] = [-((P.t + 1) >> 1), (P.t >> 1) - 1, 0, -1]
        return np.array(v, dtype=np.int64)
    v = [rnd.randrange(P.t) for _ in range(P.n)]
    v[:3] = [0, P.t - 1, P.t >> 1]
    return np.array(v, dtype=np.uint64)


def _centered_crt(p, mods):
    Qb = er.prod(mods)
    crt = [(Qb // q) * pow(Qb // q, -1, q) for q in mods]
    out = []
    for j in range(p.shape[1]):
        x = sum(int(p[k, j]) * crt[k] for k in range(len(mods))) % Qb
        out.append(x - Qb if x >= Qb >> 1 else x)
    return out


@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("batched", [True, False])
def test_round_trip(P, signed, level, batched):
    v = _values(P, 1, signed)
    for scale in (1, 5):
        for is_ntt in (True, False):
            pt = er.encode(P, level, v, scale, is_ntt=is_ntt, batched=batched)
            got = er.decode(P, level, pt, scale, is_ntt=is_ntt, batched=batched, signed=signed)
            assert got.dtype == v.dtype and np.array_equal(got, v)


def test_round_trip_half_modulus(P):
    """T >> 1 itself decodes to T >> 1 - T under the signed form (>=, bgv/encoder.go:342), and the uint64 form keeps it"""
    h = P.t >> 1
    pt = er.encode(P, 1, np.array([h, h - 1], dtype=np.uint64), 1)
    assert list(er.decode(P, 1, pt, 1, signed=True)[:2]) == [h - P.t, h - 1]
    assert list(er.decode(P, 1, pt, 1, signed=False)[:2]) == [h, h - 1]
    # int64 extremes: reduced modulo T with their sign
    ext = np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -P.t, P.t], dtype=np.int64)
    got = er.decode(P, 1, er.encode(P, 1, ext, 1), 1, signed=False)[:4]
    assert [int(x) for x in got] == [(-(1 << 63)) % P.t, ((1 << 63) - 1) % P.t, 0, 0]


def test_round_trip_control_wrong_scale(P):
    v = _values(P, 2, False)
    assert not np.array_equal(er.decode(P, 1, er.encode(P, 1, v, 5), 3), v)


@pytest.mark.parametrize("level", [0, 1])
def test_plaintext_meaning(P, level):
    """T * pt, reconstructed and centred, is congruent to the coefficient vector times the scale modulo T, on the stride and zero off it"""
    v, scale = _values(P, 3, False), 7
    mods = P.Q[:level + 1]
    coeffs = er.encode_ring_t(P, v, 1)                                   # INTT of the permuted values
    pt = er.encode(P, level, v, scale, is_ntt=False)
    tx = _centered_crt(np.stack([er._u([int(x) * P.t % q for x in pt[i]]) for i, q in enumerate(mods)]), mods)
    for j in range(P.N):
        want = int(coeffs[j // P.gap]) * scale % P.t if j % P.gap == 0 else 0
        assert tx[j] % P.t == want and abs(tx[j]) < P.t, j
    # control: without the scale-up by T^-1 the same statement fails
    raw = er.embed(P, level, v, scale, False, False, False)
    bad = _centered_crt(np.stack([er._u([int(x) * P.t % q for x in raw[i]]) for i, q in enumerate(mods)]), mods)
    assert any(bad[j] % P.t != int(coeffs[j // P.gap]) * scale % P.t for j in range(0, P.N, P.gap))


def test_ring_product_is_slotwise_product(P):
    a, b = _values(P, 4, False), _values(P, 5, False)
    s0, s1, level = 3, 5, 1
    mods, srs = P.Q[:level + 1], P.srQ[:level + 1]
    x, y = er.encode(P, level, a, s0), er.encode(P, level, b, s1)
    # T * x * y in the NTT domain: the plaintext of scale s0 * s1 tensorStandard leaves (T times the product)
    pr = np.stack([er._u([int(u) * int(w) % q * P.t % q for u, w in zip(x[i], y[i])]) for i, q in enumerate(mods)])
    want = np.array([int(u) * int(w) % P.t for u, w in zip(a, b)], dtype=np.uint64)
    assert np.array_equal(er.decode(P, level, pr, s0 * s1 % P.t), want)
    # control: encoded without the slot permutation and transform (IsBatched = false) the ring product is a convolution, not slot-wise
    x, y = er.encode(P, level, a, s0, batched=False), er.encode(P, level, b, s1, batched=False)
    pr = np.stack([er._u([int(u) * int(w) % q * P.t % q for u, w in zip(x[i], y[i])]) for i, q in enumerate(mods)])
    assert not np.array_equal(er.decode(P, level, pr, s0 * s1 % P.t, batched=False), want)


def _galois(P, pt, g):
    """X -> X^g on a coefficient-domain poly of degree N"""
    return np.stack([orc.automorphism(pt[i], g, q) for i, q in enumerate(P.Q[:pt.shape[0]])])


def _rotations_hold(P):
    v = _values(P, 6, False)
    half = P.n >> 1
    pt = er.encode(P, 1, v, 1, is_ntt=False)
    rot = er.decode(P, 1, _galois(P, pt, 5), 1, is_ntt=False)
    swap = er.decode(P, 1, _galois(P, pt, 2 * P.N - 1), 1, is_ntt=False)
    rows = v.reshape(2, half)
    return (np.array_equal(rot.reshape(2, half), np.roll(rows, -1, axis=1)) and np.array_equal(swap.reshape(2, half), rows[::-1]))


def test_galois_action_pins_permute_matrix(P):
    """X -> X^5 rotates each of the two rows by one slot, X -> X^(2N - 1) swaps the rows"""
    assert _rotations_hold(P)


def test_galois_action_control_transposed_table(P):
    inv = [0] * P.n
    for i, p in enumerate(P.perm):
        inv[p] = i
    assert inv != P.perm
    assert not _rotations_hold(er.Params(P.N, P.Q, P.t, perm=inv))


def test_permute_matrix_is_a_permutation_of_bit_reversed_odd_powers():
    for logn in (3, 4, 10):
        perm = er.permute_matrix(logn)
        assert sorted(perm) == list(range(1 << logn))
        assert perm[0] == 0 and perm[1 << (logn - 1)] == (1 << logn) - 1


def test_q2t_branches_agree_with_big_integers(P):
    """every RingQ2T branch returns T * x centred modulo Q, then modulo T -- the ModUpExact branch up to its representative"""
    rnd = random.Random(7)
    for level in (0, 1):
        mods = P.Q[:level + 1]
        Qb = er.prod(mods)
        tinv = pow(P.t, -1, Qb)
        m = [rnd.randrange(P.t) for _ in range(P.N)]
        e = [rnd.randrange(-5, 6) for _ in range(P.N)]
        x = [(mi * tinv + ei) % Qb for mi, ei in zip(m, e)]               # T * x = m + T e: a noisy plaintext
        pQ = np.stack([er._u([v % q for v in x]) for q in mods])
        got = er.ring_q2t(P, level, pQ)
        assert [int(g) % P.t for g in got] == m[::P.gap]

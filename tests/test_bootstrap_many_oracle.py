"""CPU: tests/bootstrap_many_restatement.py (the reference's pack / unpack / pair fold loops) pinned to ground truth that does not depend on the
composition:
  * INTT(pack(...)) is the sum of the negacyclic shifts X^(e_k) INTT(in_k), e_k = sum over the set bits i of k of 2^(logGap - i), in Python-integer
    coefficient arithmetic, over the inputs that exist -- so the reference's odd-tail rule (:1052-1057) IS padding with absent ciphertexts: every
    n in 1 .. 2 G + 1 at g = 1, 2, 3;
  * unpack(pack(x)) decodes, at the inputs' LogSlots, to every input vector (tests/ckks_encoder_restatement.py);
  * the pair fold Mul(1i) + Add is the product with NTT(X^(N/2)), the top GenXPow2NTT row, word for word, and the unfold Mul(-1i) the
    product with its negation.
N = 64 and N = 256, a mixed-width 3-limb chain (60, 40, 56 bits), at the top level and at level 0."""
import functools

import numpy as np
import pytest

import bootstrap_many_restatement as bm
import ckks_encoder_restatement as er
import ckks_restatement as cr
import ring_packing_restatement as rp
import rlwe_restatement as rr
from conftest import uniform_mod

LOGQ = [60, 40, 56]
SHAPES = [(64, 2), (64, 0), (256, 2), (256, 0)]                    # (N, level)
ids = ["N%d-level%d" % s for s in SHAPES]


@functools.lru_cache(maxsize=None)
def chain():
    from oracle import primes
    Q, _ = primes.gen_moduli(9, LOGQ, [61])
    return tuple(int(q) for q in Q)


@functools.lru_cache(maxsize=None)
def tables(N, L):
    mods = chain()[:L]
    logN = N.bit_length() - 1
    return rp.gen_xpow2_ntt(N, mods, logN, False), rp.gen_xpow2_ntt(N, mods, logN, True)


def random_ct(rng, N, mods):
    return [np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in (0, 1)]


def shift(coeffs, e, q):
    """X^e times a polynomial of Z_q[X] / (X^N + 1), Python integers"""
    N = len(coeffs)
    out = [0] * N
    for i, c in enumerate(coeffs):
        k = i + e
        out[k % N] = (q - c) % q if (k // N) & 1 else c
    return out


def context(N, log_slots, g, n):
    return bm.PackingContext(N, N.bit_length() - 2, log_slots + g, log_slots, n)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("g", [1, 2, 3])
def test_pack_is_the_sum_of_shifts_over_the_inputs_that_exist(shape, g):
    N, level = shape
    mods = chain()[:level + 1]
    xp, _ = tables(N, level + 1)
    log_slots = 2
    logGap = (N.bit_length() - 2) - log_slots - 1
    G = 1 << g
    rng = np.random.default_rng(100 * N + 10 * level + g)
    cts = [random_ct(rng, N, mods) for _ in range(2 * G + 1)]
    coeff = [[rr.intt(c, N, mods) for c in ct] for ct in cts]
    for n in range(1, 2 * G + 2):
        got, dims = bm.pack(cts[:n], [log_slots] * n, context(N, log_slots, g, n), xp, mods)
        assert len(got) == -(-n // G) and dims == log_slots + g
        for j, ct in enumerate(got):
            for c in (0, 1):
                have = rr.intt(ct[c], N, mods)
                for l, q in enumerate(mods):
                    want = [0] * N
                    for k in range(min(G, n - j * G)):
                        e = sum(1 << (logGap - i) for i in range(g) if k >> i & 1)
                        s = shift([int(v) for v in coeff[j * G + k][c][l]], e, q)
                        want = [(a + b) % q for a, b in zip(want, s)]
                    assert [int(v) for v in have[l]] == want, (n, j, c, l)
    assert all(np.array_equal(a, b) for ct, co in zip(cts, coeff) for a, b in zip(ct, [rr.ntt(x, N, mods) for x in co]))      # inputs untouched


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_unpack_of_pack_decodes_to_every_input(shape):
    N, level = shape
    mods = chain()[:level + 1]
    xp, xinv = tables(N, level + 1)
    log_slots, g = 2, 2
    scale = float(1 << 30)
    rng = np.random.default_rng(N + level)
    for n in (3, 4, 5, 9):
        vals = [rng.uniform(-1, 1, 1 << log_slots) + 1j * rng.uniform(-1, 1, 1 << log_slots) for _ in range(n)]
        cts = [[er.embed(v, log_slots, scale, N, list(mods)), np.stack([uniform_mod(rng, q, N) for q in mods])] for v in vals]
        packed, dims = bm.pack(cts, [log_slots] * n, context(N, log_slots, g, n), xp, mods)
        ctxt = context(N, log_slots, g, n)
        out = bm.unpack_many(packed, ctxt, xinv, mods)
        assert len(out) == n and ctxt.NbPackedCTs == 0
        for v, ct, ct_in in zip(vals, out, cts):
            re, im = er.decode(ct[0], log_slots, scale, N, list(mods))
            re0, im0 = er.decode(ct_in[0], log_slots, scale, N, list(mods))
            assert np.array_equal(re, re0) and np.array_equal(im, im0)
            assert np.max(np.abs(re - v.real)) < 2.0 ** -20 and np.max(np.abs(im - v.imag)) < 2.0 ** -20
        if n > 1:
            assert not np.array_equal(out[1][0], cts[1][0])                  # the other ciphertexts' coefficients are still there, off the gap


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_pair_fold_is_the_product_with_the_top_power_row(shape):
    N, level = shape
    mods = chain()[:level + 1]
    xp, _ = tables(N, level + 1)
    i_row, minus_i = bm.x_pow_half_ntt(N, mods), bm.x_pow_half_ntt(N, mods, neg=True)
    assert np.array_equal(i_row, xp[N.bit_length() - 2])
    rng = np.random.default_rng(N * 3 + level)
    left, right = random_ct(rng, N, mods), random_ct(rng, N, mods)
    scale = cr.Scale(2 ** 40)
    fold = bm.pair_fold(N, mods, left, right, scale)
    for c in (0, 1):
        assert np.array_equal(fold[c], bm._mul_then_add(right[c], i_row, left[c], mods))
    alone = bm.pair_fold(N, mods, left, None, scale)
    assert all(np.array_equal(a, b) for a, b in zip(alone, left))
    unfold = bm.pair_unfold(N, mods, fold, scale)
    for c in (0, 1):
        assert np.array_equal(unfold[c], rr._vec("MUL_MONT", fold[c], minus_i, mods))
    # ... which is pack / unpack with a group of 2 and that one row
    ctxt = bm.PackingContext(N, 1, 1, 0, 2)                                  # logGap = 0, one level: the row is xPow2[0] of the list handed in
    packed, _ = bm.pack([left, right], [0, 0], ctxt, [i_row], mods)
    assert len(packed) == 1 and all(np.array_equal(a, b) for a, b in zip(packed[0], fold))
    un = bm.unpack(fold, bm.PackingContext(N, 1, 1, 0, 2), [minus_i], mods)
    assert all(np.array_equal(a, b) for a, b in zip(un[0], fold)) and all(np.array_equal(a, b) for a, b in zip(un[1], unfold))


def test_pack_refusals():
    N, mods = 64, chain()
    xp, _ = tables(N, 3)
    rng = np.random.default_rng(5)
    cts = [random_ct(rng, N, mods) for _ in range(2)]
    with pytest.raises(bm.PackError, match="cts\\[0\\].LogSlots\\(\\)=3 > logMaxSlots=2"):
        bm.pack(cts, [3, 3], bm.PackingContext(N, 5, 2, 3, 2), xp, mods)
    with pytest.raises(bm.PackError, match="cts\\[1\\].PlaintextLogSlots\\(\\)=1 != cts\\[0\\].PlaintextLogSlots=2"):
        bm.pack(cts, [2, 1], context(N, 2, 1, 2), xp, mods)
    with pytest.raises(bm.PackError, match="cts\\[0\\].Value\\[0\\].N\\(\\)=64 != params.N\\(\\)=128"):
        bm.pack(cts, [2, 2], bm.PackingContext(128, 6, 3, 2, 2), xp, mods)

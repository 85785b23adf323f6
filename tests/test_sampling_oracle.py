"""CPU: the sampler stream and the restated samplers (tests/sampling_restatement.py) against their definitions, and the host half of
matrix-fhe-lattigo_amd/sampling.py (the BLAKE2b key state the device starts from, the cumulative table, the Hamming-weight sampler) against them."""
import hashlib
import math
import random
import struct

import numpy as np
import pytest

import sampling_restatement as sr
from oracle import primes

KEY = bytes(range(64))
N_STAT = 1 << 16


def small_prime(logN=10):
    """the smallest NTT-friendly prime above 2^35 for N = 2^logN: it rejects about half of its 36-bit candidates"""
    q = (1 << 35) + 1
    while not (primes.is_prime(q) and q % (2 << logN) == 1):
        q += 2 << logN
    return q


def test_key_state_and_final_block_are_blake2b(rh):
    from matrix_fhe_lattigo_amd import sampling
    for key in (KEY, b"k", bytes(range(7, 40))):
        state = sampling.blake2b_key_state(key)
        for ids in ((0, 0, 0, 0, 0), (3, 2, 1, 127, 5), (2 ** 64 - 1, 2 ** 40, 29, 8191, 2 ** 33)):
            msg = struct.pack("<5Q", *ids)
            want = struct.unpack("<8Q", hashlib.blake2b(msg, key=key, digest_size=64, person=sr.PERSON).digest())
            assert tuple(sampling.blake2b_final_block(state, msg)) == want == sr.block(key, *ids)
    with pytest.raises(rh.RingHipError, match="1 to 64 bytes"):
        sampling.KeyedPRNG(bytes(65))
    a, b = sampling.NewPRNG(), sampling.NewPRNG()
    assert len(a.key) == 64 and a.key != b.key and [a.next_call(), a.next_call()] == [0, 1]


@pytest.mark.parametrize("sigma,bound", [(3.2, 19), (3.2, 19.2), (3.2, 19.7), (1.0, 6), (40.0, 255.5)])
def test_cumulative_table(rh, sigma, bound):
    from matrix_fhe_lattigo_amd import sampling
    table = sr.gaussian_table(sigma, bound)
    assert table == sampling.gaussian_table(sigma, bound)
    assert len(table) == sr.top(bound) + 1 == (int(bound) + 1 if bound - int(bound) <= 0.5 else int(bound) + 2) and table[-1] == 1 << 63
    assert all(a < b for a, b in zip(table, table[1:]))
    other = sr.gaussian_table_by_quadrature(sigma, bound)
    assert max(abs(a - b) for a, b in zip(table, other)) <= 1               # one unit of 2^-63


def test_table_refusals(rh):
    from matrix_fhe_lattigo_amd import sampling
    with pytest.raises(rh.RingHipError, match="big-norm"):
        sampling.gaussian_table(1e6, 1024.0)
    with pytest.raises(rh.RingHipError, match="big-norm"):
        sampling.gaussian_table(1e6, 1023.7)                                # magnitudes up to 1024: one entry more than the kernel's table holds
    assert len(sampling.gaussian_table(300.0, 1023.5)) == 1024
    with pytest.raises(rh.RingHipError, match=r"\[0, 1\]"):
        sampling.ternary_threshold(1.5)
    assert sampling.ternary_threshold(0.5) == 1 << 62 and sampling.ternary_threshold(1) == 1 << 63
    assert sampling.ternary_threshold(2 / 3) == int(__import__("fractions").Fraction(2 / 3) * (1 << 63))


def _check_moments(x, var, m4, what):
    """|mean| <= 6 sqrt(var / n) and |std - sigma| <= 6 SE(std), SE(std) = sqrt((m4 - var^2) / n) / (2 sigma) (the delta method on the sample
    variance, whose variance is (m4 - var^2) / n for a zero-mean sample): moments of the sampled law itself, nothing measured"""
    n = x.size
    var, m4 = float(var), float(m4)
    mean, std = float(x.mean()), float(x.std())
    se_mean, se_std = math.sqrt(var / n), math.sqrt((m4 - var * var) / n) / (2 * math.sqrt(var))
    print("MEASURED %s mean %.5f (6 SE %.5f)  std %.5f (want %.5f, 6 SE %.5f)" % (what, mean, 6 * se_mean, std, math.sqrt(var), 6 * se_std))
    assert abs(mean) <= 6 * se_mean
    assert abs(std - math.sqrt(var)) <= 6 * se_std


def test_a_bound_with_a_fraction_above_one_half_reaches_the_next_integer():
    """|z| sigma = 2.6 <= 2.7 rounds to 3 (uint64(v + 0.5), ring/sampler_gaussian.go:164-165): the table has an entry for it and ends at 2^63"""
    table = sr.gaussian_table(1.0, 2.7)
    assert len(table) == 4 and table[-1] == 1 << 63 and table[2] < table[3]
    x = sr.gaussian(KEY, 8, 1, 1 << 12, table)[0]
    assert x.min() == -3 and x.max() == 3
    assert len(sr.gaussian_table(1.0, 2.5)) == 3 and len(sr.gaussian_table(1.0, 3)) == 4


def test_gaussian_statistics():
    table = sr.gaussian_table(3.2, 19)
    x = sr.gaussian(KEY, 7, 1, N_STAT, table)[0]
    assert x.min() >= -19 and x.max() <= 19
    _, var, m4 = sr.table_moments(table)
    assert abs(math.sqrt(float(var)) - 3.2) < 0.05                          # the rounded Gaussian's own deviation: sqrt(sigma^2 + 1/12) = 3.213
    _check_moments(x, var, m4, "gaussian(3.2, 19)")


@pytest.mark.parametrize("P", [2 / 3, 0.5])
def test_ternary_statistics(rh, P):
    from matrix_fhe_lattigo_amd import sampling
    thr = sampling.ternary_threshold(P)
    x = sr.ternary(KEY, 9, 1, N_STAT, thr)[0]
    assert set(np.unique(x)) == {-1, 0, 1}
    p = thr / float(1 << 63)
    _check_moments(x, p, p, "ternary(%.3f)" % P)                            # x^2 = x^4 = 1 with probability P


def test_uniform_rows_take_several_blocks_and_depend_on_their_ids_alone():
    q = small_prime()
    row, most = sr.uniform_row(KEY, 1, 2, 3, 1024, q)
    assert most >= 3 and int(row.max()) < q                                 # 128 groups of eight at acceptance 1/2: every group needs more than one block
    big, most_big = sr.uniform_row(KEY, 1, 2, 3, 1024, 0x1fffffffffe00001)
    assert most_big == 1 and int(big.max()) < 0x1fffffffffe00001            # a 61-bit prime just below 2^61 accepts at once
    mods = [0x1fffffffffe00001, q]
    whole = sr.uniform(KEY, 4, 3, 64, mods)
    parts = np.concatenate([sr.uniform(KEY, 4, 1, 64, mods, poly0=0), sr.uniform(KEY, 4, 2, 64, mods, poly0=1)])
    assert np.array_equal(whole, parts)
    assert np.array_equal(sr.uniform(KEY, 4, 3, 64, mods[1:], row0=1), whole[:, 1:])
    assert not np.array_equal(whole, sr.uniform(KEY, 5, 3, 64, mods))
    # the mean of a uniform row: within 6 standard errors of (q - 1) / 2, the deviation of a uniform residue being q / sqrt(12)
    assert abs(float(row.astype(np.float64).mean()) - (q - 1) / 2) <= 6 * q / math.sqrt(12 * 1024)


def test_lift_and_hamming_weight(rh):
    from matrix_fhe_lattigo_amd import sampling
    x = np.array([[0, 1, -1, 19, -19, 2 ** 31 - 1, -2 ** 31 + 1, 5]], dtype=np.int32)
    got = sr.lift(x, [97, 0x1fffffffffe00001])
    assert got[0, 0].tolist() == [v % 97 for v in x[0].tolist()] and got[0, 1, 2] == 0x1fffffffffe00000 and got[0, 1, 0] == 0

    class Rng:
        def __init__(self):
            self.r = random.Random(5)

        def randbelow(self, n):
            return self.r.randrange(n)
    s = sampling.ternary_hamming_weight(256, 64, Rng())
    assert np.count_nonzero(s) == 64 and set(np.unique(s)) == {-1, 0, 1}
    assert np.count_nonzero(sampling.ternary_hamming_weight(256, 256)) == 256 and not sampling.ternary_hamming_weight(256, 0).any()

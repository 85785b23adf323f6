"""The sampler stream and the three samplers of matrix-fhe-lattigo_amd/sampling.py restated with hashlib and numpy: what the device samplers are
compared with, bit for bit.  TEST INFRASTRUCTURE ONLY.

Block t of substream (call, poly, row, group): hashlib.blake2b(struct.pack('<5Q', call, poly, row, group, t), key=key, digest_size=64,
person=b'ringhip-sampler\\0') as eight little-endian words; coefficient i uses word i % 8 of blocks t = 0, 1, ... of group i // 8."""
import hashlib
import struct

import numpy as np

PERSON = b"ringhip-sampler\0"


def block(key, call, poly, row, group, t):
    d = hashlib.blake2b(struct.pack("<5Q", call, poly, row, group, t), key=key, digest_size=64, person=PERSON).digest()
    return struct.unpack("<8Q", d)


def words(key, call, poly, row, N):
    """the first candidate of every coefficient of a row: (N,) uint64"""
    return np.array([w for g in range(N // 8) for w in block(key, call, poly, row, g, 0)], dtype=np.uint64)


def uniform_row(key, call, poly, row, N, q):
    """ring/sampler_uniform.go:77-101 on the stream: candidate = word & Mask, Mask = 2^Len64(q - 1) - 1, accepted when < q.
    Returns the row and the number of blocks its neediest group used."""
    q = int(q)
    mask = (1 << (q - 1).bit_length()) - 1
    out = np.zeros(N, dtype=np.uint64)
    most = 0
    for g in range(N // 8):
        pending, t = set(range(8)), 0
        while pending:
            w = block(key, call, poly, row, g, t)
            for k in sorted(pending):
                c = w[k] & mask
                if c < q:
                    out[8 * g + k] = c
                    pending.discard(k)
            t += 1
        most = max(most, t)
    return out, most


def uniform(key, call, npoly, N, moduli, poly0=0, row0=0):
    """(npoly, len(moduli), N)"""
    return np.stack([np.stack([uniform_row(key, call, poly0 + p, row0 + j, N, q)[0] for j, q in enumerate(moduli)]) for p in range(npoly)])


def top(bound):
    """the largest magnitude uint64(v + 0.5) reaches for v <= bound (a v exactly half-way has probability zero)"""
    import math
    return math.ceil(bound - 0.5)


def gaussian_table(sigma, bound):
    """T[k] = floor(P(|x| <= k) 2^63), k = 0 .. ceil(bound - 1/2): |x| = floor(|z| sigma + 0.5) for a standard normal z conditioned on
    |z| sigma <= bound (ring/sampler_gaussian.go:159-172), so P(|x| <= k) = erf(min(k + 1/2, bound) / (sigma sqrt 2)) / erf(bound / (sigma sqrt 2)).
    The largest magnitude is floor(bound), or floor(bound) + 1 when the bound's fraction is above one half."""
    import mpmath
    with mpmath.workprec(256):
        s, b = mpmath.mpf(sigma) * mpmath.sqrt(2), mpmath.mpf(bound)
        whole = mpmath.erf(b / s)
        return [int(mpmath.floor(mpmath.erf(min(mpmath.mpf(k) + mpmath.mpf(1) / 2, b) / s) / whole * (1 << 63))) for k in range(top(bound) + 1)]


def gaussian_table_by_quadrature(sigma, bound):
    """the same table by a second route: the density of |z| sigma integrated numerically over each [k - 1/2, k + 1/2) cut to [0, bound], summed"""
    import mpmath
    with mpmath.workprec(256):
        sg, b = mpmath.mpf(sigma), mpmath.mpf(bound)
        pdf = lambda x: mpmath.sqrt(2 / mpmath.pi) / sg * mpmath.exp(-x * x / (2 * sg * sg))      # the half-normal density of |z| sigma
        half = mpmath.mpf(1) / 2
        cells = [mpmath.quad(pdf, [max(k - half, 0), min(k + half, b)]) for k in range(top(bound) + 1)]
        whole = mpmath.fsum(cells)
        out, acc = [], mpmath.mpf(0)
        for c in cells:
            acc += c
            out.append(int(mpmath.floor(acc / whole * (1 << 63))))
        return out


def gaussian_from_words(w, table):
    """one word per coefficient: |x| = #{k: T[k] <= word & (2^63 - 1)} (numpy.searchsorted, integers only), negative when bit 63 is set"""
    w = np.asarray(w, dtype=np.uint64)
    mag = np.searchsorted(np.array(table, dtype=np.uint64), w & np.uint64((1 << 63) - 1), side="right").astype(np.int32)
    return np.where((w >> np.uint64(63)).astype(bool), -mag, mag).astype(np.int32)


def gaussian(key, call, npoly, N, table, poly0=0):
    """(npoly, N) int32"""
    return np.stack([gaussian_from_words(words(key, call, poly0 + p, 0, N), table) for p in range(npoly)])


def ternary_from_words(w, threshold):
    """non-zero when (word >> 1) < threshold = floor(P 2^63); negative when bit 0 is set"""
    w = np.asarray(w, dtype=np.uint64)
    nz = ((w >> np.uint64(1)) < np.uint64(threshold)).astype(np.int32) if threshold < (1 << 63) else np.ones(w.shape, dtype=np.int32)
    return np.where((w & np.uint64(1)).astype(bool), -nz, nz).astype(np.int32)


def ternary(key, call, npoly, N, threshold, poly0=0):
    return np.stack([ternary_from_words(words(key, call, poly0 + p, 0, N), threshold) for p in range(npoly)])


def lift(small, moduli):
    """int32 (npoly, N) -> (npoly, len(moduli), N): x >= 0 ? x : q - |x|, the canonical 0 for 0"""
    x = np.asarray(small, dtype=np.int64)
    return np.stack([np.stack([(row % np.int64(int(q))).astype(np.uint64) if int(q) < (1 << 62) else np.array([int(v) % int(q) for v in row], dtype=np.uint64)
                               for q in moduli]) for row in x])


def table_moments(table):
    """(P(x = 0), E[x^2], E[x^4]) of the signed sample the table defines (the mean is 0 by the independent sign), as exact rationals over 2^63"""
    from fractions import Fraction
    one = Fraction(1 << 63)
    prob = [Fraction(table[0]) / one] + [Fraction(table[k] - table[k - 1]) / one for k in range(1, len(table))]
    return prob[0], sum(p * k * k for k, p in enumerate(prob)), sum(p * k ** 4 for k, p in enumerate(prob))

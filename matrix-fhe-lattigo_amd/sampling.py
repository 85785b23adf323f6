"""The samplers of ring/sampler*.go and utils/sampling/prng.go on the device, on a stream of the library's own.

The stream.  A PRNG is a key (at most 64 bytes) and a host-side call counter; every sampler Read takes the next counter value.  Block t of
substream (call, poly, row, group) is

    hashlib.blake2b(struct.pack('<5Q', call, poly, row, group, t), key=key, digest_size=64, person=b'ringhip-sampler\\0')

read as eight little-endian uint64 words.  Coefficient i belongs to group i // 8 and uses word i % 8 of blocks t = 0, 1, ...: what it gets
depends on (key, call, poly, row, i) alone, not on how the launch is cut.  `row` is the limb index for uniform polys, counting the limbs of Q
first and then those of P, and 0 for the small-norm samplers; `poly` is the index within the batch, so a batch sampled in sub-blocks with the
matching offsets is the same batch.  On the device one lane serves one group with one BLAKE2b compression per block: the chaining value after
the padded key block is computed here, once per key (blake2b_key_state).

  UniformSampler   ring/sampler_uniform.go:46-106: candidate = word & Mask, accepted when < q
  GaussianSampler  the distribution of ring/sampler_gaussian.go:159-172 -- |x| = floor(|z| sigma + 0.5) for a standard normal z conditioned on
                   |z| sigma <= bound, with an independent sign -- from a cumulative table instead of the ziggurat
  TernarySampler   ring/sampler_ternary.go: a density P on the device; an exact Hamming weight H on the host with `secrets`

Deviations from the reference, on purpose: the stream is not the Go sampler's sequential byte stream (which consumes a data-dependent number
of bytes per coefficient); the Gaussian comes from a cumulative table exact to 2^-63; a zero is the canonical 0 whatever its sign (the
reference writes q for a zero of sign 0).  Standard rings and 3N rings whose degree is a multiple of 8 (a lane serves a group of eight
coefficients; rows are addressed at N words, not at 2^logN).  The big-norm Gaussian (:99-153), conjugate-invariant rings and the other 3N
degrees are refused by name.  Conjugate-invariant rings are served behind a permit: the keyword conjugate_invariant=True, which only the
factories of ckks.Parameters set (rings_ok says why); the arithmetic is the same, N coefficients per row."""
import ctypes as C
import secrets
import struct

import numpy as np

from .ringhip import ConjugateInvariant, DevicePoly, Matrix3N, RingHipError, U64P, _check, lib

PERSON = b"ringhip-sampler\0"
_IV = (0x6a09e667f3bcc908, 0xbb67ae8584caa73b, 0x3c6ef372fe94f82b, 0xa54ff53a5f1d36f1,
       0x510e527fade682d1, 0x9b05688c2b3e6c1f, 0x1f83d9abfb41bd6b, 0x5be0cd19137e2179)
_SIGMA = ((0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15), (14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3),
          (11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4), (7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8),
          (9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13), (2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9),
          (12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11), (13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10),
          (6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5), (10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0))
_M64 = (1 << 64) - 1


def _compress(h, block, t, last):
    """RFC 7693 section 3.2 on Python integers"""
    m = struct.unpack("<16Q", block)
    v = list(h) + list(_IV)
    v[12] ^= t & _M64
    v[13] ^= t >> 64
    if last:
        v[14] ^= _M64
    rot = lambda x, r: ((x >> r) | (x << (64 - r))) & _M64

    def g(a, b, c, d, x, y):
        v[a] = (v[a] + v[b] + x) & _M64; v[d] = rot(v[d] ^ v[a], 32)
        v[c] = (v[c] + v[d]) & _M64; v[b] = rot(v[b] ^ v[c], 24)
        v[a] = (v[a] + v[b] + y) & _M64; v[d] = rot(v[d] ^ v[a], 16)
        v[c] = (v[c] + v[d]) & _M64; v[b] = rot(v[b] ^ v[c], 63)
    for r in range(12):
        s = _SIGMA[r % 10]
        g(0, 4, 8, 12, m[s[0]], m[s[1]]); g(1, 5, 9, 13, m[s[2]], m[s[3]]); g(2, 6, 10, 14, m[s[4]], m[s[5]]); g(3, 7, 11, 15, m[s[6]], m[s[7]])
        g(0, 5, 10, 15, m[s[8]], m[s[9]]); g(1, 6, 11, 12, m[s[10]], m[s[11]]); g(2, 7, 8, 13, m[s[12]], m[s[13]]); g(3, 4, 9, 14, m[s[14]], m[s[15]])
    return [h[i] ^ v[i] ^ v[8 + i] for i in range(8)]


def blake2b_key_state(key):
    """the eight chaining words of the stream's hash after its first block, the key padded to 128 bytes: what every block of every substream
    starts from.  Parameter block: 64-byte digest, the key's length, fanout 1, depth 1, the personalisation in bytes 48..63."""
    key = bytes(key)
    if not 1 <= len(key) <= 64:
        raise RingHipError("KeyedPRNG: the key must have 1 to 64 bytes")
    param = struct.pack("<BBBB", 64, len(key), 1, 1) + bytes(44) + PERSON
    h = [iv ^ p for iv, p in zip(_IV, struct.unpack("<8Q", param))]
    return _compress(h, key + bytes(128 - len(key)), 128, False)


def blake2b_final_block(state, message):
    """the digest words of a message of at most 128 bytes after the key block (what the device computes per block; tests compare it with hashlib)"""
    return _compress(state, message + bytes(128 - len(message)), 128 + len(message), True)


class KeyedPRNG:
    """sampling.NewKeyedPRNG (utils/sampling/prng.go): the key and a host-side call counter.  Two PRNGs with the same key replay the same reads."""

    def __init__(self, key):
        self.key = bytes(key)
        self.state = blake2b_key_state(self.key)
        self._state = (C.c_uint64 * 8)(*self.state)
        self.calls = 0

    def next_call(self):
        c = self.calls
        self.calls += 1
        return c


def NewPRNG():
    """sampling.NewPRNG: a 64-byte key from the operating system's generator"""
    return KeyedPRNG(secrets.token_bytes(64))


def rings_ok(who, ring, ringP=None, conjugate_invariant=False):
    """the rings of the key layer: standard rings and 3N rings with N % 8 == 0, ringQ and ringP of the same kind.
    conjugate_invariant: the permit for conjugate-invariant rings.  The samplers, KeyGenerator, Encryptor and Decryptor take it as a keyword of
    that name and hand it on; the factories of ckks.Parameters (NewKeyGenerator, NewEncryptor, NewDecryptor) are what sets it, the way the
    reference reaches such a ring through a parameters object.  A bare constructor on a conjugate-invariant ring handle keeps refusing: the
    multiparty protocols, RGSW, blind rotation and the traces build on these constructors and are not made for such rings."""
    for r in (ring, ringP):
        if r is None:
            continue
        if r.kind == ConjugateInvariant and not conjugate_invariant:
            raise RingHipError("cannot %s: conjugate-invariant rings are not supported (of the power-of-two rings, standard rings only)" % who)
        if r.kind == Matrix3N and r.N % 8:
            raise RingHipError("cannot %s: a 3N ring of degree %d: the samplers serve groups of eight coefficients (N %% 8 must be 0)" % (who, r.N))
    if ringP is not None and ringP.kind != ring.kind:
        raise RingHipError("cannot %s: ringQ and ringP must be of the same kind" % who)


class SmallPoly:
    """int32 (npoly, N) signed coefficients on the device: what the small-norm samplers write and the lift reads"""

    def __init__(self, ring, npoly):
        self.ring, self.npoly, self.N = ring, int(npoly), ring.N
        self._block = DevicePoly(ring.AtLevel(0), (self.npoly + 1) // 2, 1)         # npoly * N int32 = ceil(npoly / 2) rows of N words
        self.ptr = self._block.ptr

    @classmethod
    def from_numpy(cls, ring, arr):
        arr = np.ascontiguousarray(np.asarray(arr, dtype=np.int32))
        if arr.ndim == 1:
            arr = arr[None]
        if arr.ndim != 2 or arr.shape[1] != ring.N:
            raise RingHipError("SmallPoly: expected an (npoly, N) array of int32")
        p = cls(ring, arr.shape[0])
        p.upload(arr)
        return p

    def upload(self, arr):
        """host int32 (npoly, N) -> this block"""
        arr = np.ascontiguousarray(np.asarray(arr, dtype=np.int32)).reshape(-1)
        if arr.size != self.npoly * self.N:
            raise RingHipError("SmallPoly: expected %d x %d coefficients" % (self.npoly, self.N))
        _check(lib().rh_dev_upload(self.ring._h, self.ptr, arr.view(np.uint64).ctypes.data_as(U64P), arr.size // 2))

    def numpy(self):
        out = np.empty((self.npoly, self.N), dtype=np.int32)
        _check(lib().rh_dev_download(self.ring._h, out.view(np.uint64).ctypes.data_as(U64P), self.ptr, out.size // 2))
        return out

    def view(self, first, count):
        """polys [first, first + count) as a block of their own (first even: blocks are 16-byte aligned for every N >= 8 anyway)"""
        v = object.__new__(SmallPoly)
        v.ring, v.npoly, v.N, v._block, v.ptr = self.ring, int(count), self.N, self._block, self.ptr + 4 * first * self.N
        return v


class UniformSampler:
    """ring.UniformSampler / ringqp.UniformSampler: uniform residues under the limbs of ringQ and, for QP polys, of ringP (rows LQ, LQ + 1, ...)"""

    def __init__(self, prng, ring, ringP=None, conjugate_invariant=False):
        rings_ok("UniformSampler", ring, ringP, conjugate_invariant)
        self.prng, self.ring, self.ringP = prng, ring, ringP

    def read_rows(self, ring, ptr, out_rows, npoly, call, poly0=0, row0=0):
        """limbs 0..ring.level of npoly polys at a stride of out_rows rows per poly, from substreams (call, poly0 + poly, row0 + limb, .)"""
        _check(lib().rh_sample_uniform(ring._h, ring.level, self.prng._state, call, poly0, row0, ptr, out_rows, npoly))

    def Read(self, polQ, polP=None, call=None, poly0=0):
        """fills the DevicePoly batch polQ (and polP under ringP) at their own levels; one call counter value for the whole Read"""
        call = self.prng.next_call() if call is None else call
        self.read_rows(self.ring.AtLevel(polQ.limbs - 1), polQ.ptr, polQ.limbs, polQ.npoly, call, poly0, 0)
        if polP is not None:
            if self.ringP is None:
                raise RingHipError("UniformSampler: built without ringP")
            self.read_rows(self.ringP.AtLevel(polP.limbs - 1), polP.ptr, polP.limbs, polP.npoly, call, poly0, polQ.limbs)
        return call

    def ReadNew(self, npoly=1):
        p = self.ring.NewPoly(npoly)
        self.Read(p)
        return p


def gaussian_table(sigma, bound):
    """T[k] = floor(P(|x| <= k) 2^63), k = 0 .. top, for |x| = floor(|z| sigma + 0.5), z standard normal conditioned on |z| sigma <= bound:
    P(|x| <= k) = erf(min(k + 1/2, bound) / (sigma sqrt 2)) / erf(bound / (sigma sqrt 2)), at 256 bits.  top = ceil(bound - 1/2) is the largest
    magnitude the reference reaches: floor(bound), or floor(bound) + 1 when the bound's fraction is above one half (|z| sigma = 19.6 <= 19.7
    rounds to 20).  The last entry is 2^63 either way, so the magnitude never exceeds top."""
    import math
    import mpmath
    if not (sigma > 0 and bound > 0):
        raise RingHipError("GaussianSampler: sigma and bound must be positive")
    top = math.ceil(bound - 0.5)
    if int(bound) >= 1024 or top >= 1024:
        raise RingHipError("GaussianSampler: magnitudes up to %d, floor(bound) >= 1024 or next to it: the big-norm sampler (ring/sampler_gaussian.go:99-153) "
                           "is not built" % top)
    with mpmath.workprec(256):
        s, b = mpmath.mpf(sigma) * mpmath.sqrt(2), mpmath.mpf(bound)
        whole = mpmath.erf(b / s)
        return [int(mpmath.floor(mpmath.erf(min(mpmath.mpf(k) + mpmath.mpf(1) / 2, b) / s) / whole * (1 << 63))) for k in range(top + 1)]


class GaussianSampler:
    """ring.GaussianSampler for ring.DiscreteGaussian{Sigma, Bound}: int32 (npoly, N) signed coefficients"""

    def __init__(self, prng, ring, sigma=3.2, bound=19, conjugate_invariant=False):
        rings_ok("GaussianSampler", ring, None, conjugate_invariant)
        self.prng, self.ring, self.sigma, self.bound = prng, ring, float(sigma), float(bound)
        self.table = gaussian_table(sigma, bound)
        self._table = DevicePoly(ring.AtLevel(0), (len(self.table) + ring.N - 1) // ring.N, 1)       # whole rows of N words
        buf = np.zeros(self._table.words, dtype=np.uint64)
        buf[:len(self.table)] = self.table
        _check(lib().rh_dev_upload(ring._h, self._table.ptr, buf.ctypes.data_as(U64P), buf.size))

    def Read(self, out, call=None, poly0=0):
        call = self.prng.next_call() if call is None else call
        _check(lib().rh_sample_gaussian(self.ring._h, self.prng._state, call, poly0, self._table.ptr, len(self.table), out.ptr, out.npoly))
        return call

    def ReadNew(self, npoly=1):
        out = SmallPoly(self.ring, npoly)
        self.Read(out)
        return out


def ternary_threshold(P):
    """floor(P 2^63) for a density 0 <= P <= 1, exact on the float's own value"""
    from fractions import Fraction
    f = Fraction(P)
    if not 0 <= f <= 1:
        raise RingHipError("TernarySampler: the density P must lie in [0, 1]")
    return int(f * (1 << 63))


def ternary_hamming_weight(N, H, rng=None):
    """ring.Ternary{H}: exactly H non-zero coefficients of random sign at positions chosen by a partial Fisher-Yates shuffle, on the host with
    `secrets` (a one-off per secret key).  rng: an object with randbelow (tests pass a seeded one)."""
    rng = secrets if rng is None else rng
    if not 0 <= H <= N:
        raise RingHipError("TernarySampler: the Hamming weight must lie in [0, N]")
    idx = list(range(N))
    out = np.zeros(N, dtype=np.int32)
    for i in range(H):
        j = i + rng.randbelow(N - i)
        idx[i], idx[j] = idx[j], idx[i]
        out[idx[i]] = 1 - 2 * rng.randbelow(2)
    return out


class TernarySampler:
    """ring.TernarySampler for ring.Ternary{P} (on the device) or ring.Ternary{H} (on the host, uploaded): int32 (npoly, N)"""

    def __init__(self, prng, ring, P=None, H=None, conjugate_invariant=False):
        rings_ok("TernarySampler", ring, None, conjugate_invariant)
        if (P is None) == (H is None):
            raise RingHipError("TernarySampler: give the density P or the Hamming weight H, one of them")
        self.prng, self.ring, self.P, self.H = prng, ring, P, H
        self.threshold = ternary_threshold(P) if P is not None else None

    def Read(self, out, call=None, poly0=0):
        if self.H is not None:
            out.upload(np.stack([ternary_hamming_weight(self.ring.N, self.H) for _ in range(out.npoly)]))
            return None
        call = self.prng.next_call() if call is None else call
        _check(lib().rh_sample_ternary(self.ring._h, self.prng._state, call, poly0, self.threshold, out.ptr, out.npoly))
        return call

    def ReadNew(self, npoly=1):
        if self.H is not None:
            return SmallPoly.from_numpy(self.ring, np.stack([ternary_hamming_weight(self.ring.N, self.H) for _ in range(npoly)]))
        out = SmallPoly(self.ring, npoly)
        self.Read(out)
        return out


def lift_small(ringQ, ringP, small, outQ, outP=None, accumulate=False):
    """int32 coefficients -> residues under every limb of outQ (and of outP under ringP): x >= 0 ? x : q - |x|, what Read +
    ExtendBasisSmallNormAndCenter produce; accumulate: ReadAndAdd, out = CRed(out + lift).  outQ / outP: DevicePoly batches of small.npoly polys.
    Per coefficient, so a conjugate-invariant ring is served like a standard one (nothing builds on its refusal)."""
    rings_ok("lift_small", ringQ, ringP if outP is not None else None, conjugate_invariant=True)
    if outQ.npoly != small.npoly or (outP is not None and outP.npoly != small.npoly):
        raise RingHipError("lift_small: the blocks hold different numbers of polys")
    _check(lib().rh_small_lift(ringQ._h, ringP._h if outP is not None else None, outQ.limbs - 1, outP.limbs - 1 if outP is not None else -1, small.ptr,
                               outQ.ptr, outQ.limbs, outP.ptr if outP is not None else None, outP.limbs if outP is not None else 0, small.npoly,
                               1 if accumulate else 0))

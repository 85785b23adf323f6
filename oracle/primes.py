"""Modulus chains of other widths than the 61-bit test primes: the reference's prime generators restated over the oracle's primality
test (orc_is_prime).  TEST INFRASTRUCTURE ONLY.

NTTFriendlyPrimesGenerator (ring/primes.go:62-290): candidates 2^bits + 1 +- k * NthRoot, upstream, downstream or alternating, each
direction stopping when |log2(candidate) - bits| >= 0.5.  GenModuli (core/rlwe/params.go:902-950): 61-bit sizes are drawn downstream,
all others alternating, and the primes of one size are handed out in order, Q before P."""
import json
import math
import os

from . import ring_oracle as orc

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_U64_MAX = (1 << 64) - 1


def is_prime(x):
    return bool(orc.lib().orc_is_prime(int(x)))


class PrimesExhausted(ValueError):
    pass


class NTTFriendlyPrimes:
    """ring.NTTFriendlyPrimesGenerator: primes = 1 mod nthroot around 2^bits (NewNTTFriendlyPrimesGenerator, :71-97)"""

    def __init__(self, bits, nthroot):
        self.size, self.nthroot = float(bits), int(nthroot)
        self.next = (1 << bits) + 1
        self.prev = (1 << bits) + 1
        self.check_next = self.next <= _U64_MAX - self.nthroot
        self.check_prev = self.prev >= self.nthroot
        self.prev -= self.nthroot

    def _next_ok(self, c):
        return math.log2(float(c)) - self.size < 0.5 and c <= _U64_MAX - self.nthroot

    def _prev_ok(self, c):
        return self.size - math.log2(float(c)) < 0.5 and c >= self.nthroot

    def upstream(self):
        """NextUpstreamPrime (:141-172)"""
        c = self.next
        while self.check_next:
            if not self._next_ok(c):
                self.check_next = False
                break
            if is_prime(c):
                self.next = c + self.nthroot
                return c
            c += self.nthroot
        raise PrimesExhausted("upstream primes of %d bits = 1 mod %d exhausted" % (self.size, self.nthroot))

    def downstream(self):
        """NextDownstreamPrime (:175-207)"""
        c = self.prev
        while self.check_prev:
            if not self._prev_ok(c):
                self.check_prev = False
                break
            if is_prime(c):
                self.prev = c - self.nthroot
                return c
            c -= self.nthroot
        raise PrimesExhausted("downstream primes of %d bits = 1 mod %d exhausted" % (self.size, self.nthroot))

    def alternating(self):
        """NextAlternatingPrime (:210-290): one upstream candidate, then one downstream candidate, per step"""
        nxt, prv = self.next, self.prev
        while self.check_next or self.check_prev:
            if self.check_next:
                if not self._next_ok(nxt):
                    self.check_next = False
                elif is_prime(nxt):
                    self.next, self.prev = nxt + self.nthroot, prv
                    return nxt
                else:
                    nxt += self.nthroot
            if self.check_prev:
                if not self._prev_ok(prv):
                    self.check_prev = False
                elif is_prime(prv):
                    self.next, self.prev = nxt, prv - self.nthroot
                    return prv
                else:
                    prv -= self.nthroot
        raise PrimesExhausted("primes of %d bits = 1 mod %d exhausted in both directions" % (self.size, self.nthroot))


def gen_moduli(log_nthroot, logQ, logP):
    """GenModuli (core/rlwe/params.go:902-950) -> (Q, P)"""
    count = {}
    for b in list(logQ) + list(logP):
        count[b] = count.get(b, 0) + 1
    pool = {}
    for b, n in count.items():
        g = NTTFriendlyPrimes(b, 1 << log_nthroot)
        step = g.downstream if b == 61 else g.alternating
        pool[b] = [step() for _ in range(n)]
    Q = [pool[b].pop(0) for b in logQ]
    P = [pool[b].pop(0) for b in logP]
    return Q, P


def gen_moduli_3n(N, logQ, logP):
    """3N-friendly chain: for each size, the primes = 1 mod 3N upward from 2^bits in the stepping rule of Find3NFriendlyPrime
    (ring/primes.go:15-60, the rule tests/test_oracle_ntt3n.find_prime_3n uses), handed out in order, Q before P"""
    count = {}
    for b in list(logQ) + list(logP):
        count[b] = count.get(b, 0) + 1
    step = 3 * N
    pool = {}
    for b, n in count.items():
        c, got = ((1 << b) // step + 1) * step + 1, []
        while len(got) < n:
            if is_prime(c):
                got.append(c)
            c += step
        pool[b] = got
    return [pool[b].pop(0) for b in logQ], [pool[b].pop(0) for b in logP]


def ckks_test_moduli():
    """tests/golden/ckks_test_moduli.json: the chains the reference's CKKS tests spell out (schemes/ckks/test_utils.go:132-171)"""
    with open(os.path.join(_ROOT, "tests", "golden", "ckks_test_moduli.json")) as f:
        return json.load(f)


def overflow_margin(mods):
    """QiOverflowMargin / PiOverflowMargin (core/rlwe/params.go:646-660): int(2^64 / float64(max q))"""
    return int(2.0 ** 64 / float(max(mods)))


# ---- the named chains of the mixed-width tests ------------------------------------------------------------------------------------
def chain(name, logN=15):
    """(Q, P) of a named chain for standard rings of degree 2^logN (NthRoot = 2^(logN+1)):
    C45 / C90   the Prec45 / Prec90 fixtures (every prime = 1 mod 2^16: logN <= 15)
    B40         GenModuli(logN+1, [50]+[40]*7, [60])  (schemes/ckks/ckks_benchmarks_test.go:27)
    SPLIT       GenModuli(logN+1, [55]+[45]*9, [61, 61]): QiOverF = 255, PiOverF = 4, five digits
    SPLIT12     GenModuli(logN+1, [55]+[45]*23, [61, 61]): the same margins, twelve digits -- enough lazy terms in [0, ~1.1p) for
                their sum to pass 2^64 = 8p on a few percent of the coefficients when the P accumulator is given the Q margin
    SMALL       GenModuli(logN+1, [30]*4, [33, 32]): margins above 2^31 (Q) and just below (P)
    WIDE        GenModuli(logN+1, [61, 36, 20, 58, 45], [40]): digits wider than P, upstream and downstream primes (logN <= 13)"""
    if name in ("C45", "C90"):
        assert logN <= 15
        c = ckks_test_moduli()["prec45" if name == "C45" else "prec90"]
        return list(c["Q"]), list(c["P"])
    spec = {"B40": ([50] + [40] * 7, [60]), "SPLIT": ([55] + [45] * 9, [61, 61]), "SPLIT12": ([55] + [45] * 23, [61, 61]),
            "SMALL": ([30] * 4, [33, 32]),
            "WIDE": ([61, 36, 20, 58, 45], [40])}[name]
    return gen_moduli(logN + 1, *spec)

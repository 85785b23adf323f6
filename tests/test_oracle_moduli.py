"""CPU: the mixed-width modulus chains (oracle/primes.py, tests/golden/ckks_test_moduli.json) and the oracle at those widths.
The GPU tests of tests/test_gpu_moduli.py judge the kernels on these chains against the oracle; these tests pin the chains to the
reference's generator and the oracle to big-integer arithmetic first, and show that the margin-swap the GPU tests guard against
changes the oracle's result."""
import math

import numpy as np
import pytest

from test_oracle_bext import centered_randoms, prod, rns

NAMED = ["C45", "C90", "B40", "SPLIT", "SPLIT12", "SMALL", "WIDE"]


@pytest.fixture(scope="module")
def primes(oracle):
    from oracle import primes as pr
    return pr


def test_fixture_chains_are_ntt_friendly_primes_of_their_nominal_size(primes):
    c = primes.ckks_test_moduli()
    assert "test_utils.go" in c["source"]
    for name in ("prec45", "prec90"):
        Q, P = c[name]["Q"], c[name]["P"]
        assert len(Q) == len(c[name]["LogQ"]) and len(P) == len(c[name]["LogP"])
        assert len(set(Q + P)) == len(Q + P)
        for q, bits in zip(Q + P, c[name]["LogQ"] + c[name]["LogP"]):
            assert bits in (45, 55, 60)
            assert primes.is_prime(q), q
            assert q % (1 << 16) == 1, q                           # NTT-friendly for standard rings up to N = 2^15
            assert abs(math.log2(q) - bits) < 0.5, (q, bits)       # the generator's stop rule (ring/primes.go:150, 184)
    assert len(c["prec45"]["Q"]) == 7 and len(c["prec90"]["Q"]) == 12


@pytest.mark.parametrize("bits,log_nthroot", [(20, 14), (30, 17), (33, 17), (45, 16), (55, 16), (60, 18), (61, 17)])
@pytest.mark.parametrize("direction", ["upstream", "downstream", "alternating"])
def test_generator_properties(primes, bits, log_nthroot, direction):
    nth = 1 << log_nthroot
    g = primes.NTTFriendlyPrimes(bits, nth)
    got = []
    for _ in range(6):
        try:
            got.append(getattr(g, direction)())
        except primes.PrimesExhausted:
            break
    assert len(got) >= 2
    assert len(set(got)) == len(got)
    for q in got:
        assert primes.is_prime(q) and q % nth == 1
        assert abs(math.log2(q) - bits) < 0.5
        if direction == "upstream":
            assert q > 1 << bits
        elif direction == "downstream":
            assert q < 1 << bits
    if direction != "alternating":                                 # one direction: the primes come in order
        assert got == sorted(got, reverse=direction == "downstream")
    g2 = primes.NTTFriendlyPrimes(bits, nth)
    assert [getattr(g2, direction)() for _ in got] == got           # deterministic


def test_generator_exhaustion_and_gen_moduli_rules(primes):
    g = primes.NTTFriendlyPrimes(20, 1 << 15)                       # few candidates of 20 bits = 1 mod 2^15: both directions run dry
    seen = []
    with pytest.raises(primes.PrimesExhausted):
        for _ in range(100):
            seen.append(g.alternating())
    assert all(abs(math.log2(q) - 20) < 0.5 for q in seen)
    Q, P = primes.gen_moduli(14, [61, 61, 40], [61, 40])
    assert all(q < 1 << 61 for q in Q[:2] + P[:1])                  # 61-bit sizes go downstream only (core/rlwe/params.go:930)
    assert Q[0] > Q[1] > P[0]                                       # primes of one size handed out in order, Q before P
    g = primes.NTTFriendlyPrimes(40, 1 << 14)
    first = [g.alternating() for _ in range(2)]
    assert [Q[2], P[1]] == first


def test_gen_moduli_pins_the_prec45_fixture(primes):
    # the current generator reproduces the first six Q primes and both P primes of the Prec45 comment; its seventh Q prime was written
    # down by an older generator and is not asserted
    c = primes.ckks_test_moduli()["prec45"]
    Q, P = primes.gen_moduli(16, [55] + [45] * 5, [55, 55])
    assert Q == c["Q"][:6]
    assert P == c["P"]


@pytest.mark.parametrize("name", NAMED)
def test_named_chains(primes, name):
    for logN in {"C45": (12, 15), "C90": (12, 15), "B40": (12, 17), "SPLIT": (12, 15), "SPLIT12": (12, 14), "SMALL": (12, 16), "WIDE": (12, 13)}[name]:
        Q, P = primes.chain(name, logN)
        assert len(set(Q + P)) == len(Q + P)
        for q in Q + P:
            assert primes.is_prime(q) and q % (2 << logN) == 1 and q < 1 << 62
    Q, P = primes.chain(name, 13)
    qm, pm = primes.overflow_margin(Q) >> 1, primes.overflow_margin(P) >> 1
    if name.startswith("SPLIT"):                                    # unequal Reduce periods: QiOverF ~ 255, PiOverF = 4
        assert qm in (255, 256) and pm == 4
        assert (len(Q) + len(P) - 1) // len(P) == (5 if name == "SPLIT" else 12)
    if name == "SMALL":
        assert primes.overflow_margin(Q) > 2 ** 31                  # the quotient that does not fit an int
        assert primes.overflow_margin(primes.chain(name, 16)[1]) < 2 ** 31     # the upstream 33-bit P prime: a margin just below
    if name == "WIDE":
        assert min(q.bit_length() for q in Q) <= 21 and max(Q) > 1 << 60 and qm != pm


def test_gen_moduli_3n(primes):
    N = 3 << 13
    Q, P = primes.gen_moduli_3n(N, [31, 31, 30], [31])
    assert Q[0] < Q[1] and Q[1] < P[0]
    for q in Q + P:
        assert primes.is_prime(q) and q % (3 * N) == 1
    from test_oracle_ntt3n import find_prime_3n
    assert Q[0] == find_prime_3n(N, 31) and Q[2] == find_prime_3n(N, 30)


def _negacyclic_eval(a, q, psi, logN):
    N = 1 << logN
    out = []
    for i in range(N):
        x = pow(psi, 2 * int(format(i, "0%db" % logN)[::-1], 2) + 1, q)
        acc = 0
        for c in reversed(a):
            acc = (acc * x + c) % q
        out.append(acc)
    return out


@pytest.mark.parametrize("name", ["C45", "SMALL", "WIDE"])
@pytest.mark.parametrize("logN", [4, 6])
def test_oracle_transforms_vs_bigint_dft(oracle, primes, name, logN):
    # the forward output at bit-reversed slot i is f(psi^(2 bitrev(i) + 1)) (ring/ntt.go), on every prime of the chain
    N = 1 << logN
    Q, P = primes.chain(name, 12)
    rng = np.random.default_rng(logN * 7 + len(Q))
    for q in Q + P:
        sr = oracle.SubRingConsts(N, q)
        a = [int(x) for x in rng.integers(0, q, size=N, dtype=np.uint64)]
        a[0], a[1] = q - 1, 0
        psi = pow(sr.primitive_root, (q - 1) // (2 * N), q)
        y = oracle.ntt(a, sr)
        assert [int(v) for v in y] == _negacyclic_eval(a, q, psi, logN), q
        yl = oracle.ntt(a, sr, lazy=True)
        assert int(yl.max()) <= 6 * q - 2 and np.array_equal(yl % np.uint64(q), y)
        assert [int(v) for v in oracle.intt(y, sr)] == a
        assert [int(v) % q for v in oracle.intt(yl % np.uint64(q), sr, lazy=True)] == a


@pytest.mark.parametrize("name", ["WIDE", "SPLIT"])
def test_oracle_basis_extension_vs_bigint(oracle, primes, name):
    Q, P = primes.chain(name, 12)
    rng = np.random.default_rng(len(Q) * 13)
    n = 64
    vals = centered_randoms(rng, prod(Q), n)
    pp = oracle.modup_centered(rns(vals, Q), Q, P)
    for j, p in enumerate(P):
        assert [int(x) % p for x in pp[j]] == [v % p for v in vals]
    vals = centered_randoms(rng, prod(P), n)
    pq = oracle.modup_centered(rns(vals, P), P, Q)
    for i, q in enumerate(Q):
        assert [int(x) % q for x in pq[i]] == [v % q for v in vals]
    vals = centered_randoms(rng, prod(Q) * prod(P), n)
    out = oracle.moddown_qp_to_q(rns(vals, Q), rns(vals, P), Q, P)
    Pb = prod(P)
    for i, q in enumerate(Q):
        assert [int(x) for x in out[i]] == [((2 * v + Pb) // (2 * Pb)) % q for v in vals]


def _split_case(oracle, primes, N, seed, name="SPLIT"):
    Q, P = primes.chain(name, 13)
    rng = np.random.default_rng(seed)
    levelQ, levelP = len(Q) - 1, len(P) - 1
    beta = (levelQ + levelP + 1) // (levelP + 1)
    u = lambda m: rng.integers(0, m, size=N, dtype=np.uint64)
    cx = np.stack([u(q) for q in Q])
    evkQ = np.stack([np.stack([np.stack([u(q) for q in Q]) for _ in range(2)]) for _ in range(beta)])
    evkP = np.stack([np.stack([np.stack([u(p) for p in P]) for _ in range(2)]) for _ in range(beta)])
    return Q, P, levelQ, levelP, cx, evkQ, evkP


def test_oracle_gadget_product_on_split_vs_bigint(oracle, primes):
    # compose.gadget_product == the canonical big-integer form of the same product (every intermediate reduced), on unequal margins
    from oracle import compose
    from test_gpu_keyswitch import _generic_gadget_product
    N = 64
    Q, P, levelQ, levelP, cx, evkQ, evkP = _split_case(oracle, primes, N, 5)
    srQ = [oracle.SubRingConsts(N, q) for q in Q]
    srP = [oracle.SubRingConsts(N, p) for p in P]
    fq = lambda x, i: oracle.ntt(x, srQ[i]); iq = lambda x, i: oracle.intt(x, srQ[i])
    fp = lambda x, j: oracle.ntt(x, srP[j]); ip = lambda x, j: oracle.intt(x, srP[j])
    e = _generic_gadget_product(oracle, N, Q, P, levelQ, levelP, cx, evkQ, evkP, fq, iq, fp, ip)
    g = compose.gadget_product(N, Q, P, levelQ, levelP, cx, evkQ, evkP)
    assert np.array_equal(g[0], e[0]) and np.array_equal(g[1], e[1])


def test_swapped_reduce_margins_change_the_result(oracle, primes):
    # the sensitivity the GPU tests rely on.  A Montgomery product MRedLazy(x, y) lies in [0, p + xy/2^64), ~0.53p on average, so the P
    # accumulator (p ~ 2^61) passes 2^64 = 8p only after some fifteen terms.  With the five digits of SPLIT the swap (the Q period 255 given
    # to the P accumulator) changes nothing; with the twelve of SPLIT12 about one coefficient in twenty wraps and the result differs.
    from oracle import compose
    N = 256
    for name, differs in (("SPLIT", False), ("SPLIT12", True)):
        Q, P, levelQ, levelP, cx, evkQ, evkP = _split_case(oracle, primes, N, 11, name)
        qm, pm = primes.overflow_margin(Q) >> 1, primes.overflow_margin(P) >> 1
        assert qm > 12 > pm
        good = compose.gadget_product(N, Q, P, levelQ, levelP, cx, evkQ, evkP)
        same = compose.gadget_product(N, Q, P, levelQ, levelP, cx, evkQ, evkP, qiof=qm, piof=pm)
        bad = compose.gadget_product(N, Q, P, levelQ, levelP, cx, evkQ, evkP, qiof=pm, piof=qm)
        assert all(np.array_equal(a, b) for a, b in zip(good, same))
        assert (not all(np.array_equal(a, b) for a, b in zip(good, bad))) == differs, name
    # the single-P form on the same widths: a lower-level chain with one P modulus, margins swapped
    Qs, Ps = Q[:4], P[:1]
    dpl = [-(-q.bit_length() // 15) for q in Qs]
    rows = sum(dpl)
    rng = np.random.default_rng(3)
    u = lambda m: rng.integers(0, m, size=N, dtype=np.uint64)
    kq = np.stack([np.stack([np.stack([u(q) for q in Qs]) for _ in range(2)]) for _ in range(rows)])
    kp = np.stack([np.stack([np.stack([u(p) for p in Ps]) for _ in range(2)]) for _ in range(rows)])
    x = np.stack([u(q) for q in Qs])
    qm1, pm1 = primes.overflow_margin(Qs) >> 1, primes.overflow_margin(Ps) >> 1
    good = compose.gadget_product_single_p(N, Qs, Ps, 3, 0, x, True, 15, dpl, kq, kp)
    bad = compose.gadget_product_single_p(N, Qs, Ps, 3, 0, x, True, 15, dpl, kq, kp, qiof=pm1, piof=qm1)
    assert not all(np.array_equal(a, b) for a, b in zip(good, bad))

"""CPU: core/rlwe/ring_packing.go restated over the oracle pieces (tests/ring_packing_restatement.py) pinned to DECRYPTION under real keys, with the
bounds of the reference's own tests on log2 of the standard deviation of the error (core/rlwe/ring_packing_test.go): Split log(N/2) + 1 (:125-126),
Merge logN + 1 (:176), Expand / Extract logN + 6 (the full expansion measured against LogN + bits.Len64(17) + 1, :192-240), Pack / Repack with
zeroed garbage logN + 5 (:376), Extract -> permute -> Repack logN + 5 (:379-478).  tests/test_gpu_ring_packing.py compares the device path with the
same restatement bit for bit, on the cases below.

Chains (tests/test_rlwe_oracle.py): TAIL (N = 32, 7 | 4 limbs, and N = 16 over the same moduli for the ring switches) and REF (N = 2^10, and 2^9).
Messages carry the tag "rp"; the Galois keys are t.key's; the small secrets and the ring-switching keys (GenRingSwitchingKeys,
ring_packing_keys.go:106-109: rr.gadget_key between sk_N and the small secret at the even positions) are made here.

Measured log2 of the standard deviation of the error, the largest per family (bound in brackets): Expand TAIL 5.74 [11], REF 8.65 [16];
Pack TAIL 6.53 [10], REF 9.13 [15]; Split TAIL 2.79 [5], REF 2.71 [10]; Merge TAIL 2.73 [6], REF 3.06 [11]; Extract -> permute -> Repack on TAIL
7.09 [10] with one degree and 5.25 [10] across two; Extract alone 5.74 [11].  The control (Expand with the table of X^(2^i)) misses its bound by
more than 10 bits."""
import functools
import random

import numpy as np
import pytest

import ring_packing_restatement as rp
import rlwe_restatement as rr
import test_rlwe_oracle as t

_ids = t._ids


def log_n(N):
    return N.bit_length() - 1


# ---- keys ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def secret(name, logN):
    """the chain's own secret at its own degree, a fresh ternary one below"""
    N = t.chain(name)[0]
    if 1 << logN == N:
        return t.secrets(name)[0]
    return rr.Secret.sample(random.Random("sk %s logN %d" % (name, logN)), 1 << logN)


def embedded(sk, N):
    """the secret of a smaller ring in the ring of degree N: Y = X^(N/n)"""
    out = [0] * N
    out[::N // sk.N] = sk.coeffs
    return rr.Secret(N, out)


def key_args(name, setting):
    N, Q, P, levels = t.chain(name)
    pw2, pc = setting
    return Q, P[:pc], levels[0], pc - 1, pw2


@functools.lru_cache(maxsize=None)
def switching_key(name, setting, logNIn, logNOut):
    """RingSwitchingKeys[logNIn][logNOut], made in the larger ring (ring_packing_keys.go:106-109)"""
    big = 1 << max(logNIn, logNOut)
    rnd = random.Random("rsk %s %s %d %d" % (name, setting, logNIn, logNOut))
    return rr.gadget_key(rnd, embedded(secret(name, logNIn), big), embedded(secret(name, logNOut), big), *key_args(name, setting))


@functools.lru_cache(maxsize=None)
def galois_key(name, setting, logN, g):
    if 1 << logN == t.chain(name)[0]:
        return t.key(name, setting, "galois", g)
    rnd = random.Random("%s %s galois %d logN %d" % (name, setting, g, logN))
    return rr.galois_key(rnd, secret(name, logN), g, *key_args(name, setting))


def galois_keys(name, setting, logN, galEls):
    return {g: galois_key(name, setting, logN, g) for g in galEls}


def message(name, tag, N, size=1 << 30):
    rnd = random.Random("m %s %s %d" % (name, tag, N))
    return [rnd.randrange(-size, size + 1) for _ in range(N)]


def encrypt(name, tag, logN, level, m):
    Q = t.chain(name)[1]
    return rr.encrypt(random.Random("ct %s %s %d %d" % (name, tag, logN, level)), secret(name, logN), m, Q, level)[0]


def error(name, logN, level, ct, want):
    Q = t.chain(name)[1]
    return rr.log2_std(rr.centered_diff(rr.phase(list(ct), secret(name, logN), Q), want, rr.prod(Q[:level + 1])))


def settings(name, setting):
    N, Q, P, levels = t.chain(name)
    return N, Q, P[:setting[1]], levels


# ---- Expand -------------------------------------------------------------------------------------------------------------------------------
EXPAND = [("TAIL", (0, 4), 0, 0), ("TAIL", (0, 4), 1, 2), ("TAIL", (16, 1), 0, 1), ("REF", (0, 2), 0, 7), ("REF", (0, 2), 1, 8)]
_eid = lambda c: "%s-pw%d-p%d-l%d-gap%d" % (c[0], c[1][0], c[1][1], c[2], c[3])


@functools.lru_cache(maxsize=None)
def expand_case(name, setting, li, logGap, tag="rp"):
    """(m, ct, {index: restated output}): shared with the GPU tests"""
    N, Q, P, levels = settings(name, setting)
    level = levels[li]
    m, ct, _ = t.fresh(name, tag, level)
    keys = galois_keys(name, setting, log_n(N), rp.galois_elements_for_expand(N, log_n(N)))
    return m, ct, rp.expand(N, Q, P, ct, logGap, keys)


def one_coefficient(N, x):
    return [x] + [0] * (N - 1)


@pytest.mark.parametrize("case", EXPAND, ids=_eid)
def test_expand_decrypts(oracle, case):
    """every output has m[j] at coefficient 0 and noise elsewhere"""
    name, setting, li, logGap = case
    N, Q, P, levels = settings(name, setting)
    m, ct, outs = expand_case(*case)
    assert sorted(outs) == list(range(0, N, 1 << logGap))
    worst = max(error(name, log_n(N), levels[li], outs[j], one_coefficient(N, m[j])) for j in outs)
    t.report("expand", name, setting, levels[li], worst, log_n(N) + 6)
    assert worst <= log_n(N) + 6


def test_control_expand_with_the_wrong_table_does_not_decrypt(oracle):
    """X^(2^i) in the place of X^(-2^i): the odd halves are moved up instead of down"""
    name, setting, li, logGap = EXPAND[0]
    N, Q, P, levels = settings(name, setting)
    level = levels[li]
    m, ct, _ = t.fresh(name, "rp", level)
    keys = galois_keys(name, setting, log_n(N), rp.galois_elements_for_expand(N, log_n(N)))
    outs = rp.expand(N, Q, P, ct, logGap, keys, xinv=rp.gen_xpow2_ntt(N, Q[:level + 1], log_n(N), False))
    worst = max(error(name, log_n(N), level, outs[j], one_coefficient(N, m[j])) for j in outs if j)
    assert worst > log_n(N) + 6 + 10


# ---- Pack ---------------------------------------------------------------------------------------------------------------------------------
PACK = [("TAIL", (0, 4), tuple(range(32))), ("TAIL", (0, 4), tuple(range(0, 32, 3))), ("TAIL", (16, 1), (0, 1, 2, 5, 7, 12)),
        ("REF", (0, 2), tuple(range(0, 1024, 128))), ("REF", (0, 2), (0, 3, 6, 9, 12))]
_pid = lambda c: "%s-pw%d-p%d-%dkeys-last%d" % (c[0], c[1][0], c[1][1], len(c[2]), c[2][-1])


def pack_inputs(name, logN, level, keys, tag="rp"):
    """(m, {j: encryption of m X^-j})"""
    N = 1 << logN
    m = message(name, tag, N)
    return m, {j: encrypt(name, "%s pack %d" % (tag, j), logN, level, rr.monomial_mul(m, 2 * N - j)) for j in keys}


@functools.lru_cache(maxsize=None)
def pack_case(name, setting, keys, li=0):
    """(m, the input ciphertexts, restated Pack(cts, logN, true)): shared with the GPU tests"""
    N, Q, P, levels = settings(name, setting)
    level = levels[li]
    m, cts = pack_inputs(name, log_n(N), level, keys)
    gk = galois_keys(name, setting, log_n(N), rp.galois_elements_for_pack(N, log_n(N)))
    work = {j: [x.copy() for x in c] for j, c in cts.items()}
    return m, cts, rp.pack(N, Q, P, work, log_n(N), True, gk)


def packed(m, keys):
    return [x if j in keys else 0 for j, x in enumerate(m)]


@pytest.mark.parametrize("case", PACK, ids=_pid)
def test_pack_decrypts(oracle, case):
    name, setting, keys = case
    N, Q, P, levels = settings(name, setting)
    for li in (0, 1):
        m, _, out = pack_case(name, setting, keys, li)
        got = error(name, log_n(N), levels[li], out, packed(m, set(keys)))
        t.report("pack", name, setting, levels[li], got, log_n(N) + 5)
        assert got <= log_n(N) + 5


def test_pack_refusals_and_plan(oracle, rh):
    name, setting, keys = PACK[2]
    N, Q, P, levels = settings(name, setting)
    with pytest.raises(rp.NoCiphertext, match=r"len\(cts\) = 0"):
        rp.pack(N, Q, P, {}, 5, True, {})
    _, cts, _ = pack_case(name, setting, keys)
    with pytest.raises(rp.NoCiphertext, match="gaps between ciphertexts is smaller than inputLogGap > N"):
        rp.pack(N, Q, P, {0: cts[0], 1: cts[1]}, 0, True, {})                 # logStart = logEnd
    with pytest.raises(rh.RingHipError, match="gaps between ciphertexts is smaller than inputLogGap > N"):
        rh.rlwe.pack_plan(N, [0, 1], 0, True)
    # the module functions are the reference's formulas
    for n in (16, 32, 1024):
        assert rh.rlwe.GaloisElementsForExpand(n, log_n(n)) == rp.galois_elements_for_expand(n, log_n(n))
        for lg in (0, 3, log_n(n)):
            assert rh.rlwe.GaloisElementsForPack(n, lg) == rp.galois_elements_for_pack(n, lg)
    # the plan names every ciphertext once per level at most, and ends where the restatement's map ends
    for ks in (keys, tuple(range(0, 32, 3)), (5,), (1, 3)):
        for zero in (True, False):
            try:
                logStart, logEnd, plan, slot = rh.rlwe.pack_plan(N, list(ks), 5, zero)
            except rh.RingHipError:
                continue
            for g, xi, entries in plan:
                used = [s for mode, a, b in entries for s in ((a, b) if mode == rh.rlwe.MODE_AB else (a,))]
                assert len(used) == len(set(used))
            assert slot is None or 0 <= slot < len(ks)


# ---- Split, Merge -------------------------------------------------------------------------------------------------------------------------
SPLIT = [("TAIL", (0, 4)), ("REF", (0, 2)), ("REF", (16, 1))]


@functools.lru_cache(maxsize=None)
def split_case(name, setting, li, tag="rp"):
    N, Q, P, levels = settings(name, setting)
    m, ct, _ = t.fresh(name, tag, levels[li])
    return m, ct, rp.split(N, Q, P, ct, switching_key(name, setting, log_n(N), log_n(N) - 1))


@functools.lru_cache(maxsize=None)
def merge_case(name, setting, li, tag="rp"):
    N, Q, P, levels = settings(name, setting)
    level, lh = levels[li], log_n(N) - 1
    me, mo = message(name, tag + " even", N // 2), message(name, tag + " odd", N // 2)
    even, odd = encrypt(name, tag + " even", lh, level, me), encrypt(name, tag + " odd", lh, level, mo)
    return (me, mo), (even, odd), rp.merge(N, Q, P, even, odd, switching_key(name, setting, lh, lh + 1))


@pytest.mark.parametrize("shape", SPLIT, ids=_ids)
def test_split_and_merge_decrypt(oracle, shape):
    name, setting = shape
    N, Q, P, levels = settings(name, setting)
    lh = log_n(N) - 1
    for li in (0, 1):
        m, ct, (even, odd) = split_case(name, setting, li)
        for half, want in ((even, m[0::2]), (odd, m[1::2])):
            got = error(name, lh, levels[li], half, want)
            t.report("split", name, setting, levels[li], got, lh + 1)
            assert got <= lh + 1
        (me, mo), _, ctN = merge_case(name, setting, li)
        want = [0] * N
        want[0::2], want[1::2] = me, mo
        got = error(name, lh + 1, levels[li], ctN, want)
        t.report("merge", name, setting, levels[li], got, lh + 2)
        assert got <= lh + 2
    # without an odd half: the even half at the even positions
    (me, _), (even, _), _ = merge_case(name, setting, 0)
    only = rp.merge(N, Q, P, even, None, switching_key(name, setting, lh, lh + 1))
    want = [0] * N
    want[0::2] = me
    assert error(name, lh + 1, levels[0], only, want) <= lh + 2
    with pytest.raises(rp.NoCiphertext, match="ctEvenNHalf cannot be nil"):
        rp.merge(N, Q, P, None, even, None)


def test_split_odd_half_is_the_odd_coefficients(oracle):
    """the device path reads the odd coefficients directly where the reference multiplies by X^-1 and transforms back a second time
    (ring_packing.go:239-241): the same canonical residues"""
    for name, setting in SPLIT[:2]:
        N, Q, P, levels = settings(name, setting)
        for li in (0, 1):
            mods = [int(q) for q in Q[:levels[li] + 1]]
            _, ct, (even, odd) = split_case(name, setting, li)
            tmp = rr.apply_evaluation_key(N, Q, P, ct, switching_key(name, setting, log_n(N), log_n(N) - 1))
            for c in (0, 1):
                coeffs = rr.intt(tmp[c], N, mods)
                assert np.array_equal(rr.ntt(np.ascontiguousarray(coeffs[:, 0::2]), N // 2, mods), even[c])
                assert np.array_equal(rr.ntt(np.ascontiguousarray(coeffs[:, 1::2]), N // 2, mods), odd[c])


# ---- Extract -> permute -> Repack -----------------------------------------------------------------------------------------------------------
def packing_keys(name, setting, min_logN, max_logN):
    N, Q, P, levels = settings(name, setting)
    sw = {}
    for i in range(min_logN, max_logN):
        sw[(i, i + 1)] = switching_key(name, setting, i, i + 1)
        sw[(i + 1, i)] = switching_key(name, setting, i + 1, i)
    n = 1 << min_logN
    return rp.Keys(Q, P, min_logN, max_logN, sw,
                   repack={min_logN: galois_keys(name, setting, min_logN, rp.galois_elements_for_pack(n, min_logN))},
                   extract={min_logN: galois_keys(name, setting, min_logN, rp.galois_elements_for_expand(n, min_logN))})


def chosen(N):
    """half of the indices, shuffled by a seeded generator (ring_packing_test.go:396-408)"""
    idx = list(range(N))
    random.Random("extract %d" % N).shuffle(idx)
    return tuple(sorted(idx[:N // 2]))


EPR = [("TAIL", (0, 4), 4, False, True), ("TAIL", (0, 4), 4, True, False), ("TAIL", (0, 4), 5, False, True), ("TAIL", (0, 4), 5, True, False)]


@functools.lru_cache(maxsize=None)
def extract_case(name, setting, min_logN, naive, tag="rp"):
    N, Q, P, levels = settings(name, setting)
    keys = packing_keys(name, setting, min_logN, log_n(N))
    m, ct, _ = t.fresh(name, tag, levels[0])
    return m, ct, rp.extract(keys, ct, chosen(N), naive)


@functools.lru_cache(maxsize=None)
def extract_repack_case(name, setting, min_logN, extract_naive, repack_naive, tag="rp"):
    """(m, ct, the extracted map, the repacked ciphertext) with x -> x + N/2 mod N between the two: shared with the GPU tests"""
    N, Q, P, levels = settings(name, setting)
    keys = packing_keys(name, setting, min_logN, log_n(N))
    m, ct, cts = extract_case(name, setting, min_logN, extract_naive, tag)
    work = {(i + N // 2) & (N - 1): [x.copy() for x in c] for i, c in cts.items()}
    return m, ct, cts, rp.repack(keys, work, repack_naive)


@pytest.mark.parametrize("case", EPR, ids=lambda c: "%s-min%d-extract%s-repack%s" % (c[0], c[2], "naive" if c[3] else "", "naive" if c[4] else ""))
def test_extract_permute_repack_decrypts(oracle, case):
    name, setting, min_logN, extract_naive, repack_naive = case
    N, Q, P, levels = settings(name, setting)
    m, ct, cts, out = extract_repack_case(*case)
    assert sorted(cts) == list(chosen(N)) and all(c[0].shape[1] == 1 << min_logN for c in cts.values())
    want = [0] * N
    for k0 in chosen(N):
        want[(k0 + N // 2) & (N - 1)] = m[k0]
    got = error(name, log_n(N), levels[0], out, want)
    t.report("extract+repack", name, setting, levels[0], got, log_n(N) + 5)
    assert got <= log_n(N) + 5
    if not extract_naive:                                                 # Extract alone: every output is m[i] at coefficient 0 under the small secret
        worst = max(error(name, min_logN, levels[0], cts[i], one_coefficient(1 << min_logN, m[i])) for i in cts)
        t.report("extract", name, setting, levels[0], worst, log_n(N) + 6)
        assert worst <= log_n(N) + 6


def test_extract_with_one_index_expands_everything(oracle):
    """getMinimumGap of one key leaves logGap = 0 (ring_packing.go:101)"""
    name, setting = "TAIL", (0, 4)
    N, Q, P, levels = settings(name, setting)
    assert rp.get_minimum_gap([7])[1] == 0
    keys = packing_keys(name, setting, 5, 5)
    m, ct, _ = t.fresh(name, "rp", levels[0])
    out = rp.extract(keys, ct, (7,), False)
    assert sorted(out) == [7]
    assert error(name, 5, levels[0], out[7], one_coefficient(N, m[7])) <= 5 + 6

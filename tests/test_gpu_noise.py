"""GPU: the noise meters on the device (matrix-fhe-lattigo_amd/noise.py over csrc/noise.hip).

Every comparison is on exact integers -- the moments of rh_ring_centered_moments against tests/noise_restatement.py's centred CRT, the whole
output of rh_rlwe_gadget_phase against the composed ring calls -- or on floats that come out of the same finishing function on the same
integers: fused against composed against the restatement."""
import ctypes as C
import math
import random

import numpy as np
import pytest

import noise_restatement as nr
import rlwe_restatement as rr
import test_keygen_oracle as tko
import test_rlwe_oracle as tro
from conftest import PI60, QI60
from oracle import primes

pytestmark = pytest.mark.gpu
_CACHE = {}


def _wide(logN):
    return [int(q) for q in primes.chain("WIDE", logN)[0][:3]]                   # 61 / 36 / 20 bits


def rings_for(rh, name):
    """(ringQ view, ringP view or None): allocated one limb wider than the basis measured, so that every block is read at a row stride"""
    if name in _CACHE:
        return _CACHE[name]
    S, CI, M3 = rh.Standard, rh.ConjugateInvariant, rh.Matrix3N
    spec = {
        "n16-l1": (S, 16, QI60[:2], 1, None, 0), "n16-wide": (S, 16, _wide(4) + [QI60[1]], 3, None, 0),
        "n256-l2": (S, 256, QI60[:3], 2, None, 0), "n1024-l1": (S, 1024, QI60[:2], 1, None, 0), "n1024-wide": (S, 1024, _wide(10) + [QI60[1]], 3, None, 0),
        "n1024-l9": (S, 1024, QI60[:10], 9, None, 0), "n256-l17": (S, 256, QI60[:18], 17, None, 0),
        "n256-q25p5": (S, 256, QI60[:26], 25, PI60[:6], 5),
        "3n24-l3": (M3, 24, [int(q) for q in primes.gen_moduli_3n(24, [60, 60, 45, 45], [])[0]], 3, None, 0),
        "ci64-l3": (CI, 64, QI60[:4], 3, None, 0),
    }[name]
    kind, N, Q, lq, P, lp = spec
    rq = rh.Ring(N, Q, kind=kind).AtLevel(lq - 1)
    rp = rh.Ring(N, P, kind=kind).AtLevel(lp - 1) if P else None
    _CACHE[name] = (rq, rp)
    return rq, rp


def patterns(mods, N, rnd):
    """the polys of the issue as lists of N integers in [0, M): zero, -1 everywhere, the two sides of the `>=`, the alternating extreme, one non-zero
    coefficient, uniform (three of them: nine polys, three batches of three)"""
    M = rr.prod(mods)
    h = M >> 1
    one = [0] * N
    one[N // 3] = M - 12345 % M
    alt = [(h - 1) if i % 2 == 0 else (M - (h - 1)) % M for i in range(N)]
    return [[0] * N, [M - 1] * N, [h] * N, [h - 1] * N, alt, one] + [[rnd.randrange(M) for _ in range(N)] for _ in range(3)]


MOMENT_RINGS = ["n16-l1", "n16-wide", "n256-l2", "n1024-wide", "n1024-l9", "n256-l17", "n256-q25p5", "3n24-l3", "ci64-l3"]


@pytest.mark.parametrize("name", MOMENT_RINGS)
def test_centered_moments_are_the_exact_integers(rh, name):
    rq, rp = rings_for(rh, name)
    N = rq.N
    mq = [int(q) for q in rq.moduli[:rq.level + 1]]
    mp = [int(p) for p in rp.moduli[:rp.level + 1]] if rp is not None else []
    mods = mq + mp
    rnd = random.Random("moments " + name)
    pats = patterns(mods, N, rnd)
    for b in range(0, 9, 3):
        vals = pats[b:b + 3]
        # blocks with every limb of the ring (one more than the view's level): the rows of a poly are strided
        hq = np.array([[[v % int(m) for v in poly] for m in rq.moduli] for poly in vals], dtype=np.uint64)
        q = rh.DevicePoly.from_numpy(rq, hq)
        p = rh.DevicePoly.from_numpy(rp, np.array([[[v % int(m) for v in poly] for m in rp.moduli] for poly in vals], dtype=np.uint64)) if rp is not None else None
        assert q.limbs == rq.level + 2
        for gap in (1, 4):
            want = [nr.moments(nr.centred([[v % m for v in poly] for m in mods], mods, gap)) for poly in vals]
            got = rh.noise.centered_moments(rq, q, rp, p, gap=gap)
            assert got == want, (name, b, gap)
            if b == 6 and gap == 4:                                                 # the composed route: a download and Python integers
                assert rh.noise.centered_moments(rq, q, rp, p, gap=gap, fused=False) == want
        if rp is None:
            assert rq.CenteredMoments(q, gap=4) == want
            stds = rq.Log2OfStandardDeviation(q)
            want1 = [nr.log2_std_of(nr.centred([[v % m for v in poly] for m in mods], mods)) for poly in vals]
            assert stds == want1
        else:
            assert rh.rlwe.Log2OfStandardDeviationQP(rq, rp, rh.rlwe.PolyQP(q, p)) == [nr.log2_std_of(nr.centred([[v % m for v in poly] for m in mods], mods)) for poly in vals]
        if b == 6:                                                                  # a uniform poly has the uniform law, at any number of limbs
            M = rr.prod(mods)
            n, S1, S2, lo, hi = rh.noise.centered_moments(rq, q, rp, p)[0]
            # the sample variance of n uniform draws has the relative deviation sqrt((kurtosis - 1) / n) = sqrt(0.8 / n): six of them
            assert abs(nr.log2_std(n, S1, S2) - math.log2(M) + 0.5 * math.log2(12)) < 0.5 * math.log2(1 + 6 * math.sqrt(0.8 / n))


def test_moments_of_residues_at_or_above_the_modulus_and_of_many_polys(rh):
    """words that are no canonical residues are reduced first; 40 polys in one call (four chunks per poly, one per workgroup)"""
    rq, _ = rings_for(rh, "n1024-l9")
    mods = [int(q) for q in rq.moduli[:rq.level + 1]]
    rnd = np.random.default_rng(5)
    host = rnd.integers(0, 1 << 63, size=(40, rq.level + 2, rq.N), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    q = rh.DevicePoly.from_numpy(rq, host)
    got = rq.CenteredMoments(q)
    for k in (0, 17, 39):
        assert got[k] == nr.moments(nr.centred(host[k, :len(mods)], mods))


# ---- workgroups that take several chunks, more partials than reducing threads, more polys than one launch takes ---------------------------------------
def small_block(ring, xs, patches=()):
    """the residues of small signed coefficients xs (npoly, N) int64 under every limb of the ring (|x| below every modulus), with
    (poly, coefficient, integer) patches of any size: polys whose centred values the test chose"""
    xs = np.asarray(xs, dtype=np.int64)
    host = np.stack([xs.astype(np.uint64) + np.where(xs < 0, np.uint64(int(m)), np.uint64(0)) for m in ring.moduli], axis=1)   # wraps to m - |x|
    for k, i, v in patches:
        host[k, :, i] = [int(v) % int(m) for m in ring.moduli]
    return host


def chosen_rows(xs, patches):
    vals = [[int(v) for v in row] for row in np.asarray(xs)]
    for k, i, v in patches:
        vals[k][i] = int(v)
    return vals


def chosen_moments(xs, patches):
    """the moments are nr.moments of the integers themselves: no reconstruction on the reference's side"""
    return [nr.moments(row) for row in chosen_rows(xs, patches)]


@pytest.mark.parametrize("name,npoly", [("n1024-l1", 700), ("n1024-l9", 600)], ids=["l1-700-polys", "l9-600-polys"])
def test_moments_when_a_workgroup_takes_several_chunks(rh, name, npoly):
    """the host gives a poly min(2048 / npoly, chunks) workgroups: 700 one-limb polys at N = 1024 are two workgroups of two chunks each (chunks
    0, 2 and 1, 3), 600 nine-limb polys three workgroups over four chunks (0 and 3, 1, 2): the accumulators, the extreme vectors and the LDS
    image are carried from a workgroup's first chunk to its second.  The extremes sit in second chunks, in first chunks and in both."""
    ring = rings_for(rh, name)[0]
    N = ring.N
    mods = [int(q) for q in ring.moduli[:ring.level + 1]]
    M = rr.prod(mods)
    half = M >> 1
    rng = np.random.default_rng(npoly)
    xs = rng.integers(-(1 << 40), 1 << 40, size=(npoly, N), dtype=np.int64)
    xs[0] = 5; xs[1] = -7; xs[2] = 9; xs[3] = 11
    patches = [(0, 600, half - 1), (0, 900, 1),                # max in chunk 2 (a second chunk with two workgroups), min in chunk 3
               (1, 10, 2), (1, 800, -(M - half)),              # min in chunk 0, max |x| = M - floor(M / 2) in chunk 3: the `>=` side
               (2, 300, 0), (2, 1000, half - 1),               # min in chunk 1, max in chunk 3
               (3, 100, half - 1), (3, 101, -1), (3, 700, half - 1), (3, 701, 1)]   # ties between a first and a later chunk
    for k in range(4, 24):                                     # arbitrary integers over the whole range, anywhere
        for i in rng.integers(0, N, size=6):
            patches.append((k, int(i), random.Random("big %d %d" % (k, i)).randrange(-(M - half), half)))
    q = rh.DevicePoly.from_numpy(ring, small_block(ring, xs, patches))
    assert q.limbs == ring.level + 2
    assert ring.CenteredMoments(q) == chosen_moments(xs, patches)
    got4 = ring.CenteredMoments(q, gap=4)                      # a quarter of the lanes: one chunk per poly, the other arm of the same call
    assert got4[:8] == [nr.moments(row[::4]) for row in chosen_rows(xs, patches)[:8]]


def test_moments_with_more_partials_than_reducing_threads(rh):
    """one poly of 64 limbs at N = 2^15: chunks of 64 coefficients, 512 workgroups, so every thread of the reducing launch adds two partials and
    takes part in the tournament of the extremes with two candidates"""
    key = "n32768-l64"
    if key not in _CACHE:
        _CACHE[key] = rh.Ring(1 << 15, QI60 + PI60)
    ring = _CACHE[key]
    N = ring.N
    mods = [int(q) for q in ring.moduli]
    M = rr.prod(mods)
    half = M >> 1
    rng = np.random.default_rng(64)
    xs = rng.integers(-(1 << 50), 1 << 50, size=(1, N), dtype=np.int64)
    rnd = random.Random("64 limbs, 512 partials")
    patches = [(0, int(i), rnd.randrange(-(M - half), half)) for i in rng.integers(0, N, size=40)]
    patches += [(0, 64 * 300 + 5, half - 1), (0, 64 * 400 + 7, 0)]             # the extremes in partials 300 and 400: beyond the first 256
    q = rh.DevicePoly.from_numpy(ring, small_block(ring, xs, patches))
    assert ring.CenteredMoments(q) == chosen_moments(xs, patches)


def test_moments_of_more_polys_than_one_launch_takes(rh):
    """65 540 polys at N = 16: the grid's second dimension ends at 65 535, so the call is two launch pairs, the second at a poly offset"""
    ring = rings_for(rh, "n16-l1")[0]
    q0 = int(ring.moduli[0])
    npoly = 65540
    rng = np.random.default_rng(16)
    xs = rng.integers(-(1 << 30), 1 << 30, size=(npoly, 16), dtype=np.int64)
    patches = [(65535, 3, (q0 >> 1) - 1), (65539, 15, -(q0 - (q0 >> 1))), (0, 0, 0)]
    q = rh.DevicePoly.from_numpy(ring, small_block(ring, xs, patches))
    got = ring.CenteredMoments(q)
    rows = chosen_rows(xs, patches)
    assert len(got) == npoly
    S1 = xs.sum(axis=1)
    for k in (0, 1, 65534, 65535, 65536, 65539):
        assert got[k] == nr.moments(rows[k])
    keep = np.ones(npoly, dtype=bool)
    keep[[0, 65535, 65539]] = False
    assert np.array_equal(np.array([g[1] for g in got], dtype=object)[keep], S1.astype(object)[keep])
    assert [g[2] for g in got[1:65535]] == [int(v) for v in (xs[1:65535].astype(object) ** 2).sum(axis=1)]


# ---- rh_rlwe_gadget_phase against the composed ring calls, whole output ---------------------------------------------------------------------------------
def phase_rings(rh, pw2, pc):
    key = ("phase", pw2, pc)
    if key not in _CACHE:
        N = 64
        if pw2:
            Q, P = primes.chain("WIDE", 6)
            Q, P = [int(q) for q in Q[:3]], [int(p) for p in P[:pc]]                # 61 / 36 / 20 bits: another digit count per limb
        else:
            Q, P = QI60[:4], PI60[:pc]
        _CACHE[key] = (rh.Ring(N, Q), rh.Ring(N, P) if pc else None)
    return _CACHE[key]


def blocks(chunks):
    qs, ps = [], []
    for q, p in chunks:
        qs.append(q.numpy())
        ps.append(p.numpy() if p is not None else None)
    return np.concatenate(qs), (np.concatenate(ps) if ps[0] is not None else None)


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("setting", [(0, 2), (0, 1), (16, 1), (12, 0)], ids=lambda s: "pw%d-p%d" % s)
def test_gadget_phase_is_the_composed_sequence_word_for_word(rh, setting, nt):
    pw2, pc = setting
    rq, rp = phase_rings(rh, pw2, pc)
    rq.set_tuning("nt_streams", nt)
    try:
        kg = rh.rlwe.KeyGenerator(rq, rp, prng=rh.rlwe.KeyedPRNG(b"phase %d %d" % setting))
        sks = [kg.GenSecretKeyNew() for _ in range(3)]
        for levelQ in (rq.L - 1, 1):
            kw = dict(levelQ=levelQ, levelP=pc - 1, BaseTwoDecomposition=pw2)
            keys = [kg.GenEvaluationKeyNew(sks[2], sks[k % 2], **kw) for k in range(5)]
            if pw2 == 12:
                dpl = keys[0].digits_per_limb
                assert dpl[-1] < dpl[0]                                             # the last RNS digit has fewer power-of-two digits
            pts = [sks[2].Value.Q, sks[0].Value.Q]
            for items in ([(keys[0], 0, 0)], [(keys[k], k % 2, k % 2) for k in range(5)], [(keys[1], 1, None)]):
                fq, fp = blocks(rh.noise.gadget_phases(items, sks[:2], pts, fused=True))
                cq, cp = blocks(rh.noise.gadget_phases(items, sks[:2], pts, fused=False))
                assert fq.shape[0] == len(items) * min(keys[0].digits_per_limb or [1])
                assert np.array_equal(fq, cq) and (fp is None) == (cp is None) and (fp is None or np.array_equal(fp, cp))
    finally:
        rq.set_tuning("nt_streams", 1)


# ---- every Noise* function: fused against composed against the restatement, on keys given by samples ----------------------------------------------------
from test_gpu_keygen import device_secret, rings, split  # noqa: E402

NOISE_CASES = [c for c in tko.CASES if c[0] == "TAIL"] + [("REF", (16, 1), None)]


@pytest.mark.parametrize("case", NOISE_CASES, ids=tko._ids)
def test_noise_functions_fused_composed_and_restated_agree(rh, case):
    name, (pw2, pc), _ = case
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    rq, rp = rings(rh, name, pc)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    sk, sk_out = device_secret(rh, kg, name, 0), device_secret(rh, kg, name, 1)
    hs, hs_out = tko.secrets(name)
    want = tko.keys(case)
    kw = dict(levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=pw2)
    s = lambda which: {"a": split(want[which][0], levelQ + 1), "e": want[which][1]}
    evk = kg.GenEvaluationKeyNew(sk, sk_out, samples=s("evk_samples"), **kw)
    rlk = kg.GenRelinearizationKeyNew(sk, samples=s("rlk_samples"), **kw)
    gks = kg.GenGaloisKeysNew(tko.galois_elements(N), sk, samples=s("gks_samples"), **kw)
    R = rh.rlwe
    for got, ref in ((lambda f: R.NoiseEvaluationKey(evk, sk, sk_out, fused=f), nr.noise_evaluation_key(want["evk"], hs, hs_out, Q, P)),
                     (lambda f: R.NoiseRelinearizationKey(rlk, sk, fused=f), nr.noise_relin_key(want["rlk"], hs, Q, P)),
                     (lambda f: R.NoiseGadgetCiphertext(evk, sk.Value.Q, sk_out, fused=f), nr.noise_evaluation_key(want["evk"], hs, hs_out, Q, P))):
        a, b = got(True), got(False)
        assert a == b == ref and 0 < a <= nr.evk_bound(levelQ, levelP)
        assert got({"gadget_phase": True, "moments": False}) == ref and got({"gadget_phase": False, "moments": True}) == ref
    both = R.NoiseGaloisKeys(gks, sk), R.NoiseGaloisKeys(R.MemEvaluationKeySet(rlk, gks), sk, fused=False)
    ref = {g: nr.noise_galois_key(k, g, hs, Q, P) for g, k in zip(tko.galois_elements(N), want["gks"])}
    assert both[0] == both[1] == ref
    assert R.NoiseGaloisKey(gks[1], sk) == ref[gks[1].GaloisElement]
    if pc == len(tro.chain(name)[2]) and levelQ == len(Q) - 1:
        a, e = want["pk_samples"]
        pk = kg.GenPublicKeyNew(sk, samples={"a": split(a, len(Q)), "e": e})
        ref = nr.noise_public_key(want["pk"][0], want["pk"][1], hs, Q, P)
        assert R.NoisePublicKey(pk, sk) == R.NoisePublicKey(pk, sk, fused=False) == ref <= nr.pk_bound()


@pytest.mark.parametrize("setting", [(0, 2), (16, 1), (12, 0)], ids=lambda s: "pw%d-p%d" % s)
def test_device_keys_sit_under_the_reference_bounds_and_a_broken_key_far_above(rh, setting):
    """keys from a KeyedPRNG on the device: rlwe_test.go:451-464, :509, :559, :578 and rgsw_test.go:43-55; NoiseGaloisKeys over six elements is
    the six single calls; one row's error replaced by a uniform poly puts the key near log2(QP / sqrt(12))"""
    pw2, pc = setting
    rq, rp = phase_rings(rh, pw2, pc)
    N = rq.N
    prng = rh.rlwe.KeyedPRNG(b"noise bounds %d %d" % setting)
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk, sk_out = kg.GenSecretKeyNew(), kg.GenSecretKeyNew()
    R = rh.rlwe
    levelQ, levelP = rq.L - 1, pc - 1
    bound = nr.evk_bound(levelQ, levelP)
    kw = dict(BaseTwoDecomposition=pw2)
    evk, rlk = kg.GenEvaluationKeyNew(sk, sk_out, **kw), kg.GenRelinearizationKeyNew(sk, **kw)
    galEls = [R.GaloisElement(N, k) for k in (1, 2, 3, 5, -1)] + [2 * N - 1]
    gks = kg.GenGaloisKeysNew(galEls, sk, **kw)
    got = {"evk": R.NoiseEvaluationKey(evk, sk, sk_out), "rlk": R.NoiseRelinearizationKey(rlk, sk), "pk": R.NoisePublicKey(kg.GenPublicKeyNew(sk), sk)}
    all6 = R.NoiseGaloisKeys(gks, sk)
    assert sorted(all6) == sorted(galEls) and all6 == {g.GaloisElement: R.NoiseGaloisKey(g, sk) for g in gks}
    got.update({"gk%d" % g: v for g, v in all6.items()})
    for what, v in got.items():
        print("MEASURED %-6s pw%d-p%d %5.2f [%.2f]" % (what, pw2, pc, v, nr.pk_bound() if what == "pk" else bound))
        assert 0 < v <= (nr.pk_bound() if what == "pk" else bound), what
    enc = rh.rgsw.Encryptor(rq, rp, sk, prng=prng)
    ct, = enc.rows(sk_out.Value.Q, [0], levelQ, levelP, pw2)
    left, right = rh.rgsw.NoiseRGSWCiphertext(ct, sk_out.Value.Q, sk)
    assert (left, right) == rh.rgsw.NoiseRGSWCiphertext(ct, sk_out.Value.Q, sk, fused=False)
    assert 0 < left <= nr.RGSW_BOUND and 0 < right <= nr.RGSW_BOUND
    # component 0 of the key's second row becomes a uniform poly
    mods = [int(q) for q in rq.moduli]
    rnd = random.Random("broken key")
    row = rh.DevicePoly(rq, 1, rq.L, ptr=evk.Q.ptr + 2 * rq.L * N * 8, owner=evk.Q)
    rq.CopyLvl(rh.DevicePoly.from_numpy(rq, rr.uniform_poly(rnd, N, mods)[None]), row)
    M = rr.prod(mods + ([int(p) for p in rp.moduli] if rp is not None else []))
    broken = R.NoiseEvaluationKey(evk, sk, sk_out)
    assert broken == R.NoiseEvaluationKey(evk, sk, sk_out, fused=False)
    assert broken > bound + 10 and broken > math.log2(rr.prod(mods)) - 8 and broken < math.log2(M)


def test_noise_on_a_3n_ring_and_the_refusals_that_stay(rh):
    N = 24
    Q, P = primes.gen_moduli_3n(N, [60, 60, 45], [60])
    rq, rp = rh.Ring(N, [int(q) for q in Q], kind=rh.Matrix3N), rh.Ring(N, [int(p) for p in P], kind=rh.Matrix3N)
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=rh.rlwe.KeyedPRNG(b"noise 3n"))
    sk, sk_out = kg.GenSecretKeyNew(), kg.GenSecretKeyNew()
    evk, rlk, pk = kg.GenEvaluationKeyNew(sk, sk_out), kg.GenRelinearizationKeyNew(sk), kg.GenPublicKeyNew(sk)
    R = rh.rlwe
    for f, bound in ((lambda u: R.NoiseEvaluationKey(evk, sk, sk_out, fused=u), nr.evk_bound(2, 0)),
                     (lambda u: R.NoiseRelinearizationKey(rlk, sk, fused=u), nr.evk_bound(2, 0)), (lambda u: R.NoisePublicKey(pk, sk, fused=u), nr.pk_bound())):
        a = f(True)
        assert a == f(False) and a <= bound + 1                                    # 24 coefficients: a sample deviation, not the law
    gk = R.GaloisKey.from_device(rq, rp, evk.Q, evk.P)
    gk.GaloisElement, gk.NthRoot = 5, 3 * N
    with pytest.raises(rh.RingHipError, match="3N rings have no automorphism"):
        R.NoiseGaloisKeys([gk], sk)
    with pytest.raises(rh.RingHipError, match="conjugate-invariant rings are not supported"):
        rh.rlwe.KeyGenerator(rh.Ring(64, QI60[:2], kind=rh.ConjugateInvariant))


# ---- Norm -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coeff"])
def test_norm_of_fresh_encryptions(rh, is_ntt):
    N, Q, P, _ = tro.chain("REF")
    rq, rp = rings(rh, "REF", 2)
    prng = rh.rlwe.KeyedPRNG(b"norm")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = kg.GenSecretKeyNew()
    level = 2
    rl = rq.AtLevel(level)
    mods = [int(q) for q in Q[:level + 1]]
    rnd = random.Random("norm messages")
    ms = [[rnd.choice((-1, 1)) * rnd.randrange(1000, 1 << 30) for _ in range(N)], [0] * N, [rnd.choice((-1, 1)) * rnd.randrange(50, 60) for _ in range(N)]]
    host = np.stack([rr.ntt(rr.rns(m, mods), N, mods) if is_ntt else rr.rns(m, mods) for m in ms])
    pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rl, host), is_ntt=is_ntt)
    ct = rh.rlwe.Encryptor(rq, rp, sk, prng=prng).EncryptNew(pt)
    dec = rh.rlwe.Decryptor(rq, sk)
    got = rh.rlwe.Norm(ct, dec)
    assert got == rh.rlwe.Norm(ct, dec, fused=False)
    back = dec.DecryptNew(ct)
    if is_ntt:
        rl.INTT(back.Value, back.Value)
    arr = back.Value.numpy()
    assert got == [nr.norm_stats(nr.centred(arr[k], mods)) for k in range(3)]
    assert got[1][1] == -math.inf and got[1][0] <= math.log2(rr.SIGMA) + 1 and got[0][1] > 0 and 4.9 < got[2][2] < 6.3


# ---- GetPrecisionStats --------------------------------------------------------------------------------------------------------------------------------
def test_precision_stats_of_a_device_round_trip(rh):
    """encode -> encrypt -> decrypt on the device; the statistics from the ciphertext, the plaintext, a DeviceValues and an array are those of the
    host function fed the downloaded values; the average precision meets the reference's bound (VerifyTestVectors, precision.go:92-103)"""
    import lintrans_restatement as ltr
    N, Q, P, levels = tro.chain("REF")
    rq, rp = rings(rh, "REF", 2)
    prng = rh.rlwe.KeyedPRNG(b"precision stats")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = kg.GenSecretKeyNew()
    level = levels[0]
    ecd = rh.ckks.Encoder(rq)
    slots = N // 2
    rng = np.random.default_rng(3)
    x = rng.uniform(-1, 1, (2, slots)) + 1j * rng.uniform(-1, 1, (2, slots))
    scale = float(int(Q[level]))
    pt = ecd.NewPlaintext(level, scale, nvec=2)
    ecd.Encode(x, pt)
    ct = rh.ckks.Encryptor(rq, rp, sk, prng=prng).EncryptNew(pt)
    dec = rh.ckks.Decryptor(rq, sk)
    vals = np.array(ecd.Decode(dec.DecryptNew(ct)))
    want = [rh.precision.precision_stats(x[k], vals[k], math.log2(scale), True) for k in range(2)]
    got = rh.ckks.GetPrecisionStats(ecd, dec, x, ct, computeDCF=True)
    dv = rh.ckks.DeviceValues.from_numpy(rq, vals)
    for other in (rh.ckks.GetPrecisionStats(ecd, None, x, dec.DecryptNew(ct), computeDCF=True),
                  rh.ckks.GetPrecisionStats(ecd, None, x, dv, computeDCF=True, log2_scale=math.log2(scale)),
                  rh.ckks.GetPrecisionStats(ecd, None, x, vals, computeDCF=True, log2_scale=math.log2(scale))):
        for a, b, w in zip(got, other, want):
            assert a.String() == b.String() == w.String() and a.RealDist == b.RealDist == w.RealDist and a.L2Dist == w.L2Dist
            assert a.AVGLog2Prec == w.AVGLog2Prec and a.MEDLog2Prec == w.MEDLog2Prec and a.STDLog2Prec == w.STDLog2Prec
    one = rh.ckks.GetPrecisionStats(ecd, None, x[0], vals[0], log2_scale=math.log2(scale))
    pr, pi = ltr.avg_log2_prec(x[0], vals[0].real, vals[0].imag, math.log2(scale))
    assert abs(one.AVGLog2Prec.Real - pr) < 1e-10 and abs(one.AVGLog2Prec.Imag - pi) < 1e-10          # pairwise against sequential sums
    bound = math.log2(scale) - (N.bit_length() - 1 + 2)
    print("MEASURED fresh ckks precision real %.2f imag %.2f [>= %.2f]" % (one.AVGLog2Prec.Real, one.AVGLog2Prec.Imag, bound))
    assert min(one.AVGLog2Prec.Real, one.AVGLog2Prec.Imag) >= bound
    with pytest.raises(rh.RingHipError, match="a ciphertext needs a decryptor"):
        rh.ckks.GetPrecisionStats(ecd, None, x, ct)


# ---- refusals by name -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(rh):
    L = rh.lib()
    rq, _ = rings_for(rh, "n16-l1")
    q = rq.NewPoly(1)
    out = rq.NewPoly(4)
    with pytest.raises(rh.RingHipError, match="gap 3 does not divide N = 16"):
        rq.CenteredMoments(q, gap=3)
    assert L.rh_ring_centered_moments(rq._h, 0, q.ptr, 1, None, 0, None, 0, 3, 1, out.ptr) == -1
    assert b"rh_ring_centered_moments: gap 3 does not divide N = 16" in L.rh_last_error()
    assert L.rh_ring_centered_moments(rq._h, 0, q.ptr, 1, None, 0, None, 0, 0, 1, out.ptr) == -1
    assert L.rh_ring_centered_moments(rq._h, 5, q.ptr, 6, None, 0, None, 0, 1, 1, out.ptr) == -1 and b"level 5 out of range" in L.rh_last_error()
    # more than 64 moduli over Q and P together
    mods = QI60 + PI60 + [97]                                                        # 65 primes = 1 mod 32
    big_q, big_p = rh.Ring(16, mods[:40]), rh.Ring(16, mods[40:])
    bq, bp = big_q.NewPoly(1), big_p.NewPoly(1)
    with pytest.raises(rh.RingHipError, match="more than 64 moduli"):
        rh.noise.centered_moments(big_q, bq, big_p, bp)
    assert L.rh_ring_centered_moments(big_q._h, 39, bq.ptr, 40, big_p._h, 24, bp.ptr, 25, 1, 1, out.ptr) == -5 and b"more than 64 moduli (40 of Q and 25 of P)" in L.rh_last_error()
    vq, vp = big_q.AtLevel(38), big_p.AtLevel(24)                                    # 39 + 25 = 64 moduli are served
    rnd = random.Random("64 limbs")
    hq, hp = rr.uniform_poly(rnd, 16, mods[:40]), rr.uniform_poly(rnd, 16, mods[40:])
    bq, bp = rh.DevicePoly.from_numpy(big_q, hq[None]), rh.DevicePoly.from_numpy(big_p, hp[None])
    basis = mods[:39] + mods[40:]
    assert rh.noise.centered_moments(vq, bq, vp, bp) == [nr.moments(nr.centred(np.concatenate([hq[:39], hp]), basis))]
    # the same modulus in Q and in P
    twin = rh.Ring(16, mods[:1])
    with pytest.raises(rh.RingHipError, match="not pairwise distinct"):
        rh.noise.centered_moments(big_q.AtLevel(1), bq, twin, twin.NewPoly(1))
    # two handles on different streams
    import torch
    side = torch.cuda.Stream()
    big_p.set_stream(side.cuda_stream)
    try:
        with pytest.raises(rh.RingHipError, match="the two ring handles are on different streams"):
            rh.noise.centered_moments(vq, bq, vp, bp)
        assert L.rh_ring_centered_moments(big_q._h, 0, bq.ptr, 40, big_p._h, 0, bp.ptr, 25, 1, 1, out.ptr) == -1
    finally:
        big_p.set_stream(None)
    # the phase entry
    ci = rh.Ring(64, QI60[:2], kind=rh.ConjugateInvariant)
    assert L.rh_rlwe_gadget_phase(ci._h, None, 0, 0, None, None, 1, None, 0, None, None, None, 0, 1, None, 0) == -5
    assert b"rh_rlwe_gadget_phase: conjugate-invariant rings are not supported" in L.rh_last_error()
    sk = rq.NewPoly(1)
    tab = np.zeros(6 + 1 + 1, dtype=np.uint64)
    tdev = rq.NewPoly(1)
    call = lambda t, words=16: L.rh_rlwe_gadget_phase(rq._h, None, 0, 0, sk.ptr, None, 1, None, 0, out.ptr, None, t.ctypes.data_as(rh.ringhip.U64P), 1, 1, tdev.ptr, words)
    assert call(tab) == -1 and b"names a null or misaligned key table" in L.rh_last_error()
    key = rq.NewPoly(4)
    tab = np.array([key.ptr, 0, 2, 1, (1 << 64) - 1, 1, 0, 0], dtype=np.uint64)
    assert call(tab) == -1 and b"names secret 1 of 1" in L.rh_last_error()
    tab[3] = 0; tab[4] = 0
    assert call(tab) == -1 and b"names plaintext 0 of 0" in L.rh_last_error()
    tab[4] = np.uint64((1 << 64) - 1); tab[6] = 2
    assert call(tab) == -1 and b"names row 2 of a key of 2" in L.rh_last_error()
    tab[6] = 1; tab[7] = int(rq.moduli[0])
    assert call(tab) == -1 and b"is not a residue of limb 0" in L.rh_last_error()
    tab[7] = 0
    assert call(tab, 7) == -1 and b"the row table needs 8 words" in L.rh_last_error()
    tab[0] = out.ptr
    assert call(tab) == -1 and b"an output overlaps a key table" in L.rh_last_error()

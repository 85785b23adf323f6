"""GPU: CKKS on conjugate-invariant rings through ckks.Parameters -- the samplers, KeyGenerator, Encryptor, Decryptor, the real-only
encoder, the ring-swap keys and DomainSwitcher -- bit for bit, as whole arrays, against tests/ci_ckks_restatement.py with `samples=` and a given
roots table; fused and composed paths give identical words; under a KeyedPRNG and no host key material the reference's tests meet its bound
at n = 1024 (AVGLog2Prec >= 32 bits, see tests/test_ci_ckks_oracle.py); and every refusal of this layer, the bare constructors included.

Degrees n = 16 (the N % 8 groups of the samplers, one workgroup) and 64 (more than one wave); levels 0, a middle level and the top, the keys
and secrets being allocated wider than the level used; slot counts log_slots in {0, 1, log n - 1, log n}; one encoder case at n = 4096 (the
multi-pass transform and the gap arithmetic past a workgroup).  MulRelin, Rotate and RotateHoisted run under device keys with two moduli of P
(the gadget product of the device on such rings is pinned on arbitrary residues in tests/test_gpu_keyswitch.py): they are checked by what they
decrypt to."""
import functools
import random

import numpy as np
import pytest

import ci_ckks_restatement as cc
import ckks_encoder_restatement as er
import keygen_restatement as kr
import rlwe_restatement as rr
import sampling_restatement as sr
from oracle import primes

pytestmark = pytest.mark.gpu
KEY = b"conjugate-invariant ckks test key"
PSTD = [0x1ffffffff6c80001, 0x1ffffffff6140001]
SCALE = 2.0 ** 45


@functools.lru_cache(maxsize=None)
def chain(n):
    """(Q of four limbs, P of two) = 1 mod 4n"""
    Q, P = primes.gen_moduli((4 * n).bit_length() - 1, [55, 45, 45, 45], [60, 60])
    return [int(q) for q in Q], [int(p) for p in P]


_PARAMS = {}


def params(rh, n, pc=2, ring_type=None):
    """ckks.Parameters of a chain with its first pc moduli of P, made once per session"""
    ring_type = rh.ConjugateInvariant if ring_type is None else ring_type
    key = (n, pc, ring_type)
    if key not in _PARAMS:
        Q, P = chain(n if ring_type == rh.ConjugateInvariant else n // 2)
        _PARAMS[key] = rh.ckks.Parameters(n.bit_length() - 1, Q, P[:pc], 45, RingType=ring_type)
    return _PARAMS[key]


def rnd_for(*tag):
    return random.Random(repr(tag))


def ternary(rnd, n):
    return [rnd.randrange(-1, 2) for _ in range(n)]


def uniform(rnd, rows, n, mods):
    return np.stack([rr.uniform_poly(rnd, n, mods) for _ in range(rows)])


def errors(rnd, rows, n):
    return np.array([rr.gaussian_coeffs(rnd, n) for _ in range(rows)], dtype=np.int32)


def split(a, LQ):
    return np.ascontiguousarray(a[:, :LQ]), (np.ascontiguousarray(a[:, LQ:]) if a.shape[1] > LQ else None)


def same(key, want):
    q = key.Q.numpy().reshape(key.digits, 2, key.Q.limbs, -1)
    p = key.P.numpy().reshape(key.digits, 2, key.P.limbs, -1) if key.P is not None else None
    return np.array_equal(q, want.Q) and (p is None) == (want.P is None) and (p is None or np.array_equal(p, want.P))


# ---- parameters ------------------------------------------------------------------------------------------------------------------------------------------
def test_parameters(rh):
    p = params(rh, 64)
    Q, P = chain(64)
    assert (p.N(), p.LogN(), p.MaxLevel(), p.NthRoot(), p.RingType()) == (64, 6, 3, 256, rh.ConjugateInvariant)
    assert (p.MaxSlots(), p.LogMaxDimensions(), p.LogMaxSlots(), p.EncodingPrecision()) == (64, (0, 6), 6, 53)
    assert p.RingQ().kind == rh.ConjugateInvariant and p.RingP().kind == rh.ConjugateInvariant and p.RingQ().N == 64
    assert p.DefaultScale() == rh.ckks.Scale(1 << 45)
    assert [p.GaloisElement(k) for k in (0, 1, 2, -1)] == [1, 5, 25, pow(5, -1, 256)]
    s = p.StandardParameters()
    assert (s.N(), s.NthRoot(), s.RingType(), s.MaxSlots(), s.LogMaxDimensions()) == (128, 256, rh.Standard, 64, (0, 6))
    assert s.Q == Q and s.P == P and s.RingQ().kind == rh.Standard and s.StandardParameters() is s
    s2 = p.StandardParameters(P=PSTD[:1])
    assert s2.P == PSTD[:1] and s2.Q == Q and s2.N() == 128
    assert s.GaloisElement(1) == 5 and rh.ckks.Parameters(7, Q, [], 45).MaxSlots() == 64
    for x in (s, s2):
        x.close()
    with pytest.raises(rh.RingHipError, match="is not 1 mod NthRoot = 512"):
        rh.ckks.Parameters(7, Q, P, 45, RingType=rh.ConjugateInvariant)
    with pytest.raises(rh.RingHipError, match="RingType must be"):
        rh.ckks.Parameters(6, Q, P, 45, RingType=rh.Matrix3N)


# ---- samplers ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [16, 64])
def test_samplers_bit_for_bit(rh, n):
    p = params(rh, n)
    rq, rp = p.RingQ(), p.RingP()
    Q, P = chain(n)
    prng = rh.rlwe.KeyedPRNG(KEY)
    us = rh.rlwe.UniformSampler(prng, rq, rp, conjugate_invariant=True)
    a, b = rq.NewPoly(3), rp.NewPoly(3)
    us.Read(a, b)
    want = sr.uniform(KEY, 0, 3, n, Q + P)
    assert np.array_equal(a.numpy(), want[:, :4]) and np.array_equal(b.numpy(), want[:, 4:])
    g = rh.rlwe.GaussianSampler(prng, rq, 3.2, 19, conjugate_invariant=True).ReadNew(3)
    assert np.array_equal(g.numpy(), sr.gaussian(KEY, 1, 3, n, sr.gaussian_table(3.2, 19)))
    t = rh.rlwe.TernarySampler(prng, rq, P=2 / 3, conjugate_invariant=True)
    assert np.array_equal(t.ReadNew(3).numpy(), sr.ternary(KEY, 2, 3, n, t.threshold))
    h = rh.rlwe.TernarySampler(prng, rq, H=5, conjugate_invariant=True).ReadNew(2).numpy()
    assert h.shape == (2, n) and np.all(np.count_nonzero(h, axis=1) == 5)
    small = rh.rlwe.SmallPoly.from_numpy(rq, g.numpy())
    lq, lp = rq.NewPoly(3), rp.NewPoly(3)
    rh.rlwe.lift_small(rq, rp, small, lq, lp)
    assert np.array_equal(lq.numpy(), sr.lift(g.numpy(), Q)) and np.array_equal(lp.numpy(), sr.lift(g.numpy(), P))


# ---- keys ----------------------------------------------------------------------------------------------------------------------------------------------------
KEY_CASES = [(2, 3, 1, 0), (2, 1, 1, 0), (1, 2, 0, 16), (1, 3, 0, 0), (0, 0, -1, 12), (0, 3, -1, 20)]       # (#P, levelQ, levelP, pw2)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("case", KEY_CASES, ids=lambda c: "p%d-lq%d-lp%d-w%d" % c)
@pytest.mark.parametrize("n", [16, 64])
def test_keys_from_samples_bit_for_bit(rh, n, case, fused):
    pc, levelQ, levelP, pw2 = case
    p = params(rh, n, pc)
    Q, P = chain(n)
    P = P[:pc]
    rnd = rnd_for("keys", n, case)
    kg = rh.ckks.NewKeyGenerator(p)
    c0, c1 = ternary(rnd, n), ternary(rnd, n)
    sk, sk_out = kg.GenSecretKeyNew(samples=c0), kg.GenSecretKeyNew(samples=c1)
    h0, h1 = cc.Secret(n, c0), cc.Secret(n, c1)
    assert np.array_equal(sk.Value.Q.numpy()[0], h0.rows(Q)) and np.array_equal(sk.coeffs.numpy()[0], np.array(c0, dtype=np.int32))
    if pc:
        assert np.array_equal(sk.Value.P.numpy()[0], h0.rows(P))
    rows = kr.rows_of(Q, levelQ, levelP, pw2)
    LQ, LP = levelQ + 1, levelP + 1
    mods = Q[:LQ] + P[:LP]
    kw = dict(levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=pw2, fused=fused)

    def draw(count):
        a, e = uniform(rnd, count, n, mods), errors(rnd, count, n)
        return a, e, {"a": split(a, LQ), "e": e}
    a, e, s = draw(rows)
    assert same(kg.GenEvaluationKeyNew(sk, sk_out, samples=s, **kw), cc.evaluation_key(h0, h1, Q, P, levelQ, levelP, pw2, a, e))
    a, e, s = draw(rows)
    assert same(kg.GenRelinearizationKeyNew(sk, samples=s, **kw), cc.relin_key(h0, Q, P, levelQ, levelP, pw2, a, e))
    gals = [cc.galois_element(n, k) for k in (1, 2, -1)]
    a, e, s = draw(3 * rows)
    gks = kg.GenGaloisKeysNew(gals, sk, samples=s, **kw)
    assert [(g.GaloisElement, g.NthRoot) for g in gks] == [(g, 4 * n) for g in gals]
    for got, want in zip(gks, cc.galois_keys(h0, gals, Q, P, levelQ, levelP, pw2, a, e)):
        assert same(got, want)
    if levelQ == 3 and levelP == pc - 1:                                                            # the public key lives on the whole of QP
        a, e = uniform(rnd, 1, n, Q + P), errors(rnd, 1, n)
        pk = kg.GenPublicKeyNew(sk, samples={"a": split(a, 4), "e": e}, fused=fused)
        wq, wp = cc.public_key(h0, Q, P, a, e)
        assert np.array_equal(pk.Q.numpy().reshape(wq.shape), wq)
        assert (wp is None and pk.P is None) or np.array_equal(pk.P.numpy().reshape(wp.shape), wp)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coeff"])
@pytest.mark.parametrize("npoly", [1, 3])
@pytest.mark.parametrize("pc", [1, 0], ids=["p", "nop"])
@pytest.mark.parametrize("n", [16, 64])
def test_encryptors_and_decryptor_from_samples_bit_for_bit(rh, n, pc, npoly, is_ntt, fused):
    p = params(rh, n, pc)
    Q, P = chain(n)
    P = P[:pc]
    rq = p.RingQ()
    rnd = rnd_for("enc", n, pc, npoly, is_ntt)
    kg = rh.ckks.NewKeyGenerator(p)
    c0 = ternary(rnd, n)
    sk, h0 = kg.GenSecretKeyNew(samples=c0), cc.Secret(n, c0)
    a, e = uniform(rnd, 1, n, Q + P), errors(rnd, 1, n)
    pk = kg.GenPublicKeyNew(sk, samples={"a": split(a, 4), "e": e}, fused=fused)
    pkQ, pkP = cc.public_key(h0, Q, P, a, e)
    dec = rh.ckks.NewDecryptor(p, sk)
    for level in (0, 2, 3):                                                                         # the secret and the public key hold four limbs
        mods = Q[:level + 1]
        rl = rq.AtLevel(level)
        pts = uniform(rnd, npoly, n, mods)
        pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rl, pts), is_ntt=is_ntt, Scale=rh.ckks.Scale(1), LogDimensions=0, IsBatched=True)
        c1, es = uniform(rnd, npoly, n, mods), errors(rnd, npoly, n)
        ct = rh.ckks.NewEncryptor(p, sk).EncryptNew(pt, samples={"c1": c1, "e": es}, fused=fused)
        want = [cc.encrypt_sk(h0, Q, level, c1[k], es[k], pts[k], is_ntt) for k in range(npoly)]
        assert ct.IsNTT == is_ntt
        for c in (0, 1):
            assert np.array_equal(ct.Value[c].numpy(), np.stack([w[c] for w in want]))
        u, e0, e1 = np.array([ternary(rnd, n) for _ in range(npoly)], dtype=np.int32), errors(rnd, npoly, n), errors(rnd, npoly, n)
        ctp = rh.ckks.NewEncryptor(p, pk).EncryptNew(pt, samples={"u": u, "e0": e0, "e1": e1}, fused=fused)
        wantp = [cc.encrypt_pk(pkQ, pkP, Q, P, level, n, u[k], e0[k], e1[k], pts[k], is_ntt) for k in range(npoly)]
        for c in (0, 1):
            assert np.array_equal(ctp.Value[c].numpy(), np.stack([w[c] for w in wantp]))
        got = dec.DecryptNew(ctp, fused=fused)
        assert np.array_equal(got.Value[0].numpy(), np.stack([cc.decrypt(w, h0, Q, is_ntt) for w in wantp]))
        ct2 = rh.Ciphertext([ct.Value[0], ct.Value[1], ctp.Value[1]], is_ntt=is_ntt)               # degree 2
        ct2.Scale, ct2.LogDimensions = rh.ckks.Scale(1), 0
        got2 = dec.DecryptNew(ct2, fused=fused)
        w2 = [cc.decrypt([want[k][0], want[k][1], wantp[k][1]], h0, Q, is_ntt) for k in range(npoly)]
        assert np.array_equal(got2.Value[0].numpy(), np.stack(w2))


# ---- the real-only encoder -----------------------------------------------------------------------------------------------------------------------------------
def roots_table(n):
    re, im = er.get_roots(4 * n)
    return np.ascontiguousarray(np.stack([re, im], axis=1))


def check_encoder(rh, p, n, log_slots, levels, nvecs, tuning=None):
    Q = [int(q) for q in p.RingQ().moduli]
    enc = rh.ckks.NewEncoder(p, roots=roots_table(n))
    if tuning is not None:
        enc.set_tuning("ckks_fft_lds_log", tuning)
    assert enc.LogMaxSlots == n.bit_length() - 1 and enc.real
    slots = 1 << log_slots
    rng = np.random.default_rng(n + log_slots)
    for level in levels:
        mods = Q[:level + 1]
        for nvec in nvecs:
            for is_ntt, mont in ((True, False), (False, False), (True, True)):
                v = rng.uniform(-1, 1, (nvec, slots)) + 1j * rng.uniform(-1, 1, (nvec, slots))    # the imaginary parts are dropped
                pt = enc.NewPlaintext(level, SCALE, nvec, log_slots, is_ntt=is_ntt, is_montgomery=mont)
                enc.Encode(v, pt)
                want = np.stack([cc.embed(v[k], log_slots, SCALE, n, mods, is_ntt, mont) for k in range(nvec)])
                assert np.array_equal(pt.Value[0].numpy(), want)       # with neither flag the reference's own words: unreduced / equal to q
                if mont:
                    continue
                for logprec in (0, 20):
                    have = enc.DecodePublic(pt, None, logprec)
                    for k in range(nvec):
                        re, im = cc.decode(want[k] % np.array(mods, dtype=np.uint64)[:, None], log_slots, SCALE, n, mods, is_ntt, logprec)
                        assert np.array_equal(have[k].real, re) and np.array_equal(have[k].imag, im)
                assert np.max(np.abs(have.real - v.real)) < 1e-4 and np.max(np.abs(have.imag)) < 1e-4
    enc.close()


@pytest.mark.parametrize("n", [16, 64])
def test_encoder_bit_for_bit(rh, n):
    p = params(rh, n)
    lg = n.bit_length() - 1
    for log_slots in (0, 1, lg - 1, lg):
        check_encoder(rh, p, n, log_slots, (0, 2, 3), (1, 3))


def test_encoder_n4096_multi_pass(rh):
    """n = 4096 real slots: one workgroup's LDS block at the default tuning, the multi-pass transform with a block of 2^10"""
    n = 4096
    Q = [int(q) for q in primes.gen_moduli(14, [55, 45], [])[0]]
    p = rh.ckks.Parameters(12, Q, [], 45, RingType=rh.ConjugateInvariant)
    check_encoder(rh, p, n, 12, (1,), (1,))
    check_encoder(rh, p, n, 12, (1,), (1,), tuning=10)
    check_encoder(rh, p, n, 5, (0,), (2,), tuning=3)
    p.close()


@pytest.mark.parametrize("n", [16, 64])
def test_coefficient_encoding(rh, n):
    p = params(rh, n)
    Q = chain(n)[0]
    enc = rh.ckks.NewEncoder(p, roots=roots_table(n))
    rng = np.random.default_rng(n)
    for level in (0, 3):
        for is_ntt in (False, True):
            v = rng.uniform(-1, 1, (3, n - 3))
            pt = enc.NewPlaintext(level, SCALE, 3, is_ntt=is_ntt, is_batched=False)
            enc.Encode(v, pt)
            want = np.stack([cc.encode_coeffs(v[k], SCALE, n, Q[:level + 1], is_ntt) for k in range(3)])
            canon = want % np.array(Q[:level + 1], dtype=np.uint64)[None, :, None]
            assert np.array_equal(pt.Value[0].numpy(), want)
            have = enc.Decode(pt)
            for k in range(3):
                assert np.array_equal(have[k], cc.decode_coeffs(canon[k], SCALE, n, Q[:level + 1], is_ntt))
    enc.close()


# ---- ring swap and the domain switch ---------------------------------------------------------------------------------------------------------------------------
SWAP_CASES = [(2, 3, 1, 0), (2, 2, 1, 0), (1, 3, 0, 0), (1, 1, 0, 16), (0, 1, -1, 12)]             # (#P of the standard side, levelQ, levelP, pw2)


def swap_setting(rh, n, case, fused=None):
    pc, levelQ, levelP, pw2 = case
    pci = params(rh, n)
    Q = chain(n)[0]
    key = ("std", n, pc)
    if key not in _PARAMS:
        _PARAMS[key] = pci.StandardParameters(P=PSTD[:pc])
    pstd = _PARAMS[key]
    P = PSTD[:pc]
    rnd = rnd_for("swap", n, case)
    kgc, kgs = rh.ckks.NewKeyGenerator(pci), rh.ckks.NewKeyGenerator(pstd)
    cci, cstd = ternary(rnd, n), ternary(rnd, 2 * n)
    sk_ci, sk_std = kgc.GenSecretKeyNew(samples=cci), kgs.GenSecretKeyNew(samples=cstd)
    h_ci, h_std = cc.Secret(n, cci), rr.Secret(2 * n, cstd)
    rows = kr.rows_of(Q, levelQ, levelP, pw2)
    mods = Q[:levelQ + 1] + P[:levelP + 1]
    a = [uniform(rnd, rows, 2 * n, mods) for _ in (0, 1)]
    e = [errors(rnd, rows, 2 * n) for _ in (0, 1)]
    samples = tuple({"a": split(a[i], levelQ + 1), "e": e[i]} for i in (0, 1))
    keys = kgs.GenEvaluationKeysForRingSwapNew(sk_std, sk_ci, levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=pw2, samples=samples, fused=fused)
    want = cc.ring_swap_keys(h_std, h_ci, Q, P, levelQ, levelP, pw2, a, e)
    return pci, pstd, Q, P, kgs, sk_ci, sk_std, h_ci, h_std, keys, want


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("case", SWAP_CASES, ids=lambda c: "p%d-lq%d-lp%d-w%d" % c)
@pytest.mark.parametrize("n", [16, 64])
def test_ring_swap_keys_bit_for_bit(rh, n, case, fused):
    pci, pstd, Q, P, kgs, sk_ci, sk_std, h_ci, h_std, keys, want = swap_setting(rh, n, case, fused)
    # the identity the reference relies on: the Q rows of the mapped secret are the unfolded rows of the conjugate-invariant secret
    m = kgs.ring_swap_secret(sk_ci)
    unfolded = pstd.RingQ().NewPoly(1)
    pstd.RingQ().UnfoldConjugateInvariantToStandard(sk_ci.Value.Q, unfolded)
    assert np.array_equal(m.Value.Q.numpy(), unfolded.numpy())
    hm = cc.mapped_secret(h_ci)
    assert np.array_equal(m.Value.Q.numpy()[0], hm.rows(Q)) and np.array_equal(m.coeffs.numpy()[0], np.array(hm.coeffs, dtype=np.int32))
    if P:
        assert np.array_equal(m.Value.P.numpy()[0], hm.rows(P))
    assert same(keys[0], want[0]) and same(keys[1], want[1])


@pytest.mark.parametrize("npoly", [1, 3])
@pytest.mark.parametrize("case", SWAP_CASES, ids=lambda c: "p%d-lq%d-lp%d-w%d" % c)
@pytest.mark.parametrize("n", [16, 64])
def test_domain_switcher_bit_for_bit(rh, n, case, npoly):
    """both directions on arbitrary residues, from parameters of either type, fused and composed: identical words, and the restatement's"""
    pc, levelQ, levelP, pw2 = case
    pci, pstd, Q, P, kgs, sk_ci, sk_std, h_ci, h_std, keys, want = swap_setting(rh, n, case)
    rnd = rnd_for("switch", n, case, npoly)
    # the device gadget product reads a key at the limb counts of the evaluator's rings: an evaluator over rings of the key's levels
    own = []
    rqe = pstd.RingQ() if levelQ == 3 else rh.Ring(2 * n, Q[:levelQ + 1])
    rpe = None if levelP < 0 else rh.Ring(2 * n, P[:levelP + 1])
    own += [r for r in (rqe, rpe) if r is not None and r is not pstd.RingQ()]
    ev = rh.ckks.Evaluator(rqe, rpe)
    for which, level in ((pstd, levelQ), (pci, max(levelQ - 1, 0))):
        sw = rh.ckks.NewDomainSwitcher(which, keys[0], keys[1])
        mods = Q[:level + 1]
        cin = [uniform(rnd, npoly, n, mods) for _ in (0, 1)]
        # the input allocated one limb wider than the level used, where the ring has one
        wide = min(level + 1, 3)
        pad = [np.concatenate([c, uniform(rnd, npoly, n, Q[level + 1:wide + 1])], axis=1) if wide > level else c for c in cin]
        ct = rh.Ciphertext([rh.DevicePoly.from_numpy(pci.RingQ().AtLevel(wide), x) for x in pad], is_ntt=True)
        ct.Scale, ct.LogDimensions, ct.IsBatched = rh.ckks.Scale(1 << 45), 3, True
        outs = []
        for fused in (True, False):
            out = rh.Ciphertext([pstd.RingQ().AtLevel(level).NewPoly(npoly) for _ in (0, 1)], is_ntt=True)
            sw.RealToComplex(ev, ct, out, fused=fused)
            outs.append([v.numpy() for v in out.Value])
            assert out.Scale == ct.Scale and out.LogDimensions == 3 and out.Level() == level
        wr = [cc.real_to_complex(2 * n, Q, P, [cin[0][k], cin[1][k]], want[1]) for k in range(npoly)]
        for c in (0, 1):
            assert np.array_equal(outs[0][c], outs[1][c]) and np.array_equal(outs[0][c], np.stack([w[c] for w in wr]))
        sin = [uniform(rnd, npoly, 2 * n, mods) for _ in (0, 1)]
        ct = rh.Ciphertext([rh.DevicePoly.from_numpy(pstd.RingQ().AtLevel(level), x) for x in sin], is_ntt=True)
        ct.Scale, ct.LogDimensions, ct.IsBatched = rh.ckks.Scale(1 << 45), 3, True
        outs = []
        for fused in (True, False):
            out = sw.ComplexToRealNew(ev, ct, fused=fused)
            outs.append([v.numpy() for v in out.Value])
            assert out.Scale == rh.ckks.Scale(1 << 46) and out.Value[0].ring.N == n and out.Level() == level
        wc = [cc.complex_to_real(2 * n, Q, P, [sin[0][k], sin[1][k]], want[0]) for k in range(npoly)]
        for c in (0, 1):
            assert np.array_equal(outs[0][c], outs[1][c]) and np.array_equal(outs[0][c], np.stack([w[c] for w in wc]))
        sw.close()
    ev.close()
    for r in own:
        r.close()


# ---- end to end under a KeyedPRNG, no host key material --------------------------------------------------------------------------------------------------------
def meets(rh, want, have, bound):
    want, have = np.asarray(want), np.asarray(have)
    for k in range(want.shape[0]):
        pr = rh.precision.precision_stats(want[k], have[k], 45).AVGLog2Prec
        print("AVGLog2Prec real %.2f imag %.2f (bound %d)" % (pr.Real, pr.Imag, bound))
        if not (pr.Real >= bound and pr.Imag >= bound):
            return False
    return True


def test_end_to_end_n1024_meets_the_reference_bounds(rh):
    """testInsecurePrec45's chain (LogQ {55, 45 x 6}, scale 2^45) with two moduli of P on the conjugate-invariant side, testBridge's P on the
    standard side; batches of 2 vectors; every step at least 45 - (10 + 3) = 32 bits (45 - (11 + 2) = 32 on the standard side)"""
    n, B, BOUND = 1024, 2, 32
    Q, P = primes.gen_moduli(12, [55] + [45] * 6, [60, 60])
    pci = rh.ckks.Parameters(10, Q, P, 45, RingType=rh.ConjugateInvariant)
    pstd = pci.StandardParameters(P=PSTD)
    prng = rh.rlwe.KeyedPRNG(b"end to end conjugate-invariant")
    kg = rh.ckks.NewKeyGenerator(pci, prng)
    sk, pk = kg.GenKeyPairNew()
    rots = [1, 3, -2]
    evk = rh.rlwe.MemEvaluationKeySet(kg.GenRelinearizationKeyNew(sk), kg.GenGaloisKeysNew([pci.GaloisElement(k) for k in rots], sk))
    enc, dec, ev = rh.ckks.NewEncoder(pci), rh.ckks.NewDecryptor(pci, sk), rh.ckks.NewEvaluator(pci, evk)
    rng = np.random.default_rng(11)
    def read(ct):
        if not hasattr(ct, "LogDimensions"):                # the evaluator's New forms allocate bare ciphertexts
            ct.LogDimensions, ct.IsBatched = 10, True
        return enc.Decode(dec.DecryptNew(ct))

    def fresh(key):
        v = rng.uniform(-1, 1, (B, n))
        pt = rh.ckks.NewPlaintext(pci, pci.MaxLevel(), B)
        enc.Encode(v, pt)
        return v, rh.ckks.NewEncryptor(pci, key, prng).EncryptNew(pt)
    v, ct = fresh(sk)
    w, ct2 = fresh(pk)
    assert ct.Scale == pci.DefaultScale() and ct.LogDimensions == 10
    assert meets(rh, v, read(ct), BOUND) and meets(rh, w, read(ct2), BOUND)
    assert meets(rh, v + w, read(ev.AddNew(ct, ct2)), BOUND)
    prod = ev.MulRelinNew(ct, ct2)
    out = rh.ckks.NewCiphertext(pci, 1, pci.MaxLevel(), B)
    ev.Rescale(prod, out)
    ev.DropLevel(out, 1)
    assert out.Level() == pci.MaxLevel() - 1 and meets(rh, v * w, read(out), BOUND)
    for k in rots:
        assert meets(rh, np.roll(v, -k, axis=1), read(ev.RotateNew(ct, k)), BOUND)
    for k, r in ev.RotateHoistedNew(ct, rots).items():
        assert meets(rh, np.roll(v, -k, axis=1), read(r), BOUND)
    # testBridge (ckks_test.go:747-801)
    kgs = rh.ckks.NewKeyGenerator(pstd, prng)
    sk_std = kgs.GenSecretKeyNew()
    evkCtR, evkRtC = kgs.GenEvaluationKeysForRingSwapNew(sk_std, sk)
    sw = rh.ckks.NewDomainSwitcher(pstd, evkCtR, evkRtC)
    encs, decs, evs = rh.ckks.NewEncoder(pstd), rh.ckks.NewDecryptor(pstd, sk_std), rh.ckks.NewEvaluator(pstd)
    std = rh.ckks.NewCiphertext(pstd, 1, ct.Level(), B)
    sw.RealToComplex(evs, ct, std)
    assert std.Scale == ct.Scale and meets(rh, v, encs.Decode(decs.DecryptNew(std)), BOUND)
    evs.Add(std, evs.MulNew(std, 1j), std)
    assert meets(rh, v + 1j * v, encs.Decode(decs.DecryptNew(std)), BOUND)
    for fused in (True, False):
        back = rh.ckks.NewCiphertext(pci, 1, std.Level(), B)
        sw.ComplexToReal(evs, std, back, fused=fused)
        assert back.Scale == rh.ckks.Scale(1 << 46) and meets(rh, v, read(back), BOUND)
    for x in (sw, enc, encs, ev, evs, pstd, pci):
        x.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rh):
    E = rh.RingHipError
    n = 16
    pci = params(rh, n)
    Q, P = chain(n)
    ci, cip = pci.RingQ(), pci.RingP()
    prng = rh.rlwe.KeyedPRNG(KEY)
    kg = rh.ckks.NewKeyGenerator(pci)
    sk = kg.GenSecretKeyNew()
    # the bare constructors on a conjugate-invariant ring handle keep their texts
    for make in (lambda: rh.rlwe.KeyGenerator(ci), lambda: rh.rlwe.Encryptor(ci, None, sk), lambda: rh.rlwe.Decryptor(ci, sk),
                 lambda: rh.rlwe.UniformSampler(prng, ci), lambda: rh.rlwe.GaussianSampler(prng, ci), lambda: rh.rlwe.TernarySampler(prng, ci, P=0.5),
                 lambda: rh.ckks.Encryptor(ci, None, sk), lambda: rh.ckks.Decryptor(ci, sk)):
        with pytest.raises(E, match="conjugate-invariant rings are not supported \\(of the power-of-two rings, standard rings only\\)"):
            make()
    with pytest.raises(E, match="rh_ckks_encoder_create: conjugate-invariant rings are not supported"):
        rh.ckks.Encoder(ci)
    L = rh.lib()
    import ctypes as C
    h = C.c_void_p()
    roots = roots_table(n)
    assert L.rh_ckks_encoder_create(C.byref(h), ci._h, roots.ctypes.data_as(C.POINTER(C.c_double)), 4 * n + 1, 53) != 0
    assert b"conjugate-invariant rings are not supported" in L.rh_last_error()
    std = pci.StandardParameters()
    assert L.rh_ckks_encoder_create_real(C.byref(h), std.RingQ()._h, roots.ctypes.data_as(C.POINTER(C.c_double)), 4 * n + 1, 53) != 0
    assert b"a conjugate-invariant ring is expected" in L.rh_last_error()
    assert L.rh_ckks_encoder_create_real(C.byref(h), ci._h, roots.ctypes.data_as(C.POINTER(C.c_double)), 2 * n + 1, 53) != 0
    assert b"NthRoot + 1 = 65 expected" in L.rh_last_error()
    with pytest.raises(E, match="prec = 90 > 53"):
        rh.ckks.NewEncoder(pci, precision=90)
    with pytest.raises(E, match="ringqp.Poly \\(ringP\\) is built on standard rings only"):
        rh.ckks.Encoder(ci, ringP=cip, conjugate_invariant=True)
    enc = rh.ckks.NewEncoder(pci)
    with pytest.raises(E, match="logSlots \\(5\\) must be greater or equal to 0 and smaller than 4"):
        enc.Encode(np.zeros(4), enc.NewPlaintext(1, SCALE, 1, 5))
    with pytest.raises(E, match="#values \\(17\\) <= slots \\(16\\) <= maxCols \\(16\\)"):
        enc.Encode(np.zeros(17), enc.NewPlaintext(1, SCALE, 1, 4))
    with pytest.raises(E, match="ringqp.Poly but the encoder was built without ringP"):
        enc.Embed(np.zeros(4), enc.NewPlaintext(1, SCALE, 1, 2), rh.rlwe.PolyQP(ci.NewPoly(1), cip.NewPoly(1)))
    # keys
    with pytest.raises(E, match="Galois element must be 1 mod 4"):
        kg.GenGaloisKeyNew(3, sk)
    with pytest.raises(E, match="must be odd"):
        kg.GenGaloisKeyNew(4, sk)
    with pytest.raises(E, match="compressed"):
        kg.GenRelinearizationKeyNew(sk, compressed=True)
    kgs = rh.ckks.NewKeyGenerator(std)
    sk_std = kgs.GenSecretKeyNew()
    for a, b, gen in ((sk_std, sk_std, kgs), (sk, sk, kgs), (sk, sk_std, kgs), (sk_std, sk, kg)):
        with pytest.raises(E, match="GenEvaluationKeysForRingSwapNew: skStd must belong to the generator's standard ring of degree 2n"):
            gen.GenEvaluationKeysForRingSwapNew(a, b)
    other = rh.ckks.Parameters(4, [Q[1], Q[0]], [], 45, RingType=rh.ConjugateInvariant)
    with pytest.raises(E, match="GenEvaluationKeysForRingSwapNew: the two secrets must share the moduli Q"):
        kgs.GenEvaluationKeysForRingSwapNew(sk_std, rh.ckks.NewKeyGenerator(other).GenSecretKeyNew())
    # the evaluator and the domain switch
    ev_ci, ev_std = rh.ckks.NewEvaluator(pci), rh.ckks.NewEvaluator(std)
    ct = rh.ckks.NewCiphertext(pci, 1, 1)
    with pytest.raises(E, match="not supported when parameters.RingType\\(\\) == ring.ConjugateInvariant"):
        ev_ci.ConjugateNew(ct)
    k0, k1 = kgs.GenEvaluationKeysForRingSwapNew(sk_std, sk)
    sw = rh.ckks.NewDomainSwitcher(pci, k0, k1)
    cs = rh.ckks.NewCiphertext(std, 1, 1)
    with pytest.raises(E, match="cannot ComplexToReal: provided evaluator is not instantiated with RingType ring.Standard"):
        sw.ComplexToReal(ev_ci, cs, ct)
    with pytest.raises(E, match="cannot RealToComplex: provided evaluator is not instantiated with RingType ring.Standard"):
        sw.RealToComplex(ev_ci, ct, cs)
    with pytest.raises(E, match="cannot ComplexToReal: ctIn ring degree must be twice opOut ring degree"):
        sw.ComplexToReal(ev_std, cs, cs)
    with pytest.raises(E, match="cannot RealToComplex: opOut ring degree must be twice ctIn ring degree"):
        sw.RealToComplex(ev_std, ct, ct)
    with pytest.raises(E, match="cannot ComplexToReal: opOut is allocated at level 2 above the level 1 of the switch"):
        sw.ComplexToReal(ev_std, cs, rh.ckks.NewCiphertext(pci, 1, 2))
    with pytest.raises(E, match="cannot RealToComplex: opOut is allocated at level 3 above the level 1"):
        sw.RealToComplex(ev_std, ct, rh.ckks.NewCiphertext(std, 1, 3))
    low = kgs.GenEvaluationKeysForRingSwapNew(sk_std, sk, levelQ=1)[0]
    with pytest.raises(E, match="cannot ComplexToReal: the key is made at levels \\(Q 1, P 1\\) but the evaluator's rings hold levels \\(Q 3, P 1\\)"):
        rh.ckks.NewDomainSwitcher(std, low, None).ComplexToReal(ev_std, cs, ct)
    none = rh.ckks.NewDomainSwitcher(std)
    with pytest.raises(E, match="cannot ComplexToReal: no realToComplexEvk provided to this DomainSwitcher"):
        none.ComplexToReal(ev_std, cs, ct)
    with pytest.raises(E, match="cannot RealToComplex: no realToComplexEvk provided to this DomainSwitcher"):
        none.RealToComplex(ev_std, ct, cs)
    idx = rh.DevicePoly.from_numpy(ci.AtLevel(0), np.zeros((1, 1, n), dtype=np.uint64))
    g = std.RingQ().AtLevel(1).NewPoly(1)
    o = ci.AtLevel(1).NewPoly(1)
    assert L.rh_ckks_bridge_fold_tail(ci._h, 1, g.ptr, g.ptr, g.ptr, idx.ptr, o.ptr, o.ptr, 1) != 0 and b"the two outputs overlap" in L.rh_last_error()
    assert L.rh_ckks_bridge_fold_tail(ci._h, 9, g.ptr, g.ptr, g.ptr, idx.ptr, o.ptr, o.ptr, 1) != 0 and b"level 9 out of range" in L.rh_last_error()
    assert L.rh_ckks_bridge_fold_tail(ci._h, 1, g.ptr, g.ptr, g.ptr, None, o.ptr, o.ptr, 1) != 0 and b"null argument" in L.rh_last_error()
    # what stays out of scope on such rings keeps refusing
    with pytest.raises(E, match="conjugate-invariant"):
        rh.multiparty.PublicKeyGenProtocol(ci)
    for x in (sw, none, enc, ev_ci, ev_std, std, other):
        x.close()

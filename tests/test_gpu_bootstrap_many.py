"""GPU: rh_ckks_bootstrap_pack / rh_ckks_bootstrap_unpack (csrc/bootstrap.hip) and bootstrapping.Bootstrapper (BootstrapMany), bit for bit on whole
outputs against tests/bootstrap_many_restatement.py, which tests/test_bootstrap_many_oracle.py pins to coefficient arithmetic and to decoding.

The kernels, under every cache policy, against the restatement's loops and against the composed ring calls (MulCoeffsMontgomeryThenAdd per pair,
CopyLvl + MulCoeffsMontgomery), the inputs checked unchanged:
  S64   N = 64, a mixed-width chain of 60, 40, 56 bits: 32 coefficient pairs, fewer than a workgroup's lanes
  N13   N = 2^13, the same widths: several chunks per row
each read at the top level (dense blocks) and one level below (blocks of 3 limbs per poly read through an AtLevel(1) view: in_rows > level + 1),
tree levels g in {1, 2, 4, 5} (5: the second launch and the scratch) and n in {1, G - 1, G, G + 1, 2 G + 1} ciphertexts."""
import functools

import numpy as np
import pytest

import bootstrap_many_restatement as bm
import ring_packing_restatement as rp
from conftest import uniform_mod

pytestmark = pytest.mark.gpu
POLICIES = (0, 1, 2)
LOGQ = [60, 40, 56]
GS = (1, 2, 4, 5)
NMAX = 2 * 32 + 1


def counts(g):
    G = 1 << g
    return sorted({1, G - 1, G, G + 1, 2 * G + 1} - {0})


@functools.lru_cache(maxsize=None)
def chain(name):
    from oracle import primes
    logN = 6 if name == "S64" else 13
    Q, _ = primes.gen_moduli(logN + 1, LOGQ, [61])
    return 1 << logN, tuple(int(q) for q in Q)


@functools.lru_cache(maxsize=None)
def operands(name):
    """(c0, c1): (NMAX, 3, N) canonical residues, with 0 and q - 1 planted in every row"""
    N, Q = chain(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    out = []
    for _ in (0, 1):
        a = np.stack([np.stack([uniform_mod(rng, q, N) for q in Q]) for _ in range(NMAX)])
        for i, q in enumerate(Q):
            a[:, i, [0, 1, N - 1]] = [q - 1, 0, q - 1]
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def host_tables(name):
    N, Q = chain(name)
    logN = N.bit_length() - 1
    return rp.gen_xpow2_ntt(N, Q, logN, False), rp.gen_xpow2_ntt(N, Q, logN, True)


def geometry(name, g):
    """LogSlots 0: logGap = LogMaxSlots - 1 >= g - 1 in both rings"""
    N, _ = chain(name)
    log_max = N.bit_length() - 2
    return 0, log_max - 1, log_max


@functools.lru_cache(maxsize=None)
def expected(name, level, g, n):
    """the restatement: (packed ciphertexts, what unpack_many makes of them)"""
    N, Q = chain(name)
    mods = Q[:level + 1]
    xp, xinv = host_tables(name)
    c = operands(name)
    log_slots, _, log_max = geometry(name, g)
    cts = [[c[0][k, :level + 1], c[1][k, :level + 1]] for k in range(n)]
    packed, dims = bm.pack(cts, [log_slots] * n, bm.PackingContext(N, log_max, log_slots + g, log_slots, n), xp, mods)
    assert dims == log_slots + g
    back = bm.unpack_many(packed, bm.PackingContext(N, log_max, log_slots + g, log_slots, n), xinv, mods)
    assert len(back) == n
    return packed, back


def stack(cts, c):
    return np.stack([ct[c] for ct in cts])


@pytest.mark.parametrize("nt_streams", POLICIES, ids=["nt-never", "nt-by-size", "nt-always"])
@pytest.mark.parametrize("name", ["S64", "N13"])
def test_pack_and_unpack_kernels_against_the_restatement(rh, name, nt_streams):
    bts = rh.bootstrapping
    N, Q = chain(name)
    ring = rh.Ring(N, list(Q))
    ring.set_tuning("nt_streams", nt_streams)
    logN = N.bit_length() - 1
    xPow2, xPow2Inv = rh.rlwe.GenXPow2NTT(ring, logN, False), rh.rlwe.GenXPow2NTT(ring, logN, True)
    c = operands(name)
    for level in (2, 1):
        rq = ring.AtLevel(level)
        L = level + 1
        for g in GS:
            _, logGap, _ = geometry(name, g)
            xp, xinv = bts.pack_table(ring, xPow2, logGap, g), bts.pack_table(ring, xPow2Inv, logGap, g)      # full-level tables, read at `level`
            for n in counts(g):
                m = -(-n >> g)
                packed, back = expected(name, level, g, n)
                # level 2: dense blocks; level 1: blocks of 3 limbs per poly whose last limb is not the ring's business
                ins = [rh.DevicePoly.from_numpy(ring, a[:n]) for a in c]
                outs = [ring.NewPoly(m) for _ in (0, 1)] if level == 2 else [rq.NewPoly(m) for _ in (0, 1)]
                bts.bootstrap_pack(rq, g, ins, outs, xp)
                for k in (0, 1):
                    assert np.array_equal(outs[k].numpy()[:, :L], stack(packed, k)), (name, level, g, n, "pack", k)
                    assert np.array_equal(ins[k].numpy(), c[k][:n]), "pack wrote to its input"
                comp = [rq.NewPoly(m) for _ in (0, 1)]
                bts.pack_composed(rq, g, ins, comp, xp)
                assert all(np.array_equal(comp[k].numpy(), outs[k].numpy()[:, :L]) for k in (0, 1)), (name, level, g, n, "pack composed")
                assert all(np.array_equal(ins[k].numpy(), c[k][:n]) for k in (0, 1))
                # unpack what the pack gave: a new block
                before = [o.numpy() for o in outs]
                un = [rq.NewPoly(n) for _ in (0, 1)]
                bts.bootstrap_unpack(rq, g, n, outs, un, xinv)
                for k in (0, 1):
                    assert np.array_equal(un[k].numpy(), stack(back, k)), (name, level, g, n, "unpack", k)
                    assert np.array_equal(outs[k].numpy(), before[k]), "unpack wrote to its input"
                un2 = [rq.NewPoly(n) for _ in (0, 1)]
                bts.unpack_composed(rq, g, n, outs, un2, xinv)
                assert all(np.array_equal(un[k].numpy(), un2[k].numpy()) for k in (0, 1)), (name, level, g, n, "unpack composed")
    ring.close()


def test_pack_refusals(rh):
    bts, E = rh.bootstrapping, rh.RingHipError
    N, Q = chain("S64")
    ring = rh.Ring(N, list(Q))
    xPow2 = rh.rlwe.GenXPow2NTT(ring, 6, False)
    xp = bts.pack_table(ring, xPow2, 3, 2)
    a, b = ring.NewPoly(5), ring.NewPoly(5)
    o0, o1 = ring.NewPoly(2), ring.NewPoly(2)
    with pytest.raises(E, match="cannot pack: 5 ciphertexts over 2 tree levels give 2"):
        bts.bootstrap_pack(ring, 2, (a, b), (o0, ring.NewPoly(3)), xp)
    with pytest.raises(E, match="cannot pack: 5 ciphertexts over 2 tree levels give 2"):
        bts.bootstrap_pack(ring, 2, (a, ring.NewPoly(4)), (o0, o1), xp)
    with pytest.raises(E, match="the two components differ in limbs"):
        bts.bootstrap_pack(ring.AtLevel(1), 2, (a, ring.AtLevel(1).NewPoly(5)), (o0, o1), xp)
    with pytest.raises(E, match="hold at least level \\+ 1 = 3 limbs"):
        bts.bootstrap_pack(ring, 2, (a, b), (ring.AtLevel(1).NewPoly(2), ring.AtLevel(1).NewPoly(2)), xp)
    with pytest.raises(E, match="the table holds 2 rows per limb, 3 tree levels need 3"):
        bts.bootstrap_pack(ring, 3, (a, b), (ring.NewPoly(1), ring.NewPoly(1)), xp)
    with pytest.raises(E, match="cannot unpack: 5 ciphertexts over 2 tree levels come from 2"):
        bts.bootstrap_unpack(ring, 2, 5, (o0, o1), (a, ring.NewPoly(6)), xp)
    # the C ABI's own: an output that overlaps an input, the table or the other output
    big = ring.NewPoly(7)
    view = lambda first, count: rh.rlwe._view(big, first, count)
    with pytest.raises(E, match="rh_ckks_bootstrap_pack: an output overlaps an input or the table"):
        bts.bootstrap_pack(ring, 2, (view(0, 5), b), (view(4, 2), o1), xp)
    with pytest.raises(E, match="rh_ckks_bootstrap_pack: an output overlaps an input or the table"):
        row = rh.rlwe._view(xp, 0, 1)                                            # the output IS the table's row
        bts.bootstrap_pack(ring, 1, (ring.NewPoly(2), ring.NewPoly(2)), (row, ring.NewPoly(1)), row)
    with pytest.raises(E, match="rh_ckks_bootstrap_pack: two outputs overlap"):
        bts.bootstrap_pack(ring, 2, (a, b), (o0, o0), xp)
    with pytest.raises(E, match="rh_ckks_bootstrap_unpack: an output overlaps an input or the table"):
        bts.bootstrap_unpack(ring, 2, 5, (view(0, 2), o1), (view(1, 5), b), xp)
    with pytest.raises(E, match="rh_ckks_bootstrap_unpack: two outputs overlap"):
        bts.bootstrap_unpack(ring, 2, 5, (o0, o1), (a, a), xp)
    lib = rh.lib()
    assert lib.rh_ckks_bootstrap_pack(ring._h, 2, 5, 0, a.ptr, b.ptr, 3, o0.ptr, o1.ptr, 3, xp.ptr, 3, None, 0) != 0
    assert b"tree levels out of range" in lib.rh_last_error()
    assert lib.rh_ckks_bootstrap_pack(ring._h, 2, 40, 5, a.ptr, b.ptr, 3, o0.ptr, o1.ptr, 3, xp.ptr, 3, None, 0) != 0
    assert b"the scratch holds 0 words" in lib.rh_last_error()
    assert lib.rh_ckks_bootstrap_pack_scratch_words(64, 3, 40, 5) == 2 * 3 * 3 * 64 and lib.rh_ckks_bootstrap_pack_scratch_words(64, 3, 40, 4) == 0
    ring.close()


# ---- bootstrapping.Bootstrapper: BootstrapMany end to end at the N = 2^10 settings of tests/test_bootstrapping_oracle.py -------------------------------
import math                                                            # noqa: E402

import ckks_restatement as cr                                          # noqa: E402
import test_bootstrapping_oracle as tbo                                # noqa: E402

SCALE = 2 ** tbo.LOGSCALE
WEIGHT = 192                                                           # the dense secret of the encapsulated settings


def literals(rh, s):
    lit = lambda d: rh.dft.MatrixLiteral(d["Type"], d["LogSlots"], d["LevelQ"], d["LevelP"], d["Levels"], d["Format"], d["Scaling"], d["BitReversed"], d["LogBSGSRatio"])
    return lit(s.s2c), rh.mod1.ParametersLiteral(**s.mod1), lit(s.c2s)


class Arm:
    """one arm of BootstrapMany: the rings, the device keys of Parameters.GenEvaluationKeys under a KeyedPRNG, both Bootstrappers, the input batch"""
    _cache = {}

    def __new__(cls, rh, name):
        if name in cls._cache:
            return cls._cache[name]
        self = object.__new__(cls)
        self.name = name
        log_slots = 9 if name == "ci" else 8
        s = self.s = tbo.Setting(log_slots, True)
        self.rq, self.rp = rh.Ring(tbo.N, s.Q), rh.Ring(tbo.N, s.P)
        self.prng = prng = rh.rlwe.KeyedPRNG(b"bootstrap many " + name.encode())
        s2c, m1, c2s = literals(rh, s)
        kw = dict(ringQ=self.rq, ringP=self.rp, ResidualMaxLevel=s.residual_level, ResidualDefaultScale=SCALE, SlotsToCoeffsParameters=s2c,
                  Mod1ParametersLiteral=m1, CoeffsToSlotsParameters=c2s, EphemeralSecretWeight=32, BootstrappingSecretWeight=WEIGHT)
        self.kw = kw
        res = s.Q[:s.residual_level + 1]
        if name == "pack":                                             # N1 = N2: 5 ciphertexts of LogSlots 6 -> two packed ones, 4 + 1
            self.n, self.log_slots, self.ring1 = 5, 6, self.rq
            self.sk = rh.rlwe.KeyGenerator(self.rq, self.rp, xs=("H", WEIGHT), prng=prng).GenSecretKeyNew()
            self.enc, self.dec = rh.ckks.Encoder(self.rq), rh.ckks.Decryptor(self.rq, self.sk)
            self.encryptor = rh.ckks.Encryptor(self.rq, None, self.sk, prng)
            self.log_n_residual = tbo.LOGN
        elif name == "degree":                                         # N1 = 2^8: 3 of LogSlots 6 -> 2 in N1 -> switch -> 1 in N2
            self.n, self.log_slots = 3, 6
            self.ring1 = rh.Ring(256, res)
            kw["ResidualRingQ"] = self.ring1
            self.sk = rh.rlwe.KeyGenerator(self.ring1, None, prng=prng).GenSecretKeyNew()
            self.enc, self.dec = rh.ckks.Encoder(self.ring1), rh.ckks.Decryptor(self.ring1, self.sk)
            self.encryptor = rh.ckks.Encryptor(self.ring1, None, self.sk, prng)
            self.log_n_residual = 8
        else:                                                          # conjugate-invariant residual ring of degree 2^9: 3 ciphertexts, the third alone
            self.n, self.log_slots = 3, 9
            self.pci = rh.ckks.Parameters(9, res, s.P, tbo.LOGSCALE, RingType=rh.ConjugateInvariant)
            self.ring1 = self.pci.RingQ()
            kw["ResidualRingQ"] = self.ring1
            self.sk = rh.ckks.NewKeyGenerator(self.pci, prng).GenSecretKeyNew()
            self.enc, self.dec = rh.ckks.NewEncoder(self.pci), rh.ckks.NewDecryptor(self.pci, self.sk)
            self.encryptor = rh.ckks.NewEncryptor(self.pci, self.sk, prng)
            self.log_n_residual = 9
        self.params = rh.bootstrapping.Parameters(**kw)
        self.keys, self.skN2 = self.params.GenEvaluationKeys(self.sk, prng=prng)
        self.bts = {f: rh.bootstrapping.Bootstrapper(self.params, self.keys, fused=f) for f in (True, False)}
        rng = np.random.default_rng(len(name))
        slots = 1 << self.log_slots
        self.values = rng.uniform(-1, 1, (self.n, slots)) + (0 if name == "ci" else 1j * rng.uniform(-1, 1, (self.n, slots)))
        pt = self.enc.NewPlaintext(0, SCALE, nvec=self.n, log_slots=self.log_slots)
        self.enc.Encode(self.values, pt)
        self.ct = self.encryptor.EncryptNew(pt)
        self.before = [v.numpy() for v in self.ct.Value]
        cls._cache[name] = self
        return self

    def decode(self, ct):
        ct.IsBatched = True
        return self.enc.Decode(self.dec.DecryptNew(ct))


def words(ct):
    return [v.numpy() for v in ct.Value]


def host_cts(ct):
    w = words(ct)
    return [[w[0][k], w[1][k]] for k in range(w[0].shape[0])]


def device_ct(rh, ring, cts, like, log_slots, scale=None):
    level = cts[0][0].shape[0] - 1
    out = rh.Ciphertext([rh.DevicePoly.from_numpy(ring.AtLevel(level), np.stack([c[i] for c in cts])) for i in (0, 1)], is_ntt=True)
    out.Scale, out.LogDimensions = like.Scale if scale is None else scale, log_slots
    return out


@functools.lru_cache(maxsize=None)
def host_powers(N, mods):
    logN = N.bit_length() - 1
    return rp.gen_xpow2_ntt(N, mods, logN, False), rp.gen_xpow2_ntt(N, mods, logN, True)


def hand_composition(rh, a):
    """BootstrapMany as the composition of pieces pinned elsewhere: the restatement's host pack / fold on downloaded words, the device Evaluate,
    ApplyEvaluationKey and DomainSwitcher calls, the restatement's unpack / unfold"""
    B, s = a.bts[True], a.s
    res = tuple(s.Q[:s.residual_level + 1])
    ev, ks = B.Evaluator, B.Evaluator.Evaluator.ks
    if a.name == "ci":
        std = B.RealToComplexNew(a.ct)
        h = host_cts(std)
        sc = cr.Scale(SCALE)
        folded = [bm.pair_fold(tbo.N, res[:1], h[0], h[1], sc), bm.pair_fold(tbo.N, res[:1], h[2], None, sc)]
        out = ev.Evaluate(device_ct(rh, a.rq, folded, std, 9))
        half = out.Scale.Mul(rh.ckks.Scale(0.5))
        x = host_cts(out)
        unfolded = [x[0], bm.pair_unfold(tbo.N, res, x[0], sc), x[1]]
        return B.ComplexToRealNew(device_ct(rh, a.rq, unfolded, out, 9, half)), 9
    cts, n, ls = host_cts(a.ct), a.n, a.log_slots
    if a.name == "degree":
        xp1, xinv1 = host_powers(256, res)
        c1 = bm.PackingContext(256, 7, 7, ls, n)
        cts, d = bm.pack(cts, [ls] * n, c1, xp1, res[:1])
        small = device_ct(rh, a.ring1, cts, a.ct, d)
        big = device_ct(rh, a.rq, [[np.zeros((1, tbo.N), dtype=np.uint64)] * 2] * len(cts), a.ct, d)
        ks.ApplyEvaluationKey(small, a.keys.EvkN1ToN2, big)
        cts, ls2 = host_cts(big), d
    else:
        ls2 = ls
    xp2, xinv2 = host_powers(tbo.N, res)
    c2 = bm.PackingContext(tbo.N, tbo.LOGN - 1, 8, ls2, len(cts))
    packed, d = bm.pack(cts, [ls2] * len(cts), c2, xp2, res[:1])
    out = ev.Evaluate(device_ct(rh, a.rq, packed, a.ct, d))
    back = bm.unpack_many(host_cts(out), c2, xinv2, res)
    assert c2.NbPackedCTs == 0
    if a.name == "degree":
        big = device_ct(rh, a.rq, back, out, ls2)
        small = device_ct(rh, a.ring1, [[np.zeros((2, 256), dtype=np.uint64)] * 2] * len(back), out, ls2)
        ks.ApplyEvaluationKey(big, a.keys.EvkN2ToN1, small)
        back = bm.unpack_many(host_cts(small), c1, xinv1, res)
        assert c1.NbPackedCTs == 0
    return device_ct(rh, a.ring1, back, out, ls), ls


@pytest.mark.parametrize("name", ["pack", "degree", "ci"])
def test_bootstrap_many_end_to_end(rh, name):
    """(a) fused and composed agree on every word, the level, the scale and LogDimensions; (b) both equal the hand composition; (c) each output,
    decrypted and decoded on the device under skN1, meets the reference's bound log2(DefaultScale) - (LogN_residual + 2) - 10
    (bootstrapping_test.go:456-464): 18, 20 and 19 bits, the real part alone on the conjugate-invariant ring.  The input is left as it was."""
    a = Arm(rh, name)
    got = {f: a.bts[f].BootstrapMany(a.ct) for f in (True, False)}
    assert all(np.array_equal(x, y) for x, y in zip(words(a.ct), a.before)), "BootstrapMany wrote to its input"
    for f, out in got.items():
        assert out.Level() == a.bts[f].OutputLevel() == a.s.residual_level and out.Value[0].npoly == a.n and out.Value[0].ring.N == a.ring1.N
        assert out.Scale.Value == SCALE and out.LogDimensions == a.log_slots
    assert all(np.array_equal(x, y) for x, y in zip(words(got[True]), words(got[False]))), (name, "fused against composed")
    hand, ls = hand_composition(rh, a)
    assert all(np.array_equal(x, y) for x, y in zip(words(got[True]), words(hand))), (name, "against the hand composition")
    have = a.decode(got[True])
    bound = tbo.LOGSCALE - (a.log_n_residual + 2) - 10
    for j in range(a.n):
        re_, im_ = tbo.avg_log2_prec(a.values[j], have[j])
        print("BootstrapMany %s ciphertext %d: %.2f / %.2f bits (bound %d)" % (name, j, re_, im_, bound))
        assert (re_ if name == "ci" else min(re_, im_)) >= bound, (name, j, re_, im_)
    assert a.bts[True].Depth() == a.s.top - a.s.residual_level and a.bts[True].MinimumInputLevel() == 1
    one = a.bts[True].Bootstrap(a.bts[True]._views(a.ct, 0))
    assert one.Value[0].npoly == 1 and one.Scale.Value == SCALE and one.LogDimensions == a.log_slots


def test_gen_evaluation_keys(rh):
    """with samples= the key words are those of the key-layer calls made one by one; skN2 decrypts what EvkN1ToN2 switched; N1 = N2: skN2 is
    skN1 under every limb of Q and P"""
    a = Arm(rh, "degree")
    rq, rp_, N = a.rq, a.rp, tbo.N
    LQ, LP = len(a.s.Q), len(a.s.P)
    rows = -(-LQ // LP)
    rng = np.random.default_rng(3)
    key_samples = lambda: {"a": (np.stack([np.stack([uniform_mod(rng, q, N) for q in a.s.Q]) for _ in range(rows)]),
                                 np.stack([np.stack([uniform_mod(rng, p, N) for p in a.s.P]) for _ in range(rows)])),
                           "e": rng.integers(-19, 20, (rows, N)).astype(np.int32)}
    co = np.zeros(N, dtype=np.int32)
    co[rng.choice(N, WEIGHT, replace=False)] = rng.choice([-1, 1], WEIGHT)
    samples = {"skN2": co, "EvkN1ToN2": key_samples(), "rlk": key_samples()}
    keys, skN2 = a.params.GenEvaluationKeys(a.sk, prng=rh.rlwe.KeyedPRNG(b"samples"), samples=samples)
    gen = rh.rlwe.KeyGenerator(rq, rp_, prng=rh.rlwe.KeyedPRNG(b"one by one"))
    sk2 = gen.GenSecretKeyNew(co)
    assert np.array_equal(sk2.Value.Q.numpy(), skN2.Value.Q.numpy()) and np.array_equal(sk2.Value.P.numpy(), skN2.Value.P.numpy())
    for mine, theirs in ((keys.EvkN1ToN2, gen.GenEvaluationKeyNew(a.sk, sk2, samples=samples["EvkN1ToN2"])),
                         (keys.rlk, gen.GenRelinearizationKeyNew(sk2, samples=samples["rlk"]))):
        assert np.array_equal(mine.Q.numpy(), theirs.Q.numpy()) and np.array_equal(mine.P.numpy(), theirs.P.numpy())
    assert sorted(keys.galois_keys) == [g for g in a.params.GaloisElements() if g != 1] and keys.EvkN2ToN1 is not None
    assert keys.EvkDenseToSparse.Q.ring.L == 1 and keys.EvkDenseToSparse.P.ring.L == 1 and keys.EvkCmplxToReal is None
    # skN2 decrypts a ciphertext switched by EvkN1ToN2 (the arm's own keys)
    ks = a.bts[True].Evaluator.Evaluator.ks
    big = rh.Ciphertext([rq.AtLevel(0).NewPoly(a.n) for _ in (0, 1)], is_ntt=True)
    ks.ApplyEvaluationKey(a.ct, a.keys.EvkN1ToN2, big)
    big.Scale, big.LogDimensions, big.IsBatched = a.ct.Scale, a.log_slots, True
    enc2 = rh.ckks.Encoder(rq)
    have = enc2.Decode(rh.ckks.Decryptor(rq, a.skN2).DecryptNew(big))
    assert np.max(np.abs(have - a.values)) < 2.0 ** -20
    enc2.close()
    # N1 = N2: the same secret, extended
    p = Arm(rh, "pack")
    assert np.array_equal(p.skN2.Value.Q.numpy(), p.sk.Value.Q.numpy()) and np.array_equal(p.skN2.Value.P.numpy(), p.sk.Value.P.numpy())
    assert p.keys.EvkN1ToN2 is None and p.keys.EvkRealToCmplx is None
    c = Arm(rh, "ci")
    assert c.keys.EvkRealToCmplx is not None and c.keys.EvkCmplxToReal is not None and c.keys.EvkN1ToN2 is None


def test_bootstrapper_refusals(rh):
    a = Arm(rh, "degree")
    bts, E = rh.bootstrapping, rh.RingHipError
    k = a.keys
    missing = "cannot NewBootstrapper: evk.\\(BootstrappingKeys\\) is missing EvkN1ToN2 and EvkN2ToN1"
    with pytest.raises(E, match=missing):
        bts.Bootstrapper(a.params, bts.EvaluationKeys(k.rlk, k.galois_keys, k.EvkDenseToSparse, k.EvkSparseToDense, None, k.EvkN2ToN1))
    c = Arm(rh, "ci")
    with pytest.raises(E, match=missing):
        bts.Bootstrapper(c.params, bts.EvaluationKeys(c.keys.rlk, c.keys.galois_keys, c.keys.EvkDenseToSparse, c.keys.EvkSparseToDense, EvkRealToCmplx=c.keys.EvkRealToCmplx))
    with pytest.raises(E, match="IterationsParameters \\(META-BTS"):
        bts.Bootstrapper(bts.Parameters(**dict(a.kw, IterationsParameters={"BootstrappingPrecision": [25], "ReservedPrimeBitSize": 28})), k)
    with pytest.raises(E, match="PREC128"):
        bts.Bootstrapper(bts.Parameters(**dict(a.kw, PrecisionMode=bts.PREC128)), k)
    with pytest.raises(E, match="the moduli of ResidualRingQ are not Q\\[:ResidualMaxLevel \\+ 1\\]"):
        bts.Parameters(**dict(a.kw, ResidualRingQ=rh.Ring(256, a.s.Q[1:3])))
    B = a.bts[True]
    wide = B._like(a.ct, a.ct.Value)
    wide.LogDimensions = 9                                               # N1's LogMaxSlots is 7, the bootstrapping's 8
    with pytest.raises(E, match="cannot BootstrapMany: cannot PackAndSwitchN1ToN2: PackN1: cannot Pack: cts\\[0\\].LogSlots\\(\\)=9 > logMaxSlots=7"):
        B.BootstrapMany(wide)
    p = Arm(rh, "pack")
    wide = p.bts[True]._like(p.ct, p.ct.Value)
    wide.LogDimensions = 9
    with pytest.raises(E, match="cannot BootstrapMany: cannot PackAndSwitchN1ToN2: PackN1: cannot Pack: cts\\[0\\].LogSlots\\(\\)=9 > logMaxSlots=8"):
        p.bts[True].BootstrapMany(wide)
    with pytest.raises(E, match="cannot Pack: cts\\[0\\].Value\\[0\\].N\\(\\)=256 != params.N\\(\\)=1024"):
        p.bts[True].BootstrapMany(a.ct)                                  # a ring degree that is not the context's
    with pytest.raises(E, match="cannot EvaluateConjugateInvariant: the residual parameters are not conjugate-invariant"):
        B.EvaluateConjugateInvariant(a.ct)
    with pytest.raises(E, match="ctLeftN1Q0 cannot be nil"):
        c.bts[True].EvaluateConjugateInvariant(None)
    with pytest.raises(E, match="the ciphertexts have ring degree 256, the residual parameters 512"):
        c.bts[True].BootstrapMany(a.ct)

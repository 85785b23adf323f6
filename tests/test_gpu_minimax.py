"""GPU: rh_ckks_axpby (csrc/ckks.hip), the fused Chebyshev step of the power basis, and the minimax / comparison / inverse circuits with
bootstrapping.SecretKeyBootstrapper on device batches -- bit for bit, whole outputs, against tests/minimax_restatement.py and against
Python integers, fused and composed; ciphertexts are uploaded from the restatement, keys are real."""
import functools
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_restatement as ce
import ckks_restatement as cr
import keygen_restatement as kr
import minimax_restatement as mr
import polynomial_restatement as pr
import rlwe_restatement as rr
from oracle import primes
from test_gpu_cache_policy import policy
from test_gpu_ckks_evaluator import chain, uniform

pytestmark = pytest.mark.gpu

S = cr.Scale
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXED = (55, 45, 36, 61, 50)                                             # mixed-width chain
LOGN = 8
LONG = (55,) + (45,) * 10                                                # one level per rescaling: Goldschmidt at 2^-4 takes all 10 levels
LONG2 = (55,) + (45,) * 12                                               # two levels per rescaling: Step takes 10 levels, the extremum gate 2 more
CHAINS = {1: LONG, 2: LONG2}
SHORT = (55, 45, 45, 45, 45)                                             # X2 leaves level 2, X4 needs 3: the bootstrapper fires
X2X4 = [mr.X2, mr.X4]


# ---- rh_ckks_axpby -----------------------------------------------------------------------------------------------------------------------------------
def axpby_call(rh, ring, level, x, x_rows, t, t_rows, out, npoly, ra, rb, s0, s1):
    U = rh.ringhip.U64P
    p = lambda v: np.ascontiguousarray(v, dtype=np.uint64).ctypes.data_as(U) if v is not None else None
    ptr = lambda polys: [q.ptr if q is not None else None for q in polys] + [None] * (3 - len(polys))
    keep = [np.ascontiguousarray(v, dtype=np.uint64) if v is not None else None for v in (ra, rb, s0, s1)]
    a = [k.ctypes.data_as(U) if k is not None else None for k in keep]
    return rh.lib().rh_ckks_axpby(ring._h, level, *ptr(x), x_rows, *ptr(t), t_rows, *ptr(out), npoly, *a)


def axpby_ints(x, t, mods, ra, rb, s0, s1, first):
    """ra x - rb t - [first] s mod q in Python integers; x, t: (npoly, >= L, N) (t None: absent)"""
    L, N = len(mods), x.shape[2]
    out = np.zeros((x.shape[0], L, N), dtype=np.uint64)
    for k in range(x.shape[0]):
        for i, q in enumerate(mods):
            for j in range(N):
                v = int(ra[i]) * int(x[k, i, j])
                if t is not None:
                    v -= int(rb[i]) * int(t[k, i, j])
                if first and s0 is not None:
                    v -= int(s0[i] if j < N // 2 else s1[i])
                out[k, i, j] = v % q
    return out


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("logN,level,npoly", [(4, 0, 1), (4, 2, 3), (4, 4, 3), (12, 4, 1)])      # level 2 of 4 with 3 polys: the poly stride of x_rows, t_rows > level + 1
def test_axpby_kernel(rh, logN, level, npoly, nt):
    Q = chain(logN, MIXED)[0]
    N, mods = 1 << logN, Q[:level + 1]
    ring = rh.Ring(N, Q)
    rl = ring.AtLevel(level)
    rng = np.random.default_rng(logN * 10 + level + npoly)
    vec = lambda: np.array([int(rng.integers(0, q)) for q in mods], dtype=np.uint64)
    ra, rb, s0, s1 = vec(), vec(), vec(), vec()
    full = N <= 16 or nt == 0                                            # the Python-integer reference of every word at the small size; a stride at 2^12
    with policy(nt, ring):
        for xc, tc, xr, tr, const, inplace in [(2, 0, level + 1, 0, True, True), (3, 2, len(Q), level + 1, False, False), (2, 2, level + 1, len(Q), True, False),
                                               (3, 3, level + 1, level + 1, True, True), (3, 1, len(Q), len(Q), False, False), (1, 0, level + 1, 0, False, True)]:
            X = [np.stack([uniform(rng, Q[:xr], N) for _ in range(npoly)]) for _ in range(xc)]
            T = [np.stack([uniform(rng, Q[:tr], N) for _ in range(npoly)]) for _ in range(tc)]
            X[0][0, 0, :] = 0                                            # rows holding 0 and q - 1 throughout
            X[-1][-1, level, :] = mods[level] - 1
            if T:
                T[0][0, 0, :] = Q[0] - 1
            dx = [rh.DevicePoly.from_numpy(ring.AtLevel(xr - 1), b) for b in X]
            dt = [rh.DevicePoly.from_numpy(ring.AtLevel(tr - 1), b) for b in T]
            out = dx if inplace else [rl.NewPoly(npoly) for _ in range(xc)]
            sa, sb = (s0, s1) if const else (None, None)
            assert axpby_call(rh, ring, level, dx, xr, dt, tr, out, npoly, ra, rb if T else None, sa, sb) == 0, rh.lib().rh_last_error()
            for j in range(xc):
                got = out[j].numpy()
                if full:
                    assert np.array_equal(got, axpby_ints(X[j], T[j] if j < tc else None, mods, ra, rb, sa, sb, j == 0)), (xc, tc, j)
                # ... and the composed device calls: MulDoubleRNSScalar twice, Sub, SubDoubleRNSScalar
                a, b, w = rl.NewPoly(npoly), rl.NewPoly(npoly), rl.NewPoly(npoly)
                rl.CopyLvl(rh.DevicePoly.from_numpy(rl, np.ascontiguousarray(X[j][:, :level + 1])), w)
                rl.MulDoubleRNSScalar(w, [int(v) for v in ra], [int(v) for v in ra], a)
                if j < tc:
                    rl.MulDoubleRNSScalar(rh.DevicePoly.from_numpy(rl, np.ascontiguousarray(T[j][:, :level + 1])), [int(v) for v in rb], [int(v) for v in rb], b)
                    rl.Sub(a, b, a)
                if j == 0 and const:
                    rl.SubDoubleRNSScalar(a, [int(v) for v in s0], [int(v) for v in s1], a)
                assert np.array_equal(got, a.numpy()), (xc, tc, j, "composed")
            if not inplace:
                for d, h in zip(dx + dt, X + T):                         # inputs untouched
                    assert np.array_equal(d.numpy(), h)
    ring.close()


def test_axpby_refusals(rh):
    Q = chain(4, MIXED)[0]
    ring = rh.Ring(16, Q)
    L, level, npoly = rh.lib(), 2, 2
    rl = ring.AtLevel(level)
    a = [rl.NewPoly(npoly) for _ in range(6)]
    big = [ring.NewPoly(npoly) for _ in range(2)]
    one = np.ones(level + 1, dtype=np.uint64)
    call = lambda x, xr, t, tr, out, ra=one, rb=one, s0=None, s1=None, r=ring: axpby_call(rh, r, level, x, xr, t, tr, out, npoly, ra, rb, s0, s1)
    assert call([a[0]], level + 1, [], 0, [a[1]], rb=None) == 0
    assert call([a[0]], level, [], 0, [a[1]], rb=None) == -1 and b"fewer than level" in L.rh_last_error()
    assert call([a[0]], level + 1, [a[2]], level, [a[1]]) == -1 and b"t holds" in L.rh_last_error()
    assert call([a[0]], level + 1, [a[2], a[3]], level + 1, [a[1]]) == -1 and b"no more components than x" in L.rh_last_error()
    assert call([a[0]], level + 1, [a[2]], level + 1, [a[1]], rb=None) == -1 and b"null argument" in L.rh_last_error()
    assert call([a[0]], level + 1, [], 0, [a[1]], rb=None, s0=one) == -1 and b"null argument" in L.rh_last_error()
    assert call([a[0], a[1]], level + 1, [], 0, [a[2]], rb=None) == -1 and b"need an input and an output each" in L.rh_last_error()
    assert call([big[0]], len(Q), [], 0, [big[0]], rb=None) == -1 and b"without being that input at the same level" in L.rh_last_error()
    assert call([a[0]], level + 1, [big[1]], len(Q), [big[1]]) == -1 and b"without being that input at the same level" in L.rh_last_error()
    assert call([a[0], a[1]], level + 1, [], 0, [a[2], a[2]], rb=None) == -1 and b"two outputs overlap" in L.rh_last_error()
    over = np.array([Q[0], 0, 0], dtype=np.uint64)
    assert call([a[0]], level + 1, [], 0, [a[1]], ra=over, rb=None) == -1 and b"factor of limb 0 is not below its modulus" in L.rh_last_error()
    assert call([a[0]], level + 1, [], 0, [a[1]], rb=None, s0=over, s1=one) == -1 and b"constant of limb 0 is not below its modulus" in L.rh_last_error()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60, 60], [])[0], kind=rh.Matrix3N)
    assert call([a[0]], level + 1, [], 0, [a[1]], rb=None, r=r3) == -1 and b"3N rings are not supported" in L.rh_last_error()
    r3.close()
    ring.close()


# ---- a keyed context: real secret, relinearisation and conjugation keys, shared with the restatement ----------------------------------------------------------
class MCtx:
    _cache = {}

    def __new__(cls, rh, logQ, nb, logN=LOGN):
        key = (tuple(logQ), nb, logN)
        if key not in cls._cache:
            self = object.__new__(cls)
            self.Q, self.Pk = chain(logN, tuple(logQ))
            self.N, self.nb = 1 << logN, nb
            N, Q, Pk = self.N, self.Q, self.Pk
            self.rnd = random.Random(len(logQ) * 10 + nb)
            self.sk = rr.Secret.sample(self.rnd, N)
            rlk = rr.relin_key(self.rnd, self.sk, Q, Pk, len(Q) - 1, len(Pk) - 1)
            conj = rr.galois_key(self.rnd, self.sk, 2 * N - 1, Q, Pk, len(Q) - 1, len(Pk) - 1)
            self.scale, self.prec = 2 ** (45 * nb), max(53, 45 * nb)
            self.P = mr.Params(N, Q, Pk, rlk, conj, self.scale, None, nb, self.prec)
            self.rq, self.rp = rh.Ring(N, Q), rh.Ring(N, Pk)
            mk = lambda k: rh.rlwe.GadgetCiphertext(self.rq, self.rp, k.Q, k.P)
            self.enc = rh.ckks.Encoder(self.rq)
            self.ev = rh.ckks.Evaluator(self.rq, self.rp, rlk=mk(rlk), galois_keys={2 * N - 1: mk(conj)}, levels_consumed_per_rescaling=nb,
                                        encoding_precision=self.prec, encoder=self.enc)
            self.dsk = rh.rlwe.KeyGenerator(self.rq, self.rp).GenSecretKeyNew(samples=np.array(self.sk.coeffs, dtype=np.int32))
            cls._cache[key] = self
        return cls._cache[key]

    def sample(self, level=None):
        mods = self.Q if level is None else self.Q[:level + 1]
        return rr.uniform_poly(self.rnd, self.N, mods), np.array(rr.gaussian_coeffs(self.rnd, self.N), dtype=np.int32)

    def encrypt(self, values):
        """one restated ciphertext of the real slot values, at the top level and the default scale"""
        pt = ce.embed(np.asarray(values) + 0j, self.N.bit_length() - 2, float(self.scale), self.N, self.Q)
        c1, e = self.sample()
        return pr.Ct(kr.encrypt_sk(self.sk, self.Q, len(self.Q) - 1, c1, [int(v) for v in e], pt), S(self.scale))

    def decode(self, ct):
        re_, _ = ce.decode(kr.decrypt(ct.comps, self.sk, self.Q), self.N.bit_length() - 2, ct.scale.float64(), self.N, self.Q[:ct.level() + 1])
        return re_


def upload(rh, x, cts):
    """restated ciphertexts of one level -> a device batch"""
    out = rh.Ciphertext([rh.DevicePoly.from_numpy(x.rq.AtLevel(cts[0].level()), np.stack([c.comps[j] for c in cts])) for j in range(len(cts[0].comps))], is_ntt=True)
    out.Scale, out.LogDimensions = rh.ckks.Scale(cts[0].scale.v), x.N.bit_length() - 2
    return out


def same(out, want):
    assert out.Degree() + 1 == len(want[0].comps) and out.Level() == want[0].level() and out.IsNTT
    for j, v in enumerate(out.Value):
        assert np.array_equal(v.numpy(), np.stack([w.comps[j] for w in want])), "component %d" % j
    assert out.Scale.Value == want[0].scale.v


@functools.lru_cache(maxsize=None)
def inputs(logQ, nb, lo, hi, count=2, seed=0):
    x = MCtx._cache[(tuple(logQ), nb, LOGN)]
    rng = np.random.default_rng(7 + seed)
    vals = [rng.uniform(lo, hi, x.N // 2) for _ in range(count)]
    return vals, [x.encrypt(v) for v in vals]


# ---- PowerBasis.GenPower: fused == composed == the restatement -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_powers(nb, n, lazy):
    x = MCtx._cache[(CHAINS[nb], nb, LOGN)]
    out = []
    for ct in inputs(CHAINS[nb], nb, -1, 1)[1]:
        pb = {1: mr.copy_new(ct)}
        pr.gen_power(x.P, pb, pr.CHEBYSHEV, n, lazy)
        out.append(pb)
    return out


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("n", [2, 3, 4, 7, 8, 15])
def test_gen_power_chebyshev_step(rh, n, nb, lazy, fused):
    x = MCtx(rh, CHAINS[nb], nb)
    want = expected_powers(nb, n, lazy)
    pb = rh.polynomial.PowerBasis(upload(rh, x, inputs(CHAINS[nb], nb, -1, 1)[1]), rh.polynomial.Chebyshev, fused=fused)
    pb.GenPower(n, lazy, x.ev)
    assert sorted(pb.Value) == sorted(want[0])
    for k in pb.Value:
        same(pb.Value[k], [w[k] for w in want])


@functools.lru_cache(maxsize=None)
def small_product_powers():
    """T_a and T_b of 7 = a + b given at scales whose product, 3 x 2^38, is BELOW the scale 2^45 of T_|a - b| = T_1: the scale-matching Sub
    then multiplies the product's side by the integer ratio floor(2^45 / (3 x 2^38)) = 42 (in every generated power it is T_c's side that is
    multiplied, by a ratio near q: the product is not rescaled yet)"""
    x = MCtx._cache[(LONG, 1, LOGN)]
    a, b = pr.split_degree(7)
    assert abs(a - b) == 1 and {a, b} == {3, 4}
    rand = lambda scale: [pr.Ct([rr.uniform_poly(x.rnd, x.N, x.Q) for _ in range(2)], S(scale)) for _ in range(2)]
    given = {1: inputs(LONG, 1, -1, 1)[1], a: rand(2 ** 20), b: rand(3 * 2 ** 18)}
    want = []
    for k in range(2):
        pb = {p: mr.copy_new(v[k]) for p, v in given.items()}
        pr.gen_power(x.P, pb, pr.CHEBYSHEV, 7, False)
        want.append(pb[7])
    return given, want


@pytest.mark.parametrize("fused", [True, False])
def test_gen_power_scales_the_product_side(rh, fused):
    x = MCtx(rh, LONG, 1)
    given, want = small_product_powers()
    pb = rh.polynomial.PowerBasis(upload(rh, x, given[1]), rh.polynomial.Chebyshev, fused=fused)
    for p, cts in given.items():
        if p != 1:
            pb.Value[p] = upload(rh, x, cts)
    pb.GenPower(7, False, x.ev)
    same(pb.Value[7], want)
    assert pb.Value[7].Level() == len(x.Q) - 2 and abs(want[0].scale.float64() * x.Q[-1] / 2.0 ** 45 - 1) < 2.0 ** -50   # T_1's scale, rescaled once


# ---- minimax.Evaluate, Sign / Step / Max / Min, the inverse circuits ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected(nb, what):
    x = MCtx._cache[(CHAINS[nb], nb, LOGN)]
    mcp = mr.new_polynomial(X2X4)
    cts = inputs(CHAINS[nb], nb, -1, 1)[1]
    half = inputs(CHAINS[nb], nb, -0.5, 0.5, 4, 1)[1]
    if what == "evaluate":
        return [mr.evaluate(x.P, ct, mcp) for ct in cts]
    if what == "step":
        return [mr.step(x.P, ct, mcp) for ct in cts]
    if what == "max":
        return [mr.maximum(x.P, half[k], half[2 + k], mcp) for k in range(2)]
    if what == "min":
        return [mr.minimum(x.P, half[k], half[2 + k], mcp) for k in range(2)]
    raise KeyError(what)


def circuits(rh, x, fused, btp=None):
    mm = rh.minimax.Evaluator(x.ev, btp, x.scale, fused=fused)
    return mm, rh.comparison.Evaluator(mm, rh.minimax.Polynomial(X2X4)), rh.inverse.Evaluator(mm)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("nb", [1, 2])
def test_minimax_evaluate(rh, nb, fused, monkeypatch):
    x = MCtx(rh, CHAINS[nb], nb)
    monkeypatch.setitem(rh.polynomial.FUSED_POWER_BASIS, "chebyshev_step", fused)
    mm, cmp_, _ = circuits(rh, x, fused)
    ct = upload(rh, x, inputs(CHAINS[nb], nb, -1, 1)[1])
    before = [v.numpy() for v in ct.Value]
    out = mm.Evaluate(ct, cmp_.MinimaxCompositeSignPolynomial)
    same(out, expected(nb, "evaluate"))
    assert out.Level() == len(x.Q) - 1 - 5 * nb and out.Scale.Value == x.scale
    for v, h in zip(ct.Value, before):
        assert np.array_equal(v.numpy(), h)
    same(cmp_.Sign(ct), expected(nb, "evaluate"))


@pytest.mark.parametrize("what", ["step", "max", "min"])
@pytest.mark.parametrize("nb", [1, 2])
def test_comparisons(rh, nb, what):
    x = MCtx(rh, CHAINS[nb], nb)
    _, cmp_, _ = circuits(rh, x, None)
    if what == "step":
        out = cmp_.Step(upload(rh, x, inputs(CHAINS[nb], nb, -1, 1)[1]))
    else:
        half = inputs(CHAINS[nb], nb, -0.5, 0.5, 4, 1)[1]
        out = (cmp_.Max if what == "max" else cmp_.Min)(upload(rh, x, half[:2]), upload(rh, x, half[2:]))
    same(out, expected(nb, what))


class Sampled:
    """a bootstrapper that hands SecretKeyBootstrapper.Bootstrap the samples the restatement draws"""

    def __init__(self, btp, samples):
        self.btp, self.samples = btp, iter(samples)
        self.MinimumInputLevel, self.OutputLevel, self.Depth = btp.MinimumInputLevel, btp.OutputLevel, btp.Depth

    def Bootstrap(self, ct):
        c1, e = next(self.samples)
        return self.btp.Bootstrap(ct, samples={"c1": c1, "e": e})


def test_minimax_evaluate_bootstraps_on_a_short_chain(rh):
    x = MCtx(rh, SHORT, 1)
    vals = [np.random.default_rng(k).uniform(-1, 1, x.N // 2) for k in range(2)]
    cts = [x.encrypt(v) for v in vals]
    samples = [[x.sample() for _ in range(2)] for _ in range(2)]         # per bootstrapping, per ciphertext of the batch
    mcp = mr.new_polynomial(X2X4)
    want = []
    for k, ct in enumerate(cts):
        btp = mr.SkBootstrapper(x.N, x.Q, x.sk, x.scale, [(s[k][0], [int(v) for v in s[k][1]]) for s in samples])
        P = mr.Params(x.N, x.Q, x.Pk, x.P.rlk, x.P.conj, x.scale, btp, 1, 53)
        want.append(mr.evaluate(P, ct, mcp))
        assert btp.counter == 1
    sk_btp = rh.bootstrapping.SecretKeyBootstrapper(x.rq, x.dsk, x.enc, x.scale)
    btp = Sampled(sk_btp, [(np.stack([s[0][0], s[1][0]]), np.stack([s[0][1], s[1][1]])) for s in samples])
    mm, cmp_, _ = circuits(rh, x, None, btp)
    out = mm.Evaluate(upload(rh, x, cts), cmp_.MinimaxCompositeSignPolynomial)
    assert sk_btp.Counter == 1 and (sk_btp.Depth(), sk_btp.MinimumInputLevel(), sk_btp.OutputLevel()) == (0, 0, len(x.Q) - 1)
    same(out, want)
    got = x.decode(want[0])
    assert np.max(np.abs(got - np.array([float(mr.evaluate_exact(mcp, Fraction(v))[0]) for v in vals[0]]))) < 2.0 ** -20


@functools.lru_cache(maxsize=None)
def expected_inverse(what):
    x = MCtx._cache[(LONG, 1, LOGN)]
    rng = np.random.default_rng(11)
    if what == "goldschmidt":
        cts = [x.encrypt(rng.uniform(2.0 ** -4, 2 - 2.0 ** -4, x.N // 2)) for _ in range(2)]
        return cts, [mr.goldschmidt_division(x.P, ct, -4.0) for ct in cts]
    cts = [x.encrypt(rng.uniform(-8, 8, x.N // 2)) for _ in range(2)]
    res = [mr.interval_normalization(x.P, ct, 3.0) for ct in cts]
    return cts, ([r[0] for r in res], [r[1] for r in res])


@pytest.mark.parametrize("fused", [True, False])
def test_goldschmidt_and_interval_normalization(rh, fused):
    x = MCtx(rh, LONG, 1)
    _, _, inv = circuits(rh, x, fused)
    cts, want = expected_inverse("goldschmidt")
    same(inv.GoldschmidtDivisionNew(upload(rh, x, cts), -4.0), want)
    cts, (norm, fac) = expected_inverse("normalization")
    got = inv.IntervalNormalization(upload(rh, x, cts), 3.0, None)
    same(got[0], norm)
    same(got[1], fac)


DOMAINS = {"positive": (2.0 ** -4, 8, 41), "negative": (-8, -2.0 ** -4, 42), "full": (-8, 8, 43)}      # lo, hi, seed
NBOOT = 24                                                               # sample pairs drawn per ciphertext: more than any domain uses


@functools.lru_cache(maxsize=None)
def expected_domain(domain):
    """1 / x on [2^-4, 8], [-8, -2^-4] and their union over the 10 levels of LONG: the normalization takes 9, Goldschmidt's 10 iterations and
    the products after them do not fit, so the secret-key bootstrapper fires at the reference's conditions, the same number of times for
    every ciphertext -> (ciphertexts, samples per bootstrapping, expected, bootstrappings)"""
    x = MCtx._cache[(LONG, 1, LOGN)]
    lo, hi, seed = DOMAINS[domain]
    rng = np.random.default_rng(seed)
    cts = [x.encrypt(rng.uniform(lo, hi, x.N // 2)) for _ in range(2)]
    samples = [[x.sample() for _ in range(2)] for _ in range(NBOOT)]
    mcp = mr.new_polynomial(X2X4)
    want, counts = [], []
    for k, ct in enumerate(cts):
        btp = mr.SkBootstrapper(x.N, x.Q, x.sk, x.scale, [(s[k][0], [int(v) for v in s[k][1]]) for s in samples])
        P = mr.Params(x.N, x.Q, x.Pk, x.P.rlk, x.P.conj, x.scale, btp, 1, 53)
        want.append(mr.inverse_negative(P, ct, -4.0, 3.0) if domain == "negative" else mr.inverse(P, ct, -4.0, 3.0, domain == "full", mcp))
        counts.append(btp.counter)
    assert counts[0] == counts[1] and 1 <= counts[0] < NBOOT
    return cts, samples, want, counts[0]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("domain", ["positive", "negative", "full"])
def test_inverse_domains(rh, domain, fused):
    x = MCtx(rh, LONG, 1)
    cts, samples, want, count = expected_domain(domain)
    sk_btp = rh.bootstrapping.SecretKeyBootstrapper(x.rq, x.dsk, x.enc, x.scale)
    btp = Sampled(sk_btp, [(np.stack([s[0][0], s[1][0]]), np.stack([s[0][1], s[1][1]])) for s in samples])
    _, cmp_, inv = circuits(rh, x, fused, btp)
    ct = upload(rh, x, cts)
    before = [v.numpy() for v in ct.Value]
    if domain == "positive":
        out = inv.EvaluatePositiveDomainNew(ct, -4.0, 3.0)
    elif domain == "negative":
        out = inv.EvaluateNegativeDomainNew(ct, -4.0, 3.0)
    else:
        out = inv.EvaluateFullDomainNew(ct, -4.0, 3.0, cmp_.MinimaxCompositeSignPolynomial)
    assert sk_btp.Counter == count
    same(out, want)
    for v, h in zip(ct.Value, before):                                   # the input is left as it was
        assert np.array_equal(v.numpy(), h)


# ---- refusals and the reference's errors --------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_errors(rh):
    from conftest import QI60
    x = MCtx(rh, SHORT, 1)
    mm, cmp_, inv = circuits(rh, x, None)
    ct = upload(rh, x, [x.encrypt(np.zeros(x.N // 2))])
    deep = rh.minimax.Polynomial([["0", "1"] + ["0"] * 62])             # depth 6 > 4 levels
    with pytest.raises(rh.RingHipError, match="parameters do not enable the evaluation of the minimax composite polynomial, required levels is 6 but parameters only provide 4 levels"):
        mm.Evaluate(ct, deep)
    with pytest.raises(rh.RingHipError, match="needs a bootstrapping, and the bootstrapper is nil"):
        mm.Evaluate(ct, cmp_.MinimaxCompositeSignPolynomial)
    with pytest.raises(rh.RingHipError, match=r"cannot GoldschmidtDivisionNew: ct.Level\(\)=4 < depth=\d+ and rlwe.Bootstrapper is nil"):
        inv.GoldschmidtDivisionNew(ct, -4.0)
    with pytest.raises(rh.RingHipError, match="MinimaxCompositePolynomialEvaluator is nil but fulldomain is set to true"):
        rh.inverse.Evaluator(None).EvaluateFullDomainNew(ct, -4.0, 3.0, cmp_.MinimaxCompositeSignPolynomial)
    with pytest.raises(rh.RingHipError, match="sign polynomial is mandatory"):
        rh.comparison.Evaluator(mm, None)
    with pytest.raises(rh.RingHipError, match="sign polynomial is mandatory"):
        inv.EvaluateFullDomainNew(ct, -4.0, 3.0)
    ci = rh.Ring(x.N, QI60[:4], kind=rh.ConjugateInvariant)
    with pytest.raises(rh.RingHipError, match="conjugate-invariant and 3N rings are not supported"):
        rh.minimax.Evaluator(rh.ckks.Evaluator(ci), None, 2 ** 45)
    ci.close()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    with pytest.raises(rh.RingHipError, match="3N rings are not supported"):
        rh.minimax.Evaluator(rh.ckks.Evaluator(r3), None, 2 ** 45)
    r3.close()


# ---- end to end: keys from a KeyedPRNG on the device, the fixture polynomial ------------------------------------------------------------------------------------
def test_sign_end_to_end_with_device_keys(rh):
    """N = 2^10, Prec45 (LogQ {55, 45 x 11}, LogP {60, 60}, scale 2^45): encode -> encrypt -> Sign -> decrypt -> decode with no host key material;
    every slot with |x| >= 2^-4 is within 2^-10 of sign(x) -- a sanity bound with wide margin over the polynomial's stated 2^-21, which
    tests/test_minimax_oracle.py::test_sign_at_prec45_meets_the_sanity_bound holds the restatement to first (2^-32.9 there)"""
    Q, Pk = primes.gen_moduli(11, [55] + [45] * 11, [60, 60])
    N, Q, Pk = 1 << 10, [int(q) for q in Q], [int(p) for p in Pk]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, Pk)
    prng = rh.rlwe.KeyedPRNG(b"minimax end to end")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = kg.GenSecretKeyNew()
    evs = rh.rlwe.MemEvaluationKeySet(kg.GenRelinearizationKeyNew(sk), kg.GenGaloisKeysNew([2 * N - 1], sk))
    ecd = rh.ckks.Encoder(rq)
    ev = rh.ckks.Evaluator(rq, rp, rlk=evs.RelinearizationKey, galois_keys=evs.GaloisKeys, encoder=ecd)
    btp = rh.bootstrapping.SecretKeyBootstrapper(rq, sk, ecd, 2 ** 45, prng=prng)
    mm = rh.minimax.Evaluator(ev, btp, 2 ** 45)
    poly = rh.minimax.Polynomial.from_json(os.path.join(ROOT, "tests", "golden", "minimax_default_sign.json"), [rh.minimax.CoeffsSignX4Cheby])
    cmp_ = rh.comparison.Evaluator(mm, poly)
    x = np.random.default_rng(21).uniform(-1, 1, (2, N // 2))
    pt = ecd.NewPlaintext(len(Q) - 1, 2 ** 45, nvec=2)
    ecd.Encode(x + 0j, pt)
    ct = rh.ckks.Encryptor(rq, None, sk, prng=prng).EncryptNew(pt)
    out = cmp_.Sign(ct)
    assert btp.Counter >= 1 and out.Scale.Value == 2 ** 45
    got = np.asarray(ecd.Decode(rh.ckks.Decryptor(rq, sk).DecryptNew(out))).reshape(2, -1).real
    keep = np.abs(x) >= 2.0 ** -4
    worst = np.max(np.abs(got - np.sign(x))[keep])
    print("MEASURED Sign end to end: largest error 2^%.2f over %d slots, %d bootstrappings" % (np.log2(worst), keep.sum(), btp.Counter))
    assert worst < 2.0 ** -10
    ev.close()
    ecd.close()
    rq.close()
    rp.close()

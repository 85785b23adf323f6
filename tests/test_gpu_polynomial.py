"""GPU: polynomial evaluation on device (csrc/ckks.hip: rh_ckks_linear_combination; matrix-fhe-lattigo_amd/polynomial.py) bit for bit, whole
outputs, against tests/polynomial_restatement.py, which tests/test_polynomial_oracle.py pins to exact arithmetic and to decryption -- with the
fused baby step and with the composed sequence of evaluator calls, under every cache policy; keys are random."""
import ctypes as C
import functools
import types
from fractions import Fraction

import numpy as np
import pytest

import ckks_restatement as cr
import polynomial_restatement as pr
import rlwe_restatement as rr
from oracle import primes
from test_gpu_cache_policy import policy
from test_gpu_ckks_evaluator import Ctx, chain, uniform

pytestmark = pytest.mark.gpu

S = cr.Scale
# (logN, chain, level, npoly): N = 32 has N/2 = 16 inside one wavefront and three polys give a ragged grid tail; a mixed-width chain whose terms
# are stored at level 2 (strided AtLevel views); logN 13: more than one block per limb
SHAPES = [(5, (61, 61), 1, 3), (10, (55, 45, 45), 1, 4), (13, (61, 61), 1, 2)]
CHUNK, WIDTH = 56, 4                                                     # rh_ckks_linear_combination_chunk() / _width(), asserted below
TERMS = (0, 1, 2, 7, WIDTH - 1, WIDTH, WIDTH + 1, CHUNK, CHUNK + 1)
LONG = (55, 45, 45, 45, 45, 45, 45)                                      # the 7-limb chain of the reference's own test


# ---- rh_ckks_linear_combination through ctypes, synthetic power bases ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lc_case(logN, logQ, level, npoly):
    """CHUNK + 1 terms of three components; term k holds rows[k] limbs per poly (every second one the whole chain where it is longer than the
    level).  prefix[K][j]: the reference sequence's accumulator after K terms (every step CRed(acc + MRed(x, MForm(s))))"""
    Q = chain(logN, logQ)[0]
    mods, N = Q[:level + 1], 1 << logN
    rng = np.random.default_rng(logN * 10 + npoly)
    rows = [len(Q) if k % 2 == 0 else level + 1 for k in range(CHUNK + 1)]
    X = [[np.stack([uniform(rng, Q[:r], N) for _ in range(npoly)]) for _ in range(3)] for r in rows]
    s0 = np.stack([np.array([rng.integers(0, q) for q in mods], dtype=np.uint64) for _ in rows])
    s1 = np.stack([np.array([rng.integers(0, q) for q in mods], dtype=np.uint64) for _ in rows])
    s0[1], s1[1] = np.array([q - 1 for q in mods], dtype=np.uint64), np.zeros(len(mods), dtype=np.uint64)
    consts = {"none": None, "zero": (np.zeros(len(mods), dtype=np.uint64),) * 2,
              "real": (np.array([q - 3 for q in mods], dtype=np.uint64),) * 2,
              "complex": (np.array([q - 1 for q in mods], dtype=np.uint64), np.array([rng.integers(0, q) for q in mods], dtype=np.uint64))}
    zero = np.zeros((len(mods), N), dtype=np.uint64)
    prefix = [[[zero] * npoly for _ in range(3)]]
    for k in range(CHUNK + 1):
        prefix.append([[cr.mul_double_then_add(X[k][j][p][:level + 1], [int(v) for v in s0[k]], [int(v) for v in s1[k]], prefix[-1][j][p], mods)
                        for p in range(npoly)] for j in range(3)])
    for blocks in X:
        for b in blocks:
            b.setflags(write=False)
    return Q, mods, rows, X, s0, s1, consts, prefix


def lc_call(rh, ring, level, terms, rows, s0, s1, const, outs, table, npoly):
    """terms: K lists of device blocks; returns the status"""
    K, U = len(terms), rh.ringhip.U64P
    x = (C.c_void_p * max(3 * K, 1))()
    r = (C.c_int * max(K, 1))(*rows[:K])
    for k, t in enumerate(terms):
        for j, p in enumerate(t):
            x[3 * k + j] = p.ptr
    a, b = np.ascontiguousarray(s0[:K]).reshape(-1), np.ascontiguousarray(s1[:K]).reshape(-1)
    c0, c1 = (None, None) if const is None else (np.ascontiguousarray(const[0]), np.ascontiguousarray(const[1]))
    p = lambda v: v.ctypes.data_as(U) if v is not None and v.size else None
    ptrs = [o.ptr for o in outs] + [None] * (3 - len(outs))
    return rh.lib().rh_ckks_linear_combination(ring._h, level, K, x, r, p(a), p(b), p(c0), p(c1), *ptrs, npoly,
                                               table.ptr if table is not None else None, table.words if table is not None else 0)


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_linear_combination_kernel(rh, logN, logQ, level, npoly, nt):
    L = rh.lib()
    assert (L.rh_ckks_linear_combination_chunk(), L.rh_ckks_linear_combination_width()) == (CHUNK, WIDTH)
    c = Ctx(rh, logN, logQ)
    Q, mods, rows, X, s0, s1, consts, prefix = lc_case(logN, logQ, level, npoly)
    rl = c.rq.AtLevel(level)
    dev = [[rh.DevicePoly.from_numpy(c.rq.AtLevel(rows[k] - 1), b) for b in X[k]] for k in range(CHUNK + 1)]
    table = rh.DevicePoly(rl, 1, -(-L.rh_ckks_linear_combination_table_words(CHUNK + 1, level) // c.N))
    kinds = list(consts)
    with policy(nt, c.rq):
        for i, K in enumerate(TERMS):
            for nc in (1, 2, 3):
                kind = kinds[(i + nc) % 4] if K else kinds[1 + (i + nc) % 3]       # no terms: a constant alone
                outs = [rl.NewPoly(npoly) for _ in range(nc)]
                assert lc_call(rh, c.rq, level, [t[:nc] for t in dev[:K]], rows, s0, s1, consts[kind], outs, table, npoly) == 0, L.rh_last_error()
                for j in range(nc):
                    want = np.stack(prefix[K][j])
                    if j == 0 and consts[kind] is not None:
                        want = np.stack([cr.add_double(w, [int(v) for v in consts[kind][0]], [int(v) for v in consts[kind][1]], mods) for w in want])
                    assert np.array_equal(outs[j].numpy(), want), (K, nc, kind, j)
        for k in (0, 1, WIDTH, CHUNK):                                   # inputs untouched
            for j in range(3):
                assert np.array_equal(dev[k][j].numpy(), X[k][j])


@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_linear_combination_sums_that_fill_the_chunk(rh, logN, logQ, level, npoly):
    """every word q_i - 1, every scalar q_i - 1, the constant q_i - 1: K = CHUNK is the largest sum the 128-bit accumulator is sized for
    (and CHUNK + 1 starts a second chunk).  Expected with Python integers."""
    c = Ctx(rh, logN, logQ)
    mods, N = c.Q[:level + 1], c.N
    rl = c.rq.AtLevel(level)
    full = np.stack([np.stack([np.full(N, q - 1, dtype=np.uint64) for q in mods])] * npoly)
    block = rh.DevicePoly.from_numpy(rl, full)
    top = np.array([q - 1 for q in mods], dtype=np.uint64)
    table = rh.DevicePoly(rl, 1, -(-rh.lib().rh_ckks_linear_combination_table_words(CHUNK + 1, level) // N))
    for nt in (0, 2):
        with policy(nt, c.rq):
            for K in (CHUNK, CHUNK + 1):
                outs = [rl.NewPoly(npoly) for _ in range(3)]
                sc = np.stack([top] * K)
                assert lc_call(rh, c.rq, level, [[block] * 3] * K, [level + 1] * K, sc, sc, (top, top), outs, table, npoly) == 0
                for j, o in enumerate(outs):
                    want = np.stack([np.stack([np.full(N, (K * (q - 1) * (q - 1) + (q - 1 if j == 0 else 0)) % q, dtype=np.uint64) for q in mods])] * npoly)
                    assert np.array_equal(o.numpy(), want), (K, j)
    assert np.array_equal(block.numpy(), full)


def test_linear_combination_refusals(rh):
    logN, logQ, level, npoly = SHAPES[1]
    c = Ctx(rh, logN, logQ)
    L, rl = rh.lib(), c.rq.AtLevel(level)
    mods = c.Q[:level + 1]
    a = [rl.NewPoly(npoly) for _ in range(4)]
    table = rh.DevicePoly(rl, 1, 1)
    one = np.ones((1, level + 1), dtype=np.uint64)
    call = lambda terms, s, outs, tab, ring=c.rq, rows=(level + 1,): lc_call(rh, ring, level, terms, list(rows), s, s, None, outs, tab, npoly)
    assert call([[a[0]]], one, [a[0]], table) == -1 and b"overlaps a term" in L.rh_last_error()
    assert call([[a[0], a[1]]], one, [a[2], a[1]], table) == -1 and b"overlaps a term" in L.rh_last_error()
    big = np.array([[mods[0], 0]], dtype=np.uint64)
    assert call([[a[0]]], big, [a[1]], table) == -1 and b"not below its modulus" in L.rh_last_error()
    assert call([[a[0]]], one, [a[1]], None) == -1 and b"null table" in L.rh_last_error()
    assert call([[a[0]]], one, [a[1]], table, rows=(level,)) == -1 and b"fewer than level" in L.rh_last_error()
    assert call([[a[0]]], one, [a[1], a[2]], table) == -1 and b"has no component 1" in L.rh_last_error()
    tiny = rh.DevicePoly(c.rq.AtLevel(0), 1, 1, ptr=table.ptr, owner=table)
    tiny.words = 3
    assert call([[a[0]]], one, [a[1]], tiny) == -1 and b"the table holds 3 words" in L.rh_last_error()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    assert call([[a[0]]], one, [a[1]], table, ring=r3) == -1 and b"3N rings are not supported" in L.rh_last_error()
    r3.close()


# ---- the evaluator's own context: both evaluators of a chain, with an encoder on the standard ring ------------------------------------------------------
class PCtx:
    _cache = {}

    def __new__(cls, rh, logN, logQ=LONG):
        key = (logN, tuple(logQ))
        if key not in cls._cache:
            self = object.__new__(cls)
            c = self.c = Ctx(rh, logN, logQ)
            self.N, self.Q, self.Pk, self.rq = c.N, c.Q, c.Pk, c.rq
            self.enc = rh.ckks.Encoder(c.rq)
            rlk = rh.rlwe.GadgetCiphertext(c.rq, c.rp, *c.rlk)
            self.ev = {f: rh.ckks.Evaluator(c.rq, c.rp, rlk=rlk, fused=f, encoder=self.enc) for f in (True, False)}
            self.pe = {f: rh.polynomial.PolynomialEvaluator(self.ev[f]) for f in (True, False)}
            self.P = pr.Params(c.N, c.Q, c.Pk, rr.GadgetKey(c.rlk[0], c.rlk[1], len(c.Q) - 1, len(c.Pk) - 1, 0, None))
            cls._cache[key] = self
        return cls._cache[key]


def dev_ct(rh, c, blocks, scale):
    """blocks: per component (npoly, limbs, N)"""
    out = rh.Ciphertext([rh.DevicePoly.from_numpy(c.rq.AtLevel(b.shape[1] - 1), b) for b in blocks], is_ntt=True)
    out.Scale = rh.ckks.Scale(scale)
    return out


def same(out, want):
    """out: a device Ciphertext of npoly; want: npoly restated Cts"""
    assert out.Degree() + 1 == len(want[0].comps) and out.Level() == want[0].level() and out.IsNTT
    for j, v in enumerate(out.Value):
        assert np.array_equal(v.numpy(), np.stack([w.comps[j] for w in want])), "component %d" % j
    assert out.Scale.Value == want[0].scale.v


def rand_ct(c, rng, level, npoly, degree=1):
    return [np.stack([uniform(rng, c.Q[:level + 1], c.N) for _ in range(npoly)]) for _ in range(degree + 1)]


COEFFS = {"complex": [0.5 - 0.25j, 1.25, -0.75j, 0.3 + 0.1j, -1.5, 0.125j, 2.0 ** -7, 0.9 - 0.9j],
          "integer": [2, -3 + 1j, 0.5, 7],             # with a power at the target scale: X^1's constant is a Gaussian integer (scale 1)
          "rescales": [0.5, 0.25, 1.5, -0.75]}          # the same basis, a constant that is not one: the accumulator is rescaled mid-sum


@functools.lru_cache(maxsize=None)
def basis_case(logN, name, npoly):
    """a synthetic power basis X^1 .. X^K at levels >= the target level 2 (or one below it) with scales below the target scale (or at it)"""
    c = chain(logN, LONG)
    Q, N = c[0], 1 << logN
    co = COEFFS["complex" if name in ("fits", "below") else name]
    K = len(co) - 1
    rng = np.random.default_rng(logN + K)
    q_ = types.SimpleNamespace(Q=Q, N=N)                                 # what rand_ct reads
    target_level, target_scale = 2, S(2 ** 45).mul(S(Q[2]))
    levels = [2 + (k % 3) for k in range(K + 1)]
    scales = [S(2 ** 45 + 12345 * k) for k in range(K + 1)]
    if name in ("integer", "rescales"):
        scales[1] = target_scale
    if name == "below":
        levels[2] = 1
    blocks = {k: rand_ct(q_, rng, levels[k], npoly) for k in range(1, K + 1)}
    return co, target_level, target_scale, blocks, scales


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["fits", "integer", "rescales", "below"])
@pytest.mark.parametrize("logN", [5, 10])
def test_evaluate_polynomial_vector_from_power_basis(rh, logN, name, fused, nt):
    """the baby step alone: the fused launch where it fits, and the two cases that fall back to the composed sequence"""
    npoly = 3
    x = PCtx(rh, logN)
    co, target_level, target_scale, blocks, scales = basis_case(logN, name, npoly)
    P = rh.polynomial
    pol = P.PolynomialVector([P.Polynomial(P.Monomial, co)])
    pb = P.PowerBasis(dev_ct(rh, x.c, blocks[1], scales[1].v), P.Monomial)
    for k, b in blocks.items():
        pb.Value[k] = dev_ct(rh, x.c, b, scales[k].v)
    with policy(nt, x.rq):
        out = x.pe[fused].EvaluatePolynomialVectorFromPowerBasis(target_level, pol, pb, target_scale.v)
    want = []
    for p in range(npoly):
        ref = {k: pr.Ct([comp[p] for comp in b], scales[k]) for k, b in blocks.items()}
        want.append(pr.evaluate_from_power_basis(x.P, target_level, [pr.Poly(pr.MONOMIAL, co)], None, ref, target_scale))
    same(out, want)
    assert out.Level() == (1 if name == "below" else target_level)
    assert (out.Scale.Value == target_scale.v) == (name != "rescales")
    for k, b in blocks.items():                                         # inputs untouched
        for v, h in zip(pb.Value[k].Value, b):
            assert np.array_equal(v.numpy(), h)


# ---- PowerBasis.GenPower ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def input_ct(logN, npoly):
    Q = chain(logN, LONG)[0]
    rng = np.random.default_rng(logN * 7 + npoly)
    return [np.stack([uniform(rng, Q, 1 << logN) for _ in range(npoly)]) for _ in range(2)]


@functools.lru_cache(maxsize=None)
def expected_powers(logN, npoly, basis, n, lazy):
    Q, Pk = chain(logN, LONG)
    c = Ctx._cache[(logN, LONG)]
    Pm = pr.Params(1 << logN, Q, Pk, rr.GadgetKey(c.rlk[0], c.rlk[1], len(Q) - 1, len(Pk) - 1, 0, None))
    blocks = input_ct(logN, npoly)
    out = []
    for p in range(npoly):
        pb = {1: pr.Ct([b[p].copy() for b in blocks], S(2 ** 45))}
        pr.gen_power(Pm, pb, basis, n, lazy)
        out.append(pb)
    return out


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("basis", [pr.MONOMIAL, pr.CHEBYSHEV])
@pytest.mark.parametrize("n", [2, 3, 7, 8, 15])
def test_gen_power(rh, n, basis, lazy, fused, nt):
    logN, npoly = 5, 2
    x = PCtx(rh, logN)
    want = expected_powers(logN, npoly, basis, n, lazy)
    blocks = input_ct(logN, npoly)
    pb = rh.polynomial.PowerBasis(dev_ct(rh, x.c, blocks, 2 ** 45), basis)
    with policy(nt, x.rq):
        pb.GenPower(n, lazy, x.ev[fused])
    assert sorted(pb.Value) == sorted(want[0])
    for k in pb.Value:
        same(pb.Value[k], [w[k] for w in want])
    assert pb.Value[n].Degree() == (2 if lazy else 1)


# ---- Evaluate end to end ----------------------------------------------------------------------------------------------------------------------------
def poly_case(name, slots):
    rng = np.random.default_rng(len(name))
    if name == "monomial7":
        return pr.MONOMIAL, [float(Fraction(1, f)) for f in (1, 1, 2, 6, 24, 120, 720, 5040)], None, None
    if name == "chebyshev31":
        return pr.CHEBYSHEV, [complex(a, b) for a, b in rng.uniform(-1, 1, (32, 2))], (-1, 1), None
    if name == "degree5":                                               # Lead and MaxDeg = 5 > 8 - 2: recursePS splits once more
        return pr.MONOMIAL, [complex(a, b) for a, b in rng.uniform(-1, 1, (6, 2))], None, None
    return pr.MONOMIAL, [float(Fraction(1, f)) for f in (1, 1, 2, 6, 24, 120, 720, 5040)], None, {0: list(range(0, slots, 2))}


@functools.lru_cache(maxsize=None)
def expected_evaluate(logN, npoly, name):
    Q, Pk = chain(logN, LONG)
    c = Ctx._cache[(logN, LONG)]
    Pm = pr.Params(1 << logN, Q, Pk, rr.GadgetKey(c.rlk[0], c.rlk[1], len(Q) - 1, len(Pk) - 1, 0, None))
    basis, co, interval, mapping = poly_case(name, (1 << logN) // 2)
    blocks = input_ct(logN, npoly)
    p = pr.Poly(basis, co, interval or (0, 0))
    return [pr.evaluate(Pm, pr.Ct([b[k] for b in blocks], S(2 ** 45)), [p], mapping, S(2 ** 45)) for k in range(npoly)], p.depth()


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", ["monomial7", "chebyshev31", "degree5", "vector"])
@pytest.mark.parametrize("logN", [5, 10])
def test_evaluate(rh, logN, name, fused, nt):
    npoly = 2
    x = PCtx(rh, logN)
    want, depth = expected_evaluate(logN, npoly, name)
    basis, co, interval, mapping = poly_case(name, x.N // 2)
    P = rh.polynomial
    pol = P.Polynomial(basis, co, interval)
    if mapping is not None:
        pol = P.PolynomialVector([pol], mapping)
    blocks = input_ct(logN, npoly)
    ct = dev_ct(rh, x.c, blocks, 2 ** 45)
    with policy(nt, x.rq):
        out = x.pe[fused].Evaluate(ct, pol, 2 ** 45)
    same(out, want)
    assert out.Level() == len(x.Q) - 1 - depth and out.Degree() == 1
    assert P.InDelta(out.Scale, 2 ** 45, float(P.ScalePrecision - 12))
    for v, h in zip(ct.Value, blocks):                                   # the input is untouched: the power basis works on a copy
        assert np.array_equal(v.numpy(), h)


# ---- the named refusals ---------------------------------------------------------------------------------------------------------------------------
def test_named_refusals(rh):
    from conftest import QI60
    x = PCtx(rh, 5)
    P = rh.polynomial
    pe = x.pe[True]
    ct = dev_ct(rh, x.c, input_ct(5, 2), 2 ** 45)
    lazy = P.Polynomial(P.Monomial, [1, 2, 3, 4, 5, 6, 7, 8])
    lazy.Lazy = True
    with pytest.raises(rh.RingHipError, match="Lazy = true.*mixed degrees.*third component"):
        pe.Evaluate(ct, lazy, 2 ** 45)
    pb = P.PowerBasis(ct, P.Monomial)
    pb.GenPower(3, True, x.ev[True])                                     # X^3 of degree 2 next to X^1, X^2 of degree 1: supported
    assert [pb.Value[k].Degree() for k in (1, 2, 3)] == [1, 1, 2]
    with pytest.raises(rh.RingHipError, match="mixed degrees.*third component"):
        pe.EvaluatePolynomialVectorFromPowerBasis(3, P.PolynomialVector([P.Polynomial(P.Monomial, [1, 2, 3, 4])]), pb, S(2 ** 45).mul(S(x.Q[3])).v)
    vec = P.PolynomialVector([P.Polynomial(P.Monomial, [1, 2, 3, 4])], {0: [0, 2]})
    bare = P.PolynomialEvaluator(rh.ckks.Evaluator(x.rq, x.c.rp, rlk=x.ev[True].rlk))
    with pytest.raises(rh.RingHipError, match="need the CKKS encoder.*encoder=enc"):
        bare.Evaluate(ct, vec, 2 ** 45)
    wide = P.PolynomialEvaluator(rh.ckks.Evaluator(x.rq, x.c.rp, rlk=x.ev[True].rlk, encoder=x.enc, encoding_precision=64))
    with pytest.raises(rh.RingHipError, match="encoding_precision 64 > 53"):
        wide.Evaluate(ct, vec, 2 ** 45)
    ci = rh.Ring(x.N, QI60[:4], kind=rh.ConjugateInvariant)
    cpe = P.PolynomialEvaluator(rh.ckks.Evaluator(ci))
    with pytest.raises(rh.RingHipError, match="conjugate-invariant ring.*standard-only"):
        cpe.Evaluate(ct, vec, 2 ** 45)
    ci.close()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    with pytest.raises(rh.RingHipError, match="3N rings are not supported"):
        P.PolynomialEvaluator(rh.ckks.Evaluator(r3))
    r3.close()
    with pytest.raises(rh.RingHipError, match="levels < .* cannot evaluate poly"):
        pe.Evaluate(dev_ct(rh, x.c, [b[:, :3] for b in input_ct(5, 2)], 2 ** 45), P.Polynomial(P.Monomial, [1.0] * 32), 2 ** 45)

"""GPU: BGV polynomial evaluation on device (csrc/bgv.hip: rh_bgv_plain_combination; matrix-fhe-lattigo_amd/bgv_polynomial.py) bit for bit,
whole outputs, against tests/bgv_polynomial_restatement.py, which tests/test_bgv_polynomial_oracle.py pins to Python integers and to decryption
-- with the fused baby step and with the composed sequence of evaluator calls, in standard and in scale-invariant mode, under every cache
policy.  The circuit cases run under keys generated on the device from a KeyedPRNG; the oracle file checks for each of them that the
restatement decrypts exactly with 10 bits of noise margin, which is what makes the exact comparison of decrypted slots here meaningful."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import bgv_polynomial_restatement as bp
import rlwe_restatement as rr
from oracle import primes
from test_bgv_polynomial_oracle import FLAGS, GPU_CASES, POLYS, SETTINGS, VECTOR, chain, mapping
from test_gpu_cache_policy import policy

pytestmark = pytest.mark.gpu

T = 65537
CHUNK, WIDTH = 56, 4                                                     # LC_CHUNK / LC_WIDTH (lc_reduce.hip.hpp), asserted below
TERMS = (0, 1, 3, WIDTH, WIDTH + 1, CHUNK, CHUNK + 1)
# (logN, logQ, level, npoly): N = 32 with three polys gives a ragged grid tail; logN 13: more than one block per limb; levels 0 and top on a
# chain at the 2^61 bound and on a mixed-width one.  Below the top every second term is stored at the top level (a strided AtLevel view).
SHAPES = [(5, (61, 61), 0, 3), (5, (61, 61), 1, 3), (10, (55, 45, 45), 0, 2), (10, (55, 45, 45), 2, 2), (13, (61, 61), 1, 2)]


@functools.lru_cache(maxsize=None)
def kchain(logN, logQ):
    return [int(q) for q in primes.gen_moduli(logN + 1, list(logQ), [])[0]]


class Ctx:
    _cache = {}

    def __new__(cls, rh, logN, logQ):
        key = (logN, tuple(logQ))
        if key not in cls._cache:
            self = object.__new__(cls)
            self.Q, self.N = kchain(logN, tuple(logQ)), 1 << logN
            self.rq = rh.Ring(self.N, self.Q)
            cls._cache[key] = self
        return cls._cache[key]


def uniform(rng, mods, N):
    return np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in mods])


def to_kernel(pt, mods, t, mont=True):
    """a plaintext as Encode leaves it (the lift times T^-1) -> the entry's operand: the Montgomery form of the plain lift, pt T 2^64 mod q_i"""
    return np.stack([np.array((pt[i].astype(object) * ((t << (64 if mont else 0)) % q)) % q, dtype=np.uint64) for i, q in enumerate(mods)])


def from_kernel(m, mods, t):
    """the inverse: the Encode-form plaintext whose kernel operand is m"""
    return np.stack([np.array((m[i].astype(object) * pow((t << 64) % q, -1, q)) % q, dtype=np.uint64) for i, q in enumerate(mods)])


@functools.lru_cache(maxsize=None)
def pc_case(logN, logQ, level, npoly):
    """CHUNK + 1 terms of three components with a plaintext each; term k holds rows[k] limbs per poly.  Term 1 is a zero row, plaintext 2 is zero.
    prefix[K][j][p]: the reference sequence's accumulator after K terms, without the constant"""
    Q = kchain(logN, logQ)
    mods, N = Q[:level + 1], 1 << logN
    rng = np.random.default_rng(logN * 10 + level)
    rows = [len(Q) if k % 2 == 0 else level + 1 for k in range(CHUNK + 1)]
    X = [[np.stack([uniform(rng, Q[:r], N) for _ in range(npoly)]) for _ in range(3)] for r in rows]
    X[1] = [np.zeros_like(b) for b in X[1]]
    pts = [uniform(rng, mods, N) for _ in rows]
    pts[2] = np.zeros_like(pts[2])
    const = uniform(rng, mods, N)
    zero = np.zeros((len(mods), N), dtype=np.uint64)
    prefix = [[[zero] * npoly for _ in range(3)]]
    for k in range(CHUNK + 1):
        step = [bp.plain_combination(mods, T, [[X[k][j][p] for j in range(3)]], [pts[k]], None) for p in range(npoly)]
        prefix.append([[rr._vec("ADD", prefix[-1][j][p], step[p][j], mods) for p in range(npoly)] for j in range(3)])
    for blocks in X:
        for b in blocks:
            b.setflags(write=False)
    return Q, mods, rows, X, pts, const, prefix


def pc_call(rh, ring, level, terms, rows, m, c, cs, outs, table, npoly, table_words=None):
    """terms: K lists of device blocks, m: K device polys, c: a device poly or None; returns the status"""
    K = len(terms)
    x = (C.c_void_p * max(3 * K, 1))()
    r = (C.c_int * max(K, 1))(*rows[:K])
    mp = (C.c_void_p * max(K, 1))(*[p.ptr for p in m[:K]])
    for k, t in enumerate(terms):
        for j, p in enumerate(t):
            x[3 * k + j] = p.ptr
    ptrs = [o.ptr for o in outs] + [None] * (3 - len(outs))
    csp = np.ascontiguousarray(cs).ctypes.data_as(rh.ringhip.U64P) if cs is not None else None
    words = (table.words if table is not None else 0) if table_words is None else table_words
    return rh.lib().rh_bgv_plain_combination(ring._h, level, K, x, r, mp, c.ptr if c is not None else None, csp, *ptrs, npoly,
                                             table.ptr if table is not None else None, words)


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_plain_combination_kernel(rh, logN, logQ, level, npoly, nt):
    L = rh.lib()
    assert (L.rh_ckks_linear_combination_chunk(), L.rh_ckks_linear_combination_width()) == (CHUNK, WIDTH)
    c = Ctx(rh, logN, logQ)
    Q, mods, rows, X, pts, const, prefix = pc_case(logN, logQ, level, npoly)
    rl = c.rq.AtLevel(level)
    dev = [[rh.DevicePoly.from_numpy(c.rq.AtLevel(rows[k] - 1), b) for b in X[k]] for k in range(CHUNK + 1)]
    ms = [to_kernel(p, mods, T) for p in pts]
    dm = [rh.DevicePoly.from_numpy(rl, m[None]) for m in ms]
    cm = to_kernel(const, mods, T)
    dc = rh.DevicePoly.from_numpy(rl, cm[None])
    cs = np.array([pow(T, -1, q) for q in mods], dtype=np.uint64)
    table = rh.DevicePoly(rl, 1, -(-L.rh_bgv_plain_combination_table_words(CHUNK + 1) // c.N))
    with policy(nt, c.rq):
        for i, K in enumerate(TERMS):
            for nc in (1, 2, 3):
                with_const = K == 0 or (i + nc) % 2 == 0                  # no terms: a constant alone
                outs = [rl.NewPoly(npoly) for _ in range(nc)]
                rc = pc_call(rh, c.rq, level, [t[:nc] for t in dev[:K]], rows, dm, dc if with_const else None, cs if with_const else None, outs, table, npoly)
                assert rc == 0, L.rh_last_error()
                for j in range(nc):
                    want = np.stack(prefix[K][j])
                    if j == 0 and with_const:
                        want = np.stack([rr._vec("ADD", w, const, mods) for w in want])
                    assert np.array_equal(outs[j].numpy(), want), (K, nc, with_const, j)
        for k in (0, 1, WIDTH, CHUNK):                                   # inputs untouched
            for j in range(3):
                assert np.array_equal(dev[k][j].numpy(), X[k][j])
            assert np.array_equal(dm[k].numpy()[0], ms[k])
        assert np.array_equal(dc.numpy()[0], cm)


@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_plain_combination_sums_that_fill_the_chunk(rh, logN, logQ, level, npoly):
    """every word of every term and of every kernel plaintext q_i - 1, the constant q_i - 1: K = CHUNK is the largest sum the 128-bit
    accumulator is sized for, CHUNK + 1 starts a second chunk.  Expected with Python integers, and at N = 32 from the restatement as well."""
    c = Ctx(rh, logN, logQ)
    mods, N = c.Q[:level + 1], c.N
    rl = c.rq.AtLevel(level)
    row = np.stack([np.full(N, q - 1, dtype=np.uint64) for q in mods])
    full = np.stack([row] * npoly)
    block, m = rh.DevicePoly.from_numpy(rl, full), rh.DevicePoly.from_numpy(rl, row[None])
    one = np.ones(len(mods), dtype=np.uint64)                            # the constant's scalar 1: c 2^-64
    table = rh.DevicePoly(rl, 1, -(-rh.lib().rh_bgv_plain_combination_table_words(CHUNK + 1) // N))
    r64 = [pow(1 << 64, -1, q) for q in mods]
    for nt in (0, 2):
        with policy(nt, c.rq):
            for K in (CHUNK, CHUNK + 1):
                outs = [rl.NewPoly(npoly) for _ in range(3)]
                assert pc_call(rh, c.rq, level, [[block] * 3] * K, [level + 1] * K, [m] * K, m, one, outs, table, npoly) == 0
                for j, o in enumerate(outs):
                    want = np.stack([np.stack([np.full(N, (K * (q - 1) * (q - 1) + (q - 1 if j == 0 else 0)) * r % q, dtype=np.uint64)
                                               for q, r in zip(mods, r64)])] * npoly)
                    assert np.array_equal(o.numpy(), want), (K, j)
                if logN == 5:
                    pt = from_kernel(row, mods, T)
                    seq = bp.plain_combination(mods, T, [[row] * 3] * K, [pt] * K, None)
                    assert all(np.array_equal(outs[j].numpy()[0], rr._vec("ADD", seq[j], from_kernel(row, mods, 1) if j == 0 else np.zeros_like(row), mods)) for j in range(3))
    assert np.array_equal(block.numpy(), full)


def test_plain_combination_refusals(rh):
    logN, logQ, level, npoly = SHAPES[2]
    c = Ctx(rh, logN, logQ)
    L, rl = rh.lib(), c.rq.AtLevel(level)
    a = [rl.NewPoly(npoly) for _ in range(4)]
    m, cpoly = rl.NewPoly(1), rl.NewPoly(1)
    table = rh.DevicePoly(rl, 1, 1)
    one = np.ones(level + 1, dtype=np.uint64)
    call = lambda terms, ms, outs, tab, ring=c.rq, rows=(level + 1,), lv=level, cc=None, cs=None, words=None: \
        pc_call(rh, ring, lv, terms, list(rows), ms, cc, cs, outs, tab, npoly, words)
    assert call([[a[0]]], [m], [a[1]], table) == 0, L.rh_last_error()
    assert call([[a[0]]], [m], [a[0]], table) == -1 and b"overlaps a term or its plaintext" in L.rh_last_error()
    assert call([[a[0], a[1]]], [m], [a[2], a[1]], table) == -1 and b"overlaps a term or its plaintext" in L.rh_last_error()
    one_poly = rh.DevicePoly(rl, 1, level + 1, ptr=a[1].ptr, owner=a[1])                    # the first poly of an output, used as the plaintext
    assert call([[a[0]]], [one_poly], [a[1]], table) == -1 and b"overlaps a term or its plaintext" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], table, cc=one_poly, cs=one) == -1 and b"overlaps the constant" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1], a[1]], table) == -1 and b"two outputs overlap" in L.rh_last_error()
    as_table = rh.DevicePoly(rl, 1, 1, ptr=a[1].ptr, owner=a[1])
    assert call([[a[0]]], [m], [a[1]], as_table) == -1 and b"an output overlaps the table" in L.rh_last_error()
    term_table = rh.DevicePoly(rl, 1, 1, ptr=a[0].ptr, owner=a[0])
    assert call([[a[0]]], [m], [a[1]], term_table) == -1 and b"overlaps a term or its plaintext" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], None) == -1 and b"null table" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], table, words=4) == -1 and b"the table holds 4 words, 1 terms need 5" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], table, rows=(level,)) == -1 and b"fewer than level" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1], a[2]], table) == -1 and b"has no component 1" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], table, lv=len(c.Q)) == -1 and b"out of range" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], table, lv=-1) == -1 and b"out of range" in L.rh_last_error()
    assert call([[a[0]]], [m], [a[1]], table, cc=cpoly) == -1 and b"null argument" in L.rh_last_error()      # a constant without its scalar
    assert call([[a[0]]], [m], [a[1]], table, cc=cpoly, cs=np.array([c.Q[0]], dtype=np.uint64)) == -1 and b"not below its modulus" in L.rh_last_error()
    assert call([], [], [a[1]], None, cc=cpoly, cs=one) == 0, L.rh_last_error()                                # no terms: no table needed
    ci = rh.Ring(c.N, [int(q) for q in primes.gen_moduli(logN + 2, [55, 45], [])[0]], kind=rh.ConjugateInvariant)
    assert call([[a[0]]], [m], [a[1]], table, ring=ci) == -1 and b"needs a standard ring" in L.rh_last_error()
    ci.close()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    assert call([[a[0]]], [m], [a[1]], table, ring=r3, lv=0) == -1 and b"needs a standard ring" in L.rh_last_error()
    r3.close()


# ---- the circuit under keys generated on the device ------------------------------------------------------------------------------------------------------
class Dev:
    """rings, keys from a KeyedPRNG, the encoder and the four evaluators (standard / scale-invariant) of one setting; the relinearisation key
    as the restatement takes it"""
    _cache = {}

    def __new__(cls, rh, setting):
        if setting not in cls._cache:
            self = object.__new__(cls)
            logN, logQ, self.t = SETTINGS[setting]
            self.N = 1 << logN
            self.Q, self.Pk, self.QMul = chain(logN, tuple(logQ))
            self.rq, self.rp, self.rm = rh.Ring(self.N, self.Q), rh.Ring(self.N, self.Pk), rh.Ring(self.N, self.QMul)
            self.prng = rh.rlwe.KeyedPRNG(b"bgv polynomial " + setting.encode())
            kg = rh.rlwe.KeyGenerator(self.rq, self.rp, prng=self.prng)
            self.sk = kg.GenSecretKeyNew()
            self.rlk = kg.GenRelinearizationKeyNew(self.sk)
            self.enc = rh.bgv.Encoder(self.rq, self.t)
            self.ev = {inv: rh.bgv.Evaluator(self.rq, self.rm if inv else None, self.t, ringP=self.rp, rlk=self.rlk, scaleInvariant=inv, encoder=self.enc)
                       for inv in (False, True)}
            q = self.rlk.Q.numpy().reshape(self.rlk.digits, 2, self.rlk.Q.limbs, -1)
            p = self.rlk.P.numpy().reshape(self.rlk.digits, 2, self.rlk.P.limbs, -1)
            key = rr.GadgetKey(q, p, len(self.Q) - 1, len(self.Pk) - 1, 0, None)
            self.P = {inv: bp.Params(self.N, self.Q, self.Pk, self.t, key, inv, self.QMul) for inv in (False, True)}
            self.encryptor, self.decryptor = rh.bgv.Encryptor(self.rq, None, self.sk, prng=self.prng), rh.bgv.Decryptor(self.rq, self.sk)
            self.cts = {}
            cls._cache[setting] = self
        return cls._cache[setting]

    def encrypt(self, rh, npoly, level=None, scale=1):
        """-> (values (npoly, slots), the device ciphertext, its components on the host); one ciphertext per (npoly, level, scale), shared"""
        level = len(self.Q) - 1 if level is None else level
        key = (npoly, level, scale)
        if key not in self.cts:
            values = np.random.default_rng(self.N + npoly).integers(0, self.t, (npoly, self.enc.MaxSlots()), dtype=np.uint64)
            pt = self.enc.NewPlaintext(level, scale=scale, nvec=npoly)
            self.enc.Encode(values, pt)
            ct = self.encryptor.EncryptNew(pt)
            ct.Scale, ct.IsBatched = scale, True
            self.cts[key] = (values, ct, [v.numpy() for v in ct.Value])
        return self.cts[key]

    def decode(self, out):
        return np.asarray(self.enc.Decode(self.decryptor.DecryptNew(out)))


def polys_of(rh, name):
    """-> (the device polynomial or vector, the restatement's Polys, the mapping maker)"""
    bpm = rh.bgv_polynomial
    if name == "vector":
        return (lambda slots: bpm.PolynomialVector([bpm.Polynomial(c) for c in VECTOR], mapping(slots))), [bp.Poly(c) for c in VECTOR], mapping
    host = bp.Poly(POLYS[name])
    host.is_odd, host.is_even = FLAGS.get(name, (True, True))

    def make(slots):
        p = bpm.Polynomial(POLYS[name])
        p.IsOdd, p.IsEven = FLAGS.get(name, (True, True))
        return p
    return make, [host], None


def expected_slots(polys, mp, values, t):
    want = np.zeros_like(values)
    for p in range(values.shape[0]):
        if mp is None:
            want[p] = [bp.evaluate_exact(polys[0], v, t) for v in values[p]]
        else:
            for i, idx in mp.items():
                for j in idx:
                    want[p, j] = bp.evaluate_exact(polys[i], values[p, j], t)
    return want


def same_bits(out, wants):
    """every component of every ciphertext of the batch"""
    assert out.Degree() + 1 == len(wants[0].comps) and out.Level() == wants[0].level()
    for j, v in enumerate(out.Value):
        got = v.numpy()
        for p, w in enumerate(wants):
            assert np.array_equal(got[p], w.comps[j]), "component %d of ciphertext %d" % (j, p)


@pytest.mark.parametrize("invariant", [False, True], ids=["standard", "invariant"])
@pytest.mark.parametrize("setting,name", GPU_CASES, ids=lambda v: str(v))
def test_evaluate_fused_and_composed_match_the_restatement_and_decrypt(rh, setting, name, invariant):
    d = Dev(rh, setting)
    npoly = 3 if setting == "n7" else 1
    values, ct, host = d.encrypt(rh, npoly)
    make, polys, mp = polys_of(rh, name)
    slots = d.enc.MaxSlots()
    mp = mp(slots) if mp else None
    target = 1
    wants = [bp.evaluate(d.P[invariant], bp.Ct([h[p] for h in host], 1), polys, mp, target) for p in range(npoly)]
    degree = polys[0].degree()
    top = len(d.Q) - 1
    for fused in (True, False):
        out = rh.bgv_polynomial.Evaluator(d.ev[invariant], fused=fused).Evaluate(ct, make(slots), target)
        assert out.Scale == target == wants[0].scale
        assert out.Level() == (top if invariant else top - (degree.bit_length() - 1) - 1)     # unchanged under scale-invariant mode
        same_bits(out, wants)
        assert np.array_equal(d.decode(out), expected_slots(polys, mp, values, d.t)), "fused" if fused else "composed"
    for v, h in zip(ct.Value, host):                                     # the input untouched
        assert np.array_equal(v.numpy(), h)


@pytest.mark.parametrize("invariant", [False, True], ids=["standard", "invariant"])
@pytest.mark.parametrize("name", ["gap7", "vector"])
def test_from_power_basis_and_another_target_scale(rh, name, invariant):
    """EvaluateFromPowerBasis with a basis built beforehand (one power lazy), at a targetScale other than the ciphertext's"""
    d = Dev(rh, "n7")
    bpm = rh.bgv_polynomial
    values, ct, host = d.encrypt(rh, 3)
    make, polys, mp = polys_of(rh, name)
    slots = d.enc.MaxSlots()
    mp = mp(slots) if mp else None
    target = 77
    wants = []
    for p in range(3):
        pb = {1: bp.Ct([h[p] for h in host], 1)}
        for n in (2, 3):
            bp.gen_power(d.P[invariant], pb, n, False)
        wants.append(bp.evaluate(d.P[invariant], None, polys, mp, target, pb=pb))
    for fused in (True, False):
        pb = bpm.PowerBasis(ct)
        for n in (2, 3):
            pb.GenPower(n, False, d.ev[invariant])
        out = bpm.Evaluator(d.ev[invariant], fused=fused).EvaluateFromPowerBasis(pb, make(slots), target)
        assert out.Scale == target
        same_bits(out, wants)
        assert np.array_equal(d.decode(out), expected_slots(polys, mp, values, d.t))
    lazy = bpm.PowerBasis(ct)
    lazy.GenPower(3, True, d.ev[invariant])
    assert lazy.Value[3].Degree() == 2 and lazy.Value[2].Degree() == 1
    want = {1: bp.Ct([h[0] for h in host], 1)}
    bp.gen_power(d.P[invariant], want, 3, True)
    for j, v in enumerate(lazy.Value[3].Value):
        assert np.array_equal(v.numpy()[0], want[3].comps[j])
    assert lazy.Value[3].Scale == want[3].scale


@pytest.mark.parametrize("vector", [False, True], ids=["scalar", "vector"])
def test_baby_step_alone_every_policy(rh, vector):
    """EvaluatePolynomialVectorFromPowerBasis on a power basis whose powers sit above the target level, fused and composed, under every cache
    policy, each compared with the restatement"""
    d = Dev(rh, "n7")
    bpm = rh.bgv_polynomial
    values, ct, host = d.encrypt(rh, 3)
    ev, P = d.ev[False], d.P[False]
    slots = d.enc.MaxSlots()
    mp = mapping(slots) if vector else None
    co = VECTOR if vector else (POLYS["dense7"],)
    polys = [bp.Poly(c[:4]) for c in co]
    pol = bpm.PolynomialVector([bpm.Polynomial(c[:4]) for c in co], mp)
    pb = bpm.PowerBasis(ct)
    pb.GenPower(3, False, ev)
    level, target = pb.Value[3].Level() - 1, 91
    wants = []
    for p in range(3):
        w = {1: bp.Ct([h[p] for h in host], 1)}
        bp.gen_power(P, w, 3, False)
        wants.append(bp.evaluate_from_power_basis(P, level, polys, mp, w, target))
    for nt in (0, 1, 2):
        with policy(nt, d.rq):
            for fused in (True, False):
                out = bpm.Evaluator(ev, fused=fused).EvaluatePolynomialVectorFromPowerBasis(level, pol, pb, target)
                assert out.Scale == target
                same_bits(out, wants)


def test_the_modulus_bound_sends_the_python_side_to_the_composed_path(rh, monkeypatch):
    """The engine builds no ring with a modulus of 2^61 or more (rh_ring_create refuses it), so the entry's per-call check cannot be reached
    from a ring that exists.  What can be checked is the Python side's own test of the bound: with the bound lowered below the chain's q_0 the
    fused arm is not entered, nothing raises, and the bits are the restatement's."""
    d = Dev(rh, "n7")
    bpm = rh.bgv_polynomial
    with pytest.raises(rh.RingHipError):
        rh.Ring(32, [(1 << 61) + 2 * 32 * 7 + 1])
    values, ct, host = d.encrypt(rh, 3)
    slots = d.enc.MaxSlots()
    polys, mp = [bp.Poly(c) for c in VECTOR], mapping(slots)
    want = bp.evaluate(d.P[False], bp.Ct([h[0] for h in host], 1), polys, mp, 1)
    monkeypatch.setattr(bpm, "LC_MODULUS_BITS", 50)

    def never(*a, **k):
        raise AssertionError("the fused arm was entered")
    pe = bpm.Evaluator(d.ev[False], fused=True)
    pe._fused_vector = pe._fused_scalar = never
    out = pe.Evaluate(ct, bpm.PolynomialVector([bpm.Polynomial(c) for c in VECTOR], mp), 1)
    for j, v in enumerate(out.Value):
        assert np.array_equal(v.numpy()[0], want.comps[j])


def test_refusals_by_name(rh):
    d = Dev(rh, "n7")
    bpm = rh.bgv_polynomial
    values, ct, host = d.encrypt(rh, 3)
    pe = bpm.Evaluator(d.ev[False])
    with pytest.raises(rh.RingHipError, match="only `Monomial` is built"):
        bpm.PowerBasis(ct, rh.polynomial.Chebyshev)
    p = bpm.Polynomial(POLYS["dense7"])
    p.Basis = rh.polynomial.Chebyshev
    with pytest.raises(rh.RingHipError, match="only `Monomial` is built"):
        pe.Evaluate(ct, p, 1)
    lazy = bpm.Polynomial(POLYS["dense7"])
    lazy.Lazy = True
    with pytest.raises(rh.RingHipError, match="Lazy = true"):
        pe.Evaluate(ct, lazy, 1)
    bare = rh.bgv.Evaluator(d.rq, None, d.t, ringP=d.rp, rlk=d.rlk)
    with pytest.raises(rh.RingHipError, match="need the BGV encoder"):
        bpm.Evaluator(bare).Evaluate(ct, bpm.PolynomialVector([POLYS["dense7"]], {0: [0]}), 1)
    with pytest.raises(rh.RingHipError, match="invalid polynomial type"):
        pe.Evaluate(ct, [1, 2, 3], 1)
    empty = bpm.PowerBasis(ct)
    del empty.Value[1]
    with pytest.raises(rh.RingHipError, match=r"X\^\{1\} is nil"):
        pe.EvaluateFromPowerBasis(empty, bpm.Polynomial(POLYS["dense7"]), 1)
    _, low, _ = d.encrypt(rh, 1, level=2)
    with pytest.raises(rh.RingHipError, match=r"2 levels < 3 log\(d\) -> cannot evaluate poly"):
        pe.Evaluate(low, bpm.Polynomial(POLYS["dense7"]), 1)
    a, b = bpm.PowerBasis(ct).Value[1], bpm.PowerBasis(ct).Value[1]
    b.Scale = 5
    xpow = bpm.PowerBasis(ct)
    xpow.GenPower(2, False, d.ev[False])
    with pytest.raises(rh.RingHipError, match="evalMonomial: scale discrepency"):
        pe.EvaluateMonomial(a, b, xpow.Value[2])
    mixed = bpm.PowerBasis(ct)
    mixed.GenPower(3, True, d.ev[False])
    with pytest.raises(rh.RingHipError, match="mixed degrees"):
        pe.EvaluatePolynomialVectorFromPowerBasis(3, bpm.PolynomialVector([[1, 2, 3, 4]]), mixed, 1)
    for ring in (rh.Ring(d.N, [int(q) for q in primes.gen_moduli(9, [55, 45], [])[0]], kind=rh.ConjugateInvariant), rh.Ring(3 << 6, primes.gen_moduli_3n(3 << 6, [60, 60], [])[0], kind=rh.Matrix3N)):
        with pytest.raises(rh.RingHipError, match="conjugate-invariant and 3N rings are not supported"):
            bpm.Evaluator(types.SimpleNamespace(ringQ=ring, ScaleInvariant=False))
        ring.close()
    bare.close()

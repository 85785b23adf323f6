"""GPU: bgv.Encoder (csrc/bgv_encoder.hip, matrix-fhe-lattigo_amd/bgv.py) bit for bit, whole outputs, against the restatement of
schemes/bgv/encoder.go that tests/test_bgv_encoder_oracle.py pins; both settings of the "fused" tuning key and both cache policies; the
slice operands of bgv.Evaluator(encoder=) against the restated composition and against decryption under a real key.

Shapes (logN, Q chain, T -> n, gap), the smallest that reach each path; every T is accepted by the ring as it stands:
  n5    5,  61 61,     97              -> 16, 2     smallest ring, gap > 1: the exact-CRT branch and the strided level-0 branch
  n10   10, 55 45 45,  65537           -> 1024, 1   ModUpExact branch at levels 1 and 2, level 0
  n10w  10, 45 x 9,    55-bit T        -> 1024, 1   T above every q_i: unreduced lift, Embed without scale-up; nine limbs (the bounded <16> variant)
  n13   13, 61 61,     12289           -> 2048, 4   gap 4 across the 4096-coefficient tile boundary and the one-pass transform
  n5x4  5,  61 x 4,    97              -> 16, 2     the exact-CRT branch with three and four digits: the q_i mod q_j table, Garner constants past
                                                    the first, the multi-digit comparison with floor(Q / 2), Horner over the digits (<3>, <4>)
  n5x9  5,  61 x 9,    97              -> 16, 2     ... with five to nine digits: the register variants <5> .. <8> and the bounded <16>
  n5x17 5,  61 x 17,   97              -> 16, 2     ... at seventeen digits: the bounded <32> variant (Decode at the top level only)
  n10x17 10, 61 x 17,  65537           -> 1024, 1   the ModUpExact branch at seventeen limbs: the bounded <32> variant (top level only)
(the array form <0> starts at 33 limbs: ModUpExact stops at 32, as the reference's does; the exact-CRT branch is not run there)"""
import functools
import random

import numpy as np
import pytest

import bgv_encoder_restatement as er
import bgv_restatement as gr
from conftest import PI60, QI60
from oracle import primes
from oracle import ring_oracle as orc

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)


@functools.lru_cache(maxsize=None)
def shape(name):
    """(logN, Q, T)"""
    if name == "n5":
        return 5, tuple(QI60[:2]), 97
    if name.startswith("n5x"):
        return 5, tuple(QI60[:int(name[3:])]), 97
    if name == "n10x17":
        return 10, tuple(QI60[:17]), 65537
    if name == "n10":
        return 10, tuple(primes.gen_moduli(11, [55, 45, 45], [])[0]), 65537
    if name == "n10w":
        Q = tuple(primes.gen_moduli(11, [45] * 9, [])[0])
        return 10, Q, primes.NTTFriendlyPrimes(55, 1 << 11).upstream()          # a 55-bit prime = 1 mod 2^11, above every q_i
    return 13, tuple(QI60[:2]), 12289


SHAPES = ["n5", "n10", "n10w", "n13"]
PK = [PI60[0]]                                                                   # the key-switch ring of Embed into a (Q, P) pair


@functools.lru_cache(maxsize=None)
def params(name):
    logN, Q, t = shape(name)
    return er.Params(1 << logN, Q, t)


@functools.lru_cache(maxsize=None)
def params_p(name):
    return [orc.SubRingConsts(1 << shape(name)[0], q) for q in PK]


class Ctx:
    _cache = {}

    def __new__(cls, rh, name):
        if name not in cls._cache:
            self = object.__new__(cls)
            logN, Q, t = shape(name)
            self.N, self.Q, self.t, self.P = 1 << logN, list(Q), t, params(name)
            self.rq, self.rp = rh.Ring(self.N, self.Q), rh.Ring(self.N, PK)
            self.enc = rh.bgv.Encoder(self.rq, t, ringP=self.rp)
            cls._cache[name] = self
        return cls._cache[name]


@pytest.fixture(params=[(1, 0), (1, 2), (0, 0), (0, 2)], ids=["fused", "fused_nt", "composed", "composed_nt"])
def variant(request):
    return request.param


def tuned(c, variant):
    fused, nt = variant
    c.enc.set_tuning("fused", fused)
    for r in (c.rq, c.rp, c.enc.RingT()):
        r.set_tuning("nt_streams", nt)


def restore(c):
    c.enc.set_tuning("fused", -1)                                                  # the measured defaults
    for r in (c.rq, c.rp, c.enc.RingT()):
        r.set_tuning("nt_streams", 1)


@functools.lru_cache(maxsize=None)
def values(name, signed, nvals):
    """three vectors: the edge values first (0, T - 1, 2^64 - 1 as uint64; int64 min and max; T >> 1 on either side), the rest uniform"""
    P = params(name)
    rng = np.random.default_rng(len(name) + nvals + signed)
    h = P.t >> 1
    if signed:
        v = rng.integers(I64.min, I64.max, size=(3, nvals), dtype=np.int64, endpoint=True)
        edge = [I64.min, I64.max, 0, -1, h, h - 1, h + 1, -h, -h - 1, -P.t, P.t, -2 * P.t]
    else:
        v = rng.integers(0, (1 << 64) - 1, size=(3, nvals), dtype=np.uint64, endpoint=True)
        edge = [0, P.t - 1, (1 << 64) - 1, h, h - 1, h + 1, P.t, 2 * P.t]
    v[0, :len(edge)] = np.array(edge, dtype=v.dtype)
    v[2] = v[2] % np.array(P.t, dtype=v.dtype) if not signed else v[2] % np.int64(h)      # one vector of values already reduced
    v.setflags(write=False)
    return v


# ---- Encode -----------------------------------------------------------------------------------------------------------------------------------
ENC_FLAGS = [(True, True, False), (True, True, True), (True, False, False), (True, False, True), (False, True, False), (False, False, False)]   # (batched, IsNTT, IsMontgomery)


@functools.lru_cache(maxsize=None)
def expected_encode(name, signed, nvals, level, scale, batched, is_ntt, mont):
    P = params(name)
    return np.stack([er.encode(P, level, v, scale, is_ntt=is_ntt, batched=batched, mont=mont) for v in values(name, signed, nvals)])


@pytest.mark.parametrize("name", SHAPES)
@pytest.mark.parametrize("signed", [False, True])
def test_encode(rh, name, signed, variant):
    """Encode of three vectors at once at the top level and at level 0: batched with every (IsNTT, IsMontgomery), IsBatched = false in both
    domains; all slots given, and fewer values than slots (the rest is zero)"""
    c = Ctx(rh, name)
    tuned(c, variant)
    try:
        for level in sorted({0, len(c.Q) - 1}):
            for nvals in (c.P.n, c.P.n - 3):
                v = values(name, signed, nvals)
                for batched, is_ntt, mont in ENC_FLAGS if nvals == c.P.n else ENC_FLAGS[:1]:
                    pt = c.enc.NewPlaintext(level, 3, nvec=3, is_ntt=is_ntt, is_batched=batched)
                    pt.IsMontgomery = mont
                    c.enc.Encode(v, pt)
                    assert np.array_equal(pt.Value[0].numpy(), expected_encode(name, signed, nvals, level, 3, batched, is_ntt, mont)), (level, nvals, batched, is_ntt, mont)
        one = c.enc.NewPlaintext(len(c.Q) - 1, 3, nvec=3)                         # one row (a list for int64) is shared by the batch
        row = values(name, signed, c.P.n)[2]
        c.enc.Encode([int(x) for x in row] if signed else row, one)
        want = expected_encode(name, signed, c.P.n, len(c.Q) - 1, 3, True, True, False)[2]
        assert all(np.array_equal(g, want) for g in one.Value[0].numpy())
    finally:
        restore(c)


@functools.lru_cache(maxsize=None)
def expected_embed(name, level, is_ntt, mont, into_p):
    P = params(name)
    kw = dict(mods=PK, srs=params_p(name)) if into_p else {}
    return np.stack([er.embed(P, 0 if into_p else level, v, 5, False, is_ntt, mont, **kw) for v in values(name, False, P.n)])


@pytest.mark.parametrize("name", SHAPES)
def test_embed(rh, name, variant):
    """Embed (scaleUp = false) into a poly of ringQ and into a (Q, P) pair: raw residues modulo T in the coefficient domain without MForm --
    unreduced where T exceeds q_i -- and the reference's canonical words after its transform or MForm"""
    c = Ctx(rh, name)
    tuned(c, variant)
    try:
        level = len(c.Q) - 1
        v = values(name, False, c.P.n)
        for is_ntt, mont in ((False, False), (True, False), (False, True), (True, True)):
            md = c.enc.NewPlaintext(level, 5, nvec=3, is_ntt=is_ntt)
            md.IsMontgomery = mont
            q = c.rq.AtLevel(level).NewPoly(3)
            c.enc.Embed(v, md, q)
            assert np.array_equal(q.numpy(), expected_embed(name, level, is_ntt, mont, False)), ("Q", is_ntt, mont)
            q2, p2 = c.rq.AtLevel(level).NewPoly(3), c.rp.NewPoly(3)
            c.enc.Embed(v, md, (q2, p2))
            assert np.array_equal(q2.numpy(), expected_embed(name, level, is_ntt, mont, False)), ("QP.Q", is_ntt, mont)
            assert np.array_equal(p2.numpy(), expected_embed(name, level, is_ntt, mont, True)), ("QP.P", is_ntt, mont)
        if name == "n10w":
            raw = expected_embed(name, level, False, False, False)
            assert int(raw.max()) > max(c.Q)                                       # the case is what it says: words above every q_i
    finally:
        restore(c)


# ---- Decode -----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def polys(name, level):
    """three polys at `level`: uniform residues; a noisy encoding (T x = m + T e); all q_i - 1"""
    P = params(name)
    mods = P.Q[:level + 1]
    rng = np.random.default_rng(level + len(name))
    rnd = random.Random(level)
    uni = np.stack([rng.integers(0, q, P.N, dtype=np.uint64) for q in mods])
    Qb = er.prod(mods)
    tinv = pow(P.t, -1, Qb)
    x = [(rnd.randrange(P.t) * tinv + rnd.randrange(-5, 6)) % Qb for _ in range(P.N)]
    noisy = np.stack([np.array([v % q for v in x], dtype=np.uint64) for q in mods])
    top = np.stack([np.full(P.N, q - 1, dtype=np.uint64) for q in mods])
    a = np.stack([uni, noisy, top])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected_decode(name, level, scale, is_ntt, batched, signed):
    P = params(name)
    return np.stack([er.decode(P, level, p, scale, is_ntt=is_ntt, batched=batched, signed=signed) for p in polys(name, level)])


@functools.lru_cache(maxsize=None)
def expected_q2t(name, level):
    return np.stack([er.ring_q2t(params(name), level, p)[None] for p in polys(name, level)])


def decode_levels(name):
    L = len(shape(name)[1])
    return [L - 1] if L > 9 else list(range(L))


@pytest.mark.parametrize("name", SHAPES + ["n5x4", "n5x9", "n5x17", "n10x17"])
def test_decode(rh, name, variant):
    """Decode at every level -- level 0 with and without a gap, ModUpExact (n10, n10w, n10x17) and the exact CRT (n5, n13, n5x4, n5x9, n5x17)
    above it, with two to nine digits, and seventeen -- of arbitrary polys (uniform, a noisy encoding, all q_i - 1), both domains, batched and
    not, []uint64 and []int64; RingQ2T alone keeps the reference's representative"""
    c = Ctx(rh, name)
    tuned(c, variant)
    try:
        for level in decode_levels(name):
            blk = polys(name, level)
            src = rh.DevicePoly.from_numpy(c.rq.AtLevel(level), blk)
            for scale, is_ntt, batched, signed in ((1, False, True, False), (5, True, True, True), (5, False, False, True), (7, True, False, False)):
                pt = rh.bgv.Plaintext(src, scale, is_ntt=is_ntt, is_batched=batched)
                got = c.enc.Decode(pt, signed=signed)
                want = expected_decode(name, level, scale, is_ntt, batched, signed)
                assert got.dtype == want.dtype and np.array_equal(got, want), (level, scale, is_ntt, batched, signed)
            assert np.array_equal(src.numpy(), blk)                                # the plaintext is not modified
            pT = c.enc.RingT().NewPoly(3)
            c.enc.RingQ2T(level, True, src, pT)
            assert np.array_equal(pT.numpy(), expected_q2t(name, level)), level
    finally:
        restore(c)


@pytest.mark.parametrize("name", SHAPES)
def test_ring_t_entries(rh, name, variant):
    """EncodeRingT, DecodeRingT and RingT2Q on blocks modulo T"""
    c = Ctx(rh, name)
    tuned(c, variant)
    try:
        P = c.P
        for signed in (False, True):
            v = values(name, signed, P.n - 1)
            pT = c.enc.RingT().NewPoly(3)
            c.enc.EncodeRingT(v, 9, pT)
            want = np.stack([er.encode_ring_t(P, x, 9)[None] for x in v])
            assert np.array_equal(pT.numpy(), want)
            got = c.enc.DecodeRingT(pT, 9, signed=signed)
            assert np.array_equal(got, np.stack([er.decode_ring_t(P, w[0], 9, signed) for w in want]))
            out = np.zeros((3, 5), dtype=v.dtype)                                  # the first five values only
            assert np.array_equal(c.enc.DecodeRingT(pT, 9, out), got[:, :5])
            wide = np.zeros((3, 10), dtype=v.dtype)                                # a strided output is written through, not through a copy
            c.enc.DecodeRingT(pT, 9, wide[:, ::2])
            assert np.array_equal(wide[:, ::2], got[:, :5]) and not wide[:, 1::2].any()
            for scale_up in (True, False):
                level = len(c.Q) - 1
                pQ = c.rq.AtLevel(level).NewPoly(3)
                c.enc.RingT2Q(level, scale_up, pT, pQ)
                assert np.array_equal(pQ.numpy(), np.stack([er.ring_t2q(P, P.Q, w[0], scale_up) for w in want])), scale_up
    finally:
        restore(c)


@pytest.mark.parametrize("name", ["n5", "n10", "n13"])
def test_round_trip_on_device(rh, name, variant):
    """Decode(Encode(v)) = v from device-resident values to device-resident values, at every level"""
    c = Ctx(rh, name)
    tuned(c, variant)
    try:
        v = values(name, False, c.P.n)[2:]
        dv = rh.bgv.DeviceValues.from_numpy(c.rq, v)
        out = rh.bgv.DeviceValues(c.rq, 1, c.P.n)
        for level in range(len(c.Q)):
            pt = c.enc.NewPlaintext(level, 11)
            c.enc.Encode(dv, pt)
            assert c.enc.Decode(pt, out) is out and np.array_equal(out.numpy(), v), level
    finally:
        restore(c)


@pytest.mark.parametrize("name", SHAPES)
def test_default_tuning_gives_the_same_bits(rh, name):
    """the state at create ("fused" = -1: each kernel's measured default) against the restatement, and the tuning keys' refusals"""
    c = Ctx(rh, name)
    level = len(c.Q) - 1
    pt = c.enc.NewPlaintext(level, 3, nvec=3)
    c.enc.Encode(values(name, False, c.P.n), pt)
    assert np.array_equal(pt.Value[0].numpy(), expected_encode(name, False, c.P.n, level, 3, True, True, False))
    src = rh.DevicePoly.from_numpy(c.rq.AtLevel(level), polys(name, level))
    assert np.array_equal(c.enc.Decode(rh.bgv.Plaintext(src, 5), signed=True), expected_decode(name, level, 5, True, True, True))
    for key, value in (("fused", 2), ("fused_q2t", -2), ("nope", 1)):
        with pytest.raises(rh.RingHipError):
            c.enc.set_tuning(key, value)


# ---- queries and refusals -----------------------------------------------------------------------------------------------------------------------
def test_queries(rh):
    c = Ctx(rh, "n5")
    assert c.enc.MaxSlots() == 16 and c.enc.LogMaxDimensions() == (1, 3) and c.enc.RingT().N == 16
    assert [int(x) for x in c.enc.indexMatrix] == er.permute_matrix(4)
    assert Ctx(rh, "n13").enc.RingT().N == 2048 and Ctx(rh, "n10").enc.MaxSlots() == 1024


def test_refusals(rh):
    c = Ctx(rh, "n5")
    E = rh.RingHipError
    pt = c.enc.NewPlaintext(1)
    with pytest.raises(E, match=r"cannot EncodeRingT \(FrequencyDomain\): len\(values\)=17 > slots=16"):
        c.enc.Encode(np.zeros(17, dtype=np.uint64), pt)
    with pytest.raises(E, match=r"cannot Encode \(TimeDomain\): len\(values\)=17 > N=16"):
        c.enc.Encode(np.zeros(17, dtype=np.int64), c.enc.NewPlaintext(1, is_batched=False))
    for bad in (np.zeros(4, dtype=np.float64), np.zeros(4, dtype=np.int32), [1.5, 2.0], np.zeros(4, dtype=np.complex128)):
        with pytest.raises(E, match=r"values.\(type\) must be either \[\]uint64 or \[\]int64"):
            c.enc.Encode(bad, pt)
    with pytest.raises(E, match="must be either"):
        c.enc.Decode(pt, np.zeros(16, dtype=np.float64))
    for scale in (0, 97, 194):
        with pytest.raises(E, match="zero or not invertible modulo T"):
            c.enc.Decode(rh.bgv.Plaintext(pt.Value[0], scale))
    with pytest.raises(E, match="zero or not invertible modulo T"):
        c.enc.DecodeRingT(c.enc.RingT().NewPoly(1), 0)
    with pytest.raises(E, match="scaleUp into a ringqp.Poly is refused"):
        c.enc.EmbedScale(np.zeros(4, dtype=np.uint64), True, pt, (c.rq.NewPoly(1), c.rp.NewPoly(1)))
    with pytest.raises(E, match="scale_up into a ring other than ringQ is refused"):           # the C entry point says it too
        c.enc.RingT2Q(0, True, c.enc.RingT().NewPoly(1), c.rp.NewPoly(1))
    ci = rh.Ring(32, [QI60[0]], kind=rh.ConjugateInvariant)
    with pytest.raises(E, match="conjugate-invariant rings are not supported"):
        rh.bgv.Encoder(ci, 97)
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    with pytest.raises(E, match="3N rings are not supported"):
        rh.bgv.Encoder(r3, 97)
    with pytest.raises(E, match="cyclotomic order < 16"):
        rh.bgv.Encoder(c.rq, 7)
    with pytest.raises(E, match=r"t\|Q"):
        rh.bgv.Encoder(c.rq, c.Q[0])
    with pytest.raises(E, match="plaintext modulus t is invalid"):
        rh.bgv.Encoder(c.rq, 33)                                                   # = 1 mod 32 but not a prime: the ring refuses it
    import ctypes as C
    big = rh.Ring(64, [QI60[2]])                                                   # a "ringT" of degree 64 > N = 32
    h = C.c_void_p()
    assert rh.lib().rh_bgv_encoder_create(C.byref(h), c.rq._h, big._h) != 0
    assert b"must divide the degree of ringQ" in rh.lib().rh_last_error()
    for r in (ci, r3, big):
        r.close()


# ---- slice operands of the evaluator -----------------------------------------------------------------------------------------------------------
class Ev:
    """a secret, two ciphertexts of scales 3 and 5 and an evaluator with an encoder per shape, shared by the tests of a run"""
    _cache = {}

    def __new__(cls, rh, name):
        if name not in cls._cache:
            self = object.__new__(cls)
            c = Ctx(rh, name)
            self.c, P = c, c.P
            rnd = random.Random(len(name))
            self.s = [0] * P.N                                                      # a sparse ternary secret keeps the big-integer decryption quick
            for j in rnd.sample(range(P.N), min(P.N, 24)):
                self.s[j] = rnd.choice((-1, 1))
            self.a = np.array([rnd.randrange(P.t) for _ in range(P.n)], dtype=np.uint64)
            self.z = np.array([rnd.randrange(P.t) for _ in range(P.n)], dtype=np.uint64)
            spread = lambda v: [int(x) for x in er.ring_t2q(P, [P.Q[0]], er.encode_ring_t(P, v, 1), False)[0]]
            self.ct = gr.encrypt(rnd, P.N, P.Q, P.t, spread(self.a), self.s, 3)
            self.acc = gr.encrypt(rnd, P.N, P.Q, P.t, spread(self.z), self.s, 5)
            self.ev = rh.bgv.Evaluator(c.rq, None, P.t, encoder=c.enc)
            self.composed = rh.bgv.Evaluator(c.rq, None, P.t, fused=False, encoder=c.enc)
            cls._cache[name] = self
        return cls._cache[name]

    def up(self, rh, blocks, scale):
        out = rh.Ciphertext([rh.DevicePoly.from_numpy(self.c.rq, b[None]) for b in blocks], is_ntt=True)
        out.Scale = scale
        return out

    def slots(self, ct_dev):
        """decrypt under the real key, then decode the message times the scale: the slot values"""
        P = self.c.P
        m = gr.decrypt(P.N, P.Q, P.t, [v.numpy()[0] for v in ct_dev.Value], self.s)
        return er.decode_ring_t(P, np.array(m[::P.gap], dtype=np.uint64), ct_dev.Scale)


def same(out, want, scale):
    assert out.Degree() + 1 == len(want) and out.Scale == scale and out.IsNTT
    for v, w in zip(out.Value, want):
        assert np.array_equal(v.numpy()[0], w)


@pytest.mark.parametrize("name", ["n5", "n10"])
@pytest.mark.parametrize("signed", [False, True])
def test_evaluator_slices(rh, name, signed):
    """Add, Sub, Mul, MulRelin, MulThenAdd (scales equal and unequal) and MulRelinThenAdd with []uint64 / []int64 operands: each output is
    the restated composition bit for bit, and decrypts and decodes to the slot-wise result modulo T"""
    e = Ev(rh, name)
    P, t, mods = e.c.P, e.c.P.t, e.c.P.Q
    level = len(mods) - 1
    rng = np.random.default_rng(7 + signed)
    b = rng.integers(-(t >> 1), t >> 1, P.n, dtype=np.int64) if signed else rng.integers(0, t, P.n, dtype=np.uint64)
    bm = np.array([int(x) % t for x in b], dtype=np.uint64)
    a, z = e.a, e.z
    T_ = np.uint64(t)
    for ev in (e.ev, e.composed):
        ct = e.up(rh, e.ct, 3)
        for sub in (False, True):                                                   # the plaintext takes op0's scale (:254)
            out = ev.SubNew(ct, b) if sub else ev.AddNew(ct, b)
            want, sc = gr.add_sub(mods, t, e.ct, 3, [er.encode(P, level, b, 3)], 3, sub)
            same(out, want, sc)
            assert np.array_equal(e.slots(out), (a + (T_ - bm if sub else bm)) % T_)
        for f in (ev.MulNew, ev.MulRelinNew, ev.MulScaleInvariantNew, ev.MulRelinScaleInvariantNew):   # plaintext scale 1, tensorStandard (:529, :813, :820, :927)
            out = f(ct, b)
            want, sc = gr.tensor_standard(mods, t, e.ct, 3, [er.encode(P, level, b, 1)], 1)
            same(out, want, sc)
            assert np.array_equal(e.slots(out), a * bm % T_)
        for sacc, f in ((3, ev.MulThenAdd), (5, ev.MulThenAdd), (5, ev.MulRelinThenAdd)):   # accumulator at op0's scale, and not (:1224-1230)
            acc = e.up(rh, e.acc, sacc)                                             # (at scale 3 the accumulator holds z * 5 / 3)
            spt = pow(3, t - 2, t) * sacc % t if sacc != 3 else 1
            f(ct, b, acc)
            want, sc, _ = gr.mul_relin_then_add(mods, t, e.ct, 3, [er.encode(P, level, b, spt)], spt, e.acc, sacc, False)
            same(acc, want, sc)
            zz = z * np.uint64(5 * pow(sacc, t - 2, t) % t) % T_
            assert np.array_equal(e.slots(acc), (zz + a * bm) % T_)


def test_evaluator_without_encoder_still_refuses(rh):
    c = Ctx(rh, "n5")
    ev = rh.bgv.Evaluator(c.rq, None, c.t)
    ct = Ev(rh, "n5").up(rh, Ev(rh, "n5").ct, 3)
    with pytest.raises(rh.RingHipError, match="needs the BGV encoder, which the device path does not build"):
        ev.AddNew(ct, np.zeros(4, dtype=np.uint64))
    with pytest.raises(rh.RingHipError, match="the encoder was built for another ringQ or plaintext modulus"):
        rh.bgv.Evaluator(c.rq, None, 193, encoder=c.enc)

"""GPU: ckks.Evaluator (csrc/ckks.hip, matrix-fhe-lattigo_amd/ckks.py) bit for bit, whole outputs, against the restatement of
schemes/ckks/evaluator.go that tests/test_ckks_oracle.py pins to big-integer ground truth -- with the fused kernels and with the composed
sequence of ring calls, under every cache policy; inputs untouched where they are not the output."""
import functools
from fractions import Fraction

import numpy as np
import pytest

import ckks_restatement as cr
from bfv_restatement import _vec, _zeros
from oracle import compose, primes
from oracle import ring_oracle as orc
from test_gpu_cache_policy import policy

pytestmark = pytest.mark.gpu

KINDS = ("uniform", "sum_past_q", "q_minus_1", "zero")
NAMES = ("a0", "a1", "a2", "b0", "b1", "b2", "z0", "z1", "z2", "pt")
# (logN, logQ, level, npoly): N = 32 has N/2 = 16 inside one wavefront, and three polys give a ragged grid tail; a mixed-width chain; logN 13: more
# than one block per limb
SHAPES = [(5, (61, 61), 0, 3), (5, (61, 61), 1, 4), (10, (55, 45, 45), 2, 4), (13, (61, 61), 1, 2)]
TOP = [s for s in SHAPES if s[2] == len(s[1]) - 1]                   # the keys are used at the level they were made for
SCALARS = [3, -2, 0.5, 1.25 - 0.75j, 0]
S = cr.Scale
SA, SB = 2 ** 40, 3 * 2 ** 41 + 5                                      # SB / SA = 6.00..: ratioInt 6, not a power of two


@functools.lru_cache(maxsize=None)
def chain(logN, logQ):
    Q, Pk = primes.gen_moduli(logN + 1, list(logQ), [61, 61])
    return [int(q) for q in Q], [int(p) for p in Pk]


def uniform(rng, mods, N):
    return np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in mods])


@functools.lru_cache(maxsize=None)
def operands(logN, logQ, level, npoly):
    """ten blocks (npoly, level+1, N).  Poly k follows KINDS[k]: uniform; built so that a0 b1 + a1 b0 and the accumulate sums pass q
    (1 (q-1) + 1 (q-1) onto an accumulator of q-1); all q_i - 1; all zero."""
    mods = chain(logN, logQ)[0][:level + 1]
    N = 1 << logN
    rng = np.random.default_rng(logN * 100 + level * 10 + npoly)
    out = {}
    for name in NAMES:
        polys = []
        for kind in KINDS[:npoly]:
            if kind == "uniform":
                polys.append(uniform(rng, mods, N))
            elif kind == "zero":
                polys.append(np.zeros((len(mods), N), dtype=np.uint64))
            elif kind == "sum_past_q" and name in ("a0", "a1"):
                polys.append(np.ones((len(mods), N), dtype=np.uint64))
            else:
                polys.append(np.stack([np.full(N, q - 1, dtype=np.uint64) for q in mods]))
        a = np.stack(polys)
        a.setflags(write=False)
        out[name] = a
    return out


class Ctx:
    """ring, key-switch ring, random relinearisation and Galois keys and the two evaluators of one chain, shared by the tests of a module run"""
    _cache = {}
    ROT = (1, 2, -1)

    def __new__(cls, rh, logN, logQ):
        key = (logN, tuple(logQ))
        if key not in cls._cache:
            self = object.__new__(cls)
            self.Q, self.Pk = chain(logN, tuple(logQ))
            self.N = 1 << logN
            self.rq, self.rp = rh.Ring(self.N, self.Q), rh.Ring(self.N, self.Pk)
            rng = np.random.default_rng(logN + len(logQ))
            beta = (len(self.Q) + len(self.Pk) - 1) // len(self.Pk)

            def key_arrays():
                return (np.stack([np.stack([uniform(rng, self.Q, self.N) for _ in range(2)]) for _ in range(beta)]),
                        np.stack([np.stack([uniform(rng, self.Pk, self.N) for _ in range(2)]) for _ in range(beta)]))
            self.rlk = key_arrays()
            self.gal = {g: key_arrays() for g in [cr.galois_element(self.N, k) for k in self.ROT] + [2 * self.N - 1]}
            mk = lambda kq_kp: rh.rlwe.GadgetCiphertext(self.rq, self.rp, *kq_kp)
            keys = dict(rlk=mk(self.rlk), galois_keys={g: mk(v) for g, v in self.gal.items()})
            self.ev = {True: rh.ckks.Evaluator(self.rq, self.rp, fused=True, **keys), False: rh.ckks.Evaluator(self.rq, self.rp, fused=False, **keys)}
            cls._cache[key] = self
        return cls._cache[key]


def ct(rh, c, level, blocks, scale):
    rl = c.rq.AtLevel(level)
    out = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, b) for b in blocks], is_ntt=True)
    if scale is not None:
        out.Scale = rh.ckks.Scale(scale)
    return out


def per_poly(fn, npoly):
    """fn(k) -> list of (limbs, N) arrays; stacked per component into (npoly, limbs, N) blocks"""
    res = [fn(k) for k in range(npoly)]
    return [np.stack([r[j] for r in res]) for j in range(len(res[0]))]


def check(out, want, scale=None):
    assert out.Degree() + 1 == len(want)
    for j, w in enumerate(want):
        assert np.array_equal(out.Value[j].numpy(), w), "component %d" % j
    assert out.IsNTT
    if scale is not None:
        assert out.Scale.Value == Fraction(getattr(scale, "v", scale))


def untouched(cts, blocks):
    for c_, b in zip(cts, blocks):
        for v, h in zip(c_.Value, b):
            assert np.array_equal(v.numpy(), h)


def sel(o, names, k=None):
    return [o[n] if k is None else o[n][k] for n in names]


def key_switch(c, level, cx, key):
    """rlwe.Evaluator.GadgetProduct of one poly (levelP = 1): the oracle composition"""
    return compose.gadget_product(c.N, c.Q, c.Pk, level, len(c.Pk) - 1, cx, key[0], key[1])


# ---- the four kernels through the C ABI: every mode, 1 to 3 components, every cache policy ---------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_kernels(logN, logQ, level, npoly):
    mods = chain(logN, logQ)[0][:level + 1]
    N = 1 << logN
    o = operands(logN, logQ, level, npoly)
    one, six = S(1), S(6)
    _, _, s0, s1 = cr.rns_scalar(N, mods, S(mods[-1]), cr.to_complex(1.25 - 0.75j, 53), 53)
    want = {"s": (s0, s1)}
    A, B, Z = ("a0", "a1"), ("b0", "b1"), ("z0", "z1", "z2")
    want["regular"] = per_poly(lambda k: cr.mul_relin(mods, sel(o, A, k), one, sel(o, B, k), one)[0], npoly)
    want["square"] = per_poly(lambda k: cr.mul_relin(mods, sel(o, A, k), one, sel(o, A, k), one, True)[0], npoly)
    want["acc1"] = per_poly(lambda k: cr.mul_relin_then_add(N, mods, sel(o, A, k), one, sel(o, B, k), one, sel(o, Z, k), one, False)[0], npoly)

    def acc2(k):
        out, _, c2 = cr.mul_relin_then_add(N, mods, sel(o, A, k), one, sel(o, B, k), one, sel(o, Z[:2], k), one, True)
        return out + [c2]
    want["acc2"] = per_poly(acc2, npoly)
    cts = ("a0", "a1", "a2")
    for nc in (1, 2, 3):
        want["plain", nc, 0] = per_poly(lambda k: cr.mul_relin(mods, sel(o, cts[:nc], k), one, [o["pt"][k]], one)[0], npoly)
        want["plain", nc, 1] = per_poly(lambda k: cr.mul_relin_then_add(N, mods, sel(o, cts[:nc], k), one, [o["pt"][k]], one, sel(o, Z[:nc], k), one, False)[0], npoly)
        want["scalar", nc, 0] = per_poly(lambda k: [cr.add_double(x, s0, s1, mods) for x in sel(o, cts[:nc], k)], npoly)
        want["scalar", nc, 1] = per_poly(lambda k: [cr.sub_double(x, s0, s1, mods) for x in sel(o, cts[:nc], k)], npoly)
        want["scalar", nc, 2] = per_poly(lambda k: [cr.mul_double(x, s0, s1, mods) for x in sel(o, cts[:nc], k)], npoly)
        want["scalar", nc, 3] = per_poly(lambda k: [cr.mul_double_then_add(x, s0, s1, z, mods) for x, z in zip(sel(o, cts[:nc], k), sel(o, Z[:nc], k))], npoly)
    bs = ("b0", "b1", "b2")
    for da, db, sub, scaled_b in [(2, 2, 0, 1), (2, 3, 1, 0), (3, 1, 1, 1), (1, 3, 0, 1), (3, 3, 1, None)]:
        sa, sb = (six, one) if scaled_b == 1 else (one, six) if scaled_b == 0 else (one, one)
        want["sta", da, db, sub, scaled_b] = per_poly(lambda k: cr.add_sub(N, mods, sel(o, cts[:da], k), sa, sel(o, bs[:db], k), sb, bool(sub))[0], npoly)
    return want


@pytest.mark.parametrize("nt", [0, 1, 2])
@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_kernels_every_mode_and_cache_policy(rh, logN, logQ, level, npoly, nt):
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    w = expected_kernels(logN, logQ, level, npoly)
    rl, L, h = c.rq.AtLevel(level), rh.lib(), c.rq._h
    up = lambda names: [rh.DevicePoly.from_numpy(rl, o[n]) for n in names]
    ptrs = lambda ps, n=3: [p.ptr for p in ps] + [None] * (n - len(ps))
    same = lambda polys, want: all(np.array_equal(p.numpy(), x) for p, x in zip(polys, want)) and len(polys) == len(want)
    s0, s1 = [np.array(s, dtype=np.uint64) for s in w["s"]]
    U = rh.ringhip.U64P
    with policy(nt, c.rq):
        a, b = up(("a0", "a1")), up(("b0", "b1"))
        out = [rl.NewPoly(npoly) for _ in range(3)]
        assert L.rh_ckks_tensor(h, level, *ptrs(a, 2), *ptrs(b, 2), *ptrs(out), npoly, 0, 0) == 0 and same(out, w["regular"])
        ref = [rl.NewPoly(npoly) for _ in range(3)]
        rl.TensorDegree1(*a, *b, *ref)                                   # the bits of rh_ring_tensor_degree1
        assert same(out, [p.numpy() for p in ref])
        assert L.rh_ckks_tensor(h, level, *ptrs(a, 2), None, None, *ptrs(out), npoly, 0, 1) == 0 and same(out, w["square"])
        assert L.rh_ckks_tensor(h, level, *ptrs(a, 2), *ptrs(a, 2), *ptrs(out), npoly, 0, 1) == 0 and same(out, w["square"])
        z = up(("z0", "z1", "z2"))
        assert L.rh_ckks_tensor(h, level, *ptrs(a, 2), *ptrs(b, 2), *ptrs(z), npoly, 1, 0) == 0 and same(z, w["acc1"])
        z = up(("z0", "z1", "z2"))
        assert L.rh_ckks_tensor(h, level, *ptrs(a, 2), *ptrs(b, 2), *ptrs(z), npoly, 2, 0) == 0 and same(z, w["acc2"])
        aa = up(("a0", "a1"))                                            # the outputs ARE the first operand, c2 the second's first poly
        bb = up(("b0", "b1"))
        assert L.rh_ckks_tensor(h, level, *ptrs(aa, 2), *ptrs(bb, 2), aa[0].ptr, aa[1].ptr, bb[0].ptr, npoly, 0, 0) == 0
        assert same([aa[0], aa[1], bb[0]], w["regular"])
        untouched([rh.Ciphertext(a), rh.Ciphertext(b)], [sel(o, ("a0", "a1")), sel(o, ("b0", "b1"))])
        pt = up(("pt",))[0]
        for nc in (1, 2, 3):
            x = up(("a0", "a1", "a2")[:nc])
            out = [rl.NewPoly(npoly) for _ in range(nc)]
            assert L.rh_ckks_mul_plain(h, level, *ptrs(x), pt.ptr, *ptrs(out), npoly, 0) == 0 and same(out, w["plain", nc, 0])
            z = up(("z0", "z1", "z2")[:nc])
            assert L.rh_ckks_mul_plain(h, level, *ptrs(x), pt.ptr, *ptrs(z), npoly, 1) == 0 and same(z, w["plain", nc, 1])
            for op in (0, 1, 2):
                assert L.rh_ckks_scalar(h, level, op, *ptrs(x), *ptrs(out), npoly, s0.ctypes.data_as(U), s1.ctypes.data_as(U)) == 0
                assert same(out, w["scalar", nc, op]), (nc, op)
            z = up(("z0", "z1", "z2")[:nc])
            assert L.rh_ckks_scalar(h, level, 3, *ptrs(x), *ptrs(z), npoly, s0.ctypes.data_as(U), s1.ctypes.data_as(U)) == 0 and same(z, w["scalar", nc, 3])
            untouched([rh.Ciphertext(x)], [sel(o, ("a0", "a1", "a2")[:nc])])
            y = up(("a0", "a1", "a2")[:nc])                              # in place
            assert L.rh_ckks_scalar(h, level, 2, *ptrs(y), *ptrs(y), npoly, s0.ctypes.data_as(U), s1.ctypes.data_as(U)) == 0 and same(y, w["scalar", nc, 2])
        six = np.full(level + 1, 6, dtype=np.uint64)
        for key in [k for k in w if k[0] == "sta"]:
            _, da, db, sub, scaled_b = key
            x, y = up(("a0", "a1", "a2")[:da]), up(("b0", "b1", "b2")[:db])
            out = [rl.NewPoly(npoly) for _ in range(max(da, db))]
            ratio = six.ctypes.data_as(U) if scaled_b is not None else None
            assert L.rh_ckks_scale_then_add(h, level, *ptrs(x), *ptrs(y), *ptrs(out), npoly, ratio, sub, scaled_b or 0) == 0
            assert same(out, w[key]), key
            untouched([rh.Ciphertext(x), rh.Ciphertext(y)], [sel(o, ("a0", "a1", "a2")[:da]), sel(o, ("b0", "b1", "b2")[:db])])
    if npoly == 4 and level > 0:                                         # the polys built for it: the reduced sum, and ring.Neg of zero
        for i, q in enumerate(c.Q[:level + 1]):
            assert np.all(w["regular"][1][1, i] == (2 * (q - 1)) % q) and np.all(w["sta", 2, 3, 1, 0][2][3, i] == q)


# ---- the evaluator: Add / Sub --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_add(logN, logQ, level, npoly, d0, d1, s0, s1, sub):
    mods = chain(logN, logQ)[0][:level + 1]
    o = operands(logN, logQ, level, npoly)
    res = [cr.add_sub(1 << logN, mods, sel(o, ("a0", "a1", "a2")[:d0 + 1], k), S(s0), sel(o, ("b0", "b1", "b2")[:d1 + 1], k), S(s1), sub)
           for k in range(npoly)]
    return [np.stack([r[0][j] for r in res]) for j in range(len(res[0][0]))], res[0][1]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
@pytest.mark.parametrize("sub", [False, True])
def test_add_sub(rh, logN, logQ, level, npoly, sub, fused):
    c = Ctx(rh, logN, logQ)
    ev = c.ev[fused]
    o = operands(logN, logQ, level, npoly)
    for d0, d1 in ((1, 1), (1, 2), (2, 1), (1, 0)):                      # degree 1 +- degree 2: the copy and negate paths; a degree-0 plaintext
        an, bn = ("a0", "a1", "a2")[:d0 + 1], ("b0", "b1", "b2")[:d1 + 1]
        for s0, s1 in ((SB, SA), (SA, SA), (SA, SB)):                    # cmp 1, 0, -1
            want, scale = expected_add(logN, logQ, level, npoly, d0, d1, s0, s1, sub)
            for alias in (None, "op0", "op1"):
                if (alias == "op0" and d0 < d1) or (alias == "op1" and d1 < d0):
                    continue                                             # opOut has the larger degree
                a, b = ct(rh, c, level, sel(o, an), s0), ct(rh, c, level, sel(o, bn), s1)
                if alias is None:
                    out = (ev.SubNew if sub else ev.AddNew)(a, b)
                    untouched([a, b], [sel(o, an), sel(o, bn)])
                else:
                    out = a if alias == "op0" else b
                    (ev.Sub if sub else ev.Add)(a, b, out)
                    untouched([b if alias == "op0" else a], [sel(o, bn if alias == "op0" else an)])
                check(out, want, scale)
                assert out.Scale.Value == max(s0, s1)


# ---- scalars -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_scalars(rh, logN, logQ, level, npoly, fused):
    c = Ctx(rh, logN, logQ)
    ev = c.ev[fused]
    N, mods = c.N, c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)
    for const in SCALARS:
        for names in (("a0", "a1"), ("a0", "a1", "a2")):
            zn = ("z0", "z1", "z2")[:len(names)]
            op0 = ct(rh, c, level, sel(o, names), SA)
            for sub in (False, True):
                res = [cr.add_sub_scalar(N, mods, sel(o, names, k), S(SA), const, sub) for k in range(npoly)]
                check((ev.SubNew if sub else ev.AddNew)(op0, const), [np.stack([r[0][j] for r in res]) for j in range(len(names))], SA)
            res = [cr.mul_scalar(N, mods, sel(o, names, k), S(SA), const) for k in range(npoly)]
            want = [np.stack([r[0][j] for r in res]) for j in range(len(names))]
            check(ev.MulNew(op0, const), want, res[0][1])
            check(ev.MulRelinNew(op0, const), want, res[0][1])           # MulRelin of a scalar is Mul (:778-781)
            for sout in (SA, 4 * SA):                                    # equal scales; opOut.Scale > op0.Scale
                acc = ct(rh, c, level, sel(o, zn), sout)
                ev.MulRelinThenAdd(op0, const, acc)                      # -> MulThenAdd (:1088-1089)
                res = [cr.mul_then_add_scalar(N, mods, sel(o, names, k), S(SA), const, sel(o, zn, k), S(sout)) for k in range(npoly)]
                check(acc, [np.stack([r[0][j] for r in res]) for j in range(len(names))], res[0][1])
            untouched([op0], [sel(o, names)])
    op0 = ct(rh, c, level, sel(o, ("a0", "a1")), SA)
    inplace = ct(rh, c, level, sel(o, ("a0", "a1")), SA)
    ev.Mul(inplace, 0.5, inplace)
    check(inplace, [x.numpy() for x in ev.MulNew(op0, 0.5).Value], S(SA).mul(S(mods[-1])))
    up = ev.ScaleUpNew(op0, rh.ckks.Scale(2 ** 20))                      # ScaleUp (:456-465)
    res = [cr.mul_scalar(N, mods, sel(o, ("a0", "a1"), k), S(SA), 2 ** 20) for k in range(npoly)]
    check(up, [np.stack([r[0][j] for r in res]) for j in range(2)], SA * 2 ** 20)
    with pytest.raises(rh.RingHipError, match="op0.Scale > opOut.Scale is not supported"):
        ev.MulThenAdd(ct(rh, c, level, sel(o, ("a0", "a1")), 4 * SA), 3, ct(rh, c, level, sel(o, ("z0", "z1")), SA))


# ---- Mul, MulThenAdd, MulRelin(ThenAdd) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
def test_mul_and_mul_then_add(rh, logN, logQ, level, npoly, fused):
    c = Ctx(rh, logN, logQ)
    ev = c.ev[fused]
    N, mods = c.N, c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)
    A, B, Z = ("a0", "a1"), ("b0", "b1"), ("z0", "z1", "z2")
    w = expected_kernels(logN, logQ, level, npoly)
    op0, op1 = ct(rh, c, level, sel(o, A), SA), ct(rh, c, level, sel(o, B), SB)
    check(ev.MulNew(op0, op1), w["regular"], S(SA).mul(S(SB)))
    check(ev.MulNew(op0, op0), w["square"], SA * SA)
    if fused:                                                            # one launch reads every operand before it writes: opOut may share op1's polys
        alias = ct(rh, c, level, sel(o, B), SB)
        out = rh.Ciphertext([alias.Value[0], alias.Value[1], c.rq.AtLevel(level).NewPoly(npoly)], is_ntt=True)
        ev.MulRelin(op0, alias, out, relin=False)
        check(out, w["regular"])
    for sout, scaled in ((SA * SB, False), (SA * SB // 2, True), (SA * SB // 2 + 2 ** 40, False)):       # ratio 1; 2.0; 1.99..
        acc = ct(rh, c, level, sel(o, Z), sout)
        ev.MulThenAdd(op0, op1, acc)
        res = [cr.mul_relin_then_add(N, mods, sel(o, A, k), S(SA), sel(o, B, k), S(SB), sel(o, Z, k), S(sout), False) for k in range(npoly)]
        assert (res[0][1] == S(SA).mul(S(SB)).v) == (scaled or sout == SA * SB)
        check(acc, [np.stack([r[0][j] for r in res]) for j in range(3)], res[0][1])
    for d in (0, 1, 2):                                                  # plaintext branches: 1, 2 and 3 components
        names = ("a0", "a1", "a2")[:d + 1]
        x, pt = ct(rh, c, level, sel(o, names), SA), ct(rh, c, level, [o["pt"]], SB)
        check(ev.MulNew(x, pt), w["plain", d + 1, 0], S(SA).mul(S(SB)))
        acc = ct(rh, c, level, sel(o, Z), SA * SB)
        ev.MulRelinThenAdd(x, pt, acc)                                   # -> MulThenAdd (:1069-1070); a degree-2 accumulator
        check(acc, w["plain", d + 1, 1] + [o[n] for n in Z[d + 1:]], S(SA).mul(S(SB)))
        untouched([x, pt], [sel(o, names), [o["pt"]]])
    untouched([op0, op1], [sel(o, A), sel(o, B)])


@functools.lru_cache(maxsize=None)
def expected_relin(logN, logQ, level, npoly, mode):
    c = Ctx._cache[(logN, logQ)]
    mods = c.Q[:level + 1]
    w = expected_kernels(logN, logQ, level, npoly)
    src = w[{"regular": "regular", "square": "square", "acc": "acc2"}[mode]]

    def one(k):
        k0, k1 = key_switch(c, level, src[2][k], c.rlk)
        return [_vec("ADD", src[0][k], k0, _zeros(k0), None, mods), _vec("ADD", src[1][k], k1, _zeros(k1), None, mods)]
    return per_poly(one, npoly)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("logN,logQ,level,npoly", TOP)
def test_mul_relin_and_mul_relin_then_add(rh, logN, logQ, level, npoly, fused):
    c = Ctx(rh, logN, logQ)
    ev = c.ev[fused]
    o = operands(logN, logQ, level, npoly)
    A, B = ("a0", "a1"), ("b0", "b1")
    op0, op1 = ct(rh, c, level, sel(o, A), SA), ct(rh, c, level, sel(o, B), SB)
    check(ev.MulRelinNew(op0, op1), expected_relin(logN, logQ, level, npoly, "regular"), S(SA).mul(S(SB)))
    check(ev.MulRelinNew(op0, op0), expected_relin(logN, logQ, level, npoly, "square"), SA * SA)
    alias = ct(rh, c, level, sel(o, B), SB)
    ev.MulRelin(op0, alias, alias)                                       # opOut IS op1
    check(alias, expected_relin(logN, logQ, level, npoly, "regular"), S(SA).mul(S(SB)))
    acc = ct(rh, c, level, sel(o, ("z0", "z1")), SA * SB)
    ev.MulRelinThenAdd(op0, op1, acc)
    check(acc, expected_relin(logN, logQ, level, npoly, "acc"), S(SA).mul(S(SB)))
    acc2 = ct(rh, c, level, sel(o, ("z0", "z1", "z2")), SA * SB)         # a degree-2 accumulator keeps its last component (:1129)
    ev.MulRelinThenAdd(op0, op1, acc2)
    check(acc2, expected_relin(logN, logQ, level, npoly, "acc") + [o["z2"]])
    untouched([op0, op1], [sel(o, A), sel(o, B)])
    plain = ct(rh, c, level, sel(o, A), None)                            # callers without scales keep working, and get none
    out = rh.Ciphertext([c.rq.AtLevel(level).NewPoly(npoly) for _ in range(2)], is_ntt=True)
    ev.MulRelin(plain, ct(rh, c, level, sel(o, B), None), out)
    check(out, expected_relin(logN, logQ, level, npoly, "regular"))
    assert not hasattr(out, "Scale")


# ---- rotations -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expected_rotation(logN, logQ, level, npoly, gal):
    c = Ctx._cache[(logN, logQ)]
    mods = c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)

    def one(k):
        k0, k1 = key_switch(c, level, o["a1"][k], c.gal[gal])
        s = _vec("ADD", o["a0"][k], k0, _zeros(k0), None, mods)
        return [np.stack([orc.automorphism_ntt(x[i], gal) for i in range(level + 1)]) for x in (s, k1)]
    return per_poly(one, npoly)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("logN,logQ,level,npoly", TOP)
def test_rotations(rh, logN, logQ, level, npoly, fused):
    c = Ctx(rh, logN, logQ)
    ev = c.ev[fused]
    o = operands(logN, logQ, level, npoly)
    op0 = ct(rh, c, level, sel(o, ("a0", "a1")), SA)
    for k in (1, -1):
        assert ev.GaloisElement(k) == cr.galois_element(c.N, k)
        check(ev.RotateNew(op0, k), expected_rotation(logN, logQ, level, npoly, cr.galois_element(c.N, k)), SA)
    assert ev.GaloisElement(1) * ev.GaloisElement(-1) % (2 * c.N) == 1
    check(ev.ConjugateNew(op0), expected_rotation(logN, logQ, level, npoly, 2 * c.N - 1), SA)
    hoisted = ev.RotateHoistedNew(op0, [1, 2, -1])
    assert sorted(hoisted) == [-1, 1, 2]
    for k, out in hoisted.items():
        check(out, expected_rotation(logN, logQ, level, npoly, cr.galois_element(c.N, k)), SA)
    check(ev.RotateNew(op0, 0), sel(o, ("a0", "a1")), SA)                # Galois element 1: a copy
    untouched([op0], [sel(o, ("a0", "a1"))])
    with pytest.raises(rh.RingHipError, match=r"cannot Rotate: .*GaloisKey\[%d\] is missing" % cr.galois_element(c.N, 3)):
        ev.RotateNew(op0, 3)


# ---- Rescale, RescaleTo, SetScale, DropLevel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_rescale_to_and_levels(rh, fused):
    logN, logQ, level, npoly = SHAPES[2]
    c = Ctx(rh, logN, logQ)
    ev = c.ev[fused]
    N, mods = c.N, c.Q
    o = operands(logN, logQ, level, npoly)
    names = ("a0", "a1")
    big = mods[2] * mods[1] * 2 ** 40
    for min_scale, drops in ((2 ** 110, 0), (2 ** 80, 1), (2 ** 40, 2)):
        op0 = ct(rh, c, level, sel(o, names), big)
        res = [cr.rescale_to(N, mods, sel(o, names, k), S(big), S(min_scale)) for k in range(npoly)]
        assert cr.rescale_to_count(mods, S(big), S(min_scale))[0] == drops
        want = [np.stack([r[0][j] for r in res]) for j in range(2)]
        out = rh.Ciphertext([c.rq.AtLevel(level).NewPoly(npoly) for _ in range(2)], is_ntt=True)
        ev.RescaleTo(op0, min_scale, out)
        assert out.Level() == level - drops
        check(out, want, res[0][1])
        untouched([op0], [sel(o, names)])
        ev.RescaleTo(op0, min_scale, op0)                                # in place
        assert op0.Level() == level - drops
        check(op0, want, res[0][1])
    op0 = ct(rh, c, level, sel(o, names), big)
    res = [cr.rescale(N, mods, sel(o, names, k), S(big)) for k in range(npoly)]
    out = rh.Ciphertext([c.rq.AtLevel(level).NewPoly(npoly) for _ in range(2)], is_ntt=True)
    ev.Rescale(op0, out)                                                 # limbs 0 .. level-1 hold the result; the scale divided by q_level (:522-524)
    for j in range(2):
        assert np.array_equal(out.Value[j].numpy()[:, :level], np.stack([r[0][j] for r in res]))
    assert out.Scale.Value == res[0][1].v == S(big).div(S(mods[2])).v
    low = ev.DropLevelNew(op0, 1)
    assert low.Level() == level - 1 and low.Scale.Value == big
    check(low, [o[n][:, :level] for n in names])
    untouched([op0], [sel(o, names)])
    ev.DropLevel(op0, 2)
    check(op0, [o[n][:, :1] for n in names])
    # SetScale (:468-478): times round(ratio q_level) -- the quotient of the scales as a *big.Float is no integer type -- then RescaleTo the target
    x = ct(rh, c, level, sel(o, names), 2 ** 40)
    ev.SetScale(x, 2 ** 41)
    mul = [cr.mul_scalar(N, mods, sel(o, names, k), S(2 ** 40), Fraction(2)) for k in range(npoly)]
    assert mul[0][1] == 2 ** 40                                          # 2.0 is a Gaussian integer: scale 1, nothing to divide afterwards
    res = [cr.rescale_to(N, mods, mul[k][0], mul[k][1], S(2 ** 41)) for k in range(npoly)]
    check(x, [np.stack([r[0][j] for r in res]) for j in range(2)], 2 ** 41)
    y = ct(rh, c, level, sel(o, names), 2 ** 40)
    ev.SetScale(y, 3 * 2 ** 39)                                          # ratio 1.5: scaled by round(1.5 q_2), one level consumed
    mul = [cr.mul_scalar(N, mods, sel(o, names, k), S(2 ** 40), Fraction(3, 2)) for k in range(npoly)]
    res = [cr.rescale_to(N, mods, mul[k][0], mul[k][1], S(3 * 2 ** 39)) for k in range(npoly)]
    assert y.Level() == level - 1
    check(y, [np.stack([r[0][j] for r in res]) for j in range(2)], 3 * 2 ** 39)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(rh):
    c = Ctx(rh, 10, (55, 45, 45))
    ev, rq = c.ev[True], c.rq

    def mk(d, scale=SA, ring=rq):
        x = rh.Ciphertext([ring.NewPoly(1) for _ in range(d + 1)], True)
        if scale is not None:
            x.Scale = rh.ckks.Scale(scale)
        return x
    x, y, out1, out2 = mk(1), mk(1), mk(1), mk(2)
    for f, args in ((ev.Add, (x, [1.0, 2.0], out1)), (ev.Sub, (x, np.arange(4.0), out1)), (ev.Mul, (x, (1, 2), out1)), (ev.MulRelin, (x, [1j], out1)),
                    (ev.MulThenAdd, (x, [1], out1)), (ev.MulRelinThenAdd, (x, [1], out1)), (ev.AddNew, (x, [1])), (ev.MulNew, (x, [1]))):
        with pytest.raises(rh.RingHipError, match="needs the CKKS encoder"):
            f(*args)
    with pytest.raises(rh.RingHipError, match="invalid op1"):
        ev.Add(x, "3", out1)
    bare = mk(1, None)
    for f, args in ((ev.Add, (bare, y, out1)), (ev.Add, (x, bare, out1)), (ev.Sub, (bare, 3, out1)), (ev.Mul, (bare, y, out2)), (ev.Mul, (bare, 2, out1)),
                    (ev.MulThenAdd, (x, y, mk(2, None))), (ev.MulThenAdd, (bare, 2, out1)), (ev.Rotate, (bare, 1, out1)), (ev.Conjugate, (bare, out1)),
                    (ev.RotateHoistedNew, (bare, [1])), (ev.RescaleTo, (bare, 2 ** 30, out1)), (ev.ScaleUp, (bare, 2, out1)), (ev.SetScale, (bare, 2))):
        with pytest.raises(rh.RingHipError, match="carries no Scale"):
            f(*args)
    low = mk(1, SA, rq.AtLevel(1))
    for f, args in ((ev.Add, (x, low, out1)), (ev.Mul, (x, low, out2)), (ev.MulThenAdd, (x, low, out2)), (ev.Sub, (x, 2, low)), (ev.MulRelinThenAdd, (x, y, low))):
        with pytest.raises(rh.RingHipError, match="operands must sit at the same level"):
            f(*args)
    for f in (ev.MulThenAdd, ev.MulRelinThenAdd):
        for out in (x, y):
            with pytest.raises(rh.RingHipError, match="cannot MulThenAdd: opOut must be different from op0 and op1"):
                f(x, y, out)
    with pytest.raises(rh.RingHipError, match="opOut must have degree 2"):
        ev.Add(x, out2, out1)
    with pytest.raises(rh.RingHipError, match="opOut must have degree 2"):
        ev.MulThenAdd(x, y, out1)
    with pytest.raises(rh.RingHipError, match="opOut must have degree 2"):
        ev.Mul(x, y, out1)
    with pytest.raises(rh.RingHipError, match="opOut must have degree 1"):
        ev.MulRelin(x, y, out2)
    no_key = rh.ckks.Evaluator(rq, c.rp)
    with pytest.raises(rh.RingHipError, match="relinearization key is missing"):
        no_key.MulRelin(x, y, out1)
    with pytest.raises(rh.RingHipError, match="relinearization key is missing"):
        no_key.MulRelinThenAdd(x, y, out1)
    with pytest.raises(rh.RingHipError, match=r"cannot Conjugate: .*GaloisKey\[%d\] is missing" % (2 * c.N - 1)):
        no_key.Conjugate(x, out1)
    no_key.close()
    with pytest.raises(rh.RingHipError, match="without ringP"):
        rh.ckks.Evaluator(rq).Rotate(x, 1, out1)
    bottom = mk(1, SA, rq.AtLevel(0))
    with pytest.raises(rh.RingHipError, match="already at level 0"):
        ev.RescaleTo(bottom, 2 ** 20, bottom)
    with pytest.raises(rh.RingHipError, match="level is too low"):
        ev.Rescale(bottom, bottom)
    with pytest.raises(rh.RingHipError, match="minScale is <0"):
        ev.RescaleTo(x, 0, out1)
    with pytest.raises(rh.RingHipError, match="cannot DropLevel"):
        ev.DropLevel(x, 3)
    from conftest import QI60
    ci = rh.Ring(c.N, QI60[:2], kind=rh.ConjugateInvariant)
    cev = rh.ckks.Evaluator(ci)
    cx = mk(1, SA, ci)
    with pytest.raises(rh.RingHipError, match="not supported when parameters.RingType\\(\\) == ring.ConjugateInvariant"):
        cev.Conjugate(cx, cx)
    assert cev.GaloisElement(1) == 5 and cev.GaloisElement(-1) * 5 % (4 * c.N) == 1
    # the C entry points: negative status and rh_last_error
    L = rh.lib()
    a = [rq.NewPoly(1) for _ in range(9)]
    p = [v.ptr for v in a]
    k = np.zeros(3, dtype=np.uint64)
    kp = k.ctypes.data_as(rh.ringhip.U64P)
    assert L.rh_ckks_tensor(ci._h, 1, *p[:7], 1, 0, 0) == 0              # a conjugate-invariant ring is served
    ci.sync()
    cev.close(); ci.close()
    assert L.rh_ckks_tensor(rq._h, 3, *p[:7], 1, 0, 0) == -1 and b"level 3 out of range" in L.rh_last_error()
    assert L.rh_ckks_tensor(rq._h, 2, *p[:7], 1, 3, 0) == -1 and b"accumulate must be" in L.rh_last_error()
    assert L.rh_ckks_tensor(rq._h, 2, *p[:7], 1, 1, 1) == -1 and b"squaring case comes without accumulate" in L.rh_last_error()
    assert L.rh_ckks_tensor(rq._h, 2, *p[:7], 1, 0, 1) == -1 and b"b = NULL or b == a" in L.rh_last_error()
    assert L.rh_ckks_tensor(rq._h, 2, p[0], p[1], None, None, *p[4:7], 1, 0, 0) == -1 and b"null argument" in L.rh_last_error()
    assert L.rh_ckks_mul_plain(rq._h, 2, p[0], None, p[1], p[2], p[3], None, p[4], 1, 0) == -1 and b"component 2 needs component 1" in L.rh_last_error()
    assert L.rh_ckks_mul_plain(rq._h, 2, p[0], None, None, p[2], p[3], None, None, 1, 2) == -1 and b"accumulate must be 0 or 1" in L.rh_last_error()
    assert L.rh_ckks_scalar(rq._h, 2, 4, p[0], None, None, p[1], None, None, 1, kp, kp) == -1 and b"op must be" in L.rh_last_error()
    bigk = np.array([c.Q[0], 0, 0], dtype=np.uint64).ctypes.data_as(rh.ringhip.U64P)
    assert L.rh_ckks_scalar(rq._h, 2, 0, p[0], None, None, p[1], None, None, 1, bigk, kp) == -1 and b"not below its modulus" in L.rh_last_error()
    assert L.rh_ckks_scale_then_add(rq._h, 2, p[0], None, None, p[1], None, None, p[2], None, None, 1, bigk, 0, 0) == -1 and b"not below its modulus" in L.rh_last_error()
    assert L.rh_ckks_scale_then_add(rq._h, 2, p[0], p[3], None, p[1], None, None, p[2], None, None, 1, kp, 0, 0) == -1 and b"components of the larger operand" in L.rh_last_error()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    assert L.rh_ckks_tensor(r3._h, 1, *p[:7], 1, 0, 0) == -1 and b"3N rings are not supported" in L.rh_last_error()
    assert L.rh_ckks_scalar(r3._h, 1, 0, p[0], None, None, p[1], None, None, 1, kp, kp) == -1 and b"3N rings are not supported" in L.rh_last_error()
    r3.close()

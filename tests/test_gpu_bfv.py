"""GPU: the BFV ciphertext multiply (csrc/bfv.hip, matrix-fhe-lattigo_amd/bgv.py) bit for bit, whole outputs, against the restatement of
schemes/bgv/evaluator.go:975-1124 that tests/test_bfv_oracle.py pins to big-integer ground truth."""
import functools
import random

import numpy as np
import pytest

import bfv_restatement as br
from test_bfv_oracle import T, chain

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def params(logN, logQ):
    Q, M = chain(logN, list(logQ))
    return br.Params(1 << logN, Q, M, T)


class Ctx:
    """rings + evaluator of one chain, shared by the tests of a module run"""
    _cache = {}

    def __new__(cls, rh, logN, logQ):
        key = (logN, tuple(logQ))
        if key not in cls._cache:
            self = object.__new__(cls)
            self.P = params(logN, tuple(logQ))
            self.rq, self.rm = rh.Ring(self.P.N, self.P.Q), rh.Ring(self.P.N, self.P.QMul)
            self.ev = rh.bgv.Evaluator(self.rq, self.rm, T)
            cls._cache[key] = self
        return cls._cache[key]


def uniform(rng, mods, npoly, N):
    return np.stack([np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in mods]) for _ in range(npoly)])


def patterns(rng, mods, N):
    """three polys: uniform, all zero, all q_i - 1"""
    return np.stack([uniform(rng, mods, 1, N)[0], np.zeros((len(mods), N), dtype=np.uint64),
                     np.stack([np.full(N, int(q) - 1, dtype=np.uint64) for q in mods])])


# path: what the shape gets with the tuning key "fused_quantize" = 1 (the default, 0, sends every shape down the composed sequence)
SHAPES = [(5, (61, 61), 0, 1, 2, "fused"),            # smallest
          (10, (55, 45, 45), 2, 3, 3, "fused"),       # register path
          (10, (55, 45, 45), 0, 1, 2, "fused"),       # level 0 of the 3-limb ring: its own plans, levelQMul differs from the top's
          (10, (45,) * 9, 8, 9, 7, "composed")]       # 9 > 8 words of Q: the three existing launches


@pytest.mark.parametrize("logN,logQ,level,nq,nm,path", SHAPES)
def test_quantize_alone(rh, logN, logQ, level, nq, nm, path):
    c = Ctx(rh, logN, logQ)
    P, N = c.P, c.P.N
    Ql, Ml, _, _ = P.at(level)
    assert (len(Ql), len(Ml)) == (nq, nm) and c.ev.levelQMul[level] == nm - 1 == P.levelQMul[level]
    assert c.ev.QuantizePath(level) == "composed"                                     # the default
    rng = np.random.default_rng(logN * 10 + level)
    xq, xm = patterns(rng, Ql, N), patterns(rng, Ml, N)
    want = np.stack([br.quantize(P, level, xq[k], xm[k]) for k in range(3)])
    rl, ml = c.rq.AtLevel(level), c.rm.AtLevel(nm - 1)
    for fused in (0, 1):
        c.ev.set_tuning("fused_quantize", fused)
        try:
            assert c.ev.QuantizePath(level) == (path if fused else "composed")        # 9 limbs of Q stay composed whatever the key says
            pq, pm, out = rh.DevicePoly.from_numpy(rl, xq), rh.DevicePoly.from_numpy(ml, xm), rl.NewPoly(3)
            c.ev.Quantize(level, pq, pm, out)
            assert np.array_equal(out.numpy(), want)
            assert np.array_equal(pq.numpy(), xq) and np.array_equal(pm.numpy(), xm)  # inputs untouched
            c.ev.Quantize(level, pq, pm)                                              # in place, as the reference
            assert np.array_equal(pq.numpy(), want)
        finally:
            c.ev.set_tuning("fused_quantize", 0)
    with pytest.raises(rh.RingHipError, match="unknown key"):
        c.ev.set_tuning("no_such_key", 1)


@pytest.mark.parametrize("logN,logQ,level,nq,nm,path", SHAPES)
@pytest.mark.parametrize("square", [False, True])
def test_tensor_lazy(rh, logN, logQ, level, nq, nm, path, square):
    c = Ctx(rh, logN, logQ)
    P, N = c.P, c.P.N
    Ql, Ml, _, _ = P.at(level)
    rng = np.random.default_rng(logN * 20 + level + square)
    rl, ml = c.rq.AtLevel(level), c.rm.AtLevel(nm - 1)
    hq = [patterns(rng, Ql, N) for _ in range(4)]                # uniform, (zeros, replaced below), all q - 1
    hm = [patterns(rng, Ml, N) for _ in range(4)]
    for h, mods in ((hq, Ql), (hm, Ml)):                         # poly 1 (zeros in `patterns`): operands whose two products sum past q
        for i, q in enumerate(mods):
            h[0][1, i] = 1; h[1][1, i] = 1; h[2][1, i] = int(q) - 1; h[3][1, i] = int(q) - 1      # 1 (q-1) + 1 (q-1) = 2q - 2
    dq = [rh.DevicePoly.from_numpy(rl, a) for a in hq]
    dm = [rh.DevicePoly.from_numpy(ml, a) for a in hm]
    oq, om = [rl.NewPoly(3) for _ in range(3)], [ml.NewPoly(3) for _ in range(3)]
    c.ev.TensorLowDeg(level, dq[:2], None if square else dq[2:], oq, dm[:2], None if square else dm[2:], om)
    for h, mods, outs in ((hq, Ql, oq), (hm, Ml, om)):
        got = [o.numpy() for o in outs]
        for k in range(3):
            want = br.tensor_low_deg(mods, [h[0][k], h[1][k]], None if square else [h[2][k], h[3][k]])
            for j in range(3):
                assert np.array_equal(got[j][k], want[j]), (k, j)
        if not square:
            for i, q in enumerate(mods):
                assert np.all(got[1][1, i] == 2 * int(q) - 2)     # the unreduced sum, >= q


@pytest.mark.parametrize("logN,logQ,level", [(5, (61, 61), 0), (10, (55, 45, 45), 2), (12, (55, 45, 45), 2), (15, (61, 61), 1)])
def test_quantize_takes_the_unreduced_c1_of_tensor_lazy(rh, logN, logQ, level):
    # ringhip.h: rh_bfv_quantize accepts residues in [0, 2q), which is what rh_bfv_tensor_lazy leaves in c1 -- through every inverse
    # transform (one workgroup per limb, the 4096 tile, the two-pass launches) and both forms of the middle
    c = Ctx(rh, logN, logQ)
    P, N = c.P, c.P.N
    Ql, Ml, _, _ = P.at(level)
    rng = np.random.default_rng(logN * 7 + level)
    rl, ml = c.rq.AtLevel(level), c.rm.AtLevel(len(Ml) - 1)
    hq, hm = [uniform(rng, Ql, 2, N) for _ in range(4)], [uniform(rng, Ml, 2, N) for _ in range(4)]
    for h, mods in ((hq, Ql), (hm, Ml)):                         # poly 1: every c1 word is 2q - 2
        for i, q in enumerate(mods):
            h[0][1, i] = 1; h[1][1, i] = 1; h[2][1, i] = int(q) - 1; h[3][1, i] = int(q) - 1
    dq, dm = [rh.DevicePoly.from_numpy(rl, a) for a in hq], [rh.DevicePoly.from_numpy(ml, a) for a in hm]
    oq, om = [rl.NewPoly(2) for _ in range(3)], [ml.NewPoly(2) for _ in range(3)]
    c.ev.TensorLowDeg(level, dq[:2], dq[2:], oq, dm[:2], dm[2:], om)
    c1q, c1m = oq[1].numpy(), om[1].numpy()
    for i, q in enumerate(Ql):
        assert np.all(c1q[1, i] == 2 * int(q) - 2) and np.any(c1q[0, i] >= np.uint64(q))
    for j, p in enumerate(Ml):
        assert np.all(c1m[1, j] == 2 * int(p) - 2) and np.any(c1m[0, j] >= np.uint64(p))
    want = np.stack([br.quantize(P, level, c1q[k], c1m[k]) for k in range(2)])
    canon = np.stack([br.quantize(P, level, np.stack([c1q[k, i] % np.uint64(q) for i, q in enumerate(Ql)]),
                                  np.stack([c1m[k, j] % np.uint64(p) for j, p in enumerate(Ml)])) for k in range(2)])
    assert np.array_equal(want, canon)                           # a function of the residues
    out = rl.NewPoly(2)
    for fused in (0, 1):
        c.ev.set_tuning("fused_quantize", fused)
        try:
            c.ev.Quantize(level, oq[1], om[1], out)
            assert np.array_equal(out.numpy(), want), fused
        finally:
            c.ev.set_tuning("fused_quantize", 0)


def _cts(P, level, npoly, seed):
    rng = np.random.default_rng(seed)
    Ql = P.Q[:level + 1]
    return [uniform(rng, Ql, npoly, P.N) for _ in range(4)]         # a0, a1, b0, b1


@functools.lru_cache(maxsize=None)
def expected(logN, logQ, level, npoly, square):
    P = params(logN, logQ)
    a0, a1, b0, b1 = _cts(P, level, npoly, logN * 1000 + level * 10 + npoly)
    out = [br.tensor_scale_invariant(P, level, [a0[k], a1[k]], None if square else [b0[k], b1[k]]) for k in range(npoly)]
    return [np.stack([out[k][j] for k in range(npoly)]) for j in range(3)]


E2E = [(12, (55, 45, 45), 2), (15, (61, 61), 1), (12, (55, 45, 45), 1)]        # the last: operands below the ring's top level


@pytest.mark.parametrize("logN,logQ,level", E2E)
@pytest.mark.parametrize("npoly", [1, 3])
@pytest.mark.parametrize("case", ["normal", "square", "out_is_op1", "out_is_op0"])
@pytest.mark.parametrize("fused", [0, 1])
def test_mul_scale_invariant(rh, logN, logQ, level, npoly, case, fused):
    c = Ctx(rh, logN, logQ)
    c.ev.set_tuning("fused_quantize", fused)
    try:
        assert c.ev.QuantizePath(level) == ("fused" if fused else "composed")
        _mul_case(rh, c, logN, logQ, level, npoly, case)
    finally:
        c.ev.set_tuning("fused_quantize", 0)


def _mul_case(rh, c, logN, logQ, level, npoly, case):
    P = c.P
    rl = c.rq.AtLevel(level)
    h = _cts(P, level, npoly, logN * 1000 + level * 10 + npoly)
    d = [rh.DevicePoly.from_numpy(rl, a) for a in h]
    op0, op1 = rh.Ciphertext(d[:2], is_ntt=True), rh.Ciphertext(d[2:], is_ntt=True)
    op0.Scale, op1.Scale = 3, 5
    extra = rl.NewPoly(npoly)
    if case == "square":
        out = rh.Ciphertext([rl.NewPoly(npoly), rl.NewPoly(npoly), extra], is_ntt=True)
        c.ev.MulScaleInvariant(op0, op0, out)
        s1 = 3
    elif case == "normal":
        out = c.ev.MulScaleInvariantNew(op0, op1)
        s1 = 5
    else:
        # opOut's first two polys ARE an operand's (ct1 == opOut :983, ct0 == opOut): nothing may be written before every input is read
        src = op1 if case == "out_is_op1" else op0
        out = rh.Ciphertext([src.Value[0], src.Value[1], extra], is_ntt=True)
        c.ev.MulScaleInvariant(op0, op1, out)
        s1 = 5
    want = expected(logN, logQ, level, npoly, case == "square")
    for j in range(3):
        assert np.array_equal(out.Value[j].numpy(), want[j]), j
    assert out.IsNTT and out.Scale == br.scale_invariant(T, br.prod(P.Q[:level + 1]), 3, s1)
    if case in ("normal", "square"):                                # operands untouched
        assert np.array_equal(d[0].numpy(), h[0]) and np.array_equal(d[3].numpy(), h[3])


def test_mul_relin_scale_invariant(rh):
    # N = 2^12, L = 3, P = one 61-bit prime, random key: restatement + oracle gadget product + two adds
    logN, logQ, level, npoly = 12, (55, 45, 45), 2, 2
    N = 1 << logN
    nb = br.nb_qi_mul(params(logN, logQ).Q, logN)
    from oracle import primes
    Q, MP = primes.gen_moduli(logN + 1, list(logQ), [61] * (nb + 1))
    M, Pk = MP[:nb], MP[nb:]
    P = br.Params(N, Q, M, T)
    rng = np.random.default_rng(99)
    evkQ = np.stack([np.stack([uniform(rng, Q, 1, N)[0] for _ in range(2)]) for _ in range(len(Q))])
    evkP = np.stack([np.stack([uniform(rng, Pk, 1, N)[0] for _ in range(2)]) for _ in range(len(Q))])
    rq, rm, rp = rh.Ring(N, Q), rh.Ring(N, M), rh.Ring(N, Pk)
    rlk = rh.rlwe.GadgetCiphertext(rq, rp, evkQ, evkP)
    ev = rh.bgv.Evaluator(rq, rm, T, ringP=rp, rlk=rlk)
    h = _cts(P, level, npoly, 4242)
    d = [rh.DevicePoly.from_numpy(rq, a) for a in h]
    op0, op1 = rh.Ciphertext(d[:2], is_ntt=True), rh.Ciphertext(d[2:], is_ntt=True)
    out = ev.MulRelinScaleInvariantNew(op0, op1)
    assert out.Degree() == 1
    g = [out.Value[0].numpy(), out.Value[1].numpy()]
    for k in range(npoly):
        c = br.tensor_scale_invariant(P, level, [h[0][k], h[1][k]], [h[2][k], h[3][k]])
        w = br.relinearize(N, Q, Pk, level, c, evkQ, evkP)
        assert np.array_equal(g[0][k], w[0]) and np.array_equal(g[1][k], w[1])
    no_key = rh.bgv.Evaluator(rq, rm, T, ringP=rp)
    with pytest.raises(rh.RingHipError, match="relinearization key is missing"):
        no_key.MulRelinScaleInvariantNew(op0, op1)
    no_key.close(); ev.close(); rq.close(); rm.close(); rp.close()


def test_decryption_through_the_device_path(rh):
    # the ground truth of tests/test_bfv_oracle.py, the multiply on the device: N = 2^10, every coefficient
    logN, logQ, level = 10, (55, 45, 45), 2
    c = Ctx(rh, logN, logQ)
    P, N = c.P, c.P.N
    rnd = random.Random(2024)
    s = [rnd.randrange(-1, 2) for _ in range(N)]
    m0, m1 = [rnd.randrange(T) for _ in range(N)], [rnd.randrange(T) for _ in range(N)]
    h0, h1 = br.encrypt(rnd, P, level, m0, s), br.encrypt(rnd, P, level, m1, s)
    mk = lambda h: rh.Ciphertext([rh.DevicePoly.from_numpy(c.rq, x[None]) for x in h], is_ntt=True)
    out = c.ev.MulScaleInvariantNew(mk(h0), mk(h1))
    got = [v.numpy()[0] for v in out.Value]
    d = br.decrypt_product(P, level, got, s)
    f = T - br.prod(P.Q) % T
    assert [(x * f) % T for x in d] == br.negacyclic_mul_mod_t(m0, m1, T)
    assert out.Scale * f % T == 1


def test_error_paths(rh):
    c = Ctx(rh, 10, (55, 45, 45))
    rq, rm = c.rq, c.rm
    for bad_t, what in ((0, "zero"), (int(c.P.Q[0]) + 2, "exceeds q_0"), (int(c.P.Q[1]), "is a modulus of Q")):
        with pytest.raises(rh.RingHipError, match=what):
            rh.bgv.Evaluator(rq, rm, bad_t)
    other = rh.Ring(2048, params(11, (55, 45, 45)).QMul)
    with pytest.raises(rh.RingHipError, match="differ in N"):
        rh.bgv.Evaluator(rq, other, T)
    other.close()
    short = rh.Ring(c.P.N, c.P.QMul[:2])                          # levelQMul[2] = 2 needs three moduli
    ev = rh.bgv.Evaluator(rq, short, T)
    a = [rq.NewPoly(1) for _ in range(7)]
    with pytest.raises(rh.RingHipError, match="ringQMul has 2 moduli"):
        ev.MulScaleInvariant(rh.Ciphertext(a[:2], True), rh.Ciphertext(a[2:4], True), rh.Ciphertext(a[4:], True))
    ev.close(); short.close()
    ct = rh.Ciphertext(a[:2], True)
    pt = rh.Ciphertext(a[2:3], True)
    with pytest.raises(rh.RingHipError, match="degree-0 operand goes to tensorStandard"):
        c.ev.MulScaleInvariant(ct, pt, rh.Ciphertext(a[4:], True))
    with pytest.raises(rh.RingHipError, match="tensorStandard / Mul"):
        c.ev.MulRelinScaleInvariant(ct, 7, rh.Ciphertext(a[4:6], True))
    with pytest.raises(rh.RingHipError, match="tensorStandard / Mul"):
        c.ev.MulScaleInvariant(ct, [1, 2, 3], rh.Ciphertext(a[4:], True))
    from conftest import QI60
    ci = rh.Ring(c.P.N, QI60[:2], kind=rh.ConjugateInvariant)       # refused for its kind before anything else is looked at
    with pytest.raises(rh.RingHipError, match="standard rings"):
        rh.bgv.Evaluator(ci, rm, T)
    ci.close()

"""GPU: the BGV half of bgv.Evaluator (csrc/bgv.hip, matrix-fhe-lattigo_amd/bgv.py) bit for bit, whole outputs, against the restatement of
schemes/bgv/evaluator.go that tests/test_bgv_oracle.py pins to big-integer ground truth; inputs untouched where they are not the output."""
import functools

import numpy as np
import pytest

import bfv_restatement as br
import bgv_restatement as gr
from oracle import primes
from test_bfv_oracle import T

pytestmark = pytest.mark.gpu

KINDS = ("uniform", "sum_past_q", "q_minus_1", "zero")


@functools.lru_cache(maxsize=None)
def chain(logN, logQ):
    """Q and one 61-bit P for the relinearisation key, from one GenModuli call: the Q primes are those of tests/test_gpu_bfv.py's chains"""
    Q, Pk = primes.gen_moduli(logN + 1, list(logQ), [61])
    return [int(q) for q in Q], [int(p) for p in Pk]


def uniform(rng, mods, N):
    return np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in mods])


@functools.lru_cache(maxsize=None)
def operands(logN, logQ, level, npoly):
    """eight blocks (npoly, level+1, N): a0 a1 b0 b1 (operands), z0 z1 z2 (accumulator), pt.  Poly k follows KINDS[k]: uniform; built so that
    a0 b1 + a1 b0 and the accumulate sum pass q (1 (q-1) + 1 (q-1), accumulator q-1); all q_i - 1; all zero."""
    mods = chain(logN, logQ)[0][:level + 1]
    N = 1 << logN
    rng = np.random.default_rng(logN * 100 + level * 10 + npoly)
    out = []
    for name in ("a0", "a1", "b0", "b1", "z0", "z1", "z2", "pt"):
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
        out.append(a)
    return dict(zip(("a0", "a1", "b0", "b1", "z0", "z1", "z2", "pt"), out))


class Ctx:
    """ring, key-switch ring, a random relinearisation key and the evaluators of one chain, shared by the tests of a module run"""
    _cache = {}

    def __new__(cls, rh, logN, logQ):
        key = (logN, tuple(logQ))
        if key not in cls._cache:
            self = object.__new__(cls)
            self.Q, self.Pk = chain(logN, tuple(logQ))
            self.N = 1 << logN
            self.rq, self.rp = rh.Ring(self.N, self.Q), rh.Ring(self.N, self.Pk)
            rng = np.random.default_rng(logN + len(logQ))
            self.evkQ = np.stack([np.stack([uniform(rng, self.Q, self.N) for _ in range(2)]) for _ in self.Q])
            self.evkP = np.stack([np.stack([uniform(rng, self.Pk, self.N) for _ in range(2)]) for _ in self.Q])
            rlk = rh.rlwe.GadgetCiphertext(self.rq, self.rp, self.evkQ, self.evkP)
            self.ev = rh.bgv.Evaluator(self.rq, None, T, ringP=self.rp, rlk=rlk)               # a pure BGV evaluator: no ringQMul
            self.composed = rh.bgv.Evaluator(self.rq, None, T, ringP=self.rp, rlk=rlk, fused=False)
            cls._cache[key] = self
        return cls._cache[key]


def ct(rh, c, level, blocks, scale):
    rl = c.rq.AtLevel(level)
    out = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, b) for b in blocks], is_ntt=True)
    out.Scale = scale
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
        assert out.Scale == scale


def untouched(cts, blocks):
    for c_, b in zip(cts, blocks):
        for v, h in zip(c_.Value, b):
            assert np.array_equal(v.numpy(), h)


# (logN, logQ, level, npoly): the chains of tests/test_gpu_bfv.py; N = 32 with npoly = 3 (a grid with a ragged tail); logN 13: more than one block per limb
SHAPES = [(5, (61, 61), 0, 3), (5, (61, 61), 1, 4), (10, (55, 45, 45), 0, 4), (10, (55, 45, 45), 2, 4), (10, (45,) * 9, 8, 4), (13, (61, 61), 1, 2)]
TOP = [s for s in SHAPES if s[2] == len(s[1]) - 1]                   # the relinearisation key is used at the level it was made for
S0, S1 = 3, 5


@functools.lru_cache(maxsize=None)
def expected_tensor(logN, logQ, level, npoly, square, relin):
    mods, Pk = chain(logN, logQ)
    o = operands(logN, logQ, level, npoly)

    def one(k):
        b = [o["a0"][k], o["a1"][k]] if square else [o["b0"][k], o["b1"][k]]
        c, _ = gr.tensor_standard(mods[:level + 1], T, [o["a0"][k], o["a1"][k]], S0, b, S0 if square else S1, square)
        if relin:
            cx = Ctx._cache[(logN, logQ)]
            return br.relinearize(1 << logN, mods, Pk, level, c, cx.evkQ, cx.evkP)
        return c
    return per_poly(one, npoly)


@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
@pytest.mark.parametrize("square", [False, True])
def test_mul(rh, logN, logQ, level, npoly, square):
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    op0, op1 = ct(rh, c, level, [o["a0"], o["a1"]], S0), ct(rh, c, level, [o["b0"], o["b1"]], S1)
    out = c.ev.MulNew(op0, op0 if square else op1)
    check(out, expected_tensor(logN, logQ, level, npoly, square, False), (S0 * S0 if square else S0 * S1) % T)
    untouched([op0, op1], [[o["a0"], o["a1"]], [o["b0"], o["b1"]]])
    if not square:                                                   # the poly built for it: c1 = 2 (q - 1) T reduced, not the lazy sum
        for i, q in enumerate(c.Q[:level + 1]):
            assert np.all(out.Value[1].numpy()[1, i] == 2 * (q - 1) * T % q)


@pytest.mark.parametrize("logN,logQ,level,npoly", TOP)
@pytest.mark.parametrize("square", [False, True])
def test_mul_relin(rh, logN, logQ, level, npoly, square):
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    op0, op1 = ct(rh, c, level, [o["a0"], o["a1"]], S0), ct(rh, c, level, [o["b0"], o["b1"]], S1)
    out = c.ev.MulRelinNew(op0, op0 if square else op1)
    check(out, expected_tensor(logN, logQ, level, npoly, square, True), (S0 * S0 if square else S0 * S1) % T)
    untouched([op0, op1], [[o["a0"], o["a1"]], [o["b0"], o["b1"]]])


@pytest.mark.parametrize("logN,logQ,level,npoly", [SHAPES[0], SHAPES[3], SHAPES[5]])
@pytest.mark.parametrize("alias", ["op0", "op1"])
@pytest.mark.parametrize("relin", [False, True])
def test_mul_output_is_an_operand(rh, logN, logQ, level, npoly, alias, relin):
    if relin and (logN, logQ, level, npoly) not in TOP:
        level, npoly = len(logQ) - 1, 4
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    op0, op1 = ct(rh, c, level, [o["a0"], o["a1"]], S0), ct(rh, c, level, [o["b0"], o["b1"]], S1)
    src = op0 if alias == "op0" else op1
    if relin:
        c.ev.MulRelin(op0, op1, src)                                 # opOut IS the operand (:693-698)
        out = src
    else:                                                            # opOut's first two polys are the operand's: nothing is written before every input is read
        out = rh.Ciphertext([src.Value[0], src.Value[1], c.rq.AtLevel(level).NewPoly(npoly)], is_ntt=True)
        c.ev.Mul(op0, op1, out)
    check(out, expected_tensor(logN, logQ, level, npoly, False, relin), S0 * S1 % T)
    other, blocks = (op1, [o["b0"], o["b1"]]) if alias == "op0" else (op0, [o["a0"], o["a1"]])
    untouched([other], [blocks])


@functools.lru_cache(maxsize=None)
def expected_accumulate(logN, logQ, level, npoly, square, relin, sout):
    mods, Pk = chain(logN, logQ)
    o = operands(logN, logQ, level, npoly)
    scales = []

    def one(k):
        b = [o["a0"][k], o["a1"][k]] if square else [o["b0"][k], o["b1"][k]]
        acc = [o["z0"][k], o["z1"][k], o["z2"][k]][:2 if relin else 3]
        out, sc, c2 = gr.mul_relin_then_add(mods[:level + 1], T, [o["a0"][k], o["a1"][k]], S0, b, S0 if square else S1, acc, sout, relin)
        scales.append(sc)
        if relin:
            cx = Ctx._cache[(logN, logQ)]
            return br.relinearize(1 << logN, mods, Pk, level, out + [c2], cx.evkQ, cx.evkP)
        return out
    return per_poly(one, npoly), scales[0]


@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
@pytest.mark.parametrize("square", [False, True])
@pytest.mark.parametrize("matched", [True, False])
def test_mul_then_add(rh, logN, logQ, level, npoly, square, matched):
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    target = (S0 * S0 if square else S0 * S1) % T
    sout = target if matched else 7                                   # 7: r0 != 1 and r1 != 1
    r0, r1, _ = gr.match_scales_binary(T, target, sout)
    assert (r0, r1) == (1, 1) if matched else (r0 != 1 and r1 != 1)
    op0, op1 = ct(rh, c, level, [o["a0"], o["a1"]], S0), ct(rh, c, level, [o["b0"], o["b1"]], S1)
    acc = ct(rh, c, level, [o["z0"], o["z1"], o["z2"]], sout)
    c.ev.MulThenAdd(op0, op0 if square else op1, acc)
    want, sc = expected_accumulate(logN, logQ, level, npoly, square, False, sout)
    assert sc == sout * r1 % T
    check(acc, want, sc)
    untouched([op0, op1], [[o["a0"], o["a1"]], [o["b0"], o["b1"]]])


@pytest.mark.parametrize("logN,logQ,level,npoly", TOP)
@pytest.mark.parametrize("matched", [True, False])
def test_mul_relin_then_add(rh, logN, logQ, level, npoly, matched):
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    sout = S0 * S1 % T if matched else 7
    op0, op1 = ct(rh, c, level, [o["a0"], o["a1"]], S0), ct(rh, c, level, [o["b0"], o["b1"]], S1)
    acc = ct(rh, c, level, [o["z0"], o["z1"]], sout)
    c.ev.MulRelinThenAdd(op0, op1, acc)
    want, sc = expected_accumulate(logN, logQ, level, npoly, False, True, sout)
    check(acc, want, sc)
    untouched([op0, op1], [[o["a0"], o["a1"]], [o["b0"], o["b1"]]])
    with pytest.raises(rh.RingHipError, match="opOut must be different from op0 and op1"):
        c.ev.MulRelinThenAdd(op0, op1, op0)


@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
@pytest.mark.parametrize("degree", [1, 2])
def test_plaintext_times_ciphertext(rh, logN, logQ, level, npoly, degree):
    c = Ctx(rh, logN, logQ)
    mods = c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)
    blocks = [o["a0"], o["a1"], o["b0"]][:degree + 1]
    accb = [o["z0"], o["z1"], o["z2"]]                               # a degree-2 accumulator: with degree 1, component 2 is only scaled
    op0, pt = ct(rh, c, level, blocks, S0), ct(rh, c, level, [o["pt"]], S1)
    want = per_poly(lambda k: gr.tensor_standard(mods, T, [b[k] for b in blocks], S0, [o["pt"][k]], S1)[0], npoly)
    check(c.ev.MulNew(op0, pt), want, S0 * S1 % T)
    check(c.ev.MulRelinNew(op0, pt), want, S0 * S1 % T)              # MulRelin of a plaintext is Mul (:622-625)
    for sout in (S0 * S1 % T, 7):
        acc = ct(rh, c, level, accb, sout)
        c.ev.MulRelinThenAdd(op0, pt, acc)                           # -> MulThenAdd (:1267-1268)
        res = [gr.mul_relin_then_add(mods, T, [b[k] for b in blocks], S0, [o["pt"][k]], S1, [z[k] for z in accb], sout, False) for k in range(npoly)]
        check(acc, [np.stack([r[0][j] for r in res]) for j in range(3)], res[0][1])
    untouched([op0, pt], [blocks, [o["pt"]]])


@pytest.mark.parametrize("logN,logQ,level,npoly", SHAPES)
@pytest.mark.parametrize("sub", [False, True])
def test_add_sub(rh, logN, logQ, level, npoly, sub):
    c = Ctx(rh, logN, logQ)
    mods = c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)
    f = c.ev.SubNew if sub else c.ev.AddNew
    d1, d2 = [o["a0"], o["a1"]], [o["b0"], o["b1"], o["z2"]]
    for x, y in ((d1, [o["b0"], o["b1"]]), (d1, d2), (d2, d1)):       # degrees 1 + 1, 1 + 2, 2 + 1
        for sx, sy in ((S0, S0), (S0, S1)):                          # equal scales, different scales
            a, b = ct(rh, c, level, x, sx), ct(rh, c, level, y, sy)
            res = [gr.add_sub(mods, T, [p[k] for p in x], sx, [p[k] for p in y], sy, sub) for k in range(npoly)]
            check(f(a, b), [np.stack([r[0][j] for r in res]) for j in range(len(res[0][0]))], res[0][1])
            untouched([a, b], [x, y])
    a, b = ct(rh, c, level, d1, S0), ct(rh, c, level, [o["b0"], o["b1"]], S1)
    (c.ev.Sub if sub else c.ev.Add)(a, b, a)                         # in place on op0
    res = [gr.add_sub(mods, T, [p[k] for p in d1], S0, [o["b0"][k], o["b1"][k]], S1, sub) for k in range(npoly)]
    check(a, [np.stack([r[0][j] for r in res]) for j in range(2)], res[0][1])
    with pytest.raises(rh.RingHipError, match="opOut is op1 and the scales differ"):
        (c.ev.Sub if sub else c.ev.Add)(a, b, b)


@pytest.mark.parametrize("logN,logQ,level,npoly", [SHAPES[0], SHAPES[3], SHAPES[5]])
@pytest.mark.parametrize("v", [5, T - 2, T // 2 + 1])                 # positive, and above T/2 (centred to a negative scalar)
def test_int_scalars(rh, logN, logQ, level, npoly, v):
    c = Ctx(rh, logN, logQ)
    mods = c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)
    blocks = [o["a0"], o["a1"], o["b0"]]
    op0 = ct(rh, c, level, blocks, S0)
    stack = lambda res: [np.stack([r[j] for r in res]) for j in range(3)]
    check(c.ev.AddNew(op0, v), stack([gr.add_scalar(mods, T, [b[k] for b in blocks], S0, v)[0] for k in range(npoly)]), S0)
    check(c.ev.SubNew(op0, v), stack([gr.add_scalar(mods, T, [b[k] for b in blocks], S0, -v)[0] for k in range(npoly)]), S0)
    mul = stack([gr.mul_scalar_int(mods, T, [b[k] for b in blocks], S0, v)[0] for k in range(npoly)])
    check(c.ev.MulNew(op0, v), mul, S0)
    check(c.ev.MulRelinNew(op0, v), mul, S0)
    acc = ct(rh, c, level, [o["z0"], o["z1"], o["z2"]], S0)
    c.ev.MulThenAdd(op0, v, acc)                                     # equal scales: acc += op0 * centred v (:1162-1194)
    vc = gr.center_t(v, T)
    want = [np.stack([np.stack([(blocks[j][k, i].astype(object) * vc + o["z%d" % j][k, i].astype(object)) % q for i, q in enumerate(mods)])
                      for k in range(npoly)]).astype(np.uint64) for j in range(3)]
    check(acc, want, S0)
    untouched([op0], [blocks])


@pytest.mark.parametrize("logN,logQ,level,npoly", [s for s in SHAPES if s[2] > 0])
def test_rescale_and_match_scales(rh, logN, logQ, level, npoly):
    c = Ctx(rh, logN, logQ)
    mods = c.Q[:level + 1]
    o = operands(logN, logQ, level, npoly)
    for blocks in ([o["a0"], o["a1"]], [o["a0"], o["a1"], o["b0"]]):  # degree 1 and degree 2
        op0 = ct(rh, c, level, blocks, S0)
        res = [gr.rescale(c.N, mods, T, [b[k] for b in blocks], S0) for k in range(npoly)]
        want = [np.stack([r[0][j] for r in res]) for j in range(len(blocks))]
        assert res[0][1] == S0 * pow(mods[-1], -1, T) % T
        low = c.ev.RescaleNew(op0)                                   # allocated one level down
        assert low.Level() == level - 1
        check(low, want, res[0][1])
        same = rh.Ciphertext([c.rq.AtLevel(level).NewPoly(npoly) for _ in blocks], is_ntt=True)
        c.ev.Rescale(op0, same)                                      # allocated at op0's level: limbs 0 .. level-1 hold the result
        for j, w in enumerate(want):
            assert np.array_equal(same.Value[j].numpy()[:, :level], w)
        assert same.Scale == res[0][1]
        untouched([op0], [blocks])
    a, b = ct(rh, c, level, [o["a0"], o["a1"]], S0), ct(rh, c, level, [o["b0"], o["b1"], o["z2"]], S1)
    c.ev.MatchScalesAndLevel(a, b)
    res = [gr.match_scales_and_level(mods, T, [o["a0"][k], o["a1"][k]], S0, [o["b0"][k], o["b1"][k], o["z2"][k]], S1) for k in range(npoly)]
    check(a, [np.stack([r[0][j] for r in res]) for j in range(2)], res[0][1])
    check(b, [np.stack([r[2][j] for r in res]) for j in range(3)], res[0][3])
    assert a.Scale == b.Scale


def test_composed_sequence_gives_the_same_bits(rh):
    # fused=False issues the reference's own Ring calls: one shape per kernel (tensor overwrite / accumulate, plaintext, axpby)
    logN, logQ, level, npoly = SHAPES[3]
    c = Ctx(rh, logN, logQ)
    o = operands(logN, logQ, level, npoly)
    mk = lambda names, s: ct(rh, c, level, [o[n] for n in names], s)
    got = []
    for ev in (c.ev, c.composed):
        r = []
        op0, op1, pt = mk(("a0", "a1"), S0), mk(("b0", "b1"), S1), mk(("pt",), S1)
        r.append(ev.MulNew(op0, op1)); r.append(ev.MulNew(op0, op0)); r.append(ev.MulRelinNew(op0, op1))
        for sout in (S0 * S1 % T, 7):
            acc = mk(("z0", "z1", "z2"), sout); ev.MulThenAdd(op0, op1, acc); r.append(acc)
            acc = mk(("z0", "z1"), sout); ev.MulRelinThenAdd(op0, op1, acc); r.append(acc)
            acc = mk(("z0", "z1", "z2"), sout); ev.MulRelinThenAdd(op0, op1, acc); r.append(acc)     # a degree-2 accumulator with relin (:1311)
            acc = mk(("z0", "z1", "z2"), sout); ev.MulThenAdd(op0, pt, acc); r.append(acc)
        r.append(ev.MulNew(mk(("a0", "a1", "b0"), S0), pt))
        r.append(ev.AddNew(op0, op1)); r.append(ev.SubNew(op0, mk(("b0", "b1", "z2"), S1))); r.append(ev.SubNew(mk(("b0", "b1", "z2"), S1), op0))
        a, b = mk(("a0", "a1"), S0), mk(("b0", "b1"), S1)
        ev.MatchScalesAndLevel(a, b); r += [a, b]
        got.append(r)
    assert len(got[0]) == len(got[1])
    for x, y in zip(*got):
        assert x.Scale == y.Scale and x.Degree() == y.Degree()
        for u, v in zip(x.Value, y.Value):
            assert np.array_equal(u.numpy(), v.numpy())


def test_scale_invariant_flag(rh):
    # NewEvaluator's flag (:125-134): Mul goes to MulScaleInvariant (:460-465), Rescale does nothing (:1417)
    from test_gpu_bfv import Ctx as BfvCtx
    b = BfvCtx(rh, 10, (55, 45, 45))
    rq = b.rq
    rng = np.random.default_rng(3)
    h = [np.stack([uniform(rng, b.P.Q, b.P.N)]) for _ in range(4)]
    mk = lambda: (rh.Ciphertext([rh.DevicePoly.from_numpy(rq, x) for x in h[:2]], True), rh.Ciphertext([rh.DevicePoly.from_numpy(rq, x) for x in h[2:]], True))
    ev = rh.bgv.Evaluator(rq, b.rm, T, scaleInvariant=True)
    op0, op1 = mk()
    got = ev.MulNew(op0, op1)
    want = b.ev.MulScaleInvariantNew(op0, op1)
    for u, v in zip(got.Value, want.Value):
        assert np.array_equal(u.numpy(), v.numpy())
    assert got.Scale == want.Scale
    before = [v.numpy() for v in got.Value]
    ev.Rescale(got, got)
    assert ev.RescaleNew(got) is got and all(np.array_equal(v.numpy(), w) for v, w in zip(got.Value, before))
    std = b.ev.MulNew(op0, op1)                                      # the default evaluator: standard tensoring, even with a ringQMul
    wstd = gr.tensor_standard(b.P.Q, T, [h[0][0], h[1][0]], 1, [h[2][0], h[3][0]], 1)[0]
    for j in range(3):
        assert np.array_equal(std.Value[j].numpy()[0], wstd[j])
    ev.close()


def test_error_paths(rh):
    c = Ctx(rh, 10, (55, 45, 45))
    rq = c.rq
    a = [rq.NewPoly(1) for _ in range(8)]
    x, y = rh.Ciphertext(a[:2], True), rh.Ciphertext(a[2:4], True)
    out2, out1 = rh.Ciphertext(a[4:7], True), rh.Ciphertext(a[4:6], True)
    for f, args in ((c.ev.Add, (x, [1, 2, 3], out1)), (c.ev.Sub, (x, np.arange(4, dtype=np.uint64), out1)), (c.ev.Mul, (x, (1, 2), out1)),
                    (c.ev.MulRelin, (x, [1], out1)), (c.ev.MulThenAdd, (x, [1], out1)), (c.ev.MulRelinThenAdd, (x, [1], out1))):
        with pytest.raises(rh.RingHipError, match="needs the BGV encoder"):
            f(*args)
    low = rh.Ciphertext([rq.AtLevel(1).NewPoly(1), rq.AtLevel(1).NewPoly(1)], True)
    for f, args in ((c.ev.Add, (x, low, out1)), (c.ev.Mul, (x, low, out2)), (c.ev.MulRelin, (x, y, low)), (c.ev.MulThenAdd, (x, low, out2)),
                    (c.ev.MatchScalesAndLevel, (x, low))):
        with pytest.raises(rh.RingHipError, match="operands must sit at the same level"):
            f(*args)
    r0 = rq.AtLevel(0)
    bottom = rh.Ciphertext([r0.NewPoly(1), r0.NewPoly(1)], True)
    with pytest.raises(rh.RingHipError, match="already at level 0"):
        c.ev.Rescale(bottom, bottom)
    with pytest.raises(rh.RingHipError, match="already at level 0"):
        c.ev.RescaleNew(bottom)
    no_key = rh.bgv.Evaluator(rq, None, T, ringP=c.rp)
    with pytest.raises(rh.RingHipError, match="relinearization key is missing"):
        no_key.MulRelin(x, y, out1)
    with pytest.raises(rh.RingHipError, match="relinearization key is missing"):
        no_key.MulRelinThenAdd(x, y, out1)
    for f, args in ((no_key.MulScaleInvariant, (x, y, out2)), (no_key.MulRelinScaleInvariantNew, (x, y)), (no_key.reserve, (1,)), (no_key.QuantizePath, (0,))):
        with pytest.raises(rh.RingHipError, match="built without ringQMul"):
            f(*args)
    no_key.close()
    with pytest.raises(rh.RingHipError, match="opOut must have degree 2"):
        c.ev.Mul(x, y, out1)
    with pytest.raises(rh.RingHipError, match="opOut must have degree 1"):
        c.ev.MulRelin(x, y, out2)
    with pytest.raises(rh.RingHipError, match="degree 1 x degree 1 and degree <= 2 x degree 0"):
        c.ev.Mul(out2, y, out2)
    with pytest.raises(rh.RingHipError, match="plaintext modulus t is missing"):
        rh.bgv.Evaluator(rq)
    with pytest.raises(rh.RingHipError, match="a modulus of Q"):
        rh.bgv.Evaluator(rq, None, c.Q[1])
    # the C entry points: negative status and rh_last_error for a level out of range, a bad scalar, conjugate-invariant and 3N rings
    L = rh.lib()
    k = np.zeros(3, dtype=np.uint64)
    kp = k.ctypes.data_as(rh.ringhip.U64P)
    ptrs = [p.ptr for p in a[:7]]
    assert L.rh_bgv_tensor(rq._h, 3, *ptrs, 1, kp, None, 0) == -1 and b"level 3 out of range" in L.rh_last_error()
    assert L.rh_bgv_tensor(rq._h, 2, *ptrs, 1, kp, None, 3) == -1 and b"accumulate must be" in L.rh_last_error()
    assert L.rh_bgv_tensor(rq._h, 2, *ptrs, 1, kp, kp, 0) == -1 and b"without accumulate" in L.rh_last_error()
    big = np.array([c.Q[0], 0, 0], dtype=np.uint64)
    assert L.rh_bgv_axpby(rq._h, 2, ptrs[0], None, ptrs[1], 1, big.ctypes.data_as(rh.ringhip.U64P), None, 0) == -1 and b"not below its modulus" in L.rh_last_error()
    assert L.rh_bgv_mul_plain(rq._h, 2, ptrs[0], None, ptrs[1], ptrs[2], ptrs[3], None, ptrs[4], 1, kp, None, 0) == -1 and b"component 2 needs component 1" in L.rh_last_error()
    from conftest import QI60
    ci = rh.Ring(c.N, QI60[:2], kind=rh.ConjugateInvariant)
    assert L.rh_bgv_tensor(ci._h, 1, *ptrs, 1, kp, None, 0) == -1 and b"standard ring" in L.rh_last_error()
    assert L.rh_bgv_axpby(ci._h, 1, ptrs[0], None, ptrs[1], 1, kp, None, 0) == -1 and b"standard ring" in L.rh_last_error()
    ci.close()
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    assert L.rh_bgv_mul_plain(r3._h, 1, ptrs[0], None, None, ptrs[1], ptrs[2], None, None, 1, kp, None, 0) == -1 and b"standard ring" in L.rh_last_error()
    r3.close()

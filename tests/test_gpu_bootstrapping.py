"""GPU: the kernels of csrc/bootstrap.hip and bootstrapping.Evaluator (matrix-fhe-lattigo_amd/bootstrapping.py), bit for bit on whole outputs.

bootstrapping.Evaluator at N = 2^10, LogSlots 1 / 8 / 9, with sparse-secret encapsulation and without, batches of 2 ciphertexts under the real keys
of tests/test_bootstrapping_oracle.py, against tests/bootstrapping_restatement.py: ScaleDown from level 0 and level 1, ModUp without a message scalar (what these settings give) and with one, folded
into the kernel and not, Evaluate end to end (and its output decrypted on the host), the batched EvalMod against two calls, Bootstrap's scale, every
refusal by its text.  The kernels:

rh_ckks_bootstrap_modup against the restatement (tests/bootstrapping_restatement.py, which tests/test_bootstrapping_oracle.py pins to big
integers) and rh_ckks_double_angle against the two Adds it replaces, at three shapes, batches of 3, under every cache policy:
  TAIL  N = 32, 7 | 4 limbs of 61 bits: a row inside one wavefront
  MIX   N = 2^10, the bootstrapping test chain: q0 of 60 bits, then 40, 3 x 39, 8 x 60, 4 x 56 bits | 5 x 61 bits of P -- q0 wider than some
        limbs and narrower than others
  N13   N = 2^13, 6 | 2 limbs of 61 bits: several blocks per row
Operands: uniform residues of q0 with a catalogue planted at known positions of both components: 0, 1, (q0 >> 1) - 1, q0 >> 1, (q0 >> 1) + 1,
q0 - 1 -- the comparisons `>=` (c0, dense c1) and `>` (encapsulated c1) differ exactly at q0 >> 1 -- and, for limbs narrower than q0, q0 - k Qi
for k = 1, 2, 3: negative coefficients whose magnitude the limb divides, the canonical-zero case."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import bootstrapping_restatement as br
from conftest import PI60, QI60, uniform_mod

pytestmark = pytest.mark.gpu
B = 3
POLICIES = (0, 1, 2)
MIX_LOGQ = [60, 40, 39, 39, 39] + [60] * 8 + [56] * 4
MIX_LOGP = [61] * 5


@functools.lru_cache(maxsize=None)
def chain(name):
    from oracle import primes
    if name == "TAIL":
        return 32, tuple(QI60[:7]), tuple(PI60[:4])
    if name == "MIX":
        Q, P = primes.gen_moduli(11, MIX_LOGQ, MIX_LOGP)
        return 1024, tuple(Q), tuple(P)
    Q, P = primes.gen_moduli(14, [61] * 6, [61, 61])
    return 1 << 13, tuple(Q), tuple(P)


def catalogue(q0, mods):
    h = q0 >> 1
    cat = [0, 1, h - 1, h, h + 1, q0 - 1]
    for q in mods:
        if q < (q0 >> 2):
            cat += [q0 - k * q for k in (1, 2, 3)]
    return cat


@functools.lru_cache(maxsize=None)
def operands(name):
    """(c0, c1): (B, N) limb-0 rows, the catalogue planted from position 1 on in c0 and from the last position down in c1, in every poly"""
    N, Q, P = chain(name)
    rng = np.random.default_rng(sum(map(ord, name)))
    c = [np.stack([uniform_mod(rng, Q[0], N) for _ in range(B)]) for _ in range(2)]
    cat = catalogue(Q[0], Q + P)[:N - 2]
    for k in range(B):
        c[0][k, 1:1 + len(cat)] = cat
        c[1][k, N - 1 - len(cat):N - 1] = cat[::-1]
    return c


@functools.lru_cache(maxsize=None)
def expected(name, scalar):
    """the restatement's lifts: c0 and the dense c1 over Q, the encapsulated c1 over Q and P"""
    N, Q, P = chain(name)
    c0, c1 = operands(name)
    lift = lambda c, mods, strict: np.stack([br.lift(c[k], Q[0], mods, strict, scalar) for k in range(B)])
    return lift(c0, Q, False), lift(c1, Q, False), lift(c1, Q, True), lift(c1, P, True)


@pytest.mark.parametrize("nt_streams", POLICIES, ids=["nt-never", "nt-by-size", "nt-always"])
@pytest.mark.parametrize("name", ["TAIL", "MIX", "N13"])
def test_modup_kernel_against_the_restatement(rh, name, nt_streams):
    """dense and encapsulated arms, from level-0 blocks and from full-level blocks, without a scalar and with one folded in;
    the folded scalar against MulScalar after the NTT"""
    N, Q, P = chain(name)
    rq, rp = rh.Ring(N, list(Q)), rh.Ring(N, list(P))
    rq.set_tuning("nt_streams", nt_streams)
    LQ, LP = len(Q), len(P)
    c0, c1 = operands(name)
    scalar = (1 << 33) + 12345
    up = lambda c, ring=rq: rh.DevicePoly.from_numpy(ring.AtLevel(0), c[:, None, :])
    full = lambda ring: ring.NewPoly(B)
    for s in (None, scalar):
        w0, w1, wQ, wP = expected(name, s)
        # dense, out of place
        i0, i1, o0, o1 = up(c0), up(c1), full(rq), full(rq)
        rh.bootstrapping.modup_lift(rq, None, LQ - 1, 0, i0, i1, o0, o1, scalar=s)
        assert np.array_equal(o0.numpy(), w0) and np.array_equal(o1.numpy(), w1), (name, s, "dense")
        # dense, the inputs held in full-level blocks (in_rows = LQ: limb 0 of every poly is read, the other limbs hold garbage)
        junk = np.full((B, LQ, N), 0x5555555555555555, dtype=np.uint64)
        blocks = []
        for c in (c0, c1):
            a = junk.copy()
            a[:, 0] = c
            blocks.append(rh.DevicePoly.from_numpy(rq, a))
        f0, f1 = full(rq), full(rq)
        rh.bootstrapping.modup_lift(rq, None, LQ - 1, 0, blocks[0], blocks[1], f0, f1, scalar=s)
        assert np.array_equal(f0.numpy(), w0) and np.array_equal(f1.numpy(), w1), (name, s, "full-level inputs")
        assert np.array_equal(blocks[1].numpy()[:, 1:], junk[:, 1:]) and np.array_equal(blocks[1].numpy()[:, 0], c1)
        # encapsulated: c1 to every limb of Q and P, its input left alone
        e0, eQ, eP = full(rq), full(rq), full(rp)
        rh.bootstrapping.modup_lift(rq, rp, LQ - 1, LP - 1, i0, i1, e0, c1Q=eQ, c1P=eP, scalar=s)
        assert np.array_equal(e0.numpy(), w0) and np.array_equal(eQ.numpy(), wQ) and np.array_equal(eP.numpy(), wP), (name, s, "encapsulated")
        assert np.array_equal(i1.numpy()[:, 0], c1)
        if s is None:
            plain = (o0, o1, eQ, eP)
        else:                                                                      # :735-750: NTT, then MulScalar
            for folded, unfolded, ring in zip((o0, o1, eQ, eP), plain, (rq, rq, rq, rp)):
                ring.NTT(folded, folded)
                ring.NTT(unfolded, unfolded)
                ring.MulScalar(unfolded, scalar, unfolded)
                assert np.array_equal(folded.numpy(), unfolded.numpy()), (name, "scalar after the NTT")
    rq.close(); rp.close()


def test_modup_refusals(rh):
    N, Q, P = chain("TAIL")
    rq, rp = rh.Ring(N, list(Q)), rh.Ring(N, list(P))
    a, b, o = rq.AtLevel(0).NewPoly(B), rq.AtLevel(0).NewPoly(B), rq.NewPoly(B)
    with pytest.raises(rh.RingHipError, match="two outputs overlap"):
        rh.bootstrapping.modup_lift(rq, None, 6, 0, a, b, o, o)
    o2 = rq.NewPoly(B)
    for args in ((0, 0, a, b, b, a), (0, 0, a, b, a, b), (6, 0, o, o2, o, o2)):                # crossed, and the lift in place at level 0 and at the top
        with pytest.raises(rh.RingHipError, match="an output overlaps an input: the lift is not computed in place"):
            rh.bootstrapping.modup_lift(rq, None, *args)
    with pytest.raises(rh.RingHipError, match="holds levelQ \\+ 1 = 7 limbs"):
        rh.bootstrapping.modup_lift(rq, None, 6, 0, a, b, o, a)
    with pytest.raises(rh.RingHipError, match="output modulo P"):
        rh.bootstrapping.modup_lift(rq, rp, 6, 3, a, b, o, c1Q=rq.NewPoly(B), c1P=rp.AtLevel(1).NewPoly(B))
    rq.close(); rp.close()


@pytest.mark.parametrize("nt_streams", POLICIES, ids=["nt-never", "nt-by-size", "nt-always"])
@pytest.mark.parametrize("name", ["TAIL", "MIX", "N13"])
def test_double_angle_kernel_against_the_two_adds(rh, name, nt_streams):
    """c0 <- 2 c0 + k, c1 <- 2 c1 against Add(res, res, res), Add(res, c, res), at the top level and one below, for a real and a complex
    constant (the two halves of the coefficients take different scalars); residues q - 1 and 0 planted in both halves"""
    N, Q, P = chain(name)
    rq = rh.Ring(N, list(Q))
    rq.set_tuning("nt_streams", nt_streams)
    rng = np.random.default_rng(7)
    for level, c in ((len(Q) - 1, -0.15915494309189535), (len(Q) - 2, complex(0.3, -1.25))):
        mods = Q[:level + 1]
        comps = []
        for _ in range(2):
            a = np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(B)])
            for i, q in enumerate(mods):
                a[:, i, [0, 1, N // 2, N - 1]] = [q - 1, 0, q - 1, (q + 1) // 2]
            comps.append(a)
        got = {}
        for fused in (True, False):
            ev = rh.ckks.Evaluator(rq)
            m = rh.mod1.Evaluator(ev, None, None, fused=fused)
            ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rq.AtLevel(level), a) for a in comps], is_ntt=True)
            ct.Scale = rh.ckks.Scale(1 << 45)
            m._double_angle(ct, c)
            got[fused] = [v.numpy() for v in ct.Value]
            ev.close()
        assert all(np.array_equal(x, y) for x, y in zip(got[True], got[False])), (name, level)
        assert not np.array_equal(got[True][0], comps[0])
    rq.close()


# ---- bootstrapping.Evaluator against the restatement -------------------------------------------------------------------------------------------
import test_bootstrapping_oracle as tbo                                # noqa: E402

NB = 2                                                                 # ciphertexts per batch, different messages under one key
CASES = tbo.CASES


class BtsDev:
    """the rings, the uploaded keys, the Parameters and the Evaluators of one (LogSlots, encapsulation) case of tests/test_bootstrapping_oracle.py"""
    _cache = {}

    def __new__(cls, rh, log_slots, encap):
        if (log_slots, encap) in cls._cache:
            return cls._cache[(log_slots, encap)]
        self = object.__new__(cls)
        s = self.s = tbo.Setting(log_slots, encap)
        k = s.keys()
        self.rq, self.rp = rh.Ring(tbo.N, s.Q), rh.Ring(tbo.N, s.P)
        gc = lambda key, q=self.rq, p=self.rp: rh.rlwe.GadgetCiphertext(q, p, key.Q, key.P)
        d2s = s2d = None
        if encap:
            self.rq0, self.rp0 = rh.Ring(tbo.N, s.Q[:1]), rh.Ring(tbo.N, s.P[:1])
            d2s, s2d = gc(k["d2s"], self.rq0, self.rp0), gc(k["s2d"])
        self.keys = rh.bootstrapping.EvaluationKeys(gc(k["rlk"]), {g: gc(v) for g, v in k["galois"].items()}, d2s, s2d)
        self.params = self.parameters(rh)
        self.ev = {f: rh.bootstrapping.Evaluator(self.params, self.keys, fused=f) for f in (True, False)}
        cls._cache[(log_slots, encap)] = self
        return self

    def literals(self, rh):
        s = self.s
        lit = lambda d: rh.dft.MatrixLiteral(d["Type"], d["LogSlots"], d["LevelQ"], d["LevelP"], d["Levels"], d["Format"], d["Scaling"], d["BitReversed"], d["LogBSGSRatio"])
        return lit(s.s2c), rh.mod1.ParametersLiteral(**s.mod1), lit(s.c2s)

    def parameters(self, rh, **over):
        s2c, m1, c2s = self.literals(rh)
        kw = dict(ringQ=self.rq, ringP=self.rp, ResidualMaxLevel=self.s.residual_level, ResidualDefaultScale=2 ** tbo.LOGSCALE, SlotsToCoeffsParameters=s2c,
                  Mod1ParametersLiteral=m1, CoeffsToSlotsParameters=c2s, EphemeralSecretWeight=32 if self.s.encap else 0)
        kw.update(over)
        return rh.bootstrapping.Parameters(**kw)

    def upload(self, rh, cts, scale, level=None):
        level = cts[0][0].shape[0] - 1 if level is None else level
        out = rh.Ciphertext([rh.DevicePoly.from_numpy(self.rq.AtLevel(level), np.stack([c[i] for c in cts])) for i in range(2)], is_ntt=True)
        out.Scale, out.LogDimensions = rh.ckks.Scale(scale), self.s.log_slots
        return out


def runs(case, level=0):
    return [tbo.restated(case[0], case[1], str(j), level) for j in range(NB)]


def same_batch(ct, want):
    got = [v.numpy() for v in ct.Value]
    return all(np.array_equal(got[i][j], want[j][i]) for i in range(2) for j in range(NB))


@pytest.mark.parametrize("case", CASES, ids=tbo._ids)
def test_scale_down_and_mod_up_against_the_restatement(rh, case):
    """ScaleDown from level 0 and from level 1 (the RescaleTo arm and errScale); ModUp of its output (no message scalar: see the next test); the
    inputs are left as they were"""
    d = BtsDev(rh, *case)
    s = d.s
    r = runs(case)
    ins = [x[1] for x in r]
    ct = d.upload(rh, ins, 2 ** tbo.LOGSCALE)
    for fused in (True, False):
        ev = d.ev[fused]
        down, err = ev.ScaleDown(ct)
        want = [x[3]["ScaleDown"] for x in r]
        assert down.Level() == 0 and down.Scale.Value == want[0][1].v and err.Value == want[0][2].v and down.LogDimensions == s.log_slots
        assert same_batch(down, [w[0] for w in want]) and same_batch(ct, ins)
        before = [v.numpy() for v in down.Value]
        up = ev.ModUp(down)
        want = [x[3]["ModUp"] for x in r]
        assert up.Level() == s.top and up.Scale.Value == want[0][1].v and up.LogDimensions == s.log_slots
        assert same_batch(up, [w[0] for w in want]), (case, fused)
        assert all(np.array_equal(a, v.numpy()) for a, v in zip(before, down.Value))
    # from level 1: a ciphertext at the residual level, scale 2^40
    B = s.circuit()
    vals = [s.values("l1 %d" % j) for j in range(NB)]
    ins1 = [s.encrypt(v, 1, "l1 %d %d" % (j, case[1])) for j, v in enumerate(vals)]
    want = [tbo.br.scale_down(B, c, tbo.cr.Scale(2 ** tbo.LOGSCALE)) for c in ins1]
    down, err = d.ev[True].ScaleDown(d.upload(rh, ins1, 2 ** tbo.LOGSCALE))
    assert down.Level() == 0 and down.Scale.Value == want[0][1].v and err.Value == want[0][2].v and err.Value != 1
    assert same_batch(down, [w[0] for w in want])


@pytest.mark.parametrize("case", CASES, ids=tbo._ids)
def test_mod_up_with_a_message_scalar_against_the_restatement(rh, case):
    """In every setting here ScaleDown from level 0 lands exactly on Q0's power of two over MessageRatio, so ModUp's message scalar (:735-750,
    :781-789) is 1 and not applied.  Here the level-0 ciphertext declares a smaller scale, s = 4 or s = 2.6 (scalar 3, a scale that is no
    integer multiple of the input's): the scalar folded into the kernel and as MulScalar after the NTT, both arms, every word and the scale"""
    d = BtsDev(rh, *case)
    s = d.s
    B_ = s.circuit()
    r = runs(case)
    downs = [x[3]["ScaleDown"] for x in r]
    factor = Fraction(4) if case[0] != 8 else Fraction(13, 5)
    scale = tbo.cr.Scale(downs[0][1].v / factor)
    ratio = (float(2 ** s.mod1["LogScale"]) / float(1 << s.mod1["LogMessageRatio"])) / scale.float64()
    assert ratio > 1 and int(math.floor(ratio + 0.5)) == (4 if case[0] != 8 else 3)           # the scalar branch IS taken
    want = [tbo.br.mod_up(B_, w[0], scale) for w in downs]
    assert want[0][1].v == scale.mul(tbo.cr.Scale(ratio)).v != scale.v
    plain = [x[3]["ModUp"][0] for x in r]
    assert not np.array_equal(want[0][0][0], plain[0][0])
    got = {}
    for fused in (True, False):
        ct = d.upload(rh, [w[0] for w in downs], scale.v)
        up = d.ev[fused].ModUp(ct)
        assert up.Level() == s.top and up.Scale.Value == want[0][1].v and up.LogDimensions == s.log_slots
        assert same_batch(up, [w[0] for w in want]), (case, fused)
        got[fused] = [v.numpy() for v in up.Value]
    assert all(np.array_equal(x, y) for x, y in zip(got[True], got[False]))


@pytest.mark.parametrize("case", CASES, ids=tbo._ids)
def test_evaluate_end_to_end_against_the_restatement(rh, case):
    """Evaluate on a batch: level, scale and every word against the restatement; the device output decrypted on the host to the reference's
    minPrec; Bootstrap's scale"""
    d = BtsDev(rh, *case)
    s = d.s
    r = runs(case)
    ct = d.upload(rh, [x[1] for x in r], 2 ** tbo.LOGSCALE)
    out = d.ev[True].Evaluate(ct)
    want = [x[2] for x in r]
    assert out.Level() == s.residual_level == d.ev[True].OutputLevel() and out.Scale.Value == want[0][1].v and out.Degree() == 1
    assert same_batch(out, [w[0] for w in want]), case
    got = [v.numpy() for v in out.Value]
    for j in range(NB):
        re_, im_ = tbo.avg_log2_prec(r[j][0], s.decrypt([got[0][j], got[1][j]], out.Scale.Float64()))
        assert min(re_, im_) >= tbo.MIN_PREC, (case, j, re_, im_)
    assert d.ev[True].Depth() == s.top - s.residual_level and d.ev[True].MinimumInputLevel() == 1
    if case == CASES[0]:
        out2 = d.ev[False].Bootstrap(ct)
        assert out2.Scale.Value == 2 ** tbo.LOGSCALE and same_batch(out2, [w[0] for w in want])


@pytest.mark.parametrize("encap", [True, False], ids=["encapsulated", "dense"])
def test_batched_eval_mod_against_two_calls(rh, encap):
    """full packing: EvalMod on ctReal and ctImag as one batch of 2 npoly ciphertexts against two calls, and both against the restatement"""
    case = (tbo.LOGN - 1, encap)
    d = BtsDev(rh, *case)
    r = runs(case)
    ev = d.ev[True]
    c2s = [x[3]["CoeffsToSlots"] for x in r]
    re, rs, im, ims = [c[0][0] for c in c2s], c2s[0][0][1], [c[1][0] for c in c2s], c2s[0][1][1]
    mk = lambda cts, sc: d.upload(rh, cts, sc.v)
    a, b = ev._eval_mod_pair(mk(re, rs), mk(im, ims))
    a2, b2 = ev.EvalMod(mk(re, rs)), ev.EvalMod(mk(im, ims))
    want = [x[3]["EvalMod"] for x in r]
    for got, two, k in ((a, a2, 0), (b, b2, 1)):
        assert got.Level() == two.Level() == d.s.s2c_level and got.Scale.Value == two.Scale.Value == 2 ** tbo.LOGSCALE
        assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(got.Value, two.Value))
        assert same_batch(got, [w[k][0] for w in want])


def test_bootstrapping_refusals(rh):
    d = BtsDev(rh, 8, True)
    bts, E = rh.bootstrapping, rh.RingHipError
    new = lambda keys=d.keys, **over: bts.Evaluator(d.parameters(rh, **over), keys)
    with pytest.raises(E, match="IterationsParameters \\(META-BTS"):
        new(IterationsParameters={"BootstrappingPrecision": [25, 25], "ReservedPrimeBitSize": 28})
    with pytest.raises(E, match="PREC128"):
        new(PrecisionMode=bts.PREC128)
    with pytest.raises(E, match="conjugate-invariant residual parameters \\(EvaluateConjugateInvariant"):
        new(ResidualRingType=rh.ConjugateInvariant)
    with pytest.raises(E, match="cannot EvaluateConjugateInvariant"):
        d.ev[True].EvaluateConjugateInvariant(None)
    with pytest.raises(E, match="ResidualParameters.N = 512 != BootstrappingParameters.N = 1024: the ring-degree switch"):
        new(ResidualN=512)
    for order, name in ((bts.DecodeThenModUp, "DecodeThenModUp"), (bts.Custom, "Custom")):
        with pytest.raises(E, match="CircuitOrder %s is not built" % name):
            new(CircuitOrder=order)
    with pytest.raises(E, match="invalid CircuitOrder value"):
        new(CircuitOrder=7)
    s2c, m1, c2s = d.literals(rh)
    sin = rh.mod1.ParametersLiteral(**dict(d.s.mod1, Mod1Type=rh.mod1.SinContinuous))
    with pytest.raises(E, match="cannot use double angle formula for Mod1Type = Sin -> must use Mod1Type = Cos"):
        new(Mod1ParametersLiteral=sin)
    with pytest.raises(E, match="uses a minimum degree of 2\\*\\(K-1\\) but EvalMod degree is smaller"):
        new(Mod1ParametersLiteral=rh.mod1.ParametersLiteral(**dict(d.s.mod1, Mod1Degree=29)))
    with pytest.raises(E, match="starting level and depth of CoeffsToSlotsParameters inconsistent"):
        new(Mod1ParametersLiteral=rh.mod1.ParametersLiteral(**dict(d.s.mod1, LevelQ=d.s.mod1_level - 1)))
    with pytest.raises(E, match="starting level and depth of Mod1ParametersLiteral inconsistent"):
        new(SlotsToCoeffsParameters=rh.dft.MatrixLiteral(s2c.Type, s2c.LogSlots, s2c.LevelQ - 1, s2c.LevelP, s2c.Levels, s2c.Format, None, False, 1))
    k = d.keys
    with pytest.raises(E, match="RelinearizationKey is nil"):
        new(bts.EvaluationKeys(None, k.galois_keys, k.EvkDenseToSparse, k.EvkSparseToDense))
    g = 2 * tbo.N - 1
    with pytest.raises(E, match="GaloisKey\\[%d\\] is nil" % g):
        new(bts.EvaluationKeys(k.rlk, {a: b for a, b in k.galois_keys.items() if a != g}, k.EvkDenseToSparse, k.EvkSparseToDense))
    with pytest.raises(E, match="rlwe.EvaluationKey key dense to sparse is nil"):
        new(bts.EvaluationKeys(k.rlk, k.galois_keys, None, k.EvkSparseToDense))
    with pytest.raises(E, match="rlwe.EvaluationKey key sparse to dense is nil"):
        new(bts.EvaluationKeys(k.rlk, k.galois_keys, k.EvkDenseToSparse, None))
    # a ciphertext packed more sparsely than the bootstrapping: BootstrapMany's pack / unpack
    r = runs((8, True))
    ct = d.upload(rh, [x[1] for x in r], 2 ** tbo.LOGSCALE)
    ct.LogDimensions = 5
    for call in (d.ev[True].Evaluate, d.ev[True].Bootstrap):
        with pytest.raises(E, match="LogSlots = 5, the bootstrapping 8: the pack / unpack of sparse ciphertexts"):
            call(ct)
    # what the evaluators underneath refuse comes through: a scale too large for ScaleDown, a ciphertext above level 0 for ModUp
    ct.LogDimensions = 8
    ct.Scale = rh.ckks.Scale(2 ** 59)
    with pytest.raises(E, match="initial Q/Scale = .* < 0.5\\*Q\\[0\\]/MessageRatio"):
        d.ev[True].Evaluate(ct)
    with pytest.raises(E, match="cannot ModUp: the input must be a degree-1 ciphertext at level 0"):
        d.ev[True].ModUp(d.upload(rh, [tbo.Setting(8, True).encrypt(r[0][0], 1, "x")] * NB, 2 ** tbo.LOGSCALE))
    assert [g for g in d.params.GaloisElements() if g != 1] == d.s.galois_elements()
    assert (d.params.LogMaxSlots(), d.params.Depth()) == (8, 3 + 8 + 4)

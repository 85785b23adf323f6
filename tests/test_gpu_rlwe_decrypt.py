"""GPU: every device path that consumes an evaluation key, run on REAL keys (tests/rlwe_restatement.py) and pinned twice: bit for bit, as whole
arrays, to the oracle composition that tests/test_rlwe_oracle.py pins to decryption on the CPU, and by decrypting the device output itself on
the host -- within the reference's noise bound (core/rlwe/rlwe_test.go:703, :809, :925-929), or exactly for the external product
(core/rgsw/rgsw_test.go:98-112).  Only shapes that pass in tests/test_rlwe_oracle.py are used, with its keys and ciphertexts.

Shapes: N = 32 (TAIL, 7 | 4 limbs: a row inside one wavefront, a last digit of 3 limbs), N = 2^10 with the reference's own chain (REF: 46- and
35-bit limbs against 50-bit P) and N = 2^13 with the 61-bit chain at LevelP = 1 (Q61N13: two-pass transforms, more than one block per limb), each
with one lower-level use of its top-level key.  Batches hold 3 polys with different messages under one key: a ragged grid tail."""
import functools
import random

import numpy as np
import pytest

import ckks_restatement as cr
import rlwe_restatement as rr
import test_rlwe_oracle as t

pytestmark = pytest.mark.gpu
B = 3
_ids = t._ids


class Device:
    """the rings, the evaluator and the uploaded keys of one (chain, setting)"""

    def __init__(self, rh, name, setting, evaluator=None):
        self.rh, self.name, self.setting = rh, name, setting
        self.N, self.Q, P, self.levels = t.chain(name)
        self.P = P[:setting[1]]
        self.rq = rh.Ring(self.N, list(self.Q))
        self.rp = rh.Ring(self.N, list(self.P)) if self.P else None
        self.ev = (evaluator or rh.rlwe.Evaluator)(self.rq, self.rp)

    def gadget(self, k):
        return self.rh.rlwe.GadgetCiphertext(self.rq, self.rp, k.Q, k.P, BaseTwoDecomposition=k.pw2, digits_per_limb=k.digits_per_limb)

    def poly(self, level, arrs):
        return self.rh.DevicePoly.from_numpy(self.rq.AtLevel(level), np.stack(arrs))

    def ct(self, level, cts, is_ntt=True):
        """a batch: component c of every ciphertext of `cts` in one block"""
        return self.rh.Ciphertext([self.poly(level, [c[i] for c in cts]) for i in range(len(cts[0]))], is_ntt=is_ntt)

    def new(self, level, degree=1, is_ntt=True):
        rl = self.rq.AtLevel(level)
        return self.rh.Ciphertext([rl.NewPoly(B) for _ in range(degree + 1)], is_ntt=is_ntt)

    def close(self):
        self.ev.close(); self.rq.close()
        if self.rp is not None:
            self.rp.close()


def host(ct):
    """a device batch as B host ciphertexts"""
    vals = [v.numpy() for v in ct.Value]
    return [[v[k] for v in vals] for k in range(B)]


def same(got, want):
    """whole-array, bit-for-bit equality of B host ciphertexts with their oracle values"""
    return all(np.array_equal(np.stack(g), np.stack(w)) for g, w in zip(got, want))


@functools.lru_cache(maxsize=None)
def switch_batch(name, setting, level):
    """B uniform polys and their oracle gadget products with the sk -> skOut key (poly 0: the CPU file's own case)"""
    N, Q, P, _ = t.chain(name)
    a = [t.switch_case(name, setting, level)[0]] + [rr.uniform_poly(random.Random("a %s %d %d" % (name, level, k)), N, Q[:level + 1]) for k in range(1, B)]
    k = t.key(name, setting, "switch")
    return a, [rr.gadget_product(N, Q, P[:setting[1]], level, x, k) for x in a]


@functools.lru_cache(maxsize=None)
def fresh_batch(name, level, tag, size=1 << 30):
    return [t.fresh(name, "%s%d" % (tag, k), level, size) for k in range(B)]


GP_SHAPES = [("TAIL", (0, 4)), ("TAIL", (0, 1)), ("TAIL", (16, 1)), ("REF", (0, 2)), ("REF", (16, 1)), ("REF", (2, 0)), ("REF", (0, 1)), ("Q61N13", (0, 2))]
MULTI_P = [s for s in GP_SHAPES if s[1][1] >= 2]


@pytest.mark.parametrize("shape", GP_SHAPES, ids=_ids)
def test_gadget_product_decrypts(rh, oracle, shape):
    """GadgetProduct, and with more than one P its other forms -- GadgetProductThenAdd, GadgetProductLazy + ModDown, DecomposeNTT +
    GadgetProductHoisted -- with a top-level key at the top level and one level below"""
    name, setting = shape
    d = Device(rh, name, setting)
    gct = d.gadget(t.key(name, setting, "switch"))
    for level in d.levels[:2]:
        a, want = switch_batch(name, setting, level)
        mods = d.Q[:level + 1]
        cx = d.poly(level, a)
        out = d.new(level)
        d.ev.GadgetProduct(level, cx, gct, out)
        got = host(out)
        assert same(got, want), (name, setting, level)
        for k in range(B):
            err = t.switch_error(name, setting, level, a[k], got[k])
            print("MEASURED gpu/keyswitch %s %s level=%d poly=%d  %.2f [%.2f]" % (name, setting, level, k, err, t.bound(d.N, setting[0])))
            assert err <= t.bound(d.N, setting[0])
        if setting[1] < 2:
            continue
        levelP = setting[1] - 1
        adds = [rr.uniform_poly(random.Random("add %s %d" % (name, k)), d.N, mods) for k in range(B)]
        add0 = d.poly(level, adds)
        out2 = d.new(level)
        d.ev.GadgetProductThenAdd(level, cx, gct, add0, None, out2)
        assert same(host(out2), [[rr._add(adds[k], want[k][0], mods), want[k][1]] for k in range(B)])
        lazy = rh.rlwe.ElementQP.alloc(d.rq, d.rp, B, level, levelP)
        d.ev.GadgetProductLazy(level, cx, gct, lazy)
        out3 = d.new(level)
        d.ev.ModDown(level, levelP, lazy, out3)
        assert same(host(out3), want)
        dec = d.ev.DecomposeNTT(level, levelP, cx, True)
        out4 = d.new(level)
        d.ev.GadgetProductHoisted(level, dec, gct, out4)
        assert same(host(out4), want)
        assert np.array_equal(cx.numpy(), np.stack(a))                  # the input is left alone
    d.close()


@pytest.mark.parametrize("shape", MULTI_P, ids=_ids)
def test_apply_evaluation_key_and_automorphisms_decrypt(rh, oracle, shape):
    """ApplyEvaluationKey (sk -> skOut), Automorphism and AutomorphismHoisted (5, 5^-1 and 2N - 1) on batches of 3 encryptions"""
    name, setting = shape
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    sk, sk_out = t.secrets(name)
    sw = t.key(name, setting, "switch")
    gsw = d.gadget(sw)
    gs = [5, pow(5, -1, 2 * N), 2 * N - 1]
    gks = {g: t.key(name, setting, "galois", g) for g in gs}
    d.ev.galois_keys = {g: d.gadget(k) for g, k in gks.items()}
    for level in d.levels[:2]:
        batch = fresh_batch(name, level, "auto")
        cts = [c for _, c, _ in batch]
        Ql = rr.prod(Q[:level + 1])
        ct = d.ct(level, cts)
        out = d.new(level)
        d.ev.ApplyEvaluationKey(ct, gsw, out)
        got = host(out)
        assert same(got, [rr.apply_evaluation_key(N, Q, P, c, sw) for c in cts])
        for k in range(B):
            err = rr.log2_std(rr.centered_diff(rr.phase(got[k], sk_out, Q), batch[k][0], Ql))
            assert err <= t.bound(N, 0), (level, k, err)
        dec = d.ev.DecomposeNTT(level, setting[1] - 1, ct.Value[1], True)
        for g in (gs if level == d.levels[0] else gs[:1]):
            want = [rr.automorphism(N, Q, P, c, gks[g], g) for c in cts]
            o1, o2 = d.new(level), d.new(level)
            d.ev.Automorphism(ct, g, o1)
            d.ev.AutomorphismHoisted(level, ct, dec, g, o2)
            got = host(o1)
            assert same(got, want), (level, g)
            assert same(host(o2), want), (level, g)
            for k in range(B):
                err = t.auto_error(name, level, got[k], batch[k][0], g)
                print("MEASURED gpu/automorphism %s level=%d g=%d poly=%d  %.2f [%.2f]" % (name, level, g, k, err, t.bound(N, 0, level)))
                assert err <= t.bound(N, 0, level)
        assert same(host(ct), cts)                                      # the inputs are left alone
    d.close()


@functools.lru_cache(maxsize=None)
def tensor_batch(name, level):
    """B pairs of encryptions, their exact tensors and the products (m0 + e0)(m1 + e1)"""
    N, Q, _, _ = t.chain(name)
    x, y = fresh_batch(name, level, "tx", 1 << 20), fresh_batch(name, level, "ty", 1 << 20)
    out = []
    for (m0, c0, e0), (m1, c1, e1) in zip(x, y):
        want = rr.negacyclic_mul([a + b for a, b in zip(m0, e0)], [a + b for a, b in zip(m1, e1)])
        out.append((c0, c1, cr.mul_relin(list(Q[:level + 1]), c0, cr.Scale(1), c1, cr.Scale(1))[0], want))
    return out


@pytest.mark.parametrize("shape", MULTI_P, ids=_ids)
def test_relinearize_decrypts(rh, oracle, shape):
    name, setting = shape
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    rlk = t.key(name, setting, "relin")
    grlk = d.gadget(rlk)
    for level in d.levels[:2]:
        batch = tensor_batch(name, level)
        c2 = [c for _, _, c, _ in batch]
        out = d.new(level)
        d.ev.Relinearize(d.ct(level, c2), out, rlk=grlk)
        got = host(out)
        assert same(got, [rr.relinearize(N, Q, P, c, rlk) for c in c2])
        for k in range(B):
            err = rr.log2_std(rr.centered_diff(rr.phase(got[k], t.secrets(name)[0], Q), batch[k][3], rr.prod(Q[:level + 1])))
            assert err <= t.bound(N, 0), (level, k, err)
    d.close()


RGSW_SHAPES = [("TAIL", (0, 4)), ("TAIL", (16, 1)), ("RGSW", (0, 2)), ("REF", (0, 2)), ("REF", (16, 1)), ("REF", (0, 1)), ("REF", (16, 0)), ("Q61N13", (0, 2))]
assert set(RGSW_SHAPES) <= set(t.RGSW_SHAPES)


@pytest.mark.parametrize("shape", RGSW_SHAPES, ids=_ids)
def test_external_product_decrypts_to_the_monomials(rh, oracle, shape):
    """rgsw.Evaluator.ExternalProduct, multi-P and single-P with and without a power-of-two decomposition: RGSW(X^3) x RLWE(q0 X^k1) for three k1,
    one of which wraps with a sign, equals the oracle's loop and decrypts to +-X^(3 + k1 mod N) exactly"""
    name, setting = shape
    d = Device(rh, name, setting, evaluator=rh.rgsw.Evaluator)
    N, level = d.N, d.levels[0]
    k0, k1s = 3, (1, N - 2, 5)
    value = t.rgsw(name, setting, k0)
    ctr = rh.rgsw.Ciphertext(d.gadget(value[0]), d.gadget(value[1]))
    cases = [t.rgsw_case(name, setting, k0, k1) for k1 in k1s]
    op0 = d.ct(level, [c for c, _ in cases])
    out = d.new(level)
    d.ev.ExternalProduct(op0, ctr, out)
    got = host(out)
    assert same(got, [list(w) for _, w in cases])
    for k, k1 in enumerate(k1s):
        mono = [0] * N
        mono[k1] = 1
        assert t.decrypt_monomial(name, got[k])[0] == rr.monomial_mul(mono, k0), k1
    d.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape", t.CKKS_SHAPES, ids=_ids)
def test_ckks_evaluator_decrypts(rh, oracle, shape, fused):
    """ckks.Evaluator with a real relinearisation key and real Galois keys: MulRelinNew -> Rescale, RotateNew, ConjugateNew, RotateHoistedNew"""
    name, setting = shape
    N, Q, P, levels = t.chain(name)
    level = levels[0]
    mods = list(Q[:level + 1])
    sk = t.secrets(name)[0]
    rots = (1, -1, 3)
    gs = {k: cr.galois_element(N, k) for k in rots}
    gs[None] = 2 * N - 1
    gks = {g: t.key(name, setting, "galois", g) for g in gs.values()}
    rlk = t.key(name, setting, "relin")
    d = Device(rh, name, setting)
    ev = rh.ckks.Evaluator(d.rq, d.rp, rlk=d.gadget(rlk), galois_keys={g: d.gadget(k) for g, k in gks.items()}, fused=fused)
    # MulRelin -> Rescale
    batch = tensor_batch(name, level)
    ct0, ct1 = d.ct(level, [b[0] for b in batch]), d.ct(level, [b[1] for b in batch])
    ct0.Scale, ct1.Scale = rh.ckks.Scale(t.SA.v), rh.ckks.Scale(t.SB.v)
    prod = ev.MulRelinNew(ct0, ct1)
    res = d.new(level)
    ev.Rescale(prod, res)
    lin, low = [], []
    for c0, c1, _, _ in batch:
        c, sc = cr.mul_relin(mods, c0, t.SA, c1, t.SB)
        lin.append(rr.relinearize(N, Q, P[:setting[1]], c, rlk))
        lw, sc2 = cr.rescale(N, mods, lin[-1], sc)
        low.append(lw)
    got, gotlow = host(prod), [[x[:level] for x in c] for c in host(res)]
    assert same(got, lin) and same(gotlow, low)
    assert prod.Scale.Value == sc.v and res.Scale.Value == sc2.v == cr.Scale(t.SA.v * t.SB.v / mods[-1]).v
    for k in range(B):
        err = rr.log2_std(rr.centered_diff(rr.phase(got[k], sk, Q), batch[k][3], rr.prod(mods)))
        assert err <= t.bound(N, 0), (k, err)
        worst, limit = t.rescale_excess(name, got[k], gotlow[k])
        assert worst <= limit
    # Rotate / Conjugate / RotateHoisted
    msgs = fresh_batch(name, level, "auto")
    cts = [c for _, c, _ in msgs]
    ct = d.ct(level, cts)
    ct.Scale = rh.ckks.Scale(t.SA.v)
    hoisted = ev.RotateHoistedNew(ct, list(rots))
    for k in rots + (None,):
        g = gs[k]
        want = [rr.automorphism(N, Q, P[:setting[1]], c, gks[g], g) for c in cts]
        out = ev.ConjugateNew(ct) if k is None else ev.RotateNew(ct, k)
        got = host(out)
        assert same(got, want), k
        assert out.Scale.Value == t.SA.v
        if k is not None:
            assert ev.GaloisElement(k) == g == pow(5, k, 2 * N)
            assert same(host(hoisted[k]), want), k
        for j in range(B):
            assert t.auto_error(name, level, got[j], msgs[j][0], g) <= t.bound(N, 0, level)
    # by 1, then by -1: the messages again, within twice the bound on the standard deviation
    back = host(ev.RotateNew(ev.RotateNew(ct, 1), -1))
    for j in range(B):
        assert t.auto_error(name, level, back[j], msgs[j][0], 1) <= t.bound(N, 0, level) + 1
    ev.close()
    d.close()

"""GPU: every cache-policy variant of every kernel family at test sizes, bit for bit against the oracle.

Almost every hot kernel exists twice: with the default cache policy and with non-temporal data streams (the generated _NT bodies, the nt
template arms and arguments).  The host takes the second form once a launch's working set passes a threshold (512 MiB; 256 MiB for the key
switch's gap transform), so at test sizes only the first form ever ran, and the pipelined kernels' default-policy forms never ran at all.
The tuning key "nt_streams" forces the choice: 0 default policy everywhere, 1 by working set, 2 non-temporal at every size.  The policy is a
hint: every case here runs under 0, 1 and 2 on one ring and every policy's whole output is compared with the oracle (or, for BGV / BFV, with
the big-integer restatement), never only with another policy's output.  Operands carry a row of all q - 1 and a row that is zero at every
even index; chains are the mixed-width ones of oracle/primes.py."""
import contextlib

import numpy as np
import pytest

from conftest import uniform_mod

pytestmark = pytest.mark.gpu
POLICIES = (0, 1, 2)


@contextlib.contextmanager
def policy(value, *rings):
    """the tuning key on every ring of the case; back to 1 (by working set, the default) whatever happens: the Ctx rings of the BGV / BFV
    files are cached across tests"""
    try:
        for r in rings:
            r.set_tuning("nt_streams", value)
        yield
    finally:
        for r in rings:
            r.set_tuning("nt_streams", 1)


def chain_for(logN, L):
    """L moduli of a mixed-width chain that exists at this degree: WIDE (61, 36, 20 bits) up to 2^13, C45 (55, 45, 45) up to 2^15, B40 (50, 40, 40)"""
    from oracle import primes
    name = "WIDE" if logN <= 13 else "C45" if logN <= 15 else "B40"
    Q, P = primes.chain(name, logN)
    return [int(q) for q in (Q + P)[:L]]


def block(rng, mods, B, N):
    """B polys: poly 0 all q - 1, poly 1 zero at every even index, the others uniform"""
    a = np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(B)])
    a[0] = np.array(mods, dtype=np.uint64)[:, None] - np.uint64(1)
    if B > 1:
        a[1, :, ::2] = 0
    return a


def fwd_all(oracle, a, srs, f=None):
    f = f or oracle.ntt
    return np.stack([np.stack([f(a[k, i], srs[i]) for i in range(a.shape[1])]) for k in range(a.shape[0])])


# ---- transforms: two-pass launches and the one-pass kernels -----------------------------------------------------------------------------
@pytest.mark.parametrize("logN,one_pass", [(12, 0), (12, 1), (13, 0), (14, 0), (15, 0), (16, 0), (13, 1), (14, 1)])
def test_transforms(rh, oracle, logN, one_pass):
    """NTT and INTT, out of place and in place, and through an AtLevel view of polys with more limbs (strided rows).  one_pass = 0: the
    column and tile bodies at S1 = 0 .. 4; one_pass = 1: the whole-row kernels of N = 2^13 / 2^14 and the N = 4096 inverse"""
    N, B, L = 1 << logN, 3, 3
    mods = chain_for(logN, L)
    ring = rh.Ring(N, mods)
    ring.set_tuning("one_pass", one_pass)
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    rng = np.random.default_rng(700 + logN)
    a = block(rng, mods, B, N)
    y = fwd_all(oracle, a, srs)
    yin = y.copy()
    yin[2, :, 1::2] += np.array(mods, dtype=np.uint64)[:, None]          # inverse inputs in [q, 2q)
    view = ring.AtLevel(1)
    for pol in POLICIES:
        with policy(pol, ring):
            p, o = rh.DevicePoly.from_numpy(ring, a), ring.NewPoly(B)
            ring.NTT(p, o)
            assert np.array_equal(o.numpy(), y), ("NTT", pol)
            assert np.array_equal(p.numpy(), a), ("NTT input", pol)
            ring.INTT(rh.DevicePoly.from_numpy(ring, yin), o)
            assert np.array_equal(o.numpy(), a), ("INTT", pol)
            ring.NTT(p, p)
            assert np.array_equal(p.numpy(), y), ("NTT in place", pol)
            ring.INTT(p, p)
            assert np.array_equal(p.numpy(), a), ("INTT in place", pol)
            view.NTT(p, p)                                            # limbs 0, 1 of 3-limb polys
            got = p.numpy()
            assert np.array_equal(got[:, :2], y[:, :2]) and np.array_equal(got[:, 2], a[:, 2]), ("AtLevel NTT", pol)
            view.INTT(p, o)
            assert np.array_equal(o.numpy()[:, :2], a[:, :2]), ("AtLevel INTT", pol)
    ring.close()


# ---- pipelined spans: the policy comes from the key alone (0: the default-policy forms of the fused kernels) ---------------------------
@pytest.mark.parametrize("logN", [13, 14, 15, 16, 17])
def test_pipelined_spans(rh, oracle, logN):
    """10 polys in three blocks, spans of 2 polys (auto_span_rows = 6 at 3 limbs): rh_ring_ntt_many through the block boundaries, one
    10-poly block forward and inverse, Ring.INTTMul and Ring.PolyMul on their pipelined paths.  N = 2^14 .. 2^16 also with the C++ column
    stages inside the fused launches (asm_cols = 0)"""
    N, L = 1 << logN, 3
    mods = chain_for(logN, L)
    ring = rh.Ring(N, mods)
    ring.set_tuning("auto_span_rows", 6)
    ring.set_tuning("one_pass", 0)
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    rng = np.random.default_rng(800 + logN)
    sizes = [5, 1, 4]
    a = block(rng, mods, sum(sizes), N)
    y = fwd_all(oracle, a, srs)
    cuts = np.cumsum([0] + sizes)
    b = a[::-1].copy()
    want_im, want_pm = _products(oracle, rh, a, b, mods, srs, False), _products(oracle, rh, a, b, mods, srs, True)
    for pol, asm_cols in [(p, 1) for p in POLICIES] + [(p, 0) for p in POLICIES if 14 <= logN <= 16]:
        ring.set_tuning("asm_cols", asm_cols)
        with policy(pol, ring):
            ps = [rh.DevicePoly.from_numpy(ring, a[cuts[j]:cuts[j + 1]]) for j in range(3)]
            outs = [ps[0], ring.NewPoly(sizes[1]), ps[2]]              # blocks 0 and 2 in place, block 1 out of place
            ring.NTTMany(list(zip(ps, outs)))
            for j in range(3):
                assert np.array_equal(outs[j].numpy(), y[cuts[j]:cuts[j + 1]]), ("NTTMany", pol, j)
            p, o = rh.DevicePoly.from_numpy(ring, a), ring.NewPoly(10)
            ring.NTT(p, o)
            assert np.array_equal(o.numpy(), y), ("NTT", pol)
            ring.INTT(o, p)
            assert np.array_equal(p.numpy(), a), ("INTT", pol)
            ring.INTT(o, o)
            assert np.array_equal(o.numpy(), a), ("INTT in place", pol)
            ring.INTTMul(rh.DevicePoly.from_numpy(ring, a), rh.DevicePoly.from_numpy(ring, b), o)
            assert np.array_equal(o.numpy(), want_im), ("INTTMul", pol, asm_cols)
            ring.PolyMul(rh.DevicePoly.from_numpy(ring, a), rh.DevicePoly.from_numpy(ring, b), o)       # (its operands are consumed)
            assert np.array_equal(o.numpy(), want_pm), ("PolyMul", pol, asm_cols)
    ring.close()


@pytest.mark.parametrize("logN", [14, 15, 16])
def test_conjugate_invariant_fused_pair(rh, oracle, logN):
    # ntt_ci_fwd_fused_asm / ntt_ci_inv_fused_asm <S, nt>: the fold inside the pipelined column stages
    from oracle import primes
    N, L = 1 << logN, 3
    mods = [int(q) for q in primes.gen_moduli(logN + 2, [50, 40, 40], [])[0]]            # NthRoot = 4N
    ring = rh.Ring(N, mods, kind=rh.ConjugateInvariant)
    ring.set_tuning("auto_span_rows", 6)
    srs = [oracle.SubRingConsts(N, q, nthroot=4 * N) for q in mods]
    rng = np.random.default_rng(900 + logN)
    a = block(rng, mods, 10, N)
    y = fwd_all(oracle, a, srs, oracle.ntt_ci)
    assert np.array_equal(oracle.intt_ci(y[2, 1], srs[1]), a[2, 1])
    for pol in POLICIES:
        with policy(pol, ring):
            p, o = rh.DevicePoly.from_numpy(ring, a), ring.NewPoly(10)
            ring.NTT(p, o)
            assert np.array_equal(o.numpy(), y), ("NTT", pol)
            ring.INTT(o, p)
            assert np.array_equal(p.numpy(), a), ("INTT", pol)
    ring.close()


def _products(oracle, rh, a, b, mods, srs, ntt_first):
    """INTT(MForm(x) . y) per row, x = a, y = b (or their transforms): the values of Ring.INTTMul / Ring.PolyMul"""
    z = np.zeros(a.shape[2], dtype=np.uint64)
    out = np.empty_like(a)
    for k in range(a.shape[0]):
        for j, q in enumerate(mods):
            x, y = (oracle.ntt(a[k, j], srs[j]), oracle.ntt(b[k, j], srs[j])) if ntt_first else (a[k, j], b[k, j])
            m = oracle.vec_op(rh.OPS["MFORM"], x, None, z, 0, 0, q)
            out[k, j] = oracle.intt(oracle.vec_op(rh.OPS["MUL_MONT"], m, y, z, 0, 0, q), srs[j])
    return out


@pytest.mark.parametrize("logN,B,spans", [(12, 2, 0), (13, 2, 0), (14, 2, 0)])
def test_polymul_and_intt_mul(rh, oracle, logN, B, spans):
    """Ring.PolyMul (rh_ring_polymul: ntt_polymul_tile_asm<nt> between nt column stages; with spans, ntt_polymul_fused_asm<S, nt>) and
    Ring.INTTMul (rh_ring_intt_mul); their pipelined paths are in test_pipelined_spans.  The fused product covers 2^13 <= N <= 2^17: at N = 4096 it is refused under every policy."""
    N, L = 1 << logN, 3
    mods = chain_for(logN, L)
    ring = rh.Ring(N, mods)
    if spans:
        ring.set_tuning("auto_span_rows", spans)
    ring.set_tuning("one_pass", 0)
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    rng = np.random.default_rng(1000 + logN + B)
    a, b = block(rng, mods, B, N), block(rng, mods, B, N)[::-1].copy()
    want_im = _products(oracle, rh, a, b, mods, srs, False)
    want_pm = _products(oracle, rh, a, b, mods, srs, True) if logN > 12 else None
    for pol in POLICIES:
        with policy(pol, ring):
            got = ring.NewPoly(B)
            ring.INTTMul(rh.DevicePoly.from_numpy(ring, a), rh.DevicePoly.from_numpy(ring, b), got)
            assert np.array_equal(got.numpy(), want_im), ("INTTMul", pol)
            pa, pb = rh.DevicePoly.from_numpy(ring, a), rh.DevicePoly.from_numpy(ring, b)       # consumed by PolyMul
            if logN == 12:
                with pytest.raises(rh.RingHipError, match="polymul"):
                    ring.PolyMul(pa, pb, got)
                continue
            ring.PolyMul(pa, pb, got)
            assert np.array_equal(got.numpy(), want_pm), ("PolyMul", pol)
    ring.close()


# ---- rescale ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [14, 15, 16])
def test_rescale_ntt_domain(rh, oracle, logN):
    """DivRound / DivFloorByLastModulusNTT on three 40-bit primes (qL + q <= 8q: the hand-scheduled expand body is the one taken, then the
    tile stages fused with the subtract-multiply), against INTT -> coefficient-domain division -> NTT of the oracle"""
    from oracle import primes
    N, B, L = 1 << logN, 2, 3
    mods = [int(q) for q in primes.chain("B40", logN)[0][1:4]]
    assert max(mods) < 2 * min(mods)
    ring = rh.Ring(N, mods)
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    rng = np.random.default_rng(1100 + logN)
    a = block(rng, mods, B, N)
    y = fwd_all(oracle, a, srs)
    want = {r: fwd_all(oracle, np.stack([oracle.div_by_last_modulus_many(a[k], mods, 1, r) for k in range(B)]), srs[:L - 1]) for r in (0, 1)}
    for pol in POLICIES:
        with policy(pol, ring):
            pn = rh.DevicePoly.from_numpy(ring, y)
            for r, f in ((1, ring.DivRoundByLastModulusNTT), (0, ring.DivFloorByLastModulusNTT)):
                po = rh.DevicePoly(ring, B, L - 1)
                f(pn, po)
                assert np.array_equal(po.numpy(), want[r]), (pol, r)
            assert np.array_equal(pn.numpy(), y), ("input", pol)
    ring.close()


# ---- key switch ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN,npoly", [(14, 2), (15, 1), (16, 1)])
def test_gadget_product(rh, oracle, logN, npoly):
    """one gadget product at N = 2^14 (two polys; one at 2^15 and 2^16, for the gap transform's other sizes), Q = 4, P = 2: the pipelined digit transform with its gaps (ks_small_rows = 0) and the
    small-batch launches (default), the paired and the single subtract-multiply with and without the addend, the ModDown"""
    from oracle import compose, primes
    N = 1 << logN
    Q, P = primes.chain("C45" if logN <= 15 else "SPLIT", logN)
    Q, P = [int(q) for q in Q[:4]], [int(p) for p in P[:2]]
    nq, np_ = len(Q), len(P)
    levelQ, levelP = nq - 1, np_ - 1
    beta = (levelQ + levelP + 1) // (levelP + 1)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    be = rh.BasisExtender(rq, rp)
    rng = np.random.default_rng(1200)
    cx, add = block(rng, Q, npoly, N), block(rng, Q, npoly, N)[::-1].copy()
    key = lambda mods: np.stack([np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(2)]) for _ in range(beta)])
    evkQ, evkP = key(Q), key(P)
    want = [compose.gadget_product(N, Q, P, levelQ, levelP, cx[k], evkQ, evkP) for k in range(npoly)]
    ADD = rh.OPS["ADD"]
    wadd = [[np.stack([oracle.vec_op(ADD, want[k][c][i], add[k, i], add[k, i], 0, 0, q) for i, q in enumerate(Q)]) for c in (0, 1)] for k in range(npoly)]
    pcx = rh.DevicePoly.from_numpy(rq, cx)
    dq = rh.DevicePoly.from_numpy(rq, evkQ.reshape(beta * 2, nq, N)); dp = rh.DevicePoly.from_numpy(rp, evkP.reshape(beta * 2, np_, N))
    ev = rh.rlwe.Evaluator(rq, rp)
    gct = rh.rlwe.GadgetCiphertext(rq, rp, evkQ, evkP)
    for knobs in ({"ks_small_rows": 0}, {}, {"ks_small_rows": 0, "pair_submul": 0}):
        for k, v in knobs.items():
            rq.set_tuning(k, v)
        for pol in POLICIES:
            with policy(pol, rq, rp):
                ct0, ct1 = rh.DevicePoly(rq, npoly, nq), rh.DevicePoly(rq, npoly, nq)
                be.GadgetProduct(levelQ, levelP, pcx, dq.ptr, dp.ptr, beta, ct0, ct1)
                a0, a1 = rh.DevicePoly.from_numpy(rq, add), rh.DevicePoly.from_numpy(rq, add)
                be.GadgetProductThenAdd(levelQ, levelP, pcx, dq.ptr, dp.ptr, beta, a0, a1, a0, a1)
                g = (ct0.numpy(), ct1.numpy()); s = (a0.numpy(), a1.numpy())
                for k in range(npoly):
                    for c in (0, 1):
                        assert np.array_equal(g[c][k], want[k][c]), (knobs, pol, k, c)
                        assert np.array_equal(s[c][k], wadd[k][c]), ("then add", knobs, pol, k, c)
                assert np.array_equal(pcx.numpy(), cx)
                # the hoisted form: a caller-visible decomposition (canonical digit blocks: the gap transform without its lazy output)
                dec = ev.DecomposeNTT(levelQ, levelP, pcx, True)
                h = rh.Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=True)
                ev.GadgetProductHoisted(levelQ, dec, gct, h)
                for k in range(npoly):
                    for c in (0, 1):
                        assert np.array_equal(h.Value[c].numpy()[k], want[k][c]), ("hoisted", knobs, pol, k, c)
        rq.set_tuning("ks_small_rows", 512); rq.set_tuning("pair_submul", 1)
    ev.close(); be.close(); rq.close(); rp.close()


# ---- 3N rings --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn2", [13, 14, 15, 16])
def test_3n_transforms(rh, oracle, logn2):
    # ntt3n_layer_asm<S, inverse, nt> (S = 1, 2, 3 at N = 3 * 2^14, 2^15, 2^16) and the sub-ring's transforms (the key is handed on to
    # the sub-ring), both NTT-domain layouts
    from oracle import primes
    from test_oracle_ntt3n import omega_for
    N, B, L = 3 << logn2, 2, 2
    mods = [int(q) for q in primes.gen_moduli_3n(N, [31, 55], [])[0]]
    om = [omega_for(q, N) for q in mods]
    ring = rh.Ring(N, mods, kind=rh.Matrix3N, omega3n=om)
    rng = np.random.default_rng(1300 + logn2)
    a = block(rng, mods, B, N)
    y = np.stack([np.stack([oracle.ntt3n_forward(a[k, i], mods[i], om[i]) for i in range(L)]) for k in range(B)])
    assert np.array_equal(oracle.ntt3n_backward(y[1, 1], mods[1], om[1]), a[1, 1])
    for order in (0, 1):
        ring.set_tuning("ntt3n_block_order", order)
        for pol in POLICIES:
            with policy(pol, ring):
                p = rh.DevicePoly.from_numpy(ring, a)
                ring.NTT(p, p)
                if order:
                    ref = ring.NewPoly(B)
                    ring.NTT3NReorder(p, ref, to_reference=True)
                    got = ref.numpy()
                else:
                    got = p.numpy()
                assert np.array_equal(got, y), ("NTT", order, pol)
                ring.INTT(p, p)
                assert np.array_equal(p.numpy(), a), ("INTT", order, pol)
    ring.close()


# ---- element-wise ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [5, 13])
def test_vec_ops(rh, oracle, logN):
    """all 38 opcodes, the broadcast-row form (the broadcast row keeps the default policy), the halves form, AtLevel strides, an in-place
    call, and rh_ring_tensor_degree1 with both mform_first values"""
    from oracle import primes
    N, B, L = 1 << logN, 3, 3
    mods = [int(q) for q in primes.gen_moduli(logN + 1, [61, 36, 45], [])[0]]
    ring = rh.Ring(N, mods)
    rng = np.random.default_rng(1400 + logN)
    x, y, zz = block(rng, mods, B, N), block(rng, mods, B, N)[::-1].copy(), block(rng, mods, B, N)
    s0 = np.array([int(rng.integers(1, q)) for q in mods], dtype=np.uint64)
    s1 = np.array([int(rng.integers(1, q)) for q in mods], dtype=np.uint64)
    ops = sorted((v, k) for k, v in rh.OPS.items() if k != "COUNT")
    assert len(ops) == 38

    def scal(op):
        if op == "MASK":
            return np.array([7, 13, 0], dtype=np.uint64), np.array([(1 << 20) - 1, 0xffff, (1 << 61) - 1], dtype=np.uint64)
        return s0, s1
    rows = lambda f: np.stack([np.stack([f(k, i, q) for i, q in enumerate(mods)]) for k in range(B)])
    want = {}
    for code, op in ops:
        a0, a1 = scal(op)
        want[op] = rows(lambda k, i, q: oracle.vec_op(code, x[k, i], y[k, i], zz[k, i], a0[i], a1[i], q))
    vec = uniform_mod(rng, min(mods), N)                                  # one row for every (poly, limb)
    MM, MMA = rh.OPS["MUL_MONT"], rh.OPS["MUL_MONT_THEN_ADD_LAZY"]
    want_b = rows(lambda k, i, q: oracle.vec_op(MM, x[k, i], vec, zz[k, i], 0, 0, q))
    want_ba = rows(lambda k, i, q: oracle.vec_op(MMA, x[k, i], vec, zz[k, i], 0, 0, q))
    lo, hi = [int(v) for v in s0], [int(v) for v in s1]
    h = N // 2

    def halves(code, a_lo, a_hi):
        return rows(lambda k, i, q: np.concatenate([oracle.vec_op(code, x[k, i, :h], None, zz[k, i, :h], a_lo[i], 0, q),
                                                    oracle.vec_op(code, x[k, i, h:], None, zz[k, i, h:], a_hi[i], 0, q)]))
    mf = lambda s: [(v << 64) % q for v, q in zip(s, mods)]
    want_h = {"AddDoubleRNSScalar": halves(rh.OPS["ADD_SCALAR"], lo, hi), "SubDoubleRNSScalar": halves(rh.OPS["SUB_SCALAR"], lo, hi),
              "MulDoubleRNSScalar": halves(rh.OPS["MUL_SCALAR_MONT"], mf(lo), mf(hi)),
              "MulDoubleRNSScalarThenAdd": halves(rh.OPS["MUL_SCALAR_MONT_THEN_ADD"], mf(lo), mf(hi))}
    z = np.zeros(N, dtype=np.uint64)
    vop = lambda name, p, r, t, q: oracle.vec_op(rh.OPS[name], p, r, t, 0, 0, q)
    want_t = {}
    for mform_first in (True, False):
        c = [np.empty((B, L, N), dtype=np.uint64) for _ in range(3)]
        for k in range(B):
            for i, q in enumerate(mods):
                m0, m1 = (vop("MFORM", x[k, i], None, z, q), vop("MFORM", y[k, i], None, z, q)) if mform_first else (x[k, i], y[k, i])
                c[0][k, i] = vop("MUL_MONT", m0, zz[k, i], z, q)
                c[2][k, i] = vop("MUL_MONT", m1, x[B - 1 - k, i], z, q)
                c[1][k, i] = vop("MUL_MONT_THEN_ADD", m1, zz[k, i], vop("MUL_MONT", m0, x[B - 1 - k, i], z, q), q)
        want_t[mform_first] = c
    view = ring.AtLevel(1)
    xr = x[::-1].copy()
    for pol in POLICIES:
        with policy(pol, ring):
            px, py = rh.DevicePoly.from_numpy(ring, x), rh.DevicePoly.from_numpy(ring, y)
            for code, op in ops:
                a0, a1 = scal(op)
                pz = rh.DevicePoly.from_numpy(ring, zz)
                ring.vec_op(op, px, py, pz, s0=a0, s1=a1)
                assert np.array_equal(pz.numpy(), want[op]), (op, pol)
                pz.free()
            assert np.array_equal(px.numpy(), x) and np.array_equal(py.numpy(), y), pol
            # the output is the first operand
            pz = rh.DevicePoly.from_numpy(ring, x)
            ring.vec_op("MUL_MONT", pz, py, pz)
            assert np.array_equal(pz.numpy(), want["MUL_MONT"]), ("in place", pol)
            # limbs 0, 1 of 3-limb polys: rows strided by 3, limb 2 untouched
            pz = rh.DevicePoly.from_numpy(ring, zz)
            view.vec_op("MUL_MONT_THEN_ADD", px, py, pz)
            got = pz.numpy()
            assert np.array_equal(got[:, :2], want["MUL_MONT_THEN_ADD"][:, :2]) and np.array_equal(got[:, 2], zz[:, 2]), ("AtLevel", pol)
            # one row for every (poly, limb)
            pv = rh.DevicePoly.from_numpy(ring.AtLevel(0), vec[None, None])
            pz = rh.DevicePoly.from_numpy(ring, zz)
            ring.MulByVectorMontgomery(px, pv, pz)
            assert np.array_equal(pz.numpy(), want_b), ("bcast", pol)
            pz = rh.DevicePoly.from_numpy(ring, zz)
            ring.MulByVectorMontgomeryThenAddLazy(px, pv, pz)
            assert np.array_equal(pz.numpy(), want_ba), ("bcast then add", pol)
            assert np.array_equal(pv.numpy()[0, 0], vec), pol
            pz = rh.DevicePoly.from_numpy(ring, zz)
            view.MulByVectorMontgomery(px, pv, pz)
            got = pz.numpy()
            assert np.array_equal(got[:, :2], want_b[:, :2]) and np.array_equal(got[:, 2], zz[:, 2]), ("bcast AtLevel", pol)
            # one scalar for the first N/2 coefficients, another for the rest
            for name, w in want_h.items():
                pz = rh.DevicePoly.from_numpy(ring, zz)
                getattr(ring, name)(px, lo, hi, pz)
                assert np.array_equal(pz.numpy(), w), (name, pol)
            # degree-1 x degree-1 tensoring: (x, y) x (zz, reversed x)
            for mform_first in (True, False):
                c = [ring.NewPoly(B) for _ in range(3)]
                ring.TensorDegree1(px, py, rh.DevicePoly.from_numpy(ring, zz), rh.DevicePoly.from_numpy(ring, xr), *c, mform_first=mform_first)
                for j in range(3):
                    assert np.array_equal(c[j].numpy(), want_t[mform_first][j]), ("tensor", mform_first, j, pol)
    ring.close()


# ---- BGV and BFV: the operands and expectations of their own files ---------------------------------------------------------------------
def _bgv_shapes():
    from test_gpu_bgv import SHAPES
    return [SHAPES[0], SHAPES[3], SHAPES[5]]


@pytest.mark.parametrize("shape", [0, 1, 2])
def test_bgv_kernels(rh, shape):
    """bgv_tensor_kernel<SQUARE, ACC> (every pair), bgv_mul_plain_kernel<NC, ACC> (every pair), bgv_axpby_kernel<MODE> (all five)"""
    import bgv_restatement as gr
    import test_gpu_bgv as tb
    from test_bfv_oracle import T
    logN, logQ, level, npoly = _bgv_shapes()[shape]
    c = tb.Ctx(rh, logN, logQ)
    mods = c.Q[:level + 1]
    o = tb.operands(logN, logQ, level, npoly)
    top = level == len(logQ) - 1
    S0, S1 = tb.S0, tb.S1
    mk = lambda names, s: tb.ct(rh, c, level, [o[n] for n in names], s)
    stack = lambda res, n: [np.stack([r[j] for r in res]) for j in range(n)]
    # expectations once, shared by the three policies
    want_mul = {sq: tb.expected_tensor(logN, logQ, level, npoly, sq, False) for sq in (False, True)}
    want_acc = {}
    for sq in (False, True):
        for sout in ((S0 * S0 if sq else S0 * S1) % T, 7):
            want_acc[(sq, sout, False)] = tb.expected_accumulate(logN, logQ, level, npoly, sq, False, sout)
            if top:
                want_acc[(sq, sout, True)] = tb.expected_accumulate(logN, logQ, level, npoly, sq, True, sout)
    comps = ("a0", "a1", "b0")
    accn = ("z0", "z1", "z2")
    want_pt, want_pta = {}, {}
    for d in (0, 1, 2):
        blocks = [o[n] for n in comps[:d + 1]]
        want_pt[d] = tb.per_poly(lambda k: gr.tensor_standard(mods, T, [b[k] for b in blocks], S0, [o["pt"][k]], S1)[0], npoly)
        for sout in (S0 * S1 % T, 7):
            res = [gr.mul_relin_then_add(mods, T, [b[k] for b in blocks], S0, [o["pt"][k]], S1, [o[z][k] for z in accn], sout, False) for k in range(npoly)]
            want_pta[(d, sout)] = (stack([r[0] for r in res], 3), res[0][1])
    d1, d1b, d2 = ("a0", "a1"), ("b0", "b1"), ("b0", "b1", "z2")
    want_ax = {}
    for xn, yn in ((d1, d1b), (d1, d2), (d2, d1)):
        for sub in (False, True):
            res = [gr.add_sub(mods, T, [o[n][k] for n in xn], S0, [o[n][k] for n in yn], S1, sub) for k in range(npoly)]
            want_ax[(xn, yn, sub)] = (stack([r[0] for r in res], len(res[0][0])), res[0][1])
    for pol in POLICIES:
        with policy(pol, c.rq, c.rp):
            op0, op1 = mk(d1, S0), mk(d1b, S1)
            for sq in (False, True):                                       # <SQUARE, 0>
                tb.check(c.ev.MulNew(op0, op0 if sq else op1), want_mul[sq], (S0 * S0 if sq else S0 * S1) % T)
                for sout in ((S0 * S0 if sq else S0 * S1) % T, 7):         # <SQUARE, 1>, <SQUARE, 2>; matched scales and not
                    acc = mk(accn, sout)
                    c.ev.MulThenAdd(op0, op0 if sq else op1, acc)
                    tb.check(acc, *want_acc[(sq, sout, False)])
                    if top:
                        acc = mk(accn[:2], sout)
                        c.ev.MulRelinThenAdd(op0, op0 if sq else op1, acc)
                        tb.check(acc, *want_acc[(sq, sout, True)])
            tb.untouched([op0, op1], [[o[n] for n in d1], [o[n] for n in d1b]])
            pt = mk(("pt",), S1)
            for d in (0, 1, 2):                                            # <NC = d + 1, ACC>
                opd = mk(comps[:d + 1], S0)
                tb.check(c.ev.MulNew(opd, pt), want_pt[d], S0 * S1 % T)
                for sout in (S0 * S1 % T, 7):
                    acc = mk(accn, sout)
                    c.ev.MulThenAdd(opd, pt, acc)
                    tb.check(acc, *want_pta[(d, sout)])
            for (xn, yn, sub), (w, sc) in want_ax.items():                 # modes 0 / 1 (both), 2 (op0 alone), 3 / 4 (+- op1 alone)
                a, b = mk(xn, S0), mk(yn, S1)
                tb.check((c.ev.SubNew if sub else c.ev.AddNew)(a, b), w, sc)


@pytest.mark.parametrize("shape", [0, 1, 3])
def test_bfv_kernels(rh, shape):
    # bfv_tensor_kernel<square> with the nt argument on both rings, then the quantize (composed and fused) of its middle component
    import bfv_restatement as br
    import test_gpu_bfv as tf
    logN, logQ, level, nq, nm, path = tf.SHAPES[shape]
    c = tf.Ctx(rh, logN, logQ)
    P, N = c.P, c.P.N
    Ql, Ml, _, _ = P.at(level)
    rng = np.random.default_rng(1500 + shape)
    rl, ml = c.rq.AtLevel(level), c.rm.AtLevel(nm - 1)
    hq, hm = [tf.patterns(rng, Ql, N) for _ in range(4)], [tf.patterns(rng, Ml, N) for _ in range(4)]
    for h, mods in ((hq, Ql), (hm, Ml)):                              # poly 1: operands whose two products sum past q
        for i, q in enumerate(mods):
            h[0][1, i] = 1; h[1][1, i] = 1; h[2][1, i] = int(q) - 1; h[3][1, i] = int(q) - 1
    want = {}
    for square in (False, True):
        for side, h, mods in (("q", hq, Ql), ("m", hm, Ml)):
            res = [br.tensor_low_deg(mods, [h[0][k], h[1][k]], None if square else [h[2][k], h[3][k]]) for k in range(3)]
            want[(square, side)] = [np.stack([r[j] for r in res]) for j in range(3)]
    xq, xm = want[(False, "q")][1], want[(False, "m")][1]             # the unreduced c1 (< 2q) is what the quantize takes
    want_qz = np.stack([br.quantize(P, level, xq[k], xm[k]) for k in range(3)])
    for pol in POLICIES:
        with policy(pol, c.rq, c.rm):
            dq, dm = [rh.DevicePoly.from_numpy(rl, a) for a in hq], [rh.DevicePoly.from_numpy(ml, a) for a in hm]
            for square in (False, True):
                oq, om = [rl.NewPoly(3) for _ in range(3)], [ml.NewPoly(3) for _ in range(3)]
                c.ev.TensorLowDeg(level, dq[:2], None if square else dq[2:], oq, dm[:2], None if square else dm[2:], om)
                for j in range(3):
                    assert np.array_equal(oq[j].numpy(), want[(square, "q")][j]), (pol, square, "Q", j)
                    assert np.array_equal(om[j].numpy(), want[(square, "m")][j]), (pol, square, "QMul", j)
            for fused in (0, 1):
                c.ev.set_tuning("fused_quantize", fused)
                try:
                    out = rl.NewPoly(3)
                    c.ev.Quantize(level, rh.DevicePoly.from_numpy(rl, xq), rh.DevicePoly.from_numpy(ml, xm), out)
                    assert np.array_equal(out.numpy(), want_qz), (pol, fused)
                finally:
                    c.ev.set_tuning("fused_quantize", 0)

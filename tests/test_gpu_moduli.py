"""GPU: every kernel family on mixed-width modulus chains (oracle/primes.py), bit for bit against the oracle.

The other GPU files slice their chains from the 61-bit test primes (or primes just above 2^60), so the constants the kernels derive (Shoup
wp, Barrett b0/b1, 2^64 - q, Montgomery qinv) always had one bit pattern, and the two Reduce periods of the hybrid key switch (QiOverF,
PiOverF) were always equal.  Here: the reference's CKKS test chains (C45, C90), GenModuli chains with 20- to 61-bit primes (B40, SPLIT,
SPLIT12, SMALL, WIDE: see oracle/primes.chain), conjugate-invariant and 3N rings on small primes, and a seeded fuzz family that draws
its chain with GenModuli."""
import os

import numpy as np
import pytest

from conftest import uniform_mod
from test_oracle_bext import centered_randoms, prod, rns

pytestmark = pytest.mark.gpu
SCALE = int(os.environ.get("RH_FUZZ_SCALE", "1"))


def chain(name, logN):
    from oracle import primes
    return primes.chain(name, logN)


def _block(rng, mods, B, N):
    return np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(B)])


def _key(rng, rows, mods, N):
    return np.stack([np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(2)]) for _ in range(rows)])


# ---- transforms -------------------------------------------------------------------------------------------------------------------
TRANSFORM_CASES = [("C45", 12), ("C45", 13), ("C45", 14), ("C45", 15), ("C90", 13), ("C90", 15), ("WIDE", 12), ("WIDE", 13),
                   ("SMALL", 14), ("SMALL", 16), ("B40", 16), ("B40", 17)]


@pytest.mark.parametrize("name,logN", TRANSFORM_CASES)
def test_transforms_on_mixed_chains(rh, oracle, name, logN):
    """NTT / INTT / NTTLazy / INTTLazy under every launch choice that applies at this size (one-pass at 2^13 / 2^14, hand-scheduled column
    stages at >= 2^14, hand-scheduled tile bodies), worst-case inputs (q - 1) and inverse inputs < 2q; spot rows at N >= 2^16"""
    N = 1 << logN
    Q, P = chain(name, logN)
    mods = (Q + P)[:8]
    L = len(mods)
    ring = rh.Ring(N, mods)
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    rng = np.random.default_rng(logN * 101 + L)
    B = 3
    qv = np.array(mods, dtype=np.uint64)[:, None]
    a = _block(rng, mods, B, N)
    a[0] = qv - np.uint64(1)
    a[1, :, ::2] = 0
    rows = [(k, i) for k in range(B) for i in range(L)] if logN <= 14 else [(0, 0), (0, L - 1), (1, L // 2), (2, 1), (2, L - 1)]
    fwd = {(k, i): oracle.ntt(a[k, i], srs[i]) for k, i in rows}
    lzy = {(k, i): oracle.ntt(a[k, i], srs[i], lazy=True) for k, i in rows}
    knobs = [{}]
    if logN in (13, 14):
        knobs += [{"one_pass": 0}]
    if logN >= 14:
        knobs += [{"one_pass": 0, "asm_cols": 0}]
    knobs += [{"one_pass": 0, "asm_tile": 0}]
    p = rh.DevicePoly.from_numpy(ring, a)
    for kn in knobs:
        for k, v in kn.items():
            ring.set_tuning(k, v)
        o = ring.NewPoly(B)
        ring.NTT(p, o)
        y = o.numpy()
        for k, i in rows:
            assert np.array_equal(y[k, i], fwd[(k, i)]), (kn, k, i)
        ring.NTTLazy(p, o)
        yl = o.numpy()
        for k, i in rows:
            assert np.array_equal(yl[k, i], lzy[(k, i)]), ("lazy", kn, k, i)
        back = ring.NewPoly(B)
        ring.INTTLazy(rh.DevicePoly.from_numpy(ring, y), back)
        gl = back.numpy()
        for k, i in rows:
            assert np.array_equal(gl[k, i], oracle.intt(y[k, i], srs[i], lazy=True)), ("INTTLazy", kn, k, i)
        yin = y.copy()
        yin[2, :, 1::2] += qv                                  # inverse inputs in [q, 2q)
        ring.INTT(rh.DevicePoly.from_numpy(ring, yin), back)
        assert np.array_equal(back.numpy(), a), ("INTT", kn)
        ring.NTT(p, p); ring.INTT(p, p)                        # in place, and back
        assert np.array_equal(p.numpy(), a), ("in place", kn)
        for k in kn:
            ring.set_tuning(k, 1)
    # an AtLevel view over the block with every limb
    v = ring.AtLevel(L // 2)
    pa = rh.DevicePoly.from_numpy(ring, a)
    v.NTT(pa, pa)
    got = pa.numpy()
    for k, i in rows:
        if i <= L // 2:
            assert np.array_equal(got[k, i], fwd[(k, i)])
    assert np.array_equal(got[:, L // 2 + 1:], a[:, L // 2 + 1:])
    ring.close()


@pytest.mark.parametrize("name,logN,B", [("C45", 13, 300), ("B40", 16, 260)])
def test_transforms_past_the_pipelined_span_threshold(rh, oracle, name, logN, B):
    # more than ~2048 rows: the software-pipelined spans (two-pass) and the large-batch one-pass bodies
    N = 1 << logN
    Q, P = chain(name, logN)
    mods = Q[:8]
    ring = rh.Ring(N, mods)
    rng = np.random.default_rng(B + logN)
    base = _block(rng, mods, 5, N)
    a = np.concatenate([base] * (B // 5 + 1))[:B].copy()
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    for kn in ({}, {"one_pass": 0}):
        for k, v in kn.items():
            ring.set_tuning(k, v)
        p = rh.DevicePoly.from_numpy(ring, a)
        ring.NTT(p, p)
        y = p.numpy()
        for k, i in ((0, 0), (B - 1, len(mods) - 1), (B // 2, 3)):
            assert np.array_equal(y[k, i], oracle.ntt(a[k, i], srs[i])), (kn, k, i)
        ring.INTT(p, p)
        assert np.array_equal(p.numpy(), a), kn
        p.free()
    ring.close()


@pytest.mark.parametrize("name,logN", [("C45", 13), ("WIDE", 13), ("SMALL", 14), ("B40", 16)])
def test_seams_and_fused_products_on_mixed_chains(rh, oracle, name, logN):
    """the per-limb transformer seam (SubRings[i].NTT), the whole host Poly entry, Ring.INTTMul (rh_ring_intt_mul) with canonical and lazy
    (< 2q) operands, and Ring.PolyMul (rh_ring_polymul)"""
    N = 1 << logN
    Q, P = chain(name, logN)
    mods = (Q + P)[:6]
    L = len(mods)
    ring = rh.Ring(N, mods)
    srs = [oracle.SubRingConsts(N, q) for q in mods]
    rng = np.random.default_rng(logN + 3 * L)
    a, b = _block(rng, mods, 2, N), _block(rng, mods, 2, N)
    i = L - 1
    assert np.array_equal(ring.SubRings[i].NTT(a[0, i]), oracle.ntt(a[0, i], srs[i]))
    assert np.array_equal(ring.SubRings[0].INTT(oracle.ntt(a[0, 0], srs[0])), a[0, 0])
    host = [a[1, j].copy() for j in range(L)]
    out = [np.zeros(N, dtype=np.uint64) for _ in range(L)]
    ring.NTTHost(host, out)
    for j in range(L):
        assert np.array_equal(out[j], oracle.ntt(a[1, j], srs[j]))
    # INTTMul: INTT(MForm(a) . b) on NTT-domain operands
    z = np.zeros(N, dtype=np.uint64)
    want = np.stack([np.stack([oracle.intt(oracle.vec_op(rh.OPS["MUL_MONT"], oracle.vec_op(rh.OPS["MFORM"], a[k, j], None, z, 0, 0, mods[j]),
                                                          b[k, j], z, 0, 0, mods[j]), srs[j]) for j in range(L)]) for k in range(2)])
    got = ring.NewPoly(2)
    ring.INTTMul(rh.DevicePoly.from_numpy(ring, a), rh.DevicePoly.from_numpy(ring, b), got)
    assert np.array_equal(got.numpy(), want)
    lazy = a.copy(); lazy[:, :, ::3] += np.array(mods, dtype=np.uint64)[None, :, None]
    ring.INTTMul(rh.DevicePoly.from_numpy(ring, lazy), rh.DevicePoly.from_numpy(ring, b), got)
    assert np.array_equal(got.numpy(), want)
    # PolyMul on coefficient-domain operands = INTT(MForm(NTT a) . NTT b)
    na = np.stack([np.stack([oracle.ntt(a[k, j], srs[j]) for j in range(L)]) for k in range(2)])
    nb = np.stack([np.stack([oracle.ntt(b[k, j], srs[j]) for j in range(L)]) for k in range(2)])
    wantp = np.stack([np.stack([oracle.intt(oracle.vec_op(rh.OPS["MUL_MONT"], oracle.vec_op(rh.OPS["MFORM"], na[k, j], None, z, 0, 0, mods[j]),
                                                           nb[k, j], z, 0, 0, mods[j]), srs[j]) for j in range(L)]) for k in range(2)])
    ring.PolyMul(rh.DevicePoly.from_numpy(ring, a), rh.DevicePoly.from_numpy(ring, b), got)
    assert np.array_equal(got.numpy(), wantp)
    ring.close()


# ---- element-wise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C45", "SMALL", "WIDE"])
def test_vec_ops_on_mixed_chains(rh, oracle, name):
    # the opcode loop, the full-range lazy operands and the scalar forms of tests/test_gpu_vec.py on chains of other widths
    N = 4096
    Q, P = chain(name, 12)
    mods = (Q + P)[:5]
    L = len(mods)
    ring = rh.Ring(N, mods)
    rng = np.random.default_rng(len(name) + L)
    qs = np.array(mods, dtype=np.uint64)[None, :, None]
    x, y, zz = (rng.integers(0, 1 << 62, size=(2, L, N), dtype=np.uint64) % qs for _ in range(3))
    x[0, :, 0] = 0; x[0, :, 1] = 1; x[0, :, 2] = qs[0, :, 0] - np.uint64(1); y[0, :, :3] = qs[0] - np.uint64(1)
    s0 = np.array([int(rng.integers(1, q)) for q in mods], dtype=np.uint64)
    s1 = np.array([int(rng.integers(1, q)) for q in mods], dtype=np.uint64)
    px, py = rh.DevicePoly.from_numpy(ring, x), rh.DevicePoly.from_numpy(ring, y)
    for code, op in sorted((v, k) for k, v in rh.OPS.items() if k != "COUNT"):
        a0, a1 = s0, s1
        if op == "MASK":
            a0 = np.array([7, 13, 0, 3, 19], dtype=np.uint64)[:L]; a1 = np.array([(1 << 20) - 1, 0xffff, (1 << 61) - 1, 255, 1], dtype=np.uint64)[:L]
        pz = rh.DevicePoly.from_numpy(ring, zz)
        ring.vec_op(op, px, py, pz, s0=a0, s1=a1)
        got = pz.numpy()
        for k in range(2):
            for i, q in enumerate(mods):
                assert np.array_equal(got[k, i], oracle.vec_op(code, x[k, i], y[k, i], zz[k, i], a0[i], a1[i], q)), (op, k, i)
        pz.free()
    fx, fy, fz = (rng.integers(0, 1 << 64, size=(1, L, N), dtype=np.uint64) for _ in range(3))
    px, py = rh.DevicePoly.from_numpy(ring, fx), rh.DevicePoly.from_numpy(ring, fy)
    for op in ["ADD_LAZY", "SUB_LAZY", "MUL_LAZY", "MUL_LAZY_THEN_ADD_LAZY", "REDUCE", "REDUCE_LAZY", "MUL_BARRETT", "MUL_BARRETT_LAZY",
               "MUL_MONT_LAZY", "MUL_MONT_LAZY_THEN_ADD_LAZY", "MFORM_LAZY", "MUL_MONT_LAZY_THEN_NEG"]:
        pz = rh.DevicePoly.from_numpy(ring, fz)
        ring.vec_op(op, px, py, pz)
        for i, q in enumerate(mods):
            assert np.array_equal(pz.numpy()[0, i], oracle.vec_op(rh.OPS[op], fx[0, i], fy[0, i], fz[0, i], 0, 0, q)), op
        pz.free()
    big, sm = (1 << 200) + 12345678901234567890, 0xFFFFFFFFFFFFFFF1
    A = [[int(v) for v in x[1, i]] for i in range(L)]
    Bv = [[int(v) for v in y[1, i]] for i in range(L)]

    def run(fn, s):
        po = rh.DevicePoly.from_numpy(ring, y)
        fn(rh.DevicePoly.from_numpy(ring, x), s, po)
        return [[int(v) for v in po.numpy()[1, i]] for i in range(L)]
    res = {f: run(getattr(ring, f), s) for f, s in (("AddScalarBigint", big), ("SubScalarBigint", big), ("MulScalar", sm),
                                                     ("MulScalarBigint", big), ("MulScalarThenAdd", sm), ("MulScalarBigintThenAdd", big))}
    for i, q in enumerate(mods):
        q = int(q)
        assert res["AddScalarBigint"][i] == [(v + big) % q for v in A[i]]
        assert res["SubScalarBigint"][i] == [(v - big) % q for v in A[i]]
        assert res["MulScalar"][i] == [(v * sm) % q for v in A[i]]
        assert res["MulScalarBigint"][i] == [(v * big) % q for v in A[i]]
        assert res["MulScalarThenAdd"][i] == [(w + v * sm) % q for v, w in zip(A[i], Bv[i])]
        assert res["MulScalarBigintThenAdd"][i] == [(w + v * big) % q for v, w in zip(A[i], Bv[i])]
    ring.close()


# ---- basis extension --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C45", "SPLIT", "WIDE"])
def test_basis_extension_on_mixed_chains(rh, oracle, name):
    """ModUpQtoP, ModUpPtoQ, ModDownQPtoQ / QPtoP / QPtoQNTT and DecomposeAndSplit for every digit, unreduced outputs bit for bit"""
    N = 4096
    Q, P = chain(name, 12)
    nq, np_ = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    be = rh.BasisExtender(rq, rp)
    rng = np.random.default_rng(nq * 7 + np_)
    B = 2
    a = np.stack([rns(centered_randoms(rng, prod(Q), N), Q) for _ in range(B)])
    pp = rh.DevicePoly(rp, B, np_)
    be.ModUpQtoP(nq - 1, np_ - 1, rh.DevicePoly.from_numpy(rq, a), pp)
    for k in range(B):
        assert np.array_equal(pp.numpy()[k], oracle.modup_centered(a[k], Q, P))
    b = np.stack([rns(centered_randoms(rng, prod(P), N), P) for _ in range(B)])
    pq = rh.DevicePoly(rq, B, nq)
    be.ModUpPtoQ(np_ - 1, nq - 1, rh.DevicePoly.from_numpy(rp, b), pq)
    for k in range(B):
        assert np.array_equal(pq.numpy()[k], oracle.modup_centered(b[k], P, Q))
    vals = [centered_randoms(rng, prod(Q) * prod(P), N) for _ in range(B)]
    aq, ap = np.stack([rns(v, Q) for v in vals]), np.stack([rns(v, P) for v in vals])
    dq, dp = rh.DevicePoly.from_numpy(rq, aq), rh.DevicePoly.from_numpy(rp, ap)
    out, outp = rq.NewPoly(B), rp.NewPoly(B)
    be.ModDownQPtoQ(nq - 1, np_ - 1, dq, dp, out)
    be.ModDownQPtoP(nq - 1, np_ - 1, dq, dp, outp)
    for k in range(B):
        assert np.array_equal(out.numpy()[k], oracle.moddown_qp_to_q(aq[k], ap[k], Q, P))
        assert np.array_equal(outp.numpy()[k], oracle.moddown_qp_to_q(ap[k], aq[k], P, Q))
    srQ = [oracle.SubRingConsts(N, q) for q in Q]; srP = [oracle.SubRingConsts(N, p) for p in P]
    rq.NTT(dq, dq); rp.NTT(dp, dp)
    nqv, npv = dq.numpy(), dp.numpy()
    be.ModDownQPtoQNTT(nq - 1, np_ - 1, dq, dp, out)
    for k in range(B):
        assert np.array_equal(out.numpy()[k], oracle.moddown_qp_to_q_ntt(nqv[k], npv[k], Q, P, srQ, srP))
    beta = (nq - 1 + np_) // np_
    p0 = rh.DevicePoly.from_numpy(rq, a)
    for digit in range(beta):
        oq = rh.DevicePoly.from_numpy(rq, np.zeros((B, nq, N), dtype=np.uint64))
        op = rh.DevicePoly.from_numpy(rp, np.zeros((B, np_, N), dtype=np.uint64))
        be.DecomposeAndSplit(nq - 1, np_ - 1, np_, digit, p0, oq, op)
        for k in range(B):
            eq, ep = oracle.decompose_and_split(nq - 1, np_ - 1, np_, digit, a[k], Q, P)
            assert np.array_equal(oq.numpy()[k], eq), digit
            assert np.array_equal(op.numpy()[k], ep), digit
    be.close(); rq.close(); rp.close()


@pytest.mark.parametrize("name", ["SPLIT", "WIDE"])
def test_adversarial_floating_point_v_on_mixed_chains(rh, oracle, name):
    # the construction of tests/test_gpu_bext.py: values at the ends of the centred range put the float sum within one rounding of an integer
    N = 256
    Q, P = chain(name, 12)
    nq, np_ = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    be = rh.BasisExtender(rq, rp)
    half = prod(Q) // 2
    specials = [0, 1, -1, 2, -2, half, -half, half - 1, -(half - 1), half - 2, half // 2, -(half // 2), 3 * (half // 4)]
    specials += [s * (1 << k) for k in (10, 40, 61, 100) for s in (1, -1) if (1 << k) < half]
    specials += [half - (1 << k) for k in (1, 20, 50) if (1 << k) < half] + [-(half - (1 << k)) for k in (1, 20, 50) if (1 << k) < half]
    rng = np.random.default_rng(nq * 31 + np_)
    vals = [specials[i % len(specials)] if i < 2 * len(specials) else centered_randoms(rng, prod(Q), 1)[0] for i in range(N)]
    a = np.stack([rns(vals, Q)])
    pa = rh.DevicePoly.from_numpy(rq, a)
    pp = rh.DevicePoly(rp, 1, np_)
    be.ModUpQtoP(nq - 1, np_ - 1, pa, pp)
    assert np.array_equal(pp.numpy()[0], oracle.modup_centered(a[0], Q, P))
    oq, op = rh.DevicePoly(rq, 1, nq), rh.DevicePoly(rp, 1, np_)
    be.DecomposeAndSplit(nq - 1, np_ - 1, np_, 0, pa, oq, op)
    eq, ep = oracle.decompose_and_split(nq - 1, np_ - 1, np_, 0, a[0], Q, P)
    keep = list(range(min(np_, nq), nq))
    assert np.array_equal(oq.numpy()[0][keep], eq[keep]) and np.array_equal(op.numpy()[0], ep)
    be.close(); rq.close(); rp.close()


# ---- key switch -------------------------------------------------------------------------------------------------------------------
KS_CASES = [("SPLIT", 12, 2), ("SPLIT12", 12, 2), ("SPLIT12", 13, 2), ("C90", 13, 2), ("SMALL", 12, 2), ("C45", 14, 1)]


@pytest.mark.parametrize("name,logN,npoly", KS_CASES)
def test_gadget_product_on_mixed_chains(rh, oracle, name, logN, npoly):
    """GadgetProduct (both extension paths), the coefficient-domain ciphertext, the hoisted and lazy hoisted forms and the automorphism key
    switch against oracle/compose.py.  On SPLIT12 the Reduce periods differ (255 and 4) and the P accumulator wraps 2^64 on a few percent
    of the coefficients if it is given the Q period: any swap of QiOverF / PiOverF at a call site shows here."""
    from oracle import compose
    N = 1 << logN
    Q, P = chain(name, logN)
    if name == "C45":
        P = P[:2]
    nq, np_ = len(Q), len(P)
    levelQ, levelP = nq - 1, np_ - 1
    beta = (levelQ + levelP + 1) // (levelP + 1)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    be = rh.BasisExtender(rq, rp)
    rng = np.random.default_rng(logN * 13 + nq)
    cx = _block(rng, Q, npoly, N)
    evkQ, evkP = _key(rng, beta, Q, N), _key(rng, beta, P, N)
    want = [compose.gadget_product(N, Q, P, levelQ, levelP, cx[k], evkQ, evkP) for k in range(npoly)]
    pcx = rh.DevicePoly.from_numpy(rq, cx)
    dq = rh.DevicePoly.from_numpy(rq, evkQ.reshape(beta * 2, nq, N)); dp = rh.DevicePoly.from_numpy(rp, evkP.reshape(beta * 2, np_, N))
    for rows in (0, 1024):
        rq.set_tuning("ks_small_rows", rows)
        ct0, ct1 = rh.DevicePoly(rq, npoly, nq), rh.DevicePoly(rq, npoly, nq)
        be.GadgetProduct(levelQ, levelP, pcx, dq.ptr, dp.ptr, beta, ct0, ct1)
        for k in range(npoly):
            assert np.array_equal(ct0.numpy()[k], want[k][0]), (rows, k)
            assert np.array_equal(ct1.numpy()[k], want[k][1]), (rows, k)
    be.close()
    ev = rh.rlwe.Evaluator(rq, rp, galois_keys={5: rh.rlwe.GadgetCiphertext(rq, rp, evkQ, evkP)})
    gct = rh.rlwe.GadgetCiphertext(rq, rp, evkQ, evkP)
    # coefficient-domain ciphertext
    ct = rh.Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=False)
    ev.GadgetProduct(levelQ, pcx, gct, ct)
    for k in range(npoly):
        e0, e1 = compose.gadget_product_coeff(N, Q, P, levelQ, levelP, cx[k], evkQ, evkP)
        assert np.array_equal(ct.Value[0].numpy()[k], e0) and np.array_equal(ct.Value[1].numpy()[k], e1)
    # hoisted, and hoisted lazy + ModDown; the P accumulator of the lazy form against plain integers on one limb
    dec = ev.DecomposeNTT(levelQ, levelP, pcx, True)
    h = rh.Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=True)
    ev.GadgetProductHoisted(levelQ, dec, gct, h)
    lazy = rh.rlwe.ElementQP.alloc(rq, rp, npoly, levelQ, levelP)
    ev.GadgetProductHoistedLazy(levelQ, dec, gct, lazy)
    md = rh.Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=True)
    ev.ModDown(levelQ, levelP, lazy, md)
    for k in range(npoly):
        for c in (0, 1):
            assert np.array_equal(h.Value[c].numpy()[k], want[k][c]), ("hoisted", k, c)
            assert np.array_equal(md.Value[c].numpy()[k], want[k][c]), ("lazy", k, c)
    decp = dec[1].numpy()
    p = int(P[0]); rinv = pow(1 << 64, -1, p)
    acc = sum(evkP[d, 1, 0].astype(object) * decp[d * npoly + npoly - 1, 0].astype(object) for d in range(beta)) * rinv % p
    assert [int(v) for v in lazy.Value[1].P.numpy()[npoly - 1, 0]] == [int(v) for v in acc]
    # automorphism key switch (core/rlwe/evaluator_automorphism.go): AutomorphismNTT(c0 + ks0), AutomorphismNTT(ks1)
    c0 = _block(rng, Q, npoly, N)
    rot = rh.Ciphertext([rq.NewPoly(npoly), rq.NewPoly(npoly)], is_ntt=True)
    ev.Automorphism(rh.Ciphertext([rh.DevicePoly.from_numpy(rq, c0), pcx], is_ntt=True), 5, rot)
    for k in range(npoly):
        for i, q in enumerate(Q):
            s = oracle.vec_op(rh.OPS["ADD"], want[k][0][i], c0[k, i], want[k][0][i], 0, 0, q)
            assert np.array_equal(rot.Value[0].numpy()[k, i], oracle.automorphism_ntt(s, 5))
            assert np.array_equal(rot.Value[1].numpy()[k, i], oracle.automorphism_ntt(want[k][1][i], 5))
    ev.close(); rq.close(); rp.close()


@pytest.mark.parametrize("name,logN,pw2,levelP,is_ntt", [("SPLIT12", 12, 12, 0, True), ("C45", 13, 16, 0, False), ("C45", 12, 24, -1, True),
                                                        ("WIDE", 12, 16, 0, True), ("SMALL", 12, 0, 0, True)])
def test_gadget_product_single_p_on_mixed_chains(rh, oracle, name, logN, pw2, levelP, is_ntt):
    """the single-P / bit-decomposition branch (gadgetProductSinglePAndBitDecompLazy) with a different digit count per limb: 55- and
    45-bit limbs (C45, SPLIT12), 61- down to 20-bit limbs (WIDE)"""
    from oracle import compose
    N = 1 << logN
    Q, P = chain(name, logN)
    Q = Q[:6]
    P = P[:1]
    nq = len(Q)
    rq = rh.Ring(N, Q)
    rp = rh.Ring(N, P) if levelP == 0 else None
    rng = np.random.default_rng(logN + pw2 + nq)
    dpl = [-(-int(q).bit_length() // pw2) for q in Q] if pw2 else None
    if pw2:
        assert len(set(dpl)) > 1
    rows = sum(dpl) if pw2 else nq
    evkQ = _key(rng, rows, Q, N)
    evkP = _key(rng, rows, P, N) if rp is not None else None
    cx = _block(rng, Q, 2, N)
    ev = rh.rlwe.Evaluator(rq, rp)
    gct = rh.rlwe.GadgetCiphertext(rq, rp, evkQ, evkP, BaseTwoDecomposition=pw2, digits_per_limb=dpl)
    ct = rh.Ciphertext([rq.NewPoly(2), rq.NewPoly(2)], is_ntt=is_ntt)
    ev.GadgetProduct(nq - 1, rh.DevicePoly.from_numpy(rq, cx), gct, ct)
    for k in range(2):
        e0, e1 = compose.gadget_product_single_p(N, Q, P if levelP == 0 else [], nq - 1, levelP, cx[k], is_ntt, pw2, dpl, evkQ, evkP)
        assert np.array_equal(ct.Value[0].numpy()[k], e0) and np.array_equal(ct.Value[1].numpy()[k], e1)
    ev.close(); rq.close()
    if rp is not None:
        rp.close()


@pytest.mark.parametrize("name,logN", [("SPLIT12", 12), ("C45", 13)])
def test_external_product_on_mixed_chains(rh, oracle, name, logN):
    from oracle import compose
    N = 1 << logN
    Q, P = chain(name, logN)
    nq, np_ = len(Q), len(P)
    levelQ, levelP = nq - 1, np_ - 1
    beta = (levelQ + levelP + 1) // (levelP + 1)
    rng = np.random.default_rng(logN + nq)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    ev = rh.rgsw.Evaluator(rq, rp)
    kq = [_key(rng, beta, Q, N) for _ in (0, 1)]
    kp = [_key(rng, beta, P, N) for _ in (0, 1)]
    rgsw = rh.rgsw.Ciphertext(rh.rlwe.GadgetCiphertext(rq, rp, kq[0], kp[0]), rh.rlwe.GadgetCiphertext(rq, rp, kq[1], kp[1]))
    c = [_block(rng, Q, 1, N) for _ in (0, 1)]
    op0 = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, c[0]), rh.DevicePoly.from_numpy(rq, c[1])], is_ntt=True)
    out = rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
    ev.ExternalProduct(op0, rgsw, out)
    e0, e1 = compose.external_product(N, Q, P, levelQ, levelP, np.stack([c[0][0], c[1][0]]), True, kq, kp)
    assert np.array_equal(out.Value[0].numpy()[0], e0) and np.array_equal(out.Value[1].numpy()[0], e1)
    ev.close(); rq.close(); rp.close()


@pytest.mark.parametrize("name,logN", [("SPLIT12", 12), ("C90", 13)])
def test_limb_sharded_key_switch_one_rank_vs_oracle(rh, oracle, name, logN):
    """LimbShardedKeySwitch at one rank (its own margins from the full chain, kshard.hip) against the oracle composition directly"""
    from oracle import compose
    from matrix_fhe_lattigo_amd import sharding
    from test_gpu_kshard import _run_shard
    N = 1 << logN
    Q, P = chain(name, logN)
    nq, np_ = len(Q), len(P)
    beta = (nq - 1 + np_) // np_
    rng = np.random.default_rng(logN + 5 * nq)
    cx = _block(rng, Q, 3, N)
    evkQ, evkP = _key(rng, beta, Q, N), _key(rng, beta, P, N)
    g0, g1, ownQ, ownP, b = _run_shard(rh, sharding, N, Q, P, cx, evkQ, evkP, 0, 1, None)
    assert b == beta and ownQ == list(range(nq))
    for k in (0, 2):
        e0, e1 = compose.gadget_product(N, Q, P, nq - 1, np_ - 1, cx[k], evkQ, evkP)
        assert np.array_equal(g0[k], e0) and np.array_equal(g1[k], e1), k


# ---- rescale and the CKKS chain ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("round_", [0, 1])
@pytest.mark.parametrize("nb", [1, 3])
def test_rescale_dropping_smaller_moduli(rh, oracle, round_, nb):
    # C45: the dropped moduli (45 bits) are smaller than Q[0] (55 bits)
    from test_oracle_rescale import div_round
    N = 4096
    Q, _ = chain("C45", 12)
    L = len(Q)
    ring = rh.Ring(N, Q)
    rng = np.random.default_rng(nb * 2 + round_)
    big = prod(Q)
    vals = [[int.from_bytes(rng.bytes(big.bit_length() // 8 + 2), "little") % big for _ in range(N)] for _ in range(2)]
    a = np.stack([rns(v, Q) for v in vals])
    exp = np.stack([oracle.div_by_last_modulus_many(a[k], Q, nb, round_) for k in range(2)])
    p1 = rh.DevicePoly(ring, 2, L - nb)
    (ring.DivRoundByLastModulusMany if round_ else ring.DivFloorByLastModulusMany)(nb, rh.DevicePoly.from_numpy(ring, a), p1)
    assert np.array_equal(p1.numpy(), exp)
    want = list(vals[1][:32])
    for j in range(nb):
        want = [div_round(v, Q[L - 1 - j]) if round_ else v // Q[L - 1 - j] for v in want]
    for i in range(L - nb):
        assert [int(x) for x in p1.numpy()[1, i][:32]] == [w % Q[i] for w in want]
    pn = rh.DevicePoly.from_numpy(ring, a)
    ring.NTT(pn, pn)
    po = rh.DevicePoly.from_numpy(ring, np.zeros((2, L, N), dtype=np.uint64))
    (ring.DivRoundByLastModulusManyNTT if round_ else ring.DivFloorByLastModulusManyNTT)(nb, pn, po)
    sub = ring.AtLevel(L - nb - 1)
    chk = rh.DevicePoly.from_numpy(sub, po.numpy()[:, :L - nb].copy())
    sub.INTT(chk, chk)
    assert np.array_equal(chk.numpy(), exp)
    ring.close()


def test_ckks_mul_relin_rescale_on_c45(rh, oracle):
    from oracle import compose
    from test_gpu_ckks import oracle_tensor, vop
    N = 4096
    Q, P = chain("C45", 12)
    nq, np_ = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    rng = np.random.default_rng(45)
    beta = (nq - 1 + np_) // np_
    evkQ, evkP = _key(rng, beta, Q, N), _key(rng, beta, P, N)
    ev = rh.ckks.Evaluator(rq, rp, rlk=rh.rlwe.GadgetCiphertext(rq, rp, evkQ, evkP))
    a = np.stack([_block(rng, Q, 1, N) for _ in range(2)])
    b = np.stack([_block(rng, Q, 1, N) for _ in range(2)])
    ct0 = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, a[0]), rh.DevicePoly.from_numpy(rq, a[1])], is_ntt=True)
    ct1 = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, b[0]), rh.DevicePoly.from_numpy(rq, b[1])], is_ntt=True)
    out = rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
    ev.MulRelin(ct0, ct1, out, relin=True)
    res = rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
    ev.Rescale(out, res)
    exp = oracle_tensor(oracle, rh, a[:, 0], b[:, 0], Q)
    g0, g1 = compose.gadget_product(N, Q, P, nq - 1, np_ - 1, exp[2], evkQ, evkP)
    srQ = [oracle.SubRingConsts(N, q) for q in Q]
    for c, g in ((0, g0), (1, g1)):
        e = np.stack([vop(oracle, rh, "ADD", exp[c][i], g[i], g[i], Q[i]) for i in range(nq)])
        assert np.array_equal(out.Value[c].numpy()[0], e)
        down = oracle.div_by_last_modulus_many(np.stack([oracle.intt(e[i], srQ[i]) for i in range(nq)]), Q, 1, True)
        assert np.array_equal(res.Value[c].numpy()[0, :nq - 1], np.stack([oracle.ntt(down[i], srQ[i]) for i in range(nq - 1)]))
    ev.close(); rq.close(); rp.close()


# ---- other ring kinds -------------------------------------------------------------------------------------------------------------
def test_conjugate_invariant_ring_on_a_generated_mixed_chain(rh, oracle):
    from oracle import primes
    from test_gpu_keyswitch import _generic_gadget_product
    N = 4096
    Q, P = primes.gen_moduli(14, [50, 40, 40, 30], [55, 45])                  # NthRoot = 4N
    rq, rp = rh.Ring(N, Q, kind=rh.ConjugateInvariant), rh.Ring(N, P, kind=rh.ConjugateInvariant)
    srQ = [oracle.SubRingConsts(N, q, nthroot=4 * N) for q in Q]; srP = [oracle.SubRingConsts(N, p, nthroot=4 * N) for p in P]
    rng = np.random.default_rng(4)
    a = _block(rng, Q, 2, N)
    pa = rh.DevicePoly.from_numpy(rq, a)
    rq.NTT(pa, pa)
    got = pa.numpy()
    for k in range(2):
        for i in range(len(Q)):
            assert np.array_equal(got[k, i], oracle.ntt_ci(a[k, i], srQ[i]))
    rq.INTT(pa, pa)
    assert np.array_equal(pa.numpy(), a)
    fq = lambda x, i: oracle.ntt_ci(x, srQ[i]); iq = lambda x, i: oracle.intt_ci(x, srQ[i])
    fp = lambda x, j: oracle.ntt_ci(x, srP[j]); ip = lambda x, j: oracle.intt_ci(x, srP[j])
    nq, np_ = len(Q), len(P)
    beta = (nq - 1 + np_) // np_
    evkQ, evkP = _key(rng, beta, Q, N), _key(rng, beta, P, N)
    be = rh.BasisExtender(rq, rp)
    dq = rh.DevicePoly.from_numpy(rq, evkQ.reshape(beta * 2, nq, N)); dp = rh.DevicePoly.from_numpy(rp, evkP.reshape(beta * 2, np_, N))
    ct0, ct1 = rh.DevicePoly(rq, 2, nq), rh.DevicePoly(rq, 2, nq)
    be.GadgetProduct(nq - 1, np_ - 1, rh.DevicePoly.from_numpy(rq, a), dq.ptr, dp.ptr, beta, ct0, ct1)
    e0, e1 = _generic_gadget_product(oracle, N, Q, P, nq - 1, np_ - 1, a[1], evkQ, evkP, fq, iq, fp, ip)
    assert np.array_equal(ct0.numpy()[1], e0) and np.array_equal(ct1.numpy()[1], e1)
    be.close(); rq.close(); rp.close()


@pytest.mark.parametrize("bits,N", [(31, 3 << 13), (12, 6), (12, 12), (12, 48)])
def test_3n_transforms_on_small_primes(rh, oracle, bits, N):
    # 3N rings: 31-bit primes at N = 3 * 2^13 in both NTT-domain layouts, 12-bit primes at the small N of ring/ntt_3n_test.go
    from oracle import primes
    from test_oracle_ntt3n import omega_for
    L = 3 if bits == 31 else 1
    mods, _ = primes.gen_moduli_3n(N, [bits] * L, [])
    om = [omega_for(q, N) for q in mods]
    ring = rh.Ring(N, mods, kind=rh.Matrix3N, omega3n=om)
    rng = np.random.default_rng(bits + N)
    a = _block(rng, mods, 2, N)
    for order in ((0, 1) if bits == 31 else (0,)):
        ring.set_tuning("ntt3n_block_order", order)
        p = rh.DevicePoly.from_numpy(ring, a)
        ring.NTT(p, p)
        if order:
            ref = ring.NewPoly(2)
            ring.NTT3NReorder(p, ref, to_reference=True)
            y = ref.numpy()
        else:
            y = p.numpy()
        for k in range(2):
            for i, q in enumerate(mods):
                assert np.array_equal(y[k, i], oracle.ntt3n_forward(a[k, i], q, om[i])), (order, k, i)
        ring.INTT(p, p)
        assert np.array_equal(p.numpy(), a), order
    ring.close()


def test_3n_key_switch_with_primes_below_2_33(rh, oracle):
    # every prime < 2^33: both margins above 2^31 (the clamp of rh_overflow_margin), a five-digit product
    from oracle import primes
    from test_gpu_keyswitch import _generic_gadget_product
    from test_oracle_ntt3n import omega_for
    N = 3 << 13
    Q, P = primes.gen_moduli_3n(N, [30] * 5, [31, 31])
    assert max(Q + P) < 1 << 33
    wQ, wP = [omega_for(q, N) for q in Q], [omega_for(p, N) for p in P]
    rq, rp = rh.Ring(N, Q, kind=rh.Matrix3N, omega3n=wQ), rh.Ring(N, P, kind=rh.Matrix3N, omega3n=wP)
    fq = lambda x, i: oracle.ntt3n_forward(x, Q[i], wQ[i]); iq = lambda x, i: oracle.ntt3n_backward(x, Q[i], wQ[i])
    fp = lambda x, j: oracle.ntt3n_forward(x, P[j], wP[j]); ip = lambda x, j: oracle.ntt3n_backward(x, P[j], wP[j])
    nq, np_ = len(Q), len(P)
    beta = (nq - 1 + np_) // np_
    rng = np.random.default_rng(33)
    cx = _block(rng, Q, 2, N)
    evkQ, evkP = _key(rng, beta, Q, N), _key(rng, beta, P, N)
    be = rh.BasisExtender(rq, rp)
    dq = rh.DevicePoly.from_numpy(rq, evkQ.reshape(beta * 2, nq, N)); dp = rh.DevicePoly.from_numpy(rp, evkP.reshape(beta * 2, np_, N))
    ct0, ct1 = rh.DevicePoly(rq, 2, nq), rh.DevicePoly(rq, 2, nq)
    be.GadgetProduct(nq - 1, np_ - 1, rh.DevicePoly.from_numpy(rq, cx), dq.ptr, dp.ptr, beta, ct0, ct1)
    e0, e1 = _generic_gadget_product(oracle, N, Q, P, nq - 1, np_ - 1, cx[1], evkQ, evkP, fq, iq, fp, ip)
    assert np.array_equal(ct0.numpy()[1], e0) and np.array_equal(ct1.numpy()[1], e1)
    be.close(); rq.close(); rp.close()


# ---- seeded fuzz: chains drawn with GenModuli -------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(24 * SCALE))
def test_fuzz_generated_chains(rh, oracle, case):
    """a chain of random sizes in [20, 61] bits drawn with GenModuli, a shape drawn as in tests/test_gpu_fuzz.py; the four transforms
    through an AtLevel view and one element-wise product, checked on drawn rows.  Every case is derived from its number."""
    from oracle import primes
    from test_gpu_fuzz import _draw_shape, _spots
    rng = np.random.default_rng(9100 + case)
    logN, L, level, B = _draw_shape(rng, 400)
    logN = max(logN, 4)
    if logN >= 14:
        B = min(B, 8)
    L = min(L, 8)
    level = min(level, L - 1)
    N = 1 << logN
    lo = 20 if logN <= 12 else 30
    sizes = [int(rng.integers(lo, 62)) for _ in range(L)]
    mods, _ = primes.gen_moduli(logN + 1, sizes, [])
    ring = rh.Ring(N, mods)
    v = ring.AtLevel(level)
    a = _block(rng, mods, B, N)
    srs = [oracle.SubRingConsts(N, q) for q in mods[:level + 1]]
    spots = _spots(rng, B, level)
    which = ["NTT", "INTT", "NTTLazy", "INTTLazy"][case % 4]
    p = rh.DevicePoly.from_numpy(ring, a)
    o = rh.DevicePoly.from_numpy(ring, a)
    getattr(v, which)(p, o)
    got = o.numpy()
    for k, i in spots:
        x = a[k, i]
        want = {"NTT": lambda: oracle.ntt(x, srs[i]), "NTTLazy": lambda: oracle.ntt(x, srs[i], lazy=True),
                "INTT": lambda: oracle.intt(x, srs[i]), "INTTLazy": lambda: oracle.intt(x, srs[i], lazy=True)}[which]()
        assert np.array_equal(got[k, i], want), (case, sizes, which, k, i)
    assert np.array_equal(got[:, level + 1:], a[:, level + 1:])
    b = _block(rng, mods, B, N)
    pb = rh.DevicePoly.from_numpy(ring, b)
    v.MulCoeffsMontgomery(p, pb, pb)
    gb = pb.numpy()
    for k, i in spots:
        assert np.array_equal(gb[k, i], oracle.vec_op(rh.OPS["MUL_MONT"], a[k, i], b[k, i], b[k, i], 0, 0, mods[i])), (case, k, i)
    ring.close()

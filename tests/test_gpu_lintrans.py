"""GPU: linear transformations on the device (circuits/common/lintrans, circuits/ckks/lintrans).  The three kernels of csrc/lintrans.hip against
Python integers, whole arrays, bit for bit, under both cache policies; Encoder.Embed into a PolyQP and lintrans.Encode against the restatement;
Evaluate / EvaluateMany / EvaluateSequential -- fused and composed -- against the restatement that tests/test_lintrans_oracle.py pins to
decryption (tests/lintrans_restatement.py), and by decrypting the device output on the host; every refusal by its text.

Shapes: TAIL (N = 32: a row inside one wavefront, a last digit of 3 limbs), REF (N = 2^10, mixed-width limbs), Q61N13 (N = 2^13: more than one
block per row, 61-bit moduli); batches of 3 ciphertexts (a ragged grid tail); the top level and one below."""
import functools
import random

import numpy as np
import pytest

import ckks_encoder_restatement as cer
import ckks_restatement as cr
import lintrans_restatement as ltr
import rlwe_restatement as rr
import test_rlwe_oracle as t
from test_gpu_rlwe_decrypt import B, Device, host, same

pytestmark = pytest.mark.gpu
_ids = t._ids
SHAPES = [("TAIL", (0, 4)), ("REF", (0, 2)), ("Q61N13", (0, 2))]
SMALL_DIAGS = [-5, -1, 0, 1, 2, 3, 7]
REF_DIAGS = [-15, -4, -1, 0, 1, 2, 3, 4, 15]
R = 1 << 64


def uniform(tag, N, mods, count=B):
    return [rr.uniform_poly(random.Random("%s %d" % (tag, k)), N, mods) for k in range(count)]


def obj(arrs):
    return np.stack(arrs).astype(object)


def up(rh, ring, arrs):
    return rh.DevicePoly.from_numpy(ring, np.stack(arrs))


def col(mods):
    """the moduli as a column against (polys, limbs, N) blocks"""
    return np.array([int(q) for q in mods], dtype=object).reshape(1, -1, 1)


# ---- rh_rlwe_diag_mac_qp ------------------------------------------------------------------------------------------------------------------------
def diag_mac(rh, d, level, levelP, pts, xs, out, table):
    """terms: pts[k] = (ptQ, ptP) one-poly blocks, xs[k] = (xQ0, xQ1, xP0, xP1) batches, xP0 = xP1 = None for the baby step 0 term"""
    import ctypes as C
    K = len(pts)
    ptQ = (C.c_void_p * max(K, 1))(*[p[0].ptr for p in pts])
    ptP = (C.c_void_p * max(K, 1))(*[p[1].ptr for p in pts])
    flat = [None if b is None else b.ptr for x in xs for b in x]
    x = (C.c_void_p * max(4 * K, 1))(*flat)
    return rh.lib().rh_rlwe_diag_mac_qp(d.ev.be._h, level, levelP, K, ptQ, ptP, x, out[0].ptr, out[1].ptr, out[2].ptr, out[3].ptr, B, table.ptr, table.words)


@functools.lru_cache(maxsize=None)
def mac_operands(name, level):
    """two diagonals allocated at the TOP level (more rows than the level needs), two ciphertexts modulo QP and the pair P ct modulo Q; shared by
    the cases of a shape"""
    N, Q, P, levels = t.chain(name)
    P = P[:dict(SHAPES)[name][1]]
    top, mods, pm = levels[0], [int(q) for q in Q[:level + 1]], [int(p) for p in P]
    hpt = [(rr.uniform_poly(random.Random("ptq %s %d" % (name, a)), N, [int(q) for q in Q[:top + 1]]),
            rr.uniform_poly(random.Random("ptp %s %d" % (name, a)), N, pm)) for a in (0, 1)]
    hx = [([uniform("xq%d%d %s %d" % (b, c, name, level), N, mods) for c in (0, 1)], [uniform("xp%d%d %s" % (b, c, name), N, pm) for c in (0, 1)]) for b in (0, 1)]
    hp = [uniform("pct%d %s %d" % (c, name, level), N, mods) for c in (0, 1)]
    return hpt, hx, hp


@pytest.mark.parametrize("K", [1, 4, 56, 57, 113])
@pytest.mark.parametrize("nt_streams", [1, 2], ids=["nt-by-size", "nt-always"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_diag_mac_against_python_integers(rh, shape, nt_streams, K):
    """tmp_c = (sum_k pt_k x_{k,c}) 2^-64 mod q for K terms below, at and across the 56-term chunk, with and without the baby step 0 term (modulo Q
    only: nothing on the P rows, which are zero when it is the only term).  The terms draw on two diagonals and two pre-rotated ciphertexts, so
    the expected sum is a few whole-array products over Python integers with multiplicities; the inputs are left alone."""
    name, setting = shape
    d = Device(rh, name, setting)
    d.rq.set_tuning("nt_streams", nt_streams)
    N, Q, P = d.N, d.Q, d.P
    levelP = len(P) - 1
    pm = [int(p) for p in P]
    L = rh.lib()
    top = d.levels[0]
    rnd = random.Random("mac %s %d" % (name, K))
    for level in d.levels[:2]:
        mods = [int(q) for q in Q[:level + 1]]
        rql, rpl = d.rq.AtLevel(level), d.rp.AtLevel(levelP)
        hpt, hx, hp = mac_operands(name, level)
        dpt = [(up(rh, d.rq.AtLevel(top), [q]), up(rh, rpl, [p])) for q, p in hpt]
        dx = [(up(rh, rql, q[0]), up(rh, rql, q[1]), up(rh, rpl, p[0]), up(rh, rpl, p[1])) for q, p in hx]
        dp = (up(rh, rql, hp[0]), up(rh, rql, hp[1]), None, None)
        table = rh.DevicePoly(d.rq.AtLevel(0), max(1, -(-L.rh_rlwe_diag_mac_qp_table_words(K + 1, level, levelP) // N)), 1)
        for with0 in (False, True):
            picks = [(rnd.randrange(2), rnd.randrange(2)) for _ in range(K)]
            pts, xs = [dpt[a] for a, _ in picks], [dx[b] for _, b in picks]
            n0 = 0
            if with0:                                                   # the baby step 0 term comes first (index[j] is sorted)
                pts, xs = [dpt[picks[0][0]]] + pts[1:], [dp] + xs[1:]
                n0, picks = 1, picks[1:]
            out = [rql.NewPoly(B), rql.NewPoly(B), rpl.NewPoly(B), rpl.NewPoly(B)]
            assert diag_mac(rh, d, level, levelP, pts, xs, out, table) == 0, L.rh_last_error()
            for c in (0, 1):
                sq, sp = 0, 0
                for a in (0, 1):
                    for b in (0, 1):
                        m = picks.count((a, b))
                        if m:
                            sq = sq + m * (obj([hpt[a][0][:level + 1]]) * obj(hx[b][0][c]))
                            sp = sp + m * (obj([hpt[a][1]]) * obj(hx[b][1][c]))
                if n0:
                    sq = sq + obj([hpt[pts_first(pts, dpt)][0][:level + 1]]) * obj(hp[c])
                wq = np.zeros((B, level + 1, N), dtype=np.uint64) if isinstance(sq, int) else ((sq * np.array([pow(R, -1, q) for q in mods], dtype=object).reshape(1, -1, 1)) % col(mods)).astype(np.uint64)
                wp = np.zeros((B, len(pm), N), dtype=np.uint64) if isinstance(sp, int) else ((sp * np.array([pow(R, -1, p) for p in pm], dtype=object).reshape(1, -1, 1)) % col(pm)).astype(np.uint64)
                assert np.array_equal(out[c].numpy(), wq), (level, K, with0, c, "Q")
                assert np.array_equal(out[2 + c].numpy(), wp), (level, K, with0, c, "P")
        for (q, p), (dq, dpp) in zip(hpt, dpt):                          # the operands are read only
            assert np.array_equal(dq.numpy()[0], q) and np.array_equal(dpp.numpy()[0], p)
        for (q, p), blocks in zip(hx, dx):
            assert all(np.array_equal(blocks[c].numpy(), np.stack(q[c])) and np.array_equal(blocks[2 + c].numpy(), np.stack(p[c])) for c in (0, 1))
        assert all(np.array_equal(dp[c].numpy(), np.stack(hp[c])) for c in (0, 1))
    d.close()


def pts_first(pts, dpt):
    return 0 if pts[0] is dpt[0] else 1


def test_diag_mac_overflow_bound(rh):
    """every operand equal to q - 1 on the 61-bit chain: a full chunk of 56 terms and 113 terms, the largest sums the 128-bit accumulators and the
    one-word Montgomery step are sized for (csrc/lc_reduce.hip.hpp)"""
    name, setting = "Q61N13", (0, 2)
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    level, levelP = d.levels[0], len(P) - 1
    mods, pm = [int(q) for q in Q[:level + 1]], [int(p) for p in P]
    rql, rpl = d.rq.AtLevel(level), d.rp.AtLevel(levelP)
    full = lambda ms, n: [np.stack([np.full(N, q - 1, dtype=np.uint64) for q in ms]) for _ in range(n)]
    pt = (up(rh, rql, full(mods, 1)), up(rh, rpl, full(pm, 1)))
    x = (up(rh, rql, full(mods, B)), up(rh, rql, full(mods, B)), up(rh, rpl, full(pm, B)), up(rh, rpl, full(pm, B)))
    L = rh.lib()
    for K in (56, 113):
        table = rh.DevicePoly(d.rq.AtLevel(0), max(1, -(-L.rh_rlwe_diag_mac_qp_table_words(K, level, levelP) // N)), 1)
        out = [rql.NewPoly(B), rql.NewPoly(B), rpl.NewPoly(B), rpl.NewPoly(B)]
        assert diag_mac(rh, d, level, levelP, [pt] * K, [x] * K, out, table) == 0, L.rh_last_error()
        for c in (0, 1):
            for blk, ms in ((out[c], mods), (out[2 + c], pm)):
                got = blk.numpy()
                for i, q in enumerate(ms):
                    assert np.all(got[:, i] == np.uint64(K * (q - 1) * (q - 1) * pow(R, -1, q) % q)), (K, c, i)
    d.close()


def test_table_staging_is_shared_with_the_linear_combination(rh):
    """rh_rlwe_diag_mac_qp and rh_ckks_linear_combination stage their tables through ONE ring of four page-locked slots per calling thread
    (csrc/engine.hip: rh_stage_slot).  On a thread of its own -- fresh slots, so the schedule below does not depend on the tests before it -- the
    two alternate nine times with tables that grow and shrink: diag_mac with 1, 57, 4, 113, 0, ... terms (6 words a term; no term, no slot) and
    the linear combination with 1, 9, 2, ... terms (4 + 8 words a term at level 1).  Slots in order of use:
      0 1 2 3 | 0 1 2 (grown by their own caller) 3 (reused) | - 0 (grown under diag_mac's last use) | 1 (diag_mac reuses the other's) 2 | 3 (grown
      under the other's last use) 0 | 1 2 | 3 0
    Nothing is read back before the last call, so a slot is taken again while the copies before it may still be in flight; then every output,
    whole and bit for bit, against the Python-integer expectations of this file and of tests/test_gpu_polynomial.py."""
    import threading
    import test_gpu_polynomial as tp
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    level, levelP = d.levels[0], len(P) - 1
    mods, pm = [int(q) for q in Q[:level + 1]], [int(p) for p in P]
    rql, rpl = d.rq.AtLevel(level), d.rp.AtLevel(levelP)
    hpt, hx, _ = mac_operands(name, level)
    dpt = [(up(rh, d.rq.AtLevel(d.levels[0]), [q]), up(rh, rpl, [p])) for q, p in hpt]
    dx = [(up(rh, rql, q[0]), up(rh, rql, q[1]), up(rh, rpl, p[0]), up(rh, rpl, p[1])) for q, p in hx]
    L = rh.lib()
    mac_table = rh.DevicePoly(d.rq.AtLevel(0), -(-L.rh_rlwe_diag_mac_qp_table_words(113, level, levelP) // N), 1)

    logN, logQ, lc_level, npoly = tp.SHAPES[0]
    assert (1 << logN, npoly) == (N, B)
    c = tp.Ctx(rh, logN, logQ)
    _, _, rows, X, s0, s1, _, prefix = tp.lc_case(logN, logQ, lc_level, npoly)
    rl = c.rq.AtLevel(lc_level)
    dev = [[rh.DevicePoly.from_numpy(c.rq.AtLevel(rows[k] - 1), b) for b in X[k][:2]] for k in range(9)]
    lc_table = rh.DevicePoly(rl, 1, -(-L.rh_ckks_linear_combination_table_words(9, lc_level) // N))

    MAC_K, LC_K = [1, 57, 4, 113, 0, 1, 57, 4, 113], [1, 9, 2] * 3
    rnd = random.Random("staging")
    picks = [[(rnd.randrange(2), rnd.randrange(2)) for _ in range(K)] for K in MAC_K]
    mac_out = [[rql.NewPoly(B), rql.NewPoly(B), rpl.NewPoly(B), rpl.NewPoly(B)] for _ in MAC_K]
    lc_out = [[rl.NewPoly(npoly), rl.NewPoly(npoly)] for _ in LC_K]
    status = []

    def calls():
        for i in range(9):
            rc = diag_mac(rh, d, level, levelP, [dpt[a] for a, _ in picks[i]], [dx[b] for _, b in picks[i]], mac_out[i], mac_table)
            status.append(rc if rc == 0 else (rc, L.rh_last_error()))
            rc = tp.lc_call(rh, c.rq, lc_level, dev[:LC_K[i]], rows, s0, s1, None, lc_out[i], lc_table, npoly)
            status.append(rc if rc == 0 else (rc, L.rh_last_error()))

    th = threading.Thread(target=calls)
    th.start()
    th.join()
    assert status == [0] * 18, status
    rinv = lambda ms: np.array([pow(R, -1, q) for q in ms], dtype=object).reshape(1, -1, 1)
    for i, K in enumerate(MAC_K):
        for comp in (0, 1):
            sq, sp = np.zeros((B, level + 1, N), dtype=object), np.zeros((B, len(pm), N), dtype=object)
            for a, b in picks[i]:
                sq = sq + obj([hpt[a][0][:level + 1]]) * obj(hx[b][0][comp])
                sp = sp + obj([hpt[a][1]]) * obj(hx[b][1][comp])
            assert np.array_equal(mac_out[i][comp].numpy(), ((sq * rinv(mods)) % col(mods)).astype(np.uint64)), (i, K, comp, "Q")
            assert np.array_equal(mac_out[i][2 + comp].numpy(), ((sp * rinv(pm)) % col(pm)).astype(np.uint64)), (i, K, comp, "P")
    for i, K in enumerate(LC_K):
        for j in (0, 1):
            assert np.array_equal(lc_out[i][j].numpy(), np.stack(prefix[K][j])), (i, K, j)
    d.close()


# ---- the two rotate kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt_streams", [1, 2], ids=["nt-by-size", "nt-always"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rotate_kernels_against_python_integers(rh, shape, nt_streams):
    """rh_rlwe_rotate_sum_accumulate_qp: acc (=|+=) (c + [c == 0] tmp0)[index]; rh_rlwe_rotate_mul_accumulate_qp: acc (=|+=) pt (c + [c == 0, Q rows]
    P ct0)[index] 2^-64; for g = 5, 5^-1, 25 and 2N - 1, acc written (first) and added to, both components, Q and P rows, with the reference's index
    table; the inputs are left alone"""
    name, setting = shape
    d = Device(rh, name, setting)
    d.rq.set_tuning("nt_streams", nt_streams)
    N, Q, P = d.N, d.Q, d.P
    levelP = len(P) - 1
    Pb = rr.prod(P)
    pm = [int(p) for p in P]
    L = rh.lib()
    be = d.ev.be._h
    for level in d.levels[:2]:
        mods = [int(q) for q in Q[:level + 1]]
        rql, rpl = d.rq.AtLevel(level), d.rp.AtLevel(levelP)
        cq, cp = [uniform("cq%d %s %d" % (c, name, level), N, mods) for c in (0, 1)], [uniform("cp%d %s" % (c, name), N, pm) for c in (0, 1)]
        aq, ap = [uniform("aq%d %s %d" % (c, name, level), N, mods) for c in (0, 1)], [uniform("ap%d %s" % (c, name), N, pm) for c in (0, 1)]
        t0q, t0p = uniform("t0q %s %d" % (name, level), N, mods), uniform("t0p %s" % name, N, pm)
        c0 = uniform("c0 %s %d" % (name, level), N, mods)
        ptq, ptp = rr.uniform_poly(random.Random("rptq " + name), N, mods), rr.uniform_poly(random.Random("rptp " + name), N, pm)
        dc = [up(rh, rql, cq[0]), up(rh, rql, cq[1]), up(rh, rpl, cp[0]), up(rh, rpl, cp[1])]
        dt0q, dt0p, dc0 = up(rh, rql, t0q), up(rh, rpl, t0p), up(rh, rql, c0)
        dptq, dptp = up(rh, rql, [ptq]), up(rh, rpl, [ptp])
        # what is permuted, before the index map: (c + tmp0) for the sum kernel; pt-independent (c + P ct0) 2^-64 for the product kernel
        sumQ = [(obj(cq[0]) + obj(t0q)) % col(mods), obj(cq[1])]
        sumP = [(obj(cp[0]) + obj(t0p)) % col(pm), obj(cp[1])]
        rinvQ = np.array([pow(R, -1, q) for q in mods], dtype=object).reshape(1, -1, 1)
        rinvP = np.array([pow(R, -1, p) for p in pm], dtype=object).reshape(1, -1, 1)
        mulQ = [((obj(cq[0]) + obj(c0) * np.array([Pb % q for q in mods], dtype=object).reshape(1, -1, 1)) * rinvQ) % col(mods), (obj(cq[1]) * rinvQ) % col(mods)]
        mulP = [(obj(cp[c]) * rinvP) % col(pm) for c in (0, 1)]
        for g in (5, pow(5, -1, 2 * N), 25, 2 * N - 1):
            idx = rh.AutomorphismNTTIndex(N, 2 * N, g).astype(np.int64)
            prodQ = [(obj([ptq]) * mulQ[c][:, :, idx]) % col(mods) for c in (0, 1)]
            prodP = [(obj([ptp]) * mulP[c][:, :, idx]) % col(pm) for c in (0, 1)]
            for first in (True, False):
                acc = [up(rh, rql, aq[0]), up(rh, rql, aq[1]), up(rh, rpl, ap[0]), up(rh, rpl, ap[1])]
                rc = L.rh_rlwe_rotate_sum_accumulate_qp(be, level, levelP, g, dc[0].ptr, dc[1].ptr, dc[2].ptr, dc[3].ptr, dt0q.ptr, dt0p.ptr,
                                                        acc[0].ptr, acc[1].ptr, acc[2].ptr, acc[3].ptr, B, 1 if first else 0)
                assert rc == 0, L.rh_last_error()
                for c in (0, 1):
                    for blk, s, a, ms in ((acc[c], sumQ[c], aq[c], mods), (acc[2 + c], sumP[c], ap[c], pm)):
                        want = s[:, :, idx] if first else (s[:, :, idx] + obj(a)) % col(ms)
                        assert np.array_equal(blk.numpy(), want.astype(np.uint64)), ("sum", level, g, first, c)
                acc = [up(rh, rql, aq[0]), up(rh, rql, aq[1]), up(rh, rpl, ap[0]), up(rh, rpl, ap[1])]
                rc = L.rh_rlwe_rotate_mul_accumulate_qp(be, level, levelP, g, dptq.ptr, dptp.ptr, dc0.ptr, dc[0].ptr, dc[1].ptr, dc[2].ptr, dc[3].ptr,
                                                        acc[0].ptr, acc[1].ptr, acc[2].ptr, acc[3].ptr, B, 1 if first else 0)
                assert rc == 0, L.rh_last_error()
                for c in (0, 1):
                    for blk, s, a, ms in ((acc[c], prodQ[c], aq[c], mods), (acc[2 + c], prodP[c], ap[c], pm)):
                        want = s if first else (s + obj(a)) % col(ms)
                        assert np.array_equal(blk.numpy(), want.astype(np.uint64)), ("mul", level, g, first, c)
        for blk, h in zip(dc + [dt0q, dt0p, dc0], cq + cp + [t0q, t0p, c0]):   # the permuted operands are read only
            assert np.array_equal(blk.numpy(), np.stack(h))
        assert np.array_equal(dptq.numpy()[0], ptq) and np.array_equal(dptp.numpy()[0], ptp)
    d.close()


# ---- Encoder.Embed into a PolyQP, lintrans.Encode -------------------------------------------------------------------------------------------------
def make_diagonals(tag, idx, slots):
    rnd = random.Random("diags " + tag)
    return {i: [complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(slots)] for i in idx}


class Meta:
    def __init__(self, scale, log_slots):
        self.Scale, self.LogDimensions, self.IsNTT, self.IsMontgomery, self.IsBatched = scale, log_slots, True, True, True


@pytest.mark.parametrize("shape", SHAPES[:2], ids=_ids)
def test_embed_into_a_poly_qp(rh, shape):
    """the ringqp.Poly arm of embedDouble (schemes/ckks/encoder.go:304-311): the Q part and the P part are the same values quantized modulo the Q
    and the P moduli, NTT domain and Montgomery form as NewLinearTransformation sets the flags"""
    name, setting = shape
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    level, levelP = d.levels[1], len(P) - 1
    log_slots = N.bit_length() - 2
    rnd = random.Random("embed " + name)
    values = np.array([complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(1 << log_slots)])
    scale = float(int(Q[level]))
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    poly = rh.rlwe.PolyQP(rh.DevicePoly(d.rq.AtLevel(level), 1, level + 1), rh.DevicePoly(d.rp.AtLevel(levelP), 1, levelP + 1))
    ecd.Embed(values, Meta(scale, log_slots), poly)
    assert np.array_equal(poly.Q.numpy()[0], cer.embed(values, log_slots, scale, N, [int(q) for q in Q[:level + 1]], True, True))
    assert np.array_equal(poly.P.numpy()[0], cer.embed(values, log_slots, scale, N, [int(p) for p in P], True, True))
    pt = ecd.NewPlaintext(level, scale)                                  # a DevicePoly is encoded as before
    ecd.Embed(values, pt, pt.Value[0])
    assert np.array_equal(pt.Value[0].numpy()[0], cer.embed(values, log_slots, scale, N, [int(q) for q in Q[:level + 1]], True, False))
    plain = rh.ckks.Encoder(d.rq)
    with pytest.raises(rh.RingHipError, match="polyOut is a ringqp.Poly but the encoder was built without ringP"):
        plain.Embed(values, Meta(scale, log_slots), poly)
    ecd.close(); plain.close(); d.close()


def transformation(rh, d, ecd, diags, level, ratio, scale=None):
    """(package transformation, restated transformation) of the same diagonals"""
    N, Q, P = d.N, d.Q, d.P
    log_slots = N.bit_length() - 2
    levelP = len(P) - 1
    scale = int(Q[level]) if scale is None else scale
    params = rh.lintrans.Parameters(list(diags), level, levelP, scale, log_slots, ratio)
    lt = rh.lintrans.NewTransformation(d.rq, d.rp, params)
    rh.lintrans.Encode(ecd, rh.lintrans.Diagonals(diags), lt)
    return lt, ltr.encode(N, Q, P, diags, list(diags), level, levelP, scale, log_slots, ratio)


CASES = {"TAIL": SMALL_DIAGS, "REF": REF_DIAGS, "Q61N13": REF_DIAGS}


@pytest.mark.parametrize("ratio", [1, -1], ids=["bsgs", "naive"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=_ids)
def test_encode_matches_the_restatement(rh, shape, ratio):
    name, setting = shape
    d = Device(rh, name, setting)
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    slots = d.N >> 1
    diags = make_diagonals(name, CASES[name], slots)
    lt, want = transformation(rh, d, ecd, diags, d.levels[0], ratio)
    assert lt.N1 == want.N1 and sorted(lt.Vec) == sorted(want.Vec) and (lt.N1 == 0) == (ratio < 0)
    for k in want.Vec:
        assert np.array_equal(lt.Vec[k].Q.numpy()[0], want.Vec[k][0]) and np.array_equal(lt.Vec[k].P.numpy()[0], want.Vec[k][1]), k
    assert lt.IsNTT and lt.IsMontgomery and lt.IsBatched and lt.Scale.Value == int(d.Q[d.levels[0]])
    assert sorted(lt.GaloisElements(d.N)) == ltr.galois_elements(d.N, list(diags), slots, ratio)
    ecd.close(); d.close()


# ---- Evaluate -----------------------------------------------------------------------------------------------------------------------------------
LOG_SCALE = {"TAIL": 40, "REF": 30, "Q61N13": 45}                        # the scale the messages are encoded at, per chain


@functools.lru_cache(maxsize=None)
def messages(name, level, tag="m"):
    """B vectors of values in the box (NewTestVector(-1-1i, 1+1i)), encoded at 2^LOG_SCALE and encrypted under the chain's secret key"""
    N, Q, _, _ = t.chain(name)
    log_slots = N.bit_length() - 2
    mods = [int(q) for q in Q[:level + 1]]
    vals, cts = [], []
    for k in range(B):
        rnd = random.Random("lt values %s %s %d" % (name, tag, k))
        v = np.array([complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(1 << log_slots)])
        pt = cer.embed(v, log_slots, 2.0 ** LOG_SCALE[name], N, mods, True, False)
        ct, _ = rr.encrypt(random.Random("lt enc %s %s %d %d" % (name, tag, level, k)), t.secrets(name)[0], [0] * N, Q, level)
        vals.append(v)
        cts.append([rr._add(ct[0], pt, mods), ct[1]])
    return vals, cts


def host_keys(name, setting, galEls):
    return {g: t.key(name, setting, "galois", g) for g in galEls if g != 1}


def evaluator(rh, d, hk):
    ev = rh.ckks.Evaluator(d.rq, d.rp, galois_keys={g: d.gadget(k) for g, k in hk.items()})
    return ev, rh.lintrans.Evaluator(ev)


def check_precision(name, what, level, got, vals, diags, scale):
    """The reference's rule (VerifyTestVectors, schemes/ckks/precision.go:92-103): the average precision of the real and of the imaginary parts is
    at least log2(DefaultScale) - (LogN + 2) bits.  DefaultScale is the scale the messages are encoded at, 2^LOG_SCALE[chain] here, and LogN the
    chain's: 40 - 7 = 33 bits on TAIL, 30 - 12 = 18 on REF, 45 - 15 = 30 on Q61N13."""
    N, Q, _, _ = t.chain(name)
    log_slots = N.bit_length() - 2
    bound = LOG_SCALE[name] - (N.bit_length() - 1 + 2)
    for k in range(B):
        want = ltr.diagonals_evaluate(diags, [complex(v) for v in vals[k]])
        re, im = ltr.decrypt_slots(got[k], t.secrets(name)[0], N, Q, log_slots, scale)
        pr, pi = ltr.avg_log2_prec(want, re, im, LOG_SCALE[name])
        print("MEASURED gpu/lintrans %s %s level=%d poly=%d  real %.2f imag %.2f  [>= %d]" % (name, what, level, k, pr, pi, bound))
        assert pr >= bound and pi >= bound


EVAL = [(s, r) for s in SHAPES[:2] for r in (1, -1)] + [(SHAPES[2], 1)]


@pytest.mark.parametrize("shape,ratio", EVAL, ids=["%s-%s" % (s[0], "bsgs" if r >= 0 else "naive") for s, r in EVAL])
def test_evaluate(rh, oracle, shape, ratio):
    """fused and composed, bit for bit against the restatement: out of place at the top level and one below; opOut = ctIn; ctIn left alone; the
    scale and the metadata as the reference sets them; the fused output decrypts to Diagonals.Evaluate of the messages"""
    name, setting = shape
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    slots = N >> 1
    diags = make_diagonals(name, CASES[name], slots)
    hk = host_keys(name, setting, ltr.galois_elements(N, list(diags), slots, ratio))
    ev, lev = evaluator(rh, d, hk)
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    for level in d.levels[:2]:
        lt, rlt = transformation(rh, d, ecd, diags, level, ratio)
        vals, cts = messages(name, level)
        want = [ltr.evaluate_many(N, Q, P, c, [rlt], hk)[0] for c in cts]
        scale_out = cr.Scale(1 << LOG_SCALE[name]).mul(cr.Scale(int(Q[level])))
        for fused in (True, False):
            ct, out = d.ct(level, cts), d.new(level)
            ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << LOG_SCALE[name]), N.bit_length() - 2
            lev.Evaluate(ct, lt, out, fused=fused)
            got = host(out)
            assert same(got, want), (level, fused)
            assert out.IsNTT and same(host(ct), cts)                    # ctIn is left alone
            assert out.Scale.Value == scale_out.v and out.LogDimensions == ct.LogDimensions
            if fused:
                check_precision(name, "ratio=%d" % ratio, level, got, vals, diags, scale_out.float64())
            if level == d.levels[0]:
                lev.Evaluate(ct, lt, ct, fused=fused)                   # opOut = ctIn
                assert same(host(ct), want) and ct.Scale.Value == scale_out.v, ("in place", fused)
        new = lev.EvaluateNew(_scaled(rh, d, level, cts, name), lt)
        assert same(host(new), want) and new.Level() == level
    ecd.close(); ev.close(); d.close()


def _scaled(rh, d, level, cts, name):
    ct = d.ct(level, cts)
    ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << LOG_SCALE[name]), d.N.bit_length() - 2
    return ct


@pytest.mark.parametrize("ratio", [1, -1], ids=["bsgs", "naive"])
def test_transformation_below_the_ciphertext_level(rh, oracle, ratio):
    """lt.LevelQ below ctIn.Level() with a batch of 3: ctIn is first brought to levelQ in BuffCt (CopyLvl, lintrans_evaluator.go:165, :281), device
    blocks being strided by level + 1 rows per poly; opOut, allocated at ctIn's level, is resized to levelQ"""
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    slots = N >> 1
    diags = make_diagonals(name, CASES[name], slots)
    hk = host_keys(name, setting, ltr.galois_elements(N, list(diags), slots, ratio))
    ev, lev = evaluator(rh, d, hk)
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    top, low = d.levels[0], d.levels[1]
    lt, rlt = transformation(rh, d, ecd, diags, low, ratio)
    vals, cts = messages(name, top)
    want = [ltr.evaluate_many(N, Q, P, c, [rlt], hk)[0] for c in cts]
    for fused in (True, False):
        ct, out = _scaled(rh, d, top, cts, name), d.new(top)
        lev.Evaluate(ct, lt, out, fused=fused)
        assert out.Level() == low and same(host(out), want), fused
        assert ct.Level() == top and same(host(ct), cts)
        lev.Evaluate(ct, lt, ct, fused=fused)                           # in place: ctIn itself is resized
        assert ct.Level() == low and same(host(ct), want)
    check_precision(name, "below ratio=%d" % ratio, low, host(out), vals, diags, cr.Scale(1 << LOG_SCALE[name]).mul(cr.Scale(int(Q[low]))).float64())
    ecd.close(); ev.close(); d.close()


# ---- EvaluateMany, EvaluateSequential -----------------------------------------------------------------------------------------------------------
def test_evaluate_many_reuses_and_prunes_the_pre_rotations(rh, oracle):
    """two BSGS transformations that share baby steps: SMALL_DIAGS at ratio 1 (N1 = 4: baby steps 1, 2, 3) and [0, 1, 5, 9] (N1 = 8: baby steps 1, 5):
    the second keeps 1, drops 2 and 3 and computes 5 alone"""
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    slots = N >> 1
    level = d.levels[0]
    da, db = make_diagonals(name + "a", SMALL_DIAGS, slots), make_diagonals(name + "b", [0, 1, 5, 9], slots)
    galEls = set(ltr.galois_elements(N, list(da), slots, 1)) | set(ltr.galois_elements(N, list(db), slots, 1))
    hk = host_keys(name, setting, galEls)
    ev, lev = evaluator(rh, d, hk)
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    (lta, rlta), (ltb, rltb) = transformation(rh, d, ecd, da, level, 1), transformation(rh, d, ecd, db, level, 1)
    assert (lta.N1, ltb.N1) == (4, 8)
    vals, cts = messages(name, level)
    used = []
    want = [ltr.evaluate_many(N, Q, P, c, [rlta, rltb], hk, used if k == 0 else None) for k, c in enumerate(cts)]
    assert used == [([1, 2, 3], [1, 2, 3]), ([5], [1, 5])]
    calls = []
    pre = lev.PreRotatedCiphertextForDiagonalMatrixMultiplication

    def spy(levelQ, levelP, ctIn, dec, rots, ctPreRot):
        before = set(ctPreRot)
        pre(levelQ, levelP, ctIn, dec, rots, ctPreRot)
        calls.append((sorted(set(ctPreRot) - before), sorted(ctPreRot)))
    lev.PreRotatedCiphertextForDiagonalMatrixMultiplication = spy
    for fused in (True, False):
        del calls[:]
        ct = _scaled(rh, d, level, cts, name)
        outs = lev.EvaluateManyNew(ct, [lta, ltb], fused=fused)
        assert calls == [([1, 2, 3], [1, 2, 3]), ([5], [1, 5])]        # computed by each call, and the map after it
        for i in (0, 1):
            assert same(host(outs[i]), [w[i] for w in want]), (fused, i)
    ecd.close(); ev.close(); d.close()


def test_evaluate_sequential(rh, oracle):
    """M1(M0(ct)) with the Rescale after each (lintrans_evaluator.go:102-124): the second transformation is encoded one level below"""
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    slots = N >> 1
    top = d.levels[0]
    da, db = make_diagonals(name + "s0", SMALL_DIAGS, slots), make_diagonals(name + "s1", [0, 1, 5, 9], slots)
    hk = host_keys(name, setting, set(ltr.galois_elements(N, list(da), slots, 1)) | set(ltr.galois_elements(N, list(db), slots, -1)))
    ev, lev = evaluator(rh, d, hk)
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    (lta, rlta), (ltb, rltb) = transformation(rh, d, ecd, da, top, 1), transformation(rh, d, ecd, db, top - 1, -1)
    vals, cts = messages(name, top)
    want = [ltr.evaluate_sequential(N, Q, P, c, 1 << LOG_SCALE[name], [rlta, rltb], hk) for c in cts]
    for fused in (True, False):
        out = lev.EvaluateSequentialNew(_scaled(rh, d, top, cts, name), [lta, ltb], fused=fused)
        assert out.Level() == top - 2 and same(host(out), [w[0] for w in want]), fused
        assert out.Scale.Value == want[0][1].v
    ecd.close(); ev.close(); d.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rh, oracle):
    from conftest import QI60, PI60
    from oracle import primes
    E = rh.RingHipError
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    slots = N >> 1
    top = d.levels[0]
    diags = make_diagonals(name, SMALL_DIAGS, slots)
    galEls = ltr.galois_elements(N, list(diags), slots, 1)
    hk = host_keys(name, setting, galEls)
    ev, lev = evaluator(rh, d, hk)
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    lt, _ = transformation(rh, d, ecd, diags, top, 1)
    vals, cts = messages(name, top)
    ct, out = _scaled(rh, d, top, cts, name), d.new(top)
    with pytest.raises(E, match="output \\*rlwe.Ciphertext slice is too small"):
        lev.EvaluateMany(ct, [lt, lt], [out])
    with pytest.raises(E, match="coefficient-domain ciphertexts are not supported"):
        lev.Evaluate(d.ct(top, cts, is_ntt=False), lt, out)
    one = rh.Ciphertext([d.rq.AtLevel(top).NewPoly(1) for _ in (0, 1)], is_ntt=True)
    with pytest.raises(E, match="hold different numbers of ciphertexts"):
        lev.Evaluate(ct, lt, one)
    # all transformations share one LevelP
    lt1 = rh.lintrans.NewTransformation(d.rq, d.rp, rh.lintrans.Parameters(list(diags), top, len(P) - 2, int(Q[top]), N.bit_length() - 2, 1))
    with pytest.raises(E, match="all linearTransformations must have the same levelP"):
        lev.EvaluateMany(ct, [lt, lt1], [out, d.new(top)])
    # a key with another LevelP than the transformation's: the reference's own message
    with pytest.raises(E, match=r"LinearTransformation.LevelP = %d != GaloiKey\[\d+\].LevelP\(\) = %d" % (len(P) - 2, len(P) - 1)):
        lev.Evaluate(ct, lt1, out)
    # a missing key, found before the first launch: opOut keeps its values
    marks = [rr.uniform_poly(random.Random("mark %d" % k), N, Q[:top + 1]) for k in range(B)]
    gone = [g for g in galEls if g != 1][-1]
    saved = ev.ks.galois_keys.pop(gone)
    out = d.ct(top, [[m, m] for m in marks])
    with pytest.raises(E, match=r"GaloisKey\[%d\] is missing" % gone):
        lev.Evaluate(ct, lt, out)
    assert same(host(out), [[m, m] for m in marks])
    ev.ks.galois_keys[gone] = saved
    # Encode onto a diagonal that was not allocated, with and without BSGS
    more = dict(diags)
    more[6] = diags[0]
    rh.lintrans.Encode(ecd, rh.lintrans.Diagonals(more), lt)           # BSGS walks the ALLOCATED index (:244-252): a diagonal outside it is not read
    assert 6 not in lt.Vec
    fewer = {k: v for k, v in diags.items() if k != 7}
    with pytest.raises(E, match=r"cannot Encode: cannot At\[7 or -9\]: diagonal does not exist"):
        rh.lintrans.Encode(ecd, rh.lintrans.Diagonals(fewer), lt)       # ... and an allocated one that is not given fails in At (:256-258)
    ltn = rh.lintrans.NewTransformation(d.rq, d.rp, rh.lintrans.Parameters(list(diags), top, len(P) - 1, int(Q[top]), N.bit_length() - 2, -1))
    with pytest.raises(E, match=r"plaintext diagonal \[6\] does not exist"):
        rh.lintrans.Encode(ecd, rh.lintrans.Diagonals(more), ltn)
    # encoder precision above 53: such an encoder cannot be built on the device path, and Encode asks the encoder it is given
    with pytest.raises(E, match="prec = 64 > 53"):
        rh.ckks.Encoder(d.rq, precision=64, ringP=d.rp)

    class Big:
        def Prec(self):
            return 64
    with pytest.raises(E, match="encoder precision 64 > 53"):
        rh.lintrans.Encode(Big(), rh.lintrans.Diagonals(diags), lt)
    # the kernels' own argument checks
    L = rh.lib()
    be, levelP = d.ev.be._h, len(P) - 1
    rql, rpl = d.rq.AtLevel(top), d.rp.AtLevel(levelP)
    q = [rql.NewPoly(B) for _ in range(5)]
    p = [rpl.NewPoly(B) for _ in range(5)]
    args = lambda g, acc0: (be, top, levelP, g, q[0].ptr, q[1].ptr, p[0].ptr, p[1].ptr, q[2].ptr, p[2].ptr, acc0, q[4].ptr, p[3].ptr, p[4].ptr, B, 1)
    assert L.rh_rlwe_rotate_sum_accumulate_qp(*args(4, q[3].ptr)) == -1 and b"must be odd" in L.rh_last_error()
    assert L.rh_rlwe_rotate_sum_accumulate_qp(*args(5, q[0].ptr)) == -1 and b"rh_rlwe_rotate_sum_accumulate_qp: the accumulator cannot overlap cQP or tmp0" in L.rh_last_error()
    assert L.rh_rlwe_rotate_sum_accumulate_qp(*args(5, q[2].ptr)) == -1 and b"the accumulator cannot overlap cQP or tmp0" in L.rh_last_error()
    assert L.rh_rlwe_rotate_sum_accumulate_qp(be, top + 1, levelP, 5, *([q[0].ptr] * 10), B, 1) == -1 and b"need 0 <= levelQ" in L.rh_last_error()
    v = lt.Vec[sorted(lt.Vec)[0]]
    margs = lambda acc0: (be, top, levelP, 5, v.Q.ptr, v.P.ptr, q[2].ptr, q[0].ptr, q[1].ptr, p[0].ptr, p[1].ptr, acc0, q[4].ptr, p[2].ptr, p[3].ptr, B, 1)
    assert L.rh_rlwe_rotate_mul_accumulate_qp(*margs(q[2].ptr)) == -1 and b"rh_rlwe_rotate_mul_accumulate_qp: the accumulator cannot overlap cQP, ct0 or the diagonal" in L.rh_last_error()
    assert L.rh_rlwe_rotate_mul_accumulate_qp(*margs(None)) == -1 and b"null argument" in L.rh_last_error()
    table = rh.DevicePoly(d.rq.AtLevel(0), 1, 1)
    outs = [q[3], q[4], p[2], p[3]]
    assert diag_mac(rh, d, top, levelP, [(v.Q, v.P)], [(q[0], q[1], p[0], p[1])], [q[0], q[4], p[2], p[3]], table) == -1
    assert b"rh_rlwe_diag_mac_qp: an output (or the table) overlaps a term" in L.rh_last_error()
    import ctypes as C
    one_ptr = lambda x: (C.c_void_p * 1)(x)
    four = (C.c_void_p * 4)(q[0].ptr, q[1].ptr, p[0].ptr, p[1].ptr)
    assert L.rh_rlwe_diag_mac_qp(be, top, levelP, 1, one_ptr(v.Q.ptr), one_ptr(v.P.ptr), four, *[o.ptr for o in outs], B, table.ptr, 5) == -1
    assert b"the table holds 5 words, 1 terms need 6" in L.rh_last_error()
    assert L.rh_rlwe_diag_mac_qp(be, top, levelP, 1, one_ptr(v.Q.ptr), one_ptr(v.P.ptr), four, *[o.ptr for o in outs], B, None, 0) == -1
    assert b"null table" in L.rh_last_error()
    ecd.close(); ev.close(); d.close()
    # keys with a power-of-two decomposition, and keys with one P modulus
    for setting1, text in (((16, 1), "method is unsupported for BaseTwoDecomposition != 0"), ((0, 1), "one P modulus")):
        d1 = Device(rh, name, setting1)
        ev1, lev1 = evaluator(rh, d1, host_keys(name, setting1, galEls))
        ecd1 = rh.ckks.Encoder(d1.rq, ringP=d1.rp)
        lt1, _ = transformation(rh, d1, ecd1, diags, top, 1)
        with pytest.raises(E, match=text):
            lev1.Evaluate(_scaled(rh, d1, top, cts, name), lt1, d1.new(top))
        ecd1.close(); ev1.close(); d1.close()
    # conjugate-invariant and 3N rings
    for rq, rp in ((rh.Ring(32, QI60[:2], kind=rh.ConjugateInvariant), rh.Ring(32, PI60[:2], kind=rh.ConjugateInvariant)),
                   tuple(rh.Ring(3 << 6, m, kind=rh.Matrix3N) for m in primes.gen_moduli_3n(3 << 6, [60, 60], [60, 60]))):
        cev = rh.ckks.Evaluator(rq, rp)
        with pytest.raises(E, match="conjugate-invariant and 3N rings are not supported"):
            rh.lintrans.Evaluator(cev)
        a = [rq.NewPoly(1) for _ in range(4)]
        b = [rp.NewPoly(1) for _ in range(4)]
        rc = L.rh_rlwe_rotate_sum_accumulate_qp(cev.ks.be._h, 1, 1, 5, a[0].ptr, a[1].ptr, b[0].ptr, b[1].ptr, a[0].ptr, b[0].ptr, a[2].ptr, a[3].ptr, b[2].ptr, b[3].ptr, 1, 1)
        assert rc == -5 and b"standard rings only" in L.rh_last_error()
        cev.close(); rq.close(); rp.close()

"""GPU: sums of rotations on the device (core/rlwe/inner_sum.go and its scheme wrappers).  The two kernels of csrc/inner_sum.hip against numpy, whole
arrays, bit for bit; rlwe.Evaluator.PartialTracesSum -- fused, composed and as one C-ABI call -- against the restatement that
tests/test_inner_sum_oracle.py pins to decryption (tests/inner_sum_restatement.py), with that file's keys and ciphertexts, and by decrypting the
device output on the host within the reference's bound (core/rlwe/rlwe_test.go:1090-1136); Replicate, Trace, InnerFunction and the ckks / bgv
wrappers; every refusal by its text.

Shapes: TAIL (N = 32: a row inside one wavefront, a last digit of 3 limbs), REF (N = 2^10, mixed-width limbs), Q61N13 (N = 2^13: more than one
block per row) for the reference's own case (5, 7) only; batches of 3 ciphertexts (a ragged grid tail); the top level and one below."""
import random

import numpy as np
import pytest

import ckks_restatement as cr
import inner_sum_restatement as isr
import rlwe_restatement as rr
import test_inner_sum_oracle as so
import test_rlwe_oracle as t
from test_gpu_rlwe_decrypt import B, Device, host, same

pytestmark = pytest.mark.gpu
_ids = t._ids
SHAPES = so.SHAPES
BIG = ("Q61N13", (0, 2))
TAGS = ["sum", "sum1", "sum2"]                                          # poly 0: the CPU file's own ciphertext


def uniform(tag, N, mods, count=B):
    return [rr.uniform_poly(random.Random("%s %d" % (tag, k)), N, mods) for k in range(count)]


def keys_on(d, galEls):
    return {g: d.gadget(t.key(d.name, d.setting, "galois", g)) for g in galEls if g != 1}


# ---- the kernels ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt_streams", [1, 2], ids=["nt-by-size", "nt-always"])
@pytest.mark.parametrize("shape", SHAPES + [BIG], ids=_ids)
def test_kernels_against_numpy(rh, shape, nt_streams):
    """rh_rlwe_rotate_accumulate_qp and rh_rlwe_rotate_add_q for g = 5, 5^-1, 25 and 2N - 1: acc written (first) and added to, both components, Q and P rows,
    against acc + tmp[index] + (P mod q) ct0[index] over Python integers with the reference's index table; the inputs are left alone.
    nt_streams = 2: the non-temporal arm of the streamed operand, which these sizes do not reach by themselves"""
    name, setting = shape
    d = Device(rh, name, setting)
    d.rq.set_tuning("nt_streams", nt_streams)
    N, Q, P = d.N, d.Q, d.P
    levelP = len(P) - 1
    Pb = rr.prod(P)
    for level in d.levels[:2]:
        mods = [int(q) for q in Q[:level + 1]]
        pm = [int(p) for p in P]
        rql, rpl = d.rq.AtLevel(level), d.rp.AtLevel(levelP)
        up = lambda ring, arrs: rh.DevicePoly.from_numpy(ring, np.stack(arrs))
        tq, tp = [uniform("tq%d %s %d" % (c, name, level), N, mods) for c in (0, 1)], [uniform("tp%d %s" % (c, name), N, pm) for c in (0, 1)]
        aq, ap = [uniform("aq%d %s %d" % (c, name, level), N, mods) for c in (0, 1)], [uniform("ap%d %s" % (c, name), N, pm) for c in (0, 1)]
        c0 = uniform("c0 %s %d" % (name, level), N, mods)
        tmp = rh.rlwe.ElementQP([rh.rlwe.PolyQP(up(rql, tq[c]), up(rpl, tp[c])) for c in (0, 1)])
        dc0 = up(rql, c0)
        for g in (5, pow(5, -1, 2 * N), 25, 2 * N - 1):
            idx = rh.AutomorphismNTTIndex(N, 2 * N, g).astype(np.int64)
            for first in (True, False):
                acc = rh.rlwe.ElementQP([rh.rlwe.PolyQP(up(rql, aq[c]), up(rpl, ap[c])) for c in (0, 1)])
                d.ev.RotateAccumulateQP(level, g, dc0, tmp, acc, first)
                for c in (0, 1):
                    for part, mm, tt, aa in (("Q", mods, tq[c], aq[c]), ("P", pm, tp[c], ap[c])):
                        got = getattr(acc.Value[c], part).numpy()
                        for k in range(B):
                            for i, q in enumerate(mm):
                                want = tt[k][i][idx] if first else (tt[k][i][idx] + aa[k][i]) % np.uint64(q)
                                if part == "Q" and c == 0:
                                    want = ((want.astype(object) + c0[k][i][idx].astype(object) * (Pb % q)) % q).astype(np.uint64)
                                assert np.array_equal(got[k, i], want), (level, g, first, c, part, k, i)
            ct = Ciphertext2(rh, [up(rql, aq[c]) for c in (0, 1)])
            d.ev.RotateAddQ(level, g, Ciphertext2(rh, [tmp.Value[c].Q for c in (0, 1)]), ct)
            for c in (0, 1):
                got = ct.Value[c].numpy()
                for k in range(B):
                    for i, q in enumerate(mods):
                        assert np.array_equal(got[k, i], (aq[c][k][i] + tq[c][k][i][idx]) % np.uint64(q)), (level, g, c, k, i)
        for c in (0, 1):                                                 # the permuted operands are read only
            assert np.array_equal(tmp.Value[c].Q.numpy(), np.stack(tq[c])) and np.array_equal(tmp.Value[c].P.numpy(), np.stack(tp[c]))
        assert np.array_equal(dc0.numpy(), np.stack(c0))
    d.close()


def Ciphertext2(rh, polys):
    return rh.Ciphertext(list(polys), is_ntt=True)


# ---- PartialTracesSum -------------------------------------------------------------------------------------------------------------------------
def batch(name, setting, level, offset, n):
    cases = [so.sum_case(name, setting, level, offset, n, tag) for tag in TAGS]
    return [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases]


def check_decrypts(name, level, got, msgs, offset, n):
    N = t.chain(name)[0]
    for k in range(B):
        err = so.sum_error(name, level, got[k], so.summed(msgs[k], N, offset, n))
        print("MEASURED gpu/partialtraces %s level=%d (%d, %d) poly=%d  %.2f [%.2f]" % (name, level, offset, n, k, err, t.bound(N, 0)))
        assert err <= t.bound(N, 0)


PTS = [(s, c) for s in SHAPES for c in so.CASES] + [(BIG, (5, 7))]


@pytest.mark.parametrize("shape,case", PTS, ids=["%s-off%d-n%d" % (s[0], c[0], c[1]) for s, c in PTS])
def test_partial_traces_sum(rh, oracle, shape, case):
    """fused and composed, bit for bit against the restatement: out of place at the top level and one below; in place, and from the coefficient
    domain, at the top level; the device output decrypts to the sum of the rotated messages"""
    name, setting = shape
    offset, n = case
    d = Device(rh, name, setting)
    N, Q = d.N, d.Q
    d.ev.galois_keys = keys_on(d, so.case_elements(N, offset, n))
    for level in d.levels[:2]:
        mods = Q[:level + 1]
        msgs, cts, want = batch(name, setting, level, offset, n)
        for fused in (True, False):
            ct, out = d.ct(level, cts), d.new(level)
            d.ev.PartialTracesSum(ct, offset, n, out, fused=fused)
            got = host(out)
            assert same(got, want), (level, fused)
            assert out.IsNTT and same(host(ct), cts)                    # ctIn is left alone
            if fused:
                check_decrypts(name, level, got, msgs, offset, n)
            if level != d.levels[0]:
                continue
            d.ev.PartialTracesSum(ct, offset, n, ct, fused=fused)       # opOut = ctIn
            assert same(host(ct), want), ("in place", fused)
            coeff = [[rr.intt(x, N, mods) for x in c] for c in cts]
            ctc, outc = d.ct(level, coeff, is_ntt=False), d.new(level)
            d.ev.PartialTracesSum(ctc, offset, n, outc, fused=fused)
            assert not outc.IsNTT and same(host(ctc), coeff)
            assert same(host(outc), [[rr.intt(x, N, mods) for x in w] for w in want]), ("coefficient domain", fused)
        if level == d.levels[0]:
            d.ev.PartialTracesSum(ctc, offset, n, ctc)                  # coefficient domain, in place, the default path
            assert not ctc.IsNTT and same(host(ctc), host(outc))
    d.close()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_partial_traces_sum_of_one_copies(rh, oracle, shape):
    name, setting = shape
    d = Device(rh, name, setting)
    level = d.levels[0]
    mods = d.Q[:level + 1]
    cts = [t.fresh(name, tag, level)[1] for tag in TAGS]
    ct, out = d.ct(level, cts), d.new(level)
    ct.Scale = 12345
    d.ev.PartialTracesSum(ct, 3, 1, out)                                # no key is needed
    assert same(host(out), cts) and out.IsNTT and out.Scale == 12345    # the metadata is ctIn's
    d.ev.PartialTracesSum(ct, 3, 1, ct)
    assert same(host(ct), cts)
    # coefficient domain: the reference copies and then applies INTT to the copy (inner_sum.go:188-192, :285-288); so does the device path
    ctc, outc = d.ct(level, cts, is_ntt=False), d.new(level)
    d.ev.PartialTracesSum(ctc, 3, 1, outc)
    assert not outc.IsNTT and same(host(outc), [[rr.intt(x, d.N, mods) for x in c] for c in cts])
    d.close()


def test_partial_traces_sum_c_abi(rh, oracle):
    """rh_rlwe_partial_traces_sum: the whole sequence as ONE library call with the caller's key table equals the Python orchestration"""
    name, setting = SHAPES[1]
    offset, n = 5, 7
    d = Device(rh, name, setting)
    d.ev.galois_keys = keys_on(d, so.case_elements(d.N, offset, n))
    level = d.levels[0]
    mods = d.Q[:level + 1]
    _, cts, want = batch(name, setting, level, offset, n)
    for fused in (True, False):
        ct, out = d.ct(level, cts), d.new(level)
        d.ev.PartialTracesSumC(ct, offset, n, out, fused=fused)
        assert same(host(out), want) and same(host(ct), cts), fused
    d.ev.PartialTracesSumC(ct, offset, n, ct)
    assert same(host(ct), want)
    coeff = [[rr.intt(x, d.N, mods) for x in c] for c in cts]
    ctc, outc = d.ct(level, coeff, is_ntt=False), d.new(level)
    d.ev.PartialTracesSumC(ctc, offset, n, outc)
    assert not outc.IsNTT and same(host(outc), [[rr.intt(x, d.N, mods) for x in w] for w in want])
    one = d.new(level)
    d.ev.PartialTracesSumC(d.ct(level, cts), 3, 1, one)
    assert same(host(one), cts)
    L = rh.lib()
    args = (d.ev.be._h, level, len(d.P) - 1, ct.Value[0].ptr, ct.Value[1].ptr, 1)
    assert L.rh_rlwe_partial_traces_sum(*args, 5, 0, None, 0, out.Value[0].ptr, out.Value[1].ptr, B, 1) == -1 and b"partialtrace: invalid parameter" in L.rh_last_error()
    assert L.rh_rlwe_partial_traces_sum(*args, 5, 7, None, 0, out.Value[0].ptr, out.Value[1].ptr, B, 1) == -1
    assert b"GaloisKey[%d] is missing" % so.case_elements(d.N, 5, 7)[0] in L.rh_last_error()
    d.close()


# ---- Replicate, Trace, InnerFunction ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_replicate_trace_inner_function(rh, oracle, shape):
    name, setting = shape
    d = Device(rh, name, setting)
    N, Q = d.N, d.Q
    level = d.levels[0]
    logN = so.trace_log(name)
    galEls = so.case_elements(N, -1, 3) + isr.galois_elements_for_trace(N, logN) + so.case_elements(N, 5, 7) + so.case_elements(N, 1, 8)
    d.ev.galois_keys = keys_on(d, set(galEls))
    # Replicate(batch, n) = PartialTracesSum(-batch, n)
    msgs, cts, want = batch(name, setting, level, -1, 3)
    ct, out = d.ct(level, cts), d.new(level)
    d.ev.Replicate(ct, 1, 3, out)
    assert same(host(out), want)
    assert set(so.case_elements(N, -1, 3)) <= set(rh.rlwe.GaloisElementsForReplicate(N, 1, 3))
    # Trace
    cases = [so.trace_case(name, setting, level, logN, tag) for tag in TAGS]
    wantt = [c[2] for c in cases]
    for fused in (True, False):
        out = d.new(level)
        d.ev.Trace(ct, logN, out, fused=fused)
        got = host(out)
        assert same(got, wantt), fused
    for k in range(B):
        err = so.sum_error(name, level, got[k], isr.trace_coeffs(cases[k][0], N, logN))
        assert err <= t.bound(N, 0), (k, err)
    d.ev.Trace(ct, N.bit_length() - 2, out)                             # a gap of 1 copies
    assert same(host(out), cts)
    tin = d.ct(level, cts)
    d.ev.Trace(tin, logN, tin)                                          # in place
    assert same(host(tin), wantt)
    # InnerFunction with f = Add
    add = lambda a, b, c: [d.rq.AtLevel(level).vec_op("ADD", a.Value[i], b.Value[i], c.Value[i]) for i in (0, 1)]
    for offset, n in so.CASES[:2]:
        cases = [so.inner_function_case(name, setting, level, offset, n, tag) for tag in TAGS]
        out = d.new(level)
        d.ev.InnerFunction(ct, offset, n, add, out)
        got = host(out)
        assert same(got, [c[2] for c in cases]), (offset, n)
        check_decrypts(name, level, got, [c[0] for c in cases], offset, n)
    assert same(host(ct), cts)
    d.close()


# ---- scheme layers -----------------------------------------------------------------------------------------------------------------------------
def test_ckks_inner_sum_rotate_and_add_average(rh, oracle):
    name, setting = SHAPES[0]                                           # N = 32: 16 slots
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    level = d.levels[0]
    galEls = set(so.case_elements(N, 1, 8) + so.case_elements(N, 5, 7) + so.case_elements(N, 4, 4) + so.case_elements(N, -2, 3) + [cr.galois_element(N, 3)])
    hk = {g: t.key(name, setting, "galois", g) for g in galEls}
    ev = rh.ckks.Evaluator(d.rq, d.rp, galois_keys={g: d.gadget(k) for g, k in hk.items()})
    scale = rh.ckks.Scale(t.SA.v)
    for (offset, n), f in (((1, 8), ev.InnerSum), ((5, 7), ev.RotateAndAdd)):
        msgs, cts, want = batch(name, setting, level, offset, n)
        ct, out = d.ct(level, cts), d.new(level)
        ct.Scale = scale
        f(ct, offset, n, out)
        assert same(host(out), want) and out.Scale.Value == t.SA.v      # the scale is carried through unchanged
    f(ct, offset, n, ct)
    assert same(host(ct), want)
    cts = [t.fresh(name, tag, level)[1] for tag in TAGS]
    ct, out = d.ct(level, cts), d.new(level)
    ct.Scale = scale
    ev.Average(ct, 2, out)                                              # 16 slots, sub-vectors of 4: n = 4
    assert same(host(out), [isr.ckks_average(N, Q, P, c, 2, hk) for c in cts]) and out.Scale.Value == t.SA.v and same(host(ct), cts)
    ev.Replicate(ct, 2, 3, out)
    assert same(host(out), [isr.partial_traces_sum(N, Q, P, c, -2, 3, hk) for c in cts])
    logN = so.trace_log(name)
    ev.ks.galois_keys.update(keys_on(d, isr.galois_elements_for_trace(N, logN)))
    tr = ev.TraceNew(ct, logN)
    assert same(host(tr), [so.trace_case(name, setting, level, logN, tag)[2] for tag in TAGS]) and tr.Scale.Value == t.SA.v
    # RotateHoistedLazyNew: modulo QP, divided by P it decrypts to the rotated message
    dec = ev.ks.DecomposeNTT(level, len(P) - 1, ct.Value[1], True)
    lazy = ev.RotateHoistedLazyNew(level, [0, 3], ct, dec)
    assert sorted(lazy) == [3]
    down = d.new(level)
    ev.ks.ModDown(level, len(P) - 1, lazy[3], down)
    for k, c in enumerate(host(down)):
        assert t.auto_error(name, level, c, t.fresh(name, TAGS[k], level)[0], cr.galois_element(N, 3)) <= t.bound(N, 0, level)
    E = rh.RingHipError
    with pytest.raises(E, match=r"innersum: invalid parameter \(n <= 0 or batchSize <= 0\)"):
        ev.InnerSum(ct, 0, 4, out)
    with pytest.raises(E, match=r"innersum: invalid parameters \(n\*batchSize=32 > #slots=16\)"):
        ev.InnerSum(ct, 4, 8, out)
    with pytest.raises(E, match=r"innersum: invalid parameters \(n\*batchSize=12 does not divide #slots=16\)"):
        ev.InnerSum(ct, 2, 6, out)
    ev.close()
    d.close()


def test_bgv_rotations_and_inner_sum(rh, oracle):
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, Q, P = d.N, d.Q, d.P
    level = d.levels[0]
    b, n = so.BGV_ROWS
    rows = 2 * N - 1
    galEls = set(so.case_elements(N, b, n // 2) + so.case_elements(N, 2, 8) + so.case_elements(N, 3, 5) + [5, rows])
    hk = {g: t.key(name, setting, "galois", g) for g in galEls}
    ev = rh.bgv.Evaluator(d.rq, t=65537, ringP=d.rp)
    ev.galois_keys.update({g: d.gadget(k) for g, k in hk.items()})
    cts = [t.fresh(name, tag, level)[1] for tag in TAGS]
    ct = d.ct(level, cts)
    ct.Scale = 3
    col, row = ev.RotateColumnsNew(ct, 1), ev.RotateRowsNew(ct)
    assert same(host(col), [rr.automorphism(N, Q, P, c, hk[5], 5) for c in cts]) and col.Scale == 3
    assert same(host(row), [rr.automorphism(N, Q, P, c, hk[rows], rows) for c in cts]) and row.Scale == 3
    out = d.new(level)
    ev.InnerSum(ct, 2, 8, out)                                          # n batchSize < N: PartialTracesSum
    assert same(host(out), [isr.partial_traces_sum(N, Q, P, c, 2, 8, hk) for c in cts]) and out.Scale == 3
    for fused in (True, False):
        out = d.new(level)
        ev.InnerSum(ct, b, n, out, fused=fused)                         # n batchSize = N: both rows
        got = host(out)
        assert same(got, [so.bgv_rows_case(name, setting, level, tag)[2] for tag in TAGS]) and out.Scale == 3
    for k in range(B):
        m = t.fresh(name, TAGS[k], level)[0]
        half = so.summed(m, N, b, n // 2)
        want = [x + y for x, y in zip(half, rr.automorphism_coeffs(half, rows))]
        assert so.sum_error(name, level, got[k], want) <= t.bound(N, 0) + 1
    ev.InnerSum(ct, N, 1, out)                                          # n = 1 over both rows: a copy
    assert same(host(out), cts)
    ev.RotateAndAdd(ct, 3, 5, out)
    assert same(host(out), [so.sum_case(name, setting, level, 3, 5, tag)[2] for tag in TAGS])
    dec = ev.DecomposeNTT(level, len(P) - 1, ct.Value[1], True)
    lazy = ev.RotateHoistedLazyNew(level, [1, 0], ct, dec)
    assert sorted(lazy) == [1]
    down = d.new(level)
    ev.ModDown(level, len(P) - 1, lazy[1], down)
    for k, c in enumerate(host(down)):
        assert t.auto_error(name, level, c, t.fresh(name, TAGS[k], level)[0], 5) <= t.bound(N, 0, level)
    E = rh.RingHipError
    with pytest.raises(E, match=r"innersum: invalid parameter \(n <= 0 or batchSize <= 0\)"):
        ev.InnerSum(ct, 4, 0, out)
    with pytest.raises(E, match=r"innersum: invalid parameters \(n\*batchSize=64 > #slots=32\)"):
        ev.InnerSum(ct, 8, 8, out)
    with pytest.raises(E, match=r"innersum: invalid parameters \(n\*batchSize=12 does not divide #slots=32\)"):
        ev.InnerSum(ct, 2, 6, out)
    ev.close()
    d.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rh, oracle):
    from oracle import primes
    E = rh.RingHipError
    name, setting = SHAPES[0]
    d = Device(rh, name, setting)
    N, level = d.N, d.levels[0]
    cts = [t.fresh(name, tag, level)[1] for tag in TAGS]
    ct, out = d.ct(level, cts), d.new(level)
    for offset, n in ((0, 4), (5, 0)):
        for f in (d.ev.PartialTracesSum, d.ev.PartialTracesSumC):
            with pytest.raises(E, match=r"partialtrace: invalid parameter \(n = 0 or batchSize = 0\)"):
                f(ct, offset, n, out)
    # a missing key: named, found before the first launch -- opOut keeps its values
    used = so.case_elements(N, 5, 7)
    d.ev.galois_keys = keys_on(d, used[:-1])
    marks = uniform("marks", N, d.Q[:level + 1])
    out = d.ct(level, [[m, m] for m in marks])
    for f in (d.ev.PartialTracesSum, d.ev.PartialTracesSumC):
        with pytest.raises(E, match=r"GaloisKey\[%d\] is missing" % used[-1]):
            f(ct, 5, 7, out)
        assert same(host(out), [[m, m] for m in marks])
    with pytest.raises(E, match=r"GaloisKey\[\d+\] is missing"):
        d.ev.Trace(ct, 0, out)
    d.ev.galois_keys = keys_on(d, used)
    # degree
    with pytest.raises(E, match=r"ctIn.Degree\(\) != 1 or opOut.Degree\(\) != 1"):
        d.ev.PartialTracesSum(d.new(level, degree=2), 5, 7, out)
    with pytest.raises(E, match=r"ctIn.Degree\(\) != 1 or opOut.Degree\(\) != 1"):
        d.ev.Trace(ct, 2, d.new(level, degree=2))
    # a batch allocated at another level
    with pytest.raises(E, match="allocate it at that level"):
        d.ev.PartialTracesSum(d.ct(level - 1, [t.fresh(name, tag, level - 1)[1] for tag in TAGS]), 5, 7, out)
    # the kernels' own argument checks
    L = rh.lib()
    p = ct.Value[0].ptr
    assert L.rh_rlwe_rotate_add_q(d.rq._h, level, 4, p, p, out.Value[0].ptr, out.Value[1].ptr, B) == -1 and b"must be odd" in L.rh_last_error()
    assert L.rh_rlwe_rotate_add_q(d.rq._h, level, 5, p, p, p, out.Value[1].ptr, B) == -1 and b"cannot be the ciphertext" in L.rh_last_error()
    d.close()
    # keys with a power-of-two decomposition, and keys with one P modulus
    for setting1, text in (((16, 1), "method is unsupported for BaseTwoDecomposition != 0"), ((0, 1), "one P modulus")):
        d1 = Device(rh, name, setting1)
        d1.ev.galois_keys = keys_on(d1, used)
        with pytest.raises(E, match=text):
            d1.ev.PartialTracesSum(d1.ct(level, cts), 5, 7, d1.new(level))
        d1.close()
    # conjugate-invariant and 3N rings
    from conftest import QI60, PI60
    for rq, rp in ((rh.Ring(32, QI60[:2], kind=rh.ConjugateInvariant), rh.Ring(32, PI60[:2], kind=rh.ConjugateInvariant)),
                   tuple(rh.Ring(3 << 6, m, kind=rh.Matrix3N) for m in primes.gen_moduli_3n(3 << 6, [60, 60], [60, 60]))):
        ev = rh.rlwe.Evaluator(rq, rp)
        new = lambda: rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
        for f in (lambda: ev.PartialTracesSum(new(), 1, 2, new()), lambda: ev.Trace(new(), 0, new()), lambda: ev.PartialTracesSumC(new(), 1, 2, new())):
            with pytest.raises(E, match="3N and conjugate-invariant rings are not supported"):
                f()
        a, b = new(), new()
        assert L.rh_rlwe_rotate_add_q(rq._h, 1, 5, a.Value[0].ptr, a.Value[1].ptr, b.Value[0].ptr, b.Value[1].ptr, 1) == -5 and b"standard rings only" in L.rh_last_error()
        ev.close(); rq.close(); rp.close()

"""GPU: ring packing on the device (core/rlwe/ring_packing.go).  The five kernels of csrc/ring_packing.hip against numpy, whole arrays, bit for bit, the
inputs left alone; rlwe.RingPackingEvaluator -- Expand (fused, composed, as one C-ABI call, and on a batch of 3), Pack, Split, Merge, Extract(Naive)
and Repack(Naive) -- against the restatement that tests/test_ring_packing_oracle.py pins to decryption (tests/ring_packing_restatement.py), with that
file's keys and ciphertexts, and by decrypting the device output on the host within the reference's bounds; every refusal by its text.

Kernel shapes: N = 16 (a row of 8 pairs, the half ring of TAIL), N = 32 (TAIL), N = 2^10 (REF, mixed-width limbs), N = 2^13 (Q61N13: more than one
block per row); 1, 2 and 3 ciphertexts (a ragged grid tail); the elements N + 1, 3, 2N - 1, 5 and 25; Pack tables that mix the three modes; the top
level and one below; nt_streams 1 and 2 (the non-temporal arm, which these sizes do not reach by themselves)."""
import ctypes as C

import numpy as np
import pytest

import ring_packing_restatement as rp
import rlwe_restatement as rr
import test_ring_packing_oracle as ro
import test_rlwe_oracle as t

pytestmark = pytest.mark.gpu
TAGS = ["rp", "rp1", "rp2"]                                             # poly 0: the CPU file's own ciphertext
KSHAPES = [("TAIL16", 16), ("TAIL", 32), ("REF", 1024), ("Q61N13", 8192)]


def chain_of(name):
    if name == "TAIL16":
        N, Q, P, levels = t.chain("TAIL")
        return 16, Q, P, levels
    return t.chain(name)


def uniform(rng, mods, N, count):
    return np.stack([np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in mods]) for _ in range(count)])


def mred(a, x, mods):
    """MRed(a, x) = a x 2^-64 mod q_i, canonical, on (..., limbs, N) arrays; x: (limbs, N)"""
    out = np.empty_like(a)
    for i, q in enumerate(mods):
        rinv = pow(1 << 64, -1, int(q))
        out[..., i, :] = ((a[..., i, :].astype(object) * x[i].astype(object) * rinv) % int(q)).astype(np.uint64)
    return out


def small_rows(p, M):
    """the leading (npoly, limbs, M) words of a block: rows of a smaller ring"""
    return p.numpy().reshape(-1)[:p.npoly * p.limbs * M].reshape(p.npoly, p.limbs, M)


def up_small(rh, rl, a):
    p = rh.DevicePoly(rl, a.shape[0], a.shape[1])
    assert rh.lib().rh_dev_upload(rl._h, p.ptr, np.ascontiguousarray(a).ctypes.data_as(rh.ringhip.U64P), a.size) == 0
    return p


def qcol(mods):
    return np.array([int(q) for q in mods], dtype=np.uint64)[:, None]


@pytest.mark.parametrize("nt_streams", [1, 2], ids=["nt-by-size", "nt-always"])
@pytest.mark.parametrize("shape", KSHAPES, ids=[s[0] for s in KSHAPES])
def test_kernels_against_numpy(rh, shape, nt_streams):
    name, N = shape
    _, Q, _, levels = chain_of(name)
    ring = rh.Ring(N, list(Q))
    ring.set_tuning("nt_streams", nt_streams)
    L = rh.lib()
    rng = np.random.default_rng(N + nt_streams)
    up = lambda rl, a: rh.DevicePoly.from_numpy(rl, a)
    gens = [N + 1, 3, 2 * N - 1, 5, 25]
    for level in levels[:2]:
        mods = [int(q) for q in Q[:level + 1]]
        q = qcol(mods)
        rl = ring.AtLevel(level)
        x = uniform(rng, mods, N, 1)[0]
        dx = up(rl, x[None])
        for cnt in (1, 2, 3):
            ct = [uniform(rng, mods, N, 2 * cnt) for _ in (0, 1)]
            tmp = [uniform(rng, mods, N, cnt) for _ in (0, 1)]
            dtmp = [up(rl, a) for a in tmp]
            for g in (gens if cnt == 3 or N <= 32 else gens[cnt - 1:cnt + 1]):
                idx = rh.AutomorphismNTTIndex(N, 2 * N, g).astype(np.int64)
                # one level of Expand
                d = [up(rl, a) for a in ct]
                assert L.rh_rlwe_expand_step(rl._h, level, g, dtmp[0].ptr, dtmp[1].ptr, d[0].ptr, d[1].ptr, dx.ptr, cnt) == 0, L.rh_last_error()
                for c in (0, 1):
                    tt, lo = tmp[c][:, :, idx], ct[c][:cnt]
                    want = np.concatenate([(lo + tt) % q, mred((lo + q - tt) % q, x, mods)])
                    assert np.array_equal(d[c].numpy(), want), ("expand_step", level, cnt, g, c)
                # one level of Pack: 2 cnt slots, a table that mixes the modes (a alone, b alone, both)
                nslots = 2 * cnt
                table = [(2, 0, 1)] if cnt == 1 else [(0, 1, 1), (1, 2, 2), (2, 3, 0)][:cnt] if cnt == 2 else [(2, 5, 0), (1, 3, 3), (0, 1, 1)]
                K = len(table)
                arr = np.array([v for e in table for v in e] + [0] * (K % 2 + 2), dtype=np.int32)
                dt = rh.DevicePoly(rl, 1, 1)
                assert L.rh_dev_upload(rl._h, dt.ptr, arr.view(np.uint64).ctypes.data_as(rh.ringhip.U64P), arr.size // 2) == 0
                th = arr.ctypes.data_as(C.POINTER(C.c_int32))
                d = [up(rl, a) for a in ct]
                u = [rl.NewPoly(K) for _ in (0, 1)]
                assert L.rh_rlwe_pack_combine(rl._h, level, d[0].ptr, d[1].ptr, nslots, dt.ptr, th, K, dx.ptr, u[0].ptr, u[1].ptr) == 0, L.rh_last_error()
                after = [a.copy() for a in ct]
                for c in (0, 1):
                    wu = np.empty((K, len(mods), N), dtype=np.uint64)
                    for k, (mode, sa, sb) in enumerate(table):
                        bx = mred(ct[c][sb], x, mods)
                        if mode == 0:
                            wu[k] = ct[c][sa]
                        elif mode == 1:
                            wu[k] = after[c][sb] = bx
                        else:
                            wu[k] = (ct[c][sa] + q - bx) % q
                            after[c][sa] = (ct[c][sa] + bx) % q
                    assert np.array_equal(u[c].numpy(), wu) and np.array_equal(d[c].numpy(), after[c]), ("pack_combine", level, cnt, g, c)
                dk = [up(rl, a[:K]) for a in tmp] if K <= cnt else [up(rl, uniform(rng, mods, N, K)) for _ in (0, 1)]
                tk = [p.numpy() for p in dk]
                assert L.rh_rlwe_rotate_addsub_q(rl._h, level, g, dk[0].ptr, dk[1].ptr, d[0].ptr, d[1].ptr, nslots, dt.ptr, th, K) == 0, L.rh_last_error()
                for c in (0, 1):
                    want = after[c].copy()
                    for k, (mode, sa, sb) in enumerate(table):
                        r = tk[c][k][:, idx]
                        if mode == 1:
                            want[sb] = (after[c][sb] + q - r) % q
                        else:
                            want[sa] = (after[c][sa] + r) % q
                    assert np.array_equal(d[c].numpy(), want), ("rotate_addsub_q", level, cnt, g, c)
                    assert np.array_equal(dk[c].numpy(), tk[c])
            for c in (0, 1):                                            # the permuted operand and the table are read only
                assert np.array_equal(dtmp[c].numpy(), tmp[c])
            assert np.array_equal(dx.numpy()[0], x)
            # the coefficient maps between N and N / gap, gap = 2 (Split, Merge) and 4 (the strided forms)
            for lg in (1, 2):
                M = N >> lg
                src = [a[:cnt] for a in ct]
                din = [up(rl, a) for a in src]
                ev, od, ev2 = [[rl.NewPoly(cnt) for _ in (0, 1)] for _ in range(3)]      # rows of the small ring, in blocks with room to spare
                assert L.rh_rlwe_ring_split(rl._h, level, din[0].ptr, din[1].ptr, ev[0].ptr, ev[1].ptr, od[0].ptr, od[1].ptr, lg, cnt) == 0, L.rh_last_error()
                assert L.rh_rlwe_ring_split(rl._h, level, din[0].ptr, din[1].ptr, ev2[0].ptr, ev2[1].ptr, None, None, lg, cnt) == 0
                for c in (0, 1):
                    assert np.array_equal(small_rows(ev[c], M), src[c][:, :, 0::1 << lg]) and np.array_equal(small_rows(od[c], M), src[c][:, :, 1::1 << lg]), ("split", lg, c)
                    assert np.array_equal(small_rows(ev2[c], M), src[c][:, :, 0::1 << lg]) and np.array_equal(din[c].numpy(), src[c])
                e = [np.ascontiguousarray(a[:cnt, :, :M]) for a in ct]
                o = [np.ascontiguousarray(a[cnt:2 * cnt, :, :M]) for a in ct]
                de, do = [up_small(rh, rl, a) for a in e], [up_small(rh, rl, a) for a in o]
                out = [rl.NewPoly(cnt) for _ in (0, 1)]
                rep = lambda a: np.repeat(a, 1 << lg, axis=2)
                assert L.rh_rlwe_ring_merge(rl._h, level, de[0].ptr, de[1].ptr, do[0].ptr, do[1].ptr, dx.ptr, out[0].ptr, out[1].ptr, lg, cnt) == 0, L.rh_last_error()
                for c in (0, 1):
                    assert np.array_equal(out[c].numpy(), (rep(e[c]) + mred(rep(o[c]), x, mods)) % q), ("merge", lg, c)
                assert L.rh_rlwe_ring_merge(rl._h, level, de[0].ptr, de[1].ptr, None, None, None, out[0].ptr, out[1].ptr, lg, cnt) == 0
                assert all(np.array_equal(out[c].numpy(), rep(e[c])) for c in (0, 1))
                assert all(np.array_equal(small_rows(de[c], M), e[c]) and np.array_equal(small_rows(do[c], M), o[c]) for c in (0, 1))
    ring.close()


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------------
class Device:
    """the rings of every degree of one (chain, setting), the evaluator and the uploaded keys"""

    def __init__(self, rh, name, setting, min_logN=None, extract=False, repack=False, switching=False):
        self.rh, self.name, self.setting = rh, name, setting
        self.N, self.Q, self.P, self.levels = ro.settings(name, setting)
        self.logN = ro.log_n(self.N)
        self.min_logN = self.logN if min_logN is None else min_logN
        self.rings = {}
        for lg in range(self.min_logN, self.logN + 1):
            self.rings[lg] = (rh.Ring(1 << lg, list(self.Q)), rh.Ring(1 << lg, list(self.P)) if self.P else None)
        gal = lambda lg, els: {g: self.gadget(lg, ro.galois_key(name, setting, lg, g)) for g in els}
        n = 1 << self.min_logN
        ek = {self.min_logN: gal(self.min_logN, rp.galois_elements_for_expand(n, self.min_logN))} if extract else None
        rk = {self.min_logN: gal(self.min_logN, rp.galois_elements_for_pack(n, self.min_logN))} if repack else None
        sw = None
        if switching:
            sw = {lg: {} for lg in self.rings}
            for lg in range(self.min_logN, self.logN):
                sw[lg][lg + 1] = self.gadget(lg + 1, ro.switching_key(name, setting, lg, lg + 1))
                sw[lg + 1][lg] = self.gadget(lg + 1, ro.switching_key(name, setting, lg + 1, lg))
        self.ev = rh.rlwe.RingPackingEvaluator(self.rings, RingSwitchingKeys=sw, RepackKeys=rk, ExtractKeys=ek)

    def gadget(self, lg, k):
        rq, rp_ = self.rings[lg]
        return self.rh.rlwe.GadgetCiphertext(rq, rp_, k.Q, k.P, BaseTwoDecomposition=k.pw2, digits_per_limb=k.digits_per_limb)

    def ct(self, lg, level, cts, is_ntt=True):
        rl = self.rings[lg][0].AtLevel(level)
        return self.rh.Ciphertext([self.rh.DevicePoly.from_numpy(rl, np.stack([c[i] for c in cts])) for i in (0, 1)], is_ntt=is_ntt)

    def new(self, lg, level, npoly):
        rl = self.rings[lg][0].AtLevel(level)
        return self.rh.Ciphertext([rl.NewPoly(npoly) for _ in (0, 1)], is_ntt=True)

    def close(self):
        self.ev.close()
        for rq, rp_ in self.rings.values():
            rq.close()
            if rp_ is not None:
                rp_.close()


def host(ct):
    vals = [v.numpy() for v in ct.Value]
    return [[v[k] for v in vals] for k in range(vals[0].shape[0])]


def same(got, want):
    return len(got) == len(want) and all(np.array_equal(np.stack(g), np.stack(w)) for g, w in zip(got, want))


@pytest.mark.parametrize("case", ro.EXPAND, ids=ro._eid)
def test_expand(rh, oracle, case):
    """fused, composed and rh_rlwe_expand, one input and a batch of 3, bit for bit against the restatement; from the coefficient domain the
    outputs are NTT-domain all the same; the device outputs decrypt to m[j] at coefficient 0"""
    name, setting, li, logGap = case
    d = Device(rh, name, setting, extract=True)
    N, level = d.N, d.levels[li]
    cases = [ro.expand_case(name, setting, li, logGap, tag) for tag in TAGS]
    index = list(range(0, N, 1 << logGap))
    for B in (1, 3):
        cts = [c[1] for c in cases[:B]]
        want = [cases[b][2][j] for j in index for b in range(B)]         # slot-major: coefficient m gap of input b at m B + b
        modes = [True, False] + (["C"] if setting[1] >= 2 else [])
        for fused in (modes if B == 3 or li == 0 else modes[:1]):
            ct = d.ct(d.logN, level, cts)
            ct.Scale = 12345
            out, idx = d.ev.ExpandC(ct, logGap) if fused == "C" else d.ev.Expand(ct, logGap, fused=fused)
            got = host(out)
            assert idx == index and same(got, want), (B, fused)
            assert out.IsNTT and out.LogDimensions == 0 and out.Scale == 12345 and same(host(ct), cts)
    for b in range(3):
        for s, j in enumerate(index):
            err = ro.error(name, d.logN, level, got[s * 3 + b], ro.one_coefficient(N, cases[b][0][j]))
            assert err <= d.logN + 6, (b, j, err)
    if li == 0:
        mods = d.Q[:level + 1]
        ctc = d.ct(d.logN, level, [[rr.intt(x, N, mods) for x in cases[0][1]]], is_ntt=False)
        out, _ = d.ev.Expand(ctc, logGap)
        assert out.IsNTT and same(host(out), [cases[0][2][j] for j in index])
    d.close()


@pytest.mark.parametrize("case", ro.PACK, ids=ro._pid)
def test_pack(rh, oracle, case):
    name, setting, keys = case
    d = Device(rh, name, setting, repack=True)
    N = d.N
    for li in (0, 1):
        level = d.levels[li]
        m, cts, want = ro.pack_case(name, setting, keys, li)
        for fused in (True, False):
            batch = d.ct(d.logN, level, [cts[j] for j in keys])
            out = d.ev.Pack(batch, list(keys), d.logN, True, fused=fused)
            got = host(out)
            assert same(got, [want]), (li, fused)
            assert out.IsNTT and batch.IsNTT
        err = ro.error(name, d.logN, level, got[0], ro.packed(m, set(keys)))
        assert err <= d.logN + 5, err
    # from the coefficient domain: transformed on entry, the input's flag flips (:699-703)
    mods = d.Q[:level + 1]
    batch = d.ct(d.logN, level, [[rr.intt(x, N, mods) for x in cts[j]] for j in keys], is_ntt=False)
    out = d.ev.Pack(batch, list(keys), d.logN, True)
    assert batch.IsNTT and same(host(out), [want])
    d.close()


@pytest.mark.parametrize("shape", ro.SPLIT, ids=t._ids)
def test_split_and_merge(rh, oracle, shape):
    name, setting = shape
    d = Device(rh, name, setting, min_logN=ro.log_n(t.chain(name)[0]) - 1, switching=True)
    lh = d.logN - 1
    for li in (0, 1):
        level = d.levels[li]
        sp = [ro.split_case(name, setting, li, tag) for tag in TAGS]
        ct = d.ct(d.logN, level, [c[1] for c in sp])
        ct.LogDimensions = 7
        even, odd = d.ev.SplitNew(ct)
        assert same(host(even), [c[2][0] for c in sp]) and same(host(odd), [c[2][1] for c in sp]), li
        assert even.LogDimensions == 6 and odd.LogDimensions == 6 and even.IsNTT and same(host(ct), [c[1] for c in sp])
        only = d.new(lh, level, 3)
        d.ev.Split(ct, only, None)
        assert same(host(only), [c[2][0] for c in sp])
        for k, h in enumerate(host(odd)):
            assert ro.error(name, lh, level, h, sp[k][0][1::2]) <= lh + 1
        mg = [ro.merge_case(name, setting, li, tag) for tag in TAGS]
        e, o = d.ct(lh, level, [c[1][0] for c in mg]), d.ct(lh, level, [c[1][1] for c in mg])
        e.LogDimensions = 6
        ctN = d.ev.MergeNew(e, o)
        got = host(ctN)
        assert same(got, [c[2] for c in mg]) and ctN.LogDimensions == 7 and ctN.IsNTT, li
        assert same(host(e), [c[1][0] for c in mg]) and same(host(o), [c[1][1] for c in mg])
        for k in range(3):
            want = [0] * d.N
            want[0::2], want[1::2] = mg[k][0]
            assert ro.error(name, d.logN, level, got[k], want) <= d.logN + 1
    N, Q, P, _ = ro.settings(name, setting)
    ctN = d.ev.MergeNew(e, None)
    key = ro.switching_key(name, setting, lh, lh + 1)
    assert same(host(ctN), [rp.merge(N, Q, P, c[1][0], None, key) for c in mg])
    # SwitchCiphertextRingDegreeNTT both ways and SwitchCiphertextRingDegree down, on the last level's inputs
    mods = [int(q) for q in Q[:level + 1]]
    down = d.new(lh, level, 3)
    rh.rlwe.SwitchCiphertextRingDegreeNTT(ct, d.rings[d.logN][0], down)
    assert same(host(down), [[rp.switch_ring_degree_ntt(x, N // 2, mods) for x in c[1]] for c in sp])
    upc = d.new(d.logN, level, 3)
    rh.rlwe.SwitchCiphertextRingDegreeNTT(e, d.rings[d.logN][0], upc)
    assert same(host(upc), [[rp.switch_ring_degree_ntt(x, N, mods) for x in c[1][0]] for c in mg])
    rh.rlwe.SwitchCiphertextRingDegree(ct, down)
    assert same(host(down), [[rp.switch_ring_degree(x, N // 2) for x in c[1]] for c in sp])
    d.close()


@pytest.mark.parametrize("case", ro.EPR, ids=lambda c: "%s-min%d-extract%s-repack%s" % (c[0], c[2], "naive" if c[3] else "", "naive" if c[4] else ""))
def test_extract_permute_repack(rh, oracle, case):
    name, setting, min_logN, extract_naive, repack_naive = case
    d = Device(rh, name, setting, min_logN=min_logN, extract=True, repack=True, switching=min_logN < 5)
    N, level = d.N, d.levels[0]
    m, ct, cts, want = ro.extract_repack_case(*case)
    dct = d.ct(d.logN, level, [ct])
    got = (d.ev.ExtractNaive if extract_naive else d.ev.Extract)(dct, {i: True for i in ro.chosen(N)})
    assert sorted(got) == sorted(cts)
    for i in cts:
        assert same(host(got[i]), [cts[i]]), i
    moved = {(i + N // 2) & (N - 1): c for i, c in got.items()}
    out = (d.ev.RepackNaive if repack_naive else d.ev.Repack)(moved)
    res = host(out)
    assert same(res, [want])
    exp = [0] * N
    for k0 in ro.chosen(N):
        exp[(k0 + N // 2) & (N - 1)] = m[k0]
    assert ro.error(name, d.logN, level, res[0], exp) <= d.logN + 5
    one = d.ev.Extract(dct, {7: True})                                   # one index: logGap = 0
    assert sorted(one) == [7]
    d.close()


def test_refusals(rh, oracle):
    from conftest import QI60, PI60
    E = rh.RingHipError
    name, setting = "TAIL", (0, 4)
    d = Device(rh, name, setting, min_logN=4, extract=True, repack=True, switching=True)
    level = d.levels[0]
    ct16 = d.new(4, level, 1)
    ct32 = d.new(5, level, 1)
    deg2 = rh.Ciphertext([d.rings[4][0].AtLevel(level).NewPoly(1) for _ in range(3)], is_ntt=True)
    with pytest.raises(E, match=r"ct.Degree\(\) != 1"):
        d.ev.Expand(deg2, 0)
    with pytest.raises(E, match=r"cts\[0\].Degree\(\) != 1"):
        d.ev.Pack(deg2, [0], 4, True)
    with pytest.raises(E, match=r"len\(cts\) = 0"):
        d.ev.Pack(ct16, [], 4, True)
    with pytest.raises(E, match="gaps between ciphertexts is smaller than inputLogGap > N"):
        d.ev.Pack(ct16, [0], 0, True)
    with pytest.raises(E, match=r"eval.ExtractKeys\[5\] is nil"):
        d.ev.Expand(ct32, 0)
    with pytest.raises(E, match=r"eval.RepackKeys\[5\] is nil"):
        d.ev.Pack(ct32, [0], 5, True)
    keep = d.ev.ExtractKeys, d.ev.RepackKeys
    d.ev.ExtractKeys = d.ev.RepackKeys = None
    with pytest.raises(E, match="eval.ExtractKeys is nil"):
        d.ev.Expand(ct16, 0)
    with pytest.raises(E, match="eval.RepackKeys is nil"):
        d.ev.Pack(ct16, [0], 4, True)
    d.ev.ExtractKeys, d.ev.RepackKeys = keep
    # a missing Galois key: named, found before the first launch -- the input keeps its values
    marks = [[np.full((level + 1, 16), 7 + c, dtype=np.uint64) for c in (0, 1)]]
    for keyset, call, g in ((d.ev.ExtractKeys[4], lambda c: d.ev.Expand(c, 0), 3), (d.ev.RepackKeys[4], lambda c: d.ev.Pack(c, [0], 4, True), 31)):
        gone = keyset.pop(g)
        c = d.ct(4, level, marks)
        with pytest.raises(E, match=r"GaloisKey\[%d\] is missing" % g):
            call(c)
        assert same(host(c), marks)
        keyset[g] = gone
    with pytest.raises(E, match=r"ctN.Log\(\) must be greater than eval.MinLogN\(\)"):
        d.ev.Split(ct16, ct16, None)
    with pytest.raises(E, match="ctEvenNHalf cannot be nil"):
        d.ev.Split(ct32, None, None)
    with pytest.raises(E, match=r"ctEvenNHalf.LogN\(\) must be equal to ctN.LogN\(\)-1"):
        d.ev.Split(ct32, ct32, None)
    with pytest.raises(E, match=r"ctOddNHalf.LogN\(\) must be equal to ctN.LogN\(\)-1"):
        d.ev.Split(ct32, ct16, ct32)
    with pytest.raises(E, match="ctEvenNHalf cannot be nil"):
        d.ev.Merge(None, ct16, ct32)
    with pytest.raises(E, match=r"ctEvenNHalf.LogN\(\) must be smaller than eval.MaxLogN\(\)"):
        d.ev.Merge(ct32, None, ct32)
    with pytest.raises(E, match=r"ctN.LogN\(\) must be equal to ctEvenNHalf.LogN\(\)\+1"):
        d.ev.Merge(ct16, None, ct16)
    with pytest.raises(E, match=r"ctEvenNHalf.LogN\(\) and ctOddNHalf.LogN\(\) must be equal"):
        d.ev.Merge(ct16, ct32, ct32)
    coeff = d.new(5, level, 1)
    coeff.IsNTT = False
    with pytest.raises(E, match="Split: coefficient-domain ciphertexts are not supported by the device path"):
        d.ev.Split(coeff, ct16, None)
    c16 = d.new(4, level, 1)
    c16.IsNTT = False
    with pytest.raises(E, match="Merge: coefficient-domain ciphertexts are not supported by the device path"):
        d.ev.Merge(c16, None, ct32)
    # repack's merge loop tests [j + 1]: an odd-only index set reaches Merge without an even half
    with pytest.raises(E, match="ctEvenNHalf cannot be nil"):
        d.ev.RepackNaive({1: d.new(4, level, 1)})
    # the entries' own checks
    L = rh.lib()
    rl = d.rings[4][0].AtLevel(level)
    a, b, u, x = rl.NewPoly(2), rl.NewPoly(2), rl.NewPoly(2), rl.NewPoly(1)
    u1 = u.ptr + 8 * u.words // 2
    assert L.rh_rlwe_expand_step(rl._h, level, 4, u.ptr, u1, a.ptr, b.ptr, x.ptr, 1) == -1 and b"must be odd" in L.rh_last_error()
    assert L.rh_rlwe_expand_step(rl._h, level, 17, a.ptr, u1, a.ptr, b.ptr, x.ptr, 1) == -1 and b"cannot overlap the batch" in L.rh_last_error()
    assert L.rh_rlwe_expand_step(rl._h, level, 17, u.ptr + 8, u1, a.ptr, b.ptr, x.ptr, 1) == -1 and b"16-byte aligned" in L.rh_last_error()
    bad = np.array([2, 0, 9, 0], dtype=np.int32)
    th = bad.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.rh_rlwe_pack_combine(rl._h, level, a.ptr, b.ptr, 2, x.ptr, th, 1, x.ptr, u.ptr, u1) == -1 and b"out of range" in L.rh_last_error()
    twice = np.array([0, 1, 1, 1, 1, 1, 0, 0], dtype=np.int32)
    th = twice.ctypes.data_as(C.POINTER(C.c_int32))
    assert L.rh_rlwe_rotate_addsub_q(rl._h, level, 3, u.ptr, u1, a.ptr, b.ptr, 2, x.ptr, th, 2) == -1 and b"named by two entries" in L.rh_last_error()
    assert L.rh_rlwe_ring_split(rl._h, level, a.ptr, b.ptr, u.ptr, u1, None, None, 4, 1) == -1 and b"logGap" in L.rh_last_error()
    assert L.rh_rlwe_ring_merge(rl._h, level, a.ptr, b.ptr, a.ptr, b.ptr, None, u.ptr, u1, 1, 1) == -1 and b"needs the table of X" in L.rh_last_error()
    d.close()
    # one degree: Split, SplitNew, Merge and MergeNew are refused
    d1 = Device(rh, name, setting)
    c = d1.new(5, level, 1)
    for f in (lambda: d1.ev.Split(c, c, None), lambda: d1.ev.SplitNew(c), lambda: d1.ev.Merge(c, None, c), lambda: d1.ev.MergeNew(c, None)):
        with pytest.raises(E, match=r"method is not supported when eval.MinLogN\(\) == eval.MaxLogN\(\)"):
            f()
    d1.close()
    # conjugate-invariant rings
    rq, rp_ = rh.Ring(32, QI60[:2], kind=rh.ConjugateInvariant), rh.Ring(32, PI60[:2], kind=rh.ConjugateInvariant)
    ev = rh.rlwe.RingPackingEvaluator({5: (rq, rp_)}, RepackKeys={5: {}}, ExtractKeys={5: {}})
    new = rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
    with pytest.raises(E, match=r"method is only supported for ring.Type = ring.Standard \(X\^\{-2\^\{i\}\} does not exist in the sub-ring Z\[X \+ X\^\{-1\}\]\)"):
        ev.Expand(new, 0)
    with pytest.raises(E, match=r"procedure is only supported for ring.Type = ring.Standard \(X\^\{2\^\{i\}\} does not exist in the sub-ring Z\[X \+ X\^\{-1\}\]\)"):
        ev.Pack(new, [0], 5, True)
    assert L.rh_rlwe_ring_split(rq._h, 1, new.Value[0].ptr, new.Value[1].ptr, new.Value[0].ptr, new.Value[1].ptr, None, None, 1, 1) == -5 and b"standard rings only" in L.rh_last_error()
    ev.close(); rq.close(); rp_.close()

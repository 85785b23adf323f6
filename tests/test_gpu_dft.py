"""GPU: the homomorphic DFT on the device (circuits/ckks/dft).  GenMatrices in HBM (csrc/dft.hip) against the restatement, every diagonal with ==
on float64; NewMatrixFromLiteral against the restatement's encode and against the per-diagonal lintrans.Encode; the split / merge kernels of
csrc/ckks.hip against the calls they replace; CoeffsToSlots / SlotsToCoeffs -- fused and composed -- against the restatement that
tests/test_dft_oracle.py pins to decryption (tests/dft_restatement.py), and by decrypting the device output on the host; every refusal by its text.

Shapes (those of tests/test_gpu_lintrans.py): TAIL (N = 32: LogSlots 3 sparse and 4 full, a row inside one wavefront), REF (N = 2^10, mixed-width
limbs: LogSlots 8 and 9), Q61N13 (N = 2^13: more than one block per row, 61-bit moduli; the split / merge kernels only); batches of 3."""
import gc
import itertools
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_restatement as cer
import dft_restatement as dr
import test_dft_oracle as tdo
import test_gpu_lintrans as tgl
import test_lintrans_oracle as tlo
import test_rlwe_oracle as t
from test_gpu_rlwe_decrypt import B, Device, host, same

pytestmark = pytest.mark.gpu
E, D = dr.ENCODE, dr.DECODE
SHAPES = tgl.SHAPES
FORMATS = (dr.STANDARD, dr.SPLIT, dr.REPACK)


def rows_equal(block, index, want):
    """every diagonal with == on float64 (zeros of either sign are equal), and no NaN"""
    got = block.numpy()
    assert not np.isnan(got.view(np.float64)).any()
    for row, k in enumerate(index):
        w = np.array([complex(*x) for x in want[k]])
        if not (np.array_equal(got[row].real, w.real) and np.array_equal(got[row].imag, w.imag)):
            return False
    return True


# ---- 1. GenMatrices on the device ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [3, 4], ids=["sparse", "full"])
@pytest.mark.parametrize("tp", [E, D], ids=["encode", "decode"])
def test_gen_matrices_tail(rh, tp, ls):
    """Type x Format x BitReversed x Levels at N = 32.  sum(Levels) is the number of factors: [1,1,1], [2,1] and [3] give one FFT level per factor at
    LogSlots 3 and collapse two levels into one factor at LogSlots 4; [1,1] and [1] collapse up to four, where one diagonal receives three
    contributions (the addition order: b and c of one source after a of another) and, with rot = slots / 2, b and c of a level meet on one diagonal."""
    ring = rh.Ring(32, list(t.chain("TAIL")[1][:1]))
    for fmt, br, lv in itertools.product(FORMATS, (False, True), ([1, 1, 1], [2, 1], [3], [1, 1], [1])):
        want = dr.gen_matrices(dr.literal(tp, ls, 6, 1, lv, fmt, 0.75, br), 5)
        got = rh.dft.MatrixLiteral(tp, ls, 6, 1, lv, fmt, 0.75, br).GenMatrices(5, ring=ring)
        assert len(got) == len(want) == sum(lv)
        for g, w in zip(got, want):
            assert g.Index == sorted(w) and g.Block.n == (16 if fmt == dr.REPACK and ls == 3 else 1 << ls)
            assert rows_equal(g.Block, g.Index, w), (fmt, br, lv)
    # the three-term sums are there: in the order rot = 1, 2, 4 (a decode in natural order, an encode in bit-reversed order) a diagonal meets d, d - 4 and d + 4
    three = [len(terms) for br in (False, True) for steps, _ in rh.dft.MatrixLiteral(tp, 3, 6, 1, [1], BitReversed=br)._plan(5)[0] for step in steps for terms in step[2]]
    assert max(three) == 3
    ring.close()


@pytest.mark.parametrize("lv", [[1] * 6, [3, 3], [1, 1]], ids=["1x6", "3-3", "1-1"])
@pytest.mark.parametrize("tp", [E, D], ids=["encode", "decode"])
def test_gen_matrices_ref(rh, tp, lv):
    """N = 2^10, RepackImagAsReal, LogSlots 8 (sparse: 512 entries per diagonal, the repack matrix, the zeroed second copy) and 9; [1,1] collapses
    four and five levels into a factor (up to 63 diagonals)"""
    ring = rh.Ring(1024, list(t.chain("REF")[1][:1]))
    for ls, br in itertools.product((8, 9), (False, True)):
        want = dr.gen_matrices(dr.literal(tp, ls, 6, 1, lv, dr.REPACK, None, br), 10)
        got = rh.dft.MatrixLiteral(tp, ls, 6, 1, lv, dr.REPACK, None, br).GenMatrices(10, ring=ring)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.Index == sorted(w) and rows_equal(g.Block, g.Index, w), (ls, br)
            assert sorted(g.host()) == g.Index
    ring.close()


# ---- 2. NewMatrixFromLiteral ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0, 2])
@pytest.mark.parametrize("case", [("TAIL", 3, [2, 1]), ("TAIL", 4, [1, 1]), ("REF", 8, [1, 1]), ("REF", 9, [2])], ids=lambda c: "%s-%d-%s" % (c[0], c[1], "".join(map(str, c[2]))))
def test_new_matrix_from_literal(rh, case, ratio):
    """every encoded diagonal, Q and P parts, bit for bit against the restatement's encode and against lintrans.Encode fed the host diagonals; the
    views outlive the literal, the generator's blocks and a collection"""
    name, ls, lv = case
    d = Device(rh, name, dict(SHAPES)[name])
    N, Q, P = d.N, d.Q, d.P
    top, levelP = d.levels[0], len(P) - 1
    ecd = rh.ckks.Encoder(d.rq, ringP=d.rp)
    for tp in (E, D):
        lit = dr.literal(tp, ls, top, levelP, lv, dr.REPACK, None, False, ratio)
        pk = rh.dft.MatrixLiteral(tp, ls, top, levelP, lv, dr.REPACK, LogBSGSRatio=ratio)
        M = rh.dft.NewMatrixFromLiteral(d.rq, d.rp, pk, ecd)
        assert M.LogSlots == ls and M.MatrixLiteral is pk
        mats = M.Matrices
        host_diags = pk.GenMatrices(N.bit_length() - 1, device=False)
        del M, pk
        gc.collect()
        junk = [d.rq.NewPoly(4) for _ in range(4)]                       # whatever was freed is handed out again
        want = dr.new_matrix(N, Q, P, lit)
        assert len(mats) == len(want) == sum(lv)
        level, idx = top, 0
        for grp in lv:
            for _ in range(grp):
                lt, w = mats[idx], want[idx]
                assert lt.N1 == w.N1 and sorted(lt.Vec) == sorted(w.Vec) and (lt.LevelQ, lt.LevelP) == (top, levelP)
                assert lt.Scale.Value == w.Scale.v == dr.kth_root_scale(int(Q[level]), grp).v and lt.LogDimensions == w.LogSlots
                params = rh.lintrans.Parameters(sorted(w.Vec), top, levelP, lt.Scale, lt.LogDimensions, ratio)
                one = rh.lintrans.NewTransformation(d.rq, d.rp, params)
                rh.lintrans.Encode(ecd, host_diags[idx], one)
                for k in w.Vec:
                    q, p = lt.Vec[k].Q.numpy()[0], lt.Vec[k].P.numpy()[0]
                    assert np.array_equal(q, w.Vec[k][0]) and np.array_equal(p, w.Vec[k][1]), (tp, idx, k)
                    assert np.array_equal(q, one.Vec[k].Q.numpy()[0]) and np.array_equal(p, one.Vec[k].P.numpy()[0]), (tp, idx, k)
                idx += 1
            level -= 1
        del junk
    ecd.close(); d.close()


# ---- 3. the split / merge kernels -----------------------------------------------------------------------------------------------------------------
def edge_polys(tag, N, mods):
    """B uniform polys with q - 1 and 0 planted in every limb, in both halves of the coefficients (the two scalars)"""
    out = tgl.uniform(tag, N, mods)
    for k, p in enumerate(out):
        for i, q in enumerate(mods):
            p[i, [0, 1, N // 2, N - 1]] = [q - 1, 0, q - 1, 0] if k % 2 == 0 else [0, q - 1, 0, q - 1]
    return out


def pp(polys):
    import ctypes as C
    return (C.c_void_p * 2)(*[p.ptr for p in polys])


@pytest.mark.parametrize("nt_streams", [1, 2], ids=["nt-by-size", "nt-always"])
@pytest.mark.parametrize("shape", SHAPES, ids=tgl._ids)
def test_split_and_merge_kernels_against_the_composed_calls(rh, shape, nt_streams):
    """rh_ckks_split_real_imag against Sub, MulDoubleRNSScalar(-i), Add and rh_ckks_merge_real_imag against MulDoubleRNSScalar(i), Add, whole arrays,
    at the top level and one below; re written over zc (as CoeffsToSlots does), out over im, out over re; the inputs that are not written are left alone"""
    name, setting = shape
    d = Device(rh, name, setting)
    d.rq.set_tuning("nt_streams", nt_streams)
    ev = rh.ckks.Evaluator(d.rq, d.rp)
    L = rh.lib()
    N = d.N
    for level in d.levels[:2]:
        mods = [int(q) for q in d.Q[:level + 1]]
        rq = d.rq.AtLevel(level)
        hz = [edge_polys("z%d %s %d" % (c, name, level), N, mods) for c in (0, 1)]
        hzc = [edge_polys("zc%d %s %d" % (c, name, level), N, mods)[::-1] for c in (0, 1)]
        up = lambda hs: [tgl.up(rh, rq, h) for h in hs]
        mi = ev._rns_scalar(level, rh.ckks.Scale(1), (Fraction(0), Fraction(-1)))
        pi = ev._rns_scalar(level, rh.ckks.Scale(1), (Fraction(0), Fraction(1)))
        u64 = lambda s: np.ascontiguousarray(np.array(s, dtype=np.uint64))
        ptr = lambda a: a.ctypes.data_as(rh.ringhip.U64P)
        # composed
        z, zc = up(hz), up(hzc)
        im_c, re_c = [rq.NewPoly(B) for _ in (0, 1)], [rq.NewPoly(B) for _ in (0, 1)]
        for c in (0, 1):
            rq.Sub(z[c], zc[c], im_c[c])
            rq.MulDoubleRNSScalar(im_c[c], mi[0], mi[1], im_c[c])
            rq.Add(zc[c], z[c], re_c[c])
        want_re, want_im = [p.numpy() for p in re_c], [p.numpy() for p in im_c]
        # fused, out of place and with re = zc
        for alias in (False, True):
            z, zc = up(hz), up(hzc)
            re = zc if alias else [rq.NewPoly(B) for _ in (0, 1)]
            im = [rq.NewPoly(B) for _ in (0, 1)]
            a, b = u64(mi[0]), u64(mi[1])
            assert L.rh_ckks_split_real_imag(d.rq._h, level, pp(z), pp(zc), pp(re), pp(im), B, ptr(a), ptr(b)) == 0, L.rh_last_error()
            for c in (0, 1):
                assert np.array_equal(re[c].numpy(), want_re[c]) and np.array_equal(im[c].numpy(), want_im[c]), (level, alias, c)
                assert np.array_equal(z[c].numpy(), np.stack(hz[c])) and (alias or np.array_equal(zc[c].numpy(), np.stack(hzc[c])))
        # merge: out = im i + re
        out_c = [rq.NewPoly(B) for _ in (0, 1)]
        for c in (0, 1):
            rq.MulDoubleRNSScalar(im_c[c], pi[0], pi[1], out_c[c])
            rq.Add(out_c[c], re_c[c], out_c[c])
        want = [p.numpy() for p in out_c]
        a, b = u64(pi[0]), u64(pi[1])
        for alias in ("none", "im", "re"):
            re, im = up([list(x) for x in want_re]), up([list(x) for x in want_im])
            out = {"none": [rq.NewPoly(B) for _ in (0, 1)], "im": im, "re": re}[alias]
            assert L.rh_ckks_merge_real_imag(d.rq._h, level, pp(re), pp(im), pp(out), B, ptr(a), ptr(b)) == 0, L.rh_last_error()
            for c in (0, 1):
                assert np.array_equal(out[c].numpy(), want[c]), (level, alias, c)
                assert alias == "re" or np.array_equal(re[c].numpy(), want_re[c])
                assert alias == "im" or np.array_equal(im[c].numpy(), want_im[c])
    ev.close(); d.close()


# ---- 4. the circuits against the restatement ------------------------------------------------------------------------------------------------------
def setup(rh, name, lits):
    d = Device(rh, name, dict(SHAPES)[name])
    galEls = {2 * d.N - 1}
    for lit in lits:
        galEls |= set(dr.galois_elements(lit, d.N))
    hk = tgl.host_keys(name, dict(SHAPES)[name], galEls)
    ev, _ = tgl.evaluator(rh, d, hk)
    return d, hk, ev, rh.dft.Evaluator(ev), rh.ckks.Encoder(d.rq, ringP=d.rp)


def batch(rh, d, name, level, log_dims, tag="m"):
    _, cts = tgl.messages(name, level, tag)
    ct = d.ct(level, cts)
    ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << tgl.LOG_SCALE[name]), log_dims
    return ct, cts


CIRCUITS = [("TAIL", 3, [1, 1, 1], f) for f in FORMATS] + [("TAIL", 4, [1, 1], f) for f in FORMATS] + [("REF", 8, [1, 1], dr.REPACK), ("REF", 9, [1, 1], dr.REPACK)]
_cid = lambda c: "%s-%d-%s-f%d" % (c[0], c[1], "".join(map(str, c[2])), c[3])


@pytest.mark.parametrize("case", CIRCUITS, ids=_cid)
def test_coeffs_to_slots(rh, oracle, case):
    """CoeffsToSlotsNew and CoeffsToSlots, fused and composed, a batch of 3: the bits, the scale, the level and LogDimensions of the restatement"""
    name, ls, lv, fmt = case
    N, Q, P, levels = t.chain(name)
    P = P[:dict(SHAPES)[name][1]]
    top = levels[0]
    lit = dr.literal(E, ls, top, len(P) - 1, lv, fmt)
    d, hk, ev, dev, ecd = setup(rh, name, [lit])
    M = rh.dft.NewMatrixFromLiteral(d.rq, d.rp, rh.dft.MatrixLiteral(E, ls, top, len(P) - 1, lv, fmt), ecd)
    lts = dr.new_matrix(N, Q, P, lit)
    full = ls == N.bit_length() - 2
    scale = 1 << tgl.LOG_SCALE[name]
    _, cts = tgl.messages(name, top)
    want = [dr.coeffs_to_slots(N, Q, P, c, scale, ls, lit, lts, hk) for c in cts]
    for fused in (True, False):
        ct, _ = batch(rh, d, name, top, ls)
        re, im = dev.CoeffsToSlotsNew(ct, M, fused=fused)
        assert same(host(ct), cts)
        assert same(host(re), [w[0][0] for w in want]), fused
        assert re.Scale.Value == want[0][0][1].v and re.Level() == top - sum(lv) and re.LogDimensions == ls and re.IsNTT
        if fmt != dr.STANDARD and full:
            assert same(host(im), [w[1][0] for w in want]), fused
            assert im.Scale.Value == want[0][1][1].v and im.Level() == top - sum(lv) and im.LogDimensions == ls
        else:
            assert (im is None) == (not full) and all(w[1] is None for w in want)
    re2, im2 = d.new(top), (d.new(top) if full else None)                 # into ciphertexts of the caller, at LevelQ: they are resized
    dev.CoeffsToSlots(batch(rh, d, name, top, ls)[0], M, re2, im2)
    assert same(host(re2), [w[0][0] for w in want]) and re2.Scale.Value == want[0][0][1].v
    ecd.close(); ev.close(); d.close()


@pytest.mark.parametrize("case", CIRCUITS, ids=_cid)
def test_slots_to_coeffs(rh, oracle, case):
    name, ls, lv, fmt = case
    N, Q, P, levels = t.chain(name)
    P = P[:dict(SHAPES)[name][1]]
    top = levels[0]
    lit = dr.literal(D, ls, top, len(P) - 1, lv, fmt)
    d, hk, ev, dev, ecd = setup(rh, name, [lit])
    M = rh.dft.NewMatrixFromLiteral(d.rq, d.rp, rh.dft.MatrixLiteral(D, ls, top, len(P) - 1, lv, fmt), ecd)
    lts = dr.new_matrix(N, Q, P, lit)
    full = ls == N.bit_length() - 2
    log_dims = ls if full or fmt != dr.REPACK else ls + 1
    scale = 1 << tgl.LOG_SCALE[name]
    _, re_h = tgl.messages(name, top)
    _, im_h = tgl.messages(name, top, "im") if full else (None, [None] * B)
    want = [dr.slots_to_coeffs(N, Q, P, r, scale, i, scale, lit, lts, hk) for r, i in zip(re_h, im_h)]
    for fused in (True, False):
        re = batch(rh, d, name, top, log_dims)[0]
        im = batch(rh, d, name, top, log_dims, "im")[0] if full else None
        out = dev.SlotsToCoeffsNew(re, im, M, fused=fused)
        assert same(host(out), [w[0] for w in want]), fused
        assert out.Scale.Value == want[0][1].v and out.Level() == top - sum(lv) and out.LogDimensions == log_dims and out.IsNTT
        assert same(host(re), re_h) and (im is None or same(host(im), im_h))
    ecd.close(); ev.close(); d.close()


# ---- 5. decryption of the device output ---------------------------------------------------------------------------------------------------------
def test_coeffs_to_slots_decrypts_on_the_device_path(rh, oracle):
    """Encode/FullPacking of dft_test.go at testInsecurePrec45 (LogN 10, the prec45 chain -- REF's own ring degree with the seven moduli Levels
    [1] * 6 needs --, scale 2^45, the golden file's two P moduli as in tests/test_dft_oracle.py): the device output, bit for bit the restatement's,
    decrypts to the plaintext IFFT within VerifyTestVectors' log2(scale) - (LogN + 2) = 33 bits"""
    N, Q, P = tlo.prec45()
    level, ls = len(Q) - 1, 9
    slots = 1 << ls
    lit = dr.literal(E, ls, level, len(P) - 1, [1] * level, dr.REPACK)
    hk = tdo.keys_for(lit)
    rq, rp = rh.Ring(N, list(Q)), rh.Ring(N, list(P))
    gks = {g: rh.rlwe.GadgetCiphertext(rq, rp, k.Q, k.P, BaseTwoDecomposition=k.pw2, digits_per_limb=k.digits_per_limb) for g, k in hk.items()}
    ev = rh.ckks.Evaluator(rq, rp, galois_keys=gks)
    dev = rh.dft.Evaluator(ev)
    ecd = rh.ckks.Encoder(rq, ringP=rp)
    M = rh.dft.NewMatrixFromLiteral(rq, rp, rh.dft.MatrixLiteral(E, ls, level, len(P) - 1, [1] * level, dr.REPACK), ecd)
    values, coeffs = tdo.encode_case(ls)
    hct = tdo.encrypt("c2s %d" % ls, cer.encode_coeffs(coeffs, 2.0 ** tdo.LOG_SCALE, N, [int(q) for q in Q], is_ntt=True), level)
    ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rq.AtLevel(level), c[None]) for c in hct], is_ntt=True)
    ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << tdo.LOG_SCALE), ls
    re, im = dev.CoeffsToSlotsNew(ct, M)
    (wre, wrs), (wim, wis) = dr.coeffs_to_slots(N, Q, P, hct, 1 << tdo.LOG_SCALE, ls, lit, dr.new_matrix(N, Q, P, lit), hk)
    for what, got, w, ws, part in (("real", re, wre, wrs, values.real), ("imag", im, wim, wis, values.imag)):
        g = [v.numpy()[0] for v in got.Value]
        assert np.array_equal(np.stack(g), np.stack(w)) and got.Scale.Value == ws.v and got.Level() == 0
        vr, vi = cer.special_ifft(part, np.zeros(slots), 2 * N)
        tdo.precision("gpu encode full " + what, np.concatenate([vr, vi]), tdo.decrypt_coeffs(g, got.Scale.Float64()))
    ecd.close(); ev.close(); rq.close(); rp.close()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(rh, oracle):
    from conftest import QI60, PI60
    from oracle import primes
    Err = rh.RingHipError
    dft = rh.dft
    name = "TAIL"
    N, Q, P, levels = t.chain(name)
    top = levels[0]
    lit = dr.literal(D, 4, top, 3, [1, 1], dr.REPACK)
    d, hk, ev, dev, ecd = setup(rh, name, [lit])
    ML = lambda *a, **k: dft.MatrixLiteral(*a, **k)
    good = ML(D, 4, top, 3, [1, 1], dr.REPACK)

    class Big:
        ringP = d.rp

        def Prec(self):
            return 64
    with pytest.raises(Err, match="encoder precision 64 > 53"):
        dft.NewMatrixFromLiteral(d.rq, d.rp, good, Big())
    plain = rh.ckks.Encoder(d.rq)
    with pytest.raises(Err, match="NewMatrixFromLiteral and its encoder need ringP"):
        dft.NewMatrixFromLiteral(d.rq, d.rp, good, plain)
    with pytest.raises(Err, match="need ringP"):
        dft.NewMatrixFromLiteral(d.rq, None, good, ecd)
    with pytest.raises(Err, match="LevelsConsumedPerRescaling = 2: the PREC128 path is not built"):
        dft.NewMatrixFromLiteral(d.rq, d.rp, good, ecd, levels_consumed_per_rescaling=2)
    for ls in (0, 5):
        with pytest.raises(Err, match=r"LogSlots = %d outside \[1, LogN - 1 = 4\]" % ls):
            dft.NewMatrixFromLiteral(d.rq, d.rp, ML(D, ls, top, 3, [1]), ecd)
    with pytest.raises(Err, match=r"the chain needs sum\(Levels\) \+ 1 = 4 moduli up to LevelQ"):
        dft.NewMatrixFromLiteral(d.rq, d.rp, ML(D, 4, 2, 3, [1, 1, 1]), ecd)
    with pytest.raises(Err, match=r"LevelQ = 7, LevelP = 3 out of range"):
        dft.NewMatrixFromLiteral(d.rq, d.rp, ML(D, 4, 7, 3, [1]), ecd)
    # the circuits
    M = dft.NewMatrixFromLiteral(d.rq, d.rp, good, ecd)
    re, _ = batch(rh, d, name, top, 4)
    _, cts = tgl.messages(name, top)
    with pytest.raises(Err, match="cannot SlotsToCoeffs: coefficient-domain ciphertexts are not supported"):
        dev.SlotsToCoeffsNew(d.ct(top, cts, is_ntt=False), None, M)
    with pytest.raises(Err, match="cannot CoeffsToSlots: coefficient-domain ciphertexts are not supported"):
        dev.CoeffsToSlotsNew(d.ct(top, cts, is_ntt=False), M)
    low = batch(rh, d, name, top - 1, 4)[0]
    with pytest.raises(Err, match=r"ctReal.Level\(\) or ctImag.Level\(\) < DFTMatrix.LevelQ"):
        dev.SlotsToCoeffsNew(low, None, M)
    with pytest.raises(Err, match=r"ctReal.Level\(\) or ctImag.Level\(\) < DFTMatrix.LevelQ"):
        dev.SlotsToCoeffsNew(re, low, M)
    gone = [g for g in dr.galois_elements(lit, N) if g != 1][-1]
    saved = ev.ks.galois_keys.pop(gone)
    with pytest.raises(Err, match=r"cannot SlotsToCoeffs: .*GaloisKey\[%d\] is missing" % gone):
        dev.SlotsToCoeffsNew(re, batch(rh, d, name, top, 4, "im")[0], M)
    ev.ks.galois_keys[gone] = saved
    # the entries' own checks
    L = rh.lib()
    rq = d.rq.AtLevel(top)
    a = [rq.NewPoly(B) for _ in range(8)]
    s = np.ones(top + 1, dtype=np.uint64)
    sp = s.ctypes.data_as(rh.ringhip.U64P)
    assert L.rh_ckks_split_real_imag(d.rq._h, top + 1, pp(a[0:2]), pp(a[2:4]), pp(a[4:6]), pp(a[6:8]), B, sp, sp) == -1 and b"level 7 out of range" in L.rh_last_error()
    assert L.rh_ckks_split_real_imag(d.rq._h, top, pp(a[0:2]), pp(a[2:4]), pp(a[4:6]), pp([a[6], a[4]]), B, sp, sp) == -1 and b"two outputs overlap" in L.rh_last_error()
    assert L.rh_ckks_merge_real_imag(d.rq._h, top, pp(a[0:2]), pp(a[2:4]), pp(a[4:6]), B, None, sp) == -1 and b"rh_ckks_merge_real_imag: null argument" in L.rh_last_error()
    import ctypes as C
    shifted = (C.c_void_p * 2)(a[0].ptr + 16, a[5].ptr)
    assert L.rh_ckks_merge_real_imag(d.rq._h, top, pp(a[0:2]), pp(a[2:4]), shifted, B, sp, sp) == -1 and b"an output overlaps an input without being that input" in L.rh_last_error()
    dv = rh.ckks.DeviceValues(d.rq, 4, 16)
    tab = rh.ckks.DeviceValues(d.rq, 1, 64, complex=False)
    prog = lambda *v: (C.c_int * len(v))(*v)
    assert L.rh_ckks_dft_merge_level(d.rq._h, 16, 0, dv.ptr, dv.ptr, 1, prog(1, 0, -2, 0, -2, 0), 1, a[0].ptr, tab.ptr, 64) == -1 and b"names source 1 of 1" in L.rh_last_error()
    assert L.rh_ckks_dft_merge_level(d.rq._h, 16, 0, dv.ptr, dv.ptr, 1, prog(0, 3, -2, 0, -2, 0), 1, a[0].ptr, tab.ptr, 64) == -1 and b"names kind 3" in L.rh_last_error()
    assert L.rh_ckks_dft_merge_level(d.rq._h, 16, 0, dv.ptr, dv.ptr, 1, prog(-2, 0, -2, 0, -2, 0), 1, a[0].ptr, tab.ptr, 64) == -1 and b"has no contribution" in L.rh_last_error()
    assert L.rh_ckks_dft_merge_level(d.rq._h, 16, 0, dv.ptr, dv.ptr, 1, prog(0, 0, -2, 0, -2, 0), 1, a[0].ptr, tab.ptr, 2) == -1 and b"the table holds 2 words" in L.rh_last_error()
    assert L.rh_ckks_dft_merge_level(d.rq._h, 12, 0, dv.ptr, dv.ptr, 1, prog(0, 0, -2, 0, -2, 0), 1, a[0].ptr, tab.ptr, 64) == -1 and b"must be a power of two" in L.rh_last_error()
    assert L.rh_ckks_dft_merge_level(d.rq._h, 16, 16, dv.ptr, dv.ptr, 1, prog(0, 0, -2, 0, -2, 0), 1, a[0].ptr, tab.ptr, 64) == -1 and b"rot 16 out of range" in L.rh_last_error()
    assert L.rh_ckks_dft_level_vectors(d.rq._h, 0, 3, 8, 4, 0, dv.ptr, 33, tab.ptr, 4, a[0].ptr) == -1 and b"fft_level 4 out of range" in L.rh_last_error()
    assert L.rh_ckks_dft_level_vectors(d.rq._h, 0, 3, 8, 1, 0, dv.ptr, 32, tab.ptr, 4, a[0].ptr) == -1 and b"32 roots given, 4 slots + 1 = 33" in L.rh_last_error()
    assert L.rh_ckks_dft_level_vectors(d.rq._h, 0, 3, 24, 1, 0, dv.ptr, 33, tab.ptr, 4, a[0].ptr) == -1 and b"neither slots = 8 nor 2 slots" in L.rh_last_error()
    assert L.rh_ckks_dft_finish(d.rq._h, 16, 2, dv.ptr, dv.ptr, 1.0, 0, prog(0, 1), tab.ptr, 64) == -1 and b"rotated diagonals are not written in place" in L.rh_last_error()
    assert L.rh_ckks_dft_finish(d.rq._h, 16, 2, dv.ptr, a[0].ptr, 1.0, 0, prog(0, 16), tab.ptr, 64) == -1 and b"rotation 16 of diagonal 1 out of range" in L.rh_last_error()
    plain.close(); ecd.close(); ev.close(); d.close()
    # whatever lintrans.Evaluator refuses: keys with a power-of-two decomposition and keys with one P modulus (found when the circuit runs), and
    # conjugate-invariant and 3N rings (when the evaluator is made)
    for setting1, text in (((16, 1), "method is unsupported for BaseTwoDecomposition != 0"), ((0, 1), "one P modulus")):
        d1 = Device(rh, name, setting1)
        lit1 = dr.literal(D, 4, top, 0, [1, 1], dr.REPACK)
        ev1, _ = tgl.evaluator(rh, d1, tgl.host_keys(name, setting1, set(dr.galois_elements(lit1, N)) | {2 * N - 1}))
        ecd1 = rh.ckks.Encoder(d1.rq, ringP=d1.rp)
        M1 = dft.NewMatrixFromLiteral(d1.rq, d1.rp, ML(D, 4, top, 0, [1, 1], dr.REPACK), ecd1)
        with pytest.raises(Err, match=text):
            dft.Evaluator(ev1).SlotsToCoeffsNew(batch(rh, d1, name, top, 4)[0], batch(rh, d1, name, top, 4, "im")[0], M1)
        ecd1.close(); ev1.close(); d1.close()
    for rq, rp in ((rh.Ring(32, QI60[:2], kind=rh.ConjugateInvariant), rh.Ring(32, PI60[:2], kind=rh.ConjugateInvariant)),
                   tuple(rh.Ring(3 << 6, m, kind=rh.Matrix3N) for m in primes.gen_moduli_3n(3 << 6, [60, 60], [60, 60]))):
        cev = rh.ckks.Evaluator(rq, rp)
        with pytest.raises(Err, match="conjugate-invariant and 3N rings are not supported"):
            dft.Evaluator(cev)

        class Ecd:
            ringP = rp

            def Prec(self):
                return 53
        with pytest.raises(Err, match="cannot NewDFTMatrixFromLiteral: conjugate-invariant and 3N rings are not supported"):
            dft.NewMatrixFromLiteral(rq, rp, ML(E, 3, 1, 1, [1]), Ecd())
        cev.close(); rq.close(); rp.close()

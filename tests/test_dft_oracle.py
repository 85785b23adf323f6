"""CPU: the homomorphic DFT (circuits/ckks/dft).  The index maps and Galois elements pinned to hand-derived values, GenMatrices pinned to the encoder
restatement's special FFT / IFFT, the restatement the device path is compared with (tests/dft_restatement.py) pinned to decryption at the
reference's own test setting (dft_test.go:71-430 at testInsecurePrec45), and the package's host side against the restatement."""
import itertools
import json
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_restatement as cer
import ckks_restatement as cr
import dft_restatement as dr
import lintrans_restatement as ltr
import rlwe_restatement as rr
import test_lintrans_oracle as tlo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E, D = dr.ENCODE, dr.DECODE


# ---- index maps and Galois elements ------------------------------------------------------------------------------------------------------------
def test_index_maps_by_hand_for_log_slots_3():
    """LogSlots 3 (8 slots).  One FFT level per rotation: an encode in natural order (and a decode in bit-reversed order) rotates by 2^(level-1),
    i.e. 4, 2, 1 for levels 3, 2, 1; the other two by 2^(3-level), i.e. 1, 2, 4.  A level's map is {0, rot, 8 - rot}; merging a map with the next
    level adds i +- rot to every i.  The number of factors is sum(Levels) and factor i collapses ceil(levels left / factors left) levels, counted
    from the first factor for an encode and from the last for a decode.
      sum(Levels) = 3 ([1,1,1], [2,1], [3]): one level per factor: encode {0,4} {0,2,6} {0,1,7}; decode {0,1,7} {0,2,6} {0,4}.
      [1,1]: encode collapses 2 + 1: {0,4} with rot 2 -> {0,2,4,6}, then {0,1,7}; decode collapses 1 + 2: {0,1,7}, then {0,2,6} with rot 4 ->
             {0,4, 2,6, 6,2} = {0,2,4,6}.
      [1]:   {0,4} -> {0,2,4,6} -> with rot 1 every index.
      sparse decode with RepackImagAsReal (LogN 5): the first factor starts from {0, 8} modulo 16 and is merged with level 3 (rot 1):
             {0,1,15, 8,9,7}."""
    maps = lambda *a, logN=4, **k: [sorted(m) for m in dr.index_maps(dr.literal(*a, **k), logN)]
    for lv in ([1, 1, 1], [2, 1], [3]):
        assert maps(E, 3, 6, 1, lv) == [[0, 4], [0, 2, 6], [0, 1, 7]]
        assert maps(D, 3, 6, 1, lv) == [[0, 1, 7], [0, 2, 6], [0, 4]]
        assert maps(E, 3, 6, 1, lv, BitReversed=True) == [[0, 1, 7], [0, 2, 6], [0, 4]]
        assert maps(D, 3, 6, 1, lv, BitReversed=True) == [[0, 4], [0, 2, 6], [0, 1, 7]]
    assert maps(E, 3, 6, 1, [1, 1]) == [[0, 2, 4, 6], [0, 1, 7]]
    assert maps(D, 3, 6, 1, [1, 1]) == [[0, 1, 7], [0, 2, 4, 6]]
    assert maps(E, 3, 6, 1, [1]) == [list(range(8))] == maps(D, 3, 6, 1, [1])
    assert maps(D, 3, 6, 1, [1, 1, 1], Format=dr.REPACK, logN=5) == [[0, 1, 7, 8, 9, 15], [0, 2, 6], [0, 4]]
    assert maps(E, 3, 6, 1, [1, 1, 1], Format=dr.REPACK, logN=5) == [[0, 4], [0, 2, 6], [0, 1, 7]]      # an encode repacks AFTER the transformation


def test_galois_elements_by_hand_for_log_slots_3():
    """Sparse RepackImagAsReal at LogN 5, Levels [1,1,1], LogBSGSRatio 0 (dslots = 16, FindBestBSGSRatio asks (#baby - 1) / (#giant - 1) = 1).
    Encode: the repack rotation 8 first.  {0,4} has fewer than 3 diagonals: every index is added, 0 included (:494-499): 0, 4.
      {0,2,6}: N1 = 4 (giant {0,4}, baby {0,2}: 1 / 1): giant steps 0, 0, 4 -> 4; baby steps 0, 2, 2 -> 2.
      {0,1,7}: N1 = 2 (giant {0,6}, baby {0,1}): giant 0, 0, 6 -> 6; baby 0, 1, 1 -> 1.                       rotations {0,1,2,4,6,8}
    Decode: {0,1,7,8,9,15} with the repack mask 2 slots - 1 = 15: N1 = 4 (giant {0,4,8,12}, baby {0,1,3}: 2 / 3 < 1 ... N1 = 8: giant {0,8},
      baby {0,1,7}: 2 / 1 > 1 -> 8 / 2 = 4): giant 0,0,4,8,8,12 -> 4, 8, 12; baby 0,1,3,0,1,3 -> 1, 3.  {0,2,6}: 4, 2.  {0,4}: 0, 4.
                                                                                                               rotations {0,1,2,3,4,8,12}"""
    enc = dr.literal(E, 3, 6, 1, [1, 1, 1], dr.REPACK)
    dec = dr.literal(D, 3, 6, 1, [1, 1, 1], dr.REPACK)
    assert sorted(dr.rotations(enc, 5)) == [0, 1, 2, 4, 6, 8]
    assert sorted(dr.rotations(dec, 5)) == [0, 1, 2, 3, 4, 8, 12]
    assert dr.galois_elements(enc, 32) == sorted(pow(5, r, 64) for r in [0, 1, 2, 4, 6, 8])
    assert ltr.find_best_bsgs_ratio([0, 1, 7, 8, 9, 15], 16, 0) == 4 and ltr.find_best_bsgs_ratio([0, 2, 6], 16, 0) == 4


PINNED = list(itertools.product((8, 9), (E, D), (dr.STANDARD, dr.SPLIT, dr.REPACK), (False, True), ([1] * 6, [2, 1], [3])))


def test_index_maps_and_galois_elements_logn_10(rh):
    """LogN 10: the package against the restatement, as sorted sets (the order of a Go map is not an order), and the structure every map has:
    it is the set of diagonals GenMatrices fills, its size is at most 2^(levels collapsed + 1) - 1 (+ the repack doubling)"""
    for ls, tp, fmt, br, lv in PINNED:
        lit = dr.literal(tp, ls, 6, 1, lv, fmt, None, br)
        pk = rh.dft.MatrixLiteral(tp, ls, 6, 1, lv, fmt, None, br)
        maps = dr.index_maps(lit, 10)
        assert [sorted(m) for m in pk.computeBootstrappingDFTIndexMap(10)] == [sorted(m) for m in maps]
        assert sorted(pk.GaloisElements(1024)) == dr.galois_elements(lit, 1024)
        merge = dr.merge_plan(lit)
        assert sum(merge) == ls and len(maps) == sum(lv)
        for i, m in enumerate(maps):
            repack = ls < 9 and tp == D and i == 0 and fmt == dr.REPACK
            assert len(m) <= ((2 << merge[i]) - 1) * (2 if repack else 1)
    lit = dr.literal(E, 8, 6, 1, [1] * 6, dr.REPACK)                     # the reference's own test literal, sparse: merge 2, 2, 1, 1, 1, 1
    assert dr.merge_plan(lit) == [2, 2, 1, 1, 1, 1]
    assert [sorted(m) for m in dr.index_maps(lit, 10)][:3] == [[0, 64, 128, 192], [0, 16, 32, 48, 208, 224, 240], [0, 8, 248]]


# ---- GenMatrices against the dense transform ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("br", [False, True], ids=["natural", "bitreversed"])
@pytest.mark.parametrize("tp", [E, D], ids=["encode", "decode"])
@pytest.mark.parametrize("ls", [3, 4])
def test_gen_matrices_is_the_special_transform(ls, tp, br):
    """The product of the factors, applied with Diagonals.Evaluate, against the encoder restatement's transform of the same vector.  The encoder's
    IFFT is its butterflies followed by a bit reversal and its FFT a bit reversal followed by its butterflies (ckks_vector_ops.go:18-76); the
    factors are the butterflies alone, so in natural order
        encode: M x = BitReverse(IFFT(x))          decode: M x = FFT(BitReverse(x))
    and with BitReversed the permutation moves to the other side: encode: M x = IFFT(BitReverse(x)), decode: M x = BitReverse(FFT(x)).
    An encode carries 1 / slots (Standard) or 1 / (2 slots) (the split formats), spread over the factors; the encoder's IFFT carries 1 / slots.
    Float64 against float64 over at most 4 levels of 3-term sums: relative tolerance 2^-40."""
    n = 1 << ls
    rnd = random.Random("dense %d %d %s" % (ls, tp, br))
    x = np.array([complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(n)])
    brv = lambda y: cer.bit_reverse(y, n)

    def T(y):
        re, im = (cer.special_ifft if tp == E else cer.special_fft)(y.real, y.imag, 4 * n)
        return re + 1j * im
    if tp == E:
        want = T(brv(x)) if br else brv(T(x))
    else:
        want = brv(T(x)) if br else T(brv(x))
    for lv, fmt in itertools.product(([1] * ls, [2, 1], [1], [ls - 1]), (dr.STANDARD, dr.SPLIT, dr.REPACK)):
        lit = dr.literal(tp, ls, 6, 1, lv, fmt, None, br)
        v = list(x)
        mats = dr.gen_matrices(lit, ls + 1)                              # full packing: no repack matrix
        assert len(mats) == sum(lv)
        for m in mats:
            v = ltr.diagonals_evaluate(dr.as_complex(m), v)
        w = want / 2 if tp == E and fmt != dr.STANDARD else want
        assert np.max(np.abs(np.array(v) - w)) <= 2.0 ** -40 * np.max(np.abs(w)), (lv, fmt)


def test_sparse_repack_matrices_split_and_merge_the_halves():
    """LogSlots 3 in a ring with 16 slots, RepackImagAsReal: every diagonal has 2 slots entries.  Decode: the first factor carries the repack
    matrix [[1, i], [i, 1]] (:806-829), so a vector (vReal || vImag) comes out as FFT(BitReverse(vReal + i vImag)) in its first half.
    Encode: the second copy of the last factor is zeroed (:733-740)."""
    ls, n = 3, 8
    rnd = random.Random("sparse")
    re, im = [rnd.uniform(-1, 1) for _ in range(n)], [rnd.uniform(-1, 1) for _ in range(n)]
    v = [complex(a) for a in re + im]
    for m in dr.gen_matrices(dr.literal(D, ls, 6, 1, [1, 1], dr.REPACK), 5):
        assert all(len(d) == 2 * n for d in m.values())
        v = ltr.diagonals_evaluate(dr.as_complex(m), v)
    x = cer.bit_reverse(np.array(re) + 1j * np.array(im), n)
    wr, wi = cer.special_fft(x.real, x.imag, 4 * n)
    assert np.max(np.abs(np.array(v[:n]) - (wr + 1j * wi))) <= 2.0 ** -40 * np.max(np.abs(wr + 1j * wi))
    last = dr.gen_matrices(dr.literal(E, ls, 6, 1, [1, 1], dr.REPACK), 5)[-1]
    assert all(x == (0.0, 0.0) for d in last.values() for x in d[n:]) and any(x != (0.0, 0.0) for d in last.values() for x in d[:n])


# ---- decryption at the reference's setting ---------------------------------------------------------------------------------------------------------
LOGN, LOG_SCALE = 10, 45
BOUND = LOG_SCALE - (LOGN + 2)                                           # VerifyTestVectors (precision.go:92-103)


def keys_for(lit):
    N = 1 << LOGN
    return {g: tlo.galois_key(g) for g in set(dr.galois_elements(lit, N)) | {2 * N - 1} if g != 1}


def encrypt(tag, pt, level):
    N, Q, _ = tlo.prec45()
    ct, _ = rr.encrypt(random.Random("dft enc " + tag), tlo.secret(), [0] * N, Q, level)
    return [rr._add(ct[0], pt, [int(q) for q in Q[:level + 1]]), ct[1]]


def decrypt_coeffs(ct, scale):
    """Decrypt, then Decode with IsBatched = false: the N coefficients over the scale"""
    N, Q, _ = tlo.prec45()
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    sk = tlo.secret()
    ph = rr._vec("ADD", rr._vec("MUL_MONT", np.asarray(ct[1], dtype=np.uint64), sk.rows(mods), mods), np.asarray(ct[0], dtype=np.uint64), mods)
    return np.asarray(cer.decode_coeffs(ph, float(scale), N, mods, is_ntt=True), dtype=np.float64)


def precision(what, want, have):
    pr, pi = ltr.avg_log2_prec(want, np.real(have), np.imag(have), LOG_SCALE)
    print("MEASURED dft/%s prec45 LogN=%d  real %.2f imag %.2f  [>= %d]" % (what, LOGN, pr, pi, BOUND))
    assert pr >= BOUND and pi >= BOUND


def encode_case(log_slots):
    """testHomomorphicEncoding (dft_test.go:71-285): (values, the coefficient vector that is encoded): the bit-reversed values, real parts on
    the first half of the coefficients and imaginary parts on the second, with gaps when the packing is sparse (:174-183)"""
    N = 1 << LOGN
    slots = 1 << log_slots
    rnd = random.Random("dft encode %d" % log_slots)
    values = np.array([complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(slots)])
    brv = cer.bit_reverse(values, slots)
    gap = N // (2 * slots)
    coeffs = np.zeros(N)
    coeffs[0:slots * gap:gap] = brv.real
    coeffs[N >> 1:(N >> 1) + slots * gap:gap] = brv.imag
    return values, coeffs


@pytest.mark.parametrize("log_slots", [8, 9], ids=["sparse", "full"])
def test_coeffs_to_slots_decrypts_within_the_reference_bound(oracle, log_slots):
    """Encode/SparsePacking and Encode/FullPacking at testInsecurePrec45: LogN 10, the prec45 Q chain, scale 2^45, Levels [1] * 6,
    RepackImagAsReal.  The golden file's two P moduli are used: the reference's test has one 60-bit P, the device lintrans path (and with it this
    restatement's keys) needs two, and P does not enter the precision bound."""
    N, Q, P = tlo.prec45()
    level, slots = len(Q) - 1, 1 << log_slots
    lit = dr.literal(E, log_slots, level, len(P) - 1, [1] * level, dr.REPACK)
    values, coeffs = encode_case(log_slots)
    mods = [int(q) for q in Q]
    ct = encrypt("c2s %d" % log_slots, cer.encode_coeffs(coeffs, 2.0 ** LOG_SCALE, N, mods, is_ntt=True), level)
    lts = dr.new_matrix(N, Q, P, lit)
    (re, rs), imag = dr.coeffs_to_slots(N, Q, P, ct, 1 << LOG_SCALE, log_slots, lit, lts, keys_for(lit))
    assert re[0].shape[0] == 1                                           # six rescalings: level 0
    if log_slots < LOGN - 1:
        assert imag is None
        have = decrypt_coeffs(re, rs.float64())
        vr, vi = cer.special_ifft(np.concatenate([values.real, values.imag]), np.zeros(2 * slots), 2 * N)     # (:213-227)
        gap = N // (4 * slots)
        idx = np.arange(2 * slots) * gap
        precision("encode sparse", np.concatenate([vr, vi]), np.concatenate([have[idx], have[(N >> 1) + idx]]))
    else:
        (im, ims) = imag
        for what, ctx, s, part in (("encode full real", re, rs, values.real), ("encode full imag", im, ims, values.imag)):
            have = decrypt_coeffs(ctx, s.float64())
            vr, vi = cer.special_ifft(part, np.zeros(slots), 2 * N)      # (:254-279)
            precision(what, np.concatenate([vr, vi]), have)


@pytest.mark.parametrize("log_slots", [8, 9], ids=["sparse", "full"])
def test_slots_to_coeffs_decrypts_within_the_reference_bound(oracle, log_slots):
    """Decode/SparsePacking and Decode/FullPacking (dft_test.go:287-432): the coefficients of the output are the values bit-reversed, real parts
    on the first half and imaginary parts on the second"""
    N, Q, P = tlo.prec45()
    level, slots = len(Q) - 1, 1 << log_slots
    sparse = log_slots < LOGN - 1
    lit = dr.literal(D, log_slots, level, len(P) - 1, [1] * level, dr.REPACK)
    rnd = random.Random("dft decode %d" % log_slots)
    vr = np.array([rnd.uniform(-1, 1) for _ in range(slots)])
    vi = np.array([rnd.uniform(-1, 1) for _ in range(slots)])
    mods = [int(q) for q in Q]
    scale = 2.0 ** LOG_SCALE
    if sparse:                                                           # both vectors in one plaintext of 2 slots values (:373-378)
        v = np.concatenate([vr + 1j * vi, np.zeros(slots)])
        ct0, ct1 = encrypt("s2c", cer.embed(v, log_slots + 1, scale, N, mods, True, False), level), None
    else:
        ct0 = encrypt("s2c re", cer.embed(vr.astype(complex), log_slots, scale, N, mods, True, False), level)
        ct1 = encrypt("s2c im", cer.embed(vi.astype(complex), log_slots, scale, N, mods, True, False), level)
    lts = dr.new_matrix(N, Q, P, lit)
    out, s = dr.slots_to_coeffs(N, Q, P, ct0, 1 << LOG_SCALE, ct1, 1 << LOG_SCALE, lit, lts, keys_for(lit))
    have = decrypt_coeffs(out, s.float64())
    gap = N // (2 * slots)
    idx = np.arange(slots) * gap
    precision("decode " + ("sparse" if sparse else "full"), cer.bit_reverse(vr + 1j * vi, slots), have[idx] + 1j * have[idx + (N >> 1)])


# ---- the package's host side ------------------------------------------------------------------------------------------------------------------------
def test_matrix_literal_json_round_trip(rh):
    """testDFTMatrixLiteralMarshalling (dft_test.go:47-69), and the field names and the Scaling forms of the reference's JSON"""
    d = rh.dft
    m = d.MatrixLiteral(LogSlots=15, Type=d.HomomorphicDecode, Format=d.RepackImagAsReal, LevelQ=12, LevelP=1, LogBSGSRatio=2, Levels=[1, 1, 1], BitReversed=True)
    data = m.MarshalBinary()
    assert d.MatrixLiteral.UnmarshalBinary(data) == m
    assert json.loads(data) == {"Type": 1, "LogSlots": 15, "LevelQ": 12, "LevelP": 1, "Levels": [1, 1, 1], "Format": 2, "Scaling": None, "BitReversed": True,
                                "LogBSGSRatio": 2}
    assert list(json.loads(data)) == ["Type", "LogSlots", "LevelQ", "LevelP", "Levels", "Format", "Scaling", "BitReversed", "LogBSGSRatio"]
    for s, text in ((0.5, "0.5"), (4096.0, "4096"), (1.0 / 3, "0.3333333333333333"), (2.0 ** 40, "1.099511627776e+12"), (2.0 ** -20, "9.5367431640625e-07")):
        m.Scaling = s
        got = json.loads(m.MarshalBinary())["Scaling"]
        assert got == text and d.MatrixLiteral.UnmarshalBinary(m.MarshalBinary()).Scaling == s


def test_package_host_side_matches_the_restatement(rh):
    d = rh.dft
    for tp, fmt, br, (logN, ls, lv) in itertools.product((E, D), (0, 1, 2), (False, True), ((5, 3, [1, 1, 1]), (5, 3, [1]), (5, 4, [2, 1]), (5, 4, [1, 1]), (10, 8, [3, 3]))):
        lit = dr.literal(tp, ls, 6, 1, lv, fmt, 0.75, br)
        pk = d.MatrixLiteral(tp, ls, 6, 1, lv, fmt, 0.75, br)
        assert (pk.Depth(True), pk.Depth(False)) == (len(lv), sum(lv)) == (dr.depth(lit, True), dr.depth(lit, False))
        assert pk._merge() == dr.merge_plan(lit) and pk._scaling() == dr.scaling_of(lit)
        want = dr.gen_matrices(lit, logN)
        got = pk.GenMatrices(logN, device=False)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert sorted(g) == sorted(w)
            for k in w:
                wv = np.array([complex(*x) for x in w[k]])
                assert np.array_equal(g[k].real, wv.real) and np.array_equal(g[k].imag, wv.imag) and not np.isnan(g[k]).any(), (tp, fmt, br, lv, k)
    with pytest.raises(rh.RingHipError, match=r"LogSlots = 10 outside \[1, LogN - 1 = 9\]"):
        d.MatrixLiteral(E, 10, 6, 1, [1]).GenMatrices(10, device=False)
    with pytest.raises(rh.RingHipError, match="device=True needs a ring"):
        d.MatrixLiteral(E, 3, 6, 1, [1]).GenMatrices(5, device=True)


def golden_moduli():
    with open(os.path.join(ROOT, "tests", "golden", "ckks_test_moduli.json")) as f:
        g = json.load(f)
    return [int(q) for name in ("prec45", "prec90") for q in g[name]["Q"]]


def test_kth_root_scale(rh):
    """root^k is within one 128-bit ulp of the scale (relative 2^-127 per factor: k ulps of the root, to first order), the package and the
    restatement agree to the last bit, and Float64 is the correctly rounded float of the exact root"""
    for q in golden_moduli():
        for k in (2, 3):
            r = rh.dft.ScaleRoot(rh.ckks.Scale(q), k).Value
            assert r == dr.kth_root_scale(q, k).v
            assert r == cr.round_bits(r, 128)
            assert abs(r ** k - q) <= k * q * Fraction(1, 1 << 127)
            ulp = Fraction(1, 1 << (127 - (r.numerator.bit_length() - r.denominator.bit_length())))
            assert (r - ulp) ** k < q < (r + ulp) ** k
    assert rh.dft.ScaleRoot(rh.ckks.Scale(1 << 40), 2).Value == 1 << 20 and rh.dft.ScaleRoot(rh.ckks.Scale(7), 1).Value == 7


def test_entries_are_declared_exported_and_check_their_arguments(rh):
    L = rh.lib()
    txt = open(os.path.join(ROOT, "include", "ringhip.h")).read()
    names = ("rh_ckks_split_real_imag", "rh_ckks_merge_real_imag", "rh_ckks_dft_level_vectors", "rh_ckks_dft_merge_level", "rh_ckks_dft_finish")
    for name in names:
        assert name + "(" in txt and hasattr(L, name)
    assert L.rh_ckks_split_real_imag(None, 0, None, None, None, None, 1, None, None) == -1 and b"rh_ckks_split_real_imag: null ring handle" in L.rh_last_error()
    assert L.rh_ckks_merge_real_imag(None, 0, None, None, None, 1, None, None) == -1 and b"rh_ckks_merge_real_imag: null ring handle" in L.rh_last_error()
    assert L.rh_ckks_dft_level_vectors(None, 0, 3, 8, 1, 0, None, 33, None, 4, None) == -1 and b"rh_ckks_dft_level_vectors: null ring handle" in L.rh_last_error()
    assert L.rh_ckks_dft_merge_level(None, 8, 0, None, None, 0, None, 1, None, None, 0) == -1 and b"rh_ckks_dft_merge_level: null ring handle" in L.rh_last_error()
    assert L.rh_ckks_dft_finish(None, 8, 1, None, None, 1.0, 0, None, None, 0) == -1 and b"rh_ckks_dft_finish: null ring handle" in L.rh_last_error()
    assert set(rh.dft.Evaluator.FUSED_DFT) == {"split", "merge"}
    assert (rh.dft.HomomorphicEncode, rh.dft.HomomorphicDecode, rh.dft.Standard, rh.dft.SplitRealAndImag, rh.dft.RepackImagAsReal) == (0, 1, 0, 1, 2)

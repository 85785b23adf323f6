"""CPU: linear transformations (circuits/common/lintrans, circuits/ckks/lintrans).  The index arithmetic pinned to hand-derived values, the plain
evaluation pinned to dense matrix-vector products in exact rationals, the restatement the device path is compared with
(tests/lintrans_restatement.py) pinned to decryption at the reference's own test parameters, and the package's host side against the restatement."""
import functools
import json
import os
import random
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_restatement as cer
import lintrans_restatement as ltr
import rlwe_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIAGS = [-15, -4, -1, 0, 1, 2, 3, 4, 15]                            # lintrans_test.go:150
SMALL_DIAGS = [-5, -1, 0, 1, 2, 3, 7]


# ---- index arithmetic ----------------------------------------------------------------------------------------------------------------------------
def test_bsgs_index_and_ratio_are_pinned():
    """BSGSIndex(diags, slots, N1): rot = d mod slots, giant step floor(rot / N1) N1, baby step rot mod N1.  FindBestBSGSRatio(diags, slots, r) walks
    N1 = 1, 2, 4 ... and compares (#baby - 1) / (#giant - 1) with 2^r: equal returns N1, larger returns N1 / 2.

    REF_DIAGS, slots 512: rot = [497, 508, 511, 0, 1, 2, 3, 4, 15].
      N1 = 1: 9 giant, 1 baby: 0 / 8.   N1 = 2: giant {496, 508, 510, 0, 2, 4, 14} baby {0, 1}: 1 / 6.
      N1 = 4: giant {496, 508, 0, 4, 12} baby {0, 1, 2, 3}: 3 / 4 = 0.75.
      N1 = 8: 497 = 496 + 1, 508 = 504 + 4, 511 = 504 + 7, 0 .. 4 = 0 + (0 .. 4), 15 = 8 + 7: giant {0, 8, 496, 504}, baby {0, 1, 2, 3, 4, 7}: 5 / 3 = 1.67.
      N1 = 16: 497 = 496 + 1, 508 = 496 + 12, 511 = 496 + 15, 15 = 0 + 15: giant {0, 496}, baby {0, 1, 2, 3, 4, 12, 15}: 6 / 1 = 6.
      ratio 1 (2.0): 0, 0.17, 0.75, 1.67 stay below, 6 passes: 16 / 2 = 8.   ratio 0 (1.0): 0.75 stays below, 1.67 passes: 8 / 2 = 4.
    SMALL_DIAGS, slots 16: rot = [11, 15, 0, 1, 2, 3, 7].
      N1 = 1: 0 / 6.   N1 = 2: giant {10, 14, 0, 2, 6} baby {0, 1}: 1 / 4.   N1 = 4: 11 = 8 + 3, 15 = 12 + 3, 7 = 4 + 3: giant {0, 4, 8, 12}, baby {0, 1, 2, 3}: 3 / 3 = 1.
      N1 = 8: 11 = 8 + 3, 15 = 8 + 7, 0 .. 3, 7 = 0 + 7: giant {0, 8}, baby {0, 1, 2, 3, 7}: 4 / 1 = 4.
      ratio 1 (2.0): 1 stays below, 4 passes: 8 / 2 = 4.   ratio 2 (4.0): 4 equals: 8."""
    assert ltr.find_best_bsgs_ratio(REF_DIAGS, 512, 1) == 8
    index, n1, n2 = ltr.bsgs_index(REF_DIAGS, 512, 8)
    assert (n1, n2) == ([0, 8, 496, 504], [0, 1, 2, 3, 4, 7])
    assert index == {0: [0, 1, 2, 3, 4], 8: [7], 496: [1], 504: [4, 7]}
    assert ltr.find_best_bsgs_ratio(REF_DIAGS, 512, 0) == 4
    assert ltr.bsgs_index(REF_DIAGS, 512, 4)[1] == [0, 4, 12, 496, 508]
    assert ltr.find_best_bsgs_ratio(SMALL_DIAGS, 16, 1) == 4
    _, n1, n2 = ltr.bsgs_index(SMALL_DIAGS, 16, 4)
    assert (n1, n2) == ([0, 4, 8, 12], [0, 1, 2, 3])
    assert ltr.find_best_bsgs_ratio(SMALL_DIAGS, 16, 2) == 8
    assert ltr.bsgs_index(SMALL_DIAGS, 16, 8)[0] == {0: [0, 1, 2, 3, 7], 8: [3, 7]}


def test_ratio_division_follows_go_floats():
    """one giant step: (#baby - 1) / 0 is +Inf in Go and passes every ratio (N1 / 2); 0 / 0 is NaN, both comparisons are false and the walk goes on"""
    assert ltr.find_best_bsgs_ratio([0, 1], 16, 1) == 1                  # N1 = 1: 0 / 1; N1 = 2: giant {0}, baby {0, 1}: 1 / 0 = +Inf > 2: 2 / 2
    assert ltr.find_best_bsgs_ratio([0], 16, 1) == 1                     # 0 / 0 at every N1: the loop runs out and returns 1
    assert ltr.find_best_bsgs_ratio([0, 8], 16, 0) == 1                  # N1 = 1 .. 8: 0 / 1 < 1; the loop runs out


def test_galois_elements_are_pinned():
    """BSGS: 5^r mod 2N for the union of giant and baby steps; without BSGS: for every rotation (BSGSIndex with N1 = slots makes every rotation a
    baby step), the rotation by 0 (element 1) included"""
    N = 1024
    want = sorted(pow(5, r, 2 * N) for r in [0, 8, 496, 504, 1, 2, 3, 4, 7])
    assert ltr.galois_elements(N, REF_DIAGS, 512, 1) == want
    assert ltr.galois_elements(N, REF_DIAGS, 512, -1) == sorted(pow(5, r % 512, 2 * N) for r in REF_DIAGS)


# ---- rational identities -------------------------------------------------------------------------------------------------------------------------
def dense(diags, slots):
    """row k, column (k + d) mod slots holds diagonal d's entry k: the matrix whose diagonal traversal is `diags` (lintrans.go:24-46)"""
    M = [[Fraction(0)] * slots for _ in range(slots)]
    for d, v in diags.items():
        for k in range(slots):
            M[k][(k + d) % slots] += v[k]
    return M


@pytest.mark.parametrize("slots,idx", [(16, SMALL_DIAGS), (16, [0]), (32, [-15, -4, -1, 0, 1, 2, 3, 4, 15]), (8, list(range(8)))])
def test_diagonals_evaluate_is_the_dense_product(slots, idx):
    rnd = random.Random("dense %d %s" % (slots, idx))
    diags = {d: [Fraction(rnd.randrange(-9, 10), rnd.randrange(1, 5)) for _ in range(slots)] for d in idx}
    vec = [Fraction(rnd.randrange(-9, 10), rnd.randrange(1, 5)) for _ in range(slots)]
    M = dense(diags, slots)
    want = [sum(M[k][c] * vec[c] for c in range(slots)) for k in range(slots)]
    assert ltr.diagonals_evaluate(diags, vec) == want


def test_permutation_diagonals_apply_the_permutation():
    log_slots = 4
    slots = 1 << log_slots
    rnd = random.Random("perm")
    to = list(range(slots))
    rnd.shuffle(to)
    perm = [(i, to[i], Fraction(rnd.randrange(1, 9), 3)) for i in range(slots // 2)]      # a partial permutation, as lintrans_test.go:249
    diags = ltr.permutation_diagonals(perm, log_slots)
    vec = [Fraction(rnd.randrange(-9, 10)) for _ in range(slots)]
    want = [Fraction(0)] * slots
    for frm, t, s in perm:
        want[t] = s * vec[frm]
    assert ltr.diagonals_evaluate(diags, vec) == want


def test_at_as_written():
    m = {-1: "a", 3: "b"}
    assert ltr.diagonals_at(m, 3, 16) == "b" and ltr.diagonals_at(m, 15, 16) == "a"
    with pytest.raises(KeyError, match=r"cannot At\[0\]"):
        ltr.diagonals_at(m, -3, 16)                                     # a missing negative index: the second arm reads the local j, not i
    with pytest.raises(KeyError, match=r"cannot At\[5 or -11\]"):
        ltr.diagonals_at(m, 5, 16)


# ---- decryption at the reference's test parameters -------------------------------------------------------------------------------------------------
LOGN, LOG_SCALE = 10, 45


@functools.lru_cache(maxsize=None)
def prec45():
    with open(os.path.join(ROOT, "tests", "golden", "ckks_test_moduli.json")) as f:
        g = json.load(f)["prec45"]
    return 1 << LOGN, tuple(g["Q"]), tuple(g["P"])


@functools.lru_cache(maxsize=None)
def secret():
    return rr.Secret.sample(random.Random("lintrans sk"), 1 << LOGN)


@functools.lru_cache(maxsize=None)
def galois_key(g):
    N, Q, P = prec45()
    return rr.galois_key(random.Random("lintrans gk %d" % g), secret(), g, Q, P, len(Q) - 1, len(P) - 1)


def new_test_vector(tag, N, Q, level, log_slots, scale):
    """NewTestVector(-1-1i, 1+1i) (schemes/ckks/test_utils.go): uniform values in the box, encoded at `scale` and encrypted under the secret key"""
    rnd = random.Random("values " + tag)
    values = np.array([complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(1 << log_slots)])
    mods = [int(q) for q in Q[:level + 1]]
    pt = cer.embed(values, log_slots, float(scale), N, mods, True, False)
    ct, _ = rr.encrypt(random.Random("enc " + tag), secret(), [0] * N, Q, level)
    return values, [rr._add(ct[0], pt, mods), ct[1]]


def reference_case(case):
    N = 1 << LOGN
    slots = N >> 1
    if case == "permutation":                                            # lintrans_test.go:239-264
        rnd = random.Random("permutation")
        idx = list(range(slots))
        rnd.shuffle(idx)
        idx = idx[:slots >> 1]
        perm = [(i, idx[i], complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1))) for i in range(len(idx))]
        return ltr.permutation_diagonals(perm, LOGN - 1), 1
    if case == "bsgs":                                                   # :150-161: ones on the first half of every diagonal
        return {d: [1.0 if j < slots >> 1 else 0.0 for j in range(slots)] for d in REF_DIAGS}, 1
    return {d: [1.0] * slots for d in REF_DIAGS}, -1                     # :197-209


@pytest.mark.parametrize("case", ["bsgs", "naive", "permutation"])
def test_restatement_decrypts_within_the_reference_bound(oracle, case):
    """LinearTransform/BSGS=True, BSGS=False and Permutation (lintrans_test.go:144-290) at prec45, LogN 10, scale 2^45: the transformation encoded at
    scale Q[level], evaluated on an encryption under a real key, decrypted at scale 2^45 Q[level] (the test does not rescale) and compared with
    Diagonals.Evaluate of the values.  VerifyTestVectors (precision.go:92-103) asks log2(DefaultScale) - (LogN + 2) = 33 bits of the average
    precision of the real and of the imaginary parts."""
    N, Q, P = prec45()
    level, log_slots = len(Q) - 1, LOGN - 1
    slots = 1 << log_slots
    diags, ratio = reference_case(case)
    values, ct = new_test_vector(case, N, Q, level, log_slots, 2.0 ** LOG_SCALE)
    lt = ltr.encode(N, Q, P, diags, list(diags), level, len(P) - 1, float(Q[level]), log_slots, ratio)
    assert (lt.N1 == 0) == (ratio < 0)
    keys = {g: galois_key(g) for g in ltr.galois_elements(N, list(diags), slots, ratio) if g != 1}
    out = ltr.evaluate_many(N, Q, P, ct, [lt], keys)[0]
    want = ltr.diagonals_evaluate(diags, [complex(v) for v in values])
    re, im = ltr.decrypt_slots(out, secret(), N, Q, log_slots, 2.0 ** LOG_SCALE * float(Q[level]))
    pr, pi = ltr.avg_log2_prec(want, re, im, LOG_SCALE)
    bound = LOG_SCALE - (LOGN + 2)
    print("MEASURED lintrans/%s prec45 LogN=%d  real %.2f imag %.2f  [>= %d]" % (case, LOGN, pr, pi, bound))
    assert pr >= bound and pi >= bound


# ---- the package's host side against the restatement -----------------------------------------------------------------------------------------------
CASES = [(REF_DIAGS, 512), (SMALL_DIAGS, 16), ([0], 16), ([0, 1], 16), (list(range(64)), 64), ([3, -3, 17, 40], 64)]


def test_package_index_arithmetic_matches_the_restatement(rh):
    lt = rh.lintrans
    for diags, slots in CASES:
        for ratio in (0, 1, 2, 3):
            n1 = lt.FindBestBSGSRatio(diags, slots, ratio)
            assert n1 == ltr.find_best_bsgs_ratio(diags, slots, ratio), (diags, slots, ratio)
            if n1:
                assert lt.BSGSIndex(diags, slots, n1) == ltr.bsgs_index(diags, slots, n1)
        for ratio in (-1, 0, 1, 2):
            assert sorted(lt.GaloisElements(1024, diags, slots, ratio)) == ltr.galois_elements(1024, diags, slots, ratio)
    assert lt.FindBestBSGSRatio(REF_DIAGS, 512, 1) == 8 and lt.FindBestBSGSRatio(REF_DIAGS, 512, 0) == 4
    assert lt.BSGSIndex(REF_DIAGS, 512, 8) == ({0: [0, 1, 2, 3, 4], 8: [7], 496: [1], 504: [4, 7]}, [0, 8, 496, 504], [0, 1, 2, 3, 4, 7])
    p = lt.Parameters(REF_DIAGS, 6, 1, 2.0 ** 45, 9, 1)
    assert sorted(p.GaloisElements(1024)) == ltr.galois_elements(1024, REF_DIAGS, 512, 1)


def test_package_diagonals_and_permutation_match_the_restatement(rh):
    lt = rh.lintrans
    rnd = random.Random("pkg diags")
    for idx, slots in ((SMALL_DIAGS, 16), ([-15, -4, -1, 0, 1, 2, 3, 4, 15], 32)):
        d = {i: [Fraction(rnd.randrange(-9, 10), 3) for _ in range(slots)] for i in idx}
        vec = [Fraction(rnd.randrange(-9, 10), 7) for _ in range(slots)]
        D = lt.Diagonals(d)
        assert sorted(D.DiagonalsIndexList()) == sorted(idx)
        assert D.Evaluate(vec) == ltr.diagonals_evaluate(d, vec)
    D = lt.Diagonals({-1: "a", 3: "b"})
    assert D.At(3, 16) == "b" and D.At(15, 16) == "a"
    with pytest.raises(rh.RingHipError, match=r"cannot At\[0\]: diagonal does not exist"):
        D.At(-3, 16)
    with pytest.raises(rh.RingHipError, match=r"cannot At\[5 or -11\]: diagonal does not exist"):
        D.At(5, 16)
    to = list(range(16))
    rnd.shuffle(to)
    perm = [(i, to[i], Fraction(rnd.randrange(1, 9), 3)) for i in range(8)]
    got = lt.Permutation([lt.PermutationMapping(*m) for m in perm]).GetDiagonals(4)
    assert dict(got) == ltr.permutation_diagonals(perm, 4) and isinstance(got, lt.Diagonals)


def test_entries_are_declared_exported_and_check_their_arguments(rh):
    L = rh.lib()
    txt = open(os.path.join(ROOT, "include", "ringhip.h")).read()
    for name in ("rh_rlwe_diag_mac_qp", "rh_rlwe_diag_mac_qp_table_words", "rh_rlwe_rotate_sum_accumulate_qp", "rh_rlwe_rotate_mul_accumulate_qp"):
        assert name + "(" in txt and hasattr(L, name)
    assert L.rh_rlwe_diag_mac_qp_table_words(7, 15, 1) == 7 * 6 and L.rh_rlwe_diag_mac_qp_table_words(-1, 15, 1) == 0
    assert L.rh_rlwe_diag_mac_qp(None, 0, 0, 0, None, None, None, None, None, None, None, 1, None, 0) == -1
    assert b"rh_rlwe_diag_mac_qp: null basis extender" in L.rh_last_error()
    assert L.rh_rlwe_rotate_sum_accumulate_qp(None, 0, 0, 5, *([None] * 10), 1, 1) == -1
    assert b"rh_rlwe_rotate_sum_accumulate_qp: null basis extender" in L.rh_last_error()
    assert L.rh_rlwe_rotate_mul_accumulate_qp(None, 0, 0, 5, *([None] * 11), 1, 1) == -1
    assert b"rh_rlwe_rotate_mul_accumulate_qp: null basis extender" in L.rh_last_error()
    assert set(rh.lintrans.Evaluator.FUSED_LINTRANS) == {"diag_mac", "giant_tail", "naive_step"}

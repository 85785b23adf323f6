"""CPU: the restated noise meters (tests/noise_restatement.py) pinned three ways -- by hand on N = 4 vectors, to the reference's own loops restated
step for step at the precisions Go runs them (ring/ring.go:661-685 at 128 bits, NormStats with 64-bit mantissas), and to the bounds the
reference's tests state on restatement keys (core/rlwe/rlwe_test.go:451-464, :509, :559, :578; core/rgsw/rgsw_test.go:43-55) -- and the host half
of the device path: the assembly of rh_ring_centered_moments' pair sums, the finishing functions, the entries' checks that need no device."""
import math
import random

import numpy as np
import pytest

import noise_restatement as nr
import rlwe_restatement as rr
import test_keygen_oracle as tko
import test_rlwe_oracle as tro
from conftest import QI60

WIDE = [0x1fffffffffe00001, 0xffffee001, 0xfd801]            # 61 / 36 / 20 bits: primes = 1 mod 2^11


# ---- by hand ----------------------------------------------------------------------------------------------------------------------------------------------
def test_centred_crt_and_moments_by_hand():
    mods = [5, 7]                                              # M = 35, floor(M / 2) = 17
    vals = [0, 16, 17, 34]                                     # 17 is already negative: the `>=`
    limbs = [[v % 5 for v in vals], [v % 7 for v in vals]]
    xs = nr.centred(limbs, mods)
    assert xs == [0, 16, -18, -1]
    assert nr.moments(xs) == (4, -3, 0 + 256 + 324 + 1, 0, 18)
    assert nr.centred(limbs, mods, gap=2) == [0, -18]
    # var = (581 - 9 / 4) / 3 = 2315 / 12
    assert nr.log2_std_of(xs) == pytest.approx(0.5 * math.log2(2315 / 12), abs=1e-15)
    std, lo, hi = nr.norm_stats(xs)
    assert std == pytest.approx(0.5 * math.log2(2315 / 16), abs=1e-15) and lo == -math.inf and hi == math.log2(18)
    assert nr.norm_stats([3, -3, 3, -3]) == (math.log2(3), math.log2(3), math.log2(3))
    assert nr.log2_std_of([7, 7, 7, 7]) == -math.inf and math.isnan(nr.log2_std_of([7]))
    # residues at or above the modulus are reduced first
    assert nr.centred([[5 + 2], [7 + 2]], mods) == [2]


def test_mixed_radix_model_by_hand():
    mods = [5, 7]
    assert nr.mixed_radix(17, mods) == [2, 3] and nr.mixed_radix(34, mods) == [4, 6]
    blk = nr.moments_block([[0, 1, 2, 4], [0, 2, 3, 6]], mods)          # v = 0, 16, 17, 34 -> digits (0,0) (1,3) (2,3) (4,6), c = 0 0 1 1
    P = lambda k: blk[3 * k] | blk[3 * k + 1] << 64 | blk[3 * k + 2] << 128
    # rows d0 = 0 1 2 4, d1 = 0 3 3 6, ones, c: the upper triangle of 4 x 4, row-major
    assert [P(k) for k in range(10)] == [21, 33, 7, 6, 54, 12, 9, 4, 2, 2]
    assert blk[30:] == [0, 0, 3, 3]                                     # |x|: 0 and 18 = 3 + 5 * 3


# ---- the host half of the device path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mods", [[QI60[0]], WIDE, QI60[:9], QI60[:5] + [97, 193]], ids=["1", "wide", "9", "mixed"])
def test_assembly_of_the_pair_sums_gives_the_exact_moments(rh, mods):
    noise = rh.noise
    rnd = random.Random("assembly %d" % len(mods))
    M = rr.prod(mods)
    half = M >> 1
    N = 16
    for what in ("uniform", "edges", "small"):
        if what == "uniform":
            vals = [rnd.randrange(M) for _ in range(N)]
        elif what == "edges":
            vals = [0, M - 1, half, half - 1, half + 1, 1] + [half - 1, (half + 2) % M] * 5
        else:
            vals = [rnd.randrange(-20, 21) % M for _ in range(N)]
        limbs = [[v % m for v in vals] for m in mods]
        for gap in (1, 4):
            want = nr.moments(nr.centred(limbs, mods, gap))
            assert noise.assemble_moments(nr.moments_block(limbs, mods, gap), mods, N // gap) == want
            assert noise.moments_of(nr.centred(limbs, mods, gap)) == want
    assert noise.moments_words(len(mods)) == len(nr.moments_block([[0] * 4] * len(mods), mods))


def test_finishing_functions_agree_bit_for_bit(rh):
    noise = rh.noise
    rnd = random.Random("finish")
    for bits in (3, 40, 200, 1800):
        xs = [rnd.randrange(-(1 << bits), 1 << bits) for _ in range(64)] + [0]
        n, S1, S2, lo, hi = nr.moments(xs)
        assert noise.log2_std(n, S1, S2) == nr.log2_std(n, S1, S2)
        assert noise.NormStats(xs) == nr.norm_stats(xs)
        assert rh.rlwe.NormStats(xs)[1] == -math.inf
    assert noise.log2_std(4, 28, 196) == -math.inf and math.isnan(noise.log2_std(1, 5, 25))


# ---- the Go loops -------------------------------------------------------------------------------------------------------------------------------------------
def _close(a, b):
    return a == b or abs(a - b) <= 2.0 ** -40


@pytest.mark.parametrize("bits", [4, 61, 120, 510, 1000])
def test_exact_finishing_matches_the_go_loops(bits):
    """the agreement in log2 is within 2^-40: N relative roundings of 2^-127 (ring.go) or 2^-63 (NormStats) bound the difference by N 2^-63 relative,
    far below, for N <= 2^17"""
    rnd = random.Random("go %d" % bits)
    for N, shift in ((64, 0), (1024, 0), (256, 1 << (bits - 1))):       # the last: a large mean, where the subtraction cancels
        xs = [rnd.randrange(-(1 << bits), 1 << bits) + shift for _ in range(N)]
        assert _close(nr.log2_std_of(xs), nr.go_log2_std(xs))
        if bits <= 61:
            assert all(_close(a, b) for a, b in zip(nr.norm_stats(xs), nr.go_norm_stats(xs)))


def test_go_overflows_where_the_exact_finishing_does_not():
    """Go rounds the standard deviation to float64 BEFORE math.Log2 (ring.go:683-685): from 2^1024 on (a uniform poly modulo 18 or more 60-bit
    limbs) it reports +Inf; the exact finishing takes the logarithm first"""
    rnd = random.Random("overflow")
    xs = [rnd.randrange(-(1 << 1800), 1 << 1800) for _ in range(64)]
    assert nr.go_log2_std(xs) == math.inf and 1798 < nr.log2_std_of(xs) < 1800


def test_uniform_poly_has_the_uniform_law():
    rnd = random.Random("uniform law")
    mods = QI60[:9]
    M = rr.prod(mods)
    limbs = rr.uniform_poly(rnd, 4096, mods)
    assert abs(nr.log2_std_of(nr.centred(limbs, mods)) - math.log2(M / math.sqrt(12))) < 0.05


# ---- the reference's bounds on restatement keys -----------------------------------------------------------------------------------------------------------
BOUND_CASES = [c for c in tko.CASES if c[0] == "TAIL"] + [("REF", (16, 1), None), ("REF", (2, 0), None)]


@pytest.mark.parametrize("case", BOUND_CASES, ids=tko._ids)
def test_restatement_keys_sit_under_the_reference_bounds(oracle, case):
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    sk, sk_out = tko.secrets(case[0])
    k = tko.keys(case)
    bound = nr.evk_bound(levelQ, levelP)
    got = {"evk": nr.noise_evaluation_key(k["evk"], sk, sk_out, Q, P), "rlk": nr.noise_relin_key(k["rlk"], sk, Q, P)}
    for g, gk in zip(tko.galois_elements(N), k["gks"]):
        got["gk%d" % g] = nr.noise_galois_key(gk, g, sk, Q, P)
    for what, v in got.items():
        print("MEASURED %-6s %s %5.2f [%.2f]" % (what, tko._ids(case), v, bound))
        assert 0 < v <= bound, what
    Pall = [int(p) for p in tro.chain(case[0])[2]]
    pkq, pkp = k["pk"]
    v = nr.noise_public_key(pkq, pkp, sk, Q, Pall)
    assert v <= nr.pk_bound()
    # a key measured against the wrong input secret is far above: the phase keeps P 2^(j pw2) (skIn - skOut)
    assert nr.noise_evaluation_key(k["evk"], sk_out, sk_out, Q, P) > bound + 10


def test_restated_rgsw_ciphertext_sits_under_the_reference_bound(oracle):
    N, Q, P, _ = tro.chain("TAIL")
    rnd = random.Random("rgsw noise")
    sk = rr.Secret.sample(rnd, N)
    m = [rnd.randrange(-1, 2) for _ in range(N)]
    for levelP, pw2 in ((3, 0), (0, 16)):
        keys = rr.rgsw_encrypt(rnd, sk, m, Q, P, 6, levelP, pw2)
        left, right = nr.noise_rgsw(keys, rr.small_ntt_mont(m, N, Q[:7]), sk, Q, P)
        assert 0 < left <= nr.RGSW_BOUND and 0 < right <= nr.RGSW_BOUND


def test_noise_below_one_reports_zero(oracle):
    """the running maximum starts at 0 (utils.go:83, :95): a key with no error at all has a phase of zero, log2 = -inf, and reports 0"""
    N, Q, P, _ = tro.chain("TAIL")
    sk = tko.secrets("TAIL")[0]
    a = rr.uniform_poly(random.Random("noiseless"), N, list(Q[:3]))[None].repeat(3, axis=0)
    kq, kp, dpl = __import__("keygen_restatement").gadget(sk, sk.rows(Q[:3]), Q, P, 2, -1, 0, a, np.zeros((3, N), dtype=np.int64))
    key = rr.GadgetKey(kq, kp, 2, -1, 0, dpl)
    assert nr.noise_gadget_list(key, sk.rows(Q[:3]), sk, Q, P) == [-math.inf]
    assert nr.noise_gadget(key, sk.rows(Q[:3]), sk, Q, P) == 0.0


# ---- the entries, without a device ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_exported_and_check_their_arguments(rh):
    L = rh.lib()
    assert L.rh_ring_centered_moments_words(30) == 3 * (32 * 33 // 2) + 60 and L.rh_ring_centered_moments_words(0) == 0
    assert L.rh_rlwe_gadget_phase_table_words(4, 3, 5) == 3 * (6 + 5 + 5) and L.rh_rlwe_gadget_phase_table_words(-1, 3, 5) == 0
    assert L.rh_ring_centered_moments(None, 0, None, 1, None, 0, None, 0, 1, 1, None) == -1
    assert b"rh_ring_centered_moments: null ring handle" in L.rh_last_error()
    assert L.rh_rlwe_gadget_phase(None, None, 0, 0, None, None, 1, None, 0, None, None, None, 0, 1, None, 0) == -1
    assert b"rh_rlwe_gadget_phase: null ring handle" in L.rh_last_error()
    assert set(rh.rlwe.FUSED_NOISE) == {"gadget_phase", "moments"} and all(rh.rlwe.FUSED_NOISE.values())
    for name in ("NoisePublicKey", "NoiseRelinearizationKey", "NoiseGaloisKey", "NoiseGaloisKeys", "NoiseGadgetCiphertext", "NoiseEvaluationKey", "Norm", "NormStats"):
        assert callable(getattr(rh.rlwe, name))
    assert callable(rh.rgsw.NoiseRGSWCiphertext) and callable(rh.Ring.CenteredMoments) and callable(rh.Ring.Log2OfStandardDeviation)


# ---- ckks.GetPrecisionStats (schemes/ckks/precision.go), host -------------------------------------------------------------------------------------------------
def test_precision_stats_match_the_private_copies_of_the_oracle_tests(rh):
    """AVGLog2Prec against the three private restatements of it, each with its own Log2Scale, on vectors with exact slots among them.  They
    average with numpy's pairwise sum, this function in the reference's sequential order: n eps max|v| = 4096 * 2^-52 * 64 < 1e-10 apart"""
    import test_bootstrapping_oracle as tbo
    import test_mod1_oracle as tmo
    import test_polynomial_oracle as tpo
    rnd = np.random.default_rng(11)
    for mod, n in ((tbo, 4096), (tmo, 512), (tpo, 8)):
        want = rnd.uniform(-1, 1, n) + 1j * rnd.uniform(-1, 1, n)
        have = want + (rnd.normal(0, 2.0 ** -30, n) + 1j * rnd.normal(0, 2.0 ** -20, n))
        have[::7] = want[::7]                                          # exact slots: Log2Scale stands in
        have[3] = want[3].real + 1j * have[3].imag
        p = rh.ckks.GetPrecisionStats(None, None, want, have, log2_scale=mod.LOGSCALE)
        re_, im_ = mod.avg_log2_prec(want, have)
        assert abs(p.AVGLog2Prec.Real - re_) < 1e-10 and abs(p.AVGLog2Prec.Imag - im_) < 1e-10
        assert p.AVGLog2Err.Real == mod.LOGSCALE - p.AVGLog2Prec.Real and p.MAXLog2Prec.Real == mod.LOGSCALE == p.Log2Scale


def test_precision_stats_by_hand(rh):
    want = np.array([0, 0, 0, 0], dtype=np.complex128)
    have = np.array([2.0 ** -10 + 2.0 ** -3 * 1j, -(2.0 ** -20), 2.0 ** -12 * 1j, 2.0 ** -14 + 2.0 ** -5 * 1j])
    p = rh.ckks.GetPrecisionStats(None, None, want, have, log2_scale=30, computeDCF=True)
    # real: 10, 20, 30 (exact), 14; imag: 3, 30 (exact), 12, 5; L2 = sqrt(2 errReal^2): real - 1/2, the exact one 30
    assert (p.MINLog2Prec.Real, p.MAXLog2Prec.Real, p.AVGLog2Prec.Real, p.MEDLog2Prec.Real) == (10, 30, 18.5, 17)
    assert (p.MINLog2Prec.Imag, p.MAXLog2Prec.Imag, p.AVGLog2Prec.Imag, p.MEDLog2Prec.Imag) == (3, 30, 12.5, 8.5)
    assert (p.MINLog2Prec.L2, p.MEDLog2Prec.L2) == (9.5, 16.5) and p.MAXLog2Prec.L2 == 30
    assert p.STDLog2Prec.Real == math.sqrt((8.5 ** 2 + 1.5 ** 2 + 11.5 ** 2 + 4.5 ** 2) / 3) == p.STDLog2Err.Real
    assert (p.MAXLog2Err.Real, p.MINLog2Err.Real, p.AVGLog2Err.Imag, p.MEDLog2Err.L2) == (20, 0, 17.5, 13.5)
    # the median: odd counts and two values take the upper middle (precision.go:370-377)
    pm = rh.precision
    assert pm.calcmedian([3.0, 1.0, 2.0]) == 2.0 and pm.calcmedian([1.0, 5.0]) == 5.0 and pm.calcmedian([4.0, 1.0, 3.0, 2.0]) == 2.5
    # the CDF: 500 bins from the least to the largest precision, the count of values below each
    assert p.cdfResol == 500 and len(p.RealDist) == 500 and p.RealDist[0] == (10.0, 0)
    assert p.RealDist[1] == (10.0 + 20 / 500, 1) and p.RealDist[100] == (14.0, 1) and p.RealDist[101][1] == 2 and p.RealDist[499][1] == 3
    assert pm.calcCDF([1.0, 1.0, 2.0], 4) == [(1.0, 0), (1.25, 2), (1.5, 2), (1.75, 2)]
    s = p.String().split("\n")
    assert s[1].startswith("┌─────────┬───────┬") and s[4] == "│MIN Prec │ 10.00 │  3.00 │  9.50 │" and s[15].startswith("└") and s[14] == "│STD Err  │ %5.2f │ %5.2f │ %5.2f │" % (
        p.STDLog2Err.Real, p.STDLog2Err.Imag, p.STDLog2Err.L2)
    with pytest.raises(rh.RingHipError, match="log2_scale"):
        rh.ckks.GetPrecisionStats(None, None, want, have)

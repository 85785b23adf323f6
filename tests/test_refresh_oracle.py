"""CPU: tests/refresh_restatement.py pinned to DECRYPTION in the reference's own set-ups, and its pieces pinned to hand-computed values.

CKKS (multiparty/mpckks/mpckks_test.go: 3 parties, flooding = Xe, testInsecurePrec45: logBound 173, minLevel 3, a level-4 ciphertext, shares
at level 3): the additive shares' sum (:224), the S2E ciphertext (:239) and the refreshed ciphertext (:467) each meet VerifyTestVectors'
rule, an average log2 precision of the real and of the imaginary parts of at least LogDefaultScale - (LogN + 2) = 33 bits
(schemes/ckks/precision.go:92-103), through the restated CKKS encoder, at full and at sparse slots.  Alongside, on scaled integer
plaintexts, a bound on the coefficients' error derived from the error laws: a refreshed ciphertext carries the input's error (Xe), the 3 + 3
errors of the two shares (each of variance Xe^2 + flooding^2, keyswitch_sk.go:78-84) and the truncation of Quo (below 1): a standard
deviation of at most sqrt(Xe^2 + 6 (Xe^2 + flooding^2)) + 1, with the one bit of slack tests/test_multiparty_oracle.py gives its key switches.

BGV (multiparty/mpbgv/mpbgv_test.go on mpbgv/test_parameters.go, T = 0x101 and 0xffc001): the shares sum modulo T to the plaintext exactly
(:206-220), S2E (:224-238) and Refresh (:241-298) decrypt and decode to exactly the input values (verifyTestVectors, :509-513), and the
masked transform with a slot permutation, Decode = Encode = True, to the permuted values (:300-386)."""
import json
import math
import os
import random

import numpy as np

import refresh_restatement as rf
import rlwe_restatement as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARTIES, FLOOD = 3, 3.2
SIGMA_SHARE = math.sqrt(rr.SIGMA ** 2 + FLOOD ** 2)
BOUND = math.log2(math.sqrt(rr.SIGMA ** 2 + 2 * PARTIES * SIGMA_SHARE ** 2) + 1) + 1


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "refresh_test_params.json")) as f:
        return json.load(f)["ckks"]


def share_error(rnd, N):
    out = []
    while len(out) < N:
        x = int(round(rnd.gauss(0.0, SIGMA_SHARE)))
        if abs(x) <= 6 * SIGMA_SHARE:
            out.append(x)
    return out


def test_minimum_level_for_refresh_on_hand_computed_cases(rh):
    Q = golden()["Q"]
    # 128 + 45 = 173 bits of mask, ceil(173 + log2 3) = 175 <= 55 + 3 * 45 = 190 bits at level 3 and not 145 at level 2
    # 5 parties at scale 2^30 + 1: ceil(log2) = 31, 159 bits, ceil(159 + 2.32) = 162 <= 190 again
    # 4 sixty-one-bit limbs hold 243.99.. bits < ceil(200 + 45 + 1) = 246: no such level
    cases = [((128, 2.0 ** 45, 3, Q), (3, 173, True)), ((128, 2.0 ** 30 + 1, 5, Q), (3, 159, True)),
             ((200, 2.0 ** 45, 2, [0x1fffffffffe00001] * 4), (0, 0, False))]
    for args, want in cases:
        assert rf.get_minimum_level_for_refresh(*args) == want
        assert rh.multiparty.GetMinimumLevelForRefresh(*args) == want


def test_conversion_pieces_on_hand_computed_values():
    assert [rf.quo(x, 3, 2) for x in (5, -5, 1, -1, 0)] == [7, -7, 1, -1, 0]           # toward zero: -15 / 2 = -7, where floor gives -8
    assert rf.input_scale_int(2.0 ** 45) == 1 << 45 and rf.input_scale_int(2.0 ** 45 + 0.5) == (1 << 45) + 1
    mods = [97, 193]
    Q = 97 * 193
    vals = [0, 1, -1, Q // 2 - 1, -(Q // 2), -(Q // 2) - 1]
    rows = rf.to_rns(vals + [0, 0], mods, 16)
    assert rows[0, 4] == 96 and rows[1, 4] == 192 and not rows[:, 1::2].any()         # Euclidean residues, zeros between
    # floor(Q / 2) itself is centred to the NEGATIVE side (the >= of ring.go:532): -(Q // 2) - 1 = Q // 2 mod Q comes back as it went in,
    # and Q // 2 - 1 is the largest positive value
    assert rf.from_rns(rows, mods, 8)[:6] == vals
    assert rf.from_rns(rf.to_rns([Q // 2] + [0] * 7, mods, 16), mods, 8)[0] == Q // 2 - Q


def test_masks_are_sign_extended_uniform_bits():
    for logBound in (1, 64, 65, 173):
        m = rf.masks(b"k", 3, 0, 1, 16, logBound)[0]
        assert all(-(1 << (logBound - 1)) <= v < 1 << (logBound - 1) for v in m)
        words = (logBound + 63) // 64
        for i, v in enumerate(m):
            raw = sum(rf.stream_word(b"k", 3, 0, w, i) << (64 * w) for w in range(words))
            assert (v - raw) % (1 << logBound) == 0


def test_restated_protocols_decrypt(oracle):
    g = golden()
    N, Q = 1 << g["LogN"], g["Q"]
    rnd = random.Random("refresh oracle")
    minLevel, logBound, ok = rf.get_minimum_level_for_refresh(128, 2.0 ** g["LogDefaultScale"], PARTIES, Q)
    assert (minLevel, logBound) == (3, 173)
    level, top, n = 4, len(Q) - 1, N
    sks = [rr.Secret.sample(rnd, N) for _ in range(PARTIES)]
    ideal = rr.Secret(N, [sum(c) for c in zip(*[s.coeffs for s in sks])])
    msg = [rnd.randrange(-(1 << 46), 1 << 46) for _ in range(N)]
    ct, _ = rr.encrypt(rnd, ideal, msg, Q, level)
    rows = [s.rows(Q) for s in sks]
    std = lambda got, want, M: rr.log2_std(rr.centered_diff(got, want, M))
    # ---- EncToShare: the additive shares sum to the plaintext
    masks = [rf.masks(b"party %d" % i, 0, 0, 1, n, logBound)[0] for i in range(PARTIES)]
    pub = [rf.e2s_gen_share(rows[i], Q, minLevel, ct[1], share_error(rnd, N), masks[i]) for i in range(PARTIES)]
    agg = pub[0]
    for p in pub[1:]:
        agg = rr._vec("ADD", agg, p, Q[:minLevel + 1])
    shares = [rf.e2s_get_share(masks[0], agg, ct[0], Q, minLevel, n)] + masks[1:]
    total = [sum(v) for v in zip(*shares)]
    got = std(total, msg, rr.prod(Q[:minLevel + 1]))
    print("MEASURED E2S shares' sum against the plaintext: log2 std %.2f [%.2f]" % (got, BOUND))
    assert got <= BOUND
    # ---- ShareToEnc at the top level decrypts
    crp = rr.uniform_poly(rnd, N, Q)
    c0 = [rf.s2e_gen_share(rows[i], Q, top, crp, share_error(rnd, N), shares[i]) for i in range(PARTIES)]
    acc = c0[0]
    for p in c0[1:]:
        acc = rr._vec("ADD", acc, p, Q)
    got = std(rr.phase([acc, crp], ideal, Q), msg, rr.prod(Q))
    print("MEASURED S2E ciphertext: log2 std %.2f [%.2f]" % (got, BOUND))
    assert got <= BOUND
    # ---- Refresh (the masked transform with transform = nil), scale in = scale out and a non-integer input scale
    for scale_in, factor in ((2.0 ** 45, 1.0), (2.0 ** 44 + 0.5, (1 << 45) / ((1 << 44) + 1))):
        sh = [rf.transform_gen_share(rows[i], rows[i], Q, minLevel, Q, top, ct[1], crp, (share_error(rnd, N), share_error(rnd, N)), masks[i],
                                     2.0 ** 45, scale_in) for i in range(PARTIES)]
        a, b = sh[0]
        for x, y in sh[1:]:
            a, b = rr._vec("ADD", a, x, Q[:minLevel + 1]), rr._vec("ADD", b, y, Q)
        new_c0 = rf.transform(ct[0], a, b, Q, minLevel, Q, top, N, n, 2.0 ** 45, scale_in)
        want = [rf.quo(v, 1 << 45, rf.input_scale_int(scale_in)) for v in msg]
        got = std(rr.phase([new_c0, crp], ideal, Q), want, rr.prod(Q))
        print("MEASURED refreshed ciphertext, scale ratio %.6f: log2 std %.2f [%.2f]" % (factor, got, BOUND + math.log2(factor)))
        assert got <= BOUND + math.log2(factor)


def test_sub_ring_shortcut_equals_the_transform_of_the_spread_poly(oracle):
    """NTTSparseAndMontgomery's NTT branch (core/rlwe/utils.go:222-233): an n-point transform with the first n roots of N's table -- the powers
    of psi^(N/n), the table of the ring of degree n under the same generator -- then every value replicated N / n times, against the full
    transform of the polynomial in Y = X^(N/n), which is what the device path runs"""
    g = golden()
    N, mods, n = 1 << g["LogN"], g["Q"][:4], 64
    rnd = random.Random("sparse")
    vals = [rnd.randrange(-(1 << 172), 1 << 172) for _ in range(n)]
    full = rr.ntt(rf.to_rns(vals, mods, N), N, mods)
    small = rr.ntt(rf.to_rns(vals, mods, n), n, mods)
    assert np.array_equal(full, np.repeat(small, N // n, axis=1))


# ---- the reference's own checks: VerifyTestVectors for CKKS, exact values for BGV ------------------------------------------------------------------
import pytest  # noqa: E402

import bgv_encoder_restatement as be  # noqa: E402
import ckks_encoder_restatement as cer  # noqa: E402
import lintrans_restatement as ltr  # noqa: E402


def _fold(shares, mods):
    acc = shares[0]
    for s in shares[1:]:
        acc = rr._vec("ADD", acc, s, mods)
    return acc


def _plain_rows(ct, sk, Q):
    """Decryptor.Decrypt: c0 + c1 s, NTT domain, at the ciphertext's level"""
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    return rr._vec("ADD", rr._vec("MUL_MONT", np.asarray(ct[1], dtype=np.uint64), sk.rows(mods), mods), np.asarray(ct[0], dtype=np.uint64), mods)


def _parties(rnd, N):
    sks = [rr.Secret.sample(rnd, N) for _ in range(PARTIES)]
    return sks, rr.Secret(N, [sum(c) for c in zip(*[s.coeffs for s in sks])])


def _encrypt_rows(rnd, sk, pt_rows, Q, level):
    """an encryption of zero plus an NTT-domain plaintext (addPtToCt)"""
    ct, _ = rr.encrypt(rnd, sk, [0] * sk.N, Q, level)
    return [rr._vec("ADD", ct[0], pt_rows, [int(q) for q in Q[:level + 1]]), ct[1]]


@pytest.mark.parametrize("log_slots", [9, 4], ids=["full", "sparse"])
def test_restated_ckks_protocols_meet_verify_test_vectors(oracle, log_slots):
    """mpckks_test.go's three checks on testInsecurePrec45, 3 parties, flooding = Xe, the ciphertext dropped to level 4 and the shares at
    minLevel = 3: the additive shares sum to a plaintext (testEncToShare, VerifyTestVectors at :224), the S2E ciphertext decrypts (:239) and
    the refreshed ciphertext decrypts (testRefresh -> testRefreshParameterized, :467).  VerifyTestVectors' rule (schemes/ckks/precision.go:92-103,
    as tests/test_dft_oracle.py states it): the average log2 precision of the real and of the imaginary parts is at least
    LogDefaultScale - (LogN + 2) = 33 bits."""
    g = golden()
    N, Q, log_scale = 1 << g["LogN"], g["Q"], g["LogDefaultScale"]
    bound = log_scale - (g["LogN"] + 2)
    assert bound == 33
    rnd = random.Random("refresh vectors %d" % log_slots)
    minLevel, logBound, _ = rf.get_minimum_level_for_refresh(128, 2.0 ** log_scale, PARTIES, Q)
    level, top, n, scale = 4, len(Q) - 1, 2 << log_slots, 2.0 ** log_scale
    sks, ideal = _parties(rnd, N)
    rows = [s.rows(Q) for s in sks]
    values = np.array([complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(1 << log_slots)])
    ct = _encrypt_rows(rnd, ideal, cer.embed(values, log_slots, scale, N, Q[:level + 1]), Q, level)

    def check(what, poly, mods, is_ntt):
        re, im = cer.decode(poly, log_slots, scale, N, mods, is_ntt=is_ntt)
        pr, pi = ltr.avg_log2_prec(values, re, im, log_scale)
        print("MEASURED %s, LogSlots %d: avg log2 precision real %.2f imag %.2f [>= %d]" % (what, log_slots, pr, pi, bound))
        assert pr >= bound and pi >= bound

    masks = [rf.masks(b"vector party %d" % i, 0, 0, 1, n, logBound)[0] for i in range(PARTIES)]
    lo = Q[:minLevel + 1]
    agg = _fold([rf.e2s_gen_share(rows[i], Q, minLevel, ct[1], share_error(rnd, N), masks[i]) for i in range(PARTIES)], lo)
    shares = [rf.e2s_get_share(masks[0], agg, ct[0], Q, minLevel, n)] + masks[1:]
    check("E2S shares' sum", rf.to_rns([sum(v) for v in zip(*shares)], lo, N), lo, False)
    crp = rr.uniform_poly(rnd, N, Q)
    c0 = _fold([rf.s2e_gen_share(rows[i], Q, top, crp, share_error(rnd, N), shares[i]) for i in range(PARTIES)], Q)
    check("S2E ciphertext", _plain_rows([c0, crp], ideal, Q), Q, True)
    sh = [rf.transform_gen_share(rows[i], rows[i], Q, minLevel, Q, top, ct[1], crp, (share_error(rnd, N), share_error(rnd, N)), masks[i], scale, scale)
          for i in range(PARTIES)]
    new_c0 = rf.transform(ct[0], _fold([s[0] for s in sh], lo), _fold([s[1] for s in sh], Q), Q, minLevel, Q, top, N, n, scale, scale)
    check("refreshed ciphertext", _plain_rows([new_c0, crp], ideal, Q), Q, True)


def bgv_golden():
    with open(os.path.join(ROOT, "tests", "golden", "refresh_test_params.json")) as f:
        return json.load(f)["bgv"]


@pytest.mark.parametrize("t", bgv_golden()["T"], ids=lambda t: "T=%#x" % t)
def test_restated_bgv_protocols_decrypt_exactly(oracle, t):
    """mpbgv_test.go on its own parameters (LogN 10, 5 + 1 moduli, T = 0x101: plaintext ring 128, gap 8; T = 0xffc001: 1024, gap 1), 3 parties,
    flooding = Xe: the additive shares sum modulo T to the plaintext, whose DecodeRingT is the input (testEncToShares, :206-220); the S2E
    ciphertext decrypts and decodes to exactly the input (:224-238 with verifyTestVectors, :509-513); so does the refreshed one (testRefresh,
    :241-298) and the masked transform with a slot permutation and Decode = Encode = True gives the permuted values
    (testRefreshAndPermutation, :300-386)."""
    g = bgv_golden()
    N, Q = 1 << g["LogN"], g["Q"]
    P = be.Params(N, Q, t)
    rnd = random.Random("bgv oracle %d" % t)
    level, top, scale = 1, len(Q) - 1, 1
    sks, ideal = _parties(rnd, N)
    rows = [s.rows(Q) for s in sks]
    values = np.array([rnd.randrange(t) for _ in range(P.n)], dtype=np.uint64)
    ct = _encrypt_rows(rnd, ideal, be.encode(P, level, values, scale), Q, level)
    lo = Q[:level + 1]
    masks = [np.array([rnd.randrange(t) for _ in range(P.n)], dtype=np.uint64) for _ in range(PARTIES)]
    agg = _fold([rf.bgv_e2s_gen_share(P, rows[i], level, ct[1], share_error(rnd, N), masks[i]) for i in range(PARTIES)], lo)
    shares = [rf.bgv_e2s_get_share(P, masks[0], agg, ct[0], level)] + masks[1:]
    rec = np.array([sum(int(s[j]) for s in shares) % t for j in range(P.n)], dtype=np.uint64)
    assert np.array_equal(be.decode_ring_t(P, rec, scale), values)
    crp = rr.uniform_poly(rnd, N, Q)
    c0 = _fold([rf.bgv_s2e_gen_share(P, rows[i], top, crp, share_error(rnd, N), shares[i]) for i in range(PARTIES)], Q)
    assert np.array_equal(be.decode(P, top, _plain_rows([c0, crp], ideal, Q), scale), values)
    perm = list(range(P.n))
    rnd.shuffle(perm)
    for tf, want in ((None, values), ((True, lambda v: [v[j] for j in perm], True), values[perm])):
        sh = [rf.bgv_transform_gen_share(P, rows[i], rows[i], level, top, ct[1], crp, (share_error(rnd, N), share_error(rnd, N)), masks[i], tf, scale)
              for i in range(PARTIES)]
        new_c0 = rf.bgv_transform(P, ct[0], _fold([s[0] for s in sh], lo), _fold([s[1] for s in sh], Q), level, top, tf, scale)
        assert np.array_equal(be.decode(P, top, _plain_rows([new_c0, crp], ideal, Q), scale), want)

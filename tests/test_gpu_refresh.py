"""GPU: the share conversion of the collective refresh (csrc/mp_refresh.hip) and the CKKS refresh protocols over it
(matrix-fhe-lattigo_amd/multiparty_refresh.py).

The kernels alone are compared as whole outputs with Python integers (tests/refresh_restatement.py) on TAIL (N = 32, 61-bit limbs) and on the
45 / 55-bit chain of tests/golden/refresh_test_params.json at N = 2^10.  With `samples=` every share, aggregate and output of the four CKKS
protocols is the restatement's bit for bit, with the one-kernel recode and with its three calls.  With a fixed KeyedPRNG per party and no host
key material 3 parties refresh a level-4 ciphertext to the top level and the result decrypts on the device."""
import json
import math
import os
import random

import numpy as np
import pytest

import multiparty_restatement as mr
import refresh_restatement as rf
import rlwe_restatement as rr
from conftest import PI60, QI60

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUSED = pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
_RINGS = {}
KEY = b"refresh test key"
RH_ERR_UNSUPPORTED = -5


def ring(rh, N, mods):
    k = (N, tuple(mods))
    if k not in _RINGS:
        _RINGS[k] = rh.Ring(N, list(mods))
    return _RINGS[k]


def tail(rh, limbs=7):
    """TAIL (N = 32): 7 limbs of Q; 8 or 9 limbs take the first of the P pool after them"""
    return ring(rh, 32, (QI60[:7] + PI60[:limbs - 7])[:limbs])


def golden():
    with open(os.path.join(ROOT, "tests", "golden", "refresh_test_params.json")) as f:
        return json.load(f)["ckks"]


def ref_ring(rh):
    g = golden()
    return ring(rh, 1 << g["LogN"], g["Q"])


def mods_of(r, level):
    return [int(q) for q in r.moduli[:level + 1]]


def block(rh, r, values, W=None):
    return rh.multiparty.AdditiveShareBigint.from_ints(r, values, W)


def poly_rows(rh, r, rows):
    return rh.DevicePoly.from_numpy(r.AtLevel(rows.shape[-2] - 1), rows)


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logBound", [1, 63, 64, 65, 127, 128, 173, 511])
def test_sampler_is_the_restated_stream_whole_and_in_sub_blocks(rh, logBound):
    mp = rh.multiparty
    r, n, call = tail(rh), 32, 5
    W = logBound // 64 + 1
    want = rf.masks(KEY, call, 0, 3, n, logBound)
    assert any(v < 0 for v in want[0]) and any(v >= 0 for v in want[0])
    for words in {W, min(W + 1, 8)}:                                        # the words above the sign bit are the sign's
        whole = mp.AdditiveShareBigint(r, n, words, 3)
        mp.big_sample(rh.rlwe.KeyedPRNG(KEY), whole, logBound, call=call)
        assert whole.to_ints() == want and whole.numpy().shape == (3, n, words)
        a, b = mp.AdditiveShareBigint(r, n, words, 2), mp.AdditiveShareBigint(r, n, words, 1)
        mp.big_sample(rh.rlwe.KeyedPRNG(KEY), a, logBound, call=call)
        mp.big_sample(rh.rlwe.KeyedPRNG(KEY), b, logBound, call=call, poly0=2)
        assert a.to_ints() + b.to_ints() == want


@pytest.mark.parametrize("n", [2, 4])
def test_one_and_two_slots_are_sampled_and_recoded(rh, n):
    """n = 2 slots = 2 or 4: fewer values than a sampler lane's group of eight; the stream rule and the conversions are the same"""
    mp = rh.multiparty
    r, call, logBound = tail(rh), 9, 100
    want = rf.masks(KEY, call, 0, 3, n, logBound)
    b = mp.AdditiveShareBigint(r, n, 2, 3)
    mp.big_sample(rh.rlwe.KeyedPRNG(KEY), b, logBound, call=call)
    assert b.to_ints() == want
    level, mods = 2, mods_of(r, 2)
    rl = r.AtLevel(level)
    out = rl.NewPoly(3)
    mp.big_to_rns(rl, b, out)
    assert np.array_equal(out.numpy(), np.stack([rf.to_rns(v, mods, r.N) for v in want]))
    back = mp.AdditiveShareBigint(r, n, 3, 3)
    mp.big_from_rns(rl, out, back)
    assert back.to_ints() == want
    m, d = (1 << 45) + 7, 1 << 44
    top = r.AtLevel(6)
    for fused in (True, False):
        dst = top.NewPoly(3)
        mp.refresh_recode(top, dst, m, d, n, src_poly=out, rl_in=rl, fused=fused)
        assert np.array_equal(dst.numpy(), np.stack([rf.recode(v, m, d, mods_of(r, 6), r.N) for v in want]))


def test_sampler_refuses_a_bound_its_words_cannot_hold(rh):
    mp = rh.multiparty
    with pytest.raises(rh.RingHipError, match="logBound 128 out of range"):
        mp.big_sample(rh.rlwe.KeyedPRNG(KEY), mp.AdditiveShareBigint(tail(rh), 8, 2), 128)


# ---- from-RNS ------------------------------------------------------------------------------------------------------------------------------------------
def planted(Q, count, rnd):
    v = [0, 1, Q - 1, Q // 2 - 1, Q // 2, Q // 2 + 1]
    return v + [rnd.randrange(Q) for _ in range(count - len(v))]


@pytest.mark.parametrize("gap", [1, 4])
@pytest.mark.parametrize("level", [0, 3, 6, 7])
def test_from_rns_centres_planted_values(rh, level, gap):
    mp = rh.multiparty
    r = tail(rh, 8 if level == 7 else 7)
    N, n = r.N, r.N // gap
    mods = mods_of(r, level)
    Q = math.prod(mods)
    rnd = random.Random("from-rns %d %d" % (level, gap))
    # two polys with every limb of the ring (rows above the level and coefficients off the stride are there to be skipped)
    vals = [planted(Q, n, rnd) for _ in range(2)]
    rows = np.array([[[rnd.randrange(int(q)) for _ in range(N)] for q in r.moduli] for _ in range(2)], dtype=np.uint64)
    for p in range(2):
        for k, q in enumerate(mods):
            rows[p, k, ::gap] = [v % q for v in vals[p]]
    want = [[v - Q if v >= Q // 2 else v for v in row] for row in vals]
    assert [rf.from_rns(rows[p, :level + 1], mods, n) for p in range(2)] == want
    W = (Q.bit_length() + 1 + 63) // 64
    out = mp.AdditiveShareBigint(r, n, W, 2)
    mp.big_from_rns(r.AtLevel(level), poly_rows(rh, r, rows), out)
    assert out.to_ints() == want
    if W < 8:                                                                  # the accumulating form of GetShare, in wider words
        have = [[rnd.randrange(-Q, Q) for _ in range(n)] for _ in range(2)]
        acc = block(rh, r, have, W + 1)
        mp.big_from_rns(r.AtLevel(level), poly_rows(rh, r, rows), acc, accumulate=True)
        assert acc.to_ints() == [[a + b for a, b in zip(x, y)] for x, y in zip(have, want)]


def test_from_rns_refuses_a_modulus_beyond_eight_words(rh):
    mp = rh.multiparty
    r = tail(rh, 9)                                                            # Q ~ 2^549
    out, src = mp.AdditiveShareBigint(r, 32, 8), r.NewPoly(1)
    rc = rh.lib().rh_mp_big_from_rns(r._h, 8, src.ptr, 9, out.ptr, 32, 8, 1, 0)
    assert rc == RH_ERR_UNSUPPORTED and b"rh_mp_big_from_rns" in rh.lib().rh_last_error()
    rc = rh.lib().rh_mp_big_from_rns(r._h, 3, src.ptr, 9, out.ptr, 32, 2, 1, 0)       # four 61-bit limbs do not fit two words
    assert rc == -1 and b"does not fit 2 words" in rh.lib().rh_last_error()


# ---- to-RNS --------------------------------------------------------------------------------------------------------------------------------------------
def signed_values(W, count, rnd):
    top = 64 * W - 1
    edge = [0, 1, -1, (1 << (top - 1)), -(1 << (top - 1)), (1 << 64) - 1 if W > 1 else 5, -(1 << 64) if W > 1 else -5]
    return edge + [rnd.randrange(-(1 << top) + 1, 1 << top) for _ in range(count - len(edge))]


@pytest.mark.parametrize("chain", ["TAIL", "REF"])
@pytest.mark.parametrize("gap", [1, 4])
@pytest.mark.parametrize("W", [1, 3, 8])
def test_to_rns_is_the_euclidean_residue_under_every_limb(rh, W, gap, chain):
    mp = rh.multiparty
    r = tail(rh) if chain == "TAIL" else ref_ring(rh)
    N, n, level = r.N, r.N // gap, r.L - 1
    mods = mods_of(r, level)
    rnd = random.Random("to-rns %d %d %s" % (W, gap, chain))
    vals = [signed_values(W, n, rnd) for _ in range(2)]
    want = np.stack([rf.to_rns(v, mods, N) for v in vals])
    b = block(rh, r, vals, W)
    assert b.W == W
    rl = r.AtLevel(level)
    base = np.array([[[rnd.randrange(q) for _ in range(N)] for q in mods] for _ in range(2)], dtype=np.uint64)
    for acc in (0, 1, -1):
        out = poly_rows(rh, r, base)
        mp.big_to_rns(rl, b, out, accumulate=acc)
        if acc == 0:
            exp = want
        else:
            exp = np.stack([rr._vec("ADD" if acc > 0 else "SUB", base[p], want[p], mods) for p in range(2)])
        assert np.array_equal(out.numpy(), exp), acc


# ---- muldiv --------------------------------------------------------------------------------------------------------------------------------------------
def divisors():
    q4 = golden()["Q"][4]
    return [1 << 45, -(-(1 << 90) // q4), (1 << 150) + 12345]


@pytest.mark.parametrize("d", divisors(), ids=["pow2", "q4", "3words"])
def test_muldiv_truncates_toward_zero(rh, d):
    mp = rh.multiparty
    r, m = tail(rh), 1 << 45
    rnd = random.Random("muldiv %d" % d)
    big = rnd.getrandbits(173) | (1 << 172)
    xs = [0, 1, -1, d - 1, -(d - 1), d, -d, big, -big, d + 1, -(d + 1), 3 * d - 1, -(3 * d - 1)]
    xs += [rnd.randrange(-(1 << 172), 1 << 172) for _ in range(32 - len(xs))]
    want = [rf.quo(x, m, d) for x in xs]
    assert m == d or any(w != (x * m) // d for w, x in zip(want, xs))          # a floor division gets the negatives wrong (m = d divides exactly)
    b = block(rh, r, [xs], 4)                                                  # 173 + 45 - 45 + 1 bits at the most: four words
    out = mp.AdditiveShareBigint(r, 32, 4)
    mp.big_muldiv(b, m, d, out)
    assert out.to_ints() == [want]
    mp.big_muldiv(b, m, d)                                                     # in place
    assert b.to_ints() == [want]


def test_muldiv_refuses_a_quotient_that_cannot_fit(rh):
    mp = rh.multiparty
    b = block(rh, tail(rh), [[1 << 120] * 8], 2)
    with pytest.raises(rh.RingHipError, match="does not fit 2 words"):
        mp.big_muldiv(b, 1 << 45, 3)


# ---- the fused recode ----------------------------------------------------------------------------------------------------------------------------------
@FUSED
@pytest.mark.parametrize("double", [False, True], ids=["same-N", "Nout=2N"])
def test_recode_is_the_three_calls_and_the_restatement(rh, fused, double):
    mp = rh.multiparty
    rin = tail(rh)
    rout = ring(rh, 64, QI60[:7]) if double else rin
    level_in, level_out, n = 2, 6, 8                                           # gap 4 in, 4 or 8 out
    mods_in, mods_out = mods_of(rin, level_in), mods_of(rout, level_out)
    Q = math.prod(mods_in)
    rnd = random.Random("recode")
    m, d = 1 << 45, (1 << 45) + 1
    vals = [planted(Q, n, rnd) for _ in range(2)]
    rows = np.stack([rf.to_rns(v, mods_of(rin, 6), rin.N) for v in vals])      # every limb of the ring; level 2 is read
    cent = [[v - Q if v >= Q // 2 else v for v in row] for row in vals]
    want = np.stack([rf.recode(c, m, d, mods_out, rout.N) for c in cent])
    rli, rlo = rin.AtLevel(level_in), rout.AtLevel(level_out)
    # variant (a): from a coefficient-domain poly
    out = rlo.NewPoly(2)
    mp.refresh_recode(rlo, out, m, d, n, src_poly=poly_rows(rh, rin, rows), rl_in=rli, fused=fused)
    assert np.array_equal(out.numpy(), want)
    # variant (b): from a block, accumulating on what is there
    mp.refresh_recode(rlo, out, m, d, n, src_share=block(rh, rin, cent, 4), accumulate=-1, fused=fused)
    assert np.array_equal(out.numpy(), np.zeros_like(want))


def test_recode_refuses_more_values_than_the_target_ring_has_coefficients(rh):
    mp = rh.multiparty
    big, small = ring(rh, 64, QI60[:7]), tail(rh)
    with pytest.raises(rh.RingHipError, match="n > N_out"):
        mp.refresh_recode(small.AtLevel(6), small.NewPoly(1), 1, 1, 64, src_poly=big.NewPoly(1), rl_in=big.AtLevel(2))
    src, dst = big.NewPoly(1), small.NewPoly(1)
    rc = rh.lib().rh_mp_refresh_recode(big._h, 2, src.ptr, 7, None, 64, 4, small._h, 6, dst.ptr, 1,
                                       np.array([1], dtype=np.uint64).ctypes.data_as(rh.ringhip.U64P), 1,
                                       np.array([1], dtype=np.uint64).ctypes.data_as(rh.ringhip.U64P), 1, 0)
    assert rc == -1 and b"n > N_out" in rh.lib().rh_last_error()


# ---- the protocols -------------------------------------------------------------------------------------------------------------------------------------
PARTIES = 3
FLOOD = 3.2                                                                    # flooding = Xe, as the reference's tests set it (mpckks_test.go)


def sample_error(rnd, npoly, N, sigma=4.5):
    return np.array([[max(-27, min(27, round(rnd.gauss(0, sigma)))) for _ in range(N)] for _ in range(npoly)], dtype=np.int32)


def setting(rh, name):
    """(ring, level of the shares, top level, logBound, log2 slots)"""
    if name == "REF":
        r = ref_ring(rh)
        minLevel, logBound, ok = rh.multiparty.GetMinimumLevelForRefresh(128, 2.0 ** 45, PARTIES, [int(q) for q in r.moduli])
        assert (minLevel, logBound, ok) == (3, 173, True)
        return r, minLevel, r.L - 1, logBound, 9
    return tail(rh), 2, 6, 100, 2                                              # slots = 4: gap 4


@FUSED
@pytest.mark.parametrize("name", ["TAIL", "REF"])
def test_protocols_from_samples_bit_for_bit(rh, name, fused):
    """E2S, S2E, the masked transform (transform = None) and Refresh on a batch of 2 ciphertexts one level above the shares"""
    mp = rh.multiparty
    r, level, top, logBound, logSlots = setting(rh, name)
    N, Q, n, npoly = r.N, [int(q) for q in r.moduli], 2 << logSlots, 2
    rnd = random.Random("protocols " + name)
    rl, rt = r.AtLevel(level), r.AtLevel(top)
    kg = rh.rlwe.KeyGenerator(r, None, prng=rh.rlwe.KeyedPRNG(b"refresh keys " + name.encode()))
    sks = [kg.GenSecretKeyNew() for _ in range(PARTIES)]
    sk_rows = [s.Value.Q.numpy()[0] for s in sks]
    scale = rh.ckks.Scale(2.0 ** 45 + 0.5) if name == "REF" else rh.ckks.Scale(1 << 20)        # a non-integer scale takes the ceiling
    scale_out = rh.ckks.Scale(1 << 45) if name == "REF" else rh.ckks.Scale((1 << 20) + 3)
    ct_rows = np.array([[[[rnd.randrange(q) for _ in range(N)] for q in Q[:level + 2]] for _ in range(npoly)] for _ in range(2)], dtype=np.uint64)
    ct = rh.Ciphertext([poly_rows(rh, r, ct_rows[0]), poly_rows(rh, r, ct_rows[1])], is_ntt=True)
    ct.Scale, ct.LogDimensions, ct.IsBatched = scale, logSlots, True
    crs = mp.CRS(b"refresh crs")
    masks = [[[rnd.randrange(-(1 << (logBound - 1)), 1 << (logBound - 1)) for _ in range(n)] for _ in range(npoly)] for _ in range(PARTIES)]
    errs = [(sample_error(rnd, npoly, N), sample_error(rnd, npoly, N)) for _ in range(PARTIES)]
    W = (logBound + 64) // 64
    # ---- EncToShare
    e2s = mp.mpckks.EncToShareProtocol(r, FLOOD)
    pub, sec = [e2s.AllocateShare(level, npoly) for _ in range(PARTIES)], [mp.AdditiveShareBigint(r, n, W, npoly) for _ in range(PARTIES)]
    want_pub = []
    for i in range(PARTIES):
        e2s.GenShare(sks[i], logBound, ct, sec[i], pub[i], samples={"e": errs[i][0], "mask": masks[i]}, fused=fused)
        want_pub.append(np.stack([rf.e2s_gen_share(sk_rows[i], Q, level, ct_rows[1][p], errs[i][0][p], masks[i][p]) for p in range(npoly)]))
        assert np.array_equal(pub[i].Value.numpy(), want_pub[i]) and sec[i].to_ints() == masks[i]
    agg = e2s.AllocateShare(level, npoly)
    e2s.AggregateShares(pub, agg, fused=fused)
    want_agg = mr.aggregate(want_pub, Q[:level + 1])
    assert np.array_equal(agg.Value.numpy(), want_agg)
    Wq = (math.prod(Q[:level + 1]).bit_length() + 1 + 64) // 64
    last = block(rh, r, masks[0], Wq)
    got = mp.AdditiveShareBigint(r, n, Wq, npoly)
    e2s.GetShare(last, agg, ct, got)
    want_last = [rf.e2s_get_share(masks[0][p], want_agg[p], ct_rows[0][p], Q, level, n) for p in range(npoly)]
    assert got.to_ints() == want_last
    # ---- ShareToEnc at the top level, of the additive shares E2S left
    s2e = mp.mpckks.ShareToEncProtocol(r, FLOOD)
    crp = s2e.SampleCRP(top, crs)
    crp_rows = crp.numpy()[0]
    shares_in = [want_last] + [masks[i] for i in range(1, PARTIES)]
    c0s, want_c0 = [s2e.AllocateShare(top, npoly) for _ in range(PARTIES)], []
    for i in range(PARTIES):
        s2e.GenShare(sks[i], crp, ct, block(rh, r, shares_in[i], Wq), c0s[i], samples={"e": errs[i][1]}, fused=fused)
        want_c0.append(np.stack([rf.s2e_gen_share(sk_rows[i], Q, top, crp_rows, errs[i][1][p], shares_in[i][p]) for p in range(npoly)]))
        assert np.array_equal(c0s[i].Value.numpy(), want_c0[i])
    s2e.AggregateShares(c0s, c0s[0], fused=fused)
    out = rh.Ciphertext([rt.NewPoly(npoly), rt.NewPoly(npoly)], is_ntt=True)
    s2e.GetEncryption(c0s[0], crp, out)
    assert np.array_equal(out.Value[0].numpy(), mr.aggregate(want_c0, Q)) and all(np.array_equal(out.Value[1].numpy()[p], crp_rows) for p in range(npoly))
    # ---- the masked transform with transform = None, and Refresh, which is the same calls
    for proto in (mp.mpckks.MaskedLinearTransformationProtocol(r, r, scale_out, FLOOD), mp.mpckks.RefreshProtocol(r, scale_out, FLOOD)):
        refresh = isinstance(proto, mp.mpckks.RefreshProtocol)
        shares, want = [proto.AllocateShare(level, top, npoly) for _ in range(PARTIES)], []
        for i in range(PARTIES):
            s = {"e": errs[i], "mask": masks[i]}
            if refresh:
                proto.GenShare(sks[i], logBound, ct, crp, shares[i], samples=s, fused=fused)
            else:
                proto.GenShare(sks[i], sks[i], logBound, ct, crp, None, shares[i], samples=s, fused=fused)
            want.append([np.stack(x) for x in zip(*[rf.transform_gen_share(sk_rows[i], sk_rows[i], Q, level, Q, top, ct_rows[1][p], crp_rows, (errs[i][0][p], errs[i][1][p]),
                                                                             masks[i][p], scale_out.Value, scale.Value) for p in range(npoly)])])
            assert np.array_equal(shares[i].EncToShareShare.Value.numpy(), want[i][0])
            assert np.array_equal(shares[i].ShareToEncShare.Value.numpy(), want[i][1])
        total = proto.AllocateShare(level, top, npoly)
        proto.AggregateShares(shares, total, fused=fused)
        wa, wb = mr.aggregate([w[0] for w in want], Q[:level + 1]), mr.aggregate([w[1] for w in want], Q)
        assert np.array_equal(total.EncToShareShare.Value.numpy(), wa) and np.array_equal(total.ShareToEncShare.Value.numpy(), wb)
        res = rh.Ciphertext([rt.NewPoly(npoly), rt.NewPoly(npoly)], is_ntt=True)
        if refresh:
            proto.Finalize(ct, crp, total, res, fused=fused)
        else:
            proto.Transform(ct, None, crp, total, res, fused=fused)
        want_c0 = np.stack([rf.transform(ct_rows[0][p], wa[p], wb[p], Q, level, Q, top, N, n, scale_out.Value, scale.Value) for p in range(npoly)])
        assert np.array_equal(res.Value[0].numpy(), want_c0) and np.array_equal(res.Value[1].numpy()[1], crp_rows)
        assert res.Scale == scale_out and res.LogDimensions == logSlots


def test_three_parties_refresh_on_the_device_and_the_result_decrypts(rh):
    """no samples, no host key material: a level-4 ciphertext of the golden chain, full slots, is refreshed to the top level by 3 parties with
    a KeyedPRNG each.  The refreshed ciphertext carries the input's error, the 3 + 3 errors of the two shares (law of keyswitch_sk.go:78-84:
    sigma^2 = Xe^2 + flooding^2 each) and the truncation of Quo, below 1: its coefficients' error has standard deviation at most
    sqrt(Xe^2 + 2 * 3 * (Xe^2 + flooding^2)) + 1, and one more bit is allowed, as tests/test_gpu_multiparty.py allows its key switches."""
    mp = rh.multiparty
    r, minLevel, top, logBound, _ = setting(rh, "REF")
    N, Q, level = r.N, [int(q) for q in r.moduli], 4
    prngs = [rh.rlwe.KeyedPRNG(b"refresh party %d" % i) for i in range(PARTIES)]
    kgs = [rh.rlwe.KeyGenerator(r, None, prng=prngs[i]) for i in range(PARTIES)]
    sks = [kgs[i].GenSecretKeyNew() for i in range(PARTIES)]
    ideal = rh.rlwe.SecretKey(None, r.NewPoly(1), None)
    mp.aggregate(r, [s.Value.Q for s in sks], ideal.Value.Q)
    rnd = random.Random("refresh message")
    scale = rh.ckks.Scale(1 << 45)
    msg = [[rnd.randrange(-(1 << 46), 1 << 46) for _ in range(N)] for _ in range(2)]           # a scaled plaintext: 2^45 times values below 2
    mods = Q[:level + 1]
    rl = r.AtLevel(level)
    pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rl, np.stack([rr.ntt(rr.rns(m, mods), N, mods) for m in msg])), is_ntt=True)
    ct = rh.rlwe.Encryptor(r, None, ideal, prng=prngs[0]).EncryptNew(pt)
    ct.Scale, ct.LogDimensions, ct.IsBatched = scale, 9, True
    crss = [mp.CRS(b"refresh crs") for _ in range(PARTIES)]
    rfp = [mp.mpckks.RefreshProtocol(r, scale, FLOOD, prng=prngs[i]) for i in range(PARTIES)]
    crps = [rfp[i].SampleCRP(top, crss[i]) for i in range(PARTIES)]
    shares = [rfp[i].AllocateShare(minLevel, top, 2) for i in range(PARTIES)]
    for i in range(PARTIES):
        rfp[i].GenShare(sks[i], logBound, ct, crps[i], shares[i])
    rfp[0].AggregateShares(shares, shares[0])
    out = rh.Ciphertext([r.NewPoly(2), r.NewPoly(2)], is_ntt=True)
    rfp[0].Finalize(ct, crps[0], shares[0], out)
    assert out.Level() == top and out.Scale == scale
    dec = rh.rlwe.Decryptor(r, ideal).DecryptNew(out)
    r.INTT(dec.Value, dec.Value)
    a = dec.Value.numpy()
    got = [rr.log2_std(rr.centered_diff(rr.crt_centered(a[k], Q), msg[k], rr.prod(Q))) for k in range(2)]
    bound = math.log2(math.sqrt(rr.SIGMA ** 2 + 2 * PARTIES * (rr.SIGMA ** 2 + FLOOD ** 2)) + 1) + 1
    print("MEASURED collective refresh, log2 std of the error per ciphertext %s [%.2f]" % (got, bound))
    assert max(got) <= bound


@pytest.mark.parametrize("log_slots", [9, 4, 0], ids=["full", "sparse", "one-slot"])
def test_three_parties_refresh_meets_the_reference_precision_in_the_slots(rh, log_slots):
    """the same set-up through the CKKS encoder, full and sparse slots (gap 16): encode, encrypt under the ideal secret at level 4, refresh to
    the top level, decrypt and decode on the device.  VerifyTestVectors' rule (schemes/ckks/precision.go:92-103, as tests/test_dft_oracle.py
    states it; mpckks_test.go verifies its refresh with it): the average log2 precision of the real and of the imaginary parts is at least
    LogDefaultScale - (LogN + 2) = 33 bits"""
    mp = rh.multiparty
    r, minLevel, top, logBound, _ = setting(rh, "REF")
    g = golden()
    level, log_scale = 4, g["LogDefaultScale"]
    prngs = [rh.rlwe.KeyedPRNG(b"refresh slots party %d" % i) for i in range(PARTIES)]
    sks = [rh.rlwe.KeyGenerator(r, None, prng=prngs[i]).GenSecretKeyNew() for i in range(PARTIES)]
    ideal = rh.rlwe.SecretKey(None, r.NewPoly(1), None)
    mp.aggregate(r, [s.Value.Q for s in sks], ideal.Value.Q)
    rnd = random.Random("refresh slots %d" % log_slots)
    values = np.array([[complex(rnd.uniform(-1, 1), rnd.uniform(-1, 1)) for _ in range(1 << log_slots)]])
    enc = rh.ckks.Encoder(r)
    scale = rh.ckks.Scale(1 << log_scale)
    pt = enc.NewPlaintext(level, scale, 1, log_slots)
    enc.Encode(values, pt)
    ct = rh.ckks.Encryptor(r, None, ideal, prng=prngs[0]).EncryptNew(pt)
    rfp = [mp.mpckks.RefreshProtocol(r, scale, FLOOD, prng=prngs[i]) for i in range(PARTIES)]
    crps = [rfp[i].SampleCRP(top, mp.CRS(b"refresh slots crs")) for i in range(PARTIES)]
    shares = [rfp[i].AllocateShare(minLevel, top) for i in range(PARTIES)]
    for i in range(PARTIES):
        rfp[i].GenShare(sks[i], logBound, ct, crps[i], shares[i])
    rfp[0].AggregateShares(shares, shares[0])
    out = rh.Ciphertext([r.NewPoly(1), r.NewPoly(1)], is_ntt=True)
    rfp[0].Finalize(ct, crps[0], shares[0], out)
    assert out.Level() == top and out.LogDimensions == log_slots and out.Scale == scale
    have = enc.Decode(rh.ckks.Decryptor(r, ideal).DecryptNew(out))
    prec = []
    for part in (np.real, np.imag):
        err = np.abs(part(np.asarray(have)[0][:1 << log_slots]) - part(values[0]))
        prec.append(float(np.mean([log_scale if e == 0 else -math.log2(e) for e in err])))
    bound = log_scale - (g["LogN"] + 2)
    print("MEASURED collective refresh, LogSlots %d: avg log2 precision real %.2f imag %.2f [>= %d]" % (log_slots, prec[0], prec[1], bound))
    assert min(prec) >= bound


# ---- refusals, each by name ------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name(rh):
    mp = rh.multiparty
    r, level, top, logBound, logSlots = setting(rh, "TAIL")
    kg = rh.rlwe.KeyGenerator(r, None, prng=rh.rlwe.KeyedPRNG(b"refusals"))
    sk = kg.GenSecretKeyNew()
    rl = r.AtLevel(level)
    ct = rh.Ciphertext([rl.NewPoly(1), rl.NewPoly(1)], is_ntt=True)
    ct.Scale, ct.LogDimensions, ct.IsBatched = rh.ckks.Scale(1 << 20), logSlots, True
    proto = mp.mpckks.MaskedLinearTransformationProtocol(r, r, rh.ckks.Scale(1 << 20), FLOOD)
    crp = proto.SampleCRP(top, mp.CRS(b"x"))
    share = proto.AllocateShare(level, top)
    with pytest.raises(rh.RingHipError, match="MaskedLinearTransformationFunc is not supported"):
        proto.GenShare(sk, sk, logBound, ct, crp, lambda v: v, share)
    with pytest.raises(rh.RingHipError, match="MaskedLinearTransformationFunc is not supported"):
        proto.Transform(ct, lambda v: v, crp, share, ct)
    with pytest.raises(rh.RingHipError, match="ciphertext level is not large enough for refresh correctness"):
        proto.GenShare(sk, sk, 61 * 3 + 1, ct, crp, None, share)
    coeff = rh.Ciphertext(ct.Value, is_ntt=False)
    coeff.Scale, coeff.LogDimensions = ct.Scale, logSlots
    with pytest.raises(rh.RingHipError, match="non-NTT sparse branch"):
        proto.GenShare(sk, sk, logBound, coeff, crp, None, share)
    full = rh.Ciphertext(ct.Value, is_ntt=False)                                   # gap 1: refused too, for the unconditional INTT of GetShare
    full.Scale, full.LogDimensions = ct.Scale, 4
    with pytest.raises(rh.RingHipError, match="GetShare applies INTT whatever the domain"):
        proto.GenShare(sk, sk, logBound, full, crp, None, share)
    with pytest.raises(rh.RingHipError, match="crs level must be equal to ShareToEncShare"):
        proto.GenShare(sk, sk, logBound, ct, proto.SampleCRP(top - 1, mp.CRS(b"x")), None, share)
    with pytest.raises(rh.RingHipError, match="ct\\[1\\] level must be at least equal to EncToShareShare level"):
        proto.GenShare(sk, sk, logBound, ct, crp, None, proto.AllocateShare(level + 1, top))
    low = rh.Ciphertext([r.AtLevel(1).NewPoly(1), r.AtLevel(1).NewPoly(1)], is_ntt=True)
    low.Scale, low.LogDimensions, low.IsBatched = ct.Scale, logSlots, True
    share.MetaData = {"Scale": ct.Scale, "LogDimensions": logSlots, "IsBatched": True, "IsNTT": True}
    with pytest.raises(rh.RingHipError, match="input ciphertext level must be at least equal to e2s level"):
        proto.Transform(low, None, crp, share, ct)
    small = ring(rh, 16, QI60[:7])
    wide = rh.Ciphertext(ct.Value, is_ntt=True)
    wide.Scale, wide.LogDimensions, wide.IsBatched = ct.Scale, 4, True              # 32 values per ciphertext, a target ring of 16 coefficients
    with pytest.raises(rh.RingHipError, match="n > N_out"):
        mp.mpckks.MaskedLinearTransformationProtocol(r, small, rh.ckks.Scale(1 << 20), FLOOD).GenShare(sk, sk, logBound, wide, crp, None, share)
    ci = rh.Ring(32, QI60[:2], kind=rh.ConjugateInvariant)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        mp.mpckks.RefreshProtocol(ci, rh.ckks.Scale(1 << 20), FLOOD)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        mp.AdditiveShareBigint(ci, 8, 1)
    ci.close()
    from oracle import primes
    n3 = 3 << 6
    r3 = rh.Ring(n3, primes.gen_moduli_3n(n3, [60, 60], [])[0], kind=rh.Matrix3N)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        mp.mpckks.RefreshProtocol(r3, rh.ckks.Scale(1 << 20), FLOOD)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        mp.AdditiveShareBigint(r3, 8, 1)
    blk = mp.AdditiveShareBigint(r, 8, 1)
    assert rh.lib().rh_mp_big_to_rns(r3._h, 1, blk.ptr, 8, 1, r3.NewPoly(1).ptr, 1, 0) == RH_ERR_UNSUPPORTED and b"standard rings only" in rh.lib().rh_last_error()
    r3.close()
    with pytest.raises(rh.RingHipError, match="a power of two, at least 2"):
        mp.AdditiveShareBigint(r, 1, 1)
    with pytest.raises(rh.RingHipError, match="a power of two, at least 2"):
        mp.AdditiveShareBigint(r, 6, 1)


# ---- mpbgv ---------------------------------------------------------------------------------------------------------------------------------------------
import bgv_encoder_restatement as be  # noqa: E402


def bgv_golden():
    with open(os.path.join(ROOT, "tests", "golden", "refresh_test_params.json")) as f:
        return json.load(f)["bgv"]


_ENC = {}


def bgv_setting(rh, t):
    """(ringQ, encoder, restated params) of the reference's BGV test chain; T = 0x101 gives a plaintext ring of 128 (gap 8), 0xffc001 of 1024"""
    g = bgv_golden()
    r = ring(rh, 1 << g["LogN"], g["Q"])
    if t not in _ENC:
        _ENC[t] = rh.bgv.Encoder(r, t)
    return r, _ENC[t], be.Params(r.N, g["Q"], t)


def permute_block(perm):
    def func(dv):
        dv.upload(np.ascontiguousarray(dv.numpy()[:, perm]))
    return func


@FUSED
@pytest.mark.parametrize("t", bgv_golden()["T"], ids=lambda t: "T=%#x" % t)
def test_bgv_protocols_from_samples_bit_for_bit(rh, t, fused):
    """E2S, S2E, the masked transform (a slot permutation, Decode = Encode = True, and no transform) and Refresh on a batch of 2 ciphertexts"""
    mp = rh.multiparty
    r, enc, P = bgv_setting(rh, t)
    N, Q, n, npoly, level, top = r.N, P.Q, P.n, 2, 1, r.L - 1
    rnd = random.Random("bgv protocols %d" % t)
    rl, rt = r.AtLevel(level), r.AtLevel(top)
    kg = rh.rlwe.KeyGenerator(r, None, prng=rh.rlwe.KeyedPRNG(b"bgv refresh keys"))
    sks = [kg.GenSecretKeyNew() for _ in range(PARTIES)]
    sk_rows = [s.Value.Q.numpy()[0] for s in sks]
    ct_rows = np.array([[[[rnd.randrange(q) for _ in range(N)] for q in Q[:level + 2]] for _ in range(npoly)] for _ in range(2)], dtype=np.uint64)
    ct = rh.Ciphertext([poly_rows(rh, r, ct_rows[0]), poly_rows(rh, r, ct_rows[1])], is_ntt=True)
    ct.Scale, ct.IsBatched = 3, True
    masks = [np.array([[rnd.randrange(t) for _ in range(n)] for _ in range(npoly)], dtype=np.uint64) for _ in range(PARTIES)]
    errs = [(sample_error(rnd, npoly, N), sample_error(rnd, npoly, N)) for _ in range(PARTIES)]
    ringT = enc.RingT()
    # ---- EncToShare
    e2s = mp.mpbgv.EncToShareProtocol(enc, FLOOD)
    pub, sec, want_pub = [e2s.AllocateShare(level, npoly) for _ in range(PARTIES)], [mp.NewAdditiveShare(ringT, npoly) for _ in range(PARTIES)], []
    for i in range(PARTIES):
        e2s.GenShare(sks[i], ct, sec[i], pub[i], samples={"e": errs[i][0], "mask": masks[i]}, fused=fused)
        want_pub.append(np.stack([rf.bgv_e2s_gen_share(P, sk_rows[i], level, ct_rows[1][p], errs[i][0][p], masks[i][p]) for p in range(npoly)]))
        assert np.array_equal(pub[i].Value.numpy(), want_pub[i]) and np.array_equal(sec[i].Value.numpy()[:, 0], masks[i])
    agg = e2s.AllocateShare(level, npoly)
    e2s.AggregateShares(pub, agg, fused=fused)
    want_agg = mr.aggregate(want_pub, Q[:level + 1])
    assert np.array_equal(agg.Value.numpy(), want_agg)
    got = mp.NewAdditiveShare(ringT, npoly)
    e2s.GetShare(sec[0], agg, ct, got)
    want_last = np.stack([rf.bgv_e2s_get_share(P, masks[0][p], want_agg[p], ct_rows[0][p], level) for p in range(npoly)])
    assert np.array_equal(got.Value.numpy()[:, 0], want_last)
    # ---- ShareToEnc at the top level
    s2e = mp.mpbgv.ShareToEncProtocol(enc, FLOOD)
    crp = s2e.SampleCRP(top, mp.CRS(b"bgv refresh crs"))
    crp_rows = crp.numpy()[0]
    c0 = s2e.AllocateShare(top, npoly)
    s2e.GenShare(sks[0], crp, got, c0, samples={"e": errs[0][1]}, fused=fused)
    assert np.array_equal(c0.Value.numpy(), np.stack([rf.bgv_s2e_gen_share(P, sk_rows[0], top, crp_rows, errs[0][1][p], want_last[p]) for p in range(npoly)]))
    # ---- the masked transform with a slot permutation and without a transform, and Refresh
    perm = list(range(n))
    rnd.shuffle(perm)
    dev_tf = mp.MaskedTransformFunc(True, permute_block(perm), True)
    host_tf = (True, lambda v: [v[j] for j in perm], True)
    raw = lambda v: [v[j] for j in perm]
    protos = [(mp.mpbgv.MaskedTransformProtocol(enc, enc, FLOOD), dev_tf, host_tf), (mp.mpbgv.MaskedTransformProtocol(enc, enc, FLOOD), None, None),
              (mp.mpbgv.MaskedTransformProtocol(enc, enc, FLOOD), mp.MaskedTransformFunc(False, permute_block(perm), False), (False, raw, False)),
              (mp.mpbgv.MaskedTransformProtocol(enc, enc, FLOOD), mp.MaskedTransformFunc(True, permute_block(perm), False), (True, raw, False)),
              (mp.mpbgv.MaskedTransformProtocol(enc, enc, FLOOD), mp.MaskedTransformFunc(False, permute_block(perm), True), (False, raw, True)),
              (mp.mpbgv.RefreshProtocol(enc, FLOOD), None, None)]
    for proto, tf, htf in protos:
        refresh = isinstance(proto, mp.mpbgv.RefreshProtocol)
        shares, want = [proto.AllocateShare(level, top, npoly) for _ in range(PARTIES)], []
        for i in range(PARTIES):
            s = {"e": errs[i], "mask": masks[i]}
            if refresh:
                proto.GenShare(sks[i], ct, crp, shares[i], samples=s, fused=fused)
            else:
                proto.GenShare(sks[i], sks[i], ct, crp, tf, shares[i], samples=s, fused=fused)
            want.append([np.stack(x) for x in zip(*[rf.bgv_transform_gen_share(P, sk_rows[i], sk_rows[i], level, top, ct_rows[1][p], crp_rows,
                                                                                 (errs[i][0][p], errs[i][1][p]), masks[i][p], htf, 3) for p in range(npoly)])])
            assert np.array_equal(shares[i].EncToShareShare.Value.numpy(), want[i][0])
            assert np.array_equal(shares[i].ShareToEncShare.Value.numpy(), want[i][1])
        total = proto.AllocateShare(level, top, npoly)
        proto.AggregateShares(shares, total, fused=fused)
        wa, wb = mr.aggregate([w[0] for w in want], Q[:level + 1]), mr.aggregate([w[1] for w in want], Q)
        res = rh.Ciphertext([rt.NewPoly(npoly), rt.NewPoly(npoly)], is_ntt=True)
        res.Scale = 5                                                              # Transform decodes and encodes at the OUTPUT's scale
        if refresh:
            proto.Finalize(ct, crp, total, res, fused=fused)
        else:
            proto.Transform(ct, tf, crp, total, res, fused=fused)
        want_c0 = np.stack([rf.bgv_transform(P, ct_rows[0][p], wa[p], wb[p], level, top, htf, 5) for p in range(npoly)])
        assert np.array_equal(res.Value[0].numpy(), want_c0) and np.array_equal(res.Value[1].numpy()[1], crp_rows)


@pytest.mark.parametrize("t", bgv_golden()["T"], ids=lambda t: "T=%#x" % t)
def test_bgv_three_parties_refresh_and_permute_on_the_device_exactly(rh, t):
    """no samples, no host key material: 3 parties refresh a level-1 BGV ciphertext to the top level, and apply a slot permutation through the
    masked transform; both decrypt and decode to exactly the expected values (mpbgv_test.go: testRefresh, testRefreshAndPermutation)"""
    mp = rh.multiparty
    r, enc, P = bgv_setting(rh, t)
    n, level, top = P.n, 1, r.L - 1
    prngs = [rh.rlwe.KeyedPRNG(b"bgv party %d" % i) for i in range(PARTIES)]
    sks = [rh.rlwe.KeyGenerator(r, None, prng=prngs[i]).GenSecretKeyNew() for i in range(PARTIES)]
    ideal = rh.rlwe.SecretKey(None, r.NewPoly(1), None)
    mp.aggregate(r, [s.Value.Q for s in sks], ideal.Value.Q)
    rnd = random.Random("bgv values %d" % t)
    values = np.array([[rnd.randrange(t) for _ in range(n)]], dtype=np.uint64)
    pt = enc.NewPlaintext(level, scale=1, nvec=1)
    enc.Encode(values, pt)
    ct = rh.bgv.Encryptor(r, None, ideal, prng=prngs[0]).EncryptNew(pt)
    ct.Scale, ct.IsBatched = 1, True
    perm = list(range(n))
    rnd.shuffle(perm)
    for tf, want in ((None, values), (mp.MaskedTransformFunc(True, permute_block(perm), True), values[:, perm])):
        protos = [mp.mpbgv.MaskedTransformProtocol(enc, enc, FLOOD, prng=prngs[i]) for i in range(PARTIES)]
        crss = [mp.CRS(b"bgv crs") for _ in range(PARTIES)]
        crps = [protos[i].SampleCRP(top, crss[i]) for i in range(PARTIES)]
        shares = [protos[i].AllocateShare(level, top) for i in range(PARTIES)]
        for i in range(PARTIES):
            protos[i].GenShare(sks[i], sks[i], ct, crps[i], tf, shares[i])
        protos[0].AggregateShares(shares, shares[0])
        out = rh.Ciphertext([r.NewPoly(1), r.NewPoly(1)], is_ntt=True)
        out.Scale, out.IsBatched = 1, True
        protos[0].Transform(ct, tf, crps[0], shares[0], out)
        assert out.Level() == top
        got = enc.Decode(rh.bgv.Decryptor(r, ideal).DecryptNew(out))
        assert np.array_equal(got, want)

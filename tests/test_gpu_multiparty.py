"""GPU: the multiparty protocols on the device (matrix-fhe-lattigo_amd/multiparty.py over csrc/multiparty.hip).

With `samples=` every protocol entry is compared bit for bit, as whole arrays, with tests/multiparty_restatement.py through the set-ups of
tests/test_multiparty_oracle.py, for 3 parties on the cases of tests/test_keygen_oracle.py (TAIL N = 32 with 7 + 4 and 6 + 4 limbs, REF N = 2^10
with its four settings, Q61N13 N = 2^13), with the kernels (fused) and with the composed ring calls.  rh_mp_aggregate is also run alone against the
pairwise Ring.Add and Python integers.  With a fixed KeyedPRNG and no host key material five parties make collective keys that the existing
rlwe.Evaluator uses, and collective key switches that decrypt on the device within the reference's bounds."""
import ctypes
import math

import numpy as np
import pytest

import keygen_restatement as kr
import multiparty_restatement as mr
import rlwe_restatement as rr
import test_keygen_oracle as tko
import test_multiparty_oracle as tmo
import test_rlwe_oracle as tro

pytestmark = pytest.mark.gpu
_RINGS = {}
PARTIES = 3
FUSED = pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])


def rings(rh, name, pc):
    """(ringQ, ringP or None) of a chain with its first pc moduli of P, made once per session"""
    if (name, pc) not in _RINGS:
        N, Q, P, _ = tro.chain(name)
        _RINGS[name, pc] = (rh.Ring(N, list(Q)), rh.Ring(N, list(P[:pc])) if pc else None)
    return _RINGS[name, pc]


def qp(pair):
    """(Q block, P block or None) as numpy -> (polys, limbs of Q then P, N)"""
    q, p = pair
    return q if p is None else np.concatenate([q, p], axis=1)


def arr(x):
    """a gadget share or CRP of the device as the restatement's (rows, limbs, N); a round-one share as (rows, 2, limbs, N)"""
    a = qp(x.numpy())
    return a.reshape(-1, 2, a.shape[1], a.shape[2]) if getattr(x, "degree", 0) == 1 else a


def same_key(key, want):
    q = key.Q.numpy().reshape(key.digits, 2, key.Q.limbs, -1)
    p = key.P.numpy().reshape(key.digits, 2, key.P.limbs, -1) if key.P is not None else None
    return np.array_equal(q, want.Q) and (p is None) == (want.P is None) and (p is None or np.array_equal(p, want.P))


def secret(kg, name, i):
    return kg.GenSecretKeyNew(samples=tmo.party(name, i).coeffs)


def both_ways(proto, shares, alloc, fused):
    """the aggregate by the list form and by the reference's pairwise form (in place in its first operand)"""
    out = alloc()
    proto.AggregateShares(shares, out, fused=fused)
    for s in shares[1:]:
        proto.AggregateShares(shares[0], s, shares[0], fused=fused)
    return out, shares[0]


@FUSED
@pytest.mark.parametrize("case", tko.CASES, ids=tko._ids)
def test_key_protocols_from_samples_bit_for_bit(rh, case, fused):
    name, (pw2, pc), _ = case
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    mp = rh.multiparty
    rq, rp = rings(rh, name, pc)
    galEls = tuple(tko.galois_elements(N))
    want = tmo.protocol(case, PARTIES, galEls)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    ids = range(PARTIES)
    sk, sk_out = [secret(kg, name, i) for i in ids], [secret(kg, name, 100 + i) for i in ids]
    kw = dict(levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=pw2)
    crs, crs2 = mp.CRS(tmo.CRS_KEY), mp.CRS(tmo.CRS_KEY)
    # ---- the collective public key
    ckg = mp.PublicKeyGenProtocol(rq, rp)
    crp = ckg.SampleCRP(crs)
    assert np.array_equal(qp(crp.numpy()), want["cpk"]["crp"]) and np.array_equal(qp(ckg.SampleCRP(crs2).numpy()), want["cpk"]["crp"])
    shares = [ckg.AllocateShare() for _ in ids]
    for i in ids:
        ckg.GenShare(sk[i], crp, shares[i], samples={"e": want["cpk"]["e"][i]}, fused=fused)
        assert np.array_equal(qp(shares[i].numpy()), want["cpk"]["shares"][i])
    agg, agg2 = both_ways(ckg, shares, ckg.AllocateShare, fused)
    assert np.array_equal(qp(agg.numpy()), want["cpk"]["agg"]) and np.array_equal(qp(agg2.numpy()), want["cpk"]["agg"])
    pk = ckg.GenPublicKey(agg, crp)
    wk = want["cpk"]["key"]
    assert np.array_equal(pk.Q.numpy().reshape(wk.Q.shape), wk.Q) and (rp is None or np.array_equal(pk.P.numpy().reshape(wk.P.shape), wk.P))
    # ---- the evaluation key sk -> sk_out
    ekg = mp.EvaluationKeyGenProtocol(rq, rp)
    crp = ekg.SampleCRP(crs, **kw)
    assert np.array_equal(arr(crp), want["evk"]["crp"]) and np.array_equal(arr(ekg.SampleCRP(crs2, **kw)), want["evk"]["crp"])
    shares = [ekg.AllocateShare(**kw) for _ in ids]
    for i in ids:
        ekg.GenShare(sk[i], sk_out[i], crp, shares[i], samples={"e": want["evk"]["e"][i]}, fused=fused)
        assert np.array_equal(arr(shares[i]), want["evk"]["shares"][i])
    agg, agg2 = both_ways(ekg, shares, lambda: ekg.AllocateShare(**kw), fused)
    assert np.array_equal(arr(agg), want["evk"]["agg"]) and np.array_equal(arr(agg2), want["evk"]["agg"])
    assert same_key(ekg.GenEvaluationKey(agg, crp), want["evk"]["key"])
    # ---- the relinearisation key, two rounds
    rkg = mp.RelinearizationKeyGenProtocol(rq, rp)
    w = want["rlk"]
    crp = rkg.SampleCRP(crs, **kw)
    assert np.array_equal(arr(crp), w["crp"])
    alloc = [rkg.AllocateShare(**kw) for _ in ids]
    for i in ids:
        eph, r1, _ = alloc[i]
        rkg.GenShareRoundOne(sk[i], crp, eph, r1, samples={"u": w["u"][i], "e0": w["e0"][i], "e1": w["e1"][i]}, fused=fused)
        assert np.array_equal(arr(r1), w["r1"][i])
        assert np.array_equal(qp((eph.Value.Q.numpy(), eph.Value.P.numpy() if rp is not None else None))[0], kr.secret(w["u"][i]).rows(Q + P))
    r1_agg, _ = both_ways(rkg, [a[1] for a in alloc], lambda: rkg.AllocateShare(**kw)[1], fused)
    assert np.array_equal(arr(r1_agg), w["r1_agg"])
    for i in ids:
        eph, _, r2 = alloc[i]
        rkg.GenShareRoundTwo(eph, sk[i], r1_agg, r2, samples={"e": w["e2"][i]}, fused=fused)
        assert np.array_equal(arr(r2), w["r2"][i])
    r2_agg, _ = both_ways(rkg, [a[2] for a in alloc], lambda: rkg.AllocateShare(**kw)[2], fused)
    assert np.array_equal(arr(r2_agg), w["r2_agg"])
    assert same_key(rkg.GenRelinearizationKey(r1_agg, r2_agg), w["key"])
    # ---- three Galois keys in one GenSharesNew per party
    gkg = mp.GaloisKeyGenProtocol(rq, rp)
    w = want["gal"]
    crps = gkg.SampleCRPs(crs, len(galEls), **kw)
    for c, wc in zip(crps, w["crps"]):
        assert np.array_equal(arr(c), wc)
    per_party = [gkg.GenSharesNew(sk[i], galEls, crps, samples={"e": w["e"][i]}, fused=fused) for i in ids]
    for i in ids:
        assert [s.GaloisElement for s in per_party[i]] == list(galEls)
        for k in range(len(galEls)):
            assert np.array_equal(arr(per_party[i][k]), w["shares"][i][k])
    aggs = gkg.AllocateShares(len(galEls), **kw)
    for k in range(len(galEls)):
        gkg.AggregateShares([per_party[i][k] for i in ids], aggs[k], fused=fused)
        assert np.array_equal(arr(aggs[k]), w["aggs"][k])
    keys = gkg.GenGaloisKeysNew(aggs, crps)
    assert [k.GaloisElement for k in keys] == list(galEls) and all(same_key(k, wk) for k, wk in zip(keys, w["keys"]))
    # one element through the reference's own entry, with a CRP that is a block of its own
    one = gkg.AllocateShare(**kw)
    crp1 = gkg.SampleCRP(mp.CRS(b"unused"), **kw)
    rq.AtLevel(levelQ).CopyLvl(crps[1].Q, crp1.Q)
    if rp is not None:
        rp.AtLevel(levelP).CopyLvl(crps[1].P, crp1.P)
    rows = want["rows"]
    gkg.GenShare(sk[0], galEls[1], crp1, one, samples={"e": w["e"][0][rows:2 * rows]}, fused=fused)
    assert one.GaloisElement == galEls[1] and np.array_equal(arr(one), w["shares"][0][1])
    assert same_key(gkg.GenGaloisKey(aggs[1], crp1), w["keys"][1])


def batch(xs):
    return np.stack(xs)


@FUSED
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coeff"])
@pytest.mark.parametrize("shape", tko.ENC, ids=lambda s: "%s-p%d" % s)
def test_switching_protocols_on_a_batch_bit_for_bit(rh, shape, is_ntt, fused):
    name, pc = shape
    N, Q, P, levels = tro.chain(name)
    Q = [int(q) for q in Q]
    mp = rh.multiparty
    rq, rp = rings(rh, name, pc)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    ids = range(PARTIES)
    sk, sk_out = [secret(kg, name, i) for i in ids], [secret(kg, name, 100 + i) for i in ids]
    cks = mp.KeySwitchProtocol(rq, tmo.FLOOD)
    pcks = mp.PublicKeySwitchProtocol(rq, rp, tmo.FLOOD)
    top = levels[0]
    for level, share_level in ((top, top), (top - 1, top - 1), (top, top - 1), (top - 1, top)):
        want = tmo.switching(name, pc, PARTIES, level, is_ntt, 3)
        rl = rq.AtLevel(level)
        ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, batch([c[k] for c in want["ct"]])) for k in (0, 1)], is_ntt=is_ntt)
        low = min(level, share_level)
        wl = want if low == level else None                                 # a share below the ciphertext: its own restatement, at the share's level
        # ---- KeySwitchProtocol
        shares = [cks.AllocateShare(share_level, 3) for _ in ids]
        for i in ids:
            cks.GenShare(sk[i], sk_out[i], ct, shares[i], samples={"e": want["ks"]["e"][i]}, fused=fused)
            assert shares[i].Level() == low
            w = [mr.keyswitch_share(tmo.party(name, i).rows(Q), tmo.party(name, 100 + i).rows(Q), Q, low, want["ct"][k][1], want["ks"]["e"][i][k], is_ntt)
                 for k in range(3)] if wl is None else want["ks"]["shares"][i]
            assert np.array_equal(shares[i].Value.numpy(), batch(w))
        # ---- PublicKeySwitchProtocol
        a, ep = want["pcks"]["pk_samples"]
        split = lambda x: (np.ascontiguousarray(x[:, :len(Q)]), np.ascontiguousarray(x[:, len(Q):]) if pc else None)
        pk = kg.GenPublicKeyNew(secret(kg, name, 200), samples={"a": split(a), "e": ep})
        pshares = [pcks.AllocateShare(share_level, 3) for _ in ids]
        for i in ids:
            smp = want["pcks"]["samples"][i]
            pcks.GenShare(sk[i], pk, ct, pshares[i], samples=smp, fused=fused)
            pkq, pkp = want["pcks"]["pk"]
            w = [mr.public_keyswitch_share(tmo.party(name, i).rows(Q), pkq, pkp, Q, [int(p) for p in P[:pc]], low, want["ct"][k][1], smp["u"][k],
                                           smp["e0"][k], smp["e1"][k], smp["e"][k], is_ntt) for k in range(3)] if wl is None else want["pcks"]["shares"][i]
            for c in (0, 1):
                assert np.array_equal(pshares[i].Value[c].numpy(), batch([x[c] for x in w]))
        if wl is None:
            continue
        # ---- aggregation and the switch: by the list form out of place, by the pairwise form in place
        mk = lambda: rh.Ciphertext([rl.NewPoly(3), rl.NewPoly(3)], is_ntt=not is_ntt)
        out = mk()
        cks.KeySwitch(ct, shares, out, fused=fused)                         # ctIn[0] and every share through one call
        pout = mk()
        pcks.KeySwitch(ct, pshares, pout, fused=fused)
        for c in (0, 1):
            assert np.array_equal(out.Value[c].numpy(), batch([x[c] for x in want["ks"]["out"]]))
            assert np.array_equal(pout.Value[c].numpy(), batch([x[c] for x in want["pcks"]["out"]]))
        assert out.IsNTT == is_ntt and pout.IsNTT == is_ntt
        for s in shares[1:]:
            cks.AggregateShares(shares[0], s, shares[0], fused=fused)
        assert np.array_equal(shares[0].Value.numpy(), batch(want["ks"]["agg"]))
        for s in pshares[1:]:
            pcks.AggregateShares(pshares[0], s, pshares[0], fused=fused)
        for c in (0, 1):
            assert np.array_equal(pshares[0].Value[c].numpy(), batch([x[c] for x in want["pcks"]["agg"]]))
        ct2 = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, batch([c[k] for c in want["ct"]])) for k in (0, 1)], is_ntt=is_ntt)
        pcks.KeySwitch(ct2, pshares[0], ct2, fused=fused)                   # in place
        cks.KeySwitch(ct, shares[0], ct, fused=fused)
        for c in (0, 1):
            assert np.array_equal(ct.Value[c].numpy(), batch([x[c] for x in want["ks"]["out"]]))
            assert np.array_equal(ct2.Value[c].numpy(), batch([x[c] for x in want["pcks"]["out"]]))


@pytest.mark.parametrize("nshares", [1, 2, 5, 9])
@pytest.mark.parametrize("name", ["TAIL", "REF", "Q61N13"])
def test_aggregate_alone_against_pairwise_add_and_python_integers(rh, name, nshares):
    N, Q, _, _ = tro.chain(name)
    Q = [int(q) for q in Q]
    rq, _ = rings(rh, name, 0 if name == "REF" else len(tro.chain(name)[2]))
    mp = rh.multiparty
    rng = np.random.default_rng(nshares)
    qcol = np.array(Q, dtype=np.uint64)[None, :, None]
    for level, npoly in ((len(Q) - 1, 3), (1, 2)):
        rl = rq.AtLevel(level)
        L = level + 1
        for kind in ("worst", "random"):
            if kind == "worst":
                host = [np.broadcast_to(qcol[:, :L] - np.uint64(1), (npoly, L, N)).copy() for _ in range(nshares)]
            else:
                host = [np.stack([np.stack([rng.integers(0, Q[l], size=N, dtype=np.uint64) for l in range(L)]) for _ in range(npoly)]) for _ in range(nshares)]
            want = np.zeros((npoly, L, N), dtype=object)
            for h in host:
                want = want + h.astype(object)
            want = np.stack([np.stack([(want[p, l] % Q[l]).astype(np.uint64) for l in range(L)]) for p in range(npoly)])
            dev = [rh.DevicePoly.from_numpy(rl, h) for h in host]
            out = rl.NewPoly(npoly)
            mp.aggregate(rq, dev, out, fused=True)
            assert np.array_equal(out.numpy(), want)
            pair = rl.NewPoly(npoly)
            mp.aggregate(rq, dev, pair, fused=False)                        # the pairwise Ring.Add calls
            assert np.array_equal(pair.numpy(), want)
            for k in sorted({0, nshares - 1}):                              # in place in the first and in the last share
                dev = [rh.DevicePoly.from_numpy(rl, h) for h in host]
                mp.aggregate(rq, dev, dev[k], fused=True)
                assert np.array_equal(dev[k].numpy(), want)
                for j, d in enumerate(dev):
                    assert j == k or np.array_equal(d.numpy(), host[j])
                dev = [rh.DevicePoly.from_numpy(rl, h) for h in host]
                mp.aggregate(rq, dev, dev[k], fused=False)
                assert np.array_equal(dev[k].numpy(), want)


def _std_bits(rh, rq, sk, ct, want_coeffs, level):
    """log2 std of the device decryption's error per ciphertext of the batch, against integer messages"""
    pt = rh.rlwe.Decryptor(rq, sk).DecryptNew(ct)
    if pt.IsNTT:
        rq.AtLevel(level).INTT(pt.Value, pt.Value)
    mods = [int(q) for q in rq.moduli[:level + 1]]
    a = pt.Value.numpy()
    return [rr.log2_std(rr.centered_diff(rr.crt_centered(a[k], mods), want_coeffs[k], rr.prod(mods))) for k in range(a.shape[0])]


def _sum_secret(rh, kg, sks):
    """the ideal secret: the sum of the parties' Values (the tests' skIdeal); no small coefficients"""
    rq, rp = kg.ringQ, kg.ringP
    q = rq.NewPoly(1)
    p = rp.NewPoly(1) if rp is not None else None
    rh.multiparty.aggregate(rq, [s.Value.Q for s in sks], q)
    if p is not None:
        rh.multiparty.aggregate(rp, [s.Value.P for s in sks], p)
    return rh.rlwe.SecretKey(None, q, p)


@pytest.mark.parametrize("t_of_n", [(2, 3), (4, 5)], ids=lambda x: "%d-of-%d" % x)
def test_threshold_reconstructs_the_ideal_secret_and_drives_a_key_switch(rh, t_of_n):
    t, n = t_of_n
    name, pc = "REF", 2
    N, Q, P, levels = tro.chain(name)
    Q, P = [int(q) for q in Q], [int(p) for p in P[:pc]]
    mods = Q + P
    mp = rh.multiparty
    rq, rp = rings(rh, name, pc)
    prng = rh.rlwe.KeyedPRNG(b"threshold %d of %d" % (t, n))
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sks = [kg.GenSecretKeyNew() for _ in range(n)]
    points = list(range(1, n + 1))
    thr = mp.Thresholdizer(rq, rp, prng=prng)
    polys = [thr.GenShamirPolynomial(t, s) for s in sks]
    # bit for bit: party 0's share for point 2 against Python integers
    host_poly = [qp((c.Q.numpy(), c.P.numpy()))[0] for c in polys[0].Value]
    one = thr.AllocateThresholdSecretShare()
    thr.GenShamirSecretShare(points[1], polys[0], one)
    assert np.array_equal(qp((one.Q.numpy(), one.P.numpy()))[0], mr.shamir_share(host_poly, points[1], mods))
    received = []
    for j in range(n):
        shares = [thr.AllocateThresholdSecretShare() for _ in range(n)]
        for i in range(n):
            thr.GenShamirSecretShare(points[j], polys[i], shares[i])
        agg = thr.AllocateThresholdSecretShare()
        thr.AggregateShares(shares, agg)
        received.append(agg)
    actives = points[n - t:]                                                # the LAST t parties are the active ones
    additive = []
    for j in range(n - t, n):
        cmb = mp.Combiner(rq, rp, points[j], points, t)
        out = rh.rlwe.SecretKey(None, rq.NewPoly(1), rp.NewPoly(1))
        cmb.GenAdditiveShare(actives, points[j], received[j], out)
        assert out.coeffs is None
        want = mr.additive_share(qp((received[j].Q.numpy(), received[j].P.numpy()))[0], points[j], actives, t, mods)
        assert np.array_equal(qp((out.Value.Q.numpy(), out.Value.P.numpy()))[0], want)
        additive.append(out)
    ideal = _sum_secret(rh, kg, sks)
    again = _sum_secret(rh, kg, additive)
    assert np.array_equal(again.Value.Q.numpy(), ideal.Value.Q.numpy()) and np.array_equal(again.Value.P.numpy(), ideal.Value.P.numpy())
    with pytest.raises(rh.RingHipError, match="Not enough active players"):
        mp.Combiner(rq, rp, 1, points, t).GenAdditiveShare(points[:t - 1], 1, received[0], rh.rlwe.SecretKey(None, rq.NewPoly(1), rp.NewPoly(1)))
    with pytest.raises(rh.RingHipError, match="threshold should be >= 1"):
        thr.GenShamirPolynomial(0, sks[0])
    # the additive shares (no small coefficients) as the input secrets of a collective key switch to fresh secrets
    level = levels[0]
    ct = rh.rlwe.Encryptor(rq, rp, ideal, prng=prng).EncryptZeroNew(level, npoly=2)
    outs = [kg.GenSecretKeyNew() for _ in range(t)]
    cks = mp.KeySwitchProtocol(rq, tmo.FLOOD, prng=prng)
    shares = [cks.AllocateShare(level, 2) for _ in range(t)]
    for i in range(t):
        cks.GenShare(additive[i], outs[i], ct, shares[i])
    cks.KeySwitch(ct, shares, ct)
    got = _std_bits(rh, rq, _sum_secret(rh, kg, outs), ct, [[0] * N] * 2, level)
    bound = math.log2(mp.NoiseKeySwitch(t, rr.SIGMA, tmo.FLOOD)) + 1
    print("MEASURED threshold key switch %d of %d %s [%.2f]" % (t, n, got, bound))
    assert max(got) <= bound


@pytest.mark.parametrize("setting", [(0, 2), (16, 1)], ids=lambda s: "pw%d-p%d" % s)
def test_no_host_key_material_collective_keys_serve_the_evaluator(rh, setting):
    """5 parties, a fixed KeyedPRNG each, no host key material: a collective public key, relinearisation key and two Galois keys; the existing
    rlwe.Evaluator relinearises and rotates under them and a collective key switch to fresh secrets decrypts, all within the reference's bounds
    (multiparty_test.go:167, :392; rlwe_test.go:703, :925-929 as tests/test_gpu_keygen.py states them)"""
    name = "REF"
    pw2, pc = setting
    N, Q, P, levels = tro.chain(name)
    mp = rh.multiparty
    rq, rp = rings(rh, name, pc)
    n = 5
    level = levels[0]
    rl = rq.AtLevel(level)
    prngs = [rh.rlwe.KeyedPRNG(b"party %d %d" % (i, pw2)) for i in range(n)]
    kgs = [rh.rlwe.KeyGenerator(rq, rp, prng=prngs[i]) for i in range(n)]
    sks = [kgs[i].GenSecretKeyNew() for i in range(n)]
    ideal = _sum_secret(rh, kgs[0], sks)
    kw = dict(BaseTwoDecomposition=pw2)
    crss = [mp.CRS(b"the common reference string") for _ in range(n)]      # every party its own CRS object, the same key
    # public key
    ckg = [mp.PublicKeyGenProtocol(rq, rp, prng=prngs[i]) for i in range(n)]
    crps = [ckg[i].SampleCRP(crss[i]) for i in range(n)]
    assert all(np.array_equal(crps[i].Value.Q.numpy(), crps[0].Value.Q.numpy()) for i in range(n))
    shares = [ckg[i].AllocateShare() for i in range(n)]
    for i in range(n):
        ckg[i].GenShare(sks[i], crps[i], shares[i])
    ckg[0].AggregateShares(shares, shares[0])
    pk = ckg[0].GenPublicKey(shares[0], crps[0])
    # relinearisation key
    rkg = [mp.RelinearizationKeyGenProtocol(rq, rp, prng=prngs[i]) for i in range(n)]
    rcrp = [rkg[i].SampleCRP(crss[i], **kw) for i in range(n)]
    assert all(np.array_equal(arr(rcrp[i]), arr(rcrp[0])) for i in range(n))
    alloc = [rkg[i].AllocateShare(**kw) for i in range(n)]
    for i in range(n):
        rkg[i].GenShareRoundOne(sks[i], rcrp[i], alloc[i][0], alloc[i][1])
    r1 = rkg[0].AllocateShare(**kw)[1]
    rkg[0].AggregateShares([a[1] for a in alloc], r1)
    for i in range(n):
        rkg[i].GenShareRoundTwo(alloc[i][0], sks[i], r1, alloc[i][2])
    r2 = alloc[0][2]
    rkg[0].AggregateShares([a[2] for a in alloc], r2)
    rlk = rkg[0].GenRelinearizationKey(r1, r2)
    # two Galois keys, one launch sequence per party
    galEls = [5, 2 * N - 1]
    gkg = [mp.GaloisKeyGenProtocol(rq, rp, prng=prngs[i]) for i in range(n)]
    gcrp = [gkg[i].SampleCRPs(crss[i], 2, **kw) for i in range(n)]
    gsh = [gkg[i].GenSharesNew(sks[i], galEls, gcrp[i]) for i in range(n)]
    aggs = gkg[0].AllocateShares(2, **kw)
    for k in range(2):
        gkg[0].AggregateShares([gsh[i][k] for i in range(n)], aggs[k])
    gks = gkg[0].GenGaloisKeysNew(aggs, gcrp[0])
    evs = rh.rlwe.MemEvaluationKeySet(rlk, gks)
    ev = rh.rlwe.Evaluator(rq, rp, galois_keys=evs.galois_keys)
    # a public-key encryption under the collective key decrypts under the ideal secret
    ms = tko.message(name, level)
    mods = [int(q) for q in Q[:level + 1]]
    pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rl, np.stack([rr.ntt(rr.rns(m, mods), N, mods) for m in ms])), is_ntt=True)
    ct = rh.rlwe.Encryptor(rq, rp, pk, prng=prngs[0]).EncryptNew(pt)
    hw = n * tmo.hamming_weight(N)                                           # the ideal secret's weight is at most the parties' together
    cpk_noise = math.sqrt(n) * rr.SIGMA                                      # the collective key's noise in the place of NoiseFreshSK (:167)
    bnd = math.log2(math.sqrt((hw + 1) * (1 / 12.0 if pc else cpk_noise ** 2))) + 1
    got = _std_bits(rh, rq, ideal, ct, ms, level)
    print("MEASURED collective pk encryption pw%d-p%d %s [%.2f]" % (pw2, pc, got, bnd))
    assert max(got) <= bnd
    # rotations and the relinearisation under the collective keys.  The evaluator's bounds (LogN + pw2, rlwe_test.go:703, :925-929) are stated for
    # keys of noise NoiseFreshSK; a collective key's rows carry sqrt(5) (evaluation, Galois) and NoiseRelinearizationKey / NoiseFreshSK times it
    out = rh.Ciphertext([rl.NewPoly(3), rl.NewPoly(3)], is_ntt=True)
    extra = math.log2(mp.NoiseGaloisKey(n) / rr.SIGMA)
    for g in galEls:
        ev.Automorphism(ct, g, out)
        got = _std_bits(rh, rq, ideal, out, [rr.automorphism_coeffs(m, g) for m in ms], level)
        print("MEASURED collective auto %-4d pw%d-p%d %s [%.2f]" % (g, pw2, pc, got, tro.bound(N, pw2, level) + extra))
        assert max(got) <= tro.bound(N, pw2, level) + extra
    zero = rl.NewPoly(3)
    rl.vec_op("ZERO", None, None, zero)
    ct2 = rh.Ciphertext([ct.Value[0], zero, ct.Value[1]], is_ntt=True)
    want = rh.rlwe.Decryptor(rq, ideal).DecryptNew(ct2)
    rl.INTT(want.Value, want.Value)
    a = want.Value.numpy()
    want2 = [rr.crt_centered(a[k], mods) for k in range(3)]
    ev.GadgetProduct(level, ct.Value[1], rlk, out)
    rl.Add(out.Value[0], ct.Value[0], out.Value[0])
    extra = math.log2(mp.NoiseRelinearizationKey(tmo.hamming_weight(N), n) / rr.SIGMA)
    got = _std_bits(rh, rq, ideal, out, want2, level)
    print("MEASURED collective relin pw%d-p%d %s [%.2f]" % (pw2, pc, got, tro.bound(N, pw2) + extra))
    assert max(got) <= tro.bound(N, pw2) + extra
    # a collective key switch to fresh secrets, and a public one to a fresh key pair
    zero_ct = rh.rlwe.Encryptor(rq, rp, ideal, prng=prngs[0]).EncryptZeroNew(level, npoly=3)
    outs = [kgs[i].GenSecretKeyNew() for i in range(n)]
    cks = [mp.KeySwitchProtocol(rq, tmo.FLOOD, prng=prngs[i]) for i in range(n)]
    shares = [cks[i].AllocateShare(level, 3) for i in range(n)]
    for i in range(n):
        cks[i].GenShare(sks[i], outs[i], zero_ct, shares[i])
    res = rh.Ciphertext([rl.NewPoly(3), rl.NewPoly(3)], is_ntt=True)
    cks[0].KeySwitch(zero_ct, shares, res)
    bound = math.log2(mp.NoiseKeySwitch(n, rr.SIGMA, tmo.FLOOD)) + 1
    got = _std_bits(rh, rq, _sum_secret(rh, kgs[0], outs), res, [[0] * N] * 3, level)
    print("MEASURED collective key switch pw%d-p%d %s [%.2f]" % (pw2, pc, got, bound))
    assert max(got) <= bound
    tsk, tpk = kgs[0].GenKeyPairNew()
    pcks = [mp.PublicKeySwitchProtocol(rq, rp, tmo.FLOOD, prng=prngs[i]) for i in range(n)]
    pshares = [pcks[i].AllocateShare(level, 3) for i in range(n)]
    for i in range(n):
        pcks[i].GenShare(sks[i], tpk, zero_ct, pshares[i])
    pcks[0].KeySwitch(zero_ct, pshares, res)
    bound = math.log2(mp.NoisePublicKeySwitch(n, rr.SIGMA, tmo.FLOOD, kr.noise_fresh_pk(tmo.hamming_weight(N), pc > 0))) + 1
    got = _std_bits(rh, rq, tsk, res, [[0] * N] * 3, level)
    print("MEASURED collective public key switch pw%d-p%d %s [%.2f]" % (pw2, pc, got, bound))
    assert max(got) <= bound
    ev.close()


def test_prng_shares_equal_the_restatement_whole_and_chunked(rh):
    """no samples handed in: a party's errors come from its PRNG's stream, and the restated sampler with the same call counter gives the same
    shares; chunked over the keys (one key per chunk) the same arrays again"""
    case = ("REF", (0, 2), None)
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    rq, rp = rings(rh, "REF", 2)
    galEls = tuple(tko.galois_elements(N))
    want = tmo.protocol(case, PARTIES, galEls)
    prng = rh.rlwe.KeyedPRNG(tmo.KEY)
    gkg = rh.multiparty.GaloisKeyGenProtocol(rq, rp, prng=prng)
    sk = secret(rh.rlwe.KeyGenerator(rq, rp), "REF", 1)
    crs = rh.multiparty.CRS(tmo.CRS_KEY)
    crs.calls = tmo.CRP_GAL                                                 # where the parties' CRS stands when they sample the Galois CRPs
    crps = gkg.SampleCRPs(crs, len(galEls))
    import matrix_fhe_lattigo_amd.keygen as keygen
    cap = keygen.SCRATCH_CAP
    try:
        for c in (cap, 1):
            keygen.SCRATCH_CAP = c
            prng.calls = 1000 * (1 + 1) + 6                                 # party 1's call counter of this step (tmo.errors)
            shares = gkg.GenSharesNew(sk, galEls, crps)
            assert prng.calls == 1000 * 2 + 7
            for k in range(len(galEls)):
                assert np.array_equal(arr(shares[k]), want["gal"]["shares"][1][k])
    finally:
        keygen.SCRATCH_CAP = cap


@pytest.mark.parametrize("policy", [0, 2], ids=["default-policy", "non-temporal"])
def test_every_cache_policy_gives_the_same_bits(rh, policy):
    """one REF case of every new kernel under tuning nt_streams = 0 and 2: the same arrays as under the by-working-set rule"""
    case = ("REF", (0, 2), None)
    rq, rp = rings(rh, "REF", 2)
    try:
        for r in (rq, rp):
            r.set_tuning("nt_streams", policy)
        test_key_protocols_from_samples_bit_for_bit(rh, case, True)        # rh_mp_aggregate, rh_mp_gadget_share, both relinearisation rounds
        test_switching_protocols_on_a_batch_bit_for_bit(rh, ("REF", 2), True, True)     # rh_mp_keyswitch_share, every template arm but the product alone
        test_switching_protocols_on_a_batch_bit_for_bit(rh, ("REF", 2), False, True)    # ... and the product alone
    finally:
        for r in (rq, rp):
            r.set_tuning("nt_streams", 1)


def test_refusals(rh):
    mp = rh.multiparty
    rq, rp = rings(rh, "TAIL", 4)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    sk = secret(kg, "TAIL", 0)
    ci = rh.Ring(32, [0x1fffffffffe00001], kind=rh.ConjugateInvariant)
    for make in (lambda: mp.PublicKeyGenProtocol(ci), lambda: mp.EvaluationKeyGenProtocol(ci), lambda: mp.GaloisKeyGenProtocol(ci),
                 lambda: mp.RelinearizationKeyGenProtocol(ci), lambda: mp.KeySwitchProtocol(ci, 25.6), lambda: mp.PublicKeySwitchProtocol(ci, None, 25.6),
                 lambda: mp.Thresholdizer(ci), lambda: mp.Combiner(ci, None, 1, [1, 2], 2)):
        with pytest.raises(rh.RingHipError, match="standard rings only"):
            make()
    with pytest.raises(rh.RingHipError, match="invalid distribution type"):
        mp.KeySwitchProtocol(rq, ("uniform", 3))
    with pytest.raises(rh.RingHipError, match="invalid distribution type"):
        mp.PublicKeySwitchProtocol(rq, rp, "ternary")
    with pytest.raises(rh.RingHipError, match="big-norm"):
        mp.KeySwitchProtocol(rq, 171.0)                                     # bound = 6 sqrt(3.2^2 + 171^2) > 1024
    with pytest.raises(rh.RingHipError, match="big-norm"):
        mp.PublicKeySwitchProtocol(rq, rp, (3.2, 1024))
    ekg = mp.EvaluationKeyGenProtocol(rq, rp)
    crs = mp.CRS(b"refusals")
    share = ekg.AllocateShare()
    with pytest.raises(rh.RingHipError, match=r"crp.BaseRNSDecompositionVectorSize\(\) != shareOut.BaseRNSDecompositionVectorSize\(\)"):
        ekg.GenShare(sk, sk, ekg.SampleCRP(crs, levelQ=2), share)
    e1 = mp.EvaluationKeyGenProtocol(rq, rings(rh, "TAIL", 1)[1])
    with pytest.raises(rh.RingHipError, match=r"crp.BaseTwoDecompositionVectorSize\(\) != shareOut.BaseTwoDecompositionVectorSize\(\)"):
        e1.GenShare(sk, sk, e1.SampleCRP(crs, BaseTwoDecomposition=16), e1.AllocateShare(BaseTwoDecomposition=31))
    with pytest.raises(rh.RingHipError, match="share LevelQ do not match"):
        ekg.AggregateShares(share, ekg.AllocateShare(levelQ=5), share)
    with pytest.raises(rh.RingHipError, match="share LevelP do not match"):
        ekg.AggregateShares(share, ekg.AllocateShare(levelP=1), share)
    with pytest.raises(rh.RingHipError, match="compressed"):
        ekg.AllocateShare(compressed=True)
    with pytest.raises(rh.RingHipError, match="cannot be allocated in the compressed format"):
        mp.RelinearizationKeyGenProtocol(rq, rp).AllocateShare(compressed=True)
    gkg = mp.GaloisKeyGenProtocol(rq, rp)
    a, b = gkg.AllocateShare(), gkg.AllocateShare()
    a.GaloisElement, b.GaloisElement = 5, 25
    with pytest.raises(rh.RingHipError, match="do not share the same GaloisElement: 5 != 25"):
        gkg.AggregateShares(a, b, a)
    cks = mp.KeySwitchProtocol(rq, 25.6)
    with pytest.raises(rh.RingHipError, match="shares levels do not match"):
        cks.AggregateShares(cks.AllocateShare(3), cks.AllocateShare(2), cks.AllocateShare(3))
    L = rh.lib()
    h = rq._h
    assert L.rh_mp_aggregate(h, 0, None, 1, None, 1, None, 0) != 0 and b"null argument" in L.rh_last_error()
    assert L.rh_mp_gadget_share(h, None, 0, -1, *([None] * 9), 1, 1, None, 1, None, 0) != 0 and b"null argument" in L.rh_last_error()
    assert L.rh_mp_relin_round_one(h, None, 0, -1, *([None] * 13), None, 1, None, 0) != 0 and b"null argument" in L.rh_last_error()
    assert L.rh_mp_relin_round_two(h, None, 0, -1, *([None] * 10), 1) != 0 and b"null argument" in L.rh_last_error()
    assert L.rh_mp_keyswitch_share(h, 0, None, 1, None, None, None, None, None, 1) != 0 and b"null argument" in L.rh_last_error()
    x = rq.AtLevel(0).NewPoly(1)
    ptrs = (ctypes.c_void_p * 1)(x.ptr)
    assert L.rh_mp_aggregate(h, 9, ptrs, 1, x.ptr, 1, x.ptr, 1) != 0 and b"out of range" in L.rh_last_error()
    assert L.rh_mp_aggregate(h, 0, ptrs, 0, x.ptr, 1, x.ptr, 1) != 0 and b"shares" in L.rh_last_error()
    ci.close()

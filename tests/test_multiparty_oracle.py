"""CPU: the restated multiparty protocols (tests/multiparty_restatement.py), fed by the restated samplers (tests/sampling_restatement.py) under a
fixed key, pinned to DECRYPTION with the bounds the reference's own tests state (multiparty/multiparty_test.go), in its own set-up: 5 parties,
its test moduli (the REF chain) with the settings (pw2, #P) = (16, 1) and (0, 2), at the top level and at level 1, flooding sigma 8 * 3.2:

  collective public key                    row_noise <= log2(sqrt(5) NoiseFreshSK) + 1                                        :167
  relinearisation, evaluation, Galois key  row_noise <= log2(sqrt(BaseRNSDecompositionVectorSize) Noise...Key(params, 5)) + 1  :222-224, :277-279, :325-327
  key switch, public key switch of a zero encryption, out of place and in place
                                           log2 std <= log2(NoiseKeySwitch / NoisePublicKeySwitch(params, 5, NoiseFreshSK, 25.6)) + 1   :392, :402, :461, :471
  thresholds 1, 2 and 4 of 5, points 1..5  the additive shares of the first `threshold` parties sum to the ideal secret exactly    :555

These tests exercise the restatement, not the package.  protocol() and switching() also make the expected arrays tests/test_gpu_multiparty.py
compares the device path with, for 3 parties on the cases of tests/test_keygen_oracle.py."""
import functools
import math

import numpy as np
import pytest

import keygen_restatement as kr
import multiparty_restatement as mr
import rlwe_restatement as rr
import sampling_restatement as sr
import test_keygen_oracle as tko
import test_rlwe_oracle as tro

KEY = b"multiparty restatement key"                 # the parties' private samples
CRS_KEY = b"multiparty common reference string"     # the common reference polynomials
FLOOD = 8 * rr.SIGMA
KS_SIGMA = math.sqrt(rr.SIGMA ** 2 + FLOOD ** 2)                           # keyswitch_sk.go:78-84
KS_TABLE = sr.gaussian_table(KS_SIGMA, 6 * KS_SIGMA)
PCKS_TABLE = sr.gaussian_table(FLOOD, 6 * FLOOD)
# the call counters of the CRS, in the order the parties sample: public key, evaluation key, relinearisation key, then one per Galois key
CRP_CPK, CRP_EVK, CRP_RLK, CRP_GAL = 0, 1, 2, 3
REF_CASES = [("REF", (16, 1), None), ("REF", (16, 1), 1), ("REF", (0, 2), None), ("REF", (0, 2), 1)]


def hamming_weight(N):
    return math.ceil(N * 2 / 3)                                            # Parameters.XsHammingWeight for Ternary{P} (params.go:427-434)


def noise_relin(N, parties):
    """NoiseRelinearizationKey (utils.go:10-26)"""
    H = float(parties * hamming_weight(N))
    return math.sqrt(2 * parties * rr.SIGMA ** 2 * (H + 1))


def noise_evk(parties):
    """NoiseEvaluationKey / NoiseGaloisKey (utils.go:29-36)"""
    return math.sqrt(parties) * rr.SIGMA


def noise_switch(parties, fresh):
    """noiseDecryptWithSmudging (utils.go:49-56) with noisect = NoiseFreshSK and the flooding sigma of these tests"""
    return math.sqrt(parties * (fresh ** 2 + FLOOD ** 2) + rr.SIGMA ** 2)


@functools.lru_cache(maxsize=None)
def party(name, i):
    """party i's secret; i >= 100: the output secrets of the switching protocols"""
    return kr.secret(sr.ternary(KEY, 3000 + i, 1, tro.chain(name)[0], tko.THRESHOLD)[0])


def ideal(name, ids):
    N = tro.chain(name)[0]
    return rr.Secret(N, [sum(party(name, i).coeffs[k] for i in ids) for k in range(N)])


def errors(i, what, rows, N, table=tko.TABLE):
    """party i's error rows of protocol step `what` (a call counter of its own per party and step)"""
    return sr.gaussian(KEY, 1000 * (i + 1) + what, rows, N, table)


@functools.lru_cache(maxsize=None)
def protocol(case, parties, galEls):
    """every key protocol of a case run by `parties` parties: CRPs, samples, shares, aggregates and keys"""
    name = case[0]
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    LQ = levelQ + 1
    mods = mr.mods_of(Q, P, levelQ, levelP)
    rows = kr.rows_of(Q, levelQ, levelP, pw2)
    ids = list(range(parties))
    sk = [party(name, i).rows(mods) for i in ids]
    sk_out = [party(name, 100 + i).rows(mods) for i in ids]
    out = {"rows": rows}
    # the collective public key lives on the whole of Q and the setting's P
    full = mr.mods_of(Q, P, len(Q) - 1, levelP)
    crp = sr.uniform(CRS_KEY, CRP_CPK, 1, N, full)
    e = [errors(i, 0, 1, N) for i in ids]
    shares = [mr.public_key_share(party(name, i).rows(full), Q, P, crp, e[i]) for i in ids]
    agg = mr.aggregate(shares, full)
    out["cpk"] = dict(crp=crp, e=e, shares=shares, agg=agg, key=mr.gadget_key(agg, crp, Q, P, len(Q) - 1, levelP, 0, dpl=[1]))
    # evaluation key sk -> sk_out
    crp = sr.uniform(CRS_KEY, CRP_EVK, rows, N, mods)
    e = [errors(i, 1, rows, N) for i in ids]
    shares = [mr.gadget_share(sk[i][:LQ], sk_out[i], Q, P, levelQ, levelP, pw2, crp, e[i]) for i in ids]
    agg = mr.aggregate(shares, mods)
    out["evk"] = dict(crp=crp, e=e, shares=shares, agg=agg, key=mr.gadget_key(agg, crp, Q, P, levelQ, levelP, pw2))
    # relinearisation key, two rounds
    crp = sr.uniform(CRS_KEY, CRP_RLK, rows, N, mods)
    u = [sr.ternary(KEY, 1000 * (i + 1) + 2, 1, N, tko.THRESHOLD)[0] for i in ids]
    u_rows = [kr.secret(u[i]).rows(mods) for i in ids]
    e0, e1, e2 = ([errors(i, w, rows, N) for i in ids] for w in (3, 4, 5))
    r1 = [mr.relin_round_one(sk[i], u_rows[i], Q, P, levelQ, levelP, pw2, crp, e0[i], e1[i]) for i in ids]
    r1_agg = mr.aggregate(r1, mods)
    r2 = [mr.relin_round_two(u_rows[i], sk[i], Q, P, levelQ, levelP, r1_agg, e2[i]) for i in ids]
    r2_agg = mr.aggregate(r2, mods)
    out["rlk"] = dict(crp=crp, u=u, u_rows=u_rows, e0=e0, e1=e1, e2=e2, r1=r1, r1_agg=r1_agg, r2=r2, r2_agg=r2_agg,
                      key=mr.relin_key(r1_agg, r2_agg, Q, P, levelQ, levelP, pw2))
    # Galois keys: one CRP per element, the errors of a party key-major in one block
    crps = [sr.uniform(CRS_KEY, CRP_GAL + k, rows, N, mods) for k in range(len(galEls))]
    e = [errors(i, 6, rows * len(galEls), N) for i in ids]
    shares = [[mr.gadget_share(sk[i][:LQ], mr.galois_sk_out(sk[i], N, g), Q, P, levelQ, levelP, pw2, crps[k], e[i][k * rows:(k + 1) * rows])
               for k, g in enumerate(galEls)] for i in ids]
    aggs = [mr.aggregate([shares[i][k] for i in ids], mods) for k in range(len(galEls))]
    out["gal"] = dict(crps=crps, e=e, shares=shares, aggs=aggs, keys=[mr.gadget_key(a, c, Q, P, levelQ, levelP, pw2) for a, c in zip(aggs, crps)])
    return out


@functools.lru_cache(maxsize=None)
def switching(name, pc, parties, level, is_ntt, npoly=1):
    """the two switching protocols on a batch of `npoly` zero encryptions under the ideal secret at `level`: samples, shares, results"""
    N, Q, P = tro.chain(name)[:3]
    Q, P = [int(q) for q in Q], [int(p) for p in P[:pc]]
    mods = Q[:level + 1]
    ids = list(range(parties))
    sk_ideal = ideal(name, ids)
    sk = [party(name, i).rows(Q) for i in ids]
    sk_out = [party(name, 100 + i).rows(Q) for i in ids]
    c1, e = sr.uniform(KEY, 70, npoly, N, mods), sr.gaussian(KEY, 71, npoly, N, tko.TABLE)
    cts = [kr.encrypt_sk(sk_ideal, Q, level, c1[k], e[k], None, is_ntt) for k in range(npoly)]
    out = {"ct": cts, "sk_samples": (c1, e)}
    es = [errors(i, 7, npoly, N, KS_TABLE) for i in ids]
    shares = [[mr.keyswitch_share(sk[i], sk_out[i], Q, level, cts[k][1], es[i][k], is_ntt) for k in range(npoly)] for i in ids]
    agg = [mr.aggregate([shares[i][k] for i in ids], mods) for k in range(npoly)]
    out["ks"] = dict(e=es, shares=shares, agg=agg, out=[mr.keyswitch(cts[k], agg[k], Q) for k in range(npoly)])
    # the public key of one further party, made as tests/test_keygen_oracle.py makes its own
    target = party(name, 200)
    a, ep = sr.uniform(KEY, 72, 1, N, Q + P), sr.gaussian(KEY, 73, 1, N, tko.TABLE)
    pkq, pkp = kr.public_key(target, Q, P, a, ep)
    smp = [dict(u=sr.ternary(KEY, 1000 * (i + 1) + 8, npoly, N, tko.THRESHOLD), e0=errors(i, 9, npoly, N), e1=errors(i, 10, npoly, N),
                e=errors(i, 11, npoly, N, PCKS_TABLE)) for i in ids]
    shares = [[mr.public_keyswitch_share(sk[i], pkq, pkp, Q, P, level, cts[k][1], smp[i]["u"][k], smp[i]["e0"][k], smp[i]["e1"][k], smp[i]["e"][k],
                                         is_ntt) for k in range(npoly)] for i in ids]
    agg = [[mr.aggregate([shares[i][k][c] for i in ids], mods) for c in (0, 1)] for k in range(npoly)]
    out["pcks"] = dict(pk_samples=(a, ep), pk=(pkq, pkp), samples=smp, shares=shares, agg=agg,
                       out=[mr.public_keyswitch(cts[k], agg[k], Q) for k in range(npoly)])
    return out


def _report(what, case, got, bound):
    print("MEASURED %-10s %s  %5.2f [%.2f]" % (what, tko._ids(case), got, bound))
    assert got <= bound, what


@pytest.mark.parametrize("case", REF_CASES, ids=tko._ids)
def test_collective_keys_are_fresh_encryptions_under_the_ideal_secret(oracle, case):
    name = case[0]
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    n = 5
    g = pow(5, 64, 2 * N)                                                   # params.GaloisElement(64) (:289)
    p = protocol(case, n, (g,))
    ids = list(range(n))
    sk, sk_out = ideal(name, ids), ideal(name, [100 + i for i in ids])
    digits = rr.rns_digits(levelQ, levelP)
    if case[2] is None:
        _report("cpk", case, tko.row_noise(p["cpk"]["key"], sk, None, Q, P), math.log2(math.sqrt(n) * rr.SIGMA) + 1)
    bound = math.log2(math.sqrt(digits) * noise_evk(n)) + 1
    _report("evk", case, tko.row_noise(p["evk"]["key"], sk_out, sk, Q, P), bound)
    _report("gal", case, tko.row_noise(p["gal"]["keys"][0], sk.automorphism(rr.galois_inverse(N, g)), sk, Q, P), bound)
    _report("rlk", case, tko.row_noise(p["rlk"]["key"], sk, sk.square(), Q, P), math.log2(math.sqrt(digits) * noise_relin(N, n)) + 1)


@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coeff"])
@pytest.mark.parametrize("case", REF_CASES, ids=tko._ids)
def test_collective_key_switches_of_a_zero_encryption_decrypt(oracle, case, is_ntt):
    name, (pw2, pc), _ = case
    N, Q, P, level, levelP, pw2 = tko.dims(case)
    n = 5
    s = switching(name, pc, n, level, is_ntt)
    mods = Q[:level + 1]
    zero = [0] * N

    def std(ct, secret):
        pt = kr.decrypt(ct, secret, Q, is_ntt)
        return rr.log2_std(rr.centered_diff(rr.crt_centered(rr.intt(pt, N, mods) if is_ntt else pt, mods), zero, rr.prod(mods)))
    ks_bound = math.log2(noise_switch(n, rr.SIGMA)) + 1
    _report("ks", case, std(s["ks"]["out"][0], ideal(name, [100 + i for i in range(n)])), ks_bound)
    pk_bound = math.log2(noise_switch(n, kr.noise_fresh_pk(hamming_weight(N), pc > 0))) + 1
    _report("pcks", case, std(s["pcks"]["out"][0], party(name, 200)), pk_bound)
    # in place (:394, :463): the same arithmetic writes over ctIn; the restatement has no aliasing, so the result is the same arrays
    ct = [x.copy() for x in s["ct"][0]]
    ct[0] = mr.keyswitch(ct, s["ks"]["agg"][0], Q)[0]
    assert np.array_equal(ct[0], s["ks"]["out"][0][0]) and np.array_equal(ct[1], s["ks"]["out"][0][1])


@pytest.mark.parametrize("threshold", [1, 2, 4])
@pytest.mark.parametrize("setting", [(16, 1), (0, 2)], ids=lambda s: "pw%d-p%d" % s)
def test_threshold_additive_shares_sum_to_the_ideal_secret(oracle, setting, threshold):
    """(:475-560): every party shares its secret t-out-of-5 with points 1..5 and aggregates what it receives; the first t parties' additive shares
    sum to the ideal secret, exactly, modulo every limb of Q and of P"""
    N, Q, P, _ = tro.chain("REF")
    mods = [int(q) for q in Q] + [int(p) for p in P[:setting[1]]]
    n = 5
    points = list(range(1, n + 1))
    polys = [[party("REF", i).rows(mods)] + [sr.uniform(KEY, 5000 + 10 * i + d, 1, N, mods)[0] for d in range(1, threshold)] for i in range(n)]
    received = [mr.aggregate([mr.shamir_share(polys[i], points[j], mods) for i in range(n)], mods) for j in range(n)]
    actives = points[:threshold]
    additive = [mr.additive_share(received[j], points[j], actives, threshold, mods) for j in range(threshold)]
    assert np.array_equal(mr.aggregate(additive, mods), ideal("REF", list(range(n))).rows(mods))

"""The multiparty protocols on the device at the shape of profiles/keygen.json (N = 2^16, 25 + 5 limbs, 5 digits): writes profiles/multiparty.json.

  (a) rh_mp_aggregate for 2, 5 and 16 shares of one gadget share (its Q part) against the pairwise Add calls on the same blocks, as bytes moved
      per second (P + 1 block passes for the kernel, 3 (P - 1) for the pairwise calls);
  (b) rh_mp_gadget_share and rh_mp_keyswitch_share against their composed calls on the same prepared rows;
  (c) a whole GenShare either way: evaluation key, both relinearisation rounds, KeySwitchProtocol.GenShare at batch 1 and 8;
  (d) one party's shares for the 48 Galois keys of the bootstrapping parameters and a relinearisation key (two rounds), one launch sequence each;
  (e) the aggregation of 5 parties' Galois-key shares, every key, either way.

Method: device events around windows of calls after 2 warm-up calls, 3 alternating windows per side, the median reported with min and max;
(d) is a host clock around work that ends in a synchronise.  Usage: python tools/bench_multiparty.py [OUT.json]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import matrix_fhe_lattigo_amd as rh
from matrix_fhe_lattigo_amd import keygen as KG
from matrix_fhe_lattigo_amd import multiparty as MP
from oracle import primes

stream = torch.cuda.current_stream()


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stat(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def ab(fused, composed, reps_f, reps_c, rounds=3, warm=2):
    """alternating windows -> (fused stats, composed stats, composed / fused)"""
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(timed(fused, reps_f, warm)); tc.append(timed(composed, reps_c, warm))
    f, c = stat(tf), stat(tc)
    return {"fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 2)}


def main(out_path):
    N = 1 << 16
    Q, P = primes.gen_moduli(17, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    LQ, LP = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    prng = rh.rlwe.KeyedPRNG(b"bench multiparty")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk, sk_out = kg.GenSecretKeyNew(), kg.GenSecretKeyNew()
    crs = MP.CRS(b"bench crs")
    dpl = KG.digits_per_limb(Q, LQ - 1, LP - 1, 0)
    rows = len(dpl)
    out = {"device": torch.cuda.get_device_name(0), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "digits": rows},
           "method": __doc__.split("Method: ")[1].split("  Usage")[0].replace("\n", " ")}

    # (a) aggregation of the Q part of one gadget share
    agg = []
    block = rows * LQ * N * 8
    for n in (2, 5, 16):
        shares = [rq.NewPoly(rows) for _ in range(n)]
        for s in shares:
            kg.uniform.Read(s)
        dst = rq.NewPoly(rows)
        r = ab(lambda: MP.aggregate(rq, shares, dst, True), lambda: MP.aggregate(rq, shares, dst, False), 10, 5)
        r.update(op="%d shares of (%d, %d, N): rh_mp_aggregate vs %d pairwise Add" % (n, rows, LQ, n - 1), block_bytes=block,
                 fused_bytes_moved=(n + 1) * block, composed_bytes_moved=3 * (n - 1) * block,
                 fused_GBps=round((n + 1) * block / (r["fused"]["ms_median"] * 1e-3) / 1e9, 1),
                 composed_GBps=round(3 * (n - 1) * block / (r["composed"]["ms_median"] * 1e-3) / 1e9, 1))
        agg.append(r)
        del shares, dst
    out["aggregate"] = agg

    # (b) the share kernels on prepared rows
    kern = []
    ekg = MP.EvaluationKeyGenProtocol(rq, rp, prng=prng)
    one = KG.gadget_row_table(Q, P, LQ - 1, LP - 1, 0, dpl)
    for nkeys in (1, 8):
        R = rows * nkeys
        crp = ekg.SampleCRPs(crs, nkeys)
        cq = rh.DevicePoly(rq, R, LQ, ptr=crp[0].Q.ptr, owner=crp[0].Q)
        cp = rh.DevicePoly(rp, R, LP, ptr=crp[0].P.ptr, owner=crp[0].P)
        eQ, eP, hq, hp = rq.NewPoly(R), rp.NewPoly(R), rq.NewPoly(R), rp.NewPoly(R)
        kg.uniform.Read(eQ, eP)
        outQ, outP = rq.NewPoly(nkeys), rp.NewPoly(nkeys)
        kg.uniform.Read(outQ, outP)
        table = rh.DevicePoly(rq.AtLevel(0), (R * (LQ + 1) + N - 1) // N + 1, 1)
        call = lambda f: ekg._rows_apply(rq, rp, eQ, eP, cq, cp, hq, hp, sk.Value.Q, outQ, outP, nkeys, 0, nkeys, rows, one, table, f)
        r = ab(lambda: call(True), lambda: call(False), 10, 3)
        moved = R * (LQ + LP) * N * 8 * 3
        r.update(op="rows of %d key share(s): rh_mp_gadget_share vs MForm + MulScalarMontgomeryThenAdd + MulCoeffsMontgomeryThenSub per row" % nkeys,
                 rows=R, fused_GBps_moved=round(moved / (r["fused"]["ms_median"] * 1e-3) / 1e9, 1))
        kern.append(r)
        del crp, cq, cp, eQ, eP, hq, hp
    for B in (1, 8):
        c1, e, dst = rq.NewPoly(B), rq.NewPoly(B), rq.NewPoly(B)
        kg.uniform.Read(c1); kg.uniform.Read(e)
        a, b = sk.Value.Q, sk_out.Value.Q
        r = ab(lambda: MP._share_product(rq, c1, a, b, None, e, dst, True), lambda: MP._share_product(rq, c1, a, b, None, e, dst, False), 20, 5)
        r.update(op="c1 (skIn - skOut) + e, batch %d: rh_mp_keyswitch_share vs Sub + MulCoeffsMontgomery per ciphertext + Add" % B, rows=B * LQ)
        kern.append(r)
    out["share_kernels"] = kern

    # (c) whole calls either way
    whole = []
    crp = ekg.SampleCRP(crs)
    share = ekg.AllocateShare()
    r = ab(lambda: ekg.GenShare(sk, sk_out, crp, share, fused=True), lambda: ekg.GenShare(sk, sk_out, crp, share, fused=False), 5, 3, warm=1)
    r.update(op="EvaluationKeyGenProtocol.GenShare, whole call")
    whole.append(r)
    rkg = MP.RelinearizationKeyGenProtocol(rq, rp, prng=prng)
    eph, r1, r2 = rkg.AllocateShare()
    r = ab(lambda: rkg.GenShareRoundOne(sk, crp, eph, r1, fused=True), lambda: rkg.GenShareRoundOne(sk, crp, eph, r1, fused=False), 5, 3, warm=1)
    r.update(op="RelinearizationKeyGenProtocol.GenShareRoundOne, whole call")
    whole.append(r)
    r = ab(lambda: rkg.GenShareRoundTwo(eph, sk, r1, r2, fused=True), lambda: rkg.GenShareRoundTwo(eph, sk, r1, r2, fused=False), 5, 3, warm=1)
    r.update(op="RelinearizationKeyGenProtocol.GenShareRoundTwo, whole call")
    whole.append(r)
    cks = MP.KeySwitchProtocol(rq, 8 * 3.2, prng=prng)
    for B in (1, 8):
        ct = rh.rlwe.Encryptor(rq, rp, sk, prng=prng).EncryptZeroNew(LQ - 1, npoly=B)
        ks = cks.AllocateShare(LQ - 1, B)
        r = ab(lambda: cks.GenShare(sk, sk_out, ct, ks, fused=True), lambda: cks.GenShare(sk, sk_out, ct, ks, fused=False), 10, 5, warm=1)
        r.update(op="KeySwitchProtocol.GenShare, batch %d, NTT domain, whole call" % B)
        whole.append(r)
    out["whole_calls"] = whole
    del crp, share, r1, r2

    # (d) one party's shares for the bootstrapping key set; (e) the aggregation of five parties' shares
    B_, D, M = rh.bootstrapping, rh.dft, rh.mod1
    s2c = D.MatrixLiteral(D.HomomorphicDecode, 15, 12, LP - 1, [1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    c2s = D.MatrixLiteral(D.HomomorphicEncode, 15, 24, LP - 1, [1, 1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    m1 = M.ParametersLiteral(LevelQ=20, LogScale=60, Mod1Type=M.CosDiscrete, LogMessageRatio=8, K=16, Mod1Degree=30, DoubleAngle=3)
    params = B_.Parameters(rq, rp, 9, 1 << 40, s2c, m1, c2s, EphemeralSecretWeight=32)
    galEls = [g for g in params.GaloisElements() if g != 1]
    gkg = MP.GaloisKeyGenProtocol(rq, rp, prng=prng)
    gcrp = gkg.SampleCRPs(crs, len(galEls))
    rcrp = rkg.SampleCRP(crs)
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        gsh = gkg.GenSharesNew(sk, galEls, gcrp)
        eph, r1, r2 = rkg.AllocateShare()
        rkg.GenShareRoundOne(sk, rcrp, eph, r1)
        rkg.GenShareRoundTwo(eph, sk, r1, r2)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del eph, r1, r2
    share_bytes = rows * (LQ + LP) * N * 8
    out["bootstrapping_key_shares_one_party"] = {"galois_keys": len(galEls), "relinearization_keys": 1, "bytes_per_share": share_bytes, "wall": stat(walls)}
    parties = [gsh] + [gkg.AllocateShares(len(galEls)) for _ in range(4)]
    nk = len(galEls)
    whole_q = lambda s: rh.DevicePoly(rq, nk * rows, LQ, ptr=s[0].Q.ptr, owner=s[0].Q)      # a party's shares of every key lie in one block
    whole_p = lambda s: rh.DevicePoly(rp, nk * rows, LP, ptr=s[0].P.ptr, owner=s[0].P)
    for s in parties[1:]:
        kg.uniform.Read(whole_q(s), whole_p(s))
    dst = gkg.AllocateShares(nk)

    def run(f):
        MP.aggregate(rq, [whole_q(s) for s in parties], whole_q(dst), f)
        MP.aggregate(rp, [whole_p(s) for s in parties], whole_p(dst), f)
    r = ab(lambda: run(True), lambda: run(False), 3, 2, warm=1)
    total = nk * share_bytes
    r.update(op="5 parties' shares of %d Galois keys summed, Q and P" % nk, bytes_per_party=total,
             fused_GBps=round(6 * total / (r["fused"]["ms_median"] * 1e-3) / 1e9, 1), composed_GBps=round(12 * total / (r["composed"]["ms_median"] * 1e-3) / 1e9, 1))
    out["aggregate_five_parties"] = r

    wins = lambda rs: bool(all(x["fused"]["ms_median"] <= x["composed"]["ms_median"] for x in rs))
    # two shares are one Add either way (the same three passes): multiparty.aggregate takes the kernel from three shares on, whatever the flag
    out["aggregate_two_shares_kernel_wins"] = wins(agg[:1])
    out["fused_multiparty_default"] = {"aggregate": wins(agg[1:] + [r]), "gadget_share": wins([whole[0]]), "relin_rounds": wins(whole[1:3]),
                                       "keyswitch_share": wins(whole[3:])}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "multiparty.json"))

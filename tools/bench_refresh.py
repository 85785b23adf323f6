"""The collective refresh's share conversion on the device at N = 2^16: E2S at level 3, 25 output limbs, full slots (n = 2^16 values per
ciphertext), scale 2^45, masks of 173 bits.  Writes profiles/refresh.json.

  (a) the recode of Transform (coefficient-domain poly at level 3 -> Quo(x m, d) -> 25 limbs) and of GenShare's second half (a block of
      masks -> Quo -> 25 limbs): rh_mp_refresh_recode against rh_mp_big_from_rns + rh_mp_big_muldiv + rh_mp_big_to_rns;
  (b) RefreshProtocol.Finalize (Transform) and GenShare, whole calls, either way;
  (c) for the record, the host route of (a): the poly to numpy, Python integers per coefficient, residues back to the device.

Method: device events on the launch stream around windows of calls (1000 for the recode, 200 for the whole calls) after warm-up calls,
device-resident data, 3 alternating windows per side, the median reported with min and max.  The calls go through the Python layer, so a
figure is the time per call of a stream of calls, host work and launches included, not a kernel time; the composed recode's block is
allocated once, outside the windows (inside the whole calls it is allocated per call, as the protocols do).  A row decides for a side only where the two sides' windows do not overlap.  (c) is a host clock around one pass that ends in a synchronise.
Usage: python tools/bench_refresh.py [OUT.json]"""
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import matrix_fhe_lattigo_amd as rh
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


def ab(fused, composed, reps, rounds=3, warm=2):
    tf, tc = [], []
    for _ in range(rounds):
        tf.append(timed(fused, reps, warm)); tc.append(timed(composed, reps, warm))
    f, c = stat(tf), stat(tc)
    return {"fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 2)}


def main(out_path):
    N, level, logBound = 1 << 16, 3, 173
    Q, _ = primes.gen_moduli(17, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61])
    Q = [int(q) for q in Q]
    rq = rh.Ring(N, Q)
    rq.set_stream(stream.cuda_stream)
    top = len(Q) - 1
    rl, rt = rq.AtLevel(level), rq.AtLevel(top)
    prng = rh.rlwe.KeyedPRNG(b"bench refresh")
    kg = rh.rlwe.KeyGenerator(rq, None, prng=prng)
    sk = kg.GenSecretKeyNew()
    scale = rh.ckks.Scale(1 << 45)
    m, d = 1 << 45, (1 << 45) + 1                    # a divisor that is no power of two, as a ceiling of a non-integer scale gives
    out = {"device": torch.cuda.get_device_name(0),
           "shape": {"N": N, "level_in": level, "limbs_out": top + 1, "values_per_ciphertext": N, "logBound": logBound, "Q_in_bits": math.prod(Q[:level + 1]).bit_length()},
           "method": __doc__.split("Method: ")[1].split("Usage")[0].replace("\n", " ").strip()}

    # (a) the recode alone
    src = rl.NewPoly(1)
    kg.uniform.Read(src)
    dst = rt.NewPoly(1)
    mask = MP.AdditiveShareBigint(rq, N, 3)
    MP.big_sample(prng, mask, logBound)
    from matrix_fhe_lattigo_amd.multiparty_refresh import recode_words
    tmp_a, tmp_b = MP.AdditiveShareBigint(rq, N, recode_words(rl, m, d)), MP.AdditiveShareBigint(rq, N, mask.W)      # the composed side's blocks, made once
    ra = ab(lambda: MP.refresh_recode(rt, dst, m, d, N, src_poly=src, rl_in=rl, fused=True),
            lambda: MP.refresh_recode(rt, dst, m, d, N, src_poly=src, rl_in=rl, fused=False, scratch=tmp_a), 1000)
    ra.update(op="Transform's recode: poly at level %d -> Quo -> %d limbs; one kernel vs from-RNS + muldiv + to-RNS" % (level, top + 1))
    rb = ab(lambda: MP.refresh_recode(rt, dst, m, d, N, src_share=mask, fused=True),
            lambda: MP.refresh_recode(rt, dst, m, d, N, src_share=mask, fused=False, scratch=tmp_b), 1000)
    rb.update(op="GenShare's recode: a block of %d-bit masks -> Quo -> %d limbs; one kernel vs muldiv + to-RNS" % (logBound, top + 1))
    out["recode"] = [ra, rb]

    # (b) whole calls
    ct = rh.rlwe.Encryptor(rq, None, sk, prng=prng).EncryptZeroNew(level + 1, npoly=1)
    ct.Scale, ct.LogDimensions, ct.IsBatched = rh.ckks.Scale((1 << 45) + 0.5), 15, True
    rfp = MP.mpckks.RefreshProtocol(rq, scale, 3.2, prng=prng)
    crp = rfp.SampleCRP(top, MP.CRS(b"bench crs"))
    share = rfp.AllocateShare(level, top)
    res = rh.Ciphertext([rt.NewPoly(1), rt.NewPoly(1)], is_ntt=True)
    rg = ab(lambda: rfp.GenShare(sk, logBound, ct, crp, share, fused=True), lambda: rfp.GenShare(sk, logBound, ct, crp, share, fused=False), 200, warm=1)
    rg.update(op="RefreshProtocol.GenShare, whole call")
    rf_ = ab(lambda: rfp.Finalize(ct, crp, share, res, fused=True), lambda: rfp.Finalize(ct, crp, share, res, fused=False), 200, warm=1)
    rf_.update(op="RefreshProtocol.Finalize (Transform), whole call")
    out["whole_calls"] = [rg, rf_]

    # (c) the host route of Transform's recode, once
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = src.numpy()[0]
    mods = Q[:level + 1]
    Qin = math.prod(mods)
    parts = [(Qin // q) * pow(Qin // q, -1, q) for q in mods]
    host = np.zeros((1, top + 1, N), dtype=np.uint64)
    vals = []
    for i in range(N):
        v = sum(int(rows[k, i]) * parts[k] for k in range(level + 1)) % Qin
        v = v - Qin if v >= Qin // 2 else v
        p = v * m
        vals.append(-((-p) // d) if p < 0 else p // d)
    for k, q in enumerate(Q):
        host[0, k] = [v % q for v in vals]
    back = rh.DevicePoly.from_numpy(rt, host)
    torch.cuda.synchronize()
    out["host_route_recode_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    MP.refresh_recode(rt, dst, m, d, N, src_poly=src, rl_in=rl, fused=True)
    out["host_route_equals_device"] = bool(np.array_equal(back.numpy(), dst.numpy()))

    # a row decides only where the windows of its two sides do not overlap; the default is the kernel when a row decides for it and none against
    rows_ = (ra, rb, rg, rf_)
    for x in rows_:
        f, c = x["fused"], x["composed"]
        x["decides"] = "fused" if f["ms_max"] < c["ms_min"] else "composed" if c["ms_max"] < f["ms_min"] else "undecided"
    verdicts = [x["decides"] for x in rows_]
    out["fused_refresh_default"] = {"refresh_recode": bool("fused" in verdicts and "composed" not in verdicts)}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "refresh.json"))

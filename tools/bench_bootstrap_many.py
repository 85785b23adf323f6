"""BootstrapMany at N = 2^16, the 25 + 5-limb chain shape of profiles/bootstrap.json (10 residual limbs), bootstrapping LogSlots 15, real device
keys from Parameters.GenEvaluationKeys under a KeyedPRNG: writes profiles/bootstrap_many.json.

  (a) rh_ckks_bootstrap_pack and rh_ckks_bootstrap_unpack against the composed ring calls (MulCoeffsMontgomeryThenAdd per pair and level; CopyLvl
      + MulCoeffsMontgomery) on the same prepared rows at the residual level, g in 1, 3, 5 and n = G and G + 1 ciphertexts;
  (b) a whole BootstrapMany of 8 ciphertexts of LogSlots 12 at level 0, FUSED_BOOTSTRAP_MANY on and off, against the only way to bootstrap them
      without it: a bootstrapping.Evaluator built at LogSlots 12 given the batch of 8;
  (c) the same with the residual ring of degree N1 = 2^15 (pack to 2 in N1, switch, pack to 1 in N2, and back).

Every figure is a CALL RATE: device events around windows of back-to-back calls through the Python layer after two warm-up calls, the arms of
a comparison alternating window by window, five windows each ((a): 20 calls a window; (b), (c): 2), median with min and max.  None is a kernel
trace.  The ciphertexts hold uniform residues: the timings do not depend on the values.
Usage: python tools/bench_bootstrap_many.py [OUT.json]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import matrix_fhe_lattigo_amd as rh
from oracle import primes

stream = torch.cuda.current_stream()
LOGN, LS, RES = 16, 15, 9
LOGQ = [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4


def window(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def stat(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def compare(arms, reps, windows=5):
    """arms: {name: fn}; alternating windows"""
    for fn in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    got = {k: [] for k in arms}
    for _ in range(windows):
        for k, fn in arms.items():
            got[k].append(window(fn, reps))
    return {k: stat(v) for k, v in got.items()}


def parameters(rq, rp, log_slots, **kw):
    B, D, M = rh.bootstrapping, rh.dft, rh.mod1
    top, LP = len(LOGQ) - 1, rp.L
    s2c = D.MatrixLiteral(D.HomomorphicDecode, log_slots, RES + 3, LP - 1, [1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    c2s = D.MatrixLiteral(D.HomomorphicEncode, log_slots, top, LP - 1, [1, 1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    m1 = M.ParametersLiteral(LevelQ=RES + 11, LogScale=60, Mod1Type=M.CosDiscrete, LogMessageRatio=8 + min(max(15 - log_slots, 0), 8), K=16, Mod1Degree=30,
                             DoubleAngle=3)
    return B.Parameters(rq, rp, RES, 1 << 40, s2c, m1, c2s, EphemeralSecretWeight=32, BootstrappingSecretWeight=192, **kw)


def batch(us, n, log_slots):
    """n ciphertexts at the level of the sampler's ring view"""
    ct = rh.Ciphertext([us.ReadNew(n), us.ReadNew(n)], is_ntt=True)
    ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << 40), log_slots
    return ct


def main(out_path):
    N = 1 << LOGN
    Q, P = primes.gen_moduli(LOGN + 1, LOGQ, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    prng = rh.rlwe.KeyedPRNG(b"bench bootstrap many")
    B = rh.bootstrapping
    res = {"device": torch.cuda.get_device_name(0), "shape": {"N": N, "limbs_Q": len(Q), "limbs_P": len(P), "log_q": LOGQ, "residual_limbs": RES + 1,
                                                              "bootstrapping_log_slots": LS},
           "method": __doc__.split("\n\n")[2].replace("\n", " "), "kernels": [], "whole": []}

    # (a) the kernels against the composed calls, at the residual level
    rr = rq.AtLevel(RES)
    us = rh.rlwe.UniformSampler(prng, rr)
    xPow2, xPow2Inv = rh.rlwe.GenXPow2NTT(rr, LOGN, False), rh.rlwe.GenXPow2NTT(rr, LOGN, True)
    for g in (1, 3, 5):
        xp, xinv = B.pack_table(rr, xPow2, LOGN - 2, g), B.pack_table(rr, xPow2Inv, LOGN - 2, g)
        for n in (1 << g, (1 << g) + 1):
            m = -(-n >> g)
            ins = [us.ReadNew(n), us.ReadNew(n)]
            o1, o2 = [rr.NewPoly(m) for _ in (0, 1)], [rr.NewPoly(m) for _ in (0, 1)]
            u1, u2 = [rr.NewPoly(n) for _ in (0, 1)], [rr.NewPoly(n) for _ in (0, 1)]
            work = [rr.NewPoly(n) for _ in (0, 1)]                                 # the composed pack's copies of its inputs: allocated outside the windows
            r = compare({"kernel": lambda: B.bootstrap_pack(rr, g, ins, o1, xp), "composed": lambda: B.pack_composed(rr, g, ins, o2, xp, work)}, 20)
            same = bool(all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(o1, o2)))
            res["kernels"].append(dict(op="pack", g=g, n=n, same_words=same, rows_in=2 * n * (RES + 1), rows_out=2 * m * (RES + 1),
                                       ratio_composed_over_kernel=round(r["composed"]["ms_median"] / r["kernel"]["ms_median"], 3), **r))
            r = compare({"kernel": lambda: B.bootstrap_unpack(rr, g, n, o1, u1, xinv), "composed": lambda: B.unpack_composed(rr, g, n, o1, u2, xinv)}, 20)
            same = bool(all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(u1, u2)))
            res["kernels"].append(dict(op="unpack", g=g, n=n, same_words=same, rows_in=2 * m * (RES + 1), rows_out=2 * n * (RES + 1),
                                       ratio_composed_over_kernel=round(r["composed"]["ms_median"] / r["kernel"]["ms_median"], 3), **r))
            del ins, o1, o2, u1, u2, work

    # (b), (c) whole calls: 8 ciphertexts of LogSlots 12 at level 0
    base_params = parameters(rq, rp, 12)
    sk = rh.rlwe.KeyGenerator(rq, rp, xs=("H", 192), prng=prng).GenSecretKeyNew()
    base_keys, _ = base_params.GenEvaluationKeys(sk, prng=prng)
    base = B.Evaluator(base_params, base_keys)
    ct8 = batch(rh.rlwe.UniformSampler(prng, rq.AtLevel(0)), 8, 12)
    torch.cuda.synchronize()
    for name, n1 in (("N1 = N2 = 2^16", None), ("N1 = 2^15", 1 << 15)):
        kw = {}
        if n1 is None:
            sk1, cts = sk, ct8
        else:
            r1 = rh.Ring(n1, Q[:RES + 1])
            kw["ResidualRingQ"] = r1
            sk1 = rh.rlwe.KeyGenerator(r1, None, prng=prng).GenSecretKeyNew()
            cts = batch(rh.rlwe.UniformSampler(prng, r1.AtLevel(0)), 8, 12)
        params = parameters(rq, rp, LS, **kw)
        keys, _ = params.GenEvaluationKeys(sk1, prng=prng)
        bts = {f: B.Bootstrapper(params, keys, fused=f) for f in (True, False)}
        a, b = bts[True].BootstrapMany(cts), bts[False].BootstrapMany(cts)
        same = bool(all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a.Value, b.Value)))
        r = compare({"BootstrapMany_kernels": lambda: bts[True].BootstrapMany(cts), "BootstrapMany_composed": lambda: bts[False].BootstrapMany(cts),
                     "Evaluator_at_LogSlots_12_batch_8": lambda: base.Evaluate(ct8)}, 2)
        k, c, e = (r[x]["ms_median"] for x in ("BootstrapMany_kernels", "BootstrapMany_composed", "Evaluator_at_LogSlots_12_batch_8"))
        res["whole"].append(dict(arm=name, ciphertexts=8, log_slots=12, same_words=same, ms_per_ciphertext_kernels=round(k / 8, 3),
                                 ms_per_ciphertext_baseline=round(e / 8, 3), ratio_baseline_over_bootstrap_many=round(e / k, 3),
                                 ratio_composed_over_kernels=round(c / k, 3), kernels_never_slower=bool(k <= c), **r))
        for x in bts.values():
            x.close()
        del bts, keys
    res["fused_bootstrap_many_default"] = bool(all(w["kernels_never_slower"] for w in res["whole"]))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bootstrap_many.json"))

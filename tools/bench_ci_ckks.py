"""Conjugate-invariant CKKS at n = 2^16 (standard side 2^17), 25 + 5 limbs, real keys from a KeyedPRNG: writes profiles/ci_ckks.json.

  (a) the tail of ComplexToReal on prepared blocks: rh_ckks_bridge_fold_tail against the composed Add + two FoldStandardToConjugateInvariant
      calls, batches of 1 and 8;
  (b) whole DomainSwitcher.ComplexToReal and RealToComplex calls, fused and composed (FUSED_BRIDGE), batches of 1 and 8;
  (c) Encode and Decode at 2^16 real slots from / into device values, batches of 1 and 8 (beside the standard encoder's figures in
      profiles/ckks_encoder.json: the same entry points, one FFT size larger);
  (d) GenRelinearizationKeyNew on the conjugate-invariant ring.

Every figure is a CALL RATE: device events around windows of back-to-back calls through the Python layer after two warm-up calls, the two arms
of a comparison alternating window by window, five windows each, median with min and max; (d) is a host clock around whole calls that end in
a synchronise, three calls after one untimed.  None is a kernel trace.
Usage: python tools/bench_ci_ckks.py [OUT.json]"""
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
from oracle import primes

stream = torch.cuda.current_stream()


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


def main(out_path):
    logn = 16
    n = 1 << logn
    Q, P = primes.gen_moduli(logn + 2, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    pci = rh.ckks.Parameters(logn, Q, P, 40, RingType=rh.ConjugateInvariant)
    pstd = pci.StandardParameters()
    prng = rh.rlwe.KeyedPRNG(b"bench conjugate-invariant ckks")
    kgc, kgs = rh.ckks.NewKeyGenerator(pci, prng), rh.ckks.NewKeyGenerator(pstd, prng)
    sk, sk_std = kgc.GenSecretKeyNew(), kgs.GenSecretKeyNew()
    level = pci.MaxLevel()
    res = {"device": torch.cuda.get_device_name(0), "shape": {"n_conjugate_invariant": n, "N_standard": 2 * n, "limbs_Q": len(Q), "limbs_P": len(P)},
           "method": __doc__.split("\n\n")[2].replace("\n", " "), "fold_tail": [], "switch": [], "encoder": []}

    # (d) key generation
    kgc.GenRelinearizationKeyNew(sk)
    torch.cuda.synchronize()
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        kgc.GenRelinearizationKeyNew(sk)
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    res["GenRelinearizationKeyNew_conjugate_invariant"] = stat(t)

    t0 = time.perf_counter()
    k0, k1 = kgs.GenEvaluationKeysForRingSwapNew(sk_std, sk)
    torch.cuda.synchronize()
    res["GenEvaluationKeysForRingSwapNew_ms_once"] = round((time.perf_counter() - t0) * 1e3, 2)
    sw = rh.ckks.NewDomainSwitcher(pstd, k0, k1)
    ev = rh.ckks.NewEvaluator(pstd)
    rs, rc = sw.stdRingQ.AtLevel(level), sw.conjugateRingQ.AtLevel(level)
    us, uc = rh.rlwe.UniformSampler(prng, pstd.RingQ()), rh.rlwe.UniformSampler(prng, pci.RingQ(), conjugate_invariant=True)

    for B in (1, 8):
        # (a) the tail alone
        g0, g1, c0 = (us.ReadNew(B) for _ in range(3))
        t0_, o0, o1, p0, p1 = rs.NewPoly(B), rc.NewPoly(B), rc.NewPoly(B), rc.NewPoly(B), rc.NewPoly(B)

        def fused():
            rh.ringhip._check(rh.lib().rh_ckks_bridge_fold_tail(rc._h, level, g0.ptr, g1.ptr, c0.ptr, sw._index.ptr, o0.ptr, o1.ptr, B))

        def composed():
            rs.Add(g0, c0, t0_)
            rc.FoldStandardToConjugateInvariant(t0_, sw._index, p0)
            rc.FoldStandardToConjugateInvariant(g1, sw._index, p1)
        r = compare({"fused": fused, "composed": composed}, 50 if B == 1 else 20)
        same = bool(np.array_equal(o0.numpy(), p0.numpy()) and np.array_equal(o1.numpy(), p1.numpy()))
        res["fold_tail"].append(dict(batch=B, same_words=same, ratio_composed_over_fused=round(r["composed"]["ms_median"] / r["fused"]["ms_median"], 3), **r))
        # (b) whole switches
        cstd = rh.Ciphertext([us.ReadNew(B), us.ReadNew(B)], is_ntt=True)
        cci = rh.Ciphertext([uc.ReadNew(B), uc.ReadNew(B)], is_ntt=True)
        for c in (cstd, cci):
            c.Scale, c.LogDimensions, c.IsBatched = pci.DefaultScale(), logn, True
        ostd = rh.ckks.NewCiphertext(pstd, 1, level, B)
        oci = rh.ckks.NewCiphertext(pci, 1, level, B)
        for name, fn in (("ComplexToReal", lambda f: sw.ComplexToReal(ev, cstd, oci, fused=f)), ("RealToComplex", lambda f: sw.RealToComplex(ev, cci, ostd, fused=f))):
            r = compare({"fused": lambda: fn(True), "composed": lambda: fn(False)}, 10 if B == 1 else 4)
            res["switch"].append(dict(op=name, batch=B, ratio_composed_over_fused=round(r["composed"]["ms_median"] / r["fused"]["ms_median"], 3), **r))
        del g0, g1, c0, t0_, o0, o1, p0, p1, cstd, cci, ostd, oci

    # (c) the real-only encoder at n slots
    enc = rh.ckks.NewEncoder(pci)
    rng = np.random.default_rng(1)
    for B in (1, 8):
        enc.reserve(B)
        vals = rh.ckks.DeviceValues.from_numpy(pci.RingQ(), (rng.uniform(-1, 1, (B, n)) + 0j))
        out = rh.ckks.DeviceValues(pci.RingQ(), B, n, True)
        pt = rh.ckks.NewPlaintext(pci, level, B)
        r = compare({"Encode": lambda: enc.Encode(vals, pt), "Decode": lambda: enc.Decode(pt, out)}, 20 if B == 1 else 5)
        err = float(np.max(np.abs(out.numpy().real - vals.numpy().real)))
        res["encoder"].append(dict(batch=B, slots=n, level=level, round_trip_max_error=err, **r))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "ci_ckks.json"))

"""The BGV polynomial evaluator's switch, bgv_polynomial.FUSED_BGV_POLYNOMIAL, at N = 2^15 and 2^16, 8 + 2 limbs (LogQ {60, 50 x 7},
LogP {61, 61}, T = 65537, standard tensoring), batches of 1 and 8 ciphertexts, under real keys made on the device: writes
profiles/bgv_polynomial.json.

  (a) Evaluate end to end (power basis, baby steps, giant steps, the last rescale) of a dense degree-31 polynomial ("scalar": the baby steps
      are rh_ckks_linear_combination launches) and of a degree-15 PolynomialVector of two polynomials mapped to interleaved slots ("vector":
      rh_bgv_plain_combination launches after ONE batched Embed per baby step);
  (b) the baby steps alone -- every EvaluateBabyStep of the same two decompositions on a power basis built once.

The composed side issues the reference's own Add and MulThenAdd calls through bgv.Evaluator: entries that exist without this module, timed HERE,
alternating with the fused side.  An arm's default follows (a), the whole calls it decides: fused only where at EVERY shape its median is below
the composed median by more than the run-to-run spread (the larger of the two sides' max - min over the windows); otherwise composed.

Method: device events around windows of calls after warm-up calls, 5 alternating windows per side, the median reported with min and max; both
sides give the same bits at the shape that is timed (asserted).  Usage: python tools/bench_bgv_polynomial.py [OUT.json]"""
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import matrix_fhe_lattigo_amd as rh
from oracle import primes

stream = torch.cuda.current_stream()
ROUNDS = 5
T = 65537


def timed(fn, reps, warm=1):
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


def same_bits(a, b):
    return a.Level() == b.Level() and a.Scale == b.Scale and all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a.Value, b.Value))


def main(out_path):
    Bp = rh.bgv_polynomial
    rnd = random.Random("bench bgv polynomial")
    results = []

    def record(part, arm, name, logN, B, fn, reps, decides):
        """fn(fused) runs one call and returns its result"""
        assert same_bits(fn(True), fn(False)), "fused and composed differ: %s, N = 2^%d, batch %d" % (name, logN, B)
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(timed(lambda: fn(True), reps)); tc.append(timed(lambda: fn(False), reps))
        f, c = stat(tf), stat(tc)
        spread = round(max(c["ms_max"] - c["ms_min"], f["ms_max"] - f["ms_min"]), 4)
        e = {"part": part, "arm": arm, "op": name, "logN": logN, "batch": B, "decides": decides, "fused": f, "composed": c,
             "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3), "run_to_run_spread_ms": spread,
             "fused_faster_beyond_spread": bool(c["ms_median"] - f["ms_median"] > spread), "windows": ROUNDS, "calls_per_window": reps}
        results.append(e)
        print(json.dumps(e), flush=True)

    shape = {}
    for logN in (15, 16):
        N = 1 << logN
        Q, P = primes.gen_moduli(logN + 1, [60] + [50] * 7, [61, 61])
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        shape = {"limbs_Q": len(Q), "limbs_P": len(P), "T": T}
        rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
        rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
        prng = rh.rlwe.KeyedPRNG(b"bench bgv polynomial")
        kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
        sk = kg.GenSecretKeyNew()
        enc = rh.bgv.Encoder(rq, T)
        ev = rh.bgv.Evaluator(rq, None, T, ringP=rp, rlk=kg.GenRelinearizationKeyNew(sk), encoder=enc)
        slots = enc.MaxSlots()
        scalar = Bp.Polynomial([rnd.randrange(1, T) for _ in range(32)])
        vector = Bp.PolynomialVector([[rnd.randrange(1, T) for _ in range(16)] for _ in range(2)], {0: list(range(0, slots, 2)), 1: list(range(1, slots, 2))})
        pes = {f: Bp.Evaluator(ev, fused=f) for f in (True, False)}
        for B in (1, 8):
            values = np.random.default_rng(B).integers(0, T, (B, slots), dtype=np.uint64)
            pt = enc.NewPlaintext(len(Q) - 1, scale=1, nvec=B)
            enc.Encode(values, pt)
            ct = rh.bgv.Encryptor(rq, None, sk, prng=prng).EncryptNew(pt)
            ct.Scale, ct.IsBatched = 1, True
            for arm, pol, name in (("scalar", scalar, "degree 31, one polynomial"), ("vector", vector, "degree 15, two polynomials on interleaved slots")):
                out = pes[True].Evaluate(ct, pol, 1)                     # the result is the polynomial, slot by slot, before anything is timed
                got = np.asarray(enc.Decode(rh.bgv.Decryptor(rq, sk).DecryptNew(out)))
                polys = [pol] if arm == "scalar" else pol.Value
                for i, p in enumerate(polys):
                    idx = list(range(slots))[:64] if arm == "scalar" else pol.Mapping[i][:64]
                    assert all(int(got[0, j]) == p.Evaluate(int(values[0, j]), T) for j in idx), "wrong result: %s" % name
                record("a", arm, "Evaluate: " + name, logN, B, lambda f, pol=pol: pes[f].Evaluate(ct, pol, 1), 8, arm)
                # ---- (b) the baby steps alone, on a power basis built once
                pb = Bp.PowerBasis(ct)
                polyVec = pes[True]._poly_vector(pol)
                logDegree = polyVec.Value[0].Degree().bit_length()
                pb.GenPower(1 << (logDegree - 1), False, ev)
                for i in range((1 << Bp.OptimalSplit(logDegree)) - 1, 2, -1):
                    pb.GenPower(i, False, ev)
                PS = polyVec.PatersonStockmeyerPolynomial(pes[True]._sim(), ct.Level(), 1, 1)
                steps = len(PS.Value[0].Value)

                def baby(f, PS=PS, pb=pb, steps=steps):
                    return [pes[f].EvaluateBabyStep(i, PS, pb).Value for i in range(steps)][-1]
                record("b", arm, "the %d baby steps alone: %s" % (steps, name), logN, B, baby, 16, None)
                del pb
                torch.cuda.empty_cache()
            del ct, pt
            torch.cuda.empty_cache()
        ev.close(); enc.close(); rq.close(); rp.close()
    from bench import csrc_tree_hash
    defaults = {arm: bool(all(e["fused_faster_beyond_spread"] for e in results if e["decides"] == arm)) for arm in ("scalar", "vector")}
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": dict(shape, logN=[15, 16], batches=[1, 8]),
           "method": __doc__.split("Method: ")[1].split("  Usage")[0].replace("\n", " "),
           "rule": "an arm is fused by default only where, at every shape of part (a), the fused median is below the composed median by more than the run-to-run spread",
           "fused_bgv_polynomial_default": defaults, "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"fused_bgv_polynomial_default": defaults}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgv_polynomial.json"))

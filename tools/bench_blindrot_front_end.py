"""A whole blindrot.Evaluator.Evaluate with the host front end (mod switch, programs and monomials in Python, what the commit before the device
front end runs) against the device one (rh_blindrot_mod_switch, rh_blindrot_program, rh_blindrot_monomials), at the shape of profiles/blindrot.json:
N_BR = 2^10, Q = 0x7fff801, N_LWE = 2^9, pw2 = 7, 512 RGSW keys and 11 automorphism keys of uniformly random words (timing needs no encryption),
sample ciphertexts of uniformly random residues in the NTT domain.  16, 64 and 256 accumulators from one and from four sample ciphertexts.

Host wall clock, the device drained before and after each window; every figure is the best of WINDOWS windows, with the spread (max - min) / min of
the windows next to it.  `back_end_ms` is everything Evaluate does after the front end (transform of the monomials, product, first automorphism,
the accumulator kernel), timed on device-resident programs; the front end's share of a path is 1 - back_end_ms / its whole time.

  python tools/bench_blindrot_front_end.py [OUT.json]        writes profiles/blindrot_front_end.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (first: one HIP runtime per process)
import matrix_fhe_lattigo_amd as rh  # noqa: E402

WINDOWS = 5


def _windows(fn, sync, reps):
    """best wall-clock ms per call over WINDOWS windows of `reps` calls, and the windows' spread"""
    fn()
    sync()
    t = []
    for _ in range(WINDOWS):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        t.append((time.perf_counter() - t0) * 1e3 / reps)
    return min(t), (max(t) - min(t)) / min(t)


def _random_gadget(rng, rq, q, N, rows, pw2):
    return rh.rlwe.GadgetCiphertext(rq, None, rng.integers(0, q, size=(rows, 2, 1, N), dtype=np.uint64), None, BaseTwoDecomposition=pw2, digits_per_limb=[rows])


def keygen_group():
    """blindrot.GenEvaluationKeyNew on the device -- N_LWE RGSW ciphertexts in one launch sequence and eleven Galois keys -- with rh_rgsw_encrypt and
    rh_rlwe_gadget_encrypt against the composed ring calls (fused=False: the same samplers, lifts and transforms, three ring calls per row and limb
    set), at N_BR = 2^10 and 2^11; and the RGSW rows alone.  The numpy restatement of the key set (tests/lut_restatement.py, Python loops over the
    oracle) is not timed here: it takes minutes at these shapes and is test infrastructure, not a path of the package."""
    out = []
    for N, q, NL in ((1024, 0x7fff801, 512), (2048, 0x7ff6001, 512)):
        rq, rl = rh.Ring(N, [q]), rh.Ring(NL, [0x3001])
        prng = rh.rlwe.KeyedPRNG(b"bench blind rotation keys")
        kg = rh.rlwe.KeyGenerator(rq, prng=prng)
        sk, sk_lwe = kg.GenSecretKeyNew(), rh.rlwe.KeyGenerator(rl, prng=prng).GenSecretKeyNew()
        sync = rq.sync
        e = {"N_BR": N, "N_LWE": NL, "pw2": 7, "rgsw_rows": NL * 2 * 4}
        for name, fused in (("kernel", True), ("composed", False)):
            ms, sp = _windows(lambda: rh.blindrot.GenEvaluationKeyNew(kg, sk, rl, sk_lwe, BaseTwoDecomposition=7, fused=fused), sync, 1)
            e[name + "_keyset_ms"], e[name + "_spread"] = round(ms, 3), round(sp, 3)
        enc = rh.rgsw.Encryptor(rq, None, sk, prng=prng)
        pt = rq.NewPoly(3)
        rq.vec_op("ZERO", None, None, pt)
        idx = [k % 3 for k in range(NL)]
        for name, fused in (("kernel", True), ("composed", False)):
            ms, sp = _windows(lambda: enc.rows(pt, idx, 0, -1, 7, fused=fused), sync, 1)
            e[name + "_rgsw_rows_ms"], e[name + "_rgsw_rows_spread"] = round(ms, 3), round(sp, 3)
        e["kernel_over_composed_keyset"] = round(e["composed_keyset_ms"] / e["kernel_keyset_ms"], 2)
        out.append(e)
        print(json.dumps(e), flush=True)
        rq.close(); rl.close()
    return out


def main(out_path):
    N, q, NL, ql, pw2, rows = 1024, 0x7fff801, 512, 0x3001, 7, 4
    rng = np.random.default_rng(3)
    rq, rl = rh.Ring(N, [q]), rh.Ring(NL, [ql])
    ev = rh.blindrot.Evaluator(rq, rl)
    BRK = rh.blindrot.MemBlindRotationEvaluationKeySet(
        [rh.rgsw.Ciphertext(_random_gadget(rng, rq, q, N, rows, pw2), _random_gadget(rng, rq, q, N, rows, pw2)) for _ in range(NL)],
        {g: _random_gadget(rng, rq, q, N, rows, pw2) for g in rh.blindrot.GaloisElements(N)})
    F = rh.blindrot.InitTestPolynomial(lambda x: 1.0 if x > 0 else -1.0, float(q) / 4.0, rq, -1, 1)
    sync = lambda: (rl.sync(), rq.sync())
    results = []
    for ncts in (1, 4):
        cts = [rh.Ciphertext([rh.DevicePoly.from_numpy(rl, rng.integers(0, ql, size=(1, 1, NL), dtype=np.uint64)) for _ in (0, 1)], is_ntt=True)
               for _ in range(ncts)]
        for accs in (16, 64, 256):
            polys = {i: F for i in range(accs // ncts)}
            r0 = rq.AtLevel(0)
            a2n, b, jobs, jd = ev._samples_device(cts, polys.keys())
            off, ops = ev._program_device(a2n, ncts, jd, len(jobs), BRK.device_tables(rq)[2])

            def back_end():
                acc = rh.Ciphertext([r0.NewPoly(len(jobs)), r0.NewPoly(len(jobs))], is_ntt=True)
                rh.lib().rh_blindrot_monomials(r0._h, 0, b.ptr, len(jobs), acc.Value[1].ptr)
                ev._accumulators(r0, acc, [F] * len(jobs))
                ev._launch_core(off.ptr, ops.ptr, ops.size, len(jobs), acc, BRK)
                r0.sync()
            back, back_sp = _windows(back_end, sync, 2)
            dev, dev_sp = _windows(lambda: ev.Evaluate(cts, polys, BRK, front_end=True), sync, 2)
            host, host_sp = _windows(lambda: ev.Evaluate(cts, polys, BRK, front_end=False), sync, 1)
            results.append({"sample_ciphertexts": ncts, "accumulators": accs, "back_end_ms": round(back, 3), "back_end_spread": round(back_sp, 3),
                            "host_front_end_evaluate_ms": round(host, 3), "host_spread": round(host_sp, 3),
                            "host_front_end_share": round(1 - back / host, 3),
                            "device_front_end_evaluate_ms": round(dev, 3), "device_spread": round(dev_sp, 3),
                            "device_front_end_share": round(max(0.0, 1 - back / dev), 3),
                            "device_accumulators_per_s": round(accs / (dev * 1e-3), 1), "host_accumulators_per_s": round(accs / (host * 1e-3), 1),
                            "device_over_host": round(host / dev, 2)})
            print(json.dumps(results[-1]), flush=True)
    keygen = keygen_group()
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(),
           "shape": {"N_BR": N, "Q_BR": hex(q), "N_LWE": NL, "Q_LWE": hex(ql), "pw2": pw2, "digits": rows, "rgsw_keys": NL, "automorphism_keys": 11},
           "method": "host wall clock around a whole Evaluate, device drained before and after every window; best of %d windows (2 calls each for the "
                     "device front end and the back end, 1 call for the host front end) after one warm-up call; spread = (max - min) / min of the "
                     "windows; clocks left to the driver's default governor" % WINDOWS,
           "front_end_default": bool(all(e["device_front_end_evaluate_ms"] <= e["host_front_end_evaluate_ms"] * (1 + e["host_spread"]) for e in results)),
           "results": results, "keygen": keygen,
           "rgsw_encrypt_default": bool(all(e["kernel_keyset_ms"] <= e["composed_keyset_ms"] * (1 + e["composed_spread"]) for e in keygen))}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    ev.close(); rq.close(); rl.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "blindrot_front_end.json"))

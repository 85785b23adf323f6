"""The minimax circuits' three switches at N = 2^16, 25 + 5 limbs (LogQ {60, 55 x 24}, LogP {61 x 5}, scale 2^55, one level per rescaling),
batches of 1 and 8 ciphertexts, under real keys made on the device: writes profiles/minimax.json.  The scale is 2^55 and not the 2^45 of the
test set-up because the fixture composite multiplies the error of its input by about 2^3.5 per polynomial before its last two polynomials
contract it: at N = 2^16 and 2^45 the error before them reaches 2^-0.8 (measured), one draw decrypts to within 2^-26.7 of the sign and another
flips a slot.  The timings do not depend on the scale; the chain is a benchmark shape, wider than a 128-bit secure one at this N.

  (a) the step after a product of a Chebyshev power basis on prepared rows: one rh_ckks_axpby against the composed calls (Add(X, X, X), then
      Add(X, -1, X), or the scale-matching Sub(X, T_c, X) with T_c at X's level and one level above, where the composed path copies it down);
  (b) a whole Chebyshev PowerBasis.GenPower(31), polynomial.FUSED_POWER_BASIS["chebyshev_step"] on and off;
  (c) res + Conjugate(res), minimax.FUSED_MINIMAX["conjugate_add"] on and off; constant - x, FUSED_MINIMAX["affine"] on and off;
  (d) one comparison.Evaluator.Sign with the fixture polynomial (tests/golden/minimax_default_sign.json, 40 levels: the secret-key
      bootstrapper fires), every switch on against every switch off, and its largest error on the slots with |x| >= 2^-4.

The composed side is the parent commit's code and is timed HERE, alternating with the fused side.  A switch's default follows the whole calls
it decides ((b) for chebyshev_step, (c) for the other two): on only where no batch finds it slower than composed beyond the composed windows'
run-to-run spread, the rule of tools/bench_ops.py (ckks_group).

Method: device events around windows of calls after warm-up calls, 5 alternating windows per side, the median reported with min and max; both
sides give the same bits at the shape that is timed (asserted, except Sign, whose bootstrapper draws fresh randomness).  A window of (a), (b)
or (c) repeats one call on the same blocks, so the evaluator's memo of host scalars is warm on both sides.  Usage: python tools/bench_minimax.py [OUT.json]"""
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

dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
ROUNDS = 5


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


def rand_block(B, mods, N):
    qs = torch.tensor(mods, dtype=torch.int64, device=dev).view(1, len(mods), 1)
    return torch.randint(0, 1 << 62, (B, len(mods), N), dtype=torch.int64, device=dev) % qs


def same_bits(a, b):
    return a.Level() == b.Level() and a.Scale.Value == b.Scale.Value and all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a.Value, b.Value))


def main(out_path):
    Pm, Mm, Sc = rh.polynomial, rh.minimax, rh.ckks.Scale
    N, logN = 1 << 16, 16
    Q, P = primes.gen_moduli(logN + 1, [60] + [55] * 24, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    LQ, LP, top = len(Q), len(P), len(Q) - 1
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    prng = rh.rlwe.KeyedPRNG(b"bench minimax")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = kg.GenSecretKeyNew()
    evs = rh.rlwe.MemEvaluationKeySet(kg.GenRelinearizationKeyNew(sk), kg.GenGaloisKeysNew([2 * N - 1], sk))
    ecd = rh.ckks.Encoder(rq)
    ev = rh.ckks.Evaluator(rq, rp, rlk=evs.RelinearizationKey, galois_keys=evs.GaloisKeys, encoder=ecd)
    default_scale = 2 ** 55
    results = []

    def random_ct(B, level, scale):
        ct = rh.Ciphertext([rh.DevicePoly.from_torch(rq.AtLevel(level), rand_block(B, Q[:level + 1], N)) for _ in range(2)], is_ntt=True)
        ct.Scale, ct.LogDimensions = Sc(scale), logN - 1
        return ct

    def record(part, name, B, fn, reps, check=None, warm=2, decides=None, extra=None):
        """fn(fused) runs one call; check() -> whether both sides gave the same bits at this shape"""
        if check is not None:
            assert check(), "fused and composed differ: %s, batch %d" % (name, B)
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(timed(lambda: fn(True), reps, warm)); tc.append(timed(lambda: fn(False), reps, warm))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        e = {"part": part, "op": name, "batch": B, "decides": decides, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
             "composed_run_to_run_spread_ms": spread, "fused_not_slower_beyond_spread": bool(f["ms_median"] <= c["ms_median"] + spread),
             "windows": ROUNDS, "calls_per_window": reps}
        e.update(extra or {})
        results.append(e)
        print(json.dumps(e), flush=True)

    for B in (1, 8):
        # ---- (a) the step alone, on prepared rows: X = the product not yet rescaled (scale 2^110), T_c rescaled (scale 2^55)
        for name, level, c_level in (("2 X - 1", top, None), ("2 X - k T_c, T_c at X's level", top - 1, top - 1), ("2 X - k T_c, T_c one level above X", top - 1, top)):
            c = 0 if c_level is None else 1
            first = random_ct(B, level, default_scale * default_scale)
            Tc = random_ct(B, c_level, default_scale) if c else None
            scale0 = first.Scale

            def step(fused, xn, c=c, Tc=Tc, scale0=scale0):
                xn.Scale = scale0                                       # every call starts from the product's scale
                pb = Pm.PowerBasis.__new__(Pm.PowerBasis)
                pb.Basis, pb.fused, pb.Value = Pm.Chebyshev, fused, ({2: xn, 1: Tc} if c else {2: xn})
                if fused:
                    assert pb._chebyshev_step(2, c, False, ev)
                    return
                ev.Add(xn, xn, xn)                                      # PowerBasis._gen's composed arm, the parent commit's code
                if c == 0:
                    ev.Add(xn, -1, xn)
                else:
                    ev.Sub(xn, Pm._at_level(ev, Tc, xn.Level()), xn)

            def check(first=first, step=step):
                a, b = Pm._copy_new(first), Pm._copy_new(first)
                step(True, a); step(False, b)
                return same_bits(a, b)
            rows = 8.0 * N * (level + 1) * B * 2                        # one row of every limb, both components
            record("a", "Chebyshev step on prepared rows: " + name, B, lambda f, first=first, step=step: step(f, first), 20, check,
                   extra={"rows_read_written_fused": [2 if c else 1, 1], "bytes_per_row_set": rows})
            del first, Tc
            torch.cuda.empty_cache()
        # ---- (b) a whole GenPower(31)
        ct = random_ct(B, top, default_scale)

        def gen_power(fused, ct=ct):
            pb = Pm.PowerBasis(ct, Pm.Chebyshev, fused=fused)
            pb.GenPower(31, False, ev)
            return pb.Value[31]
        record("b", "PowerBasis.GenPower(31), Chebyshev", B, gen_power, 3 if B == 1 else 2, lambda: same_bits(gen_power(True), gen_power(False)), warm=1,
               decides="chebyshev_step")
        torch.cuda.empty_cache()
        # ---- (c) res + Conjugate(res), constant - x
        mms = {f: Mm.Evaluator(ev, None, default_scale, fused=f) for f in (True, False)}

        def check_conj(ct=ct):
            a, b = Pm._copy_new(ct), Pm._copy_new(ct)
            mms[True]._add_conjugate(a); mms[False]._add_conjugate(b)
            return same_bits(a, b)
        record("c", "res + Conjugate(res)", B, lambda f, ct=ct: mms[f]._add_conjugate(ct), 10, check_conj, decides="conjugate_add")
        record("c", "1 - x, in place", B, lambda f, ct=ct: Pm.affine_minus(ev, ct, 1, f, ct), 20,
               lambda ct=ct: same_bits(Pm.affine_minus(ev, ct, 1, True), Pm.affine_minus(ev, ct, 1, False)), decides="affine")
        del ct
        torch.cuda.empty_cache()
        # ---- (d) Sign with the fixture polynomial, every switch on against every switch off
        btp = rh.bootstrapping.SecretKeyBootstrapper(rq, sk, ecd, default_scale, prng=prng)
        poly = Mm.Polynomial.from_json(os.path.join(ROOT, "tests", "golden", "minimax_default_sign.json"), [Mm.CoeffsSignX4Cheby])
        cmps = {f: rh.comparison.Evaluator(Mm.Evaluator(ev, btp, default_scale, fused=f), poly) for f in (True, False)}
        x = np.random.default_rng(21).uniform(-1, 1, (B, N // 2))
        pt = ecd.NewPlaintext(top, default_scale, nvec=B)
        ecd.Encode(x + 0j, pt)
        ct = rh.ckks.Encryptor(rq, None, sk, prng=prng).EncryptNew(pt)
        was = Pm.FUSED_POWER_BASIS["chebyshev_step"]

        def sign(fused, ct=ct):
            Pm.FUSED_POWER_BASIS["chebyshev_step"] = fused
            try:
                return cmps[fused].Sign(ct)
            finally:
                Pm.FUSED_POWER_BASIS["chebyshev_step"] = was
        worst = {}
        for f in (True, False):
            before = btp.Counter
            got = np.asarray(ecd.Decode(rh.ckks.Decryptor(rq, sk).DecryptNew(sign(f)))).reshape(B, -1).real
            worst[f] = float(np.log2(np.max(np.abs(got - np.sign(x))[np.abs(x) >= 2.0 ** -4])))
            boots = btp.Counter - before
        record("d", "comparison.Sign, the fixture polynomial (9 polynomials, 40 levels)", B, sign, 1, None, warm=1,
               extra={"bootstrappings_per_call": boots, "log2_largest_error_fused": round(worst[True], 2), "log2_largest_error_composed": round(worst[False], 2)})
        results[-1].update({side + "_ms_per_ciphertext": round(results[-1][side]["ms_median"] / B, 3) for side in ("fused", "composed")})
        del ct, pt
        torch.cuda.empty_cache()
    from bench import csrc_tree_hash
    defaults = {k: bool(all(e["fused_not_slower_beyond_spread"] for e in results if e["decides"] == k)) for k in ("chebyshev_step", "affine", "conjugate_add")}
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batches": [1, 8], "scale_log2": 55},
           "method": __doc__.split("Method: ")[1].split("  Usage")[0].replace("\n", " "),
           "fused_power_basis_default": {"chebyshev_step": defaults["chebyshev_step"]},
           "fused_minimax_default": {"affine": defaults["affine"], "conjugate_add": defaults["conjugate_add"]}, "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    ev.close(); ecd.close(); rq.close(); rp.close()


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "minimax.json"))

#!/usr/bin/env python3
"""Secondary measurements (not the headline metric): inverse NTT, element-wise kernels, basis extension and the 3N
transform at the BASELINE config sizes, each against its algorithmic bytes.  Prints one JSON object.
`bench_ops.py bfv [OUT.json]` runs the BFV group alone (quantize composed vs fused, the whole scale-invariant multiply) and writes
profiles/bfv_ops.json (or OUT.json); `bench_ops.py bgv [OUT.json]` the BGV group (standard tensoring and multiply-accumulate, one kernel each
against the reference's sequence of ring calls) and writes profiles/bgv_ops.json; `bench_ops.py ckks [OUT.json]` the CKKS group
(MulThenAdd, MulRelinThenAdd, scale-matched Add and scalar Mul at the config 5 ring, fused against composed) and writes profiles/ckks_ops.json;
`bench_ops.py ckks_encoder [OUT.json]` the CKKS encoder (Encode, Decode and the two transforms at N = 2^16, 24 limbs, full slots, 64 vectors)
against its algorithmic bytes, and writes profiles/ckks_encoder.json; `bench_ops.py bgv_encoder [OUT.json]` the BGV encoder (Encode, Decode,
the lift and Q to T alone, one kernel each against the reference's sequence of ring calls, at N = 2^16, 24 limbs, 64 vectors, T = 65537 for
gap 2 and T = 786433 for gap 1) and writes profiles/bgv_encoder.json; `bench_ops.py inner_sum [OUT.json]` the sums of rotations
(PartialTracesSum for n = 7 and n = 8 at the config 5 ring, fused against composed, and each of the two kernels of csrc/inner_sum.hip against the
passes it replaces) and writes profiles/inner_sum.json; `bench_ops.py ring_packing [OUT.json]` the ring-packing evaluator (Expand, Pack, Split, Merge at the
config 5 ring and at N = 2^12, fused against composed, batched against per-ciphertext) and writes profiles/ring_packing.json;
`bench_ops.py polynomial [OUT.json]` the polynomial evaluator (the baby step and the whole Evaluate at N = 2^16, 16 limbs, batches of 1 and 64,
K = 7, 15, 31: rh_ckks_linear_combination against the composed sequence of MulThenAdd calls) and writes profiles/ckks_polynomial.json;
`bench_ops.py lintrans [OUT.json]` the linear transformations (lintrans.Evaluator.Evaluate at the config 5 ring, batches of 1 and 8: the reference
test's nine diagonals with and without BSGS and a dense 64-diagonal matrix, each kernel of csrc/lintrans.hip alone against the ring calls it
replaces and inside the whole Evaluate) and writes profiles/lintrans.json; `bench_ops.py dft [OUT.json]` the homomorphic DFT (matrix generation and encoding on the
device against host diagonals through the per-diagonal Encode, the real / imaginary split and merge kernels alone and inside CoeffsToSlots /
SlotsToCoeffs at the config 5 ring, LogSlots 15, batches of 1 and 8) and writes profiles/dft.json; `bench_ops.py blindrot [OUT.json [BASELINE.json]]` the blind rotation's
accumulator loop at the reference test's parameters (N = 2^10 / 2^9, Q = 0x7fff801, pw2 = 7) with 16, 64 and 256 accumulators, the kernel against
the composed calls, and writes profiles/blindrot.json; `bench_ops.py bootstrap [OUT.json]` CKKS bootstrapping at the N16QP1546H192H32 chain shape (N = 2^16, 25 + 5
limbs, LogSlots 15, batches of 1 and 8: the ModUp kernel alone against its write volume, EvalMod alone, the whole Evaluate split by stage, FUSED_BOOTSTRAP
on and off) and writes profiles/bootstrap.json; `bench_ops.py blindrot_baseline [OUT.json]` one ExternalProduct and one key-switched
automorphism at npoly = 1 through calls that predate the kernel (run it on the parent commit: BASELINE.json above)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import matrix_fhe_lattigo_amd as rh
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import QI60, PI60

dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream()
PEAK = 8000.0


def timed(fn, reps=10, warm=2):
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


def rand_block(B, mods, N):
    qs = torch.tensor(mods, dtype=torch.int64, device=dev).view(1, len(mods), 1)
    return torch.randint(0, 1 << 62, (B, len(mods), N), dtype=torch.int64, device=dev) % qs


def entry(name, ms, alg_bytes, units, unit_name):
    gbs = alg_bytes / (ms * 1e-3) / 1e9
    return {"op": name, "ms": round(ms, 4), unit_name + "_per_s": units / (ms * 1e-3), "algorithmic_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / PEAK, 3)}


def bfv_group(out_path):
    """N = 2^15, 8 limbs of Q (GenModuli [55] + [45]*7: 7 limbs of QMul, the register variant of the fused quantize), batch 64.
    (a) quantize through the three existing entry points, (b) rh_bfv_quantize (fused kernel), (c) the whole multiply.  (a) uses only entry
    points the library had before the BFV ones and is timed HERE, in the same process as (b) and alternating with it, not in a run of an older
    build: the two then see the same machine state (the extension kernels it launches compute what they did before); every figure is the median of `rounds` windows of `reps` calls, with the windows' min and max as the spread."""
    import statistics
    from oracle import primes
    logN, B, rounds, reps = 15, 64, 7, 20
    N = 1 << logN
    Q, M = primes.gen_moduli(logN + 1, [55] + [45] * 7, [61] * 8)
    ring_bits = 1
    for q in Q:
        ring_bits *= q
    M = M[:-(-(ring_bits.bit_length() + logN) // 61)]
    LQ, LM, T = len(Q), len(M), 65537
    rq, rm = rh.Ring(N, Q), rh.Ring(N, M); rq.set_stream(stream.cuda_stream); rm.set_stream(stream.cuda_stream)
    ev = rh.bgv.Evaluator(rq, rm, T); ev.reserve(B)
    be = rh.BasisExtender(rq, rm)
    assert ev.QuantizePath(LQ - 1) == "composed" and ev.levelQMul[LQ - 1] == LM - 1      # the default; "fused_quantize" = 1 selects the kernel
    xq, xm = rand_block(B, Q, N), rand_block(B, M, N)
    pq, pm = rh.DevicePoly.from_torch(rq, xq), rh.DevicePoly.from_torch(rm, xm)
    tq, tm, oq = (rh.DevicePoly.from_torch(rq, torch.empty_like(xq)), rh.DevicePoly.from_torch(rm, torch.empty_like(xm)),
                  rh.DevicePoly.from_torch(rq, torch.empty_like(xq)))

    def composed():                                   # quantize (schemes/bgv/evaluator.go:1104-1124) call by call, public API of the parent commit
        rq.INTTLazy(pq, tq); rm.INTTLazy(pm, tm)
        be.ModDownQPtoP(LQ - 1, LM - 1, tq, tm, tm)
        be.ModUpPtoQ(LM - 1, LQ - 1, tm, tq)
        rq.MulScalar(tq, T, tq)
        rq.NTT(tq, oq)

    def fused():
        ev.Quantize(LQ - 1, pq, pm, oq)
    composed(); ref = oq.numpy().copy(); fused()
    assert np.array_equal(ref, oq.numpy()), "composed path inside rh_bfv_quantize differs from the call-by-call sequence"
    ev.set_tuning("fused_quantize", 1); fused()
    assert ev.QuantizePath(LQ - 1) == "fused" and np.array_equal(ref, oq.numpy()), "fused quantize differs from the composed sequence"
    ta, tb, tinner = [], [], []
    for _ in range(rounds):
        ta.append(timed(composed, reps=reps)); tb.append(timed(fused, reps=reps))
        ev.set_tuning("fused_quantize", 0); tinner.append(timed(fused, reps=reps)); ev.set_tuning("fused_quantize", 1)
    ev.set_tuning("fused_quantize", 0)
    mk = lambda: rh.DevicePoly.from_torch(rq, rand_block(B, Q, N))
    ct0, ct1 = rh.Ciphertext([mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True)
    out = rh.Ciphertext([mk(), mk(), mk()], is_ntt=True)
    tc, tcf = [], []
    for _ in range(rounds):
        tc.append(timed(lambda: ev.MulScaleInvariant(ct0, ct1, out), reps=5, warm=2))
        ev.set_tuning("fused_quantize", 1); tcf.append(timed(lambda: ev.MulScaleInvariant(ct0, ct1, out), reps=5, warm=2)); ev.set_tuning("fused_quantize", 0)
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    q_tr = 16.0 * (2 * LQ + LM)                        # the three transforms of a quantize, bytes per coefficient
    bytes_a, bytes_b = q_tr + 8.0 * (4 * LQ + 3 * LM), q_tr + 8.0 * (2 * LQ + LM)     # ModDownQPtoP LQ + 2 LM, ModUpPtoQ LM + LQ, MulScalar 2 LQ; fused: LQ + LM in, LQ out
    mul_bytes = 296.0 * LQ + 224.0 * LM               # 10 LQ + 7 LM limb transforms, ModUp, tensor, fused quantize middle
    mul_bytes_composed = mul_bytes + 3 * 8.0 * (2 * LQ + 2 * LM)     # the composed middle moves 8 (2 LQ + 2 LM) more per quantize
    a, b, c = stat(ta), stat(tb), stat(tc)
    gbs = lambda byt, ms: round(byt * N * B / (ms * 1e-3) / 1e9, 1)
    a.update(op="(a) quantize composed: INTTLazy x2, rh_bext_moddown_qp_to_p, rh_bext_modup_p_to_q, MulScalar, NTT", algorithmic_GBps=gbs(bytes_a, a["ms_median"]))
    b.update(op="(b) rh_bfv_quantize, fused kernel (fused_quantize = 1)", algorithmic_GBps=gbs(bytes_b, b["ms_median"]))
    inner = stat(tinner); inner.update(op="(a') rh_bfv_quantize as shipped (fused_quantize = 0: the composed sequence on the handle's scratch)")
    cf = stat(tcf); cf.update(op="(c') the same with fused_quantize = 1", ctmul_per_s=round(B / (cf["ms_median"] * 1e-3), 1),
                              algorithmic_bytes_per_coefficient=mul_bytes, algorithmic_GBps=gbs(mul_bytes, cf["ms_median"]),
                              frac_of_8TBps=round(gbs(mul_bytes, cf["ms_median"]) / PEAK, 3))
    c.update(op="(c) rh_bfv_mul_scale_invariant as shipped (no relinearisation)", ctmul_per_s=round(B / (c["ms_median"] * 1e-3), 1),
             limb_transforms_per_ctmul=10 * LQ + 7 * LM, algorithmic_bytes_per_coefficient=mul_bytes_composed,
             algorithmic_GBps=gbs(mul_bytes_composed, c["ms_median"]), frac_of_8TBps=round(gbs(mul_bytes_composed, c["ms_median"]) / PEAK, 3))
    spread = max(a["ms_max"] - a["ms_min"], b["ms_max"] - b["ms_min"])
    from bench import csrc_tree_hash                 # ties the numbers to the kernel sources they were taken on, as tools/make_traffic.py does
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_QMul": LM, "batch": B, "t": T},
           "method": "%d alternating windows of %d calls each (5 for the multiply), device events, 2 warm-up calls per window" % (rounds, reps),
           "results": [a, inner, b, c, cf], "run_to_run_spread_ms": round(spread, 4),
           "fused_beats_composed_by_more_than_spread": bool(a["ms_median"] - b["ms_median"] > spread)}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    ev.close(); be.close(); rq.close(); rm.close()


def bgv_group(out_path):
    """N = 2^15, 16 limbs of Qi60, 4 of Pi60, batch 32: one block is 128 MiB, an operand set 0.9 GiB, far beyond the Infinity Cache.
    bgv.Evaluator with fused=True (rh_bgv_tensor) against fused=False, which issues the reference's own sequence of ring calls through entry
    points the library had before (MulRNSScalarMontgomery, MulScalar, MulCoeffsMontgomery(ThenAdd)): the composed path is the baseline, timed
    HERE, alternating with the fused one.  Medians of `rounds` windows of `reps` calls, the windows' min and max as the spread.  Algorithmic
    bytes count whole-limb passes of the tensoring alone (7 vs 17; accumulate with r0, r1 != 1: 10 vs 30 into degree 2, 8 vs 25 with relin);
    the relinearisation and the rescale are the same launches on both sides and are reported as times only."""
    import statistics
    N, LQ, LP, B, T, rounds, reps = 1 << 15, 16, 4, 32, 65537, 7, 10
    Q, P = QI60[:LQ], PI60[:LP]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    digits = (LQ + LP - 1) // LP
    evkQ, evkP = rand_block(2 * digits, Q, N).cpu().numpy().astype(np.uint64), rand_block(2 * digits, P, N).cpu().numpy().astype(np.uint64)
    rlk = rh.rlwe.GadgetCiphertext(rq, rp, evkQ.reshape(digits, 2, LQ, N), evkP.reshape(digits, 2, LP, N))
    evs = {True: rh.bgv.Evaluator(rq, None, T, ringP=rp, rlk=rlk, fused=True), False: rh.bgv.Evaluator(rq, None, T, ringP=rp, rlk=rlk, fused=False)}
    mk = lambda: rh.DevicePoly.from_torch(rq, rand_block(B, Q, N))
    ct0, ct1 = rh.Ciphertext([mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True)
    ct0.Scale, ct1.Scale = 3, 5
    out2, out1, low = rh.Ciphertext([mk(), mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True)

    def set7(ct):                                     # an accumulator whose scale differs from the product's: r0 != 1 and r1 != 1 on every call
        ct.Scale = 7
    cases = {
        "Mul (tensorStandard, no relinearisation)": (lambda ev: ev.Mul(ct0, ct1, out2), 7, 17),
        "MulThenAdd into degree 2, r0, r1 != 1": (lambda ev: (set7(out2), ev.MulThenAdd(ct0, ct1, out2)), 10, 30),
        "MulRelin + Rescale": (lambda ev: (ev.MulRelin(ct0, ct1, out1), ev.Rescale(out1, low)), 7, 17),
        "MulRelinThenAdd, r0, r1 != 1": (lambda ev: (set7(out1), ev.MulRelinThenAdd(ct0, ct1, out1)), 8, 25),
    }
    # same bits first, on the shapes that are timed (seeded inputs, both paths from the same accumulator)
    for name, (fn, _, _) in cases.items():
        acc = out2 if "degree 2" in name or "no relin" in name else out1
        keep = [v.numpy().copy() for v in acc.Value]
        res = []
        for fused in (True, False):
            for v, h in zip(acc.Value, keep):
                _ = rh.DevicePoly.from_numpy(rq, h); rq.CopyLvl(_, v)
            fn(evs[fused]); res.append([v.numpy() for v in (low.Value if "Rescale" in name else acc.Value)])
        assert all(np.array_equal(x, y) for x, y in zip(*res)), "fused and composed differ: " + name
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    results = []
    for name, (fn, pf, pc) in cases.items():
        tf, tc = [], []
        n = reps if "Relin" in name else 5 * reps      # the tensoring alone is a fraction of a millisecond: longer windows
        for _ in range(rounds):
            tf.append(timed(lambda: fn(evs[True]), reps=n)); tc.append(timed(lambda: fn(evs[False]), reps=n))
        f, c = stat(tf), stat(tc)
        limb_bytes = 8.0 * N * LQ * B
        entry_ = {"op": name, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
                  "tensor_passes_fused": pf, "tensor_passes_composed": pc}
        if "Relin" not in name:                       # the tensoring alone: algorithmic bandwidth means something
            f["algorithmic_GBps"] = round(pf * limb_bytes / (f["ms_median"] * 1e-3) / 1e9, 1)
            c["algorithmic_GBps"] = round(pc * limb_bytes / (c["ms_median"] * 1e-3) / 1e9, 1)
            f["frac_of_8TBps"] = round(f["algorithmic_GBps"] / PEAK, 3)
        results.append(entry_)
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batch": B, "t": T},
           "method": "%d alternating windows of %d calls each (%d for the two cases without relinearisation), device events, 2 warm-up calls per window; "
                     "clocks left to the driver's default governor" % (rounds, reps, 5 * reps),
           "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    for ev in evs.values():
        ev.close()
    rq.close(); rp.close()


def ckks_group(out_path):
    """The config 5 ring: N = 2^16, 24 limbs of Qi60, 6 of Pi60, batch 64 (one block is 768 MiB, far beyond the Infinity Cache).
    ckks.Evaluator with fused=True (csrc/ckks.hip) against fused=False, which issues the reference's own sequence of ring calls through entry
    points the library had before: the composed path is the baseline, timed HERE, alternating with the fused one.  Medians of `rounds` windows
    of `reps` calls; the spread is the composed windows' max - min, and `fused_default` says whether the fused median is within that spread of
    the composed one or below it -- the rule the evaluator's FUSED_DEFAULT table follows.  Whole-limb passes of the element-wise part: MulThenAdd
    10 vs 20, scale-matched Add 6 vs 10, scalar Mul 4 vs 4 (one launch vs four); the relinearisation is the same launches on both sides."""
    import statistics
    N, LQ, LP, B, rounds, reps = 1 << 16, 24, 6, 64, 7, 10
    Q, P = QI60[:LQ], PI60[:LP]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    digits = (LQ + LP - 1) // LP
    evq, evp = rand_block(2 * digits, Q, N), rand_block(2 * digits, P, N)
    rlk = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
    rlk.digits, rlk.levelQ, rlk.levelP, rlk.BaseTwoDecomposition, rlk.digits_per_limb = digits, LQ - 1, LP - 1, 0, None
    rlk.Q, rlk.P = rh.DevicePoly.from_torch(rq, evq), rh.DevicePoly.from_torch(rp, evp)
    evs = {f: rh.ckks.Evaluator(rq, rp, rlk=rlk, fused=f) for f in (True, False)}
    mk = lambda: rh.DevicePoly.from_torch(rq, rand_block(B, Q, N))
    Sc = rh.ckks.Scale
    ct0, ct1, ct6 = (rh.Ciphertext([mk(), mk()], is_ntt=True) for _ in range(3))
    ct0.Scale, ct1.Scale, ct6.Scale = Sc(2 ** 40), Sc(2 ** 40), Sc(6 * 2 ** 40)
    out2, out1 = rh.Ciphertext([mk(), mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True)

    def matched(ct):                                  # an accumulator at the product's scale: nothing but the multiply-accumulate on every call
        ct.Scale = Sc(2 ** 80)
    cases = {
        "MulThenAdd ct x ct into degree 2": (lambda ev: (matched(out2), ev.MulThenAdd(ct0, ct1, out2)), out2, 10, 20),
        "MulRelinThenAdd": (lambda ev: (matched(out1), ev.MulRelinThenAdd(ct0, ct1, out1)), out1, 9, 19),
        "Add, scales 1 : 6": (lambda ev: ev.Add(ct0, ct6, out1), out1, 6, 10),
        "Mul by 0.5 on a degree-1 ciphertext": (lambda ev: ev.Mul(ct0, 0.5, out1), out1, 4, 4),
    }
    for name, (fn, acc, _, _) in cases.items():       # same bits first, on the shapes that are timed, both paths from the same accumulator
        keep = [rh.DevicePoly.from_torch(rq, rand_block(B, Q, N)) for _ in acc.Value]
        res = []
        for fused in (True, False):
            for v, h in zip(acc.Value, keep):
                rq.CopyLvl(h, v)
            fn(evs[fused]); res.append([v.numpy() for v in acc.Value])
        assert all(np.array_equal(x, y) for x, y in zip(*res)), "fused and composed differ: " + name
        del keep, res
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    results = []
    for name, (fn, _, pf, pc) in cases.items():
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(evs[True]), reps=reps)); tc.append(timed(lambda: fn(evs[False]), reps=reps))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        limb_bytes = 8.0 * N * LQ * B
        entry_ = {"op": name, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
                  "composed_run_to_run_spread_ms": spread, "fused_default": bool(f["ms_median"] <= c["ms_median"] + spread),
                  "passes_fused": pf, "passes_composed": pc}
        if "Relin" not in name:                       # the element-wise part alone: algorithmic bandwidth means something
            f["algorithmic_GBps"] = round(pf * limb_bytes / (f["ms_median"] * 1e-3) / 1e9, 1)
            c["algorithmic_GBps"] = round(pc * limb_bytes / (c["ms_median"] * 1e-3) / 1e9, 1)
            f["frac_of_8TBps"] = round(f["algorithmic_GBps"] / PEAK, 3)
        results.append(entry_)
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batch": B},
           "method": "%d alternating windows of %d calls each, device events, 2 warm-up calls per window; clocks left to the driver's default governor"
                     % (rounds, reps),
           "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    for ev in evs.values():
        ev.close()
    rq.close(); rp.close()


def ckks_encoder_group(out_path):
    """The CKKS encoder (csrc/ckks_encoder.hip) at N = 2^16, 24 limbs of Qi60, full slots (2^15), nvec = 64, device-resident values and
    plaintexts: Encode and Decode in the NTT domain, and the two transforms alone.  There is no earlier implementation to compare with, so
    each line stands against its algorithmic bytes: per vector 16 slots in and 8 L N out for the quantizer plus 16 N per limb for the
    Ring.NTT pass (Encode); the mirror image for Decode (16 N per limb for Ring.INTT, 8 L 2 slots gathered, 16 slots out); 16 slots in and
    16 slots out for a transform alone -- its global stages (3 at 2^15 slots with 2^12-value LDS blocks) are overhead against that figure.
    Medians of `rounds` alternating windows of `reps` calls, device events, 2 warm-up calls per window."""
    import statistics
    N, L, B, rounds, reps = 1 << 16, 24, 64, 7, 5
    logs, slots = 15, 1 << 15
    Q = QI60[:L]
    rq = rh.Ring(N, Q); rq.set_stream(stream.cuda_stream)
    enc = rh.ckks.Encoder(rq)
    enc.reserve(B)
    rng = np.random.default_rng(0)
    host = rng.uniform(-1, 1, (B, slots)) + 1j * rng.uniform(-1, 1, (B, slots))
    vals, work, out = (rh.ckks.DeviceValues.from_numpy(rq, host) for _ in range(3))
    pt = enc.NewPlaintext(L - 1, 2.0 ** 45, nvec=B)
    enc.Encode(vals, pt)
    enc.Decode(pt, out)
    err = float(np.max(np.abs(out.numpy() - host)))
    assert err < 2.0 ** -28, "Encode then Decode lost the values: %g" % err      # log2(scale) - (logN + 2) = 27 bits (ckks_test.go:272-298)
    per_ntt = 16.0 * N * L
    cases = {
        "Encode (IFFT, quantize, NTT)": (lambda: enc.Encode(vals, pt), 16.0 * slots + 8.0 * L * N + per_ntt),
        "Decode (INTT, CRT to double, FFT)": (lambda: enc.Decode(pt, out), per_ntt + 8.0 * L * 2 * slots + 16.0 * slots),
        "special IFFT alone": (lambda: enc.IFFT(work, logs), 32.0 * slots),
        "special FFT alone": (lambda: enc.FFT(work, logs), 32.0 * slots),
    }
    times = {k: [] for k in cases}
    for _ in range(rounds):
        for name, (fn, _) in cases.items():
            times[name].append(timed(fn, reps=reps))
    results = []
    for name, (_, vec_bytes) in cases.items():
        v = times[name]
        ms = statistics.median(v)
        gbs = vec_bytes * B / (ms * 1e-3) / 1e9
        results.append({"op": name, "ms_median": round(ms, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                        "vectors_per_s": round(B / (ms * 1e-3), 1), "algorithmic_bytes_per_vector": vec_bytes,
                        "algorithmic_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / PEAK, 4)})
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": L, "log_slots": logs, "nvec": B},
           "round_trip_max_abs_error": err,
           "method": "%d alternating windows of %d calls each, device events, 2 warm-up calls per window; clocks left to the driver's default governor"
                     % (rounds, reps),
           "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    enc.close()
    rq.close()


def bgv_encoder_group(out_path):
    """The BGV encoder (csrc/bgv_encoder.hip) at N = 2^16, 24 limbs of Qi60, nvec = 64, device-resident values and plaintexts, top level:
    T = 65537 (n = 2^15, gap 2: Q to T is the exact-CRT branch, which has one form) and T = 786433 (n = 2^16, gap 1: the ModUpExact branch).
    Every line is timed with "fused" = 1 and = 0 (the reference's sequence of ring and basis-extension calls) in the same process, in
    alternating windows, and stands against its algorithmic bytes per vector: lift 8 n in + 8 L N out; Q to T 8 L n in + 8 n out; a Ring
    transform 16 N per limb; the transform modulo T 16 n; slots 8 n in + 8 n out.  Medians of `rounds` windows of `reps` calls, device
    events, 2 warm-up calls per window; the spread is the windows' max - min."""
    import hashlib
    import statistics
    N, L, B, rounds, reps = 1 << 16, 24, 64, 7, 5
    Q = QI60[:L]
    rq = rh.Ring(N, Q); rq.set_stream(stream.cuda_stream)
    rng = np.random.default_rng(0)
    lines = []
    for T in (65537, 786433):
        enc = rh.bgv.Encoder(rq, T)
        enc.reserve(B)
        n = enc.MaxSlots()
        host = rng.integers(0, T, (B, n), dtype=np.uint64)
        vals = rh.bgv.DeviceValues.from_numpy(rq, host)
        out = rh.bgv.DeviceValues(rq, B, n)
        pt = enc.NewPlaintext(L - 1, 3, nvec=B)
        pT = enc.RingT().NewPoly(B)
        pt0 = rq.AtLevel(0).NewPoly(B)
        pt_nb = rh.bgv.Plaintext(rq.AtLevel(0).NewPoly(B), 3, is_ntt=False, is_batched=False)      # the slot kernel has no entry of its own: its shortest caller
        enc.Encode(vals, pt)
        rq.AtLevel(0).CopyLvl(pt.Value[0], pt0)
        enc.Decode(pt, out)
        assert np.array_equal(out.numpy(), host), "Encode then Decode lost the values"
        digest = {}
        for fused in (1, 0):                              # both forms give the same bits at this size too
            enc.set_tuning("fused", fused)
            enc.Encode(vals, pt); enc.Decode(pt, out); enc.RingQ2T(L - 1, True, pt.Value[0], pT)
            digest[fused] = [hashlib.sha256(a.numpy()).hexdigest() for a in (pt.Value[0], out, pT)]
        assert digest[0] == digest[1], "fused and composed differ"
        del digest
        per_ntt, lift, q2t = 16.0 * N * L, 8.0 * n + 8.0 * L * N, 8.0 * L * n + 8.0 * n
        cases = {
            "Encode (slots, INTT mod T, lift, NTT)": (lambda: enc.Encode(vals, pt), 16.0 * n + 16.0 * n + lift + per_ntt),
            "Decode (INTT, Q to T, NTT mod T, slots)": (lambda: enc.Decode(pt, out), per_ntt + q2t + 16.0 * n + 16.0 * n),
            "EncodeRingT (slots, INTT mod T, MulScalar)": (lambda: enc.EncodeRingT(vals, 3, pT), 16.0 * n + 16.0 * n + 16.0 * n),
            "lift alone (RingT2Q, scaleUp)": (lambda: enc.RingT2Q(L - 1, True, pT, pt.Value[0]), lift),
            "Q to T alone (RingQ2T)": (lambda: enc.RingQ2T(L - 1, True, pt.Value[0], pT), q2t),
            "Q to T alone at level 0": (lambda: enc.RingQ2T(0, True, pt0, pT), 16.0 * n),
            "slots + one-limb lift (Encode, IsBatched = false, level 0, coefficient domain)": (lambda: enc.Encode(vals, pt_nb), 8.0 * n + 16.0 * n + 8.0 * N),
        }
        times = {(k, f): [] for k in cases for f in (1, 0)}
        for _ in range(rounds):
            for name, (fn, _) in cases.items():
                for fused in (1, 0):
                    enc.set_tuning("fused", fused)
                    times[(name, fused)].append(timed(fn, reps=reps))
        enc.set_tuning("fused", -1)
        for name, (_, vec_bytes) in cases.items():
            f, c = times[(name, 1)], times[(name, 0)]
            ms, msc = statistics.median(f), statistics.median(c)
            gbs = vec_bytes * B / (ms * 1e-3) / 1e9
            lines.append({"T": T, "n": n, "gap": N // n, "op": name, "fused_ms_median": round(ms, 4), "fused_ms_min": round(min(f), 4),
                          "fused_ms_max": round(max(f), 4), "composed_ms_median": round(msc, 4), "composed_ms_min": round(min(c), 4),
                          "composed_ms_max": round(max(c), 4), "composed_spread_ms": round(max(c) - min(c), 4),
                          "fused_wins_by_more_than_spread": bool(msc - ms > max(c) - min(c)),
                          "vectors_per_s": round(B / (ms * 1e-3), 1), "algorithmic_bytes_per_vector": vec_bytes,
                          "algorithmic_GBps": round(gbs, 1), "frac_of_8TBps": round(gbs / PEAK, 4)})
        enc.close()
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": L, "nvec": B, "level": L - 1},
           "method": "%d alternating windows of %d calls each per form, device events, 2 warm-up calls per window; clocks left to the driver's default governor"
                     % (rounds, reps),
           "results": lines}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    rq.close()


def inner_sum_group(out_path):
    """The config 5 ring of ckks_group: N = 2^16, 24 limbs of Qi60, 6 of Pi60, batch 64.  rlwe.Evaluator.PartialTracesSum(offset 1) for n = 7 (three
    decompositions, two lazy rotations accumulated modulo QP, two hoisted ones, one ModDown) and n = 8 (three hoisted rotations), with fused=True
    (csrc/inner_sum.hip) against fused=False, the same sequence composed from DecomposeNTT / AutomorphismHoisted(Lazy) / Add / ModDown; and each
    kernel alone against the passes it replaces.  Both paths are timed HERE, in alternating windows, as in ckks_group; `fused_default` is the rule
    rlwe.Evaluator.FUSED_INNER_SUM follows: the fused median within the composed windows' max - min of the composed median, or below it.
    Whole-row passes (row-words moved per coefficient set): the accumulate tail 13 against 23, the rotate-add tail 6 against 10."""
    import statistics
    N, LQ, LP, B, rounds, reps = 1 << 16, 24, 6, 64, 7, 10
    Q, P = QI60[:LQ], PI60[:LP]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    digits = (LQ + LP - 1) // LP
    level, levelP = LQ - 1, LP - 1

    def key():
        k = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
        k.digits, k.levelQ, k.levelP, k.BaseTwoDecomposition, k.digits_per_limb = digits, level, levelP, 0, None
        k.Q, k.P = rh.DevicePoly.from_torch(rq, rand_block(2 * digits, Q, N)), rh.DevicePoly.from_torch(rp, rand_block(2 * digits, P, N))
        return k
    galEls = sorted({g for n in (7, 8) for kind, g, _ in rh.rlwe.partial_traces_plan(N, 1, n) if kind != rh.rlwe.CLOSE})
    ev = rh.rlwe.Evaluator(rq, rp, galois_keys={g: key() for g in galEls})
    mkq = lambda: rh.DevicePoly.from_torch(rq, rand_block(B, Q, N))
    mkp = lambda: rh.DevicePoly.from_torch(rp, rand_block(B, P, N))
    ct, out = rh.Ciphertext([mkq(), mkq()], is_ntt=True), rh.Ciphertext([mkq(), mkq()], is_ntt=True)
    qp = lambda: rh.rlwe.ElementQP([rh.rlwe.PolyQP(mkq(), mkp()), rh.rlwe.PolyQP(mkq(), mkp())])
    tmp, acc, rot = qp(), qp(), qp()
    g = galEls[-1]
    Pbig = 1
    for p in P:
        Pbig *= int(p)

    def tail_composed():                              # AutomorphismHoistedLazy after its product, then ringQP.Add: 1 + 4 + 4 passes
        rq.MulScalarBigintThenAdd(ct.Value[0], Pbig, tmp.Value[0].Q)
        for c in (1, 0):
            rq.AutomorphismNTT(tmp.Value[c].Q, g, rot.Value[c].Q); rp.AutomorphismNTT(tmp.Value[c].P, g, rot.Value[c].P)
        for c in (0, 1):
            rq.vec_op("ADD", acc.Value[c].Q, rot.Value[c].Q, acc.Value[c].Q); rp.vec_op("ADD", acc.Value[c].P, rot.Value[c].P, acc.Value[c].P)

    def rotate_add_composed():                        # the end of AutomorphismHoisted, then ringQ.Add: 2 + 2 passes
        for c in (0, 1):
            rq.AutomorphismNTT(tmp.Value[c].Q, g, rot.Value[c].Q)
        for c in (0, 1):
            rq.vec_op("ADD", out.Value[c], rot.Value[c].Q, out.Value[c])
    tq = rh.Ciphertext([tmp.Value[0].Q, tmp.Value[1].Q], is_ntt=True)
    cases = {
        "PartialTracesSum n = 7": (lambda f: ev.PartialTracesSum(ct, 1, 7, out, fused=f), None, None),
        "PartialTracesSum n = 8": (lambda f: ev.PartialTracesSum(ct, 1, 8, out, fused=f), None, None),
        "rotate and accumulate modulo QP, the kernel alone": (lambda f: ev.RotateAccumulateQP(level, g, ct.Value[0], tmp, acc, False) if f else tail_composed(), 13, 23),
        "rotate and add modulo Q, the kernel alone": (lambda f: ev.RotateAddQ(level, g, tq, out) if f else rotate_add_composed(), 6, 10),
    }
    res = []
    for fused in (True, False):                       # same bits first, at the timed shape
        ev.PartialTracesSum(ct, 1, 7, out, fused=fused)
        res.append([v.numpy() for v in out.Value])
    assert all(np.array_equal(x, y) for x, y in zip(*res)), "fused and composed PartialTracesSum differ"
    del res
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    results = []
    row_bytes = 8.0 * N * B                           # one row-word per coefficient set: (LQ + LP) rows modulo QP, LQ modulo Q
    for name, (fn, pf, pc) in cases.items():
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), reps=reps)); tc.append(timed(lambda: fn(False), reps=reps))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        entry_ = {"op": name, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
                  "composed_run_to_run_spread_ms": spread, "fused_default": bool(f["ms_median"] <= c["ms_median"] + spread)}
        if pf == 13:                                  # per coefficient set: 2 (acc in, out) + 1 (tmp) per Q and P row and component, + ct0 on the Q rows of one = 13 / 23 words
            words = lambda per_qp, extra_q: (per_qp * 2 * (LQ + LP) + extra_q * LQ) * row_bytes
            f["algorithmic_GBps"] = round(words(3, 1) / (f["ms_median"] * 1e-3) / 1e9, 1)
            c["algorithmic_GBps"] = round(words(5, 3) / (c["ms_median"] * 1e-3) / 1e9, 1)
        elif pf == 6:
            f["algorithmic_GBps"] = round(6 * LQ * row_bytes / (f["ms_median"] * 1e-3) / 1e9, 1)
            c["algorithmic_GBps"] = round(10 * LQ * row_bytes / (c["ms_median"] * 1e-3) / 1e9, 1)
        if pf:
            entry_["row_words_fused"], entry_["row_words_composed"] = pf, pc
            f["frac_of_8TBps"] = round(f["algorithmic_GBps"] / PEAK, 3)
        results.append(entry_)
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batch": B, "offset": 1},
           "method": "%d alternating windows of %d calls each, device events, 2 warm-up calls per window; clocks left to the driver's default governor"
                     % (rounds, reps),
           "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    ev.close()
    rq.close(); rp.close()


def ring_packing_group(out_path):
    """rlwe.RingPackingEvaluator at the config 5 ring of ckks_group (N = 2^16, 24 limbs of Qi60, 6 of Pi60) and at a small ring (N = 2^12, 4 | 2 limbs):
    Expand to 64 outputs (logGap = 10) and the small ring's full expansion (4096 outputs), Pack of the same counts, Split and Merge of 64 ciphertexts;
    fused=True (csrc/ring_packing.hip) against fused=False, the same sequence composed from AutomorphismNTT and vec_op passes; each kernel alone
    against the passes it replaces; and the batched level sequence against one launch sequence per ciphertext, what a port of the reference's loop
    would issue.  Alternating windows as in inner_sum_group; `fused_default` is the rule RingPackingEvaluator.FUSED_RING_PACKING follows.  The keys
    are random words (one block serves every Galois element): the timing does not read them."""
    import statistics
    from bench import csrc_tree_hash
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}

    def compare(name, fn, rounds, reps, extra=None, labels=("fused", "composed")):
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), reps=reps, warm=1)); tc.append(timed(lambda: fn(False), reps=reps, warm=1))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        e = {"op": name, labels[0]: f, labels[1]: c, "ratio_%s_over_%s" % (labels[1], labels[0]): round(c["ms_median"] / f["ms_median"], 3),
             "%s_run_to_run_spread_ms" % labels[1]: spread, "windows": rounds, "calls_per_window": reps}
        if labels[0] == "fused":
            e["fused_default"] = bool(f["ms_median"] <= c["ms_median"] + spread)
        e.update(extra or {})
        print(json.dumps(e), flush=True)
        return e

    def setup(logN, LQ, LP, two_degrees):
        N = 1 << logN
        Q, P = QI60[:LQ], PI60[:LP]
        rings = {}
        for lg in ((logN - 1, logN) if two_degrees else (logN,)):
            rq, rp = rh.Ring(1 << lg, Q), rh.Ring(1 << lg, P)
            rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
            rings[lg] = (rq, rp)
        rq, rp = rings[logN]
        digits = (LQ + LP - 1) // LP
        k = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
        k.digits, k.levelQ, k.levelP, k.BaseTwoDecomposition, k.digits_per_limb = digits, LQ - 1, LP - 1, 0, None
        k.Q, k.P = rh.DevicePoly.from_torch(rq, rand_block(2 * digits, Q, N)), rh.DevicePoly.from_torch(rp, rand_block(2 * digits, P, N))
        gal = {g: k for g in set(rh.rlwe.GaloisElementsForExpand(N, logN) + rh.rlwe.GaloisElementsForPack(N, logN))}
        sw = {logN: {logN - 1: k}, logN - 1: {logN: k}} if two_degrees else None
        ev = rh.rlwe.RingPackingEvaluator(rings, RingSwitchingKeys=sw, RepackKeys={logN: gal}, ExtractKeys={logN: gal})
        mk = lambda lg, B: rh.Ciphertext([rh.DevicePoly.from_torch(rings[lg][0], rand_block(B, Q, 1 << lg)) for _ in (0, 1)], is_ntt=True)
        return N, Q, rings, ev, mk, k

    def expand_per_ciphertext(ev, ct, logGap):
        """the reference's loop (ring_packing.go:549-583) with the fused kernel: one key switch and one launch per ciphertext of every level.  Timing only:
        a level's second outputs land next to their sources, not where Expand puts them."""
        logN, e, keys = ev._expand_checks(ct, logGap)
        out, rq, level, B = ev._expand_head(ct, logN, logGap, e)
        N, gap = 1 << logN, 1 << logGap
        tmp = [e.buffer("rpOne%d" % c, rq, 1, level + 1) for c in (0, 1)]
        L = rh.lib()
        for i in range(logN):
            n = 1 << i
            g = N // n + 1
            for p in range(max(n // gap, 1)):
                c = [rh.rlwe._view(out.Value[k], 2 * p if n >= gap else p, 1) for k in (0, 1)]
                ev._key_switch(e, level, c[0], c[1], keys[g], tmp[0], tmp[1])
                if n >= gap:
                    rh.rlwe._check(L.rh_rlwe_expand_step(rq._h, level, g, tmp[0].ptr, tmp[1].ptr, c[0].ptr, c[1].ptr, ev.XInvPow2NTT[logN][i].ptr, 1))
                else:
                    e.RotateAddQ(level, g, rh.Ciphertext(tmp, is_ntt=True), rh.Ciphertext(c, is_ntt=True))
        return out

    results, shapes = [], {}
    # ---- the config 5 ring ----
    logN, LQ, LP, nout = 16, 24, 6, 64
    N, Q, rings, ev, mk, key = setup(logN, LQ, LP, True)
    shapes["config5"] = {"N": N, "limbs_Q": LQ, "limbs_P": LP, "outputs": nout, "logGap": logN - 6}
    rq = rings[logN][0]
    level = LQ - 1
    ct = mk(logN, 1)
    res = [[v.numpy() for v in ev.Expand(ct, logN - 6, fused=f)[0].Value] for f in (True, False)]      # same bits first, at the timed shape
    assert all(np.array_equal(x, y) for x, y in zip(*res)), "fused and composed Expand differ"
    del res
    results.append(compare("Expand to 64 outputs, config 5", lambda f: ev.Expand(ct, logN - 6, fused=f), 5, 4))
    results.append(compare("Expand to 64 outputs, config 5: batched levels against one launch sequence per ciphertext",
                           lambda f: ev.Expand(ct, logN - 6, fused=True) if f else expand_per_ciphertext(ev, ct, logN - 6), 5, 4, labels=("batched", "per_ciphertext")))
    keys64 = [m << (logN - 6) for m in range(nout)]
    batch = mk(logN, nout)
    results.append(compare("Pack of 64 ciphertexts, config 5", lambda f: ev.Pack(batch, keys64, logN, True, fused=f), 5, 3))
    # the kernels alone, 32 ciphertexts (the last level of the expansion): row moves per component 5 against 13, 5 + 3 against 14
    cnt = 32
    e = ev.Evaluators[logN]
    big, tmp, rot = mk(logN, 2 * cnt), mk(logN, cnt), mk(logN, cnt)
    xi, xp = ev.XInvPow2NTT[logN][15], ev.XPow2NTT[logN][0]
    g = N // (1 << 15) + 1
    L = rh.lib()
    lo = [rh.rlwe._view(big.Value[c], 0, cnt) for c in (0, 1)]
    hi = [rh.rlwe._view(big.Value[c], cnt, cnt) for c in (0, 1)]
    xrep = ev._replicated(xi, cnt, rq.AtLevel(level), level)

    def step(f):
        if f:
            rh.rlwe._check(L.rh_rlwe_expand_step(rq._h, level, g, tmp.Value[0].ptr, tmp.Value[1].ptr, big.Value[0].ptr, big.Value[1].ptr, xi.ptr, cnt))
            return
        for c in (0, 1):
            rq.AutomorphismNTT(tmp.Value[c], g, rot.Value[c]); rq.Sub(lo[c], rot.Value[c], hi[c]); rq.Add(lo[c], rot.Value[c], lo[c])
            rq.MulCoeffsMontgomery(hi[c], xrep, hi[c])
    row = 8.0 * N * cnt * LQ * 2
    ent = compare("expand step, the kernel alone (32 ciphertexts)", step, 7, 10, {"row_moves_fused": 5, "row_moves_composed": 11,
                  "note": "composed: AutomorphismNTT 2, Sub 3, Add 3, MulCoeffsMontgomery 3 row moves = 11; the reference's own sequence adds the CopyNew (2): 13"})
    ent["fused"]["algorithmic_GBps"] = round(5 * row / (ent["fused"]["ms_median"] * 1e-3) / 1e9, 1)
    ent["fused"]["frac_of_8TBps"] = round(ent["fused"]["algorithmic_GBps"] / PEAK, 3)
    results.append(ent)
    entries = [(rh.rlwe.MODE_AB, p, cnt + p) for p in range(cnt)]
    arr = np.array([v for en in entries for v in en] + [0, 0], dtype=np.int32)
    dt = rh.DevicePoly(rq, 1, 1)
    rh.rlwe._check(L.rh_dev_upload(rq._h, dt.ptr, arr.view(np.uint64).ctypes.data_as(rh.ringhip.U64P), arr.size // 2))
    import ctypes as C
    th = arr.ctypes.data_as(C.POINTER(C.c_int32))
    u = mk(logN, cnt)
    xprep = ev._replicated(xp, cnt, rq.AtLevel(level), level)

    def combine(f):
        if f:
            rh.rlwe._check(L.rh_rlwe_pack_combine(rq._h, level, big.Value[0].ptr, big.Value[1].ptr, 2 * cnt, dt.ptr, th, cnt, xp.ptr, u.Value[0].ptr, u.Value[1].ptr))
            return
        for c in (0, 1):
            rq.MulCoeffsMontgomery(hi[c], xprep, hi[c]); rq.Sub(lo[c], hi[c], u.Value[c]); rq.Add(lo[c], hi[c], lo[c])

    def finish(f):
        if f:
            rh.rlwe._check(L.rh_rlwe_rotate_addsub_q(rq._h, level, g, tmp.Value[0].ptr, tmp.Value[1].ptr, big.Value[0].ptr, big.Value[1].ptr, 2 * cnt, dt.ptr, th, cnt))
            return
        for c in (0, 1):
            rq.AutomorphismNTT(tmp.Value[c], g, rot.Value[c]); rq.Add(lo[c], rot.Value[c], lo[c])
    results.append(compare("pack combine, the kernel alone (32 pairs, batched passes)", combine, 7, 10, {"row_moves_fused": 5, "row_moves_composed": 9}))
    results.append(compare("pack finish, the kernel alone (32 ciphertexts)", finish, 7, 10, {"row_moves_fused": 3, "row_moves_composed": 5}))
    # Split and Merge of 64 ciphertexts
    B = 64
    ctN, even, odd = mk(logN, B), mk(logN - 1, B), mk(logN - 1, B)
    results.append({"op": "Split of 64 ciphertexts, config 5", "ms": stat([timed(lambda: ev.Split(ctN, even, odd), reps=5, warm=1) for _ in range(5)])})
    results.append({"op": "Merge of 64 ciphertexts, config 5", "ms": stat([timed(lambda: ev.Merge(even, odd, ctN), reps=5, warm=1) for _ in range(5)])})
    print(json.dumps(results[-2:]), flush=True)
    t0, t1 = mk(logN, B), mk(logN, B)
    xinv0, x0 = ev._replicated(ev.XInvPow2NTT[logN][0], B, rq.AtLevel(level), level), ev._replicated(xp, B, rq.AtLevel(level), level)

    def split_kernel(f):
        if f:
            rh.rlwe._check(L.rh_rlwe_ring_split(rq._h, level, t0.Value[0].ptr, t0.Value[1].ptr, even.Value[0].ptr, even.Value[1].ptr, odd.Value[0].ptr, odd.Value[1].ptr, 1, B))
            return
        # the reference's route to the odd half (:239-241): times X^-1, a second inverse transform; then both strided copies
        for c in (0, 1):
            rq.MulCoeffsMontgomery(t0.Value[c], xinv0, t1.Value[c]); rq.INTT(t1.Value[c], t1.Value[c])
        rh.rlwe._check(L.rh_rlwe_ring_split(rq._h, level, t0.Value[0].ptr, t0.Value[1].ptr, even.Value[0].ptr, even.Value[1].ptr, None, None, 1, B))
        rh.rlwe._check(L.rh_rlwe_ring_split(rq._h, level, t1.Value[0].ptr, t1.Value[1].ptr, odd.Value[0].ptr, odd.Value[1].ptr, None, None, 1, B))

    def merge_kernel(f):
        o = odd.Value if f else (None, None)
        rh.rlwe._check(L.rh_rlwe_ring_merge(rq._h, level, even.Value[0].ptr, even.Value[1].ptr, o[0].ptr if f else None, o[1].ptr if f else None, xp.ptr if f else None,
                                            t0.Value[0].ptr, t0.Value[1].ptr, 1, B))
        if not f:                                     # (:429-434): two replications, MulCoeffsMontgomeryThenAdd
            rh.rlwe._check(L.rh_rlwe_ring_merge(rq._h, level, odd.Value[0].ptr, odd.Value[1].ptr, None, None, None, t1.Value[0].ptr, t1.Value[1].ptr, 1, B))
            for c in (0, 1):
                rq.MulCoeffsMontgomeryThenAdd(t1.Value[c], x0, t0.Value[c])
    results.append(compare("ring split, the kernel alone (64 ciphertexts) against X^-1, a second INTT and two strided copies", split_kernel, 5, 5))
    results.append(compare("ring merge, the kernel alone (64 ciphertexts) against two replications and MulCoeffsMontgomeryThenAdd", merge_kernel, 5, 5))
    del big, tmp, rot, u, batch, ctN, even, odd, t0, t1, xrep, xprep, xinv0, x0, lo, hi
    ev._xrep.clear()
    ev.close()
    # ---- a small ring, full expansion ----
    logN, LQ, LP = 12, 4, 2
    N, Q, rings, ev, mk, key = setup(logN, LQ, LP, False)
    shapes["small"] = {"N": N, "limbs_Q": LQ, "limbs_P": LP, "outputs": N, "logGap": 0}
    ct = mk(logN, 1)
    results.append(compare("Expand, full expansion to 4096 outputs, N = 2^12", lambda f: ev.Expand(ct, 0, fused=f), 5, 3))
    results.append(compare("Expand, full expansion, N = 2^12: batched levels against one launch sequence per ciphertext",
                           lambda f: ev.Expand(ct, 0, fused=True) if f else expand_per_ciphertext(ev, ct, 0), 3, 1, labels=("batched", "per_ciphertext")))
    batch = mk(logN, N)
    results.append(compare("Pack of 4096 ciphertexts, N = 2^12", lambda f: ev.Pack(batch, list(range(N)), logN, True, fused=f), 3, 1,
                           {"note": "composed: one launch per ciphertext and pass around the level's one key switch, as the reference's loop issues them"}))
    ev.close()
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shapes": shapes,
           "method": "alternating windows (counts per entry), device events, 1 warm-up call per window; clocks left to the driver's default governor",
           "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))


def polynomial_group(out_path):
    """N = 2^16, 16 limbs of Q (GenModuli [55] + [45] * 15, scale 2^45: the regime the reference's own test runs in), 4 of P, batches of 1 and 64.
    The baby step: EvaluatePolynomialVectorFromPowerBasis of a degree-K polynomial on a synthetic power basis of K degree-1 powers at the target
    level, K = 7, 15, 31 -- one rh_ckks_linear_combination (fused=True) against the Add and K MulThenAdd calls of the composed path, which is the
    baseline, timed HERE, alternating with the fused one.  Rows moved per component and limb: K + 1 against 3 K (the first MulThenAdd included,
    the zeroing of the accumulator not).  Then the whole Evaluate of a degree-K polynomial (the powers, K's baby steps, the giant steps with their
    relinearisations and rescalings), where the baby steps are a small share.  Every window repeats one evaluation, so the evaluator's memo of the
    host scalars (ckks.Evaluator._rns_scalar) is warm on both sides: the figures are the steady state of a circuit that is evaluated again and again.  Medians of `rounds` windows; `fused_default` as in ckks_group."""
    import statistics
    from oracle import primes
    N, LQ, LP, rounds = 1 << 16, 16, 4, 5
    Qg, Pg = primes.gen_moduli(17, [55] + [45] * (LQ - 1), [61] * LP)
    Q, P = [int(q) for q in Qg], [int(p) for p in Pg]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    digits = (LQ + LP - 1) // LP
    evq, evp = rand_block(2 * digits, Q, N), rand_block(2 * digits, P, N)
    rlk = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
    rlk.digits, rlk.levelQ, rlk.levelP, rlk.BaseTwoDecomposition, rlk.digits_per_limb = digits, LQ - 1, LP - 1, 0, None
    rlk.Q, rlk.P = rh.DevicePoly.from_torch(rq, evq), rh.DevicePoly.from_torch(rp, evp)
    evs = {f: rh.ckks.Evaluator(rq, rp, rlk=rlk) for f in (True, False)}          # every other kernel by its measured default on both sides
    for f, ev in evs.items():
        ev.fused["linear_combination"] = f
    pes = {f: rh.polynomial.PolynomialEvaluator(evs[f]) for f in (True, False)}
    Pm, Sc = rh.polynomial, rh.ckks.Scale
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    rng = np.random.default_rng(7)
    results = []

    def record(name, B, K, fn, reps, extra, warm=2):
        outs = [fn(f) for f in (True, False)]                           # same bits first, at the shape that is timed
        same = all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(outs[0].Value, outs[1].Value)) and outs[0].Scale.Value == outs[1].Scale.Value
        assert same, "fused and composed differ: %s B=%d K=%d" % (name, B, K)
        del outs
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), reps=reps, warm=warm)); tc.append(timed(lambda: fn(False), reps=reps, warm=warm))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        e = {"op": name, "batch": B, "K": K, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
             "composed_run_to_run_spread_ms": spread, "fused_default": bool(f["ms_median"] <= c["ms_median"] + spread)}
        e.update(extra(f, c))
        results.append(e)
        print(json.dumps(e), flush=True)

    for B in (1, 64):
        for K in (7, 15, 31):
            co = [complex(a, b) for a, b in rng.uniform(-1, 1, (K + 1, 2))]
            pol = Pm.PolynomialVector([Pm.Polynomial(Pm.Monomial, co)])
            # ---- the baby step: K powers at the target level, scales below the target scale
            first = rh.Ciphertext([rh.DevicePoly.from_torch(rq, rand_block(B, Q, N)) for _ in range(2)], is_ntt=True)
            first.Scale = Sc(2 ** 45)
            pb = Pm.PowerBasis(first, Pm.Monomial)
            for k in range(2, K + 1):
                pb.Value[k] = rh.Ciphertext([rh.DevicePoly.from_torch(rq, rand_block(B, Q, N)) for _ in range(2)], is_ntt=True)
                pb.Value[k].Scale = Sc(2 ** 45 + k)
            target = Sc(2 ** 45).Mul(Sc(Q[LQ - 1]))
            row_bytes = 8.0 * N * LQ * B * 2                            # one row of every limb, both components

            def bw(f, c, K=K, row_bytes=row_bytes):
                f["algorithmic_GBps"] = round((K + 1) * row_bytes / (f["ms_median"] * 1e-3) / 1e9, 1)
                f["frac_of_8TBps"] = round(f["algorithmic_GBps"] / PEAK, 3)
                c["algorithmic_GBps"] = round(3 * K * row_bytes / (c["ms_median"] * 1e-3) / 1e9, 1)
                return {"rows_fused": K + 1, "rows_composed": 3 * K}
            record("baby step: EvaluatePolynomialVectorFromPowerBasis", B, K,
                   lambda f: pes[f].EvaluatePolynomialVectorFromPowerBasis(LQ - 1, pol, pb, target), 10 if B == 1 else 5, bw)
            del pb, first
            torch.cuda.empty_cache()
            # ---- the whole Evaluate
            ct = rh.Ciphertext([rh.DevicePoly.from_torch(rq, rand_block(B, Q, N)) for _ in range(2)], is_ntt=True)
            ct.Scale = Sc(2 ** 45)
            record("Evaluate", B, K, lambda f: pes[f].Evaluate(ct, pol.Value[0], 2 ** 45), 5 if B == 1 else 2, lambda f, c: {}, warm=1)
            del ct
            torch.cuda.empty_cache()
    from bench import csrc_tree_hash
    baby64 = [e for e in results if e["op"].startswith("baby") and e["batch"] == 64]
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batches": [1, 64], "K": [7, 15, 31]},
           "method": "%d alternating windows per case, device events, 2 warm-up calls per window (1 for Evaluate); clocks left to the driver's default governor" % rounds,
           "linear_combination_default": bool(all(e["fused_default"] for e in baby64)),
           "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    for ev in evs.values():
        ev.close()
    rq.close(); rp.close()


def lintrans_group(out_path):
    """The config 5 ring of ckks_group: N = 2^16, 24 limbs of Qi60, 6 of Pi60, batches of 1 and 8 ciphertexts.  lintrans.Evaluator.Evaluate of the
    reference test's nine diagonals with BSGS ratio 1, of a dense 64-diagonal matrix (ratio 1) and of the nine diagonals without BSGS; each of the
    three kernels of csrc/lintrans.hip alone against the ring calls it replaces, and inside the whole Evaluate (that kernel fused, the other passes
    composed) against the composed Evaluate.  Both sides are timed HERE, in alternating windows, as in inner_sum_group; `fused_default` is the rule
    lintrans.Evaluator.FUSED_LINTRANS follows: the fused median within the composed windows' max - min of the composed median, or below it, alone
    AND in the whole call, at every batch.  Diagonals and keys hold uniform residues: the passes do not look at values."""
    import statistics
    N, LQ, LP, rounds, reps = 1 << 16, 24, 6, 5, 3
    Q, P = QI60[:LQ], PI60[:LP]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    digits = (LQ + LP - 1) // LP
    level, levelP = LQ - 1, LP - 1
    log_slots = 15
    slots = 1 << log_slots
    lt_ = rh.lintrans

    def key():
        k = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
        k.digits, k.levelQ, k.levelP, k.BaseTwoDecomposition, k.digits_per_limb = digits, level, levelP, 0, None
        k.Q, k.P = rh.DevicePoly.from_torch(rq, rand_block(2 * digits, Q, N)), rh.DevicePoly.from_torch(rp, rand_block(2 * digits, P, N))
        return k

    def transformation(diags, ratio):
        lt = lt_.NewTransformation(rq, rp, lt_.Parameters(diags, level, levelP, 1 << 40, log_slots, ratio))
        for k in lt.Vec:
            lt.Vec[k] = rh.rlwe.PolyQP(rh.DevicePoly.from_torch(rq, rand_block(1, Q, N)), rh.DevicePoly.from_torch(rp, rand_block(1, P, N)))
        return lt
    nine = [-15, -4, -1, 0, 1, 2, 3, 4, 15]
    lts = {"nine diagonals, BSGS ratio 1": transformation(nine, 1), "dense 64 diagonals, BSGS ratio 1": transformation(list(range(64)), 1),
           "nine diagonals, no BSGS": transformation(nine, -1)}
    galEls = sorted({g for lt in lts.values() for g in lt.GaloisElements(N) if g != 1})
    cev = rh.ckks.Evaluator(rq, rp, galois_keys={g: key() for g in galEls})
    lev = lt_.Evaluator(cev)
    ks = cev.ks
    g = rh.rlwe.GaloisElement(N, 8)
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    results = []

    def measure(name, B, fn, kernel, reps=reps):
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), reps=reps)); tc.append(timed(lambda: fn(False), reps=reps))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        results.append({"op": name, "batch": B, "kernel": kernel, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
                        "composed_run_to_run_spread_ms": spread, "fused_default": bool(f["ms_median"] <= c["ms_median"] + spread)})
    for B in (1, 8):
        mkq = lambda n=B: rh.DevicePoly.from_torch(rq, rand_block(n, Q, N))
        mkp = lambda n=B: rh.DevicePoly.from_torch(rp, rand_block(n, P, N))
        ct, out = rh.Ciphertext([mkq(), mkq()], is_ntt=True), rh.Ciphertext([mkq(), mkq()], is_ntt=True)
        ct.Scale = rh.ckks.Scale(1 << 40)
        qp = lambda: rh.rlwe.ElementQP([rh.rlwe.PolyQP(mkq(), mkp()), rh.rlwe.PolyQP(mkq(), mkp())])
        tmp, acc, cqp, rot = qp(), qp(), qp(), qp()
        pct = rh.Ciphertext([mkq(), mkq()], is_ntt=True)
        pres = [qp() for _ in range(3)]
        rql, rpl = rq.AtLevel(level), rp.AtLevel(levelP)
        for name, lt in lts.items():                      # same bits first, at the timed shape
            res = []
            for fused in (True, False):
                lev.Evaluate(ct, lt, out, fused=fused)
                res.append([v.numpy() for v in out.Value])
            assert all(np.array_equal(x, y) for x, y in zip(*res)), "fused and composed Evaluate differ: " + name
            del res
        pts = list(lts["dense 64 diagonals, BSGS ratio 1"].Vec.values())
        for K in (5, 8):                                  # the baby steps of one giant step: the nine diagonals' longest, the dense matrix's
            terms = [(pts[0], None)] + [(pts[k], pres[k % 3]) for k in range(1, K)]
            measure("baby-step sum of %d terms, the kernel alone" % K, B,
                    lambda f: lev._diag_mac(level, levelP, terms, pct, tmp, B) if f else lev._diag_mac_composed(rql, rpl, terms, pct, tmp), "diag_mac", reps=30)

        def tail(f):
            if f:
                rh.ringhip._check(rh.lib().rh_rlwe_rotate_sum_accumulate_qp(ks.be._h, level, levelP, g, cqp.Value[0].Q.ptr, cqp.Value[1].Q.ptr, cqp.Value[0].P.ptr,
                                  cqp.Value[1].P.ptr, tmp.Value[0].Q.ptr, tmp.Value[0].P.ptr, acc.Value[0].Q.ptr, acc.Value[1].Q.ptr, acc.Value[0].P.ptr, acc.Value[1].P.ptr, B, 0))
                return
            rql.Add(cqp.Value[0].Q, tmp.Value[0].Q, cqp.Value[0].Q); rpl.Add(cqp.Value[0].P, tmp.Value[0].P, cqp.Value[0].P)
            for c in (0, 1):
                rql.AutomorphismNTT(cqp.Value[c].Q, g, rot.Value[c].Q); rpl.AutomorphismNTT(cqp.Value[c].P, g, rot.Value[c].P)
                rql.Add(acc.Value[c].Q, rot.Value[c].Q, acc.Value[c].Q); rpl.Add(acc.Value[c].P, rot.Value[c].P, acc.Value[c].P)
        measure("giant-step tail, the kernel alone", B, tail, "giant_tail", reps=50)
        Pbig = 1
        for p in P:
            Pbig *= int(p)
        ct0P = mkq()
        pt = pts[1]

        def step(f):
            if f:
                rh.ringhip._check(rh.lib().rh_rlwe_rotate_mul_accumulate_qp(ks.be._h, level, levelP, g, pt.Q.ptr, pt.P.ptr, ct.Value[0].ptr, cqp.Value[0].Q.ptr, cqp.Value[1].Q.ptr,
                                  cqp.Value[0].P.ptr, cqp.Value[1].P.ptr, acc.Value[0].Q.ptr, acc.Value[1].Q.ptr, acc.Value[0].P.ptr, acc.Value[1].P.ptr, B, 0))
                return
            rql.Add(cqp.Value[0].Q, ct0P, cqp.Value[0].Q)     # P ct0 is formed once per call, outside the step
            for c in (0, 1):
                rql.AutomorphismNTT(cqp.Value[c].Q, g, rot.Value[c].Q); rpl.AutomorphismNTT(cqp.Value[c].P, g, rot.Value[c].P)
                lev._mul_diag(rql, pt.Q, rot.Value[c].Q, acc.Value[c].Q, False); lev._mul_diag(rpl, pt.P, rot.Value[c].P, acc.Value[c].P, False)
        measure("one diagonal without BSGS, the kernel alone", B, step, "naive_step", reps=50)
        for name, lt in lts.items():
            for kernel in (("naive_step",) if lt.N1 == 0 else ("diag_mac", "giant_tail")):
                measure("Evaluate, %s, %s fused" % (name, kernel), B, lambda f: lev.Evaluate(ct, lt, out, fused={k: f and k == kernel for k in lev.FUSED_LINTRANS}), kernel)
            measure("Evaluate, %s, every kernel fused" % name, B, lambda f: lev.Evaluate(ct, lt, out, fused=f), "all")
    defaults = {k: bool(all(e["fused_default"] for e in results if e["kernel"] == k)) for k in lt_.Evaluator.FUSED_LINTRANS}
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batches": [1, 8], "slots": slots},
           "method": "%d alternating windows of %d calls each (30 to 50 for a kernel alone), device events, 2 warm-up calls per window; clocks left to the "
                     "driver's default governor" % (rounds, reps),
           "fused_lintrans_default": defaults, "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    cev.close()
    rq.close(); rp.close()


def dft_group(out_path):
    """The config 5 ring of lintrans_group: N = 2^16, 24 limbs of Qi60, 6 of Pi60; LogSlots 15 (full packing), CoeffsToSlots with Levels [1,1,1,1] and
    SlotsToCoeffs with Levels [1,1,1] (16 + 31 + 31 + 15 and 63 + 63 + 32 diagonals of 32768 values), RepackImagAsReal, BSGS ratio 0, batches of 1 and 8.
    (a) NewMatrixFromLiteral's two halves on the device -- the diagonals generated in HBM, one Embed per factor -- against numpy diagonals generated on
    the host and pushed through the per-diagonal lintrans.Encode; host wall clock, the device drained before and after, best of 3.  (b) each kernel of
    dft.Evaluator.FUSED_DFT alone against the evaluator calls it replaces, and inside the whole circuit; (c) the whole circuits per ciphertext.  Both
    sides of (b) and (c) are timed HERE in alternating windows, as in lintrans_group, whose rule `fused_default` follows.  Keys hold uniform residues."""
    import statistics
    N, LQ, LP, rounds, reps = 1 << 16, 24, 6, 5, 3
    Q, P = QI60[:LQ], PI60[:LP]
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    digits = (LQ + LP - 1) // LP
    level, levelP, ls = LQ - 1, LP - 1, 15
    D, lt_ = rh.dft, rh.lintrans
    ecd = rh.ckks.Encoder(rq, ringP=rp)
    lits = {"CoeffsToSlots": D.MatrixLiteral(D.HomomorphicEncode, ls, level, levelP, [1, 1, 1, 1], D.RepackImagAsReal),
            "SlotsToCoeffs": D.MatrixLiteral(D.HomomorphicDecode, ls, level, levelP, [1, 1, 1], D.RepackImagAsReal)}

    def wall(fn):
        best, keep = None, None
        for _ in range(3):
            keep = None
            torch.cuda.synchronize(); t0 = time.perf_counter()
            keep = fn()
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
            best = ms if best is None else min(best, ms)
        return round(best, 3), keep

    def host_encode(lit, diags):
        out = []
        for i, dg in enumerate(diags):
            lt = lt_.NewTransformation(rq, rp, lt_.Parameters(sorted(dg), level, levelP, Q[level - i], ls, lit.LogBSGSRatio))
            lt_.Encode(ecd, dg, lt)
            out.append(lt)
        return out

    def device_encode(lit, blocks):
        return [lt_.NewTransformationFromBlock(rq, rp, lt_.Parameters(b.Index, level, levelP, Q[level - i], ls, lit.LogBSGSRatio), ecd, b.Index, b.Block)
                for i, b in enumerate(blocks)]
    generation, mats = [], {}
    for name, lit in lits.items():
        rots = lambda f, index: D._bsgs_rotations(index, 1 << ls, lit.LogBSGSRatio)
        gen_dev, blocks = wall(lambda: D._gen_device(lit, 16, None, rq, rots))
        enc_dev, dev_lts = wall(lambda: device_encode(lit, blocks))
        gen_host, diags = wall(lambda: lit.GenMatrices(16, device=False))
        enc_host, host_lts = wall(lambda: host_encode(lit, diags))
        k = sorted(dev_lts[0].Vec)[1]                          # same bits, at the timed shape: one diagonal of the first factor
        assert np.array_equal(dev_lts[0].Vec[k].Q.numpy(), host_lts[0].Vec[k].Q.numpy()) and np.array_equal(dev_lts[0].Vec[k].P.numpy(), host_lts[0].Vec[k].P.numpy())
        generation.append({"matrix": name, "factors": len(blocks), "diagonals": [len(b.Index) for b in blocks],
                           "device": {"generate_ms": gen_dev, "encode_ms": enc_dev}, "host_per_diagonal": {"generate_ms": gen_host, "encode_ms": enc_host},
                           "ratio_host_over_device": {"generate": round(gen_host / gen_dev, 2), "encode": round(enc_host / enc_dev, 2),
                                                      "both": round((gen_host + enc_host) / (gen_dev + enc_dev), 2)}})
        del blocks, diags, host_lts, dev_lts
        mats[name] = D.NewMatrixFromLiteral(rq, rp, lit, ecd)

    def key():
        k = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
        k.digits, k.levelQ, k.levelP, k.BaseTwoDecomposition, k.digits_per_limb = digits, level, levelP, 0, None
        k.Q, k.P = rh.DevicePoly.from_torch(rq, rand_block(2 * digits, Q, N)), rh.DevicePoly.from_torch(rp, rand_block(2 * digits, P, N))
        return k
    galEls = sorted({g for lit in lits.values() for g in lit.GaloisElements(N) if g != 1} | {2 * N - 1})
    cev = rh.ckks.Evaluator(rq, rp, galois_keys={g: key() for g in galEls})
    dev = D.Evaluator(cev)
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    results = []

    def measure(name, B, fn, kernel, reps=reps):
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), reps=reps)); tc.append(timed(lambda: fn(False), reps=reps))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        results.append({"op": name, "batch": B, "kernel": kernel, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
                        "fused_ms_per_ciphertext": round(f["ms_median"] / B, 4), "composed_ms_per_ciphertext": round(c["ms_median"] / B, 4),
                        "composed_run_to_run_spread_ms": spread, "fused_default": bool(f["ms_median"] <= c["ms_median"] + spread)})
    for B in (1, 8):
        def new(lv=level):
            ct = rh.Ciphertext([rh.DevicePoly.from_torch(rq.AtLevel(lv), rand_block(B, Q[:lv + 1], N)) for _ in (0, 1)], is_ntt=True)
            ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << 40), ls
            return ct
        ct, re, im, out = new(), new(), new(), new()
        res = []
        for fused in (True, False):                            # same bits first, at the timed shape
            r, i = dev.CoeffsToSlotsNew(ct, mats["CoeffsToSlots"], fused=fused)
            o = dev.SlotsToCoeffsNew(re, im, mats["SlotsToCoeffs"], fused=fused)
            res.append([v.numpy() for x in (r, i, o) for v in x.Value])
        assert all(np.array_equal(x, y) for x, y in zip(*res)), "fused and composed circuits differ"
        del res, r, i, o
        low = level - 4                                        # the split runs after four rescalings, the merge at LevelQ
        z, zc, tmp = new(low), new(low), new(low)

        def split(f):
            dev._split(z, zc, tmp, f)
        measure("real / imaginary split at level %d, the kernel alone" % low, B, split, "split", reps=50)
        measure("real / imaginary merge at level %d, the kernel alone" % level, B, lambda f: dev._merge_parts(re, im, out, f), "merge", reps=50)
        cre, cim = new(), new()
        measure("CoeffsToSlots, Levels [1,1,1,1]", B, lambda f: dev.CoeffsToSlots(ct, mats["CoeffsToSlots"], cre, cim, fused=f), "split")
        measure("SlotsToCoeffs, Levels [1,1,1]", B, lambda f: dev.SlotsToCoeffs(re, im, mats["SlotsToCoeffs"], out, fused=f), "merge")
    defaults = {k: bool(all(e["fused_default"] for e in results if e["kernel"] == k)) for k in D.Evaluator.FUSED_DFT}
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "batches": [1, 8], "log_slots": ls},
           "method": "circuits and kernels: %d alternating windows of %d calls each (50 for a kernel alone), device events, 2 warm-up calls per window; "
                     "matrix generation and encoding: host wall clock around one call, the device drained before and after, best of 3; clocks left to the "
                     "driver's default governor" % (rounds, reps),
           "matrix_generation": generation, "fused_dft_default": defaults, "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    ecd.close(); cev.close()
    rq.close(); rp.close()


def bootstrap_group(out_path):
    """CKKS bootstrapping at the N16QP1546H192H32 chain shape: N = 2^16, 10 residual + 3 (SlotsToCoeffs, 39 bits) + 8 (EvalMod, 60) + 4 (CoeffsToSlots, 56)
    limbs of Q and 5 of P, scale 2^40, LogSlots 15, CosDiscrete K = 16 / degree 30 / r = 3, sparse-secret encapsulation; batches of 1 and 8.
    (a) rh_ckks_bootstrap_modup alone, dense and encapsulated, without and with the folded scalar, as bytes per second against its WRITE volume;
    (b) the lift, the transforms and the message scaling with the scalar folded into the kernel against MulScalar after the NTT;
    (c) EvalMod alone (on 2 B ciphertexts: ctReal and ctImag as one batch) with rh_ckks_double_angle against the two Adds;
    (d) the whole Evaluate split by stage, FUSED_BOOTSTRAP on and off.  Both sides of (b), (c), (d) are timed HERE in alternating windows.
    Keys and ciphertexts hold uniform residues: the timings do not depend on the values."""
    import statistics
    from oracle import primes
    N, ls, rounds, reps = 1 << 16, 15, 3, 3
    Q, P = primes.gen_moduli(17, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    LQ, LP = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    rq0, rp0 = rh.Ring(N, Q[:1]), rh.Ring(N, P[:1]); rq0.set_stream(stream.cuda_stream); rp0.set_stream(stream.cuda_stream)
    B_, D, M = rh.bootstrapping, rh.dft, rh.mod1
    res_level, s2c_level, mod1_level, top = 9, 12, 20, 24
    digits = (LQ + LP - 1) // LP

    def key(ringq=rq, ringp=rp, mq=Q, mp=P, rows=digits):
        k = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
        k.digits, k.levelQ, k.levelP, k.BaseTwoDecomposition, k.digits_per_limb = rows, len(mq) - 1, len(mp) - 1, 0, None
        k.Q, k.P = rh.DevicePoly.from_torch(ringq, rand_block(2 * rows, mq, N)), rh.DevicePoly.from_torch(ringp, rand_block(2 * rows, mp, N))
        return k
    s2c = D.MatrixLiteral(D.HomomorphicDecode, ls, s2c_level, LP - 1, [1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    c2s = D.MatrixLiteral(D.HomomorphicEncode, ls, top, LP - 1, [1, 1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    m1 = M.ParametersLiteral(LevelQ=mod1_level, LogScale=60, Mod1Type=M.CosDiscrete, LogMessageRatio=8, K=16, Mod1Degree=30, DoubleAngle=3)
    params = B_.Parameters(rq, rp, res_level, 1 << 40, s2c, m1, c2s, EphemeralSecretWeight=32)
    keys = B_.EvaluationKeys(key(), {g: key() for g in params.GaloisElements() if g != 1}, key(rq0, rp0, Q[:1], P[:1], 1), key())
    evs = {f: B_.Evaluator(params, keys, fused=f) for f in (True, False)}
    stat = lambda v: {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    kernel, results = [], []

    def measure(name, B, fn, choice, reps=reps):
        """choice: the FUSED_BOOTSTRAP key the two sides differ in, or None where both run the same code (a stage the flags do not reach: its two
        columns are two samples of one thing).  A side whose slowest window is more than 1.5 times its fastest is marked bimodal; a row decides a
        default only when it has a choice and neither side is bimodal, else the row says why not."""
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), reps=reps)); tc.append(timed(lambda: fn(False), reps=reps))
        f, c = stat(tf), stat(tc)
        spread = round(c["ms_max"] - c["ms_min"], 4)
        bimodal = [side for side, v in (("fused", f), ("composed", c)) if v["ms_max"] > 1.5 * v["ms_min"]]
        e = {"op": name, "batch": B, "choice": choice, "fused": f, "composed": c, "fused_ms_per_ciphertext": round(f["ms_median"] / B, 4),
             "composed_ms_per_ciphertext": round(c["ms_median"] / B, 4), "composed_run_to_run_spread_ms": spread, "bimodal_windows": bimodal}
        if choice is not None:
            e["ratio_composed_over_fused"] = round(c["ms_median"] / f["ms_median"], 3)
            if bimodal:
                e["fused_default"] = None
                e["undecided"] = "windows of one side differ by more than 1.5x: the medians do not decide"
            else:
                e["fused_default"] = bool(f["ms_median"] <= c["ms_median"] + spread)
                e["difference_within_spread"] = bool(abs(f["ms_median"] - c["ms_median"]) <= spread)
        results.append(e)
    scalar = (1 << 20) + 12345
    for B in (1, 8, 48):                                          # 48: 1.26 / 1.38 GB written per call, beyond the 256 MiB Infinity Cache and the 512 MiB non-temporal threshold; the kernel alone
        blk = lambda ring, mods: rh.DevicePoly.from_torch(ring, rand_block(B, mods, N))
        i0, i1 = blk(rq.AtLevel(0), Q[:1]), blk(rq.AtLevel(0), Q[:1])
        o0, o1, eQ, eP = rq.NewPoly(B), rq.NewPoly(B), rq.NewPoly(B), rp.NewPoly(B)
        for arm, call, rows in (("dense", lambda sc: B_.modup_lift(rq, None, LQ - 1, 0, i0, i1, o0, o1, scalar=sc), 2 * LQ),
                                ("encapsulated", lambda sc: B_.modup_lift(rq, rp, LQ - 1, LP - 1, i0, i1, o0, c1Q=eQ, c1P=eP, scalar=sc), 2 * LQ + LP)):
            for sc in (None, scalar):
                ms = timed(lambda: call(sc), reps=50)
                wr = 8.0 * N * B * rows
                e = {"op": "rh_ckks_bootstrap_modup, %s%s" % (arm, ", scalar folded" if sc else ""), "batch": B, "ms": round(ms, 4), "bytes_written": wr,
                     "bytes_read": 16.0 * N * B, "write_GBps": round(wr / (ms * 1e-3) / 1e9, 1)}
                if wr > (512 << 20):                            # only there is the store rate a rate of HBM: below, the 50 calls of a window rewrite blocks the Infinity Cache holds
                    e["frac_of_8TBps_hbm"] = round(wr / (ms * 1e-3) / 1e9 / PEAK, 3)
                else:
                    e["note"] = "the blocks written fit the 256 MiB Infinity Cache and the window rewrites them: a cache-assisted store rate, not a share of HBM peak"
                kernel.append(e)
        if B > 8:
            del i0, i1, o0, o1, eQ, eP
            continue

        def lift_and_scale(fold):                               # the encapsulated arm's lift, three transforms and the scaling (:703-750)
            B_.modup_lift(rq, rp, LQ - 1, LP - 1, i0, i1, o0, c1Q=eQ, c1P=eP, scalar=scalar if fold else None)
            rq.NTT(eQ, eQ); rp.NTT(eP, eP); rq.NTT(o0, o0)
            if not fold:
                rq.MulScalar(eQ, scalar, eQ); rp.MulScalar(eP, scalar, eP); rq.MulScalar(o0, scalar, o0)
        measure("ModUp's lift, transforms and message scaling (encapsulated arm, scalar forced)", B, lift_and_scale, "modup_scale", reps=20)
        ct = rh.Ciphertext([i0, i1], is_ntt=True)
        ct.Scale, ct.LogDimensions = rh.ckks.Scale(1 << 40), ls
        st = {}
        for f in (True, False):                                 # same bits first, at the timed shape
            ev = evs[f]
            down, _ = ev.ScaleDown(ct)
            up = ev.ModUp(down)
            re, im = ev.CoeffsToSlots(up)
            a, b = ev._eval_mod_pair(re, im)
            out = ev.SlotsToCoeffs(a, b)
            st[f] = (down, up, re, im, a, b, out)
        assert all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(st[True][-1].Value, st[False][-1].Value)), "FUSED_BOOTSTRAP on and off differ"
        down, up, re, im, a, b, out = st[True]
        measure("EvalMod alone on ctReal and ctImag as one batch (2 B ciphertexts)", B, lambda f: evs[f]._eval_mod_pair(re, im), "double_angle")
        measure("Evaluate: ScaleDown", B, lambda f: evs[f].ScaleDown(ct), None)
        applies = (evs[True].Mod1Parameters.ScalingFactor().Float64() / evs[True].Mod1Parameters.MessageRatio()) / down.Scale.Float64() > 1     # :735
        measure("Evaluate: ModUp (key switches, lift, Trace)%s" % ("" if applies else "; no message scalar in this setting: both sides run the same code"), B,
                lambda f: evs[f].ModUp(down), "modup_scale" if applies else None)
        measure("Evaluate: CoeffsToSlots", B, lambda f: evs[f].CoeffsToSlots(up), None)
        measure("Evaluate: EvalMod", B, lambda f: evs[f]._eval_mod_pair(re, im), "double_angle")
        measure("Evaluate: SlotsToCoeffs", B, lambda f: evs[f].SlotsToCoeffs(a, b), None)
        measure("Evaluate, whole", B, lambda f: evs[f].Evaluate(ct), None, reps=2)
        del st
    # a default follows the rows that decide (a choice, no bimodal side): the kernel unless one of them finds it slower beyond the spread
    deciding = {k: [e for e in results if e["choice"] == k and e.get("fused_default") is not None] for k in M.Evaluator.FUSED_BOOTSTRAP}
    defaults = {k: bool(all(e["fused_default"] for e in v)) for k, v in deciding.items()}
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(),
           "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "log_q": [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, "batches": [1, 8], "kernel_alone_batches": [1, 8, 48], "log_slots": ls,
                     "message_scalar_of_the_setting": "about 1: EvalMod's scale 2^60 / MessageRatio is Q0 / MessageRatio, so ModUp of this chain multiplies by no scalar; (b) forces one"},
           "method": "%d alternating windows of %d calls each (50 for the kernel alone, 20 for (b), 2 for the whole Evaluate), device events, 2 warm-up calls per "
                     "window; clocks left to the driver's default governor" % (rounds, reps),
           "modup_kernel": kernel, "fused_bootstrap_default": defaults,
           "fused_bootstrap_default_rests_on": {k: [(e["op"], e["batch"]) for e in v] for k, v in deciding.items()}, "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    for ev in evs.values():
        ev.close()
    for r in (rq, rp, rq0, rp0):
        r.close()


def _wall_ms(fn, sync, reps, warm=1):
    """host wall clock around `reps` calls, the device drained before and after: what a caller waits for"""
    for _ in range(warm):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) * 1e3 / reps


def _random_gadget(rng, rq, q, N, rows, pw2):
    return rh.rlwe.GadgetCiphertext(rq, None, rng.integers(0, q, size=(rows, 2, 1, N), dtype=np.uint64), None, BaseTwoDecomposition=pw2, digits_per_limb=[rows])


def blindrot_baseline(out_path):
    """One rgsw ExternalProduct and one key-switched automorphism (GadgetProduct, Add, two AutomorphismNTT) on ONE ciphertext at N = 2^10, one
    55-bit modulus, no P, pw2 = 14: the launch-per-ring-call cost of one step of a blind rotation, through calls the commit before the kernel has."""
    N, q, pw2, rows = 1024, 0x7ffffffffb4001, 14, 4
    rng = np.random.default_rng(1)
    rq = rh.Ring(N, [q])
    ev = rh.rgsw.Evaluator(rq, None)
    rgsw = rh.rgsw.Ciphertext(_random_gadget(rng, rq, q, N, rows, pw2), _random_gadget(rng, rq, q, N, rows, pw2))
    gk = _random_gadget(rng, rq, q, N, rows, pw2)
    new = lambda: rh.DevicePoly.from_numpy(rq, rng.integers(0, q, size=(1, 1, N), dtype=np.uint64))
    ct, tmp = rh.Ciphertext([new(), new()], is_ntt=True), rh.Ciphertext([new(), new()], is_ntt=True)

    def auto():
        ev.GadgetProduct(0, ct.Value[1], gk, tmp)
        rq.Add(tmp.Value[0], ct.Value[0], tmp.Value[0])
        rq.AutomorphismNTT(tmp.Value[0], 5, ct.Value[0])
        rq.AutomorphismNTT(tmp.Value[1], 5, ct.Value[1])
    ext_ms = min(_wall_ms(lambda: ev.ExternalProduct(ct, rgsw, ct), rq.sync, 200, warm=20) for _ in range(3))
    auto_ms = min(_wall_ms(auto, rq.sync, 200, warm=20) for _ in range(3))
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": {"N": N, "modulus_bits": 55, "limbs_P": 0, "pw2": pw2, "npoly": 1},
           "method": "host wall clock over 200 back-to-back calls after 20 warm-up calls, device drained before and after, best of 3 windows",
           "external_product_us": round(ext_ms * 1e3, 2), "automorphism_us": round(auto_ms * 1e3, 2)}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    ev.close(); rq.close()


def blindrot_group(out_path, baseline_path=None):
    """The reference test's parameters (core/rgsw/blindrot/blindrot_test.go:53-71): N_BR = 2^10, Q = 0x7fff801, N_LWE = 2^9, pw2 = 7 (4 digits), 512
    RGSW keys and 11 automorphism keys (uniformly random words: timing needs no encryption), accumulators with uniformly random odd a vectors.
    The accumulator loop (Evaluator._run) as one kernel launch against the composed ExternalProduct / Automorphism calls, for 16, 64 and 256
    accumulators; the composed calls walk one accumulator at a time, so they are timed on the first 4 accumulators of each batch."""
    N, q, NL, pw2, rows = 1024, 0x7fff801, 512, 7, 4
    rng = np.random.default_rng(2)
    rq, rl = rh.Ring(N, [q]), rh.Ring(NL, [0x3001])
    ev = rh.blindrot.Evaluator(rq, rl)
    BRK = rh.blindrot.MemBlindRotationEvaluationKeySet(
        [rh.rgsw.Ciphertext(_random_gadget(rng, rq, q, N, rows, pw2), _random_gadget(rng, rq, q, N, rows, pw2)) for _ in range(NL)],
        {g: _random_gadget(rng, rq, q, N, rows, pw2) for g in rh.blindrot.GaloisElements(N)})
    baseline = json.load(open(baseline_path)) if baseline_path else None
    results = []
    for slots in (16, 64, 256):
        a = rng.integers(0, N, size=(slots, NL)) * 2 + 1
        progs = [rh.blindrot.blind_rotate_program([int(x) for x in row], N, ev.galoisGenDiscreteLog) for row in a]
        n_ext = NL
        n_auto = sum(1 for p in progs for kind, _ in p if kind == rh.blindrot.AUTO) / slots
        acc = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, rng.integers(0, q, size=(slots, 1, N), dtype=np.uint64)) for _ in (0, 1)], is_ntt=True)
        fused_ms = min(_wall_ms(lambda: ev._run(progs, acc, BRK, True), rq.sync, 3) for _ in range(3))
        nc = 4
        sub = rh.Ciphertext([rh.rlwe._view(v, 0, nc) for v in acc.Value], is_ntt=True)
        comp_ms = _wall_ms(lambda: ev._run(progs[:nc], sub, BRK, False), rq.sync, 1, warm=1) / nc      # per accumulator
        e = {"accumulators": slots, "ext_steps_per_accumulator": n_ext, "auto_steps_per_accumulator": round(n_auto, 1),
             "fused_ms": round(fused_ms, 3), "fused_accumulators_per_s": round(slots / (fused_ms * 1e-3), 1),
             "fused_us_per_ext_step_of_a_chain": round(fused_ms * 1e3 / n_ext, 3), "fused_us_per_ext_step_of_the_batch": round(fused_ms * 1e3 / (n_ext * slots), 4),
             "composed_ms_per_accumulator": round(comp_ms, 3), "composed_accumulators_per_s": round(1e3 / comp_ms, 2),
             "composed_us_per_ext_step": round(comp_ms * 1e3 / n_ext, 3), "composed_accumulators_timed": nc,
             "fused_over_composed": round((slots / fused_ms) / (1.0 / comp_ms), 1)}
        if baseline:
            proj = (n_ext * baseline["external_product_us"] + n_auto * baseline["automorphism_us"]) * 1e-3
            e["parent_projected_ms_per_accumulator"] = round(proj, 3)
            e["fused_over_parent_projection"] = round((slots / fused_ms) / (1.0 / proj), 1)
        results.append(e)
    from bench import csrc_tree_hash
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(),
           "shape": {"N_BR": N, "Q_BR": hex(q), "N_LWE": NL, "pw2": pw2, "digits": rows, "rgsw_keys": NL, "automorphism_keys": 11},
           "method": "host wall clock around Evaluator._run (program upload, launch and drain included), best of 3 windows of 3 calls for the kernel; one call "
                     "after one warm-up call on 4 accumulators for the composed calls; clocks left to the driver's default governor",
           "parent_commit_baseline": baseline, "fused_blindrot_default": bool(all(e["fused_over_composed"] >= 1.0 for e in results)), "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res, indent=1))
    ev.close(); rq.close(); rl.close()


if sys.argv[1:2] == ["blindrot_baseline"]:
    blindrot_baseline(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "blindrot_baseline.json"))
    sys.exit(0)


if sys.argv[1:2] == ["blindrot"]:
    blindrot_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "blindrot.json"), sys.argv[3] if len(sys.argv) > 3 else None)
    sys.exit(0)


if sys.argv[1:2] == ["bootstrap"]:
    bootstrap_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bootstrap.json"))
    sys.exit(0)

if sys.argv[1:2] == ["dft"]:
    dft_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "dft.json"))
    sys.exit(0)


if sys.argv[1:2] == ["lintrans"]:
    lintrans_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lintrans.json"))
    sys.exit(0)


if sys.argv[1:2] == ["polynomial"]:
    polynomial_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ckks_polynomial.json"))
    sys.exit(0)


if sys.argv[1:2] == ["ring_packing"]:
    ring_packing_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ring_packing.json"))
    sys.exit(0)


if sys.argv[1:2] == ["inner_sum"]:
    inner_sum_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "inner_sum.json"))
    sys.exit(0)


if sys.argv[1:2] == ["bgv_encoder"]:
    bgv_encoder_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bgv_encoder.json"))
    sys.exit(0)


if sys.argv[1:2] == ["ckks_encoder"]:
    ckks_encoder_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ckks_encoder.json"))
    sys.exit(0)


if sys.argv[1:2] == ["ckks"]:
    ckks_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "ckks_ops.json"))
    sys.exit(0)


if sys.argv[1:2] == ["bgv"]:
    bgv_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bgv_ops.json"))
    sys.exit(0)


if sys.argv[1:2] == ["bfv"]:
    bfv_group(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "bfv_ops.json"))
    sys.exit(0)


res = []
# ---- N = 2^16, 16 limbs, batch 512 (4 GiB) ----
N, L, B = 1 << 16, 16, 512
ring = rh.Ring(N, QI60[:L]); ring.set_stream(stream.cuda_stream)
a, b, c = rand_block(B, QI60[:L], N), rand_block(B, QI60[:L], N), rand_block(B, QI60[:L], N)
pa, pb, pc = (rh.DevicePoly.from_torch(ring, t) for t in (a, b, c))
res.append(entry("Ring.NTT N=2^16 L=16", timed(lambda: ring.NTT(pa, pa)), 16.0 * N * L * B, B, "poly"))
res.append(entry("Ring.INTT N=2^16 L=16", timed(lambda: ring.INTT(pa, pa)), 16.0 * N * L * B, B, "poly"))
res.append(entry("Ring.NTTLazy (exact reference representatives) N=2^16 L=16", timed(lambda: ring.NTTLazy(pa, pc)), 16.0 * N * L * B, B, "poly"))
for op, nops in (("ADD", 3), ("MUL_MONT", 3), ("MUL_MONT_THEN_ADD", 4), ("MFORM", 2), ("MUL_BARRETT", 3), ("REDUCE", 2), ("MUL_MONT_LAZY_THEN_ADD_LAZY", 4)):
    res.append(entry("vec " + op + " N=2^16 L=16", timed(lambda: ring.vec_op(op, pa, pb, pc)), 8.0 * nops * N * L * B, B, "poly"))
# rescale (ring/scaling.go): NTT-domain rounded division by the last modulus, 16 -> 15 limbs
po = rh.DevicePoly.from_torch(ring, torch.empty((B, L - 1, N), dtype=torch.int64, device=dev))
res.append(entry("DivRoundByLastModulusNTT N=2^16 L=16->15 (1 INTT + 15 NTT + 2 elementwise passes)",
                 timed(lambda: ring.DivRoundByLastModulusNTT(pa, po), reps=5), 8.0 * N * (2 * (L - 1) + 1) * B + 16.0 * N * L * B, B, "poly"))
# automorphism in the NTT domain (ring/automorphism.go:12-109): an index gather over every limb
res.append(entry("AutomorphismNTT (X -> X^5) N=2^16 L=16", timed(lambda: ring.AutomorphismNTT(pa, 5, pc)), 16.0 * N * L * B, B, "poly"))
del pa, pb, pc, a, b, c, po
ring.close(); torch.cuda.empty_cache()
# conjugate-invariant ring (ring/ntt.go:716-1311): fold + the negacyclic core on the 4N-th-root tables.  QI60 moduli are 1 mod 2^18 = 4N.
ring = rh.Ring(N, QI60[:L], kind=rh.ConjugateInvariant); ring.set_stream(stream.cuda_stream)
a = rand_block(B, QI60[:L], N); pa = rh.DevicePoly.from_torch(ring, a)
res.append(entry("conjugate-invariant Ring.NTT N=2^16 L=16", timed(lambda: ring.NTT(pa, pa)), 16.0 * N * L * B, B, "poly"))
res.append(entry("conjugate-invariant Ring.INTT N=2^16 L=16", timed(lambda: ring.INTT(pa, pa)), 16.0 * N * L * B, B, "poly"))
del pa, a
ring.close(); torch.cuda.empty_cache()

# ---- config 3: N = 2^15, 16 limbs: c = INTT(NTT(a) * NTT(b)) as schemes/ckks/evaluator.go:821-834 sequences it ----
N, L, B = 1 << 15, 16, 512
ring = rh.Ring(N, QI60[:L]); ring.set_stream(stream.cuda_stream)
a, b = rand_block(B, QI60[:L], N), rand_block(B, QI60[:L], N)
pa, pb = rh.DevicePoly.from_torch(ring, a), rh.DevicePoly.from_torch(ring, b)
def polymul():
    ring.NTT(pa, pa); ring.NTT(pb, pb); ring.MForm(pa, pa); ring.MulCoeffsMontgomery(pa, pb, pa); ring.INTT(pa, pa)
ms = timed(polymul, reps=5)
e = entry("config3 poly-mul N=2^15 L=16 (NTT,NTT,MForm,MulCoeffsMontgomery,INTT)", ms, 88.0 * N * L * B, B, "polymul")
e["frac_vs_fused_lower_bound_24NL"] = round(24.0 * N * L * B / (ms * 1e-3) / 1e9 / PEAK, 3)
res.append(e)
def polymul_fused():
    ring.NTT(pa, pa); ring.NTT(pb, pb); ring.INTTMul(pa, pb, pa)
ms = timed(polymul_fused, reps=5)
e = entry("config3 poly-mul N=2^15 L=16, MForm + MulCoeffsMontgomery formed on load by the inverse transform (Ring.INTTMul)", ms, 88.0 * N * L * B, B, "polymul")
e["frac_vs_fused_lower_bound_24NL"] = round(24.0 * N * L * B / (ms * 1e-3) / 1e9 / PEAK, 3)
res.append(e)
def polymul_many():
    ring.NTTMany([(pa, pa), (pb, pb)]); ring.INTTMul(pa, pb, pa)
ms = timed(polymul_many, reps=5)
e = entry("config3 poly-mul N=2^15 L=16, one pipeline through both forward transforms (Ring.NTTMany) + Ring.INTTMul", ms, 88.0 * N * L * B, B, "polymul")
e["frac_vs_fused_lower_bound_24NL"] = round(24.0 * N * L * B / (ms * 1e-3) / 1e9 / PEAK, 3)
res.append(e)
def polymul_tile():
    ring.PolyMul(pa, pb, pa)
ms = timed(polymul_tile, reps=5)
e = entry("config3 poly-mul N=2^15 L=16, Ring.PolyMul: forward tile stages of both operands + product + inverse tile stages as ONE kernel (72 B per coefficient)", ms, 88.0 * N * L * B, B, "polymul")
e["frac_vs_fused_lower_bound_24NL"] = round(24.0 * N * L * B / (ms * 1e-3) / 1e9 / PEAK, 3)
res.append(e)
del pa, pb, a, b
ring.close(); torch.cuda.empty_cache()

# ---- config 5 shapes: N = 2^16, Q = Qi60[0:24], P = Pi60[0:6]: DecomposeAndSplit digit, ModDownQPtoQNTT ----
N, B = 1 << 16, 64
rq, rp = rh.Ring(N, QI60[:24]), rh.Ring(N, PI60[:6]); rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
be = rh.BasisExtender(rq, rp)
xq, xp = rand_block(B, QI60[:24], N), rand_block(B, PI60[:6], N)
oq, op_ = torch.zeros_like(xq), torch.zeros_like(xp)
pq, pp, poq, pop = rh.DevicePoly.from_torch(rq, xq), rh.DevicePoly.from_torch(rp, xp), rh.DevicePoly.from_torch(rq, oq), rh.DevicePoly.from_torch(rp, op_)
res.append(entry("DecomposeAndSplit N=2^16 alpha=6 -> 18 Q + 6 P limbs", timed(lambda: be.DecomposeAndSplit(23, 5, 6, 1, pq, poq, pop), reps=5), 8.0 * N * (6 + 24) * B, B, "poly"))
res.append(entry("ModUpPtoQ N=2^16 6 -> 24 limbs", timed(lambda: be.ModUpPtoQ(5, 23, pp, poq), reps=5), 8.0 * N * (6 + 24) * B, B, "poly"))
res.append(entry("ModDownQPtoQ N=2^16 (24+6) -> 24 limbs", timed(lambda: be.ModDownQPtoQ(23, 5, pq, pp, poq), reps=5), 8.0 * N * (6 + 24 + 24) * B, B, "poly"))
res.append(entry("ModDownQPtoQNTT N=2^16 (24+6) -> 24 limbs", timed(lambda: be.ModDownQPtoQNTT(23, 5, pq, pp, poq), reps=5), 8.0 * N * (6 + 24 + 24) * B + 16.0 * N * 30 * B, B, "poly"))
# config 5: GadgetProduct (key-switch of one ciphertext component), beta = 4 digits, key shared by the batch
beta = 4
evq, evp = rand_block(beta * 2, QI60[:24], N), rand_block(beta * 2, PI60[:6], N)
c0, c1 = torch.zeros_like(xq), torch.zeros_like(xq)
p0, p1 = rh.DevicePoly.from_torch(rq, c0), rh.DevicePoly.from_torch(rq, c1)
ms = timed(lambda: be.GadgetProduct(23, 5, pq, evq.data_ptr(), evp.data_ptr(), beta, p0, p1), reps=3, warm=1)
limb_ntts = 24 + beta * 24 + 2 * 30                      # INTT(cx) + per digit (18 Q + 6 P) + 2 x ModDownNTT (6 INTT + 24 NTT)
e = entry("config5 GadgetProduct N=2^16 Q=24 P=6 beta=4 (per ciphertext component, key shared by batch of %d)" % B, ms,
          16.0 * N * limb_ntts * B + 2.0 * beta * 30 * 8 * N, B, "keyswitch")
e["limb_ntt_equivalents_per_keyswitch"] = limb_ntts
res.append(e)
# CKKS ct x ct multiply with relinearisation, then rescale (schemes/ckks/evaluator.go:786-881, 500-535) at the config 5 parameters
gct = rh.rlwe.GadgetCiphertext.__new__(rh.rlwe.GadgetCiphertext)
gct.digits, gct.levelQ, gct.levelP = beta, 23, 5
gct.Q, gct.P = rh.DevicePoly.from_torch(rq, evq), rh.DevicePoly.from_torch(rp, evp)
cev = rh.ckks.Evaluator(rq, rp, rlk=gct)
mk = lambda: rh.DevicePoly.from_torch(rq, rand_block(B, QI60[:24], N))
ctA, ctB = rh.Ciphertext([mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True)
ctO, ctR = rh.Ciphertext([mk(), mk()], is_ntt=True), rh.Ciphertext([mk(), mk()], is_ntt=True)
def mulrelin_rescale():
    cev.MulRelin(ctA, ctB, ctO, relin=True)
    cev.Rescale(ctO, ctR)
ms = timed(mulrelin_rescale, reps=3, warm=1)
e = entry("CKKS MulRelin + Rescale N=2^16 Q=24 P=6 (tensor, key switch, 2 adds, rescale of both components; batch %d)" % B, ms,
          0.0, B, "ctmul")
e.pop("algorithmic_GBps"); e.pop("frac_of_8TBps")
res.append(e)
# rotations of one ciphertext with a shared decomposition (core/rlwe/evaluator_automorphism.go:62-105): DecomposeNTT once, then per rotation
# GadgetProductHoisted + Add + two NTT-domain automorphisms
gal = 5
kev = rh.rlwe.Evaluator(rq, rp, galois_keys={gal: gct})
dec = kev.DecomposeNTT(23, 5, ctA.Value[1], True)
ms_dec = timed(lambda: kev.DecomposeNTT(23, 5, ctA.Value[1], True, dec), reps=3, warm=1)
ms_rot = timed(lambda: kev.AutomorphismHoisted(23, ctA, dec, gal, ctO), reps=3, warm=1)
e = entry("hoisted rotation N=2^16 Q=24 P=6: DecomposeNTT once (%.3f ms per batch of %d), then per rotation" % (ms_dec, B), ms_rot, 0.0, B, "rotation")
e.pop("algorithmic_GBps"); e.pop("frac_of_8TBps")
res.append(e)
# rotations accumulated modulo QP under ONE ModDown (AutomorphismHoistedLazy, core/rlwe/evaluator_automorphism.go:103-160): the pattern of linear transformations
lz = rh.rlwe.ElementQP.alloc(rq, rp, B, 23, 5)
ms_lazy = timed(lambda: kev.AutomorphismHoistedLazy(23, ctA, dec, gal, lz), reps=3, warm=1)
ms_md = timed(lambda: kev.ModDown(23, 5, lz, ctO), reps=3, warm=1)
e = entry("lazy hoisted rotation N=2^16 Q=24 P=6 (result modulo QP; one ModDown per sum of rotations: %.3f ms per batch of %d)" % (ms_md, B), ms_lazy, 0.0, B, "rotation")
e.pop("algorithmic_GBps"); e.pop("frac_of_8TBps")
res.append(e)
del dec, lz
kev.close()
del ctA, ctB, ctO, ctR, gct
cev.close()
del pq, pp, poq, pop, xq, xp, oq, op_, p0, p1, c0, c1, evq, evp
be.close(); rq.close(); rp.close(); torch.cuda.empty_cache()

# ---- config 2 / 4 rings: 3N transform ----
sys.path.insert(0, os.path.join(ROOT, "tools"))
from primes3n import moduli_3n
for N, L, B in ((3 << 13, 1, 1024), (3 << 16, 24, 16), (3 << 14, 24, 64)):       # config 2; config 4 at both readings of its "logN = 16" (SURVEY 8(d)), the same bytes per batch
    mods = moduli_3n(N, L)
    ring = rh.Ring(N, mods, kind=rh.Matrix3N); ring.set_stream(stream.cuda_stream)
    x = rand_block(B, mods, N)
    px = rh.DevicePoly.from_torch(ring, x)
    res.append(entry("3N NTT N=%d L=%d" % (N, L), timed(lambda: ring.NTT(px, px), reps=5), 16.0 * N * L * B, B, "poly"))
    res.append(entry("3N INTT N=%d L=%d" % (N, L), timed(lambda: ring.INTT(px, px), reps=5), 16.0 * N * L * B, B, "poly"))
    ring.set_tuning("ntt3n_block_order", 1)
    res.append(entry("3N NTT N=%d L=%d, device NTT domain in block order (no permutation pass)" % (N, L), timed(lambda: ring.NTT(px, px), reps=5), 16.0 * N * L * B, B, "poly"))
    res.append(entry("3N INTT N=%d L=%d, block order" % (N, L), timed(lambda: ring.INTT(px, px), reps=5), 16.0 * N * L * B, B, "poly"))
    ring.set_tuning("ntt3n_block_order", 0)
    if L == 24:
        # config 4: matrix_ckks.Evaluator.Mul on degree-1 ciphertexts given in the coefficient domain
        # (schemes/matrix_ckks/evaluator.go:114-192): 4 NTT + 3 MulCoeffsMontgomery + 1 ...ThenAdd + 3 INTT
        blocks = [rh.DevicePoly.from_torch(ring, rand_block(B, mods, N)) for _ in range(7)]
        ct0, ct1 = rh.Ciphertext(blocks[0:2]), rh.Ciphertext(blocks[2:4])
        out = rh.Ciphertext(blocks[4:7])
        ev = rh.MatrixCKKSEvaluator(ring, block_order=False)

        def mul():
            ct0.IsNTT = ct1.IsNTT = False
            ev.Mul(ct0, ct1, out)
        res.append(entry("config4 matrix_ckks Mul N=%d L=%d, reference-order NTT domain (block_order=False)" % (N, L),
                         timed(mul, reps=5), (7 * 16.0 + 3 * 24.0 + 32.0) * N * L * B, B, "ctmul"))
        ev = rh.MatrixCKKSEvaluator(ring)                    # the default since round 3: block order, carried as per-block tags
        res.append(entry("config4 matrix_ckks Mul N=%d L=%d (4 NTT, tensoring, 3 INTT; DEFAULT evaluator: block-order device NTT domain, tagged per block)" % (N, L),
                         timed(mul, reps=5), (7 * 16.0 + 3 * 24.0 + 32.0) * N * L * B, B, "ctmul"))
        ring.ntt3n_layout = None
        del blocks, ct0, ct1, out
    del px, x
    ring.close(); torch.cuda.empty_cache()
print(json.dumps({"device": torch.cuda.get_device_name(0), "results": res}, indent=1))

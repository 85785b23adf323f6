"""The BGV linear transformation's switch, bgv_lintrans.FUSED_BGV_LINTRANS, at N = 2^13 and 2^15, 8 + 2 limbs (LogQ {60, 50 x 7}, LogP {61, 61},
T = 65537: 2 x N/2 slots, no gap), under real keys made on the device: writes profiles/bgv_lintrans.json.

  (a) the encoding of a transformation of 9 diagonals (the reference's list) and of 64 (0 .. 63), BSGS ratio 1 (every diagonal rotated by its
      giant step) and naive (no rotation), onto a transformation allocated once, from host arrays of uint64: ONE EmbedRows (one upload, one
      gather, one inverse transform over T, one lift onto Q and P, the forward transforms) against the reference's per-diagonal path -- the host
      rotation of each row, then Embed into the diagonal's (Q, P) pair, i.e. two rh_bgv_encode calls per diagonal: entries that exist
      without rh_bgv_embed_qp, timed HERE, alternating with the fused side;
  (b) whole Evaluate calls of the 9-diagonal transformation on batches of 1 and 8 ciphertexts, BSGS and naive, with the kernels of
      csrc/lintrans.hip (fused=True, lintrans.Evaluator's measured default) and with the reference's own ring calls: for information, the
      encoding plays no part in them.

The default of "encode" follows (a): fused only where at EVERY shape the windows of the fused side lie entirely below the windows of the
per-diagonal side (max fused < min composed); if the windows of the two sides overlap anywhere, the default stays composed.

Method: a host clock around windows of calls that end in a device synchronise (the per-diagonal side is bound by its host calls and uploads,
which a user pays for), after warm-up calls of the same shape; the calls per window are chosen so that a window lasts about a quarter of a
second; 5 alternating windows per side, the median reported with min and max; both sides give the same bits at the shape that is timed
(asserted).  Usage: python tools/bench_bgv_lintrans.py [OUT.json]"""
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
ROUNDS = 5
WINDOW_S = 0.25
T = 65537
REF_DIAGS = [-15, -4, -1, 0, 1, 2, 3, 4, 15]


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def stat(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main(out_path):
    bl = rh.bgv_lintrans
    results = []

    def record(part, name, logN, extra, fn, same):
        """fn(fused) runs one call and returns its result; same(a, b) compares the two sides' (None: the caller has compared them)"""
        assert same is None or same(fn(True), fn(False)), "fused and composed differ: %s, N = 2^%d %s" % (name, logN, extra)
        fn(True); fn(False)                                               # warm-up of the shape
        reps = max(3, min(400, int(WINDOW_S * 1e3 / max(window(lambda: fn(False), 3), window(lambda: fn(True), 3)))))
        tf, tc = [], []
        for _ in range(ROUNDS):
            tf.append(window(lambda: fn(True), reps)); tc.append(window(lambda: fn(False), reps))
        f, c = stat(tf), stat(tc)
        e = dict({"part": part, "op": name, "logN": logN}, **extra)
        e.update({"fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 3),
                  "windows_overlap": bool(f["ms_max"] >= c["ms_min"]), "windows": ROUNDS, "calls_per_window": reps})
        results.append(e)
        print(json.dumps(e), flush=True)

    shape = {}
    for logN in (13, 15):
        N = 1 << logN
        Q, P = primes.gen_moduli(logN + 1, [60] + [50] * 7, [61, 61])
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        shape = {"limbs_Q": len(Q), "limbs_P": len(P), "T": T}
        rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
        rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
        prng = rh.rlwe.KeyedPRNG(b"bench bgv lintrans")
        kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
        sk = kg.GenSecretKeyNew()
        enc = rh.bgv.Encoder(rq, T, ringP=rp)
        enc.reserve(64)
        ev = rh.bgv.Evaluator(rq, None, T, ringP=rp, encoder=enc)
        lev = bl.Evaluator(ev)
        n, dims = enc.MaxSlots(), enc.LogMaxDimensions()
        cols = 1 << dims[1]
        top, levelP = len(Q) - 1, len(P) - 1
        rng = np.random.default_rng(logN)
        # ---- (a) the encoding
        for index in (REF_DIAGS, list(range(64))):
            diags = bl.Diagonals({k: rng.integers(0, T, n, dtype=np.uint64) for k in index})
            for ratio in (1, -1):
                lt = bl.NewLinearTransformation(rq, rp, bl.Parameters(index, top, levelP, 1, dims, ratio))

                def encode(fused, lt=lt, diags=diags):
                    bl.Encode(enc, diags, lt, fused=fused)
                    return lt.Block.Q.numpy(), lt.Block.P.numpy()
                wf, wc = encode(True), encode(False)                      # both sides write the same block: compared here, one after the other
                assert np.array_equal(wf[0], wc[0]) and np.array_equal(wf[1], wc[1]), "fused and per-diagonal encodings differ"
                record("a", "Encode, %d diagonals, %s" % (len(index), "BSGS ratio 1" if ratio >= 0 else "naive"), logN,
                       {"diagonals": len(index), "bsgs": ratio >= 0}, lambda fused, lt=lt, diags=diags: bl.Encode(enc, diags, lt, fused=fused), None)
        # ---- (b) whole Evaluate calls
        diags = bl.Diagonals({k: rng.integers(0, T, n, dtype=np.uint64) for k in REF_DIAGS})
        for ratio in (1, -1):
            params = bl.Parameters(REF_DIAGS, top, levelP, 1, dims, ratio)
            galEls = [g for g in params.GaloisElements(N) if g != 1 and g not in ev.galois_keys]
            ev.galois_keys.update(zip(galEls, kg.GenGaloisKeysNew(galEls, sk)))
            lt = bl.NewLinearTransformation(rq, rp, params)
            bl.Encode(enc, diags, lt)
            for B in (1, 8):
                values = rng.integers(0, T, (B, n), dtype=np.uint64)
                pt = enc.NewPlaintext(top, scale=1, nvec=B)
                enc.Encode(values, pt)
                ct = rh.bgv.Encryptor(rq, None, sk, prng=prng).EncryptNew(pt)
                ct.Scale, ct.IsBatched = 1, True
                out = lev.EvaluateNew(ct, lt)                             # the result is Diagonals.Evaluate, slot by slot, before anything is timed
                got = np.asarray(enc.Decode(rh.bgv.Decryptor(rq, sk).DecryptNew(out)))
                want = np.zeros(n, dtype=object)
                for k, d in diags.items():
                    for r in (0, 1):
                        want[r * cols:(r + 1) * cols] += d[r * cols:(r + 1) * cols].astype(object) * np.roll(values[0, r * cols:(r + 1) * cols], -k).astype(object)
                assert np.array_equal(got[0], (want % T).astype(np.uint64)), "wrong result"
                outs = {f: lev.EvaluateNew(ct, lt, fused=f) for f in (True, False)}

                def evaluate(fused, ct=ct, lt=lt, outs=outs):
                    lev.Evaluate(ct, lt, outs[fused], fused=fused)
                    return outs[fused]
                record("b", "Evaluate, 9 diagonals, %s" % ("BSGS ratio 1" if ratio >= 0 else "naive"), logN, {"batch": B, "bsgs": ratio >= 0}, evaluate,
                       lambda a, b: all(np.array_equal(x.numpy(), y.numpy()) for x, y in zip(a.Value, b.Value)))
                del ct, pt, outs
                torch.cuda.empty_cache()
        ev.close(); enc.close(); rq.close(); rp.close()
    from bench import csrc_tree_hash
    default = {"encode": bool(all(not e["windows_overlap"] and e["fused"]["ms_median"] < e["composed"]["ms_median"] for e in results if e["part"] == "a"))}
    res = {"device": torch.cuda.get_device_name(0), "csrc_tree": csrc_tree_hash(), "shape": dict(shape, logN=[13, 15], diagonals=[9, 64], batches=[1, 8]),
           "method": __doc__.split("Method: ")[1].split("  Usage")[0].replace("\n", " "),
           "rule": "encode is fused by default only where, at every shape of part (a), every fused window is below every per-diagonal window",
           "fused_bgv_lintrans_default": default, "results": results}
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"fused_bgv_lintrans_default": default}))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "bgv_lintrans.json"))

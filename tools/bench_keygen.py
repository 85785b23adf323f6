"""Key generation on the device at the bootstrapping chain shape (N = 2^16, 25 + 5 limbs, 5 digits): writes profiles/keygen.json.

  (a) the samplers alone, as bytes WRITTEN per second, next to the write rate profiles/bootstrap.json reports for the ModUp kernel;
  (b) rh_rlwe_gadget_encrypt and rh_rlwe_mul_pk against the composed ring calls on the same prepared rows (alternating windows), and a whole
      key either way;
  (c) the wall time of a relinearisation key plus the Galois keys of the bootstrapping parameters' GaloisElements, one launch sequence;
  (d) one such key made on the host (numpy samples, the CPU oracle's transforms and products) and uploaded through GadgetCiphertext(...),
      times the number of keys: the path a user had before.

Method: device events around windows of calls after 2 warm-up calls, 3 alternating windows per side, the median reported with min and max;
(c) and (d) are host clocks around work that ends in a synchronise.  Usage: python tools/bench_keygen.py [OUT.json]"""
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


def main(out_path):
    N = 1 << 16
    Q, P = primes.gen_moduli(17, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    LQ, LP = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    prng = rh.rlwe.KeyedPRNG(b"bench keygen")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = kg.GenSecretKeyNew()
    rounds = 3
    out = {"device": torch.cuda.get_device_name(0), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "digits": (LQ + LP - 1) // LP},
           "method": __doc__.split("Method: ")[1].split("  Usage")[0].replace("\n", " ")}
    try:
        with open(os.path.join(ROOT, "profiles", "bootstrap.json")) as f:
            mk = json.load(f)["modup_kernel"]
        out["modup_write_GBps_reference"] = {"%s, batch %d" % (e["op"], e["batch"]): e["write_GBps"] for e in mk}
    except (OSError, KeyError):
        out["modup_write_GBps_reference"] = None

    # (a) samplers
    samplers = []
    for B in (4, 32):
        q, p = rq.NewPoly(B), rp.NewPoly(B)
        small = rh.rlwe.SmallPoly(rq, B * (LQ + LP))
        tern = rh.rlwe.TernarySampler(prng, rq, P=2 / 3)
        rows = [("UniformSampler.Read, %d polys of %d + %d limbs" % (B, LQ, LP), lambda: kg.uniform.Read(q, p), B * (LQ + LP) * N * 8),
                ("GaussianSampler.Read (3.2, 19), %d polys, int32" % (B * (LQ + LP)), lambda: kg.gauss.Read(small), B * (LQ + LP) * N * 4),
                ("TernarySampler.Read (P = 2/3), %d polys, int32" % (B * (LQ + LP)), lambda: tern.Read(small), B * (LQ + LP) * N * 4),
                ("lift_small, %d polys to %d + %d limbs" % (B, LQ, LP), lambda: rh.rlwe.lift_small(rq, rp, small.view(0, B), q, p), B * (LQ + LP) * N * 8)]
        for name, fn, written in rows:
            t = stat([timed(fn, 20) for _ in range(rounds)])
            samplers.append({"op": name, **t, "bytes_written": written, "write_GBps": round(written / (t["ms_median"] * 1e-3) / 1e9, 1)})
    out["samplers"] = samplers

    # (b) the kernel against the composed calls, on prepared rows; and a whole key either way
    enc = []
    for nkeys in (1, 8):
        dpl = KG.digits_per_limb(Q, LQ - 1, LP - 1, 0)
        rows = len(dpl) * nkeys
        tabQ, tabP = rq.NewPoly(2 * rows), rp.NewPoly(2 * rows)
        kg.uniform.Read(tabQ, tabP)
        eQ, eP = rq.NewPoly(rows), rp.NewPoly(rows)
        kg.uniform.Read(eQ, eP)
        outQ, outP = rq.NewPoly(nkeys), rp.NewPoly(nkeys)
        kg.uniform.Read(outQ, outP)
        one = KG.gadget_row_table(Q, P, LQ - 1, LP - 1, 0, dpl)
        rt = np.array([[k] + r[1:] for k in range(nkeys) for r in one], dtype=np.uint64)
        table = rh.DevicePoly(rq.AtLevel(0), (rows * (LQ + 1) + N - 1) // N + 1, 1)
        L = rh.lib()

        def fused():
            rh.ringhip._check(L.rh_rlwe_gadget_encrypt(rq._h, rp._h, LQ - 1, LP - 1, eQ.ptr, eP.ptr, tabQ.ptr, tabP.ptr, outQ.ptr, outP.ptr, sk.Value.Q.ptr,
                                                       nkeys, 1, rt.ctypes.data_as(rh.ringhip.U64P), rows, table.ptr, table.words))

        def composed():
            kg._rows_composed(rq, rp, tabQ, tabP, eQ, eP, sk.Value.Q, outQ, outP, 0, nkeys, len(dpl), one)
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(fused, 10)); tc.append(timed(composed, 3))
        f, c = stat(tf), stat(tc)
        moved = rows * (LQ + LP) * N * 8 * 3                              # e and a read, b written; the secrets stay in cache
        enc.append({"op": "rows of %d key(s): rh_rlwe_gadget_encrypt vs MForm + MulCoeffsMontgomeryThenSub + MulScalarMontgomeryThenAdd per row" % nkeys,
                    "rows": rows, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 2),
                    "fused_GBps_moved": round(moved / (f["ms_median"] * 1e-3) / 1e9, 1)})
    for name, fn in (("GenRelinearizationKeyNew, whole call", lambda f: kg.GenRelinearizationKeyNew(sk, fused=f)),
                     ("GenGaloisKeysNew of 8 elements, whole call", lambda f: kg.GenGaloisKeysNew([pow(5, i, 2 * N) for i in range(1, 9)], sk, fused=f))):
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: fn(True), 3, warm=1)); tc.append(timed(lambda: fn(False), 3, warm=1))
        f, c = stat(tf), stat(tc)
        enc.append({"op": name, "fused": f, "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 2)})
    for B in (1, 8):                                                      # the public-key encryptor's two products: one launch that reads u once
        u, k0, k1, o = rq.NewPoly(B), rq.NewPoly(1), rq.NewPoly(1), [rq.NewPoly(B), rq.NewPoly(B)]
        for blk in (u, k0, k1):
            kg.uniform.Read(blk)
        tf, tc = [], []
        for _ in range(rounds):
            tf.append(timed(lambda: rh.rlwe.Encryptor._mul_pk(rq, LQ - 1, u, k0, k1, o, True), 20))
            tc.append(timed(lambda: rh.rlwe.Encryptor._mul_pk(rq, LQ - 1, u, k0, k1, o, False), 5))
        f, c = stat(tf), stat(tc)
        enc.append({"op": "u pk0, u pk1 modulo Q, batch %d: rh_rlwe_mul_pk vs two MulCoeffsMontgomery per ciphertext" % B, "rows": B * LQ, "fused": f,
                    "composed": c, "ratio_composed_over_fused": round(c["ms_median"] / f["ms_median"], 2)})
    out["gadget_encrypt"] = enc
    decided = [e for e in enc if "rows" in e or "whole call" in e["op"]]
    out["fused_keygen_default"] = bool(all(e["fused"]["ms_median"] <= e["composed"]["ms_median"] for e in decided))

    # (c) the bootstrapping key set on the device
    B_, D, M = rh.bootstrapping, rh.dft, rh.mod1
    s2c = D.MatrixLiteral(D.HomomorphicDecode, 15, 12, LP - 1, [1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    c2s = D.MatrixLiteral(D.HomomorphicEncode, 15, 24, LP - 1, [1, 1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    m1 = M.ParametersLiteral(LevelQ=20, LogScale=60, Mod1Type=M.CosDiscrete, LogMessageRatio=8, K=16, Mod1Degree=30, DoubleAngle=3)
    params = B_.Parameters(rq, rp, 9, 1 << 40, s2c, m1, c2s, EphemeralSecretWeight=32)
    galEls = [g for g in params.GaloisElements() if g != 1]
    key_bytes = 2 * len(dpl) * (LQ + LP) * N * 8
    walls = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rlk = kg.GenRelinearizationKeyNew(sk)
        gks = kg.GenGaloisKeysNew(galEls, sk)
        torch.cuda.synchronize()
        walls.append((time.perf_counter() - t0) * 1e3)
        del rlk, gks
    nk = 1 + len(galEls)
    out["bootstrapping_key_set_on_device"] = {"keys": nk, "bytes_per_key": key_bytes, "wall": stat(walls),
                                              "write_GBps_of_key_bytes": round(nk * key_bytes / (statistics.median(walls) * 1e-3) / 1e9, 1)}

    # (d) one key on the host and uploaded, times the number of keys
    from oracle import ring_oracle as orc
    from oracle.compose import OPS
    rng = np.random.default_rng(1)
    mods = Q + P
    srs = [orc.SubRingConsts(N, q) for q in mods]
    s_rows = np.concatenate([sk.Value.Q.numpy()[0], sk.Value.P.numpy()[0]])
    t0 = time.perf_counter()
    rows = []
    z = np.zeros(N, dtype=np.uint64)
    for r in range(len(dpl)):
        e = np.rint(rng.normal(0, 3.2, N)).astype(np.int64)
        b, a = [], []
        for j, q in enumerate(mods):
            aj = rng.integers(0, q, N, dtype=np.uint64)
            ej = orc.vec_op(OPS["MFORM"], orc.ntt((e % q).astype(np.uint64), srs[j]), None, z, 0, 0, q)
            bj = orc.vec_op(OPS["SUB"], ej, orc.vec_op(OPS["MUL_MONT"], aj, s_rows[j], z, 0, 0, q), z, 0, 0, q)
            if j < LQ and one[r][1 + j]:
                bj = orc.vec_op(OPS["ADD"], bj, orc.vec_op(OPS["MUL_SCALAR_MONT"], s_rows[j], None, z, one[r][1 + j], 0, q), z, 0, 0, q)
            b.append(bj); a.append(aj)
        rows.append(np.stack([np.stack(b), np.stack(a)]))
    key = np.stack(rows)
    t1 = time.perf_counter()
    g = rh.rlwe.GadgetCiphertext(rq, rp, key[:, :, :LQ], key[:, :, LQ:])
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    out["one_key_on_host_and_uploaded"] = {"make_ms": round((t1 - t0) * 1e3, 1), "upload_ms": round((t2 - t1) * 1e3, 1),
                                           "times_keys_of_the_set_ms": round((t2 - t0) * 1e3 * nk, 1),
                                           "note": "one key measured (numpy samples, the CPU oracle's NTT and Montgomery products, single thread), multiplied by the key count"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "keygen.json"))

"""The noise meters at the bootstrapping chain shape (N = 2^16, 25 + 5 limbs, 5 digits), real keys from a KeyedPRNG: writes profiles/noise.json.

  (a) NoiseGaloisKeys over the Galois keys of the bootstrapping parameters and NoiseRelinearizationKey: the kernels (FUSED_NOISE) against the
      composed ring calls for the phase, both ending in rh_ring_centered_moments; wall clocks around whole calls that end in a download;
  (b) the rh_rlwe_gadget_phase CALL alone over all keys, as bytes of key READ per second, next to rh_rlwe_gadget_encrypt's rate in
      profiles/keygen.json, which is taken the same way: device events around whole C calls on a prepared row table and preallocated blocks,
      so the staging copy of the row table is inside the figure -- a call rate, not a kernel trace;
  (c) the rh_ring_centered_moments call alone on 1 and on 64 polys modulo QP, likewise (its table build and staging copy included);
  (d) the host route for ONE key: the composed phase, a download, Python integers.  Measured once, for one key, and reported as that.

Method: (a) host clocks around whole calls that end in a synchronise, one untimed call of each arm first, then three timed calls per arm in
alternation; (b), (c) one side each: device events around windows of back-to-back calls after 2 warm-up calls, each window at least 0.25 s of
device time (200 calls of the phase, 500 and 60 of the moments), three windows, the median reported with min and max; (d) a host clock, once.
Usage: python tools/bench_noise.py [OUT.json]"""
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
from matrix_fhe_lattigo_amd import noise as NZ
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


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def stat(v):
    return {"ms_median": round(statistics.median(v), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def main(out_path):
    N = 1 << 16
    Q, P = primes.gen_moduli(17, [60] + [40] * 9 + [39] * 3 + [60] * 8 + [56] * 4, [61] * 5)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    LQ, LP = len(Q), len(P)
    rq, rp = rh.Ring(N, Q), rh.Ring(N, P)
    rq.set_stream(stream.cuda_stream); rp.set_stream(stream.cuda_stream)
    prng = rh.rlwe.KeyedPRNG(b"bench noise")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = kg.GenSecretKeyNew()
    out = {"device": torch.cuda.get_device_name(0), "shape": {"N": N, "limbs_Q": LQ, "limbs_P": LP, "digits": (LQ + LP - 1) // LP},
           "method": __doc__.split("Method: ")[1].split("\nUsage")[0].replace("\n", " ")}
    try:
        with open(os.path.join(ROOT, "profiles", "keygen.json")) as f:
            out["gadget_encrypt_GBps_reference"] = [e["fused_GBps_moved"] for e in json.load(f)["gadget_encrypt"] if "fused_GBps_moved" in e]
    except (OSError, KeyError):
        out["gadget_encrypt_GBps_reference"] = None

    B_, D, M = rh.bootstrapping, rh.dft, rh.mod1
    s2c = D.MatrixLiteral(D.HomomorphicDecode, 15, 12, LP - 1, [1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    c2s = D.MatrixLiteral(D.HomomorphicEncode, 15, 24, LP - 1, [1, 1, 1, 1], D.RepackImagAsReal, LogBSGSRatio=1)
    m1 = M.ParametersLiteral(LevelQ=20, LogScale=60, Mod1Type=M.CosDiscrete, LogMessageRatio=8, K=16, Mod1Degree=30, DoubleAngle=3)
    params = B_.Parameters(rq, rp, 9, 1 << 40, s2c, m1, c2s, EphemeralSecretWeight=32)
    galEls = [g for g in params.GaloisElements() if g != 1]
    rlk = kg.GenRelinearizationKeyNew(sk)
    gks = kg.GenGaloisKeysNew(galEls, sk)
    key_bytes = 2 * rlk.digits * (LQ + LP) * N * 8
    out["keys"] = {"galois_keys": len(gks), "bytes_per_key": key_bytes}

    # (a) whole calls
    calls = []
    for name, fn in (("NoiseGaloisKeys over %d keys" % len(gks), lambda f: rh.rlwe.NoiseGaloisKeys(gks, sk, fused=f)),
                     ("NoiseRelinearizationKey", lambda f: rh.rlwe.NoiseRelinearizationKey(rlk, sk, fused=f))):
        arms = {"fused": {"gadget_phase": True, "moments": True}, "composed_phase": {"gadget_phase": False, "moments": True}}
        fn(arms["fused"]); fn(arms["composed_phase"])
        t = {k: [] for k in arms}
        res = {}
        for _ in range(3):
            for k, a in arms.items():
                ms, res[k] = wall(lambda: fn(a))
                t[k].append(ms)
        same = res["fused"] == res["composed_phase"]
        worst = max(res["fused"].values()) if isinstance(res["fused"], dict) else res["fused"]
        calls.append({"op": name, "fused": stat(t["fused"]), "composed_phase": stat(t["composed_phase"]), "same_floats": bool(same),
                      "ratio_composed_over_fused": round(statistics.median(t["composed_phase"]) / statistics.median(t["fused"]), 2),
                      "largest_log2_std": worst})
    out["whole_calls"] = calls

    # (b) the phase call alone over all Galois keys: the entry on a prepared row table, preallocated output and scratch; then the Python call
    # around it (stacking the secrets, building the table, allocating and freeing the output)
    items = [(g, 0, 0) for g in gks]
    sks = [sk]
    pts = [sk.Value.Q]
    Pb = 1
    for m in P:
        Pb *= m
    scal = [(Pb << 64) % q for q in Q]
    rows = list(range(gks[0].digits))
    rt = np.array([[g.Q.ptr, g.P.ptr, g.digits, 0, 0, len(rows)] + rows + scal for g in gks], dtype=np.uint64)
    outQ, outP = rq.NewPoly(len(gks)), rp.NewPoly(len(gks))
    tdev = rh.DevicePoly(rq.AtLevel(0), (rt.size + N - 1) // N + 1, 1)
    L = rh.lib()

    def entry():
        rh.ringhip._check(L.rh_rlwe_gadget_phase(rq._h, rp._h, LQ - 1, LP - 1, sk.Value.Q.ptr, sk.Value.P.ptr, 1, sk.Value.Q.ptr, 1, outQ.ptr, outP.ptr,
                                                 rt.ctypes.data_as(rh.ringhip.U64P), len(gks), len(rows), tdev.ptr, tdev.words))

    def phase(fused):
        for _ in NZ.gadget_phases(items, sks, pts, fused=fused):
            pass
    e = stat([timed(entry, 200) for _ in range(3)])
    f = stat([timed(lambda: phase(True), 10) for _ in range(3)])
    read = len(gks) * key_bytes
    written = len(gks) * (LQ + LP) * N * 8
    out["gadget_phase_alone"] = {"keys": len(gks), "what": "call rates: device events around whole calls, the row table's staging copy included",
                                 "entry": e, "python_call": f, "key_bytes_read": read, "bytes_written": written,
                                 "entry_read_TBps_of_key_bytes": round(read / (e["ms_median"] * 1e-3) / 1e12, 2),
                                 "entry_TBps_moved": round((read + written) / (e["ms_median"] * 1e-3) / 1e12, 2),
                                 "python_call_read_TBps_of_key_bytes": round(read / (f["ms_median"] * 1e-3) / 1e12, 2)}

    # (c) the moments alone
    mom = []
    for B in (1, 64):
        q, p = rq.NewPoly(B), rp.NewPoly(B)
        kg.uniform.Read(q, p)
        W = NZ.moments_words(LQ + LP)
        blk = rh.DevicePoly(rq.AtLevel(0), (B * W + N - 1) // N + 1, 1)

        def fn():
            rh.ringhip._check(L.rh_ring_centered_moments(rq._h, LQ - 1, q.ptr, LQ, rp._h, LP - 1, p.ptr, LP, 1, B, blk.ptr))
        t = stat([timed(fn, 500 if B == 1 else 60) for _ in range(3)])
        read = B * (LQ + LP) * N * 8
        mom.append({"op": "rh_ring_centered_moments call, %d uniform poly(s) modulo QP (%d limbs)" % (B, LQ + LP), **t, "bytes_read": read,
                    "read_GBps": round(read / (t["ms_median"] * 1e-3) / 1e9, 1),
                    "coefficients_per_us": round(B * N / (t["ms_median"] * 1e3), 1)})
    out["moments_alone"] = mom

    # (d) the host route, one key
    ms, v = wall(lambda: rh.rlwe.NoiseGaloisKey(gks[0], sk, fused=False))
    ms_f, v_f = wall(lambda: rh.rlwe.NoiseGaloisKey(gks[0], sk, fused=True))
    out["host_route_one_key"] = {"composed_phase_download_python_integers_ms": round(ms, 1), "fused_ms": round(ms_f, 2), "same_float": bool(v == v_f),
                                 "note": "ONE key, measured once; not multiplied by the key count"}
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "noise.json"))

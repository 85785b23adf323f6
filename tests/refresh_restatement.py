"""The share conversion and the protocols of the reference's multiparty/mpckks package in plain Python integers, with EXPLICIT samples: what
matrix-fhe-lattigo_amd/multiparty_refresh.py and csrc/mp_refresh.hip are compared with, bit for bit.  TEST INFRASTRUCTURE ONLY.

Polys are numpy uint64 arrays (limbs, N); a secret is handed in as its rows in the NTT domain and in Montgomery form, as in
tests/multiparty_restatement.py; shares of integers are lists of Python ints, n = 2 * slots of them, value i at coefficient i * (N / n)."""
import hashlib
import math
import struct

import numpy as np

import multiparty_restatement as mr
import rlwe_restatement as rr

PERSON = b"ringhip-sampler\0"


# ---- the mask law: mpckks/sharing.go:120-129 on the samplers' stream ------------------------------------------------------------------------------
def stream_word(key, call, poly, row, i):
    """word i % 8 of block t = 0 of substream (call, poly, row, group = i // 8)"""
    d = hashlib.blake2b(struct.pack("<5Q", call, poly, row, i // 8, 0), key=key, digest_size=64, person=PERSON).digest()
    return struct.unpack("<8Q", d)[i % 8]


def masks(key, call, poly0, npoly, n, logBound):
    """RandInt(prng, 2^logBound), then - 2^logBound when >= 2^(logBound - 1): the low logBound bits of the words (row = word index), centred"""
    words = (logBound + 63) // 64
    out = []
    for p in range(npoly):
        row = []
        for i in range(n):
            v = sum(stream_word(key, call, poly0 + p, w, i) << (64 * w) for w in range(words)) & ((1 << logBound) - 1)
            row.append(v - (1 << logBound) if v >= 1 << (logBound - 1) else v)
        out.append(row)
    return out


# ---- ring/ring.go:433-447, :503-543 and core/rlwe/utils.go:187-245 -------------------------------------------------------------------------------------
def to_rns(values, mods, N):
    """SetCoefficientsBigint + the spread of NTTSparseAndMontgomery: (limbs, N), coefficient domain; Python's % is big.Int.Mod's Euclidean residue"""
    gap = N // len(values)
    out = np.zeros((len(mods), N), dtype=np.uint64)
    for k, q in enumerate(mods):
        out[k, ::gap] = [v % q for v in values]
    return out


def from_rns(rows, mods, n):
    """PolyToBigintCentered(p, gap, .): v - Q when v >= floor(Q / 2)"""
    Q = math.prod(mods)
    N = rows.shape[-1]
    gap = N // n
    parts = [(Q // q) * pow(Q // q, -1, q) for q in mods]
    out = []
    for i in range(n):
        v = sum(int(rows[k, i * gap]) * parts[k] for k in range(len(mods))) % Q
        out.append(v - Q if v >= Q // 2 else v)
    return out


def quo(x, m, d):
    """big.Int.Quo(x * m, d): truncated toward zero"""
    p = x * m
    return -((-p) // d) if p < 0 else p // d


def input_scale_int(scale):
    """.Int plus one when that truncated (mpckks/transform.go:364-370)"""
    return math.ceil(scale)


def recode(values, m, d, mods_out, N_out):
    return to_rns([quo(v, m, d) for v in values], mods_out, N_out)


def get_minimum_level_for_refresh(lam, scale, nParties, moduli):
    """mpckks/utils.go:16-39"""
    logBound = lam + int(math.ceil(math.log2(float(scale))))
    maxBound = math.ceil(float(logBound) + math.log2(float(nParties)))
    minLevel, logQ = -1, 0.0
    for i in range(len(moduli) + 1):
        if not logQ < maxBound:
            break
        if i >= len(moduli):
            return 0, 0, False
        logQ += math.log2(float(moduli[i]))
        minLevel += 1
    return minLevel, logBound, True


# ---- the protocols ---------------------------------------------------------------------------------------------------------------------------------
def _spread_ntt(values, mods, N):
    return rr.ntt(to_rns(values, mods, N), N, mods)


def e2s_gen_share(sk_rows, Q, level, c1, e, mask):
    """EncToShareProtocol.GenShare (sharing.go:90-143): c1 sk + e - NTT(spread(mask)), NTT domain"""
    mods = [int(q) for q in Q[:level + 1]]
    N = sk_rows.shape[-1]
    zero = np.zeros_like(sk_rows)
    pub = mr.keyswitch_share(sk_rows, zero, Q, level, c1, e)
    return rr._vec("SUB", pub, _spread_ntt(mask, mods, N), mods)


def e2s_get_share(secret, agg, c0, Q, level, n):
    """EncToShareProtocol.GetShare (sharing.go:150-186)"""
    mods = [int(q) for q in Q[:level + 1]]
    N = agg.shape[-1]
    x = from_rns(rr.intt(mr.add(agg[:level + 1], np.asarray(c0, dtype=np.uint64)[:level + 1], mods), N, mods), mods, n)
    return x if secret is None else [a + b for a, b in zip(secret, x)]


def s2e_gen_share(sk_rows, Q, level, crp, e, share):
    """ShareToEncProtocol.GenShare (sharing.go:234-262): -crp sk + e + NTT(spread(share))"""
    mods = [int(q) for q in Q[:level + 1]]
    N = sk_rows.shape[-1]
    zero = np.zeros_like(sk_rows)
    return mr.add(mr.keyswitch_share(zero, sk_rows, Q, level, crp, e), _spread_ntt(share, mods, N), mods)


def transform_gen_share(sk_in, sk_out, Qin, level_in, Qout, level_out, c1, crp, e, mask, scale_out, scale_in):
    """MaskedLinearTransformationProtocol.GenShare with transform = nil (transform.go:153-199) -> (e2s share, s2e share)"""
    m, d = int(scale_out), input_scale_int(scale_in)
    return (e2s_gen_share(sk_in, Qin, level_in, c1, e[0], mask),
            s2e_gen_share(sk_out, Qout, level_out, crp, e[1], [quo(v, m, d) for v in mask]))


def transform(c0, e2s_agg, s2e_agg, Qin, level_in, Qout, level_out, N_out, n, scale_out, scale_in):
    """Transform with transform = nil (transform.go:220-300) -> the new c0 (c1 is the CRP)"""
    mods = [int(q) for q in Qout[:level_out + 1]]
    x = e2s_get_share(None, e2s_agg, c0, Qin, level_in, n)
    y = rr.ntt(recode(x, int(scale_out), input_scale_int(scale_in), mods, N_out), N_out, mods)
    return mr.add(y, s2e_agg, mods)


# ---- mpbgv (mpbgv/sharing.go, mpbgv/transform.go): P a bgv_encoder_restatement.Params, shares (n,) arrays modulo T -------------------------------------
def _bgv_lift(P, level, pT):
    import bgv_encoder_restatement as be
    mods = P.Q[:level + 1]
    return rr.ntt(be.ring_t2q(P, mods, pT, True), P.N, mods)


def bgv_e2s_gen_share(P, sk_rows, level, c1, e, mask):
    """EncToShareProtocol.GenShare (sharing.go:91-99)"""
    pub = mr.keyswitch_share(sk_rows, np.zeros_like(sk_rows), P.Q, level, c1, e)
    return rr._vec("SUB", pub, _bgv_lift(P, level, mask), P.Q[:level + 1])


def bgv_e2s_get_share(P, secret, agg, c0, level):
    """EncToShareProtocol.GetShare (sharing.go:106-117)"""
    import bgv_encoder_restatement as be
    mods = P.Q[:level + 1]
    x = be.ring_q2t(P, level, rr.intt(mr.add(agg[:level + 1], np.asarray(c0, dtype=np.uint64)[:level + 1], mods), P.N, mods))
    x = np.array([int(v) for v in x], dtype=np.uint64)
    cred = lambda v: v - P.t if v >= P.t else v                              # ringT.Add: one conditional subtraction
    return x if secret is None else np.array([cred(int(a) + int(b)) for a, b in zip(secret, x)], dtype=np.uint64)


def bgv_s2e_gen_share(P, sk_rows, level, crp, e, share):
    """ShareToEncProtocol.GenShare (sharing.go:168-184)"""
    return mr.add(mr.keyswitch_share(np.zeros_like(sk_rows), sk_rows, P.Q, level, crp, e), _bgv_lift(P, level, share), P.Q[:level + 1])


def bgv_apply(P, transform, mask, scale):
    """Decode, Func, Encode of mpbgv/transform.go:101-123: transform = (decode, func on a list of ints, encode) or None"""
    import bgv_encoder_restatement as be
    if transform is None:
        return mask
    decode, func, encode = transform
    vals = be.decode_ring_t(P, mask, scale) if decode else [int(v) for v in mask]
    vals = func([int(v) for v in vals])
    return be.encode_ring_t(P, np.array(vals, dtype=np.uint64), scale) if encode else np.array(vals, dtype=np.uint64)


def bgv_transform_gen_share(P, sk_in, sk_out, level_in, level_out, c1, crp, e, mask, transform, scale):
    """MaskedTransformProtocol.GenShare (transform.go:89-129), Decode / Encode at ct.Scale"""
    return (bgv_e2s_gen_share(P, sk_in, level_in, c1, e[0], mask),
            bgv_s2e_gen_share(P, sk_out, level_out, crp, e[1], bgv_apply(P, transform, mask, scale)))


def bgv_transform(P, c0, e2s_agg, s2e_agg, level_in, level_out, transform, scale_out):
    """Transform (transform.go:149-198), Decode / Encode at ciphertextOut.Scale -> the new c0"""
    x = bgv_apply(P, transform, bgv_e2s_get_share(P, None, e2s_agg, c0, level_in), scale_out)
    return mr.add(_bgv_lift(P, level_out, x), s2e_agg, P.Q[:level_out + 1])

"""The reference's BGV encoder, schemes/bgv/encoder.go, restated step by step in numpy and Python integers over the pinned oracle pieces
(oracle.ring_oracle: ntt / intt, modup_centered = AddScalarBigint + ModUpExact + SubScalarBigint, oracle/ring_oracle.h:83-88).  TEST
INFRASTRUCTURE ONLY: the GPU tests compare the device path against it bit for bit, tests/test_bgv_encoder_oracle.py pins it to facts that
do not depend on it.

Polys are numpy uint64 arrays of shape (limbs, N); a poly modulo T is a (n,) array; values are numpy uint64 or int64 vectors.  Where a
reference step ends in MRed / BRedAdd of a value below 2^64 its result is the canonical residue, written here as Python's %."""
import numpy as np

from oracle import ring_oracle as orc


def prod(mods):
    out = 1
    for m in mods:
        out *= int(m)
    return out


def plaintext_ring_degree(N, t):
    """bgv/params.go:110-121"""
    order = 1 << int(t).bit_length()
    while order and t & (order - 1) != 1:
        order >>= 1
    assert order >= 16
    return min(N, order >> 1)


def permute_matrix(logn):
    """permuteMatrix (:98-121)"""
    n = 1 << logn
    perm = [0] * n
    pow5, mask = 1, 2 * n - 1
    for i in range(n >> 1):
        pos = int(format(pow5 >> 1, "0%db" % logn)[::-1], 2)         # utils.BitReverse64(pow >> 1, logN)
        perm[i], perm[i + (n >> 1)] = pos, n - pos - 1
        pow5 = pow5 * 5 & mask
    return perm


class Params:
    """ringQ (or any ring of degree N: the moduli of P for Embed), ringT and the index matrix, as NewEncoder (:49-96) holds them"""

    def __init__(self, N, Q, t, perm=None):
        self.N, self.Q, self.t = int(N), [int(q) for q in Q], int(t)
        self.n = plaintext_ring_degree(self.N, self.t)
        self.gap = self.N // self.n
        self.srQ = [orc.SubRingConsts(self.N, q) for q in self.Q]
        self.srT = orc.SubRingConsts(self.n, self.t)
        self.perm = permute_matrix(self.n.bit_length() - 1) if perm is None else list(perm)


def _u(x):
    return np.array([int(v) for v in x], dtype=np.uint64)


def reduce_values(values, t):
    """[]uint64: ringT.Reduce (:208); []int64: sign / abs (:221-228, :159-166) -- a negative multiple of T gives the word T"""
    values = np.asarray(values)
    assert values.dtype in (np.uint64, np.int64)
    if values.dtype == np.uint64:
        return [int(c) % t for c in values]
    out = []
    for c in values:
        c = int(c)
        sign = 1 if c < 0 else 0
        a = (-c if sign else c) & ((1 << 64) - 1)                     # uint64(c * ((sign ^ 1) - sign)): int64 min wraps to 2^63
        a %= t
        out.append(t - a if sign else a)
    return out


def encode_ring_t(P, values, scale):
    """EncodeRingT (:187-246) -> (n,) modulo T"""
    assert len(values) <= P.n
    pt = [0] * P.n
    for i, w in enumerate(reduce_values(values, P.t)):
        pt[P.perm[i]] = w % P.t                                       # the word T of a negative multiple: INTT's canonical output is that of 0
    pt = orc.intt(_u(pt), P.srT)                                      # :242
    return _u([int(x) * (scale % P.t) % P.t for x in pt])            # :243 MulScalar = MRed(x, MForm(scale))


def ring_t2q(P, mods, pT, scale_up):
    """RingT2Q (:357-386) into the limbs `mods` (a prefix of Q, or of P): the residue modulo T UNREDUCED at stride gap, then MulScalarBigint
    by T^-1 mod Q_level, which is MRed(x, MForm(T^-1 mod q_i)) = x T^-1 mod q_i per limb"""
    out = np.zeros((len(mods), P.N), dtype=np.uint64)
    for i, q in enumerate(mods):
        row = [int(x) for x in pT]
        if scale_up:
            tinv = pow(P.t, -1, prod(mods)) % q
            row = [x * tinv % q for x in row]
        out[i, ::P.gap] = _u(row)
    return out


def finish(P, mods, srs, p, is_ntt, mont):
    """NTT (:270-272) and MForm (:274-276) of EmbedScale"""
    if is_ntt:
        p = np.stack([orc.ntt(_u([int(x) % q for x in p[i]]), srs[i]) for i, q in enumerate(mods)])
    if mont:
        p = np.stack([_u([(int(x) << 64) % q for x in p[i]]) for i, q in enumerate(mods)])
    return p


def embed(P, level, values, scale, scale_up, is_ntt, mont, mods=None, srs=None):
    """EmbedScale (:252-316) into a ring.Poly at `level`; mods / srs: another ring of degree N (the P half of a ringqp.Poly)"""
    mods = P.Q[:level + 1] if mods is None else mods[:level + 1]
    srs = P.srQ[:level + 1] if srs is None else srs[:level + 1]
    return finish(P, mods, srs, ring_t2q(P, mods, encode_ring_t(P, values, scale), scale_up), is_ntt, mont)


def encode(P, level, values, scale, is_ntt=True, batched=True, mont=False):
    """Encode (:130-184)"""
    if batched:
        return embed(P, level, values, scale, True, is_ntt, mont)
    assert len(values) <= P.n
    pt = [w % P.t for w in reduce_values(values, P.t)] + [0] * (P.n - len(values))
    pt = _u([x * (scale % P.t) % P.t for x in pt])                   # :175
    return finish(P, P.Q[:level + 1], P.srQ[:level + 1], ring_t2q(P, P.Q[:level + 1], pt, True), is_ntt, False)


def ring_q2t(P, level, pQ):
    """RingQ2T (:391-439) with scaleDown = true -> (n,) as the reference leaves it (the gap = 1 branch above level 0 is not canonical)"""
    mods, t = P.Q[:level + 1], P.t
    poly = [[int(x) * t % q for x in pQ[i]] for i, q in enumerate(mods)]          # :398 MulScalar(pQ, T)
    if level > 0 and P.gap == 1:                                      # :409-411
        return orc.modup_centered(np.stack([_u(r) for r in poly]), mods, [t])[0]
    if level > 0:                                                     # :413-414 PolyToBigintCentered(gap) + SetCoefficientsBigint
        Qb = prod(mods)
        crt = [(Qb // q) * pow(Qb // q, -1, q) for q in mods]
        out = []
        for j in range(0, P.N, P.gap):
            x = sum(poly[k][j] * crt[k] for k in range(len(mods))) % Qb
            if x >= Qb >> 1:
                x -= Qb
            out.append(x % t)
        return _u(out)
    q0 = mods[0]
    half = q0 >> 1
    out = []
    for j in range(0, P.N, P.gap):                                    # :417-437
        x = poly[0][j] + half
        x = x - q0 if x >= q0 else x                                  # AddScalar
        x %= t                                                        # Reduce
        x = x + t - half % t                                          # SubScalar
        out.append(x - t if x >= t else x)
    return _u(out)


def _signed(vals, t, signed):
    if not signed:
        return np.array(vals, dtype=np.uint64)
    return np.array([v - t if v >= t >> 1 else v for v in vals], dtype=np.int64)      # :342: >=


def decode_ring_t(P, pT, scale, signed=False):
    """DecodeRingT (:323-353)"""
    sinv = pow(scale % P.t, P.t - 2, P.t)                             # ring.ModExp(scale, T - 2, T)
    tmp = orc.ntt(_u([int(x) * sinv % P.t for x in pT]), P.srT)       # :325-326
    return _signed([int(tmp[P.perm[i]]) for i in range(P.n)], P.t, signed)


def decode(P, level, pQ, scale, is_ntt=True, batched=True, signed=False):
    """Decode (:442-487)"""
    if is_ntt:
        pQ = np.stack([orc.intt(pQ[i], P.srQ[i]) for i in range(level + 1)])
    bufT = ring_q2t(P, level, pQ)
    if batched:
        return decode_ring_t(P, bufT, scale, signed)
    sinv = pow(scale % P.t, P.t - 2, P.t)
    return _signed([int(x) * sinv % P.t for x in bufT], P.t, signed)  # :457-479

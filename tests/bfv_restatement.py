"""The reference's scale-invariant (BFV) tensoring, schemes/bgv/evaluator.go, restated step by step over the pinned oracle pieces
(oracle.ring_oracle: ntt / intt, vec_op, modup_centered) plus big-integer constants formed here.  TEST INFRASTRUCTURE ONLY: the GPU tests
compare the device path against it, tests/test_bfv_oracle.py pins it to big-integer ground truth that does not depend on the composition.

Polys are numpy uint64 arrays of shape (limbs, N); a ciphertext is a list of such arrays (NTT domain)."""
import numpy as np

from oracle import ring_oracle as orc
from oracle.compose import OPS


def prod(mods):
    out = 1
    for m in mods:
        out *= int(m)
    return out


def level_qmul(Q, logN):
    """newEvaluatorPrecomp (:51-56): levelQMul[i] = ceil((bitlen(q_0 .. q_i) + logN) / 61) - 1"""
    return [-(-(prod(Q[:i + 1]).bit_length() + logN) // 61) - 1 for i in range(len(Q))]


def nb_qi_mul(Q, logN):
    """bgv/params.go:98-108: the size of RingQMul, ceil((bitlen(Q_max) + logN) / 61)"""
    return -(-(prod(Q).bit_length() + logN) // 61)


def scale_invariant(t, Q_level, a, b):
    """MulScaleInvariant (:1045-1051) with rlwe.Scale's arithmetic modulo T (core/rlwe/scale.go:77-119)"""
    return (a * b) % t * pow(t - Q_level % t, -1, t) % t


class Params:
    """ringQ, ringQMul and the plaintext modulus, as the evaluator holds them"""

    def __init__(self, N, Q, QMul, t):
        self.N, self.logN, self.t = N, N.bit_length() - 1, int(t)
        self.Q, self.QMul = [int(q) for q in Q], [int(p) for p in QMul]
        self.srQ = [orc.SubRingConsts(N, q) for q in self.Q]
        self.srM = [orc.SubRingConsts(N, p) for p in self.QMul]
        self.levelQMul = level_qmul(self.Q, self.logN)

    def at(self, level):
        lq = self.levelQMul[level]
        assert lq < len(self.QMul), "ringQMul too short for level %d" % level
        return self.Q[:level + 1], self.QMul[:lq + 1], self.srQ[:level + 1], self.srM[:lq + 1]


def _vec(op, p1, p2, p3, s0, mods):
    return np.stack([orc.vec_op(OPS[op], p1[i], p2[i] if p2 is not None else None, p3[i], s0[i] if s0 is not None else 0, 0, mods[i])
                     for i in range(len(mods))])


def _zeros(a):
    return np.zeros_like(a)


def ntt(x, srs, lazy=False):
    return np.stack([orc.ntt(x[i], srs[i], lazy=lazy) for i in range(len(srs))])


def intt(x, srs, lazy=False):
    return np.stack([orc.intt(x[i], srs[i], lazy=lazy) for i in range(len(srs))])


def mod_up_and_ntt(P, level, ct):
    """modUpAndNTT (:1053-1060): per component ringQ.INTT -> ModUpQtoP(level, levelQMul) -> ringQMul.NTTLazy"""
    Ql, Ml, srQ, srM = P.at(level)
    out = []
    for c in ct:
        buff = intt(c, srQ)                                          # :1056
        up = orc.modup_centered(buff, Ql, Ml)                        # :1057 (ring/basis_extension.go:188-200)
        out.append(ntt(up, srM, lazy=True))                          # :1058
    return out


def tensor_low_deg(mods, ct0, ct1):
    """tensorLowDeg (:1062-1102) in ONE ring: ct1 None = the squaring case.  Returns [c0, c1, c2]; c1 is not reduced after the add."""
    c00 = _vec("MFORM", ct0[0], None, _zeros(ct0[0]), None, mods)    # :1069 / :1075
    c01 = _vec("MFORM", ct0[1], None, _zeros(ct0[1]), None, mods)    # :1070 / :1076
    z = _zeros(ct0[0])
    if ct1 is None:
        c0 = _vec("MUL_MONT", c00, ct0[0], z, None, mods)            # :1080 / :1085
        c2 = _vec("MUL_MONT", c01, ct0[1], z, None, mods)            # :1081 / :1086
        c1 = _vec("MUL_MONT", c00, ct0[1], z, None, mods)            # :1082 / :1087
        c1 = _vec("ADD_LAZY", c1, c1, z, None, mods)                 # :1083 / :1088
    else:
        c0 = _vec("MUL_MONT", c00, ct1[0], z, None, mods)            # :1092 / :1097
        c2 = _vec("MUL_MONT", c01, ct1[1], z, None, mods)            # :1093 / :1098
        c1 = _vec("MUL_MONT", c00, ct1[1], z, None, mods)            # :1094 / :1099
        c1 = _vec("MUL_MONT_THEN_ADD_LAZY", c01, ct1[0], c1, None, mods)   # :1095 / :1100
    return [c0, c1, c2]


def mod_down_qp_to_p(p1Q, p1P, Ql, Ml):
    """ModDownQPtoP (ring/basis_extension.go:264-278): ModUpQtoP into buffP, then per limb of P
    SubThenMulScalarMontgomeryTwoModulus(buffP, p1P, p - modDownConstantsQtoP) with the constant MForm(Q^-1 mod p) (:25-49)"""
    buff = orc.modup_centered(p1Q, Ql, Ml)                           # :270
    Qb = prod(Ql)
    sc = [p - ((pow(Qb % p, -1, p) << 64) % p) for p in Ml]
    return _vec("SUB_THEN_MUL_SCALAR_MONT_TWO_MODULUS", buff, p1P, _zeros(p1P), sc, Ml)   # :273-276


def quantize(P, level, c2Q1, c2Q2):
    """quantize (:1104-1124): NTT-domain (Q, QMul) -> NTT-domain Q"""
    Ql, Ml, srQ, srM = P.at(level)
    q1 = intt(c2Q1, srQ, lazy=True)                                  # :1111
    q2 = intt(c2Q2, srM, lazy=True)                                  # :1112
    q2 = mod_down_qp_to_p(q1, q2, Ql, Ml)                            # :1115
    q1 = orc.modup_centered(q2, Ml, Ql)                              # :1118 (ring/basis_extension.go:205-217)
    tm = [(P.t << 64) % q for q in Ql]                               # MulScalar: MForm(T) (ring/operations.go:201-205)
    q1 = _vec("MUL_SCALAR_MONT", q1, None, _zeros(q1), tm, Ql)       # :1121
    return ntt(q1, srQ)                                              # :1123


def tensor_scale_invariant(P, level, ct0, ct1):
    """tensorScaleInvariant (:975-1014) without relinearisation.  ct1 None (or ct1 is ct0): squaring, one lifted operand (:995-997).
    The operand swap of :982-987 only decides which operand is put in Montgomery form: every product below is a canonical MRed, so it
    does not change a bit of the result and is not restated.  Returns [c0, c1, c2] in Q, NTT domain."""
    Ql, Ml, _, _ = P.at(level)
    if ct1 is ct0:
        ct1 = None
    t0 = mod_up_and_ntt(P, level, ct0)                               # :993
    t1 = mod_up_and_ntt(P, level, ct1) if ct1 is not None else None  # :996
    cq = tensor_low_deg(Ql, ct0, ct1)                                # :1010, ringQ half
    cm = tensor_low_deg(Ml, t0, t1)                                  #        ringQMul half
    return [quantize(P, level, cq[k], cm[k]) for k in range(3)]      # :1012-1014


def relinearize(N, Q, Pk, level, c, evkQ, evkP):
    """the relin branch (:1016-1035) for a key with ONE P modulus: GadgetProduct of c2, then two ringQ.Add"""
    from oracle import compose
    k0, k1 = compose.gadget_product_single_p(N, Q, Pk, level, 0, c[2], True, 0, None, evkQ, evkP)
    Ql = Q[:level + 1]
    return [_vec("ADD", c[0], k0, _zeros(c[0]), None, Ql), _vec("ADD", c[1], k1, _zeros(c[1]), None, Ql)]


# ---- big-integer helpers for the ground truth --------------------------------------------------------------------------------------
def rns(vals, mods):
    return np.stack([np.array([int(v) % int(m) for v in vals], dtype=np.uint64) for m in mods])


def crt(limbs, mods):
    """(len(mods), N) residues -> N Python ints in [0, prod(mods))"""
    M = prod(mods)
    w = [(M // m) * pow(M // m, -1, m) for m in mods]
    return [sum(int(limbs[i][j]) * w[i] for i in range(len(mods))) % M for j in range(limbs.shape[1])]


def centered(vals, M):
    """the representative the reference's centred extensions carry: ((v + floor(M/2)) mod M) - floor(M/2)"""
    h = M >> 1
    return [((int(v) + h) % M) - h for v in vals]


def negacyclic_mul_small(a, s):
    """a * s in Z[X]/(X^N+1) for a list of Python ints a and a small-coefficient s, exact"""
    N = len(a)
    a = np.array(a, dtype=object)
    acc = np.zeros(N, dtype=object)
    for j, sj in enumerate(s):
        sj = int(sj)
        if sj:
            acc = acc + sj * np.concatenate([-a[N - j:], a[:N - j]])
    return list(acc)


def negacyclic_mul_mod_t(m0, m1, t):
    """m0 * m1 mod (X^N+1, t) for coefficients below 2^20 (int64 is exact up to N = 2^20)"""
    N = len(m0)
    full = np.convolve(np.asarray(m0, dtype=np.int64), np.asarray(m1, dtype=np.int64))
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return [int(x) % t for x in out]


def encrypt(rnd, P, level, m, s):
    """a degree-1 ciphertext of scale 1 with phase c0 + c1 s = m T^-1 + e (mod Q_level), |e| <= 3; NTT domain, [c0, c1]"""
    Ql, _, srQ, _ = P.at(level)
    Qb = prod(Ql)
    tinv = pow(P.t, -1, Qb)
    a = [rnd.randrange(Qb) for _ in range(P.N)]
    e = [rnd.randrange(-3, 4) for _ in range(P.N)]
    a_s = negacyclic_mul_small(a, s)
    c0 = [(int(mi) * tinv + ei - x) % Qb for mi, ei, x in zip(m, e, a_s)]
    return [ntt(rns(c0, Ql), srQ), ntt(rns(a, Ql), srQ)]


def decrypt_product(P, level, c, s):
    """d = T (c0 + c1 s + c2 s^2) centred modulo Q_level, then d mod t: N Python ints"""
    Ql, _, srQ, _ = P.at(level)
    Qb = prod(Ql)
    v = [crt(intt(ck, srQ), Ql) for ck in c]
    c1s = negacyclic_mul_small(v[1], s)
    c2s2 = negacyclic_mul_small(negacyclic_mul_small(v[2], s), s)
    d = centered([P.t * (x + y + z) for x, y, z in zip(v[0], c1s, c2s2)], Qb)
    return [x % P.t for x in d]

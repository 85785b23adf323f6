"""core/rgsw/blindrot restated on the CPU over tests/rlwe_restatement.py and the pinned oracle pieces: GenEvaluationKeyNew (keys.go:45-108), Evaluate and
BlindRotateCore (evaluator.go:46-229), InitTestPolynomial (blindrot.go:12-39), and the 32-bit external product as the reference's literal loop
(core/rgsw/evaluator.go:54-61, :82-117: NTTLazy digits, wrapping 64-bit products, IMForm).  TEST INFRASTRUCTURE ONLY: what the device path of
matrix_fhe_lattigo_amd.blindrot is compared with, bit for bit, and what tests/test_blindrot_oracle.py pins to decryption.

Single-modulus rings without P, keys with a power-of-two decomposition (the reference's own test setting).  Polys are (1, N) uint64 arrays, NTT
domain; a ciphertext is a list of two."""
import functools
import math

import numpy as np

import rlwe_restatement as rr
from oracle import ring_oracle as orc
from oracle.compose import OPS
from oracle import compose

GaloisGen, windowSize = 5, 10


@functools.lru_cache(maxsize=None)
def _consts(q):
    L = orc.lib()
    b = np.zeros(2, dtype=np.uint64)
    L.orc_gen_bred_constant(int(q), orc._p(b))
    return L.orc_gen_mred_constant(int(q)), b


def _op(name, p1, p2, p3, q, s0=0, s1=0):
    mred, bred = _consts(int(q))
    return orc.vec_op(OPS[name], p1, p2, p3, s0, s1, q, mred, bred)


# ---- blindrot.go, utils.go ------------------------------------------------------------------------------------------------------------------------
def scale_up(value, scale, Q):
    """utils.go:26-53: big.Float at 53 bits is float64: floor(|scale value| + 0.5) mod Q, Q - that for a negative value"""
    neg = value < 0
    x = -scale * value if neg else scale * value
    res = int(math.floor(x + 0.5)) % Q
    return Q - res if neg else res


def lut_coeffs(g, scale, N, q, a=-1.0, b=1.0):
    """InitTestPolynomial before its NTT: N residues"""
    norm = lambda x: (x * (b - a) + b + a) / 2.0
    interval = 2.0 / float(N)
    F = [scale_up(g(norm(-interval * float(i))), scale, q) for i in range((N >> 1) + 1)]
    F += [scale_up(-g(norm(interval * float(N - i))), scale, q) for i in range((N >> 1) + 1, N)]
    return F


def init_test_polynomial(g, scale, N, q, a=-1.0, b=1.0):
    return rr.ntt(np.array([lut_coeffs(g, scale, N, q, a, b)], dtype=np.uint64), N, [q])


# ---- keys.go --------------------------------------------------------------------------------------------------------------------------------------
def monomial(N, i):
    """ring.NewMonomialXi (ring/ring.go:408-430) as small integers"""
    i &= 2 * N - 1
    m = [0] * N
    if i >= N:
        m[i - N] = -1
    else:
        m[i] = 1
    return m


def galois_elements(N):
    return [pow(GaloisGen, i + 1, 2 * N) for i in range(windowSize)] + [2 * N - GaloisGen]


class KeySet:
    """BlindRotationKeys: per LWE secret coefficient the two rr.GadgetKey of RGSW(X^{s_i}); AutomorphismKeys: {Galois element: rr.GadgetKey}"""

    def __init__(self, brk, gks, pw2):
        self.BlindRotationKeys, self.AutomorphismKeys, self.pw2 = brk, gks, pw2


def gen_evaluation_key(rnd, N, q, sk_br, sk_lwe, pw2):
    """GenEvaluationKeyNew (keys.go:45-108): s_i read centred from the LWE secret, RGSW(X^{s_i}) under sk_br, and the 11 Galois keys"""
    Q = [int(q)]
    brk = [rr.rgsw_encrypt(rnd, sk_br, monomial(N, int(si)), Q, [], 0, -1, pw2) for si in sk_lwe.coeffs]
    gks = {g: rr.galois_key(rnd, sk_br, g, Q, [], 0, -1, pw2) for g in galois_elements(N)}
    return KeySet(brk, gks, pw2)


# ---- core/rgsw/evaluator.go ---------------------------------------------------------------------------------------------------------------------
def external_product_32bit(N, q, ct, key, pw2):
    """externalProduct32Bit (:82-117) and the two IMForm that close it (:60-61), statement by statement.  ct: [c0, c1] (1, N) NTT-domain;
    key: [GadgetKey, GadgetKey].  The accumulators are plain 64-bit words: MulCoeffsLazy(ThenAddLazy) wraps, and never has to (:57)."""
    assert int(q) >> 29 == 0
    sr = rr.subring(N, q)
    mask = (1 << pw2) - 1
    acc = [np.zeros(N, dtype=np.uint64), np.zeros(N, dtype=np.uint64)]
    for i in (0, 1):
        inv = orc.intt(ct[i][0], sr)                                            # ringQ.INTT(ct0.Value[i], eval.BuffInvNTT)
        for j in range(key[i].Q.shape[0]):
            cw = _op("MASK", inv, None, np.zeros(N, dtype=np.uint64), q, j * pw2, mask)
            cwn = orc.ntt(cw, sr, lazy=True)                                    # subRing.NTTLazy(cw, cwNTT)
            name = "MUL_LAZY" if (i == 0 and j == 0) else "MUL_LAZY_THEN_ADD_LAZY"
            for c in (0, 1):
                acc[c] = _op(name, key[i].Q[j, c, 0], cwn, acc[c], q)
    return [_op("IMFORM", acc[c], None, acc[c], q)[None] for c in (0, 1)]


def external_product_montgomery(N, q, ct, key, pw2):
    """externalProductInPlaceSinglePAndBitDecomp + CopyLvl (:62-72, :119-186) over the oracle composition"""
    dpl = key[0].digits_per_limb
    out = compose.external_product_single_p(N, [int(q)], [], 0, -1, np.stack([ct[0], ct[1]]), pw2, dpl, [key[0].Q, key[1].Q], [None, None])
    return [np.asarray(out[0]), np.asarray(out[1])]


def external_product(N, q, ct, key, pw2):
    """ExternalProduct (:42-80) at levelQ = 0, levelP = -1: the branch the reference takes for this modulus"""
    return (external_product_32bit if int(q) >> 29 == 0 else external_product_montgomery)(N, q, ct, key, pw2)


def automorphism(N, q, ct, gk, g):
    return rr.automorphism(N, [int(q)], [], ct, gk, g)


# ---- evaluator.go ---------------------------------------------------------------------------------------------------------------------------------
def galois_inverse_map(N):
    out, pw = {}, 1
    for i in range(N >> 1):
        out[pw] = i
        out[2 * N - pw] = -i
        pw = pw * GaloisGen & (2 * N - 1)
    return out


def discrete_log_sets(a, N):
    dlog, sets = galois_inverse_map(N), {}
    for i, ai in enumerate(a):
        if ai & 1 != 1 and ai != 0:
            raise ValueError("getDiscreteLogSets: a[i] is not odd")
        sets.setdefault(dlog.get(ai, 0), []).append(i)                          # a missing key reads as 0, like a Go map
    return sets


def blind_rotate_core(a, N, ext, auto):
    """BlindRotateCore (:134-186) with evaluateFromDiscreteLogSets (:189-229) inlined as `step`; ext(j) / auto(g) act on the caller's accumulator"""
    sets = discrete_log_sets(a, N)
    gal = lambda k: pow(GaloisGen, k, 2 * N)

    def step(k, v):
        if k in sets:
            if v != 0:
                auto(gal(v))
                v = 0
            for j in sets[k]:
                ext(j)
        v += 1
        if v == windowSize or k == 1:
            auto(gal(v))
            v = 0
        return v

    v = 0
    for i in range((N >> 1) - 1, 0, -1):
        v = step(-i, v)
    step(N << 1, 0)
    auto(2 * N - GaloisGen)
    for i in range((N >> 1) - 1, 0, -1):
        v = step(i, v)
    step(0, 0)


def program(a, N):
    """the steps BlindRotateCore issues, as (kind, argument) pairs"""
    out = []
    blind_rotate_core(a, N, lambda j: out.append(("EXT", j)), lambda g: out.append(("AUTO", g)))
    return out


def run_program(prog, N, q, acc, keys):
    for kind, x in prog:
        if kind == "EXT":
            acc = external_product(N, q, acc, keys.BlindRotationKeys[x], keys.pw2)
        else:
            acc = automorphism(N, q, acc, keys.AutomorphismKeys[x], x)
    return acc


def mod_switch(coeffs, Q, twoN, make_odd):
    out = []
    for x in coeffs:
        y, r = divmod(int(x) * twoN, Q)
        if 2 * r >= Q:
            y += 1
        y &= twoN - 1
        if make_odd and y & 1 == 0 and y != 0:
            y ^= 1
        out.append(y)
    return out


def lwe_samples(ct, is_ntt, NLWE, qlwe, NBR, indices):
    """(:62-103): {index: (a, b)} modulo 2 N_BR for the requested indices, walked in ascending order.  ct: [c0, c1] (1, N_LWE)"""
    c = [rr.intt(x, NLWE, [qlwe])[0] if is_ntt else np.asarray(x)[0] for x in ct]
    mask = 2 * NBR - 1
    a2n = mod_switch(c[1], qlwe, 2 * NBR, True)
    a = [a2n[0]] + [-a2n[NLWE - j] & mask for j in range(1, NLWE)]
    b2n = mod_switch(c[0], qlwe, 2 * NBR, False)
    out, prev = {}, 0
    for index in sorted(i for i in indices if 0 <= i < NLWE):
        n = index - prev
        if n:
            a = a[NLWE - n:] + a[:NLWE - n]
            for j in range(n):
                a[j] = -a[j] & mask
        prev = index
        out[index] = (list(a), b2n[index])
    return out


def initial_accumulator(N, q, F, b):
    """(:108-113): (phi_{2N - g}(F * NTT(X^b)), 0)"""
    xb = rr.small_ntt_mont(monomial(N, b), N, [q])
    prod = rr._vec("MUL_MONT", F, xb, [q])
    return [np.stack([orc.automorphism_ntt(prod[0], 2 * N - GaloisGen)]), np.zeros((1, N), dtype=np.uint64)]


def evaluate(ct, is_ntt, NLWE, qlwe, NBR, q, test_polys, keys, ntt_flag=True):
    """Evaluate (:46-132): {index: [c0, c1]}"""
    res = {}
    for index, (a, b) in lwe_samples(ct, is_ntt, NLWE, qlwe, NBR, test_polys.keys()).items():
        acc = run_program(program(a, NBR), NBR, q, initial_accumulator(NBR, q, test_polys[index], b), keys)
        res[index] = acc if ntt_flag else [rr.intt(x, NBR, [q]) for x in acc]
    return res


# ---- what the rotation must be, from the algorithm ----------------------------------------------------------------------------------------------
def effective_a(a, N):
    """The value each a[i] acts as in the reference: 0 is not in the discrete-log map and reads as set 0 (like 1); 2N - 1 is stored as -0 = 0 and
    lands in set 0 as well (like 1)."""
    return [1 if x in (0, 2 * N - 1) else x for x in a]


def rotation(a, b, s, N):
    """u with acc -> F(X) X^u: the initial accumulator is F(X^-g) X^(-g b); every automorphism after a step multiplies the exponents gathered so far,
    and the automorphisms after the step of set k multiply to +-g^k = a[i] (the total is g^N = 1), so X^(s_i) enters as X^(a_i s_i) and X^(-g b)
    leaves as X^b: u = b + <a, s> mod 2N with the PLUS sign, a read through effective_a"""
    return (b + sum(x * int(y) for x, y in zip(effective_a(a, N), s))) % (2 * N)


def simulate_exponents(prog, s, N):
    """A direct evaluation of the step list on m = F(X^alpha) X^beta with beta's b-part left out: AUTO(g) maps (alpha, beta) to (alpha g, beta g),
    EXT(j) adds s_j to beta.  Starts from alpha = 2N - g (the initial automorphism)."""
    alpha, beta = 2 * N - GaloisGen, 0
    for kind, x in prog:
        if kind == "EXT":
            beta = (beta + int(s[x])) % (2 * N)
        else:
            alpha, beta = alpha * x % (2 * N), beta * x % (2 * N)
    return alpha, beta


# ---- the reference's own test setting (blindrot_test.go:48-167), built once per session and left unchanged ------------------------------------
def sign(x):
    return 1.0 if x > 0 else (0.0 if x == 0 else -1.0)


class Setting:
    pass


@functools.lru_cache(maxsize=None)
def setting(NBR, QBR, NLWE, QLWE, pw2, slots, seed):
    """keys, secrets, the sample ciphertext of `slots` values -1 + 2 i / slots at scale Q_LWE / 4 (NTT domain) and the sign test polynomial at
    scale Q_BR / 4, from one seeded generator"""
    import random
    rnd = random.Random(seed)
    st = Setting()
    st.NBR, st.QBR, st.NLWE, st.QLWE, st.pw2, st.slots = NBR, QBR, NLWE, QLWE, pw2, slots
    st.sk_lwe, st.sk_br = rr.Secret.sample(rnd, NLWE), rr.Secret.sample(rnd, NBR)
    st.values = [-1 + float(2 * i) / float(slots) for i in range(slots)]
    scale = float(QLWE) / 4.0
    st.pt = [0] * NLWE
    for i, v in enumerate(st.values):
        st.pt[i] = QLWE - int(-v * scale) if v < 0 else int(v * scale)
    st.ct, _ = rr.encrypt(rnd, st.sk_lwe, st.pt, [QLWE], 0)
    st.keys = gen_evaluation_key(rnd, NBR, QBR, st.sk_br, st.sk_lwe, pw2)
    st.scaleBR = float(QBR) / 4.0
    st.Fc = lut_coeffs(sign, st.scaleBR, NBR, QBR)
    st.F = rr.ntt(np.array([st.Fc], dtype=np.uint64), NBR, [QBR])
    return st


def expected_plaintext(Fc, q, u, N):
    """F(X) X^u as centred integers"""
    c = [x - q if 2 * x > q else x for x in (int(v) % q for v in Fc)]
    return rr.monomial_mul(c, u)

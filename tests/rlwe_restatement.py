"""A toy key generator, encryptor and decryptor over Python big integers and the pinned oracle pieces: the data-level behaviour of the reference's
core/rlwe key generator (keygenerator.go), gadget ciphertexts (gadgetciphertext.go), secret-key encryptor (encryptor.go) and core/rgsw encryptor
(core/rgsw/encryptor.go), restated so that the key-switch compositions (oracle/compose.py) and the device path can be pinned to DECRYPTION under real
keys, the statement the reference's own tests make (core/rlwe/rlwe_test.go:690-1079, core/rgsw/rgsw_test.go:61-113).
TEST INFRASTRUCTURE ONLY.  The one key generator under tests/: tests/test_bgv_oracle.py takes its relinearisation key from here too.

Polys are numpy uint64 arrays of shape (limbs, N).  Keys are in the NTT domain and in Montgomery form, in the (rows, 2, limbs, N) layout of
rh.rlwe.GadgetCiphertext; ciphertexts are lists of NTT-domain polys (not Montgomery); secrets and messages are lists of N Python ints.
Sampling draws from a seeded random.Random; nothing here is meant to be secure."""
import functools
import math
from fractions import Fraction

import numpy as np

from oracle import ring_oracle as orc
from oracle.compose import OPS

SIGMA, BOUND = 3.2, 19                                                   # rlwe.DefaultNoise, floor(DefaultNoiseBound) (core/rlwe/security.go:9-13)


def prod(mods):
    out = 1
    for m in mods:
        out *= int(m)
    return out


@functools.lru_cache(maxsize=None)
def subring(N, q):
    return orc.SubRingConsts(N, int(q))


def _vec(op, p1, p2, mods, s0=None):
    z = np.zeros(p1.shape[1], dtype=np.uint64)
    return np.stack([orc.vec_op(OPS[op], p1[i], p2[i] if p2 is not None else None, z, s0[i] if s0 is not None else 0, 0, mods[i])
                     for i in range(len(mods))])


def ntt(x, N, mods):
    return np.stack([orc.ntt(x[i], subring(N, q)) for i, q in enumerate(mods)])


def intt(x, N, mods):
    return np.stack([orc.intt(x[i], subring(N, q)) for i, q in enumerate(mods)])


def rns(vals, mods):
    v = np.array([int(x) for x in vals], dtype=object)
    return np.stack([(v % int(q)).astype(np.uint64) for q in mods])


def crt_centered(limbs, mods):
    """ring.PolyToBigintCentered (ring/ring.go:503-560): (len(mods), N) residues -> N Python ints in (-Q/2, Q/2]"""
    M = prod(mods)
    acc = np.zeros(limbs.shape[1], dtype=object)
    for i, q in enumerate(mods):
        w = (M // int(q)) * pow(M // int(q), -1, int(q))
        acc = acc + limbs[i].astype(object) * w
    acc = acc % M
    return [int(x) - M if 2 * int(x) > M else int(x) for x in acc]


def small_ntt_mont(vals, N, mods):
    """a poly with small integer coefficients under every modulus of `mods`, NTT domain, Montgomery form (how SecretKey.Value is held, and what
    ExtendBasisSmallNormAndCenterNTTMontgomery gives for the other moduli, core/rlwe/utils.go:250-266)"""
    return _vec("MFORM", ntt(rns(vals, mods), N, mods), None, mods)


# ---- index maps on coefficient lists (plain integers: independent of the oracle's automorphisms) -------------------------------------------------
def automorphism_coeffs(m, g):
    """m(X) -> m(X^g) in Z[X]/(X^N+1) (ring.Automorphism, ring/automorphism.go:113-128, on integers)"""
    N = len(m)
    out = [0] * N
    for i, x in enumerate(m):
        j = i * g % (2 * N)
        if j >= N:
            out[j - N] = -x
        else:
            out[j] = x
    return out


def monomial_mul(m, k):
    """m(X) * X^k in Z[X]/(X^N+1)"""
    N = len(m)
    out = [0] * N
    for i, x in enumerate(m):
        j = (i + k) % (2 * N)
        if j >= N:
            out[j - N] -= x
        else:
            out[j] += x
    return out


def negacyclic_mul(a, b):
    """a * b in Z[X]/(X^N+1), exact on int64: |a_i b_j| N < 2^63 is the caller's business"""
    N = len(a)
    full = np.convolve(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64))
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return [int(x) for x in out]


def galois_inverse(N, g):
    """Parameters.ModInvGaloisElement (core/rlwe/params.go:677-681): g^(2N-1) mod 2N"""
    return pow(int(g), 2 * N - 1, 2 * N)


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------------
def uniform_poly(rnd, N, mods):
    """ring.UniformSampler: i.i.d. uniform residues per limb (96 random bits reduced: a bias below 2^-32 for every modulus below 2^64)"""
    return np.stack([np.array([rnd.getrandbits(96) % int(q) for _ in range(N)], dtype=np.uint64) for q in mods])


def gaussian_coeffs(rnd, N):
    """ring.GaussianSampler with the reference's default error (DefaultXe, core/rlwe/security.go:9-17): a rounded Gaussian of sigma 3.2 truncated at 19"""
    out = []
    while len(out) < N:
        x = int(round(rnd.gauss(0.0, SIGMA)))
        if abs(x) <= BOUND:
            out.append(x)
    return out


class Secret:
    """rlwe.SecretKey (GenSecretKey, core/rlwe/keygenerator.go:39-72): a ternary poly, held as its N small ints and, per modulus, as an
    NTT-domain Montgomery-form row.  Each coefficient is -1, 0 or 1 with probability 1/3 (DefaultXs = ring.Ternary{P: 2/3}, core/rlwe/security.go:19)."""

    def __init__(self, N, coeffs):
        self.N, self.coeffs = N, [int(x) for x in coeffs]
        self._rows = {}

    @classmethod
    def sample(cls, rnd, N):
        return cls(N, [rnd.randrange(-1, 2) for _ in range(N)])

    def rows(self, mods):
        """(len(mods), N): NTT domain, Montgomery form"""
        miss = [int(q) for q in mods if int(q) not in self._rows]
        if miss:
            for q, r in zip(miss, small_ntt_mont(self.coeffs, self.N, miss)):
                self._rows[q] = r
        return np.stack([self._rows[int(q)] for q in mods])

    def automorphism(self, g):
        return Secret(self.N, automorphism_coeffs(self.coeffs, g))

    def square(self):
        return Secret(self.N, negacyclic_mul(self.coeffs, self.coeffs))


def encrypt_zero(rnd, sk, mods):
    """Encryptor.encryptZeroSk (core/rlwe/encryptor.go:355-463) for an NTT-domain, Montgomery-form element: (-a sk + e, a) with a uniform (the
    uniform sample IS the Montgomery form of a uniform poly) and e the default Gaussian.  Returns (b, a, e): two (len(mods), N) arrays and e's ints."""
    N = sk.N
    mods = [int(q) for q in mods]
    a = uniform_poly(rnd, N, mods)
    e = gaussian_coeffs(rnd, N)
    e_m = small_ntt_mont(e, N, mods)
    a_s = _vec("MUL_MONT", a, sk.rows(mods), mods)                      # a R * s R / R = (a s) R
    return _vec("SUB", e_m, a_s, mods), a, e


# ---- gadget ciphertexts ----------------------------------------------------------------------------------------------------------------------------
def rns_digits(levelQ, levelP):
    """Parameters.BaseRNSDecompositionVectorSize (core/rlwe/params.go:634-642)"""
    return levelQ + 1 if levelP == -1 else (levelQ + levelP + 1) // (levelP + 1)


def digits_per_limb(Q, levelQ, levelP, pw2):
    """Parameters.BaseTwoDecompositionVectorSize (core/rlwe/params.go:613-632) for the RNS digits of a gadget ciphertext at (levelQ, levelP):
    ceil(round(log2 q_i) / pw2), or 1 without a power-of-two decomposition or with more than one P modulus"""
    n = rns_digits(levelQ, levelP)
    if pw2 == 0 or levelP > 0:
        return [1] * n
    return [(int(round(math.log2(float(int(q))))) + pw2 - 1) // pw2 for q in Q[:n]]


def _gadget(rnd, sk_out, pt_rows, Q, P, levelQ, levelP, pw2, count):
    """`count` gadget ciphertexts (1: an evaluation key, 2: an RGSW ciphertext) at (levelQ, levelP): every row an encryption of zero under sk_out
    (genEvaluationKey, core/rlwe/keygenerator.go:276-309; rgsw EncryptZero, core/rgsw/encryptor.go:74-118), then pt times the gadget vector added to
    component u of ciphertext u (AddPolyTimesGadgetVectorToGadgetCiphertext, core/rlwe/gadgetciphertext.go:172-241): row (i, j) gains
    P * 2^(j pw2) * pt on the Q-limbs i (levelP+1) + k, k <= levelP, that exist at levelQ; the factor is 1 and the digits single limbs without P.
    pt_rows: (levelQ+1, N), NTT domain, Montgomery form.  Row (i, j) is flat row sum(dpl[:i]) + j: Value[i][j], which the evaluators read with i in
    the outer and j in the inner loop (core/rlwe/evaluator_gadget_product.go:226-236).
    Returns [(valueQ, valueP or None)] * count and dpl."""
    N = sk_out.N
    Ql, Pl = [int(q) for q in Q[:levelQ + 1]], [int(p) for p in P[:levelP + 1]] if levelP >= 0 else []
    mods = Ql + Pl
    dpl = digits_per_limb(Q, levelQ, levelP, pw2)
    Pb = prod(Pl)                                                       # 1 without P (:183-188)
    width = max(levelP, 0) + 1
    out = [[] for _ in range(count)]
    for i in range(len(dpl)):
        for j in range(dpl[i]):
            f = Pb << (j * pw2)                                         # P * w^j (:184, :237)
            for u in range(count):
                b, a, _ = encrypt_zero(rnd, sk_out, mods)
                row = [b, a]
                for k in range(width):
                    index = i * width + k                               # (:215)
                    if index >= levelQ + 1:                             # #pj does not divide #qi (:217-220)
                        break
                    q = Ql[index]
                    term = orc.vec_op(OPS["MUL_SCALAR_MONT"], pt_rows[index], None, np.zeros(N, dtype=np.uint64), (f << 64) % q, 0, q)
                    row[u][index] = orc.vec_op(OPS["ADD"], row[u][index], term, row[u][index], 0, 0, q)      # (:225-230)
                out[u].append(np.stack(row))
    res = []
    for rows in out:
        key = np.stack(rows)                                            # (rows, 2, limbs of Q then P, N)
        res.append((key[:, :, :levelQ + 1].copy(), key[:, :, levelQ + 1:].copy() if Pl else None))
    return res, dpl


class GadgetKey:
    """one gadget ciphertext as rh.rlwe.GadgetCiphertext takes it: Q / P (rows, 2, limbs, N), pw2, digits_per_limb (None without pw2)"""

    def __init__(self, Q, P, levelQ, levelP, pw2, dpl):
        self.Q, self.P, self.levelQ, self.levelP, self.pw2 = Q, P, levelQ, levelP, pw2
        self.digits_per_limb = dpl if pw2 else None


def gadget_key(rnd, sk_in, sk_out, Q, P, levelQ, levelP, pw2=0):
    """GenEvaluationKey (core/rlwe/keygenerator.go:256-316): re-encrypts from sk_in to sk_out"""
    (kq, kp), = _gadget(rnd, sk_out, sk_in.rows(Q[:levelQ + 1]), Q, P, levelQ, levelP, pw2, 1)[0]
    return GadgetKey(kq, kp, levelQ, levelP, pw2, digits_per_limb(Q, levelQ, levelP, pw2))


def relin_key(rnd, sk, Q, P, levelQ, levelP, pw2=0):
    """GenRelinearizationKey (core/rlwe/keygenerator.go:115-120): sk_in = sk^2, sk_out = sk"""
    return gadget_key(rnd, sk.square(), sk, Q, P, levelQ, levelP, pw2)


def galois_key(rnd, sk, g, Q, P, levelQ, levelP, pw2=0):
    """GenGaloisKey (core/rlwe/keygenerator.go:140-174): sk_in = sk, sk_out = pi_{g^-1}(sk) -- the gadget product re-encrypts under pi_{g^-1}(sk) and
    the automorphism of g that follows it brings the ciphertext back under sk (:150-153)"""
    return gadget_key(rnd, sk, sk.automorphism(galois_inverse(sk.N, g)), Q, P, levelQ, levelP, pw2)


def rgsw_encrypt(rnd, sk, m, Q, P, levelQ, levelP, pw2=0):
    """rgsw.Encryptor.Encrypt (core/rgsw/encryptor.go:25-70): two gadget ciphertexts of zero, m times the gadget vector added to component 0 of the
    first and component 1 of the second (the `u` loop of gadgetciphertext.go:225-231).  Returns [GadgetKey, GadgetKey]."""
    pt = small_ntt_mont(m, sk.N, Q[:levelQ + 1])
    res, dpl = _gadget(rnd, sk, pt, Q, P, levelQ, levelP, pw2, 2)
    return [GadgetKey(kq, kp, levelQ, levelP, pw2, dpl) for kq, kp in res]


# ---- rlwe ciphertexts ------------------------------------------------------------------------------------------------------------------------------
def encrypt(rnd, sk, m, Q, level):
    """Encryptor.Encrypt with a secret key (core/rlwe/encryptor.go:148-175, :355-430, addPtToCt :512-530): (-a sk + e + m, a), NTT domain.  Returns ([c0, c1], e)."""
    mods = [int(q) for q in Q[:level + 1]]
    N = sk.N
    a = uniform_poly(rnd, N, mods)
    e = gaussian_coeffs(rnd, N)
    me = ntt(rns([x + y for x, y in zip(m, e)], mods), N, mods)
    return [_vec("SUB", me, _vec("MUL_MONT", a, sk.rows(mods), mods), mods), a], e


def phase(ct, sk, Q):
    """Decryptor.Decrypt (core/rlwe/decryptor.go:51-92) followed by PolyToBigintCentered: c0 + c1 s (+ c2 s^2), Horner in s limb-wise in the NTT
    domain, one INTT, one CRT, centred modulo the product of the ciphertext's moduli.  N Python ints."""
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    s = sk.rows(mods)
    acc = np.asarray(ct[-1], dtype=np.uint64)
    for c in reversed(ct[:-1]):
        acc = _vec("ADD", _vec("MUL_MONT", acc, s, mods), np.asarray(c, dtype=np.uint64), mods)
    return crt_centered(intt(acc, sk.N, mods), mods)


def centered_diff(a, b, M):
    """a - b centred modulo M"""
    out = []
    for x, y in zip(a, b):
        d = (x - y) % M
        out.append(d - M if 2 * d > M else d)
    return out


def log2_std(coeffs):
    """Ring.Log2OfStandardDeviation (ring/ring.go:647-686): log2 of the sample standard deviation (N-1 in the denominator) of the centred
    coefficients; exact rationals here instead of 128-bit floats"""
    n = len(coeffs)
    mean = Fraction(sum(coeffs), n)
    var = sum((Fraction(x) - mean) ** 2 for x in coeffs) / (n - 1)
    if var == 0:
        return float("-inf")
    return 0.5 * (math.log2(var.numerator) - math.log2(var.denominator))


# ---- the evaluators' call sequences over the oracle compositions (what the device path is compared with, bit for bit) ---------------------------
def gadget_product(N, Q, P, levelQ, cx, key, is_ntt=True):
    """Evaluator.GadgetProduct (core/rlwe/evaluator_gadget_product.go:16-30, :102-113): the multi-P or the single-P / bit-decomposition branch by
    key.levelP, at min(levelQ, key.levelQ)"""
    from oracle import compose
    levelQ = min(levelQ, key.levelQ)
    if key.levelP >= 1:
        f = compose.gadget_product if is_ntt else compose.gadget_product_coeff
        return f(N, Q, P, levelQ, key.levelP, cx, key.Q, key.P)
    dpl = key.digits_per_limb[:levelQ + 1] if key.pw2 else None
    return compose.gadget_product_single_p(N, Q, P, levelQ, key.levelP, cx, is_ntt, key.pw2, dpl, key.Q, key.P)


def _add(a, b, mods):
    return _vec("ADD", np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64), mods)


def apply_evaluation_key(N, Q, P, ct, key):
    """applyEvaluationKey (core/rlwe/evaluator_evaluationkey.go:105-112): (c0 + KS(c1)_0, KS(c1)_1)"""
    level = ct[0].shape[0] - 1
    k0, k1 = gadget_product(N, Q, P, level, ct[1], key)
    return [_add(ct[0], k0, Q[:level + 1]), k1]


def relinearize(N, Q, P, ct, key):
    """Relinearize (core/rlwe/evaluator_evaluationkey.go:125-153): (c0 + KS(c2)_0, c1 + KS(c2)_1)"""
    level = ct[0].shape[0] - 1
    k0, k1 = gadget_product(N, Q, P, level, ct[2], key)
    return [_add(ct[0], k0, Q[:level + 1]), _add(ct[1], k1, Q[:level + 1])]


def automorphism(N, Q, P, ct, key, g, map_g=None):
    """Evaluator.Automorphism (core/rlwe/evaluator_automorphism.go:14-60): the key switch with GaloisKey[g], then AutomorphismNTT of g on both
    components.  map_g: the element whose index map is applied, when it is not g (the negative controls)."""
    out = apply_evaluation_key(N, Q, P, ct, key)
    g = g if map_g is None else map_g
    return [np.stack([orc.automorphism_ntt(x[i], g) for i in range(x.shape[0])]) for x in out]

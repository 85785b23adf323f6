"""The noise meters of the reference restated over Python integers and the pinned oracle pieces: ring.PolyToBigintCentered and
Log2OfStandardDeviation (ring/ring.go:503-543, :647-686), the Noise* functions, Norm and NormStats of core/rlwe/utils.go:13-183 and
rgsw.NoiseRGSWCiphertext (core/rgsw/utils.go), written from those line references.
What matrix-fhe-lattigo_amd/noise.py is compared with.  TEST INFRASTRUCTURE ONLY.

Polys are numpy uint64 arrays (limbs, N) or lists of rows of Python ints; keys are rr.GadgetKey, secrets rr.Secret (tests/rlwe_restatement.py)."""
import math
from fractions import Fraction

import mpmath
import numpy as np

import rlwe_restatement as rr
from oracle import ring_oracle as orc


# ---- centred CRT and moments --------------------------------------------------------------------------------------------------------------------------
def centred(limbs, mods, gap=1):
    """PolyToBigintCentered(p, gap, .): v = CRT of the residues of coefficient i gap, v - M when v >= floor(M / 2) (`sign == 1 || sign == 0`)"""
    mods = [int(m) for m in mods]
    M = rr.prod(mods)
    w = [(M // m) * pow(M // m, -1, m) for m in mods]
    half = M >> 1
    out = []
    for j in range(0, len(limbs[0]), gap):
        v = sum(int(limbs[i][j]) % mods[i] * w[i] for i in range(len(mods))) % M
        out.append(v - M if v >= half else v)
    return out


def moments(xs):
    xs = [int(x) for x in xs]
    return len(xs), sum(xs), sum(x * x for x in xs), min(abs(x) for x in xs), max(abs(x) for x in xs)


def log2_of(x):
    """log2 of a non-negative rational at 256 bits, one rounding to float64; -inf at 0"""
    x = Fraction(x)
    if x == 0:
        return -math.inf
    with mpmath.workprec(256):
        return float(mpmath.log(mpmath.mpf(x.numerator) / mpmath.mpf(x.denominator), 2))


def log2_std(n, S1, S2, divisor=None):
    """log2 sqrt((S2 - S1^2 / n) / divisor) with exact rationals, sqrt and log2 at 256 bits, one rounding; divisor n - 1 unless given"""
    divisor = n - 1 if divisor is None else divisor
    if n == 0 or divisor == 0:
        return math.nan
    var = Fraction(n * S2 - S1 * S1, n * divisor)
    if var == 0:
        return -math.inf
    with mpmath.workprec(256):
        return float(mpmath.log(mpmath.sqrt(mpmath.mpf(var.numerator) / mpmath.mpf(var.denominator)), 2))


def log2_std_of(xs):
    n, S1, S2, _, _ = moments(xs)
    return log2_std(n, S1, S2)


def norm_stats(xs):
    n, S1, S2, lo, hi = moments(xs)
    return log2_std(n, S1, S2, divisor=n), log2_of(lo), log2_of(hi)


# ---- the Go loops, step for step, at the precisions Go runs them ------------------------------------------------------------------------------------------
def go_log2_std(xs):
    """ring.go:661-685 with every big.Float operation rounded to 128 bits (bignum.NewFloat(., 128); SetInt on a receiver of precision 128 rounds)"""
    with mpmath.workprec(128):
        N = len(xs)
        mean = mpmath.mpf(0)
        for x in xs:
            mean = mean + mpmath.mpf(int(x))
        mean = mean / mpmath.mpf(float(N))
        std = mpmath.mpf(0)
        for x in xs:
            t = mpmath.mpf(int(x)) - mean
            t = t * t
            std = std + t
        std = std / mpmath.mpf(float(N - 1))
        std = mpmath.sqrt(std)
        f = float(std) if std < mpmath.mpf(2) ** 1024 else math.inf       # big.Float.Float64 overflows to +Inf
        return math.log2(f) if f != 0 else -math.inf


def go_norm_stats(xs):
    """utils.go:135-183: the running sums are big.Floats made by SetFloat64 (precision 53); Add, Sub, Mul and Quo round to the receiver's precision
    once it is set, or to the largest operand precision when it is 0 -- the integers themselves enter at max(bit length, 64) bits.  Restated with a
    64-bit mantissa for every operation, the least precision any step of it keeps for integers below 2^64."""
    with mpmath.workprec(64):
        vf = [mpmath.mpf(int(x)) for x in xs]
        lo = min(abs(int(x)) for x in xs)
        hi = max(abs(int(x)) for x in xs)
        n = mpmath.mpf(float(len(xs)))
        mean = mpmath.mpf(0)
        for c in vf:
            mean = mean + c
        mean = mean / n
        err = mpmath.mpf(0)
        for c in vf:
            t = c - mean
            t = t * t
            err = err + t
        err = mpmath.sqrt(err / n)
        lg = lambda v: math.log2(float(v)) if v != 0 else -math.inf
        return lg(err), lg(mpmath.mpf(lo)), lg(mpmath.mpf(hi))


# ---- a model of what rh_ring_centered_moments writes (include/ringhip.h): mixed-radix digits and their pair sums -----------------------------------------
def mixed_radix(v, mods):
    out = []
    for m in mods:
        out.append(v % m)
        v //= m
    return out


def moments_block(limbs, mods, gap=1):
    """the output block of one poly as a list of words: the 192-bit pair sums of the digit rows d_0 .. d_{L-1}, 1, c, then the digits of the
    smallest and of the largest |x|"""
    mods = [int(m) for m in mods]
    L, M = len(mods), rr.prod(mods)
    xs = centred(limbs, mods, gap)
    rows = []
    for x in xs:
        v = x % M
        rows.append(mixed_radix(v, mods) + [1, 1 if x != v else 0])
    words = []
    for i in range(L + 2):
        for j in range(i, L + 2):
            s = sum(r[i] * r[j] for r in rows)
            words += [s & (2 ** 64 - 1), (s >> 64) & (2 ** 64 - 1), s >> 128]
    ab = [abs(x) for x in xs]
    return words + mixed_radix(min(ab), mods) + mixed_radix(max(ab), mods)


# ---- the Noise* functions (core/rlwe/utils.go) over restatement keys ---------------------------------------------------------------------------------------
def _mods(key, Q, P):
    Ql = [int(q) for q in Q[:key.levelQ + 1]]
    Pl = [int(p) for p in P[:key.levelP + 1]] if key.levelP >= 0 else []
    return Ql, Pl


def gadget_phase(key, pt_rows, sk_out, Q, P):
    """utils.go:62-88 and :95-99 up to the INTT: per j < min_i len(Value[i]) the (LQ + LP, N) rows of
    sum_i (Value[i][j][0] + Value[i][j][1] sk) - pt P 2^(j pw2) (the subtraction on Q alone), NTT domain, Montgomery form"""
    Ql, Pl = _mods(key, Q, P)
    mods = Ql + Pl
    N = sk_out.N
    dpl = key.digits_per_limb if key.digits_per_limb is not None else [1] * key.Q.shape[0]
    first = [sum(dpl[:i]) for i in range(len(dpl))]
    s = sk_out.rows(mods)
    out = []
    pt = None if pt_rows is None else np.asarray(pt_rows, dtype=np.uint64)[:len(Ql)].copy()
    if pt is not None and Pl:
        pt = rr._vec("MUL_SCALAR_MONT", pt, None, Ql, s0=[(rr.prod(Pl) << 64) % q for q in Ql])
    for j in range(min(dpl)):
        acc = None
        for f in first:
            val = key.Q[f + j] if not Pl else np.concatenate([key.Q[f + j], key.P[f + j]], axis=1)
            z = rr._vec("ADD", rr._vec("MUL_MONT", val[1], s, mods), val[0], mods)
            acc = z if acc is None else rr._vec("ADD", acc, z, mods)
        if pt is not None:
            acc[:len(Ql)] = rr._vec("SUB", acc[:len(Ql)], pt, Ql)
            pt = rr._vec("MUL_SCALAR_MONT", pt, None, Ql, s0=[((1 << key.pw2) << 64) % q for q in Ql])
        out.append(acc)
    return out


def phase_noise(rows, N, mods):
    """INTT, IMForm, Log2OfStandardDeviation modulo QP (:90-93)"""
    z = rr._vec("IMFORM", rr.intt(rows, N, mods), None, mods)
    return log2_std_of(centred(z, mods))


def noise_gadget_list(key, pt_rows, sk_out, Q, P):
    Ql, Pl = _mods(key, Q, P)
    return [phase_noise(z, sk_out.N, Ql + Pl) for z in gadget_phase(key, pt_rows, sk_out, Q, P)]


def noise_gadget(key, pt_rows, sk_out, Q, P):
    """NoiseGadgetCiphertext (:51-102): the running maximum starts at 0"""
    m = 0.0
    for v in noise_gadget_list(key, pt_rows, sk_out, Q, P):
        m = max(m, v)
    return m


def noise_public_key(pkq, pkp, sk, Q, P):
    """NoisePublicKey (:13-25); pkq: (1, 2, LQ, N), pkp: (1, 2, LP, N) or None"""
    key = rr.GadgetKey(pkq, pkp, pkq.shape[2] - 1, (pkp.shape[2] - 1) if pkp is not None else -1, 0, None)
    return noise_gadget_list(key, None, sk, Q, P)[0]


def noise_evaluation_key(key, sk_in, sk_out, Q, P):
    return noise_gadget(key, sk_in.rows(Q[:key.levelQ + 1]), sk_out, Q, P)


def noise_relin_key(key, sk, Q, P):
    """(:28-32): sk^2 by MulCoeffsMontgomery on the rows"""
    mods = [int(q) for q in Q[:key.levelQ + 1]]
    s = sk.rows(mods)
    return noise_gadget(key, rr._vec("MUL_MONT", s, s, mods), sk, Q, P)


def noise_galois_key(key, g, sk, Q, P):
    """(:35-48): skOut by AutomorphismNTT with g^-1 mod NthRoot on the rows of sk"""
    Ql, Pl = _mods(key, Q, P)
    inv = rr.galois_inverse(sk.N, g)
    so = rr.Secret(sk.N, sk.coeffs)
    so._rows = {q: orc.automorphism_ntt(r, inv) for q, r in zip(Ql + Pl, sk.rows(Ql + Pl))}
    return noise_gadget(key, sk.rows(Ql), so, Q, P)


def noise_rgsw(keys, pt_rows, sk, Q, P):
    """core/rgsw/utils.go: Value[0] against pt, Value[1] against pt sk"""
    mods = [int(q) for q in Q[:keys[0].levelQ + 1]]
    pt = np.asarray(pt_rows, dtype=np.uint64)[:len(mods)]
    ptsk = rr._vec("MUL_MONT", pt, sk.rows(mods), mods)
    return noise_gadget(keys[0], pt, sk, Q, P), noise_gadget(keys[1], ptsk, sk, Q, P)


def evk_bound(levelQ, levelP):
    """rlwe_test.go:509, :559, :578: log2(sqrt(BaseRNSDecompositionVectorSize) NoiseFreshSK) + 1"""
    return math.log2(math.sqrt(rr.rns_digits(levelQ, levelP)) * rr.SIGMA) + 1


def pk_bound():
    """rlwe_test.go:451-464: log2(NoiseFreshSK) + 1"""
    return math.log2(rr.SIGMA) + 1


RGSW_BOUND = 10.0     # rgsw_test.go:43

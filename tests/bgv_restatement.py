"""The BGV half of the reference's evaluator, schemes/bgv/evaluator.go, restated call for call over the pinned oracle pieces
(oracle.ring_oracle: vec_op, ntt / intt, div_by_last_modulus_many): tensorStandard (:665-751), mulRelinThenAdd (:1289-1403), matchScalesBinary
(:1620-1659), the Add / Sub scale matching (:270-305), the scalar branches, MatchScalesAndLevel (:1593-1614) and Rescale (:1415-1445).
TEST INFRASTRUCTURE ONLY: the GPU tests compare the device path against it bit for bit, tests/test_bgv_oracle.py pins it to Python big integers.

Polys are numpy uint64 arrays of shape (limbs, N), NTT domain; a ciphertext is a list of such arrays; scales are Python ints modulo t."""
import functools
import math

import numpy as np

from bfv_restatement import _vec, _zeros, centered, crt, intt, negacyclic_mul_small, ntt, prod, rns
from oracle import ring_oracle as orc


@functools.lru_cache(maxsize=None)
def subrings(N, mods):
    return [orc.SubRingConsts(N, q) for q in mods]


def t_montgomery(t, mods):
    """newEvaluatorPrecomp (:68-70): MForm(T * 2^64 mod q_i) = T * 2^128 mod q_i"""
    return [(int(t) << 128) % q for q in mods]


def mform(r, mods):
    return [(int(r) << 64) % q for q in mods]


def mul_scalar(p, r, mods):
    """ring.MulScalar (ring/operations.go:201-205)"""
    return _vec("MUL_SCALAR_MONT", p, None, _zeros(p), mform(r, mods), mods)


def mul_scalar_then_add(p, r, acc, mods):
    """:208-212"""
    return _vec("MUL_SCALAR_MONT_THEN_ADD", p, None, acc, mform(r, mods), mods)


def mul_scalar_then_sub(p, r, acc, mods):
    """:223-228: acc += p * MForm(q - BRedAdd(scalar))"""
    return _vec("MUL_SCALAR_MONT_THEN_ADD", p, None, acc, [((q - int(r) % q) << 64) % q for q in mods], mods)


def center(x, thalf, t):
    return t - x if x >= thalf else x


def match_scales_binary(t, scale0, scale1):
    """matchScalesBinary (:1620-1659), line for line"""
    thalf = t >> 1
    assert math.gcd(scale0, t) == 1
    a, b = t, 0
    A = pow(scale0, t - 2, t) * scale1 % t                           # :1636
    B = 1
    r0, r1 = A, B
    e = center(A, thalf, t) + 1                                      # :1641
    while A != 0:
        q = a // A
        a, A = A, a % A
        x = t + b - (B * q) % t                                      # :1647: CRed(t + b - BRed(B, q))
        b, B = B, (x - t if x >= t else x)
        if A != 0 and math.gcd(A, t) == 1:
            tmp = center(A, thalf, t) + center(B, thalf, t)
            if tmp < e:
                e = tmp
                r0, r1 = A, B
    return r0, r1, e


def tensor_standard(mods, t, op0, s0, op1, s1, square=False):
    """tensorStandard (:665-751) without the relin branch.  op1 with one component: the plaintext branch.  The operand swap of :693-698 only
    decides which operand meets tMontgomery: every product is a canonical MRed, so it changes no bit and is not restated.
    Returns ([c0, c1, c2] or one array per component of op0, scale)."""
    tm = t_montgomery(t, mods)
    scale = s0 * s1 % t                                              # :669
    z = _zeros(op0[0])
    if len(op0) == 2 and len(op1) == 2:
        c00 = _vec("MUL_SCALAR_MONT", op0[0], None, z, tm, mods)     # :701
        c01 = _vec("MUL_SCALAR_MONT", op0[1], None, z, tm, mods)     # :702
        c0 = _vec("MUL_MONT", c00, op1[0], z, None, mods)            # :705 / :711
        c2 = _vec("MUL_MONT", c01, op1[1], z, None, mods)            # :706 / :712
        c1 = _vec("MUL_MONT", c00, op1[1], z, None, mods)            # :707 / :713
        if square:
            c1 = _vec("ADD", c1, c1, z, None, mods)                  # :708
        else:
            c1 = _vec("MUL_MONT_THEN_ADD", c01, op1[0], c1, None, mods)   # :714
        return [c0, c1, c2], scale
    c00 = _vec("MUL_SCALAR_MONT", op1[0], None, z, tm, mods)         # :744
    return [_vec("MUL_MONT", x, c00, z, None, mods) for x in op0], scale   # :745-747


def mul_relin_then_add(mods, t, op0, s0, op1, s1, out, sout, relin):
    """mulRelinThenAdd (:1289-1403) up to the gadget product.  out: the accumulator's components (all of them are scaled by r1, :1324 / :1386).
    Returns (components, scale, c2): with relin, c2 is the plain product of :1353 for the caller's relinearisation and the components are
    the accumulator's own; without, c2 is None and the degree-2 term is accumulated in place."""
    tm = t_montgomery(t, mods)
    out = [x.copy() for x in out]
    z = _zeros(op0[0])
    r0 = 1
    target = s0 * s1 % t                                             # :1320 / :1382
    if sout != target:
        r0, r1, _ = match_scales_binary(t, target, sout)             # :1322
        out = [mul_scalar(x, r1, mods) for x in out]                 # :1324-1326
        sout = sout * r1 % t                                         # :1328
    if len(op0) == 2 and len(op1) == 2:
        c00 = _vec("MUL_SCALAR_MONT", op0[0], None, z, tm, mods)     # :1332
        c01 = _vec("MUL_SCALAR_MONT", op0[1], None, z, tm, mods)     # :1333
        if r0 != 1:
            c00, c01 = mul_scalar(c00, r0, mods), mul_scalar(c01, r0, mods)   # :1336-1339
        out[0] = _vec("MUL_MONT_THEN_ADD", c00, op1[0], out[0], None, mods)   # :1341
        out[1] = _vec("MUL_MONT_THEN_ADD", c00, op1[1], out[1], None, mods)   # :1342
        out[1] = _vec("MUL_MONT_THEN_ADD", c01, op1[0], out[1], None, mods)   # :1343
        if relin:
            return out, sout, _vec("MUL_MONT", c01, op1[1], z, None, mods)    # :1353
        out[2] = _vec("MUL_MONT_THEN_ADD", c01, op1[1], out[2], None, mods)   # :1366
        return out, sout, None
    c00 = _vec("MUL_SCALAR_MONT", op1[0], None, z, tm, mods)         # :1377
    if r0 != 1:
        c00 = mul_scalar(c00, r0, mods)                              # :1393-1395
    for i in range(len(op0)):
        out[i] = _vec("MUL_MONT_THEN_ADD", op0[i], c00, out[i], None, mods)   # :1397-1399
    return out, sout, None


def add_sub(mods, t, op0, s0, op1, s1, sub):
    """Add / Sub of two ciphertexts (:181-195, :350-366): evaluateInPlace (:270-286) for equal scales, matchScaleThenEvaluateInPlace
    (:288-305) otherwise.  Returns (components, scale)."""
    d0, d1 = len(op0), len(op1)
    z = _zeros(op0[0])
    if s0 == s1:
        out = [_vec("SUB" if sub else "ADD", op0[i], op1[i], z, None, mods) for i in range(min(d0, d1))]
        largest = op0 if d0 > d1 else op1
        out += [largest[i].copy() for i in range(min(d0, d1), max(d0, d1))]   # copied, under Sub too (:281-285)
        return out, max(s0, s1)                                      # :278
    r0, r1, _ = match_scales_binary(t, s0, s1)                       # :290
    out = [mul_scalar(x, r0, mods) for x in op0]                     # :292-294
    out += [z.copy() for _ in range(d0, max(d0, d1))]                # :296-298
    f = mul_scalar_then_sub if sub else mul_scalar_then_add
    for i in range(d1):
        out[i] = f(op1[i], r1, out[i], mods)                         # :300-302
    return out, s0 * r0 % t                                          # :304


def center_t(v, t):
    v %= t
    return v - t if v > (t >> 1) else v


def add_scalar(mods, t, op0, s0, v):
    """Add with a *big.Int (:197-227)"""
    v = center_t(v * s0, t) * pow(t, -1, prod(mods))                 # :209-219
    out = [x.copy() for x in op0]
    out[0] = _vec("ADD_SCALAR", op0[0], None, _zeros(op0[0]), [v % q for q in mods], mods)   # AddScalarBigint (:221)
    return out, s0


def mul_scalar_int(mods, t, op0, s0, v):
    """Mul with a *big.Int (:481-503): MulScalarBigint by the scalar centred modulo T"""
    v = center_t(v, t)
    return [_vec("MUL_SCALAR_MONT", x, None, _zeros(x), mform(v % prod(mods), mods), mods) for x in op0], s0


def match_scales_and_level(mods, t, ct0, s0, ct1, s1):
    """MatchScalesAndLevel (:1593-1614)"""
    r0, r1, _ = match_scales_binary(t, s0, s1)
    return [mul_scalar(x, r0, mods) for x in ct0], s0 * r0 % t, [mul_scalar(x, r1, mods) for x in ct1], s1 * r1 % t


def div_round_by_last_modulus_ntt(x, N, mods):
    """ring.DivRoundByLastModulusNTT (ring/scaling.go:130-156) of one poly at level len(mods)-1: its values are those of INTT, the
    coefficient-domain division, NTT (every output word is canonical)"""
    sr = subrings(N, tuple(mods))
    down = orc.div_by_last_modulus_many(intt(x, sr), list(mods), 1, True)
    return ntt(down, sr[:-1])


def rescale(N, mods, t, op0, s0):
    """Rescale (:1415-1445)"""
    return [div_round_by_last_modulus_ntt(x, N, mods) for x in op0], s0 * pow(mods[-1] % t, -1, t) % t    # :1436-1443


# ---- big-integer ground truth: encryption and decryption (real keys: tests/rlwe_restatement.py) --------------------------------------------------------
def encrypt(rnd, N, mods, t, m, s, scale=1):
    """a degree-1 ciphertext of the given scale: phase c0 + c1 s = (m scale) T^-1 + e (mod Q), |e| <= 3, i.e. T * phase = m scale + T e, the
    BGV encryption c0 = -a s + m + T e up to the factor T^-1 this evaluator carries (tensorStandard multiplies it back in)"""
    Qb = prod(mods)
    tinv = pow(t, -1, Qb)
    a = [rnd.randrange(Qb) for _ in range(N)]
    e = [rnd.randrange(-3, 4) for _ in range(N)]
    a_s = negacyclic_mul_small(a, s)
    c0 = [(int(mi) * scale % t * tinv + ei - x) % Qb for mi, ei, x in zip(m, e, a_s)]
    sr = subrings(N, tuple(mods))
    return [ntt(rns(c0, mods), sr), ntt(rns(a, mods), sr)]


def decrypt(N, mods, t, c, s):
    """T * (c0 + c1 s + c2 s^2 ...) centred modulo Q, then modulo t: the message times the ciphertext's scale"""
    Qb = prod(mods)
    sr = subrings(N, tuple(mods))
    acc = [0] * N
    for ck in reversed(c):                                           # Horner in s
        acc = [x + y for x, y in zip(negacyclic_mul_small(acc, s), crt(intt(ck, sr), mods))]
    return [x % t for x in centered([t * x for x in acc], Qb)]

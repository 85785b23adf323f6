"""The reference's CKKS evaluator, schemes/ckks/evaluator.go, restated call for call over the pinned oracle pieces (oracle.ring_oracle: vec_op,
ntt / intt, div_by_last_modulus_many): evaluateInPlace (:246-431), evaluateWithScalar (:433-447), bigComplexToRNSScalar (scaling.go:10-43),
Mul with a scalar (:646-683), mulRelin (:786-881), MulThenAdd with a scalar (:937-984), mulRelinThenAdd (:1095-1178), Rescale (:500-535) and
RescaleTo (:543-602), with a Scale of its own on fractions (core/rlwe/scale.go at ScalePrecision = 128).
TEST INFRASTRUCTURE ONLY: the GPU tests compare the device path against it bit for bit, tests/test_ckks_oracle.py pins it to Python big integers.

Polys are numpy uint64 arrays of shape (limbs, N), NTT domain; a ciphertext is a list of such arrays.

Go's big.Float rule restated here (there is no Go toolchain to run the reference against): z.Mul(x, y) / z.Quo(x, y) on a fresh z take the
larger operand precision and round to nearest, ties to even; z.Add(z, 0.5) rounds at z's precision; Int truncates toward zero;
SetPrec(p).SetFloat64 / SetInt / Set round the value to p bits."""
import functools
from fractions import Fraction

import numpy as np

from bfv_restatement import _vec, _zeros, intt, ntt
from oracle import ring_oracle as orc

PREC = 128                                                               # rlwe.ScalePrecision


def round_bits(x, prec):
    """x rounded to prec significant bits, ties to even"""
    x = Fraction(x)
    if x == 0:
        return x
    sign, x = (-1 if x < 0 else 1), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()            # 2^(e-1) < x < 2^(e+1)
    if x < Fraction(2) ** e:
        e -= 1                                                           # 2^e <= x < 2^(e+1)
    ulp = Fraction(2) ** (e - prec + 1)
    n, r = divmod(x, ulp)
    if 2 * r > ulp or (2 * r == ulp and n % 2):
        n += 1
    return sign * n * ulp


class Scale:
    """rlwe.Scale without Mod"""

    def __init__(self, v):
        self.v = round_bits(v.v if isinstance(v, Scale) else v, PREC)    # NewScale: SetPrec(128).Set...

    def mul(self, o):
        return Scale(self.v * o.v)                                       # :77-93

    def div(self, o):
        return Scale(self.v / o.v)                                       # :99-119

    def cmp(self, o):
        return (self.v > o.v) - (self.v < o.v)                           # :125-127

    def max(self, o):
        return o if self.cmp(o) < 0 else self                            # :153-160

    def float64(self):
        return self.v.numerator / self.v.denominator                     # correctly rounded, as big.Float.Float64

    def __eq__(self, o):
        return Fraction(getattr(o, "v", getattr(o, "Value", o))) == self.v

    def __repr__(self):
        return "Scale(%s)" % self.v


@functools.lru_cache(maxsize=None)
def subrings(N, mods):
    return [orc.SubRingConsts(N, q) for q in mods]


def roots_forward_1(N, mods):
    """SubRing.RootsForward[1] of every limb, in Montgomery form as the ring holds it"""
    return [int(sr.roots_fwd[1]) for sr in subrings(N, tuple(mods))]


def to_complex(value, prec):
    """bignum.ToComplex (utils/bignum/complex.go:22-55): (real, imag), each rounded to prec bits whatever the type"""
    if isinstance(value, complex):
        return round_bits(Fraction(value.real), prec), round_bits(Fraction(value.imag), prec)
    return round_bits(Fraction(value), prec), Fraction(0)


def is_int(c):
    return c[0].denominator == 1 and c[1].denominator == 1               # Complex.IsInt (:58-60)


def scaled_part(x, scale, prec):
    """scaling.go:16-27"""
    p = max(prec, PREC)
    r = round_bits(x * scale.v, p)
    if x > 0:
        r = round_bits(r + Fraction(1, 2), p)
    elif x < 0:
        r = round_bits(r - Fraction(1, 2), p)
    return int(r)


def rns_scalar(N, mods, scale, c, prec):
    """bigComplexToRNSScalar (scaling.go:10-43), then the scalar half of evaluateWithScalar (:439-442).  Returns (real, imag, s0, s1): the two
    big integers and the RNS scalars for coefficients [0, N/2) and [N/2, N)."""
    real, imag = scaled_part(c[0], scale, prec), scaled_part(c[1], scale, prec)
    w = roots_forward_1(N, mods)
    s0, s1 = [], []
    for i, q in enumerate(mods):
        im = orc.lib().orc_mred(imag % q, w[i], q, orc.lib().orc_gen_mred_constant(q))          # :440
        s0.append((real % q + im) % q)                                   # :441
        s1.append((real % q + q - im) % q)
    return real, imag, s0, s1


def _halves(op, p, acc, s0, s1, mods, mont):
    """Ring.{Add,Sub,Mul}DoubleRNSScalar(ThenAdd) (ring/operations.go:167-184, :250-266): s0 on coefficients [0, N/2), s1 on [N/2, N)"""
    h = p.shape[1] // 2
    f = (lambda s: [(int(v) << 64) % q for v, q in zip(s, mods)]) if mont else (lambda s: s)
    acc = _zeros(p) if acc is None else acc
    return np.concatenate([_vec(op, p[:, :h], None, acc[:, :h], f(s0), mods), _vec(op, p[:, h:], None, acc[:, h:], f(s1), mods)], axis=1)


def add_double(p, s0, s1, mods):
    return _halves("ADD_SCALAR", p, None, s0, s1, mods, False)


def sub_double(p, s0, s1, mods):
    return _halves("SUB_SCALAR", p, None, s0, s1, mods, False)


def mul_double(p, s0, s1, mods):
    return _halves("MUL_SCALAR_MONT", p, None, s0, s1, mods, True)


def mul_double_then_add(p, s0, s1, acc, mods):
    return _halves("MUL_SCALAR_MONT_THEN_ADD", p, acc, s0, s1, mods, True)


def rescale_scale(mods, nb):
    """:665-671"""
    s = Scale(mods[-1])
    for i in range(1, nb):
        s = s.mul(Scale(mods[-1 - i]))
    return s


def mul_scalar(N, mods, ct, scale, const, prec=53, nb=1):
    """Mul with a scalar (:646-683).  Returns (components, scale)."""
    c = to_complex(const, prec)
    sc = Scale(1) if is_int(c) else rescale_scale(mods, nb)
    _, _, s0, s1 = rns_scalar(N, mods, sc, c, prec)
    return [mul_double(x, s0, s1, mods) for x in ct], scale.mul(sc)


def add_sub_scalar(N, mods, ct, scale, const, sub, prec=53):
    """Add / Sub with a scalar (:82-101, :178-197): component 0 only, the rest copied"""
    _, _, s0, s1 = rns_scalar(N, mods, scale, to_complex(const, prec), prec)
    return [(sub_double if sub else add_double)(ct[0], s0, s1, mods)] + [x.copy() for x in ct[1:]], scale


def add_sub(N, mods, c0, scale0, c1, scale1, sub, alias=None, prec=53):
    """Add / Sub of two elements: evaluateInPlace (:246-431) and the Neg of Sub (:173-177).  alias: None, "op0" or "op1" -- which operand
    opOut is; it selects the branch (:263, :310, :356) and with it where the scaled operand lands, never a value."""
    cmp = scale0.cmp(scale1)
    tmp0, tmp1 = c0, c1
    if cmp != 0:
        ratio_int = int((scale0.div(scale1) if cmp == 1 else scale1.div(scale0)).v)              # ratioFlo.Int(nil)
        if ratio_int > 0:
            small, sscale = (c1, scale1) if cmp == 1 else (c0, scale0)
            scaled, _ = mul_scalar(N, mods, small, sscale, ratio_int, prec)                      # eval.Mul(ct, ratioInt, tmp / ct)
            if cmp == 1:
                tmp1 = scaled                                            # BuffCt (:273, :366) or opOut itself (:319)
            else:
                tmp0 = scaled                                            # c0 in place (:295) or BuffCt (:336, :390)
    lo = min(len(c0), len(c1))
    z = _zeros(c0[0])
    out = [_vec("SUB" if sub else "ADD", tmp0[i], tmp1[i], z, None, mods) for i in range(lo)]   # :413-415
    if len(c0) > len(c1):
        out += [x.copy() for x in tmp0[lo:]]                             # :422-425 (or already in place)
    elif len(c1) > len(c0):
        rest = [x.copy() for x in tmp1[lo:]]                             # :426-430
        if sub:
            rest = [_vec("NEG", x, None, z, None, mods) for x in rest]  # :173-177
        out += rest
    return out, scale0.max(scale1)                                       # :417


def mul_relin(mods, op0, scale0, op1, scale1, square=False):
    """mulRelin (:786-881) up to the gadget product.  op1 with one component: the plaintext branch (:856-878).  The operand swap of :815-819
    only decides which operand is put in Montgomery form: every product is a canonical MRed, so it changes no bit and is not restated."""
    z = _zeros(op0[0])
    scale = scale0.mul(scale1)                                           # :790
    if len(op0) == 2 and len(op1) == 2:
        c00 = _vec("MFORM", op0[0], None, z, None, mods)                 # :821
        c01 = _vec("MFORM", op0[1], None, z, None, mods)                 # :822
        c0 = _vec("MUL_MONT", c00, op1[0], z, None, mods)                # :825 / :831
        c2 = _vec("MUL_MONT", c01, op1[1], z, None, mods)                # :826 / :832
        c1 = _vec("MUL_MONT", c00, op1[1], z, None, mods)                # :827 / :833
        if square:
            c1 = _vec("ADD", c1, c1, z, None, mods)                      # :828
        else:
            c1 = _vec("MUL_MONT_THEN_ADD", c01, op1[0], c1, None, mods)  # :834
        return [c0, c1, c2], scale
    pt, ct = (op0, op1) if len(op0) == 1 else (op1, op0)
    c0 = _vec("MFORM", pt[0], None, z, None, mods)                       # :864 / :869
    return [_vec("MUL_MONT", c0, x, z, None, mods) for x in ct], scale   # :875-877


def mul_relin_then_add(N, mods, op0, scale0, op1, scale1, out, sout, relin, prec=53, nb=1):
    """mulRelinThenAdd (:1095-1178) up to the gadget product.  Returns (components, scale, c2): with relin and two degree-1 operands c2 is the
    plain product of :1150 for the caller's relinearisation."""
    out = [x.copy() for x in out]
    z = _zeros(op0[0])
    res = scale0.mul(scale1)                                             # :1099
    if sout.cmp(res) == -1:
        ratio = res.div(sout)
        if ratio.float64() >= 2.0:                                       # :1104
            out, _ = mul_scalar(N, mods, out, sout, ratio.v, prec, nb)   # eval.Mul(opOut, &ratio.Value, opOut) (:1105)
            sout = res                                                   # :1108
    if len(op0) == 2 and len(op1) == 2:
        c00 = _vec("MFORM", op0[0], None, z, None, mods)                 # :1135
        c01 = _vec("MFORM", op0[1], None, z, None, mods)                 # :1136
        out[0] = _vec("MUL_MONT_THEN_ADD", c00, op1[0], out[0], None, mods)   # :1138
        out[1] = _vec("MUL_MONT_THEN_ADD", c00, op1[1], out[1], None, mods)   # :1139
        out[1] = _vec("MUL_MONT_THEN_ADD", c01, op1[0], out[1], None, mods)   # :1140
        if relin:
            return out, sout, _vec("MUL_MONT", c01, op1[1], z, None, mods)    # :1150
        out[2] = _vec("MUL_MONT_THEN_ADD", c01, op1[1], out[2], None, mods)   # :1161
        return out, sout, None
    c00 = _vec("MFORM", op1[0], None, z, None, mods)                     # :1171
    for i in range(len(op0)):
        out[i] = _vec("MUL_MONT_THEN_ADD", op0[i], c00, out[i], None, mods)   # :1172-1174
    return out, sout, None


def mul_then_add_scalar(N, mods, op0, scale0, const, out, sout, prec=53, nb=1):
    """MulThenAdd with a scalar (:937-984).  Returns (components, scale); raises ValueError where the reference returns its error."""
    c = to_complex(const, prec)
    out = [x.copy() for x in out]
    cmp = scale0.cmp(sout)
    if cmp == 0:
        if is_int(c):
            s = Scale(1)                                                 # :960
        else:
            s = rescale_scale(mods, nb)                                  # :962-966
            out, _ = mul_scalar(N, mods, out, sout, int(s.v), prec, nb)  # :968-972: a *big.Int, through ToComplex like any scalar
            sout = sout.mul(s)                                           # :973
    elif cmp == -1:
        s = sout.div(scale0)                                             # :977
    else:
        raise ValueError("cannot MulThenAdd: op0.Scale > opOut.Scale is not supported")
    _, _, s0, s1 = rns_scalar(N, mods, s, c, prec)                       # :982
    return [mul_double_then_add(x, s0, s1, o, mods) for x, o in zip(op0, out)], sout   # :984


def div_round_by_last_modulus_many_ntt(x, N, mods, nb):
    """ring.DivRoundByLastModulusManyNTT (ring/scaling.go:130-156, 160-192): the values of INTT, the coefficient-domain division, NTT"""
    sr = subrings(N, tuple(mods))
    down = orc.div_by_last_modulus_many(intt(x, sr), list(mods), nb, True)
    return ntt(down, sr[:len(mods) - nb])


def rescale(N, mods, ct, scale, nb=1):
    """Rescale (:500-535)"""
    for i in range(nb):
        scale = scale.div(Scale(mods[-1 - i]))                           # :522-524
    return [div_round_by_last_modulus_many_ntt(x, N, mods, nb) for x in ct], scale


def rescale_to_count(mods, scale, min_scale):
    """the loop of RescaleTo (:553-584): (number of divisions, new scale)"""
    min_scale = min_scale.div(Scale(2))                                  # :553
    level, nb = len(mods) - 1, 0
    while level >= 0:
        s = scale.div(Scale(mods[level]))                                # :574
        if s.cmp(min_scale) == -1:
            break
        scale = s
        nb += 1
        level -= 1
    return nb, scale


def rescale_to(N, mods, ct, scale, min_scale):
    """RescaleTo (:543-602)"""
    nb, scale = rescale_to_count(mods, scale, min_scale)
    if nb == 0:
        return [x.copy() for x in ct], scale
    return [div_round_by_last_modulus_many_ntt(x, N, mods, nb) for x in ct], scale


def galois_element(N, k):
    """core/rlwe/params.go:671-675 on a standard ring: 5^(k & (2N - 1)) mod 2N"""
    return pow(5, k & (2 * N - 1), 2 * N)

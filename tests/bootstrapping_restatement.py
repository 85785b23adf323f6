"""circuits/ckks/bootstrapping/evaluator.go restated in plain Python on the oracle's ring and the existing restatements.  TEST INFRASTRUCTURE,
written from the reference, not from the package.

  ModUp's lift   :678-696 (c0), :703-722 (c1 under sparse-secret encapsulation, modulo Q and P), :762-775 (c1, dense), with ring.BRedAdd
                 (ring/modular_reduction.go:110-117) on Python integers
  the scaling    :735-750 / :781-789: MulScalar by uint64(round(scale)) after the NTT -- restated where the lift is compared in the
                 coefficient domain as the product modulo the limb, the NTT being linear

  the circuit     ScaleDown :596-643 with checkMessageRatio :541-546, ModUp :646-794, CoeffsToSlots, EvalMod, SlotsToCoeffs, bootstrap :548-587,
                 initialize's two scalings :205-221, over dft_restatement, mod1_restatement, inner_sum_restatement and rlwe_restatement

One deviation, shared with the device: the reference writes (Q[i] - tmp) * neg, which is Q[i] itself when Q[i] divides |coeff| of a negative
coefficient; the canonical 0 is written here."""
import math
from fractions import Fraction

import numpy as np

import ckks_restatement as cr
import dft_restatement as dr
import inner_sum_restatement as isr
import mod1_restatement as mr
import polynomial_restatement as pr
import rlwe_restatement as rr
from oracle import compose

M64 = (1 << 64) - 1


def bred_constant(q):
    """BRedConstant[0] (ring/modular_reduction.go GenBRedConstant): the high word of floor(2^128 / q)"""
    return ((1 << 128) // int(q)) >> 64


def bred_add(a, q, brc0):
    """ring.BRedAdd (:110-117)"""
    r = (a - ((a * brc0) >> 64) * q) & M64
    return r - q if r >= q else r


def lift_coeff(coeff, q0, mods, brcs, strict):
    """one coefficient of the loops at :683-696 (strict False: coeff >= q >> 1), :703-722 (strict True: coeff > q >> 1), :762-775"""
    pos, neg = 1, 0
    if (coeff > (q0 >> 1)) if strict else (coeff >= (q0 >> 1)):
        coeff = q0 - coeff
        pos, neg = 0, 1
    out = []
    for q, brc in zip(mods, brcs):
        tmp = bred_add(coeff, q, brc)
        v = tmp * pos + (q - tmp) * neg
        out.append(0 if v == q else v)                                              # the canonical zero (see the module's docstring)
    return out


def lift(row, q0, mods, strict, scalar=None):
    """row: the N limb-0 residues of one poly -> (len(mods), N) uint64, each limb multiplied by `scalar` modulo the limb when one is given"""
    mods = [int(q) for q in mods]
    brcs = [bred_constant(q) for q in mods]
    cols = [lift_coeff(int(c), int(q0), mods, brcs, strict) for c in row]
    out = np.array(cols, dtype=object).T
    if scalar is not None:
        for i, q in enumerate(mods):
            out[i] = (out[i] * (int(scalar) % q)) % q
    return out.astype(np.uint64)


def centered_mod(row, q0, mods, strict):
    """what the lift means, on big integers: the representative of coeff centred around q0 -- in (-q0/2, q0/2] for strict, [-q0/2, q0/2) else --
    reduced modulo every limb"""
    h = int(q0) >> 1
    out = []
    for q in mods:
        out.append([((int(c) - int(q0)) if ((int(c) > h) if strict else (int(c) >= h)) else int(c)) % int(q) for c in row])
    return np.array(out, dtype=object).astype(np.uint64)


# ---- the circuit -------------------------------------------------------------------------------------------------------------------------------
class Circuit:
    """what bootstrapping.Evaluator holds after initialize (:187-246).  N, Q, P: the bootstrapping ring; residual_level; default_scale: both
    parameter sets' DefaultScale; evm: mod1_restatement.params; c2s / s2c: dft_restatement literals WITHOUT the circuit's scalings (they are
    multiplied in here); rlk, galois: {element: key}; d2s / s2d: the encapsulation keys or None"""

    def __init__(self, N, Q, P, residual_level, default_scale, evm, c2s, s2c, rlk, galois, d2s=None, s2d=None):
        self.N, self.Q, self.P = N, [int(q) for q in Q], [int(p) for p in P]
        self.residual_level, self.default_scale, self.evm = residual_level, cr.Scale(default_scale), evm
        self.rlk, self.galois, self.d2s, self.s2d = rlk, galois, d2s, s2d
        self.message_ratio = float(1 << evm.log_message_ratio)
        scaling_factor = float(2 ** evm.log_scale)
        q_div = min(scaling_factor / 2.0 ** math.floor(math.log2(float(self.Q[0])) + 0.5), 1.0)                  # :205-210
        c2s_scaling = q_div / (evm.K * evm.qdiff)                                                                  # :220
        s2c_scaling = self.default_scale.float64() / (scaling_factor / self.message_ratio)                        # :217-221
        self.c2s = dict(c2s, Scaling=c2s_scaling if c2s["Scaling"] is None else float(Fraction(c2s["Scaling"]) * Fraction(c2s_scaling)))
        self.s2c = dict(s2c, Scaling=s2c_scaling if s2c["Scaling"] is None else float(Fraction(s2c["Scaling"]) * Fraction(s2c_scaling)))
        self.c2s_lts = dr.new_matrix(N, self.Q, self.P, self.c2s)
        self.s2c_lts = dr.new_matrix(N, self.Q, self.P, self.s2c)
        self.P_poly = pr.Params(N, self.Q, self.P, rlk)
        self.log_slots = c2s["LogSlots"]


def big_int(scale):
    """rlwe.Scale.BigInt (core/rlwe/scale.go): the value plus one half at 128 bits, truncated"""
    return int(cr.round_bits(scale.v + Fraction(1, 2), cr.PREC))


def check_message_ratio(B, level, scale):
    """:541-546"""
    cur = cr.Scale(rr.prod(B.Q[:level + 1])).div(scale)
    return cur.cmp(cr.Scale(B.Q[level]).mul(cr.Scale(B.message_ratio))) > -1


def scale_down(B, ct, scale):
    """ScaleDown (:596-643) -> (ct, scale, errScale)"""
    level = ct[0].shape[0] - 1
    while level != 0 and check_message_ratio(B, level, scale):           # :603-605
        level -= 1
    ct = [x[:level + 1].copy() for x in ct]
    mods = B.Q[:level + 1]
    cur = cr.Scale(rr.prod(mods)).div(scale)                             # :608-609
    target = cr.Scale(B.message_ratio)                                   # :612
    scale_up = cur.div(target)                                           # :615
    assert scale_up.cmp(cr.Scale(0.5)) != -1, "initial Q/Scale < 0.5*Q[0]/MessageRatio"
    k = big_int(scale_up)                                                # :621
    ct, _ = cr.mul_scalar(B.N, mods, ct, scale, k)                       # :623: a *big.Int through bignum.ToComplex at the encoding precision
    scale = scale.mul(cr.Scale(k))                                       # :627
    target_scale = cr.round_bits(Fraction(B.Q[0]) / Fraction(B.message_ratio), 256)      # :630-631
    if level != 0:
        ct, scale = cr.rescale_to(B.N, mods, ct, scale, cr.Scale(target_scale))          # :633-637
    return ct, scale, scale.div(cr.Scale(target_scale))                  # :640


def hoisted_product_of_one_poly(B, levelQ, c2q, c2p, key):
    """GadgetProductHoisted (core/rlwe/evaluator_gadget_product.go:326-429) fed ONE PolyQP as every digit's decomposition (:724-730), then
    the ModDown: the accumulation and its reduction schedule as inner_sum_restatement.lazy_product writes them"""
    levelP = key.levelP
    Ql, Pl = B.Q[:levelQ + 1], B.P[:levelP + 1]
    beta = (levelQ + levelP + 1) // (levelP + 1)
    accQ, accP = [None, None], [None, None]
    qiof = int(2.0 ** 64 / float(max(Ql))) >> 1
    piof = int(2.0 ** 64 / float(max(Pl))) >> 1
    reduce = 0
    for d in range(beta):
        for c in (0, 1):
            accQ[c] = compose._mac(accQ[c], key.Q[d, c][:levelQ + 1], c2q, Ql, d == 0)
            accP[c] = compose._mac(accP[c], key.P[d, c], c2p, Pl, d == 0)
        if reduce % qiof == qiof - 1:
            accQ = [compose._reduce(a, Ql) for a in accQ]
        if reduce % piof == piof - 1:
            accP = [compose._reduce(a, Pl) for a in accP]
        reduce += 1
    if reduce % qiof:
        accQ = [compose._reduce(a, Ql) for a in accQ]
    if reduce % piof:
        accP = [compose._reduce(a, Pl) for a in accP]
    return isr.moddown(B.N, B.Q, B.P, levelQ, levelP, accQ, accP)


def mod_up(B, ct, scale):
    """ModUp (:646-794) on a level-0 ciphertext -> (ct at the top level, scale)"""
    N, Q, P = B.N, B.Q, B.P
    if B.d2s is not None:                                                # :649-653
        ct = rr.apply_evaluation_key(N, Q, P, ct, B.d2s)
    q0 = Q[0]
    c = [rr.intt(np.asarray(x[:1], dtype=np.uint64), N, [q0])[0] for x in ct]        # :660-662
    levelQ = len(Q) - 1
    s = (float(2 ** B.evm.log_scale) / B.message_ratio) / scale.float64()            # :735 / :781
    scalar = int(math.floor(s + 0.5)) if s > 1 else None                 # uint64(math.Round(scale))
    c0 = rr.ntt(lift(c[0], q0, Q, False), N, Q)                          # :683-696, :732 / :777
    if B.s2d is not None:
        c1q, c1p = rr.ntt(lift(c[1], q0, Q, True), N, Q), rr.ntt(lift(c[1], q0, P, True), N, P)      # :703-730
        if scalar is not None:                                           # :735-750
            c1q, c1p, c0 = isr._mul_scalar(c1q, scalar, Q), isr._mul_scalar(c1p, scalar, P), isr._mul_scalar(c0, scalar, Q)
        t0, t1 = hoisted_product_of_one_poly(B, levelQ, c1q, c1p, B.s2d)                 # :757
        out = [rr._add(c0, t0, Q), t1]                                   # :758
    else:
        c1 = rr.ntt(lift(c[1], q0, Q, False), N, Q)                      # :762-778
        if scalar is not None:                                           # :781-789
            c0, c1 = isr._mul_scalar(c0, scalar, Q), isr._mul_scalar(c1, scalar, Q)
        out = [c0, c1]
    if scalar is not None:
        scale = scale.mul(cr.Scale(s))
    return isr.trace(N, Q, P, out, B.log_slots, B.galois), scale          # :793


def eval_mod(B, ct, scale):
    """EvalMod (:802-809)"""
    out = mr.evaluate(B.P_poly, pr.Ct(ct, scale), B.evm)
    return out.comps, B.default_scale


def bootstrap(B, ct, scale, trace=None):
    """bootstrap (:548-587) -> (ct, scale, errScale).  trace: a dict that receives every stage's (ciphertext, scale)"""
    keep = (lambda k, v: trace.__setitem__(k, v)) if trace is not None else (lambda k, v: None)
    ct, scale, err_scale = scale_down(B, ct, scale)
    keep("ScaleDown", (ct, scale, err_scale))
    ct, scale = mod_up(B, ct, scale)
    keep("ModUp", (ct, scale))
    (re, rs), imag = dr.coeffs_to_slots(B.N, B.Q, B.P, ct, scale, B.log_slots, B.c2s, B.c2s_lts, B.galois)
    keep("CoeffsToSlots", ((re, rs), imag))
    re, rs = eval_mod(B, re, rs)
    if imag is not None:
        im, ims = eval_mod(B, imag[0], imag[1])
    else:
        im, ims = None, None
    keep("EvalMod", ((re, rs), (im, ims) if im is not None else None))
    out, s = dr.slots_to_coeffs(B.N, B.Q, B.P, re, rs, im, ims, B.s2c, B.s2c_lts, B.galois)
    return out, s, err_scale

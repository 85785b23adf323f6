"""circuits/ckks/bootstrapping/evaluator.go, the passes BootstrapMany adds around Evaluate, restated over the pinned oracle pieces: pack (:1008-1065),
unpack (:965-1004), the packingContext bookkeeping of PackAndSwitchN1ToN2 / UnpackAndSwitchN2ToN1 (:880-961) and the pair fold / unfold of
EvaluateConjugateInvariant (:507-511, :531) through the scalar route of evaluateWithScalar (tests/ckks_restatement.py: mul_scalar).
TEST INFRASTRUCTURE ONLY: what rh_ckks_bootstrap_pack / rh_ckks_bootstrap_unpack and bootstrapping.Bootstrapper are compared with bit for bit,
itself pinned to coefficient arithmetic and to decoding by tests/test_bootstrap_many_oracle.py.

The loops are the reference's, line by line and one ciphertext at a time -- NOT the sums and groups of the device kernels.  Ciphertexts are lists
[c0, c1] of (limbs, N) uint64 arrays in the NTT domain; xPow2 / xPow2Inv: ring_packing_restatement.gen_xpow2_ntt."""
import numpy as np

import ckks_restatement as cr
import rlwe_restatement as rr


class PackError(ValueError):
    """the reference's error returns"""


class PackingContext:
    """packingContext (:871-876): N and LogMaxSlots of the ring packed in, the dimension packed up to, the ciphertexts' own, their number"""

    def __init__(self, N, ParamsLogMaxSlots, LogMaxDimensions, LogSlots, NbPackedCTs):
        self.N, self.ParamsLogMaxSlots, self.LogMaxDimensions, self.LogSlots, self.NbPackedCTs = N, ParamsLogMaxSlots, LogMaxDimensions, LogSlots, NbPackedCTs


def _mul_then_add(a, b, acc, mods):
    z = np.stack([rr.orc.vec_op(rr.OPS["MUL_MONT_THEN_ADD"], a[i], b[i], acc[i], 0, 0, mods[i]) for i in range(len(mods))])
    return z


def pack(cts, log_slots, ctxt, xPow2, mods):
    """pack (:1008-1065).  cts: the ciphertexts; log_slots: their LogSlots, one per ciphertext.  -> (packed ciphertexts, their LogDimensions).
    eve is modified in place in the reference; here the inputs are copied first."""
    logSlots, logMaxSlots = ctxt.LogSlots, ctxt.LogMaxDimensions
    if logSlots > logMaxSlots:
        raise PackError("cannot Pack: cts[0].LogSlots()=%d > logMaxSlots=%d" % (logSlots, logMaxSlots))
    for i, ct in enumerate(cts):
        if log_slots[i] != logSlots:
            raise PackError("cannot Pack: cts[%d].PlaintextLogSlots()=%d != cts[0].PlaintextLogSlots=%d" % (i, log_slots[i], logSlots))
        if ct[0].shape[1] != ctxt.N:
            raise PackError("cannot Pack: cts[%d].Value[0].N()=%d != params.N()=%d" % (i, ct[0].shape[1], ctxt.N))
    logPackCTs = logMaxSlots - logSlots
    logGap = ctxt.ParamsLogMaxSlots - logSlots - 1
    cts = [[c.copy() for c in ct] for ct in cts]
    if logPackCTs == 0:
        return cts, logSlots
    L = len(mods)
    for i in range(logPackCTs):
        for j in range(len(cts) >> 1):
            eve, odd = cts[2 * j], cts[2 * j + 1]
            eve[0] = _mul_then_add(odd[0], xPow2[logGap - i][:L], eve[0], mods)
            eve[1] = _mul_then_add(odd[1], xPow2[logGap - i][:L], eve[1], mods)
            cts[j] = eve
        if len(cts) & 1:
            cts[len(cts) >> 1] = cts[-1]
            cts = cts[:(len(cts) >> 1) + 1]
        else:
            cts = cts[:len(cts) >> 1]
    return cts, logMaxSlots


def unpack(ct, ctxt, xPow2Inv, mods):
    """unpack (:965-1004) of ONE packed ciphertext -> list of ciphertexts"""
    logPackCTs = ctxt.LogMaxDimensions - ctxt.LogSlots
    cts = [[c.copy() for c in ct]]
    if logPackCTs == 0:
        return cts
    n = min(ctxt.NbPackedCTs, 1 << logPackCTs)
    cts += [[c.copy() for c in ct] for _ in range(n - 1)]
    logGap = ctxt.ParamsLogMaxSlots - ctxt.LogSlots - 1
    L = len(mods)
    for i in range(min((n - 1).bit_length(), logPackCTs)):
        step = 1 << (i + 1)
        for j in range(0, n, step):
            for k in range(step >> 1, step):
                if j + k >= n:
                    break
                for c in (0, 1):
                    cts[j + k][c] = rr._vec("MUL_MONT", cts[j + k][c], xPow2Inv[logGap - i][:L], mods)
    return cts


def unpack_many(cts, ctxt, xPow2Inv, mods):
    """the loop of UnpackAndSwitchN2ToN1 (:922-931 / :942-950): NbPackedCTs goes down by what every packed ciphertext gave"""
    out = []
    for ct in cts:
        got = unpack(ct, ctxt, xPow2Inv, mods)
        out += got
        ctxt.NbPackedCTs -= len(got)
    return out


def pair_fold(N, mods, left, right, scale):
    """:507-511: Mul(right, 1i, right); Add(left, right, left) -- the scalar route of evaluateWithScalar; the scale is left as it is (an integer
    constant).  right None: the nil arm."""
    if right is None:
        return [c.copy() for c in left]
    r, s = cr.mul_scalar(N, mods, right, scale, 1j)
    assert s.v == scale.v
    return [rr._vec("ADD", left[c], r[c], mods) for c in (0, 1)]


def pair_unfold(N, mods, ct, scale):
    """:531: Mul(ct, -1i, ct) -> the right-hand ciphertext before ComplexToReal"""
    r, s = cr.mul_scalar(N, mods, ct, scale, -1j)
    assert s.v == scale.v
    return r


def x_pow_half_ntt(N, mods, neg=False):
    """NTT(X^(N/2)) in Montgomery form (the top GenXPow2NTT row), or its negation: i and -i of the canonical embedding"""
    p = np.zeros((len(mods), N), dtype=np.uint64)
    for j, q in enumerate(mods):
        p[j, N // 2] = (1 << 64) % int(q)
    p = rr.ntt(p, N, mods)
    return rr._vec("NEG", p, None, mods) if neg else p

"""core/rlwe/inner_sum.go restated over the pinned oracle pieces: PartialTracesSum (:152-291), Trace (:36-121), GaloisElementsForInnerSum (:444-468),
and the scheme wrappers schemes/ckks/evaluator.go:1284-1317, schemes/ckks/linear_transformation.go:24-52 and schemes/bgv/evaluator.go:1527-1566.
TEST INFRASTRUCTURE ONLY: what the device path (rlwe.Evaluator.PartialTracesSum, fused and composed, and rh_rlwe_partial_traces_sum) is compared
with bit for bit, itself pinned to decryption by tests/test_inner_sum_oracle.py.

The loops below are the reference's, line by line, NOT the plan the device path derives from them (rlwe.partial_traces_plan): the lazy product is
the loop of oracle/compose.py's gadget_product without its last line, then + P ct0, orc.automorphism_ntt per limb, canonical adds and
orc.moddown_qp_to_q_ntt.  Ciphertexts are lists [c0, c1] of (limbs, N) uint64 arrays in the NTT domain; keys: {Galois element: rr.GadgetKey}."""
import numpy as np

import rlwe_restatement as rr
from oracle import compose
from oracle import ring_oracle as orc

OPS = compose.OPS


def galois_element(N, k):
    """Parameters.GaloisElement (core/rlwe/params.go:671-675)"""
    return pow(5, k % (2 * N), 2 * N)


def lazy_product(N, Q, P, levelQ, levelP, cx, evkQ, evkP):
    """gadgetProductMultiplePLazy (core/rlwe/evaluator_gadget_product.go:122-188) = compose.gadget_product without the ModDown: ([accQ0, accQ1], [accP0, accP1])"""
    LQ, LP = levelQ + 1, levelP + 1
    Ql, Pl = Q[:LQ], P[:LP]
    srQ = [orc.SubRingConsts(N, q) for q in Ql]
    srP = [orc.SubRingConsts(N, p) for p in Pl]
    beta = (levelQ + levelP + 1) // (levelP + 1)
    cxinv = np.stack([orc.intt(cx[i], srQ[i]) for i in range(LQ)])
    accQ, accP = [None, None], [None, None]
    qiof = int(2.0 ** 64 / float(max(Ql))) >> 1
    piof = int(2.0 ** 64 / float(max(Pl))) >> 1
    reduce = 0
    for d in range(beta):
        c2q, c2p = orc.decompose_and_split(levelQ, levelP, LP, d, cxinv, Q, P)
        st, ed = d * LP, min(d * LP + LP, LQ)
        c2q = np.stack([cx[i] if st <= i < ed else orc.ntt(c2q[i], srQ[i]) for i in range(LQ)])
        c2p = np.stack([orc.ntt(c2p[j], srP[j]) for j in range(LP)])
        for c in (0, 1):
            accQ[c] = compose._mac(accQ[c], evkQ[d, c], c2q, Ql, d == 0)
            accP[c] = compose._mac(accP[c], evkP[d, c], c2p, Pl, d == 0)
        if reduce % qiof == qiof - 1:
            accQ = [compose._reduce(a, Ql) for a in accQ]
        if reduce % piof == piof - 1:
            accP = [compose._reduce(a, Pl) for a in accP]
        reduce += 1
    if reduce % qiof:
        accQ = [compose._reduce(a, Ql) for a in accQ]
    if reduce % piof:
        accP = [compose._reduce(a, Pl) for a in accP]
    return accQ, accP


def moddown(N, Q, P, levelQ, levelP, accQ, accP):
    Ql, Pl = Q[:levelQ + 1], P[:levelP + 1]
    srQ = [orc.SubRingConsts(N, q) for q in Ql]
    srP = [orc.SubRingConsts(N, p) for p in Pl]
    return [orc.moddown_qp_to_q_ntt(accQ[c], accP[c], Ql, Pl, srQ, srP) for c in (0, 1)]


def _auto(x, g):
    return np.stack([orc.automorphism_ntt(x[i], g) for i in range(x.shape[0])])


def automorphism_hoisted_lazy(N, Q, P, ct, key, g):
    """AutomorphismHoistedLazy (core/rlwe/evaluator_automorphism.go:107-160), NTT-domain ctQP: (phi(KS_0 + P ct0), phi(KS_1)) modulo Q and
    (phi(KS_0), phi(KS_1)) modulo P"""
    level = ct[0].shape[0] - 1
    Ql = [int(q) for q in Q[:level + 1]]
    accQ, accP = lazy_product(N, Q, P, level, key.levelP, ct[1], key.Q, key.P)
    Pb = rr.prod(P[:key.levelP + 1])
    scaled = np.stack([((ct[0][i].astype(object) * (Pb % q)) % q).astype(np.uint64) for i, q in enumerate(Ql)])     # MulScalarBigint (:140)
    accQ[0] = rr._add(accQ[0], scaled, Ql)                                                                         # (:143)
    return [_auto(a, g) for a in accQ], [_auto(a, g) for a in accP]


def partial_traces_sum(N, Q, P, ct, offset, n, keys, used=None):
    """PartialTracesSum (:152-291) on an NTT-domain ciphertext.  used: a list that receives the Galois elements applied, in order"""
    if n == 0 or offset == 0:
        raise ValueError("partialtrace: invalid parameter (n = 0 or batchSize = 0)")
    level = ct[0].shape[0] - 1
    Ql = [int(q) for q in Q[:level + 1]]
    ctin = [np.array(c, dtype=np.uint64) for c in ct]
    if n == 1:
        return ctin
    used = [] if used is None else used
    out, acc = None, None
    state, copy = False, True
    i, j = 0, n
    while j > 0:
        if j & 1 == 1:
            k = n - (n & ((2 << i) - 1))
            k *= offset
            if k != 0:
                rot = galois_element(N, k)
                used.append(rot)
                cq, cp = automorphism_hoisted_lazy(N, Q, P, ctin, keys[rot], rot)
                if copy:
                    acc, copy = (cq, cp), False
                else:
                    levelP = keys[rot].levelP
                    Pl = [int(p) for p in P[:levelP + 1]]
                    acc = ([rr._add(acc[0][c], cq[c], Ql) for c in (0, 1)], [rr._add(acc[1][c], cp[c], Pl) for c in (0, 1)])    # ringQP.Add (:245-246)
            else:
                state = True
                if n & (n - 1) != 0:
                    levelP = acc[1][0].shape[0] - 1
                    down = moddown(N, Q, P, level, levelP, acc[0], acc[1])
                    out = [rr._add(down[c], ctin[c], Ql) for c in (0, 1)]
                else:
                    out = [c.copy() for c in ctin]
        if not state:
            rot = galois_element(N, (1 << i) * offset)
            used.append(rot)
            cq = [ctin[0].copy(), ctin[1].copy()] if rot == 1 else rr.automorphism(N, Q, P, ctin, keys[rot], rot)     # AutomorphismHoisted (:62-102)
            ctin = [rr._add(ctin[c], cq[c], Ql) for c in (0, 1)]
        i, j = i + 1, j >> 1
    return out


def inner_function_add(N, Q, P, ct, batchSize, n, keys):
    """InnerFunction (:316-440) with f = Add: the same tree over plain Evaluator.Automorphism calls (one ModDown per rotation), accumulated modulo Q"""
    level = ct[0].shape[0] - 1
    Ql = [int(q) for q in Q[:level + 1]]
    ctin = [np.array(c, dtype=np.uint64) for c in ct]
    if n == 1:
        return ctin
    f = lambda a, b: [rr._add(a[c], b[c], Ql) for c in (0, 1)]
    out, acc = None, None
    state, copy = False, True
    i, j = 0, n
    while j > 0:
        if j & 1 == 1:
            k = n - (n & ((2 << i) - 1))
            k *= batchSize
            if k != 0:
                rot = galois_element(N, k)
                cq = rr.automorphism(N, Q, P, ctin, keys[rot], rot)
                if copy:
                    acc, copy = cq, False
                else:
                    acc = f(acc, cq)
            else:
                state = True
                out = f(acc, ctin) if n & (n - 1) != 0 else [c.copy() for c in ctin]
        if not state:
            rot = galois_element(N, (1 << i) * batchSize)
            ctin = f(ctin, rr.automorphism(N, Q, P, ctin, keys[rot], rot))
        i, j = i + 1, j >> 1
    return out


def galois_elements_for_inner_sum(N, batch, n):
    """GaloisElementsForInnerSum (:444-468) as a set"""
    rot = set()
    i = 1
    while i < n:
        rot.add(i * batch)
        rot.add((n - (n & ((i << 1) - 1))) * batch)
        i <<= 1
    return {galois_element(N, k) for k in rot}


def galois_elements_for_trace(N, logN):
    """GaloisElementsForTrace (:125-146), standard ring"""
    top = N.bit_length() - 1
    out = [galois_element(N, 1 << i) for i in range(logN, top - 1)]
    if logN == 0:
        out.append(2 * N - 1)
    return out


def _mul_scalar(x, s, mods):
    return np.stack([((x[i].astype(object) * (s % int(q))) % int(q)).astype(np.uint64) for i, q in enumerate(mods)])


def trace(N, Q, P, ct, logN, keys):
    """Trace (:36-121) on an NTT-domain ciphertext of a standard ring"""
    level = ct[0].shape[0] - 1
    Ql = [int(q) for q in Q[:level + 1]]
    top = N.bit_length() - 1
    gap = 1 << (top - logN - 1)
    if logN == 0:
        gap <<= 1
    if gap <= 1:
        return [np.array(c, dtype=np.uint64) for c in ct]
    ninv = pow(gap, -1, rr.prod(Ql))
    out = [_mul_scalar(np.asarray(c, dtype=np.uint64), ninv, Ql) for c in ct]
    gs = [galois_element(N, 1 << i) for i in range(logN, top - 1)]
    if logN == 0:
        gs.append(2 * N - 1)
    for g in gs:
        buff = rr.automorphism(N, Q, P, out, keys[g], g)
        out = [rr._add(out[c], buff[c], Ql) for c in (0, 1)]
    return out


def trace_coeffs(m, N, logN):
    """what Trace leaves of a message: sigma_{5^(2^i)} negates X^k for k an odd multiple of N / 2^(i+2), so after i = logN .. log2(N) - 2 the
    coefficients at multiples of gap = N / 2^(logN+1) are left (times gap gap^-1 = 1) and the others vanish; logN = 0 adds X -> X^-1, which
    removes X^(N/2) too: the constant coefficient alone"""
    gap = (N >> (logN + 1)) << (1 if logN == 0 else 0)
    return [x if i % gap == 0 else 0 for i, x in enumerate(m)]


# ---- scheme layers --------------------------------------------------------------------------------------------------------------------------
def _innersum_checks(slots, batchSize, n):
    l = n * batchSize
    if n <= 0 or batchSize <= 0:
        raise ValueError("innersum: invalid parameter (n <= 0 or batchSize <= 0)")
    if l > slots:
        raise ValueError("innersum: invalid parameters (n*batchSize=%d > #slots=%d)" % (l, slots))
    if l & (l - 1) != 0:
        raise ValueError("innersum: invalid parameters (n*batchSize=%d does not divide #slots=%d)" % (l, slots))
    return l


def ckks_inner_sum(N, Q, P, ct, batchSize, n, keys, slots=None):
    """ckks.Evaluator.InnerSum (schemes/ckks/evaluator.go:1284-1299)"""
    _innersum_checks(N // 2 if slots is None else slots, batchSize, n)
    return partial_traces_sum(N, Q, P, ct, batchSize, n, keys)


def ckks_average(N, Q, P, ct, logBatchSize, keys, log_slots=None):
    """ckks.Evaluator.Average (schemes/ckks/linear_transformation.go:24-52)"""
    log_slots = N.bit_length() - 2 if log_slots is None else log_slots
    level = ct[0].shape[0] - 1
    Ql = [int(q) for q in Q[:level + 1]]
    n = 1 << (log_slots - logBatchSize)
    out = [np.stack([((np.asarray(c[i], dtype=np.uint64).astype(object) * pow(n, q - 2, q)) % q).astype(np.uint64) for i, q in enumerate(Ql)]) for c in ct]
    return ckks_inner_sum(N, Q, P, out, 1 << logBatchSize, n, keys, 1 << log_slots)


def bgv_inner_sum(N, Q, P, ct, batchSize, n, keys):
    """bgv.Evaluator.InnerSum (schemes/bgv/evaluator.go:1527-1566): N slots as a 2 x N/2 matrix; n batchSize = N sums over both rows"""
    l = _innersum_checks(N, batchSize, n)
    level = ct[0].shape[0] - 1
    Ql = [int(q) for q in Q[:level + 1]]
    if l == N:
        if n == 1:
            return [np.array(c, dtype=np.uint64) for c in ct]
        out = partial_traces_sum(N, Q, P, ct, batchSize, n // 2, keys)
        g = 2 * N - 1                                                    # GaloisElementForRowRotation
        tmp = rr.automorphism(N, Q, P, out, keys[g], g)                  # RotateRows (:1488-1490)
        return [rr._add(out[c], tmp[c], Ql) for c in (0, 1)]
    return partial_traces_sum(N, Q, P, ct, batchSize, n, keys)

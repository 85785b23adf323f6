"""The key generator, both encryptors and the decryptor of core/rlwe (keygenerator.go, encryptor.go, decryptor.go) with EXPLICIT samples, over the
pinned oracle pieces and the helpers of tests/rlwe_restatement.py: what matrix-fhe-lattigo_amd/keygen.py is compared with, bit for bit, when it
is handed the same samples.  TEST INFRASTRUCTURE ONLY.

Polys are numpy uint64 arrays (limbs, N); keys are (rows, 2, limbs, N) in the NTT domain and in Montgomery form; small samples are int arrays."""
import numpy as np

import rlwe_restatement as rr
from oracle import ring_oracle as orc
from oracle.compose import OPS


def secret(coeffs):
    """GenSecretKey (keygenerator.go:60-72) from its N coefficients"""
    return rr.Secret(len(coeffs), [int(x) for x in coeffs])


def zero_row(sk, mods, a, e):
    """encryptZeroSkFromC1QP (encryptor.go:432-460), NTT domain and Montgomery form: (MForm(NTT(e)) - a sk, a)"""
    mods = [int(q) for q in mods]
    e_m = rr.small_ntt_mont([int(x) for x in e], sk.N, mods)
    a = np.asarray(a, dtype=np.uint64)
    return rr._vec("SUB", e_m, rr._vec("MUL_MONT", a, sk.rows(mods), mods), mods), a


def gadget(sk_out, pt_rows, Q, P, levelQ, levelP, pw2, a, e, dpl=None):
    """one gadget ciphertext (genEvaluationKey, keygenerator.go:276-316): a (rows, LQ + LP, N) uniform, e (rows, N) errors; pt_rows (LQ, N) NTT
    domain, Montgomery form, or None for rows of zero encryptions.  The plaintext term as AddPolyTimesGadgetVectorToGadgetCiphertext
    (gadgetciphertext.go:172-241) forms it.  Returns (valueQ, valueP or None, dpl)."""
    N = sk_out.N
    Ql, Pl = [int(q) for q in Q[:levelQ + 1]], [int(p) for p in P[:levelP + 1]] if levelP >= 0 else []
    mods = Ql + Pl
    dpl = rr.digits_per_limb(Q, levelQ, levelP, pw2) if dpl is None else dpl
    Pb = rr.prod(Pl)
    width = max(levelP, 0) + 1
    rows, r = [], 0
    for i in range(len(dpl)):
        for j in range(dpl[i]):
            f = Pb << (j * pw2)
            b, a_r = zero_row(sk_out, mods, a[r], e[r])
            if pt_rows is not None:
                for k in range(width):
                    index = i * width + k
                    if index >= levelQ + 1:
                        break
                    q = Ql[index]
                    term = orc.vec_op(OPS["MUL_SCALAR_MONT"], pt_rows[index], None, np.zeros(N, dtype=np.uint64), (f << 64) % q, 0, q)
                    b[index] = orc.vec_op(OPS["ADD"], b[index], term, b[index], 0, 0, q)
            rows.append(np.stack([b, a_r]))
            r += 1
    key = np.stack(rows)
    return key[:, :, :levelQ + 1].copy(), (key[:, :, levelQ + 1:].copy() if Pl else None), dpl


def rows_of(Q, levelQ, levelP, pw2):
    return sum(rr.digits_per_limb(Q, levelQ, levelP, pw2))


def public_key(sk, Q, P, a, e):
    """GenPublicKey (:74-90): one zero row modulo QP.  a: (1, LQ + LP, N), e: (1, N)"""
    kq, kp, _ = gadget(sk, None, Q, P, len(Q) - 1, len(P) - 1, 0, a, e, dpl=[1])
    return kq, kp


def evaluation_key(sk_in, sk_out, Q, P, levelQ, levelP, pw2, a, e):
    kq, kp, dpl = gadget(sk_out, sk_in.rows(Q[:levelQ + 1]), Q, P, levelQ, levelP, pw2, a, e)
    return rr.GadgetKey(kq, kp, levelQ, levelP, pw2, dpl)


def relin_key(sk, Q, P, levelQ, levelP, pw2, a, e):
    """(:115-120): skIn = sk^2 by MulCoeffsMontgomery on the rows"""
    mods = [int(q) for q in Q[:levelQ + 1]]
    s = sk.rows(mods)
    kq, kp, dpl = gadget(sk, rr._vec("MUL_MONT", s, s, mods), Q, P, levelQ, levelP, pw2, a, e)
    return rr.GadgetKey(kq, kp, levelQ, levelP, pw2, dpl)


def galois_keys(sk, galEls, Q, P, levelQ, levelP, pw2, a, e):
    """GenGaloisKeysNew (:195-205): a, e key-major over all keys.  skOut by the NTT automorphism of g^-1 on the rows of sk (:150-170)."""
    rows = rows_of(Q, levelQ, levelP, pw2)
    mods = [int(q) for q in Q[:levelQ + 1]] + ([int(p) for p in P[:levelP + 1]] if levelP >= 0 else [])
    out = []
    for k, g in enumerate(galEls):
        inv = rr.galois_inverse(sk.N, g)
        so = rr.Secret(sk.N, sk.coeffs)
        so._rows = {q: orc.automorphism_ntt(r, inv) for q, r in zip(mods, sk.rows(mods))}
        kq, kp, dpl = gadget(so, sk.rows(mods[:levelQ + 1]), Q, P, levelQ, levelP, pw2, a[k * rows:(k + 1) * rows], e[k * rows:(k + 1) * rows])
        out.append(rr.GadgetKey(kq, kp, levelQ, levelP, pw2, dpl))
    return out


def encrypt_sk(sk, Q, level, c1, e, pt=None, is_ntt=True):
    """encryptZeroSk + addPtToCt (encryptor.go:355-424, :512-530): c1 the uniform sample, e the error ints, pt in the ciphertext's domain"""
    mods = [int(q) for q in Q[:level + 1]]
    N = sk.N
    c1 = np.asarray(c1, dtype=np.uint64)
    if is_ntt:
        c0 = rr._vec("SUB", rr.ntt(rr.rns(e, mods), N, mods), rr._vec("MUL_MONT", c1, sk.rows(mods), mods), mods)
    else:
        c1n = rr.ntt(c1, N, mods)                                        # the sample is read as coefficients and transformed (:369-371)
        neg = rr._vec("SUB", np.zeros_like(c1), rr._vec("MUL_MONT", c1n, sk.rows(mods), mods), mods)
        c0 = rr._vec("ADD", rr.intt(neg, N, mods), rr.rns(e, mods), mods)
        c1 = rr.intt(c1n, N, mods)
    if pt is not None:
        c0 = rr._vec("ADD", c0, np.asarray(pt, dtype=np.uint64), mods)
    return [c0, c1]


def encrypt_pk(pkQ, pkP, Q, P, level, N, u, e0, e1, pt=None, is_ntt=True):
    """encryptZeroPk for a ciphertext (encryptor.go:218-308: levelP = 0), or encryptZeroPkNoP (:310-350) when P is empty.
    pkQ: (1, 2, LQ, N), pkP: (1, 2, LP, N) or None."""
    mq = [int(q) for q in Q[:level + 1]]
    if not len(P):
        un = rr.ntt(rr.rns(u, mq), N, mq)
        ct = []
        for c, e in ((0, e0), (1, e1)):
            x = rr._vec("MUL_MONT", un, pkQ[0, c, :level + 1], mq)
            if is_ntt:
                x = rr._vec("ADD", x, rr.ntt(rr.rns(e, mq), N, mq), mq)
            else:
                x = rr._vec("ADD", rr.intt(x, N, mq), rr.rns(e, mq), mq)
            ct.append(x)
    else:
        mp = [int(P[0])]
        uq, up = rr.ntt(rr.rns(u, mq), N, mq), rr.ntt(rr.rns(u, mp), N, mp)
        ct = []
        for c, e in ((0, e0), (1, e1)):
            xq = rr._vec("ADD", rr.intt(rr._vec("MUL_MONT", uq, pkQ[0, c, :level + 1], mq), N, mq), rr.rns(e, mq), mq)
            xp = rr._vec("ADD", rr.intt(rr._vec("MUL_MONT", up, pkP[0, c, :1], mp), N, mp), rr.rns(e, mp), mp)
            x = orc.moddown_qp_to_q(xq, xp, mq, mp)
            ct.append(rr.ntt(x, N, mq) if is_ntt else x)
    if pt is not None:
        ct[0] = rr._vec("ADD", ct[0], np.asarray(pt, dtype=np.uint64), mq)
    return ct


def decrypt(ct, sk, Q, is_ntt=True):
    """Decryptor.Decrypt (decryptor.go:51-92): the Horner sum in the NTT domain, canonical, back in the ciphertext's domain"""
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    N = sk.N
    vals = [np.asarray(c, dtype=np.uint64) if is_ntt else rr.ntt(np.asarray(c, dtype=np.uint64), N, mods) for c in ct]
    s = sk.rows(mods)
    acc = vals[-1]
    for c in reversed(vals[:-1]):
        acc = rr._vec("ADD", rr._vec("MUL_MONT", acc, s, mods), c, mods)
    return acc if is_ntt else rr.intt(acc, N, mods)


# ---- the noise bounds of the reference's tests -----------------------------------------------------------------------------------------------------
def noise_fresh_sk(sigma=rr.SIGMA):
    """Parameters.NoiseFreshSK (core/rlwe/params.go:474-476)"""
    return sigma


def noise_fresh_pk(hamming_weight, has_p, sigma=rr.SIGMA):
    """Parameters.NoiseFreshPK (core/rlwe/params.go:454-470) on a standard ring"""
    import math
    std = float(hamming_weight + 1)
    std *= 1 / 12.0 if has_p else sigma * sigma
    return math.sqrt(std)

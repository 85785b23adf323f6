"""The protocols of the reference's multiparty/ package with EXPLICIT samples, over the pinned oracle pieces and the helpers of
tests/rlwe_restatement.py and tests/keygen_restatement.py: what matrix-fhe-lattigo_amd/multiparty.py is compared with, bit for bit, when it is
handed the same samples.  TEST INFRASTRUCTURE ONLY.

Polys are numpy uint64 arrays (limbs, N), limbs of Q first and then of P; a secret is handed in as its rows (limbs, N) in the NTT domain and in
Montgomery form, so that an additive share out of the Combiner -- which has no small coefficients -- is an input like any other.  Shares and
CRPs of the gadget protocols are (rows, limbs, N), flat row sum(dpl[:i]) + j for Value[i][j]; a round-one relinearisation share is
(rows, 2, limbs, N).  Every result is canonical."""
import numpy as np

import keygen_restatement as kr
import rlwe_restatement as rr
from oracle import ring_oracle as orc
from oracle.compose import OPS


def mods_of(Q, P, levelQ, levelP):
    return [int(q) for q in Q[:levelQ + 1]] + ([int(p) for p in P[:levelP + 1]] if levelP >= 0 else [])


def add(a, b, mods):
    return rr._vec("ADD", np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64), mods)


def aggregate(shares, mods):
    """AggregateShares of every protocol, folded pairwise as the reference does (keygen_evk.go:213-242): arrays of (..., limbs, N)"""
    shares = [np.asarray(s, dtype=np.uint64) for s in shares]
    shape = shares[0].shape
    flat = [s.reshape(-1, shape[-2], shape[-1]) for s in shares]
    out = flat[0]
    for s in flat[1:]:
        out = np.stack([add(x, y, mods) for x, y in zip(out, s)])
    return out.reshape(shape)


def _digit_scalars(Q, P, levelQ, levelP, pw2, dpl):
    """per flat row, {limb of Q: P 2^(j pw2) in Montgomery form} on the limbs of the row's digit (keygen_evk.go:183-199)"""
    Pb = rr.prod([int(p) for p in P[:levelP + 1]]) if levelP >= 0 else 1
    width = max(levelP, 0) + 1
    rows = []
    for i in range(len(dpl)):
        for j in range(dpl[i]):
            f = Pb << (j * pw2)
            row = {}
            for k in range(width):
                index = i * width + k
                if index >= levelQ + 1:
                    break
                row[index] = (f << 64) % int(Q[index])
            rows.append(row)
    return rows


def _mul_scalar_mont(row, s, q):
    return orc.vec_op(OPS["MUL_SCALAR_MONT"], row, None, np.zeros(row.shape[0], dtype=np.uint64), s, 0, q)


def gadget_share(sk_in_rows, sk_out_rows, Q, P, levelQ, levelP, pw2, crp, e, dpl=None):
    """EvaluationKeyGenProtocol.GenShare (keygen_evk.go:115-210): per row MForm(NTT(e)) + skIn P 2^(j pw2) on the digit limbs - crp skOut.
    sk_in_rows (LQ, N) or None (a row without a plaintext term: PublicKeyGenProtocol.GenShare, keygen_cpk.go:70-83); sk_out_rows (LQ + LP, N);
    crp (rows, LQ + LP, N); e (rows, N) ints.  Returns (rows, LQ + LP, N)."""
    mods = mods_of(Q, P, levelQ, levelP)
    N = np.asarray(crp).shape[-1]
    dpl = rr.digits_per_limb(Q, levelQ, levelP, pw2) if dpl is None else dpl
    out = []
    for r, scal in enumerate(_digit_scalars(Q, P, levelQ, levelP, pw2, dpl)):
        h = rr.small_ntt_mont([int(x) for x in e[r]], N, mods)
        if sk_in_rows is not None:
            for index, s in scal.items():
                h[index] = orc.vec_op(OPS["ADD"], h[index], _mul_scalar_mont(sk_in_rows[index], s, mods[index]), h[index], 0, 0, mods[index])
        out.append(rr._vec("SUB", h, rr._vec("MUL_MONT", np.asarray(crp[r], dtype=np.uint64), sk_out_rows, mods), mods))
    return np.stack(out)


def public_key_share(sk_rows, Q, P, crp, e):
    """(keygen_cpk.go:70-83): crp (1, LQ + LP, N), e (1, N)"""
    return gadget_share(None, sk_rows, Q, P, len(Q) - 1, len(P) - 1, 0, crp, e, dpl=[1])


def gadget_key(share, crp, Q, P, levelQ, levelP, pw2, dpl=None):
    """GenEvaluationKey (keygen_evk.go:245-268) / GenPublicKey (keygen_cpk.go:91-94): Value[r] = (share[r], crp[r]) as an rr.GadgetKey"""
    key = np.stack([np.asarray(share, dtype=np.uint64), np.asarray(crp, dtype=np.uint64)], axis=1)
    dpl = rr.digits_per_limb(Q, levelQ, levelP, pw2) if dpl is None else dpl
    return rr.GadgetKey(key[:, :, :levelQ + 1].copy(), key[:, :, levelQ + 1:].copy() if levelP >= 0 else None, levelQ, levelP, pw2, dpl)


def galois_sk_out(sk_rows, N, g):
    """the NTT automorphism of g^-1 on every row of the secret (keygen_gal.go:65-74)"""
    inv = rr.galois_inverse(N, g)
    return np.stack([orc.automorphism_ntt(r, inv) for r in sk_rows])


def relin_round_one(sk_rows, u_rows, Q, P, levelQ, levelP, pw2, crp, e0, e1):
    """GenShareRoundOne (keygen_relin.go:130-222): (NTT(e0) + IMForm(P 2^(j pw2) sk) on the digit limbs - u crp, NTT(e1) + sk crp); no MForm of
    the errors.  Returns (rows, 2, LQ + LP, N)."""
    mods = mods_of(Q, P, levelQ, levelP)
    N = np.asarray(crp).shape[-1]
    dpl = rr.digits_per_limb(Q, levelQ, levelP, pw2)
    out = []
    for r, scal in enumerate(_digit_scalars(Q, P, levelQ, levelP, pw2, dpl)):
        a = np.asarray(crp[r], dtype=np.uint64)
        h0 = rr.ntt(rr.rns(e0[r], mods), N, mods)
        for index, s in scal.items():
            q = mods[index]
            sk_p = orc.vec_op(OPS["IMFORM"], _mul_scalar_mont(sk_rows[index], s, q), None, np.zeros(N, dtype=np.uint64), 0, 0, q)
            h0[index] = orc.vec_op(OPS["ADD"], h0[index], sk_p, h0[index], 0, 0, q)
        h0 = rr._vec("SUB", h0, rr._vec("MUL_MONT", u_rows, a, mods), mods)
        h1 = add(rr.ntt(rr.rns(e1[r], mods), N, mods), rr._vec("MUL_MONT", sk_rows, a, mods), mods)
        out.append(np.stack([h0, h1]))
    return np.stack(out)


def relin_round_two(u_rows, sk_rows, Q, P, levelQ, levelP, round1, e):
    """GenShareRoundTwo (keygen_relin.go:231-270): round1[0] sk + NTT(e) + (u - sk) round1[1].  Returns (rows, LQ + LP, N)."""
    mods = mods_of(Q, P, levelQ, levelP)
    N = sk_rows.shape[-1]
    delta = rr._vec("SUB", u_rows, sk_rows, mods)
    out = []
    for r in range(round1.shape[0]):
        h = add(rr._vec("MUL_MONT", round1[r, 0], sk_rows, mods), rr.ntt(rr.rns(e[r], mods), N, mods), mods)
        out.append(add(h, rr._vec("MUL_MONT", delta, round1[r, 1], mods), mods))
    return np.stack(out)


def relin_key(round1, round2, Q, P, levelQ, levelP, pw2):
    """GenRelinearizationKey (keygen_relin.go:297-312): (MForm(round2), MForm(round1[1]))"""
    mods = mods_of(Q, P, levelQ, levelP)
    mf = lambda x: rr._vec("MFORM", x, None, mods)
    return gadget_key(np.stack([mf(x) for x in round2]), np.stack([mf(x) for x in round1[:, 1]]), Q, P, levelQ, levelP, pw2)


def keyswitch_share(sk_in_rows, sk_out_rows, Q, level, c1, e, is_ntt=True):
    """KeySwitchProtocol.GenShare (keyswitch_sk.go:118-149) on one ciphertext: c1 (>= level + 1, N) in the ciphertext's domain, e (N,) ints"""
    mods = [int(q) for q in Q[:level + 1]]
    N = sk_in_rows.shape[-1]
    c1 = np.asarray(c1, dtype=np.uint64)[:level + 1]
    delta = rr._vec("SUB", sk_in_rows[:level + 1], sk_out_rows[:level + 1], mods)
    if is_ntt:
        return add(rr._vec("MUL_MONT", c1, delta, mods), rr.ntt(rr.rns(e, mods), N, mods), mods)
    return add(rr.intt(rr._vec("MUL_MONT", rr.ntt(c1, N, mods), delta, mods), N, mods), rr.rns(e, mods), mods)


def keyswitch(ct, combined, Q):
    """KeySwitchProtocol.KeySwitch (keyswitch_sk.go:164-178): (ct[0] + combined, ct[1])"""
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    return [add(ct[0], combined, mods), np.asarray(ct[1], dtype=np.uint64)]


def public_keyswitch_share(sk_rows, pkQ, pkP, Q, P, level, c1, u, e0, e1, e, is_ntt=True):
    """PublicKeySwitchProtocol.GenShare (keyswitch_pk.go:73-108): a zero encryption under pk (kr.encrypt_pk), then share[0] += c1 sk + e.
    P: the moduli of P the public key was made with ([] for none).  Returns [share0, share1]."""
    mods = [int(q) for q in Q[:level + 1]]
    N = sk_rows.shape[-1]
    zero = kr.encrypt_pk(pkQ, pkP, Q, P, level, N, u, e0, e1, None, is_ntt)
    c1 = np.asarray(c1, dtype=np.uint64)[:level + 1]
    if is_ntt:
        term = add(rr._vec("MUL_MONT", c1, sk_rows[:level + 1], mods), rr.ntt(rr.rns(e, mods), N, mods), mods)
    else:
        term = add(rr.intt(rr._vec("MUL_MONT", rr.ntt(c1, N, mods), sk_rows[:level + 1], mods), N, mods), rr.rns(e, mods), mods)
    return [add(zero[0], term, mods), zero[1]]


def public_keyswitch(ct, combined, Q):
    """PublicKeySwitchProtocol.KeySwitch (keyswitch_pk.go:125-137): (ct[0] + combined[0], combined[1])"""
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    return [add(ct[0], combined[0], mods), np.asarray(combined[1], dtype=np.uint64)]


# ---- threshold.go -------------------------------------------------------------------------------------------------------------------------------------
def lagrange(mods, this, that):
    """Combiner.lagrangeCoeff (:169-179): that (that - this)^-1 per modulus, Python integers"""
    return [int(that) % q * pow((int(that) - int(this)) % q, -1, q) % q for q in (int(m) for m in mods)]


def shamir_share(poly, point, mods):
    """GenShamirSecretShare (:102-104): Horner at the point (Ring.EvalPolyScalar), per limb on Python integers.  poly: [(limbs, N)] constant first"""
    out = []
    for i, q in enumerate(int(m) for m in mods):
        acc = poly[-1][i].astype(object)
        for c in reversed(poly[:-1]):
            acc = (acc * int(point) + c[i].astype(object)) % q
        out.append(np.array([int(x) % q for x in acc], dtype=np.uint64))
    return np.stack(out)


def additive_share(share, own, actives, threshold, mods):
    """GenAdditiveShare (:148-167): the own aggregated Shamir share times the product of the Lagrange factors of the first `threshold` actives"""
    out = []
    for i, q in enumerate(int(m) for m in mods):
        f = 1
        for a in actives[:threshold]:
            if a != own:
                f = f * lagrange([q], own, a)[0] % q
        out.append(np.array([int(x) * f % q for x in share[i].astype(object)], dtype=np.uint64))
    return np.stack(out)

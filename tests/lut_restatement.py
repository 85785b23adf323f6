"""Keys and key switching between ring degrees (core/rlwe/keygenerator.go:256-274, evaluator_evaluationkey.go:50-93, element.go:250-287), RGSW
encryption with its noise (core/rgsw/encryptor.go, utils.go) and the blind rotation key set (core/rgsw/blindrot/keys.go:45-108) restated on the CPU over
tests/rlwe_restatement.py and tests/keygen_restatement.py, with explicit samples.  TEST INFRASTRUCTURE ONLY: what KeyGenerator.GenEvaluationKeyNew,
Evaluator.ApplyEvaluationKey with NIn != NOut, rgsw.Encryptor and blindrot.GenEvaluationKeyNew are compared with, bit for bit, and what
tests/test_lut_oracle.py pins to decryption.

The reference's statements are kept literal: the smaller key goes up by REPEATING its NTT rows (ring.MapSmallDimensionToLargerDimensionNTT) and
is extended to further moduli from limb 0 alone (ExtendBasisSmallNormAndCenterNTTMontgomery).  tests/test_lut_oracle.py checks that this gives
the rows of s(X^(N/n)), which is how the device path states it."""
import numpy as np

import keygen_restatement as kr
import rlwe_restatement as rr


def embed(sk, N):
    """s(Y) with Y = X^(N/n): the coefficients of the smaller secret at every (N/n)-th place"""
    gap = N // sk.N
    c = [0] * N
    c[::gap] = sk.coeffs
    return rr.Secret(N, c)


def map_up_ntt(rows, gap):
    """ring.MapSmallDimensionToLargerDimensionNTT (ring/operations.go:380-392): every NTT coefficient gap times"""
    return np.repeat(np.asarray(rows, dtype=np.uint64), gap, axis=-1)


def extend_small_norm(row0, N, q0, mods):
    """ExtendBasisSmallNormAndCenterNTTMontgomery (core/rlwe/utils.go:250-284): INTT and IMForm of limb 0, centred at q0 >> 1 (`coeff > QHalf`
    is negative), reduced under `mods`, NTT, MForm"""
    x = rr._vec("IMFORM", rr.intt(np.asarray(row0, dtype=np.uint64)[None], N, [q0]), None, [q0])[0]
    c = [int(v) - q0 if int(v) > (q0 >> 1) else int(v) for v in x]
    return rr.small_ntt_mont(c, N, mods)


def mapped_secret(sk, N, Q, P, levelQ, levelP, as_input):
    """The smaller key as GenEvaluationKey holds it (:262-272).  As skOutput: Q rows repeated (as many as the small key has), P from limb 0.  As
    skInput: limb 0 repeated, then EVERY Q row from it.  Returned as a Secret of degree N whose rows are those literal words."""
    gap = N // sk.N
    Ql, Pl = [int(q) for q in Q[:levelQ + 1]], [int(p) for p in P[:levelP + 1]] if levelP >= 0 else []
    up = map_up_ntt(sk.rows(Ql), gap)
    out = embed(sk, N)
    if as_input:
        out._rows = dict(zip(Ql, extend_small_norm(up[0], N, Ql[0], Ql)))
    else:
        out._rows = dict(zip(Ql, up))
        if Pl:
            out._rows.update(zip(Pl, extend_small_norm(up[0], N, Ql[0], Pl)))
    return out


def degree_key(sk_in, sk_out, Q, P, levelQ, levelP, pw2, a, e):
    """GenEvaluationKey (:256-274) between degrees with explicit samples: the key lives in N = max of the two degrees"""
    N = max(sk_in.N, sk_out.N)
    si = mapped_secret(sk_in, N, Q, P, levelQ, -1, True) if sk_in.N < N else sk_in
    so = mapped_secret(sk_out, N, Q, P, levelQ, levelP, False) if sk_out.N < N else sk_out
    return kr.evaluation_key(si, so, Q, P, levelQ, levelP, pw2, a, e)


def random_degree_key(rnd, sk_in, sk_out, Q, P, levelQ, levelP, pw2):
    """the same key with the restatement's own samplers"""
    N = max(sk_in.N, sk_out.N)
    rows = kr.rows_of(Q, levelQ, levelP, pw2)
    mods = [int(q) for q in Q[:levelQ + 1]] + ([int(p) for p in P[:levelP + 1]] if levelP >= 0 else [])
    a = np.stack([rr.uniform_poly(rnd, N, mods) for _ in range(rows)])
    e = [rr.gaussian_coeffs(rnd, N) for _ in range(rows)]
    return degree_key(sk_in, sk_out, Q, P, levelQ, levelP, pw2, a, e)


def switch_degree_ntt(ct, NIn, NOut, Q):
    """SwitchCiphertextRingDegreeNTT (core/rlwe/element.go:250-287).  ct: [c0, c1] of (level + 1, NIn)"""
    mods = [int(q) for q in Q[:ct[0].shape[0]]]
    if NIn < NOut:
        return [map_up_ntt(c, NOut // NIn) for c in ct]
    gap = NIn // NOut
    return [rr.ntt(np.ascontiguousarray(rr.intt(np.asarray(c, dtype=np.uint64), NIn, mods)[:, ::gap]), NOut, mods) for c in ct]


def apply_evaluation_key(NIn, NOut, Q, P, ct, key):
    """Evaluator.ApplyEvaluationKey (core/rlwe/evaluator_evaluationkey.go:37-123), every branch"""
    if NIn < NOut:
        return rr.apply_evaluation_key(NOut, Q, P, switch_degree_ntt(ct, NIn, NOut, Q), key)
    if NIn > NOut:
        return switch_degree_ntt(rr.apply_evaluation_key(NIn, Q, P, ct, key), NIn, NOut, Q)
    return rr.apply_evaluation_key(NIn, Q, P, ct, key)


# ---- core/rgsw/encryptor.go, utils.go; core/rgsw/blindrot/keys.go ---------------------------------------------------------------------------------------
def rgsw_encrypt(sk, pt_rows, Q, P, levelQ, levelP, pw2, a, e):
    """rgsw.Encryptor.Encrypt (core/rgsw/encryptor.go:25-118) with explicit samples: a (2 rows, LQ + LP, N) and e (2 rows, N), the rows of Value[0]
    before those of Value[1].  Every row is an encryption of zero; pt w goes onto component 0 of Value[0] and component 1 of Value[1]
    (AddPolyTimesGadgetVectorToGadgetCiphertext, core/rlwe/gadgetciphertext.go:172-241).  pt_rows: (LQ, N), NTT domain, Montgomery form, or None.
    Returns [GadgetKey, GadgetKey]."""
    from oracle import ring_oracle as orc
    from oracle.compose import OPS
    rows = kr.rows_of(Q, levelQ, levelP, pw2)
    N = sk.N
    kq0, kp0, dpl = kr.gadget(sk, pt_rows, Q, P, levelQ, levelP, pw2, a[:rows], e[:rows])
    kq1, kp1, _ = kr.gadget(sk, None, Q, P, levelQ, levelP, pw2, a[rows:], e[rows:])
    if pt_rows is not None:
        Ql = [int(q) for q in Q[:levelQ + 1]]
        Pb = rr.prod(P[:levelP + 1]) if levelP >= 0 else 1
        width = max(levelP, 0) + 1
        r = 0
        for i in range(len(dpl)):
            for j in range(dpl[i]):
                f = Pb << (j * pw2)
                for k in range(width):
                    index = i * width + k
                    if index >= levelQ + 1:
                        break
                    q = Ql[index]
                    term = orc.vec_op(OPS["MUL_SCALAR_MONT"], pt_rows[index], None, np.zeros(N, dtype=np.uint64), (f << 64) % q, 0, q)
                    kq1[r, 1, index] = orc.vec_op(OPS["ADD"], kq1[r, 1, index], term, kq1[r, 1, index], 0, 0, q)
                r += 1
    return [rr.GadgetKey(kq0, kp0, levelQ, levelP, pw2, dpl), rr.GadgetKey(kq1, kp1, levelQ, levelP, pw2, dpl)]


def noise_gadget(key, pt_rows, sk, Q, P):
    """rlwe.NoiseGadgetCiphertext (core/rlwe/utils.go:51-102): decrypt every row, sum the RNS digits, subtract P 2^(j pw2) pt, INTT, IMForm, and the
    largest Log2OfStandardDeviation over the power-of-two digits"""
    levelQ, levelP, pw2 = key.levelQ, key.levelP, key.pw2
    Ql, Pl = [int(q) for q in Q[:levelQ + 1]], [int(p) for p in P[:levelP + 1]] if levelP >= 0 else []
    mods = Ql + Pl
    N = sk.N
    full = np.concatenate([key.Q, key.P], axis=2) if Pl else key.Q
    s = sk.rows(mods)
    dec = [rr._vec("ADD", full[r, 0], rr._vec("MUL_MONT", full[r, 1], s, mods), mods) for r in range(full.shape[0])]
    dpl = key.digits_per_limb if key.digits_per_limb is not None else [1] * full.shape[0]
    start = [sum(dpl[:i]) for i in range(len(dpl))]
    pt = [[int(v) * (rr.prod(Pl) if Pl else 1) % q for v in pt_rows[u]] for u, q in enumerate(Ql)]
    worst = float("-inf")
    for j in range(min(dpl)):
        acc = dec[start[0] + j]
        for i in range(1, len(dpl)):
            acc = rr._vec("ADD", acc, dec[start[i] + j], mods)
        acc = acc.copy()
        for u, q in enumerate(Ql):
            acc[u] = (acc[u].astype(object) - np.array(pt[u], dtype=object)) % q
        acc = acc.astype(np.uint64)
        x = rr._vec("IMFORM", rr.intt(acc, N, mods), None, mods)
        worst = max(worst, rr.log2_std(rr.crt_centered(x, mods)))
        pt = [[v * (1 << pw2) % q for v in pt[u]] for u, q in enumerate(Ql)]
    return worst


def noise_rgsw(value, pt_rows, sk, Q, P):
    """rgsw.NoiseRGSWCiphertext (core/rgsw/utils.go:10-14): Value[0] against pt, Value[1] against pt sk"""
    Ql = [int(q) for q in Q[:value[0].levelQ + 1]]
    ptsk = rr._vec("MUL_MONT", np.asarray(pt_rows, dtype=np.uint64), sk.rows(Ql), Ql)
    return noise_gadget(value[0], pt_rows, sk, Q, P), noise_gadget(value[1], ptsk, sk, Q, P)


def monomial_rows(N, i, mods):
    """MForm(NTT(ring.NewMonomialXi(i))): X^i, or -X^(i - N) for N <= i mod 2N"""
    import blindrot_restatement as br
    return rr.small_ntt_mont(br.monomial(N, i), N, mods)


def blind_rotation_keys(sk_br, sk_lwe, N, q, pw2, a_rgsw, e_rgsw, a_gal, e_gal):
    """blindrot.GenEvaluationKeyNew (core/rgsw/blindrot/keys.go:45-108) with explicit samples at one modulus without P: RGSW(X^{s_i}) per LWE
    coefficient (a_rgsw: (N_LWE * 2 rows, 1, N), key-major) and the eleven Galois keys (a_gal: (11 rows, 1, N)) -> blindrot_restatement.KeySet"""
    import blindrot_restatement as br
    Q = [int(q)]
    rows = kr.rows_of(Q, 0, -1, pw2)
    brk = [rgsw_encrypt(sk_br, monomial_rows(N, int(si), Q), Q, [], 0, -1, pw2, a_rgsw[2 * rows * i:2 * rows * (i + 1)], e_rgsw[2 * rows * i:2 * rows * (i + 1)])
           for i, si in enumerate(sk_lwe.coeffs)]
    els = br.galois_elements(N)
    gks = dict(zip(els, kr.galois_keys(sk_br, els, Q, [], 0, -1, pw2, a_gal, e_gal)))
    return br.KeySet(brk, gks, pw2)

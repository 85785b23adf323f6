"""CKKS on the conjugate-invariant ring Z[X + X^-1]/(X^2n + 1), restated on the CPU over the pinned oracle pieces: the arms of the reference
that differ from the standard ring, on top of keygen_restatement, ckks_encoder_restatement, ckks_restatement and oracle/compose.py.
TEST INFRASTRUCTURE ONLY: tests/test_ci_ckks_oracle.py pins it to things that are not it (the canonical embedding, exact integers, decryption
bounds); tests/test_gpu_ci_ckks.py compares the device with it bit for bit.

  ntt / intt                 ring.NumberTheoreticTransformerConjugateInvariant     oracle.ntt_ci / intt_ci with NthRoot = 4n
  Secret, public_key, ...    core/rlwe/keygenerator.go, encryptor.go, decryptor.go  keygen_restatement with the transforms above (ci_ring)
  galois_keys                GenGaloisKeysNew :195-205                              elements 5^k mod 4n, inverse modulo 4n
  embed / decode             schemes/ckks/encoder.go, the ConjugateInvariant arms   :225-228, utils.go:145-147, :825-831, :938-944
  mapped_secret              GenEvaluationKeysForRingSwapNew :207-228               from the small coefficients; unfold identity in the tests
  complex_to_real / real_to_complex   schemes/ckks/bridge.go :55-129                gadget product on the STANDARD ring (rlwe_restatement)
  gadget_product, relinearize, rotate, rescale   the evaluator's calls on the conjugate-invariant ring (not bit-pinned on the device here: the
                             device's gadget product on such rings is pinned on arbitrary residues in tests/test_gpu_keyswitch.py)

Polys are numpy uint64 arrays (limbs, n)."""
import contextlib
import functools

import numpy as np

import ckks_encoder_restatement as er
import keygen_restatement as kr
import rlwe_restatement as rr
from oracle import ring_oracle as orc
from oracle.compose import OPS, fold_standard_to_ci, unfold_ci_to_standard


@functools.lru_cache(maxsize=None)
def subring(n, q):
    return orc.SubRingConsts(n, int(q), nthroot=4 * n)


def ntt(x, n, mods):
    return np.stack([orc.ntt_ci(x[i], subring(n, q)) for i, q in enumerate(mods)])


def intt(x, n, mods):
    return np.stack([orc.intt_ci(x[i], subring(n, q)) for i, q in enumerate(mods)])


@contextlib.contextmanager
def ci_ring():
    """rlwe_restatement's transforms (what keygen_restatement and Secret.rows call) are the conjugate-invariant ones inside the block"""
    saved = rr.ntt, rr.intt
    rr.ntt, rr.intt = ntt, intt
    try:
        yield
    finally:
        rr.ntt, rr.intt = saved


class Secret(rr.Secret):
    """a secret of the conjugate-invariant ring: rows through the conjugate-invariant NTT"""

    def rows(self, mods):
        with ci_ring():
            return rr.Secret.rows(self, mods)


def _ci(f):
    @functools.wraps(f)
    def run(*a, **kw):
        with ci_ring():
            return f(*a, **kw)
    return run


public_key, evaluation_key, relin_key = _ci(kr.public_key), _ci(kr.evaluation_key), _ci(kr.relin_key)
encrypt_sk, encrypt_pk, decrypt = _ci(kr.encrypt_sk), _ci(kr.encrypt_pk), _ci(kr.decrypt)


def galois_element(n, k):
    """core/rlwe/params.go:671-675 with NthRoot = 4n"""
    return pow(5, k % (4 * n), 4 * n)


def galois_keys(sk, galEls, Q, P, levelQ, levelP, pw2, a, e):
    """keygen_restatement.galois_keys with the index map over NthRoot = 4n and ModInvGaloisElement modulo 4n"""
    rows = kr.rows_of(Q, levelQ, levelP, pw2)
    mods = [int(q) for q in Q[:levelQ + 1]] + ([int(p) for p in P[:levelP + 1]] if levelP >= 0 else [])
    out = []
    with ci_ring():
        for k, g in enumerate(galEls):
            inv = pow(int(g), 4 * sk.N - 1, 4 * sk.N)
            so = Secret(sk.N, sk.coeffs)
            so._rows = {q: orc.automorphism_ntt_ci(r, inv) for q, r in zip(mods, sk.rows(mods))}
            kq, kp, dpl = kr.gadget(so, sk.rows(mods[:levelQ + 1]), Q, P, levelQ, levelP, pw2, a[k * rows:(k + 1) * rows], e[k * rows:(k + 1) * rows])
            out.append(rr.GadgetKey(kq, kp, levelQ, levelP, pw2, dpl))
    return out


# ---- the real-only encoder ------------------------------------------------------------------------------------------------------------------------
def embed_coeffs(values, log_slots, scale, n, moduli):
    """embedDouble on a conjugate-invariant ring up to the quantizer, with the stride-gap spread: the imaginary parts are dropped (:225-228),
    the IFFT runs with m = 4n, the real parts alone are quantized (utils.go:145-147) at stride n / slots"""
    slots = 1 << log_slots
    values = np.asarray(values)
    assert values.ndim == 1 and len(values) <= slots <= n
    re = np.zeros(slots)
    re[:len(values)] = values.real
    re, _ = er.special_ifft(re, np.zeros(slots), 4 * n)
    gap = n // slots
    out = np.zeros((len(moduli), n), dtype=np.uint64)
    out[:, 0:slots * gap:gap] = er.quantize(re, scale, moduli)
    return out


def _canonical(words, moduli):
    return words % np.array([int(q) for q in moduli], dtype=np.uint64)[:, None]


def embed(values, log_slots, scale, n, moduli, is_ntt=True, is_montgomery=False):
    """with neither flag the quantizer's own words (positive values unreduced, the word q for a negative multiple of q); with either the
    canonical residues, which is what the reference's transform / MForm makes of them"""
    out = embed_coeffs(values, log_slots, scale, n, moduli)
    if is_ntt or is_montgomery:
        out = _canonical(out, moduli)
    if is_ntt:
        out = ntt(out, n, moduli)
    if is_montgomery:
        out = np.stack([er.mform(out[j], q) for j, q in enumerate(moduli)])
    return out


def encode_coeffs(values, scale, n, moduli, is_ntt=False):
    values = np.asarray(values, dtype=np.float64)
    out = np.zeros((len(moduli), n), dtype=np.uint64)
    out[:, :len(values)] = er.quantize(values, scale, moduli)
    return ntt(_canonical(out, moduli), n, moduli) if is_ntt else out


def decode(poly, log_slots, scale, n, moduli, is_ntt=True, logprec=0, real_only=False):
    """decodePublic on a conjugate-invariant ring: the `isreal` arms of polyToComplexNoCRT / polyToComplexCRT -- the first `slots` strided
    coefficients are the real parts and values[i] -= complex(0, real(values[slots - i])) for i >= 1 -- then the special FFT with m = 4n and the
    rounding as written.  Returns (re, im)."""
    slots, scale = 1 << log_slots, float(scale)
    gap = n // slots
    if is_ntt:
        poly = intt(poly, n, moduli)
    re = np.array([er.centred_double(poly[:, i * gap], moduli) for i in range(slots)]) / scale
    im = np.zeros(slots)
    im[1:] = 0.0 - re[:0:-1]
    re, im = er.special_fft(re, im, 4 * n)
    if logprec != 0:
        import math
        p2 = math.pow(2.0, logprec)

        def rnd(a):
            return np.array([math.copysign(math.floor(abs(v)) + (1.0 if abs(v) - math.floor(abs(v)) >= 0.5 else 0.0), v) for v in a])
        re = rnd(re * p2) / p2
        im = np.zeros_like(im) if real_only else rnd(im * p2) / p2
    return re, im


def decode_coeffs(poly, scale, n, moduli, is_ntt=False):
    if is_ntt:
        poly = intt(poly, n, moduli)
    return np.array([er.centred_double(poly[:, i], moduli) for i in range(n)]) / float(scale)


# ---- ring swap and the domain switch --------------------------------------------------------------------------------------------------------------
def mapped_coeffs(coeffs):
    """s(X + X^-1) in Z[X]/(X^2n + 1) from the n small coefficients: m[0] = s_0, m[i] = s_i, m[2n - i] = -s_i (1 <= i < n), m[n] = 0"""
    n = len(coeffs)
    m = [0] * (2 * n)
    m[0] = int(coeffs[0])
    for i in range(1, n):
        m[i] = int(coeffs[i])
        m[2 * n - i] = -int(coeffs[i])
    return m


def mapped_secret(sk):
    """the conjugate-invariant secret as a secret of the standard ring of twice the degree (GenEvaluationKeysForRingSwapNew :212-217)"""
    return rr.Secret(2 * sk.N, mapped_coeffs(sk.coeffs))


def ring_swap_keys(sk_std, sk_ci, Q, P, levelQ, levelP, pw2, a, e):
    """(stdToci, ciToStd): a, e pairs of samples, one entry per key"""
    m = mapped_secret(sk_ci)
    return (kr.evaluation_key(sk_std, m, Q, P, levelQ, levelP, pw2, a[0], e[0]), kr.evaluation_key(m, sk_std, Q, P, levelQ, levelP, pw2, a[1], e[1]))


def automorphism_index(N):
    """ring.AutomorphismNTTIndex(N, 2N, 2N - 1) (ring/automorphism.go:12-34)"""
    lg = N.bit_length() - 1
    mask = 2 * N - 1
    rev = lambda x: int(format(x, "0%db" % lg)[::-1], 2) if lg else 0
    return [rev((((2 * N - 1) * (2 * rev(i) + 1) & mask) - 1) >> 1) for i in range(N)]


def complex_to_real(N, Q, P, ct, key):
    """DomainSwitcher.ComplexToReal (:55-87) at the level of ct: GadgetProduct of c1, Add with c0, the two folds.  ct: two (L, N) arrays in
    the NTT domain of the standard ring of degree N; returns two (L, N / 2) arrays.  The scale doubles (the caller's bookkeeping)."""
    level = ct[0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    g0, g1 = rr.gadget_product(N, Q, P, level, ct[1], key)
    t0 = rr._add(g0, ct[0], mods)
    index = automorphism_index(N)
    return [np.stack([fold_standard_to_ci(t[i], index, mods[i]) for i in range(level + 1)]) for t in (t0, g1)]


def real_to_complex(N, Q, P, ct, key):
    """DomainSwitcher.RealToComplex (:96-129): the two unfolds, GadgetProduct of the unfolded c1, Add onto the unfolded c0, copy"""
    level = ct[0].shape[0] - 1
    mods = [int(q) for q in Q[:level + 1]]
    u0, u1 = (np.stack([unfold_ci_to_standard(c[i]) for i in range(level + 1)]) for c in ct)
    g0, g1 = rr.gadget_product(N, Q, P, level, u1, key)
    return [rr._add(u0, g0, mods), g1]


# ---- the evaluator's calls on the conjugate-invariant ring ------------------------------------------------------------------------------------------
def _vec(op, a, b, acc, mods):
    return np.stack([orc.vec_op(OPS[op], a[i], b[i] if b is not None else None, acc[i], 0, 0, mods[i]) for i in range(len(mods))])


def gadget_product(n, Q, P, levelQ, cx, key):
    """Evaluator.GadgetProduct, NTT-domain input, RNS digits (no power-of-two decomposition), levelP >= 0: per digit DecomposeSingleNTT and the
    product with the key row, summed canonically (the reference sums lazily and reduces: the same residues), then the ModDown taken in the
    coefficient domain (INTT, ModDownQPtoQ, NTT: the canonical words of ModDownQPtoQNTT, the transform being linear)"""
    levelQ, levelP = min(levelQ, key.levelQ), key.levelP
    assert levelP >= 0 and not key.pw2
    LQ, LP = levelQ + 1, levelP + 1
    Ql, Pl = [int(q) for q in Q[:LQ]], [int(p) for p in P[:LP]]
    cxinv = intt(cx, n, Ql)
    accQ = [np.zeros((LQ, n), dtype=np.uint64) for _ in (0, 1)]
    accP = [np.zeros((LP, n), dtype=np.uint64) for _ in (0, 1)]
    for d in range((levelQ + levelP + 1) // (levelP + 1)):
        c2q, c2p = orc.decompose_and_split(levelQ, levelP, LP, d, cxinv, Q, P)
        st, ed = d * LP, min(d * LP + LP, LQ)
        c2q = np.stack([cx[i] if st <= i < ed else orc.ntt_ci(c2q[i], subring(n, Ql[i])) for i in range(LQ)])
        c2p = ntt(c2p, n, Pl)
        for c in (0, 1):
            accQ[c] = _vec("MUL_MONT_THEN_ADD", key.Q[d, c, :LQ], c2q, accQ[c], Ql)
            accP[c] = _vec("MUL_MONT_THEN_ADD", key.P[d, c, :LP], c2p, accP[c], Pl)
    return [ntt(orc.moddown_qp_to_q(intt(accQ[c], n, Ql), intt(accP[c], n, Pl), Ql, Pl), n, Ql) for c in (0, 1)]


def relinearize(n, Q, P, ct, key):
    level = ct[0].shape[0] - 1
    k0, k1 = gadget_product(n, Q, P, level, ct[2], key)
    return [rr._add(ct[0], k0, Q[:level + 1]), rr._add(ct[1], k1, Q[:level + 1])]


def rotate(n, Q, P, ct, key, g):
    """Evaluator.Automorphism: the key switch with GaloisKey[g], then the NTT automorphism of g over NthRoot = 4n on both components"""
    level = ct[0].shape[0] - 1
    k0, k1 = gadget_product(n, Q, P, level, ct[1], key)
    out = [rr._add(ct[0], k0, Q[:level + 1]), k1]
    return [np.stack([orc.automorphism_ntt_ci(x[i], g) for i in range(x.shape[0])]) for x in out]


def rescale(n, mods, ct):
    """DivRoundByLastModulusNTT on every component: INTT, the coefficient-domain division, NTT"""
    mods = [int(q) for q in mods]
    return [ntt(orc.div_by_last_modulus_many(intt(x, n, mods), mods, 1, True), n, mods[:-1]) for x in ct]

"""CPU: the restated key generator, encryptors and decryptor (tests/keygen_restatement.py), fed by the restated samplers
(tests/sampling_restatement.py), pinned to DECRYPTION with the bounds the reference's own tests state (core/rlwe/rlwe_test.go):

  fresh secret-key encryption, every row of a public or evaluation key minus its plaintext term   log2(NoiseFreshSK) + 1    :451-464, :634, :661
  fresh public-key encryption                                                                      log2(NoiseFreshPK) + 1    :608, params.go:454-470
  a gadget product under a restated key                                                            LogN + pw2                :703
  an automorphism under a restated key                                                             LogN + pw2 (+ log2(level + 1) + 1 with pw2)   :925-929

Chains and settings are those of tests/test_rlwe_oracle.py (TAIL, REF, Q61N13; multi-P, single-P with pw2, no P), plus TAIL cut to six limbs of Q
under four of P, where #P does not divide #Q in another way (a last digit of two limbs).  tests/test_gpu_keygen.py runs the same samples through
the device path and compares whole arrays."""
import functools
import math
import random

import numpy as np
import pytest

import keygen_restatement as kr
import rlwe_restatement as rr
import sampling_restatement as sr
import test_rlwe_oracle as tro
from oracle import ring_oracle as orc
from oracle.compose import OPS

KEY = b"keygen restatement key"
TABLE = sr.gaussian_table(rr.SIGMA, rr.BOUND)
THRESHOLD = int(__import__("fractions").Fraction(2 / 3) * (1 << 63))
# (chain, (pw2, #P), levelQ of the keys or None for the top)
CASES = [("TAIL", (0, 4), None), ("TAIL", (0, 1), None), ("TAIL", (16, 1), None), ("TAIL", (0, 4), 5),
         ("REF", (0, 2), None), ("REF", (16, 1), None), ("REF", (2, 0), None), ("REF", (0, 1), None), ("Q61N13", (0, 2), None)]
_ids = lambda c: "%s-pw%d-p%d%s" % (c[0], c[1][0], c[1][1], "" if c[2] is None else "-l%d" % c[2])
GALOIS = (5, 25, -1)                                                     # three elements at once; -1 stands for 2N - 1


def dims(case):
    name, (pw2, pc), lq = case
    N, Q, P, levels = tro.chain(name)
    levelQ = levels[0] if lq is None else lq
    return N, [int(q) for q in Q], [int(p) for p in P[:pc]], levelQ, pc - 1, pw2


@functools.lru_cache(maxsize=None)
def secret_coeffs(name, which=0):
    N = tro.chain(name)[0]
    return sr.ternary(KEY, 1000 + which, 1, N, THRESHOLD)[0]


def secrets(name):
    return kr.secret(secret_coeffs(name, 0)), kr.secret(secret_coeffs(name, 1))


def gadget_samples(case, call, nkeys=1, dpl=None):
    """what one gadget_rows call of the device draws with call counters (call, call + 1): a (rows, LQ + LP, N), rows counting Q then P; e (rows, N)"""
    N, Q, P, levelQ, levelP, pw2 = dims(case)
    rows = nkeys * (kr.rows_of(Q, levelQ, levelP, pw2) if dpl is None else sum(dpl))
    mods = Q[:levelQ + 1] + P[:levelP + 1]
    return sr.uniform(KEY, call, rows, N, mods), sr.gaussian(KEY, call + 1, rows, N, TABLE)


def galois_elements(N):
    return [g % (2 * N) for g in GALOIS]


@functools.lru_cache(maxsize=None)
def keys(case):
    """{"pk", "evk", "rlk", "gks", samples ...} of a case, made once and shared with the GPU tests"""
    N, Q, P, levelQ, levelP, pw2 = dims(case)
    sk, sk_out = secrets(case[0])
    out = {}
    a, e = gadget_samples((case[0], (0, len(tro.chain(case[0])[2])), None), 10, dpl=[1])
    Pall = [int(p) for p in tro.chain(case[0])[2]]
    out["pk_samples"], out["pk"] = (a, e), kr.public_key(sk, Q, Pall, a, e)
    a, e = gadget_samples(case, 20)
    out["evk_samples"], out["evk"] = (a, e), kr.evaluation_key(sk, sk_out, Q, P, levelQ, levelP, pw2, a, e)
    a, e = gadget_samples(case, 30)
    out["rlk_samples"], out["rlk"] = (a, e), kr.relin_key(sk, Q, P, levelQ, levelP, pw2, a, e)
    a, e = gadget_samples(case, 40, nkeys=len(GALOIS))
    out["gks_samples"], out["gks"] = (a, e), kr.galois_keys(sk, galois_elements(N), Q, P, levelQ, levelP, pw2, a, e)
    return out


def fresh_bound():
    return math.log2(kr.noise_fresh_sk()) + 1


def row_noise(key, sk_out, sk_in, Q, P):
    """log2 std of every row's phase minus its plaintext term, modulo Q and modulo P (rlwe_test.go:440-464 on each row): (max over rows) per ring"""
    N = sk_out.N
    dpl = key.digits_per_limb if key.digits_per_limb is not None else [1] * key.Q.shape[0]
    Ql, Pl = Q[:key.levelQ + 1], P[:key.levelP + 1] if key.levelP >= 0 else []
    Pb = rr.prod(Pl)
    width = max(key.levelP, 0) + 1
    worst, r = [], 0
    for i in range(len(dpl)):
        for j in range(dpl[i]):
            for mods, val, in_q in ((Ql, key.Q, True), (Pl, key.P, False)):
                if not mods:
                    continue
                z = rr._vec("ADD", rr._vec("MUL_MONT", val[r, 1], sk_out.rows(mods), mods), val[r, 0], mods)
                if in_q and sk_in is not None:
                    for k in range(width):
                        index = i * width + k
                        if index >= key.levelQ + 1:
                            break
                        q = Ql[index]
                        term = orc.vec_op(OPS["MUL_SCALAR_MONT"], sk_in.rows([q])[0], None, np.zeros(N, dtype=np.uint64), ((Pb << (j * key.pw2)) << 64) % q, 0, q)
                        z[index] = orc.vec_op(OPS["SUB"], z[index], term, z[index], 0, 0, q)
                z = rr._vec("IMFORM", rr.intt(z, N, mods), None, mods)
                worst.append(rr.log2_std(rr.crt_centered(z, mods)))
            r += 1
    return max(worst)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_key_rows_are_fresh_encryptions(oracle, case):
    N, Q, P, levelQ, levelP, pw2 = dims(case)
    sk, sk_out = secrets(case[0])
    k = keys(case)
    Pall = [int(p) for p in tro.chain(case[0])[2]]
    pkq, pkp = k["pk"]
    pk = rr.GadgetKey(pkq, pkp, len(Q) - 1, len(Pall) - 1, 0, None)
    got = {"pk": row_noise(pk, sk, None, Q, Pall), "evk": row_noise(k["evk"], sk_out, sk, Q, P), "rlk": row_noise(k["rlk"], sk, sk.square(), Q, P)}
    for g, gk in zip(galois_elements(N), k["gks"]):
        got["gk%d" % g] = row_noise(gk, sk.automorphism(rr.galois_inverse(N, g)), sk, Q, P)
    for what, v in got.items():
        print("MEASURED %-8s %s  %5.2f [%.2f]" % (what, _ids(case), v, fresh_bound()))
        assert v <= fresh_bound(), what


def _levels(case):
    N, Q, P, levelQ, levelP, pw2 = dims(case)
    return sorted({levelQ, max(levelQ - 1, 0)}, reverse=True)


@functools.lru_cache(maxsize=None)
def operand(name, level):
    N, Q = tro.chain(name)[:2]
    return rr.uniform_poly(random.Random("kg a %s %d" % (name, level)), N, Q[:level + 1])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_restated_keys_switch_relinearize_and_rotate(oracle, case):
    N, Q, P, levelQ, levelP, pw2 = dims(case)
    sk, sk_out = secrets(case[0])
    k = keys(case)
    for level in _levels(case):
        mods = Q[:level + 1]
        M = rr.prod(mods)
        a = operand(case[0], level)
        zero = np.zeros_like(a)
        want = rr.phase([zero, a], sk, Q)
        got = rr.phase(list(rr.gadget_product(N, Q, P, level, a, k["evk"])), sk_out, Q)                       # (rlwe_test.go:733-749)
        v = rr.log2_std(rr.centered_diff(got, want, M))
        print("MEASURED switch  %s level %d  %5.2f [%.2f]" % (_ids(case), level, v, tro.bound(N, pw2)))
        assert v <= tro.bound(N, pw2)
        want2 = rr.phase([zero, zero, a], sk, Q)
        got2 = rr.phase(rr.relinearize(N, Q, P, [zero, zero, a], k["rlk"]), sk, Q)
        v = rr.log2_std(rr.centered_diff(got2, want2, M))
        print("MEASURED relin   %s level %d  %5.2f [%.2f]" % (_ids(case), level, v, tro.bound(N, pw2)))
        assert v <= tro.bound(N, pw2)
        for g, gk in zip(galois_elements(N), k["gks"]):
            out = rr.automorphism(N, Q, P, [zero, a], gk, g)
            v = rr.log2_std(rr.centered_diff(rr.phase(out, sk, Q), rr.automorphism_coeffs(want, g), M))
            print("MEASURED auto %-4d %s level %d  %5.2f [%.2f]" % (g, _ids(case), level, v, tro.bound(N, pw2, level)))
            assert v <= tro.bound(N, pw2, level)


def message(name, level, npoly=3):
    """a batch of small messages (|m| < 2^20) as NTT- and coefficient-domain plaintext rows"""
    N, Q = tro.chain(name)[:2]
    rnd = random.Random("kg m %s %d" % (name, level))
    return [[rnd.randrange(-(1 << 20), 1 << 20) for _ in range(N)] for _ in range(npoly)]


@functools.lru_cache(maxsize=None)
def encryptions(name, pc, level, is_ntt):
    """a batch of 3 under the secret key and under the public key (the chain's first pc moduli of P): samples, plaintexts and ciphertexts"""
    N, Q, P = tro.chain(name)[:3]
    Q, P = [int(q) for q in Q], [int(p) for p in P[:pc]]
    mods = Q[:level + 1]
    sk, _ = secrets(name)
    ms = message(name, level)
    pts = [rr.ntt(rr.rns(m, mods), N, mods) if is_ntt else rr.rns(m, mods) for m in ms]
    c1 = sr.uniform(KEY, 50, 3, N, mods)
    e = sr.gaussian(KEY, 51, 3, N, TABLE)
    out = {"m": ms, "pt": pts, "sk_samples": (c1, e), "sk": [kr.encrypt_sk(sk, Q, level, c1[k], e[k], pts[k], is_ntt) for k in range(3)]}
    a, ep = sr.uniform(KEY, 60, 1, N, Q + P), sr.gaussian(KEY, 61, 1, N, TABLE)
    pkq, pkp = kr.public_key(sk, Q, P, a, ep)
    u, e0, e1 = sr.ternary(KEY, 62, 3, N, THRESHOLD), sr.gaussian(KEY, 63, 3, N, TABLE), sr.gaussian(KEY, 64, 3, N, TABLE)
    out.update(pk_key_samples=(a, ep), pk_key=(pkq, pkp), pk_samples=(u, e0, e1),
               pk=[kr.encrypt_pk(pkq, pkp, Q, P, level, N, u[k], e0[k], e1[k], pts[k], is_ntt) for k in range(3)])
    return out


ENC = [("TAIL", 4), ("TAIL", 1), ("REF", 2), ("REF", 0), ("Q61N13", 2)]


@pytest.mark.parametrize("shape", ENC, ids=lambda s: "%s-p%d" % s)
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coeff"])
def test_fresh_encryptions_decrypt(oracle, shape, is_ntt):
    name, pc = shape
    N, Q, P, levels = tro.chain(name)
    Q = [int(q) for q in Q]
    sk, _ = secrets(name)
    hw = math.ceil(N * 2 / 3)                                              # Parameters.XsHammingWeight for Ternary{P} (params.go:427-434)
    for level in (levels[0], levels[0] - 1):
        mods = Q[:level + 1]
        enc = encryptions(name, pc, level, is_ntt)
        for what, bnd in (("sk", fresh_bound()), ("pk", math.log2(kr.noise_fresh_pk(hw, pc > 0)) + 1)):
            for k in range(3):
                pt = kr.decrypt(enc[what][k], sk, Q, is_ntt)
                coeffs = rr.crt_centered(rr.intt(pt, N, mods) if is_ntt else pt, mods)
                v = rr.log2_std([x - m for x, m in zip(coeffs, enc["m"][k])])
                print("MEASURED %s %s-p%d level %d %s  %5.2f [%.2f]" % (what, name, pc, level, "ntt" if is_ntt else "coeff", v, bnd))
                assert v <= bnd


def test_degree_two_decrypts(oracle):
    """c0 + s c1 + s^2 c2 by Horner: the tensor of two fresh encryptions decrypts to the product of the messages, exactly modulo Q up to its noise"""
    name = "REF"
    N, Q, P, levels = tro.chain(name)
    Q = [int(q) for q in Q]
    level = levels[0]
    mods = Q[:level + 1]
    sk, _ = secrets(name)
    enc = encryptions(name, 2, level, True)
    a, b = enc["sk"][0], enc["sk"][1]
    mf = lambda x: rr._vec("MFORM", x, None, mods)
    mul = lambda x, y: rr._vec("MUL_MONT", mf(x), y, mods)
    ct2 = [mul(a[0], b[0]), rr._vec("ADD", mul(a[0], b[1]), mul(a[1], b[0]), mods), mul(a[1], b[1])]
    got = rr.crt_centered(rr.intt(kr.decrypt(ct2, sk, Q), N, mods), mods)
    pa = rr.crt_centered(rr.intt(kr.decrypt(a, sk, Q), N, mods), mods)
    pb = rr.crt_centered(rr.intt(kr.decrypt(b, sk, Q), N, mods), mods)
    M = rr.prod(mods)
    want = [0] * N
    for i, x in enumerate(pa):
        for j, y in enumerate(pb):
            if i + j < N:
                want[i + j] += x * y
            else:
                want[i + j - N] -= x * y
    assert rr.centered_diff(got, want, M) == [0] * N

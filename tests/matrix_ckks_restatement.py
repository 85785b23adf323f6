"""schemes/matrix_ckks restated on the host: the encoder (both `negatives` forms), the scheme's own encryptor and decryptor, and key generation,
encryption and decryption of core/rlwe on a 3N ring given omega.  TEST INFRASTRUCTURE ONLY.

The key layer is tests/keygen_restatement.py as it stands: inside `ring3n(omegas)` the two transforms it calls (rlwe_restatement.ntt / intt) are
the oracle's 3N transforms (oracle.ring_oracle.ntt3n_forward / ntt3n_backward, the reference's ascending-totative order), so every formula of
that file is evaluated on Z_q[X]/(X^N - X^(N/2) + 1).  The ground truth of a product is naive_mul: the schoolbook product reduced with
X^N = X^(N/2) - 1 (ring/ntt_3n_test.go:103-107)."""
import contextlib
import struct

import numpy as np

import keygen_restatement as kr
import rlwe_restatement as rr
from oracle import ring_oracle as orc

M64 = (1 << 64) - 1
BIG = 1.8446744073709552e+19


def omega_for(q, N):
    """Find3NPrimitiveRoot (ring/subring.go:255-290)"""
    g = orc.lib().orc_primitive_root(int(q))
    return pow(g, (int(q) - 1) // (3 * N), int(q))


@contextlib.contextmanager
def ring3n(omegas):
    """omegas: {modulus: omega}.  keygen_restatement / rlwe_restatement transform with the 3N transforms while the block runs."""
    saved = rr.ntt, rr.intt
    rr.ntt = lambda x, N, mods: np.stack([orc.ntt3n_forward(x[i], int(q), omegas[int(q)]) for i, q in enumerate(mods)])
    rr.intt = lambda x, N, mods: np.stack([orc.ntt3n_backward(x[i], int(q), omegas[int(q)]) for i, q in enumerate(mods)])
    try:
        yield kr
    finally:
        rr.ntt, rr.intt = saved


def naive_mul(a, b):
    """a b in Z[X]/(X^N - X^(N/2) + 1) on Python integers"""
    N = len(a)
    c = [0] * (2 * N - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            c[i + j] += int(x) * int(y)
    for k in range(2 * N - 2, N - 1, -1):
        c[k - N // 2] += c[k]
        c[k - N] -= c[k]
        c[k] = 0
    return c[:N]


# ---- the encoder (schemes/matrix_ckks/encoder.go:367-445) ---------------------------------------------------------------------------------------------
def as_float(v):
    """the float64 a value stands for: float64(val) for uint64, the real part of a complex128"""
    if isinstance(v, (complex, np.complexfloating)):
        return float(v.real)
    return float(int(v)) if isinstance(v, (int, np.integer)) else float(v)


def reference_word(value, scale):
    """SingleFloat64ToFixedPointCRT (:384-426) up to the per-limb CRed: (the 64-bit word the reference reduces, the signed integer it stands
    for when read with its sign)"""
    value, scale = float(value), float(scale)
    if value == 0:
        return 0, 0
    neg = value < 0
    if neg:
        scale *= -1
    value *= scale
    if value >= BIG:
        exact = int(value)                                               # big.Float.Int of a float that is an integer
        return exact & M64, -exact if neg else exact
    c = int(value)                                                       # uint64(value): truncation
    return ((-c) & M64 if neg else c), (-c if neg else c)


def reference_stored(value, scale, q):
    """what the reference stores: ring.CRed(word, q), ONE conditional subtraction"""
    w, _ = reference_word(value, scale)
    return w - q if w >= q else w


def encode(values, scale, mods, N, negatives="as_written"):
    """one vector -> (len(mods), N) canonical residues; coefficients past the values are 0"""
    out = np.zeros((len(mods), N), dtype=np.uint64)
    for i, v in enumerate(values):
        w, signed = reference_word(as_float(v), scale)
        for l, q in enumerate(mods):
            out[l, i] = signed % int(q) if (negatives == "signed" and signed < 0) else w % int(q)
    return out


def decode(limb0, q0, scale, nvals):
    """polyToFloatNoCRT (:430-445)"""
    q0, scale = int(q0), float(scale)
    return np.array([-float(q0 - int(c)) / scale if int(c) >= q0 >> 1 else float(int(c)) / scale for c in limb0[:nvals]], dtype=np.float64)


# ---- the scheme's own encryptor and decryptor, as written (encryptor.go:48-86, decryptor.go:31-74) ------------------------------------------------------
def matrix_encrypt(sk_rows, mods, pt, a, e):
    """ct = (pt + e - MRed(a, sk.Value.Q), a): a and e small samples, the product coefficient-wise on the stored form of the secret"""
    c1, er = rr.rns(a, mods), rr.rns(e, mods)
    c0 = rr._vec("SUB", rr._vec("ADD", np.asarray(pt, dtype=np.uint64), er, mods), rr._vec("MUL_MONT", c1, sk_rows, mods), mods)
    return [c0, c1]


def matrix_decrypt(sk_rows, mods, ct):
    return rr._vec("ADD", ct[0], rr._vec("MUL_MONT", sk_rows, ct[1], mods), mods)


def float_bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]

"""circuits/bgv/lintrans/lintrans.go and the BGV arm of circuits/common/lintrans (rows = 2, integer scales, bgv.Evaluator.Rescale) restated on
host integers over the pinned pieces.  TEST INFRASTRUCTURE ONLY: what the device path (matrix-fhe-lattigo_amd/bgv_lintrans.py, fused and
composed, and rh_bgv_embed_qp) is compared with bit for bit, itself pinned to decryption by tests/test_bgv_lintrans_oracle.py.

What does not depend on the scheme is tests/lintrans_restatement.py's and is imported, not restated again: the index arithmetic, Diagonals.At,
MultiplyByDiagMatrix(BSGS), the pre-rotations and EvaluateMany (they read a transformation as (Q rows, P rows) per diagonal, whatever encoded
it).  The encoder is tests/bgv_encoder_restatement.py's, Rescale tests/bgv_restatement.py's.

A diagonal holds 2 * cols values, row 0 then row 1; ciphertexts are lists [c0, c1] of (limbs, N) uint64 arrays in the NTT domain; keys:
{Galois element: rr.GadgetKey}."""
import math

import numpy as np

import bgv_encoder_restatement as be
import bgv_restatement as br
import lintrans_restatement as ltr
import rlwe_restatement as rr
from lintrans_restatement import (Transformation, bsgs_index, diagonals_at, evaluate_many, find_best_bsgs_ratio, galois_elements,  # noqa: F401
                                  multiply_by_diag_matrix, multiply_by_diag_matrix_bsgs, rotate)
from oracle import ring_oracle as orc


# ---- circuits/bgv/lintrans/lintrans.go ---------------------------------------------------------------------------------------------------------
def diagonals_evaluate(m, vector, t):
    """Diagonals.Evaluate (:24-58) on integers modulo t: the BSGS schedule of ratio 1 on each half of the 2 x slots matrix"""
    slots = len(vector) >> 1                                             # (:26)
    keys = list(m)
    n1 = find_best_bsgs_ratio(keys, slots, 1)
    index, _, _ = bsgs_index(keys, slots, n1)
    vector = [int(x) for x in vector]
    res = [0] * (2 * slots)
    for j in index:
        rot = -j & (slots - 1)
        tmp = [0] * (2 * slots)
        for i in index[j]:
            v = [int(x) for x in (m[j + i] if j + i in m else m[j + i - slots])]
            for lo in (0, slots):                                        # (:49-50)
                a, b = rotate(vector[lo:lo + slots], i), rotate(v[lo:lo + slots], rot)
                tmp[lo:lo + slots] = [(z + x * y) % t for x, y, z in zip(a, b, tmp[lo:lo + slots])]
        for lo in (0, slots):                                            # (:53-54)
            res[lo:lo + slots] = [(x + y) % t for x, y in zip(res[lo:lo + slots], rotate(tmp[lo:lo + slots], j))]
    return res


def dense_apply(m, vector, t):
    """the definition: out[r][c] = sum_k diag_k[r][c] * vector[r][(c + k) mod slots] -- each row a slots x slots matrix in diagonal form"""
    slots = len(vector) >> 1
    out = [0] * (2 * slots)
    for k, d in m.items():
        for r in (0, 1):
            for c in range(slots):
                out[r * slots + c] = (out[r * slots + c] + int(d[r * slots + c]) * int(vector[r * slots + (c + k) % slots])) % t
    return out


def permutation_diagonals(perm, log_slots):
    """Permutation.GetDiagonals (:80-107); perm: a pair of lists [(From, To, Scaling)], one per row"""
    slots = 1 << (log_slots - 1)                                         # (:82)
    out = {}
    for i, row in enumerate(perm):
        offset = i * slots
        for frm, to, scaling in row:
            d = (slots + frm - to) & (slots - 1)
            if d not in out:
                out[d] = [0] * (2 * slots)
            out[d][to + offset] = scaling
    return out


# ---- circuits/common/lintrans/lintrans.go with rows = 2 -----------------------------------------------------------------------------------------
def rotate_rows(v, rot, cols):
    """rotateAndEncodeDiagonal's loop (:283-285): each row of cols values rotated to the left by rot & (cols - 1)"""
    rot &= cols - 1
    v = list(v)
    return [x for r in range(len(v) // cols) for x in rotate(v[r * cols:(r + 1) * cols], rot)]


class Rings:
    """ringQ with the plaintext ring (be.Params) and the moduli of P with their sub-ring constants"""

    def __init__(self, N, Q, P, t):
        self.N, self.Q, self.P, self.t = int(N), [int(q) for q in Q], [int(p) for p in P], int(t)
        self.enc = be.Params(self.N, self.Q, self.t)
        self.srP = [orc.SubRingConsts(self.N, p) for p in self.P]
        self.n, self.cols = self.enc.n, self.enc.n >> 1
        self.log_cols = self.cols.bit_length() - 1


def _values(v, t):
    a = np.asarray(v)
    return a if a.dtype in (np.uint64, np.int64) else np.array([int(x) % t for x in v], dtype=np.uint64)


def embed_qp(R, levelQ, levelP, values, scale):
    """Embed into a ringqp.Poly (schemes/bgv/encoder.go:252-320, the ringqp.Poly arm :292-311): NTT domain, Montgomery form, no scale-up"""
    v = _values(values, R.t)
    return (be.embed(R.enc, levelQ, v, scale, False, True, True),
            be.embed(R.enc, levelP, v, scale, False, True, True, mods=R.P, srs=R.srP))


def embed_rows(R, levelQ, levelP, values, rots, scale):
    """what rh_bgv_embed_qp is defined by: per vector, the host rotation of each row, then Embed into Q and into P -> [(Q rows, P rows)]"""
    return [embed_qp(R, levelQ, levelP, v if rots is None else _values(rotate_rows(list(v), rots[k], R.cols), R.t), scale) for k, v in enumerate(values)]


def encode(R, diags, index_list, levelQ, levelP, scale, log_ratio):
    """NewLinearTransformation (:148-201) with DiagonalsIndexList = index_list, then Encode (:205-292) of diags with rows = 2"""
    cols = R.cols
    if log_ratio < 0:                                                    # (:162-170)
        n1 = 0
        allocated = {i + cols if i < 0 else i for i in index_list}
    else:                                                                # (:171-178)
        n1 = find_best_bsgs_ratio(index_list, cols, log_ratio)
        index, _, _ = bsgs_index(index_list, cols, n1)
        allocated = {j + i for j in index for i in index[j]}
    vec = {}
    if n1 == 0:                                                          # (:221-241)
        for i in diags:
            idx = i + cols if i < 0 else i
            if idx not in allocated:
                raise KeyError("cannot Encode: error encoding on LinearTransformation: plaintext diagonal [%d] does not exist" % idx)
            vec[idx] = embed_qp(R, levelQ, levelP, diagonals_at(diags, i, cols), scale)
    else:                                                                # (:242-266)
        index, _, _ = bsgs_index(sorted(allocated), cols, n1)
        for j in index:
            rot = -j & (cols - 1)
            for i in index[j]:
                vec[i + j] = embed_qp(R, levelQ, levelP, rotate_rows(diagonals_at(diags, i + j, cols), rot, cols), scale)
    return Transformation(n1, levelQ, levelP, vec, int(scale), R.log_cols, log_ratio)


# ---- lintrans_evaluator.go on BGV ciphertexts ------------------------------------------------------------------------------------------------
def evaluate(R, ct, scale, lt, keys):
    """Evaluate -> (ciphertext, scale): opOut.Scale = ctIn.Scale * lt.Scale (lintrans_evaluator.go:137, :264) modulo T"""
    return evaluate_many(R.N, R.Q, R.P, ct, [lt], keys)[0], int(scale) * int(lt.Scale) % R.t


def evaluate_sequential(R, ct, scale, lts, keys):
    """EvaluateSequential (:102-124) -> (ciphertext, scale): bgv.Evaluator.Rescale (schemes/bgv/evaluator.go:1415-1445) after every transformation"""
    for lt in lts:
        ct, scale = evaluate(R, ct, scale, lt, keys)
        ct, scale = br.rescale(R.N, R.Q[:ct[0].shape[0]], R.t, ct, scale)
    return ct, scale


# ---- encryption, decryption to slots, the noise ------------------------------------------------------------------------------------------------
def encrypt(rnd, R, sk, values, level, scale=1):
    """bgv.Encoder.Encode at `scale`, then Encryptor.Encrypt under sk"""
    mods = R.Q[:level + 1]
    pt = be.encode(R.enc, level, _values(values, R.t), scale)
    ct, _ = rr.encrypt(rnd, sk, [0] * R.N, R.Q, level)
    return [rr._add(ct[0], pt, mods), ct[1]]


def decrypt_slots(R, ct, sk, scale):
    """-> (the decoded slots, log2 of the infinity norm of the noise, log2(Q_level / (2T))): T * phase = M + T e with M centred modulo T"""
    level = ct[0].shape[0] - 1
    mods = R.Q[:level + 1]
    ph = rr._vec("ADD", rr._vec("MUL_MONT", np.asarray(ct[1], dtype=np.uint64), sk.rows(mods), mods), np.asarray(ct[0], dtype=np.uint64), mods)
    vals = be.decode(R.enc, level, ph, scale)
    Qb, t = be.prod(mods), R.t
    worst = 0
    for x in rr.phase(ct, sk, R.Q):
        v = t * x % Qb
        v = v - Qb if 2 * v > Qb else v
        m = v % t
        m = m - t if 2 * m > t else m
        worst = max(worst, abs((v - m) // t))
    return [int(v) for v in vals], math.log2(max(worst, 1)), math.log2(Qb) - 1 - math.log2(t)

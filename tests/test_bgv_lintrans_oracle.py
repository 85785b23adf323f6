"""tests/bgv_lintrans_restatement.py pinned to ground truth, and the host side of matrix-fhe-lattigo_amd/bgv_lintrans.py with it: the index
arithmetic of the two-row shapes, Diagonals.Evaluate against a dense 2-block matrix-vector product modulo T, Permutation.GetDiagonals against
the definition, Encode against decoding, and whole evaluations against decryption under a real key (encrypt, Evaluate with BSGS and naive,
decrypt, decode: Diagonals.Evaluate slot by slot modulo T, exactly).  It also holds the condition under which tests/test_gpu_bgv_lintrans.py
is meaningful: for every shape used there the restatement decrypts exactly with the noise at least MARGIN_BITS below Q_level / (2T).  CPU only."""
import functools
import random

import numpy as np
import pytest

import bgv_encoder_restatement as be
import bgv_lintrans_restatement as blr
import rlwe_restatement as rr
from oracle import primes
from oracle import ring_oracle as orc

MARGIN_BITS = 10                                                         # a safety margin on the choice of inputs, not a measurement

SMALL_DIAGS = [-5, -1, 0, 1, 2, 3, 7]
GAP_DIAGS = [-3, -1, 0, 1, 2]                                            # distinct modulo 8
REF_DIAGS = [-15, -4, -1, 0, 1, 2, 3, 4, 15]                             # the reference's (circuits/bgv/lintrans/lintrans_test.go)
# name -> (logN, logQ, logP, T, diagonals).  Two P moduli everywhere: the hoisted products of the device path take no single-modulus P.
SHAPES = {
    "TAIL": (5, (61, 61, 61), (61, 61), 65537, SMALL_DIAGS),             # n = 32, cols 16, no gap: a row inside one wavefront
    "GAP2": (5, (61, 61, 61), (61, 61), 97, GAP_DIAGS),                  # n = 16, cols 8, gap 2: the strided lift
    "N10": (10, (55, 45, 45), (61, 61), 65537, REF_DIAGS),               # rescale in EvaluateSequential, transformations below the ciphertext's level
    "N13G4": (13, (61, 61), (61, 61), 12289, REF_DIAGS),                 # n = 2048, gap 4: several blocks per row, the gap across the 4096-coefficient tile
}


@functools.lru_cache(maxsize=None)
def rings(name):
    logN, logQ, logP, t, _ = SHAPES[name]
    Q, P = primes.gen_moduli(logN + 1, list(logQ), list(logP))
    return blr.Rings(1 << logN, Q, P, t)


@functools.lru_cache(maxsize=None)
def diagonals(name, tag=""):
    """both rows of every diagonal filled with values modulo T (the reference's own test leaves the second row zero)"""
    R = rings(name)
    rnd = random.Random("bgv lintrans diagonals %s %s" % (name, tag))
    return {k: [rnd.randrange(R.t) for _ in range(R.n)] for k in SHAPES[name][4]}


def message(name, k):
    R = rings(name)
    rnd = random.Random("bgv lintrans message %s %d" % (name, k))
    return [rnd.randrange(R.t) for _ in range(R.n)]


class Keyed:
    """a secret key and Galois keys from the restated key layer, made on demand"""
    _cache = {}

    def __new__(cls, name):
        if name not in cls._cache:
            self = object.__new__(cls)
            self.R = rings(name)
            self.rnd = random.Random("bgv lintrans keys " + name)
            self.sk = rr.Secret.sample(self.rnd, self.R.N)
            self.keys = {}
            cls._cache[name] = self
        return cls._cache[name]

    def galois(self, galEls):
        R = self.R
        for g in galEls:
            if g != 1 and g not in self.keys:
                self.keys[g] = rr.galois_key(self.rnd, self.sk, g, R.Q, R.P, len(R.Q) - 1, len(R.P) - 1)
        return self.keys


def check_margin(what, noise, room):
    print("MEASURED bgv/lintrans %s  noise 2^%.2f  log2(Q_level / 2T) %.2f  margin %.2f bits  [>= %d]" % (what, noise, room, room - noise, MARGIN_BITS))
    assert room - noise >= MARGIN_BITS


# ---- index arithmetic ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_index_arithmetic_of_the_two_row_shapes(rh, name):
    """the rotations act on rows of cols = n / 2 slots: the package's Galois elements and the keys of Vec against the restatement, and every
    rotation below cols"""
    R = rings(name)
    bl = rh.bgv_lintrans
    diags = SHAPES[name][4]
    assert (R.n, R.cols) == {"TAIL": (32, 16), "GAP2": (16, 8), "N10": (1024, 512), "N13G4": (2048, 1024)}[name]
    for ratio in (1, 0, -1):
        params = bl.Parameters(diags, len(R.Q) - 1, len(R.P) - 1, 1, (1, R.log_cols), ratio)
        got = sorted(params.GaloisElements(R.N))
        assert got == blr.galois_elements(R.N, diags, R.cols, ratio)
        N1, keys = rh.lintrans._vec_keys(diags, R.cols, ratio)
        want = blr.find_best_bsgs_ratio(diags, R.cols, ratio) if ratio >= 0 else 0
        assert N1 == want and sorted(keys) == sorted({d & (R.cols - 1) for d in diags})
        g5 = [pow(5, r, 2 * R.N) for r in range(R.cols)]
        assert all(g in g5 for g in got)                                 # column rotations only, each by less than cols
    with pytest.raises(rh.RingHipError, match=r"LogDimensions of a BGV linear transformation is \(Rows, Cols\)"):
        bl.Parameters(diags, 0, 0, 1, R.log_cols)
    with pytest.raises(rh.RingHipError, match="has two rows"):
        bl.Parameters(diags, 0, 0, 1, (0, R.log_cols))


# ---- Diagonals.Evaluate, Permutation.GetDiagonals ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["TAIL", "GAP2", "N10"])
def test_diagonals_evaluate_is_the_dense_product_on_each_row(rh, name):
    R = rings(name)
    diags = diagonals(name)
    v = message(name, 0)
    want = blr.dense_apply(diags, v, R.t)
    assert blr.diagonals_evaluate(diags, v, R.t) == want
    pk = rh.bgv_lintrans.Diagonals(diags)
    assert pk.Evaluate(v, t=R.t) == want
    assert [x % R.t for x in pk.Evaluate(v)] == want                     # exact integers without t
    seen = []

    def muladd(a, b, c):                                                 # the reference's callbacks write into c
        seen.append(len(a))
        c[:] = [(z + x * y) % R.t for x, y, z in zip(a, b, c)]

    def add(a, b, c):
        c[:] = [(x + y) % R.t for x, y in zip(a, b)]
    assert pk.Evaluate(v, lambda size: [0] * size, add, muladd) == want
    assert set(seen) == {R.cols}                                         # each half on its own
    assert sorted(pk.DiagonalsIndexList()) == sorted(diags)
    assert pk.At(R.cols - 1, R.cols) == diags[-1]                        # a missing positive index falls back to i - slots
    with pytest.raises(rh.RingHipError, match=r"cannot At\[0\]"):
        rh.bgv_lintrans.Diagonals({1: diags[1]}).At(-2, R.cols)


def test_rows_rotate_independently():
    """the diagonal 1 of all ones is RotateColumns by 1: each row moves on its own and nothing crosses between them"""
    R = rings("GAP2")
    v = list(range(1, R.n + 1))
    out = blr.diagonals_evaluate({1: [1] * R.n}, v, R.t)
    assert out == blr.rotate(v[:R.cols], 1) + blr.rotate(v[R.cols:], 1)
    assert blr.rotate_rows(v, 3, R.cols) == blr.rotate(v[:R.cols], 3) + blr.rotate(v[R.cols:], 3)
    assert blr.rotate_rows(v, -1, R.cols) == blr.rotate_rows(v, R.cols - 1, R.cols) and blr.rotate_rows(v, R.cols, R.cols) == v


def shuffled_permutation(name, keep):
    """the reference's permutation test (lintrans_test.go): a shuffled map per row, truncated to `keep` entries, random scalings modulo T"""
    R = rings(name)
    rnd = random.Random("bgv lintrans permutation " + name)
    rows = []
    for _ in (0, 1):
        to = list(range(R.cols))
        rnd.shuffle(to)
        rows.append([(frm, to[frm], rnd.randrange(1, R.t)) for frm in range(R.cols)][:keep])
    return rows


@pytest.mark.parametrize("keep", [16, 11])
def test_permutation_diagonals_against_the_definition(rh, keep):
    """out[row][To] = Scaling * in[row][From] for every mapping, zero elsewhere; a different (partial, when keep < cols) map per row"""
    R = rings("TAIL")
    rows = shuffled_permutation("TAIL", keep)
    assert rows[0] != rows[1]
    diags = blr.permutation_diagonals(rows, R.log_cols + 1)
    bl = rh.bgv_lintrans
    pk = bl.Permutation([[bl.PermutationMapping(*m) for m in row] for row in rows]).GetDiagonals(R.log_cols + 1)
    assert dict(pk) == diags and all(len(d) == R.n for d in diags.values())
    v = message("TAIL", 1)
    want = [0] * R.n
    for r, row in enumerate(rows):
        for frm, to, s in row:
            want[r * R.cols + to] = s * v[r * R.cols + frm] % R.t
    assert blr.diagonals_evaluate(diags, v, R.t) == want == blr.dense_apply(diags, v, R.t)
    with pytest.raises(rh.RingHipError, match="a pair of lists"):
        bl.Permutation([[], [], []])


# ---- Encode ------------------------------------------------------------------------------------------------------------------------------------------------
def decode_rows(R, rows, mods, srs, scale):
    """a poly in the NTT domain and Montgomery form, not scaled up, back to its slots: every limb holds the residues modulo T themselves"""
    out = []
    for i, q in enumerate(mods):
        plain = np.array([int(x) * pow(1 << 64, -1, q) % q for x in rows[i]], dtype=np.uint64)
        co = orc.intt(plain, srs[i])
        assert not np.any(np.delete(co, np.arange(0, R.N, R.enc.gap)))    # zero off the stride
        out.append([int(x) for x in be.decode_ring_t(R.enc, co[::R.enc.gap], scale)])
    assert all(o == out[0] for o in out)
    return out[0]


@pytest.mark.parametrize("ratio", [1, -1], ids=["bsgs", "naive"])
@pytest.mark.parametrize("name", ["TAIL", "GAP2"])
def test_encode_decodes_back_to_the_rotated_rows(name, ratio):
    R = rings(name)
    diags = diagonals(name)
    levelQ, levelP, scale = len(R.Q) - 2, len(R.P) - 1, 3
    lt = blr.encode(R, diags, list(diags), levelQ, levelP, scale, ratio)
    assert (lt.N1 == 0) == (ratio < 0) and sorted(lt.Vec) == sorted(k & (R.cols - 1) for k in diags)
    index = lt.bsgs_index()[0] if lt.N1 else {0: sorted(lt.Vec)}
    rotated = 0
    for j in index:
        for i in index[j]:
            k = i + j
            rot = (-j & (R.cols - 1)) if lt.N1 else 0
            want = blr.rotate_rows(diags[k] if k in diags else diags[k - R.cols], rot, R.cols)
            rotated += rot != 0
            q, p = lt.Vec[k]
            assert q.shape == (levelQ + 1, R.N) and p.shape == (levelP + 1, R.N)
            assert decode_rows(R, q, R.Q[:levelQ + 1], R.enc.srQ, scale) == want, k
            assert decode_rows(R, p, R.P[:levelP + 1], R.srP, scale) == want, k
    assert (rotated > 0) == (ratio >= 0)


def test_embed_rows_is_the_host_rotation_then_embed():
    R = rings("GAP2")
    v = np.array([message("GAP2", k) for k in range(3)], dtype=np.uint64)
    got = blr.embed_rows(R, 1, 1, v, [0, 1, R.cols - 1], 5)
    for k, rot in enumerate([0, 1, R.cols - 1]):
        assert decode_rows(R, got[k][0], R.Q[:2], R.enc.srQ, 5) == blr.rotate_rows([int(x) for x in v[k]], rot, R.cols)
    plain = blr.embed_rows(R, 1, 1, v, None, 5)
    assert np.array_equal(plain[0][0], got[0][0]) and not np.array_equal(plain[1][0], got[1][0])


# ---- end to end on the restatement: the condition on the inputs --------------------------------------------------------------------------------------------
EVAL = [("TAIL", 1), ("TAIL", -1), ("GAP2", 1), ("GAP2", -1), ("N10", 1), ("N10", -1), ("N13G4", 1)]


@pytest.mark.parametrize("name,ratio", EVAL, ids=["%s-%s" % (n, "bsgs" if r >= 0 else "naive") for n, r in EVAL])
def test_evaluate_decrypts_exactly_with_margin(name, ratio):
    R = rings(name)
    k = Keyed(name)
    diags = diagonals(name)
    top = len(R.Q) - 1
    keys = k.galois(blr.galois_elements(R.N, list(diags), R.cols, ratio))
    lt_scale, ct_scale = (3, 7) if ratio >= 0 else (R.t - 1, 1)
    lt = blr.encode(R, diags, list(diags), top, len(R.P) - 1, lt_scale, ratio)
    v = message(name, 0)
    ct = blr.encrypt(k.rnd, R, k.sk, v, top, ct_scale)
    out, scale = blr.evaluate(R, ct, ct_scale, lt, keys)
    assert scale == ct_scale * lt_scale % R.t and out[0].shape == (top + 1, R.N)
    slots, noise, room = blr.decrypt_slots(R, out, k.sk, scale)
    check_margin("%s ratio=%d level=%d" % (name, ratio, top), noise, room)
    assert slots == blr.diagonals_evaluate(diags, v, R.t)


@pytest.mark.parametrize("ratio", [1, -1], ids=["bsgs", "naive"])
def test_evaluate_below_the_ciphertext_level_and_sequential_decrypt_exactly_with_margin(ratio):
    """N10: a transformation one level below the ciphertext, and EvaluateSequential of two transformations -- the level drops by BGV's rescale
    each time, the scale is divided by the prime consumed modulo T"""
    name = "N10"
    R = rings(name)
    k = Keyed(name)
    da, db = diagonals(name), diagonals(name, "second")
    top = len(R.Q) - 1
    keys = k.galois(blr.galois_elements(R.N, list(da), R.cols, ratio))
    v = message(name, 1)
    ct = blr.encrypt(k.rnd, R, k.sk, v, top, 1)
    low = blr.encode(R, da, list(da), top - 1, len(R.P) - 1, 1, ratio)
    out, scale = blr.evaluate(R, ct, 1, low, keys)
    assert out[0].shape[0] == top
    slots, noise, room = blr.decrypt_slots(R, out, k.sk, scale)
    check_margin("%s below ratio=%d level=%d" % (name, ratio, top - 1), noise, room)
    assert slots == blr.diagonals_evaluate(da, v, R.t)
    lts = [blr.encode(R, da, list(da), top, len(R.P) - 1, 3, ratio), blr.encode(R, db, list(db), top - 1, len(R.P) - 1, R.t - 1, ratio)]
    out, scale = blr.evaluate_sequential(R, ct, 1, lts, keys)
    assert out[0].shape[0] == top - 1
    want_scale = 3 * pow(R.Q[top] % R.t, -1, R.t) % R.t * (R.t - 1) % R.t * pow(R.Q[top - 1] % R.t, -1, R.t) % R.t
    assert scale == want_scale
    slots, noise, room = blr.decrypt_slots(R, out, k.sk, scale)
    check_margin("%s sequential ratio=%d level=%d" % (name, ratio, top - 2), noise, room)
    assert slots == blr.diagonals_evaluate(db, blr.diagonals_evaluate(da, v, R.t), R.t)


def test_permutation_decrypts_exactly_with_margin():
    """the reference's permutation test at TAIL: a shuffled, truncated map per row through GetDiagonals, evaluated (BSGS ratio 1 as there)"""
    name = "TAIL"
    R = rings(name)
    k = Keyed(name)
    rows = shuffled_permutation(name, 11)
    diags = blr.permutation_diagonals(rows, R.log_cols + 1)
    top = len(R.Q) - 1
    keys = k.galois(blr.galois_elements(R.N, list(diags), R.cols, 1))
    lt = blr.encode(R, diags, list(diags), top, len(R.P) - 1, 1, 1)
    v = message(name, 2)
    out, scale = blr.evaluate(R, blr.encrypt(k.rnd, R, k.sk, v, top, 1), 1, lt, keys)
    slots, noise, room = blr.decrypt_slots(R, out, k.sk, scale)
    check_margin("%s permutation" % name, noise, room)
    want = [0] * R.n
    for r, row in enumerate(rows):
        for frm, to, s in row:
            want[r * R.cols + to] = s * v[r * R.cols + frm] % R.t
    assert slots == want

"""GPU: BGV linear transformations on the device (matrix-fhe-lattigo_amd/bgv_lintrans.py) and the one-pass encoding of a transformation
(csrc/bgv_encoder.hip: rh_bgv_embed_qp) bit for bit, whole outputs, against tests/bgv_lintrans_restatement.py, which
tests/test_bgv_lintrans_oracle.py pins to Python integers and to decryption -- fused and composed, under both cache policies, and by
decrypting the device output.  Batches of 2 ciphertexts with different messages under keys generated on the device from a KeyedPRNG; the
oracle file checks for each shape that the restatement decrypts exactly with 10 bits of noise margin, which is what makes the exact
comparison of decrypted slots here meaningful.  Shapes: tests/test_bgv_lintrans_oracle.py SHAPES."""
import ctypes as C
import functools
import types

import numpy as np
import pytest

import bgv_lintrans_restatement as blr
import rlwe_restatement as rr
from oracle import primes
from test_bgv_lintrans_oracle import SHAPES, diagonals, message, rings, shuffled_permutation
from test_gpu_cache_policy import policy

pytestmark = pytest.mark.gpu
B = 2
I64 = np.iinfo(np.int64)


class Dev:
    """the rings of a shape, a secret key and Galois keys from the device KeyGenerator (also as the restatement takes them), the encoder,
    the evaluator and its lintrans evaluator"""
    _cache = {}

    def __new__(cls, rh, name):
        if name not in cls._cache:
            self = object.__new__(cls)
            self.rh, self.name = rh, name
            self.R = R = rings(name)
            self.rq, self.rp = rh.Ring(R.N, R.Q), rh.Ring(R.N, R.P)
            self.prng = rh.rlwe.KeyedPRNG(b"bgv lintrans " + name.encode())
            self.kg = rh.rlwe.KeyGenerator(self.rq, self.rp, prng=self.prng)
            self.sk = self.kg.GenSecretKeyNew()
            self.enc = rh.bgv.Encoder(self.rq, R.t, ringP=self.rp)
            self.ev = rh.bgv.Evaluator(self.rq, None, R.t, ringP=self.rp, encoder=self.enc)
            self.lev = rh.bgv_lintrans.Evaluator(self.ev)
            self.encryptor, self.decryptor = rh.bgv.Encryptor(self.rq, None, self.sk, prng=self.prng), rh.bgv.Decryptor(self.rq, self.sk)
            self.host_keys, self.cts = {}, {}
            cls._cache[name] = self
        return cls._cache[name]

    def galois(self, galEls):
        """the keys of galEls on the evaluator; -> {Galois element: rr.GadgetKey} for the restatement"""
        new = [g for g in galEls if g != 1 and g not in self.host_keys]
        for g, gk in zip(new, self.kg.GenGaloisKeysNew(new, self.sk)):
            self.ev.galois_keys[g] = gk
            q = gk.Q.numpy().reshape(gk.digits, 2, gk.Q.limbs, -1)
            p = gk.P.numpy().reshape(gk.digits, 2, gk.P.limbs, -1)
            self.host_keys[g] = rr.GadgetKey(q, p, len(self.R.Q) - 1, len(self.R.P) - 1, 0, None)
        return self.host_keys

    def encrypt(self, level=None, scale=1):
        """-> (messages (B, n), the device ciphertext, per ciphertext its [c0, c1] on the host); one per (level, scale), shared"""
        R = self.R
        level = len(R.Q) - 1 if level is None else level
        if (level, scale) not in self.cts:
            values = np.array([message(self.name, k) for k in range(B)], dtype=np.uint64)
            pt = self.enc.NewPlaintext(level, scale=scale, nvec=B)
            self.enc.Encode(values, pt)
            ct = self.encryptor.EncryptNew(pt)
            host = [v.numpy() for v in ct.Value]
            self.cts[(level, scale)] = (values, host)
        values, host = self.cts[(level, scale)]
        return values, self.ct(host, scale), [[host[0][p], host[1][p]] for p in range(B)]

    def ct(self, host, scale):
        """a fresh device copy: Evaluate(ct, lt, ct) overwrites its input"""
        rh = self.rh
        level = host[0].shape[1] - 1
        ct = rh.Ciphertext([rh.DevicePoly.from_numpy(self.rq.AtLevel(level), h) for h in host], is_ntt=True)
        ct.Scale, ct.IsBatched = scale, True
        return ct

    def new(self, rh, level, fill=None):
        rl = self.rq.AtLevel(level)
        if fill is None:
            return rh.Ciphertext([rl.NewPoly(B) for _ in (0, 1)], is_ntt=True)
        return rh.Ciphertext([rh.DevicePoly.from_numpy(rl, np.full((B, level + 1, self.R.N), fill, dtype=np.uint64)) for _ in (0, 1)], is_ntt=True)

    def decode(self, out):
        return np.asarray(self.enc.Decode(self.decryptor.DecryptNew(out)))


def same(out, wants):
    """every word of both components of every ciphertext of the batch"""
    assert out.Degree() == 1 and out.Value[0].limbs == wants[0][0].shape[0]
    for c, v in enumerate(out.Value):
        got = v.numpy()
        for p, w in enumerate(wants):
            assert np.array_equal(got[p], w[c]), "component %d of ciphertext %d" % (c, p)


def transformation(rh, d, diags, level, ratio, scale, fused=None):
    """(the package transformation through NewLinearTransformation + Encode, the restated one)"""
    R, bl = d.R, rh.bgv_lintrans
    params = bl.Parameters(list(diags), level, len(R.P) - 1, scale, d.enc.LogMaxDimensions(), ratio)
    lt = bl.NewLinearTransformation(d.rq, d.rp, params)
    bl.Encode(d.enc, bl.Diagonals(diags), lt, fused=fused)
    return lt, blr.encode(R, diags, list(diags), level, len(R.P) - 1, scale, ratio)


def same_vec(lt, want):
    assert sorted(lt.Vec) == sorted(want.Vec) and lt.N1 == want.N1
    for k in want.Vec:
        assert np.array_equal(lt.Vec[k].Q.numpy()[0], want.Vec[k][0]) and np.array_equal(lt.Vec[k].P.numpy()[0], want.Vec[k][1]), k


# ---- rh_bgv_embed_qp -----------------------------------------------------------------------------------------------------------------------------------
def edge_block(R, signed):
    """three vectors: the edge values of tests/test_gpu_bgv_encoder.py first (0, T - 1, 2^64 - 1 as uint64; int64 min and max; T >> 1 on either
    side), spread over both rows, the rest uniform"""
    rng = np.random.default_rng(R.N + R.t + signed)
    h = R.t >> 1
    if signed:
        v = rng.integers(-R.t, R.t, (3, R.n), dtype=np.int64)
        edge = [I64.min, I64.max, 0, -1, h, h - 1, h + 1, -h, -h - 1, -R.t, R.t, -2 * R.t]
    else:
        v = rng.integers(0, R.t, (3, R.n), dtype=np.uint64)
        edge = [0, R.t - 1, (1 << 64) - 1, h, h - 1, h + 1, R.t, 2 * R.t]
    half = len(edge) // 2
    v[0, :half] = np.array(edge[:half], dtype=v.dtype)
    v[0, R.n - (len(edge) - half):] = np.array(edge[half:], dtype=v.dtype)
    return v


@functools.lru_cache(maxsize=None)
def embed_case(name, signed):
    """the block, the rotations (0, 1, cols - 1: a different one per vector) and the restated outputs with and without them, one level below
    the top of Q; computed once, shared by the variants"""
    R = rings(name)
    v = edge_block(R, signed)
    rots = [0, 1, R.cols - 1]
    levelQ, levelP = len(R.Q) - 2, len(R.P) - 1
    v.setflags(write=False)
    return v, rots, levelQ, levelP, blr.embed_rows(R, levelQ, levelP, v, rots, 3), blr.embed_rows(R, levelQ, levelP, v, None, 3)


@pytest.mark.parametrize("nt", [0, 2], ids=["nt-never", "nt-always"])
@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "composed"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_embed_qp_whole_outputs(rh, name, fused, nt):
    d = Dev(rh, name)
    R = d.R
    meta = types.SimpleNamespace(Scale=3, IsNTT=True, IsMontgomery=True)
    d.enc.set_tuning("fused", fused)
    try:
        with policy(nt, d.rq, d.rp, d.enc.ringT):
            for signed in (False, True):
                v, rots, levelQ, levelP, want_rot, want_plain = embed_case(name, signed)
                qp = rh.rlwe.PolyQP(d.rq.AtLevel(levelQ).NewPoly(3), d.rp.AtLevel(levelP).NewPoly(3))
                dv = rh.bgv.DeviceValues.from_numpy(d.rq, v)
                for r, want in ((rots, want_rot), (None, want_plain), ([R.cols, R.cols + 1, -1], want_rot)):      # reduced modulo cols
                    d.enc.EmbedRows(dv, r, R.cols, meta, qp)
                    gq, gp = qp.Q.numpy(), qp.P.numpy()
                    for k in range(3):
                        assert np.array_equal(gq[k], want[k][0]) and np.array_equal(gp[k], want[k][1]), (signed, r, k)
                assert np.array_equal(dv.numpy(), v)                     # the values are read only
                assert np.array_equal(want_rot[0][0], want_plain[0][0]) and not np.array_equal(want_rot[1][0], want_plain[1][0])
                assert not np.array_equal(want_rot[2][1], want_plain[2][1])
    finally:
        d.enc.set_tuning("fused", -1)


@pytest.mark.parametrize("fused", [1, 0], ids=["fused", "composed"])
def test_embed_qp_short_vectors_and_plain_metadata(rh, fused):
    """without rotations: fewer values than slots (zero past nvals), and the coefficient-domain, non-Montgomery words Embed leaves"""
    d = Dev(rh, "GAP2")
    R = d.R
    v = edge_block(R, False)[:, :R.n - 3]
    d.enc.set_tuning("fused", fused)
    try:
        for ntt, mont in ((True, True), (False, False), (True, False), (False, True)):
            meta = types.SimpleNamespace(Scale=5, IsNTT=ntt, IsMontgomery=mont)
            qp = rh.rlwe.PolyQP(d.rq.NewPoly(3), d.rp.NewPoly(3))
            d.enc.EmbedRows(v, None, R.cols, meta, qp)
            for k in range(3):
                assert np.array_equal(qp.Q.numpy()[k], blr.be.embed(R.enc, len(R.Q) - 1, v[k], 5, False, ntt, mont)), (ntt, mont, k)
                assert np.array_equal(qp.P.numpy()[k], blr.be.embed(R.enc, len(R.P) - 1, v[k], 5, False, ntt, mont, mods=R.P, srs=R.srP)), (ntt, mont, k)
    finally:
        d.enc.set_tuning("fused", -1)


# ---- Encode, NewTransformationFromBlock ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [1, -1], ids=["bsgs", "naive"])
@pytest.mark.parametrize("name", ["TAIL", "GAP2", "N10"])
def test_encode_and_the_block_form_give_the_restated_words(rh, name, ratio):
    d = Dev(rh, name)
    R, bl = d.R, rh.bgv_lintrans
    diags = diagonals(name)
    level = len(R.Q) - 2
    want = None
    for fused in (True, False):
        lt, want = transformation(rh, d, diags, level, ratio, 3, fused=fused)
        same_vec(lt, want)
        assert lt.IsNTT and lt.IsMontgomery and lt.IsBatched and lt.Scale == 3 and lt.LogDimensions == (1, R.log_cols)
        assert (lt.LevelQ, lt.LevelP) == (level, len(R.P) - 1) and (lt.N1 == 0) == (ratio < 0)
        assert sorted(lt.GaloisElements(R.N)) == blr.galois_elements(R.N, list(diags), R.cols, ratio)
        index = [k & (R.cols - 1) for k in diags]
        params = bl.Parameters(list(diags), level, len(R.P) - 1, 3, (1, R.log_cols), ratio)
        rows = np.array([diags[k] for k in diags], dtype=np.uint64)
        for block in (rows, rh.bgv.DeviceValues.from_numpy(d.rq, rows), rows.astype(np.int64)):
            blk = bl.NewTransformationFromBlock(d.rq, d.rp, params, d.enc, index, block, fused=fused)
            same_vec(blk, want)
            assert blk.Block.Q.npoly == len(index) and blk.Vec[index[1]].Q.ptr == blk.Block.Q.ptr + (level + 1) * R.N * 8
    partial = bl.NewLinearTransformation(d.rq, d.rp, bl.Parameters(list(diags), level, len(R.P) - 1, 3, (1, R.log_cols), ratio))
    if ratio < 0:                                                        # the naive form encodes the diagonals it is given (:221-241)
        some = {k: diags[k] for k in list(diags)[:2]}
        for fused in (True, False):
            bl.Encode(d.enc, bl.Diagonals(some), partial, fused=fused)
            for k in some:
                assert np.array_equal(partial.Vec[k & (R.cols - 1)].Q.numpy()[0], want.Vec[k & (R.cols - 1)][0])
    with pytest.raises(rh.RingHipError, match=r"cannot Encode: (error encoding on LinearTransformation: plaintext diagonal \[6\] does not exist|cannot At)"):
        bl.Encode(d.enc, bl.Diagonals({6: diags[0]}), partial)                # a diagonal that was not allocated (naive), diagonals that are missing (BSGS)
    with pytest.raises(rh.RingHipError, match="holds 2 \\* cols"):
        bl.Encode(d.enc, bl.Diagonals({k: v[:R.cols] for k, v in diags.items()}), partial)


# ---- Evaluate ------------------------------------------------------------------------------------------------------------------------------------------------
def expected_slots(diags, values, t):
    return np.array([blr.diagonals_evaluate(diags, [int(x) for x in v], t) for v in values], dtype=np.uint64)


EVAL = [(n, r) for n in ("TAIL", "GAP2", "N10") for r in (1, -1)]


@pytest.mark.parametrize("name,ratio", EVAL, ids=["%s-%s" % (n, "bsgs" if r >= 0 else "naive") for n, r in EVAL])
def test_evaluate(rh, name, ratio):
    """fused and composed, every word against the restatement; the scale ctIn.Scale * lt.Scale mod T for lt.Scale 1, 3 and T - 1; the decrypted
    slots equal Diagonals.Evaluate in both rows; opOut = ctIn; ctIn left alone"""
    d = Dev(rh, name)
    R = d.R
    diags = diagonals(name)
    top = len(R.Q) - 1
    hk = d.galois(blr.galois_elements(R.N, list(diags), R.cols, ratio))
    values, _, host = d.encrypt(top, 7)
    slots = expected_slots(diags, values, R.t)
    assert np.array_equal(np.asarray(rh.bgv_lintrans.Diagonals(diags).Evaluate([int(x) for x in values[1]], t=R.t), dtype=np.uint64), slots[1])
    for lt_scale in (1, 3, R.t - 1):
        lt, rlt = transformation(rh, d, diags, top, ratio, lt_scale)
        wants = [blr.evaluate(R, h, 7, rlt, hk)[0] for h in host]
        for fused in (True, False):
            _, ct, _ = d.encrypt(top, 7)
            out = d.new(rh, top)
            d.lev.Evaluate(ct, lt, out, fused=fused)
            same(out, wants)
            assert out.Scale == 7 * lt_scale % R.t and out.IsNTT and out.IsBatched
            same(ct, host)                                               # ctIn is left alone
            assert np.array_equal(d.decode(out), slots), (lt_scale, fused)
            d.lev.Evaluate(ct, lt, ct, fused=fused)                      # opOut = ctIn
            same(ct, wants)
            assert ct.Scale == 7 * lt_scale % R.t
    new = d.lev.EvaluateNew(d.encrypt(top, 7)[1], lt)
    same(new, wants)
    assert new.Level() == top


def test_evaluate_many_shares_the_pre_rotations(rh):
    """N10, two BSGS transformations one level below the ciphertext: one decomposition, the baby steps of the second reused from the first;
    the outputs are those of two single calls and of the restatement"""
    name = "N10"
    d = Dev(rh, name)
    R = d.R
    da, db = diagonals(name), diagonals(name, "second")
    top = len(R.Q) - 1
    hk = d.galois(blr.galois_elements(R.N, list(da), R.cols, 1))
    values, _, host = d.encrypt(top, 1)
    (lta, rlta), (ltb, rltb) = transformation(rh, d, da, top - 1, 1, 3), transformation(rh, d, db, top - 1, 1, 5)
    wants = [blr.evaluate_many(R.N, R.Q, R.P, h, [rlta, rltb], hk) for h in host]
    calls = []
    pre = d.lev.PreRotatedCiphertextForDiagonalMatrixMultiplication

    def spy(levelQ, levelP, ctIn, dec, rots, ctPreRot):
        before = set(ctPreRot)
        pre(levelQ, levelP, ctIn, dec, rots, ctPreRot)
        calls.append(sorted(set(ctPreRot) - before))
    d.lev.PreRotatedCiphertextForDiagonalMatrixMultiplication = spy
    try:
        for fused in (True, False):
            del calls[:]
            _, ct, _ = d.encrypt(top, 1)
            outs = d.lev.EvaluateManyNew(ct, [lta, ltb], fused=fused)
            assert len(calls) == 2 and calls[0] and calls[1] == []       # the second transformation computes no rotation of its own
            for i, (lt, diags, s) in enumerate(((lta, da, 3), (ltb, db, 5))):
                same(outs[i], [w[i] for w in wants])
                assert outs[i].Level() == top - 1 and outs[i].Scale == s and ct.Level() == top
                single = d.lev.EvaluateNew(ct, lt, fused=fused)
                same(single, [w[i] for w in wants])
                assert np.array_equal(d.decode(outs[i]), expected_slots(diags, values, R.t))
    finally:
        del d.lev.PreRotatedCiphertextForDiagonalMatrixMultiplication


@pytest.mark.parametrize("ratio", [1, -1], ids=["bsgs", "naive"])
def test_evaluate_sequential_rescales_as_bgv_does(rh, ratio):
    name = "N10"
    d = Dev(rh, name)
    R = d.R
    da, db = diagonals(name), diagonals(name, "second")
    top = len(R.Q) - 1
    hk = d.galois(blr.galois_elements(R.N, list(da), R.cols, ratio))
    values, _, host = d.encrypt(top, 1)
    (lta, rlta), (ltb, rltb) = transformation(rh, d, da, top, ratio, 3), transformation(rh, d, db, top - 1, ratio, R.t - 1)
    wants = [blr.evaluate_sequential(R, h, 1, [rlta, rltb], hk) for h in host]
    slots = expected_slots(db, expected_slots(da, values, R.t), R.t)
    for fused in (True, False):
        _, ct, _ = d.encrypt(top, 1)
        out = d.lev.EvaluateSequentialNew(ct, [lta, ltb], fused=fused)
        assert out.Level() == top - 2 and out.Scale == wants[0][1]
        same(out, [w[0] for w in wants])
        assert np.array_equal(d.decode(out), slots)
        same(ct, host)


def test_permutation_of_each_row(rh):
    """the reference's permutation test at TAIL: a shuffled, truncated map per row, random scalings modulo T, through GetDiagonals"""
    name = "TAIL"
    d = Dev(rh, name)
    R, bl = d.R, rh.bgv_lintrans
    rows = shuffled_permutation(name, 11)
    diags = bl.Permutation([[bl.PermutationMapping(*m) for m in row] for row in rows]).GetDiagonals(R.log_cols + 1)
    assert dict(diags) == blr.permutation_diagonals(rows, R.log_cols + 1)
    top = len(R.Q) - 1
    hk = d.galois(blr.galois_elements(R.N, list(diags), R.cols, 1))
    lt, rlt = transformation(rh, d, dict(diags), top, 1, 1)
    values, ct, host = d.encrypt(top, 1)
    out = d.lev.EvaluateNew(ct, lt)
    same(out, [blr.evaluate(R, h, 1, rlt, hk)[0] for h in host])
    want = np.zeros_like(values)
    for r, row in enumerate(rows):
        for frm, to, s in row:
            want[:, r * R.cols + to] = (s * values[:, r * R.cols + frm].astype(object)) % R.t
    assert np.array_equal(d.decode(out), want)


def test_evaluate_n13_gap4(rh):
    name = "N13G4"
    d = Dev(rh, name)
    R = d.R
    diags = diagonals(name)
    top = len(R.Q) - 1
    hk = d.galois(blr.galois_elements(R.N, list(diags), R.cols, 1))
    lt, rlt = transformation(rh, d, diags, top, 1, 3)
    values, ct, host = d.encrypt(top, 1)
    out = d.lev.EvaluateNew(ct, lt)
    same(out, [blr.evaluate(R, h, 1, rlt, hk)[0] for h in host])
    assert out.Scale == 3 and np.array_equal(d.decode(out), expected_slots(diags, values, R.t))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_evaluator(rh):
    name = "TAIL"
    d = Dev(rh, name)
    R, bl = d.R, rh.bgv_lintrans
    diags = diagonals(name)
    top = len(R.Q) - 1
    d.galois(blr.galois_elements(R.N, list(diags), R.cols, 1))
    lt, _ = transformation(rh, d, diags, top, 1, 1)
    _, ct, host = d.encrypt(top, 1)
    for ring in (rh.Ring(R.N, [int(q) for q in primes.gen_moduli(7, [55, 45], [])[0]], kind=rh.ConjugateInvariant),
                 rh.Ring(3 << 6, primes.gen_moduli_3n(3 << 6, [60, 60], [])[0], kind=rh.Matrix3N)):
        with pytest.raises(rh.RingHipError, match="conjugate-invariant and 3N rings are not supported"):
            bl.Evaluator(types.SimpleNamespace(ringQ=ring, ringP=None))
        ring.close()
    bare = rh.bgv.Evaluator(d.rq, None, R.t)
    with pytest.raises(rh.RingHipError, match="built without ringP"):
        bl.Evaluator(bare)
    bare.close()
    coeff = d.ct([h for h in d.cts[(top, 1)][1]], 1)
    coeff.IsNTT = False
    with pytest.raises(rh.RingHipError, match="coefficient-domain ciphertexts are not supported"):
        d.lev.Evaluate(coeff, lt, d.new(rh, top))
    three = rh.Ciphertext([d.rq.NewPoly(3) for _ in (0, 1)], is_ntt=True)
    with pytest.raises(rh.RingHipError, match="hold different numbers of ciphertexts"):
        d.lev.Evaluate(ct, lt, three)
    low = bl.NewLinearTransformation(d.rq, d.rp, bl.Parameters(list(diags), top, 0, 1, (1, R.log_cols), 1))
    with pytest.raises(rh.RingHipError, match="all linearTransformations must have the same levelP"):
        d.lev.EvaluateManyNew(ct, [lt, low])
    # keys the hoisted products do not take, and a missing key: found before the first launch, opOut untouched
    ev = rh.bgv.Evaluator(d.rq, None, R.t, ringP=d.rp, encoder=d.enc)
    lev = bl.Evaluator(ev)
    galEls = [g for g in lt.GaloisElements(R.N) if g != 1]
    out = d.new(rh, top, fill=12345)
    for make, text in ((lambda: d.kg.GenGaloisKeysNew(galEls, d.sk, levelP=0, BaseTwoDecomposition=16), "unsupported for BaseTwoDecomposition != 0"),
                       (lambda: d.kg.GenGaloisKeysNew(galEls, d.sk, levelP=0), "has one P modulus"),
                       (lambda: d.kg.GenGaloisKeysNew(galEls, d.sk)[:-1], r"GaloisKey\[\d+\] is missing")):
        ev.galois_keys.clear()
        ev.galois_keys.update({k.GaloisElement: k for k in make()})
        for fused in (True, False):
            with pytest.raises(rh.RingHipError, match=text):
                lev.Evaluate(ct, lt, out, fused=fused)
        assert all(np.all(v.numpy() == 12345) for v in out.Value)
    same(ct, host)
    ev.close()


def test_refusals_of_the_kernel_entry(rh):
    d = Dev(rh, "TAIL")
    R = d.R
    L, e = rh.lib(), d.enc._h
    dv = rh.bgv.DeviceValues.from_numpy(d.rq, edge_block(R, False))
    q, p = d.rq.NewPoly(3), d.rp.NewPoly(3)
    rot = (C.c_int * 3)(0, 1, 2)
    lq, lp = len(R.Q) - 1, len(R.P) - 1

    def call(enc=e, ringP=d.rp._h, levelQ=lq, levelP=lp, values=dv.ptr, nvals=R.n, nvec=3, r=rot, cols=R.cols, outQ=q.ptr, outP=p.ptr):
        return L.rh_bgv_embed_qp(enc, ringP, levelQ, levelP, 3, values, nvals, 0, nvec, r, cols, outQ, outP, 1, 1)
    assert call() == 0, L.rh_last_error()
    fresh = rh.bgv.Encoder(d.rq, R.t, ringP=d.rp)                        # more vectors than reserved: the scratch grows, as in the other entries
    fresh.reserve(1)
    q2, p2 = d.rq.NewPoly(3), d.rp.NewPoly(3)
    assert call(enc=fresh._h, outQ=q2.ptr, outP=p2.ptr) == 0, L.rh_last_error()
    assert np.array_equal(q2.numpy(), q.numpy()) and np.array_equal(p2.numpy(), p.numpy())
    fresh.close()
    assert call(nvec=0) == 0 and call(r=None, nvals=R.n - 1, cols=0) == 0, L.rh_last_error()
    assert call(enc=None) == -1 and b"null encoder handle" in L.rh_last_error()
    assert call(ringP=None) == -1 and b"null ring handle" in L.rh_last_error()
    for kw in (dict(values=None), dict(outQ=None), dict(outP=None)):
        assert call(**kw) == -1 and b"rh_bgv_embed_qp: null argument" in L.rh_last_error()
    for kw in (dict(levelQ=-1), dict(levelQ=lq + 1), dict(levelP=-1), dict(levelP=lp + 1)):
        assert call(**kw) == -1 and b"out of range" in L.rh_last_error()
    assert call(nvec=-1) == -1 and b"nvec = -1 out of range" in L.rh_last_error()
    assert call(r=None, nvals=R.n + 1) == -1 and b"len(values)=33 > slots=32" in L.rh_last_error()
    assert call(cols=12) == -1 and b"cols = 12 is not a power of two" in L.rh_last_error()
    assert call(cols=0) == -1 and b"is not a power of two" in L.rh_last_error()
    assert call(cols=8) == -1 and b"nvals = n = 2 * cols" in L.rh_last_error()
    assert call(nvals=16, cols=8) == -1 and b"nvals = n = 2 * cols" in L.rh_last_error()
    assert call(outQ=dv.ptr) == -1 and b"an output overlaps the values" in L.rh_last_error()
    assert call(outP=dv.ptr + 8 * R.n) == -1 and b"an output overlaps the values" in L.rh_last_error()
    assert call(outP=q.ptr + 8 * R.N * (lq + 1)) == -1 and b"outQ and outP overlap" in L.rh_last_error()
    other = rh.Ring(2 * R.N, [int(x) for x in primes.gen_moduli(R.N.bit_length() + 1, [55, 45], [])[0]])
    assert call(ringP=other._h) == -1 and b"another standard ring of degree 32 on the same device" in L.rh_last_error()
    other.close()
    ci = rh.Ring(R.N, [int(x) for x in primes.gen_moduli(7, [55, 45], [])[0]], kind=rh.ConjugateInvariant)
    assert call(ringP=ci._h) == -1 and b"another standard ring of degree 32" in L.rh_last_error()
    ci.close()
    # through the package: shapes and rings that do not fit
    meta = types.SimpleNamespace(Scale=1, IsNTT=True, IsMontgomery=True)
    qp = rh.rlwe.PolyQP(q, p)
    with pytest.raises(rh.RingHipError, match="2 rotations given for a block of 3 polys"):
        d.enc.EmbedRows(dv, [0, 1], R.cols, meta, qp)
    with pytest.raises(rh.RingHipError, match="must be ringqp.Poly"):
        d.enc.EmbedRows(dv, None, R.cols, meta, q)
    with pytest.raises(rh.RingHipError, match="must pair a block of ringQ with a block of ringP"):
        d.enc.EmbedRows(dv, None, R.cols, meta, rh.rlwe.PolyQP(q, d.rp.NewPoly(2)))
    plain = rh.bgv.Encoder(d.rq, R.t)
    with pytest.raises(rh.RingHipError, match="the encoder was built without ringP"):
        plain.EmbedRows(dv, None, R.cols, meta, qp)
    plain.close()

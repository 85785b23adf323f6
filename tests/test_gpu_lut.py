"""GPU: the front end of blindrot.Evaluator.Evaluate on the device -- rh_blindrot_mod_switch, rh_blindrot_program, rh_blindrot_monomials -- whole and
bit for bit against tests/blindrot_restatement.py (mod_switch, lwe_samples, program, evaluate) and against the host front end; keys and key
switching between ring degrees, rgsw.Encryptor and blindrot.GenEvaluationKeyNew against tests/lut_restatement.py; and the chain from device keys to a
decrypted look-up table with no host key material."""
import ctypes as C
import functools

import numpy as np
import pytest

import blindrot_restatement as br
import lut_restatement as lr
import rlwe_restatement as rr
from conftest import QI60, PI60, uniform_mod
from oracle import primes
from test_gpu_blindrot import Q27, Q27_4096, Q55, QLWE, _dev_keyset

pytestmark = pytest.mark.gpu

Q61 = QI60[0]


# ---- mod switch ------------------------------------------------------------------------------------------------------------------------------------
def _planted(rng, q, NBR, n):
    """n coefficients below q: 0, q - 1 (rounds up to 2N, wraps to 0), the two integers either side of every rounding threshold q (2k + 1) / (4N) for
    several k (the first, the last -- 2N - 1 against 0 -- and some between), values that switch to an even non-zero number, and random ones"""
    twoN = 2 * NBR
    x = [0, q - 1, 1, q // 2, q // 2 + 1]
    for k in (0, 1, 2, NBR // 2, NBR - 1, NBR, twoN - 2, twoN - 1):
        t = q * (2 * k + 1) // (2 * twoN)                              # floor of the threshold between k and k + 1
        x += [t, t + 1]
        x.append(min(q * k // twoN + 1, q - 1))                        # well inside k: even non-zero for even k > 0
    x = [int(v) % q for v in x][:n]
    out = np.array(x + [int(v) for v in uniform_mod(rng, q, n - len(x))], dtype=np.uint64)
    return out[rng.permutation(n)] if n > len(x) else out


@pytest.mark.parametrize("NLWE,q,NBR,qbr", [(32, QLWE, 64, Q27), (512, QLWE, 1024, Q27), (64, Q55, 2048, Q27_4096), (64, Q61, 2048, Q27_4096)])
@pytest.mark.parametrize("is_ntt", [False, True])
@pytest.mark.parametrize("ncts", [1, 3])
def test_mod_switch(rh, oracle, NLWE, q, NBR, qbr, is_ntt, ncts):
    rng = np.random.default_rng(NLWE + ncts)
    rq, rl = rh.Ring(NBR, [qbr]), rh.Ring(NLWE, [q])
    ev = rh.blindrot.Evaluator(rq, rl)
    x = np.stack([np.stack([_planted(rng, q, NBR, NLWE) for _ in (0, 1)]) for _ in range(ncts)])            # (ncts, 2, NLWE), coefficient domain
    want = np.array([[br.mod_switch(x[c, k], q, 2 * NBR, k == 1) for k in (0, 1)] for c in range(ncts)], dtype=np.int32)
    assert (want[:, 0] == 0).any() and (want[:, 1] == 2 * NBR - 1).any() and (want[:, 1] == 0).any()
    assert (x == q - 1).any() and br.mod_switch([q - 1], q, 2 * NBR, False) == [0]          # q - 1 rounds up to 2N and wraps to 0
    raw = np.array([[br.mod_switch(x[c, 1], q, 2 * NBR, False)] for c in range(ncts)])
    assert ((raw != 0) & (raw % 2 == 0)).any()                          # an even non-zero value in c1 before ^ 1
    host = [[rr.ntt(x[c, k][None], NLWE, [q]) if is_ntt else x[c, k][None] for k in (0, 1)] for c in range(ncts)]
    cts = [rh.Ciphertext([rh.DevicePoly.from_numpy(rl, p[None]) for p in h], is_ntt=is_ntt) for h in host]
    indices = [0, 3, NLWE - 1, NLWE + 4, -1]                           # the last two are outside the samples and make no job
    a2n, b, jobs = ev.lwe_samples_device(cts, indices)
    assert jobs == [(c, i) for c in range(ncts) for i in (0, 3, NLWE - 1)]
    assert np.array_equal(a2n.numpy(), want)
    assert np.array_equal(b.numpy(), np.array([want[c, 0, i] for c, i in jobs], dtype=np.int32))
    ev.close(); rq.close(); rl.close()


# ---- programs ----------------------------------------------------------------------------------------------------------------------------------------
def _decode(rh, NBR, off, ops, j):
    seg = [int(v) for v in ops.reshape(-1)[off[j]:off[j + 1]]]
    while seg and seg[-1] == rh.blindrot.OP_SKIP:
        seg.pop()
    assert rh.blindrot.OP_SKIP not in seg
    els = rh.blindrot.GaloisElements(NBR)
    return [("EXT", v) if v >= 0 else ("AUTO", els[-v - 1]) for v in seg]


def _job_vector(c1, index, NBR):
    """the a of a job from the switched c1, as lwe_samples forms it (evaluator.go:62-103)"""
    n, mask = len(c1), 2 * NBR - 1
    a = [int(c1[0])] + [-int(c1[n - j]) & mask for j in range(1, n)]
    if index:
        a = a[n - index:] + a[:n - index]
        for j in range(index):
            a[j] = -a[j] & mask
    return a


@pytest.mark.parametrize("NBR,qbr,NLWE,indices", [(64, Q27, 32, list(range(32))), (1024, Q27, 512, [0, 5, 511]), (2048, Q27_4096, 1024, [1023])])
def test_program_of_switched_samples(rh, oracle, NBR, qbr, NLWE, indices):
    """two sample ciphertexts with DIFFERENT index lists in one call of rh_blindrot_program: decoded ops equal br.program of br.lwe_samples"""
    rng = np.random.default_rng(NBR)
    rq, rl = rh.Ring(NBR, [qbr]), rh.Ring(NLWE, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl)
    host = [[uniform_mod(rng, QLWE, NLWE)[None] for _ in (0, 1)] for _ in (0, 1)]
    cts = [rh.Ciphertext([rh.DevicePoly.from_numpy(rl, p[None]) for p in h], is_ntt=False) for h in host]
    a2n, _, _ = ev.lwe_samples_device(cts, [])
    jobs = [(0, i) for i in indices] + [(1, i) for i in indices[:1] + [NLWE // 2]]
    off, ops = ev.program_device(a2n, jobs)
    off, ops = off.numpy(), ops.numpy()
    stride = ops.shape[1]
    assert np.array_equal(off, np.arange(len(jobs) + 1, dtype=np.int32) * stride)
    want = [br.lwe_samples(host[c], False, NLWE, QLWE, NBR, [i for cc, i in jobs if cc == c]) for c in (0, 1)]
    for j, (c, i) in enumerate(jobs):
        assert _decode(rh, NBR, off, ops, j) == br.program(want[c][i][0], NBR), "job %d: ciphertext %d, index %d" % (j, c, i)
    ev.close(); rq.close(); rl.close()


@pytest.mark.parametrize("NBR,qbr,NLWE", [(64, Q27, 32), (1024, Q27, 512)])
def test_program_of_planted_rows(rh, oracle, NBR, qbr, NLWE):
    """hand-planted switched rows: one set holds everything; all entries 0 (the map quirk: set 0); 2N - 1 (stored as -0); +-g^k for N_LWE distinct k;
    only the sets k = 1 and k = N/2 - 1, with either sign"""
    twoN, h = 2 * NBR, NBR // 2
    g = lambda k: pow(5, k, twoN)
    rng = np.random.default_rng(7)
    ks = rng.permutation(h)[:NLWE] if NLWE <= h else None
    rows = [[g(3)] * NLWE, [twoN - g(h - 1)] * NLWE, [0] * NLWE, [twoN - 1] * NLWE, [1] * NLWE,
            [g(1)] + [twoN - g(h - 1)] * (NLWE - 1), [twoN - g(1)] + [g(h - 1)] * (NLWE - 1), [g(h - 1)] + [twoN - g(1)] * (NLWE - 1),
            [g(i % h) if i & 1 else twoN - g(i % h) for i in range(NLWE)]]
    if ks is not None:
        rows.append([g(int(k)) if i & 1 else twoN - g(int(k)) for i, k in enumerate(ks)])
    a2n = np.zeros((len(rows), 2, NLWE), dtype=np.int32)
    a2n[:, 1] = np.array(rows, dtype=np.int32)
    rq, rl = rh.Ring(NBR, [qbr]), rh.Ring(NLWE, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl)
    jobs = [(c, i) for c in range(len(rows)) for i in (0, 1, NLWE - 1)]
    off, ops = ev.program_device(a2n, jobs)
    off, ops = off.numpy(), ops.numpy()
    for j, (c, i) in enumerate(jobs):
        assert _decode(rh, NBR, off, ops, j) == br.program(_job_vector(rows[c], i, NBR), NBR), "row %d, index %d" % (c, i)
    a2n[0, 1, 3] = 6                                                   # an even non-zero a: the reference panics
    with pytest.raises(rh.RingHipError, match="not odd"):
        ev.program_device(a2n, [(0, 0)])
    ev.close(); rq.close(); rl.close()


# ---- Evaluate ----------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want(NBR, NLWE, seed, indices, is_ntt):
    """the restatement's Evaluate, computed once per setting and left unchanged"""
    st = br.setting(NBR, Q27, NLWE, QLWE, 7, 16, seed)
    host = st.ct if is_ntt else [rr.intt(x, NLWE, [QLWE]) for x in st.ct]
    return st, host, br.evaluate(host, is_ntt, NLWE, QLWE, NBR, Q27, {i: st.F for i in indices}, st.keys)


def _evaluate_both(rh, NBR, NLWE, seed, indices, is_ntt, ntt_flag):
    st, host, want = _want(NBR, NLWE, seed, tuple(indices), is_ntt)
    rq, rl = rh.Ring(NBR, [Q27]), rh.Ring(NLWE, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl, NTTFlag=ntt_flag)
    BRK = _dev_keyset(rh, rq, st.keys)
    ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in host], is_ntt=is_ntt)
    F = rh.blindrot.InitTestPolynomial(br.sign, st.scaleBR, rq, -1, 1)
    dev = ev.Evaluate(ct, {i: F for i in indices}, BRK, front_end=True)
    hst = ev.Evaluate(ct, {i: F for i in indices}, BRK, front_end=False)
    assert sorted(dev) == sorted(hst) == sorted(indices)
    for i in indices:
        assert dev[i].IsNTT is ntt_flag
        for comp in (0, 1):
            got = dev[i].Value[comp].numpy()[0]
            assert np.array_equal(got, hst[i].Value[comp].numpy()[0]), "slot %d, component %d: device against host front end" % (i, comp)
            w = want[i][comp] if ntt_flag else rr.intt(want[i][comp], NBR, [Q27])
            assert np.array_equal(got, w), "slot %d, component %d: against the restatement" % (i, comp)
    ev.close(); rq.close(); rl.close()


@pytest.mark.parametrize("is_ntt", [True, False])
@pytest.mark.parametrize("ntt_flag", [True, False])
def test_evaluate_every_slot_of_a_small_ring(rh, oracle, is_ntt, ntt_flag):
    _evaluate_both(rh, 64, 32, 64, list(range(32)), is_ntt, ntt_flag)


@pytest.mark.parametrize("is_ntt,ntt_flag", [(True, True), (False, False)])
def test_evaluate_at_the_reference_setting(rh, oracle, is_ntt, ntt_flag):
    _evaluate_both(rh, 1024, 512, 2022198, [0, 5], is_ntt, ntt_flag)


def test_evaluate_takes_a_list_of_ciphertexts(rh, oracle):
    """two DIFFERENT sample ciphertexts (the second is the first times X^3) in one call, and the default switch"""
    st, host, want = _want(64, 32, 64, (3, 9), True)
    rq, rl = rh.Ring(64, [Q27]), rh.Ring(32, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl)
    BRK = _dev_keyset(rh, rq, st.keys)
    F = rh.blindrot.InitTestPolynomial(br.sign, st.scaleBR, rq, -1, 1)
    c0 = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in st.ct], is_ntt=True)
    shifted = [rr.intt(x, 32, [QLWE]) for x in st.ct]
    shifted = [np.concatenate([(QLWE - x[0, -3:]) % QLWE, x[0, :-3]])[None].astype(np.uint64) for x in shifted]
    c1 = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in shifted], is_ntt=False)
    want1 = br.evaluate(shifted, False, 32, QLWE, 64, Q27, {3: st.F, 9: st.F}, st.keys)
    res = ev.Evaluate([c0, c1], {3: F, 9: F}, BRK, front_end=True)
    assert len(res) == 2
    for r, w in zip(res, (want, want1)):
        assert sorted(r) == [3, 9]
        for i in (3, 9):
            for comp in (0, 1):
                assert np.array_equal(r[i].Value[comp].numpy()[0], w[i][comp])
    assert ev.Evaluate([], {3: F}, BRK, front_end=True) == [] and ev.Evaluate(c0, {40: F}, BRK, front_end=True) == {}
    ev.close(); rq.close(); rl.close()


# ---- refusals, by name -------------------------------------------------------------------------------------------------------------------------------
def test_front_end_refusals(rh, oracle):
    st = br.setting(64, Q27, 32, QLWE, 7, 16, 64)
    N = 64
    rng = np.random.default_rng(5)
    rq, rl2 = rh.Ring(N, [Q27]), rh.Ring(32, [QLWE, 0x10001])
    BRK = _dev_keyset(rh, rq, st.keys)
    F = rh.blindrot.InitTestPolynomial(br.sign, st.scaleBR, rq, -1, 1)
    ev = rh.blindrot.Evaluator(rq, rl2)
    two = rh.Ciphertext([rl2.NewPoly(1), rl2.NewPoly(1)], is_ntt=True)
    with pytest.raises(rh.RingHipError, match="above level 0"):        # multi-limb samples
        ev.Evaluate(two, {0: F}, BRK, front_end=True)
    ev.close()
    rl = rh.Ring(32, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl)
    ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in st.ct], is_ntt=True)
    with pytest.raises(rh.RingHipError, match="composed path"):        # the loop forced onto the composed calls
        ev.Evaluate(ct, {0: F}, BRK, fused=False, front_end=True)
    few = rh.blindrot.MemBlindRotationEvaluationKeySet(BRK.BlindRotationKeys[:31], BRK.AutomorphismKeys)
    with pytest.raises(rh.RingHipError, match=r"BlindRotationKeys\[31\] is missing"):
        ev.Evaluate(ct, {0: F}, few, front_end=True)
    gone = rh.blindrot.GaloisElements(N)[4]
    less = rh.blindrot.MemBlindRotationEvaluationKeySet(BRK.BlindRotationKeys, {g: k for g, k in BRK.AutomorphismKeys.items() if g != gone})
    with pytest.raises(rh.RingHipError, match=r"GaloisKey\[%d\] is missing" % gone):
        ev.Evaluate(ct, {0: F}, less, front_end=True)
    ev.close()
    Q, P = QI60[:2], PI60[:2]                                          # a hybrid key set takes the composed path
    rq2, rp2 = rh.Ring(N, Q), rh.Ring(N, P)
    hyb = lambda: rh.rlwe.GadgetCiphertext(rq2, rp2, np.stack([np.stack([np.stack([uniform_mod(rng, q, N) for q in Q]) for _ in (0, 1)])]),
                                           np.stack([np.stack([np.stack([uniform_mod(rng, p, N) for p in P]) for _ in (0, 1)])]))
    HYB = rh.blindrot.MemBlindRotationEvaluationKeySet([rh.rgsw.Ciphertext(hyb(), hyb())], {g: hyb() for g in rh.blindrot.GaloisElements(N)})
    ev = rh.blindrot.Evaluator(rq2, rl, ringP=rp2)
    with pytest.raises(rh.RingHipError, match="composed path"):
        ev.Evaluate(ct, {0: F}, HYB, front_end=True)
    ev.close()
    L = rh.lib()
    one = (C.c_int32 * 11)(*range(11))
    p = rq.NewPoly(1)
    n3 = 3 << 6
    for r in (rh.Ring(N, QI60[:1], kind=rh.ConjugateInvariant), rh.Ring(n3, primes.gen_moduli_3n(n3, [60], [])[0], kind=rh.Matrix3N)):
        name = b"standard rings only"
        assert L.rh_blindrot_mod_switch(r._h, 6, p.ptr, 0, p.ptr, p.ptr, 0, p.ptr) == -5 and name in L.rh_last_error()
        assert L.rh_blindrot_program(r._h, 32, p.ptr, 0, p.ptr, 0, p.ptr, one, 4096, p.ptr, p.ptr, p.ptr) == -5 and name in L.rh_last_error()
        assert L.rh_blindrot_monomials(r._h, 0, p.ptr, 0, p.ptr) == -5 and name in L.rh_last_error()
        with pytest.raises(rh.RingHipError, match="conjugate-invariant and 3N"):
            rh.blindrot.Evaluator(rq, r)
        r.close()
    assert L.rh_blindrot_program(rq._h, 4096, p.ptr, 0, p.ptr, 0, p.ptr, one, 1 << 20, p.ptr, p.ptr, p.ptr) == -5 and b"what one workgroup holds" in L.rh_last_error()
    assert L.rh_blindrot_program(rq._h, 32, p.ptr, 0, p.ptr, 0, p.ptr, one, 8, p.ptr, p.ptr, p.ptr) == -1 and b"stride" in L.rh_last_error()
    for r in (rq, rl, rl2, rq2, rp2):
        r.close()


# ---- keys and key switching between ring degrees ----------------------------------------------------------------------------------------------------
def _table(key):
    q = key.Q.numpy().reshape(key.digits, 2, key.Q.limbs, -1)
    p = key.P.numpy().reshape(key.digits, 2, key.P.limbs, -1) if key.P is not None else None
    return q, p


@pytest.mark.parametrize("Q,P,pw2", [(QI60[:2], PI60[:1], 0), ([Q27], [], 7), (QI60[:2], PI60[:2], 0)],
                         ids=["two-limbs-one-P", "one-limb-pw2-7", "two-limbs-two-P"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
def test_keys_and_key_switch_between_ring_degrees(rh, oracle, Q, P, pw2, fused):
    """GenEvaluationKeyNew between N = 128 and n = 64 with samples=, and ApplyEvaluationKey in both directions at the top level and at level 0, whole and
    bit for bit against tests/lut_restatement.py; the small secret once with its int32 coefficients and once without (read back from limb 0)"""
    import random
    N, n = 128, 64
    rnd = random.Random(N + pw2)
    rng = np.random.default_rng(N + pw2)
    levelQ, levelP = len(Q) - 1, len(P) - 1
    rq, rp, rs = rh.Ring(N, list(Q)), (rh.Ring(N, list(P)) if P else None), rh.Ring(n, list(Q))
    kg, kgs = rh.rlwe.KeyGenerator(rq, rp), rh.rlwe.KeyGenerator(rs)
    host_big, host_small = rr.Secret.sample(rnd, N), rr.Secret.sample(rnd, n)
    sk_big, sk_small = kg.GenSecretKeyNew(samples=host_big.coeffs), kgs.GenSecretKeyNew(samples=host_small.coeffs)
    bare = rh.rlwe.SecretKey(None, sk_small.Value.Q, None)              # a key without host coefficients: INTT, IMForm and centring of limb 0
    rows = sum(rr.digits_per_limb(Q, levelQ, levelP, pw2))
    mods = list(Q) + list(P)
    ev = rh.rlwe.Evaluator(rq, rp)
    for direction, small in (("down", sk_small), ("up", bare)):
        a = np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(rows)])
        e = rng.integers(-19, 20, size=(rows, N)).astype(np.int32)
        h_in, h_out = (host_big, host_small) if direction == "down" else (host_small, host_big)
        d_in, d_out = (sk_big, small) if direction == "down" else (small, sk_big)
        want = lr.degree_key(h_in, h_out, Q, P, levelQ, levelP, pw2, a, e)
        aQ, aP = np.ascontiguousarray(a[:, :levelQ + 1]), (np.ascontiguousarray(a[:, levelQ + 1:]) if P else None)
        evk = kg.GenEvaluationKeyNew(d_in, d_out, BaseTwoDecomposition=pw2, samples={"a": (aQ, aP), "e": e}, fused=fused)
        q, p = _table(evk)
        assert np.array_equal(q, want.Q) and (p is None) == (want.P is None) and (p is None or np.array_equal(p, want.P)), direction
        NIn, NOut = (N, n) if direction == "down" else (n, N)
        rin, rout = (rq, rs) if direction == "down" else (rs, rq)
        for level in sorted({levelQ, 0}):
            ct = [np.stack([np.stack([uniform_mod(rng, q, NIn) for q in Q[:level + 1]]) for _ in range(2)]) for _ in (0, 1)]      # a batch of 2
            dct = rh.Ciphertext([rh.DevicePoly.from_numpy(rin.AtLevel(level), c) for c in ct], is_ntt=True)
            out = rh.Ciphertext([rout.AtLevel(level).NewPoly(2), rout.AtLevel(level).NewPoly(2)], is_ntt=True)
            ev.ApplyEvaluationKey(dct, evk, out)
            for b in range(2):
                w = lr.apply_evaluation_key(NIn, NOut, Q, P, [ct[0][b], ct[1][b]], want)
                for comp in (0, 1):
                    assert np.array_equal(out.Value[comp].numpy()[b], w[comp]), "%s, level %d, ciphertext %d, component %d" % (direction, level, b, comp)
    ev.close()
    for r in (rq, rp, rs):
        if r is not None:
            r.close()


def test_ring_degree_refusals(rh, oracle):
    N, n = 128, 64
    rq, rs, ro = rh.Ring(N, QI60[:2]), rh.Ring(n, QI60[:2]), rh.Ring(n, [QI60[1], QI60[0]])
    kg = rh.rlwe.KeyGenerator(rq)
    sk, sks, sko = kg.GenSecretKeyNew(), rh.rlwe.KeyGenerator(rs).GenSecretKeyNew(), rh.rlwe.KeyGenerator(ro).GenSecretKeyNew()
    with pytest.raises(rh.RingHipError, match="prefix"):               # non-prefix moduli between the degrees
        kg.GenEvaluationKeyNew(sk, sko)
    with pytest.raises(rh.RingHipError, match="N != n"):               # the generator of the smaller ring
        rh.rlwe.KeyGenerator(rs).GenEvaluationKeyNew(sk, sks)
    evk = kg.GenEvaluationKeyNew(sk, sks, levelP=-1, BaseTwoDecomposition=20)
    ev = rh.rlwe.Evaluator(rs, None)                                   # the evaluator of the smaller ring
    big = rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
    small = rh.Ciphertext([rs.NewPoly(1), rs.NewPoly(1)], is_ntt=True)
    with pytest.raises(rh.RingHipError, match="ctIn ring degree does not match evaluator params ring degree"):
        ev.ApplyEvaluationKey(big, evk, small)
    with pytest.raises(rh.RingHipError, match="opOut ring degree does not match evaluator params ring degree"):
        ev.ApplyEvaluationKey(small, evk, big)
    with pytest.raises(rh.RingHipError, match="coefficient-domain"):   # still refused
        rh.rlwe.Evaluator(rq, None).ApplyEvaluationKey(rh.Ciphertext(big.Value, is_ntt=False), evk, small)
    ev.close()
    for r in (rq, rs, ro):
        r.close()


# ---- RGSW encryption and blind rotation keys on the device ---------------------------------------------------------------------------------------------
def _same(key, want):
    q, p = _table(key)
    return np.array_equal(q, want.Q) and (p is None) == (want.P is None) and (p is None or np.array_equal(p, want.P))


@pytest.mark.parametrize("Q,P,pw2", [([Q27], [], 7), (QI60[:2], PI60[:2], 0)], ids=["one-limb-pw2-7", "two-limbs-two-P"])
@pytest.mark.parametrize("fused", [True, False], ids=["kernel", "composed"])
def test_rgsw_encryptor_from_samples(rh, oracle, Q, P, pw2, fused):
    """rgsw.Encryptor with samples= against tests/lut_restatement.py, whole tables: the four plaintext forms of core/rgsw/encryptor.go:44-57, a zero
    encryption, and a list of three ciphertexts with a plaintext batch in one launch sequence"""
    import random
    N = 64
    rnd = random.Random(N + pw2 + int(fused))
    rng = np.random.default_rng(N + pw2)
    levelQ, levelP = len(Q) - 1, len(P) - 1
    mods = list(Q) + list(P)
    rq, rp = rh.Ring(N, list(Q)), (rh.Ring(N, list(P)) if P else None)
    host_sk = rr.Secret.sample(rnd, N)
    sk = rh.rlwe.KeyGenerator(rq, rp).GenSecretKeyNew(samples=host_sk.coeffs)
    enc = rh.rgsw.Encryptor(rq, rp, sk)
    rows = sum(rr.digits_per_limb(Q, levelQ, levelP, pw2))

    def samples(n):
        a = np.stack([np.stack([uniform_mod(rng, q, N) for q in mods]) for _ in range(2 * rows * n)])
        e = rng.integers(-19, 20, size=(2 * rows * n, N)).astype(np.int32)
        return a, e, {"a": (np.ascontiguousarray(a[:, :levelQ + 1]), np.ascontiguousarray(a[:, levelQ + 1:]) if P else None), "e": e}

    msgs = [rr.Secret.sample(rnd, N) for _ in range(3)]
    coeff = lambda m: rr.rns(m.coeffs, Q)                              # coefficient domain, not Montgomery
    forms = {(False, False): lambda m: coeff(m), (False, True): lambda m: rr._vec("MFORM", coeff(m), None, list(Q)),
             (True, False): lambda m: rr.ntt(coeff(m), N, list(Q)), (True, True): lambda m: m.rows(Q)}
    for (is_ntt, is_mont), make in forms.items():
        a, e, s = samples(1)
        ct = rh.rgsw.NewCiphertext(rq, rp, levelQ, levelP, pw2)
        pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rq, make(msgs[0])[None]), is_ntt=is_ntt, IsMontgomery=is_mont)
        enc.Encrypt(pt, ct, samples=s, fused=fused)
        want = lr.rgsw_encrypt(host_sk, msgs[0].rows(Q), Q, P, levelQ, levelP, pw2, a, e)
        assert _same(ct.Value[0], want[0]) and _same(ct.Value[1], want[1]), (is_ntt, is_mont)
    a, e, s = samples(1)
    ct = rh.rgsw.NewCiphertext(rq, rp, levelQ, levelP, pw2)
    enc.EncryptZero(ct, samples=s, fused=fused)
    want = lr.rgsw_encrypt(host_sk, None, Q, P, levelQ, levelP, pw2, a, e)
    assert _same(ct.Value[0], want[0]) and _same(ct.Value[1], want[1])
    a, e, s = samples(3)
    cts = rh.rgsw.NewCiphertext(rq, rp, levelQ, levelP, pw2, n=3)
    pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rq, np.stack([m.rows(Q) for m in msgs])), is_ntt=True, IsMontgomery=True)
    enc.Encrypt(pt, cts, samples=s, fused=fused)
    for k in range(3):
        want = lr.rgsw_encrypt(host_sk, msgs[k].rows(Q), Q, P, levelQ, levelP, pw2, a[2 * rows * k:2 * rows * (k + 1)], e[2 * rows * k:2 * rows * (k + 1)])
        assert _same(cts[k].Value[0], want[0]) and _same(cts[k].Value[1], want[1]), k
    for r in (rq, rp):
        if r is not None:
            r.close()


@pytest.mark.parametrize("fused", [True, False], ids=["kernel", "composed"])
def test_blind_rotation_keys_from_samples(rh, oracle, fused):
    """blindrot.GenEvaluationKeyNew with samples= at (N_BR, N_LWE) = (64, 32) against the restatement, the LWE secret with and without its host
    coefficients; the key set then runs Evaluate with the device front end to the restatement's bits"""
    import random
    NBR, NLWE, pw2 = 64, 32, 7
    st = br.setting(NBR, Q27, NLWE, QLWE, pw2, 16, 64)
    rng = np.random.default_rng(11)
    rq, rl = rh.Ring(NBR, [Q27]), rh.Ring(NLWE, [QLWE])
    kg = rh.rlwe.KeyGenerator(rq)
    sk_br = kg.GenSecretKeyNew(samples=st.sk_br.coeffs)
    sk_lwe = rh.rlwe.KeyGenerator(rl).GenSecretKeyNew(samples=st.sk_lwe.coeffs)
    rows = 4
    a_r = np.stack([uniform_mod(rng, Q27, NBR)[None] for _ in range(2 * rows * NLWE)])
    e_r = rng.integers(-19, 20, size=(2 * rows * NLWE, NBR)).astype(np.int32)
    a_g = np.stack([uniform_mod(rng, Q27, NBR)[None] for _ in range(11 * rows)])
    e_g = rng.integers(-19, 20, size=(11 * rows, NBR)).astype(np.int32)
    want = lr.blind_rotation_keys(st.sk_br, st.sk_lwe, NBR, Q27, pw2, a_r, e_r, a_g, e_g)
    s = {"rgsw": {"a": (a_r, None), "e": e_r}, "galois": {"a": (a_g, None), "e": e_g}}
    for lwe in (sk_lwe, rh.rlwe.SecretKey(None, sk_lwe.Value.Q, None)):
        BRK = rh.blindrot.GenEvaluationKeyNew(kg, sk_br, rl, lwe, BaseTwoDecomposition=pw2, samples=s, fused=fused)
        assert len(BRK.BlindRotationKeys) == NLWE and sorted(BRK.AutomorphismKeys) == sorted(want.AutomorphismKeys)
        for got, w in zip(BRK.BlindRotationKeys, want.BlindRotationKeys):
            assert _same(got.Value[0], w[0]) and _same(got.Value[1], w[1])
        for g, w in want.AutomorphismKeys.items():
            assert _same(BRK.AutomorphismKeys[g], w), g
    ev = rh.blindrot.Evaluator(rq, rl)
    F = rh.blindrot.InitTestPolynomial(br.sign, st.scaleBR, rq, -1, 1)
    ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in st.ct], is_ntt=True)
    res = ev.Evaluate(ct, {i: F for i in (0, 7)}, BRK, front_end=True)
    w = br.evaluate(st.ct, True, NLWE, QLWE, NBR, Q27, {i: st.F for i in (0, 7)}, want)
    for i in (0, 7):
        for comp in (0, 1):
            assert np.array_equal(res[i].Value[comp].numpy()[0], w[i][comp])
    ev.close(); rq.close(); rl.close()


E2E_KEY = b"look-up table, end to end"


def test_end_to_end_without_host_key_material(rh, oracle):
    """KeyedPRNG throughout: secrets for a large ring (N = 64, Q = [QLWE]), the LWE ring (N = 32) and the blind rotation ring (N = 64, Q27, pw2 = 7); the
    degree-crossing key and the blind rotation key set made on the device; 16 values encrypted, brought down to the LWE degree with
    ApplyEvaluationKey, Evaluate with the device front end and the kernel, decrypted on the device.  Every accumulator meets the criterion of
    tests/test_gpu_blindrot.py: the rotation recomputed from the samples (read back through lwe_samples_device) and the LWE secret; noise below
    Q_BR / 8 everywhere and below Q_BR / 64 at coefficient 0.  The criterion does not hang on the seed: an accumulator's noise is the sum of about
    N_LWE external products and 60 key switches with digits below 2^7, a standard deviation near 2^16 against the bound Q_BR / 64 = 2^21 at
    coefficient 0 (tests/test_lut_oracle.py runs the same check on the CPU with restated keys at these parameters)."""
    N, NLWE, NBR, pw2, slots = 64, 32, 64, 7, 16
    prng = rh.rlwe.KeyedPRNG(E2E_KEY)
    rbig, rl, rq = rh.Ring(N, [QLWE]), rh.Ring(NLWE, [QLWE]), rh.Ring(NBR, [Q27])
    kbig, kl, kbr = (rh.rlwe.KeyGenerator(r, prng=prng) for r in (rbig, rl, rq))
    sk_big, sk_lwe, sk_br = kbig.GenSecretKeyNew(), kl.GenSecretKeyNew(), kbr.GenSecretKeyNew()
    evk = kbig.GenEvaluationKeyNew(sk_big, sk_lwe, BaseTwoDecomposition=4)
    BRK = rh.blindrot.GenEvaluationKeyNew(kbr, sk_br, rl, sk_lwe, BaseTwoDecomposition=pw2)
    values = [-1 + float(2 * i) / float(slots) for i in range(slots)]
    scale = float(QLWE) / 4.0
    m = np.zeros((1, 1, N), dtype=np.uint64)
    for i, v in enumerate(values):
        m[0, 0, 2 * i] = QLWE - int(-v * scale) if v < 0 else int(v * scale)       # Y = X^2: slot i of the LWE ring
    pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rbig, m), is_ntt=False)
    rbig.NTT(pt.Value, pt.Value)
    pt.IsNTT = True
    ct = rh.rlwe.Encryptor(rbig, None, sk_big, prng=prng).EncryptNew(pt)
    small = rh.Ciphertext([rl.NewPoly(1), rl.NewPoly(1)], is_ntt=True)
    evb = rh.rlwe.Evaluator(rbig, None)
    evb.ApplyEvaluationKey(ct, evk, small)
    ev = rh.blindrot.Evaluator(rq, rl)
    F = rh.blindrot.InitTestPolynomial(br.sign, float(Q27) / 4.0, rq, -1, 1)
    Fc = br.lut_coeffs(br.sign, float(Q27) / 4.0, NBR, Q27)
    indices = list(range(slots))
    res = ev.Evaluate(small, {i: F for i in indices}, BRK, front_end=True, fused=True)
    a2n, b, jobs = ev.lwe_samples_device([small], indices)
    a2n, b = a2n.numpy(), b.numpy()
    s_lwe = [int(x) for x in sk_lwe.coeffs.numpy()[0]]
    dec = rh.rlwe.Decryptor(rq, sk_br)
    for j, (_, i) in enumerate(jobs):
        a = _job_vector(a2n[0, 1], i, NBR)
        u = br.rotation(a, int(b[j]), s_lwe, NBR)
        got = rh.rlwe.Plaintext(rq.NewPoly(1), is_ntt=True)
        dec.Decrypt(res[i], got)
        rq.INTT(got.Value, got.Value)
        ph = [int(x) - Q27 if 2 * int(x) > Q27 else int(x) for x in got.Value.numpy()[0, 0]]
        noise = rr.centered_diff(ph, br.expected_plaintext(Fc, Q27, u, NBR), Q27)
        assert max(abs(x) for x in noise) < Q27 // 8 and abs(noise[0]) < Q27 // 64, "slot %d" % i
    ev.close(); evb.close()
    for r in (rbig, rl, rq):
        r.close()


def test_rgsw_encryptor_refusals(rh, oracle):
    rq = rh.Ring(64, QI60[:1])
    kg = rh.rlwe.KeyGenerator(rq)
    sk = kg.GenSecretKeyNew()
    pk = kg.GenPublicKeyNew(sk)
    with pytest.raises(rh.RingHipError, match="public-key encryption is not supported"):
        rh.rgsw.Encryptor(rq, None, pk)
    with pytest.raises(rh.RingHipError, match="no encryption key"):
        rh.rgsw.Encryptor(rq).EncryptZero(rh.rgsw.NewCiphertext(rq, None, 0, -1, 20))
    ci = rh.Ring(64, QI60[:1], kind=rh.ConjugateInvariant)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        rh.rgsw.NewCiphertext(ci, None, 0, -1, 20)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        rh.blindrot.GenEvaluationKeyNew(kg, sk, ci, sk)
    L = rh.lib()
    assert L.rh_rgsw_encrypt(rq._h, None, 0, -1, None, None, None, None, None, None, None, 0, None, 0, None, 0) == -1 and b"null argument" in L.rh_last_error()
    ci.close(); rq.close()

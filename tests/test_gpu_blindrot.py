"""GPU: blind rotation on the device (matrix_fhe_lattigo_amd.blindrot, rh_blindrot_core) and the two evaluator branches it needs -- the 32-bit
ExternalProduct and Automorphism with keys of LevelP <= 0 -- bit for bit against tests/blindrot_restatement.py, and pinned to the rotation
tests/test_blindrot_oracle.py derives."""
import ctypes as C

import numpy as np
import pytest

import blindrot_restatement as br
import rlwe_restatement as rr
from conftest import QI60, PI60, uniform_mod

pytestmark = pytest.mark.gpu

Q27 = 0x7fff801                                                        # the reference's blind rotation modulus: 1 mod 2^11, so N <= 1024
Q27_4096 = 0x7ff6001                                                   # the largest prime below 2^27 that is 1 mod 4096: N = 2048 in the 32-bit branch
Q55 = 0x7ffffffffb4001                                                 # the largest prime below 2^55 that is 1 mod 2^13
QLWE = 0x3001


def _gadget_key(rng, N, q, pw2):
    rows = rr.digits_per_limb([q], 0, -1, pw2)[0]
    return rr.GadgetKey(np.stack([np.stack([uniform_mod(rng, q, N)[None] for _ in (0, 1)]) for _ in range(rows)]), None, 0, -1, pw2, [rows])


def _dev_gadget(rh, rq, rp, k):
    return rh.rlwe.GadgetCiphertext(rq, rp, k.Q, k.P, BaseTwoDecomposition=k.pw2, digits_per_limb=k.digits_per_limb)


def _dev_keyset(rh, rq, keys):
    brk = [rh.rgsw.Ciphertext(_dev_gadget(rh, rq, None, k[0]), _dev_gadget(rh, rq, None, k[1])) for k in keys.BlindRotationKeys]
    return rh.blindrot.MemBlindRotationEvaluationKeySet(brk, {g: _dev_gadget(rh, rq, None, k) for g, k in keys.AutomorphismKeys.items()})


# ---- ExternalProduct, 32-bit branch -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 1024])
@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("worst", [False, True])
def test_external_product_32bit_branch(rh, oracle, N, inplace, worst):
    """core/rgsw/evaluator.go:54-61, :82-117 against the literal loop; worst: every coefficient and every key word q - 1"""
    q, pw2, B = Q27, 7, 3
    rng = np.random.default_rng(N + inplace)
    rq = rh.Ring(N, [q])
    ev = rh.rgsw.Evaluator(rq, None)
    key = [_gadget_key(rng, N, q, pw2) for _ in (0, 1)]
    c = [np.stack([uniform_mod(rng, q, N)[None] for _ in range(B)]) for _ in (0, 1)]
    if worst:
        for k in key:
            k.Q[:] = q - 1
        for x in c:
            x[:] = q - 1
    rgsw = rh.rgsw.Ciphertext(_dev_gadget(rh, rq, None, key[0]), _dev_gadget(rh, rq, None, key[1]))
    op0 = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, c[0]), rh.DevicePoly.from_numpy(rq, c[1])], is_ntt=True)
    out = op0 if inplace else rh.Ciphertext([rq.NewPoly(B), rq.NewPoly(B)], is_ntt=True)
    ev.ExternalProduct(op0, rgsw, out)
    got = [out.Value[0].numpy(), out.Value[1].numpy()]
    for b in range(B):
        want = br.external_product_32bit(N, q, [c[0][b], c[1][b]], key, pw2)
        for comp in (0, 1):
            assert np.array_equal(got[comp][b], want[comp]), "component %d, poly %d" % (comp, b)
    if not inplace:
        assert np.array_equal(op0.Value[0].numpy(), c[0]) and np.array_equal(op0.Value[1].numpy(), c[1])
    ev.close(); rq.close()


# ---- Automorphism with keys of LevelP <= 0 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [64, 4096])
@pytest.mark.parametrize("levelP,pw2", [(-1, 20), (0, 0)])
def test_automorphism_with_single_p_and_power_of_two_keys(rh, oracle, N, levelP, pw2):
    """core/rlwe/evaluator_automorphism.go:14-60 with the other branch of GadgetProduct (evaluator_gadget_product.go:109-113): elements 5 and 2N - 1"""
    Q, P = QI60[:2], PI60[:1] if levelP == 0 else []
    rng = np.random.default_rng(N + pw2)
    B, levelQ = 2, 1
    rq = rh.Ring(N, Q)
    rp = rh.Ring(N, P) if P else None
    dpl = rr.digits_per_limb(Q, levelQ, levelP, pw2)
    keys = {}
    for g in (5, 2 * N - 1):
        kq = np.stack([np.stack([np.stack([uniform_mod(rng, q, N) for q in Q]) for _ in (0, 1)]) for _ in range(sum(dpl))])
        kp = np.stack([np.stack([np.stack([uniform_mod(rng, p, N) for p in P]) for _ in (0, 1)]) for _ in range(sum(dpl))]) if P else None
        keys[g] = rr.GadgetKey(kq, kp, levelQ, levelP, pw2, dpl)
    ev = rh.rlwe.Evaluator(rq, rp, galois_keys={g: _dev_gadget(rh, rq, rp, k) for g, k in keys.items()})
    c = [np.stack([np.stack([uniform_mod(rng, q, N) for q in Q]) for _ in range(B)]) for _ in (0, 1)]
    for g in keys:
        ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, c[0]), rh.DevicePoly.from_numpy(rq, c[1])], is_ntt=True)
        out = rh.Ciphertext([rq.NewPoly(B), rq.NewPoly(B)], is_ntt=True)
        ev.Automorphism(ct, g, out)
        ev.Automorphism(ct, g, ct)                                     # and in place
        for b in range(B):
            want = rr.automorphism(N, Q, P, [c[0][b], c[1][b]], keys[g], g)
            for comp in (0, 1):
                assert np.array_equal(out.Value[comp].numpy()[b], want[comp]), "g = %d, component %d, poly %d" % (g, comp, b)
                assert np.array_equal(ct.Value[comp].numpy()[b], want[comp]), "in place: g = %d, component %d, poly %d" % (g, comp, b)
    ev.close(); rq.close()
    if rp is not None:
        rp.close()


# ---- rh_blindrot_core on hand-made programs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,q,pw2", [(64, Q27, 7), (512, Q27, 7), (1024, Q27, 7), (2048, Q27_4096, 7),
                                      (64, Q55, 14), (512, Q55, 14), (1024, Q55, 14), (2048, Q55, 14)])
def test_core_kernel_on_hand_made_programs(rh, oracle, N, q, pw2):
    """four accumulators with DIFFERENT programs in one launch -- a single EXT, a single AUTO, EXT EXT AUTO EXT and the empty program -- in both
    arithmetic branches of the reference (q < 2^29: the 32-bit loop; larger: MulCoeffsMontgomery): the kernel, the composed calls and the
    restatement give the same bits.  Uniformly random keys: arithmetic parity needs no encryption."""
    rng = np.random.default_rng(N + pw2)
    g1, g2 = 5, 2 * N - 5
    keys = br.KeySet([[_gadget_key(rng, N, q, pw2) for _ in (0, 1)] for _ in range(3)], {g: _gadget_key(rng, N, q, pw2) for g in (g1, g2)}, pw2)
    progs = [[("EXT", 2)], [("AUTO", g2)], [("EXT", 0), ("EXT", 1), ("AUTO", g1), ("EXT", 2)], []]
    B = len(progs)
    c = [np.stack([uniform_mod(rng, q, N)[None] for _ in range(B)]) for _ in (0, 1)]
    c[0][0, 0, :] = q - 1                                              # a worst-case operand among the random ones
    want = [br.run_program(p, N, q, [c[0][b], c[1][b]], keys) for b, p in enumerate(progs)]
    rq = rh.Ring(N, [q])
    ev = rh.blindrot.Evaluator(rq, rq)
    BRK = _dev_keyset(rh, rq, keys)
    for fused in (True, False):
        acc = rh.Ciphertext([rh.DevicePoly.from_numpy(rq, c[0]), rh.DevicePoly.from_numpy(rq, c[1])], is_ntt=True)
        ev._run(progs, acc, BRK, fused)
        got = [acc.Value[0].numpy(), acc.Value[1].numpy()]
        for b in range(B):
            for comp in (0, 1):
                assert np.array_equal(got[comp][b], want[b][comp]), "fused = %s, accumulator %d, component %d" % (fused, b, comp)
    ev.close(); rq.close()


# ---- Evaluate ----------------------------------------------------------------------------------------------------------------------------------------
def _evaluate_and_check(rh, st, indices, is_ntt, fused):
    rq, rl = rh.Ring(st.NBR, [st.QBR]), rh.Ring(st.NLWE, [st.QLWE])
    ev = rh.blindrot.Evaluator(rq, rl)
    BRK = _dev_keyset(rh, rq, st.keys)
    host = st.ct if is_ntt else [rr.intt(x, st.NLWE, [st.QLWE]) for x in st.ct]
    ct = rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in host], is_ntt=is_ntt)
    F = rh.blindrot.InitTestPolynomial(br.sign, st.scaleBR, rq, -1, 1)
    assert np.array_equal(F.numpy()[0], st.F)
    res = ev.Evaluate(ct, {i: F for i in indices}, BRK, fused=fused)
    want = br.evaluate(host, is_ntt, st.NLWE, st.QLWE, st.NBR, st.QBR, {i: st.F for i in indices}, st.keys)
    ab = br.lwe_samples(host, is_ntt, st.NLWE, st.QLWE, st.NBR, indices)
    assert sorted(res) == sorted(indices)
    for i in indices:
        got = [res[i].Value[0].numpy()[0], res[i].Value[1].numpy()[0]]
        for comp in (0, 1):
            assert np.array_equal(got[comp], want[i][comp]), "slot %d, component %d" % (i, comp)
        u = br.rotation(ab[i][0], ab[i][1], st.sk_lwe.coeffs, st.NBR)   # the rotation tests/test_blindrot_oracle.py pins
        noise = rr.centered_diff(rr.phase(got, st.sk_br, [st.QBR]), br.expected_plaintext(st.Fc, st.QBR, u, st.NBR), st.QBR)
        assert max(abs(x) for x in noise) < st.QBR // 8 and abs(noise[0]) < st.QBR // 64, "slot %d" % i
    ev.close(); rq.close(); rl.close()


@pytest.mark.parametrize("is_ntt", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_evaluate_every_slot_of_a_small_ring(rh, oracle, is_ntt, fused):
    st = br.setting(64, Q27, 32, QLWE, 7, 16, 64)
    _evaluate_and_check(rh, st, list(range(32)), is_ntt, fused)


@pytest.mark.parametrize("is_ntt,fused", [(True, True), (False, True), (True, False)])
def test_evaluate_at_the_reference_setting(rh, oracle, is_ntt, fused):
    """core/rgsw/blindrot/blindrot_test.go:48-167 with two slots, index 0 and a non-adjacent one: the monomial shift between them is 5"""
    st = br.setting(1024, Q27, 512, QLWE, 7, 16, 2022198)
    _evaluate_and_check(rh, st, [0, 5], is_ntt, fused)


def test_evaluate_takes_a_list_of_ciphertexts(rh, oracle):
    st = br.setting(64, Q27, 32, QLWE, 7, 16, 64)
    rq, rl = rh.Ring(64, [Q27]), rh.Ring(32, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl)
    BRK = _dev_keyset(rh, rq, st.keys)
    F = rh.blindrot.InitTestPolynomial(br.sign, st.scaleBR, rq, -1, 1)
    cts = [rh.Ciphertext([rh.DevicePoly.from_numpy(rl, x[None]) for x in st.ct], is_ntt=True) for _ in (0, 1)]
    res = ev.Evaluate(cts, {3: F, 9: F}, BRK)
    want = br.evaluate(st.ct, True, 32, QLWE, 64, Q27, {3: st.F, 9: st.F}, st.keys)
    assert len(res) == 2
    for r in res:
        for i in (3, 9):
            for comp in (0, 1):
                assert np.array_equal(r[i].Value[comp].numpy()[0], want[i][comp])
    ev.close()
    ev = rh.blindrot.Evaluator(rq, rl, NTTFlag=False)                  # paramsBR.NTTFlag() = false: the closing INTT (evaluator.go:123-127)
    res = ev.Evaluate(cts[0], {9: F}, BRK)
    assert res[9].IsNTT is False
    for comp in (0, 1):
        assert np.array_equal(res[9].Value[comp].numpy()[0], rr.intt(want[9][comp], 64, [Q27]))
    ev.close(); rq.close(); rl.close()


# ---- refusals, by name ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(rh, oracle):
    N = 64
    rng = np.random.default_rng(5)
    Q, P = QI60[:2], PI60[:2]
    rq, rp, rl = rh.Ring(N, Q), rh.Ring(N, P), rh.Ring(32, [QLWE])
    ev = rh.blindrot.Evaluator(rq, rl, ringP=rp)
    hyb = lambda: rh.rlwe.GadgetCiphertext(rq, rp, np.stack([np.stack([np.stack([uniform_mod(rng, q, N) for q in Q]) for _ in (0, 1)])]),
                                           np.stack([np.stack([np.stack([uniform_mod(rng, p, N) for p in P]) for _ in (0, 1)])]))
    BRK = rh.blindrot.MemBlindRotationEvaluationKeySet([rh.rgsw.Ciphertext(hyb(), hyb())], {g: hyb() for g in rh.blindrot.GaloisElements(N)})
    acc = rh.Ciphertext([rq.NewPoly(1), rq.NewPoly(1)], is_ntt=True)
    with pytest.raises(rh.RingHipError, match="P modulus"):            # a hybrid key with the fused switch forced
        ev.BlindRotateCore([1], acc, BRK, fused=True)
    with pytest.raises(rh.RingHipError, match="not odd"):              # an even non-zero a[i]
        ev.BlindRotateCore([6], acc, BRK)
    with pytest.raises(rh.RingHipError, match="coefficient-domain accumulator"):
        ev.BlindRotateCore([1], rh.Ciphertext(acc.Value, is_ntt=False), BRK)
    ev.close()
    ci = rh.Ring(N, QI60[:1], kind=rh.ConjugateInvariant)
    with pytest.raises(rh.RingHipError, match="conjugate-invariant"):
        rh.blindrot.Evaluator(ci, rl)
    p = ci.NewPoly(1)
    one = (C.c_uint64 * 1)(5)
    L = rh.lib()
    assert L.rh_blindrot_core(ci._h, 7, 4, p.ptr, 1, p.ptr, one, 1, p.ptr, p.ptr, 0, p.ptr, p.ptr, 0) == -5 and b"standard rings only" in L.rh_last_error()
    big = rh.Ring(4096, QI60[:1])
    assert L.rh_blindrot_core(big._h, 7, 4, None, 0, None, one, 0, None, None, 0, None, None, 0) == -5 and b"what one workgroup holds" in L.rh_last_error()
    assert L.rh_blindrot_core(rq._h, 0, 4, None, 0, None, one, 0, None, None, 0, None, None, 0) == -1 and b"power-of-two decomposition" in L.rh_last_error()
    for r in (ci, big, rq, rp, rl):
        r.close()

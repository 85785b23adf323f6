"""GPU: the device key generator, encryptors and decryptor (matrix-fhe-lattigo_amd/keygen.py over csrc/keygen.hip).

With `samples=` every arithmetic entry is compared bit for bit, as whole arrays, with tests/keygen_restatement.py on the cases of
tests/test_keygen_oracle.py (TAIL N = 32, REF N = 2^10, Q61N13 N = 2^13; multi-P, single-P with pw2, no P), with FUSED_KEYGEN on and off, in
batches of 3.  With a fixed KeyedPRNG and no host key material the device keys feed the existing rlwe.Evaluator and the device decryption meets
the reference's bounds; one CKKS program runs end to end through the package."""
import math

import numpy as np
import pytest

import keygen_restatement as kr
import lintrans_restatement as ltr
import rlwe_restatement as rr
import test_keygen_oracle as tko
import test_rlwe_oracle as tro

pytestmark = pytest.mark.gpu
_RINGS = {}


def rings(rh, name, pc):
    """(ringQ, ringP or None) of a chain with its first pc moduli of P, made once per session"""
    if (name, pc) not in _RINGS:
        N, Q, P, _ = tro.chain(name)
        _RINGS[name, pc] = (rh.Ring(N, list(Q)), rh.Ring(N, list(P[:pc])) if pc else None)
    return _RINGS[name, pc]


def split(a, LQ):
    """(rows, LQ + LP, N) -> (aQ, aP or None)"""
    return np.ascontiguousarray(a[:, :LQ]), (np.ascontiguousarray(a[:, LQ:]) if a.shape[1] > LQ else None)


def table(key):
    """a device key as the (rows, 2, limbs, N) arrays the restatement returns"""
    q = key.Q.numpy().reshape(key.digits, 2, key.Q.limbs, -1)
    p = key.P.numpy().reshape(key.digits, 2, key.P.limbs, -1) if key.P is not None else None
    return q, p


def same(key, want):
    q, p = table(key)
    return np.array_equal(q, want.Q) and (p is None) == (want.P is None) and (p is None or np.array_equal(p, want.P))


def device_secret(rh, kg, name, which=0):
    return kg.GenSecretKeyNew(samples=tko.secret_coeffs(name, which))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("case", tko.CASES, ids=tko._ids)
def test_keys_from_samples_bit_for_bit(rh, case, fused):
    name, (pw2, pc), _ = case
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    rq, rp = rings(rh, name, pc)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    sk, sk_out = device_secret(rh, kg, name, 0), device_secret(rh, kg, name, 1)
    host_sk = tko.secrets(name)[0]
    assert np.array_equal(sk.Value.Q.numpy()[0], host_sk.rows(Q)) and np.array_equal(sk.coeffs.numpy()[0], tko.secret_coeffs(name, 0))
    if rp is not None:
        assert np.array_equal(sk.Value.P.numpy()[0], host_sk.rows(P))
    want = tko.keys(case)
    kw = dict(levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=pw2, fused=fused)
    LQ = levelQ + 1
    s = lambda which: {"a": split(want[which][0], LQ), "e": want[which][1]}
    assert same(kg.GenEvaluationKeyNew(sk, sk_out, samples=s("evk_samples"), **kw), want["evk"])
    assert same(kg.GenRelinearizationKeyNew(sk, samples=s("rlk_samples"), **kw), want["rlk"])
    gks = kg.GenGaloisKeysNew(tko.galois_elements(N), sk, samples=s("gks_samples"), **kw)          # three keys in one launch sequence
    assert [g.GaloisElement for g in gks] == tko.galois_elements(N)
    for got, w in zip(gks, want["gks"]):
        assert same(got, w)
    if pc == len(tro.chain(name)[2]) and levelQ == len(Q) - 1:                                      # the public key lives on the whole of QP
        a, e = want["pk_samples"]
        pk = kg.GenPublicKeyNew(sk, samples={"a": split(a, len(Q)), "e": e}, fused=fused)
        wq, wp = want["pk"]
        assert np.array_equal(pk.Q.numpy().reshape(wq.shape), wq) and np.array_equal(pk.P.numpy().reshape(wp.shape), wp)
        el = rh.rlwe.ElementQP.alloc(rq, rp, 1, len(Q) - 1, len(P) - 1)                            # the Element[ringqp.Poly] target of EncryptZero
        rh.rlwe.Encryptor(rq, rp, sk).EncryptZero(el, samples={"a": split(a, len(Q)), "e": e}, fused=fused)
        for c in (0, 1):
            assert np.array_equal(el.Value[c].Q.numpy()[0], wq[0, c]) and np.array_equal(el.Value[c].P.numpy()[0], wp[0, c])


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("is_ntt", [True, False], ids=["ntt", "coeff"])
@pytest.mark.parametrize("shape", tko.ENC, ids=lambda s: "%s-p%d" % s)
def test_encryptors_and_decryptor_from_samples_bit_for_bit(rh, shape, is_ntt, fused):
    name, pc = shape
    N, Q, P, levels = tro.chain(name)
    Q = [int(q) for q in Q]
    rq, rp = rings(rh, name, pc)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    sk = device_secret(rh, kg, name, 0)
    host_sk = tko.secrets(name)[0]
    dec = rh.rlwe.Decryptor(rq, sk)
    for level in (levels[0], levels[0] - 1):                                                        # the top level and one below
        want = tko.encryptions(name, pc, level, is_ntt)
        rl = rq.AtLevel(level)
        pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rl, np.stack(want["pt"])), is_ntt=is_ntt)
        c1, e = want["sk_samples"]
        ct = rh.rlwe.Encryptor(rq, rp, sk).EncryptNew(pt, samples={"c1": c1, "e": e}, fused=fused)
        assert ct.IsNTT == is_ntt
        for c in (0, 1):
            assert np.array_equal(ct.Value[c].numpy(), np.stack([w[c] for w in want["sk"]]))
        a, ep = want["pk_key_samples"]
        pk = kg.GenPublicKeyNew(sk, samples={"a": split(a, len(Q)), "e": ep}, fused=fused)
        u, e0, e1 = want["pk_samples"]
        ctp = rh.rlwe.Encryptor(rq, rp, pk).EncryptNew(pt, samples={"u": u, "e0": e0, "e1": e1}, fused=fused)
        for c in (0, 1):
            assert np.array_equal(ctp.Value[c].numpy(), np.stack([w[c] for w in want["pk"]]))
        got = dec.DecryptNew(ctp, fused=fused)
        assert got.IsNTT == is_ntt
        assert np.array_equal(got.Value.numpy(), np.stack([kr.decrypt(w, host_sk, Q, is_ntt) for w in want["pk"]]))
        # degree 2: (c0, c1, c1') of two ciphertexts stacked is a valid operand of the Horner sum, whatever it decrypts to
        ct2 = rh.Ciphertext([ct.Value[0], ct.Value[1], ctp.Value[1]], is_ntt=is_ntt)
        got2 = dec.DecryptNew(ct2, fused=fused)
        w2 = [kr.decrypt([want["sk"][k][0], want["sk"][k][1], want["pk"][k][1]], host_sk, Q, is_ntt) for k in range(3)]
        assert np.array_equal(got2.Value.numpy(), np.stack(w2))


def _std_bits(rq, dec, ct, want_coeffs, level):
    """log2 std of the device decryption's error per ciphertext of the batch, against integer messages"""
    pt = dec.DecryptNew(ct)
    if pt.IsNTT:
        rq.AtLevel(level).INTT(pt.Value, pt.Value)
    mods = [int(q) for q in rq.moduli[:level + 1]]
    M = rr.prod(mods)
    arr = pt.Value.numpy()
    return [rr.log2_std(rr.centered_diff(rr.crt_centered(arr[k], mods), want_coeffs[k], M)) for k in range(arr.shape[0])]


@pytest.mark.parametrize("case", [c for c in tko.CASES if c[2] is None], ids=tko._ids)
def test_no_host_key_material_evaluator_and_decryption_meet_the_reference_bounds(rh, case):
    """keys, ciphertexts and decryptions from a fixed KeyedPRNG alone: GadgetProduct, Relinearize and Automorphism of the existing rlwe.Evaluator
    under device keys, decrypted on the device (rlwe_test.go:703, :925-929; fresh encryptions :608, :634)"""
    name, (pw2, pc), _ = case
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    rq, rp = rings(rh, name, pc)
    prng = rh.rlwe.KeyedPRNG(b"end to end " + name.encode())
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk, sk_out = kg.GenSecretKeyNew(), kg.GenSecretKeyNew()
    s = sk.coeffs.numpy()[0]
    assert set(np.unique(s)) <= {-1, 0, 1} and abs(np.count_nonzero(s) - 2 * N / 3) <= 6 * math.sqrt(N * 2 / 9)
    kw = dict(BaseTwoDecomposition=pw2)
    evk, rlk = kg.GenEvaluationKeyNew(sk, sk_out, **kw), kg.GenRelinearizationKeyNew(sk, **kw)
    galEls = tko.galois_elements(N)
    evs = rh.rlwe.MemEvaluationKeySet(rlk, kg.GenGaloisKeysNew(galEls, sk, **kw))
    ev = rh.rlwe.Evaluator(rq, rp, galois_keys=evs.galois_keys)
    enc, dec, dec_out = rh.rlwe.Encryptor(rq, rp, sk, prng=prng), rh.rlwe.Decryptor(rq, sk), rh.rlwe.Decryptor(rq, sk_out)
    level = levelQ
    rl = rq.AtLevel(level)
    mods = Q[:level + 1]
    ms = tko.message(name, level)
    pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rl, np.stack([rr.ntt(rr.rns(m, mods), N, mods) for m in ms])), is_ntt=True)
    ct = enc.EncryptNew(pt)
    fresh = math.log2(kr.noise_fresh_sk()) + 1
    got = _std_bits(rq, dec, ct, ms, level)
    print("MEASURED fresh sk %s %s [%.2f]" % (tko._ids(case), got, fresh))
    assert max(got) <= fresh
    if pc == len(tro.chain(name)[2]):
        pk = kg.GenPublicKeyNew(sk)
        bnd = math.log2(kr.noise_fresh_pk(math.ceil(N * 2 / 3), pc > 0)) + 1
        got = _std_bits(rq, dec, rh.rlwe.Encryptor(rq, rp, pk, prng=prng).EncryptNew(pt), ms, level)
        print("MEASURED fresh pk %s %s [%.2f]" % (tko._ids(case), got, bnd))
        assert max(got) <= bnd
    # key switch sk -> sk_out: (c0 + KS(c1)_0, KS(c1)_1) decrypts under sk_out to the same messages
    out = rh.Ciphertext([rl.NewPoly(3), rl.NewPoly(3)], is_ntt=True)
    ev.GadgetProduct(level, ct.Value[1], evk, out)
    rl.Add(out.Value[0], ct.Value[0], out.Value[0])
    got = _std_bits(rq, dec_out, out, ms, level)
    print("MEASURED switch   %s %s [%.2f]" % (tko._ids(case), got, tro.bound(N, pw2)))
    assert max(got) <= tro.bound(N, pw2)
    for g in galEls:
        ev.Automorphism(ct, g, out)
        got = _std_bits(rq, dec, out, [rr.automorphism_coeffs(m, g) for m in ms], level)
        print("MEASURED auto %-4d %s %s [%.2f]" % (g, tko._ids(case), got, tro.bound(N, pw2, level)))
        assert max(got) <= tro.bound(N, pw2, level)
    # the relinearisation key, sk^2 -> sk: (c0, 0, c1) decrypts to c0 + s^2 c1, and (c0 + KS(c1)_0, KS(c1)_1) must decrypt to the same under sk
    # (:703).  GadgetProduct and the Add serve every setting; Relinearize itself takes keys with levelP >= 1.
    zero = rl.NewPoly(3)
    rl.vec_op("ZERO", None, None, zero)
    ct2 = rh.Ciphertext([ct.Value[0], zero, ct.Value[1]], is_ntt=True)
    want = dec.DecryptNew(ct2)
    rl.INTT(want.Value, want.Value)
    arr = want.Value.numpy()
    want2 = [rr.crt_centered(arr[k], mods) for k in range(3)]
    ev.GadgetProduct(level, ct.Value[1], rlk, out)
    rl.Add(out.Value[0], ct.Value[0], out.Value[0])
    got = _std_bits(rq, dec, out, want2, level)
    print("MEASURED relin    %s %s [%.2f]" % (tko._ids(case), got, tro.bound(N, pw2)))
    assert max(got) <= tro.bound(N, pw2)
    if levelP >= 1:
        ev.Relinearize(ct2, out)
        assert max(_std_bits(rq, dec, out, want2, level)) <= tro.bound(N, pw2)
    # the same PRNG key replays the same keys
    kg2 = rh.rlwe.KeyGenerator(rq, rp, prng=rh.rlwe.KeyedPRNG(b"end to end " + name.encode()))
    assert np.array_equal(kg2.GenSecretKeyNew().coeffs.numpy(), sk.coeffs.numpy())
    ev.close()


def test_prng_keys_equal_the_restatement(rh):
    """no samples handed in: the device draws them from the stream, and the restated samplers with the same call counters give the same key"""
    case = ("REF", (0, 2), None)
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    rq, rp = rings(rh, "REF", 2)
    prng = rh.rlwe.KeyedPRNG(tko.KEY)
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk = device_secret(rh, kg, "REF", 0)
    prng.calls = 40                                                                                  # where test_keygen_oracle.keys draws its Galois keys
    gks = kg.GenGaloisKeysNew(tko.galois_elements(N), sk)
    assert prng.calls == 42
    for got, w in zip(gks, tko.keys(case)["gks"]):
        assert same(got, w)
    import matrix_fhe_lattigo_amd.keygen as keygen
    cap = keygen.SCRATCH_CAP
    try:                                                                                             # chunked over the keys: the same tables
        keygen.SCRATCH_CAP = 1
        prng.calls = 40
        for got, w in zip(kg.GenGaloisKeysNew(tko.galois_elements(N), sk), tko.keys(case)["gks"]):
            assert same(got, w)
    finally:
        keygen.SCRATCH_CAP = cap


def test_ckks_program_end_to_end(rh):
    """encode -> encrypt (pk) -> MulRelin -> Rescale -> Rotate -> decrypt -> decode at N = 2^10 (the REF chain), every step in the package, against
    the plain computation.  tests/test_ckks_oracle.py holds no precision bound; the bound is the one every CKKS test of this project takes from the
    reference (VerifyTestVectors, schemes/ckks/precision.go:92-103, as tests/test_gpu_lintrans.py states it): the average precision of the real and
    of the imaginary parts is at least log2(DefaultScale) - (LogN + 2) bits, DefaultScale being the scale the messages are encoded at, q_L here
    (the product then comes back to that scale after the rescale): 35.0 - 12 = 23.0 bits."""
    N, Q, P, levels = tro.chain("REF")
    logN = N.bit_length() - 1
    rq, rp = rings(rh, "REF", 2)
    prng = rh.rlwe.KeyedPRNG(b"ckks program")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk, pk = kg.GenKeyPairNew()
    k = 3
    galEl = rh.ckks.GaloisElement(N, k)
    evs = rh.rlwe.MemEvaluationKeySet(kg.GenRelinearizationKeyNew(sk), kg.GenGaloisKeysNew([galEl], sk))
    level = levels[0]
    ecd = rh.ckks.Encoder(rq)
    ev = rh.ckks.Evaluator(rq, rp, rlk=evs.RelinearizationKey, galois_keys=evs.GaloisKeys)
    slots = N // 2
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
    y = rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
    scale = float(int(Q[level]))
    enc, dec = rh.ckks.Encryptor(rq, rp, pk, prng=prng), rh.ckks.Decryptor(rq, sk)
    ptx, pty = ecd.NewPlaintext(level, scale), ecd.NewPlaintext(level, scale)
    ecd.Encode(x, ptx)
    ecd.Encode(y, pty)
    cx, cy = enc.EncryptNew(ptx), enc.EncryptNew(pty)
    assert cx.Scale.Float64() == scale and cx.LogDimensions == ptx.LogDimensions and cx.IsBatched
    prod = ev.MulRelinNew(cx, cy)
    low = rq.AtLevel(level - 1)
    res = rh.Ciphertext([low.NewPoly(1), low.NewPoly(1)], is_ntt=True)
    ev.Rescale(prod, res)
    rot = ev.RotateNew(res, k)
    rot.LogDimensions, rot.IsBatched = cx.LogDimensions, cx.IsBatched       # the evaluator carries the scale; the slot layout is the caller's
    out = dec.DecryptNew(rot)
    assert out.Level() == level - 1
    got = np.asarray(ecd.Decode(out)).reshape(-1)[:slots]
    want = np.roll(x * y, -k)
    pr, pi = ltr.avg_log2_prec(want, got.real, got.imag, math.log2(scale))
    bound = math.log2(scale) - (logN + 2)
    worst = -math.log2(max(np.abs(got.real - want.real).max(), np.abs(got.imag - want.imag).max()))
    print("MEASURED ckks program precision real %.2f imag %.2f (worst slot %.2f) [>= %.2f]" % (pr, pi, worst, bound))
    assert pr >= bound and pi >= bound
    ev.close()
    ecd.close()


def test_bgv_program_end_to_end(rh):
    """encode -> encrypt (sk and pk) -> decrypt -> decode through bgv.Encryptor / Decryptor: the values come back exactly, the plaintext's Scale
    and IsBatched travel with the ciphertext"""
    N, Q, P, levels = tro.chain("REF")
    rq, rp = rings(rh, "REF", 2)
    t = 65537
    prng = rh.rlwe.KeyedPRNG(b"bgv program")
    kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
    sk, pk = kg.GenKeyPairNew()
    ecd = rh.bgv.Encoder(rq, t)
    values = np.random.default_rng(5).integers(0, t, size=(2, N), dtype=np.uint64)
    pt = ecd.NewPlaintext(levels[0], scale=3, nvec=2)
    ecd.Encode(values, pt)
    dec = rh.bgv.Decryptor(rq, sk)
    for key in (sk, pk):
        ct = rh.bgv.Encryptor(rq, rp, key, prng=prng).EncryptNew(pt)
        assert ct.Scale == 3 and ct.IsBatched and ct.IsNTT
        out = dec.DecryptNew(ct)
        assert out.Scale == 3 and np.array_equal(np.asarray(ecd.Decode(out)).reshape(2, -1)[:, :N], values)
    ecd.close()


@pytest.mark.parametrize("policy", [0, 2], ids=["default-policy", "non-temporal"])
def test_every_cache_policy_gives_the_same_bits(rh, policy):
    """the new kernels' data streams under tuning nt_streams = 0 (default policy everywhere) and 2 (non-temporal at every size): the same arrays as
    under the by-working-set rule the other tests run"""
    case = ("REF", (0, 2), None)
    N, Q, P, levelQ, levelP, pw2 = tko.dims(case)
    rq, rp = rings(rh, "REF", 2)
    try:
        for r in (rq, rp):
            r.set_tuning("nt_streams", policy)
        prng = rh.rlwe.KeyedPRNG(tko.KEY)
        kg = rh.rlwe.KeyGenerator(rq, rp, prng=prng)
        sk = device_secret(rh, kg, "REF", 0)
        prng.calls = 40
        for got, w in zip(kg.GenGaloisKeysNew(tko.galois_elements(N), sk), tko.keys(case)["gks"]):      # sampler, lift and rh_rlwe_gadget_encrypt
            assert same(got, w)
        want = tko.encryptions("REF", 2, levelQ, True)
        pt = rh.rlwe.Plaintext(rh.DevicePoly.from_numpy(rq, np.stack(want["pt"])), is_ntt=True)
        c1, e = want["sk_samples"]
        ct = rh.rlwe.Encryptor(rq, rp, sk).EncryptNew(pt, samples={"c1": c1, "e": e})
        a, ep = want["pk_key_samples"]
        pk = kg.GenPublicKeyNew(sk, samples={"a": split(a, len(Q)), "e": ep})
        u, e0, e1 = want["pk_samples"]
        ctp = rh.rlwe.Encryptor(rq, rp, pk).EncryptNew(pt, samples={"u": u, "e0": e0, "e1": e1})
        for c in (0, 1):
            assert np.array_equal(ct.Value[c].numpy(), np.stack([w[c] for w in want["sk"]]))
            assert np.array_equal(ctp.Value[c].numpy(), np.stack([w[c] for w in want["pk"]]))
        host_sk = tko.secrets("REF")[0]
        got = rh.rlwe.Decryptor(rq, sk).DecryptNew(ctp)
        assert np.array_equal(got.Value.numpy(), np.stack([kr.decrypt(w, host_sk, Q) for w in want["pk"]]))
    finally:
        for r in (rq, rp):
            r.set_tuning("nt_streams", 1)


def test_refusals(rh):
    rq, rp = rings(rh, "TAIL", 4)
    kg = rh.rlwe.KeyGenerator(rq, rp)
    sk = device_secret(rh, kg, "TAIL", 0)
    with pytest.raises(rh.RingHipError, match="compressed"):
        kg.GenRelinearizationKeyNew(sk, compressed=True)
    with pytest.raises(rh.RingHipError, match="RingSwap"):
        kg.GenEvaluationKeysForRingSwapNew(sk, sk)
    big = rh.Ring(64, [int(q) for q in tro.chain("TAIL")[1]])
    other = rh.rlwe.KeyGenerator(big).GenSecretKeyNew()
    with pytest.raises(rh.RingHipError, match="N != n"):
        kg.GenEvaluationKeyNew(sk, other)
    ci = rh.Ring(32, [0x1fffffffffe00001], kind=rh.ConjugateInvariant)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        rh.rlwe.KeyGenerator(ci)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        rh.rlwe.Encryptor(ci, None, sk)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        rh.rlwe.Decryptor(ci, sk)
    with pytest.raises(rh.RingHipError, match="no encryption key"):
        rh.rlwe.Encryptor(rq, rp).EncryptZeroNew(2)
    with pytest.raises(rh.RingHipError, match="must be odd"):
        kg.GenGaloisKeyNew(4, sk)
    L = rh.lib()
    assert L.rh_rlwe_decrypt(rq._h, 0, None, None, None, None, None, 1) != 0 and b"null argument" in L.rh_last_error()
    ci.close()
    big.close()

"""CPU: core/rgsw/blindrot restated (tests/blindrot_restatement.py) and pinned to decryption at the reference's own test setting
(core/rgsw/blindrot/blindrot_test.go:48-167); the 32-bit external product's literal loop against the Montgomery branch; the step program of
matrix_fhe_lattigo_amd.blindrot against the restatement and against a direct evaluation of Algorithm 3 on exponents."""
import random

import numpy as np
import pytest

import blindrot_restatement as br
import rlwe_restatement as rr

NBR, QBR, NLWE, QLWE, PW2, SLOTS, SEED = 1024, 0x7fff801, 512, 0x3001, 7, 16, 2022198


@pytest.fixture(scope="module")
def rotated():
    """the restated Evaluate at the reference's setting, once: (setting, {index: ciphertext}, {index: (a, b)})"""
    st = br.setting(NBR, QBR, NLWE, QLWE, PW2, SLOTS, SEED)
    polys = {i: st.F for i in range(SLOTS)}
    res = br.evaluate(st.ct, True, NLWE, QLWE, NBR, QBR, polys, st.keys)
    return st, res, br.lwe_samples(st.ct, True, NLWE, QLWE, NBR, range(SLOTS))


def _noise(st, res, ab):
    """per slot: (u, Dec(res) - F X^u centred)"""
    out = {}
    for i in range(SLOTS):
        a, b = ab[i]
        u = br.rotation(a, b, st.sk_lwe.coeffs, NBR)
        dec = rr.phase(res[i], st.sk_br, [QBR])
        out[i] = (u, rr.centered_diff(dec, br.expected_plaintext(st.Fc, QBR, u, NBR), QBR))
    return out


def test_decrypts_to_the_rotated_test_polynomial_within_the_decoding_bound(rotated):
    """Dec(res_i) - F X^(u_i), u_i = b_i + <a, s> mod 2N with the PLUS sign (blindrot_restatement.rotation derives it) and the map's quirks applied.
    The reference decodes round(4 c / Q * 8) / 8 (blindrot_test.go:153-164): a step of Q / 32, so the constant coefficient's noise must stay below
    half a step, Q / 64 -- a bound from the decoding, not from what the code gives."""
    st, res, ab = rotated
    noise = _noise(st, res, ab)
    worst0 = max(abs(d[0]) for _, d in noise.values())
    sup = max(max(abs(x) for x in d) for _, d in noise.values())
    print("MEASURED blind rotation noise: constant coefficient %d (2^%.2f), all coefficients %d (2^%.2f), bound Q/64 = %d"
          % (worst0, np.log2(max(worst0, 1)), sup, np.log2(max(sup, 1)), QBR // 64))
    assert worst0 < QBR // 64
    # a wrong rotation is off by the whole test polynomial, Q / 4 on every coefficient where the signs differ: the sup-norm tells them apart
    assert sup < QBR // 8


def test_decoded_signs(rotated):
    """the assertion the reference's test has commented out (blindrot_test.go:164): round(a * 8) / 8 == sign(values[i]) for values != 0.  A slot
    may be left out only when the mod switch moved its rotation across a sign change of the table, at most 2 of the 16, each named."""
    st, res, ab = rotated
    left_out = []
    for i, v in enumerate(st.values):
        if v == 0:
            continue
        a, b = ab[i]
        u = br.rotation(a, b, st.sk_lwe.coeffs, NBR)
        ideal = v * NBR / 2.0                                          # v Q_LWE / 4 * 2 N_BR / Q_LWE
        drift = (u - ideal + NBR) % (2 * NBR) - NBR
        # the table changes sign at rotation 0 (and nowhere else within reach: X^N = -1 continues it at +-N/2): the drift must not carry u across it
        if abs(drift) >= abs(ideal):
            left_out.append((i, v, drift))
            continue
        c = rr.phase(res[i], st.sk_br, [QBR])[0] % QBR                 # the decrypted constant coefficient (blindrot_test.go:147-153)
        x = -float(QBR - c) / st.scaleBR if c >= QBR >> 1 else float(c) / st.scaleBR
        assert round(x * 8) / 8 == br.sign(v), "slot %d: value %g decodes to %g" % (i, v, round(x * 8) / 8)
    for i, v, drift in left_out:
        print("LEFT OUT slot %d (value %g): mod-switch drift %g" % (i, v, drift))
    assert len(left_out) <= 2, left_out


@pytest.mark.parametrize("N", [64, 1024])
def test_32bit_product_is_the_montgomery_branch(N):
    """core/rgsw/evaluator.go:57: the wrapping sum never overflows, so IMForm of it is the canonical residue MulCoeffsMontgomeryThenAdd accumulates.
    Random operands, and the worst case: every coefficient and every key word q - 1."""
    rng = np.random.default_rng(N)
    q, pw2, digits = QBR, PW2, 4
    for worst in (False, True):
        draw = (lambda *s: np.full(s, q - 1, dtype=np.uint64)) if worst else (lambda *s: (rng.integers(0, q, size=s, dtype=np.uint64)))
        key = [rr.GadgetKey(draw(digits, 2, 1, N), None, 0, -1, pw2, [digits]) for _ in (0, 1)]
        ct = [draw(1, N), draw(1, N)]
        a = br.external_product_32bit(N, q, ct, key, pw2)
        b = br.external_product_montgomery(N, q, ct, key, pw2)
        for c in (0, 1):
            assert np.array_equal(a[c], b[c]) and int(a[c].max()) < q


def _powers(N):
    g = lambda k: pow(5, k, 2 * N)
    return g, (lambda k: 2 * N - g(k))


def _hand_made(N):
    g, m = _powers(N)
    return {
        "empty": [],                                                    # every set empty
        "one far set": [g(25)],                                         # ten and more empty k's in a row below it: the window fires
        "k = 1 occupied": [g(1), g(7), m(1)],
        "k = 1 empty": [g(2), m(3), g(0)],
        "zero": [g(4), 0, m(4), 0],                                     # a[i] = 0 reads as set 0
        "minus one": [2 * N - 1, g(3)],                                 # 2N - 1 is stored as -0
        "both signs, shared k": [g(9), m(9), g(9), m(20), g(20), g(31), m(31), 1],
        "every k once": [g(k) for k in range(N >> 1)] + [m(k) for k in range(1, N >> 1)],
    }


@pytest.mark.parametrize("N", [64, 128])
def test_step_program_against_a_direct_evaluation(rh, N):
    rnd = random.Random(N)
    g, m = _powers(N)
    for name, a in _hand_made(N).items():
        prog = rh.blindrot.blind_rotate_program(a, N)
        assert prog == br.program(a, N), name
        assert sorted(j for kind, j in prog if kind == "EXT") == list(range(len(a))), name       # every key once
        assert all(x in rh.blindrot.GaloisElements(N) for kind, x in prog if kind == "AUTO"), name      # only elements that have a key
        s = [rnd.randrange(-1, 2) for _ in a]
        alpha, beta = br.simulate_exponents(prog, s, N)
        assert alpha == 1, name
        assert beta == br.rotation(a, 0, s, N), name
    assert rh.blindrot.getDiscreteLogSets([g(4), 0, m(4), 0], rh.blindrot.getGaloisElementInverseMap(N)) == {4: [0], 0: [1, 3], -4: [2]}
    assert rh.blindrot.getDiscreteLogSets([2 * N - 1], rh.blindrot.getGaloisElementInverseMap(N)) == {0: [0]}
    far = rh.blindrot.blind_rotate_program([g(25)], N)
    assert ("AUTO", g(10)) in far[:far.index(("EXT", 0))]               # window steps before the one occupied set
    occ = rh.blindrot.blind_rotate_program([g(1)], N)
    assert occ[-2:] == [("EXT", 0), ("AUTO", g(1))]                     # k = 1 occupied: the product, then the step the k == 1 rule forces
    emp = rh.blindrot.blind_rotate_program([g(0)], N)
    assert emp[-1] == ("EXT", 0) and emp[-2][0] == "AUTO"               # k = 1 empty: the rule still fires before set 0
    with pytest.raises(rh.RingHipError, match="not odd"):
        rh.blindrot.blind_rotate_program([g(1), 6], N)


def test_host_helpers_match_the_restatement(rh):
    assert rh.blindrot.GaloisElements(NBR) == br.galois_elements(NBR) and len(br.galois_elements(NBR)) == 11
    assert rh.blindrot.getGaloisElementInverseMap(64) == br.galois_inverse_map(64)
    for v in (-1.0, -0.3, 0.0, 0.49999, 1.0):
        assert rh.blindrot.scaleUp(v, QBR / 4.0, QBR) == br.scale_up(v, QBR / 4.0, QBR)
    a = list(range(1, 17))
    assert rh.blindrot.mulBySmallMonomialMod2N(127, a, 3) == [(-x) & 127 for x in a[13:]] + a[:13]


def test_entry_point_refuses_bad_arguments_without_a_device(rh):
    L = rh.lib()
    assert L.rh_blindrot_core(None, 7, 4, None, 0, None, None, 0, None, None, 0, None, None, 0) == -1
    assert b"rh_blindrot_core: null ring handle" in L.rh_last_error()

"""CPU: the host-side pieces of matrix-fhe-lattigo_amd/multiparty.py against Python integers: the noise formulas of multiparty/utils.go at
hand-computed values, the Lagrange factors of threshold.go, the row tables the share kernels read, and the common-reference-string rule."""
import math
import struct

import pytest

import multiparty_restatement as mr
import sampling_restatement as sr
import test_rlwe_oracle as tro


def test_noise_formulas_at_hand_computed_values(rh):
    mp = rh.multiparty
    # NoiseRelinearizationKey: H = 5 * 683 = 3415, e = 5 * 3.2^2 = 51.2, sqrt(2 * 51.2 * 3416) = sqrt(349798.4)
    assert mp.NoiseRelinearizationKey(683, 5) == pytest.approx(math.sqrt(349798.4), rel=1e-15)
    assert mp.NoiseRelinearizationKey(1, 1, sigma=1.0) == 2.0                                      # sqrt(2 * 1 * 2)
    assert mp.NoiseEvaluationKey(4) == 6.4 and mp.NoiseGaloisKey(4) == 6.4                        # sqrt(4) * 3.2
    assert mp.NoiseEvaluationKey(9, sigma=2.0) == 6.0
    # noiseDecryptWithSmudging: sqrt(parties * (fresh^2 + flood^2) + ct^2)
    assert mp.NoiseKeySwitch(5, 3.2, 25.6) == pytest.approx(math.sqrt(5 * (10.24 + 655.36) + 10.24), rel=1e-15)
    assert mp.NoiseKeySwitch(1, 0.0, 4.0, sigma=3.0) == 5.0
    assert mp.NoisePublicKeySwitch(4, 3.0, 0.0, 2.0) == 5.0                                        # sqrt(4 * 4 + 9)
    assert mp.NoisePublicKeySwitch(5, 3.2, 25.6, 7.5) == pytest.approx(math.sqrt(5 * (56.25 + 655.36) + 10.24), rel=1e-15)


@pytest.mark.parametrize("name", ["REF", "TAIL"])
def test_lagrange_coefficient_against_python_integers(rh, name):
    _, Q, P, _ = tro.chain(name)
    mods = [int(q) for q in Q] + [int(p) for p in P]
    points = [1, 2, 3, 4, 5, 1 << 40, (1 << 64) - 1]
    for this in points:
        for that in points:
            if this == that:
                continue
            got = rh.multiparty.lagrange_coefficient(mods, this, that)
            assert got == mr.lagrange(mods, this, that)
            for c, q in zip(got, mods):
                assert 0 <= c < q and c * ((that - this) % q) % q == that % q
    # the factors of any t points interpolate a polynomial of degree t - 1 at zero
    coeffs = [123456789, 987654321, 555]
    for q in mods:
        f = lambda x: sum(c * pow(x, k, q) for k, c in enumerate(coeffs)) % q
        pts = [2, 5, 9]
        total = 0
        for own in pts:
            w = 1
            for other in pts:
                if other != own:
                    w = w * rh.multiparty.lagrange_coefficient([q], own, other)[0] % q
            total = (total + f(own) * w) % q
        assert total == coeffs[0] % q
    with pytest.raises(rh.RingHipError, match="equal"):
        rh.multiparty.lagrange_coefficient(mods, 3, 3)


def _scalar(P, j, pw2, q):
    Pb = 1
    for p in P:
        Pb *= p
    return ((Pb << (j * pw2)) << 64) % q


def test_share_row_tables(rh):
    table = rh.multiparty.gadget_row_table
    dpl_of = rh.multiparty.digits_per_limb
    _, Q, P, _ = tro.chain("TAIL")
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    # 7 limbs of Q under 4 of P: two digits, the last of three limbs
    rows = table(Q, P, 6, 3, 0, dpl_of(Q, 6, 3, 0))
    assert len(rows) == 2 and all(len(r) == 8 for r in rows)
    assert rows[0][1:] == [_scalar(P, 0, 0, q) for q in Q[:4]] + [0, 0, 0]
    assert rows[1][1:] == [0, 0, 0, 0] + [_scalar(P, 0, 0, q) for q in Q[4:7]]
    # cut to 6 limbs: the last digit has two
    rows = table(Q, P, 5, 3, 0, dpl_of(Q, 5, 3, 0))
    assert len(rows) == 2 and rows[1][1:] == [0, 0, 0, 0] + [_scalar(P, 0, 0, q) for q in Q[4:6]]
    # one P modulus and a power-of-two decomposition: a digit is one limb, row (i, j) carries P 2^(j pw2)
    dpl = dpl_of(Q, 6, 0, 16)
    assert dpl == [4] * 7                                                                          # 61-bit moduli: ceil(61 / 16)
    rows = table(Q, P[:1], 6, 0, 16, dpl)
    assert len(rows) == 28
    for i in range(7):
        for j in range(4):
            want = [0] * 7
            want[i] = _scalar(P[:1], j, 16, Q[i])
            assert rows[4 * i + j] == [0] + want
    # no P: the factor is 1, so the scalar is the Montgomery form of 2^(j pw2)
    rows = table(Q, [], 2, -1, 30, dpl_of(Q, 2, -1, 30))
    assert [r[1:] for r in rows[:3]] == [[(1 << 64) % Q[0], 0, 0], [(1 << 94) % Q[0], 0, 0], [(1 << 124) % Q[0], 0, 0]]
    # the restatement reads the same scalars
    for r, scal in zip(rows, mr._digit_scalars(Q, [], 2, -1, 30, dpl_of(Q, 2, -1, 30))):
        assert {k: v for k, v in enumerate(r[1:]) if v} == scal


def test_crs_rule(rh):
    """equal key and equal order give equal CRP words: the CRS is the keyed stream of the samplers, a CRP one Read under the next call counter"""
    from matrix_fhe_lattigo_amd.sampling import blake2b_final_block as final_block
    key = b"a common reference string"
    a, b = rh.multiparty.CRS(key), rh.multiparty.CRS(key)
    assert list(a.state) == list(b.state) and a.state != rh.multiparty.CRS(key + b"!").state
    assert [a.next_call() for _ in range(3)] == [b.next_call() for _ in range(3)] == [0, 1, 2]
    # the words of the stream as the device computes them (one compression after the key block) are sampling_restatement's
    for call, poly, row, group in [(0, 0, 0, 0), (1, 3, 5, 7), (2, 17, 1, 127)]:
        got = final_block(a.state, struct.pack("<5Q", call, poly, row, group, 0))
        assert tuple(got) == sr.block(key, call, poly, row, group, 0)
    # ... so a CRP row is sampling_restatement.uniform's: candidate = word & mask, accepted when < q
    q = int(tro.chain("REF")[1][0])
    want = sr.uniform(key, 1, 1, 32, [q])[0, 0]
    mask = (1 << (q - 1).bit_length()) - 1
    for i in range(32):
        t = 0
        while True:
            w = final_block(a.state, struct.pack("<5Q", 1, 0, 0, i // 8, t))[i % 8] & mask
            if w < q:
                break
            t += 1
        assert w == int(want[i])


def test_flooding_laws_refused_by_name(rh):
    with pytest.raises(rh.RingHipError, match="invalid distribution type"):
        rh.multiparty._flooding(("ternary", 0.5))
    with pytest.raises(rh.RingHipError, match="invalid distribution type"):
        rh.multiparty._flooding("gaussian")
    assert rh.multiparty._flooding(25.6) == (25.6, 6 * 25.6) and rh.multiparty._flooding((4.0, 19)) == (4.0, 19.0)
    assert set(rh.multiparty.FUSED_MULTIPARTY) == {"aggregate", "gadget_share", "relin_rounds", "keyswitch_share"}

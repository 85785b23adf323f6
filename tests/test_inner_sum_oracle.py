"""CPU: core/rlwe/inner_sum.go restated over the oracle pieces (tests/inner_sum_restatement.py) pinned to DECRYPTION under real keys, the statement
the reference's own test makes (core/rlwe/rlwe_test.go:1090-1136: PartialTracesSum(ct, batch, n) decrypts to sum_{i<n} sigma_{5^(i batch)}(m), the
standard deviation of the error within NoiseBound = log2 N).  tests/test_gpu_inner_sum.py compares the device path with the same restatement bit
for bit, on the cases below.

Chains (tests/test_rlwe_oracle.py): TAIL (N = 32, 7 | 4 limbs) and REF (the reference's own, N = 2^10, 5 | 2 limbs), keys made at the top level and
used at the top level and one below.  Cases (offset, n): (5, 7) the reference's own -- a first lazy rotation and a second one accumulated;
(1, 8) hoisted rotations only; (3, 5) one lazy rotation, odd n; (-1, 3) a negative offset (Replicate); (2, 6) an even n with one lazy rotation.

Measured log2 of the standard deviation of the error, the largest over the cases (bound in brackets): TAIL 3.88 [5.00], REF 4.43 [10.00];
Trace with a gap of 4: TAIL 3.15 [5.00], REF 3.73 [10.00]; bgv.InnerSum over both rows (n batchSize = N): TAIL 3.89 [6.00]."""
import functools

import numpy as np
import pytest

import inner_sum_restatement as isr
import rlwe_restatement as rr
import test_rlwe_oracle as t

SHAPES = [("TAIL", (0, 4)), ("REF", (0, 2))]
CASES = [(5, 7), (1, 8), (3, 5), (-1, 3), (2, 6)]
_ids = t._ids


def keys_for(name, setting, galEls):
    return {g: t.key(name, setting, "galois", g) for g in galEls if g != 1}


def case_elements(N, offset, n):
    """the Galois elements PartialTracesSum(offset, n) applies: a dry run of the restatement's loop"""
    used, state, i, j = [], False, 0, n
    while j > 0:
        if j & 1:
            k = (n - (n & ((2 << i) - 1))) * offset
            if k:
                used.append(isr.galois_element(N, k))
            else:
                state = True
        if not state:
            used.append(isr.galois_element(N, (1 << i) * offset))
        i, j = i + 1, j >> 1
    return used


@functools.lru_cache(maxsize=None)
def sum_case(name, setting, level, offset, n, tag="sum"):
    """(m, ct, restated PartialTracesSum of ct): shared with the GPU tests"""
    N, Q, P, _ = t.chain(name)
    m, ct, _ = t.fresh(name, tag, level)
    keys = keys_for(name, setting, case_elements(N, offset, n))
    return m, ct, isr.partial_traces_sum(N, Q, P[:setting[1]], ct, offset, n, keys)


def summed(m, N, offset, n):
    """sum_{i<n} sigma_{5^(i offset)}(m) on integers"""
    out = [0] * N
    for i in range(n):
        out = [a + b for a, b in zip(out, rr.automorphism_coeffs(m, isr.galois_element(N, i * offset)))]
    return out


def sum_error(name, level, out, want):
    N, Q, _, _ = t.chain(name)
    return rr.log2_std(rr.centered_diff(rr.phase(list(out), t.secrets(name)[0], Q), want, rr.prod(Q[:level + 1])))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_lazy_product_then_moddown_is_the_gadget_product(oracle, shape):
    name, setting = shape
    N, Q, P, levels = t.chain(name)
    P = P[:setting[1]]
    k = t.key(name, setting, "switch")
    for level in levels[:2]:
        a, want = t.switch_case(name, setting, level)
        accQ, accP = isr.lazy_product(N, Q, P, level, k.levelP, a, k.Q, k.P)
        got = isr.moddown(N, Q, P, level, k.levelP, accQ, accP)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "off%d-n%d" % c)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_partial_traces_sum_decrypts(oracle, shape, case):
    name, setting = shape
    offset, n = case
    N, Q, P, levels = t.chain(name)
    for level in levels[:2]:
        m, ct, out = sum_case(name, setting, level, offset, n)
        got = sum_error(name, level, out, summed(m, N, offset, n))
        t.report("partialtraces", name, setting, level, got, t.bound(N, 0))
        assert got <= t.bound(N, 0)


@functools.lru_cache(maxsize=None)
def inner_function_case(name, setting, level, offset, n, tag="sum"):
    N, Q, P, _ = t.chain(name)
    m, ct, _ = t.fresh(name, tag, level)
    keys = keys_for(name, setting, case_elements(N, offset, n))
    return m, ct, isr.inner_function_add(N, Q, P[:setting[1]], ct, offset, n, keys)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_inner_function_with_add_decrypts(oracle, shape):
    """InnerFunction with f = Add is the inner sum with one ModDown per rotation: the same message, the same bound"""
    name, setting = shape
    N, Q, P, levels = t.chain(name)
    for offset, n in CASES[:2]:
        m, ct, out = inner_function_case(name, setting, levels[0], offset, n)
        got = sum_error(name, levels[0], out, summed(m, N, offset, n))
        t.report("innerfunction", name, setting, levels[0], got, t.bound(N, 0))
        assert got <= t.bound(N, 0)


def test_partial_traces_sum_edges(oracle):
    name, setting = SHAPES[0]
    N, Q, P, levels = t.chain(name)
    m, ct, _ = t.fresh(name, "sum", levels[0])
    out = isr.partial_traces_sum(N, Q, P, ct, 3, 1, {})
    assert all(np.array_equal(a, b) for a, b in zip(out, ct))                            # n = 1 copies
    for offset, n in ((0, 4), (3, 0)):
        with pytest.raises(ValueError, match="partialtrace: invalid parameter"):
            isr.partial_traces_sum(N, Q, P, ct, offset, n, {})


@pytest.mark.parametrize("N", [32, 1024])
def test_galois_elements_for_inner_sum(rh, N):
    """the module function is the reference's formula, and lists every element PartialTracesSum applies -- plus, as in the reference, the
    rotation by 0 when the formula meets it and a last power of two the loop does not reach"""
    for offset, n in CASES + [(4, 4), (1, 2), (7, 1)]:
        ref = isr.galois_elements_for_inner_sum(N, offset, n)
        assert set(rh.rlwe.GaloisElementsForInnerSum(N, offset, n)) == ref
        assert set(rh.rlwe.GaloisElementsForReplicate(N, offset, n)) == isr.galois_elements_for_inner_sum(N, -offset, n)
        used = set(case_elements(N, offset, n)) if n > 1 else set()
        assert used <= ref
        plan = rh.rlwe.partial_traces_plan(N, offset, n) if n > 1 else []
        assert [g for kind, g, _ in plan if kind != rh.rlwe.CLOSE] == (case_elements(N, offset, n) if n > 1 else [])
    # exactly which rotations the reference lists beyond the ones it applies, case by case: the rotation by 0 once the formula's mask covers n,
    # and n itself (n a power of two, or n even) -- the list may not grow unnoticed
    extras = {(5, 7): {0}, (1, 8): {8}, (3, 5): {0}, (-1, 3): {0}, (2, 6): {0, 6}}
    for (offset, n), rot in extras.items():
        got = set(rh.rlwe.GaloisElementsForInnerSum(N, offset, n)) - set(case_elements(N, offset, n))
        assert got == {isr.galois_element(N, k * offset) for k in rot}, (offset, n)
    for logN in (0, 2, N.bit_length() - 3):
        assert rh.rlwe.GaloisElementsForTrace(N, logN) == isr.galois_elements_for_trace(N, logN)


@functools.lru_cache(maxsize=None)
def trace_case(name, setting, level, logN, tag="sum"):
    N, Q, P, _ = t.chain(name)
    m, ct, _ = t.fresh(name, tag, level)
    keys = keys_for(name, setting, isr.galois_elements_for_trace(N, logN))
    return m, ct, isr.trace(N, Q, P[:setting[1]], ct, logN, keys)


def trace_log(name):
    return t.chain(name)[0].bit_length() - 1 - 3                                          # a gap of 4: two automorphisms


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_trace_decrypts(oracle, shape):
    name, setting = shape
    N, Q, P, levels = t.chain(name)
    logN = trace_log(name)
    for level in levels[:2]:
        m, ct, out = trace_case(name, setting, level, logN)
        got = sum_error(name, level, out, isr.trace_coeffs(m, N, logN))
        t.report("trace", name, setting, level, got, t.bound(N, 0))
        assert got <= t.bound(N, 0)
    m, ct, _ = t.fresh(name, "sum", levels[0])
    same = isr.trace(N, Q, P[:setting[1]], ct, N.bit_length() - 2, {})                    # gap 1: a copy
    assert all(np.array_equal(a, b) for a, b in zip(same, ct))


BGV_ROWS = (4, 8)                                                                         # (batchSize, n) with n batchSize = N on TAIL


@functools.lru_cache(maxsize=None)
def bgv_rows_case(name, setting, level, tag="sum"):
    N, Q, P, _ = t.chain(name)
    b, n = BGV_ROWS
    assert b * n == N
    m, ct, _ = t.fresh(name, tag, level)
    keys = keys_for(name, setting, case_elements(N, b, n // 2) + [2 * N - 1])
    return m, ct, isr.bgv_inner_sum(N, Q, P[:setting[1]], ct, b, n, keys)


def test_bgv_inner_sum_over_both_rows(oracle):
    """n batchSize = N (schemes/bgv/evaluator.go:1541-1562): PartialTracesSum with n / 2, RotateRows, Add.  Two sums of key-switched ciphertexts,
    each within the bound on its standard deviation: their sum within one bit more."""
    name, setting = SHAPES[0]
    N, Q, P, levels = t.chain(name)
    b, n = BGV_ROWS
    level = levels[0]
    m, ct, out = bgv_rows_case(name, setting, level)
    half = summed(m, N, b, n // 2)
    want = [x + y for x, y in zip(half, rr.automorphism_coeffs(half, 2 * N - 1))]
    got = sum_error(name, level, out, want)
    t.report("bgv/innersum", name, setting, level, got, t.bound(N, 0) + 1)
    assert got <= t.bound(N, 0) + 1
    # the other branch is PartialTracesSum itself
    keys = keys_for(name, setting, case_elements(N, 2, 8))
    assert all(np.array_equal(a, c) for a, c in zip(isr.bgv_inner_sum(N, Q, P, ct, 2, 8, keys), isr.partial_traces_sum(N, Q, P, ct, 2, 8, keys)))
    for b_, n_, text in ((0, 4, "n <= 0 or batchSize <= 0"), (16, 4, "> #slots"), (3, 4, "does not divide")):
        with pytest.raises(ValueError, match="innersum: invalid parameter.*" + text):
            isr.bgv_inner_sum(N, Q, P, ct, b_, n_, {})

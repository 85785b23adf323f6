"""GPU: the device samplers (csrc/keygen.hip through matrix-fhe-lattigo_amd/sampling.py) bit for bit against tests/sampling_restatement.py, as
whole arrays.  Chain: one 61-bit limb, one 55-bit limb and the smallest NTT-friendly prime above 2^35, which rejects about half of its
candidates so that nearly every group of eight needs several blocks; N = 64 (one partial workgroup), N = 2^10 and N = 2^13 (1024 groups per row:
four workgroups along blockIdx.y, the launch shape of every larger ring); batches of 3 polys."""
import functools

import numpy as np
import pytest

import sampling_restatement as sr
from oracle import primes
from test_sampling_oracle import small_prime

pytestmark = pytest.mark.gpu
KEY = b"device sampler test key"


@functools.lru_cache(maxsize=None)
def chain(N):
    log = max(10, N.bit_length() - 1)                                     # primes = 1 modulo 2^(log + 1): N = 64 shares the chain of N = 2^10
    Q, _ = primes.gen_moduli(log + 1, [61, 55], [])
    return [int(q) for q in Q] + [small_prime(log)]


@pytest.fixture(scope="module", params=[64, 1024, 8192], ids=["N64", "N1024", "N8192"])
def ring(rh, request):
    r = rh.Ring(request.param, chain(request.param))
    yield r
    r.close()


@pytest.fixture(scope="module")
def want(ring):
    """the restated batch of call 0, computed once per ring"""
    return sr.uniform(KEY, 0, 3, ring.N, chain(ring.N))


def test_uniform_whole_batch_sub_blocks_and_successive_reads(rh, ring, want):
    prng = rh.rlwe.KeyedPRNG(KEY)
    us = rh.rlwe.UniformSampler(prng, ring)
    p = us.ReadNew(3)
    assert np.array_equal(p.numpy(), want)
    assert sr.uniform_row(KEY, 0, 0, 2, ring.N, chain(ring.N)[2])[1] >= 3           # the small prime's rows go through the multi-block path
    # the same polys as sub-blocks with the matching poly offsets, under the same call counter
    a, b = ring.NewPoly(1), ring.NewPoly(2)
    us.Read(a, call=0, poly0=0)
    us.Read(b, call=0, poly0=1)
    assert np.array_equal(np.concatenate([a.numpy(), b.numpy()]), want)
    # a second Read takes the next counter value
    q = us.ReadNew(3)
    assert prng.calls == 2 and not np.array_equal(q.numpy(), want)
    assert np.array_equal(q.numpy(), sr.uniform(KEY, 1, 3, ring.N, chain(ring.N)))
    # ... and at a lower level, with the rows counted from row0 (the P limbs of a QP poly)
    low = ring.AtLevel(1).NewPoly(3)
    us.read_rows(ring.AtLevel(1), low.ptr, 2, 3, 0, poly0=0, row0=0)
    assert np.array_equal(low.numpy(), want[:, :2])


def test_uniform_strided_write_into_a_key_table(rh, ring, want):
    """component 1 of a (rows, 2, limbs, N) table: rows stride 2 * limbs, component 0 untouched"""
    L, N = ring.L, ring.N
    table = rh.DevicePoly.from_numpy(ring, np.full((6, L, N), 7, dtype=np.uint64))
    us = rh.rlwe.UniformSampler(rh.rlwe.KeyedPRNG(KEY), ring)
    us.read_rows(ring, table.ptr + L * N * 8, 2 * L, 3, 0)
    got = table.numpy().reshape(3, 2, L, N)
    assert np.array_equal(got[:, 1], want) and (got[:, 0] == 7).all()


def test_gaussian_and_ternary(rh, ring):
    prng = rh.rlwe.KeyedPRNG(KEY)
    gs = rh.rlwe.GaussianSampler(prng, ring, 3.2, 19)
    assert gs.table == sr.gaussian_table(3.2, 19)
    e = gs.ReadNew(3)
    assert np.array_equal(e.numpy(), sr.gaussian(KEY, 0, 3, ring.N, gs.table))
    part = rh.rlwe.SmallPoly(ring, 2)
    gs.Read(part, call=0, poly0=1)
    assert np.array_equal(part.numpy(), sr.gaussian(KEY, 0, 2, ring.N, gs.table, poly0=1))
    wide = rh.rlwe.GaussianSampler(prng, ring, 40.0, 255.5)               # a table of 256 entries
    assert np.array_equal(wide.ReadNew(3).numpy(), sr.gaussian(KEY, 1, 3, ring.N, sr.gaussian_table(40.0, 255.5)))
    odd = rh.rlwe.GaussianSampler(prng, ring, 1.0, 2.7)                   # a bound whose fraction is above one half: magnitudes up to 3
    assert len(odd.table) == 4
    got = odd.ReadNew(3).numpy()
    assert np.array_equal(got, sr.gaussian(KEY, 2, 3, ring.N, sr.gaussian_table(1.0, 2.7))) and (ring.N < 1024 or np.abs(got).max() == 3)
    for P in (2 / 3, 0.5, 1.0):
        ts = rh.rlwe.TernarySampler(prng, ring, P=P)
        call = prng.calls
        assert np.array_equal(ts.ReadNew(3).numpy(), sr.ternary(KEY, call, 3, ring.N, ts.threshold))
    hw = rh.rlwe.TernarySampler(prng, ring, H=ring.N // 4).ReadNew(3).numpy()
    assert (np.count_nonzero(hw, axis=1) == ring.N // 4).all() and set(np.unique(hw)) == {-1, 0, 1}


def test_lift_and_accumulate(rh, ring):
    mods = chain(ring.N)
    rp = rh.Ring(ring.N, [0x1ffffffff6c80001])
    rng = np.random.default_rng(3)
    x = rng.integers(-19, 20, size=(3, ring.N)).astype(np.int32)
    x[0, :4] = [0, -(2 ** 31) + 1, 2 ** 31 - 1, -1]
    small = rh.rlwe.SmallPoly.from_numpy(ring, x)
    assert np.array_equal(small.numpy(), x)
    q, p = ring.NewPoly(3), rp.NewPoly(3)
    rh.rlwe.lift_small(ring, rp, small, q, p)
    wq, wp = sr.lift(x, mods), sr.lift(x, [0x1ffffffff6c80001])
    assert np.array_equal(q.numpy(), wq) and np.array_equal(p.numpy(), wp)
    base = np.stack([np.stack([rng.integers(0, m, size=ring.N, dtype=np.uint64) for m in mods]) for _ in range(3)])
    acc = rh.DevicePoly.from_numpy(ring, base)
    rh.rlwe.lift_small(ring, None, small, acc, accumulate=True)
    want = np.stack([np.stack([((base[k, j].astype(object) + wq[k, j].astype(object)) % m).astype(np.uint64) for j, m in enumerate(mods)]) for k in range(3)])
    assert np.array_equal(acc.numpy(), want)
    rp.close()


def test_refusals(rh, ring):
    prng = rh.rlwe.KeyedPRNG(KEY)
    with pytest.raises(rh.RingHipError, match="big-norm"):
        rh.rlwe.GaussianSampler(prng, ring, 1e6, 1024.0)
    with pytest.raises(rh.RingHipError, match="one of them"):
        rh.rlwe.TernarySampler(prng, ring)
    ci = rh.Ring(ring.N, [0x1fffffffffe00001], kind=rh.ConjugateInvariant)
    for cls in (rh.rlwe.UniformSampler, rh.rlwe.GaussianSampler):
        with pytest.raises(rh.RingHipError, match="standard rings only"):
            cls(prng, ci)
    with pytest.raises(rh.RingHipError, match="standard rings only"):
        rh.rlwe.TernarySampler(prng, ci, P=0.5)
    ci.close()
    L = rh.lib()
    p = ring.NewPoly(1)
    assert L.rh_sample_uniform(ring._h, 0, prng._state, 0, 0, 0, p.ptr, 0, 1) != 0 and b"out_rows" in L.rh_last_error()
    assert L.rh_sample_gaussian(ring._h, prng._state, 0, 0, p.ptr, 2000, p.ptr, 1) != 0 and b"big-norm" in L.rh_last_error()

"""CPU: what the entries of the blind rotation front end decide on the host -- the stride rh_blindrot_program reserves per job holds the longest
program BlindRotateCore can issue, and the argument checks that need no device."""
import random

import pytest


def _rows(N, n, rnd):
    """switched rows that make long programs: far-apart sets, every set non-empty, one set, the map's quirks, random odd values"""
    twoN, h = 2 * N, N // 2
    g = lambda k: pow(5, k, twoN)
    yield [g(i % h) if i & 1 else twoN - g(i % h) for i in range(n)]
    yield [g((i * 10 + 1) % h) for i in range(n)]
    yield [twoN - g((i * 11 + 5) % h) for i in range(n)]
    yield [g(1)] * n
    yield [0] * n
    yield [twoN - 1] * n
    for _ in range(4):
        yield [rnd.randrange(twoN) | 1 for _ in range(n)]


@pytest.mark.parametrize("N,n", [(64, 32), (64, 64), (64, 200), (256, 7), (1024, 512), (2048, 1024)])
def test_the_stride_holds_every_program(rh, N, n):
    L = rh.lib()
    stride = L.rh_blindrot_program_stride(N, n)
    assert stride == n + min(n, N - 1) + (N - 2) // 10 + 3
    rnd = random.Random(N + n)
    dlog = rh.blindrot.getGaloisElementInverseMap(N)
    for a in _rows(N, n, rnd):
        prog = rh.blindrot.blind_rotate_program(a, N, dlog)
        assert len(prog) < stride
        assert sum(1 for kind, _ in prog if kind == rh.blindrot.EXT) == n


def test_front_end_argument_errors_without_device(rh):
    L = rh.lib()
    assert L.rh_blindrot_mod_switch(None, 10, None, 0, None, None, 0, None) == -1 and b"null ring handle" in L.rh_last_error()
    assert L.rh_blindrot_program(None, 32, None, 0, None, 0, None, None, 0, None, None, None) == -1 and b"null ring handle" in L.rh_last_error()
    assert L.rh_blindrot_monomials(None, 0, None, 0, None) == -1 and b"null ring handle" in L.rh_last_error()
    assert L.rh_blindrot_program_stride(1, 4) == 0 and L.rh_blindrot_program_stride(64, -1) == 0

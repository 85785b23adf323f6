"""Restatement of the float64 path of schemes/ckks/encoder.go on standard rings: the reference's loops in numpy float64 on separate real and
imaginary arrays (element-wise ufuncs are single IEEE operations, nothing is fused), Python integers for the big paths, the ring transforms
through the CPU oracle.  tests/test_ckks_encoder_oracle.py pins it to the definition of the canonical embedding and to big-integer ground
truth; tests/test_gpu_ckks_encoder.py compares the device with it bit for bit.

  get_roots            GetRootsComplex128            utils.go:53-77
  rot_group            NewEncoder                    encoder.go:77-83
  special_ifft / fft   SpecialIFFTDouble / FFT       ckks_vector_ops.go:18-76 (the unrolled-8 variants compute the same butterflies)
  quantize_one         SingleFloat64ToFixedPointCRT  utils.go:171-234
  embed                embedDouble                   encoder.go:204-320 with NTTSparseAndMontgomery, core/rlwe/utils.go:187-245
  encode_coeffs        Encode, IsBatched = false     encoder.go:147-170
  to_float             scaleDown                     scaling.go:46-52, big.Float.Float64 / float64(uint64)
  decode               decodePublic, IsBatched       encoder.go:476-575, polyToComplexNoCRT / polyToComplexCRT :796-1003
  decode_coeffs        decodePublic, not batched     encoder.go:730-732, polyToFloatNoCRT / polyToFloatCRT :1006-1185
"""
import functools
import math

import numpy as np

from oracle import ring_oracle as orc

TWO64 = 1.8446744073709552e+19


def get_roots(m):
    """(re, im) of the m + 1 roots, by the reference's rule: one math.cos per entry of the first quarter, the rest by symmetry"""
    re, im = np.zeros(m + 1), np.zeros(m + 1)
    quarm = m >> 2
    angle = 2 * 3.141592653589793 / float(m)
    for i in range(quarm):
        re[i] = math.cos(angle * float(i))
    for i in range(quarm):
        im[quarm - i] += re[i]
    for i in range(1, quarm + 1):
        re[i + quarm], im[i + quarm] = -re[quarm - i], im[quarm - i]
        re[i + 2 * quarm], im[i + 2 * quarm] = -re[i], -im[i]
        re[i + 3 * quarm], im[i + 3 * quarm] = re[quarm - i], -im[quarm - i]
    re[m], im[m] = re[0], im[0]
    return re, im


def rot_group(m):
    out, five = [], 1
    for _ in range(m >> 2):
        out.append(five)
        five = five * 5 & (m - 1)
    return np.array(out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def tables(m):
    re, im = get_roots(m)
    rot = rot_group(m)
    for a in (re, im, rot):
        a.setflags(write=False)
    return re, im, rot


def bit_reverse(a, n):
    logn = n.bit_length() - 1
    idx = np.array([int(format(i, "0%db" % logn)[::-1], 2) if logn else 0 for i in range(n)], dtype=np.int64)
    return a[..., idx]


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def special_ifft(re, im, m):
    """values (..., n) as two float64 arrays -> new arrays"""
    rr, ri, rot = tables(m)
    re, im = np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)
    n = re.shape[-1]
    logn, logm = n.bit_length() - 1, m.bit_length() - 1
    assert n >= 1 and 1 << logn == n and m >= 4 * n
    lead = re.shape[:-1]
    for loglen in range(logn, 0, -1):
        ln, lenh, lenq = 1 << loglen, 1 << (loglen - 1), 4 << loglen
        gap, mask = logm - 2 - loglen, lenq - 1
        idx = (lenq - (rot[:lenh] & mask)) << gap
        xr, xi = re.reshape(lead + (n // ln, ln)), im.reshape(lead + (n // ln, ln))
        ur, ui, vr, vi = xr[..., :lenh], xi[..., :lenh], xr[..., lenh:], xi[..., lenh:]
        sr, si = ur + vr, ui + vi
        dr, di = ur - vr, ui - vi
        pr, pi = _cmul(dr, di, rr[idx], ri[idx])
        re = np.concatenate([sr, pr], axis=-1).reshape(lead + (n,))
        im = np.concatenate([si, pi], axis=-1).reshape(lead + (n,))
    # values[i] /= complex(float64(N), 0): Go's complex128 division (Smith's algorithm, |re m| >= |im m|)
    nf = np.float64(n)
    ratio = np.float64(0.0) / nf
    denom = nf + ratio * np.float64(0.0)
    e, f = (re + im * ratio) / denom, (im - re * ratio) / denom
    return bit_reverse(e, n), bit_reverse(f, n)


def special_fft(re, im, m):
    rr, ri, rot = tables(m)
    re, im = np.array(re, dtype=np.float64), np.array(im, dtype=np.float64)
    n = re.shape[-1]
    logn, logm = n.bit_length() - 1, m.bit_length() - 1
    assert n >= 1 and 1 << logn == n and m >= 4 * n
    lead = re.shape[:-1]
    re, im = bit_reverse(re, n), bit_reverse(im, n)
    for loglen in range(1, logn + 1):
        ln, lenh, lenq = 1 << loglen, 1 << (loglen - 1), 4 << loglen
        gap, mask = logm - 2 - loglen, lenq - 1
        idx = (rot[:lenh] & mask) << gap
        xr, xi = re.reshape(lead + (n // ln, ln)), im.reshape(lead + (n // ln, ln))
        ur, ui = xr[..., :lenh], xi[..., :lenh]
        vr, vi = _cmul(xr[..., lenh:], xi[..., lenh:], rr[idx], ri[idx])
        re = np.concatenate([ur + vr, ur - vr], axis=-1).reshape(lead + (n,))
        im = np.concatenate([ui + vi, ui - vi], axis=-1).reshape(lead + (n,))
    return re, im


# ---- quantizer ------------------------------------------------------------------------------------------------------------------------
def quantize_one(value, scale, moduli):
    """SingleFloat64ToFixedPointCRT as written: the words of one coefficient, one per modulus (Python ints, possibly unreduced or equal to q)"""
    value, scale = float(value), float(scale)
    if value == 0:
        return [0] * len(moduli)
    neg = value < 0
    if neg:
        scale *= -1
    value *= scale
    if value >= TWO64:
        # big.NewFloat(value).Add(0.5) at 53 bits is a no-op from 2^53 on; .Int is then the exact integer of the double
        x = int(value)
        return [q - x % q if neg else x % q for q in moduli]
    c = int(value + 0.5)
    if neg:
        return [q - c % q if c > q else q - c for q in moduli]
    return [c % q if c > 0x1fffffffffffffff else c for q in moduli]


def quantize(vals, scale, moduli):
    """(n,) floats -> (L, n) uint64"""
    out = np.zeros((len(moduli), len(vals)), dtype=np.uint64)
    for i, v in enumerate(vals):
        if v != 0:
            out[:, i] = np.array(quantize_one(v, scale, moduli), dtype=np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def subring(N, q):
    return orc.SubRingConsts(N, int(q))


def mform(words, q):
    return np.array([(int(w) << 64) % q for w in words], dtype=np.uint64)


def finish(coeffs, N, moduli, is_ntt, is_montgomery):
    """the oracle's NTT on the words as the quantizer left them (unreduced / equal to q where the reference leaves them so), then MForm"""
    out = coeffs
    if is_ntt:
        out = np.stack([orc.ntt(out[j], subring(N, q)) for j, q in enumerate(moduli)])
    if is_montgomery:
        out = np.stack([mform(out[j], q) for j, q in enumerate(moduli)])
    return out


def embed_coeffs(values, log_slots, scale, N, moduli):
    """embedDouble up to the quantizer plus the stride-gap spread: (L, N) words in the coefficient domain, standard form"""
    slots = 1 << log_slots
    values = np.asarray(values)
    assert values.ndim == 1 and len(values) <= slots <= N // 2
    re, im = np.zeros(slots), np.zeros(slots)
    re[:len(values)] = values.real
    im[:len(values)] = values.imag if np.iscomplexobj(values) else 0.0
    re, im = special_ifft(re, im, 2 * N)
    gap = N // (2 * slots)
    out = np.zeros((len(moduli), N), dtype=np.uint64)
    out[:, 0:slots * gap:gap] = quantize(re, scale, moduli)
    out[:, N // 2:N // 2 + slots * gap:gap] = quantize(im, scale, moduli)
    return out


def embed(values, log_slots, scale, N, moduli, is_ntt=True, is_montgomery=False):
    return finish(embed_coeffs(values, log_slots, scale, N, moduli), N, moduli, is_ntt, is_montgomery)


def encode_coeffs(values, scale, N, moduli, is_ntt=False):
    values = np.asarray(values, dtype=np.float64)
    assert len(values) <= N
    out = np.zeros((len(moduli), N), dtype=np.uint64)
    out[:, :len(values)] = quantize(values, scale, moduli)
    return finish(out, N, moduli, is_ntt, False)


# ---- decoder --------------------------------------------------------------------------------------------------------------------------
def to_float(x):
    """nearest double, ties to even, of a Python integer by the device's steps: top 64 bits, sticky bit, 53-bit rounding"""
    neg, a = x < 0, abs(x)
    bl = a.bit_length()
    if bl <= 64:
        mant, sh = a, 0
        if bl > 53:
            sh = bl - 53
            rem, mant = a & ((1 << sh) - 1), a >> sh
            half = 1 << (sh - 1)
            if rem > half or (rem == half and mant & 1):
                mant += 1
        r = math.ldexp(float(mant), sh)
    else:
        hi, sticky = a >> (bl - 64), a & ((1 << (bl - 64)) - 1)
        mant, rem = hi >> 11, hi & 0x7ff
        if rem > 0x400 or (rem == 0x400 and (sticky or mant & 1)):
            mant += 1
        try:
            r = math.ldexp(float(mant), bl - 53)
        except OverflowError:             # past the largest double: big.Float.Float64 gives the infinity, as ldexp does on the device
            r = math.inf
    return -r if neg else r


def crt(residues, moduli):
    Q = 1
    for q in moduli:
        Q *= q
    x = 0
    for r, q in zip(residues, moduli):
        Qi = Q // q
        x += int(r) * Qi * pow(Qi, -1, q)
    return x % Q, Q


def centred_double(residues, moduli):
    c, Q = crt(residues, moduli)
    if c >= Q >> 1:
        c -= Q
    return to_float(c)


def decode(poly, log_slots, scale, N, moduli, is_ntt=True, logprec=0, real_only=False):
    """poly (L, N) canonical words -> (re, im) of the slots"""
    slots, scale = 1 << log_slots, float(scale)
    gap = N // (2 * slots)
    if is_ntt:
        poly = np.stack([orc.intt(poly[j], subring(N, q)) for j, q in enumerate(moduli)])
    re = np.array([centred_double(poly[:, i * gap], moduli) for i in range(slots)]) / scale
    im = np.array([centred_double(poly[:, N // 2 + i * gap], moduli) for i in range(slots)]) / scale
    re, im = special_fft(re, im, 2 * N)
    if logprec != 0:
        p2 = math.pow(2.0, logprec)

        def rnd(a):                       # math.Round: half away from zero; |v| - floor|v| is exact, the sign of a zero survives
            return np.array([math.copysign(math.floor(abs(v)) + (1.0 if abs(v) - math.floor(abs(v)) >= 0.5 else 0.0), v) for v in a])
        re = rnd(re * p2) / p2
        im = np.zeros_like(im) if real_only else rnd(im * p2) / p2
    return re, im


def decode_coeffs(poly, scale, N, moduli, is_ntt=False):
    """plaintextToFloat at level 0 or at the ring's top level (moduli is then the whole chain, so the full-ring PolyToBigint of
    polyToFloatCRT sees the plaintext alone): (N,) doubles, every coefficient's centred integer over the scale; logprec plays no part"""
    if is_ntt:
        poly = np.stack([orc.intt(poly[j], subring(N, q)) for j, q in enumerate(moduli)])
    return np.array([centred_double(poly[:, i], moduli) for i in range(N)]) / float(scale)

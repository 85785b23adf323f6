"""Host-side mirror of core/rgsw/blindrot (LMKCDEY blind rotation, eprint 2022/198): a look-up table evaluated on LWE samples of an RLWE ciphertext.

  InitTestPolynomial, scaleUp, normalizeInv     core/rgsw/blindrot/blindrot.go:9-39, utils.go:22-53
  MemBlindRotationEvaluationKeySet, windowSize  keys.go:12-43        GaloisElements: the elements GenEvaluationKeyNew generates (:94-99)
  Evaluator.Evaluate                            evaluator.go:46-132  BlindRotateCore  :134-186   evaluateFromDiscreteLogSets  :189-229
  getGaloisElementInverseMap, getDiscreteLogSets, modSwitchRLWETo2NLvl, mulBySmallMonomialMod2N   :231-307, utils.go:10-20

  GenEvaluationKeyNew                           keys.go:45-108: the key set made on the device -- N_LWE RGSW ciphertexts in one launch sequence
                                                (rgsw.Encryptor, rh_rgsw_encrypt) and the eleven Galois keys (rlwe.KeyGenerator.GenGaloisKeysNew)

The accumulator loop -- per accumulator a strictly sequential chain of about N_LWE external products and N_BR / 10 key-switched automorphisms on
an 8 KiB polynomial -- runs as ONE kernel, one workgroup per accumulator (rh_blindrot_core, csrc/blindrot_kernels.hip.hpp), driven by the per-
accumulator program that blind_rotate_program derives from the discrete-log sets.  The kernel covers keys at levelQ = 0 without P and with a
power-of-two decomposition on standard rings of degree 2^6 .. 2^11; every other key setting takes the composed path, the reference's sequence of
ExternalProduct and Automorphism calls on one accumulator at a time.  Both walk the same program and give the same bits.  Everything outside the
loop (the monomials' transform, the product with the test polynomial, the first automorphism, the closing inverse transform) is one launch
sequence over all accumulators of a call.

Two properties of the reference's discrete-log map are reproduced, because the device path must give the reference's bits:
  * a[i] = 0 is not in the map; the Go map look-up returns 0, so index i lands in discrete-log set 0, exactly as if a[i] were 1;
  * a[i] = 2N - 1 is stored as -0 = 0 (getGaloisElementInverseMap writes map[2N - g^0] = -0), so it lands in set 0 as well, as if it were 1; the
    set "2N" that evaluator.go:163 looks up is therefore always empty.
An even non-zero a[i] raises, like the reference's panic.

The front end of Evaluate -- everything between the sample ciphertexts and that launch -- has a device twin (front_end=, FUSED_BLINDROT["front_end"]):
rh_blindrot_mod_switch (the exact integer rounding of modSwitchRLWETo2NLvl for every coefficient of every sample ciphertext, and b of every job),
rh_blindrot_program (one workgroup per job: a read through the reversal and the X^index map, the discrete-log sets, the steps in the kernel's
encoding at a fixed stride per job, the tail padded with ops the kernel skips) and rh_blindrot_monomials (the X^b rows).  No coefficient and no
program returns to the host.  It covers sample ciphertexts at level 0 in either domain, lists of them, and the kernel path of the loop; samples above
level 0 and the composed path stay on the host front end, which gives the same bits."""
import ctypes as C
import math

import numpy as np

from .ringhip import DevicePoly, RingHipError, Standard, U64P, _check, lib
from .rlwe import GaloisElement, GaloisGen, _view
from .schemes import Ciphertext
from . import rgsw

windowSize = 10                                                        # keys.go:12-15: parameter w of Algorithm 3

EXT, AUTO = "EXT", "AUTO"


OP_SKIP = 0x7fffffff                                                   # the padding of a device-built program: an op rh_blindrot_core skips
MAX_NLWE_DEVICE = 2048                                                 # what one workgroup of rh_blindrot_program holds


class DeviceInt32:
    """int32 words on the device -- the switched samples, b, the jobs, the programs of the device front end; numpy() brings them back (tests)"""

    def __init__(self, ring, shape, host=None):
        self.shape = tuple(int(x) for x in shape)
        self.size = int(np.prod(self.shape, dtype=np.int64))
        self._r0 = ring.AtLevel(0)
        self._words = max(-(-self.size // 2), 1)
        self._p = DevicePoly(self._r0, -(-self._words // self._r0.N), 1)
        self.ptr = self._p.ptr
        if host is not None:
            w = np.zeros(2 * self._words, dtype=np.int32)
            w[:self.size] = np.asarray(host, dtype=np.int32).reshape(-1)
            _check(lib().rh_dev_upload(self._r0._h, self.ptr, w.view(np.uint64).ctypes.data_as(U64P), self._words))

    def numpy(self):
        w = np.empty(self._words, dtype=np.uint64)
        _check(lib().rh_dev_download(self._r0._h, w.ctypes.data_as(U64P), self.ptr, self._words))
        return w.view(np.int32)[:self.size].reshape(self.shape).copy()


# ---- utils.go, blindrot.go ----------------------------------------------------------------------------------------------------------------------
def normalizeInv(x, a, b):
    return (x * (b - a) + b + a) / 2.0


def scaleUp(value, scale, Q):
    """utils.go:26-53: floor(|scale value| + 0.5) mod Q in float64 arithmetic, Q - that for a negative value (Q itself when that is 0, as written)"""
    neg = value < 0
    x = (-scale * value) if neg else (scale * value)
    res = int(math.floor(x + 0.5)) % int(Q)
    return int(Q) - res if neg else res


def InitTestPolynomial(g, scale, ringQ, a, b):
    """blindrot.go:12-39: the test polynomial of g on [a, b] at `scale` (a float), one poly at the level of `ringQ`, NTT domain"""
    N, L = ringQ.N, ringQ.level + 1
    F = np.zeros((1, L, N), dtype=np.uint64)
    interval = 2.0 / float(N)
    for j in range(L):
        qi = int(ringQ.moduli[j])
        for i in range((N >> 1) + 1):
            F[0, j, i] = scaleUp(g(normalizeInv(-interval * float(i), a, b)), scale, qi)
        for i in range((N >> 1) + 1, N):
            F[0, j, i] = scaleUp(-g(normalizeInv(interval * float(N - i), a, b)), scale, qi)
    p = DevicePoly.from_numpy(ringQ, F)
    ringQ.NTT(p, p)
    return p


def mulBySmallMonomialMod2N(mask, pol, n):
    """utils.go:10-20 on a list: pol * X^n modulo X^len + 1 and 2N, 0 <= n < len"""
    if n == 0:
        return list(pol)
    N = len(pol)
    out = list(pol[N - n:]) + list(pol[:N - n])
    for j in range(n):
        out[j] = -out[j] & mask
    return out


def GaloisElements(N):
    """the 11 elements of GenEvaluationKeyNew (keys.go:94-99): GaloisGen^1 .. GaloisGen^windowSize and 2N - GaloisGen"""
    return [GaloisElement(N, i + 1) for i in range(windowSize)] + [2 * int(N) - GaloisGen]


def getGaloisElementInverseMap(N):
    """evaluator.go:231-255: {+-GaloisGen^k mod 2N: +-k}, 0 <= k < N / 2, written in the reference's order (so 2N - 1 maps to -0 = 0)"""
    if N <= 0:
        raise RingHipError("invalid N: N=%d should be greater than zero" % N)
    twoN, mask = N << 1, (N << 1) - 1
    out, pw = {}, 1
    for i in range(N >> 1):
        out[pw] = i
        out[twoN - pw] = -i
        pw = (pw * GaloisGen) & mask
    return out


def getDiscreteLogSets(a, dlog):
    """evaluator.go:258-280: {k: [i ...]} with a[i] = +-GaloisGen^k.  A value the map does not hold reads as 0, like a Go map (a[i] = 0)."""
    sets = {}
    for i, ai in enumerate(a):
        ai = int(ai)
        if ai & 1 != 1 and ai != 0:
            raise RingHipError("getDiscreteLogSets: a[i] is not odd and thus not an element of Z_{2N}^{*} -> a[i] = (+/- 1) * g^{k} does not exist.")
        sets.setdefault(dlog.get(ai, 0), []).append(i)
    return sets


def blind_rotate_program(a, N, dlog=None):
    """BlindRotateCore (evaluator.go:134-186) with evaluateFromDiscreteLogSets (:189-229) as the list of steps it issues on the accumulator:
    (EXT, j): ExternalProduct with BlindRotationKeys[j]; (AUTO, g): Automorphism by the Galois element g.  The reference's code, statement by
    statement: the counter v of the first half-loop is carried into the second one (the look-up of set 2N at :163 passes 0 and drops its result),
    and `k == 1` holds in the second half-loop only."""
    dlog = getGaloisElementInverseMap(N) if dlog is None else dlog
    sets = getDiscreteLogSets(a, dlog)
    steps = []

    def from_sets(k, v):
        if k in sets:
            if v != 0:
                steps.append((AUTO, GaloisElement(N, v)))
                v = 0
            steps.extend((EXT, j) for j in sets[k])
        v += 1
        if v == windowSize or k == 1:
            steps.append((AUTO, GaloisElement(N, v)))
            v = 0
        return v

    Nhalf, v = N >> 1, 0
    for i in range(Nhalf - 1, 0, -1):
        v = from_sets(-i, v)
    from_sets(N << 1, 0)
    steps.append((AUTO, 2 * N - GaloisGen))
    for i in range(Nhalf - 1, 0, -1):
        v = from_sets(i, v)
    from_sets(0, 0)
    return steps


# ---- keys.go ------------------------------------------------------------------------------------------------------------------------------------
class MemBlindRotationEvaluationKeySet:
    """keys.go:31-43.  BlindRotationKeys: rgsw.Ciphertext per LWE secret coefficient, RGSW(X^{s_i}); AutomorphismKeys: {Galois element:
    rlwe.GadgetCiphertext} for GaloisElements(N_BR).  For the kernel every key is copied ONCE into two contiguous device tables,
    [key][k < 2][digit][component < 2][N] and [element][digit][component < 2][N]."""

    def __init__(self, BlindRotationKeys, AutomorphismKeys):
        self.BlindRotationKeys = list(BlindRotationKeys)
        self.AutomorphismKeys = dict(AutomorphismKeys)
        self._tables = None

    def GetBlindRotationKey(self, i):
        return self.BlindRotationKeys[i]

    def GetEvaluationKeySet(self):
        return self.AutomorphismKeys

    def kernel_refusal(self):
        """None when rh_blindrot_core takes this key set, else why it does not"""
        if not self.BlindRotationKeys:
            return "the key set holds no blind rotation key"
        k0 = self.BlindRotationKeys[0].Value[0]
        shape = (k0.LevelQ(), k0.LevelP(), k0.BaseTwoDecomposition, k0.digits)
        if k0.LevelP() >= 0:
            return "keys with a P modulus (LevelP = %d: single-P and hybrid keys) take the composed path" % k0.LevelP()
        if k0.LevelQ() != 0:
            return "keys above level 0 (LevelQ = %d) take the composed path" % k0.LevelQ()
        if k0.BaseTwoDecomposition <= 0:
            return "keys without a power-of-two decomposition take the composed path"
        every = [g for brk in self.BlindRotationKeys for g in brk.Value] + list(self.AutomorphismKeys.values())
        if any((g.LevelQ(), g.LevelP(), g.BaseTwoDecomposition, g.digits) != shape for g in every):
            return "the keys differ in their levels or decompositions"
        if len(self.AutomorphismKeys) > 16:
            return "more than 16 automorphism keys"
        return None

    def device_tables(self, ring):
        """(rgsw table, galois table, Galois elements in slot order, pw2, digits): built on first use, kept with the key set"""
        if self._tables is None:
            k0 = self.BlindRotationKeys[0].Value[0]
            rows = 2 * k0.digits                                       # polys of one gadget ciphertext
            r0 = ring.AtLevel(0)
            tk = DevicePoly(r0, len(self.BlindRotationKeys) * 2 * rows, 1)
            for j, brk in enumerate(self.BlindRotationKeys):
                for k in (0, 1):
                    r0.CopyLvl(brk.Value[k].Q, _view(tk, (2 * j + k) * rows, rows, r0))
            els = list(self.AutomorphismKeys)
            tg = DevicePoly(r0, max(len(els), 1) * rows, 1)
            for e, g in enumerate(els):
                r0.CopyLvl(self.AutomorphismKeys[g].Q, _view(tg, e * rows, rows, r0))
            self._tables = (tk, tg, els, k0.BaseTwoDecomposition, k0.digits)
        return self._tables


# ---- evaluator.go -------------------------------------------------------------------------------------------------------------------------------
class Evaluator:
    """blindrot.Evaluator (evaluator.go:16-44).  ringBR / ringLWE: the rings of the blind rotation and of the samples; ringP: the special modulus
    of the blind rotation keys, when they have one (composed path); NTTFlag: paramsBR.NTTFlag(), the domain of the results.

    fused (per call, or FUSED_BLINDROT when None): the accumulator loop as one kernel (True) or as the reference's ExternalProduct and Automorphism
    calls (False).  None uses the kernel where it covers the keys and the composed calls elsewhere; True refuses what the kernel does not cover."""

    # The kernel is the default: profiles/blindrot.json (tools/bench_ops.py blindrot) records it against the composed calls.
    # and the device front end against the host one: profiles/blindrot_front_end.json (tools/bench_blindrot_front_end.py), not slower at any size.
    FUSED_BLINDROT = {"core": True, "front_end": True}

    def __init__(self, ringBR, ringLWE, ringP=None, NTTFlag=True):
        for r, who in ((ringBR, "blind rotation"), (ringLWE, "LWE")):
            if r.kind != Standard:
                raise RingHipError("blindrot.Evaluator: the %s ring must be a standard ring (conjugate-invariant and 3N rings are not supported)" % who)
        self.ringBR, self.ringLWE, self.NTTFlag = ringBR, ringLWE, bool(NTTFlag)
        self.ev = rgsw.Evaluator(ringBR, ringP)
        self.galoisGenDiscreteLog = getGaloisElementInverseMap(ringBR.N)
        self._dlog_dev = self._flag_dev = None

    def close(self):
        self.ev.close()

    def _use_kernel(self, fused, BRK):
        want = self.FUSED_BLINDROT["core"] if fused is None else bool(fused)
        if not want:
            return False
        why = BRK.kernel_refusal()
        if why is None and not (6 <= self.ringBR.N.bit_length() - 1 <= 11):
            why = "ring degree %d outside 2^6 .. 2^11, what one workgroup holds" % self.ringBR.N
        if why is None:
            return True
        if fused is None:
            return False
        raise RingHipError("blindrot: the fused accumulator loop does not cover this setting: " + why)

    # -- the accumulator loop ----------------------------------------------------------------------------------------------------------------------
    def BlindRotateCore(self, a, acc, BRK, fused=None):
        """evaluator.go:134-186 on one accumulator (a degree-1, NTT-domain Ciphertext of one poly), in place"""
        self._core([a], acc, BRK, fused)

    def _core(self, a_list, acc, BRK, fused):
        """the loop on a batch: accumulator b of `acc` (npoly = len(a_list)) is rotated by a_list[b]"""
        if acc.Degree() != 1 or acc.IsNTT is not True:
            raise RingHipError("BlindRotateCore: the accumulator is a degree-1 ciphertext in the NTT domain (a coefficient-domain accumulator is not supported)")
        if acc.Value[0].npoly != len(a_list):
            raise RingHipError("BlindRotateCore: %d accumulators for %d vectors" % (acc.Value[0].npoly, len(a_list)))
        self._run([blind_rotate_program(a, self.ringBR.N, self.galoisGenDiscreteLog) for a in a_list], acc, BRK, fused)

    def _run(self, progs, acc, BRK, fused):
        """accumulator b of `acc` walks progs[b], a list of (EXT, key index) and (AUTO, Galois element) steps: in one launch, or call by call"""
        nkeys = len(BRK.BlindRotationKeys)
        for p in progs:
            for kind, x in p:
                if kind == EXT and x >= nkeys:
                    raise RingHipError("BlindRotateCore: BlindRotationKeys[%d] is missing" % x)
                if kind == AUTO and x not in BRK.AutomorphismKeys:
                    raise RingHipError("cannot apply Automorphism: GaloisKey[%d] is missing" % x)
        if self._use_kernel(fused, BRK):
            return self._core_kernel(progs, acc, BRK)
        self.ev.galois_keys = BRK.AutomorphismKeys                    # eval.Evaluator.WithKey(evk) (:143)
        one = len(progs) == 1
        for b, p in enumerate(progs):
            ct = acc if one else Ciphertext([_view(v, b, 1) for v in acc.Value], is_ntt=True)
            for kind, x in p:
                if kind == EXT:
                    self.ev.ExternalProduct(ct, BRK.BlindRotationKeys[x], ct)
                else:
                    self.ev.Automorphism(ct, x, ct)

    def _core_kernel(self, progs, acc, BRK):
        tk, tg, els, pw2, digits = BRK.device_tables(self.ringBR)
        slot = {g: e for e, g in enumerate(els)}
        off = np.zeros(len(progs) + 1, dtype=np.int32)
        ops = []
        for b, p in enumerate(progs):
            ops.extend(x if kind == EXT else -(slot[x] + 1) for kind, x in p)
            off[b + 1] = len(ops)
        words = np.concatenate([off, np.asarray(ops, dtype=np.int32)]).astype(np.int32)
        if words.size & 1:
            words = np.append(words, np.int32(0))
        r0 = self.ringBR.AtLevel(0)
        N = r0.N
        prog = DevicePoly(r0, -(-(words.size // 2) // N), 1)          # the program as device words: int32 offsets, then int32 ops
        _check(lib().rh_dev_upload(r0._h, prog.ptr, words.view(np.uint64).ctypes.data_as(U64P), words.size // 2))
        self._launch_core(prog.ptr, prog.ptr + 4 * off.size, len(ops), len(progs), acc, BRK)
        r0.sync()                                                      # `prog` is freed on return

    def _launch_core(self, off_ptr, ops_ptr, nops, nacc, acc, BRK):
        tk, tg, els, pw2, digits = BRK.device_tables(self.ringBR)
        r0 = self.ringBR.AtLevel(0)
        gel = (C.c_uint64 * max(len(els), 1))(*els)
        _check(lib().rh_blindrot_core(r0._h, pw2, digits, tk.ptr, len(BRK.BlindRotationKeys), tg.ptr, gel, len(els), off_ptr, ops_ptr, nops,
                                      acc.Value[0].ptr, acc.Value[1].ptr, nacc))

    # -- the front end on the device ----------------------------------------------------------------------------------------------------------------
    def _front_end(self, front_end, cts, BRK, fused):
        """whether this call takes the device front end: front_end (per call), else FUSED_BLINDROT["front_end"]; True refuses what it does not cover"""
        want = self.FUSED_BLINDROT["front_end"] if front_end is None else bool(front_end)
        if not want:
            return False
        why = None
        if any(c.Level() != 0 for c in cts):
            why = "sample ciphertexts above level 0 (more than one modulus) stay on the host front end"
        elif self.ringLWE.N > MAX_NLWE_DEVICE:
            why = "LWE degree %d above %d, what one workgroup holds" % (self.ringLWE.N, MAX_NLWE_DEVICE)
        elif not self._use_kernel(fused, BRK):
            why = "the composed path of the accumulator loop stays on the host front end (" + (BRK.kernel_refusal() or "fused = False") + ")"
        if why is None:
            return True
        if front_end is None:
            return False
        raise RingHipError("blindrot: the device front end does not cover this setting: " + why)

    def _dlog_pos(self):
        """the discrete-log table as rh_blindrot_program reads it, uploaded once per evaluator: for every value of Z_2N the step of BlindRotateCore's
        walk that visits its set -- k = -(N/2 - 1) .. -1, then N/2 - 1 .. 1, then 0 -- and -1 for an even non-zero value.  A value the map does
        not hold reads as set 0, like the Go map."""
        if self._dlog_dev is None:
            N = self.ringBR.N
            h = N >> 1
            pos = np.full(2 * N, -1, dtype=np.int32)
            for x in range(2 * N):
                if x == 0 or x & 1:
                    k = self.galoisGenDiscreteLog.get(x, 0)
                    pos[x] = k + h - 1 if k < 0 else (2 * h - 2 - k)
            self._dlog_dev = DeviceInt32(self.ringBR, pos.shape, pos)
        return self._dlog_dev

    def _jobs(self, ncts, indices):
        NLWE = self.ringLWE.N
        return [(ci, index) for ci in range(ncts) for index in sorted(indices) if 0 <= index < NLWE]

    def _samples_device(self, cts, indices):
        rl = self.ringLWE.AtLevel(0)
        for c in cts:
            if c.Degree() != 1 or c.Value[0].npoly != 1:
                raise RingHipError("blindrot.Evaluate: one degree-1 sample ciphertext at a time (pass a list for several)")
            if c.Level() != 0:
                raise RingHipError("blindrot: the device front end does not cover this setting: sample ciphertexts above level 0 (more than one "
                                   "modulus) stay on the host front end")
        x = DevicePoly(rl, 2 * len(cts), 1)
        for ci, c in enumerate(cts):
            for k, v in enumerate(c.Value):
                (rl.INTT if c.IsNTT else rl.CopyLvl)(v, _view(x, 2 * ci + k, 1))
        jobs = self._jobs(len(cts), indices)
        a2n = DeviceInt32(self.ringBR, (len(cts), 2, rl.N))
        b = DeviceInt32(self.ringBR, (len(jobs),))
        jd = DeviceInt32(self.ringBR, (len(jobs), 2), np.asarray(jobs, dtype=np.int32).reshape(-1, 2))
        _check(lib().rh_blindrot_mod_switch(rl._h, self.ringBR.N.bit_length() - 1, x.ptr, len(cts), a2n.ptr, jd.ptr, len(jobs), b.ptr))
        rl.sync()                                                      # `x` is freed on return; what follows runs on the blind rotation ring's stream
        return a2n, b, jobs, jd

    def lwe_samples_device(self, cts, indices):
        """The device twin of lwe_samples for a list of sample ciphertexts at level 0: (a2n, b, jobs).  a2n: DeviceInt32 (ncts, 2, N_LWE), both
        components switched to 2N (component 1 made odd); jobs: [(ciphertext, index)], ciphertext-major, indices ascending; b: DeviceInt32 (jobs,).
        The a vector of a job is not materialised: rh_blindrot_program reads a2n through the reversal and the X^index map."""
        a2n, b, jobs, _ = self._samples_device(list(cts), indices)
        return a2n, b, jobs

    def _program_device(self, a2n, ncts, jd, njobs, els, flag=None):
        N, NLWE = self.ringBR.N, self.ringLWE.N
        slot = {g: e for e, g in enumerate(els)}
        for g in GaloisElements(N):
            if g not in slot:
                raise RingHipError("cannot apply Automorphism: GaloisKey[%d] is missing" % g)
        slots = (C.c_int32 * 11)(*[slot[g] for g in GaloisElements(N)])
        stride = lib().rh_blindrot_program_stride(N, NLWE)
        off = DeviceInt32(self.ringBR, (njobs + 1,))
        ops = DeviceInt32(self.ringBR, (njobs, stride))
        if flag is None:                                               # Evaluate: a mod-switched c1 is odd or zero, and the stride holds every program
            if self._flag_dev is None:
                self._flag_dev = DeviceInt32(self.ringBR, (2,), [0, 0])
            flag = self._flag_dev
        _check(lib().rh_blindrot_program(self.ringBR.AtLevel(0)._h, NLWE, a2n.ptr, ncts, jd.ptr, njobs, self._dlog_pos().ptr, slots, stride, off.ptr,
                                         ops.ptr, flag.ptr))
        return off, ops

    def program_device(self, a2n, jobs, elements=None):
        """(offsets, ops), both DeviceInt32, of the jobs [(ciphertext, index)] over a2n (a DeviceInt32 of lwe_samples_device, or a host int array
        (ncts, 2, N_LWE)), as rh_blindrot_core reads them: ops[offsets[j] : offsets[j + 1]] is job j's program followed by OP_SKIP padding; op >= 0:
        ExternalProduct with that key, op < 0: Automorphism with key slot -op - 1 of `elements` (GaloisElements(N_BR) when None)."""
        if not isinstance(a2n, DeviceInt32):
            a2n = DeviceInt32(self.ringBR, np.shape(a2n), a2n)
        if len(a2n.shape) != 3 or a2n.shape[1:] != (2, self.ringLWE.N):
            raise RingHipError("program_device: a2n is (ncts, 2, N_LWE = %d) int32, got %s" % (self.ringLWE.N, a2n.shape))
        jobs = list(jobs)
        jd = DeviceInt32(self.ringBR, (len(jobs), 2), np.asarray(jobs, dtype=np.int32).reshape(-1, 2))
        fl = DeviceInt32(self.ringBR, (2,), [0, 0])
        off, ops = self._program_device(a2n, a2n.shape[0], jd, len(jobs), GaloisElements(self.ringBR.N) if elements is None else list(elements), fl)
        flag = int(fl.numpy()[0])
        if flag & 1:
            raise RingHipError("getDiscreteLogSets: a[i] is not odd and thus not an element of Z_{2N}^{*} -> a[i] = (+/- 1) * g^{k} does not exist.")
        if flag:
            raise RingHipError("rh_blindrot_program: internal error, flag %d" % flag)
        return off, ops

    def _evaluate_device(self, cts, testPolyWithSlotIndex, BRK, many):
        """Evaluate with the front end on the device: the samples, the programs and the monomials never leave it"""
        NLWE = self.ringLWE.N
        if len(BRK.BlindRotationKeys) < NLWE:                          # the host never sees the program: what it could name is checked up front
            raise RingHipError("BlindRotateCore: BlindRotationKeys[%d] is missing" % len(BRK.BlindRotationKeys))
        for g in GaloisElements(self.ringBR.N):
            if g not in BRK.AutomorphismKeys:
                raise RingHipError("cannot apply Automorphism: GaloisKey[%d] is missing" % g)
        rq = self.ringBR.AtLevel(0)
        N = rq.N
        a2n, b, jobs, jd = self._samples_device(cts, testPolyWithSlotIndex.keys())
        res = [dict() for _ in cts]
        if not jobs:
            return res if many else res[0]
        B = len(jobs)
        els = BRK.device_tables(self.ringBR)[2]
        off, ops = self._program_device(a2n, len(cts), jd, B, els)
        acc = Ciphertext([rq.NewPoly(B), rq.NewPoly(B)], is_ntt=True)
        _check(lib().rh_blindrot_monomials(rq._h, 0, b.ptr, B, acc.Value[1].ptr))          # Xb = MForm(X^b) (:108)
        self._accumulators(rq, acc, [testPolyWithSlotIndex[index] for _, index in jobs])
        self._launch_core(off.ptr, ops.ptr, ops.size, B, acc, BRK)
        rq.sync()                                                      # the programs are freed on return
        return self._results(rq, acc, [(ci, index) for ci, index in jobs], res, many)

    def _accumulators(self, rq, acc, polys):
        """(:109-113) on the batch: acc = (phi_{2N - g}(F * NTT(Xb)), 0), Xb in acc.Value[1] on entry"""
        N, L, B = rq.N, rq.level + 1, acc.Value[1].npoly
        rq.NTT(acc.Value[1], acc.Value[1])
        if L == 1 and all(p is polys[0] for p in polys):
            rq.MulByVectorMontgomery(acc.Value[1], polys[0], acc.Value[1])             # MulCoeffsMontgomery(testPoly, Xb) (:111), one vector for all
        else:
            F = rq.NewPoly(B)
            for j, p in enumerate(polys):
                rq.CopyLvl(p, _view(F, j, 1))
            rq.MulCoeffsMontgomery(F, acc.Value[1], acc.Value[1])
        rq.AutomorphismNTT(acc.Value[1], 2 * N - GaloisGen, acc.Value[0])               # (:112)
        rq.vec_op("ZERO", None, None, acc.Value[1])                                     # (:113)

    def _results(self, rq, acc, jobs, res, many):
        if not self.NTTFlag:                                                            # (:123-127)
            for v in acc.Value:
                rq.INTT(v, v)
        for j, (ci, index) in enumerate(jobs):
            res[ci][index] = Ciphertext([_view(v, j, 1) for v in acc.Value], is_ntt=self.NTTFlag)
        return res if many else res[0]

    # -- Evaluate ----------------------------------------------------------------------------------------------------------------------------------
    def modSwitchRLWETo2NLvl(self, level, coeffs, makeOdd):
        """evaluator.go:284-307 on the N_LWE big integers of a polynomial (PolyToBigint): round(x 2N / Q) mod 2N, an even non-zero result made odd"""
        Q = 1
        for q in self.ringLWE.moduli[:level + 1]:
            Q *= int(q)
        twoN = self.ringBR.N << 1
        out = []
        for x in coeffs:
            y, r = divmod(int(x) * twoN, Q)                            # bignum.DivRound on non-negative operands: half rounds up
            if 2 * r >= Q:
                y += 1
            y &= twoN - 1
            if makeOdd and y & 1 == 0 and y != 0:
                y ^= 1
            out.append(y)
        return out

    def lwe_samples(self, ct, indices):
        """The (a, b) of evaluator.go:62-103 for one sample ciphertext: {index: (a vector mod 2N, b mod 2N)} for the requested indices in ascending
        order -- inverse transform, mod switch, the reversal a_0, -a_{N-1}, ..., -a_1, and mulBySmallMonomialMod2N between successive indices"""
        level = ct.Level()
        rl = self.ringLWE.AtLevel(level)
        if ct.Degree() != 1 or ct.Value[0].npoly != 1:
            raise RingHipError("blindrot.Evaluate: one degree-1 sample ciphertext at a time (pass a list for several)")
        coeff = []
        for v in ct.Value:
            t = v
            if ct.IsNTT:
                t = rl.NewPoly(1)
                rl.INTT(v, t)
            coeff.append(rl.PolyToBigint(t))
        NLWE = rl.N
        mask = (self.ringBR.N << 1) - 1
        a2n = self.modSwitchRLWETo2NLvl(level, coeff[1], True)
        a = [a2n[0]] + [-a2n[NLWE - j] & mask for j in range(1, NLWE)]
        b2n = self.modSwitchRLWETo2NLvl(level, coeff[0], False)
        out, prev = {}, 0
        for index in sorted(indices):
            if not 0 <= index < NLWE:
                continue                                               # the reference's loop never reaches such a key of the map
            a = mulBySmallMonomialMod2N(mask, a, index - prev)
            prev = index
            out[index] = (list(a), b2n[index])
        return out

    def Evaluate(self, ct, testPolyWithSlotIndex, BRK, fused=None, front_end=None):
        """evaluator.go:46-132: {slot index: Ciphertext} with the blind rotation of every requested slot of `ct`, f(X) X^(b + <a, s>); a list of sample
        ciphertexts gives a list of such dicts.  testPolyWithSlotIndex: {index: test polynomial (InitTestPolynomial)}.  All accumulators of the call
        share every launch outside the loop, and the loop's one launch when the kernel runs it.  front_end (per call, or FUSED_BLINDROT["front_end"]
        when None): the mod switch, the programs and the monomials on the device (True) or on the host (False); same bits."""
        many = isinstance(ct, (list, tuple))
        cts = list(ct) if many else [ct]
        if self._front_end(front_end, cts, BRK, fused):
            return self._evaluate_device(cts, testPolyWithSlotIndex, BRK, many)
        level = BRK.GetBlindRotationKey(0).LevelQ()
        rq = self.ringBR.AtLevel(level)
        N, L = rq.N, level + 1
        jobs = []                                                      # (sample ciphertext, index, a, b)
        for ci, c in enumerate(cts):
            for index, (a, b) in self.lwe_samples(c, testPolyWithSlotIndex.keys()).items():
                jobs.append((ci, index, a, b))
        res = [dict() for _ in cts]
        if not jobs:
            return res if many else res[0]
        B = len(jobs)
        # Xb = MForm(NTT(X^b)) (:108-110): the monomial is written in Montgomery form and transformed (the transform is linear and canonical)
        xb = np.zeros((B, L, N), dtype=np.uint64)
        for j, (_, _, _, b) in enumerate(jobs):
            i = b & (2 * N - 1)
            for u in range(L):
                q = int(rq.moduli[u])
                r = (1 << 64) % q
                xb[j, u, i if i < N else i - N] = r if i < N else q - r
        acc = Ciphertext([rq.NewPoly(B), DevicePoly.from_numpy(rq, xb)], is_ntt=True)
        self._accumulators(rq, acc, [testPolyWithSlotIndex[index] for _, index, _, _ in jobs])
        self._core([a for _, _, a, _ in jobs], acc, BRK, fused)
        return self._results(rq, acc, [(ci, index) for ci, index, _, _ in jobs], res, many)


# ---- keys.go:45-108 --------------------------------------------------------------------------------------------------------------------------------
def GenEvaluationKeyNew(kgenBR, skBR, ringLWE, skLWE, levelQ=None, levelP=None, BaseTwoDecomposition=0, samples=None, fused=None):
    """keys.go:46-108: the blind rotation key set of the LWE secret skLWE under the blind rotation secret skBR, made on the device.  kgenBR: the
    rlwe.KeyGenerator of the blind rotation ring (its PRNG and error law are used).  The centred coefficients s_i of the LWE secret come from
    skLWE.coeffs, or from INTT + IMForm + centring when it has none (one N_LWE-word download).  The N_LWE ciphertexts RGSW(X^{s_i}) are ONE launch
    sequence of rgsw.Encryptor (chunked under keygen.SCRATCH_CAP), sharing the secret and one plaintext per distinct s_i (X^-1, X^0, X^1 for a
    ternary secret); the eleven Galois keys come from KeyGenerator.GenGaloisKeysNew.  samples: {"rgsw": {"a", "e"}, "galois": {"a", "e"}} in
    place of the PRNG (rgsw: key-major, the rows of Value[0] before those of Value[1]); fused: FUSED_KEYGEN when None."""
    from .keygen import centred_coeffs
    rq = kgenBR.ringQ
    if rq.kind != Standard or ringLWE.kind != Standard:
        raise RingHipError("blindrot.GenEvaluationKeyNew: standard rings only (conjugate-invariant and 3N rings are not supported)")
    levelQ, levelP, pw2 = kgenBR._levels(levelQ, levelP, BaseTwoDecomposition, False)
    N = rq.N
    s = [int(x) for x in centred_coeffs(skLWE)]
    values = sorted(set(s))
    rl = rq.AtLevel(levelQ)
    mono = np.zeros((len(values), levelQ + 1, N), dtype=np.uint64)    # ring.NewMonomialXi (ring/ring.go:408-430): X^i, -X^(i - N) for N <= i mod 2N
    for k, v in enumerate(values):
        i = v & (2 * N - 1)
        for u in range(levelQ + 1):
            mono[k, u, i if i < N else i - N] = 1 if i < N else int(rq.moduli[u]) - 1
    pt = DevicePoly.from_numpy(rl, mono)
    rl.NTT(pt, pt)                                                     # pt.IsNTT = true (:81-83)
    rl.MForm(pt, pt)                                                   # rgsw.Encryptor.Encrypt on a plaintext that is not in Montgomery form (encryptor.go:52-53)
    enc = rgsw.Encryptor(rq, kgenBR.ringP, skBR, xs=kgenBR.xs, xe=kgenBR.xe)
    enc.kg = kgenBR                                                    # one PRNG stream for the whole key set
    samples = samples or {}
    where = {v: k for k, v in enumerate(values)}
    brk = enc.rows(pt, [where[x] for x in s], levelQ, levelP, pw2, samples.get("rgsw"), fused)
    gks = kgenBR.GenGaloisKeysNew(GaloisElements(N), skBR, levelQ=levelQ, levelP=levelP, BaseTwoDecomposition=pw2, samples=samples.get("galois"), fused=fused)
    return MemBlindRotationEvaluationKeySet(brk, {int(g.GaloisElement): g for g in gks})

"""ckks.GetPrecisionStats and PrecisionStats (schemes/ckks/precision.go): the statistics of -log2 |have - want| over the slots, on the host, in the
reference's sequential float64 order, from the device Decode.

Kept as the reference writes it: errL2 = errReal^2 + errReal^2 (:133-134: the imaginary part is not in it), an error of zero counts as Log2Scale
(:146-156), the maxima start at 0 and the minima at 1e10, MAXLog2Prec is capped at Log2Scale, the median of an even count is the mean of the two
middle values except for two values (:370-377), the 500-bin CDF (:349-368) and String() (:47-75).
Log2Scale: the reference reads params.DefaultScale(); here it is `log2_scale`, by default the scale of `have` when it carries one."""
import math

import numpy as np

from .ringhip import RingHipError


class Stats:
    """(:43-45)"""

    def __init__(self, Real=0.0, Imag=0.0, L2=0.0):
        self.Real, self.Imag, self.L2 = Real, Imag, L2

    def __eq__(self, o):
        return isinstance(o, Stats) and (self.Real, self.Imag, self.L2) == (o.Real, o.Imag, o.L2)

    def __repr__(self):
        return "Stats(Real=%r, Imag=%r, L2=%r)" % (self.Real, self.Imag, self.L2)


_ROWS = ("MIN", "MAX", "AVG", "MED", "STD")


class PrecisionStats:
    """(:18-39)"""

    def __init__(self):
        for r in _ROWS:
            setattr(self, r + "Log2Prec", Stats())
            setattr(self, r + "Log2Err", Stats())
        self.Log2Scale = 0.0
        self.RealDist, self.ImagDist, self.L2Dist = [], [], []
        self.cdfResol = 0

    def String(self):
        bar = lambda l, m, r: l + "─" * 9 + m + ("─" * 7 + m) * 2 + "─" * 7 + r
        out = ["", bar("┌", "┬", "┐"), "│    Log2 │ REAL  │ IMAG  │ L2    │", bar("├", "┼", "┤")]
        for kind, label in (("Prec", "Prec"), ("Err", "Err ")):
            for r in _ROWS:
                s = getattr(self, "%sLog2%s" % (r, kind))
                out.append("│%s %s │ %5.2f │ %5.2f │ %5.2f │" % (r, label, s.Real, s.Imag, s.L2))
            out.append(bar("├", "┼", "┤") if kind == "Prec" else bar("└", "┴", "┘"))
        return "\n".join(out) + "\n"

    __str__ = String


def calcmedian(values):
    """(:370-377); sorts `values` in place, as the reference does"""
    values.sort()
    index = len(values) // 2
    if len(values) & 1 == 1 or index + 1 == len(values):
        return values[index]
    return (values[index - 1] + values[index]) / 2


def calcCDF(precs, resol=500):
    """(:349-368): [(Prec, Count)] * resol; a bin no value reaches keeps (0.0, 0)"""
    s = sorted(precs)
    lo, hi = s[0], s[-1]
    res = []
    for i in range(resol):
        cur = lo + float(i) * (hi - lo) / float(resol)
        hit = (0.0, 0)
        for count, p in enumerate(s):
            if p >= cur:
                hit = (cur, count)
                break
        res.append(hit)
    return res


def _log2(x):
    return math.log2(x) if x > 0 else -math.inf if x == 0 else math.nan


def precision_stats(want, have, log2_scale, computeDCF=False):
    """getPrecisionStats (:106-259) on two vectors of complex (or real) values"""
    want = np.asarray(want, dtype=np.complex128).reshape(-1)
    have = np.asarray(have, dtype=np.complex128).reshape(-1)
    if want.size == 0 or have.size < want.size:
        raise RingHipError("GetPrecisionStats: %d values to compare with %d" % (have.size, want.size))
    S = float(log2_scale)
    cols = ([], [], [])
    avg, mx, mn = [0.0] * 3, [0.0] * 3, [1e10] * 3
    for i in range(want.size):
        er = float(have[i].real) - float(want[i].real)
        ei = float(have[i].imag) - float(want[i].imag)
        l2 = er * er
        l2 = l2 + er * er                                          # (:133-134)
        vals = [-_log2(abs(er)), -_log2(abs(ei)), -_log2(math.sqrt(l2))]
        for k in range(3):
            v = S if math.isinf(vals[k]) else vals[k]
            cols[k].append(v)
            avg[k] += v
            mx[k] = max(mx[k], v)
            mn[k] = min(mn[k], v)
    n = float(want.size)
    avg = [a / n for a in avg]
    std = []
    for k in range(3):
        acc = 0.0
        for x in cols[k]:
            x -= avg[k]
            acc += x * x
        std.append(math.sqrt(acc / (n - 1)) if n > 1 else math.nan)
    p = PrecisionStats()
    dist = [list(c) for c in cols] if computeDCF else None        # the median sorts its columns in place (:206-208): the CDF sorts copies
    med = [calcmedian(c) for c in cols]
    p.MINLog2Prec, p.MAXLog2Prec = Stats(*mn), Stats(*[min(m, S) for m in mx])
    p.AVGLog2Prec, p.MEDLog2Prec, p.STDLog2Prec = Stats(*avg), Stats(*med), Stats(*std)
    p.MAXLog2Err = Stats(*[S - v for v in mn])
    p.MINLog2Err = Stats(*[S - min(m, S) for m in mx])
    p.AVGLog2Err, p.MEDLog2Err, p.STDLog2Err = Stats(*[S - v for v in avg]), Stats(*[S - v for v in med]), Stats(*std)
    p.Log2Scale = S
    if computeDCF:
        p.cdfResol = 500
        p.RealDist, p.ImagDist, p.L2Dist = (calcCDF(c, 500) for c in dist)
    return p


def GetPrecisionStats(encoder, decryptor, want, have, logprec=0, computeDCF=False, log2_scale=None):
    """(:80-82).  want: complex or real values, (slots,) or (nvec, slots).  have: a ciphertext (decrypted with `decryptor`), a plaintext, a
    DeviceValues or an array; ciphertexts and plaintexts go through the device DecodePublic(., logprec).  One PrecisionStats, or a list of nvec
    when `want` has two dimensions."""
    from .ckks import DeviceValues
    scale = getattr(have, "Scale", None)
    if hasattr(have, "Value"):
        pt = have
        if isinstance(have.Value, (list, tuple)) and len(have.Value) > 1:
            if decryptor is None:
                raise RingHipError("GetPrecisionStats: a ciphertext needs a decryptor")
            pt = decryptor.DecryptNew(have)
        vals = encoder.DecodePublic(pt, None, logprec)
    elif isinstance(have, DeviceValues):
        vals = have.numpy()
    else:
        vals = np.asarray(have)
    if log2_scale is None:
        if scale is None:
            raise RingHipError("GetPrecisionStats: log2_scale (the parameters' DefaultScale) must be given when `have` carries no scale")
        log2_scale = math.log2(scale.Float64() if hasattr(scale, "Float64") else float(scale))
    w = np.asarray(want)
    if w.ndim == 2:
        vals = np.asarray(vals).reshape(w.shape[0], -1)
        return [precision_stats(w[k], vals[k], log2_scale, computeDCF) for k in range(w.shape[0])]
    return precision_stats(w, np.asarray(vals).reshape(-1), log2_scale, computeDCF)

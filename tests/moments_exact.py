"""The exact velocity moments (include/pic1dp_hip.h pic1dp_hip_moments_exact) restated in numpy and Python
integers.  The terms are tests/moments_reference.py's -- the very float64 products of the kernel, a0 = wl q, b0 = (1 - wl) q,
a_k = a_(k-1) v, each rounded on its own.  Here every term t of power k becomes n = round_half_even(t 2^-e[k]) with
e[k] = kb + k kvm - 40, kb = charge_quantum + 52, kvm = ceil(log2 v_max); a term with |n| >= 2^44, or a NaN, is not summed but
counted per plane; the integers of a bin are added exactly; the total T is handed out as the normalised limbs hi = T >> 32
(floor), lo = T & (2^32 - 1), and as the double float(T) 2^e[k] (float(int): one rounding to nearest even).

Two evaluations: quantise_py / python_limbs in plain Python integers, marker by marker (the definition), and reference() in
numpy for the sizes of the GPU tests; tests/test_moments_exact_host.py holds the second against the first.  A helper of the
tests, not collected."""
import math

import numpy as np

import moments_reference as MR

LIMIT = 2 ** 44
SETS = MR.SETS


def ceil_log2(a):
    m, k = math.frexp(a)           # a = m 2^k, m in [0.5, 1)
    return k - 1 if m == 0.5 else k


def quanta(inp, ispecies=0):
    """e[0 ... 3] from the input alone; the bound B_s is the library's (pic1dp_amd.charge_quantum = ceil(log2 B_s) - 52)"""
    import pic1dp_amd
    kb = pic1dp_amd.charge_quantum(inp, ispecies) + 52
    kvm = ceil_log2(inp.v_max)
    return [kb + k * kvm - 40 for k in range(4)]


def quantise_py(t, e):
    """n = round_half_even(t 2^-e) in Python integers, or None: not summed (|n| >= 2^44, NaN, infinite)"""
    t = float(t)
    if t != t or t in (math.inf, -math.inf):
        return None
    num, den = t.as_integer_ratio()             # exact
    if e >= 0:
        den <<= e
    else:
        num <<= -e
    q, r = divmod(num, den)                     # floor, 0 <= r < den
    if 2 * r > den or (2 * r == den and (q & 1)):
        q += 1
    return q if abs(q) < LIMIT else None


def limbs_of(total):
    """(hi, lo) normalised: total = hi 2^32 + lo, 0 <= lo < 2^32"""
    return total >> 32, total & 0xFFFFFFFF


def to_double(total, e):
    """what moments_convert makes of a bin: the integer converted once, times 2^e"""
    return float(total) * math.ldexp(1.0, e)


def python_limbs(x, v, q, inp, e):
    """(totals [4][nx] Python ints, rejected [4]): the definition marker by marker on MR.python_moments' terms"""
    lists = MR.python_moments(x, v, q, inp)
    totals = [[0] * inp.nx for _ in range(4)]
    rejected = [0] * 4
    for k in range(4):
        for b in range(inp.nx):
            for t in lists[k][b]:
                n = quantise_py(t, e[k])
                if n is None:
                    rejected[k] += 1
                else:
                    totals[k][b] += n
    return totals, rejected


def quantise(t, e):
    """numpy: (n as float64 integers, summed-or-not); t 2^-e is exact (or so small that it rounds to 0 either way)"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        r = np.rint(np.ldexp(np.asarray(t, dtype=np.float64), -e))
        ok = np.abs(r) < float(LIMIT)           # (NaN compares false)
    return r, ok


def _set_totals(cell, ts, nx, e):
    """[4][nx] Python ints and [4] rejected counts for one weight set's terms"""
    totals, rejected = [], []
    for k in range(4):
        r, ok = quantise(ts[k], e[k])
        n = r[ok].astype(np.int64)
        c = cell[ok]
        rejected.append(int(np.count_nonzero(~ok)))
        # exact integer sums through float64 bincounts of the two halves: each half-sum stays below 2^53
        cnt = np.bincount(c, minlength=nx)
        assert cnt.max(initial=0) < 2 ** 20
        lo = np.bincount(c, weights=(n & 0xFFFFFFFF).astype(np.float64), minlength=nx)
        hi = np.bincount(c, weights=(n >> 32).astype(np.float64), minlength=nx)
        totals.append([(int(h) << 32) + int(l) for h, l in zip(hi.tolist(), lo.tolist())])
    return totals, rejected


def reference(x, v, p, w, inp, which=3, ispecies=0):
    """dict(e, limbs int64 (nsets, 4, 2, nx) normalised, totals [nsets][4][nx] Python ints, doubles {"total" / "pertb": (4, nx)},
    rejected int (nsets, 4), count (nx,) terms per bin) over the markers given (the valid ones)"""
    nx = inp.nx
    e = quanta(inp, ispecies)
    names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
    qs = [q for bit, q in ((1, p), (2, w)) if which & bit]
    limbs = np.zeros((len(names), 4, 2, nx), dtype=np.int64)
    rejected = np.zeros((len(names), 4), dtype=np.int64)
    doubles, totals_all, count = {}, [], None
    for j, (name, q) in enumerate(zip(names, qs)):
        cell, ts = MR.terms(x, v, q, inp)
        count = np.bincount(cell, minlength=nx)
        totals, rej = _set_totals(cell, ts, nx, e)
        totals_all.append(totals)
        rejected[j] = rej
        d = np.zeros((4, nx))
        for k in range(4):
            for b, t in enumerate(totals[k]):
                hi, lo = limbs_of(t)
                limbs[j, k, 0, b], limbs[j, k, 1, b] = hi, lo
                d[k, b] = to_double(t, e[k])
        doubles[name] = d
    return dict(e=e, limbs=limbs, totals=totals_all, doubles=doubles, rejected=rejected, count=count)


def in_range(ref):
    """the condition on a test's INPUTS: the definition itself sums every term"""
    return not np.any(ref["rejected"])

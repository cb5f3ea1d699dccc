"""The exact wave-particle power (include/pic1dp_hip.h pic1dp_hip_power_exact) restated in numpy and Python
integers.  The terms are tests/power_reference.py's terms() -- the very float64 products of the kernel: t_q = (v e) q, and for
a marker with bins the four products w00 t_q ... w11 t_q.  Here every term t becomes n = round_half_even(t 2^-e) with ONE
exponent for a call,
    e = max(kb + kvm + kE - 40, -1000),
kb = charge_quantum + 52, kvm = ceil(log2 v_max), kE = ceil(log2 max |E|) (0 for a field of zeros); a term with |n| >= 2^44,
or a NaN, is not summed but counted, per weight set, separately for bins and for rest; the integers of a bin (and of rest)
are added exactly; the total T is handed out as the normalised limbs hi = T >> 32 (floor), lo = T & (2^32 - 1), and as the
double float(T) 2^e (float(int): one rounding to nearest even).  The v-profile of a row is float(sum of the row's T) 2^e.

The quantisation is tests/moments_exact.py's (quantise, quantise_py, limbs_of, to_double).  A helper of the tests, not
collected."""
import numpy as np

import moments_exact as MX
import power_reference as PR

MIN_E = -1000
SETS = PR.SETS


def quantum(inp, max_abs_E, ispecies=0):
    """e of a call from the input and max |E| (finite, >= 0): the rule in Python"""
    import pic1dp_amd
    kb = pic1dp_amd.charge_quantum(inp, ispecies) + 52
    kvm = MX.ceil_log2(inp.v_max)
    kE = MX.ceil_log2(max_abs_E) if max_abs_E > 0.0 else 0
    return max(kb + kvm + kE - 40, MIN_E)


def set_len(inp):
    return 2 * inp.nx_opd * inp.nv_opd + 2


def pack(totals, rest):
    """one weight set's normalised limbs [hi plane | lo plane | rest hi | rest lo] from its totals (Python ints)"""
    his, los = zip(*(MX.limbs_of(t) for t in totals)) if totals else ((), ())
    rh, rl = MX.limbs_of(rest)
    return np.array(list(his) + list(los) + [rh, rl], dtype=np.int64)


def totals_of(limbs_set, nxv):
    """(bin totals, rest total) as Python ints from one set's limbs, normalised or not (lo read as signed int64 here: sums
    of normalised limbs over ranks stay far below 2^63)"""
    a = [int(t) for t in limbs_set.tolist()]
    return [a[b] * 2**32 + a[nxv + b] for b in range(nxv)], a[2 * nxv] * 2**32 + a[2 * nxv + 1]


def doubles_of(totals, rest, e, nxo, nvo):
    """what power_convert makes of a set's totals: dict(xv, v, rest) -- every total converted once, the v-profile from the
    integer row sums"""
    xv = np.array([MX.to_double(t, e) for t in totals]).reshape(nvo, nxo)
    v = np.array([MX.to_double(sum(totals[iv * nxo:(iv + 1) * nxo]), e) for iv in range(nvo)])
    return dict(xv=xv, v=v, rest=MX.to_double(rest, e))


def _int_sums(cell, n, nbins):
    """exact integer sums per bin through float64 bincounts of the two halves: each half-sum stays below 2^53"""
    cnt = np.bincount(cell, minlength=nbins)
    assert cnt.max(initial=0) < 2 ** 20
    lo = np.bincount(cell, weights=(n & 0xFFFFFFFF).astype(np.float64), minlength=nbins)
    hi = np.bincount(cell, weights=(n >> 32).astype(np.float64), minlength=nbins)
    return [(int(h) << 32) + int(l) for h, l in zip(hi.tolist(), lo.tolist())], cnt


def reference(x, v, p, w, E, inp, which=3, ispecies=0):
    """dict(e, limbs int64 (nsets, 2 nxv + 2) normalised, totals [nsets] lists of Python ints, rest [nsets] Python ints,
    doubles {"total" / "pertb": dict(xv, v, rest)}, rejected int (nsets, 2) (bins, rest), count {"name": (nvo, nxo) terms per
    bin}, rest_count {"name": int}) over the markers given (the valid ones) and the field E (finite)"""
    E = np.asarray(E, dtype=np.float64)
    assert np.all(np.isfinite(E))
    nxo, nvo = inp.nx_opd, inp.nv_opd
    nxv = nxo * nvo
    e = quantum(inp, float(np.max(np.abs(E))), ispecies)
    names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
    qs = [q for bit, q in ((1, p), (2, w)) if which & bit]
    limbs = np.zeros((len(names), 2 * nxv + 2), dtype=np.int64)
    rejected = np.zeros((len(names), 2), dtype=np.int64)
    out = dict(e=e, limbs=limbs, totals=[], rest=[], doubles={}, rejected=rejected, count={}, rest_count={})
    for j, (name, q) in enumerate(zip(names, qs)):
        cell, t, rt = PR.terms(x, v, q, E, inp)
        r, ok = MX.quantise(t, e)
        totals, cnt = _int_sums(cell[ok], r[ok].astype(np.int64), nxv)
        rr, rok = MX.quantise(rt, e)
        rest = sum(int(a) for a in rr[rok].astype(np.int64).tolist())
        rejected[j] = (np.count_nonzero(~ok), np.count_nonzero(~rok))
        limbs[j] = pack(totals, rest)
        out["totals"].append(totals), out["rest"].append(rest)
        out["doubles"][name] = doubles_of(totals, rest, e, nxo, nvo)
        out["count"][name] = cnt.reshape(nvo, nxo)
        out["rest_count"][name] = int(np.count_nonzero(rok))
    return out


def in_range(ref):
    """the condition on a test's INPUTS: the definition itself sums every term"""
    return not np.any(ref["rejected"])


def python_limbs(x, v, q, E, inp, e):
    """(bin totals, rest total, rejected [bins, rest]) in plain Python integers, marker by marker, on PR.python_power's terms"""
    bins, rest = PR.python_power(x, v, q, E, inp)
    rejected = [0, 0]
    totals = []
    for lst in bins:
        s = 0
        for t in lst:
            n = MX.quantise_py(t, e)
            if n is None:
                rejected[0] += 1
            else:
                s += n
        totals.append(s)
    rs = 0
    for t in rest:
        n = MX.quantise_py(t, e)
        if n is None:
            rejected[1] += 1
        else:
            rs += n
    return totals, rs, rejected

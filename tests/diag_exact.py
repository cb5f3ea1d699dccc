"""The exact diagnostics sum (kind 1 of include/pic1dp_hip.h set_diag_sum) restated in numpy and
Python integers: the terms of the pass in float64 as the reference forms them (cells and weights from
diag_reference.bins), each rounded once to whole quanta with np.rint, the integers of a bin summed exactly, the total
converted once (float(int): round to nearest even) and scaled by 2^e; the v histograms as the integer row sums of the
(x, v) planes.  A helper of the tests, not collected."""
import math

import numpy as np

import diag_reference as dr

HIST_LIMIT = 44      # a histogram term of 2^44 quanta or more is not summed
KIN_LIMIT = 62       # ... a kinetic term of 2^62 or more
NAMES = ("markr", "total", "pertb")


def quantise(t, e, limit):
    """(n, kept): n = rint(t 2^-e) as int64 for the terms with |n| < 2^limit (NaN is not kept)"""
    q = np.rint(np.asarray(t, dtype=np.float64) * 2.0 ** -e)
    with np.errstate(invalid="ignore"):
        kept = np.abs(q) < 2.0 ** limit
    return q[kept].astype(np.int64), kept


def _bin_sums(idx, n, nbins):
    """Python-int sums of the int64 terms n per bin: the two 32-bit halves through np.bincount (float64 weights below
    2^32, fewer than 2^21 terms per bin: exact), joined as Python integers"""
    lo = np.bincount(idx, weights=(n & 0xffffffff).astype(np.float64), minlength=nbins)
    hi = np.bincount(idx, weights=(n >> 32).astype(np.float64), minlength=nbins)
    return [(int(h) << 32) + int(l) for h, l in zip(hi, lo)]


def to_double(n, e):
    return math.ldexp(float(n), e)


def exact(x, v, p, w, np_valid, lx, v_max, nx_opd, nv_opd, deltaf, e):
    """the definition for one species' slots: the first np_valid are its markers (histograms and kinetic sums), the rest
    its tail slots (kinetic sums only).  e: the six log2 quanta (diag_quanta).  Returns dict(raw = the six planes as
    ptcldist(finish=False) returns them, sums = energy_sums, ints = the planes' and sums' integers, rejected = terms
    not summed per plane / sum)"""
    x, v, p, w = (np.asarray(a, dtype=np.float64) for a in (x, v, p, w))
    nxv = nx_opd * nv_opd
    rejected = [0] * 6
    ints = {}
    # kinetic sums over every slot
    v2 = v * v
    terms = (v2, v2 * p, v2 * w) if deltaf else (v2, v2 * p)
    sums = []
    for k, t in enumerate(terms):
        n, kept = quantise(t, e[3 + k], KIN_LIMIT)
        rejected[3 + k] = int(np.count_nonzero(~kept))
        tot = sum(int(a) for a in n)
        ints["kin%d" % k] = tot
        sums.append(to_double(tot, e[3 + k]))
    if not deltaf:
        sums.append(sums[1])
    # histograms over the markers
    xm, vm, pm, wm = x[:np_valid], v[:np_valid], p[:np_valid], w[:np_valid]
    inside, ix, ixr, iv, ivu, sx, sv = dr.bins(xm, vm, lx, v_max, nx_opd, nv_opd)
    pm, wm = pm[inside], wm[inside]
    sxr, svu = 1.0 - sx, 1.0 - sv
    cells = np.concatenate([iv * nx_opd + ix, ivu * nx_opd + ix, iv * nx_opd + ixr, ivu * nx_opd + ixr])
    wts = np.concatenate([sx * sv, sx * svu, sxr * sv, sxr * svu])
    raw = {}
    planes = (wts, wts * np.tile(pm, 4), wts * np.tile(wm, 4) if deltaf else None)
    for k, t in enumerate(planes):
        if t is None:
            tot = [0] * nxv
        else:
            n, kept = quantise(t, e[k], HIST_LIMIT)
            rejected[k] = int(np.count_nonzero(~kept))
            tot = _bin_sums(cells[kept], n, nxv)
        ints[NAMES[k] + "_xv"] = tot
        raw[NAMES[k] + "_xv"] = np.array([to_double(n, e[k]) for n in tot])
        rows = [sum(tot[r * nx_opd:(r + 1) * nx_opd]) for r in range(nv_opd)]      # the v histograms: integer row sums
        ints[NAMES[k] + "_v"] = rows
        raw[NAMES[k] + "_v"] = np.array([to_double(n, e[k]) for n in rows])
    return dict(raw=raw, sums=np.array(sums), ints=ints, rejected=rejected)


def limbs_of(ints, nxv):
    """the integers of `exact` as the library's limbs: [3 planes][2][nxv] (hi row, lo row) then [3 sums][2]"""
    out = np.zeros(6 * nxv + 6, dtype=np.int64)
    for k, name in enumerate(NAMES):
        for i, n in enumerate(ints[name + "_xv"]):
            out[2 * k * nxv + i] = n >> 32
            out[(2 * k + 1) * nxv + i] = n & 0xffffffff
    for k in range(3):
        n = ints.get("kin%d" % k, 0)
        out[6 * nxv + 2 * k] = n >> 32
        out[6 * nxv + 2 * k + 1] = n & 0xffffffff
    return out

"""The velocity moments on the field grid (include/pic1dp_hip.h pic1dp_hip_moments) restated in numpy: cells and left
weights from tests/exact_charge.py cells() (the deposit's wrap and cell, ix == nx folded to 0), the right-hand cell
ir = (ix + 1) mod nx, and the terms in the stated order -- a0 = wl q, b0 = (1 - wl) q, a_k = a_(k-1) v, every product
rounded on its own -- so that they are the kernel's terms bit for bit.  Per bin: the exact sum of the float64 terms
(math.fsum: correctly rounded), the sum of their magnitudes and their number.

The bound on an FP64 sum in any order through at most one LDS copy per workgroup: n_b terms of a bin reach the result
through at most n_b + workgroups additions (a workgroup's terms into its copy, the copies into the global plane), each
with a relative error of at most 2^-53 of a partial sum that never exceeds the sum of magnitudes:
    |got - exact| <= (n_b + workgroups) 2^-53 sum |terms| (1 + 2^-20)
(the last factor covers the second-order terms and the rounding of the sum of magnitudes itself).  Nothing is measured
for it.  A helper of the tests, not collected."""
import math

import numpy as np

from exact_charge import cells

U = 2.0 ** -53
SETS = ("total", "pertb")      # the weights p, the weights w


def terms(x, v, q, inp):
    """(cell [2 n], [4] term arrays [2 n]): the left-hand terms a_k of every marker, then the right-hand terms b_k"""
    x, v, q = (np.asarray(a, dtype=np.float64) for a in (x, v, q))
    _, ix, wl = cells(x, inp)
    ir = (ix + 1) % inp.nx
    a = wl * q
    b = (1.0 - wl) * q
    out = [np.concatenate([a, b])]
    for _ in range(3):
        a = a * v
        b = b * v
        out.append(np.concatenate([a, b]))
    return np.concatenate([ix, ir]), out


def _exact_bins(cell, t, nx):
    """the exact sum of the terms of every bin, rounded once (math.fsum)"""
    order = np.argsort(cell, kind="stable")
    ts = t[order].tolist()
    ends = np.cumsum(np.bincount(cell, minlength=nx)).tolist()
    out = np.zeros(nx)
    lo = 0
    for b, hi in enumerate(ends):
        if hi > lo:
            out[b] = math.fsum(ts[lo:hi])
        lo = hi
    return out


def reference(x, v, p, w, inp, which=3):
    """{"total": ..., "pertb": ...} for the sets of `which`, each dict(exact (4, nx), abs (4, nx), count (nx,)) over the
    markers given (the valid ones: the caller cuts the tail off)"""
    nx = inp.nx
    out = {}
    for bit, name, q in ((1, "total", p), (2, "pertb", w)):
        if not which & bit:
            continue
        cell, ts = terms(x, v, q, inp)
        out[name] = dict(exact=np.stack([_exact_bins(cell, t, nx) for t in ts]),
                         abs=np.stack([np.bincount(cell, weights=np.abs(t), minlength=nx) for t in ts]),
                         count=np.bincount(cell, minlength=nx))
    return out


def bincount_sums(x, v, q, inp):
    """(4, nx): np.bincount sums of the same terms (float64 additions in marker order) -- a second summation of the very
    terms, for sizes at which the exact sum would take too long"""
    cell, ts = terms(x, v, q, inp)
    return np.stack([np.bincount(cell, weights=t, minlength=inp.nx) for t in ts])


def workgroups(np_markers, num_cu=256):
    """workgroups of a pass over np_markers markers (launch_policy.cpp moments_plan): one per CU, never more than the
    marker pairs fill with 1024 threads; num_cu = 256 bounds every device the library runs on"""
    return max(1, min(num_cu, ((int(np_markers) >> 1) + 1023) // 1024))


def bound(ref_set, nworkgroups, additions=None):
    """(4, nx): the bound above for one set of reference(); additions: the additions a bin's terms pass through, if not
    count + workgroups (np.bincount: count)"""
    n = ref_set["count"] + nworkgroups if additions is None else additions
    return n[None, :] * U * ref_set["abs"] * (1.0 + 2.0 ** -20)


def python_moments(x, v, q, inp):
    """[4][nx] lists of the terms of every bin, marker by marker in plain Python floats (the self-check of the numpy path)"""
    nx, lx = inp.nx, inp.lx
    out = [[[] for _ in range(nx)] for _ in range(4)]
    for xi, vi, qi in zip(map(float, x), map(float, v), map(float, q)):
        px = math.fmod(xi, lx)
        if px < 0.0:
            px = px + lx
        sx = px / lx * float(nx)
        fl = math.floor(sx)
        wl = 1.0 - (sx - fl)
        ix = int(fl) if fl < nx else 0
        ir = 0 if ix + 1 == nx else ix + 1
        a = wl * qi
        b = (1.0 - wl) * qi
        for k in range(4):
            if k > 0:
                a = a * vi
                b = b * vi
            out[k][ix].append(a)
            out[k][ir].append(b)
    return out

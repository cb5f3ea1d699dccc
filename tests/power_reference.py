"""The velocity-resolved wave-particle power on the output grid (include/pic1dp_hip.h pic1dp_hip_power) restated in numpy.

Per marker: the wrapped position, the field cell and the left weight come from tests/exact_charge.py cells() (the deposit's
wrap and cell, ix == nx folded to 0), the right-hand cell is ir = (ix + 1) mod nx, and
    e = E[ix] * wl;  e = e + E[ir] * (1.0 - wl);  c = v * e;  t_q = c * q
every product and sum rounded on its own, so that t_q is the kernel's term bit for bit.  The bins are a numpy restatement of
the output grid's stencil (pic1dp_amd/csrc/device_diag.hpp dist_stencil; src/pic1dp_output.F90:239-315) with its IEEE
divisions px / lx and (v + v_max) / (v_max * 2.0) and its two edge rules: the x cell nx_opd folds to 0 (and the right-hand
neighbour of the last x cell is cell 0), and the top v row keeps a marker whose upper row would carry weight 0.  A marker
with |v| >= v_max has no bins: its term goes to `rest`.

Per bin (and for rest): the exact sum of the float64 terms (math.fsum: correctly rounded), the sum of their magnitudes and
their number.

The bound.  The n_b terms of a bin reach the result through additions of two kinds: a term into a workgroup's LDS copy
(at most n_b of them in all, the first into a zero), and a workgroup's copy into the global plane (at most `workgroups`).
Every addition rounds its result with a relative error of at most 2^-53, and no partial sum exceeds the sum of the
magnitudes S of the bin's terms, so
    |got - exact| <= (n_b + workgroups) 2^-53 S (1 + 2^-20),
the last factor covering the second-order terms and the rounding of S itself.  `rest` goes through per-thread register
sums, wave shuffles, sixteen LDS partials and one global atomic per workgroup: additions of an exact zero are exact, a tree
over n_r non-zero leaves has at most n_r - 1 additions of two non-zero operands, and the global word takes one per
workgroup -- the same bound with n_b = n_r.  Nothing is measured for it.  A helper of the tests, not collected."""
import math

import numpy as np

from exact_charge import cells

U = 2.0 ** -53
SETS = ("total", "pertb")      # the weights p, the weights w


def gather(x, v, E, inp):
    """(px, c = v * e, ix, ir, wl) per marker: the push's gather at the wrapped position"""
    x, v, E = (np.asarray(a, dtype=np.float64) for a in (x, v, E))
    px, ix, wl = cells(x, inp)
    ir = (ix + 1) % inp.nx
    e = E[ix] * wl
    e = e + E[ir] * (1.0 - wl)
    return px, v * e, ix, ir, wl


def stencil(px, v, inp):
    """(has bins [n] bool, cells [4][n] (c00, c01, c10, c11; 0 where no bins), weights [4][n])"""
    nxo, nvo, lx, vmax = inp.nx_opd, inp.nv_opd, inp.lx, inp.v_max
    px, v = np.asarray(px, dtype=np.float64), np.asarray(v, dtype=np.float64)
    has = ~(np.abs(v) >= vmax)
    vv = np.where(has, v, 0.0)
    sx = px / lx * float(nxo)
    fx = np.floor(sx)
    ix = fx.astype(np.int64)
    sx = 1.0 - (sx - fx)
    ix = np.where(ix == nxo, 0, ix)
    sv = (vv + vmax) / (vmax * 2.0) * float(nvo - 1)
    fv = np.floor(sv)
    iv = fv.astype(np.int64)
    sv = 1.0 - (sv - fv)
    assert np.all((ix >= 0) & (ix < nxo)) and np.all((iv >= 0) & (iv < nvo))
    ivu = np.where(iv + 1 < nvo, iv + 1, iv)
    ixr = np.where(ix + 1 > nxo - 1, 0, ix + 1)
    sxr, svu = 1.0 - sx, 1.0 - sv
    cs = [iv * nxo + ix, ivu * nxo + ix, iv * nxo + ixr, ivu * nxo + ixr]
    ws = [sx * sv, sx * svu, sxr * sv, sxr * svu]
    return has, [np.where(has, c, 0) for c in cs], ws


def terms(x, v, q, E, inp):
    """(cell [4 m], term [4 m], rest terms [r]) of one weight set: the four products w * t_q of the m markers with bins,
    corner by corner, and the t_q of the r markers without"""
    q = np.asarray(q, dtype=np.float64)
    px, c, _, _, _ = gather(x, v, E, inp)
    t = c * q
    has, cs, ws = stencil(px, v, inp)
    return (np.concatenate([cc[has] for cc in cs]), np.concatenate([(w * t)[has] for w in ws]), t[~has])


def _exact_bins(cell, t, n):
    """the exact sum of the terms of every bin, rounded once (math.fsum)"""
    order = np.argsort(cell, kind="stable")
    ts = t[order].tolist()
    ends = np.cumsum(np.bincount(cell, minlength=n)).tolist()
    out = np.zeros(n)
    lo = 0
    for b, hi in enumerate(ends):
        if hi > lo:
            out[b] = math.fsum(ts[lo:hi])
        lo = hi
    return out


def reference(x, v, p, w, E, inp, which=3):
    """{"total": ..., "pertb": ...} for the sets of `which`, each dict(exact, abs (nv_opd, nx_opd), count (nv_opd, nx_opd),
    rest dict(exact, abs, count)) over the markers given (the valid ones: the caller cuts the tail off)"""
    nxo, nvo = inp.nx_opd, inp.nv_opd
    nxv = nxo * nvo
    out = {}
    for bit, name, q in ((1, "total", p), (2, "pertb", w)):
        if not which & bit:
            continue
        cell, t, rt = terms(x, v, q, E, inp)
        out[name] = dict(exact=_exact_bins(cell, t, nxv).reshape(nvo, nxo),
                         abs=np.bincount(cell, weights=np.abs(t), minlength=nxv).reshape(nvo, nxo),
                         count=np.bincount(cell, minlength=nxv).reshape(nvo, nxo),
                         rest=dict(exact=math.fsum(rt.tolist()), abs=float(np.sum(np.abs(rt))), count=int(rt.size)))
    return out


def bincount_sums(x, v, q, E, inp):
    """((nv_opd, nx_opd), rest): np.bincount sums of the same terms (float64 additions in marker order) -- a second summation
    of the very terms, for sizes at which the exact sum would take too long"""
    cell, t, rt = terms(x, v, q, E, inp)
    return np.bincount(cell, weights=t, minlength=inp.nx_opd * inp.nv_opd).reshape(inp.nv_opd, inp.nx_opd), float(np.sum(rt))


def workgroups(np_markers, num_cu=256):
    """workgroups of a pass over np_markers markers (launch_policy.cpp power_plan): one per CU, never more than the marker
    pairs fill with 1024 threads; num_cu = 256 bounds every device the library runs on"""
    return max(1, min(num_cu, ((int(np_markers) >> 1) + 1023) // 1024))


def bound(ref_set, nworkgroups, additions=None):
    """(nv_opd, nx_opd): the bound above for the plane of one set of reference(); additions: the additions a bin's terms
    pass through, if not count + workgroups (np.bincount: count)"""
    n = ref_set["count"] + nworkgroups if additions is None else additions
    return n * U * ref_set["abs"] * (1.0 + 2.0 ** -20)


def bound_rest(ref_set, nworkgroups):
    r = ref_set["rest"]
    return (r["count"] + nworkgroups) * U * r["abs"] * (1.0 + 2.0 ** -20)


def bound_v(ref_set, nworkgroups):
    """(nv_opd,): the v-profile is the plane summed over ix ascending in doubles: the bins' bounds, and nx_opd - 1 more
    additions of partial sums that stay below the row's sum of magnitudes (plus what the bins' own errors add to them)"""
    b = bound(ref_set, nworkgroups)
    nxo = ref_set["abs"].shape[1]
    return b.sum(axis=1) + (nxo - 1) * U * (ref_set["abs"].sum(axis=1) + b.sum(axis=1)) * (1.0 + 2.0 ** -20)


def python_power(x, v, q, E, inp):
    """([nv_opd nx_opd] lists of the terms of every bin, list of the rest terms), marker by marker in plain Python floats
    (the self-check of the numpy path)"""
    nx, lx, nxo, nvo, vmax = inp.nx, inp.lx, inp.nx_opd, inp.nv_opd, inp.v_max
    E = [float(a) for a in E]
    bins = [[] for _ in range(nxo * nvo)]
    rest = []
    for xi, vi, qi in zip(map(float, x), map(float, v), map(float, q)):
        px = math.fmod(xi, lx)
        if px < 0.0:
            px = px + lx
        s = px / lx * float(nx)
        fl = math.floor(s)
        wl = 1.0 - (s - fl)
        ix = int(fl) if fl < nx else 0
        ir = 0 if ix + 1 == nx else ix + 1
        e = E[ix] * wl
        e = e + E[ir] * (1.0 - wl)
        c = vi * e
        t = c * qi
        if abs(vi) >= vmax:
            rest.append(t)
            continue
        sx = px / lx * float(nxo)
        fx = math.floor(sx)
        jx = int(fx)
        sx = 1.0 - (sx - fx)
        if jx == nxo:
            jx = 0
        sv = (vi + vmax) / (vmax * 2.0) * float(nvo - 1)
        fv = math.floor(sv)
        jv = int(fv)
        sv = 1.0 - (sv - fv)
        jvu = jv + 1 if jv + 1 < nvo else jv
        jxr = 0 if jx + 1 > nxo - 1 else jx + 1
        sxr, svu = 1.0 - sx, 1.0 - sv
        bins[jv * nxo + jx].append(sx * sv * t)
        bins[jvu * nxo + jx].append(sx * svu * t)
        bins[jv * nxo + jxr].append(sxr * sv * t)
        bins[jvu * nxo + jxr].append(sxr * svu * t)
    return bins, rest

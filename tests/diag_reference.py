"""Exact host reference of the diagnostics pass of output_all (k_ptcldist, k_step_full<DIAG>): the (x, v) and v histograms
of output_ptcldist and the kinetic sums of output_field, src/pic1dp_output.F90:126-151 and :239-313.

Every term is formed in float64 as the reference forms it -- sx = x / lx * nx_opd, sv = (v + v_max) / (v_max * 2) *
(nv_opd - 1), then (sx * sv) * p, (sx * (1 - sv)) * w, ... and v * v, (v * v) * p, (v * v) * w -- with the two edge rules
of the library: ix == nx_opd folds to cell 0 with sx = 1; iv == nv_opd - 1 (sv == 1) keeps row iv and drops
the weight-0 writes to row iv + 1.  The terms of a bin are summed exactly: each plane is scaled by 2^-e with 2^e =
2^-104 of a bound on its terms (2^-100 of its largest term or finer), the scaled terms rounded to integers (exact for
every term above 2^53 quanta), split into three 35-bit limbs, and the limbs summed with np.bincount per chunk of
2^15 markers (float64: at most 2^17 limbs of at most 2^35 per bin, exact), then in int64 across chunks and in Python ints at the end.  The
result per bin is n 2^e, off the exact sum of the float64 terms by at most count 2^(e-1) (`qerr`; 0 where every term is a
whole number of quanta).

Besides the v histograms of the reference (terms sv, sv p, sv w), the `vrow` planes hold the same rows in the form the
LDS path of the pass forms them: the sums of the row's (x, v) terms sx sv, (1 - sx) sv.

Error bounds of the library's two ways of summing (`double_bound`, `fixed_bound`) are rigorous first-order bounds with
a factor 2 of slack.  A helper of the tests, not collected."""
import math
from fractions import Fraction
from concurrent.futures import ThreadPoolExecutor

import numpy as np

U = 2.0 ** -53
CHUNK = 1 << 15
LIMB = 35
PLANES = ("markr_xv", "total_xv", "pertb_xv", "markr_v", "total_v", "pertb_v")


def bins(x, v, lx, v_max, nx_opd, nv_opd):
    """(inside, ix, ixr, iv, ivu, sx, sv): the markers with |v| < v_max and their cells and weights, as the pass forms
    them (device_diag.hpp ptcldist_one)"""
    x = np.asarray(x, dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    inside = np.abs(v) < v_max
    x, v = x[inside], v[inside]
    sx = x / lx * float(nx_opd)
    fx = np.floor(sx)
    sx = 1.0 - (sx - fx)
    ix = fx.astype(np.int64)
    ix[ix == nx_opd] = 0                                    # x == lx: the periodic image of x = 0 (sx == 1)
    sv = (v + v_max) / (v_max * 2.0) * float(nv_opd - 1)
    fv = np.floor(sv)
    sv = 1.0 - (sv - fv)
    iv = fv.astype(np.int64)
    assert np.all((ix >= 0) & (ix < nx_opd) & (iv >= 0) & (iv < nv_opd)), "positions outside [0, lx]"
    ivu = np.minimum(iv + 1, nv_opd - 1)                    # iv == nv_opd - 1: sv == 1, the row above gets weight 0
    ixr = np.where(ix + 1 > nx_opd - 1, 0, ix + 1)
    return inside, ix, ixr, iv, ivu, sx, sv


def _limbs(t, e, nl=3):
    """signed limbs (l2, l1, l0), |l| <= 2^35, with t = (l2 2^70 + l1 2^35 + l0) 2^e up to the rounding of t to a whole
    number of quanta 2^e (to nearest, ties to even); and whether any term was rounded.  Each step takes a multiple of
    the next limb's unit off the remainder by the magic-constant rounding (c + 1.5 2^(k+52)) - 1.5 2^(k+52), so the
    remainders are exact"""
    out = []
    r = np.asarray(t, dtype=np.float64)
    for k in range((nl - 1) * LIMB, -1, -LIMB):
        m = 1.5 * 2.0 ** (e + k + 52)
        h = (r + m) - m
        r = r - h
        out.append(np.ldexp(h, -(e + k)))
    rounded = bool(np.any(r != 0.0))
    assert np.all(np.abs(out[0]) <= 2.0 ** LIMB), "a term beyond the plane's bound"
    return out, rounded


class _Plane:
    def __init__(self, nbins, bound, e_min=None):
        _, eb = math.frexp(bound if bound > 0.0 else 1.0)   # every |term| <= bound < 2^eb
        self.e = eb - 3 * LIMB + 1                          # terms below 2^104 quanta
        self.nl = 3
        if e_min is not None:                               # quantum 2^e_min (-1074: every float64 term exact), more limbs
            self.e = e_min
            self.nl = -(-(eb - e_min) // LIMB) + 1
        self.limbs = [np.zeros(nbins, dtype=np.int64) for _ in range(self.nl)]
        self.abs = np.zeros(nbins)
        self.count = np.zeros(nbins, dtype=np.int64)
        self.rounded = False
        self.nbins = nbins

    def add(self, idx, t, count):
        ls, rnd = _limbs(t, self.e, self.nl)
        self.rounded |= rnd
        if self.nbins == 1:
            for k in range(self.nl):
                self.limbs[k] += np.int64(np.sum(ls[k]))
            self.abs += np.sum(np.abs(t))
        else:
            for k in range(self.nl):
                self.limbs[k] += np.bincount(idx, weights=ls[k], minlength=self.nbins).astype(np.int64)
            self.abs += np.bincount(idx, weights=np.abs(t), minlength=self.nbins)
        self.count += count

    def merge(self, other):
        for k in range(self.nl):
            self.limbs[k] += other.limbs[k]
        self.abs += other.abs
        self.count += other.count
        self.rounded |= other.rounded

    def finish(self, rows=None):
        """rows = nx_opd: the sums over the rows of this (x, v) plane (the `vrow` form)"""
        limbs, a, count = self.limbs, self.abs, self.count
        if rows:
            limbs = [l.reshape(-1, rows).sum(axis=1) for l in limbs]        # (int64: below 2^63 for 2^25 markers)
            a, count = a.reshape(-1, rows).sum(axis=1), count.reshape(-1, rows).sum(axis=1)
        ints = [sum(int(l) << (LIMB * (self.nl - 1 - j)) for j, l in enumerate(ls)) for ls in zip(*limbs)]
        if self.e > -900:       # float(n) rounds once, the scaling is exact
            value = np.array([math.ldexp(float(n), self.e) for n in ints])
        else:                   # (the product may be subnormal, n beyond the float range: one rounding of the rational)
            value = np.array([float(Fraction(n, 1 << -self.e)) for n in ints])
        qerr = count * 2.0 ** (self.e - 1) if self.rounded else np.zeros(count.size)
        return dict(ints=ints, e=self.e, value=value, abs=a * (1.0 + 1e-12), count=count, qerr=qerr)


def _planes(nxv, nv_opd, qb, kb, e_min):
    return ([_Plane(nxv, b, e_min) for b in qb], [_Plane(nv_opd, b, e_min) for b in qb], [_Plane(1, b, e_min) for b in kb])


def _run(x, v, p, w, lx, v_max, nx_opd, nv_opd, deltaf, planes, starts, chunk):
    xv, vh, kin = planes
    nxv = nx_opd * nv_opd
    nk = 3 if deltaf else 2
    for i0 in starts:
        sl = slice(i0, min(x.size, i0 + chunk))
        xc, vc, pc, wc = x[sl], v[sl], p[sl], w[sl]
        v2 = vc * vc
        for k, t in enumerate((v2, v2 * pc, v2 * wc)[:nk]):
            kin[k].add(None, t, t.size)
        inside, ix, ixr, iv, ivu, sx, sv = bins(xc, vc, lx, v_max, nx_opd, nv_opd)
        pc, wc = pc[inside], wc[inside]
        sxr, svu = 1.0 - sx, 1.0 - sv
        cells = np.concatenate([iv * nx_opd + ix, ivu * nx_opd + ix, iv * nx_opd + ixr, ivu * nx_opd + ixr])
        wts = np.concatenate([sx * sv, sx * svu, sxr * sv, sxr * svu])
        cnt = np.bincount(cells, minlength=nxv)
        xv[0].add(cells, wts, cnt)
        xv[1].add(cells, wts * np.tile(pc, 4), cnt)
        if deltaf:
            xv[2].add(cells, wts * np.tile(wc, 4), cnt)
        vrows = np.concatenate([iv, ivu])
        vw = np.concatenate([sv, svu])
        cnt = np.bincount(vrows, minlength=nv_opd)
        vh[0].add(vrows, vw, cnt)
        vh[1].add(vrows, vw * np.tile(pc, 2), cnt)
        if deltaf:
            vh[2].add(vrows, vw * np.tile(wc, 2), cnt)
    return planes


def reference(x, v, p, w, lx, v_max, nx_opd, nv_opd, deltaf, chunk=CHUNK, threads=8, e_min=None):
    """the exact diagnostics of markers x, v, p, w (w ignored for full f).  Returns {plane: dict(ints, e, value, abs,
    count, qerr)} for the six planes of PLANES, the three `vrow` planes ("markr_vrow", ...), and "kinetic" (three
    entries: sum v^2, v^2 p, v^2 w).  Chunks are spread over `threads` threads (numpy releases the GIL); the sums are
    exact, so the split does not change them.  e_min = -1074: the sums exact for any float64 terms (a few markers)"""
    x, v, p = (np.asarray(a, dtype=np.float64) for a in (x, v, p))
    w = np.asarray(w, dtype=np.float64) if deltaf else np.zeros_like(v)
    n = x.size
    mp = float(np.max(np.abs(p), initial=0.0))
    mw = float(np.max(np.abs(w), initial=0.0))
    vv = float(np.max(np.abs(v), initial=0.0)) ** 2
    qb, kb = (1.0, mp, mw), (vv, vv * mp, vv * mw)
    starts = list(range(0, n, chunk))
    nt = max(1, min(threads, len(starts)))
    args = (x, v, p, w, lx, v_max, nx_opd, nv_opd, deltaf)
    with ThreadPoolExecutor(nt) as ex:
        parts = list(ex.map(lambda j: _run(*args, _planes(nx_opd * nv_opd, nv_opd, qb, kb, e_min), starts[j::nt], chunk), range(nt)))
    xv, vh, kin = parts[0]
    for part in parts[1:]:
        for mine, theirs in zip(xv + vh + kin, part[0] + part[1] + part[2]):
            mine.merge(theirs)
    out = {}
    for k, name in enumerate(("markr", "total", "pertb")):
        out[name + "_xv"] = xv[k].finish()
        out[name + "_v"] = vh[k].finish()
        out[name + "_vrow"] = xv[k].finish(rows=nx_opd)
    out["kinetic"] = [kin[k].finish() for k in range(3)]
    return out


def combine(a, b):
    """one plane from two (the sums of the markers of a and of b): exact, on the finer of the two quanta"""
    e = min(a["e"], b["e"])
    ints = [(x << (a["e"] - e)) + (y << (b["e"] - e)) for x, y in zip(a["ints"], b["ints"])]
    value = np.array([float(Fraction(n) * Fraction(2) ** e) for n in ints])
    return dict(ints=ints, e=e, value=value, abs=a["abs"] + b["abs"], count=a["count"] + b["count"],
                qerr=a["qerr"] + b["qerr"])


def error(got, plane):
    """a lower bound on |got - exact sum| per bin (got: float64 array): what a comparison with a bound on the error may
    hold against `got` after the reference's own roundings (to float64, and its quantum) are taken off"""
    got = np.asarray(got, dtype=np.float64)
    val = plane["value"]
    return np.maximum(np.abs(got - val) * (1.0 - 4 * U) - 0.5 * np.spacing(np.abs(val)) - plane["qerr"], 0.0)


def double_bound(plane, workgroups, extra=0):
    """|double sum in any order - exact| for `count` terms added into LDS or global bins, workgroup copies flushed with
    atomics (workgroups), `extra` further additions per bin (the LDS path's row sums: nx_opd per workgroup)"""
    n = plane["count"] + workgroups + extra + 2
    return 2.0 * n * U * plane["abs"]


def dist_quanta(np_markers, num_cu, deltaf, bound_p, bound_w, threads=1024):
    """2^e of the three planes' fixed-point sums: make_dist_scale (launch_policy.cpp) restated, for the launch of
    diag_launch there (LDS path: min(num_cu, the workgroups the markers fill)).  bound_p / bound_w: the bounds the pass was
    scaled for (2 max |p|, margin x max |w| of the pass before: capi_diag.cpp diag_fx_bounds)"""
    need = ((np_markers >> 1) + 1023) // 1024
    blocks = max(1, min(num_cu, need))
    per_wg = 2.0 * threads * math.ceil(((np_markers >> 1) + 1) / (blocks * threads)) + 2.0
    e_n = math.ceil(math.log2(per_wg)) + 1
    mag = min(62 - e_n, 50)
    out = []
    for b in (1.0, bound_p, bound_w if deltaf else 1.0):
        _, eb = math.frexp(b)
        out.append(2.0 ** (eb - mag))
    return out, blocks


def fixed_bound(plane, quantum, workgroups):
    """|fixed-point pass - exact|: each term rounded once to the quantum, the per-workgroup integer sums converted to
    double (one rounding) and added across workgroups in doubles"""
    n = plane["count"]
    return 2.0 * (n * 0.5 * quantum + (workgroups + 2) * U * (plane["abs"] + n * quantum))


def on_grid(got, quantum):
    """the bins that are whole multiples of the quantum (every bin of a fixed-point pass is)"""
    s = np.asarray(got, dtype=np.float64) / quantum
    return s == np.floor(s)


def _ulps(a, k):
    """a moved by k units in the last place (k may be negative; 0 and the sign handled as nextafter does)"""
    out = float(a)
    step = math.inf if k > 0 else -math.inf
    for _ in range(abs(k)):
        out = math.nextafter(out, step)
    return out


def top_velocities(v_max, nv_opd):
    """the velocities just below v_max whose sv comes out as exactly nv_opd - 1 (the pass keeps them in the top row)"""
    out, v = [], v_max
    for _ in range(64):
        v = math.nextafter(v, -math.inf)
        if (v + v_max) / (v_max * 2.0) * float(nv_opd - 1) == float(nv_opd - 1):
            out.append(v)
    return out


def edge_positions(lx, nx_opd):
    """0, the smallest subnormal, the cell boundaries k lx / nx_opd +- 1, 2 ulps (k = 0, 1, nx_opd / 2, nx_opd - 1,
    nx_opd), lx - ulp, lx -- all inside [0, lx]"""
    xs = [0.0, 5e-324, _ulps(lx, -1), lx]
    for k in sorted({0, 1, nx_opd // 2, nx_opd - 1, nx_opd}):
        b = lx * k / nx_opd
        xs += [_ulps(b, d) for d in (-2, -1, 1, 2)]
    return sorted({x for x in xs if 0.0 <= x <= lx})


def edge_velocities(v_max, nv_opd):
    """-v_max, -v_max + ulp, the bin boundaries +- 1, 2 ulps (k = 0, 1, (nv_opd - 1) / 2, nv_opd - 2, nv_opd - 1), +-0,
    v_max - 1 ... 4 ulps, the top-row velocities, +-v_max (the last two and -v_max leave the histograms)"""
    dv = v_max * 2.0
    vs = [-v_max, _ulps(-v_max, 1), 0.0, -0.0, v_max] + [_ulps(v_max, -k) for k in range(1, 5)] + top_velocities(v_max, nv_opd)
    for k in sorted({0, 1, (nv_opd - 1) // 2, max(nv_opd - 2, 0), nv_opd - 1}):
        b = -v_max + dv * k / (nv_opd - 1)
        vs += [_ulps(b, d) for d in (-2, -1, 1, 2)]
    return [v for v in dict.fromkeys(vs) if -v_max <= v <= v_max]


def edge_markers(lx, v_max, nx_opd, nv_opd, seed=0):
    """every edge velocity once, with the edge positions in turn, |p| and |w| up to 3"""
    xs, vs = edge_positions(lx, nx_opd), edge_velocities(v_max, nv_opd)
    n = max(len(xs), len(vs))
    rng = np.random.default_rng(seed)
    x = np.array([xs[i % len(xs)] for i in range(n)])
    v = np.array([vs[(5 * i) % len(vs)] if len(vs) % 5 else vs[i % len(vs)] for i in range(n)])
    p = rng.uniform(-3.0, 3.0, n)
    w = rng.uniform(-3.0, 3.0, n)
    return x, v, p, w


def batches(x, v, lx, v_max, nx_opd, nv_opd):
    """the markers split into batches in which no two markers share a v row (hence no (x, v) bin either): every bin of
    a batch's histograms then holds at most one marker's term, and the LDS path's row sums two terms of one marker"""
    inside, ix, ixr, iv, ivu, sx, sv = bins(x, v, lx, v_max, nx_opd, nv_opd)
    rows = {}
    j = 0
    for i in range(len(x)):
        if inside[i]:
            rows[i] = {int(iv[j]), int(ivu[j])}
            j += 1
    out, used = [], []
    for i in range(len(x)):
        r = rows.get(i, set())
        for b, u in zip(out, used):
            if not (r & u):
                b.append(i)
                u |= r
                break
        else:
            out.append([i])
            used.append(set(r))
    return out

"""The Fourier-Hermite spectrum of the markers (include/pic1dp_hip.h pic1dp_hip_hermite) restated in numpy: the wrapped
position from tests/exact_charge.py cells(), u = (v - v0) * (1.0 / vt), the recurrence psi_0 = 1, psi_1 = u,
psi_(n+1) = (u psi_n) ra[n] - psi_(n-1) rb[n] with every product and the difference rounded on their own, theta = kk px with
kk = 2.0 * pi / lx * m, numpy's cos and sin, y = q cos, q sin, and the terms T = psi_n * y.  Per (set, mode, trig, n): the
exact sum of the float64 terms (math.fsum: correctly rounded), the sum of their magnitudes and their number.

The bound the definition states: with n_p valid markers and B partial sums merged by the launch (the plan says how many),
    |out - exact| <= (n_p + B + 16) 2^-53 sum |T| (1 + 2^-20);
the 16 covers the device's sincos within 4 ulp (8 half-ulps), numpy's own cos and sin (2) and the two products on either
side (4).  Nothing is measured for it.  A helper of the tests, not collected."""
import math

import numpy as np

from exact_charge import cells

U = 2.0 ** -53
SETS = ("total", "pertb")      # the weights p, the weights w


def tables(nherm):
    n1 = np.arange(1, nherm + 1, dtype=np.float64)
    return 1.0 / np.sqrt(n1), np.sqrt(n1 - 1.0) / np.sqrt(n1)


def psi(u, nherm):
    """(nherm, len(u)): the recurrence, operation by operation"""
    u = np.asarray(u, dtype=np.float64)
    ra, rb = tables(nherm)
    out = np.empty((nherm, u.size))
    prev, cur = np.zeros(u.size), np.ones(u.size)
    with np.errstate(all="ignore"):
        for n in range(nherm):
            out[n] = cur
            if n == 0:
                nxt = u.copy()
            else:
                a = u * cur
                b = a * ra[n]
                c = prev * rb[n]
                nxt = b - c
            prev, cur = cur, nxt
    return out


def columns(x, q, inp, modes):
    """[(mode index, trig 0 cos / 1 sin, y array)] of one weight set"""
    px = cells(x, inp)[0]
    out = []
    for a, m in enumerate(modes):
        kk = 2.0 * np.pi / inp.lx * float(m)
        th = kk * px
        out.append((a, 0, q * np.cos(th)))
        out.append((a, 1, q * np.sin(th)))
    return out


def reference(x, v, p, w, inp, modes=(1,), nherm=64, v0=0.0, vt=1.0, which=3):
    """{"total": ..., "pertb": ...} for the sets of `which`, each dict(exact, abs (nmodes, 2, nherm), count) over the markers
    given (the valid ones: the caller cuts the tail off)"""
    x, v = (np.asarray(a, dtype=np.float64) for a in (x, v))
    ivt = 1.0 / vt
    ps = psi((v - v0) * ivt, nherm)
    out = {}
    with np.errstate(all="ignore"):
        for bit, name, q in ((1, "total", p), (2, "pertb", w)):
            if not which & bit:
                continue
            q = np.asarray(q, dtype=np.float64)
            exact = np.zeros((len(modes), 2, nherm))
            mag = np.zeros((len(modes), 2, nherm))
            for a, t, y in columns(x, q, inp, modes):
                T = ps * y[None, :]
                mag[a, t] = np.abs(T).sum(axis=1)
                for n in range(nherm):
                    row = T[n]
                    exact[a, t, n] = math.fsum(row.tolist()) if np.all(np.isfinite(row)) else np.nan
            out[name] = dict(exact=exact, abs=mag, count=x.size)
    return out


def bound(ref_set, partials):
    return (ref_set["count"] + partials + 16) * U * ref_set["abs"] * (1.0 + 2.0 ** -20)


def raw(got_complex):
    """the dict entry of Pic1dp.hermite (C - iS, (nmodes, nherm)) as raw sums (nmodes, 2, nherm)"""
    g = np.asarray(got_complex)
    return np.stack([g.real, -g.imag], axis=1)


def worst(got, ref_set, partials):
    """max error / bound over the words (0 where both vanish, inf where only the bound does)"""
    err = np.abs(got - ref_set["exact"])
    b = bound(ref_set, partials)
    return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))

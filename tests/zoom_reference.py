"""The rule of pic1dp_hip_zoom (include/pic1dp_hip.h) restated: the indices in numpy, one IEEE operation per
line as the header writes them, the quanta and the sums in Python integers.  From downloaded (or crafted) arrays of the VALID
markers; nothing here comes from the library but the two log2 quanta the caller passes (amd.diag_quanta(inp, s)[1:3])."""
import math

import numpy as np

PLANES = ("markr", "total", "pertb")
LIMIT = 2 ** 44

# the two windows of the issue at which the clamp is reached (at lx = make_input's default box, 0x1.1740afa84ad8ap+4)
CLAMP_X = dict(x=(float.fromhex("0x1.db7810db9b148p+1"), float.fromhex("0x1.287245922309ep+1")), nxb=1)
CLAMP_V = dict(v=(float.fromhex("-0x1.b1ac38e155210p-1"), float.fromhex("0x1.68d948684dcdap+2")), nvb=2)


def wrap(x, lx):
    """the deposit's wrap: fmod, then + lx where negative"""
    with np.errstate(invalid="ignore"):
        r = np.fmod(np.asarray(x, dtype=np.float64), np.float64(lx))
        return np.where(r < 0.0, r + np.float64(lx), r)


def scales(lx, xw, vw, bins):
    x_lo, x_hi, v_lo, v_hi = (np.float64(t) for t in (*xw, *vw))
    lw = (x_hi + np.float64(lx)) - x_lo if x_lo > x_hi else x_hi - x_lo
    with np.errstate(divide="ignore"):
        return lw, np.float64(bins[0]) / lw, np.float64(bins[1]) / (v_hi - v_lo)


def cells(x, v, lx, xw, vw, bins, raw=False):
    """(inside, ix, jv) per marker; ix, jv hold 0 outside.  raw: the indices before the clamp"""
    x_lo, x_hi, v_lo, v_hi = (np.float64(t) for t in (*xw, *vw))
    nxb, nvb = bins
    v = np.asarray(v, dtype=np.float64)
    px = wrap(x, lx)
    with np.errstate(invalid="ignore"):
        in_x = ((x_lo <= px) & (px < x_hi)) if x_lo <= x_hi else ((px >= x_lo) | (px < x_hi))
        in_v = (v_lo <= v) & (v < v_hi)
    inside = in_x & in_v
    ix, jv = np.zeros(px.shape, dtype=np.int64), np.zeros(px.shape, dtype=np.int64)
    if inside.any():
        _, sx, sv = scales(lx, xw, vw, bins)
        d = px[inside] - x_lo
        d = np.where(d < 0.0, d + np.float64(lx), d)
        i = (d * sx).astype(np.int64)
        j = ((v[inside] - v_lo) * sv).astype(np.int64)
        assert i.min() >= 0 and j.min() >= 0 and i.max() <= nxb and j.max() <= nvb      # the overshoot is one cell at most
        if not raw:
            i, j = np.minimum(i, nxb - 1), np.minimum(j, nvb - 1)
        ix[inside], jv[inside] = i, j
    return inside, ix, jv


def quantise(t, e):
    """(n as int64, summed or not): n = rint(t 2^-e); a term of 2^44 quanta or more, or a NaN, is not summed"""
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(np.ldexp(np.asarray(t, dtype=np.float64), -int(e)))
        ok = np.abs(r) < float(LIMIT)
    return np.where(ok, r, 0.0).astype(np.int64), ok


def limbs_of(t):
    return t >> 32, t & 0xffffffff


def reference(x, v, p, w, lx, xw, vw, bins, which, e_p, e_w):
    """dict(totals [plane][cell] Python integers, limbs (nplanes, 2, nvb, nxb) int64 normalised, rejected [3], doubles
    (nplanes, nvb, nxb), inside: the count of markers in the window)"""
    nxb, nvb = bins
    ncell = nxb * nvb
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    if xw[0] == xw[1]:
        inside, cell = np.zeros(x.shape, dtype=bool), np.zeros(x.shape, dtype=np.int64)
    else:
        inside, ix, jv = cells(x, v, lx, xw, vw, bins)
        cell = jv * nxb + ix
    rejected = [0, 0, 0]
    totals, doubles = [], []
    for k, (term, e) in enumerate(((None, 0), (p, e_p), (w, e_w))):
        if not which & (1 << k):
            continue
        tot = [0] * ncell
        c = cell[inside]
        if k == 0:
            for ci in c.tolist():
                tot[ci] += 1
        else:
            n, ok = quantise(np.asarray(term, dtype=np.float64)[inside], e)
            rejected[k] = int(np.count_nonzero(~ok))
            for ci, ni in zip(c[ok].tolist(), n[ok].tolist()):
                tot[ci] += ni
        totals.append(tot)
        doubles.append(np.array([math.ldexp(float(t), e) for t in tot]).reshape(nvb, nxb))
    limbs = np.zeros((len(totals), 2, nvb, nxb), dtype=np.int64)
    for j, tot in enumerate(totals):
        hl = [limbs_of(t) for t in tot]
        limbs[j, 0] = np.array([h for h, _ in hl], dtype=np.int64).reshape(nvb, nxb)
        limbs[j, 1] = np.array([l for _, l in hl], dtype=np.int64).reshape(nvb, nxb)
    return dict(totals=totals, limbs=limbs, rejected=rejected, doubles=np.array(doubles), inside=int(np.count_nonzero(inside)))


def planted(lx, xw, vw, e_p, e_w, reject=False):
    """markers on every edge of the window xw x vw: x, v, p, w.  The x cases at a v inside, the v cases at an x inside.
    reject: with the terms that are not summed (2^44 quanta, a NaN) among them"""
    x_lo, x_hi = xw
    v_lo, v_hi = vw
    inf = math.inf
    straddle = x_lo > x_hi
    lw = (x_hi + lx) - x_lo if straddle else x_hi - x_lo
    x_in = math.fmod(x_lo + 0.5 * lw, lx)
    v_in = v_lo + 0.25 * (v_hi - v_lo)
    xs = [x_lo, math.nextafter(x_lo, inf), math.nextafter(x_lo, -inf), math.nextafter(x_hi, 0.0), x_hi, math.nextafter(x_hi, inf),
          x_in, x_in + lx, x_in - lx, x_in + 5.0 * lx, x_in - 7.0 * lx,
          -1e-300, -5e-324, 0.0, -0.0, lx, math.nextafter(lx, 0.0), 2.0 * lx, -lx, math.nan, inf, -inf,
          math.fmod(x_hi + 0.25 * (lx - lw), lx), math.fmod(x_lo + 0.999999 * lw, lx), math.fmod(x_lo + 1e-9 * lw, lx)]
    if straddle:
        xs += [0.5 * x_hi, 0.5 * (x_lo + lx), math.nextafter(lx, 0.0), 0.0]            # both sides of the boundary
    vs = [v_lo, math.nextafter(v_lo, -inf), math.nextafter(v_lo, inf), math.nextafter(v_hi, -inf), v_hi, math.nextafter(v_hi, inf),
          0.0, -0.0, math.nan, inf, -inf, v_in, 0.5 * (v_lo + v_hi)]
    x = np.array(xs + [x_in] * len(vs))
    v = np.array([v_in] * len(xs) + vs)
    n = x.size
    p = math.ldexp(1.0, e_p) * (3.0 + 0.5 * np.arange(n))                              # ties among them: 3, 3.5 -> 4, 4, 4.5 -> 4, ...
    w = -math.ldexp(1.0, e_w) * (1000.25 + 7.0 * np.arange(n))
    big, just_below = math.ldexp(1.0, e_p + 44), math.ldexp(float(2 ** 44 - 1), e_p)
    extra_p = [just_below, -just_below] + ([big, -big, math.nan, inf] if reject else [])
    extra_w = [math.ldexp(float(2 ** 44 - 1), e_w)] * 2 + ([math.ldexp(1.0, e_w + 44), 1.0, math.nan, 1.0] if reject else [])
    x = np.concatenate([x, np.full(len(extra_p), x_in)])
    v = np.concatenate([v, np.full(len(extra_p), v_in)])
    p = np.concatenate([p, extra_p])
    w = np.concatenate([w, extra_w])
    return x, v, p, w


def assert_same(limbs, ref, what=""):
    """limb for limb, then the words of a failure: the first cell that differs"""
    got = np.asarray(limbs)
    assert got.shape == ref["limbs"].shape, (what, got.shape, ref["limbs"].shape)
    if got.tobytes() != ref["limbs"].tobytes():
        bad = np.argwhere(got != ref["limbs"])
        j, h, jv, ix = bad[0]
        raise AssertionError("%s: %d limbs differ, the first at plane %d limb %d row %d column %d: %d, expected %d"
                             % (what, len(bad), j, h, jv, ix, got[j, h, jv, ix], ref["limbs"][j, h, jv, ix]))

"""The selection rule of pic1dp_hip_select (include/pic1dp_hip.h) restated in numpy, independently of the
library: the deposit's wrap as tests/ref_hotpath.py states it, mix64 in uint64 arithmetic (mod 2^64 by wrap-around), the
windows as plain comparisons.  The result of a selection is np.nonzero(mask)[0] and the arrays indexed by it; everything is
compared bit for bit."""
import math

import numpy as np

from ref_hotpath import wrapped

GOLD = np.uint64(0x9E3779B97F4A7C15)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
U64 = (1 << 64) - 1


def mix64(z):
    """the splitmix64 finaliser on an array of uint64"""
    with np.errstate(over="ignore"):
        z = np.asarray(z, dtype=np.uint64).copy()
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return z


def mix64_int(z):
    """the same on one Python integer"""
    z &= U64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & U64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & U64
    z ^= z >> 31
    return z


def hashes(n, key=0, origin=0):
    """h(g) of g = origin + i, i < n: mix64(key + (g + 1) * GOLD) mod 2^64"""
    with np.errstate(over="ignore"):
        g = np.uint64(origin & U64) + np.arange(n, dtype=np.uint64)
        return mix64(np.uint64(key & U64) + (g + np.uint64(1)) * GOLD)


def thin_of(fraction):
    """max(1, floor(fraction 2^64)) in exact integer arithmetic; 0 for fraction >= 1"""
    if fraction >= 1.0:
        return 0
    m, e = math.frexp(fraction)                      # fraction = m 2^e, m a 53-bit fraction
    num = int(m * (1 << 53)) << 64                   # fraction 2^64 = num 2^(e - 53)
    sh = 53 - e
    return max(1, num >> sh if sh >= 0 else num << -sh)


def mask(x, v, lx, x_window=(-np.inf, np.inf), v_window=(-np.inf, np.inf), thin=0, key=0, origin=0):
    """which of the valid markers (x, v) the rule selects"""
    x, v = np.asarray(x, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        px = wrapped(x, lx)
        x_lo, x_hi = x_window
        in_x = ((x_lo <= px) & (px < x_hi)) if x_lo <= x_hi else ((px >= x_lo) | (px < x_hi))
        in_v = (v_window[0] <= v) & (v < v_window[1])
    keep = np.ones(x.size, dtype=bool) if thin == 0 else hashes(x.size, key, origin) < np.uint64(thin)
    return in_x & in_v & keep


def select(g, lx, n=None, **rule):
    """dict(count, index, x, v, p, w) of the markers g = dict(x, v, p, w) whose first n are the valid ones"""
    n = g["x"].size if n is None else n
    idx = np.nonzero(mask(g["x"][:n], g["v"][:n], lx, **rule))[0].astype(np.int64)
    out = {"count": int(idx.size), "index": idx}
    out.update({k: g[k][:n][idx] for k in "xvpw"})
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def assert_same(got, ref, upto=None, what=""):
    """count, index and the four arrays of a selection against the reference's, bit for bit; upto: the first min(count,
    upto) only (a truncated selection)"""
    assert got["count"] == ref["count"], (what, got["count"], ref["count"])
    m = ref["count"] if upto is None else min(ref["count"], upto)
    assert got["index"].dtype == np.int64 and np.array_equal(got["index"], ref["index"][:m]), what
    for k in "xvpw":
        assert same_bits(got[k], ref[k][:m]), (what, k)


def edge_markers(lx, v_lo, v_hi, seed=7, nrandom=300):
    """the crafted markers: every edge position crossed with every edge velocity, then random ones; returns x, v, p, w"""
    xs = [0.0, -0.0, lx, math.nextafter(lx, 0.0), lx + 1e-13, -1e-300, 7.3 * lx, -7.3 * lx, float("nan")]
    vs = [v_lo, math.nextafter(v_lo, -math.inf), v_hi, math.nextafter(v_hi, -math.inf), float("nan"), math.inf, -math.inf]
    x = [a for a in xs for _ in vs]
    v = [b for _ in xs for b in vs]
    rng = np.random.default_rng(seed)
    x = np.concatenate([np.array(x), rng.uniform(-2.0 * lx, 3.0 * lx, nrandom)])
    v = np.concatenate([np.array(v), rng.uniform(v_lo - 2.0, v_hi + 2.0, nrandom)])
    p = rng.normal(0.0, 1.0, x.size)
    w = rng.normal(0.0, 1.0, x.size)
    return x, v, p, w


def windows(lx, v_lo, v_hi):
    """(name, x window, v window): plain, straddling, empty, everything"""
    inf = np.inf
    return [("plain", (0.25 * lx, 0.75 * lx), (v_lo, v_hi)),
            ("plain_to_lx", (0.0, lx), (v_lo, v_hi)),
            ("straddling", (0.75 * lx, 0.25 * lx), (v_lo, v_hi)),
            ("straddling_all_v", (math.nextafter(lx, 0.0), 1e-300), (-inf, inf)),
            ("empty", (0.5 * lx, 0.5 * lx), (-inf, inf)),
            ("empty_v", (-inf, inf), (v_lo, v_lo)),
            ("everything", (-inf, inf), (-inf, inf))]

"""The exact phase-space histogram on a caller's window and grid (include/pic1dp_hip.h pic1dp_hip_zoom), the
parts that need no GPU: the rule on host arrays (pic1dp_hip_host_zoom) against tests/zoom_reference.py limb for limb on
random and planted markers, the conversion of rank-summed limbs against Python integers, the lengths and every refusal, the
pass plan (through the probe library), and the stand-alone checker under the host's sanitizers."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import zoom_reference as Z
from conftest import ROOT

CAP_WORDS = 150 * 1024 // 8            # launch_policy.hpp kDiagLdsCap / 8 = 19 200
INF = math.inf


def quanta(amd, inp, s=0):
    e = amd.diag_quanta(inp, s)
    return e[1], e[2]


def host_against_reference(amd, inp, x, v, p, w, xw, vw, bins, which, what=""):
    e_p, e_w = quanta(amd, inp)
    ref = Z.reference(x, v, p, w, inp.lx, xw, vw, bins, which, e_p, e_w)
    limbs, rej = amd.host_zoom(inp, x, v, p if which & 2 else None, w if which & 4 else None, x=xw, v=vw, bins=bins, which=which)
    Z.assert_same(limbs, ref, what)
    assert rej.tolist() == ref["rejected"], what
    assert np.all((limbs[:, 1] >= 0) & (limbs[:, 1] < 2**32))
    return ref, limbs


# ---------------------------------------------------------------------------
# the rule on host arrays
# ---------------------------------------------------------------------------
WINDOWS = [((0.0, None), (-8.0, 8.0), (64, 64)),              # the whole box (None: lx)
           ((1.0, 3.0), (3.0, 5.0), (7, 5)),
           ((15.0, 2.0), (-1.5, 2.25), (5, 3)),                # straddling
           ((None, 3.0), (-2.0, 2.0), (3, 4)),                 # straddling from lx itself
           ((4.0, 4.0), (-2.0, 2.0), (3, 4)),                  # empty
           ((2.0, 9.0), (-3.0, 0.5), (1, 1)), ((2.0, 9.0), (-3.0, 0.5), (1, 64)), ((2.0, 9.0), (-3.0, 0.5), (64, 1))]


@pytest.mark.parametrize("xw,vw,bins", WINDOWS)
def test_host_zoom_on_random_markers(amd, xw, vw, bins):
    inp = amd.make_input(nparticle_max=1000, nx=16)
    xw = tuple(inp.lx if t is None else t for t in xw)
    rng = np.random.default_rng(bins[0] * 100 + bins[1])
    n = 20_000
    x = rng.uniform(-1.0, 2.0, n) * inp.lx
    v = rng.normal(0.0, 3.0, n)
    p, w = rng.uniform(0.0, 0.1, n), rng.normal(0.0, 0.01, n)
    for which in range(1, 8):
        ref, _ = host_against_reference(amd, inp, x, v, p, w, xw, vw, bins, which, "which %d" % which)
        if xw[0] == xw[1]:
            assert ref["inside"] == 0
        elif which == 7:
            assert ref["inside"] > 100 and sum(ref["totals"][0]) == ref["inside"]
            sel = amd.host_select(inp, x, v, x_window=xw, v_window=vw)[0]            # the window is select's
            assert sel == ref["inside"]


@pytest.mark.parametrize("xw,vw,bins", WINDOWS[:4] + [(Z.CLAMP_X["x"], (-1.0, 1.0), (Z.CLAMP_X["nxb"], 3)),
                                                       ((1.0, 3.0), Z.CLAMP_V["v"], (3, Z.CLAMP_V["nvb"]))])
def test_host_zoom_on_planted_markers(amd, xw, vw, bins):
    inp = amd.make_input(nparticle_max=1000, nx=16)
    xw = tuple(inp.lx if t is None else t for t in xw)
    e_p, e_w = quanta(amd, inp)
    for reject in (False, True):
        x, v, p, w = Z.planted(inp.lx, xw, vw, e_p, e_w, reject=reject)
        ref, limbs = host_against_reference(amd, inp, x, v, p, w, xw, vw, bins, 7, "planted")
        assert ref["rejected"] == ([0, 4, 2] if reject else [0, 0, 0])
        assert ref["inside"] >= 10
    # the planted set does what it says: px == x_lo is in, px == x_hi is out, nextafter(x_hi, 0) is in the last column
    x, v, p, w = Z.planted(inp.lx, xw, vw, e_p, e_w)
    inside, ix, jv = Z.cells(x, v, inp.lx, xw, vw, bins)
    assert inside[0] and ix[0] == 0 and inside[3] and ix[3] == bins[0] - 1
    assert not inside[4] or xw[1] == inp.lx                              # (a stored x == lx wraps to 0)
    assert not inside[np.isnan(v)].any() and not inside[np.isinf(v)].any() and not inside[np.isnan(x) | np.isinf(x)].any()
    k = len(x) - 2 - 13                                                  # the v cases: v_lo first
    assert v[k] == vw[0] and inside[k] and jv[k] == 0 and not inside[k + 1] and not inside[k + 4] and inside[k + 3] and jv[k + 3] == bins[1] - 1
    assert Z.wrap(np.array([-1e-300]), inp.lx)[0] == inp.lx              # px == lx from a tiny negative x


def test_the_clamp_is_reached_at_both_upper_edges(amd):
    inp = amd.make_input(nparticle_max=1000, nx=16)
    assert inp.lx == float.fromhex("0x1.1740afa84ad8ap+4")
    xw, nxb = Z.CLAMP_X["x"], Z.CLAMP_X["nxb"]
    vw, nvb = Z.CLAMP_V["v"], Z.CLAMP_V["nvb"]
    x, v = np.array([math.nextafter(xw[1], 0.0)]), np.array([math.nextafter(vw[1], -INF)])
    _, ix, _ = Z.cells(x, np.zeros(1), inp.lx, xw, (-1.0, 1.0), (nxb, 1), raw=True)
    _, _, jv = Z.cells(np.full(1, 2.0), v, inp.lx, (1.0, 3.0), vw, (1, nvb), raw=True)
    assert ix[0] == nxb and jv[0] == nvb                                 # raw index one past the last cell
    limbs, _ = amd.host_zoom(inp, x, np.zeros(1), x=xw, v=(-1.0, 1.0), bins=(nxb, 1), which=1)
    assert limbs[0, 1].tolist() == [[1]]
    limbs, _ = amd.host_zoom(inp, np.full(1, 2.0), v, x=(1.0, 3.0), v=vw, bins=(1, nvb), which=1)
    assert limbs[0, 1].ravel().tolist() == [0, 1]


def test_quantum_terms_at_the_limit(amd):
    inp = amd.make_input(nparticle_max=1000, nx=16)
    e_p, e_w = quanta(amd, inp)
    q = math.ldexp(1.0, e_p)
    terms = [(2.0**44 - 1.0) * q, -(2.0**44 - 1.0) * q, 2.0**44 * q, -(2.0**44) * q, math.nan, 2.5 * q, 3.5 * q, -2.5 * q, 0.4999 * q]
    n = len(terms)
    limbs, rej = amd.host_zoom(inp, np.full(n, 1.0), np.zeros(n), np.array(terms), None, x=(0.0, 2.0), v=(-1.0, 1.0), bins=(1, 1), which=3)
    assert rej.tolist() == [0, 3, 0]
    assert limbs[0, 1, 0, 0] == n                                        # a marker whose p is rejected still counts in markr
    assert int(limbs[1, 0, 0, 0]) * 2**32 + int(limbs[1, 1, 0, 0]) == 2 + 4 - 2 + 0
    for t in terms[:2] + terms[5:]:
        assert amd.diag_quantise(t, e_p) == int(Z.quantise(np.array([t]), e_p)[0][0])       # the very function the header names
    for t in terms[2:5]:
        with pytest.raises(amd.Pic1dpError):
            amd.diag_quantise(t, e_p)


# ---------------------------------------------------------------------------
# the conversion
# ---------------------------------------------------------------------------
def test_convert_of_rank_summed_limbs_is_the_conversion_of_their_sum(amd):
    inp = amd.make_input(nparticle_max=1000, nx=16)
    e_p, e_w = quanta(amd, inp)
    nxb, nvb = 4, 3
    rng = np.random.default_rng(9)
    base = [0, 1, -1, 2**53 + 1, -(2**53 + 1), 2**53 + 3, 2**32, -(2**32), 2**32 - 1, 2**60, -(2**60), (2**44 - 1) * 2**17]
    assert len(base) == nxb * nvb
    kw = dict(x=(1.0, 2.0), v=(0.0, 1.0), bins=(nxb, nvb))
    for ranks in (1, 2, 8):
        limbs = np.zeros((3, 2, nvb, nxb), dtype=np.int64)
        want = []
        for j in range(3):
            totals = [abs(base[(c + 5 * j) % len(base)]) if j == 0 else base[(c + 5 * j) % len(base)] for c in range(nxb * nvb)]
            for c, t in enumerate(totals):
                parts = [int(rng.integers(-2**40, 2**40)) for _ in range(ranks - 1)]
                parts.append(t - sum(parts))
                hi, lo = (sum(h) for h in zip(*(Z.limbs_of(s) for s in parts)))      # element-wise sums of normalised pairs
                assert hi * 2**32 + lo == t
                limbs[j, 0].flat[c], limbs[j, 1].flat[c] = hi, lo
            e = (0, e_p, e_w)[j]
            want.append(np.array([math.ldexp(float(t), e) for t in totals]).reshape(nvb, nxb))
        got = amd.zoom_convert(inp, limbs, which=7, **kw)
        assert list(got)[:3] == ["markr", "total", "pertb"]
        for j, name in enumerate(Z.PLANES):
            assert got[name].tobytes() == want[j].tobytes(), (ranks, name)
            assert got[name].shape == (nvb, nxb)
        one = amd.zoom_convert(inp, limbs[2:3], which=4, **kw)
        assert list(one)[:1] == ["pertb"] and one["pertb"].tobytes() == want[2].tobytes()
        two = amd.zoom_convert(inp, limbs[[0, 2]], which=5, **kw)
        assert two["markr"].tobytes() == want[0].tobytes() and two["pertb"].tobytes() == want[2].tobytes()
    assert float(2**53 + 1) == 2.0**53 and float(2**53 + 3) == 2.0**53 + 4                  # the ties go to even
    assert np.array_equal(got["x_edges"], 1.0 + np.arange(nxb + 1) / nxb) and got["v_edges"].shape == (nvb + 1,)
    with pytest.raises(ValueError):
        amd.zoom_convert(inp, limbs[:2], which=7, **kw)


# ---------------------------------------------------------------------------
# lengths and refusals
# ---------------------------------------------------------------------------
def test_lengths(amd):
    for which, n in ((1, 1), (2, 1), (4, 1), (3, 2), (5, 2), (6, 2), (7, 3)):
        assert amd.zoom_len((0.0, 1.0), (0.0, 1.0), (7, 5), which) == n * 35
        z, m = amd.Zoom(0.0, 1.0, 0.0, 1.0, 7, 5), C.c_int64()
        assert amd._lib.load().pic1dp_hip_zoom_limbs_len(C.byref(z), which, C.byref(m)) == 0 and m.value == 2 * n * 35
    assert amd.zoom_len((0.0, 1.0), (0.0, 1.0), (1024, 1024), 7) == 3 * 2**20
    assert amd.zoom_len((0.0, 1.0), (0.0, 1.0), (4096, 256), 1) == 2**20


def test_every_argument_error(amd):
    L = amd._lib.load()
    inp = amd.make_input(nparticle_max=1000, nx=16)
    full = amd.make_input(nparticle_max=10, nx=16, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    lx = inp.lx
    n = 4
    x, v, p, w = (np.zeros(n) for _ in range(4))
    limbs = np.full(3 * 2 * 16, -7, dtype=np.int64)
    rej = np.full(3, -7, dtype=np.int64)
    out = np.full(3 * 16, -7.0)
    P = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731

    def host(z, which=7, i=inp, isp=0, xs=x, np_=n, lim=limbs, rj=rej):
        return L.pic1dp_hip_host_zoom(C.byref(i) if i is not None else None, isp, C.byref(z) if z is not None else None, which,
                                      P(xs) if xs is not None else None, P(v), P(p), P(w), np_, P(lim) if lim is not None else None,
                                      P(rj) if rj is not None else None)

    def convert(z, which=7, i=inp, isp=0):
        return L.pic1dp_hip_zoom_convert(C.byref(i), isp, C.byref(z), which, P(limbs), P(out))

    ok = (1.0, 2.0, -1.0, 1.0, 4, 4)
    assert host(amd.Zoom(*ok)) == 0 and not np.any(limbs) and not np.any(rej)
    limbs[:], rej[:] = -7, -7
    bad = {"not finite": [(math.nan, 2.0, -1.0, 1.0, 4, 4), (1.0, INF, -1.0, 1.0, 4, 4), (1.0, 2.0, -INF, 1.0, 4, 4), (1.0, 2.0, -1.0, math.nan, 4, 4)],
           "[0, lx]": [(-1e-300, 2.0, -1.0, 1.0, 4, 4), (1.0, math.nextafter(lx, INF), -1.0, 1.0, 4, 4), (2 * lx, 1.0, -1.0, 1.0, 4, 4)],
           "v_lo < v_hi": [(1.0, 2.0, 1.0, 1.0, 4, 4), (1.0, 2.0, 1.0, -1.0, 4, 4)],
           "1..4096": [(1.0, 2.0, -1.0, 1.0, 0, 4), (1.0, 2.0, -1.0, 1.0, 4, 0), (1.0, 2.0, -1.0, 1.0, 4097, 1), (1.0, 2.0, -1.0, 1.0, 1, 4097), (1.0, 2.0, -1.0, 1.0, -1, 4)],
           "2^20": [(1.0, 2.0, -1.0, 1.0, 2048, 513), (1.0, 2.0, -1.0, 1.0, 4096, 257)],
           "extent": [(1.0, 2.0, -1.7e308, 1.7e308, 4, 4), (0.0, 5e-324, -1.0, 1.0, 4096, 4)]}
    for text, cases in bad.items():
        for zc in cases:
            for call in (host, convert):
                assert call(amd.Zoom(*zc)) == 1 and text.encode() in L.pic1dp_hip_last_error(), (zc, L.pic1dp_hip_last_error())
    for which in (0, 8, -1):
        for call in (host, convert):
            assert call(amd.Zoom(*ok), which=which) == 1 and b"which = %d" % which in L.pic1dp_hip_last_error()
        assert L.pic1dp_hip_zoom_len(C.byref(amd.Zoom(*ok)), which, C.byref(C.c_int64())) == 1
    for which in (4, 5, 6, 7):                                                             # pertb of a full-f input
        for call in (host, convert):
            assert call(amd.Zoom(*ok), which=which, i=full) == 1 and b"full-f" in L.pic1dp_hip_last_error()
    assert host(amd.Zoom(*ok), which=3, i=full) == 0
    limbs[:], rej[:] = -7, -7
    for call in (host, convert):
        assert call(amd.Zoom(*ok), isp=1) == 1 and call(amd.Zoom(*ok), isp=-1) == 1          # an unknown species
    assert host(None) == 1 and host(amd.Zoom(*ok), i=None) == 1 and host(amd.Zoom(*ok), xs=None) == 1          # null pointers
    assert host(amd.Zoom(*ok), lim=None) == 1 and host(amd.Zoom(*ok), rj=None) == 1 and host(amd.Zoom(*ok), np_=-1) == 1
    assert L.pic1dp_hip_zoom_convert(C.byref(inp), 0, C.byref(amd.Zoom(*ok)), 7, None, P(out)) == 1
    assert L.pic1dp_hip_zoom_convert(C.byref(inp), 0, C.byref(amd.Zoom(*ok)), 7, P(limbs), None) == 1
    assert L.pic1dp_hip_zoom_len(None, 7, C.byref(C.c_int64())) == 1 and L.pic1dp_hip_zoom_len(C.byref(amd.Zoom(*ok)), 7, None) == 1
    assert L.pic1dp_hip_zoom_limbs_len(None, 7, C.byref(C.c_int64())) == 1
    assert L.pic1dp_hip_zoom_len(C.byref(amd.Zoom(1.0, 2.0, -1.0, 1.0, 2048, 513)), 7, C.byref(C.c_int64())) == 1
    for f in (L.pic1dp_hip_zoom, L.pic1dp_hip_zoom_local_exact):
        assert f(None, 0, C.byref(amd.Zoom(*ok)), 7, P(out)) == 1 and b"null context" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_zoom_stats(None, None, None, None) == 1
    assert np.all(limbs == -7) and np.all(rej == -7) and np.all(out == -7.0)                # nothing was written by any refusal
    assert host(amd.Zoom(1.0, 1.0, -1.0, 1.0, 4, 4)) == 0 and not np.any(limbs)              # x_lo == x_hi: legal, empty


# ---------------------------------------------------------------------------
# the pass plan
# ---------------------------------------------------------------------------
def exact_blocks(np_, cu):
    return max(1, min(cu, -(-np_ // 2**17)))


def check_plan(pl, nxb, nvb, which, np_, cu, cap):
    n = bin(which).count("1")
    passes = pl["passes"]
    assert pl["selected"] == n and 1 <= len(passes) <= max(cap, 1)
    covered = np.zeros(nvb, dtype=int)
    for ps in passes:
        assert ps["planes"] == which and ps["threads"] == 1024 and ps["blocks"] == exact_blocks(np_, cu)
        assert ps["rows"] >= 1 and ps["first_row"] >= 0 and ps["first_row"] + ps["rows"] <= nvb
        covered[ps["first_row"]:ps["first_row"] + ps["rows"]] += 1
        if ps["lds"]:
            assert ps["bytes"] == 8 * n * ps["rows"] * nxb <= 8 * CAP_WORDS
        else:
            assert ps["bytes"] == 0 and len(passes) == 1 and ps["rows"] == nvb
        assert ps["nt"] == int(8 * (2 + bool(which & 2) + bool(which & 4)) * np_ > 288 * 2**20)
    assert np.all(covered == 1)                                           # the rows tile [0, nvb) exactly once per plane
    return [ps["lds"] for ps in passes]


def test_plan_on_both_sides_of_every_boundary(probe):
    cap = probe.host_zoom_plan(64, 64, 7, 1, 1000, 256)["pass_cap"]
    assert 1 <= cap <= 64
    np_ = 200_000
    # the grids of the issue
    assert check_plan(probe.host_zoom_plan(64, 64, 7, 1, np_, 256), 64, 64, 7, np_, 256, cap) == [1]               # 12 288 words fit
    pl = probe.host_zoom_plan(160, 160, 7, 1, np_, 256)
    assert [(ps["first_row"], ps["rows"]) for ps in pl["passes"]] == [(0, 40), (40, 40), (80, 40), (120, 40)] or cap < 4
    for nxb, nvb in ((1, 1), (1, 64), (64, 1), (1, 4096), (4096, 1)):
        for which in range(1, 8):
            assert check_plan(probe.host_zoom_plan(nxb, nvb, which, 1, np_, 256), nxb, nvb, which, np_, 256, cap) == [1]
    # fits / banded: the last grid of one pass and the first of two, per number of planes
    for which, n in ((1, 1), (3, 2), (7, 3), (4, 1), (6, 2)):
        for nxb in (1, 7, 64, 100, 4096):
            rows = CAP_WORDS // (n * nxb)
            if rows <= 4096:
                assert len(probe.host_zoom_plan(nxb, rows, which, 1, np_, 256)["passes"]) == 1
            if rows + 1 <= 4096 and nxb * (rows + 1) <= 2**20:
                pl = probe.host_zoom_plan(nxb, rows + 1, which, 1, np_, 256, pass_cap=2)
                assert [(ps["first_row"], ps["rows"], ps["lds"]) for ps in pl["passes"]] == [(0, rows, 1), (rows, 1, 1)]
            # banded / memory: exactly `c` bands still sweep bands, one row more goes to memory
            for c in (1, 2, cap, 16):
                nvb = c * rows
                if nvb <= 4096 and nxb * nvb <= 2**20:
                    got = check_plan(probe.host_zoom_plan(nxb, nvb, which, 1, np_, 256, pass_cap=c), nxb, nvb, which, np_, 256, c)
                    assert got == [1] * c
                if nvb + 1 <= 4096 and nxb * (nvb + 1) <= 2**20:
                    got = check_plan(probe.host_zoom_plan(nxb, nvb + 1, which, 1, np_, 256, pass_cap=c), nxb, nvb + 1, which, np_, 256, c)
                    assert got == [0]
    # the library's own cap, and 512 x 512 x 3: 12 rows a pass, 43 bands
    pl = probe.host_zoom_plan(512, 512, 7, 1, 10**8, 256)
    assert [ps["lds"] for ps in pl["passes"]] == ([0] if cap < 43 else [1] * 43)
    assert len(probe.host_zoom_plan(512, 12 * cap, 7, 1, 10**8, 256)["passes"]) == cap
    assert [ps["lds"] for ps in probe.host_zoom_plan(512, 12 * cap + 1, 7, 1, 10**8, 256)["passes"]] == [0]
    assert all(ps["nt"] == 1 for ps in pl["passes"]) and pl["passes"][0]["blocks"] == 256
    # a sweep: every property at many grids
    rng = np.random.default_rng(3)
    for _ in range(300):
        nxb, nvb = int(rng.integers(1, 4097)), int(rng.integers(1, 4097))
        if nxb * nvb > 2**20:
            nvb = max(1, 2**20 // nxb)
        which, c = int(rng.integers(1, 8)), int(rng.choice([0, 1, 3, 8, 64]))
        np_r, cu = int(rng.choice([0, 1, 2**17, 2**17 + 1, 10**6, 10**8])), int(rng.choice([8, 256]))
        check_plan(probe.host_zoom_plan(nxb, nvb, which, 1, np_r, cu, pass_cap=c), nxb, nvb, which, np_r, cu, c or cap)
    # the grid
    blocks = lambda np_, cu=256: probe.host_zoom_plan(64, 64, 7, 1, np_, cu)["passes"][0]["blocks"]   # noqa: E731
    assert [blocks(n) for n in (0, 1, 2**17, 2**17 + 1, 255 * 2**17, 255 * 2**17 + 1, 10**9)] == [1, 1, 1, 2, 255, 256, 256]
    assert blocks(10**8, 8) == 8 and blocks(100_001) == 1 and blocks(2**17 + 4097) == 2
    # no plan
    for args in ((0, 4, 7, 1), (4, 0, 7, 1), (4097, 1, 7, 1), (1, 4097, 7, 1), (2048, 513, 7, 1), (4, 4, 0, 1), (4, 4, 8, 1), (4, 4, 4, 0), (4, 4, 7, 0)):
        assert probe.host_zoom_plan(*args, 1000, 256)["passes"] == [], args
    assert len(probe.host_zoom_plan(4, 4, 3, 0, 1000, 256)["passes"]) == 1


# ---------------------------------------------------------------------------
# the stand-alone checker
# ---------------------------------------------------------------------------
def test_host_arithmetic_under_the_host_sanitizers(tmp_path):
    """tests/zoom_fx_check.cpp, a program of its own, built with AddressSanitizer and UndefinedBehaviorSanitizer (host code
    only; nothing of it touches a GPU): csrc/zoom_fx.cpp against __int128 arithmetic"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("pic1dp_amd_build", os.path.join(ROOT, "pic1dp_amd", "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    exe = str(tmp_path / "zoom_fx_check")
    subprocess.check_call([build.hipcc(), "--offload-arch=gfx950", "-x", "hip", "--offload-host-only", "-O1", "-g", "-std=c++17",
                           "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tests", "zoom_fx_check.cpp"), "-o", exe, "-lpthread"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failed"), r.stdout


# ---------------------------------------------------------------------------
# declared, bound, documented
# ---------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_documented(amd, probe):
    lib = C.CDLL(amd._lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    mod = open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_hip_mod.F90")).read()
    for name in ("zoom_len", "zoom_limbs_len", "zoom_local_exact", "zoom_convert", "zoom", "host_zoom", "zoom_stats"):
        assert hasattr(lib, "pic1dp_hip_" + name), name
        assert "pic1dp_hip_" + name in amd._lib.SIGNATURES, name
        assert re.search(r"\bint pic1dp_hip_%s\(" % name, header), name
        assert 'bind(C, name="pic1dp_hip_%s")' % name in mod, name
    assert callable(amd.Pic1dp.zoom) and callable(amd.Pic1dp.zoom_local_exact) and callable(amd.Pic1dp.zoom_stats)
    for name in ("zoom_convert", "host_zoom", "zoom_len"):
        assert callable(getattr(amd, name)) and name in amd.__all__
    assert "pic1dp_probe_host_zoom_plan" in open(os.path.join(ROOT, "include", "pic1dp_probe.h")).read()
    for line in ("ix   = (int)(d * sx);         if (ix > nxb - 1) ix = nxb - 1", "jv   = (int)((v - v_lo) * sv); if (jv > nvb - 1) jv = nvb - 1",
                 "limbs[((j * 2 + h) * nvb + jv) * nxb + ix]", "d    = px - x_lo;  if (d < 0) d = d + lx"):
        assert line in header, line
    assert "#define PIC1DP_ABI_VERSION" in header
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "2.20" in design and "zoom_plan" in design

"""The wave-particle power on the output grid (include/pic1dp_hip.h pic1dp_hip_power), the parts that need
no GPU: the declarations, power_len, tests/power_reference.py against a plain-Python evaluation marker by marker, and the pass
plan (pic1dp_amd/csrc/launch_policy.cpp power_plan, through the probe library) at its boundaries, values written out."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import power_reference as PR
from conftest import ROOT

CAP = 150 * 1024                   # launch_policy.hpp kDiagLdsCap = 153 600
NT_BYTES = 288 * 1048576           # the threshold of diag_launch


def tile(nx):
    return (8 * (nx + 1) + 15) // 16 * 16


def test_entry_points_are_declared_bound_and_documented(amd):
    lib = C.CDLL(amd._lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    fortran = open(os.path.join(ROOT, "pic1dp_amd", "fortran", "pic1dp_hip_mod.F90")).read()
    for name in ("pic1dp_hip_power", "pic1dp_hip_power_len"):
        assert hasattr(lib, name), name
        assert name in amd._lib.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
        assert 'name="%s"' % name in fortran, name
    assert callable(amd.Pic1dp.power)
    for line in ("e = E[ix] * wl;  e = e + E[ir] * (1.0 - wl)", "c = v * e", "t_q = c * q", "rest[q] += t_q",
                 "P[q][c00] += w00 * t_q    P[q][c01] += w01 * t_q    P[q][c10] += w10 * t_q    P[q][c11] += w11 * t_q"):
        assert line in header, line
    assert re.search(r"which = 20", header)
    probe_header = open(os.path.join(ROOT, "include", "pic1dp_probe.h")).read()
    assert "pic1dp_probe_host_power_plan" in probe_header


def power_len(amd, inp, which):
    n = C.c_int64(-1)
    rc = amd._lib.load().pic1dp_hip_power_len(C.byref(inp), which, C.byref(n))
    return rc, n.value


def test_power_len(amd):
    inp = amd.make_input(nparticle_max=10, nx_opd=64, nv_opd=64)
    assert power_len(amd, inp, 1) == (0, 64 * 64 + 64 + 1)
    assert power_len(amd, inp, 2) == (0, 64 * 64 + 64 + 1)
    assert power_len(amd, inp, 3) == (0, 2 * (64 * 64 + 64 + 1))
    inp = amd.make_input(nparticle_max=10, nx_opd=3, nv_opd=5)
    assert power_len(amd, inp, 3) == (0, 2 * (15 + 5 + 1)) and power_len(amd, inp, 2) == (0, 21)
    inp = amd.make_input(nparticle_max=10, nx_opd=1, nv_opd=2)
    assert power_len(amd, inp, 1) == (0, 2 + 2 + 1)
    L = amd._lib.load()
    for which in (0, 4, -1):
        assert power_len(amd, inp, which)[0] == 1 and b"which = %d" % which in L.pic1dp_hip_last_error()
    full = amd.make_input(nparticle_max=10, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    assert power_len(amd, full, 1)[0] == 0
    for which in (2, 3):
        assert power_len(amd, full, which)[0] == 1 and b"full-f" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_power_len(None, 1, C.byref(C.c_int64())) == 1 and b"null" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_power_len(C.byref(inp), 1, None) == 1 and b"null" in L.pic1dp_hip_last_error()
    for kw in (dict(nx_opd=0, nv_opd=8), dict(nx_opd=8, nv_opd=1)):
        bad = amd.make_input(nparticle_max=10)
        for k, val in kw.items():
            setattr(bad, k, val)
        assert power_len(amd, bad, 1)[0] == 1 and b"nx_opd >= 1 and nv_opd >= 2" in L.pic1dp_hip_last_error()


def crafted(inp, n_random=300, seed=11):
    """markers on every edge of both grids: x = 0, -0, lx, just below lx, the last field cell, wrapped positions; v = 0,
    +-v_max, one ulp on either side of +-v_max, far outside"""
    lx, nx, vm = inp.lx, inp.nx, inp.v_max
    below = math.nextafter(lx, 0.0)
    xs = [0.0, -0.0, lx, below, lx * (nx - 1) / nx + 0.25 * lx / nx, lx + 1e-13, -1e-300, 7.3 * lx, -7.3 * lx, 0.5 * lx / nx,
          lx / inp.nx_opd, math.nextafter(lx / inp.nx_opd, 0.0)]
    vs = [0.0, vm, -vm, math.nextafter(vm, 0.0), -math.nextafter(vm, 0.0), math.nextafter(vm, math.inf), -math.nextafter(vm, math.inf),
          2.0 * vm, -2.0 * vm, 0.3, -2.5]
    x = [xs[i % len(xs)] for i in range(len(xs) * len(vs))]
    v = [vs[i // len(xs)] for i in range(len(xs) * len(vs))]
    rng = np.random.default_rng(seed)
    x = np.concatenate([x, rng.uniform(-2.0 * lx, 3.0 * lx, n_random)])
    v = np.concatenate([v, rng.normal(0.0, 0.6 * vm, n_random)])
    p = rng.uniform(0.5, 1.5, x.size) * np.where(np.arange(x.size) % 5 == 3, -1.0, 1.0)
    w = rng.normal(0.0, 0.3, x.size)
    E = rng.normal(0.0, 1.0, nx) + 0.3
    return x, v, p, w, E


@pytest.mark.parametrize("nx,nxo,nvo", [(2, 1, 2), (3, 3, 5), (8, 64, 64), (77, 7, 9)])
def test_reference_equals_a_marker_by_marker_evaluation(amd, nx, nxo, nvo):
    inp = amd.make_input(nparticle_max=1000, nx=nx, nx_opd=nxo, nv_opd=nvo)
    x, v, p, w, E = crafted(inp)
    assert np.any(np.abs(v) >= inp.v_max) and np.any(E > 0) and np.any(E < 0)
    ref = PR.reference(x, v, p, w, E, inp, which=3)
    assert sorted(ref) == ["pertb", "total"]
    n_rest = int(np.count_nonzero(np.abs(v) >= inp.v_max))
    assert n_rest >= 6 * 12           # +-v_max, one ulp above, +-2 v_max -- and not one ulp below
    for name, q in (("total", p), ("pertb", w)):
        bins, rest = PR.python_power(x, v, q, E, inp)
        r = ref[name]
        assert r["exact"].shape == r["abs"].shape == r["count"].shape == (nvo, nxo)
        assert int(r["count"].sum()) == 4 * (x.size - n_rest) and r["rest"]["count"] == n_rest == len(rest)
        for b, ts in enumerate(bins):
            iv, ix = divmod(b, nxo)
            assert r["count"][iv, ix] == len(ts)
            assert r["exact"][iv, ix] == math.fsum(ts), (name, iv, ix)        # the very terms: the exact sums agree bit for bit
            s = math.fsum(abs(t) for t in ts)
            assert abs(r["abs"][iv, ix] - s) <= len(ts) * PR.U * s
        assert r["rest"]["exact"] == math.fsum(rest)
        # bins plus rest account for every marker: sum_i t_i, within the roundings of the four weights (which sum to 1 +- 3 ulp)
        _, c, _, _, _ = PR.gather(x, v, E, inp)
        tot = math.fsum((c * q).tolist())
        got = math.fsum(r["exact"].ravel().tolist()) + r["rest"]["exact"]
        assert abs(got - tot) <= 8 * PR.U * (r["abs"].sum() + r["rest"]["abs"]) + 1e-300
    assert list(PR.reference(x, v, p, w, E, inp, which=1)) == ["total"] and list(PR.reference(x, v, p, w, E, inp, which=2)) == ["pertb"]


def test_reference_of_one_marker_written_out(amd):
    """nx 4, a 2 x 3 output grid, one marker in the middle of field cell 1 at v = 0: everything by hand"""
    inp = amd.make_input(nparticle_max=10, nx=4, nx_opd=2, nv_opd=3)
    lx, vm = inp.lx, inp.v_max
    E = np.array([1.0, 2.0, -4.0, 8.0])
    x = 1.5 * lx / 4
    one = PR.reference([x], [0.5 * vm], [3.0], [0.0], E, inp, which=1)["total"]
    s = x / lx * 4.0
    wl = 1.0 - (s - 1.0)
    e = 2.0 * wl + -4.0 * (1.0 - wl)
    t = 0.5 * vm * e * 3.0
    sx = x / lx * 2.0              # output cell 0
    sx = 1.0 - sx
    sv = (0.5 * vm + vm) / (vm * 2.0) * 2.0      # row 1, half way to row 2
    sv = 1.0 - (sv - 1.0)
    want = np.zeros((3, 2))
    want[1, 0], want[2, 0], want[1, 1], want[2, 1] = sx * sv * t, sx * (1.0 - sv) * t, (1.0 - sx) * sv * t, (1.0 - sx) * (1.0 - sv) * t
    assert np.array_equal(one["exact"], want) and one["rest"]["count"] == 0 and int(one["count"].sum()) == 4
    out = PR.reference([x], [vm], [3.0], [0.0], E, inp, which=1)["total"]
    assert not np.any(out["exact"]) and out["rest"]["exact"] == vm * e * 3.0
    assert np.all(PR.bound(one, 1) <= 2.0 * PR.U * one["abs"] * (1 + 1e-6))


FIELDS = ("blocks", "threads", "nt", "bytes", "sets", "lds", "first_set", "nsets")


def passes(probe, nx, nxo, nvo, which, deltaf=1, np_=200_001, cu=256):
    return probe.host_power_plan(nx, nxo, nvo, which, deltaf, np_, cu)


def test_plan_at_the_boundaries_of_the_issue(probe):
    blocks = ((200_001 >> 1) + 1023) // 1024
    assert blocks == 98
    # nx 1024, 64 x 64, which 3: one pass, planes in LDS
    pl = passes(probe, 1024, 64, 64, 3)
    assert pl["tile"] == 8208 and pl["plane"] == 32768 and pl["selected"] == 2
    assert pl["passes"] == [dict(blocks=98, threads=1024, nt=0, bytes=8208 + 65536, sets=3, lds=1, first_set=0, nsets=2)]
    # nx 8192, 64 x 64, which 3: one pass; 65 552 + 65 536 = 131 088 <= 153 600
    pl = passes(probe, 8192, 64, 64, 3)
    assert pl["tile"] == 65552
    assert pl["passes"] == [dict(blocks=98, threads=1024, nt=0, bytes=131088, sets=3, lds=1, first_set=0, nsets=2)]
    # nx 8192, 96 x 96, which 3: 65 552 + 147 456 > cap, 65 552 + 73 728 = 139 280 <= cap: two passes, p then w
    pl = passes(probe, 8192, 96, 96, 3)
    assert pl["plane"] == 73728 and 65552 + 147456 > CAP and 139280 <= CAP
    assert pl["passes"] == [dict(blocks=98, threads=1024, nt=0, bytes=139280, sets=1, lds=1, first_set=0, nsets=1),
                            dict(blocks=98, threads=1024, nt=0, bytes=139280, sets=2, lds=1, first_set=1, nsets=1)]
    # nx 8192, 96 x 96, which 2: one pass
    pl = passes(probe, 8192, 96, 96, 2)
    assert pl["passes"] == [dict(blocks=98, threads=1024, nt=0, bytes=139280, sets=2, lds=1, first_set=0, nsets=1)]
    assert passes(probe, 8192, 96, 96, 1)["passes"] == [dict(blocks=98, threads=1024, nt=0, bytes=139280, sets=1, lds=1, first_set=0, nsets=1)]
    # nx 64, 160 x 160: the plane is 204 800 B: straight into memory, the tile alone in LDS
    for which, sets in ((1, 1), (2, 2), (3, 3)):
        pl = passes(probe, 64, 160, 160, which)
        assert pl["plane"] == 204800 and pl["tile"] == 528
        assert pl["passes"] == [dict(blocks=98, threads=1024, nt=0, bytes=528, sets=sets, lds=0, first_set=0, nsets=2 if which == 3 else 1)]


def test_plan_flips_at_the_exact_byte(probe):
    """tile + nsets plane <= cap: one pass; else tile + plane <= cap: a pass per set; else straight.  nv_opd = 2 makes a plane
    16 nx_opd bytes, the tile is 16-byte granular: both sides of every flip are reachable"""
    assert CAP == 153600
    nx = 1023                                   # tile = 8192 exactly
    assert tile(nx) == 8192 and tile(1024) == 8208 and tile(1) == 16 and tile(2) == 32
    room = CAP - 8192                            # 145 408 B for the planes
    # which 3, one pass <-> two passes: 2 plane <= room  <=>  16 nxo <= 72 704  <=>  nxo <= 4544
    assert 2 * 16 * 4544 == room
    pl = passes(probe, nx, 4544, 2, 3)
    assert [ps["bytes"] for ps in pl["passes"]] == [CAP] and pl["passes"][0]["lds"] == 1 and pl["passes"][0]["sets"] == 3
    pl = passes(probe, nx, 4545, 2, 3)
    assert [(ps["bytes"], ps["sets"], ps["lds"], ps["first_set"]) for ps in pl["passes"]] == [(8192 + 72720, 1, 1, 0), (8192 + 72720, 2, 1, 1)]
    # a pass per set <-> straight: plane <= room  <=>  nxo <= 9088
    assert 16 * 9088 == room
    for which, n in ((3, 2), (2, 1), (1, 1)):
        pl = passes(probe, nx, 9088, 2, which)
        assert [(ps["bytes"], ps["lds"]) for ps in pl["passes"]] == [(CAP, 1)] * n
        pl = passes(probe, nx, 9089, 2, which)
        assert [(ps["bytes"], ps["lds"], ps["nsets"]) for ps in pl["passes"]] == [(8192, 0, n)]
    # the tile's own 16 bytes: nx 1023 -> 1024 moves the tile by 16 B and takes the 4544-wide pair of planes out of one pass
    assert len(passes(probe, 1024, 4544, 2, 3)["passes"]) == 2 and len(passes(probe, 1022, 4544, 2, 3)["passes"]) == 1
    # the same rule, swept: every plan's bytes are its tile plus its planes, never beyond the cap
    for nx_ in (1, 2, 64, 1023, 1024, 8191, 8192):
        for nxo, nvo in ((1, 2), (3, 5), (64, 64), (96, 96), (97, 96), (128, 75), (160, 160), (4544, 2), (9089, 2)):
            for which in (1, 2, 3):
                pl = passes(probe, nx_, nxo, nvo, which)
                t, plane, ns = tile(nx_), 8 * nxo * nvo, 2 if which == 3 else 1
                assert (pl["tile"], pl["plane"], pl["selected"]) == (t, plane, ns)
                if t + ns * plane <= CAP:
                    want = [(t + ns * plane, 1, ns)]
                elif t + plane <= CAP:
                    want = [(t + plane, 1, 1)] * ns
                else:
                    want = [(t, 0, ns)]
                assert [(ps["bytes"], ps["lds"], ps["nsets"]) for ps in pl["passes"]] == want, (nx_, nxo, nvo, which)
                assert all(ps["bytes"] <= CAP and ps["threads"] == 1024 for ps in pl["passes"])
                assert sum(ps["nsets"] for ps in pl["passes"]) == ns


def test_plan_blocks_nt_and_refusals(probe):
    for np_, cu, want in ((0, 256, 1), (1, 256, 1), (2, 256, 1), (2049, 256, 1), (2050, 256, 2), (10**8, 256, 256), (10**8, 8, 8), (135171, 256, 67)):
        assert [ps["blocks"] for ps in passes(probe, 64, 64, 64, 3, np_=np_, cu=cu)["passes"]] == [want]
    # 24 B per marker with one weight set, 32 B with both; a pass per set reads 24 B
    for which, per in ((1, 24), (2, 24), (3, 32)):
        edge = NT_BYTES // per
        assert edge * per == NT_BYTES
        assert [ps["nt"] for ps in passes(probe, 1024, 64, 64, which, np_=edge)["passes"]] == [0]
        assert [ps["nt"] for ps in passes(probe, 1024, 64, 64, which, np_=edge + 1)["passes"]] == [1]
    edge = NT_BYTES // 24
    assert [ps["nt"] for ps in passes(probe, 8192, 96, 96, 3, np_=edge)["passes"]] == [0, 0]
    assert [ps["nt"] for ps in passes(probe, 8192, 96, 96, 3, np_=edge + 1)["passes"]] == [1, 1]
    for which in (0, 4, -1):
        assert passes(probe, 64, 64, 64, which)["passes"] == []
    assert passes(probe, 64, 64, 64, 2, deltaf=0)["passes"] == [] and passes(probe, 64, 64, 64, 3, deltaf=0)["passes"] == []
    assert len(passes(probe, 64, 64, 64, 1, deltaf=0)["passes"]) == 1
    assert passes(probe, 64, 0, 64, 1)["passes"] == [] and passes(probe, 64, 64, 1, 1)["passes"] == [] and passes(probe, 0, 64, 64, 1)["passes"] == []

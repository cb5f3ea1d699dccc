"""The velocity moments on the field grid, the parts that need no GPU: tests/moments_reference.py against a plain-Python
evaluation marker by marker, and the pass plan of pic1dp_hip_moments (pic1dp_amd/csrc/launch_policy.cpp moments_plan,
through the probe library) against its rule written out here."""
import math
import re
import os

import numpy as np
import pytest

import moments_reference as MR
from conftest import ROOT

DIAG_LDS_CAP = 150 * 1024          # launch_policy.hpp kDiagLdsCap
NT_BYTES = 288 * 1048576           # the threshold of diag_launch


def crafted(inp, n_random=300, seed=7):
    lx, nx = inp.lx, inp.nx
    below = math.nextafter(lx, 0.0)
    xs = [0.0, -0.0, lx, below, lx + 1e-13, -1e-300, 7.3 * lx, -7.3 * lx, 2.0 * lx - below, lx / nx, lx * (nx - 1) / nx,
          math.nextafter(lx * (nx - 1) / nx, lx), 0.5 * lx / nx]
    vs = [0.0, inp.v_max, -inp.v_max, 1e100, -1e100, 0.3, -2.5]
    qs = [1.0, -1.0, 0.0, 2.75, -0.125]
    x = [xs[i % len(xs)] for i in range(len(xs) * len(vs))]
    v = [vs[i // len(xs)] for i in range(len(xs) * len(vs))]
    rng = np.random.default_rng(seed)
    x = np.concatenate([x, rng.uniform(-2.0 * lx, 3.0 * lx, n_random)])
    v = np.concatenate([v, rng.normal(0.0, 3.0, n_random)])
    p = np.array([qs[i % len(qs)] for i in range(x.size)]) * rng.uniform(0.5, 1.5, x.size)
    w = np.array([qs[(i + 2) % len(qs)] for i in range(x.size)]) * rng.uniform(0.5, 1.5, x.size)
    return x, v, p, w


@pytest.mark.parametrize("nx", [2, 3, 8, 77])
def test_reference_equals_a_marker_by_marker_evaluation(amd, nx):
    inp = amd.make_input(nparticle_max=1000, nx=nx)
    x, v, p, w = crafted(inp)
    ref = MR.reference(x, v, p, w, inp, which=3)
    assert sorted(ref) == ["pertb", "total"]
    for name, q in (("total", p), ("pertb", w)):
        lists = MR.python_moments(x, v, q, inp)
        r = ref[name]
        assert r["exact"].shape == r["abs"].shape == (4, nx) and int(r["count"].sum()) == 2 * x.size
        for k in range(4):
            for b in range(nx):
                ts = lists[k][b]
                assert r["count"][b] == len(ts)
                assert r["exact"][k, b] == math.fsum(ts), (name, k, b)        # the very terms: the exact sums agree bit for bit
                s = math.fsum(abs(t) for t in ts)
                assert abs(r["abs"][k, b] - s) <= len(ts) * MR.U * s
    # which = 1, 2: the sets alone
    assert list(MR.reference(x, v, p, w, inp, which=1)) == ["total"] and list(MR.reference(x, v, p, w, inp, which=2)) == ["pertb"]
    # a single-term bin holds the term itself; the bound is a few units in its last place
    one = MR.reference([0.25 * inp.lx / nx], [1.5], [3.0], [0.0], inp, which=1)["total"]
    wl = 1.0 - (0.25 * inp.lx / nx / inp.lx * nx)
    assert one["exact"][2, 0] == wl * 3.0 * 1.5 * 1.5 and one["exact"][2, 1] == (1.0 - wl) * 3.0 * 1.5 * 1.5
    assert np.all(MR.bound(one, 1)[:, :2] <= 2.0 * 2.0 ** -53 * one["abs"][:, :2] * (1 + 1e-6))


def plan_rule(nx, which, deltaf, np_, num_cu):
    """the rule of the issue, written out: the selected planes in output order, groups of at most cap / (8 nx) planes, cut
    in output order, never across two weight sets unless all eight fit; powers {0, 1} then {2, 3} where four do not fit"""
    if which not in (1, 2, 3) or (which & 2 and not deltaf):
        return None
    sets = [s for bit, s in ((1, "p"), (2, "w")) if which & bit]
    planes = [(s, k) for s in sets for k in range(4)]
    g = min(DIAG_LDS_CAP // (8 * nx), len(planes))
    if g >= 8:
        groups = [planes]
    elif g >= 4:
        groups = [planes[i:i + 4] for i in range(0, len(planes), 4)]
    else:
        assert g >= 2
        groups = [planes[i:i + 2] for i in range(0, len(planes), 2)]
    blocks = max(1, min(num_cu, ((np_ >> 1) + 1023) // 1024))
    out = []
    first = 0
    for grp in groups:
        ss = {s for s, _ in grp}
        nbytes = 8 * (2 + len(ss)) * np_
        out.append(dict(blocks=blocks, threads=1024, nt=int(nbytes > NT_BYTES), bytes=8 * nx * len(grp),
                        sets=(1 if "p" in ss else 0) | (2 if "w" in ss else 0), kmask=sum(1 << k for k in {k for _, k in grp}),
                        first_plane=first, planes=len(grp)))
        first += len(grp)
    return out


@pytest.mark.parametrize("nx", [2, 3, 77, 192, 1024, 2048, 2049, 4096, 4800, 4801, 8192])
def test_pass_plan_follows_the_rule(probe, nx):
    seen = set()
    for which in (1, 2, 3):
        for deltaf in (0, 1):
            for np_, cu in ((0, 256), (1, 256), (2049, 8), (65537, 256), (10**8, 256), (10**8, 8)):
                got = probe.host_moments_plan(nx, which, deltaf, np_, cu)
                want = plan_rule(nx, which, deltaf, np_, cu)
                if want is None:
                    assert got["passes"] == []
                    continue
                assert got["passes"] == want, (nx, which, deltaf, np_, cu)
                assert got["selected"] == (8 if which == 3 else 4) and got["group"] == want[0]["planes"]
                for ps in got["passes"]:
                    assert 0 < ps["bytes"] <= DIAG_LDS_CAP and ps["blocks"] >= 1
                    seen.add((ps["sets"], ps["kmask"]))
                assert sum(ps["planes"] for ps in got["passes"]) == got["selected"]
    assert len(seen) <= 7
    # the table of the boundaries: passes for which = 3 and for one weight set
    n3, n1 = len(probe.host_moments_plan(nx, 3, 1, 65537, 256)["passes"]), len(probe.host_moments_plan(nx, 1, 1, 65537, 256)["passes"])
    assert (n3, n1) == ((1, 1) if 64 * nx <= DIAG_LDS_CAP else (2, 1) if 32 * nx <= DIAG_LDS_CAP else (4, 2))
    if nx in (2048, 4096, 8192):
        assert (n3, n1) == {2048: (1, 1), 4096: (2, 1), 8192: (4, 2)}[nx]
        assert probe.host_moments_plan(nx, 3, 1, 65537, 256)["passes"][0]["bytes"] == 128 * 1024


def test_pass_plan_instances_and_refusals(probe):
    combos = set()
    for nx in (192, 4096, 8192):
        for which in (1, 2, 3):
            for ps in probe.host_moments_plan(nx, which, 1, 10**6, 256)["passes"]:
                combos.add((ps["sets"], ps["kmask"]))
    assert combos == {(3, 0xF), (1, 0xF), (2, 0xF), (1, 0x3), (1, 0xC), (2, 0x3), (2, 0xC)}
    for which in (0, 4, -1):
        assert probe.host_moments_plan(192, which, 1, 1000, 256)["passes"] == []
    assert probe.host_moments_plan(192, 2, 0, 1000, 256)["passes"] == [] and probe.host_moments_plan(192, 3, 0, 1000, 256)["passes"] == []
    assert len(probe.host_moments_plan(192, 1, 0, 1000, 256)["passes"]) == 1


def test_non_temporal_loads_start_exactly_above_288_mib(probe):
    """24 B per marker with one weight set, 32 B with both"""
    for which, per in ((1, 24), (2, 24), (3, 32)):
        edge = NT_BYTES // per
        assert edge * per == NT_BYTES
        assert [ps["nt"] for ps in probe.host_moments_plan(1024, which, 1, edge, 256)["passes"]] == [0]
        assert [ps["nt"] for ps in probe.host_moments_plan(1024, which, 1, edge + 1, 256)["passes"]] == [1]
    # which = 3 beyond nx 2400: a pass per weight set, 24 B each
    edge = NT_BYTES // 24
    assert [ps["nt"] for ps in probe.host_moments_plan(4096, 3, 1, edge, 256)["passes"]] == [0, 0]
    assert [ps["nt"] for ps in probe.host_moments_plan(4096, 3, 1, edge + 1, 256)["passes"]] == [1, 1]


def test_entry_point_is_declared_bound_and_documented(amd):
    """the C symbol, the Python signature and the engine's method exist; the header states the definition the reference
    restates"""
    import ctypes as C
    assert hasattr(C.CDLL(amd._lib.LIB_PATH), "pic1dp_hip_moments")
    assert "pic1dp_hip_moments" in amd._lib.SIGNATURES and callable(amd.Pic1dp.moments)
    header = open(os.path.join(ROOT, "include", "pic1dp_hip.h")).read()
    for line in ("a0 = wl * q", "b0 = (1.0 - wl) * q", "a1 = a0 * v    a2 = a1 * v    a3 = a2 * v", "M[q][k][ix] += a_k            M[q][k][ir] += b_k"):
        assert line in header, line
    assert re.search(r"which = 16", header)

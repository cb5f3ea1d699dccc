"""The exact diagnostics reference (tests/diag_reference.py) on the host: against the C oracle's output_ptcldist and
kinetic sums (orc_ptcldist, orc_energy_sums through oracle.Sim) within the bound of a double sum, against Fraction
sums, at the edges of the grid, and fast enough for the GPU tests' 2^24-marker cases."""
import math
import time
from fractions import Fraction

import numpy as np
import pytest

import diag_reference as dr

LX_DEFAULT = 2.0 * 3.1415926535897932384626 / 0.36
GRIDS = [(64, 64), (3, 2), (7, 5), (16, 200), (40, 200)]


def oracle_diag(oracle_mod, x, v, p, w, lx, v_max, nxo, nvo, deltaf):
    n = x.size
    kw = dict(nparticle_max=n, lx=lx, v_max=v_max, nx_opd=nxo, nv_opd=nvo, deltaf=deltaf)
    if not deltaf:
        kw.update(iptcldist=0, species_density=[1.0], species_v0=[0.0])
    sim = oracle_mod.Sim(oracle_mod.make_input(**kw))
    assert sim.rank_nalloc(0) == n
    for k, a in zip("xvpw", (x, v, p, w)):
        sim.array(0, 0, k)[:] = a
    sim.set_rank_np(0, n)
    return sim.ptcldist(0, finish=False), sim.energy_sums(0)


def check_against_oracle(oracle_mod, x, v, p, w, lx, v_max, nxo, nvo, deltaf):
    ref = dr.reference(x, v, p, w, lx, v_max, nxo, nvo, deltaf)
    got, sums = oracle_diag(oracle_mod, x, v, p, w, lx, v_max, nxo, nvo, deltaf)
    for k in dr.PLANES:
        if k == "pertb_xv" and not deltaf or k == "pertb_v" and not deltaf:
            assert not np.any(got[k])
            continue
        err, bound = dr.error(got[k], ref[k]), dr.double_bound(ref[k], 0)
        assert np.all(err <= bound), (k, float(np.max(err - bound)))
    for k in range(3 if deltaf else 2):
        kin = ref["kinetic"][k]
        assert dr.error([sums[k]], kin)[0] <= dr.double_bound(kin, 0)[0], k
    return ref


def random_markers(n, lx, v_max, seed, spread=1.2):
    rng = np.random.default_rng(seed)
    x = rng.uniform(0.0, lx, n)
    v = rng.uniform(-spread * v_max, spread * v_max, n)
    p = rng.uniform(-3.0, 3.0, n)
    w = rng.normal(0.0, 0.5, n)
    return x, v, p, w


@pytest.mark.parametrize("deltaf", [1, 0], ids=["deltaf", "fullf"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
def test_reference_matches_the_oracle_on_random_markers(oracle_mod, grid, deltaf):
    """1e5 random markers (a fifth of them at |v| >= v_max), each grid, v_max and lx of the GPU tests in turn"""
    for i, (lx, v_max) in enumerate([(LX_DEFAULT, 8.0), (17.0, 10.0), (1.0 / 3.0, 7.3)]):
        x, v, p, w = random_markers(100_000 if i == 0 else 20_000, lx, v_max, 7 + i)
        check_against_oracle(oracle_mod, x, v, p, w, lx, v_max, *grid, deltaf)


@pytest.mark.parametrize("deltaf", [1, 0], ids=["deltaf", "fullf"])
@pytest.mark.parametrize("grid", GRIDS, ids=lambda g: "%dx%d" % g)
@pytest.mark.parametrize("lx", [LX_DEFAULT, 17.0, 1.0 / 3.0], ids=["lx_default", "lx17", "lx_third"])
@pytest.mark.parametrize("v_max", [8.0, 10.0, 7.3])
def test_reference_matches_the_oracle_at_the_edges(oracle_mod, grid, deltaf, lx, v_max):
    """the crafted edge markers of the GPU tests (x = 0, 5e-324, cell boundaries +- ulps, lx; v at the bin boundaries,
    the top-row velocities, +-v_max): the oracle and the reference keep the same markers in the same bins"""
    x, v, p, w = dr.edge_markers(lx, v_max, *grid)
    ref = check_against_oracle(oracle_mod, x, v, p, w, lx, v_max, *grid, deltaf)
    inside = np.count_nonzero(np.abs(v) < v_max)
    # every marker with |v| < v_max is in the histograms with its whole weight: the position edge (x == lx) folds to
    # cell 0, the velocity edge (sv == nv_opd - 1) stays in the top row
    assert float(sum(Fraction(n) for n in ref["markr_xv"]["ints"]) * Fraction(2) ** ref["markr_xv"]["e"]) == inside
    assert abs(ref["markr_v"]["value"].sum() - inside) <= 1e-12 * inside


def test_edge_markers_reach_both_edges():
    for v_max, nvo in [(8.0, 64), (10.0, 5), (8.0, 200), (10.0, 2)]:      # (v_max = 7.3 has no such velocity)
        top = dr.top_velocities(v_max, nvo)
        assert top and all(v < v_max for v in top), (v_max, nvo)
        _, _, _, iv, _, _, sv = dr.bins(np.zeros(len(top)), np.array(top), 1.0, v_max, 3, nvo)
        assert np.all(iv == nvo - 1) and np.all(sv == 1.0)
    xs = dr.edge_positions(17.0, 7)
    assert 17.0 in xs and 5e-324 in xs and 0.0 in xs
    _, ix, _, _, _, sx, _ = dr.bins(np.array([17.0]), np.array([0.0]), 17.0, 8.0, 7, 5)
    assert ix[0] == 0 and sx[0] == 1.0


def fraction_sums(x, v, p, w, lx, v_max, nxo, nvo):
    """the (x, v) and v histograms and kinetic sums by Python Fractions, marker by marker, with the same float64 terms"""
    xv = [[Fraction(0)] * (nxo * nvo) for _ in range(3)]
    vh = [[Fraction(0)] * nvo for _ in range(3)]
    kin = [Fraction(0)] * 3
    for xi, vi, pi, wi in zip(*(map(float, a) for a in (x, v, p, w))):
        v2 = vi * vi
        for k, t in enumerate((v2, v2 * pi, v2 * wi)):
            kin[k] += Fraction(t)
        if abs(vi) >= v_max:
            continue
        sx = xi / lx * float(nxo)
        ix = math.floor(sx)
        sx = 1.0 - (sx - ix)
        if ix == nxo:
            ix = 0
        sv = (vi + v_max) / (v_max * 2.0) * float(nvo - 1)
        iv = math.floor(sv)
        sv = 1.0 - (sv - iv)
        ivu = min(iv + 1, nvo - 1)
        ixr = 0 if ix + 1 > nxo - 1 else ix + 1
        for cell, wt in ((iv * nxo + ix, sx * sv), (ivu * nxo + ix, sx * (1.0 - sv)),
                         (iv * nxo + ixr, (1.0 - sx) * sv), (ivu * nxo + ixr, (1.0 - sx) * (1.0 - sv))):
            for k, t in enumerate((wt, wt * pi, wt * wi)):
                xv[k][cell] += Fraction(t)
        for row, wt in ((iv, sv), (ivu, 1.0 - sv)):
            for k, t in enumerate((wt, wt * pi, wt * wi)):
                vh[k][row] += Fraction(t)
    return xv, vh, kin


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "random"])
def test_exact_sums_equal_fraction_sums(dyadic):
    """on 3000 markers the limb sums are the Fraction sums: equal where every term is a whole number of quanta
    (dyadic positions and weights), within the reference's own count 2^(e-1) otherwise"""
    lx, v_max, nxo, nvo = (16.0, 8.0, 16, 17) if dyadic else (17.0, 7.3, 7, 5)
    x, v, p, w = random_markers(3000, lx, v_max, 3)
    x, v = np.concatenate([x, dr.edge_positions(lx, nxo)]), np.concatenate([v, np.zeros(len(dr.edge_positions(lx, nxo)))])
    n = x.size
    p, w = np.resize(p, n), np.resize(w, n)
    if dyadic:
        x, v = np.round(x * 64) / 64, np.round(v * 64) / 64
        p, w = np.round(p * 2**20) / 2**20, np.round(w * 2**20) / 2**20
    ref = dr.reference(x, v, p, w, lx, v_max, nxo, nvo, 1, chunk=1000)
    xv, vh, kin = fraction_sums(x, v, p, w, lx, v_max, nxo, nvo)
    names = ("markr", "total", "pertb")
    for k in range(3):
        for plane, want in ((ref[names[k] + "_xv"], xv[k]), (ref[names[k] + "_v"], vh[k]), (ref["kinetic"][k], [kin[k]])):
            q = Fraction(2) ** plane["e"]
            for b, f in enumerate(want):
                d = abs(Fraction(plane["ints"][b]) * q - f)
                if dyadic:
                    assert d == 0, (k, b)
                else:
                    assert d <= plane["count"][b] * q / 2, (k, b)
            if dyadic:
                assert not np.any(plane["qerr"])


def test_reference_of_2_24_markers_in_15_s():
    n = 1 << 24
    x, v, p, w = random_markers(n, 17.0, 8.0, 11, spread=0.5)
    t0 = time.perf_counter()
    ref = dr.reference(x, v, p, w, 17.0, 8.0, 64, 64, 1)
    dt = time.perf_counter() - t0
    assert int(ref["markr_xv"]["count"].sum()) == 4 * n
    assert dt <= 15.0, dt


def test_one_marker_fails_the_double_bound_by_100x():
    """the sensitivity the GPU scale tests rely on: taking one marker out of the reference leaves some bin outside the
    double-sum bound by 100x"""
    n = 1 << 20
    x, v, p, w = random_markers(n, LX_DEFAULT, 8.0, 5, spread=0.5)
    full = dr.reference(x, v, p, w, LX_DEFAULT, 8.0, 64, 64, 1)
    less = dr.reference(x[1:], v[1:], p[1:], w[1:], LX_DEFAULT, 8.0, 64, 64, 1)
    for k in dr.PLANES:
        b = dr.double_bound(less[k], 256, 64)
        ratio = np.max(dr.error(full[k]["value"], less[k])[b > 0] / b[b > 0])
        assert ratio >= 100.0, (k, ratio)

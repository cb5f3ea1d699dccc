"""The exact charge sum (kind 1 of include/pic1dp_hip.h set_charge_sum) on the host: the test helper's restatement
against plain Python-int arithmetic, and the quantum rule pic1dp_hip_charge_quantum against the loader's markers."""
import ctypes as C

import numpy as np
import pytest

import exact_charge as X
from conftest import DIST_CASES


def crafted(inp, e, n=4000, seed=7):
    """random markers plus the awkward ones: both edge cells, x = 0, x = lx, ties at half a quantum, +-0, negative
    weights"""
    rng = np.random.default_rng(seed)
    lx = inp.lx
    x = list(rng.uniform(-0.5 * lx, 1.5 * lx, n)) + [0.0, -0.0, lx, lx * (1 - 2 ** -52), lx / inp.nx, lx - lx / inp.nx, 2 * lx]
    q = list(rng.normal(0.0, 1.0, n) * 2.0 ** (e + 40))
    q += [2.0 ** (e + 52), -(2.0 ** (e + 52)), 0.0, -0.0, 1.5 * 2.0 ** e, 2.5 * 2.0 ** e, -0.5 * 2.0 ** e]
    # exact ties: a weight 2^(e+k) + half a quantum at a marker whose left weight is 1 (x on a cell edge)
    x += [0.0, 0.0, lx / inp.nx]
    q += [2.0 ** (e + 3) + 0.5 * 2.0 ** e, -(2.0 ** (e + 7)) - 0.5 * 2.0 ** e, 3.5 * 2.0 ** e]
    return np.array(x), np.array(q)


@pytest.mark.parametrize("nx", [2, 3, 64, 1024])
def test_helper_agrees_with_python_ints(amd, nx):
    inp = amd.make_input(nx=nx)
    e = amd.charge_quantum(inp, 0)
    x, q = crafted(inp, e)
    hi, lo = X.species_limbs(x, q, inp, e)
    assert X.totals(hi, lo) == X.python_int_totals(x, q, inp, e)
    nh, nl = X.normalise(hi, lo)
    assert np.all((nl >= 0) & (nl < 2 ** 32)) and X.totals(nh, nl) == X.totals(hi, lo)
    # the conversion: one rounding of the exact integer (a few totals beyond 2^53 included)
    t = X.totals(hi, lo) + [(1 << 60) + 1, -(1 << 60) - 3, (1 << 53) + 1, -(1 << 80) + 12345]
    for v in t:
        assert float(v) == float(round(v))   # (float(int) is the reference the library's conversion must meet)


def test_quantum_ignores_the_rank_split_and_bounds_the_markers(amd):
    import test_host_logic as H   # (the host loader's wrapper)
    L = amd._lib.load()
    for _, kw in DIST_CASES:
        for linear in (0, 1):
            inp = amd.make_input(nparticle_max=20000, nx=64, linear=linear, **kw)
            e = amd.charge_quantum(inp, 0)
            for mype, npe in ((0, 1), (1, 2), (3, 4)):
                inp2 = amd.make_input(nparticle_max=20000, nx=64, linear=linear, **kw)
                assert amd.charge_quantum(inp2, 0) == e
                (x, v, p, w), n = H.host_load(amd, inp2, mype, npe)
                bound = 2.0 ** (e + 52)
                assert np.max(np.abs(p)) <= bound and np.max(np.abs(w)) <= bound
                assert np.max(np.abs(p)) > bound / 2 ** 12   # a bound, not a guess orders of magnitude off
    got = C.c_int32()
    inp = amd.make_input()
    assert L.pic1dp_hip_charge_quantum(C.byref(inp), 3, C.byref(got)) == 1   # no such species


def test_quantum_of_two_species(amd):
    inp = amd.make_input(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 1836.0],
                         species_density=[1.0, 1.0], species_nparticle_init=[6400000, 6400000], species_temperature=[1.0, 1.0],
                         nparticle_max=12800000, iptcldist=0, species_v0=[0.0, 0.0])
    e0, e1 = amd.charge_quantum(inp, 0), amd.charge_quantum(inp, 1)
    assert e1 > e0   # the heavy species' narrower Maxwellian has the higher peak

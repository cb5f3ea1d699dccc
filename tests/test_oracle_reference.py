"""The oracle against the reference's own hot path: its load, deposit, push, field solve, marker optimisation and
|delta f|(v) sources compiled where they lie behind a serial PETSc stand-in (oracle/petsc_standin, oracle/Makefile target
ref), one library per case of oracle/ref_cases.json.  Every stage of tests/ref_hotpath.py, bit for bit: live against the
libraries in oracle/_ref (about 20 011 markers; skipped where they are not built), and against the records those
libraries wrote into tests/golden/ (4 096 markers; always).  CPU only."""
import json
import os

import numpy as np
import pytest

import ref_hotpath
from util import ulp_diff

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle", "ref_cases.json")) as _f:
    CASES = list(json.load(_f)["cases"])


def live(oracle, case):
    if not oracle.Ref.available(case):
        pytest.skip("oracle/_ref holds no library for %s (no reference tree or no flang where it was built)" % case)
    return oracle.Ref.get(case)


def test_cases_cover_the_shared_distributions(oracle_mod):
    """the cases the comparison is made for: the seven shared distributions, linear, full-f, two species, three kept
    modes on an odd grid, the shape arrays, and merge + remove (both types) + split events, with one and two species"""
    from conftest import DIST_CASES
    for name, kw in DIST_CASES:
        got = oracle_mod.ref_case_kwargs(name)
        assert {k: got[k] for k in kw} == kw and got["nparticle_max"] == 20011 and got["nx"] == 64
        assert oracle_mod.ref_case_values(name)["iptclshape"] == 4
    v = oracle_mod.ref_case_values
    assert v("linear")["linear"] == 1 and v("full_f")["deltaf"] == 0 and v("two_species")["nspecies"] == 2
    assert v("three_modes_odd_nx")["nmode"] == 3 and v("three_modes_odd_nx")["nx"] % 2 == 1
    assert v("shape3")["iptclshape"] == 3
    assert v("optimize")["nmerge"] and v("optimize")["nremove"] and v("optimize")["nsplit"]
    assert {v("optimize")["typeremove"], v("optimize_threshold")["typeremove"]} == {1, 2}
    two = v("optimize_two_species")
    assert two["nspecies"] == 2 and two["species_charge"] == [-1.0, 1.0] and two["species_mass"] == [1.0, 4.0]
    assert two["nmerge"] and two["nremove"] and two["nsplit"] and two["typeremove"] == 2 and two["iptcldist"] == 0
    assert two["tmerge"][0] == two["tremove"][0] == two["tsplit"][0] == 0.3
    for name in CASES:
        assert v(name + "_small")["nparticle_max"] <= 4096


def test_missing_library_is_reported(oracle_mod):
    assert not oracle_mod.Ref.available("no_such_case")
    with pytest.raises(oracle_mod.RefUnavailable):
        oracle_mod.Ref("no_such_case")


def test_reference_build_uses_the_host_libm(oracle_mod):
    """the one place a compiler could come between source and result: the run-time exp of the reference's build, element
    by element and as an array expression, against the host libm's on the weight equation's argument range, and its cos /
    sin pair (the loader's, which a compiler may merge into sincos) against libm's cos and sin.  Measured distance: 0 ulp
    each -- so every comparison below demands bits; a build where this fails needs the measured distance in the w rule"""
    ref = live(oracle_mod, "bump_on_tail")
    rng = np.random.default_rng(7)
    x = np.concatenate([-260.0 * rng.random(1_000_000), -rng.random(300_000) ** 4, -745.0 * rng.random(200_000),
                        700.0 * rng.random(200_000), -np.logspace(-300, 2, 20001), [0.0, -0.0]])
    want = np.empty_like(x)
    oracle_mod.lib().orc_exp_array(x, want, x.size)
    for vector in (False, True):
        d = ulp_diff(ref.exp(x, vector), want)
        print("reference build exp (array expression: %s) vs libm: max %d ulp" % (vector, d.max()))
        assert d.max() == 0
    t = np.concatenate([rng.uniform(-50.0, 50.0, 1_000_000), 2 * np.pi * rng.random(500_000)])
    c, s = ref.cos_sin(t)
    dc, ds = ulp_diff(c, np.cos(t)).max(), ulp_diff(s, np.sin(t)).max()
    print("reference build cos / sin pair vs libm: max %d / %d ulp" % (dc, ds))
    assert dc == 0 and ds == 0


@pytest.mark.parametrize("case", CASES)
def test_oracle_against_live_reference(oracle_mod, case):
    """load (and the stream after it), deposit (loaded, pushed, far-out positions), both pushes with imposed fields
    (x, v, w, xb, vb, wb), field solve with its tables, the optimisation event (markers, counts, stream), |delta f|(v),
    one step and 20 steps through the driver's call sequence: bit for bit"""
    ref = live(oracle_mod, case)
    rec = ref_hotpath.record(ref)
    ref_hotpath.check_oracle(rec, oracle_mod, ref.inp)


@pytest.mark.parametrize("case", CASES)
def test_oracle_against_recorded_reference(oracle_mod, case):
    """the same stages against what the reference's modules wrote into tests/golden/ref_hotpath_<case>.npz: the pin
    holds on a checkout without the reference"""
    with np.load(ref_hotpath.fixture_path(case)) as f:
        rec = {k: f[k] for k in f.files}
    inp = oracle_mod.make_input(**oracle_mod.ref_case_kwargs(case + "_small"))
    ref_hotpath.check_oracle(rec, oracle_mod, inp)


@pytest.mark.parametrize("case", CASES)
def test_recorded_reference_is_what_the_live_one_writes(oracle_mod, case):
    ref = live(oracle_mod, case + "_small")
    rec = ref_hotpath.record(ref)
    with np.load(ref_hotpath.fixture_path(case)) as f:
        assert sorted(f.files) == sorted(rec)
        for k in f.files:
            assert np.array_equal(f[k], rec[k]), k


def test_shape_arrays_and_on_the_fly_shape_record_the_same():
    """the reference's iptclshape 3 (cell and weight kept in arrays between deposit and push) and 4 (formed where
    needed) are the same arithmetic: their records agree in every array, which is why the engine, built for 4 only, is
    held to both"""
    with np.load(ref_hotpath.fixture_path("shape3")) as a, np.load(ref_hotpath.fixture_path("bump_on_tail")) as b:
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k]), k

"""The planted edge markers of tests/test_gpu_step_lockstep.py stay on their edges: the census of the ORACLE's state
before every step (tests/step_lockstep.py), checked here without a GPU.  A one-pass step of the library is predicted from
the second step on (the first step after an upload has no prediction to start from), so every class of edge has to be
present at the start of a step later than the first -- a planted set that drifts off its edges fails here instead of
passing quietly on the GPU.  Linear delta-f: x and v do not depend on the field, so the oracle's own run holds the very
positions the GPU test meets."""
import numpy as np
import pytest

import step_lockstep as ls

NSTEPS = 10          # the steps the GPU test takes: the ladder puts a marker on x == lx at the start of steps 2 .. 9


def planted_sim(oracle_mod, **kw):
    sim = oracle_mod.Sim(oracle_mod.make_input(nparticle_max=ls.N_SWEEP, **kw))
    assert sim.load() == 0
    pop = ls.sim_plant(sim)
    sim.collect_charge()
    sim.solve_field()
    return sim, pop


def run_census(sim, nsteps):
    out = []
    for _ in range(nsteps):
        out.append(ls.sim_census(sim))
        sim.step(1)
    return out


def test_planted_slots():
    """where the planted set goes: the head (slots 0, 1, 126 .. 129), an odd start in the middle, the far end of the
    slab, the last slot"""
    lx, nx, n = ls.EDGE_DYADIC["lx"], ls.EDGE_DYADIC["nx"], ls.N_SWEEP
    rng = np.random.default_rng(0)
    base = dict(x=rng.uniform(0.01, 0.02, n), v=rng.uniform(1, 2, n), p=np.full(n, 3.0), w=np.full(n, 5.0))
    pop = ls.plant(base, lx, nx)
    planted = np.flatnonzero(pop["p"] != 3.0)
    L = ls.edge_markers(lx, nx, n)[0].size
    assert planted.size == 4 * L and L > 130
    assert set(range(0, 130)) <= set(planted) and n - 1 in planted
    assert planted[L] & 1 and planted[L] > n // 2 - 2           # the middle block starts on the second marker of a pair
    assert np.sum(planted >= 3 * n // 4) == 2 * L               # the rows a narrow launch draws, and the tail
    assert pop["x"][0] == 0.0 and not np.signbit(pop["x"][0]) and np.signbit(pop["x"][1])


def test_every_edge_class_is_present_at_a_predicted_step(oracle_mod):
    sim, pop = planted_sim(oracle_mod, **ls.EDGE_DYADIC)
    v0 = sim.gather("v")
    cs = run_census(sim, NSTEPS)
    for it, c in enumerate(cs):
        print(it, c)
    assert ls.missing_classes(cs[1:]) == []
    # and not at one step only: every class but x == lx (the ladder: steps 2 .. 9) at EVERY step, x == lx at eight
    for it, c in enumerate(cs):
        assert ls.missing_classes([c], [k for k in ls.CLASSES if k != "x_lx"]) == [], it
    assert [it for it, c in enumerate(cs) if c["x_lx"] > 0] == list(range(0, 9))
    assert np.array_equal(sim.gather("v").view(np.int64), v0.view(np.int64))          # linear: v never changes
    assert np.isfinite(sim.gather("w")).all() and np.isfinite(sim.gather("x")).all()


def test_general_geometry_holds_its_edges_at_the_first_step(oracle_mod):
    sim, pop = planted_sim(oracle_mod, **ls.EDGE_GENERAL)
    cs = run_census(sim, 3)
    assert ls.missing_classes(cs[:1], ls.CLASSES_FIRST_STEP) == []
    for k in "xvw":
        assert np.isfinite(sim.gather(k)).all(), k


def test_census_notices_a_set_that_drifts(oracle_mod):
    """the same set with a time step that is no power of two: dt v is no whole number of cells, the rings leave their
    boundaries after the first step and the census says so"""
    sim, pop = planted_sim(oracle_mod, **dict(ls.EDGE_DYADIC, dt=0.05))
    cs = run_census(sim, 4)
    missing = ls.missing_classes(cs[1:])
    assert "xh_zero" in missing or "xh_lx" in missing or "x_lx" in missing, missing

"""What a step launches, scenario by scenario: the launch counts of every marker kernel and of the counters beside them
(kernel_stats rows 0-7, 10, 11) and the name and bytes of the whole-step kernels launched last (kernel_bytes 3 / 4 / 6)
after a fixed script of calls, against tests/golden/step_launches.json -- recorded from the library as it stood before the
step path's decisions moved into step_plan.cpp (tests/golden/gen_step_launches.py, on a GPU).  The numbers are that
library's, not derived here: whatever changes which kernel a step runs, how often, or what it reports of it shows as a
difference in one of these rows.  nx 32 and 1001 markers (odd, below one workgroup), a few thousand where a scenario
needs them; one engine per scenario."""
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "step_launches.json")
ROWS = (0, 1, 2, 3, 4, 5, 6, 7, 10, 11)
ENV = ("PIC1DP_FUSE_SOLVE", "PIC1DP_PRED_KIND", "PIC1DP_PREDICT", "PIC1DP_CALL_PAIR", "PIC1DP_LAZY_CALLS", "PIC1DP_TAIL")
BASE = dict(nx=32, nparticle_max=1001, dt=0.05, ntime_max=100000, time_max=1000.0, output_interval=0.0)
OPT = dict(nparticle_max=3001, species_nparticle_init=[2001], nv=64, nmerge=1, tmerge=[0.12], thshmerge=[0.3])
TWO = dict(nspecies=2, species_nparticle_init=[1001, 1001], species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0],
           species_temperature=[1.0, 0.5], species_temperature2=[1.0, 0.5], species_density=[1.0, 1.0], species_v0=[0.0, 0.0],
           iptcldist=0)


NONPOW2 = dict(iptcldist=3, species_temperature=[1.3], species_temperature2=[0.7], species_mass=[1.1], species_density=[0.85],
               species_v0=[4.5])      # general divisor constants (the one-exp form of -f0'/f0 serves them too: nothing is carried)


def steps(n, times=1):
    def script(e):
        for _ in range(times):
            e.step(n)
    return script


def knob(name, *args):
    def script(e):
        getattr(e, name)(*args)
        e.step(5)
    return script


def output(fusion):
    """output_interval 0.2 at dt 0.05: output_all follows steps 4 and 8 -- the first falls inside a step(6), where the host
    cannot call it, the second at the end of the step(2) that follows"""
    def script(e):
        e.set_output_fusion(fusion)
        e.step(6)
        e.step(2)
        e.output_all()
        e.step(3)
    return script


def empty_first_species(e):
    """create() wants markers in every species: the first one's are taken away again (an upload with no valid marker)"""
    g = e.particles_download(0)
    e.particles_upload(g["x"], g["v"], g["p"], g["w"], 0, np_valid=0)
    assert e.local_sizes(0)[1] == 0 and e.local_sizes(1)[1] == 1001


def call_sites(e):
    for _ in range(4):
        for irk in (1, 2):
            e.interaction_push_particle(irk)
            e.interaction_collect_charge()
            e.field_solve_electric()


# name: (environment, input keywords, script[, what comes between particle_load and the first collect_charge])
SCENARIOS = {
    "default_step5": ({}, {}, steps(5)),
    "step1_five_times": ({}, {}, steps(1, 5)),
    "fuse_solve_0": ({"PIC1DP_FUSE_SOLVE": "0"}, {}, steps(5)),
    "tiles_1_mode": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=1, modes=[1]), steps(5)),
    "tiles_2_modes": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=2, modes=[1, 2]), steps(5)),
    "tiles_3_modes": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=3, modes=[1, 2, 3]), steps(5)),
    "tiles_4_modes": ({"PIC1DP_PRED_KIND": "1"}, dict(nmode=4, modes=[1, 2, 3, 4]), steps(5)),
    "predict_0": ({"PIC1DP_PREDICT": "0"}, {}, steps(5)),
    "step_mode_1": ({}, {}, knob("set_step_mode", 1)),
    "charge_sum_1": ({}, {}, knob("set_charge_sum", 1)),
    "field_transform_1": ({}, {}, knob("set_field_transform", 1)),
    "field_solver_1": ({}, {}, knob("set_field_solver", 1)),
    "launch_64_1": ({}, {}, knob("set_launch", 64, 1)),
    "output_fusion_0": ({}, dict(output_interval=0.2), output(0)),
    "output_fusion_1": ({}, dict(output_interval=0.2), output(1)),
    "output_fusion_2": ({}, dict(output_interval=0.2), output(2)),
    "output_fusion_1_two_passes": ({"PIC1DP_PREDICT": "0"}, dict(output_interval=0.2), output(1)),
    "optimisation_inside_the_call": ({}, OPT, steps(5)),
    "call_sites_pair_1": ({"PIC1DP_CALL_PAIR": "1"}, {}, call_sites),
    "call_sites_pair_0": ({"PIC1DP_CALL_PAIR": "0"}, {}, call_sites),
    "general_divisors_two_passes": ({"PIC1DP_PREDICT": "0"}, NONPOW2, steps(5)),
    "general_divisors_one_pass": ({}, NONPOW2, steps(5)),
    "two_workgroups": ({}, dict(nparticle_max=4001), steps(5)),
    "two_species_first_empty": ({}, TWO, steps(5), empty_first_species),
}


def observe(amd, setenv, delenv, name):
    """the scenario's engine after its script: the launches of ROWS in order; read, written, carry, name of kernel_bytes 3, 4, 6"""
    env, kw, script = SCENARIOS[name][:3]
    for k in ENV:
        delenv(k)
    for k, v in env.items():
        setenv(k, v)
    e = amd.Pic1dp(amd.make_input(**dict(BASE, **kw)))
    try:
        e.particle_load()
        for prepare in SCENARIOS[name][3:]:
            prepare(e)
        e.kernel_stats_enable(True)
        e.interaction_collect_charge()
        e.field_solve_electric()
        script(e)
        e.sync()
        return {"launches": [e.kernel_stats(r)[1] for r in ROWS],
                "bytes": [[e.kernel_bytes(w)[n] for n in ("read", "written", "carry", "name")] for w in (3, 4, 6)]}
    finally:
        e.close()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(GOLDEN))


def test_every_scenario_is_recorded(golden):
    assert set(golden) == set(SCENARIOS)


@pytest.mark.parametrize("name", sorted(SCENARIOS))
def test_the_step_launches_what_it_did(amd, monkeypatch, golden, name):
    got = observe(amd, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False), name)
    want = golden[name]
    assert len(want["launches"]) == len(ROWS)
    bad = {r: (g, w) for r, g, w in zip(ROWS, got["launches"], want["launches"]) if g != w}
    assert not bad, "kernel_stats rows (got, recorded): %r" % bad
    assert got["bytes"] == want["bytes"]

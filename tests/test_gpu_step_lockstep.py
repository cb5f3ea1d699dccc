"""Every whole-step marker kernel against the materialised sub-steps, marker by marker and bit for bit (DESIGN.md 2.2,
2.3: given E0 and Eh the whole-step kernels push with the reference's operations in its order; a cache policy changes no
value).  Engine `a` takes whole steps -- the tiles (k_step_one) with one, two and three kept modes, the six sums in
registers (k_step_sums, which forms Eh as A[i] re + B[i] im instead of reading it from a tile), the two-pass pair
k_step_half + k_step_full, and at the non-temporal size also the private sums (k_step_one<sums>) --, engine `b` the two
sub-steps of every step on a's fields, and where the case is small the oracle runs beside them on the same fields
(tests/step_lockstep.py).  On loader markers in a field of order 0.1, on planted edge markers that a PREDICTED step
meets (the census of tests/test_step_lockstep_host.py), and at the smallest marker count at which a launch streams
non-temporally, where the head of the slab goes through plain accesses and the rest through non-temporal ones."""
import time

import numpy as np
import pytest

import step_lockstep as ls
from conftest import DIST_CASES
from util import both_inputs

pytestmark = pytest.mark.gpu

N = ls.N_SWEEP
DIST = dict(DIST_CASES)
# (unequal densities: the load perturbs both species alike, and equal ones of opposite charge would cancel in the field)
TWO_SPECIES = dict(nspecies=2, iptcldist=0, species_charge=[-1.0, 1.0], species_mass=[1.0, 25.0],
                   species_temperature=[1.0, 0.5], species_temperature2=[1.0, 1.0], species_density=[1.0, 0.5],
                   species_v0=[0.0, 0.0], lx=4 * np.pi)


def kept_modes(modes):
    """the field keeps `modes`, and the load perturbs every one of them: amplitudes 0.2, 0.1, 0.1"""
    m = len(modes)
    return dict(nmode=m, modes=modes, init_nmode=m, init_mode=modes, init_mode_cos=[0.0] * m, init_mode_sin=[0.2, 0.1, 0.1][:m])


# (id, family, kernel pic1dp_hip_kernel_bytes names, input)
KERNELS = [
    ("tiles_one_mode", "tiles", None, dict(nx=96, **kept_modes([1]))),
    ("tiles_two_modes", "tiles", None, dict(nx=96, **kept_modes([1, 2]))),
    ("tiles_three_modes", "tiles", None, dict(nx=96, **kept_modes([1, 2, 5]))),
    ("register_sums_nx1024", "register_sums", None, dict(nx=1024, **kept_modes([1]))),
    ("own_choice_nx2543", "own_choice", "k_step_sums", dict(nx=2543, **kept_modes([1]))),     # the first grid the tiles do not hold
    ("two_pass", "two_pass", None, dict(nx=96, **kept_modes([1]))),
]
# (id, input, environment): an exp in both forms of -f0'/f0, constants that are no powers of two (the fast division with
# its fallback; with the reference's form: the species whose -f0'/f0 is carried through memory), linear, full-f, two species
PHYSICS = [
    ("bump", {}, {}),
    ("bump_ref_form", {}, dict(PIC1DP_DLNF0="ref")),
    ("bump_nonpow2", DIST["bump_nonpow2"], {}),
    ("bump_nonpow2_ref_form", DIST["bump_nonpow2"], dict(PIC1DP_DLNF0="ref")),
    ("bump_linear", dict(linear=1), {}),
    ("maxwellian_nonpow2", DIST["maxwellian_nonpow2"], {}),
    ("full_f", dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]), {}),
    ("two_species", dict(TWO_SPECIES, species_nparticle_init=[N, 70001]), {}),
]


def started(e):
    e.interaction_collect_charge()
    e.field_solve_electric()
    return e


def loaded_trio(oracle_mod, amd, monkeypatch, family, env, **kw):
    """a, b and the oracle on the loader's markers"""
    ls.family_env(monkeypatch, family, **env)
    o, g = both_inputs(oracle_mod, amd, **kw)
    a, b = amd.Pic1dp(g), amd.Pic1dp(g)
    for e in (a, b):
        e.particle_load()
        started(e)
    sim = oracle_mod.Sim(o)
    assert sim.load() == 0
    sim.collect_charge()
    return a, b, sim


@pytest.mark.parametrize("pname,pkw,env", PHYSICS, ids=[p[0] for p in PHYSICS])
@pytest.mark.parametrize("kname,family,kernel,kkw", KERNELS, ids=[k[0] for k in KERNELS])
def test_whole_step_equals_substeps_and_oracle(oracle_mod, amd, probe, monkeypatch, kname, family, kernel, kkw, pname, pkw, env):
    """loader markers, an odd count, a perturbation of order 0.2: E and the weight updates are of order 0.1 and the
    markers are visibly accelerated.  Four steps, three of them predicted."""
    monkeypatch.delenv("PIC1DP_DLNF0", raising=False)
    kw = dict(kkw, nparticle_max=N, **pkw)
    ns = kw.get("nspecies", 1)
    a, b, sim = loaded_trio(oracle_mod, amd, monkeypatch, family, env, **kw)
    E = a.get_field(chargeden=False)["electric"]
    assert 0.02 < np.max(np.abs(E)) < 5.0, np.max(np.abs(E))
    v0 = ls.valid(a, 0)["v"]
    nsteps = 4
    ls.lockstep(a, b, nsteps, ns, sim, probe)
    ls.assert_family_ran(a, family, nsteps, ns, kernel)
    if kw.get("linear", 0) == 0:
        assert np.max(np.abs(ls.valid(a, 0)["v"] - v0)) > 1e-3          # accelerated


@pytest.mark.parametrize("n", [1, 2, 127, 129])
@pytest.mark.parametrize("kname,family,kernel,kkw", KERNELS, ids=[k[0] for k in KERNELS])
def test_whole_step_tiny_counts(oracle_mod, amd, probe, monkeypatch, kname, family, kernel, kkw, n):
    """the scalar tail alone, one pair, one wave of pairs less one marker and plus one; the carried -f0'/f0"""
    kw = dict(kkw, nparticle_max=n, **DIST["bump_nonpow2"])
    a, b, sim = loaded_trio(oracle_mod, amd, monkeypatch, family, dict(PIC1DP_DLNF0="ref"), **kw)
    ls.lockstep(a, b, 4, 1, sim, probe)
    ls.assert_family_ran(a, family, 4, 1, kernel)


# --------------------------------------------------------------------------
# planted edge markers
# --------------------------------------------------------------------------
def planted_trio(oracle_mod, amd, monkeypatch, family, narrow, **kw):
    ls.family_env(monkeypatch, family)
    o, g = both_inputs(oracle_mod, amd, nparticle_max=N, **kw)
    sim = oracle_mod.Sim(o)
    assert sim.load() == 0
    pop = ls.sim_plant(sim)
    sim.collect_charge()
    a, b = amd.Pic1dp(g), amd.Pic1dp(g)
    for e in (a, b):
        e.particles_upload(pop["x"], pop["v"], pop["p"], pop["w"])
        started(e)
    if narrow:
        a.set_launch(64, 1)
    # the first deposit: far-out positions, x + lx -> lx, the signs of zero
    ls.assert_same_bits(ls.valid(a, 0)["x"], sim.gather("x"), "x after the first deposit")
    return a, b, sim


def assert_narrow_launch_draws(probe, family):
    """set_launch(64, 1): one workgroup of one wave per CU, so the 67 585 pairs are three rows and more for a workgroup
    on any GPU of up to 352 CUs, of which dyn_tail sixteenths are DRAWN chunk by chunk: the planted block in the last
    fifth of the slab and the one at its end lie in drawn rows"""
    tail = probe.host_settings()["dyn_tail_full" if family == "two_pass" else "dyn_tail"]
    assert (3 * tail) >> 4 >= 1, tail


EDGE_RUNS = [("tiles", False), ("tiles", True), ("private_sums", False), ("register_sums", False), ("register_sums", True),
             ("two_pass", False), ("two_pass", True)]      # (the private sums' workgroup size is fixed: no narrow launch)


@pytest.mark.parametrize("family,narrow", EDGE_RUNS, ids=["%s%s" % (f, "-narrow" if n else "") for f, n in EDGE_RUNS])
def test_planted_edges_at_predicted_steps(oracle_mod, amd, probe, monkeypatch, family, narrow):
    """linear delta-f in a geometry of powers of two: the planted markers sit on their edges at every step, so the
    one-pass kernels meet them in PREDICTED steps (the step after the upload takes two passes).  Ten steps, a, b and
    the oracle bit for bit after each, the sign of a zero position included; the census of the oracle's state shows
    every class of edge at the start of a predicted step."""
    if narrow:
        assert_narrow_launch_draws(probe, family)
    a, b, sim = planted_trio(oracle_mod, amd, monkeypatch, family, narrow, **ls.EDGE_DYADIC)
    cs = []
    nsteps = 10
    ls.lockstep(a, b, nsteps, 1, sim, probe, before_step=lambda it: cs.append(ls.sim_census(sim)))
    ls.assert_family_ran(a, family, nsteps)
    assert ls.missing_classes(cs[1:]) == []
    assert sum(c["x_lx"] > 0 for c in cs[1:]) == 8
    assert np.isfinite(ls.valid(a, 0)["w"]).all()


@pytest.mark.parametrize("family", ["two_pass", "tiles", "private_sums"])
def test_planted_edges_general_geometry(oracle_mod, amd, probe, monkeypatch, family):
    """nonlinear delta-f, nothing a power of two, species constants that take the fast division with its fallback: the
    edges are met at the first step -- k_step_half and the second kernel of the family -- and x, v AND w stay bit for
    bit over the steps that follow (no exp in this distribution)"""
    a, b, sim = planted_trio(oracle_mod, amd, monkeypatch, family, False, **ls.EDGE_GENERAL)
    cs = []
    ls.lockstep(a, b, 3, 1, sim, probe, before_step=lambda it: cs.append(ls.sim_census(sim)))
    ls.assert_family_ran(a, family, 3)
    assert ls.missing_classes(cs[:1], ls.CLASSES_FIRST_STEP) == []


# --------------------------------------------------------------------------
# the non-temporal instances
# --------------------------------------------------------------------------
N_NT = 9_437_185          # the smallest count with 32 n > 288 MiB; odd
NT_CASES = [
    ("tiles", "tiles", dict(nx=96, nparticle_max=N_NT)),
    ("private_sums", "private_sums", dict(nx=1024, nparticle_max=N_NT)),
    ("register_sums", "register_sums", dict(nx=1024, nparticle_max=N_NT)),
    ("two_pass", "two_pass", dict(nx=96, nparticle_max=N_NT)),
    ("two_species", "private_sums", dict(TWO_SPECIES, nx=1024, nparticle_max=6_291_457, species_nparticle_init=[6_291_457, 3_145_729])),
]


@pytest.mark.parametrize("name,family,kw", NT_CASES, ids=[c[0] for c in NT_CASES])
def test_non_temporal_instance_equals_plain_substeps(amd, probe, monkeypatch, name, family, kw):
    """the non-temporal instance of every whole-step kernel -- in the one-pass kernels with the head of the slab through
    plain accesses and the rest through non-temporal ones -- against b's sub-step kernels, which stay plain at this
    size (their threshold is 2 GiB): the same bits in x, v and w after each of three steps.  Loaded on the device (a
    host load of 9e6 markers takes longer than the test); no oracle at this size."""
    t0 = time.perf_counter()
    ls.family_env(monkeypatch, family)
    ns = kw.get("nspecies", 1)
    counts = kw["species_nparticle_init"] if ns > 1 else [kw["nparticle_max"]]
    settings = probe.host_settings()
    assert 32.0 * sum(counts) > settings["nt_threshold_full"]          # a's whole-step launches stream non-temporally
    assert 32.0 * sum(counts) <= settings["nt_threshold_half"]         # b's sub-step launches do not
    for n in counts:
        chunks = probe.host_plain_chunks(sum(counts), n)
        assert 0 < chunks < ((n >> 1) + 63) >> 6, (n, chunks)          # a plain head AND a streamed rest
    inp = amd.make_input(init_mode_sin=[0.2], **kw)
    a, b = amd.Pic1dp(inp), amd.Pic1dp(inp)
    for e in (a, b):
        e.particle_load_device(1)
        started(e)
    for s, n in enumerate(counts):
        assert a.local_sizes(s)[1] == n
    ls.lockstep(a, b, 3, ns)
    ls.assert_family_ran(a, family, 3, ns)
    print("%s: non-temporal launch of %s (%d B of state against %d), %.2f s" % (
        name, a.kernel_bytes(4 if family == "two_pass" else 6)["name"], 32 * sum(counts), settings["nt_threshold_full"],
        time.perf_counter() - t0))

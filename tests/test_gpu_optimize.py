"""Marker optimisation: particle_merge / particle_remove /
particle_split (src/pic1dp_particle.F90:356-813) through the engine against the
oracle.  The routines are sequential and run on the host inside the library; the
tests feed both sides identical markers right before an optimisation event and
require identical results (positions, velocities, weights, counts) -- one event,
two species, chains of events, markers beyond +-v_max and crafted ones on the v
grid's nodes and ends --, hold the steps around an event to the oracle and to one
another through every step path, and check whole runs statistically."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from ref_hotpath import assert_defined_in_reference
from util import both_inputs, relerr

pytestmark = pytest.mark.gpu


def synced_pair(oracle, amd, npe, **kw):
    o, g = both_inputs(oracle, amd, **kw)
    sim = oracle.Sim(o, npe=npe)
    assert sim.load() == 0
    eng = amd.Pic1dp(g, npe=npe)
    eng.particle_load()
    sim.collect_charge()
    sim.solve_field()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    return sim, eng


def compare_blocks(sim, eng, npe, isp=0):
    """valid markers of every block, in block order, bit for bit"""
    nalloc, npv = eng.local_sizes(isp)
    assert npv == sum(sim.rank_np(r, isp) for r in range(npe))
    got = eng.particles_download(isp)
    for k in "xvpw":
        assert np.array_equal(got[k][:npv], sim.gather(k, isp)), (k, isp)
    return npv


def species_counts(sim, npe):
    return [sum(sim.rank_np(r, isp) for r in range(npe)) for isp in range(sim.inp.nspecies)]


def align_markers(sim, eng, npe, names="xvpw"):
    """the engine's valid markers of every species onto the oracle's rank blocks (the engine keeps the valid markers of
    its blocks in block order; both sides hold the same count per block: every event before was compared)"""
    for isp in range(sim.inp.nspecies):
        got = eng.particles_download(isp)
        off = 0
        for r in range(npe):
            n = sim.rank_np(r, isp)
            for k in names:
                sim.array(r, isp, k)[:n] = got[k][off:off + n]
            off += n
        assert off == eng.local_sizes(isp)[1]


@pytest.mark.parametrize("kind,kw", [
    ("merge", dict(nmerge=1, tmerge=[0.3], thshmerge=[0.5])),
    ("merge_all", dict(nmerge=2, tmerge=[0.3, 0.4], thshmerge=[2.0, 2.0])),
    ("remove_profile", dict(nremove=1, tremove=[0.3], typeremove=2)),
    ("remove_threshold", dict(nremove=1, tremove=[0.3], typeremove=1, thshremove=[0.4], remove_frac=0.7)),
    ("split", dict(nsplit=1, tsplit=[0.3], thshsplit=[0.3], split_ngroup=3)),
    ("split_until_full", dict(nsplit=1, tsplit=[0.3], thshsplit=[0.01], split_ngroup=5)),
    ("all_three", dict(nmerge=1, tmerge=[0.3], thshmerge=[0.3], nremove=1, tremove=[0.3], typeremove=2,
                       nsplit=1, tsplit=[0.3], thshsplit=[0.6])),
], ids=lambda v: v if isinstance(v, str) else "")
@pytest.mark.parametrize("npe", [1, 3])
def test_optimisation_event_is_bit_identical(oracle_mod, amd, kind, kw, npe):
    base = dict(nparticle_max=60000, species_nparticle_init=[36000], nx=32, nv=64)
    n_after = aligned_event(oracle_mod, amd, npe, dict(base, **kw))[-1][0]
    if kind.startswith("merge") or kind.startswith("remove"):
        assert n_after < 36000
    if kind.startswith("split"):
        assert n_after > 36000


def aligned_event(oracle_mod, amd, npe, kw, times=(0.3,), pair=None, before_event=None, after_event=None):
    """Both sides through the events at `times` (every entry of tmerge / tremove / tsplit that is to fire, a time once
    however many kinds share it).  Steps without an event: step(1) on both sides.  A step in which one fires (t + dt >= the
    event's time on the library's clock, src/pic1dp_particle.F90:742-770): the engine's markers of every species and its
    field put on the oracle, then the step by hand on both sides through the call sites, w re-aligned after either push,
    and after the event every valid marker of every block and species bit for bit.  Returns the per-species counts after
    every event.  pair: a (sim, eng) of synced_pair to go on with afterwards; before_event(sim, eng, i) runs after the
    second push of event step i with both sides aligned, after_event(sim, eng, i) after the comparison."""
    sim, eng = pair if pair is not None else synced_pair(oracle_mod, amd, npe, **kw)
    ns, dt = sim.inp.nspecies, sim.inp.dt
    pending = sorted(times)
    counts = []
    for _ in range(200):
        if not pending:
            break
        assert eng.time == sim.time and eng.itime == sim.itime
        if not sim.time + dt >= pending[0]:
            # identical steps (they agree bit for bit in x, and in v and w to rounding)
            sim.step(1)
            eng.step(1)
            continue
        pending = [t for t in pending if not sim.time + dt >= t]
        align_markers(sim, eng, npe)
        sim.set_field(eng.get_field()["electric"])
        for irk in (1, 2):
            sim.push(irk)
            eng.interaction_push_particle(irk)
            # weights may differ in the last bits (exp): re-align after either push
            align_markers(sim, eng, npe, "w")
            if irk == 2 and before_event is not None:
                before_event(sim, eng, len(counts))
            did_o = sim.optimize(irk)
            did_g = eng.particle_optimize(irk)
            assert did_o == did_g == (irk == 2)
            if irk == 2:
                for isp in range(ns):
                    compare_blocks(sim, eng, npe, isp)
                counts.append(species_counts(sim, npe))
                if after_event is not None:
                    after_event(sim, eng, len(counts) - 1)
            sim.collect_charge()
            eng.interaction_collect_charge()
            sim.solve_field()
            eng.field_solve_electric()
            sim.set_field(eng.get_field()["electric"])
        assert relerr(eng.get_field()["chargeden"], sim.get_field()[1]) < 1e-11
        # nothing further is due in this step
        assert not eng.particle_optimize(2)
        # the driver's clock (src/pic1dp.F90:92-93), as a host that swaps the call sites keeps it
        t_next = sim.time + dt
        sim.set_time(sim.itime + 1, t_next)
        eng.set_time(eng.itime + 1, t_next)
    assert not pending and len(counts) == len(set(_event_steps(sim.inp, times)))
    return counts


def _event_steps(inp, times):
    """the step (counted from 0) in which each time fires, on the clock the drivers keep: t = t + dt from 0"""
    steps = []
    for T in times:
        t, it = 0.0, 0
        while not t + inp.dt >= T:
            t, it = t + inp.dt, it + 1
        steps.append(it)
    return steps


@pytest.mark.parametrize("threads", ["1", "2", "7"])
def test_event_walks_on_host_threads_change_nothing(oracle_mod, amd, monkeypatch, threads):
    """the blocks of an event are walked side by side on host threads (one random stream, one set of
    keys per block: the reference runs them as separate ranks, src/pic1dp_particle.F90:411-746) -- whatever the number
    of threads, every block bit for bit what the oracle's routines leave (seven blocks; one, two, seven workers)"""
    monkeypatch.setenv("PIC1DP_OPT_THREADS", threads)
    kw = dict(nparticle_max=70000, species_nparticle_init=[42000], nx=32, nv=64, nmerge=1, tmerge=[0.3], thshmerge=[0.3],
              nremove=1, tremove=[0.3], typeremove=2, nsplit=1, tsplit=[0.3], thshsplit=[0.6])
    aligned_event(oracle_mod, amd, 7, kw)


def random_event_case(rng):
    nmax = int(rng.integers(3000, 70000))
    ninit = int(nmax * rng.uniform(0.35, 1.0))
    kw = dict(nparticle_max=nmax, species_nparticle_init=[ninit], nx=int(rng.choice([4, 8, 32, 100])),
              nv=int(rng.choice([8, 16, 64, 128])), iptcldist=int(rng.choice([0, 2, 3, 3])))
    kinds = rng.permutation(["merge", "remove", "split"])[:int(rng.integers(1, 4))]
    for k in kinds:
        if k == "merge":
            kw.update(nmerge=1, tmerge=[0.3], thshmerge=[float(rng.choice([0.05, 0.3, 0.6, 2.0]))])
        elif k == "remove":
            kw.update(nremove=1, tremove=[0.3], typeremove=int(rng.choice([1, 2])),
                      thshremove=[float(rng.uniform(0.1, 0.8))], remove_frac=float(rng.uniform(0.2, 0.9)))
        else:
            kw.update(nsplit=1, tsplit=[0.3], thshsplit=[float(rng.choice([0.01, 0.2, 0.5, 0.9]))],
                      split_ngroup=int(rng.integers(2, 7)))
    return kw, int(rng.choice([1, 1, 2, 3, 5]))


_BASE = int(os.environ.get("PIC1DP_FUZZ_BASE", "0"))
_MULT = int(os.environ.get("PIC1DP_FUZZ_MULT", "1"))


@pytest.mark.parametrize("seed", range(_BASE, _BASE + 12 * _MULT))
def test_random_optimisation_events(oracle_mod, amd, seed):
    """seeded random events (kinds and their combinations, thresholds, both kinds of removal, group sizes, marker counts
    with and without free tail slots, grids, distributions, 1 ... 5 reference ranks) with the markers on the device,
    against the oracle on aligned inputs: every valid marker of every block bit for bit.  A longer campaign:
    PIC1DP_FUZZ_BASE=1000 PIC1DP_FUZZ_MULT=20 (as tests/test_gpu_fuzz.py)"""
    kw, npe = random_event_case(np.random.default_rng(77000 + seed))
    aligned_event(oracle_mod, amd, npe, kw)


def test_whole_step_path_runs_the_events(oracle_mod, amd):
    """pic1dp_hip_step notices due events and takes those steps through the
    sub-step kernels; marker counts follow the oracle's exactly as long as the
    thresholds are not borderline, energies statistically"""
    kw = dict(nparticle_max=200000, species_nparticle_init=[120000], nx=64, nv=64,
              nmerge=1, tmerge=[1.0], thshmerge=[0.2], nsplit=1, tsplit=[2.0], thshsplit=[0.5])
    sim, eng = synced_pair(oracle_mod, amd, 2, **kw)
    sim.step(60)
    eng.step(60)
    n_g = eng.local_sizes()[1]
    n_o = sim.rank_np(0) + sim.rank_np(1)
    assert n_g != 120000 and abs(n_g - n_o) <= 0.002 * n_o
    assert abs(eng.field_energy() / sim.field_energy() - 1.0) < 0.05
    assert relerr(eng.energy_sums(), sim.energy_sums()) < 1e-2


def test_optimisation_needs_loader_stream_and_delta_f(amd):
    inp = amd.make_input(nparticle_max=2000, nx=16, nv=32, nremove=1, tremove=[0.05])
    eng = amd.Pic1dp(inp)
    n = 2000
    rng = np.random.default_rng(0)
    eng.particles_upload(rng.uniform(0, inp.lx, n), rng.uniform(-8, 8, n), rng.uniform(0.5, 1, n),
                         rng.uniform(-1e-3, 1e-3, n))
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.interaction_push_particle(1)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    eng.interaction_push_particle(2)
    with pytest.raises(amd.Pic1dpError) as ei:      # remove needs the block's random stream
        eng.particle_optimize(2)
    assert ei.value.code == 4
    full_f = amd.Pic1dp(amd.make_input(nparticle_max=2000, nx=16, nv=32, nmerge=1, tmerge=[0.05], deltaf=0,
                                       iptcldist=0, species_density=[1.0], species_v0=[0.0]))
    full_f.particle_load()
    full_f.interaction_collect_charge()
    full_f.field_solve_electric()
    full_f.step(3)
    assert full_f.local_sizes()[1] == 2000            # "now only support optimization for delta f"


def test_call_site_path_needs_the_library_clock(amd):
    """a host that swaps only the call sites must hand its clock to the
    library after every step (pic1dp_hip_set_time) -- particle_optimize compares the event times
    with the library's time + dt like src/pic1dp_particle.F90:742-770 with global_time + dt.  With
    the clock the merge fires in the same step as under pic1dp_hip_step; without it, never."""
    kw = dict(nparticle_max=120000, species_nparticle_init=[90000], nx=32, nv=64, nmerge=1, tmerge=[0.2],
              thshmerge=[0.3])

    def fresh():
        e = amd.Pic1dp(amd.make_input(**kw))
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        return e

    def drive(e, nsteps, clock):
        fired = []
        for it in range(nsteps):
            for irk in (1, 2):
                e.interaction_push_particle(irk)
                if e.particle_optimize(irk):
                    fired.append(it)
                e.interaction_collect_charge()
                e.field_solve_electric()
            if clock:
                e.set_time(e.itime + 1, e.time + e.inp.dt)
        return fired

    ref = fresh()
    counts = []
    for it in range(6):
        ref.step(1)
        counts.append(ref.local_sizes()[1])
    step_fired = [it for it in range(6) if counts[it] != (counts[it - 1] if it else 90000)]
    assert step_fired == [3]                    # the step that starts at t = 0.15: 0.15 + dt >= 0.2
    with_clock = fresh()
    assert drive(with_clock, 6, True) == step_fired
    assert with_clock.local_sizes()[1] == counts[-1]
    without = fresh()
    assert drive(without, 6, False) == [] and without.local_sizes()[1] == 90000


@pytest.mark.parametrize("kind,kw", [
    ("merge", dict(nmerge=1, tmerge=[0.1], thshmerge=[0.5])),
    ("remove_profile", dict(nremove=1, tremove=[0.1], typeremove=2)),
    ("remove_threshold", dict(nremove=1, tremove=[0.1], typeremove=1, thshremove=[0.4], remove_frac=0.7)),
    ("split", dict(nsplit=1, tsplit=[0.1], thshsplit=[0.3], split_ngroup=3)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_event_moves_keys_not_markers_over_pcie(amd, monkeypatch, kind, kw):
    """the markers stay on the device during an event -- |delta f|(v) is summed there (in the
    reference's order of additions), one small key per marker goes to the host for the sequential walk, and the
    walk's decisions come back: at most 9 B per marker between host and device (the host-side pass moves 64 per
    allocated slot), with the same markers afterwards as the pass on host copies (PIC1DP_OPT_HOST=1)."""
    n = 2_000_000
    base = dict(nparticle_max=n + n // 2, species_nparticle_init=[n], nx=64, nv=64, **kw)

    def run(host):
        monkeypatch.setenv("PIC1DP_OPT_HOST", "1" if host else "0")
        e = amd.Pic1dp(amd.make_input(**base), npe=2)
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        e.step(1)                       # t = 0.05: the event fires in the next step (0.05 + dt >= 0.1)
        before = e.kernel_stats(8)[1]
        e.step(1)
        return e, e.kernel_stats(8)[1] - before

    dev, bytes_dev = run(False)
    ref, bytes_host = run(True)
    nalloc, npv = dev.local_sizes()
    assert npv != n and npv == ref.local_sizes()[1]
    assert bytes_host == 64 * nalloc
    print("%s: %.2f B per marker between host and device (host-side pass: %.0f)" % (kind, bytes_dev / n, bytes_host / n))
    assert 0 < bytes_dev <= 9 * n, bytes_dev / n
    # the two engines' fields differ in the last bits by then (order of the charge atomics), hence v and w too: the same
    # markers in the same slots to rounding (bit for bit against the oracle on aligned inputs: the tests above)
    a, b = dev.particles_download(), ref.particles_download()
    for k in "xvpw":
        assert np.allclose(a[k][:npv], b[k][:npv], rtol=1e-9, atol=1e-18), k
    assert relerr(dev.energy_sums(), ref.energy_sums()) < 1e-12      # (the whole local vector: tail slots too)


# ---- two species -----------------------------------------------------------------------------------------------------
TWO_SPECIES = dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0],
                   species_temperature2=[1.0, 1.0], species_density=[1.0, 1.0], species_v0=[0.0, 0.0], iptcldist=0)

# the kind under test at t = 0.3 and a second event that draws random numbers at t = 0.4: a block's stream is shared by
# its species in their order, so a stream left at another place by the first event shows in the second one's bits
TWO_SPECIES_EVENTS = [
    ("merge", dict(nmerge=1, tmerge=[0.3], thshmerge=[0.5], nsplit=1, tsplit=[0.4], thshsplit=[0.3], split_ngroup=3)),
    ("remove_profile", dict(nremove=2, tremove=[0.3, 0.4], typeremove=2)),
    ("remove_threshold", dict(nremove=2, tremove=[0.3, 0.4], typeremove=1, thshremove=[0.4, 0.6], remove_frac=0.7)),
    ("split", dict(nsplit=2, tsplit=[0.3, 0.4], thshsplit=[0.7, 0.4], split_ngroup=3)),
    ("all_three", dict(nmerge=1, tmerge=[0.3], thshmerge=[0.3], nremove=2, tremove=[0.3, 0.4], typeremove=2,
                       nsplit=1, tsplit=[0.3], thshsplit=[0.6])),
]


@pytest.mark.parametrize("kind,kw", TWO_SPECIES_EVENTS, ids=[c[0] for c in TWO_SPECIES_EVENTS])
@pytest.mark.parametrize("npe", [1, 3])
def test_two_species_event_is_bit_identical(oracle_mod, amd, kind, kw, npe):
    """two species of unequal counts, charges and masses: the per-species |delta f|(v) (its own histogram, peak and
    limit), the species of a block in order on the block's random stream, the per-species re-pack -- every valid marker
    of every block and species bit for bit after the event and after a second, random-consuming one"""
    n0 = [36000, 12000]
    base = dict(TWO_SPECIES, nparticle_max=60000, species_nparticle_init=n0, nx=32, nv=64)
    first, second = aligned_event(oracle_mod, amd, npe, dict(base, **kw), times=(0.3, 0.4))
    print(kind, npe, n0, first, second)
    for isp in range(2):
        if kind == "merge" or kind.startswith("remove"):
            assert first[isp] < n0[isp]
        elif kind == "split":
            assert first[isp] > n0[isp]
        else:
            assert first[isp] != n0[isp]
        assert second[isp] != first[isp] or first[isp] == 60000


@pytest.mark.parametrize("npe", [1, 3])
def test_split_skips_a_full_species_only(oracle_mod, amd, npe):
    """species 1 within fewer than 2 split_ngroup - 1 slots of full in every block, species 0 with room
    (src/pic1dp_particle.F90:656-657): the split leaves species 1 alone, count and bits, draws nothing for it, and splits
    species 0 -- twice, the second split on the stream the first one left"""
    ng, nmax = 3, 60000
    n0 = [36000, nmax - 3]
    kw = dict(TWO_SPECIES, nparticle_max=nmax, species_nparticle_init=n0, nx=32, nv=64, nsplit=2, tsplit=[0.3, 0.4],
              thshsplit=[0.9, 0.7], split_ngroup=ng)
    held = {}

    def before(sim, eng, i):
        for r in range(npe):
            assert sim.rank_nalloc(r) - sim.rank_np(r, 1) < 2 * ng - 1 <= sim.rank_nalloc(r) - sim.rank_np(r, 0)
        held["before"] = eng.particles_download(1)

    def after(sim, eng, i):
        assert eng.local_sizes(1)[1] == n0[1]
        got = eng.particles_download(1)
        for k in "xvpw":
            assert np.array_equal(got[k][:n0[1]], held["before"][k][:n0[1]]), k

    first, second = aligned_event(oracle_mod, amd, npe, kw, times=(0.3, 0.4), before_event=before, after_event=after)
    print(npe, first, second)
    assert first[1] == second[1] == n0[1]
    assert n0[0] < first[0] < second[0]


# ---- event chains ------------------------------------------------------------------------------------------------------
CHAIN = dict(nmerge=2, tmerge=[0.3, 0.6], thshmerge=[0.5, 0.2], nsplit=2, tsplit=[0.4, 0.7], thshsplit=[0.3, 0.6],
             nremove=2, tremove=[0.5, 0.8], thshremove=[0.4, 0.25], remove_frac=0.7)
CHAIN_TIMES = (0.3, 0.4, 0.5, 0.6, 0.7, 0.8)      # merge, split, remove, merge, split, remove


def chain_kw(typeremove, nspecies, nmax=60000):
    kw = dict(CHAIN, typeremove=typeremove, nparticle_max=nmax, nx=32, nv=64)
    if nspecies == 2:
        kw.update(TWO_SPECIES, species_nparticle_init=[nmax // 2, nmax // 5])
    else:
        kw.update(iptcldist=0, species_density=[1.0], species_v0=[0.0], species_nparticle_init=[nmax * 3 // 5])
    return kw


@pytest.mark.parametrize("nspecies", [1, 2], ids=lambda v: "species%d" % v)
@pytest.mark.parametrize("npe", [1, 3], ids=lambda v: "npe%d" % v)
@pytest.mark.parametrize("typeremove", [1, 2], ids=lambda v: "typeremove%d" % v)
def test_event_chain_is_bit_identical(oracle_mod, amd, typeremove, npe, nspecies):
    """two events of every kind one after the other: the thresholds of the second ones (thresholds[kind][counter - 1]),
    every event after the first on a re-packed slab, tail slots that a merge or remove freed taken by a later split --
    each of the six events bit for bit.  That the second merge ran with ITS threshold: the oracle's merge of the same
    markers with thshmerge[0] leaves another count"""
    kw = chain_kw(typeremove, nspecies)
    with_first = {}

    def before(sim, eng, i):
        if i != 3:
            return
        other = oracle_mod.Sim(oracle_mod.make_input(**dict(kw, nmerge=1, tmerge=[CHAIN["tmerge"][1]],
                                                            thshmerge=[CHAIN["thshmerge"][0]], nsplit=0, nremove=0)), npe=npe)
        assert other.load() == 0
        for isp in range(nspecies):
            for r in range(npe):
                n = sim.rank_np(r, isp)
                other.set_rank_np(r, n, isp)
                for k in "xvpw":
                    other.array(r, isp, k)[:n] = sim.array(r, isp, k)[:n]
        other.set_time(sim.itime, sim.time)
        assert other.optimize(2)
        with_first["counts"] = species_counts(other, npe)

    counts = aligned_event(oracle_mod, amd, npe, kw, times=CHAIN_TIMES, before_event=before)
    print(typeremove, npe, nspecies, counts, with_first)
    assert len(counts) == 6
    for isp in range(nspecies):
        c = [kw["species_nparticle_init"][isp]] + [n[isp] for n in counts]
        assert c[1] < c[0] and c[2] > c[1] and c[3] < c[2] and c[4] < c[3] and c[5] > c[4] and c[6] < c[5]
        assert counts[3][isp] != with_first["counts"][isp]


# ---- markers beyond +-v_max ------------------------------------------------------------------------------------------
FAR = dict(nparticle_max=60000, species_nparticle_init=[36000], nx=32, nv=64, imarker=1, v_max=2.0, iptcldist=0,
           species_density=[1.0], species_v0=[0.0])
FAR_EVENTS = [
    ("merge", dict(nmerge=1, tmerge=[0.3], thshmerge=[0.5])),
    ("remove_profile", dict(nremove=1, tremove=[0.3], typeremove=2)),
    ("remove_threshold", dict(nremove=1, tremove=[0.3], typeremove=1, thshremove=[0.4], remove_frac=0.7)),
    ("split", dict(nsplit=1, tsplit=[0.3], thshsplit=[0.3], split_ngroup=3)),
    ("all_three", dict(nmerge=1, tmerge=[0.3], thshmerge=[0.3], nremove=1, tremove=[0.3], typeremove=2,
                       nsplit=1, tsplit=[0.3], thshsplit=[0.6])),
]


@pytest.mark.parametrize("kind,kw", FAR_EVENTS, ids=[c[0] for c in FAR_EVENTS])
@pytest.mark.parametrize("npe", [1, 3])
def test_event_with_markers_beyond_v_max(oracle_mod, amd, kind, kw, npe):
    """Gaussian-loaded markers (imarker 1) do not know v_max: with v_max = 2 thermal speeds 4.6 % lie outside, on both
    sides -- the dump bin of the |delta f|(v) sum and both end branches of its interpolation, in the merge keys, the
    remove values and scaling and the split flags; bit for bit"""
    seen = {}

    def before(sim, eng, i):
        x, v = sim.gather("x"), sim.gather("v")
        assert_defined_in_reference(x, sim.inp.lx)
        far = np.abs(v) >= sim.inp.v_max
        seen.update(n=v.size, far=int(far.sum()), up=int((v[far] > 0).sum()), down=int((v[far] < 0).sum()))

    def after(sim, eng, i):
        seen["far_after"] = int((np.abs(sim.gather("v")) >= sim.inp.v_max).sum())

    (n_after,), = aligned_event(oracle_mod, amd, npe, dict(FAR, **kw), before_event=before, after_event=after)
    print(kind, npe, seen, n_after)
    assert seen["far"] >= 0.02 * seen["n"] and seen["up"] > 0 and seen["down"] > 0
    assert n_after != 36000
    if kind == "merge" or kind.startswith("remove"):
        assert seen["far_after"] < seen["far"]


def crafted_markers(inp, nalloc):
    """x, v, p, w (padded to nalloc) and the number of valid markers: a random bulk whose heavy weights sit around
    v = 4.1 (the peak of |delta f|(v): everything else is unimportant at thshmerge 0.5), and on top of it pairs that
    share a bin -- same velocity, same cell, same sign of w -- at every node of the nv grid, at +-v_max, at the doubles
    next to +-v_max on either side, at +-400 and +-600 (which the step carries to negative positions and into
    [lx, 3 lx): every step starts from wrapped ones), at +-1e300, and at rest on exact multiples of lx / nx"""
    lx, nx, nv, vmax = inp.lx, inp.nx, inp.nv, inp.v_max
    rng = np.random.default_rng(20260)
    nb = 12000
    xb = rng.uniform(-lx, 3.0 * lx, nb)
    vb = rng.uniform(-vmax, vmax, nb)
    wb = rng.choice([-1.0, 1.0], nb) * rng.uniform(0.2, 1.0, nb) * (1e-6 + 1e-3 * np.exp(-8.0 * (vb - 4.1) ** 2))
    nodes = [-vmax + (2.0 * vmax) * j / (nv - 1) for j in range(nv)] + [(2.0 * j / (nv - 1) - 1.0) * vmax for j in range(nv)]
    edge = [vmax, -vmax, np.nextafter(vmax, 0.0), np.nextafter(-vmax, 0.0), np.nextafter(vmax, np.inf),
            np.nextafter(-vmax, -np.inf), 400.0, -400.0, 600.0, -600.0, 1e300, -1e300]
    xs, vs, ws = [], [], []
    dx = lx / nx
    for n, v in enumerate(nodes + edge):
        cell = (5 * n + 3) % nx
        x0 = (cell + 0.5) * dx + (-lx if n % 3 == 0 else 2.0 * lx if n % 3 == 1 else 0.0)
        for sign in (1.0, -1.0):
            for k in range(3):                       # three of a sign in a bin: one pair merges, the third waits
                xs.append(x0 + 0.01 * dx * k)
                vs.append(v)
                ws.append(sign * 1e-6 * (1.0 + 0.25 * k + 0.01 * n))
    for k in list(range(-nx, 3 * nx + 1, 5)) + [0, nx, 2 * nx]:      # at rest: the position stays what it is
        for xk in (dx * k, lx * k / nx):
            for sign in (1.0, -1.0):
                for rep in range(2):
                    xs.append(xk)
                    vs.append(0.0)
                    ws.append(sign * 1e-6 * (1.0 + rep))
    x = np.concatenate([xb, xs])
    v = np.concatenate([vb, vs])
    w = np.concatenate([wb, ws])
    order = rng.permutation(x.size)
    x, v, w = x[order], v[order], w[order]
    p = np.full(x.size, 1e-3) + np.abs(w)
    n = x.size
    assert n <= nalloc
    pad = lambda a: np.concatenate([a, np.zeros(nalloc - n)])
    return pad(x), pad(v), pad(p), pad(w), n


@pytest.mark.parametrize("host", [0, 1], ids=["device_pass", "host_pass"])
def test_merge_of_crafted_markers_at_the_grids_ends(oracle_mod, amd, monkeypatch, host):
    """velocities exactly on the nodes and ends of the v grid, one ulp inside and outside them and at +-1e300 (the
    comparison on the double that keeps the integer conversion from overflowing), positions outside [0, lx) and on cell
    edges: the merge of uploaded markers against the oracle's on the same arrays, bit for bit -- through the pass that
    keeps the markers on the device and through the one on host copies (PIC1DP_OPT_HOST=1; it summed the right-hand
    share of a marker that lands on the last node one element past the histogram, and converted before it compared).
    linear = 1: the pushes leave v alone; the field is held at zero so that the weights stay what they are"""
    monkeypatch.setenv("PIC1DP_OPT_HOST", str(host))
    # the event is what is looked at: the pushes around it one kernel per call, nothing predicted
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    kw = dict(nparticle_max=20000, nx=32, nv=64, linear=1, iptcldist=0, species_density=[1.0], species_v0=[0.0],
              nmerge=1, tmerge=[0.3], thshmerge=[0.5])
    o, g = both_inputs(oracle_mod, amd, **kw)
    sim = oracle_mod.Sim(o, npe=1)
    assert sim.load() == 0
    eng = amd.Pic1dp(g, npe=1)
    x, v, p, w, n = crafted_markers(o, sim.rank_nalloc(0))
    eng.particles_upload(x, v, p, w, np_valid=n)
    sim.set_rank_np(0, n)
    for k, a in zip("xvpw", (x, v, p, w)):
        sim.array(0, 0, k)[:] = a
    zero = np.zeros(o.nx)
    sim.collect_charge()
    eng.interaction_collect_charge()
    sim.solve_field()
    eng.field_solve_electric()
    sim.set_time(5, 0.25)
    eng.set_time(5, 0.25)
    for irk in (1, 2):
        sim.set_field(zero)
        eng.set_electric(zero)
        sim.push(irk)
        eng.interaction_push_particle(irk)
        align_markers(sim, eng, 1)
        if irk == 1:
            assert not sim.optimize(1) and not eng.particle_optimize(1)
            sim.collect_charge()
            eng.interaction_collect_charge()
            sim.solve_field()
            eng.field_solve_electric()
    xe, ve, we = sim.gather("x"), sim.gather("v"), sim.gather("w")
    assert np.array_equal(ve, v[:n]) and np.array_equal(we, w[:n])
    assert_defined_in_reference(xe, o.lx)
    at_rest = ve == 0.0
    assert np.any(xe < 0.0) and np.any((xe >= o.lx) & (xe < 3.0 * o.lx)) and np.any(xe[at_rest] == o.lx / o.nx * 8)
    huge = np.abs(ve) == 1e300
    assert huge.sum() == 12
    assert sim.optimize(2) and eng.particle_optimize(2)
    n_after = compare_blocks(sim, eng, 1)
    va = sim.gather("v")
    print("crafted markers: %d -> %d; at +-1e300: 12 -> %d" % (n, n_after, (np.abs(va) >= 1e299).sum()))
    assert n_after < n - 200
    # of the six at +1e300 (three of a sign in one bin) and of the six at -1e300 some merged; nothing overflowed
    assert (va >= 1e299).sum() < 6 and (va <= -1e299).sum() < 6 and np.all(np.isfinite(va))
    assert np.all(np.isfinite(sim.gather("x"))) and np.all(np.isfinite(sim.gather("w")))


# ---- the steps around an event ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmode", [1, 2], ids=lambda v: "modes%d" % v)
def test_steps_after_an_event_follow_the_oracle(oracle_mod, amd, nmode):
    """after an event both sides hold the same markers: ten steps in one step() call from there -- which start from
    whatever prediction and half-step field the library still holds -- against the oracle's, int E^2 dx at every step
    within the oracle bar for the field energy (1e-10: README, tests/test_gpu_physics.py), counts equal.  One kept mode
    and two (the prediction tiles).  What the event's own state_version bump protects (the deposit that follows bumps it
    as well, so the prediction is dropped either way) is what is cached against it between the push and that deposit:
    the kinetic sums asked for right before the event and right after it -- the second answer must be the new markers',
    within the suite's oracle bar for them (tests/test_gpu_parity.py: `relerr(eng.energy_sums(), sim.energy_sums()) <
    1e-11`)"""
    kw = dict(nparticle_max=60000, species_nparticle_init=[36000], nx=32, nv=64, nmerge=1, tmerge=[0.3], thshmerge=[0.3],
              nremove=1, tremove=[0.3], typeremove=2, nsplit=1, tsplit=[0.3], thshsplit=[0.6])
    if nmode == 2:
        kw.update(nmode=2, modes=[1, 2])
    npe = 3
    sim, eng = pair = synced_pair(oracle_mod, amd, npe, **kw)
    sums = {}

    def before(sim, eng, i):
        sums["before"] = eng.energy_sums()

    def after(sim, eng, i):
        sums["after"], sums["oracle"] = eng.energy_sums(), sim.energy_sums()

    (n_after,), = aligned_event(oracle_mod, amd, npe, kw, pair=pair, before_event=before, after_event=after)
    assert n_after != 36000
    print("kinetic sums before the event", sums["before"], "after", sums["after"], "oracle", sums["oracle"])
    assert relerr(sums["before"], sums["oracle"]) > 1e-6          # the event changed them by far more than the bar
    assert relerr(sums["after"], sums["oracle"]) < 1e-11
    k = 10
    done = len(eng.energy_history())
    eng.step(k)
    eo = []
    for _ in range(k):
        sim.step(1)
        eo.append(sim.field_energy())
    eg = eng.energy_history()[done:]
    assert len(eg) == k
    err = np.max(np.abs(eg / np.array(eo) - 1.0))
    print("modes %d (prediction kind %d): energy of the %d steps after the event off by %.3g" % (nmode, eng.predict_kind(), k, err))
    assert err < 1e-10
    assert eng.local_sizes()[1] == species_counts(sim, npe)[0] == n_after
    assert eng.time == sim.time


EXACT_STEPS = 18
WAYS = ("step_n", "step_1", "substep", "calls")


def exact_chain_run(amd, way, nsteps=EXACT_STEPS):
    """the chain under the exact charge sum, 40 000 slots, two species, three blocks, through one of the step paths"""
    kw = chain_kw(2, 2, 40000)
    eng = amd.Pic1dp(amd.make_input(**kw), npe=3)
    eng.particle_load()
    eng.set_charge_sum(1)
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    dt = eng.inp.dt
    if way == "step_n":
        eng.step(nsteps)
    for _ in range(0 if way == "step_n" else nsteps):
        if way == "step_1":
            eng.step(1)
            continue
        for irk in (1, 2):
            if way == "substep":
                eng.substep(irk)
            else:
                eng.interaction_push_particle(irk)
                eng.particle_optimize(irk)
                eng.interaction_collect_charge()
                eng.field_solve_electric()
        eng.set_time(eng.itime + 1, eng.time + dt)
    out = dict(E=eng.get_field()["electric"], time=np.array([eng.time]), np=np.array([eng.local_sizes(s)[1] for s in range(2)]))
    for s in range(2):
        g = eng.particles_download(s)
        for k in "xvpw":
            out["%s%d" % (k, s)] = g[k][:out["np"][s]]
    assert not eng.particle_optimize(2)
    eng.close()
    return out


CODE = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import numpy as np, pic1dp_amd as amd; "
        "import test_gpu_optimize as T; np.savez(%r, **T.exact_chain_run(amd, 'calls'))")


def test_exact_charge_chain_is_bit_identical_through_every_path(amd, tmp_path):
    """set_charge_sum(1) promises the same bits whatever the step path -- across six events too: step(n), step(1) n
    times, substep pairs, and the call sites lazy and eager (PIC1DP_LAZY_CALLS=0 is read when the context is made: a
    child process), the last three with the clock handed over after every step"""
    base = exact_chain_run(amd, "step_n")
    n0 = chain_kw(2, 2, 40000)["species_nparticle_init"]
    assert all(base["np"][s] != n0[s] for s in range(2))
    runs = {way: exact_chain_run(amd, way) for way in WAYS[1:]}
    out = str(tmp_path / "eager.npz")
    env = dict(os.environ, PIC1DP_LAZY_CALLS="0")
    subprocess.run([sys.executable, "-c", CODE % (ROOT, os.path.join(ROOT, "tests"), out)], env=env, check=True, timeout=300)
    with np.load(out) as f:
        runs["calls_eager"] = {k: f[k] for k in f.files}
    for way, r in runs.items():
        assert sorted(r) == sorted(base), way
        for k in base:
            assert np.array_equal(r[k], base[k]), (way, k)


def test_step_across_events_equals_the_call_sites(amd, monkeypatch):
    """one step(12) call across two merges, a split and a remove (default charge sum) against the eager call sites
    with the clock, and step(1) twelve times for the counts in between: counts equal after every step, energies
    within the bar of the whole-step against call-site comparison of tests/test_gpu_one_pass.py
    (test_one_pass_with_the_hosts_own_reduction: `assert abs(a.field_energy() / b.field_energy() - 1.0) < 1e-11, it`)"""
    kw = chain_kw(2, 1)
    nsteps = 12

    def fresh():
        e = amd.Pic1dp(amd.make_input(**kw), npe=3)
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        return e

    a, b = fresh(), fresh()
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    c = fresh()
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    a.step(nsteps)
    counts_b, counts_c, energy_c = [], [], []
    for it in range(nsteps):
        b.step(1)
        counts_b.append(b.local_sizes()[1])
        for irk in (1, 2):
            c.interaction_push_particle(irk)
            c.particle_optimize(irk)
            c.interaction_collect_charge()
            c.field_solve_electric()
        c.set_time(c.itime + 1, c.time + c.inp.dt)
        counts_c.append(c.local_sizes()[1])
        energy_c.append(c.field_energy())
    print(counts_c)
    assert len(set(counts_c)) >= 4                    # the events of steps 5, 8, 10 and 11 changed the count
    assert counts_b == counts_c and a.local_sizes()[1] == counts_c[-1]
    ea, eb, ec = a.energy_history(), b.energy_history(), np.array(energy_c)
    assert len(ea) == len(eb) == nsteps
    print("step(%d) against the call sites: %.3g; step(1): %.3g" % (nsteps, np.max(np.abs(ea / ec - 1.0)), np.max(np.abs(eb / ec - 1.0))))
    assert np.max(np.abs(ea / ec - 1.0)) < 1e-11
    assert np.max(np.abs(eb / ec - 1.0)) < 1e-11

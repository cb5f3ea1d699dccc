"""Randomised differential test: seeded random configurations (grid size, kept
modes, distribution, linear / nonlinear / full-f, species, masses and
temperatures, virtual ranks, unloaded tails, odd marker counts) run for a few
time steps on the GPU and in the oracle; the field-energy series must agree to
1e-10 and positions to the trajectory-following tolerance."""
import os

import numpy as np
import pytest

from util import both_inputs

pytestmark = pytest.mark.gpu

# a longer campaign on request: PIC1DP_FUZZ_BASE=1000 PIC1DP_FUZZ_MULT=10 pytest tests/test_gpu_fuzz.py -m gpu
# (seeds BASE ... BASE + MULT * the default count; the default, BASE 0 / MULT 1, is what the suite runs)
_BASE = int(os.environ.get("PIC1DP_FUZZ_BASE", "0"))
_MULT = int(os.environ.get("PIC1DP_FUZZ_MULT", "1"))


def seeds(n):
    return range(_BASE, _BASE + n * _MULT)


class Checked:
    """an engine whose every call is followed by pic1dp_hip_check_state(deep): the relations between the flags of the
    state machine and the zeroness of the accumulator sets nobody owes anything to, asserted at
    every API boundary of a random call sequence"""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        attr = getattr(self._eng, name)
        if not callable(attr) or name in ("check_state", "close"):
            return attr

        def call(*a, **k):
            out = attr(*a, **k)
            self._eng.check_state(True)
            return out
        return call


def random_case(rng):
    nsp = int(rng.integers(1, 4))
    nx = int(rng.choice([2, 3, 17, 64, 100, 192, 255, 512, 1000, 2048]))
    nmode_max = max(1, min(6, nx // 2))
    nmode = int(rng.integers(1, nmode_max + 1))
    modes = sorted(rng.choice(np.arange(1, max(2, nx // 2 + 1)), size=nmode, replace=False).tolist())
    dist = int(rng.integers(0, 4))
    deltaf = 1 if dist in (1, 2, 3) or rng.random() < 0.7 else 0
    linear = int(rng.random() < 0.3) if deltaf else 0
    nmax = int(rng.integers(2000, 30000))
    ninit = [int(nmax - rng.integers(0, nmax // 4)) if rng.random() < 0.3 else nmax for _ in range(nsp)]
    pow2 = rng.random() < 0.4
    def pick(vals_p2, lo, hi):
        return float(rng.choice(vals_p2)) if pow2 else float(rng.uniform(lo, hi))
    kw = dict(
        nspecies=nsp, nx=nx, nmode=nmode, modes=[int(m) for m in modes], iptcldist=dist, deltaf=deltaf,
        linear=linear, nparticle_max=nmax, species_nparticle_init=ninit,
        species_charge=[float(rng.choice([-1.0, 1.0, -2.0])) for _ in range(nsp)],
        species_mass=[pick([0.5, 1.0, 2.0, 4.0], 0.5, 30.0) for _ in range(nsp)],
        species_temperature=[pick([0.5, 1.0, 2.0], 0.5, 2.0) for _ in range(nsp)],
        species_temperature2=[pick([0.5, 1.0, 2.0], 0.5, 2.0) for _ in range(nsp)],
        species_density=[float(rng.uniform(0.6, 0.95)) for _ in range(nsp)],
        species_v0=[float(rng.uniform(2.0, 5.0)) for _ in range(nsp)],
        lx=float(rng.uniform(5.0, 40.0)), dt=float(rng.choice([0.05, 0.1, 0.02])),
        init_nmode=2, init_mode=[1, int(rng.integers(1, 4))],
        init_mode_cos=[float(rng.uniform(-1e-4, 1e-4)), 0.0], init_mode_sin=[1e-5, float(rng.uniform(-1e-5, 1e-5))],
        multirand_al_int=int(rng.choice([1, 2, 3])), multirand_warmup=int(rng.integers(0, 3)),
    )
    npe = int(rng.choice([1, 1, 2, 3]))
    # keep the case inside the reference's own domain: with a heavy, cold species both Maxwellians of -f0'/f0 underflow
    # at the edge of the velocity range (exp(-(v_max + v0)^2 m / 2T) = 0), the reference's ratio is 0/0 there, its markers
    # turn NaN and index out of the grid (seed 1040: m = 16, T = 0.65) -- nothing to compare; the mass is capped instead
    for i in range(nsp):
        cold = min(kw["species_temperature"][i], kw["species_temperature2"][i])
        cap = 1300.0 * cold / (8.0 + kw["species_v0"][i]) ** 2
        kw["species_mass"][i] = min(kw["species_mass"][i], cap)
    return kw, npe


@pytest.mark.parametrize("seed", seeds(24))
def test_random_configuration(oracle_mod, amd, seed):
    rng = np.random.default_rng(1000 + seed)
    kw, npe = random_case(rng)
    o, g = both_inputs(oracle_mod, amd, **kw)
    sim = oracle_mod.Sim(o, npe=npe)
    assert sim.load() == 0
    eng = amd.Pic1dp(g, npe=npe)
    eng.particle_load()
    for isp in range(kw["nspecies"]):
        got = eng.particles_download(isp)
        npv = eng.local_sizes(isp)[1]
        for k in "xvpw":
            assert np.array_equal(got[k][:npv], sim.gather(k, isp)), (k, isp)
    if seed % 2:
        eng.set_step_mode(1)
    sim.collect_charge()
    sim.solve_field()
    eng.interaction_collect_charge()
    eng.field_solve_electric()
    nsteps = 6
    eo = [sim.field_energy()]
    eg = [eng.field_energy()]
    for _ in range(nsteps):
        sim.step(1)
        eo.append(sim.field_energy())
    eng.step(nsteps)
    eg = np.concatenate([eg, eng.energy_history()])
    eo = np.array(eo)
    # energies can be tiny (or zero when no kept mode is excited): absolute floor
    scale = max(np.max(eo), 1e-300)
    assert np.max(np.abs(eg - eo)) <= 1e-10 * scale, (kw, npe)
    for isp in range(kw["nspecies"]):
        got = eng.particles_download(isp)
        npv = eng.local_sizes(isp)[1]
        assert np.max(np.abs(got["x"][:npv] - sim.gather("x", isp))) < 1e-8
        assert np.max(np.abs(got["v"][:npv] - sim.gather("v", isp))) < 1e-8


@pytest.mark.parametrize("seed", seeds(16))
def test_random_call_sequences_lazy_equals_eager(amd, monkeypatch, seed):
    """differential test of the lazy call sites: random sequences of the hot-path
    calls, field changes and inspections, applied to an engine with lazy call sites
    and to one launching a kernel per call; every inspection and the final state
    must agree bit for bit (fields are copied over after every solve so that both
    push with the same bits)"""
    rng = np.random.default_rng(1000 + seed)
    kw = dict(nparticle_max=20001, nx=int(rng.choice([32, 48, 96])), linear=int(rng.integers(0, 2)),
              iptcldist=int(rng.choice([0, 1, 2, 3])))
    if kw["iptcldist"] == 2:
        kw.update(species_density=[1.0], species_v0=[3.0])
    engines = []
    for lazy in ("1", "0"):
        monkeypatch.setenv("PIC1DP_LAZY_CALLS", lazy)
        e = Checked(amd.Pic1dp(amd.make_input(**kw)))
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
        engines.append(e)
    a, b = engines
    b.set_electric(a.get_field()["electric"])
    nx = kw["nx"]

    def same(tag):
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k], equal_nan=True), (tag, k)

    ops = ["push1", "collect", "solve", "push2", "collect", "solve"]      # the reference's order, mostly
    log = []
    for i in range(48):
        r = rng.random()
        if r < 0.70:
            op = ops[i % 6]
        else:
            op = str(rng.choice(["push1", "push2", "collect", "solve", "setE", "look", "bak", "sums", "dist", "optimize",
                                 "hostsum", "setcd"]))      # (round 6: the split-phase deposit and a host's own charge density, anywhere)
        pushes = [o for o in log if o in ("push1", "push2")]
        if op == "push2" and not (pushes and pushes[-1] == "push1"):
            op = "push1"       # push(2) without a push(1) before it reads an undefined RK backup
        log.append(op)
        if op in ("push1", "push2"):
            for e in (a, b):
                e.interaction_push_particle(int(op[-1]))
        elif op == "collect":
            for e in (a, b):
                e.interaction_collect_charge()
        elif op == "solve":
            for e in (a, b):
                e.field_solve_electric()
            b.set_electric(a.get_field()["electric"])
        elif op == "setE":
            E = 0.02 * np.sin(2 * np.pi * np.arange(nx) / nx + rng.random()) + 0.002 * rng.standard_normal(nx)
            for e in (a, b):
                e.set_electric(E)
        elif op == "look":
            same("look after " + " ".join(log[-6:]))
        elif op == "bak":
            # the RK backup is defined between push(1) and push(2) only
            pushes = [o for o in log if o in ("push1", "push2")]
            if pushes and pushes[-1] == "push1":
                ba, bb = a.particles_download_bak(), b.particles_download_bak()
                for k in ("xb", "vb", "wb"):
                    assert np.array_equal(ba[k], bb[k], equal_nan=True), (k, log[-6:])
        elif op == "sums":
            assert np.allclose(a.energy_sums(), b.energy_sums(), rtol=1e-12, atol=0, equal_nan=True)
        elif op == "dist":
            da, db = a.ptcldist(0, finish=False), b.ptcldist(0, finish=False)
            assert np.allclose(da["markr_xv"], db["markr_xv"], rtol=1e-11, atol=1e-9, equal_nan=True)
        elif op == "optimize":
            for e in (a, b):
                e.particle_optimize(2)
        elif op == "hostsum":                   # a host that owns the reduction: charge_local / charge_reduced in place of collect_charge
            for e in (a, b):
                e.charge_reduced(e.charge_local())
        elif op == "setcd":
            cd = b.get_field()["chargeden"]
            for e in (a, b):
                e.set_chargeden(cd)
    same("end: " + " ".join(log[-8:]))


@pytest.mark.parametrize("kind", [1, 2], ids=["tiles", "sums"])
@pytest.mark.parametrize("seed", seeds(10))
def test_random_call_sequences_predicted_equals_two_pass(amd, monkeypatch, seed, kind):
    """differential test of the state machine behind the one-pass step (state_version,
    field_version, pred_version, eh_*, t2_version, cd_lazy, lz): random VALID sequences of every entry point that
    reads, bumps or voids one of them -- step(n), substep, the three call sites, the split-phase deposit
    (charge_local / charge_reduced), set_chargeden, set_electric, set_field_solver, diagnostics, downloads --
    on the default engine (lazy call sites, prediction as tiles or as the six sums) and on one that runs every
    call eagerly with two marker passes per step (PIC1DP_LAZY_CALLS=0, PIC1DP_PREDICT=0).  The prediction is the
    same algebra regrouped, so the two follow each other to rounding: fields, energies and markers within
    1e-10 at every look and at the end -- a stale prediction, a stale carry or a stale half-step field would show
    at 1e-5 (the size of the perturbation) or worse."""
    rng = np.random.default_rng(7000 + seed)
    dist = int(rng.choice([0, 2, 3, 3]))
    kw = dict(nparticle_max=30001, nx=int(rng.choice([32, 64, 96])), iptcldist=dist,
              linear=int(rng.random() < 0.25), init_mode_sin=[1e-3])
    if dist == 2:
        kw.update(species_density=[1.0], species_v0=[3.0])
    if rng.random() < 0.3:
        kw.update(species_temperature=[1.3], species_temperature2=[0.7], species_mass=[1.1])
    monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    a = Checked(amd.Pic1dp(amd.make_input(**kw)))
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    b = Checked(amd.Pic1dp(amd.make_input(**kw)))
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    monkeypatch.delenv("PIC1DP_PREDICT")
    assert a.predict_kind() == kind and b.predict_kind() == 0
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()
    nx = kw["nx"]
    TOL = 1e-10

    def close(x, y, what):
        scale = max(np.max(np.abs(y)), 1e-300)
        assert np.max(np.abs(x - y)) <= TOL * scale, (what, log[-8:], float(np.max(np.abs(x - y)) / scale))

    def look(tag):
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            close(ga[k], gb[k], (tag, k))
        fa, fb = a.get_field(), b.get_field()
        close(fa["electric"], fb["electric"], (tag, "E"))

    def sub_step(irk, how):
        """one RK sub-step, four ways"""
        if how == "substep":
            for e in (a, b):
                e.substep(irk)
            return
        for e in (a, b):
            e.interaction_push_particle(irk)
        if how == "host_sum":                   # a host that owns the reduction (MPI): charge_local / charge_reduced
            for e in (a, b):
                e.charge_reduced(e.charge_local())
        elif how == "set_cd":                   # ... or that hands the charge density in itself
            for e in (a, b):
                e.interaction_collect_charge()
            cd = b.get_field()["chargeden"]
            if not (kind == 2 and irk == 1):    # with the six sums a's chargeden holds the kept mode's content only
                close(a.get_field()["chargeden"], cd, "chargeden")
            for e in (a, b):
                e.set_chargeden(cd)
        else:
            for e in (a, b):
                e.interaction_collect_charge()
        for e in (a, b):
            e.field_solve_electric()

    log, phase, fd = [], 0, 0
    for i in range(40):
        r = rng.random()
        if phase == 1:                          # mid-step: finish it, perhaps after a look or a field change
            op = str(rng.choice(["sub2", "sub2", "sub2", "look", "setE", "sums", "resolve"]))
        elif r < 0.45:
            op = "step"
        elif r < 0.75:
            op = "sub1"
        else:
            op = str(rng.choice(["look", "setE", "sums", "dist", "solver", "resolve"]))
        log.append(op)
        if op == "step":
            n = int(rng.integers(1, 4))
            for e in (a, b):
                e.step(n)
        elif op in ("sub1", "sub2"):
            how = str(rng.choice(["calls", "calls", "substep", "host_sum", "set_cd"]))
            log[-1] = op + ":" + how
            sub_step(int(op[-1]), how)
            phase = 1 - phase
        elif op == "look":
            look("look")
        elif op == "setE":
            E = 0.02 * np.sin(2 * np.pi * np.arange(nx) / nx + rng.random()) + 0.002 * rng.standard_normal(nx)
            for e in (a, b):
                e.set_electric(E)
        elif op == "sums":
            # (sum v^2 w cancels -- w has both signs --, so its bar is that of its TERMS: the markers agree to TOL of max |w|,
            # hence the sum to TOL * sum v^2 * max |w|; found flaking once in 4 320 seeds against a bar relative to the sum itself)
            sa, sb = a.energy_sums(), b.energy_sums()
            wmax = float(np.max(np.abs(b.particles_download()["w"])))
            assert np.allclose(sa[:2], sb[:2], rtol=1e-9, atol=0)
            assert abs(sa[2] - sb[2]) <= 1e-9 * abs(sb[2]) + TOL * sb[0] * wmax, (sa, sb, wmax)
        elif op == "dist":
            da, db = a.ptcldist(0, finish=False), b.ptcldist(0, finish=False)
            assert np.allclose(da["markr_xv"], db["markr_xv"], rtol=1e-9, atol=1e-9)
        elif op == "solver":                    # the opt-in finite-difference solver and back
            fd = 1 - fd
            for e in (a, b):
                e.set_field_solver(fd)
        elif op == "resolve":                   # solve again from the chargeden at hand (an out-of-order solve_field)
            for e in (a, b):
                e.field_solve_electric()
    if phase == 1:
        sub_step(2, "calls")
    for e in (a, b):
        e.step(2)
    look("end")
    ha, hb = a.energy_history(), b.energy_history()
    assert len(ha) == len(hb)
    if len(hb):
        close(ha, hb, "energy history")


@pytest.mark.parametrize("disturb", ["nothing", "set_electric", "look", "look_chargeden", "step", "substep1", "substep2"])
def test_solve_field_twice_for_the_half_step(amd, monkeypatch, disturb):
    """through the call sites the solve_field of a half step launches nothing (its field came out of the previous
    step's pair solve) -- field_chargeden must nevertheless be what a SECOND solve_field for the same half step solves from
    (the kept mode's content of the half-step charge density), also after the host has overwritten field_electric, looked
    at chargeden, or taken a step or sub-step in between: against an engine that runs every call eagerly, 1e-10 on the
    field and on the markers after the step"""
    kw = dict(nparticle_max=40001, nx=64, init_mode_sin=[1e-3])
    a = Checked(amd.Pic1dp(amd.make_input(**kw)))
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    b = Checked(amd.Pic1dp(amd.make_input(**kw)))
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    monkeypatch.delenv("PIC1DP_PREDICT")
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()

    def calls(e, irk):
        e.interaction_push_particle(irk)
        e.interaction_collect_charge()
        e.field_solve_electric()

    def close(x, y, what):
        assert np.max(np.abs(x - y)) <= 1e-10 * max(np.max(np.abs(y)), 1e-300), what

    def close_chargeden(ca, cb, what):          # by a's flag: the whole vector, or the kept mode's coefficients
        if not a.chargeden_kept_mode_only():
            close(ca, cb, what)
            return
        ka, kb = _kept_coefficients(ca, [1]), _kept_coefficients(cb, [1])
        assert np.max(np.abs(ka - kb)) <= 1e-10 * max(np.max(np.abs(kb)), np.max(np.abs(cb))), what

    for e in (a, b):                            # two whole steps through the call sites: the pair solve is in use from the second
        for _ in range(2):
            calls(e, 1)
            calls(e, 2)
    skips = a.kernel_stats(11)[1]
    for e in (a, b):
        calls(e, 1)                             # a: push noted, collect_charge and solve_field launch nothing
    assert a.kernel_stats(11)[1] == skips + 1   # (the case this test is about)
    if disturb == "set_electric":
        E = 0.01 * np.cos(2 * np.pi * np.arange(64) / 64)
        for e in (a, b):
            e.set_electric(E)
    elif disturb == "look":
        close(a.get_field()["electric"], b.get_field()["electric"], "half-step field")
    elif disturb == "look_chargeden":
        fa, fb = a.get_field(), b.get_field()
        close(fa["electric"], fb["electric"], "half-step field")
        close_chargeden(fa["chargeden"], fb["chargeden"], "half-step chargeden")
    elif disturb in ("step", "substep1", "substep2"):
        for e in (a, b):
            e.step(1) if disturb == "step" else e.substep(int(disturb[-1]))
    for e in (a, b):
        e.field_solve_electric()                # once more: from field_chargeden
    close(a.get_field()["electric"], b.get_field()["electric"], "half-step field solved again")
    close_chargeden(a.get_field()["chargeden"], b.get_field()["chargeden"], "chargeden solved from")
    for e in (a, b):
        if disturb in ("step", "substep2"):     # (the RK backup push(2) reads is push(1)'s: a whole step again)
            calls(e, 1)
        calls(e, 2)
    ga, gb = a.particles_download(), b.particles_download()
    for k in "xvw":
        close(ga[k], gb[k], k)
    close(a.get_field()["electric"], b.get_field()["electric"], "field after the step")


def _two_engines(amd, monkeypatch, kw, kind, npe=1):
    """a: the default engine (lazy call sites, prediction kind `kind`); b: every call eager, two marker passes per step"""
    if kind:
        monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    a = Checked(amd.Pic1dp(amd.make_input(**kw), npe=npe))
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    b = Checked(amd.Pic1dp(amd.make_input(**kw), npe=npe))
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    monkeypatch.delenv("PIC1DP_PREDICT")
    if kind:
        monkeypatch.delenv("PIC1DP_PRED_KIND")
    return a, b


def _kept_coefficients(cd, modes):
    """the kept modes' Fourier coefficients of a charge density (what the mode-filter solve looks at), in extended precision"""
    nx = cd.size
    j = np.arange(nx, dtype=np.longdouble)
    c = np.asarray(cd, dtype=np.longdouble)
    out = []
    for m in modes:
        ang = 2 * np.pi * (m * j % nx) / nx
        out += [np.sum(c * np.cos(ang)), -np.sum(c * np.sin(ang))]
    return np.array(out, dtype=np.float64)


class _Compare:
    """the comparisons of the single-call differential: within TOL of the larger side's max, or bit for bit (exact)"""

    def __init__(self, a, b, kind, modes, exact, log):
        self.a, self.b, self.kind, self.modes, self.exact, self.log = a, b, kind, modes, exact, log

    def close(self, x, y, what, tol=1e-10):
        if self.exact:
            assert np.array_equal(x, y), (what, self.log[-10:], float(np.max(np.abs(x - y), initial=0.0)))
            return
        scale = max(np.max(np.abs(y), initial=0.0), 1e-300)
        assert np.max(np.abs(x - y), initial=0.0) <= tol * scale, (what, self.log[-10:], float(np.max(np.abs(x - y)) / scale))

    def markers(self, tag):
        ga, gb = self.a.particles_download(), self.b.particles_download()
        for k in "xvw":
            self.close(ga[k], gb[k], (tag, k))

    def field(self, tag, chargeden):
        fa, fb = self.a.get_field(chargeden=chargeden), self.b.get_field(chargeden=chargeden)
        for k in ("electric", "mode_re", "mode_im"):
            self.close(fa[k], fb[k], (tag, k))
        if not chargeden:
            return
        assert not self.b.chargeden_kept_mode_only()
        if not self.a.chargeden_kept_mode_only():       # the reference's vector: all of it (kept-mode content only fails here)
            self.close(fa["chargeden"], fb["chargeden"], (tag, "chargeden"))
            return
        assert self.kind == 2 and not self.exact, (tag, "kept-mode-only chargeden outside the six sums", self.log[-10:])
        ca, cb = _kept_coefficients(fa["chargeden"], self.modes), _kept_coefficients(fb["chargeden"], self.modes)
        scale = max(np.max(np.abs(cb)), np.max(np.abs(fb["chargeden"])), 1e-300)
        assert np.max(np.abs(ca - cb)) <= 1e-10 * scale, (tag, "kept modes of chargeden", self.log[-10:])

    def history(self, tag):
        ha, hb = self.a.energy_history(), self.b.energy_history()
        assert len(ha) == len(hb), (tag, len(ha), len(hb), self.log[-10:])
        if len(hb):
            self.close(ha, hb, (tag, "energy history"))


# the calls the single-call differential inserts between two calls of the reference's sequence
_INTRUDERS = ["step", "substep1", "substep2", "look_cd", "look_E", "download", "setE", "setcd", "hostsum", "solver",
              "transform", "dist", "sums", "optimize", "upload"]


def _single_calls(amd, monkeypatch, seed, kind, exact):
    rng = np.random.default_rng((9100 if exact else 8100) + 97 * kind + seed)
    nx = int(rng.choice([32, 48, 64, 96, 100]))
    # kind 2 with one kept mode on one rank is the pair path (the half-step field out of the previous solve): mostly that
    nmode = 1 if (kind == 2 and rng.random() < 0.75) else int(rng.choice([1, 2]))
    modes = [1] if nmode == 1 else sorted(rng.choice(np.arange(1, nx // 2), size=2, replace=False).tolist())
    npe = int(rng.choice([1, 2]))
    dist = int(rng.choice([0, 2, 3, 3]))
    kw = dict(nparticle_max=30001, nx=nx, nmode=nmode, modes=[int(m) for m in modes], iptcldist=dist,
              linear=int(rng.random() < 0.25), init_nmode=nmode, init_mode=[int(m) for m in modes],
              init_mode_sin=[1e-3] * nmode, init_mode_cos=[0.0] * nmode)
    if dist == 2:
        kw.update(species_density=[1.0], species_v0=[3.0])
    if rng.random() < 0.3:
        kw.update(species_temperature=[1.3], species_temperature2=[0.7], species_mass=[1.1])
    a, b = _two_engines(amd, monkeypatch, kw, 0 if exact else kind, npe)
    assert b.predict_kind() == 0
    for e in (a, b):
        e.particle_load()
        if exact:
            e.set_charge_sum(1)
        e.interaction_collect_charge()
        e.field_solve_electric()
    pair_case = not exact and kind == 2 and nmode == 1
    if pair_case:
        assert a.predict_kind() == 2
    log = []
    cmp = _Compare(a, b, kind, modes, exact, log)
    ran = dict.fromkeys(_INTRUDERS, 0)

    ref = ["push1", "collect", "solve", "push2", "collect", "solve"]
    cursor, rk_ok, fd, tr = 0, False, 0, 0
    nops = 64
    # the pair path is reached from quiet steps: twice per seed two whole steps and the next push(1), collect_charge (and in
    # the second, its solve_field) go without intruders, and one follows at once -- the states HalfPair / HalfPairSolved
    plan = sorted(rng.choice(np.arange(2, nops - 30), size=2, replace=False).tolist()) if pair_case else []
    setups, quiet, force = [14, 15], 0, False
    skips0 = a.kernel_stats(11)[1]
    i = 0
    while i < nops:
        i += 1
        if plan and i >= plan[0] and cursor == 0 and quiet == 0 and not force:
            plan.pop(0)
            quiet = setups.pop(0)
            for e in (a, b):                    # the fused / predicted paths need the dense-table mode-filter solve
                e.set_field_solver(0)
                e.set_field_transform(0)
            fd = tr = 0
            log.append("pair-setup")
        intrude = force or (quiet == 0 and rng.random() < 0.3)
        if intrude:
            force = False
            op = str(rng.choice(_INTRUDERS))
            if op == "substep2" and not rk_ok:
                op = "substep1"
            log.append(op)
            ran[op] += 1
            if op == "step":
                n = int(rng.integers(1, 3))
                for e in (a, b):
                    e.step(n)
                rk_ok = False
            elif op in ("substep1", "substep2"):
                for e in (a, b):
                    e.substep(int(op[-1]))
                rk_ok = op == "substep1"
            elif op == "look_cd":
                cmp.field(op, True)
            elif op == "look_E":
                cmp.field(op, False)
            elif op == "download":
                cmp.markers(op)
            elif op == "setE":
                E = 0.02 * np.sin(2 * np.pi * np.arange(nx) / nx + rng.random()) + 0.002 * rng.standard_normal(nx)
                for e in (a, b):
                    e.set_electric(E)
            elif op == "setcd":
                cd = b.get_field()["chargeden"] * (1.0 + 0.25 * rng.random())
                for e in (a, b):
                    e.set_chargeden(cd)
            elif op == "hostsum":               # a host that owns the reduction
                for e in (a, b):
                    if exact:
                        e.charge_reduced_exact(e.charge_local_exact())
                    else:
                        e.charge_reduced(e.charge_local())
            elif op == "solver":
                fd = 1 - fd
                for e in (a, b):
                    e.set_field_solver(fd)
            elif op == "transform":
                tr = 1 - tr
                for e in (a, b):
                    e.set_field_transform(tr)
            elif op == "dist":
                da, db = a.ptcldist(0, finish=False), b.ptcldist(0, finish=False)
                assert np.allclose(da["markr_xv"], db["markr_xv"], rtol=1e-9, atol=1e-9), log[-10:]
            elif op == "sums":
                sa, sb = a.energy_sums(), b.energy_sums()
                wmax = float(np.max(np.abs(b.particles_download()["w"])))
                assert np.allclose(sa[:2], sb[:2], rtol=1e-9, atol=0), log[-10:]
                assert abs(sa[2] - sb[2]) <= 1e-9 * abs(sb[2]) + 1e-10 * sb[0] * wmax, (sa, sb, wmax, log[-10:])
            elif op == "optimize":
                for e in (a, b):
                    e.particle_optimize(2)
                rk_ok = False
            elif op == "upload":                # b's markers, into both
                d = b.particles_download()
                npv = b.local_sizes(0)[1]
                for e in (a, b):
                    e.particles_upload(d["x"], d["v"], d["p"], d["w"], np_valid=npv)
                rk_ok = False
            continue
        op = ref[cursor]
        if op == "push2" and not rk_ok:         # push(2) reads the RK backup: only behind a push(1) / substep(1)
            cursor, op = 0, "push1"
        log.append(op)
        if op in ("push1", "push2"):
            for e in (a, b):
                e.interaction_push_particle(int(op[-1]))
            rk_ok = op == "push1"
        elif op == "collect":
            for e in (a, b):
                e.interaction_collect_charge()
        else:
            for e in (a, b):
                e.field_solve_electric()
        cursor = (cursor + 1) % 6
        if quiet:
            quiet -= 1
            force = quiet == 0
    for tag in ("end", "end, looked again"):    # (a second look: what the first one settled stays settled)
        cmp.field(tag, True)
        cmp.markers(tag)
    cmp.history("end")
    skips = a.kernel_stats(11)[1] - skips0
    if pair_case:
        assert skips >= 1, ("the pair path was never served", log)
    return ran, skips


@pytest.mark.parametrize("kind", [1, 2], ids=["tiles", "sums"])
@pytest.mark.parametrize("seed", seeds(8))
def test_random_single_calls_predicted_equals_two_pass(amd, monkeypatch, seed, kind):
    """differential test of the call sites one CALL at a time: the reference's sequence push(1), collect_charge,
    solve_field, push(2), collect_charge, solve_field with an intruder at random boundaries (_INTRUDERS: step, substep,
    looks at the field with and without chargeden, downloads, set_electric, set_chargeden, the split-phase deposit, solver
    and transform switches, diagnostics, marker optimisation, re-upload), on the default engine (lazy calls, prediction as
    tiles or six sums) and on one that runs every call eagerly with two passes per step.  Between collect_charge and its
    solve_field is where a predicted or pair-solved stand-in can go stale: markers, E, the kept modes, the energy history and
    chargeden (by its flag: the whole vector, or the kept modes' coefficients where the flag says that is all there is)
    within 1e-10 at every look and at the end."""
    ran, skips = _single_calls(amd, monkeypatch, seed, kind, exact=False)
    print("intruders:", ran, "pair skips:", skips)


@pytest.mark.parametrize("seed", seeds(6))
def test_random_single_calls_exact_sum_bit_identical(amd, monkeypatch, seed):
    """the single-call differential with the exact charge sum on both engines (set_charge_sum(1) right after particle_load):
    no prediction runs, and the charge is independent of the summation order -- markers, fields, the kept
    modes, chargeden and the energy history bit for bit, across call sites, step, substep, solver and transform switches;
    the diagnostics keep their tolerance"""
    ran, _ = _single_calls(amd, monkeypatch, seed, 1, exact=True)
    print("intruders:", ran)


@pytest.mark.parametrize("intruder", ["step", "substep1", "substep2", "look_chargeden", "look_chargeden_twice", "download_solver",
                                      "download_transform", "reload", "upload"])
def test_owed_half_step_field_after_an_intruder(amd, monkeypatch, intruder):
    """the pair path's owed adoption (collect_charge of a noted push(1) served by the previous solve: HalfPair,
    AdoptHalfField) with a call between that collect_charge and its solve_field.  The adoption stands for a solve from the
    half-step charge density; whatever replaces that density (step, substep), rebuilds it (get_field with chargeden) or
    takes the markers away from the half step (a download, then a solver / transform switch; a new particle_load or
    upload) must leave solve_field doing what the eager engine does -- solve from field_chargeden as the eager calls left
    it.  E, the kept modes and chargeden against an engine that runs every call eagerly, 1e-10; the chargeden flag says
    "full" only over the whole vector"""
    kw = dict(nparticle_max=40001, nx=64, init_mode_sin=[1e-3])
    a, b = _two_engines(amd, monkeypatch, kw, 2)
    assert a.predict_kind() == 2
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()

    def calls(e, irk):
        e.interaction_push_particle(irk)
        e.interaction_collect_charge()
        e.field_solve_electric()

    log = [intruder]
    cmp = _Compare(a, b, 2, [1], False, log)
    for e in (a, b):                            # two whole steps through the call sites: the pair solve is in use from the second
        for _ in range(2):
            calls(e, 1)
            calls(e, 2)
    skips = a.kernel_stats(11)[1]
    for e in (a, b):
        e.interaction_push_particle(1)
        e.interaction_collect_charge()          # a: nothing launched, the half-step field owed for adoption
    if intruder in ("step", "substep1", "substep2"):
        for e in (a, b):
            e.step(2) if intruder == "step" else e.substep(int(intruder[-1]))
    elif intruder.startswith("look_chargeden"):
        cmp.field("look", True)
        if intruder.endswith("twice"):
            cmp.field("look again", True)
    elif intruder.startswith("download"):
        cmp.markers("download")
        for e in (a, b):
            e.set_field_solver(1) if intruder.endswith("solver") else e.set_field_transform(1)
    elif intruder == "reload":
        for e in (a, b):
            e.particle_load()
    elif intruder == "upload":
        d = b.particles_download()
        for e in (a, b):
            e.particles_upload(d["x"], d["v"], d["p"], d["w"], np_valid=b.local_sizes(0)[1])
    for e in (a, b):
        e.field_solve_electric()
    cmp.field("solved after " + intruder, True)
    cmp.field("looked again", True)
    for e in (a, b):                            # and on: a whole step (the RK backup of push(2) is not defined after some intruders)
        calls(e, 1)
        calls(e, 2)
    cmp.markers("after the next step")
    cmp.field("after the next step", True)
    cmp.history("after the next step")
    assert a.kernel_stats(11)[1] >= skips       # (served from the pair again once the sequence resumes)


@pytest.mark.parametrize("after", ["look", "field_energy", "substep1", "next_step", "set_electric", "transform_substep1"])
def test_field_after_the_collect_of_a_pair_solved_step(amd, monkeypatch, after):
    """(found by the single-call fuzz, seeds 19 and 63 of a 10x campaign) push(1), collect_charge, solve_field served by the
    pair solve, then push(2), collect_charge: the whole-step kernel reads the step-start field from field_electric, which
    still holds it -- the solve_field that follows overwrites it.  What the host may see or push with before that solve is
    the half-step field, as after eager calls: E and the kept modes on a look, the field a sub-step or the next step
    pushes with (markers), the kept modes behind a set_electric.  Against an engine that runs every call eagerly, 1e-10."""
    kw = dict(nparticle_max=40001, nx=64, init_mode_sin=[1e-3])
    a, b = _two_engines(amd, monkeypatch, kw, 2)
    assert a.predict_kind() == 2
    for e in (a, b):
        e.particle_load()
        e.interaction_collect_charge()
        e.field_solve_electric()

    def calls(e, irk):
        e.interaction_push_particle(irk)
        e.interaction_collect_charge()
        e.field_solve_electric()

    log = [after]
    cmp = _Compare(a, b, 2, [1], False, log)
    for e in (a, b):                            # the pair solve in use from the second step on
        for _ in range(2):
            calls(e, 1)
            calls(e, 2)
    skips = a.kernel_stats(11)[1]
    for e in (a, b):
        calls(e, 1)                             # a: served by the pair solve
        e.interaction_push_particle(2)
        e.interaction_collect_charge()
    assert a.kernel_stats(11)[1] == skips + 1
    if after == "look":
        cmp.field("look", False)
    elif after == "field_energy":
        cmp.close(np.array([a.field_energy()]), np.array([b.field_energy()]), "field energy")
    elif after == "set_electric":
        for e in (a, b):
            e.set_electric(0.01 * np.cos(2 * np.pi * np.arange(64) / 64))
        cmp.field("after set_electric", False)
    else:
        for e in (a, b):
            if after == "transform_substep1":
                e.set_field_transform(1)
            if after == "next_step":
                calls(e, 1)
                calls(e, 2)
            else:
                e.substep(1)
        cmp.markers(after)
    for e in (a, b):
        e.field_solve_electric()
        calls(e, 1)
        calls(e, 2)
    cmp.markers("after the next step")
    cmp.field("after the next step", True)
    cmp.history("after the next step")

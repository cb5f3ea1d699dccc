"""The staged run of the reference's own hot path that pins the oracle and the kernels.

`record(ref)` drives an `oracle.Ref` (the reference's modules behind the serial stand-in) through load, deposit, the two
pushes with imposed fields, the field solve, a marker optimisation event, one step and a 20-step run, and returns every
stage's outputs as arrays.  tests/golden/gen_ref_hotpath.py stores such a record per case; the live CPU test makes one on
the spot.  `check_oracle(rec, ...)` holds the oracle to a record bit for bit; tests/test_gpu_reference.py holds the HIP
library to the stored ones.

Inputs of a stage that a checker needs are the outputs of the stage before it or are rebuilt here by the same IEEE
operations (`smooth_field`, `far_positions`), so a record stays small.
"""
import os

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RUN_STEPS = 20
EVENT_TIME = (5, 0.25)      # itime, time before the step in which t + dt >= 0.3 fires the cases' events
NDRAWS = 8


def fixture_path(case):
    return os.path.join(GOLDEN_DIR, "ref_hotpath_%s.npz" % case)


def smooth_field(nx, seed, amp=0.05):
    """the imposed field of a push stage: one period of a sine plus noise (every operation correctly rounded but
    sin -- the fixtures therefore store the fields they were made with, see record)"""
    rng = np.random.default_rng(seed)
    ix = np.arange(nx)
    return amp * np.sin(2 * np.pi * ix / nx + 0.3) + 0.2 * amp * rng.standard_normal(nx)


def far_positions(x, lx):
    """positions several periods out on both sides (the general fmod of the wrap), from wrapped ones"""
    return x * 7.25 - 3.0 * lx


def wrapped(x, lx):
    """the reference's wrap (mod, then + lx where negative) in numpy's fmod, which is C's"""
    xm = np.fmod(x, lx)
    return np.where(xm < 0.0, xm + lx, xm)


def assert_defined_in_reference(x, lx):
    """the reference indexes outside its arrays for a position that wraps to exactly lx (undefined in the
    reference; project rule in 2.1): no stage may be fed one"""
    assert not np.any(wrapped(x, lx) == lx), "a position wraps to exactly lx: undefined in the reference"


def has_events(inp):
    return inp.deltaf == 1 and (inp.nmerge > 0 or inp.nremove > 0 or inp.nsplit > 0)


def exp_free(inp):
    return inp.deltaf == 0 or inp.iptcldist in (0, 1)


def record(ref):
    inp, ns, lx, nx = ref.inp, ref.nspecies, ref.inp.lx, ref.nx
    d = {}

    def marks(tag, names, count=None):
        for isp in range(ns):
            n = ref.rank_np(0, isp) if count is None else count
            for k in names:
                d["%s_%s%d" % (tag, k, isp)] = ref.array(isp, k)[:n].copy()

    # ---- load, and the random stream after it
    ref.load()
    d["np"] = np.array([ref.rank_np(0, i) for i in range(ns)], dtype=np.int64)
    marks("load", "xvpw", count=ref.nalloc)
    d["rng_after_load"] = ref.rng_ints(NDRAWS)
    ref.load()
    if has_events(inp):
        ref.set_time(*EVENT_TIME)
    # ---- deposit on the loaded markers (all inside [0, lx): x must come back unchanged)
    for isp in range(ns):
        assert_defined_in_reference(ref.gather("x", isp), lx)
    ref.collect_charge()
    for isp in range(ns):
        assert np.array_equal(ref.array(isp, "x"), d["load_x%d" % isp])
    d["dep0_rho"] = ref.get_field()[1]
    # ---- the two pushes with imposed fields, a deposit after each
    for irk, seed in ((1, 11), (2, 12)):
        E = smooth_field(nx, seed)
        d["E%d" % irk] = E
        ref.set_field(E)
        ref.push(irk)
        marks("p%d" % irk, "xvw")
        for isp in range(ns):   # the backup is the state before the first push, whole vector
            assert np.array_equal(ref.array(isp, "xb"), d["load_x%d" % isp])
            assert np.array_equal(ref.array(isp, "vb"), d["load_v%d" % isp])
            if inp.deltaf == 1:
                assert np.array_equal(ref.array(isp, "wb"), d["load_w%d" % isp])
            assert_defined_in_reference(ref.gather("x", isp), lx)
        if irk == 1:
            assert not ref.optimize(1)
            ref.collect_charge()
            ref.solve_field()
            d["half_E"] = ref.get_field()[0]       # the field a whole step pushes its second half with
            d["half_rho"] = ref.get_field()[1]
            marks("dep1", "x")
    # ---- the optimisation event after the second push
    if has_events(inp):
        assert ref.optimize(2)
        d["ev_np"] = np.array([ref.rank_np(0, i) for i in range(ns)], dtype=np.int64)
        assert not np.array_equal(d["ev_np"], d["np"])
        marks("ev", "xvpw")
        d["ev_spare"] = np.array(ref.gaussian_spare(), dtype=np.float64)
        d["ev_rng"] = ref.rng_ints(NDRAWS)
        assert not ref.optimize(2)
    ref.collect_charge()
    marks("dep2", "x")
    d["dep2_rho"] = ref.get_field()[1]
    # ---- field solve on that charge density; the operators as field_init filled them
    ref.solve_field()
    _, _, d["fs_re"], d["fs_im"] = ref.get_field()
    d["fs_E"] = ref.get_field()[0]
    d["tab_re"], d["tab_im"], d["grad_inv"] = ref.tables()
    # ---- |delta f|(v) of these markers
    d["hist"] = ref.dist_pertb_abs_v()
    # ---- deposit of positions several periods out
    for isp in range(ns):
        far = far_positions(ref.gather("x", isp), lx)
        assert_defined_in_reference(far, lx)
        assert far.min() < -lx and far.max() > 2 * lx
        ref.set_array(isp, "x", far)
    ref.collect_charge()
    marks("far", "x")
    d["far_rho"] = ref.get_field()[1]
    # ---- one whole step from the loaded state with E1 imposed: the driver's call sequence
    ref.load()
    ref.set_field(d["E1"])
    ref.step(1)
    if has_events(inp):
        assert ref.opt_index() == tuple(int(n > 0) for n in (inp.nmerge, inp.nremove, inp.nsplit))   # nothing fired at t = 0
    marks("st", "xvw")
    d["st_E"] = ref.get_field()[0]
    # ---- RUN_STEPS steps from the loaded state (events fire on the way where the case has them)
    ref.load()
    ref.collect_charge()
    ref.solve_field()
    d["run_E0"] = ref.get_field()[0]
    ref.step(RUN_STEPS)
    d["run_np"] = np.array([ref.rank_np(0, i) for i in range(ns)], dtype=np.int64)
    marks("run", "xvw")
    d["run_E"], d["run_rho"] = ref.get_field()[:2]
    d["run_time"] = np.array([ref.time])
    d["run_spare"] = np.array(ref.gaussian_spare(), dtype=np.float64)
    d["run_rng"] = ref.rng_ints(NDRAWS)
    for isp in range(ns):
        assert_defined_in_reference(d["run_x%d" % isp], lx)
    return d


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, "%s: shape %r, reference %r" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.view(np.int64).ravel() != want.view(np.int64).ravel())
    assert bad.size == 0, "%s: %d of %d differ from the reference, first at %d: %r, reference %r" % (
        what, bad.size, want.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def same_values(got, want, what):
    """equal as numbers (the sign of a zero is not part of it: the tables are read through a product)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %r, reference %r" % (what, got.shape, want.shape)
    bad = np.flatnonzero(got.ravel() != want.ravel())
    assert bad.size == 0, "%s: %d of %d differ from the reference, first at %d: %r, reference %r" % (
        what, bad.size, want.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]])


def sim_gaussian_spare(oracle, sim):
    import ctypes as C
    g = C.cast(oracle.lib().orc_sim_rank_rng(sim.s, 0), C.POINTER(oracle.OrcMultirand)).contents
    return np.array([g.gaussian64buf_filled, g.gaussian64buf if g.gaussian64buf_filled else 0.0], dtype=np.float64)


def sim_rng_ints(oracle, sim, n):
    a = np.empty(n, dtype=np.int64)
    oracle.lib().orc_multirand_int_array64(oracle.lib().orc_sim_rank_rng(sim.s, 0), a, n)
    return a


def check_oracle(rec, oracle, inp):
    """the oracle (one rank) through the stages of `record`, every output against the record bit for bit: the run-time
    exp, sin and cos of the reference's build are the host libm's (measured distance 0), so no stage has a
    tolerance."""
    ns, nx, lx = inp.nspecies, inp.nx, inp.lx
    import ctypes as C

    def fresh():
        s = oracle.Sim(inp, npe=1)
        assert s.load() == 0
        return s

    def marks(sim, tag, names, count=None):
        for isp in range(ns):
            n = sim.rank_np(0, isp) if count is None else count
            assert count is not None or n == rec["%s_x%d" % (tag, isp)].size, "%s: %d valid markers, reference %d" % (
                tag, n, rec["%s_x%d" % (tag, isp)].size)
            for k in names:
                same_bits(sim.array(0, isp, k)[:n], rec["%s_%s%d" % (tag, k, isp)], "%s %s species %d" % (tag, k, isp))

    sim = fresh()
    assert [sim.rank_np(0, i) for i in range(ns)] == list(rec["np"])
    marks(sim, "load", "xvpw", count=sim.rank_nalloc(0))
    same_bits(sim_rng_ints(oracle, sim, NDRAWS), rec["rng_after_load"], "random stream after the load")
    sim = fresh()
    if True:
        if has_events(inp):
            sim.set_time(*EVENT_TIME)
        sim.collect_charge()
        marks(sim, "load", "x", count=sim.rank_nalloc(0))
        same_bits(sim.get_field()[1], rec["dep0_rho"], "chargeden of the loaded markers")
        for irk in (1, 2):
            sim.set_field(rec["E%d" % irk])
            sim.push(irk)
            marks(sim, "p%d" % irk, "xvw")
            for isp in range(ns):
                n = sim.rank_nalloc(0)
                same_bits(sim.array(0, isp, "xb")[:n], rec["load_x%d" % isp], "xb after push %d" % irk)
                same_bits(sim.array(0, isp, "vb")[:n], rec["load_v%d" % isp], "vb after push %d" % irk)
                if inp.deltaf == 1:
                    same_bits(sim.array(0, isp, "wb")[:n], rec["load_w%d" % isp], "wb after push %d" % irk)
            if irk == 1:
                assert not sim.optimize(1)
                sim.collect_charge()
                sim.solve_field()
                marks(sim, "dep1", "x")
                same_bits(sim.get_field()[1], rec["half_rho"], "chargeden after push 1")
                same_bits(sim.get_field()[0], rec["half_E"], "E after push 1")
        if has_events(inp):
            assert sim.optimize(2)
            assert [sim.rank_np(0, i) for i in range(ns)] == list(rec["ev_np"])
            marks(sim, "ev", "xvpw")
            same_bits(sim_gaussian_spare(oracle, sim), rec["ev_spare"], "spare Gaussian after the event")
            same_bits(sim_rng_ints(oracle, sim, NDRAWS), rec["ev_rng"], "random stream after the event")
            assert not sim.optimize(2)
        sim.collect_charge()
        marks(sim, "dep2", "x")
        same_bits(sim.get_field()[1], rec["dep2_rho"], "chargeden after push 2")
        sim.solve_field()
        E, _, re, im = sim.get_field()
        same_bits(re, rec["fs_re"], "mode_re")
        same_bits(im, rec["fs_im"], "mode_im")
        same_bits(E, rec["fs_E"], "E")
        tre, tim, ginv = oracle.Field(inp).tables()
        same_values(tre, rec["tab_re"], "cos table")
        same_values(tim, rec["tab_im"], "-sin table")
        same_bits(ginv, rec["grad_inv"], "mode_grad_inv")
        # the stand-alone solve entry (the one the GPU field tests use) on the same charge density
        E2, re2, im2 = oracle.Field(inp).solve(rec["dep2_rho"], 1)
        same_bits(E2, rec["fs_E"], "E (orc_field_solve_ranks)")
        same_bits(re2, rec["fs_re"], "mode_re (orc_field_solve_ranks)")
        same_bits(im2, rec["fs_im"], "mode_im (orc_field_solve_ranks)")
        # |delta f|(v): the same sequential sum in marker order on one rank
        for isp in range(ns):
            n = sim.rank_np(0, isp)
            h = np.zeros(inp.nv)
            oracle.lib().orc_dist_pertb_abs_v(C.byref(inp), n, sim.array(0, isp, "v")[:n].copy(), sim.array(0, isp, "w")[:n].copy(), h)
            same_bits(h, rec["hist"][isp], "|delta f|(v) species %d" % isp)
        for isp in range(ns):
            n = sim.rank_np(0, isp)
            sim.array(0, isp, "x")[:n] = far_positions(sim.array(0, isp, "x")[:n], lx)
        sim.collect_charge()
        marks(sim, "far", "x")
        same_bits(sim.get_field()[1], rec["far_rho"], "chargeden of far-out positions")
    if True:
        sim = fresh()
        sim.set_field(rec["E1"])
        sim.step(1)
        marks(sim, "st", "xvw")
        same_bits(sim.get_field()[0], rec["st_E"], "E after one step")
    if True:
        sim = fresh()
        sim.collect_charge()
        sim.solve_field()
        same_bits(sim.get_field()[0], rec["run_E0"], "initial E")
        sim.step(RUN_STEPS)
        assert [sim.rank_np(0, i) for i in range(ns)] == list(rec["run_np"])
        marks(sim, "run", "xvw")
        same_bits(sim.get_field()[0], rec["run_E"], "E after the run")
        same_bits(sim.get_field()[1], rec["run_rho"], "chargeden after the run")
        assert sim.time == rec["run_time"][0]
        same_bits(sim_gaussian_spare(oracle, sim), rec["run_spare"], "spare Gaussian after the run")
        same_bits(sim_rng_ints(oracle, sim, NDRAWS), rec["run_rng"], "random stream after the run")

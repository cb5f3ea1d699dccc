"""helpers of the lock-step tests of the whole-step marker kernels (tests/test_gpu_step_lockstep.py, and the oracle-only
census of tests/test_step_lockstep_host.py):

* the lock-step itself: engine `a` takes whole steps (pic1dp_hip_step: k_step_one in its three families, or k_step_half +
  k_step_full), engine `b` takes the two materialised sub-steps of every step ON a's FIELDS, an oracle Sim (optional) does
  the same on the CPU -- so that x, v and w can be compared marker by marker, bit for bit, after every step;
* the planted edge markers: a set that, in a geometry made of powers of two and with linear delta-f (v never changes),
  sits on its edges at EVERY step, and the census that says so from the oracle's state.
"""
import numpy as np

N_SWEEP = 2 ** 17 + 2 ** 12 + 3            # odd: several workgroups, a scalar tail
V_MAX = 8.0                                # input_v_max of the default input: the loader's |v| <= 8

# the geometry in which the planted markers stay on their edges exactly: the cell is 0.25 wide, dt v is a whole cell for
# |v| = 4 and two cells for |v| = 8, dt/2 v half a cell and a whole one; a Maxwellian at rest (no exp: w is bit-exact
# against the oracle; -f0'/f0 = v, so a marker at rest keeps its weight) in linear delta-f
EDGE_DYADIC = dict(lx=16.0, nx=64, dt=0.0625, linear=1, deltaf=1, iptcldist=0, species_density=[1.0], species_v0=[0.0],
                   init_mode_sin=[0.2])
# ... and one in which nothing is a power of two and v changes: the edges are met at the first step only
EDGE_GENERAL = dict(nx=96, linear=0, deltaf=1, iptcldist=0, species_density=[1.0], species_v0=[0.3],
                    species_temperature=[1.7], species_mass=[0.9], init_mode_sin=[0.2])

# every class of the census; a class is PRESENT at a step when at least one marker is in it at the step's start
CLASSES = ("x_plus_zero", "x_minus_zero", "x_lx", "x_last", "x_on_boundary", "x_below_boundary", "x_above_boundary",
           "xh_on_boundary", "xh_zero", "xh_lx", "crosses_end", "several_periods", "v_zero", "v_minus_zero",
           "v_beyond_vmax", "w_zero", "p_zero", "w_eq_p", "w_negative", "w_large")
# what the general geometry can hold at its first step (a half-step position exactly on a boundary needs dt/2 v exact)
CLASSES_FIRST_STEP = tuple(c for c in CLASSES if not c.startswith("xh_"))


def weight_unit(lx, n):
    """the marker weight of a uniform load, lx 2 v_max / n (src/pic1dp_particle.F90:183-217): the scale of p and w"""
    return lx * 2.0 * V_MAX / n


def exact_boundaries(lx, nx):
    """the cells k whose boundary k lx/nx the reference's own arithmetic x / lx * nx (src/pic1dp_interaction.F90:106,
    250) maps to k exactly: a marker there has left weight 1 exactly, its lower neighbour lies in cell k - 1"""
    k = np.arange(1, nx)
    x = k * lx / nx
    return [int(i) for i in k[x / lx * nx == k]]


def edge_markers(lx, nx, n):
    """(x, v, p, w) of the planted set.  vq = v_max / 2; in the dyadic geometry dt vq is one cell exactly."""
    h = lx / nx
    vq = V_MAX / 2
    u = weight_unit(lx, n)
    kb = exact_boundaries(lx, nx)
    assert len(kb) >= 5, "too few cell boundaries that x / lx * nx hits exactly"
    some = sorted({kb[0], kb[1], kb[len(kb) // 2], kb[-2], kb[-1]})
    xs, vs = [], []

    def add(x, v):
        xs.append(x)
        vs.append(v)

    # at rest (v = +0, -0 in turn): zero of both signs, the last representable position, positions that the first
    # deposit turns into lx (x + lx rounds to lx), the neighbours of zero, several periods out on both sides, and
    # every class of cell boundary: on it, one ulp below, one ulp above
    rest = [0.0, -0.0, np.nextafter(lx, 0.0), -1e-17, -5e-324, -1e-300, 5e-324, 1e-300, lx, np.nextafter(lx, 2 * lx),
            2.5 * lx, -3.25 * lx, 1e6 * lx + h / 2, -1e6 * lx - h / 2, 2 * lx, -lx, np.nextafter(-lx, 0.0), 0.5 * h]
    for k in some:
        rest += [k * lx / nx, np.nextafter(k * lx / nx, 0.0), np.nextafter(k * lx / nx, lx)]
    for i, x in enumerate(rest):
        add(x, -0.0 if i & 1 else 0.0)
    # the ladder: one ulp below the boundaries 1 .. 8, one cell down per step -- marker k is at -ulp after step k, which
    # the deposit stores as lx: x == lx at the start of the steps 2 .. 9
    for k in range(1, 9):
        add(np.nextafter(k * lx / nx, 0.0), -vq)
    # beyond v_max: three cells, 250 cells and four whole periods per step (the wrap's general path, the integer wrap
    # of the prediction's cell)
    for v in (3 * vq, -3 * vq, 1000.0, -1000.0, 1024.0, -1024.0):
        for x in (3 * h, 0.5 * h, 0.0, lx - h):
            add(x, v)
    # rings: a marker on every boundary for every velocity that moves it by whole cells -- the ring turns rigidly, so
    # at EVERY step somebody sits on 0, crosses either end, and (|v| = 2 vq) has its half-step position on a boundary,
    # on 0 and on lx; mid-cell markers with |v| = vq: half a cell in half a step, onto a boundary
    for v in (vq, -vq, 2 * vq, -2 * vq):
        for k in range(nx):
            add(k * lx / nx, v)
    for v in (vq, -vq):
        for k in range(nx):
            add(k * lx / nx + 0.5 * h, v)
    # weights, in turn: w = 0 (both signs), p = 0, w = p (tmp1 = 0 in nonlinear delta-f), negative, tiny; one marker in 64
    # a LARGE weight (128 u: all of them together weigh about what the loader's markers do, so the field stays of order
    # one).  A marker beyond v_max has -f0'/f0 ~ v of order 1000: its p and w are 2^-20 of the others', or its weight
    # update would come to rule the field within a few steps.
    pw = [(u, 0.0), (0.0, 0.5 * u), (0.75 * u, 0.75 * u), (u, -2.5 * u), (1.25 * u, 1e-300), (u, -0.0), (0.5 * u, 0.25 * u)]
    p = np.array([pw[i % len(pw)][0] for i in range(len(xs))])
    w = np.array([pw[i % len(pw)][1] for i in range(len(xs))])
    large = np.arange(len(xs)) % 64 == 5
    p[large], w[large] = u, 128.0 * u
    fast = np.abs(np.array(vs)) > V_MAX
    p[fast] *= 2.0 ** -20
    w[fast] *= 2.0 ** -20
    return np.array(xs), np.array(vs), p, w


def plant(base, lx, nx):
    """the loader population `base` (dict of x, v, p, w) with the planted set written over it at the head (slots 0, 1,
    126 .. 129), in the middle from an odd slot on (the other marker of each pair), far back (the rows a workgroup DRAWS
    when the launch is narrow enough to give it several) and at the very end, a ladder marker in the last slot (odd
    count: the scalar tail); returns the new dict"""
    n = base["x"].size
    ex, ev, ep, ew = edge_markers(lx, nx, n)
    L = ex.size
    assert n >= 8 * L and n & 1
    last = int(np.flatnonzero(ev == -V_MAX / 2)[0])            # the ladder's first marker: on lx at the second step
    out = {k: np.array(base[k], dtype=np.float64, copy=True) for k in "xvpw"}
    for start, roll in ((0, 0), ((n // 2) | 1, 3), ((4 * n // 5) & ~1, 5), (n - L, L - 1 - last)):
        for k, e in zip("xvpw", (ex, ev, ep, ew)):
            out[k][start:start + L] = np.roll(e, roll)
    assert out["v"][n - 1] == -V_MAX / 2 and out["x"][n - 1] == np.nextafter(lx / nx, 0.0)
    return out


def census(x, v, p, w, lx, nx, dt, n=None):
    """how many markers are in every class of CLASSES, from the state at the start of a step -- with the reference's own
    operations (x / lx * nx, :106, 250; x + dt/2 v and x + dt v, :261)"""
    u = weight_unit(lx, x.size if n is None else n)
    inside = (x > 0.0) & (x < lx)

    def on_boundary(y):
        s = y / lx * nx
        return s == np.floor(s)

    on_b = inside & on_boundary(x)
    xh = x + (0.5 * dt) * v
    xn = x + dt * v
    moving = v != 0.0
    return dict(
        x_plus_zero=int(np.sum((x == 0.0) & ~np.signbit(x))), x_minus_zero=int(np.sum((x == 0.0) & np.signbit(x))),
        x_lx=int(np.sum(x == lx)), x_last=int(np.sum(x == np.nextafter(lx, 0.0))), x_on_boundary=int(np.sum(on_b)),
        x_below_boundary=int(np.sum(inside & ~on_b & on_boundary(np.nextafter(x, np.inf)) & (np.nextafter(x, np.inf) < lx))),
        x_above_boundary=int(np.sum(inside & ~on_b & on_boundary(np.nextafter(x, -np.inf)) & (np.nextafter(x, -np.inf) > 0.0))),
        xh_on_boundary=int(np.sum(moving & (xh > 0.0) & (xh < lx) & on_boundary(xh))),
        xh_zero=int(np.sum(moving & (xh == 0.0))), xh_lx=int(np.sum(moving & (xh == lx))),
        crosses_end=int(np.sum(moving & ((xn < 0.0) | (xn >= lx)))),
        several_periods=int(np.sum((xn <= -2.0 * lx) | (xn >= 3.0 * lx))),
        v_zero=int(np.sum((v == 0.0) & ~np.signbit(v))), v_minus_zero=int(np.sum((v == 0.0) & np.signbit(v))),
        v_beyond_vmax=int(np.sum(np.abs(v) > V_MAX)),
        w_zero=int(np.sum(w == 0.0)), p_zero=int(np.sum(p == 0.0)), w_eq_p=int(np.sum((w == p) & (p != 0.0))),
        w_negative=int(np.sum(w < -2.0 * u)), w_large=int(np.sum(np.abs(w) >= 100.0 * u)))


def sim_state(sim, isp=0):
    return {k: sim.gather(k, isp) for k in "xvpw"}


def sim_census(sim):
    g = sim_state(sim)
    return census(g["x"], g["v"], g["p"], g["w"], sim.inp.lx, sim.inp.nx, sim.inp.dt)


def missing_classes(censuses, classes=CLASSES):
    """the classes that none of the censuses holds"""
    return [c for c in classes if not any(cs[c] > 0 for cs in censuses)]


def sim_plant(sim):
    """plant the edge set into a loaded one-rank, one-species oracle Sim; returns the planted population"""
    pop = plant(sim_state(sim), sim.inp.lx, sim.inp.nx)
    for k in "xvpw":
        sim.array(0, 0, k)[:pop[k].size] = pop[k]
    return pop


# --------------------------------------------------------------------------
# the lock-step
# --------------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def assert_same_bits(got, want, what):
    """bit for bit, the sign of a zero included"""
    ga, wa = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert ga.shape == wa.shape, what
    bad = np.flatnonzero(ga.view(np.int64) != wa.view(np.int64))
    assert bad.size == 0, "%s: %d of %d markers differ, the first at %d: %r against %r" % (
        what, bad.size, ga.size, bad[0], ga[bad[0]], wa[bad[0]])


def valid(eng, isp):
    """x, v, p, w of the species' loaded markers"""
    g = eng.particles_download(isp)
    npv = eng.local_sizes(isp)[1]
    return {k: g[k][:npv] for k in "xvpw"}


# family -> (environment of the engine, the name pic1dp_hip_kernel_bytes gives the kernel of the second sub-step)
FAMILIES = {
    "tiles": (dict(PIC1DP_PREDICT="1", PIC1DP_PRED_KIND="1"), "k_step_one"),
    "private_sums": (dict(PIC1DP_PREDICT="1", PIC1DP_PRED_KIND="2"), "k_step_one<sums>"),
    "register_sums": (dict(PIC1DP_PREDICT="1", PIC1DP_PRED_KIND="3"), "k_step_sums"),
    "own_choice": (dict(PIC1DP_PREDICT="1"), None),
    "two_pass": (dict(PIC1DP_PREDICT="0"), "k_step_full"),
}


def family_env(monkeypatch, family, **more):
    monkeypatch.delenv("PIC1DP_PRED_KIND", raising=False)
    for k, val in dict(FAMILIES[family][0], **more).items():
        monkeypatch.setenv(k, val)


def assert_family_ran(a, family, nsteps, nspecies=1, kernel=None):
    """the kernel that took the second sub-steps, as the library names it, and the passes: a one-pass family takes ONE
    first-sub-step pass per species (the very first step, which has no prediction to start from) and its kernel every
    step -- all steps but the first are predicted --, the two-pass pair k_step_half and k_step_full every step"""
    kernel = kernel or FAMILIES[family][1]
    half, full, one = (a.kernel_stats(k)[1] for k in (3, 4, 6))
    if family == "two_pass":
        name = a.kernel_bytes(4)["name"]
        assert name.startswith(kernel), name
        assert (half, full, one) == (nsteps * nspecies, nsteps * nspecies, 0), (half, full, one)
        assert a.kernel_bytes(3)["name"].startswith("k_step_half")
        return
    name = a.kernel_bytes(6)["name"]
    assert name.startswith(kernel) and (kernel != "k_step_one" or not name.startswith("k_step_one<sums>")), name
    assert (half, full, one) == (nspecies, 0, nsteps * nspecies), (half, full, one)
    assert nsteps >= 3, "a one-pass case holds at least two predicted steps"


def check_w(probe, inp, v_at, w_gpu, w_orc, wb_orc):
    """w of one push against the oracle's: bit for bit where -f0'/f0 holds no exp (and in full-f, where w is not
    evolved), else within the bounds tests/test_gpu_parity.py derives for one push"""
    from test_gpu_parity import assert_w_close, assert_w_close_one_exp, one_exp_active, w_cancellation
    if inp.deltaf == 0 or inp.iptcldist in (0, 1):
        assert_same_bits(w_gpu, w_orc, "w against the oracle")
    elif one_exp_active(probe, inp):
        assert_w_close_one_exp(inp, v_at, w_gpu, w_orc, wb_orc)
    else:
        assert_w_close(w_gpu, w_orc, wb_orc, False, w_cancellation(inp, v_at))


def lockstep(a, b, nsteps, nspecies=1, sim=None, probe=None, before_step=None):
    """a.step(1) against b's two materialised sub-steps on a's fields, after every step x, v, w of every species bit for
    bit.  With an oracle Sim beside them (same markers, the same fields imposed): after EITHER sub-step x and v bit for
    bit against b, w as check_w says -- and the oracle then takes b's w, so that the next push starts from the same
    weights on both sides (its own differ where an exp is involved).  before_step(it) is called at every step's start."""
    a.kernel_stats_enable(True)
    E0 = a.get_field(chargeden=False)["electric"]
    b.set_electric(E0)
    for it in range(nsteps):
        if before_step:
            before_step(it)
        a.step(1)
        Eh = a.get_field_half()
        E1 = a.get_field(chargeden=False)["electric"]
        for irk, E in ((1, E0), (2, Eh)):
            b.substep(irk)                        # (its own field, from its own deposit, is overwritten below)
            if sim is not None:
                sim.set_field(E)
                before = [(sim.gather("v", s), sim.gather("w", s) if irk == 1 else sim.gather("wb", s)) for s in range(nspecies)]
                sim.push(irk)
                sim.collect_charge()              # (wraps x, as b's deposit has)
                for s in range(nspecies):
                    g = valid(b, s)
                    assert_same_bits(g["x"], sim.gather("x", s), "x against the oracle, step %d sub-step %d species %d" % (it, irk, s))
                    assert_same_bits(g["v"], sim.gather("v", s), "v against the oracle, step %d sub-step %d species %d" % (it, irk, s))
                    check_w(probe, sim.inp, before[s][0], g["w"], sim.gather("w", s), before[s][1])
                    sim.array(0, s, "w")[:g["w"].size] = g["w"]
            b.set_electric(Eh if irk == 1 else E1)
        for s in range(nspecies):
            ga, gb = valid(a, s), valid(b, s)
            for k in "xvw":
                assert np.isfinite(ga[k]).all(), (k, it, s)       # (equal NaNs would prove nothing)
                assert_same_bits(ga[k], gb[k], "%s of whole step %d against the sub-steps, species %d" % (k, it, s))
        E0 = E1

"""The wave-particle power on the output grid (include/pic1dp_hip.h pic1dp_hip_power) on the GPU against
tests/power_reference.py: the exact sums of the very terms, and the bound on an FP64 sum in any order
(n_b + workgroups) 2^-53 sum |terms| (1 + 2^-20), which nothing here measures.  Every case sets a random field that is not
symmetric and changes sign, so that a wrong cell, weight or guard cell shows."""
import math

import numpy as np
import pytest

import moments_reference as MR
import power_reference as PR
from exact_charge import cells

pytestmark = pytest.mark.gpu

NAMES = ("total", "pertb")


def loaded(amd, **kw):
    e = amd.Pic1dp(amd.make_input(**kw))
    e.particle_load()
    return e


def started(amd, **kw):
    e = loaded(amd, **kw)
    e.interaction_collect_charge()
    e.field_solve_electric()
    return e


def uploaded(amd, x, v, p, w, junk=None, **kw):
    """a context holding exactly these markers as its valid ones; the tail slots hold `junk` (or zeros)"""
    n = len(x)
    e = amd.Pic1dp(amd.make_input(nparticle_max=max(n, 1), **kw))
    nalloc, _ = e.local_sizes()
    arrs = []
    for k, a in enumerate((x, v, p, w)):
        full = np.zeros(nalloc) if junk is None else np.full(nalloc, junk[k])
        full[:n] = a
        arrs.append(full)
    e.particles_upload(*arrs, np_valid=n)
    return e


def valid(e, s=0):
    g = e.particles_download(s)
    n = e.local_sizes(s)[1]
    return {k: a[:n] for k, a in g.items()}


def random_field(nx, seed):
    """not symmetric, with sign changes, no two neighbours alike"""
    E = np.random.default_rng(seed).normal(0.0, 1.0, nx) + 0.25
    if nx >= 2:
        E[0], E[-1] = 1.75, -2.5           # the guard cell's two candidates differ in sign and size
    assert nx < 2 or (np.any(E > 0) and np.any(E < 0))
    return E


def ratio(err, b):
    return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))


def within(got, ref_set, nwg, what=""):
    """plane, v-profile and rest of one set against the reference, each within its bound; returns the worst fraction"""
    worst = 0.0
    for key, g, exact, b in (("xv", got["xv"], ref_set["exact"], PR.bound(ref_set, nwg)),
                             ("v", got["v"], ref_set["exact"].sum(axis=1), PR.bound_v(ref_set, nwg)),
                             ("rest", np.array([got["rest"]]), np.array([ref_set["rest"]["exact"]]), np.array([PR.bound_rest(ref_set, nwg)]))):
        if key == "v":       # the exact row sums, not the sum of the rounded exact bins
            exact = np.array([math.fsum(row) for row in ref_set["exact"].tolist()])
            b = b + ref_set["exact"].shape[1] * PR.U * np.abs(ref_set["exact"]).sum(axis=1)
        err = np.abs(g - exact)
        r = ratio(err, b)
        worst = max(worst, r)
        assert np.all(err <= b), (what, key, r)
    print("power %s: worst error / bound = %.3g" % (what, worst))
    return worst


def check_against_markers(e, E, which=3, s=0, what=""):
    g = valid(e, s)
    n = g["x"].size
    ref = PR.reference(g["x"], g["v"], g["p"], g["w"], E, e.inp, which=which)
    got = e.power(s, which)
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert got[name]["xv"].shape == (e.inp.nv_opd, e.inp.nx_opd) and got[name]["v"].shape == (e.inp.nv_opd,)
        within(got[name], ref[name], PR.workgroups(n), "%s %s" % (what, name))
    return got, ref


# ---------------------------------------------------------------------------
# 1. edges
# ---------------------------------------------------------------------------
def edge_markers(lx, nx, v_max):
    xs = [0.0, lx, math.nextafter(lx, 0.0), -0.0, lx * (nx - 1) / nx + 0.25 * lx / nx]
    below = math.nextafter(v_max, 0.0)
    vs = [0.0, below, -below, v_max, -v_max, 2.0 * v_max, -2.0 * v_max]
    qs = [1.5, -2.25, 0.75]
    x, v, p, w = [], [], [], []
    for i, xi in enumerate(xs):
        for j, vj in enumerate(vs):
            x.append(xi), v.append(vj), p.append(qs[(i + j) % 3]), w.append(qs[(i + 2 * j + 1) % 3])
    return [np.array(a) for a in (x, v, p, w)]


@pytest.mark.parametrize("nx,nxo,nvo", [(2, 1, 2), (3, 3, 5), (8, 64, 64)])
def test_edges(amd, nx, nxo, nvo):
    inp0 = amd.make_input(nparticle_max=1, nx=nx, nx_opd=nxo, nv_opd=nvo)
    x, v, p, w = edge_markers(inp0.lx, nx, inp0.v_max)
    E = random_field(nx, 100 + nx)
    e = uploaded(amd, x, v, p, w, nx=nx, nx_opd=nxo, nv_opd=nvo)
    e.set_electric(E)
    got, ref = check_against_markers(e, E, 3, what="edges nx %d %d x %d" % (nx, nxo, nvo))
    singles = 0
    for name in NAMES:                      # bins with a single term: bit for bit
        one = ref[name]["count"] == 1
        assert np.array_equal(got[name]["xv"][one], ref[name]["exact"][one]), name
        assert not np.any(got[name]["xv"][ref[name]["count"] == 0])
        singles += int(one.sum())
        assert ref[name]["rest"]["count"] == 5 * 4
    assert singles > 0 or nxo * nvo <= 15
    # every marker on its own (slot 0; the others are tail slots now)
    nalloc, _ = e.local_sizes()
    rests = 0
    for i in range(x.size):
        arrs = [np.roll(np.concatenate([a, np.zeros(nalloc - a.size)]), -i) for a in (x, v, p, w)]
        e.particles_upload(*arrs, np_valid=1)
        g1 = e.power(0, 3)
        r1 = PR.reference(x[i:i + 1], v[i:i + 1], p[i:i + 1], w[i:i + 1], E, e.inp)
        for name in NAMES:
            cnt = r1[name]["count"]
            one = cnt == 1
            assert np.array_equal(g1[name]["xv"][one], r1[name]["exact"][one]), (i, name)
            assert not np.any(g1[name]["xv"][cnt == 0]), (i, name)
            within(g1[name], r1[name], 1, "marker %d alone %s" % (i, name))
            singles += int(one.sum())
            if abs(v[i]) >= e.inp.v_max:      # no bins: rest is the marker's term, bit for bit
                assert cnt.sum() == 0 and r1[name]["rest"]["count"] == 1
                assert g1[name]["rest"] == r1[name]["rest"]["exact"] != 0.0, (i, name)
                assert not np.any(g1[name]["xv"]) and not np.any(g1[name]["v"])
                rests += 1
            else:
                assert cnt.sum() == 4 and g1[name]["rest"] == 0.0
    # v = 0 and v just above -v_max have four distinct cells where nx_opd >= 2: 10 markers x 4 bins x 2 sets (v just below
    # +v_max rounds onto the top row, whose two rows coincide)
    assert rests == 2 * 5 * 4 and (singles >= 80 or nxo == 1)


# ---------------------------------------------------------------------------
# 2. shapes of the sweep, tail slots
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loader_markers(amd):
    """bump-on-tail markers from the loader, once.  The loader keeps |v| < v_max = 8; the contexts that take these markers
    have v_max = 4, so that some of them have no bins and feed rest"""
    n = 2**17 + 2**12 + 3
    e = loaded(amd, nparticle_max=n, nx=64)
    assert e.inp.v_max == 8.0
    g = valid(e)
    e.close()
    assert np.count_nonzero(np.abs(g["v"]) >= 4.0) > 100
    return g


@pytest.fixture(scope="module")
def loader_reference(amd, loader_markers):
    """the reference of all the loader's markers at nx 64, 64 x 64, once"""
    g = loader_markers
    inp = amd.make_input(nparticle_max=g["x"].size, nx=64, v_max=4.0)
    E = random_field(64, 7)
    return E, PR.reference(g["x"], g["v"], g["p"], g["w"], E, inp)


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2049, 2**17 + 2**12 + 3])
def test_shapes_of_the_sweep(amd, loader_markers, loader_reference, n):
    g = {k: a[:n] for k, a in loader_markers.items()}
    E, full = loader_reference
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    assert (e.inp.nx_opd, e.inp.nv_opd) == (64, 64)
    e.set_electric(E)
    if n == loader_markers["x"].size:
        got = e.power(0, 3)
        for name in NAMES:
            within(got[name], full[name], PR.workgroups(n), "np %d %s" % (n, name))
    else:
        got, _ = check_against_markers(e, E, 3, what="np %d" % n)
    if n == 0:
        for name in NAMES:
            assert not np.any(got[name]["xv"]) and not np.any(got[name]["v"]) and got[name]["rest"] == 0.0
    for which, name in ((1, "total"), (2, "pertb")):       # each set alone: the same terms
        one = e.power(0, which)
        assert list(one) == [name]
        if n <= 2:
            assert np.array_equal(one[name]["xv"], got[name]["xv"]) and one[name]["rest"] == got[name]["rest"]


def test_tail_slots_do_not_count(amd, loader_markers):
    """garbage in [np, nalloc) changes nothing, bit for bit (2049 markers: one workgroup... and the odd last marker)"""
    n = 2049
    g = {k: a[:n] for k, a in loader_markers.items()}
    E = random_field(64, 8)
    res = []
    for junk in (None, (3.3, -4.4, 7.0, -9.0)):
        e = amd.Pic1dp(amd.make_input(nparticle_max=n + 1500, nx=64, v_max=4.0))
        nalloc, _ = e.local_sizes()
        assert nalloc > n + 1
        arrs = []
        for k, key in enumerate("xvpw"):
            full = np.zeros(nalloc) if junk is None else np.full(nalloc, junk[k])
            full[:n] = g[key]
            arrs.append(full)
        e.particles_upload(*arrs, np_valid=n)
        assert e.local_sizes() == (nalloc, n)
        e.set_electric(E)
        check_against_markers(e, E, 3, what="np < nalloc, junk %s" % (junk is not None))
        res.append(e.power(0, 3))
    # 2049 markers are 1024 pairs in one workgroup, one pair per thread: every bin's additions have one order only where a
    # bin takes a single term, so "bit for bit" is asserted on what garbage would change: a counted tail slot adds terms
    for name in NAMES:
        a, b = res[0][name], res[1][name]
        tol = 2.0 * PR.bound(PR.reference(g["x"], g["v"], g["p"], g["w"], E, amd.make_input(nparticle_max=n, nx=64, v_max=4.0))[name], 1)
        assert np.all(np.abs(a["xv"] - b["xv"]) <= tol)
    # and bit for bit with a single valid marker, whose sums have one order
    outs = []
    for junk in (0.0, 5.5):
        e = amd.Pic1dp(amd.make_input(nparticle_max=600, nx=64, v_max=4.0))
        nalloc, _ = e.local_sizes()
        arrs = [np.full(nalloc, junk) for _ in range(4)]
        for a, key in zip(arrs, "xvpw"):
            a[0] = g[key][0]
        e.particles_upload(*arrs, np_valid=1)
        e.set_electric(E)
        outs.append(e.power(0, 3))
    for name in NAMES:
        assert np.any(outs[0][name]["xv"]) or outs[0][name]["rest"] != 0.0
        assert outs[0][name]["xv"].tobytes() == outs[1][name]["xv"].tobytes() and outs[0][name]["rest"] == outs[1][name]["rest"]
        assert outs[0][name]["v"].tobytes() == outs[1][name]["v"].tobytes()


# ---------------------------------------------------------------------------
# 3. every branch of the plan
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_markers():
    n = 200_001
    rng = np.random.default_rng(2017)
    return dict(u=rng.uniform(0.0, 1.0, n), v=rng.normal(0.0, 2.2, n), p=rng.uniform(0.5, 1.5, n), w=rng.normal(0.0, 0.1, n))


@pytest.mark.parametrize("nx,nxo,nvo,launches3,launches2", [(8192, 96, 96, 2, 1), (64, 160, 160, 1, 1), (8192, 64, 64, 1, 1)],
                         ids=["pass_per_set", "straight", "one_pass"])
def test_every_branch_of_the_plan(amd, probe, plan_markers, nx, nxo, nvo, launches3, launches2):
    m = plan_markers
    n = m["u"].size
    inp0 = amd.make_input(nparticle_max=n, nx=nx, nx_opd=nxo, nv_opd=nvo, v_max=4.0)
    x = m["u"] * inp0.lx
    assert np.count_nonzero(np.abs(m["v"]) >= inp0.v_max) > 100
    e = uploaded(amd, x, m["v"], m["p"], m["w"], nx=nx, nx_opd=nxo, nv_opd=nvo, v_max=4.0)
    E = random_field(nx, nx + nxo)
    e.set_electric(E)
    ref = PR.reference(x, m["v"], m["p"], m["w"], E, e.inp)
    nwg = PR.workgroups(n)
    plan = probe.host_power_plan(nx, nxo, nvo, 3, 1, n, 256)
    assert len(plan["passes"]) == launches3 and plan["passes"][0]["lds"] == (0 if nxo == 160 else 1)
    count = lambda: e.kernel_stats(20)[1]       # noqa: E731
    c0 = count()
    both = e.power(0, 3)
    assert count() - c0 == launches3
    for name in NAMES:
        within(both[name], ref[name], nwg, "nx %d %d x %d which 3 %s" % (nx, nxo, nvo, name))
    for which, name in ((1, "total"), (2, "pertb")):
        c0 = count()
        one = e.power(0, which)
        assert count() - c0 == launches2 and list(one) == [name]
        within(one[name], ref[name], nwg, "nx %d %d x %d which %d" % (nx, nxo, nvo, which))


def test_non_temporal_instance(amd, probe):
    """above 288 MiB of x, v, p, w the loads are non-temporal: against np.bincount sums of the same terms -- both lie
    within their bounds of the exact sum, so the tolerance is the sum of the two bounds"""
    n, nx = 9_500_000, 1024
    assert 32 * n > 288 * 1048576 and probe.host_power_plan(nx, 64, 64, 3, 1, n, 256)["passes"][0]["nt"] == 1
    e = loaded(amd, nparticle_max=n, nx=nx)
    E = random_field(nx, 5)
    e.set_electric(E)
    g = valid(e)
    c0 = e.kernel_stats(20)[1]
    got = e.power(0, 3)
    assert e.kernel_stats(20)[1] - c0 == 1
    nwg = PR.workgroups(n)
    for name, q in (("total", g["p"]), ("pertb", g["w"])):
        cell, t, rt = PR.terms(g["x"], g["v"], q, E, e.inp)
        nxv = e.inp.nx_opd * e.inp.nv_opd
        cnt = np.bincount(cell, minlength=nxv).reshape(e.inp.nv_opd, e.inp.nx_opd)
        ref_set = dict(abs=np.bincount(cell, weights=np.abs(t), minlength=nxv).reshape(cnt.shape), count=cnt)
        host = np.bincount(cell, weights=t, minlength=nxv).reshape(cnt.shape)
        tol = PR.bound(ref_set, nwg) + PR.bound(ref_set, 0, additions=cnt)
        err = np.abs(got[name]["xv"] - host)
        print("power NT %s: worst error / tolerance = %.3g" % (name, ratio(err, tol)))
        assert np.all(err <= tol), name
        sa = float(np.sum(np.abs(rt)))
        assert abs(got[name]["rest"] - math.fsum(rt.tolist())) <= (rt.size + nwg) * PR.U * sa * (1.0 + 2.0 ** -20), name


# ---------------------------------------------------------------------------
# 4. against the moments: sum of bins + rest = sum_ix E[ix] M1[ix]
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw,which", [(dict(), 2), (dict(), 1), (dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]), 1)],
                         ids=["deltaf_w", "deltaf_p", "full_f"])
def test_total_power_is_the_field_times_the_first_moment(amd, loader_markers, kw, which):
    """sum_i q v (E[ix] wl + E[ir] (1 - wl)) by two routes that share no kernel code but wrap and locate.  The bound, from the
    per-term roundings (nothing measured): each route rounds every marker's contribution a handful of times (the moments:
    wl q, times v, times E, and the sums; the power: two products and a sum for e, times v, times q, four weights) -- fewer
    than 16 roundings per marker and route beside the n additions of either sum -- so
        |difference| <= 2 (n + 16) 2^-53 sum_i (|E[ix]| wl + |E[ir]| (1 - wl)) |q v| (1 + 2^-20)"""
    if kw:      # full-f: the loader's own markers (none beyond v_max: rest stays empty)
        n = 200_001
        e = loaded(amd, nparticle_max=n, nx=64, **kw)
    else:       # delta f: the module's markers at half their v_max, rest is fed
        lm = loader_markers
        n = lm["x"].size
        e = uploaded(amd, lm["x"], lm["v"], lm["p"], lm["w"], nx=64, v_max=4.0)
    E = random_field(64, 21)
    e.set_electric(E)
    name = "pertb" if which == 2 else "total"
    g = valid(e)
    q = g["w"] if which == 2 else g["p"]
    pw = e.power(0, which)[name]
    assert kw or pw["rest"] != 0.0
    m1 = e.moments(0, which)[name][1]
    lhs = math.fsum(pw["xv"].ravel().tolist()) + pw["rest"]
    rhs = math.fsum((E * m1).tolist())
    _, ix, wl = cells(g["x"], e.inp)
    ir = (ix + 1) % e.inp.nx
    s = float(np.sum((np.abs(E[ix]) * wl + np.abs(E[ir]) * (1.0 - wl)) * np.abs(q * g["v"])))
    b = 2.0 * (n + 16) * PR.U * s * (1.0 + 2.0 ** -20)
    print("power vs moments %s: |diff| / bound = %.3g (sum %.6g)" % (name, abs(lhs - rhs) / b, lhs))
    assert b > 0 and lhs != 0.0 and abs(lhs - rhs) <= b
    # the v-profile sums to the plane
    assert abs(math.fsum(pw["v"].tolist()) - math.fsum(pw["xv"].ravel().tolist())) <= 64 * PR.U * float(np.abs(pw["xv"]).sum())


# ---------------------------------------------------------------------------
# 5. where the field comes from
# ---------------------------------------------------------------------------
def test_field_source(amd, loader_markers):
    n = 2049
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=64, v_max=4.0)
    e.set_electric(np.zeros(64))
    z = e.power(0, 3)
    for name in NAMES:
        assert not np.any(z[name]["xv"]) and not np.any(z[name]["v"]) and z[name]["rest"] == 0.0
    E1, E2 = random_field(64, 31), random_field(64, 32)
    e.set_electric(E1)
    check_against_markers(e, E1, 3, what="E1")
    e.set_electric(E2)
    got, ref = check_against_markers(e, E2, 3, what="E2 after E1")
    assert np.any(np.abs(got["total"]["xv"] - PR.reference(g["x"], g["v"], g["p"], g["w"], E1, e.inp)["total"]["exact"]) >
                  2.0 * PR.bound(ref["total"], 1))


def test_after_twenty_steps_of_the_default_case(amd):
    e = started(amd, nparticle_max=200_000)
    assert e.inp.nx == 192
    e.step(20)
    g = valid(e)
    E = e.get_field()["electric"]
    assert np.any(E > 0) and np.any(E < 0)
    ref = PR.reference(g["x"], g["v"], g["p"], g["w"], E, e.inp)
    got = e.power(0, 3)
    for name in NAMES:
        within(got[name], ref[name], PR.workgroups(g["x"].size), "after 20 steps %s" % name)
        assert np.any(got[name]["xv"])


# ---------------------------------------------------------------------------
# 6. nothing changes between steps
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [(2, dict()), (1, dict(nmode=2, modes=[1, 2]))], ids=["six_sums", "tiles_two_modes"])
def test_between_steps_nothing_changes(amd, monkeypatch, kind, kw):
    """the prediction (and with the six sums the fused solve) survives the call: the steps after it stay one pass, and the
    run is the run that never asked, bit for bit (96 markers, nx 32: the sums have one order)"""
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    if kind == 2:
        monkeypatch.setenv("PIC1DP_FUSE_SOLVE", "2")
    a, b = (started(amd, nparticle_max=96, nx=32, **kw) for _ in range(2))
    for e in (a, b):
        assert e.predict_kind() == kind
        e.kernel_stats_enable(True)
        e.step(5)
    got = a.power(0, 3)
    assert np.any(got["total"]["xv"]) and a.kernel_stats(20)[1] == 1 and b.kernel_stats(20)[1] == 0
    for e in (a, b):
        e.step(5)
    for e in (a, b):
        if kind == 2:
            assert e.kernel_stats(7)[1] == 8                                # all but the last step of each call
        assert e.kernel_stats(3)[1] == 1 and e.kernel_stats(6)[1] == 10    # one first-sub-step pass: the run's first step
    assert a.state_digest().tolist() == b.state_digest().tolist()
    fa, fb = a.get_field(), b.get_field()
    for k in ("electric", "chargeden", "mode_re", "mode_im"):
        assert fa[k].tobytes() == fb[k].tobytes(), k
    assert a.energy_history().tobytes() == b.energy_history().tobytes()
    assert a.get_field_half().tobytes() == b.get_field_half().tobytes()


# ---------------------------------------------------------------------------
# 7. inside a step
# ---------------------------------------------------------------------------
def marker_launches(e):
    """push, deposit and whole-step kernels launched so far (kernel stats enabled)"""
    return sum(e.kernel_stats(which)[1] for which in (0, 1, 2, 3, 4, 6))


def test_inside_a_step_the_noted_push_is_materialised(amd, monkeypatch):
    kw = dict(nparticle_max=50_001, nx=96)
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", "2")
    a = started(amd, **kw)
    monkeypatch.setenv("PIC1DP_PREDICT", "0")
    monkeypatch.delenv("PIC1DP_PRED_KIND")
    monkeypatch.setenv("PIC1DP_LAZY_CALLS", "0")
    b = started(amd, **kw)
    monkeypatch.delenv("PIC1DP_LAZY_CALLS")
    b.set_electric(a.get_field()["electric"])
    for e in (a, b):
        e.kernel_stats_enable(True)
    nwg = PR.workgroups(kw["nparticle_max"])
    for it in range(2):
        for irk in (1, 2):
            for e in (a, b):
                e.interaction_push_particle(irk)
            if irk == 1:
                # the lazy context has only noted its push: the call materialises it (a marker kernel runs); the eager one launches none
                before = [marker_launches(e) for e in (a, b)]
                pa = a.power(0, 3)
                pb = b.power(0, 3)
                assert marker_launches(a) > before[0] and marker_launches(b) == before[1]
                g = valid(b)
                E = b.get_field()["electric"]
                ref = PR.reference(g["x"], g["v"], g["p"], g["w"], E, b.inp)
                for name in NAMES:
                    within(pb[name], ref[name], nwg, "eager, inside step %d %s" % (it, name))
                    within(pa[name], ref[name], nwg, "lazy, inside step %d %s" % (it, name))
            for e in (a, b):
                e.interaction_collect_charge()
                e.field_solve_electric()
            fa, fb = a.get_field(), b.get_field()
            assert np.max(np.abs(fa["electric"] - fb["electric"])) <= 1e-11 * np.max(np.abs(fb["electric"])), (it, irk)
            b.set_electric(fa["electric"])
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k]), (k, it)


# ---------------------------------------------------------------------------
# 8. two contexts as two ranks
# ---------------------------------------------------------------------------
def test_two_ranks_local_power_adds_up_on_the_host(amd, loader_markers):
    kw = dict(nparticle_max=40_002, nx=64, v_max=4.0)
    engs = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2, device=0) for r in range(2)]
    E = random_field(64, 77)
    for r, e in enumerate(engs):          # the halves of one marker set
        nalloc, _ = e.local_sizes()
        assert nalloc >= 20_001
        arrs = []
        for k in "xvpw":
            full = np.zeros(nalloc)
            full[:20_001] = loader_markers[k][r * 20_001:(r + 1) * 20_001]
            arrs.append(full)
        e.particles_upload(*arrs, np_valid=20_001)
        e.set_electric(E)
    parts = [valid(e) for e in engs]
    local = [e.power(0, 3) for e in engs]
    allm = {k: np.concatenate([g[k] for g in parts]) for k in "xvpw"}
    ref = PR.reference(allm["x"], allm["v"], allm["p"], allm["w"], E, engs[0].inp)
    refs = [PR.reference(g["x"], g["v"], g["p"], g["w"], E, engs[0].inp) for g in parts]
    for name in NAMES:
        total = local[0][name]["xv"] + local[1][name]["xv"]
        # each rank within its own bound, and one more addition by the host
        b = sum(PR.bound(r[name], PR.workgroups(g["x"].size)) for r, g in zip(refs, parts)) + PR.U * ref[name]["abs"] * (1.0 + 2.0 ** -20)
        err = np.abs(total - ref[name]["exact"])
        print("power two ranks %s: worst error / bound = %.3g" % (name, ratio(err, b)))
        assert np.all(err <= b), name
        rest = local[0][name]["rest"] + local[1][name]["rest"]
        br = sum(PR.bound_rest(r[name], PR.workgroups(g["x"].size)) for r, g in zip(refs, parts)) + PR.U * ref[name]["rest"]["abs"] * (1.0 + 2.0 ** -20)
        assert ref[name]["rest"]["count"] > 10 and abs(rest - ref[name]["rest"]["exact"]) <= br, name


# ---------------------------------------------------------------------------
# 9. refusals
# ---------------------------------------------------------------------------
def test_refusals_name_the_cause(amd):
    e = loaded(amd, nparticle_max=1000, nx=16, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    for which in (2, 3):
        with pytest.raises(amd.Pic1dpError) as ei:
            e.power(0, which)
        assert ei.value.code == 1 and "full-f" in str(ei.value) and "which = %d" % which in str(ei.value)
    for which in (0, 4):
        with pytest.raises(amd.Pic1dpError) as ei:
            e.power(0, which)
        assert ei.value.code == 1 and "which = %d" % which in str(ei.value)
    with pytest.raises(amd.Pic1dpError) as ei:
        e.power(1, 1)
    assert ei.value.code == 1 and "species" in str(ei.value)
    L = amd._lib.load()
    assert L.pic1dp_hip_power(e._ctx, 0, 1, None) == 1 and b"null output" in L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_power(None, 0, 1, None) == 1 and b"null context" in L.pic1dp_hip_last_error()
    assert list(e.power(0, 1)) == ["total"]
    assert MR.workgroups(1000) == PR.workgroups(1000)

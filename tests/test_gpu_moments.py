"""The velocity moments of the markers on the field grid (include/pic1dp_hip.h pic1dp_hip_moments) on the
GPU against tests/moments_reference.py: the exact sums of the very terms, and the bound on an FP64 sum in any order
(n_b + workgroups) 2^-53 sum |terms| (1 + 2^-20), which nothing here measures."""
import math

import numpy as np
import pytest

import moments_reference as MR
from util import relerr

pytestmark = pytest.mark.gpu

TWO = dict(nspecies=2, species_charge=[-1.0, 1.0], species_mass=[1.0, 4.0], species_temperature=[1.0, 1.0],
           species_temperature2=[1.0, 1.0], species_density=[0.9, 0.9], species_v0=[5.0, 5.0])


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


def within(got, ref_set, nwg, factor=1.0, what=""):
    err = np.abs(got - ref_set["exact"])
    b = MR.bound(ref_set, nwg) * factor
    worst = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))
    print("moments %s: worst error / bound = %.3g" % (what, worst))
    assert np.all(err <= b), (what, worst)


def check_against_markers(e, which=3, s=0, what="", factor=1.0):
    g = valid(e, s)
    n = g["x"].size
    ref = MR.reference(g["x"], g["v"], g["p"], g["w"], e.inp, which=which)
    got = e.moments(s, which)
    assert sorted(got) == sorted(ref)
    for name in ref:
        assert got[name].shape == (4, e.inp.nx)
        within(got[name], ref[name], MR.workgroups(n), factor, "%s %s" % (what, name))
    return got, ref


# ---------------------------------------------------------------------------
# 1. edges
# ---------------------------------------------------------------------------
def edge_markers(lx, nx, v_max):
    below = math.nextafter(lx, 0.0)
    xs = [0.0, -0.0, lx, below, lx + 1e-13, -1e-300, 7.3 * lx, -7.3 * lx, -1e-16,              # (-1e-16 + lx rounds to exactly lx)
          0.5 * lx / nx, lx * (nx - 1) / nx + 0.25 * lx / nx]
    vs = [0.0, v_max, -v_max, 1e100, -1e100, 1.1, -2.7]
    qs = [1.5, -2.25, 0.0]
    x, v, p, w = [], [], [], []
    for i, xi in enumerate(xs):
        for j, vj in enumerate(vs):
            x.append(xi), v.append(vj), p.append(qs[(i + j) % 3]), w.append(qs[(i + 2 * j + 1) % 3])
    return [np.array(a) for a in (x, v, p, w)]


@pytest.mark.parametrize("nx", [2, 3, 8])
def test_edges(amd, nx):
    inp0 = amd.make_input(nparticle_max=1, nx=nx)
    x, v, p, w = edge_markers(inp0.lx, nx, inp0.v_max)
    assert (-1e-300 + inp0.lx) == inp0.lx and (-1e-16 + inp0.lx) == inp0.lx
    e = uploaded(amd, x, v, p, w, nx=nx)
    check_against_markers(e, 3, what="edges nx %d" % nx)
    # every marker on its own (slot 0; the others are tail slots now): its two bins receive a single term -- bit for bit
    nalloc, _ = e.local_sizes()
    singles = 0
    for i in range(x.size):
        arrs = []
        for a in (x, v, p, w):
            full = np.roll(np.concatenate([a, np.zeros(nalloc - a.size)]), -i)
            arrs.append(full)
        e.particles_upload(*arrs, np_valid=1)
        g1 = e.moments(0, 3)
        r1 = MR.reference(x[i:i + 1], v[i:i + 1], p[i:i + 1], w[i:i + 1], e.inp)
        for name in ("total", "pertb"):
            one = r1[name]["count"] == 1
            assert one.sum() == 2 and r1[name]["count"].sum() == 2
            assert np.array_equal(g1[name][:, one], r1[name]["exact"][:, one]), (i, name)
            assert not np.any(g1[name][:, ~one])
            singles += int(np.count_nonzero(r1[name]["exact"]))
    assert singles > 100


# ---------------------------------------------------------------------------
# 2. shapes of the sweep
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loader_markers(amd):
    """bump-on-tail markers from the loader, once"""
    n = 2**17 + 2**12 + 3
    e = loaded(amd, nparticle_max=n, nx=192)
    g = valid(e)
    e.close()
    return g


@pytest.mark.parametrize("n", [0, 1, 2, 2047, 2049, 2**17 + 2**12 + 3])
def test_shapes_of_the_sweep(amd, loader_markers, n):
    g = {k: a[:n] for k, a in loader_markers.items()}
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=192)
    got, _ = check_against_markers(e, 3, what="np %d" % n)
    if n == 0:
        assert not np.any(got["total"]) and not np.any(got["pertb"])


@pytest.mark.parametrize("drawn", ["0", "16"])
def test_rows_all_dealt_and_all_drawn(amd, monkeypatch, tuning, loader_markers, drawn):
    """tuning knob PIC1DP_DYN_TAIL at its two ends -- every row of a workgroup dealt, every row drawn by its waves: every pair
    exactly once whoever takes it, each weight set alone and both, within the bound of the default setting"""
    g = loader_markers
    monkeypatch.setenv("PIC1DP_DYN_TAIL", drawn)
    e = uploaded(amd, g["x"], g["v"], g["p"], g["w"], nx=192)
    _, ref = check_against_markers(e, 3, what="PIC1DP_DYN_TAIL=%s" % drawn)
    for which, name in ((1, "total"), (2, "pertb")):
        got = e.moments(0, which)
        assert list(got) == [name]
        within(got[name], ref[name], MR.workgroups(g["x"].size), 1.0, "PIC1DP_DYN_TAIL=%s which %d" % (drawn, which))


def test_tail_slots_do_not_count(amd, loader_markers):
    n = 2049
    g = {k: a[:n] for k, a in loader_markers.items()}
    inp = amd.make_input(nparticle_max=n + 1500, nx=192)
    e = amd.Pic1dp(inp)
    nalloc, _ = e.local_sizes()
    assert nalloc > n
    arrs = []
    for k, junk in zip("xvpw", (3.3, -4.4, 7.0, -9.0)):      # non-zero junk in the tail slots
        full = np.full(nalloc, junk)
        full[:n] = g[k]
        arrs.append(full)
    e.particles_upload(*arrs, np_valid=n)
    assert e.local_sizes() == (nalloc, n)
    check_against_markers(e, 3, what="np < nalloc")


# ---------------------------------------------------------------------------
# 3. plan boundaries
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx,launches3,launches1", [(2048, 1, 1), (2400, 1, 1), (4096, 2, 1), (4800, 2, 1), (8192, 4, 2)])
def test_plan_boundaries(amd, nx, launches3, launches1):
    """(nx 2400 with eight planes and nx 4800 with four fill a pass's LDS to the cap, 153 600 B)"""
    n = 2**16 + 1
    rng = np.random.default_rng(nx)
    inp0 = amd.make_input(nparticle_max=n, nx=nx)
    x = rng.uniform(0.0, inp0.lx, n)
    v = rng.normal(0.0, 2.0, n)
    p = rng.uniform(0.5, 1.5, n)
    w = rng.normal(0.0, 0.1, n)
    e = uploaded(amd, x, v, p, w, nx=nx)
    ref = MR.reference(x, v, p, w, e.inp)
    nwg = MR.workgroups(n)
    count = lambda: e.kernel_stats(16)[1]       # noqa: E731
    c0 = count()
    both = e.moments(0, 3)
    assert count() - c0 == launches3
    for name in ("total", "pertb"):
        within(both[name], ref[name], nwg, what="nx %d which 3 %s" % (nx, name))
    for which, name in ((1, "total"), (2, "pertb")):
        c0 = count()
        one = e.moments(0, which)
        assert count() - c0 == launches1 and list(one) == [name]
        within(one[name], ref[name], nwg, what="nx %d which %d" % (nx, which))
        assert np.all(np.abs(one[name] - both[name]) <= 2.0 * MR.bound(ref[name], nwg))


# ---------------------------------------------------------------------------
# 4. the non-temporal instance
# ---------------------------------------------------------------------------
def test_non_temporal_instance(amd):
    """above 288 MiB of x, v, p, w the loads are non-temporal: against np.bincount sums of the same terms -- both lie
    within their bounds of the exact sum, so the tolerance is the sum of the two bounds"""
    n, nx = 9_500_000, 1024
    assert 32 * n > 288 * 1048576
    e = loaded(amd, nparticle_max=n, nx=nx)
    g = valid(e)
    got = e.moments(0, 3)
    nwg = MR.workgroups(n)
    for name, q in (("total", g["p"]), ("pertb", g["w"])):
        cell, ts = MR.terms(g["x"], g["v"], q, e.inp)
        cnt = np.bincount(cell, minlength=nx)
        ref_set = dict(abs=np.stack([np.bincount(cell, weights=np.abs(t), minlength=nx) for t in ts]), count=cnt)
        host = np.stack([np.bincount(cell, weights=t, minlength=nx) for t in ts])
        tol = MR.bound(ref_set, nwg) + MR.bound(ref_set, 0, additions=cnt)
        err = np.abs(got[name] - host)
        print("moments NT %s: worst error / tolerance = %.3g" % (name, float(np.max(err / np.where(tol > 0, tol, 1.0)))))
        assert np.all(err <= tol), name


# ---------------------------------------------------------------------------
# 5. against the deposit
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kw,which", [(dict(), 2), (dict(deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0]), 1),
                                      (dict(species_nparticle_init=[20000, 7001], **TWO), 2),
                                      (dict(species_nparticle_init=[20000, 7001], deltaf=0, iptcldist=0, **dict(TWO, species_v0=[0.0, 0.0])), 1)],
                         ids=["deltaf", "full_f", "deltaf_two_species", "full_f_two_species"])
def test_zeroth_moment_is_the_deposited_charge(amd, kw, which):
    e = loaded(amd, nparticle_max=20000, nx=64, **kw)
    e.interaction_collect_charge()
    cd = e.get_field()["chargeden"]
    inp = e.inp
    name = "pertb" if which == 2 else "total"
    c2 = np.zeros(inp.nx)
    for s in range(inp.nspecies):
        c2 = c2 + e.moments(s, which)[name][0] * inp.species_charge[s]
    mine = c2 * float(inp.nx) / inp.lx
    if not inp.deltaf:
        for s in range(inp.nspecies):
            mine = mine - inp.species_charge[s] * inp.species_density[s]
    scale = np.max(np.abs(cd))
    print("moments vs deposit: max |diff| / max |chargeden| = %.3g" % (np.max(np.abs(mine - cd)) / scale))
    assert scale > 0 and np.max(np.abs(mine - cd)) <= 1e-12 * scale
    if inp.nspecies == 2:
        assert e.local_sizes(0)[1] != e.local_sizes(1)[1]


def test_w_of_a_full_f_context_is_refused_by_name(amd):
    e = loaded(amd, nparticle_max=1000, nx=16, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    for which in (2, 3):
        with pytest.raises(amd.Pic1dpError) as ei:
            e.moments(0, which)
        assert ei.value.code == 1 and "full-f" in str(ei.value) and "which = %d" % which in str(ei.value)
    for which in (0, 4):
        with pytest.raises(amd.Pic1dpError) as ei:
            e.moments(0, which)
        assert ei.value.code == 1
    with pytest.raises(amd.Pic1dpError) as ei:
        e.moments(1, 1)
    assert ei.value.code == 1
    assert list(e.moments(0, 1)) == ["total"]


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
    got = a.moments(0, 3)
    assert np.any(got["total"]) and a.kernel_stats(16)[1] == 1 and b.kernel_stats(16)[1] == 0
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
    for it in range(2):
        for irk in (1, 2):
            for e in (a, b):
                e.interaction_push_particle(irk)
            if irk == 1:
                # the lazy context has only noted its push: the call materialises it (a marker kernel runs); the eager one launches none
                before = [marker_launches(e) for e in (a, b)]
                ma = a.moments(0, 3)
                b.moments(0, 3)
                assert marker_launches(a) > before[0] and marker_launches(b) == before[1]
                mb, ref = check_against_markers(b, 3, what="eager, inside step %d" % it)
                nwg = MR.workgroups(kw["nparticle_max"])
                for name in ("total", "pertb"):
                    within(ma[name], ref[name], nwg, what="lazy, inside step %d %s" % (it, name))
                    assert np.all(np.abs(ma[name] - mb[name]) <= 2.0 * MR.bound(ref[name], nwg)), name
            for e in (a, b):
                e.interaction_collect_charge()
                e.field_solve_electric()
            fa, fb = a.get_field(), b.get_field()
            assert relerr(fa["electric"], fb["electric"]) < 1e-11, (it, irk)
            b.set_electric(fa["electric"])
        ga, gb = a.particles_download(), b.particles_download()
        for k in "xvw":
            assert np.array_equal(ga[k], gb[k]), (k, it)


# ---------------------------------------------------------------------------
# 8. after steps, on the GPU's own markers
# ---------------------------------------------------------------------------
def test_after_twenty_steps_of_the_default_case(amd):
    e = started(amd, nparticle_max=200_000)
    assert e.inp.nx == 192
    e.step(20)
    check_against_markers(e, 3, what="after 20 steps")


# ---------------------------------------------------------------------------
# 9. two contexts as two ranks
# ---------------------------------------------------------------------------
def test_two_ranks_local_moments_add_up_on_the_host(amd):
    kw = dict(nparticle_max=40_002, nx=64)
    engs = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2, device=0) for r in range(2)]
    for e in engs:
        e.particle_load()
    parts = [valid(e) for e in engs]
    local = [e.moments(0, 3) for e in engs]
    allm = {k: np.concatenate([g[k] for g in parts]) for k in "xvpw"}
    ref = MR.reference(allm["x"], allm["v"], allm["p"], allm["w"], engs[0].inp)
    refs = [MR.reference(g["x"], g["v"], g["p"], g["w"], engs[0].inp) for g in parts]
    for name in ("total", "pertb"):
        total = local[0][name] + local[1][name]
        b = sum(MR.bound(r[name], MR.workgroups(g["x"].size)) for r, g in zip(refs, parts))
        err = np.abs(total - ref[name]["exact"])
        print("moments two ranks %s: worst error / bound = %.3g" % (name, float(np.max(err / b))))
        assert np.all(err <= b), name

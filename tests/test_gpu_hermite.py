"""The Fourier-Hermite spectrum of the markers (include/pic1dp_hip.h pic1dp_hip_hermite) on the GPU against
tests/hermite_reference.py: the exact sums of the very terms, and the stated bound on an FP64 sum in any order
(n_p + B + 16) 2^-53 sum |T| (1 + 2^-20), B the partial sums the plan says the launch merges.  Nothing here measures a
tolerance."""
import ctypes as C
import math

import numpy as np
import pytest

import hermite_reference as HR
from util import relerr

pytestmark = pytest.mark.gpu

NUM_CU = 256                 # MI355X; below 2^21 markers the plan does not depend on it
NAN4 = (math.nan,) * 4
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


def uploaded(amd, x, v, p, w, junk=NAN4, spare=64, **kw):
    """a context holding exactly these markers as its valid ones; the tail slots (at least `spare`) hold `junk`: NaN"""
    n = len(x)
    e = amd.Pic1dp(amd.make_input(nparticle_max=n + spare, **kw))
    nalloc, _ = e.local_sizes()
    assert nalloc >= n + spare
    arrs = []
    for k, a in enumerate((x, v, p, w)):
        full = np.full(nalloc, junk[k])
        full[:n] = a
        arrs.append(full)
    e.particles_upload(*arrs, np_valid=n)
    assert e.local_sizes() == (nalloc, n)
    return e


def valid(e, s=0):
    g = e.particles_download(s)
    n = e.local_sizes(s)[1]
    return {k: a[:n] for k, a in g.items()}


def partials(probe, n, nherm, nmodes, which, deltaf=1):
    pl = probe.host_hermite_plan(nherm, nmodes, which, deltaf, n, NUM_CU)
    assert pl["blocks"] >= 1
    return pl["partials"]


def sub(ref_set, cols=None, nherm=None):
    """the modes `cols` and the first nherm rows of a reference set"""
    cols = slice(None) if cols is None else list(cols)
    return dict(exact=ref_set["exact"][cols][:, :, :nherm], abs=ref_set["abs"][cols][:, :, :nherm], count=ref_set["count"])


def within(got, ref_set, B, what=""):
    worst = HR.worst(HR.raw(got), ref_set, B)
    print("hermite %s: worst error / bound = %.3g" % (what, worst))
    assert worst <= 1.0, (what, worst)
    return worst


def check(e, probe, modes, nherm, v0, vt, which, s=0, ref=None, what=""):
    g = valid(e, s)
    if ref is None:
        ref = HR.reference(g["x"], g["v"], g["p"], g["w"], e.inp, modes, nherm, v0, vt, which)
    got = e.hermite(s, modes, nherm, v0, vt, which)
    assert sorted(got) == sorted(n for bit, n in ((1, "total"), (2, "pertb")) if which & bit)
    B = partials(probe, g["x"].size, nherm, len(modes), which, e.inp.deltaf)
    for name in got:
        assert got[name].shape == (len(modes), nherm) and got[name].dtype == np.complex128
        within(got[name], ref[name], B, "%s %s" % (what, name))
        for a, m in enumerate(modes):
            if m == 0:
                assert not np.any(got[name][a].imag), "mode 0: the sin row is exactly 0"
    return got, ref


def host_markers(amd, n, **kw):
    """n valid markers of the loader, generated on the host"""
    inp = amd.make_input(nparticle_max=n, **kw)
    L = amd._lib.load()
    na, nv = C.c_int64(), C.c_int64()
    amd._lib.check(L.pic1dp_hip_block_sizes(C.byref(inp), 0, 0, 1, C.byref(na), C.byref(nv)))
    arrs = [np.empty(inp.nspecies * na.value) for _ in range(4)]
    amd._lib.check(L.pic1dp_hip_host_particle_load(C.byref(inp), 0, 1, *[a.ctypes.data_as(C.c_void_p) for a in arrs], na.value))
    assert nv.value >= n
    return [a[:n].copy() for a in arrs]


# ---------------------------------------------------------------------------
# 1. the recurrence
# ---------------------------------------------------------------------------
def test_recurrence_is_numpys_bit_for_bit(probe):
    u = np.array([0.0, 1.0, -1.0, 8.0, -8.0, 16.0, -16.0, 1e-300])
    dev = probe.hermite(u, 256)
    ref = HR.psi(u, 256).T
    assert dev.shape == (8, 256) and np.array_equal(dev, ref)
    big = np.max(np.abs(dev[5:7]))
    assert np.all(np.isfinite(dev)) and 3.6e27 < big < 3.8e27
    for nherm in (1, 2, 17):
        assert np.array_equal(probe.hermite(u, nherm), ref[:, :nherm])


# ---------------------------------------------------------------------------
# 2. the lane map, on planted markers
# ---------------------------------------------------------------------------
PLANT = dict(x=1.7, v=0.9, p=1.5, w=-2.25)


def single_terms(inp, modes, nherm, v0, vt):
    """psi_n q trig of the planted marker for both sets: (2, nmodes, 2, nherm), from numpy"""
    one = {k: np.array([val]) for k, val in PLANT.items()}
    ref = HR.reference(one["x"], one["v"], one["p"], one["w"], inp, modes, nherm, v0, vt, 3)
    return np.stack([ref["total"]["exact"], ref["pertb"]["exact"]])


def assert_single(got, terms, what):
    raw = np.stack([HR.raw(got["total"]), HR.raw(got["pertb"])])
    assert np.all(np.abs(raw - terms) <= 18 * HR.U * np.abs(terms)), what
    assert not np.any(raw[:, 0, 1]), what                       # mode 0: the sin row is exactly 0
    assert np.all(raw[:, 1:] != 0.0) and np.all(raw[:, 0, 0] != 0.0), what


def test_one_marker_with_nan_in_the_tail(amd):
    modes, nherm, v0, vt = (0, 1, 3), 64, 0.25, 1.5
    e = uploaded(amd, *[np.array([PLANT[k]]) for k in "xvpw"], nx=8)
    terms = single_terms(e.inp, modes, nherm, v0, vt)
    th = 2.0 * np.pi / e.inp.lx * PLANT["x"]
    assert abs(abs(math.cos(th)) - abs(math.sin(th))) > 0.1 and PLANT["p"] != PLANT["w"]
    assert_single(e.hermite(0, modes, nherm, v0, vt, 3), terms, "one marker")
    for which, name, j in ((1, "total", 0), (2, "pertb", 1)):
        got = e.hermite(0, modes, nherm, v0, vt, which)
        assert list(got) == [name]
        assert np.all(np.abs(HR.raw(got[name]) - terms[j]) <= 18 * HR.U * np.abs(terms[j]))


@pytest.mark.parametrize("at", [0, 1, 3, 4, 63, 64])
def test_one_marker_among_weightless_ones(amd, at):
    """65 valid markers of which one has weights: every k slot and group of the fragment, and the second chunk"""
    modes, nherm, v0, vt = (0, 1, 3), 64, 0.25, 1.5
    rng = np.random.default_rng(at)
    inp0 = amd.make_input(nparticle_max=1, nx=8)
    x, v = rng.uniform(0.0, inp0.lx, 65), rng.normal(0.0, 2.0, 65)
    p, w = np.zeros(65), np.zeros(65)
    x[at], v[at], p[at], w[at] = (PLANT[k] for k in "xvpw")
    e = uploaded(amd, x, v, p, w, nx=8)
    assert_single(e.hermite(0, modes, nherm, v0, vt, 3), single_terms(e.inp, modes, nherm, v0, vt), "marker at %d" % at)


# ---------------------------------------------------------------------------
# 3. counts around the tiles
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loader_markers(amd):
    """bump-on-tail markers from the loader (on the host), once, and their reference columns are computed per count"""
    return host_markers(amd, 8193, nx=64)


@pytest.mark.parametrize("n", [1, 3, 5, 63, 65, 255, 257, 4095, 4097, 8191, 8193])
def test_counts_around_the_tiles(amd, probe, loader_markers, n):
    """a chunk of 64 markers +- 1, every wave of a workgroup with one chunk +- 1 (64 x 4), one and two workgroups' fill
    (4096, 8192) +- 1; the last marker odd, NaN in the tail slots"""
    x, v, p, w = (a[:n] for a in loader_markers)
    e = uploaded(amd, x, v, p, w, nx=64)
    pl = probe.host_hermite_plan(70, 2, 3, 1, n, NUM_CU)
    assert pl["blocks"] == (n + 4095) // 4096 and pl["nb"] == 8
    check(e, probe, (1, 3), 70, 0.5, 1.25, 3, what="np %d" % n)


# ---------------------------------------------------------------------------
# 4. edges
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [2, 64])
@pytest.mark.parametrize("nherm", [1, 15, 16, 17, 100, 256])
def test_edges(amd, probe, nx, nherm):
    inp0 = amd.make_input(nparticle_max=1, nx=nx)
    lx, vm = inp0.lx, inp0.v_max
    xs = [0.0, lx, math.nextafter(lx, 0.0), -0.0, 2.5 * lx, -0.25 * lx]
    vs = [0.3, -1.1, 1.5 * vm, -2.0 * vm]
    x = np.array([xi for xi in xs for _ in vs])
    v = np.array([vj for _ in xs for vj in vs])
    p = np.linspace(0.5, 1.5, x.size)
    w = np.linspace(-0.3, 0.4, x.size)
    e = uploaded(amd, x, v, p, w, nx=nx)
    modes = (0, 1) if nx == 2 else (0, 1, 32)
    got, ref = check(e, probe, modes, nherm, 0.5, 1.25, 3, what="edges nx %d nherm %d" % (nx, nherm))
    assert np.all(np.isfinite(got["total"])) and np.all(ref["total"]["abs"][1] > 0)
    for which, name in ((1, "total"), (2, "pertb")):
        one = e.hermite(0, modes, nherm, 0.5, 1.25, which)
        within(one[name], ref[name], partials(probe, x.size, nherm, len(modes), which), "edges which %d" % which)


# ---------------------------------------------------------------------------
# 5. a random state after steps
# ---------------------------------------------------------------------------
MODES4 = (0, 1, 2, 4)


@pytest.fixture(scope="module")
def stepped(amd):
    e = started(amd, nparticle_max=2**16, nx=64, species_nparticle_init=[2**16, 20_001], **TWO)
    e.step(10)
    yield e
    e.close()


@pytest.mark.parametrize("s", [0, 1])
def test_random_state_after_ten_steps(amd, probe, stepped, s):
    e = stepped
    g = valid(e, s)
    assert g["x"].size == (2**16, 20_001)[s]
    ref = HR.reference(g["x"], g["v"], g["p"], g["w"], e.inp, MODES4, 64, 5.0, 1.0, 3)
    worst = 0.0
    for which in (1, 2, 3):
        names = [n for bit, n in ((1, "total"), (2, "pertb")) if which & bit]
        for modes, cols in ((MODES4, None), ((1,), [1])):
            got = e.hermite(s, modes, 64, 5.0, 1.0, which)
            assert list(got) == names
            B = partials(probe, g["x"].size, 64, len(modes), which)
            for name in names:
                worst = max(worst, within(got[name], sub(ref[name], cols), B, "species %d which %d modes %s %s" % (s, which, modes, name)))
    print("hermite random state species %d: worst error / bound over all calls = %.3g" % (s, worst))


# ---------------------------------------------------------------------------
# 6. against the moments
# ---------------------------------------------------------------------------
def test_rows_zero_and_one_of_mode_zero_are_the_moments(amd, probe, stepped):
    """sum q psi_0 = sum_ix M_0 and sum q psi_1 = (sum_ix M_1 - v0 sum_ix M_0) ivt.  Either side is held to its own stated
    bound in units of the sum of the magnitudes of the terms it stands for: the spectrum's (n_p + B + 16) 2^-53; the
    moments' (n_b + workgroups) 2^-53 per bin, n_b <= 2 n_p terms of a bin, so (2 n_p + workgroups) 2^-53 for the planes
    summed.  Nothing is added to the sum of the two bounds: the planes are summed over ix with math.fsum (one rounding), and the
    three operations that form the right-hand side get no allowance of their own.  For row 0 the unit is sum |q|; for row 1
    it is ivt (sum |q v| + |v0| sum |q|), the terms of both sides before they cancel."""
    import moments_reference as MR
    e, s, v0, vt = stepped, 0, 5.0, 1.25
    ivt = 1.0 / vt
    g = valid(e, s)
    n = g["x"].size
    mom = e.moments(s, 3)
    her = e.hermite(s, (0,), 2, v0, vt, 3)
    B = partials(probe, n, 2, 1, 3)
    ops = (n + B + 16) + (2 * n + MR.workgroups(n))
    for name, q in (("total", g["p"]), ("pertb", g["w"])):
        m0, m1 = math.fsum(mom[name][0].tolist()), math.fsum(mom[name][1].tolist())
        s0 = np.sum(np.abs(q))
        s1 = ivt * (np.sum(np.abs(q * g["v"])) + abs(v0) * s0)
        d0 = abs(her[name][0, 0].real - m0)
        d1 = abs(her[name][0, 1].real - (m1 - v0 * m0) * ivt)
        print("hermite vs moments %s: row 0 %.3g of its bound, row 1 %.3g" % (name, d0 / (ops * HR.U * s0), d1 / (ops * HR.U * s1)))
        assert d0 <= ops * HR.U * s0 * (1 + 2.0**-20) and d1 <= ops * HR.U * s1 * (1 + 2.0**-20), name
        assert s0 > 0 and her[name][0, 0].real != 0.0


# ---------------------------------------------------------------------------
# 7. nothing changes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,kw", [(2, dict()), (1, dict(nmode=2, modes=[1, 2]))], ids=["six_sums", "tiles_two_modes"])
def test_between_steps_nothing_changes(amd, monkeypatch, kind, kw):
    """the model is test_gpu_moments.py: the prediction (and with the six sums the fused solve) survives the call, and the run
    is the run that never asked, bit for bit"""
    monkeypatch.setenv("PIC1DP_PREDICT", "1")
    monkeypatch.setenv("PIC1DP_PRED_KIND", str(kind))
    if kind == 2:
        monkeypatch.setenv("PIC1DP_FUSE_SOLVE", "2")
    a, b = (started(amd, nparticle_max=96, nx=32, **kw) for _ in range(2))
    for e in (a, b):
        assert e.predict_kind() == kind
        e.kernel_stats_enable(True)
        e.step(5)
    got = a.hermite(0, (0, 1), 64, 5.0, 1.0, 3)
    assert np.any(got["total"]) and a.hermite_stats()[1] == 1 and b.hermite_stats()[1] == 0
    a.hermite(0, (1,), 256, 0.0, 2.0, 2)
    assert a.hermite_stats()[1] == 2 and a.hermite_stats()[0] > 0.0
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


def marker_launches(e):
    """push, deposit and whole-step kernels launched so far (kernel stats enabled)"""
    return sum(e.kernel_stats(which)[1] for which in (0, 1, 2, 3, 4, 6))


def test_inside_a_step_the_noted_push_is_materialised(amd, probe, monkeypatch):
    kw = dict(nparticle_max=20_001, nx=96)
    modes, nherm, v0, vt = (1, 2), 32, 5.0, 1.0
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
    B = partials(probe, kw["nparticle_max"], nherm, len(modes), 3)
    for it in range(2):
        for irk in (1, 2):
            for e in (a, b):
                e.interaction_push_particle(irk)
            if irk == 1:
                # the lazy context has only noted its push: the call materialises it (a marker kernel runs); the eager one launches none
                before = [marker_launches(e) for e in (a, b)]
                ha = a.hermite(0, modes, nherm, v0, vt, 3)
                b.hermite(0, modes, nherm, v0, vt, 3)
                assert marker_launches(a) > before[0] and marker_launches(b) == before[1]
                hb, ref = check(b, probe, modes, nherm, v0, vt, 3, what="eager, inside step %d" % it)
                for name in ("total", "pertb"):
                    within(ha[name], ref[name], B, "lazy, inside step %d %s" % (it, name))
                    assert np.all(np.abs(HR.raw(ha[name]) - HR.raw(hb[name])) <= 2.0 * HR.bound(ref[name], B)), name
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
# 8. two contexts as two ranks
# ---------------------------------------------------------------------------
def test_two_ranks_local_spectra_add_up_on_the_host(amd, probe):
    kw = dict(nparticle_max=20_002, nx=64)
    modes, nherm, v0, vt = (1, 3), 48, 5.0, 1.0
    engs = [amd.Pic1dp(amd.make_input(**kw), rank=r, nranks=2, device=0) for r in range(2)]
    for e in engs:
        e.particle_load()
    parts = [valid(e) for e in engs]
    local = [e.hermite(0, modes, nherm, v0, vt, 3) for e in engs]
    allm = {k: np.concatenate([g[k] for g in parts]) for k in "xvpw"}
    ref = HR.reference(allm["x"], allm["v"], allm["p"], allm["w"], engs[0].inp, modes, nherm, v0, vt, 3)
    B = sum(partials(probe, g["x"].size, nherm, len(modes), 3) for g in parts) + 1      # and the host's addition
    for name in ("total", "pertb"):
        within(local[0][name] + local[1][name], ref[name], B, "two ranks %s" % name)
    assert parts[0]["x"].size > 0 and parts[1]["x"].size > 0


# ---------------------------------------------------------------------------
# 9. errors
# ---------------------------------------------------------------------------
def test_every_argument_error_and_nothing_is_written(amd):
    e = loaded(amd, nparticle_max=1000, nx=16)
    L = amd._lib.load()
    out = np.full(2 * 8 * 2 * 256, 7.0)
    ptr = out.ctypes.data_as(C.c_void_p)

    def call(which=3, isp=0, out_ptr=ptr, h_null=False, **kw):
        args = dict(modes=(1,), nherm=8, v0=0.0, vt=1.0)
        args.update(kw)
        h = amd.make_hermite(**args)
        return L.pic1dp_hip_hermite(e._ctx, isp, which, None if h_null else C.byref(h), out_ptr)

    assert call() == 0 and np.all(out[:32] != 7.0) and np.all(out[32:] == 7.0)
    out[:] = 7.0
    bad = [dict(which=0), dict(which=4), dict(nherm=0), dict(nherm=257), dict(modes=()), dict(modes=tuple(range(9)), which=1),
           dict(modes=(0, 1, 2, 3, 4)), dict(modes=(1, 1)), dict(modes=(-1,)), dict(modes=(9,)), dict(vt=0.0), dict(vt=-1.0),
           dict(vt=math.inf), dict(vt=math.nan), dict(v0=math.inf), dict(v0=math.nan), dict(isp=1), dict(isp=-1),
           dict(out_ptr=None), dict(h_null=True)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert L.pic1dp_hip_last_error()
    assert L.pic1dp_hip_hermite(None, 0, 3, C.byref(amd.make_hermite()), ptr) == 1
    assert np.all(out == 7.0)
    assert call(modes=(8,)) == 0                         # nx / 2 itself is a mode
    assert e.hermite_stats()[1] == 2
    f = loaded(amd, nparticle_max=1000, nx=16, deltaf=0, iptcldist=0, species_density=[1.0], species_v0=[0.0])
    for which in (2, 3):
        with pytest.raises(amd.Pic1dpError) as ei:
            f.hermite(0, (1,), 8, which=which)
        assert ei.value.code == 1 and "full-f" in str(ei.value)
    assert list(f.hermite(0, (1,), 8, which=1)) == ["total"]
    empty = amd.Pic1dp(amd.make_input(nparticle_max=1000, nx=16))
    with pytest.raises(amd.Pic1dpError):
        empty.hermite()                                  # no particles yet
